"""The C ABI of the adjustment stage (orb_adjust_consecutive) as far as it can be checked without a device: the
header's declarations and structs against the Python mirror and the library's exports, and the layouts the kernels read and write."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs(tinyorb):
    text = open(HEADER).read()
    P = tinyorb._AdjustParams
    assert ctypes.sizeof(P) == 32 and tinyorb.OrbAdjustParams is P
    fields = ("fx", "fy", "cx", "cy", "max_reproj_px", "rounds", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [4 * i for i in range(7)]
    assert _struct_fields(text, "OrbAdjustParams") == list(fields)
    D = tinyorb.ADJUSTED_POSE_DTYPE
    names = ("r", "t", "cost_before", "cost_after", "observations", "status")
    assert D.itemsize == 64 and D.names == names and [D.fields[k][1] for k in names] == [0, 36, 48, 52, 56, 60]
    assert _struct_fields(text, "OrbAdjustedPose") == list(names)
    for i, n in enumerate(("HELD", "REFINED", "FEW", "FAILED")):
        assert getattr(tinyorb, "ORB_ADJUST_" + n) == i and re.search(r"#define ORB_ADJUST_%s %du\b" % (n, i), text)
    sigs = dict(re.findall(r"^int (orb_adjust_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_adjust_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbAdjustParams *params, void *stream",
                    "orb_adjust_read": "OrbProgram *p, uint32_t frame, OrbAdjustedPose *pose, OrbLandmark *landmarks, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_adjust_consecutive", "orb_adjust_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbAdjustParams(fx=100.0, fy=100.0)
    assert L.orb_adjust_consecutive(None, 3, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_adjust_consecutive(None, 3, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_adjust_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any(n.startswith("k_ba_") for n in names)


def test_rounds_out_of_range_and_the_key_limit():
    """The ranges orb_adjust_consecutive checks before it touches the device, read from its source: rounds above 16, and
    n_frames * max_features at or above 2^32 - 1 (BA-3: a key below the word for `no owner`)."""
    import adjust_ref as ar
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_api.hip")).read()
    body = text[text.index("int orb_adjust_consecutive("):text.index("int orb_adjust_read(")]
    assert "g.rounds > %du" % ar.MAX_ROUNDS in body and ar.MAX_ROUNDS == 16
    assert "(unsigned long long)n_frames * cap >= 0xffffffffull" in body and ar.NONE == 0xFFFFFFFF
    assert "if (!g.rounds) g.rounds = 4u;" in body and "if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;" in body


def test_the_restatement_reads_the_mirror_and_the_kernels_the_same_layout():
    import adjust_ref as ar
    from tinyslam_amd import orb
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_adjust.h")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)

    assert int(const("kBaFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kBaPoseWords").rstrip("u")) * 4 == orb.ADJUSTED_POSE_DTYPE.itemsize
    assert int(const("kBaMinObs").rstrip("u")) == ar.MIN_OBSERVATIONS == 6
    assert int(const("kBaNone").rstrip("u"), 16) == ar.NONE
    assert int(const("kBaSums").rstrip("u")) == 28
    # the words k_ba_index reads of a frame record (rec[q], q < 12; rec[14]; rec[17]) and of a landmark record (lo.w; hi.x's low
    # half, hi.y, hi.z), and those k_ba_motion writes
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("r", "t", "origin", "status")] == [0, 9, 14, 17]
    assert [orb.LANDMARK_DTYPE.fields[k][1] for k in ("x", "flags", "views", "inliers", "origin", "tail_index", "reserved")] == [0, 12, 16, 18, 20, 24, 28]
    assert [orb.ADJUSTED_POSE_DTYPE.fields[k][1] // 4 for k in ("t", "cost_before", "cost_after", "observations", "status")] == [9, 12, 13, 14, 15]
    p = ar.defaults(1, 1, 0, 0)
    assert (float(p["max_reproj_px"]), p["rounds"]) == (2.0, 4)
    assert (orb.ORB_ADJUST_HELD, orb.ORB_ADJUST_REFINED, orb.ORB_ADJUST_FEW, orb.ORB_ADJUST_FAILED) == (0, 1, 2, 3)
