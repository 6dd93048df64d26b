"""The C ABI of the bridge stage (orb_bridge_consecutive) as far as it can be checked without a device: the
header's declarations and structs against the Python mirror and the library's exports, and the layouts the kernels write."""
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
    P = tinyorb._BridgeParams
    assert ctypes.sizeof(P) == 64 and tinyorb.OrbBridgeParams is P
    fields = ("fx", "fy", "cx", "cy", "max_reproj_px", "hypotheses", "max_distance", "ratio", "seed", "max_hops", "window", "min_shared",
              "scale_tolerance", "consistent_permille", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [4 * i for i in range(15)]
    assert _struct_fields(text, "OrbBridgeParams") == list(fields)
    D = tinyorb.BRIDGE_POSE_DTYPE
    names = ("r", "t", "scale", "gain", "root", "anchor", "candidates", "inliers", "hypothesis", "shared", "consistent", "fix", "status", "reserved")
    assert D.itemsize == 96 and D.names == names and [D.fields[k][1] for k in names] == [0, 36] + [48 + 4 * i for i in range(12)]
    assert _struct_fields(text, "OrbBridgePose") == list(names)
    for i, n in enumerate(("COPIED", "MOVED", "FIXED", "JOINED", "UNFIXED")):
        assert getattr(tinyorb, "ORB_BRIDGE_" + n) == i and re.search(r"#define ORB_BRIDGE_%s %du\b" % (n, i), text)
    sigs = dict(re.findall(r"^int (orb_bridge_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_bridge_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbBridgeParams *params, void *stream",
                    "orb_bridge_read": "OrbProgram *p, uint32_t frame, OrbBridgePose *pose, uint8_t *inliers, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_bridge_consecutive", "orb_bridge_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbBridgeParams(fx=100.0, fy=100.0)
    assert L.orb_bridge_consecutive(None, 3, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_bridge_consecutive(None, 3, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_bridge_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any(n.startswith("k_br_") for n in names)


def test_the_restatement_reads_the_mirror_and_the_kernels_the_same_layout():
    import bridge_ref as brr
    from tinyslam_amd import orb
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_bridge.h")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)

    assert int(const("kBrSeedSalt").rstrip("u"), 16) == brr.SEED_SALT == 0x42523031
    assert int(const("kBrFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kBrOutWords").rstrip("u")) * 4 == orb.BRIDGE_POSE_DTYPE.itemsize
    assert int(const("kBrMaxHops").rstrip("u")) == brr.MAX_HOPS == 16
    D = orb.BRIDGE_POSE_DTYPE
    assert [D.fields[k][1] // 4 for k in ("gain", "root", "status")] == [13, 14, 22]  # the words br_similarity reads back
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("t", "scale", "origin", "status")] == [9, 12, 14, 17]
    assert [orb.LANDMARK_DTYPE.fields[k][1] for k in ("views", "tail_index")] == [16, 24]  # hi.x's low half and hi.z
    assert [orb.FIX_DTYPE.fields[k][1] // 4 for k in ("step", "candidates", "inliers", "hypothesis", "status")] == [12, 13, 14, 15, 16]
    p = brr.defaults(1, 1, 0, 0)
    assert (p["max_reproj_px"], p["hypotheses"], p["max_distance"], p["max_hops"], p["window"], p["min_shared"], p["consistent_permille"]) == \
        (2.0, 512, 64, 4, 32, 8, 500) and abs(float(p["ratio"]) - 0.8) < 1e-7 and abs(float(p["scale_tolerance"]) - 0.1) < 1e-8
