"""The C ABI of the localisation stage (orb_localize_consecutive) as far as it can be checked without a device:
the header's declarations, structs and constants against the Python mirror and the library's exports."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs_and_constants(tinyorb):
    text = open(HEADER).read()
    P = tinyorb._LocalizeParams
    assert ctypes.sizeof(P) == 64 and tinyorb.OrbLocalizeParams is P
    fields = ("fx", "fy", "cx", "cy", "max_reproj_px", "hypotheses", "max_distance", "ratio", "seed", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36]
    assert _struct_fields(text, "OrbLocalizeParams") == list(fields)
    assert tinyorb.FIX_DTYPE.itemsize == 80
    names = ("r", "t", "step", "candidates", "inliers", "hypothesis", "status", "reserved")
    assert [tinyorb.FIX_DTYPE.fields[k][1] for k in names] == [0, 36, 48, 52, 56, 60, 64, 68]
    assert _struct_fields(text, "OrbFrameFix") == list(names)
    consts = dict(re.findall(r"#define\s+(ORB_LOCALIZE_[A-Z_]+)\s+(\d+)u\b", text))
    assert sorted(consts) == ["ORB_LOCALIZE_DEGENERATE", "ORB_LOCALIZE_FEW", "ORB_LOCALIZE_MINIMAL", "ORB_LOCALIZE_NOMAP", "ORB_LOCALIZE_OK"]
    for name, value in consts.items():
        assert int(value) == getattr(tinyorb, name), name
    assert [tinyorb.ORB_LOCALIZE_OK, tinyorb.ORB_LOCALIZE_NOMAP, tinyorb.ORB_LOCALIZE_FEW, tinyorb.ORB_LOCALIZE_DEGENERATE,
            tinyorb.ORB_LOCALIZE_MINIMAL] == [0, 1, 2, 3, 4]
    sigs = dict(re.findall(r"^int (orb_localize_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_localize_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbLocalizeParams *params, void *stream",
                    "orb_localize_read": "OrbProgram *p, uint32_t pair, OrbFrameFix *fix, uint8_t *inliers, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_localize_consecutive", "orb_localize_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbLocalizeParams(fx=100.0, fy=100.0)
    assert L.orb_localize_consecutive(None, 3, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_localize_consecutive(None, 3, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_localize_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("k_loc" in n for n in names)


def test_restatement_constants_match_the_kernels():
    """The salt, the draws, the sample size, the pivot ratio, the steps and the sums of LO-2..LO-6 as the kernel header spells them."""
    import localize_ref as lr
    text = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_localize.h")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, text).group(1)

    assert int(const("kLocSeedSalt").rstrip("u"), 16) == lr.SEED_SALT == 0x4C4F3031
    assert int(const("kLocDraws").rstrip("u")) == lr.DRAWS and int(const("kLocSample").rstrip("u")) == lr.SAMPLE
    assert int(const("kLocSteps").rstrip("u")) == lr.GN_STEPS and int(const("kLocSums").rstrip("u")) == 27
    assert const("kLocPivotRatio") == "1.0f / 4194304.0f" and float(lr.PIVOT_RATIO) == 1.0 / 4194304.0
    assert int(const("kLocRow").rstrip("u")) == 11 * 12 + 1
