"""The C ABI of the loop stage (orb_loop_pairs) as far as it can be checked without a device: the header's
declarations and structs against the Python mirror and the library's exports, the layouts the kernels write, and the salt, the
defaults and the ranges in the source against the restatement's (tests/loop_ref.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs_and_signatures(tinyorb):
    text = open(HEADER).read()
    P = tinyorb._LoopParams
    assert ctypes.sizeof(P) == 64 and tinyorb.OrbLoopParams is P
    fields = ("fx", "fy", "cx", "cy", "max_reproj_px", "hypotheses", "max_distance", "ratio", "seed", "reserved")
    assert [f[0] for f in P._fields_] == list(fields) and [getattr(P, k).offset for k in fields] == [4 * i for i in range(10)]
    assert _struct_fields(text, "OrbLoopParams") == list(fields)
    D = tinyorb.LOOP_FIX_DTYPE
    names = ("r", "t", "step", "pose_r", "pose_t", "origin", "query_origin", "candidates", "inliers", "hypothesis", "status", "reserved")
    assert D.itemsize == 128 and D.names == names
    assert [D.fields[k][1] for k in names] == [0, 36, 48, 52, 88, 100, 104, 108, 112, 116, 120, 124]
    assert _struct_fields(text, "OrbLoopFix") == list(names)
    assert tinyorb.ORB_LOOP_NO_ORIGIN == 0xFFFFFFFF
    sigs = dict(re.findall(r"^int (orb_loop_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_loop_pairs": "OrbProgram *p, uint32_t n_pairs, const OrbLoopParams *params, void *stream",
                    "orb_loop_pairs_read": "OrbProgram *p, uint32_t pair, OrbLoopFix *fix, uint8_t *inliers, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_loop_pairs", "orb_loop_pairs_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb.OrbLoopParams(fx=100.0, fy=100.0)
    assert L.orb_loop_pairs(None, 1, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_loop_pairs(None, 1, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_loop_pairs_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any(n.startswith("k_lc_") for n in names)  # no profile ids for the new kernels


def test_the_source_states_what_the_restatement_states():
    import bridge_ref as brr
    import epipolar_ref as er
    import localize_ref as lr
    import loop_ref as lpr
    from tinyslam_amd import orb
    kern = open(os.path.join(CSRC, "orb_kernels_loop.h")).read()
    api = open(os.path.join(CSRC, "orb_api.hip")).read()

    def const(name):
        return re.search(r"constexpr \w+ %s = ([^;]+);" % name, kern).group(1)

    assert int(const("kLcSeedSalt").rstrip("u"), 16) == lpr.SEED_SALT == 0x4C433031
    salts = [int(v, 16) for v in re.findall(r"constexpr uint32_t k\w+SeedSalt = (0x[0-9A-Fa-f]+)u;", "".join(
        open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(".h")))]
    assert sorted(salts) == sorted({er.SEED_SALT, lr.SEED_SALT, brr.SEED_SALT, lpr.SEED_SALT}) and 0 not in salts  # 0: the homography verifier's
    assert int(const("kLcFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kLcFixWords").rstrip("u")) * 4 == orb.LOOP_FIX_DTYPE.itemsize
    assert int(const("kLcNone").rstrip("u"), 16) == lpr.NONE == orb.ORB_LOOP_NO_ORIGIN
    D = orb.LOOP_FIX_DTYPE
    assert [D.fields[k][1] // 4 for k in ("step", "pose_r", "pose_t", "origin", "query_origin", "candidates", "inliers", "hypothesis", "status")] == \
        [12, 13, 22, 25, 26, 27, 28, 29, 30]  # the words k_lc_refine writes
    assert orb.FRAME_POSE_DTYPE.fields["origin"][1] // 4 == 14 and orb.FRAME_PAIR_DTYPE.names == ("query", "target")  # rec[14]; list[e].x, .y
    assert [orb.LANDMARK_DTYPE.fields[k][1] for k in ("flags", "views", "origin")] == [12, 16, 20]  # lo.w, hi.x's low half, hi.y
    # the existing kernel is not redefined, and the fit is section 21's: no solver and no second refit in the loop or the bridge header
    for text in (kern, open(os.path.join(CSRC, "orb_kernels_bridge.h")).read()):
        code = re.sub(r"//[^\n]*", "", text)
        assert "k_loc_score" not in code and "_solve6" not in text and "verify_solve_n" not in code and "loc_accumulate" not in code
        assert code.count("loc_fit(") == 1
    call = api[api.index("int orb_loop_pairs("):api.index("int orb_loop_pairs_read(")]
    assert "hipLaunchKernelGGL(k_loc_score, dim3(n_pairs, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a.loc);" in call
    assert "loc_args(p, p->loop, g, kLcSeedSalt)" in call
    # the order of the checks: the parameters, then the state, then n_pairs and L * capacity
    order = [call.index(s) for s in ("reserved words must be 0", "check_intrinsics(p, ST_LOOP", "max_reproj_px must be finite", "ransac_params(p, ST_LOOP",
                                     "stages_fresh(p, ST_LOOP", "n_pairs < 1u || n_pairs > st[ST_PAIRS].extent", "(unsigned long long)n_frames * cap >= 0xffffffffull",
                                     "stage_open(p, ST_LOOP")]
    assert order == sorted(order)
    assert "if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;" in call
    ransac = api[api.index("int ransac_params("):api.index("int check_intrinsics(")]
    assert "*hypotheses > kVerifyMaxHyp || *max_distance > 256u" in ransac
    assert "if (!*hypotheses) *hypotheses = 512u;" in ransac and "if (!*max_distance) *max_distance = 64u;" in ransac and "*ratio = 0.8f;" in ransac
    d = lpr.defaults(1, 1, 0, 0)
    assert (float(d["max_reproj_px"]), d["hypotheses"], d["max_distance"], d["seed"]) == (2.0, 512, 64, 0) and abs(float(d["ratio"]) - 0.8) < 1e-7
    assert (lpr.MAX_HYPOTHESES, lpr.MAX_DISTANCE) == (4096, 256) and int(re.search(r"kVerifyMaxHyp = (\d+)u", open(os.path.join(CSRC, "orb_kernels_verify.h")).read()).group(1)) == 4096
    # the stage's row of the stage table, and its buffers, named once
    assert re.search(r'\{"loop_pairs", "loop_pairs_read",\s*1u << ST_PAIRS \|[^\n]*\n\s*1u << ST_MATCH \|[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_LANDMARK\}', api)
    assert "ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT" in api and api.count("case ST_LOOP:") == 1 and api.count("&p->d_lowner") == 1
