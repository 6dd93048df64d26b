"""The C ABI of orb_join_pairs as far as it can be checked without a device: the header's declarations and
structs against the Python mirror and the library's exports, and the constants, the defaults and the order of the checks in the
source against the restatement's (tests/join_ref.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")
NAMES = ("orb_join_pairs", "orb_join_read", "orb_join_segments", "orb_join_links", "orb_debug_loop_mask_buffer")


def _fields(text, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{((?:[^}]|\n)*?)\} %s;" % name, text).group(1), flags=re.S)
    return re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)


def test_structs_constants_and_signatures(tinyorb):
    text = open(HEADER).read()
    P = tinyorb.JOIN_POSE_DTYPE
    assert P.itemsize == 64 and P.names == ("r", "t", "scale", "gain", "root", "status") and [P.fields[k][1] for k in P.names] == [0, 36, 48, 52, 56, 60]
    assert _fields(text, "OrbJoinPose") == [("float", "r", "9"), ("float", "t", "3"), ("float", "scale", ""), ("float", "gain", ""),
                                            ("uint32_t", "root", ""), ("uint32_t", "status", "")]
    S = tinyorb.JOIN_SEGMENT_DTYPE
    assert S.itemsize == 64 and S.names == ("r", "t", "sigma", "root", "link", "status") and [S.fields[k][1] for k in S.names] == [0, 36, 48, 52, 56, 60]
    assert _fields(text, "OrbJoinSegment") == [("float", "r", "9"), ("float", "t", "3"), ("float", "sigma", ""), ("uint32_t", "root", ""),
                                               ("uint32_t", "link", ""), ("uint32_t", "status", "")]
    K = tinyorb.JOIN_LINK_DTYPE
    assert K.itemsize == 32 and K.names == ("verdict", "origin", "query_origin", "shared", "consistent", "gamma", "chosen", "reserved")
    assert [K.fields[k][1] for k in K.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert _fields(text, "OrbJoinLink") == [("uint32_t", "verdict", ""), ("uint32_t", "origin", ""), ("uint32_t", "query_origin", ""),
                                            ("uint32_t", "shared", ""), ("uint32_t", "consistent", ""), ("float", "gamma", ""),
                                            ("uint32_t", "chosen", ""), ("uint32_t", "reserved", "")]
    Q = tinyorb.OrbJoinParams
    assert ctypes.sizeof(Q) == 32
    assert [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("min_inliers", 0), ("min_shared", 4), ("scale_tolerance", 8),
                                                                  ("consistent_permille", 12), ("flags", 16), ("reserved", 20)]
    assert _fields(text, "OrbJoinParams") == [("uint32_t", "min_inliers", ""), ("uint32_t", "min_shared", ""), ("float", "scale_tolerance", ""),
                                              ("uint32_t", "consistent_permille", ""), ("uint32_t", "flags", ""), ("uint32_t", "reserved", "3")]
    for k, name in enumerate(("COPIED", "MOVED")):
        assert re.search(r"#define ORB_JOIN_%s %du\b" % (name, k), text) and getattr(tinyorb, "ORB_JOIN_" + name) == k
    for k, name in enumerate(("NONE", "ROOT", "LINKED")):
        assert re.search(r"#define ORB_JOIN_SEGMENT_%s %du\b" % (name, k), text) and getattr(tinyorb, "ORB_JOIN_SEGMENT_" + name) == k
    for k, name in enumerate(("HOLDS", "STATUS", "FEW", "RANGE", "SAME", "FORWARD", "NONFINITE", "RATIO_FEW", "RATIO_SPREAD")):
        assert re.search(r"#define ORB_JOIN_LINK_%s %du\b" % (name, k), text) and getattr(tinyorb, "ORB_JOIN_LINK_" + name) == k
    assert re.search(r"#define ORB_JOIN_USE_MINIMAL 1u\b", text) and tinyorb.ORB_JOIN_USE_MINIMAL == 1 and tinyorb.ORB_JOIN_NO_LINK == 0xFFFFFFFF
    sigs = dict(re.findall(r"^int (orb_join_\w+|orb_debug_loop_mask_buffer)\(([^)]*)\);", text, re.M))
    assert sigs == {
        "orb_join_pairs": "OrbProgram *p, uint32_t n_pairs, const OrbJoinParams *params, void *stream",
        "orb_join_read": "OrbProgram *p, uint32_t frame, OrbJoinPose *pose",
        "orb_join_segments": "OrbProgram *p, OrbJoinSegment *dst, size_t n",
        "orb_join_links": "OrbProgram *p, OrbJoinLink *dst, size_t n",
        "orb_debug_loop_mask_buffer": "OrbProgram *p, void **mask"}
    assert "int orb_debug_loop_buffer(OrbProgram *p, void **fixes);" in text  # stays as it is
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in NAMES:
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    assert L.orb_join_pairs(None, 1, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_join_pairs(None, 1, ctypes.byref(tinyorb.OrbJoinParams()), None) == tinyorb.ORB_EINVAL
    assert L.orb_join_read(None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_join_segments(None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_join_links(None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_debug_loop_mask_buffer(None, None) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("sj_" in n or "join" in n for n in names)  # no profile ids for the new kernels


def test_constants_defaults_and_the_order_of_the_checks():
    import join_ref as jr
    import trajectory_ref as tr
    from tinyslam_amd import orb
    api = open(os.path.join(CSRC, "orb_api.hip")).read()
    kern = open(os.path.join(CSRC, "orb_kernels_join.h")).read()

    def const(name):
        return re.search(r"\b%s = ([^;,]+)[;,]" % name, kern).group(1).strip()

    assert int(const("kSjFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kSjFixWords").rstrip("u")) * 4 == orb.LOOP_FIX_DTYPE.itemsize
    assert int(const("kSjPoseWords").rstrip("u")) * 4 == orb.JOIN_POSE_DTYPE.itemsize
    assert int(const("kSjSegWords").rstrip("u")) * 4 == orb.JOIN_SEGMENT_DTYPE.itemsize
    assert int(const("kSjLinkWords").rstrip("u")) * 4 == orb.JOIN_LINK_DTYPE.itemsize
    assert int(const("kSjNone").rstrip("u"), 16) == jr.NONE == orb.ORB_LOOP_NO_ORIGIN == orb.ORB_JOIN_NO_LINK
    assert int(const("kSjThreads").rstrip("u")) == 256
    for k, name in enumerate(("kSjHolds", "kSjStatus", "kSjFew", "kSjRange", "kSjSame", "kSjForward", "kSjNonfinite", "kSjRatioFew", "kSjRatioSpread")):
        assert int(const(name).rstrip("u")) == k
    # the words the kernels read and write by number
    D = orb.LOOP_FIX_DTYPE
    assert [D.fields[k][1] // 4 for k in ("pose_r", "pose_t", "origin", "query_origin", "inliers", "status")] == [13, 22, 25, 26, 28, 30]
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("r", "t", "scale", "origin")] == [0, 9, 12, 14]
    assert [orb.JOIN_SEGMENT_DTYPE.fields[k][1] // 4 for k in ("sigma", "root", "link", "status")] == [12, 13, 14, 15]
    assert [orb.JOIN_LINK_DTYPE.fields[k][1] // 4 for k in ("gamma", "chosen")] == [5, 6]
    # the owners' kernel, the polar step and the compose are section 28's and section 20's: included, not restated (the step once, in
    # SJ-4; the compose in SJ-6 and in the frames' records); no fused operation
    code = re.sub(r"//[^\n]*", "", kern)
    assert '#include "orb_kernels_loop.h"' in kern and "k_lc_index" not in code
    assert code.count("traj_polar_step(") == 1 and code.count("traj_compose(") == 2
    assert "fmaf" not in code and "__fmaf" not in code and "atomicAdd(&g." not in code  # the only global atomics are integer atomicMax
    assert code.count("atomicMax(") == 2 and "float" not in "".join(re.findall(r"atomic\w+\(([^;]*);", code))
    # the order of the checks: the parameters, then the state, then n_pairs and the owners' key
    call = api[api.index("int orb_join_pairs("):api.index("int orb_join_read(")]
    order = [call.index(s) for s in ("if (!p) return ORB_EINVAL", "reserved words must be 0", "g.consistent_permille > 1000u || (g.flags & ~ORB_JOIN_USE_MINIMAL)",
                                     "scale_tolerance must be finite", "stages_fresh(p, ST_JOIN", "n_pairs < 1u || n_pairs > st[ST_LOOP].extent",
                                     "(unsigned long long)L * cap >= 0xffffffffull", "stage_open(p, ST_JOIN")]
    assert order == sorted(order)
    assert "if (params) g = *params;" in call  # NULL: the defaults
    for line in ("a.min_inliers = g.min_inliers ? g.min_inliers : 12u;", "a.min_shared = g.min_shared ? g.min_shared : 8u;",
                 "a.tol = g.scale_tolerance == 0.0f ? 0.1f : g.scale_tolerance;", "a.permille = g.consistent_permille ? g.consistent_permille : 500u;",
                 "const uint32_t F = st[ST_TRAJ].extent;", "const uint32_t L = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, F));",
                 "o.owner = p->d_sowner;", "a.owner = p->d_sowner;"):
        assert line in call, line
    assert "d_lowner" not in call  # SJ-2: the loop stage's owners may be stale
    d, t = jr.defaults(), tr.defaults()
    assert (d["min_inliers"], d["min_shared"], float(d["scale_tolerance"]), d["consistent_permille"], d["flags"]) == (12, 8, float(t["scale_tolerance"]), 500, 0)
    assert (t["min_shared"], t["consistent_permille"]) == (8, 500)  # TJ-3, TJ-4's own defaults
    assert "p->last_stream" not in call.replace("// p->last_stream stays", "")
    # the stage's row of the stage table: readers_of stays derived from it; its buffers, named once
    assert re.search(r'\{"join_pairs", "join_read",\n\s*1u << ST_MATCH \|[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_LANDMARK \|[^\n]*\n\s*1u << ST_PAIRS \|[^\n]*\n'
                     r'\s*1u << ST_LOOP\}', api)
    assert "constexpr ReadersOf kReaders = readers_of();" in api and api.count("case ST_JOIN:") == 1
    for buf in ("d_sowner", "d_sratio", "d_slink", "d_skey", "d_sseg", "d_spose"):
        assert api.count("add(&p->%s" % buf) == 1
    assert re.search(r"enum StageId \{[^}]*\bST_GRAPH, ST_JOIN\b[^}]*ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT \}", api)
    # the mask buffer's address is refused until a loop call has run
    dbg = api[api.index("int orb_debug_loop_mask_buffer("):api.index("int orb_join_pairs(")]
    assert "!p->stage[ST_LOOP].extent" in dbg and "ORB_ESTATE" in dbg and "p->loop.mask" in dbg


def test_the_consensus_and_the_compose_are_stated_once():
    """TJ-3/TJ-4's select and BR-4's compose live in orb_kernels_traj.h; the stages after it call them and hold no copy."""
    code = {n: re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "orb_kernels_%s.h" % n)).read()) for n in ("traj", "bridge", "join", "loop")}
    for n in ("bridge", "join", "loop"):
        assert "hist[" not in code[n] and "__shfl_up" not in code[n], n
        assert "_compose(" not in code[n].replace("traj_compose(", ""), n
    assert code["bridge"].count("traj_consensus<") == 1 and code["join"].count("traj_consensus<") == 1
    # a definition has its return type in front of the name; a call does not
    assert len(re.findall(r"\bTrajConsensus traj_consensus\(", code["traj"])) == 1
    assert len(re.findall(r"\bvoid traj_compose\(", code["traj"])) == 1
