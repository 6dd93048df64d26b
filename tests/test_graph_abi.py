"""The C ABI of orb_graph_pairs as far as it can be checked without a device: the header's declarations and
structs against the Python mirror and the library's exports, and the constants, the defaults and the order of the checks in the
source against the restatement's (tests/graph_ref.py)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")
NAMES = ("orb_graph_pairs", "orb_graph_read", "orb_graph_edges", "orb_debug_loop_buffer")


def _fields(text, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{((?:[^}]|\n)*?)\} %s;" % name, text).group(1), flags=re.S)
    return re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)


def test_structs_constants_and_signatures(tinyorb):
    text = open(HEADER).read()
    P = tinyorb.GRAPH_POSE_DTYPE
    assert P.itemsize == 64 and P.names == ("r", "t", "cost_before", "cost_after", "loops", "status")
    assert [P.fields[k][1] for k in P.names] == [0, 36, 48, 52, 56, 60]
    assert _fields(text, "OrbGraphPose") == [("float", "r", "9"), ("float", "t", "3"), ("float", "cost_before", ""), ("float", "cost_after", ""),
                                             ("uint32_t", "loops", ""), ("uint32_t", "status", "")]
    E = tinyorb.GRAPH_EDGE_DTYPE
    assert E.itemsize == 16 and E.names == ("verdict", "cost_before", "cost_after", "origin") and [E.fields[k][1] for k in E.names] == [0, 4, 8, 12]
    assert _fields(text, "OrbGraphEdge") == [("uint32_t", "verdict", ""), ("float", "cost_before", ""), ("float", "cost_after", ""), ("uint32_t", "origin", "")]
    S = tinyorb.OrbGraphParams
    assert ctypes.sizeof(S) == 32
    assert [(n, getattr(S, n).offset) for n, _ in S._fields_] == [("rounds", 0), ("cg_iterations", 4), ("min_inliers", 8), ("loop_weight", 12),
                                                                  ("rotation_weight", 16), ("flags", 20), ("reserved", 24)]
    assert _fields(text, "OrbGraphParams") == [("uint32_t", "rounds", ""), ("uint32_t", "cg_iterations", ""), ("uint32_t", "min_inliers", ""),
                                               ("float", "loop_weight", ""), ("float", "rotation_weight", ""), ("uint32_t", "flags", ""),
                                               ("uint32_t", "reserved", "2")]
    for k, name in enumerate(("HELD", "UNCHANGED", "REFINED", "STALLED", "FAILED", "INVALID")):
        assert re.search(r"#define ORB_GRAPH_%s %du\b" % (name, k), text) and getattr(tinyorb, "ORB_GRAPH_" + name) == k
    for k, name in enumerate(("USED", "STATUS", "FEW", "RANGE", "SEGMENT", "NONFINITE", "SEGMENT_INVALID")):
        assert re.search(r"#define ORB_GRAPH_EDGE_%s %du\b" % (name, k), text) and getattr(tinyorb, "ORB_GRAPH_EDGE_" + name) == k
    assert re.search(r"#define ORB_GRAPH_USE_MINIMAL 1u\b", text) and tinyorb.ORB_GRAPH_USE_MINIMAL == 1
    sigs = dict(re.findall(r"^int (orb_graph_\w+|orb_debug_loop_buffer)\(([^)]*)\);", text, re.M))
    assert sigs == {
        "orb_graph_pairs": "OrbProgram *p, uint32_t n_pairs, const OrbGraphParams *params, void *stream",
        "orb_graph_read": "OrbProgram *p, uint32_t frame, OrbGraphPose *pose",
        "orb_graph_edges": "OrbProgram *p, OrbGraphEdge *dst, size_t n",
        "orb_debug_loop_buffer": "OrbProgram *p, void **fixes"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in NAMES:
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    assert L.orb_graph_pairs(None, 1, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_graph_pairs(None, 1, ctypes.byref(tinyorb.OrbGraphParams()), None) == tinyorb.ORB_EINVAL
    assert L.orb_graph_read(None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_graph_edges(None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_debug_loop_buffer(None, None) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("pg_" in n or "graph" in n for n in names)  # no profile ids for the new kernels


def test_constants_defaults_and_the_order_of_the_checks():
    import graph_ref as gr
    from tinyslam_amd import orb
    api = open(os.path.join(CSRC, "orb_api.hip")).read()
    kern = open(os.path.join(CSRC, "orb_kernels_graph.h")).read()

    def const(name):
        return re.search(r"\b%s = ([^;,]+)[;,]" % name, kern).group(1).strip()

    assert int(const("kPgFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kPgFixWords").rstrip("u")) * 4 == orb.LOOP_FIX_DTYPE.itemsize
    assert int(const("kPgPoseWords").rstrip("u")) * 4 == orb.GRAPH_POSE_DTYPE.itemsize
    assert int(const("kPgEdgeWords").rstrip("u")) * 4 == orb.GRAPH_EDGE_DTYPE.itemsize
    assert int(const("kPgNone").rstrip("u"), 16) == gr.NONE == orb.ORB_LOOP_NO_ORIGIN
    assert int(const("kPgMaxCg").rstrip("u")) == gr.MAX_CG == 512 and int(const("kPgLdsNodes").rstrip("u")) == gr.LDS_NODES
    # the node's words and the LDS bound derived from them: 78 words of 512 nodes and the partials within a CU's 160 KiB
    words = [int(const(n).rstrip("u")) for n in ("kPgPose", "kPgGrad", "kPgDinv", "kPgX", "kPgR", "kPgP", "kPgHp", "kPgNodeWords")]
    assert words == [0, 12, 18, 54, 60, 66, 72, 78]
    assert 78 * gr.LDS_NODES * 4 + 2 * 256 * 4 + 64 <= 160 * 1024 < 78 * (gr.LDS_NODES + 8) * 4 + 2 * 256 * 4
    # the words the kernels read by number
    D = orb.LOOP_FIX_DTYPE
    assert [D.fields[k][1] // 4 for k in ("r", "t", "origin", "query_origin", "inliers", "status")] == [0, 9, 25, 26, 28, 30]
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("r", "t", "origin", "status")] == [0, 9, 14, 17]
    # the solver and the polar step are section 21's and section 20's: included, not restated
    code = re.sub(r"//[^\n]*", "", kern)
    assert '#include "orb_kernels_localize.h"' in kern and '#include "orb_kernels_traj.h"' in kern
    assert code.count("verify_solve_n<6>(") == 1 and code.count("traj_polar_step(") == 1 and "fmaf" not in code and "__fmaf" not in code
    # the order of the checks: the parameters, then the state, then n_pairs
    call = api[api.index("int orb_graph_pairs("):api.index("int orb_graph_read(")]
    order = [call.index(s) for s in ("if (!p) return ORB_EINVAL", "reserved words must be 0", "g.rounds > 16u || g.cg_iterations > kPgMaxCg || (g.flags & ~ORB_GRAPH_USE_MINIMAL)",
                                     "loop_weight and rotation_weight must be finite", "stages_fresh(p, ST_GRAPH", "n_pairs < 1u || n_pairs > st[ST_LOOP].extent",
                                     "stage_open(p, ST_GRAPH")]
    assert order == sorted(order)
    assert "if (params) g = *params;" in call  # NULL: the defaults
    for line in ("a.min_inliers = g.min_inliers ? g.min_inliers : 12u;", "a.rounds = g.rounds ? g.rounds : 4u;", "a.cg_iterations = g.cg_iterations;",
                 "a.loop_weight = g.loop_weight == 0.0f ? 1.0f : g.loop_weight;", "a.rotation_weight = g.rotation_weight == 0.0f ? 1.0f : g.rotation_weight;",
                 "a.n_frames = st[ST_TRAJ].extent;"):
        assert line in call, line
    d = gr.defaults()
    assert (d["rounds"], d["cg_iterations"], d["min_inliers"], float(d["loop_weight"]), float(d["rotation_weight"]), d["flags"]) == (4, 0, 12, 1.0, 1.0, 0)
    assert gr.MAX_ROUNDS == 16 and "min(g.n, kPgMaxCg)" in kern
    assert "p->last_stream" not in call.replace("// p->last_stream stays", "")
    # the stage's row of the stage table: readers_of stays derived from it; its buffers, named once
    assert re.search(r'\{"graph_pairs", "graph_read",[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_PAIRS \|[^\n]*\n\s*1u << ST_LOOP\}', api)
    assert "constexpr ReadersOf kReaders = readers_of();" in api and api.count("case ST_GRAPH:") == 1 and api.count("&p->d_gwork") == 1
    assert re.search(r"enum StageId \{[^}]*\bST_GRAPH\b[^}]*ST_COUNT \}", api)
    # the loop buffer's address is refused until a loop call has run
    dbg = api[api.index("int orb_debug_loop_buffer("):api.index("int orb_graph_pairs(")]
    assert "!p->stage[ST_LOOP].extent" in dbg and "ORB_ESTATE" in dbg
