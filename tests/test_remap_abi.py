"""The C ABI of orb_remap_frames as far as it can be checked without a device: the header's declarations and
structs against the Python mirror and the library's exports, and the constants, the order of the checks, the stage's row and its
buffers in the source."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")
NAMES = ("orb_remap_frames", "orb_remap_read", "orb_remap_landmarks")


def _fields(text, name):
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct \{((?:[^}]|\n)*?)\} %s;" % name, text).group(1), flags=re.S)
    return re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)


def test_structs_constants_and_signatures(tinyorb):
    text = open(HEADER).read()
    P = tinyorb.REMAP_POSE_DTYPE
    assert P.itemsize == 64 and P.names == ("r", "t", "scale", "gain", "root", "status") and [P.fields[k][1] for k in P.names] == [0, 36, 48, 52, 56, 60]
    assert _fields(text, "OrbRemapPose") == [("float", "r", "9"), ("float", "t", "3"), ("float", "scale", ""), ("float", "gain", ""),
                                             ("uint32_t", "root", ""), ("uint32_t", "status", "")]
    R = tinyorb.REMAP_ROW_DTYPE
    assert R.itemsize == 16 and R.names == ("good", "moved", "dropped", "root") and [R.fields[k][1] for k in R.names] == [0, 4, 8, 12]
    assert _fields(text, "OrbRemapRow") == [("uint32_t", "good", ""), ("uint32_t", "moved", ""), ("uint32_t", "dropped", ""), ("uint32_t", "root", "")]
    Q = tinyorb.OrbRemapParams
    assert ctypes.sizeof(Q) == 32 and [(n, getattr(Q, n).offset) for n, _ in Q._fields_] == [("flags", 0), ("reserved", 4)]
    assert _fields(text, "OrbRemapParams") == [("uint32_t", "flags", ""), ("uint32_t", "reserved", "7")]
    for name, v in (("GRAPH", 1), ("JOIN", 2), ("FROM_GRAPH", 1), ("MOVED", 2)):
        assert re.search(r"#define ORB_REMAP_%s %du\b" % (name, v), text) and getattr(tinyorb, "ORB_REMAP_" + name) == v
    sigs = dict(re.findall(r"^int (orb_remap_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {
        "orb_remap_frames": "OrbProgram *p, const OrbRemapParams *params, void *stream",
        "orb_remap_read": "OrbProgram *p, uint32_t frame, OrbRemapPose *pose",
        "orb_remap_landmarks": "OrbProgram *p, uint32_t pair, OrbRemapRow *row, OrbLandmark *landmarks, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    L = tinyorb.load_library()
    for n in NAMES:
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    assert L.orb_remap_frames(None, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_remap_frames(None, ctypes.byref(tinyorb.OrbRemapParams()), None) == tinyorb.ORB_EINVAL
    assert L.orb_remap_read(None, 0, None) == tinyorb.ORB_EINVAL
    assert L.orb_remap_landmarks(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("rm_" in n or "remap" in n for n in names)  # no profile ids for the new kernels


def test_constants_the_order_of_the_checks_and_the_stage():
    import remap_ref as rr
    from tinyslam_amd import orb
    api = open(os.path.join(CSRC, "orb_api.hip")).read()
    kern = open(os.path.join(CSRC, "orb_kernels_remap.h")).read()

    def const(name):
        return re.search(r"\b%s = ([^;,]+)[;,]" % name, kern).group(1).strip()

    assert int(const("kRmFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize
    assert int(const("kRmGraphWords").rstrip("u")) * 4 == orb.GRAPH_POSE_DTYPE.itemsize
    assert int(const("kRmSegWords").rstrip("u")) * 4 == orb.JOIN_SEGMENT_DTYPE.itemsize
    assert int(const("kRmPoseWords").rstrip("u")) * 4 == orb.REMAP_POSE_DTYPE.itemsize
    assert int(const("kRmRowWords").rstrip("u")) * 4 == orb.REMAP_ROW_DTYPE.itemsize == orb.LANDMARK_ROW_DTYPE.itemsize
    assert int(const("kRmNone").rstrip("u"), 16) == rr.NONE and int(const("kRmThreads").rstrip("u")) == 256
    assert (int(const("kRmFromGraph").rstrip("u")), int(const("kRmMoved").rstrip("u"))) == (orb.ORB_REMAP_FROM_GRAPH, orb.ORB_REMAP_MOVED)
    assert int(const("kRmSegLinked").rstrip("u")) == orb.ORB_JOIN_SEGMENT_LINKED
    assert (int(const("kRmGraphRefined").rstrip("u")), int(const("kRmGraphFailed").rstrip("u"))) == (orb.ORB_GRAPH_REFINED, orb.ORB_GRAPH_FAILED)
    assert (orb.ORB_GRAPH_REFINED, orb.ORB_GRAPH_STALLED, orb.ORB_GRAPH_FAILED) == (2, 3, 4)  # a range in the kernel, a set in the restatement
    # the words the kernels read and write by number
    assert [orb.FRAME_POSE_DTYPE.fields[k][1] // 4 for k in ("r", "t", "scale", "origin")] == [0, 9, 12, 14]
    assert [orb.GRAPH_POSE_DTYPE.fields[k][1] // 4 for k in ("r", "t", "status")] == [0, 9, 15]
    assert [orb.JOIN_SEGMENT_DTYPE.fields[k][1] // 4 for k in ("r", "t", "sigma", "root", "status")] == [0, 9, 12, 13, 15]
    assert [orb.LANDMARK_DTYPE.fields[k][1] for k in ("x", "flags", "views", "origin")] == [0, 12, 16, 20] and orb.LANDMARK_DTYPE.itemsize == 32
    assert orb.LANDMARK_ROW_DTYPE.fields["origin"][1] == 12
    # the compose is section 20's: included, called once, not restated; no fused operation; integer atomics only
    code = re.sub(r"//[^\n]*", "", kern)
    assert '#include "orb_kernels_traj.h"' in kern and code.count("traj_compose(") == 1 and "traj_polar_step" not in code
    assert "fmaf" not in code and "__fmaf" not in code and "fma(" not in code
    atomics = re.findall(r"(atomic\w+)\(([^;]*);", code)
    assert [a for a, _ in atomics] == ["atomicAdd"] * 3 and all(arg.startswith("&row[") and "float" not in arg for _, arg in atomics)
    assert re.search(r"uint32_t\* const row = g\.rows", code) and "__ballot(" in code
    # no existing header is edited for it: the stage's kernels live in the new one
    for other in os.listdir(CSRC):
        if other != "orb_kernels_remap.h" and other.endswith(".h"):
            assert "k_rm_" not in open(os.path.join(CSRC, other)).read(), other
    # the order of the checks: the parameters, then the freshness, then the sources' extents, then the launches
    call = api[api.index("int orb_remap_frames("):api.index("int orb_remap_read(")]
    order = [call.index(s) for s in ("if (!p) return ORB_EINVAL", "reserved words must be 0", "g.flags & ~(ORB_REMAP_GRAPH | ORB_REMAP_JOIN)",
                                     "stages_fresh(p, ST_REMAP, reads)", "st[ST_GRAPH].extent != F", "stage_open(p, ST_REMAP, stream, reads", "hipLaunchKernelGGL(k_rm_pose",
                                     "stage_end(p, ST_REMAP")]
    assert order == sorted(order)
    assert "if (params) g = *params;" in call and call.count("ORB_ESTATE") == 1 and "st[ST_JOIN].extent != F" in call
    assert "const uint32_t reads = 1u << ST_TRAJ | 1u << ST_LANDMARK | (graph ? 1u << ST_GRAPH : 0u) | (join ? 1u << ST_JOIN : 0u);" in call
    assert "const uint32_t pairs = std::min(st[ST_LANDMARK].extent, F - 1u);" in call and "p->remap_pairs = pairs;" in call
    assert "p->last_stream" not in call.replace("// p->last_stream stays", "")
    for other in ("d_jframe", "d_gpose", "d_sseg", "d_mland", "d_mrow"):  # read, and only as a kernel's const input
        assert re.search(r"a\.\w+ = [^;]*p->%s" % other, call), other
    # the stage's row; readers_of stays derived; its buffers, named once
    assert re.search(r'\{"remap_frames", "remap_read",[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_LANDMARK \|[^\n]*\n\s*1u << ST_GRAPH \|[^\n]*\n\s*1u << ST_JOIN\}', api)
    assert "constexpr ReadersOf kReaders = readers_of();" in api and api.count("case ST_REMAP:") == 1
    for buf in ("d_rpose", "d_rrow", "d_rland"):
        assert api.count("add(&p->%s" % buf) == 1
    assert re.search(r"enum StageId \{[^}]*\bST_GRAPH, ST_JOIN, ST_REMAP\b[^}]*ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT \}", api)
    # the landmark read goes through read_stage behind the pairs kept beside the stage
    rd = api[api.index("int orb_remap_landmarks("):api.index("int orb_match_guided(")]
    assert "pair >= p->remap_pairs" in rd and "read_stage(p, ST_REMAP, pair, row, p->d_rrow, sizeof(OrbRemapRow), landmarks, p->d_rland, sizeof(OrbLandmark), n)" in rd
