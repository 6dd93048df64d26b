"""The C ABI of the anchor stage (orb_anchor_frames and its reads) as far as it can be checked without a
device: the header's structs and declarations against the Python mirror and the library's exports, the NULL errors that need no
device, the order of the checks, the stage table's new row and its place, the generation check, and that the stage uses the join
stage's, the trajectory stage's and the loop stage's pieces instead of copies of them."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")
CALLS = ("orb_anchor_frames", "orb_anchor_read", "orb_anchor_segments", "orb_anchor_links", "orb_anchor_landmarks", "orb_debug_keyframe_buffers")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def test_structs_constants_and_signatures(tinyorb):
    T = tinyorb
    text = open(HEADER).read()
    for dtype, name, size, offsets in (
            (T.ANCHOR_POSE_DTYPE, "OrbAnchorPose", 64, dict(r=0, t=36, scale=48, gain=52, slot=56, status=60)),
            (T.ANCHOR_SEGMENT_DTYPE, "OrbAnchorSegment", 96, dict(r=0, t=36, gamma=48, slot=52, link=56, map_origin=60, map_frame=64, user=68, status=76, reserved=80)),
            (T.ANCHOR_LINK_DTYPE, "OrbAnchorLink", 32, dict(verdict=0, query_origin=4, slot=8, shared=12, consistent=16, gamma=20, chosen=24, reserved=28)),
            (T.ANCHOR_ROW_DTYPE, "OrbAnchorRow", 32, dict(good=0, moved=4, dropped=8, origin=12, slot=16, map_origin=20, reserved=24))):
        assert dtype.itemsize == size and dtype.names == tuple(offsets) and [dtype.fields[k][1] for k in offsets] == list(offsets.values()), name
        assert _struct_fields(text, name) == list(offsets), name
    P = T.OrbAnchorParams
    assert ctypes.sizeof(P) == 32 and [f[0] for f in P._fields_] == [f[0] for f in T.OrbJoinParams._fields_] == _struct_fields(text, "OrbAnchorParams")
    assert [getattr(P, k).offset for k in ("min_inliers", "min_shared", "scale_tolerance", "consistent_permille", "flags", "reserved")] == [0, 4, 8, 12, 16, 20]

    def define(name):
        return int(re.search(r"#define %s (\w+?)u?\b" % name, text).group(1), 0)

    assert [define("ORB_ANCHOR_LINK_" + k) for k in ("HOLDS", "STATUS", "FEW", "RANGE", "NONFINITE", "RATIO_FEW", "RATIO_SPREAD")] == list(range(7)) == \
        [T.ORB_ANCHOR_LINK_HOLDS, T.ORB_ANCHOR_LINK_STATUS, T.ORB_ANCHOR_LINK_FEW, T.ORB_ANCHOR_LINK_RANGE, T.ORB_ANCHOR_LINK_NONFINITE,
         T.ORB_ANCHOR_LINK_RATIO_FEW, T.ORB_ANCHOR_LINK_RATIO_SPREAD]
    assert [define("ORB_ANCHOR_SEGMENT_" + k) for k in ("NONE", "FREE", "ANCHORED")] == [T.ORB_ANCHOR_SEGMENT_NONE, T.ORB_ANCHOR_SEGMENT_FREE, T.ORB_ANCHOR_SEGMENT_ANCHORED] == [0, 1, 2]
    assert (define("ORB_ANCHOR_FREE"), define("ORB_ANCHOR_ANCHORED")) == (T.ORB_ANCHOR_FREE, T.ORB_ANCHOR_ANCHORED) == (0, 1)
    assert define("ORB_ANCHOR_USE_MINIMAL") == T.ORB_ANCHOR_USE_MINIMAL == T.ORB_JOIN_USE_MINIMAL == 1 and define("ORB_ANCHOR_NONE") == T.ORB_ANCHOR_NONE == 0xFFFFFFFF
    sigs = dict(re.findall(r"^int (orb_anchor_\w+|orb_debug_keyframe_buffers)\(([^)]*)\);", text, re.M))
    sigs = {k: " ".join(v.split()) for k, v in sigs.items()}
    assert sigs == {
        "orb_anchor_frames": "OrbProgram *p, uint32_t n, const OrbAnchorParams *params, void *stream",
        "orb_anchor_read": "OrbProgram *p, uint32_t frame, OrbAnchorPose *pose",
        "orb_anchor_segments": "OrbProgram *p, OrbAnchorSegment *dst, size_t n",
        "orb_anchor_links": "OrbProgram *p, OrbAnchorLink *dst, size_t n",
        "orb_anchor_landmarks": "OrbProgram *p, uint32_t pair, OrbAnchorRow *row, OrbLandmark *landmarks, size_t n",
        "orb_debug_keyframe_buffers": "OrbProgram *p, void **rows, void **fixes, void **mask"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    T = tinyorb
    L = T.load_library()
    for n in CALLS:
        assert n in T.EXPORTS and hasattr(L, n)
    prm = T.OrbAnchorParams()
    E = T.ORB_EINVAL
    assert L.orb_anchor_frames(None, 1, ctypes.byref(prm), None) == E and L.orb_anchor_frames(None, 1, None, None) == E
    assert L.orb_anchor_read(None, 0, np.zeros((), T.ANCHOR_POSE_DTYPE).ctypes.data) == E
    assert L.orb_anchor_segments(None, None, 0) == E and L.orb_anchor_links(None, None, 0) == E
    assert L.orb_anchor_landmarks(None, 0, None, None, 0) == E and L.orb_debug_keyframe_buffers(None, None, None, None) == E
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(T.ORB_KERNEL_COUNT)]
    assert T.ORB_KERNEL_COUNT == 25 and not any(n.startswith("k_an_") for n in names)  # no profile ids for the new kernels


def test_the_order_of_the_checks_and_the_generation():
    api = open(os.path.join(CSRC, "orb_api.hip")).read()
    call = api[api.index("int orb_anchor_frames("):api.index("int orb_anchor_read(")]
    marks = ("if (!p) return ORB_EINVAL", "reserved words must be 0", "g.consistent_permille > 1000u || (g.flags & ~ORB_ANCHOR_USE_MINIMAL)",
             "scale_tolerance must be finite", "stages_fresh(p, ST_ANCHOR, kStages[ST_ANCHOR].reads)", "p->kf_match_gen != p->kf_gen",
             "p->kf_loc_call != p->kf_match_call", "n < 1u || n > st[ST_KF_LOC].extent", "(unsigned long long)L * cap >= 0xffffffffull",
             "stage_open(p, ST_ANCHOR, stream, kStages[ST_ANCHOR].reads", "hipMemsetAsync(p->d_nowner, 0xff", "hipLaunchKernelGGL(k_lc_index", "hipLaunchKernelGGL(k_an_ratio",
             "hipLaunchKernelGGL(k_an_segment", "hipLaunchKernelGGL(k_an_write", "hipLaunchKernelGGL(k_an_land", "stage_end(p, ST_ANCHOR")
    at = [call.index(m) for m in marks]
    assert at == sorted(at), marks
    assert "if (params) g = *params;" in call and call.count("ORB_ESTATE") == 2  # NULL: the defaults; the two generation checks
    for line in ("a.min_inliers = g.min_inliers ? g.min_inliers : 12u;", "a.min_shared = g.min_shared ? g.min_shared : 8u;",
                 "a.tol = g.scale_tolerance == 0.0f ? 0.1f : g.scale_tolerance;", "a.permille = g.consistent_permille ? g.consistent_permille : 500u;",
                 "const uint32_t F = st[ST_TRAJ].extent;", "const uint32_t L = std::min(st[ST_LANDMARK].extent + 1u, std::min(st[ST_MATCH].extent, F));",
                 "o.owner = p->d_nowner;", "a.owner = p->d_nowner;",
                 "hipLaunchKernelGGL(k_lc_index, dim3(L - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, o);"):
        assert line in call, line
    for other in ("d_lowner", "d_sowner", "d_kowner", "d_aowner"):  # AN-2: an owner buffer of the stage's own
        assert other not in call
    assert "p->last_stream" not in call.replace("// p->last_stream stays", "")
    # what it reads is a kernel's const input; it reads no intrinsics
    for src in ("d_counts", "d_kmlist", "d_kmrows", "d_jframe", "d_mland", "d_mrow", "kfloc.fix", "kfloc.mask", "d_khead", "d_kpoints"):
        assert re.search(r"a\.\w+ = [^;]*p->%s;" % re.escape(src), call), src
    assert "fx" not in call and "check_intrinsics" not in call
    # every bump of the store's generation is seen: insert, load, remove, reserve
    assert api.count("p->kf_gen++") == 4 and api.count("p->kf_match_gen = p->kf_gen;") == 1
    assert "p->kf_match_call++;" in api[api.index("int orb_match_keyframes("):api.index("int orb_match_keyframes_read(")]
    assert "p->kf_loc_call = p->kf_match_call;" in api[api.index("int orb_localize_keyframes("):api.index("int orb_localize_keyframes_read(")]
    # load and remove wait on the host for an anchor call in flight; insert waits on its stream through the derived readers
    access = api[api.index("static int keyframes_host_access("):api.index("static int keyframes_clear_slot(")]
    assert "for (int st : {ST_KEYFRAMES, ST_KF_MATCH, ST_KF_LOC, ST_ANCHOR})" in access
    # the reads
    rd = api[api.index("int orb_anchor_landmarks("):api.index("int orb_debug_keyframe_buffers(")]
    assert "pair >= p->anchor_pairs" in rd and "read_stage(p, ST_ANCHOR, pair, row, p->d_nrow, sizeof(OrbAnchorRow), landmarks, p->d_nland, sizeof(OrbLandmark), n)" in rd
    dbg = api[api.index("int orb_debug_keyframe_buffers("):api.index("int orb_match_guided(")]
    assert "!p->stage[ST_KF_LOC].extent" in dbg and "ORB_ESTATE" in dbg and "p->kfloc.mask" in dbg and "p->kfloc.fix" in dbg and "p->d_kmrows" in dbg


def test_stage_table_placement_and_buffers():
    api = open(os.path.join(CSRC, "orb_api.hip")).read()
    assert re.search(r"enum StageId \{[^}]*\bST_GRAPH, ST_JOIN, ST_REMAP, ST_ANCHOR, ST_PLACE, ST_PAIRS, ST_KEYFRAMES, ST_KF_MATCH, ST_KF_LOC, ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT \}", api)
    rows = re.findall(r'^    \{"(\w+)", "(\w+)"', api[api.index("constexpr StageInfo kStages"):api.index("static_assert(kStages[ST_COUNT - 1]")], re.M)
    ids = re.search(r"enum StageId \{ ([^}]*) \}", api).group(1).replace(" = 0", "").split(", ")
    assert len(rows) == len(ids) - 1 <= 32 and ids[-1] == "ST_COUNT"  # the stages are bits of a uint32_t
    at = ids.index("ST_ANCHOR")
    assert rows[at] == ("anchor_frames", "anchor_read") and rows[at - 1][0] == "remap_frames" and rows[at + 1][0] == "place_frames"
    assert re.search(r'\{"anchor_frames", "anchor_read",\n\s*1u << ST_MATCH \|[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_LANDMARK \|[^\n]*\n\s*1u << ST_KF_MATCH \|[^\n]*\n'
                     r'\s*1u << ST_KF_LOC \|[^\n]*\n\s*1u << ST_KEYFRAMES\}', api)
    # readers_of stays derived; the store does not go stale with the batch
    assert "constexpr ReadersOf kReaders = readers_of();" in api and "constexpr uint32_t kOutlivesBatch = 1u << ST_KEYFRAMES;" in api
    assert api.count("case ST_ANCHOR:") == 1
    for buf in ("d_nowner", "d_nratio", "d_nlink", "d_nkey", "d_nseg", "d_npose", "d_nrow", "d_nland"):
        assert api.count("add(&p->%s," % buf) == 1, buf


def test_the_stage_uses_the_existing_pieces():
    src = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}
    code = {f: re.sub(r"//[^\n]*", "", t) for f, t in src.items()}
    everything = "\n".join(code.values())
    kern, an = src["orb_kernels_anchor.h"], code["orb_kernels_anchor.h"]

    def const(name):
        return re.search(r"\b%s = ([^;,]+)[;,]" % name, kern).group(1).strip()

    from tinyslam_amd import orb
    assert int(const("kAnFrameWords").rstrip("u")) * 4 == orb.FRAME_POSE_DTYPE.itemsize and int(const("kAnFixWords").rstrip("u")) * 4 == orb.KEYFRAME_FIX_DTYPE.itemsize
    assert int(const("kAnPoseWords").rstrip("u")) * 4 == orb.ANCHOR_POSE_DTYPE.itemsize and int(const("kAnSegWords").rstrip("u")) * 4 == orb.ANCHOR_SEGMENT_DTYPE.itemsize
    assert int(const("kAnLinkWords").rstrip("u")) * 4 == orb.ANCHOR_LINK_DTYPE.itemsize and int(const("kAnRowWords").rstrip("u")) * 4 == orb.ANCHOR_ROW_DTYPE.itemsize
    assert int(const("kAnLmRowWords").rstrip("u")) * 4 == orb.LANDMARK_ROW_DTYPE.itemsize and int(const("kAnThreads").rstrip("u")) == 256
    assert int(const("kAnNone").rstrip("u"), 16) == orb.ORB_ANCHOR_NONE
    for k, name in enumerate(("kAnHolds", "kAnStatus", "kAnFew", "kAnRange", "kAnNonfinite", "kAnRatioFew", "kAnRatioSpread")):
        assert int(const(name).rstrip("u")) == k
    # the words the kernels read and write by number
    D = orb.KEYFRAME_FIX_DTYPE
    assert [D.fields[k][1] // 4 for k in ("r", "t", "pose_r", "pose_t", "inliers", "status")] == [0, 9, 13, 22, 28, 30]
    assert [orb.KEYFRAME_DTYPE.fields[k][1] // 4 for k in ("keypoints", "frame", "origin", "user", "status")] == [13, 15, 16, 17, 19]
    assert [orb.ANCHOR_SEGMENT_DTYPE.fields[k][1] // 4 for k in ("gamma", "slot", "link", "map_origin", "map_frame", "user", "status")] == [12, 13, 14, 15, 16, 17, 19]
    assert [orb.ANCHOR_ROW_DTYPE.fields[k][1] // 4 for k in ("origin", "slot", "map_origin")] == [3, 4, 5] and orb.LANDMARK_ROW_DTYPE.fields["origin"][1] == 12
    assert [orb.LANDMARK_DTYPE.fields[k][1] for k in ("x", "flags", "views", "origin")] == [0, 12, 16, 20]
    # reused, not restated: each exists once in the tree, and the anchor header only calls it
    for fn, ret in (("sj_camera", "bool"), ("sj_similarity", "bool"), ("traj_verdict", "uint32_t"), ("traj_compose", "void"), ("traj_consensus", "TrajConsensus")):
        assert len(re.findall(r"\b%s %s\(" % (ret, fn), everything)) == 1 and not re.search(r"\b%s %s\(" % (ret, fn), an), fn
    assert len(re.findall(r"__global__[^;{]*\bvoid k_lc_index\(", everything)) == 1 and "k_lc_index" not in an
    assert '#include "orb_kernels_join.h"' in kern and '#include "orb_kernels_keyframes.h"' in kern
    assert an.count("traj_consensus<kAnThreads>") == 1 and an.count("sj_similarity(") == 2 and an.count("traj_compose(") == 1 and an.count("traj_verdict(") == 1
    assert "traj_polar_step" not in an and "hist[" not in an and "__shfl_up" not in an
    # no fused operation; integer atomics only
    assert "fmaf" not in an and "__fmaf" not in an and "fma(" not in an
    atomics = re.findall(r"(atomic\w+)\(([^;]*);", an)
    assert sorted(a for a, _ in atomics) == ["atomicAdd"] * 3 + ["atomicMax"] * 3 and all("float" not in arg for _, arg in atomics)
    assert "__ballot(" in an and re.search(r"const float4 Y = pts\[k\];", an)  # the stored point is one 16-byte load
    # the new kernels live in the new header only
    for f, t in src.items():
        if f != "orb_kernels_anchor.h" and f.endswith((".h", ".inc")):
            assert "k_an_" not in t, f
    assert len(re.findall(r"__global__[^;{]*\bvoid k_an_\w+\(", an)) == 4
