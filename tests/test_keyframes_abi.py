"""The C ABI of the keyframe store (orb_keyframes_*, orb_match_keyframes, orb_localize_keyframes) as far as
it can be checked without a device: the header's structs and declarations against the Python mirror and the library's exports,
the NULL and range errors that need no device, the stage table's new rows, and that the stage uses the loop stage's index, score
and fit and the two matcher bodies instead of copies of them."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
CSRC = os.path.join(ROOT, "tinyslam_amd", "csrc")
CALLS = ("orb_keyframes_reserve", "orb_keyframes_insert", "orb_keyframes_read", "orb_keyframes_load", "orb_keyframes_remove",
         "orb_match_keyframes", "orb_match_keyframes_read", "orb_localize_keyframes", "orb_localize_keyframes_read")


def _struct_fields(text, name):
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", body)


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}


def test_structs_constants_and_signatures(tinyorb):
    T = tinyorb
    text = open(HEADER).read()
    D = T.KEYFRAME_DTYPE
    names = ("r", "t", "scale", "keypoints", "points", "frame", "origin", "user", "status", "reserved")
    assert D.itemsize == 96 and D.names == names and [D.fields[k][1] for k in names] == [0, 36, 48, 52, 56, 60, 64, 68, 76, 80]
    assert _struct_fields(text, "OrbKeyframe") == list(names)
    M = T.MAP_POINT_DTYPE
    assert M.itemsize == 16 and M.names == ("x", "y", "z", "key") and _struct_fields(text, "OrbMapPoint") == ["x", "y", "z", "key"]
    X = T.KEYFRAME_FIX_DTYPE
    assert X.itemsize == 128 and X.names == tuple("slot" if k == "query_origin" else k for k in T.LOOP_FIX_DTYPE.names)
    assert [X.fields[k][1] for k in X.names] == [T.LOOP_FIX_DTYPE.fields[k][1] for k in T.LOOP_FIX_DTYPE.names]
    assert _struct_fields(text, "OrbKeyframeFix") == list(X.names)
    assert T.KEYFRAME_ENTRY_DTYPE.itemsize == 16 and T.KEYFRAME_ENTRY_DTYPE.names == ("frame", "slot", "user")
    assert T.KEYFRAME_PAIR_DTYPE.itemsize == 8 and T.KEYFRAME_PAIR_DTYPE.names == ("query", "slot")
    assert _struct_fields(text, "OrbKeyframeEntry") == ["frame", "slot", "user"] and _struct_fields(text, "OrbKeyframePair") == ["query", "slot"]

    def define(name):
        return int(re.search(r"#define %s (\w+?)u?\b" % name, text).group(1), 0)

    assert define("ORB_KEYFRAME_SLOTS_MAX") == T.ORB_KEYFRAME_SLOTS_MAX == define("ORB_PLACE_DB_MAX") == 1024
    assert define("ORB_KEYFRAME_NONE") == T.ORB_KEYFRAME_NONE == 0xFFFFFFFF
    assert [define("ORB_KEYFRAME_" + k) for k in ("EMPTY", "STORED", "NOMAP")] == [T.ORB_KEYFRAME_EMPTY, T.ORB_KEYFRAME_STORED, T.ORB_KEYFRAME_NOMAP] == [0, 1, 2]
    sigs = dict(re.findall(r"^(?:extern )?int (orb_\w*keyframes\w*)\(([^)]*)\);", text, re.M))
    sigs = {k: " ".join(v.split()) for k, v in sigs.items()}
    assert sigs == {
        "orb_keyframes_reserve": "OrbProgram *p, uint32_t slots",
        "orb_keyframes_insert": "OrbProgram *p, const OrbKeyframeEntry *list, uint32_t n, void *stream",
        "orb_keyframes_read": "OrbProgram *p, uint32_t slot, OrbKeyframe *header, CornerData *corners, CornerDescriptor *descriptors, OrbMapPoint *points, size_t n",
        "orb_keyframes_load": "OrbProgram *p, uint32_t slot, const OrbKeyframe *header, const CornerData *corners, const CornerDescriptor *descriptors, "
                              "const OrbMapPoint *points, size_t n",
        "orb_keyframes_remove": "OrbProgram *p, uint32_t slot",
        "orb_match_keyframes": "OrbProgram *p, const OrbKeyframePair *list, uint32_t n, void *stream",
        "orb_match_keyframes_read": "OrbProgram *p, uint32_t entry, OrbMatch *dst, size_t n",
        "orb_localize_keyframes": "OrbProgram *p, uint32_t n, const OrbLoopParams *params, void *stream",
        "orb_localize_keyframes_read": "OrbProgram *p, uint32_t entry, OrbKeyframeFix *fix, uint8_t *inliers, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_exports_and_null_arguments(tinyorb):
    T = tinyorb
    L = T.load_library()
    for n in CALLS:
        assert n in T.EXPORTS and hasattr(L, n)
    prm = T.OrbLoopParams(fx=100.0, fy=100.0)
    entry = np.zeros(1, T.KEYFRAME_ENTRY_DTYPE)
    pair = np.zeros(1, T.KEYFRAME_PAIR_DTYPE)
    head = np.zeros((), T.KEYFRAME_DTYPE)
    E = T.ORB_EINVAL
    assert L.orb_keyframes_reserve(None, 1) == E
    assert L.orb_keyframes_insert(None, entry.ctypes.data, 1, None) == E
    assert L.orb_keyframes_read(None, 0, head.ctypes.data, None, None, None, 0) == E
    assert L.orb_keyframes_load(None, 0, head.ctypes.data, None, None, None, 0) == E
    assert L.orb_keyframes_remove(None, 0) == E
    assert L.orb_match_keyframes(None, pair.ctypes.data, 1, None) == E
    assert L.orb_match_keyframes_read(None, 0, None, 0) == E
    assert L.orb_localize_keyframes(None, 1, ctypes.byref(prm), None) == E and L.orb_localize_keyframes(None, 1, None, None) == E
    assert L.orb_localize_keyframes_read(None, 0, None, None, 0) == E
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(T.ORB_KERNEL_COUNT)]
    assert T.ORB_KERNEL_COUNT == 25 and not any(n.startswith(("k_kf_", "k_match_kf")) for n in names)  # no profile ids for the new kernels


def test_the_order_of_the_checks_in_the_source():
    api = _sources()["orb_api.hip"]

    def body(name, until):
        return api[api.index("int %s(" % name):api.index("int %s(" % until)]

    def ordered(text, marks):
        at = [text.index(m) for m in marks]
        assert at == sorted(at), marks

    ordered(body("orb_keyframes_reserve", "orb_keyframes_insert"),
            ("if (!p) return ORB_EINVAL;", "slots < 1u || slots > ORB_KEYFRAME_SLOTS_MAX", "p->kf_slots == slots ? ORB_OK : fail(p, ORB_ESTATE", "alloc_all_or_none(p, ST_KEYFRAMES"))
    ordered(body("orb_keyframes_insert", "orb_keyframes_read"),
            ("if (!p) return ORB_EINVAL;", "before orb_keyframes_reserve", "before a batch", "!list || n < 1u || n > p->plan.max_batch",
             "e.frame >= p->last_batch || e.slot >= p->kf_slots || named[e.slot]", "stages_fresh(p, ST_KEYFRAMES", "(unsigned long long)n_frames * cap >= 0xffffffffull",
             "stage_open(p, ST_KEYFRAMES", "hipMemsetAsync(p->d_kowner, 0xff", "k_lc_index", "k_kf_head", "k_kf_insert", "p->kf_gen++", "stage_end(p, ST_KEYFRAMES"))
    ordered(body("orb_keyframes_load", "orb_keyframes_remove"),
            ("if (!p) return ORB_EINVAL;", "keyframes_host_access(p", "n != header->keypoints || n > cap", "header->status != ORB_KEYFRAME_STORED",
             "reserved words must be 0", "keys != header->points", "keyframes_clear_slot(p, slot)", "p->kf_gen++"))
    ordered(body("orb_match_keyframes", "orb_match_keyframes_read"),
            ("if (!p) return ORB_EINVAL;", "before orb_keyframes_reserve", "before a batch", "!list || n < 1u || n > P", "e.query >= p->last_batch || e.slot >= p->kf_slots",
             "which is empty", "stage_open(p, ST_KF_MATCH", "p->kf_match_gen = p->kf_gen", "stage_end(p, ST_KF_MATCH"))
    call = body("orb_localize_keyframes", "orb_localize_keyframes_read")
    ordered(call, ("params is NULL", "reserved words must be 0", "check_intrinsics(p, ST_KF_LOC", "max_reproj_px must be finite", "ransac_params(p, ST_KF_LOC",
                   "stages_fresh(p, ST_KF_LOC", "p->kf_match_gen != p->kf_gen", "n < 1u || n > st[ST_KF_MATCH].extent", "stage_open(p, ST_KF_LOC"))
    assert "loc_args(p, p->kfloc, g, kLcSeedSalt)" in call and "if (g.max_reproj_px == 0.0f) g.max_reproj_px = 2.0f;" in call
    assert "hipLaunchKernelGGL(k_loc_score, dim3(n, (g.hypotheses + kVerifyHypPerWg - 1u) / kVerifyHypPerWg), dim3(256), 0, s, a.loc);" in call
    assert "match_form(p) != 1 && cap <= (size_t)kMatch4MaxCap" in body("orb_match_keyframes", "orb_match_keyframes_read")  # chosen as orb_match_pairs chooses
    assert "p->kf_gen++" in body("orb_keyframes_remove", "orb_match_keyframes")


def test_stage_table_placement_and_buffers():
    api = _sources()["orb_api.hip"]
    assert re.search(r"enum StageId \{[^}]*\bST_PLACE, ST_PAIRS, ST_KEYFRAMES, ST_KF_MATCH, ST_KF_LOC, ST_PAIRS_VERIFY, ST_LOOP, ST_COUNT \}", api)
    assert re.search(r"enum StageId \{[^}]*\bST_GRAPH, ST_JOIN, ST_REMAP\b", api)
    rows = re.findall(r'^    \{"(\w+)", "(\w+)"', api[api.index("constexpr StageInfo kStages"):api.index("static_assert(kStages[ST_COUNT - 1]")], re.M)
    ids = re.search(r"enum StageId \{ ([^}]*) \}", api).group(1).replace(" = 0", "").split(", ")
    assert len(rows) == len(ids) - 1 and ids[-1] == "ST_COUNT"
    at = ids.index("ST_KEYFRAMES")
    assert rows[at:at + 3] == [("keyframes_insert", "keyframes_read"), ("match_keyframes", "match_keyframes_read"), ("localize_keyframes", "localize_keyframes_read")]
    assert rows[at - 1][0] == "match_pairs" and rows[at + 3][0] == "verify_pairs"
    assert re.search(r'\{"keyframes_insert", "keyframes_read",[^\n]*\n\s*1u << ST_MATCH \|[^\n]*\n\s*1u << ST_TRAJ \|[^\n]*\n\s*1u << ST_LANDMARK\}', api)
    assert re.search(r'\{"match_keyframes", "match_keyframes_read",\s*1u << ST_KEYFRAMES\}', api)
    assert re.search(r'\{"localize_keyframes", "localize_keyframes_read",\s*1u << ST_KF_MATCH \|[^\n]*\n\s*1u << ST_KEYFRAMES\}', api)
    # readers_of stays derived; the store does not go stale with the batch
    assert "constexpr ReadersOf kReaders = readers_of();" in api and "constexpr uint32_t kOutlivesBatch = 1u << ST_KEYFRAMES;" in api
    fresh = api[api.index("int stages_fresh("):api.index("int stage_begin(")]
    assert "need &= ~kOutlivesBatch;" in fresh
    # the buffers are listed once, and the owner buffer is the stage's own
    for case in ("ST_KEYFRAMES", "ST_KF_MATCH", "ST_KF_LOC"):
        assert api.count("case %s:" % case) == 1
    for buf in ("d_khead", "d_kcorners", "d_kdesc", "d_kcounts", "d_kpoints", "d_kdesc4", "d_kowner", "d_klist", "h_klist", "d_kmlist", "h_kmlist", "d_kmrows"):
        assert api.count("add(&p->%s," % buf) == 1, buf
    assert api.count("&p->d_lowner") == 1 and api.count("PnpState& l = p->kfloc;") == 1


def test_the_stage_uses_the_existing_kernels_and_bodies():
    src = _sources()
    code = {f: re.sub(r"//[^\n]*", "", t) for f, t in src.items()}
    everything = "\n".join(code.values())
    for kernel in ("k_lc_index", "k_loc_score", "k_desc_expand4"):
        assert len(re.findall(r"__global__[^;{]*\bvoid %s\(" % kernel, everything)) == 1, kernel
    assert len(re.findall(r"\bLocFit loc_fit\(", everything)) == 1
    kf = code["orb_kernels_keyframes.h"]
    assert kf.count("loc_fit(") == 1 and "k_loc_score" not in kf and "_solve6" not in kf and "loc_accumulate" not in kf and "atomicMin" not in kf
    assert kf.count("traj_compose(") == 1 and kf.count("loc_slot_bytes(") == 1 and kf.count("loc_compact(") == 1 and kf.count("loc_transform(") == 1
    assert kf.count('#include "orb_match_fp4_body.inc"') == 1 and kf.count('#include "orb_match_valu_body.inc"') == 1
    # the two bodies exist once, and are as the parent's two users include them
    for inc, users in (("orb_match_fp4_body.inc", 3), ("orb_match_valu_body.inc", 3)):
        assert sum(t.count('#include "%s"' % inc) for t in code.values()) == users
    assert "__builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4" not in "".join(t for f, t in code.items() if f != "orb_match_fp4_body.inc")
    assert sum(t.count("__builtin_popcount(a0[q].x ^ b0[g].x)") for t in code.values()) == 1
    api = code["orb_api.hip"]
    ins = api[api.index("int orb_keyframes_insert("):api.index("int orb_keyframes_read(")]
    assert "hipLaunchKernelGGL(k_lc_index, dim3(n_frames - 1u, (unsigned)((cap + kLcThreads - 1u) / kLcThreads)), dim3(kLcThreads), 0, s, a.lc);" in ins
    assert "hipLaunchKernelGGL(k_desc_expand4" in api[api.index("int orb_match_keyframes("):api.index("int orb_match_keyframes_read(")]
