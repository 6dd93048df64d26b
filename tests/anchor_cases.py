"""Inputs of the anchor tests, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_anchor_frames reads the trajectory's frame records, the landmark records and rows, the matcher's
consecutive records (the owners' walk), the list and rows of orb_match_keyframes, the fixes and inlier bytes of
orb_localize_keyframes, the listed slots of the store and the raw counters.  `rail` is join_cases.rail with every frame inserted
into a store by keyframes_ref's KF-2 (slot = frame): a keyframe of segment 0 and a query of segment 3 are the join stage's two
sides with the keyframe on the far one; `fix` is the true OrbKeyframeFix of a rail entry (q, slot of T), `row` and `mask` its true
row and inlier bytes.  `two_batches` is the real thing on the CPU: keyframes_cases.second_batch against the eleven keyframes of
loop_cases.out_and_back.  The `inputs`, `load_kf`, `device_store`, `inject`, `hold` and `check` helpers drive a device program.
"""
import collections

import numpy as np

import anchor_ref as ar
import join_cases as J
import keyframes_cases as KC
import keyframes_ref as kfr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
from tinyslam_amd import orb

F = np.float32
NONE = 0xFFFFFFFF
OK, MINIMAL, FEW_FIX, NOMAP_FIX = orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_MINIMAL, orb.ORB_LOCALIZE_FEW, orb.ORB_LOCALIZE_NOMAP
TWO = J.TWO  # segments 0 (frames 0-2) and 3 (frames 3-5)
V = dict(HOLDS=orb.ORB_ANCHOR_LINK_HOLDS, STATUS=orb.ORB_ANCHOR_LINK_STATUS, FEW=orb.ORB_ANCHOR_LINK_FEW, RANGE=orb.ORB_ANCHOR_LINK_RANGE,
         NONFINITE=orb.ORB_ANCHOR_LINK_NONFINITE, RATIO_FEW=orb.ORB_ANCHOR_LINK_RATIO_FEW, RATIO_SPREAD=orb.ORB_ANCHOR_LINK_RATIO_SPREAD)
FREE, ANCHORED = orb.ORB_ANCHOR_FREE, orb.ORB_ANCHOR_ANCHORED
SEG_NONE, SEG_FREE, SEG_ANCHORED = orb.ORB_ANCHOR_SEGMENT_NONE, orb.ORB_ANCHOR_SEGMENT_FREE, orb.ORB_ANCHOR_SEGMENT_ANCHORED


def entries(n):
    """Frame f into slot f, with a caller's pair of words that tells the slots apart."""
    return [(f, f, 7 * f + 1, 1000 + f) for f in range(n)]


def rail(plan=TWO, K_=12, cap=16, scales=None, seed=0, desc_seed=7):
    """(batch, landmark records, landmark rows, descriptors, store) of the rail camera under `plan`: join_cases.rail, and every frame
    of it inserted into slot f of a store of its own (KF-2 of keyframes_ref)."""
    b, _ = J.rail(plan, K_, cap, scales, seed)
    lms, lrows = L.run(b)
    lms = [lm.copy() for lm in lms]
    desc = K.plant(b, np.random.default_rng(desc_seed))
    nq, corners, descs, matches = KC.batch_inputs(b, desc)
    store = kfr.insert({}, entries(b["n"]), nq, corners, descs, matches, b["frames"], lms, b["cap"], L=b["n"])
    return b, lms, np.array(lrows), desc, store


def as_keyframe_fix(rec, slot):
    """An OrbLoopFix as the OrbKeyframeFix of `slot`: the same words, the slot where the query's origin is."""
    a = np.frombuffer(np.asarray(rec, orb.LOOP_FIX_DTYPE).tobytes(), orb.KEYFRAME_FIX_DTYPE).copy()
    a["slot"] = slot
    return a[0]


def fix(b, q, T, slot=None, **kw):
    """The true OrbKeyframeFix of the rail entry (q, slot of T): camera q relative to camera T and in the frame and unit of T's
    segment."""
    return as_keyframe_fix(J.fix(b, q, T, **kw), T if slot is None else slot)


def fixes(b, pairs, **kw):
    return np.array([fix(b, q, s, **kw) for q, s in pairs], orb.KEYFRAME_FIX_DTYPE)


row, mask = J.row, J.mask


def run(case, pairs, rows=None, fx=None, masks=None, frames=None, n=None, trace=None, counts=None, store=None, lms=None, **params):
    """anchor_ref.anchor_frames on a rail case; rows, fixes and masks default to the true ones of every entry (slot = frame)."""
    b, lms0, lrows, _, store0 = case
    lms = lms0 if lms is None else lms
    nq = lc.stored(b) if counts is None else counts
    n = b["n"] if n is None else n
    rows = [row(b, min(q, b["n"] - 1), s) for q, s in pairs] if rows is None else rows
    fx = fixes(b, pairs) if fx is None else fx
    masks = [mask(b, min(q, b["n"] - 1)) for q, s in pairs] if masks is None else masks
    return ar.anchor_frames(nq, [b["matches"][f] for f in range(n - 1)], rows, pairs, b["frames"] if frames is None else frames, lrows[:n - 1], lms[:n - 1], fx,
                            masks, store0 if store is None else store, b["cap"], L=n, trace=trace, **params)


def two_batches(seed, lost_pair=None):
    """out_and_back(seed) inserted whole (slot = frame) and second_batch(seed) localised against keyframes_cases.SECOND_PAIRS, all by
    the restatements.  lost_pair: that pair of the second batch is LOW_PARALLAX, so the frame behind it starts a second segment.
    Returns a dict of everything anchor_ref.anchor_frames takes, with both batches."""
    b1, b2 = K.out_and_back(seed), KC.second_batch(seed)
    if lost_pair is not None:
        b2["poses"]["status"][lost_pair] = orb.ORB_POSE_LOW_PARALLAX
    d1, d2 = KC.plant_pair(b1, b2, 100 + seed)
    fr1, lms1, store = KC.reference(b1, d1, [(f, f, 7 * f + 1, 1000 + f) for f in range(b1["n"])], traj=L.FULL_TRAJ)
    fr2, lms2, lrows2 = L.reference(b2, b2["n"], traj=L.FULL_TRAJ)
    intr = lc.intrinsics(b2["W"], b2["H"], b2["focal"])
    nq, corners, descs, matches = KC.batch_inputs(b2, d2)
    pairs = KC.SECOND_PAIRS
    rows = kfr.match_keyframes(nq, descs, store, pairs, b2["cap"])
    fx, masks = kfr.localize_keyframes(nq, corners, rows, pairs, store, b2["cap"], **intr)
    return dict(b1=b1, b2=b2, d1=d1, d2=d2, fr1=fr1, store=store, nq=nq, matches=matches, rows=rows, pairs=pairs, frames=fr2, lrows=np.array(lrows2),
                lms=[lm.copy() for lm in lms2], fixes=fx, masks=masks, cap=b2["cap"], intr=intr)


def anchor(c, **params):
    """anchor_ref.anchor_frames on a two_batches dict."""
    return ar.anchor_frames(c["nq"], c["matches"], c["rows"], c["pairs"], c["frames"], c["lrows"], c["lms"], c["fixes"], c["masks"], c["store"], c["cap"], **params)


def true_gamma(b1, b2, o=0, s=0):
    """Units of the first batch's segment o per unit of the second batch's segment s: a unit is the baseline of the segment's first pair."""
    return float(np.linalg.norm(b2["steps"][s][1]) / np.linalg.norm(b1["steps"][o][1]))


# 2 x the float64 yardstick's worst over seeds 0-3 (tests/test_anchor_ref.py measures them and checks these figures): gamma relative to
# the true unit ratio, rotation in degrees, position in units of the store's segment 0
BOUNDS = (2 * 0.027034, 2 * 0.16139, 2 * 0.089592)

# ---- the device -------------------------------------------------------------------------------------------------------------
W0, H0, INTR = J.W0, J.H0, J.INTR
Inputs = collections.namedtuple("Inputs", "nq corners matches frames lrows lms L cap")
program = J.program


def inputs(prog, n_frames, L_frames, cap):
    """What an anchor call reads of the batch, as the device holds it."""
    i = J.inputs(prog, n_frames, L_frames, cap, None)
    lrows = np.array([prog.landmarks_read(p, 0)[0] for p in range(L_frames - 1)], orb.LANDMARK_ROW_DTYPE).reshape(-1)
    return Inputs(i.nq, i.corners, i.matches, i.frames, lrows, i.lms, L_frames, cap)


def load_kf(prog, slot, kf):
    prog.keyframes_load(slot, kf["head"], kf["corners"], np.ascontiguousarray(kf["desc"], np.uint32).view(orb.DESCRIPTOR_DTYPE).reshape(-1), kf["points"])


def device_store(prog, slots):
    """The listed slots as orb_keyframes_read gives them."""
    out = {}
    for s in slots:
        head, corners, desc, points = prog.keyframes_read(s)
        out[s] = dict(head=head, corners=corners, desc=kfr.desc_words(desc), points=points)
    return out


def inject(prog, rows=None, fixes_=None, masks=None, first=0):
    """Overwrites entries first .. of what the last match_keyframes and localize_keyframes left (orb_debug_keyframe_buffers): rows of
    `cap` MATCH_DTYPE records, KEYFRAME_FIX_DTYPE records, rows of `cap` inlier bytes, each optional.  Ordered as
    graph_cases.inject_fixes.  No stage's freshness changes."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    P, cap = orb.ORB_PAIRS_PER_FRAME * cfg.max_batch, cfg.max_features
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    d_rows, d_fix, d_mask = prog.debug_keyframe_buffers()
    if rows is not None:
        a = np.ascontiguousarray(rows, dtype=orb.MATCH_DTYPE)
        assert a.ndim == 2 and a.shape[1] == cap and first + len(a) <= P, (a.shape, first, P, cap)
        node.as_tensor(d_rows, (P, cap * 2), "<i4", dev)[first:first + len(a)].copy_(torch.from_numpy(a.view(np.int32).reshape(len(a), cap * 2)))
    if fixes_ is not None:
        a = np.ascontiguousarray(fixes_, dtype=orb.KEYFRAME_FIX_DTYPE)
        assert a.ndim == 1 and first + len(a) <= P, (a.shape, first, P)
        node.as_tensor(d_fix, (P, 32), "<i4", dev)[first:first + len(a)].copy_(torch.from_numpy(a.view(np.int32).reshape(len(a), 32)))
    if masks is not None:
        a = np.ascontiguousarray(masks, dtype=np.uint8)
        assert a.ndim == 2 and a.shape[1] == cap and first + len(a) <= P, (a.shape, first, P, cap)
        node.as_tensor(d_mask, (P, cap), "|u1", dev)[first:first + len(a)].copy_(torch.from_numpy(a))
    torch.cuda.synchronize(dev)


def hold(prog, inp, pairs, n):
    """The rows, fixes and inlier bytes of entries 0 .. n - 1 as the device holds them now."""
    rows = [prog.match_keyframes_read(i, int(inp.nq[q])) for i, (q, s) in enumerate(pairs[:n])]
    recs = [prog.localize_keyframes_read(i, inp.cap) for i in range(n)]
    return rows, np.array([r for r, _ in recs]), np.array([m for _, m in recs])


def check(prog, inp, pairs, n=None, stream=None, call=True, held=None, store=None, **params):
    """anchor_frames (call=False: the last one's results), then all five outputs against the restatement fed with what the device
    holds (`held`, `store`: what it held when the call was made), byte for byte.  Returns (poses, segments, links, rows, landmarks,
    the bytes of all five)."""
    n = len(pairs) if n is None else n
    nF = len(inp.frames)
    rows, fx, masks = hold(prog, inp, pairs, n) if held is None else held
    store = device_store(prog, sorted(set(s for q, s in pairs[:n]))) if store is None else store
    if call:
        prog.anchor_frames(n, stream=stream, **params)
    want = ar.anchor_frames(inp.nq, inp.matches, rows, pairs, inp.frames, inp.lrows, inp.lms, fx, masks, store, inp.cap, L=inp.L, n=n, **params)
    poses = np.array([prog.anchor_read(f) for f in range(nF)])
    segs, links = prog.anchor_segments(nF), prog.anchor_links(n)
    land = [prog.anchor_landmarks(p, inp.cap) for p in range(inp.L - 1)]
    arows = np.array([r for r, _ in land], orb.ANCHOR_ROW_DTYPE).reshape(-1)
    for name, got, exp in (("links", links, want[2]), ("segments", segs, want[1]), ("poses", poses, want[0]), ("rows", arows, want[3])):
        assert len(got) == len(exp), (name, len(got), len(exp))
        for k in range(len(exp)):
            assert got[k].tobytes() == exp[k].tobytes(), (name, k, params, got[k], exp[k])
    for p in range(inp.L - 1):
        got, exp = land[p][1], want[4][p]
        assert got.tobytes() == exp.tobytes(), ("landmarks", p, np.nonzero(got != exp)[0][:8])
    blob = poses.tobytes() + segs.tobytes() + links.tobytes() + arows.tobytes() + b"".join(l.tobytes() for _, l in land)
    return poses, segs, links, arows, [l for _, l in land], blob
