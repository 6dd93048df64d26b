"""CPU restatement of the anchor stage, AN-1..AN-7 of DESIGN.md section 33, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_anchor.h
perform, in the same order: the OrbAnchorPose, OrbAnchorSegment, OrbAnchorLink, OrbAnchorRow and OrbLandmark bytes of
orb_anchor_frames must equal what this module returns, bit for bit.  The owners are loop_ref's (LC-2), the median, the consistent
count and the verdict trajectory_ref's (TJ-3, TJ-4), the camera, the similarity and the compose join_ref's (SJ-3, SJ-4, BR-4); an
entry's ratios and a pair's landmarks are vectorised over the slots.
"""
import numpy as np

import join_ref as jr
import loop_ref as lpr
import trajectory_ref as tr
from tinyslam_amd.orb import (ANCHOR_LINK_DTYPE, ANCHOR_POSE_DTYPE, ANCHOR_ROW_DTYPE, ANCHOR_SEGMENT_DTYPE, LANDMARK_DTYPE, ORB_ANCHOR_ANCHORED,
                              ORB_ANCHOR_FREE, ORB_ANCHOR_LINK_FEW, ORB_ANCHOR_LINK_HOLDS, ORB_ANCHOR_LINK_NONFINITE, ORB_ANCHOR_LINK_RANGE,
                              ORB_ANCHOR_LINK_RATIO_FEW, ORB_ANCHOR_LINK_RATIO_SPREAD, ORB_ANCHOR_LINK_STATUS, ORB_ANCHOR_SEGMENT_ANCHORED,
                              ORB_ANCHOR_SEGMENT_FREE, ORB_ANCHOR_SEGMENT_NONE, ORB_ANCHOR_USE_MINIMAL, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_OK,
                              ORB_POINT_GOOD)

F = np.float32
NONE = 0xFFFFFFFF
_IDENTITY = [F(1), F(0), F(0), F(0), F(1), F(0), F(0), F(0), F(1)]


def defaults(min_inliers=0, min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0):
    """OrbAnchorParams with its zero fields replaced by the defaults: OrbJoinParams'."""
    return jr.defaults(min_inliers, min_shared, scale_tolerance, consistent_permille, flags)


def refused(L, cap):
    """AN-2: LC-2's refusal."""
    return lpr.refused(L, cap)


def _lists(rec, r="r", t="t"):
    return [F(x) for x in rec[r]], [F(x) for x in rec[t]]


# ---- AN-3 --------------------------------------------------------------------------------------------------------------------
def query_origin(frames, q):
    """b: the origin word of frame q's record; 0 when q lies outside the trajectory's frames (the link record's word)."""
    return int(frames[q]["origin"]) if q < len(frames) else 0


def first_verdict(frames, q, fix, L, p):
    """Clauses 1-4 of AN-3: the first that applies, or None when the ratios are to be computed."""
    st, nF = int(fix["status"]), len(frames)
    if not (st == ORB_LOCALIZE_OK or (st == ORB_LOCALIZE_MINIMAL and p["flags"] & ORB_ANCHOR_USE_MINIMAL)):
        return ORB_ANCHOR_LINK_STATUS
    if int(fix["inliers"]) < p["min_inliers"]:
        return ORB_ANCHOR_LINK_FEW
    b = query_origin(frames, q)
    if q >= nF or q >= L or b == NONE or b >= nF:
        return ORB_ANCHOR_LINK_RANGE
    Rq, tq = jr.camera(frames, q, b)
    if not jr._finite(fix["r"], fix["t"], fix["pose_r"], fix["pose_t"], Rq, tq):
        return ORB_ANCHOR_LINK_NONFINITE
    return None


def ratios(nq_q, row, mask, kf, own_q, lms, cap, r, t, Rq, tq):
    """AN-3: the depth ratios of an entry in the order of the query's slots.  kf: the slot (keyframes_ref's Keyframe); r, t: the
    fix's relative pose."""
    nq_q, nt = int(nq_q), min(int(kf["head"]["keypoints"]), cap)
    if nq_q == 0 or nt == 0:
        return np.zeros(0, F)
    k = row["index"][:nq_q].astype(np.int64)
    ok = (np.asarray(mask[:nq_q]) == 1) & (k < nt)
    pts = kf["points"]
    Y = pts[np.where(ok, k, 0)]
    kb = own_q[:nq_q]
    ok &= (Y["key"] != NONE) & (kb != NONE)
    sel = np.nonzero(ok)[0]
    if not len(sel):
        return np.zeros(0, F)
    pp, ii = np.divmod(kb[sel], cap)
    XB = np.array([lms[a][b] for a, b in zip(pp, ii)], dtype=lms[0].dtype)
    Y = Y[sel]
    with np.errstate(all="ignore"):
        za = ((r[6] * Y["x"] + r[7] * Y["y"]) + r[8] * Y["z"]) + t[2]
        zb = ((Rq[6] * XB["x"] + Rq[7] * XB["y"]) + Rq[8] * XB["z"]) + tq[2]
        rho = (za / zb).astype(F)
        good = np.isfinite(rho) & (rho > F(0))
    return rho[good]


# ---- AN-7 --------------------------------------------------------------------------------------------------------------------
def landmarks(segs, lrow, lm):
    """AN-7 of one pair: lm is LANDMARK_DTYPE (cap,), lrow its OrbLandmarkRow.  Returns (ANCHOR_ROW_DTYPE record, LANDMARK_DTYPE (cap,))."""
    out = np.array(lm, LANDMARK_DTYPE)
    row = np.zeros((), ANCHOR_ROW_DTYPE)
    o = int(lrow["origin"])
    good = (out["flags"] & ORB_POINT_GOOD) != 0
    S = segs[o] if o < len(segs) and int(segs[o]["status"]) == ORB_ANCHOR_SEGMENT_ANCHORED else None
    row["good"], row["origin"] = int(good.sum()), o
    row["slot"], row["map_origin"] = (NONE, NONE) if S is None else (S["slot"], S["map_origin"])
    if S is None:
        return row, out
    sel = good & (out["views"] != 0) & (out["origin"] == o)
    A, a = _lists(S)
    gamma = F(S["gamma"])
    with np.errstate(all="ignore"):
        e = [gamma * out[k][sel].astype(F) - a[i] for i, k in enumerate("xyz")]
        x = [(A[k] * e[0] + A[3 + k] * e[1]) + A[6 + k] * e[2] for k in range(3)]
    fin = np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
    new = out[sel]
    new["x"], new["y"], new["z"] = [np.where(fin, v, F(0)) for v in x]
    new["flags"] = np.where(fin, new["flags"], 0)
    out[sel] = new
    row["moved"], row["dropped"] = int(fin.sum()), int((~fin).sum())
    return row, out


# ---- AN-1 .. AN-7 ------------------------------------------------------------------------------------------------------------
def anchor_frames(counts, matches, rows, pairs, frames, lrows, lms, fixes, masks, store, cap, L=None, n=None, trace=None, **params):
    """counts: the counters of the batch's frames (clipped to the capacity here); matches[g]: MATCH_DTYPE of frame g's stored
    queries (the last match_consecutive), g < L - 1; rows[i]: MATCH_DTYPE of entry i's query frame (the last match_keyframes); pairs:
    its list of (query, slot); frames: FRAME_POSE_DTYPE of the last trajectory call, all its F frames; lrows[p], lms[p]:
    LANDMARK_ROW_DTYPE and LANDMARK_DTYPE (cap,) of pair p of the last landmarks call; fixes, masks: the records and inlier bytes of
    the last localize_keyframes; store: slot -> keyframes_ref's Keyframe; L: LC-1's frames (default: the landmark pairs + 1).
    `trace`: a dict that receives each computed entry's ratios.
    Returns (ANCHOR_POSE_DTYPE (F,), ANCHOR_SEGMENT_DTYPE (F,), ANCHOR_LINK_DTYPE (n,), ANCHOR_ROW_DTYPE (L - 1,), [LANDMARK_DTYPE (cap,)] * (L - 1))."""
    p = defaults(**params)
    L = len(lms) + 1 if L is None else L
    nF = len(frames)
    pairs = [(int(e["query"]), int(e["slot"])) for e in pairs] if isinstance(pairs, np.ndarray) and pairs.dtype.names else \
        [(int(q), int(s)) for q, s in np.asarray(pairs).reshape(-1, 2)]
    n = len(pairs) if n is None else n
    nq = [min(int(c), cap) for c in counts]
    own = lpr.owners(nq, matches, frames, lms, cap, L)  # AN-2
    jp = dict(min_shared=p["min_shared"], scale_tolerance=p["scale_tolerance"], consistent_permille=p["consistent_permille"])
    links = np.zeros(n, ANCHOR_LINK_DTYPE)
    keys = {}   # AN-5: segment -> (consistent, -index)
    sims = {}
    for i, (q, s) in enumerate(pairs[:n]):
        fx, lk = fixes[i], links[i]
        lk["query_origin"], lk["slot"] = query_origin(frames, q), s
        v = first_verdict(frames, q, fx, L, p)
        if v is not None:
            lk["verdict"] = v
            continue
        b = int(lk["query_origin"])
        r, t = _lists(fx)
        P, pt = _lists(fx, "pose_r", "pose_t")
        Rq, tq = jr.camera(frames, q, b)
        rho = ratios(nq[q], rows[i], masks[i], store[s], own[q], lms, cap, r, t, Rq, tq)
        if trace is not None:
            trace[i] = rho
        m, g, consistent, verdict = tr.joint(rho, jp)
        v = {tr.HOLDS: ORB_ANCHOR_LINK_HOLDS, tr.FEW: ORB_ANCHOR_LINK_RATIO_FEW, tr.SPREAD: ORB_ANCHOR_LINK_RATIO_SPREAD}[verdict]
        if v == ORB_ANCHOR_LINK_HOLDS:
            A, a, fin = jr.similarity(P, pt, Rq, tq, g)  # AN-4
            if not fin:
                lk["verdict"] = ORB_ANCHOR_LINK_NONFINITE
                continue
            sims[i] = (A, a, g)
            if b not in keys or (consistent, -i) > keys[b]:
                keys[b] = (consistent, -i)
        lk["verdict"], lk["shared"], lk["consistent"], lk["gamma"] = v, m, consistent, g
    # AN-6
    seg = np.zeros(nF, ANCHOR_SEGMENT_DTYPE)
    is_origin = np.zeros(nF, bool)
    named = frames["origin"].astype(np.int64)
    is_origin[named[named < nF]] = True
    for b in range(nF):
        S = seg[b]
        S["r"], S["gamma"], S["slot"], S["link"], S["map_origin"], S["map_frame"] = _IDENTITY, F(1), NONE, NONE, NONE, NONE
        S["status"] = ORB_ANCHOR_SEGMENT_FREE if is_origin[b] else ORB_ANCHOR_SEGMENT_NONE
        if b in keys:
            i = -keys[b][1]
            h = store[pairs[i][1]]["head"]
            A, a, g = sims[i]
            S["r"], S["t"], S["gamma"], S["slot"], S["link"] = A, a, g, pairs[i][1], i
            S["map_origin"], S["map_frame"], S["user"], S["status"] = h["origin"], h["frame"], h["user"], ORB_ANCHOR_SEGMENT_ANCHORED
            links[i]["chosen"] = 1
    out = np.zeros(nF, ANCHOR_POSE_DTYPE)
    for f in range(nF):
        rec, o = frames[f], out[f]
        b = int(rec["origin"])
        if b >= nF or int(seg[b]["status"]) != ORB_ANCHOR_SEGMENT_ANCHORED:
            o["r"], o["t"], o["scale"], o["gain"], o["slot"], o["status"] = rec["r"], rec["t"], rec["scale"], F(1), NONE, ORB_ANCHOR_FREE
            continue
        R, t = jr.camera(frames, f, b)
        S = seg[b]
        gamma = F(S["gamma"])
        A, a = _lists(S)
        Rn, tn = jr.compose(R, t, gamma, A, a)
        with np.errstate(all="ignore"):
            o["scale"] = gamma * F(rec["scale"])
        o["r"], o["t"], o["gain"], o["slot"], o["status"] = Rn, tn, gamma, S["slot"], ORB_ANCHOR_ANCHORED
    # AN-7
    res = [landmarks(seg, lrows[k], lms[k]) for k in range(L - 1)]
    return out, seg, links, np.array([r for r, _ in res], ANCHOR_ROW_DTYPE).reshape(-1), [l for _, l in res]
