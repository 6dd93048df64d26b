"""CPU restatement of the join stage, SJ-1..SJ-7 of DESIGN.md section 30, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_join.h
perform, in the same order: the OrbJoinPose, OrbJoinSegment and OrbJoinLink bytes of orb_join_pairs must equal what this module
returns, bit for bit.  The owners are loop_ref's (LC-2), the median, the consistent count and the verdict trajectory_ref's (TJ-3,
TJ-4), the polar step and compose trajectory_ref's (TJ-5 / BR-4); an entry's ratios are vectorised over the query's slots.
"""
import numpy as np

import landmark_ref as lmr
import loop_ref as lpr
import trajectory_ref as tr
from tinyslam_amd.orb import (JOIN_LINK_DTYPE, JOIN_POSE_DTYPE, JOIN_SEGMENT_DTYPE, ORB_JOIN_COPIED, ORB_JOIN_LINK_FEW, ORB_JOIN_LINK_FORWARD,
                              ORB_JOIN_LINK_HOLDS, ORB_JOIN_LINK_NONFINITE, ORB_JOIN_LINK_RANGE, ORB_JOIN_LINK_RATIO_FEW,
                              ORB_JOIN_LINK_RATIO_SPREAD, ORB_JOIN_LINK_SAME, ORB_JOIN_LINK_STATUS, ORB_JOIN_MOVED, ORB_JOIN_SEGMENT_LINKED,
                              ORB_JOIN_SEGMENT_NONE, ORB_JOIN_SEGMENT_ROOT, ORB_JOIN_USE_MINIMAL, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_OK)

F = np.float32
NONE = 0xFFFFFFFF
_IDENTITY = [F(1), F(0), F(0), F(0), F(1), F(0), F(0), F(0), F(1)]


def defaults(min_inliers=0, min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0):
    """OrbJoinParams with its zero fields replaced by the defaults."""
    return dict(min_inliers=min_inliers or 12, min_shared=min_shared or 8, scale_tolerance=F(scale_tolerance) if scale_tolerance else F(0.1),
                consistent_permille=consistent_permille or 500, flags=flags)


def refused(L, cap):
    """SJ-2: LC-2's refusal."""
    return lpr.refused(L, cap)


def _finite(*lists):
    return all(bool(np.isfinite(v)) for l in lists for v in l)


def camera(frames, q, b):
    """LM-2's camera(q, b) as lists of np.float32."""
    R, t = lmr.camera(frames, q, b)
    return [F(v) for v in R], [F(v) for v in t]


# ---- SJ-3 --------------------------------------------------------------------------------------------------------------------
def first_verdict(frames, q, T, fix, L, p):
    """Clauses 1-6 of SJ-3: the first that applies, or None when the ratios are to be computed."""
    st, nF = int(fix["status"]), len(frames)
    o, b = int(fix["origin"]), int(fix["query_origin"])
    if not (st == ORB_LOCALIZE_OK or (st == ORB_LOCALIZE_MINIMAL and p["flags"] & ORB_JOIN_USE_MINIMAL)):
        return ORB_JOIN_LINK_STATUS
    if int(fix["inliers"]) < p["min_inliers"]:
        return ORB_JOIN_LINK_FEW
    if q >= nF or T >= nF or q >= L or b == NONE or b >= nF:
        return ORB_JOIN_LINK_RANGE
    if o == b:
        return ORB_JOIN_LINK_SAME
    if o > b:
        return ORB_JOIN_LINK_FORWARD
    Rq, tq = camera(frames, q, b)
    if not _finite(fix["pose_r"], fix["pose_t"], Rq, tq):
        return ORB_JOIN_LINK_NONFINITE
    return None


def ratios(nq_q, nq_T, row, mask, own_T, own_q, lms, cap, P, p, Rq, tq):
    """SJ-3: the depth ratios of an entry in the order of the query's slots.  own_T is None for a target at or above L (no owner)."""
    nq_q, nq_T = int(nq_q), int(nq_T)
    if own_T is None or nq_q == 0:
        return np.zeros(0, F)
    k = row["index"][:nq_q].astype(np.int64)
    ok = (np.asarray(mask[:nq_q]) == 1) & (k < nq_T)
    ka = own_T[np.where(ok, k, 0)]
    kb = own_q[:nq_q]
    ok &= (ka != NONE) & (kb != NONE)
    sel = np.nonzero(ok)[0]
    if not len(sel):
        return np.zeros(0, F)

    def land(keys):
        pp, ii = np.divmod(keys, cap)
        return np.array([lms[a][b] for a, b in zip(pp, ii)], dtype=lms[0].dtype)

    XA, XB = land(ka[sel]), land(kb[sel])
    with np.errstate(all="ignore"):
        za = ((P[6] * XA["x"] + P[7] * XA["y"]) + P[8] * XA["z"]) + p[2]
        zb = ((Rq[6] * XB["x"] + Rq[7] * XB["y"]) + Rq[8] * XB["z"]) + tq[2]
        rho = (za / zb).astype(F)
        good = np.isfinite(rho) & (rho > F(0))
    return rho[good]


# ---- SJ-4 --------------------------------------------------------------------------------------------------------------------
def similarity(P, p, Rq, tq, gamma):
    """SJ-4: (A, a, finite) with gamma X_b = A X_o + a."""
    with np.errstate(all="ignore"):
        v = [p[k] - gamma * tq[k] for k in range(3)]
        a = [(Rq[r] * v[0] + Rq[3 + r] * v[1]) + Rq[6 + r] * v[2] for r in range(3)]
        A = [(Rq[r] * P[c] + Rq[3 + r] * P[3 + c]) + Rq[6 + r] * P[6 + c] for r in range(3) for c in range(3)]
        A = tr.polar_step(A)
    return A, a, _finite(A, a, [gamma])


def compose(Ra, ta, s, Rb, tb):
    """BR-4: (Ra Rb after one polar step, Ra tb + s ta)."""
    return tr.compose(Ra, ta, Rb, tb, s)


# ---- SJ-1 .. SJ-7 ------------------------------------------------------------------------------------------------------------
def join_pairs(counts, matches, rows, pairs, frames, lms, fixes, masks, cap, L=None, n_pairs=None, trace=None, **params):
    """counts: the counters of the batch's frames (clipped to the capacity here); matches[g]: MATCH_DTYPE of frame g's stored
    queries (the last match_consecutive), g < L - 1; rows[i]: MATCH_DTYPE of entry i's query frame (the last match_pairs); pairs: its
    list; frames: FRAME_POSE_DTYPE of the last trajectory call, all its F frames; lms[p]: LANDMARK_DTYPE (cap,) of pair p of the last
    landmarks call; fixes, masks: the records and inlier bytes of the last loop call; L: the landmarks call's frames (default: its
    pairs + 1).  `trace`: a dict that receives each computed entry's ratios.
    Returns (JOIN_POSE_DTYPE (F,), JOIN_SEGMENT_DTYPE (F,), JOIN_LINK_DTYPE (n_pairs,))."""
    p = defaults(**params)
    L = len(lms) + 1 if L is None else L
    nF = len(frames)
    pairs = [(int(q), int(T)) for q, T in np.asarray(pairs).reshape(-1, 2)] if not isinstance(pairs, np.ndarray) or pairs.dtype.names is None \
        else [(int(e["query"]), int(e["target"])) for e in pairs]
    n = len(pairs) if n_pairs is None else n_pairs
    nq = [min(int(c), cap) for c in counts]
    own = lpr.owners(nq, matches, frames, lms, cap, L)  # SJ-2
    jp = dict(min_shared=p["min_shared"], scale_tolerance=p["scale_tolerance"], consistent_permille=p["consistent_permille"])
    links = np.zeros(n, JOIN_LINK_DTYPE)
    keys = {}   # SJ-5: segment -> (consistent, -index)
    sims = {}
    for i, (q, T) in enumerate(pairs[:n]):
        fx, lk = fixes[i], links[i]
        lk["origin"], lk["query_origin"] = fx["origin"], fx["query_origin"]
        v = first_verdict(frames, q, T, fx, L, p)
        if v is not None:
            lk["verdict"] = v
            continue
        b = int(fx["query_origin"])
        P, pt = [F(x) for x in fx["pose_r"]], [F(x) for x in fx["pose_t"]]
        Rq, tq = camera(frames, q, b)
        rho = ratios(nq[q], nq[T], rows[i], masks[i], own[T] if T < L else None, own[q], lms, cap, P, pt, Rq, tq)
        if trace is not None:
            trace[i] = rho
        m, g, consistent, verdict = tr.joint(rho, jp)
        v = {tr.HOLDS: ORB_JOIN_LINK_HOLDS, tr.FEW: ORB_JOIN_LINK_RATIO_FEW, tr.SPREAD: ORB_JOIN_LINK_RATIO_SPREAD}[verdict]
        if v == ORB_JOIN_LINK_HOLDS:
            A, a, fin = similarity(P, pt, Rq, tq, g)
            if not fin:
                lk["verdict"] = ORB_JOIN_LINK_NONFINITE
                continue
            sims[i] = (A, a, g)
            if b not in keys or (consistent, -i) > keys[b]:
                keys[b] = (consistent, -i)
        lk["verdict"], lk["shared"], lk["consistent"], lk["gamma"] = v, m, consistent, g
    # SJ-6
    seg = np.zeros(nF, JOIN_SEGMENT_DTYPE)
    is_origin = np.zeros(nF, bool)
    named = frames["origin"].astype(np.int64)
    is_origin[named[named < nF]] = True
    for b in range(nF):
        A, a, sigma, root, link = list(_IDENTITY), [F(0)] * 3, F(1), b, NONE
        if is_origin[b] and b in keys:
            i = -keys[b][1]
            o = int(fixes[i]["origin"])
            Al, al, g = sims[i]
            Ao, ao, so = [F(x) for x in seg[o]["r"]], [F(x) for x in seg[o]["t"]], F(seg[o]["sigma"])
            An, an = compose(Al, al, so, Ao, ao)
            with np.errstate(all="ignore"):
                sn = so * g
            if _finite(An, an, [sn]):
                A, a, sigma, root, link = An, an, sn, int(seg[o]["root"]), i
                links[i]["chosen"] = 1
        s = seg[b]
        s["r"], s["t"], s["sigma"], s["root"], s["link"] = A, a, sigma, root, link
        s["status"] = ORB_JOIN_SEGMENT_LINKED if link != NONE else (ORB_JOIN_SEGMENT_ROOT if is_origin[b] else ORB_JOIN_SEGMENT_NONE)
    out = np.zeros(nF, JOIN_POSE_DTYPE)
    for f in range(nF):
        rec, o = frames[f], out[f]
        b = int(rec["origin"])
        root = int(seg[b]["root"]) if b < nF else b
        if root == b:
            o["r"], o["t"], o["scale"], o["gain"], o["root"], o["status"] = rec["r"], rec["t"], rec["scale"], F(1), b, ORB_JOIN_COPIED
            continue
        R, t = camera(frames, f, b)
        s = seg[b]
        sigma = F(s["sigma"])
        Rn, tn = compose(R, t, sigma, [F(x) for x in s["r"]], [F(x) for x in s["t"]])
        with np.errstate(all="ignore"):
            o["scale"] = sigma * F(rec["scale"])
        o["r"], o["t"], o["gain"], o["root"], o["status"] = Rn, tn, sigma, root, ORB_JOIN_MOVED
    return out, seg, links
