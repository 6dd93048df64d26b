"""CPU restatement of the bridge stage, BR-1..BR-7 of DESIGN.md section 23, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_bridge.h
perform, in the same order: the OrbBridgePose and inlier bytes of orb_bridge_consecutive must equal what this module returns, bit
for bit.  The candidates of a landmark row are vectorised; the fix is localize_ref's LO-2..LO-7 with the frame's index in the mix
and the bridge's salt; the join is trajectory_ref's TJ-3 and TJ-4; the chain runs on scalars, as one lane runs it.
"""
import numpy as np

import localize_ref as lr
import trajectory_ref as tr
import verify_ref as vr
from tinyslam_amd.orb import (BRIDGE_POSE_DTYPE, ORB_BRIDGE_COPIED, ORB_BRIDGE_FIXED, ORB_BRIDGE_JOINED, ORB_BRIDGE_MOVED, ORB_BRIDGE_UNFIXED,
                              ORB_LOCALIZE_NOMAP, ORB_LOCALIZE_OK, ORB_MATCH_NONE as _NONE, ORB_POINT_GOOD, ORB_TRAJ_LOST, ORB_TRAJ_ORIGIN,
                              ORB_TRAJ_START)

F = np.float32
SEED_SALT = 0x42523031  # BR-3: the draw stream's seed is lowbias32(seed ^ SEED_SALT)
MAX_HOPS = 16
_IDENTITY = [F(1), F(0), F(0), F(0), F(1), F(0), F(0), F(0), F(1)]


def defaults(fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0, max_hops=0, window=0, min_shared=0,
             scale_tolerance=0.0, consistent_permille=0):
    """OrbBridgeParams with its zero fields replaced by the defaults."""
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), max_reproj_px=F(max_reproj_px) if max_reproj_px else F(2.0),
                hypotheses=hypotheses or 512, max_distance=max_distance or 64, ratio=F(ratio) if ratio else F(0.8), seed=seed & 0xFFFFFFFF,
                max_hops=max_hops or 4, window=window or 32, min_shared=min_shared or 8,
                scale_tolerance=F(scale_tolerance) if scale_tolerance else F(0.1), consistent_permille=consistent_permille or 500)


# ---- BR-1 --------------------------------------------------------------------------------------------------------------------
def anchors(status, max_hops):
    """BR-1 on the frames' trajectory statuses: per frame (kind, T) -- kind 0: no gap end; 1: a gap end that is NOMAP; 2: a gap
    end with a usable anchor; T: the largest frame below it that is not LOST (0 for frames that are no gap end)."""
    out, last = [], 0
    for g, st in enumerate(status):
        if int(st) != ORB_TRAJ_LOST:
            last = g
            out.append((0, 0))
        else:
            out.append((1 if int(status[last]) == ORB_TRAJ_ORIGIN or g - last > max_hops else 2, last))
    return out


# ---- BR-2 --------------------------------------------------------------------------------------------------------------------
def candidates(g, T, nq, corners_g, matches, frames, lms, cap, p):
    """BR-2 for the gap end g with anchor T.  nq: the stored counts; corners_g: frame g's stored records; matches[s]: the matcher's
    records of frame s's stored queries; frames: the trajectory's records; lms[q]: LANDMARK_DTYPE (cap,) of pair q.
    Returns (k_g (M,), rec (M, 7): Yx, Yy, Yz, u, v, dx, dy; the number of candidates before the clip at the capacity; their
    (row, slot) pairs)."""
    o = int(frames["origin"][T])
    R, t = frames["r"][T].astype(F), frames["t"][T].astype(F)
    ks, Xs, src = [], [], []
    for q in range(max(o, T - p["window"], 0), T):
        n = int(nq[q])
        lm = lms[q][:n]
        ok = (lm["views"] != 0) & ((lm["flags"] & ORB_POINT_GOOD) != 0) & (q + lm["views"].astype(np.int64) - 1 == T)
        k = lm["tail_index"].astype(np.int64)
        for s in range(T, g):
            ok &= k < int(nq[s])
            if not ok.any():
                break
            m = matches[s][:int(nq[s])][np.where(ok, k, 0)]
            d, second = m["distance"], m["second"]
            k = m["index"].astype(np.int64)
            ok &= (m["index"] != _NONE) & (k < int(nq[s + 1])) & (d <= p["max_distance"]) & (d.astype(F) < p["ratio"] * second.astype(F))
        sel = np.nonzero(ok)[0]
        ks.append(k[sel])
        Xs.append(lm[sel])
        src += [(q, int(i)) for i in sel]
    total = len(src)
    k = np.concatenate(ks)[:cap] if ks else np.zeros(0, np.int64)
    X = np.concatenate(Xs)[:cap] if Xs else np.zeros(0, lms[0].dtype if len(lms) else F)
    if not len(k):
        return np.zeros(0, np.int64), np.zeros((0, 7), F), total, src
    with np.errstate(all="ignore"):
        Y = [((R[3 * c] * X["x"] + R[3 * c + 1] * X["y"]) + R[3 * c + 2] * X["z"]) + t[c] for c in range(3)]
        u, v = vr.level0(corners_g[k])
        dx, dy = (u - p["cx"]) / p["fx"], (v - p["cy"]) / p["fy"]
    return k, np.stack(Y + [u, v, dx, dy], 1).astype(F).reshape(-1, 7), total, src


# ---- BR-3 --------------------------------------------------------------------------------------------------------------------
def fix(rec, g, p, nomap=False, trace=None):
    """BR-3: LO-2..LO-7 on the candidate list with g in the mix and the bridge's salt.  Returns (FIX_DTYPE record, inlier flags)."""
    return lr.localize_points(rec, g, nomap=nomap, trace=trace, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], max_reproj_px=p["max_reproj_px"],
                              hypotheses=p["hypotheses"], max_distance=p["max_distance"], ratio=p["ratio"],
                              seed=p["seed"] ^ lr.SEED_SALT ^ SEED_SALT)


# ---- BR-4 --------------------------------------------------------------------------------------------------------------------
def compose(Ra, ta, s, Rb, tb):
    """BR-4: (Ra Rb after one polar step, Ra tb + s ta) on lists of np.float32 -- TJ-5's function."""
    return tr.compose(Ra, ta, Rb, tb, s)


# ---- BR-5 --------------------------------------------------------------------------------------------------------------------
def join_ratios(rec, k, inl, rx, tx, points_g):
    """BR-5: the depth ratios of the candidates that are inliers of the written fix, in candidate order."""
    j = k[inl]
    Yc = rec[inl]
    pts = points_g[j]
    ok = (pts["flags"] & ORB_POINT_GOOD) != 0
    with np.errstate(all="ignore"):
        yz = ((rx[6] * Yc[:, 0] + rx[7] * Yc[:, 1]) + rx[8] * Yc[:, 2]) + tx[2]
        rho = (yz / pts["z"]).astype(F)
        ok &= np.isfinite(rho) & (rho > F(0))
    return rho[ok]


# ---- BR-6 --------------------------------------------------------------------------------------------------------------------
def similarity(out, o, f):
    """S_o as frame f sees it: frame o's own pose, gain and root when it is JOINED, else (I, 0, 1, o)."""
    if o < f and int(out[o]["status"]) == ORB_BRIDGE_JOINED:
        return [F(v) for v in out[o]["r"]], [F(v) for v in out[o]["t"]], F(out[o]["gain"]), int(out[o]["root"])
    return list(_IDENTITY), [F(0)] * 3, F(1), o


def bridge(counts, corners, matches, points, frames, lms, cap, n_frames=None, trace=None, **params):
    """BR-1..BR-7.  counts: the stored counts n_q of the frames; corners[f]: the stored records of frame f; matches[s]: MATCH_DTYPE of
    frame s's stored queries; points[q]: POINT_DTYPE (cap,) of pair q; frames: FRAME_POSE_DTYPE of the last trajectory call; lms[q]:
    LANDMARK_DTYPE (cap,) of pair q.  `trace`: a dict that receives, per gap end, its candidate slots, (row, slot) sources, unclipped
    count, per-candidate inlier flags, record of the fix and join (m, gamma, consistent, verdict).
    Returns (BRIDGE_POSE_DTYPE (n,), uint8 (n, cap))."""
    p = defaults(**params)
    n = len(frames) if n_frames is None else n_frames
    nq = [min(int(c), cap) for c in counts[:n]]
    status = [int(s) for s in frames["status"][:n]]
    anch = anchors(status, p["max_hops"])
    out = np.zeros(n, BRIDGE_POSE_DTYPE)
    masks = np.zeros((n, cap), np.uint8)
    jp = dict(min_shared=p["min_shared"], scale_tolerance=p["scale_tolerance"], consistent_permille=p["consistent_permille"])
    RT, tT, oT = list(_IDENTITY), [F(0)] * 3, 0
    for f in range(n):
        P, o = frames[f], out[f]
        o["r"], o["t"], o["scale"], o["root"], o["fix"] = P["r"], P["t"], P["scale"], f, ORB_LOCALIZE_NOMAP
        R, t = [F(v) for v in P["r"]], [F(v) for v in P["t"]]
        if status[f] != ORB_TRAJ_LOST:
            org = int(P["origin"])
            A, a, sigma, root = similarity(out, org, f)
            RT, tT, oT = R, t, org
            if f == 0 or root == org:
                o["status"], o["gain"], o["root"] = ORB_BRIDGE_COPIED, F(1), 0 if f == 0 else org
            else:
                Rn, tn = compose(R, t, sigma, A, a)
                with np.errstate(all="ignore"):
                    o["scale"] = sigma * F(P["scale"])
                o["r"], o["t"], o["gain"], o["root"], o["status"] = Rn, tn, sigma, root, ORB_BRIDGE_MOVED
            continue
        kind, T = anch[f]
        o["status"], o["anchor"] = ORB_BRIDGE_UNFIXED, T
        if kind != 2:
            continue
        k, rec, total, src = candidates(f, T, nq, corners[f], matches, frames, lms, cap, p)
        X, inl = fix(rec, f, p)
        masks[f][k[inl]] = 1
        o["candidates"], o["inliers"], o["hypothesis"], o["fix"] = X["candidates"], X["inliers"], X["hypothesis"], X["status"]
        joined, m, gam, consistent, verdict = False, 0, F(0), 0, tr.FEW
        rx, tx = [F(v) for v in X["r"]], [F(v) for v in X["t"]]
        if int(X["status"]) == ORB_LOCALIZE_OK and f <= n - 2 and status[f + 1] == ORB_TRAJ_START:
            m, gam, consistent, verdict = tr.joint(join_ratios(rec, k, inl, rx, tx, points[f]), jp)
            joined = verdict == tr.HOLDS
            o["shared"], o["consistent"] = m, consistent
        if trace is not None:
            trace[f] = dict(k=k, src=src, total=total, inliers=inl, fix=X, join=(m, gam, consistent, verdict))
        if int(X["status"]) != ORB_LOCALIZE_OK:
            continue
        Rg, tg = compose(rx, tx, F(1), RT, tT)  # BR-4: camera f in segment oT
        A, a, sigma, root = similarity(out, oT, f)
        if root != oT:
            Rg, tg = compose(Rg, tg, sigma, A, a)
        with np.errstate(all="ignore"):
            sc = sigma * F(X["step"])
            sg = sigma * gam if joined else F(0)
        if not (np.isfinite(sc) and np.isfinite(sg) and all(np.isfinite(v) for v in Rg) and all(np.isfinite(v) for v in tg)):
            continue
        o["r"], o["t"], o["scale"], o["gain"], o["root"] = Rg, tg, sc, sg, root
        o["status"] = ORB_BRIDGE_JOINED if joined else ORB_BRIDGE_FIXED
    return out, masks
