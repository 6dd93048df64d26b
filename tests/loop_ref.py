"""CPU restatement of the loop stage, LC-1..LC-7 of DESIGN.md section 28, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_loop.h
perform, in the same order: the OrbLoopFix and inlier bytes of orb_loop_pairs must equal what this module returns, bit for bit.
The owners of LC-2 are a plain minimum over the landmarks' walks; the candidates of a list entry are vectorised; the fix is
localize_ref's LO-2..LO-7 with the list index in the mix and the stage's salt; the pose in the map is trajectory_ref's compose.
"""
import numpy as np

import landmark_ref as lmr
import localize_ref as lr
import trajectory_ref as tr
import verify_ref as vr
from tinyslam_amd.orb import (LOOP_FIX_DTYPE, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_NOMAP, ORB_LOCALIZE_OK, ORB_MATCH_NONE as _NONE, ORB_POINT_GOOD)

F = np.float32
SEED_SALT = 0x4C433031  # LC-4: the draw stream's seed is lowbias32(seed ^ SEED_SALT) ("LC01")
NONE = 0xFFFFFFFF       # LC-2: a keypoint without an owner; LC-6: query_origin of a query above the trajectory call's frames
MAX_HYPOTHESES, MAX_DISTANCE = 4096, 256


def defaults(fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0):
    """OrbLoopParams with its zero fields replaced by the defaults: the localisation stage's."""
    return lr.defaults(fx, fy, cx, cy, max_reproj_px, hypotheses, max_distance, ratio, seed)


def refused(L, cap):
    """LC-2: the call is refused when a key p * cap + i could reach the word that says "no owner"."""
    return L * cap >= 0xFFFFFFFF


# ---- LC-2 --------------------------------------------------------------------------------------------------------------------
def owners(nq, matches, frames, lms, cap, L, registered=None):
    """LC-2.  nq: the stored counts of the frames; matches[g]: MATCH_DTYPE of frame g's stored queries, g < L - 1; frames: the
    trajectory's records; lms[p]: LANDMARK_DTYPE (cap,) of pair p, p < L - 1.  Returns (L, cap) int64: the smallest key
    p * cap + i over the registered landmarks of every view, NONE where there is none.  `registered`: an (L, cap) integer array
    that receives the number of landmarks registered at every view (tests look for contended ones)."""
    own = np.full((L, cap), NONE, np.int64)
    for p in range(L - 1):
        rec = lms[p]
        v = rec["views"].astype(np.int64)
        sel = np.nonzero((v != 0) & ((rec["flags"] & ORB_POINT_GOOD) != 0) & (p + v <= L))[0]
        views, o = v[sel], rec["origin"][sel].astype(np.int64)
        rows, k = np.arange(len(sel)), sel.astype(np.int64)
        s = 0
        while len(rows):
            g = p + s
            go = k < int(nq[g])  # the walk stops where a view is not a stored keypoint
            rows, k = rows[go], k[go]
            reg = o[rows] == int(frames["origin"][g])  # whatever the frame's status
            np.minimum.at(own[g], k[reg], p * cap + sel[rows[reg]])
            if registered is not None:
                np.add.at(registered[g], k[reg], 1)
            go = views[rows] > s + 1
            rows, k = rows[go], k[go]
            if len(rows):
                k = matches[g]["index"][k].astype(np.int64)
            s += 1
    return own


# ---- LC-3 --------------------------------------------------------------------------------------------------------------------
def target(frames, T, L):
    """LC-3: (o, R_T, t_T) of LM-2's camera(T, o), or None when the entry is NOMAP: T outside the map, or an entry of that pose
    not finite."""
    if T >= L:
        return None
    o = int(frames["origin"][T])
    R, t = lmr.camera(frames, T, o)
    R, t = np.asarray(R, F), np.asarray(t, F)
    if not (np.isfinite(R).all() and np.isfinite(t).all()):
        return None
    return o, R, t


def candidates(nq_q, nq_T, corners_q, row, own_T, lms, cap, R, t, p):
    """LC-3 for a list entry whose target has the pose (R, t): the stored counts of q and T, frame q's stored records, the entry's
    row of the last match_pairs, owners[T], the landmark records.  Returns (the slots a of frame q that are candidates, ascending;
    rec (M, 7) float32: Yx, Yy, Yz, u, v, dx, dy)."""
    nq_q, nq_T = int(nq_q), int(nq_T)
    m = row[:nq_q]
    k = m["index"].astype(np.int64)
    d, second = m["distance"], m["second"]
    ok = (m["index"] != _NONE) & (k < nq_T) & (d <= p["max_distance"]) & (d.astype(F) < p["ratio"] * second.astype(F))
    key = own_T[np.where(ok, k, 0)] if nq_q else np.zeros(0, np.int64)
    ok &= key != NONE
    sel = np.nonzero(ok)[0]
    if not len(sel):
        return sel, np.zeros((0, 7), F)
    pp, ii = np.divmod(key[sel], cap)
    X = np.array([lms[a][b] for a, b in zip(pp, ii)], dtype=lms[0].dtype)
    with np.errstate(all="ignore"):
        Y = [((R[3 * c] * X["x"] + R[3 * c + 1] * X["y"]) + R[3 * c + 2] * X["z"]) + t[c] for c in range(3)]
        u, v = vr.level0(corners_q[sel])
        dx, dy = (u - p["cx"]) / p["fx"], (v - p["cy"]) / p["fy"]
    return sel, np.stack(Y + [u, v, dx, dy], 1).astype(F).reshape(-1, 7)


# ---- LC-4 --------------------------------------------------------------------------------------------------------------------
def fix(rec, i, p, nomap=False, trace=None):
    """LC-4: LO-2..LO-7 on the candidate list with the list index i in the mix and the stage's salt.  Returns (FIX_DTYPE record,
    inlier flags)."""
    return lr.localize_points(rec, i, nomap=nomap, trace=trace, fx=p["fx"], fy=p["fy"], cx=p["cx"], cy=p["cy"], max_reproj_px=p["max_reproj_px"],
                              hypotheses=p["hypotheses"], max_distance=p["max_distance"], ratio=p["ratio"],
                              seed=p["seed"] ^ lr.SEED_SALT ^ SEED_SALT)


# ---- LC-5 --------------------------------------------------------------------------------------------------------------------
def pose_in_map(r, t, R_T, t_T):
    """LC-5: compose(R, t, 1; R_T, t_T) of BR-4 / TJ-5 on lists of np.float32: (R R_T after one polar step, R t_T + 1 t), or zeros
    when an entry is not finite."""
    Rp, tp = tr.compose([F(v) for v in r], [F(v) for v in t], [F(v) for v in R_T], [F(v) for v in t_T], F(1))
    if not (all(np.isfinite(v) for v in Rp) and all(np.isfinite(v) for v in tp)):
        return [F(0)] * 9, [F(0)] * 3
    return Rp, tp


# ---- LC-1 .. LC-6 ------------------------------------------------------------------------------------------------------------
def loop_pairs(counts, corners, matches, rows, pairs, frames, lms, cap, L=None, n_pairs=None, trace=None, **params):
    """LC-1..LC-6.  counts: the counters of the batch's frames (clipped to the capacity here); corners[f]: the stored records of
    frame f; matches[g]: MATCH_DTYPE of frame g's stored queries (the last match_consecutive); rows[i]: MATCH_DTYPE of entry i's
    query frame (the last match_pairs); pairs: its list, (query, target) per entry; frames: FRAME_POSE_DTYPE of the last trajectory
    call, all its frames; lms[p]: LANDMARK_DTYPE (cap,) of pair p of the last landmarks call; L: that call's frames (default: its
    pairs + 1).  `trace`: a dict that receives, per entry, its candidate slots, candidate records and per-candidate inlier flags.
    Returns (LOOP_FIX_DTYPE (n_pairs,), uint8 (n_pairs, cap))."""
    p = defaults(**params)
    L = len(lms) + 1 if L is None else L
    pairs = [(int(q), int(T)) for q, T in np.asarray(pairs).reshape(-1, 2)] if not isinstance(pairs, np.ndarray) or pairs.dtype.names is None \
        else [(int(e["query"]), int(e["target"])) for e in pairs]
    n = len(pairs) if n_pairs is None else n_pairs
    nq = [min(int(c), cap) for c in counts]
    own = owners(nq, matches, frames, lms, cap, L)
    out = np.zeros(n, LOOP_FIX_DTYPE)
    masks = np.zeros((n, cap), np.uint8)
    for i, (q, T) in enumerate(pairs[:n]):
        tgt = target(frames, T, L)
        if tgt is None:
            out[i]["status"] = ORB_LOCALIZE_NOMAP
            continue
        o, R_T, t_T = tgt
        sel, rec = candidates(nq[q], nq[T], corners[q], rows[i], own[T], lms, cap, R_T, t_T, p)
        X, inl = fix(rec, i, p)
        if trace is not None:
            trace[i] = dict(slots=sel, rec=rec, inliers=inl, fix=X)
        out[i]["status"] = X["status"]
        if int(X["status"]) not in (ORB_LOCALIZE_OK, ORB_LOCALIZE_MINIMAL):
            continue
        masks[i][sel[inl]] = 1
        for k in ("r", "t", "step", "candidates", "inliers", "hypothesis"):
            out[i][k] = X[k]
        out[i]["pose_r"], out[i]["pose_t"] = pose_in_map(X["r"], X["t"], R_T, t_T)
        out[i]["origin"] = o
        out[i]["query_origin"] = int(frames["origin"][q]) if q < len(frames) else NONE
    return out, masks
