"""CPU restatement of the keyframe store, KF-1..KF-5 of DESIGN.md section 32, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_keyframes.h
perform, in the same order: what orb_keyframes_read, orb_match_keyframes_read and orb_localize_keyframes_read hand out must equal
what this module returns, bit for bit.  The owners and the camera of an inserted frame are loop_ref's LC-2 and LC-3, the rows
constructed.match_ref (pairs_ref checks it against the matcher's definition), the fix loop_ref's LC-4 and LC-5: only the
candidates are restated here, on the slot's records where loop_ref takes the target frame's.
"""
import numpy as np

import constructed as C
import loop_ref as lpr
import verify_ref as vr
from tinyslam_amd.orb import (CORNER_DTYPE, DESCRIPTOR_DTYPE, KEYFRAME_DTYPE, KEYFRAME_FIX_DTYPE, MAP_POINT_DTYPE, ORB_KEYFRAME_NOMAP,
                              ORB_KEYFRAME_STORED, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_NOMAP, ORB_LOCALIZE_OK, ORB_MATCH_NONE as _NONE)

F = np.float32
NONE = lpr.NONE  # KF-2: the key of a keypoint without a landmark, the origin of a NOMAP keyframe
SLOTS_MAX = 1024

Keyframe = dict  # head: KEYFRAME_DTYPE (), corners: CORNER_DTYPE (n,), desc: uint32 (n, 8), points: MAP_POINT_DTYPE (n,)


def empty():
    """KF-1: an EMPTY slot is all zero."""
    return dict(head=np.zeros((), KEYFRAME_DTYPE), corners=np.zeros(0, CORNER_DTYPE), desc=np.zeros((0, 8), np.uint32), points=np.zeros(0, MAP_POINT_DTYPE))


def desc_words(desc):
    """DESCRIPTOR_DTYPE (n,) or uint32 (n, 8) as uint32 (n, 8)."""
    d = np.ascontiguousarray(desc)
    return d.view(np.uint32).reshape(-1, 8) if d.dtype == DESCRIPTOR_DTYPE else np.asarray(d, np.uint32).reshape(-1, 8)


# ---- KF-2 --------------------------------------------------------------------------------------------------------------------
def insert(store, entries, counts, corners, descs, matches, frames, lms, cap, L=None):
    """KF-2 on `store` (a dict slot -> Keyframe, changed in place).  entries: (frame, slot) or (frame, slot, user0, user1);
    counts: the counters of the batch's frames; corners[f], descs[f]: the stored records of frame f; matches[g]: MATCH_DTYPE of
    frame g's stored queries (the last match_consecutive); frames: FRAME_POSE_DTYPE of the last trajectory call; lms[p]:
    LANDMARK_DTYPE (cap,) of pair p of the last landmarks call; L: LC-1's frames (default: its pairs + 1)."""
    L = len(lms) + 1 if L is None else L
    nq = [min(int(c), cap) for c in counts]
    own = lpr.owners(nq, matches, frames, lms, cap, L)
    for e in entries:
        g, slot = int(e[0]), int(e[1])
        user = (int(e[2]), int(e[3])) if len(e) > 2 else (0, 0)
        n = nq[g]
        head = np.zeros((), KEYFRAME_DTYPE)
        pts = np.zeros(n, MAP_POINT_DTYPE)
        pts["key"] = NONE
        head["keypoints"], head["frame"], head["user"] = n, g, user
        tgt = lpr.target(frames, g, L)
        if tgt is None:
            head["origin"], head["status"] = NONE, ORB_KEYFRAME_NOMAP
        else:
            o, R, t = tgt
            head["r"], head["t"], head["scale"], head["origin"], head["status"] = R, t, frames["scale"][g], o, ORB_KEYFRAME_STORED
            key = own[g][:n]
            has = np.nonzero(key != NONE)[0]
            if len(has):
                pp, ii = np.divmod(key[has], cap)
                X = np.array([lms[a][b] for a, b in zip(pp, ii)], dtype=lms[0].dtype)
                with np.errstate(all="ignore"):
                    Y = [((R[3 * c] * X["x"] + R[3 * c + 1] * X["y"]) + R[3 * c + 2] * X["z"]) + t[c] for c in range(3)]
                pts["x"][has], pts["y"][has], pts["z"][has] = Y
                pts["key"][has] = key[has]
            head["points"] = len(has)
        store[slot] = dict(head=head, corners=np.array(corners[g][:n], CORNER_DTYPE), desc=desc_words(descs[g])[:n].copy(), points=pts)
    return store


def check_loadable(kf, cap):
    """KF-5: what orb_keyframes_load accepts."""
    h = kf["head"]
    n = int(h["keypoints"])
    return (n == len(kf["corners"]) == len(kf["desc"]) == len(kf["points"]) and n <= cap and int(h["status"]) in (ORB_KEYFRAME_STORED, ORB_KEYFRAME_NOMAP)
            and not h["reserved"].any() and int(h["points"]) == int((kf["points"]["key"] != NONE).sum()))


# ---- KF-3 --------------------------------------------------------------------------------------------------------------------
def match_keyframes(counts, descs, store, pairs, cap):
    """KF-3: row i is MP-2's record for every stored keypoint of frame query_i against the slot's `keypoints` records."""
    return [C.match_ref(desc_words(descs[q])[:min(int(counts[q]), cap)], store[s]["desc"][:int(store[s]["head"]["keypoints"])]) for q, s in pairs]


# ---- KF-4 --------------------------------------------------------------------------------------------------------------------
def candidates(nq_q, corners_q, row, kf, p):
    """LC-3 on a slot: the slot's keypoints for n_q(T), key != NONE for the owner test, the stored point as it is."""
    nq_q, nt = int(nq_q), int(kf["head"]["keypoints"])
    m = row[:nq_q]
    k = m["index"].astype(np.int64)
    d, second = m["distance"], m["second"]
    ok = (m["index"] != _NONE) & (k < nt) & (d <= p["max_distance"]) & (d.astype(F) < p["ratio"] * second.astype(F))
    pts = kf["points"]
    key = pts["key"][np.where(ok, k, 0)].astype(np.int64) if nq_q and nt else np.full(nq_q, NONE, np.int64)
    ok &= key != NONE
    sel = np.nonzero(ok)[0]
    if not len(sel):
        return sel, np.zeros((0, 7), F)
    Y = pts[k[sel]]
    with np.errstate(all="ignore"):
        u, v = vr.level0(corners_q[sel])
        dx, dy = (u - p["cx"]) / p["fx"], (v - p["cy"]) / p["fy"]
    return sel, np.stack([Y["x"], Y["y"], Y["z"], u, v, dx, dy], 1).astype(F).reshape(-1, 7)


def localize_keyframes(counts, corners, rows, pairs, store, cap, n=None, trace=None, **params):
    """KF-4.  counts, corners: the batch's; rows[i]: MATCH_DTYPE of entry i (the last match_keyframes); pairs: (query, slot) per
    entry.  Returns (KEYFRAME_FIX_DTYPE (n,), uint8 (n, cap))."""
    p = lpr.defaults(**params)
    pairs = [(int(q), int(s)) for q, s in pairs]
    n = len(pairs) if n is None else n
    out = np.zeros(n, KEYFRAME_FIX_DTYPE)
    masks = np.zeros((n, cap), np.uint8)
    for i, (q, s) in enumerate(pairs[:n]):
        kf = store[s]
        h = kf["head"]
        if int(h["status"]) != ORB_KEYFRAME_STORED:
            out[i]["status"] = ORB_LOCALIZE_NOMAP
            continue
        nq = min(int(counts[q]), cap)
        sel, rec = candidates(nq, corners[q][:nq], rows[i], kf, p)
        X, inl = lpr.fix(rec, i, p)
        if trace is not None:
            trace[i] = dict(slots=sel, rec=rec, inliers=inl, fix=X)
        out[i]["status"] = X["status"]
        if int(X["status"]) not in (ORB_LOCALIZE_OK, ORB_LOCALIZE_MINIMAL):
            continue
        masks[i][sel[inl]] = 1
        for k in ("r", "t", "step", "candidates", "inliers", "hypothesis"):
            out[i][k] = X[k]
        out[i]["pose_r"], out[i]["pose_t"] = lpr.pose_in_map(X["r"], X["t"], h["r"], h["t"])
        out[i]["origin"], out[i]["slot"] = h["origin"], s
    return out, masks
