"""CPU restatement of the remap stage, RM-1..RM-6 of DESIGN.md section 31, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_remap.h
perform, in the same order: the OrbRemapPose, OrbRemapRow and OrbLandmark bytes of orb_remap_frames must equal what this module
returns, bit for bit.  It is fed graph_ref's and join_ref's outputs or the device's read-backs; the compose is trajectory_ref's
(TJ-5 / BR-4); a pair's landmarks are vectorised over its slots.
"""
import numpy as np

import trajectory_ref as tr
from tinyslam_amd.orb import (LANDMARK_DTYPE, ORB_GRAPH_FAILED, ORB_GRAPH_REFINED, ORB_GRAPH_STALLED, ORB_JOIN_SEGMENT_LINKED, ORB_POINT_GOOD,
                              ORB_REMAP_FROM_GRAPH, ORB_REMAP_GRAPH, ORB_REMAP_JOIN, ORB_REMAP_MOVED, REMAP_POSE_DTYPE, REMAP_ROW_DTYPE)

F = np.float32
NONE = 0xFFFFFFFF
_MOVED_BY_GRAPH = (ORB_GRAPH_REFINED, ORB_GRAPH_STALLED, ORB_GRAPH_FAILED)


def sources(flags):
    """RM-1: (graph is a source, join is a source)."""
    flags = flags or (ORB_REMAP_GRAPH | ORB_REMAP_JOIN)
    return bool(flags & ORB_REMAP_GRAPH), bool(flags & ORB_REMAP_JOIN)


def from_graph(gposes, f):
    """RM-2: the graph moved frame f (gposes None: the graph is no source)."""
    return gposes is not None and int(gposes[f]["status"]) in _MOVED_BY_GRAPH


def camera(frames, gposes, f):
    """RM-2: G(f), the record whose r, t are taken word for word."""
    return gposes[f] if from_graph(gposes, f) else frames[f]


def similarity(segs, b, nF):
    """RM-3: the segment record of origin b when it is LINKED, else None."""
    if segs is None or b >= nF or int(segs[b]["status"]) != ORB_JOIN_SEGMENT_LINKED:
        return None
    return segs[b]


def _lists(rec):
    return [F(x) for x in rec["r"]], [F(x) for x in rec["t"]]


def pose(frames, gposes, segs, f):
    """RM-4: the OrbRemapPose of frame f."""
    nF = len(frames)
    out = np.zeros((), REMAP_POSE_DTYPE)
    rec = frames[f]
    b = int(rec["origin"])
    cam = camera(frames, gposes, f)
    status = ORB_REMAP_FROM_GRAPH if from_graph(gposes, f) else 0
    S = similarity(segs, b, nF)
    if S is None:
        out["r"], out["t"], out["scale"], out["gain"], out["root"], out["status"] = cam["r"], cam["t"], rec["scale"], F(1), b, status
        return out
    R, t = _lists(cam)
    A, a = _lists(S)
    sigma = F(S["sigma"])
    Rn, tn = tr.compose(R, t, A, a, sigma)
    with np.errstate(all="ignore"):
        out["scale"] = sigma * F(rec["scale"])
    out["r"], out["t"], out["gain"], out["root"], out["status"] = Rn, tn, sigma, S["root"], status | ORB_REMAP_MOVED
    return out


def landmarks(frames, gposes, segs, lrow, lm, p):
    """RM-5, RM-6 of pair p: lm is LANDMARK_DTYPE (cap,), lrow its OrbLandmarkRow.  Returns (REMAP_ROW_DTYPE record, LANDMARK_DTYPE (cap,))."""
    nF = len(frames)
    out = np.array(lm, LANDMARK_DTYPE)
    row = np.zeros((), REMAP_ROW_DTYPE)
    o = int(lrow["origin"])
    good = (out["flags"] & ORB_POINT_GOOD) != 0
    row["good"] = int(good.sum())
    anchor = o < nF and p != o and int(frames[p]["origin"]) == o and from_graph(gposes, p)
    S = similarity(segs, o, nF) if o < nF else None
    row["root"] = o if S is None else S["root"]
    if not (anchor or S is not None):
        return row, out
    sel = good & (out["views"] != 0) & (out["origin"] == o)
    x = [out["x"][sel].astype(F), out["y"][sel].astype(F), out["z"][sel].astype(F)]
    with np.errstate(all="ignore"):
        if anchor:
            R, t = _lists(frames[p])
            Rg, tg = _lists(gposes[p])
            c = [((R[3 * r] * x[0] + R[3 * r + 1] * x[1]) + R[3 * r + 2] * x[2]) + t[r] for r in range(3)]
            d = [c[r] - tg[r] for r in range(3)]
            x = [(Rg[k] * d[0] + Rg[3 + k] * d[1]) + Rg[6 + k] * d[2] for k in range(3)]
        if S is not None:
            A, a = _lists(S)
            sigma = F(S["sigma"])
            e = [sigma * x[r] - a[r] for r in range(3)]
            x = [(A[k] * e[0] + A[3 + k] * e[1]) + A[6 + k] * e[2] for k in range(3)]
    fin = np.isfinite(x[0]) & np.isfinite(x[1]) & np.isfinite(x[2])
    new = out[sel]
    if S is not None:
        new["origin"] = S["root"]
    new["x"], new["y"], new["z"] = [np.where(fin, v, F(0)) for v in x]
    new["flags"] = np.where(fin, new["flags"], 0)
    out[sel] = new
    row["moved"], row["dropped"] = int(fin.sum()), int((~fin).sum())
    return row, out


def remap_frames(frames, lrows, lms, gposes=None, segs=None, flags=0):
    """frames: FRAME_POSE_DTYPE of the last trajectory call, all its F frames; lrows, lms: LANDMARK_ROW_DTYPE and LANDMARK_DTYPE (cap,)
    of every pair of the last landmarks call; gposes: GRAPH_POSE_DTYPE (F,) of the last graph call, segs: JOIN_SEGMENT_DTYPE (F,) of the
    last join call (each needed only when `flags` names it).
    Returns (REMAP_POSE_DTYPE (F,), REMAP_ROW_DTYPE (P_l,), [LANDMARK_DTYPE (cap,)] * P_l)."""
    use_graph, use_join = sources(flags)
    g = gposes if use_graph else None
    s = segs if use_join else None
    assert (not use_graph or len(g) == len(frames)) and (not use_join or len(s) == len(frames))
    nF = len(frames)
    pairs = min(len(lms), nF - 1)
    poses = np.array([pose(frames, g, s, f) for f in range(nF)], REMAP_POSE_DTYPE)
    res = [landmarks(frames, g, s, lrows[p], lms[p], p) for p in range(pairs)]
    return poses, np.array([r for r, _ in res], REMAP_ROW_DTYPE), [l for _, l in res]
