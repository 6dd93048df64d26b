"""CPU restatement of the landmark stage, LM-1..LM-6 of DESIGN.md section 22, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_landmark.h
perform, in the same order: the OrbLandmark and OrbLandmarkRow bytes of orb_landmarks_consecutive must equal what this module
returns, bit for bit.  The starts of a pair are vectorised: they step through the same frames, as the threads of a workgroup do,
and a start that has no further view drops out of the active set.
"""
import numpy as np

import verify_ref as vr
from tinyslam_amd.orb import LANDMARK_DTYPE, LANDMARK_ROW_DTYPE, ORB_LANDMARK_NO_ORIGIN, ORB_POINT_GOOD, ORB_POINT_PARALLAX, ORB_TRAJ_LOST

F = np.float32
_IDENTITY = np.eye(3, dtype=F).ravel()


def defaults(fx, fy, cx, cy, max_reproj_px=0.0, min_views=0):
    """OrbLandmarkParams with its zero fields replaced by the defaults."""
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), max_reproj_px=F(max_reproj_px) if max_reproj_px else F(2.0), min_views=min_views or 2)


def segments(frames, n):
    """LM-2: (mapped, origin) of the n - 1 pairs."""
    return ([int(frames["status"][p + 1]) != ORB_TRAJ_LOST for p in range(n - 1)], [int(frames["origin"][p + 1]) for p in range(n - 1)])


def live_flags(nq, points, mapped, cap):
    """LM-3: per pair, the flags of every slot that is live and 0 elsewhere, (cap,) uint32."""
    out = []
    for p, m in enumerate(mapped):
        fl = np.zeros(cap, np.uint32)
        if m:
            f = points[p]["flags"][:nq[p]]
            fl[:nq[p]] = np.where((f & ORB_POINT_GOOD) != 0, f, 0)
        out.append(fl)
    return out


def continues(p, n, mapped, origin):
    """LM-3: links out of pair p may continue -- pair p + 1 exists, is mapped and belongs to the same segment."""
    return mapped[p] and p + 1 <= n - 2 and mapped[p + 1] and origin[p + 1] == origin[p]


def predecessors(nq, matches, live, mapped, origin, n, cap):
    """LM-3: per pair, a byte per slot: 1 iff a live slot of the pair before continues into it."""
    pred = [np.zeros(cap, np.uint8) for _ in range(n - 1)]
    for p in range(n - 2):
        if not continues(p, n, mapped, origin):
            continue
        i = np.nonzero(live[p])[0]
        j = matches[p]["index"][i].astype(np.int64)
        j = j[j < nq[p + 1]]
        pred[p + 1][j[live[p + 1][j] != 0]] = 1
    return pred


def camera(frames, g, o):
    """LM-2: camera g's pose in the segment of origin o."""
    if g == o:
        return _IDENTITY, np.zeros(3, F)
    return frames["r"][g].astype(F), frames["t"][g].astype(F)


def walk(p, starts, nq, corners, matches, live, mapped, origin, frames, n):
    """LM-3: the views of pair p's starts, step by step in ascending frame order.  Returns a list of steps
    (rows: which of `starts`, g: the frame, k: the keypoint slot of each row, R, t, u, v) and the PARALLAX flag of every start."""
    o = origin[p]
    rows, k, fl = np.arange(len(starts)), starts.astype(np.int64), live[p][starts]
    par = np.zeros(len(starts), np.uint32)
    steps, g = [], p
    while len(rows):
        R, t = camera(frames, g, o)
        u, v = vr.level0(corners[g][k])
        steps.append(dict(rows=rows, g=g, k=k, R=R, t=t, u=u.astype(F), v=v.astype(F)))
        go = fl != 0
        rows, k, fl = rows[go], k[go], fl[go]
        if not len(rows):
            break
        par[rows] |= fl & ORB_POINT_PARALLAX
        j = matches[g]["index"][k].astype(np.int64)
        go = j < nq[g + 1]
        rows, k = rows[go], j[go]
        g += 1
        fl = live[g][k] if (g + 1 < n and mapped[g] and origin[g] == o) else np.zeros(len(rows), np.uint32)
    return steps, par


def accumulate(steps, m, p):
    """LM-4: the six sums of A (00, 01, 02, 11, 12, 22) and the three of b over the views of m starts."""
    A, b = np.zeros((6, m), F), np.zeros((3, m), F)
    with np.errstate(all="ignore"):
        for s in steps:
            R, t, rows = s["R"], s["t"], s["rows"]
            d0, d1, d2 = (s["u"] - p["cx"]) / p["fx"], (s["v"] - p["cy"]) / p["fy"], F(1)
            w = [(R[c] * d0 + R[3 + c] * d1) + R[6 + c] * d2 for c in range(3)]
            c = [-((R[c] * t[0] + R[3 + c] * t[1]) + R[6 + c] * t[2]) for c in range(3)]
            nn = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
            q = {}
            for k, (r_, c_) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
                q[r_, c_] = q[c_, r_] = (F(1) if r_ == c_ else F(0)) - (w[r_] * w[c_]) / nn
                A[k, rows] = A[k, rows] + q[r_, c_]
            for r_ in range(3):
                e = (q[r_, 0] * c[0] + q[r_, 1] * c[1]) + q[r_, 2] * c[2]
                b[r_, rows] = b[r_, rows] + e
    return A, b


def solve(A, b):
    """LM-4: (X (3, m), solved (m,)) by RP-4's cofactors of the symmetric A."""
    with np.errstate(all="ignore"):
        m = [A[0], A[1], A[2], A[1], A[3], A[4], A[2], A[4], A[5]]
        r0, r1, r2 = m[0:3], m[3:6], m[6:9]

        def cross(a, c):
            return [a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]]

        C = cross(r1, r2) + cross(r2, r0) + cross(r0, r1)
        det = (A[0] * C[0] + A[1] * C[1]) + A[2] * C[2]
        X = np.stack([((C[3 * r] * b[0] + C[3 * r + 1] * b[1]) + C[3 * r + 2] * b[2]) / det for r in range(3)]).astype(F)
        ok = np.isfinite(det) & (det > F(0)) & np.isfinite(X).all(0)
    return X, ok


def check(steps, X, m, p):
    """LM-5: the number of inlier views of m starts."""
    inl = np.zeros(m, np.int64)
    r2 = p["max_reproj_px"] * p["max_reproj_px"]
    with np.errstate(all="ignore"):
        for s in steps:
            R, t, rows = s["R"], s["t"], s["rows"]
            x = X[:, rows]
            y = [((R[3 * r] * x[0] + R[3 * r + 1] * x[1]) + R[3 * r + 2] * x[2]) + t[r] for r in range(3)]
            ex = p["fx"] * y[0] + (p["cx"] - s["u"]) * y[2]
            ey = p["fy"] * y[1] + (p["cy"] - s["v"]) * y[2]
            inl[rows] += (y[2] > F(0)) & (ex * ex + ey * ey <= r2 * (y[2] * y[2]))
    return inl


def landmarks(counts, corners, matches, points, frames, cap, n_frames=None, return_views=False, **params):
    """LM-1..LM-6.  counts: the stored counts n_q of the frames; corners[f]: the stored records of frame f; matches[p]: MATCH_DTYPE of
    pair p's stored queries; points[p]: POINT_DTYPE (cap,) of the last pose call; frames: FRAME_POSE_DTYPE of the last trajectory call.
    Returns (LANDMARK_DTYPE (n - 1, cap), LANDMARK_ROW_DTYPE (n - 1,)); with return_views also {(pair, slot): [(frame, keypoint slot),
    ...]} of every start."""
    p = defaults(**params)
    n = len(frames) if n_frames is None else n_frames
    nq = [min(int(c), cap) for c in counts[:n]]
    mapped, origin = segments(frames, n)
    live = live_flags(nq, points, mapped, cap)
    pred = predecessors(nq, matches, live, mapped, origin, n, cap)
    out = np.zeros((n - 1, cap), LANDMARK_DTYPE)
    rows = np.zeros(n - 1, LANDMARK_ROW_DTYPE)
    views_of = {}
    for q in range(n - 1):
        rows[q]["origin"] = origin[q] if mapped[q] else ORB_LANDMARK_NO_ORIGIN
        starts = np.nonzero((live[q] != 0) & (pred[q] == 0))[0]
        m = len(starts)
        if not m:
            continue
        steps, par = walk(q, starts, nq, corners, matches, live, mapped, origin, frames, n)
        views, tail = np.zeros(m, np.int64), np.zeros(m, np.int64)
        for s in steps:
            views[s["rows"]] += 1
            tail[s["rows"]] = s["k"]
        X, ok = solve(*accumulate(steps, m, p))
        inl = np.where(ok, check(steps, X, m, p), 0)
        good = ok & (views >= p["min_views"]) & (inl == views)
        o = out[q]
        for c, k in enumerate("xyz"):
            o[k][starts] = np.where(ok, X[c], F(0))
        o["flags"][starts] = np.where(good, ORB_POINT_GOOD | par, 0)
        o["views"][starts], o["inliers"][starts], o["origin"][starts], o["tail_index"][starts] = views, inl, origin[q], tail
        rows[q]["landmarks"], rows[q]["good"], rows[q]["longest"] = m, int(good.sum()), int(views.max())
        if return_views:
            for s in steps:
                for r, k in zip(s["rows"], s["k"]):
                    views_of.setdefault((q, int(starts[r])), []).append((s["g"], int(k)))
    return (out, rows, views_of) if return_views else (out, rows)
