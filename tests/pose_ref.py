"""CPU restatement of relative pose recovery and triangulation, RP-1..RP-7 of DESIGN.md section 19, in NumPy (test infrastructure,
not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_pose.h
perform, in the same order: the OrbPairPose and OrbPoint bytes of orb_pose_consecutive must equal what this module returns, bit for
bit.  The four candidates are built on scalars (as one lane builds them); the correspondences are vectorised.  svd_pose is the
float64 textbook decomposition, a yardstick for the closed form and nothing the kernels are compared with.
"""
import numpy as np

import verify_ref as vr
from tinyslam_amd.orb import (ORB_POINT_GOOD, ORB_POINT_PARALLAX, ORB_POSE_AMBIGUOUS, ORB_POSE_FEW, ORB_POSE_LOW_PARALLAX, ORB_POSE_NOMODEL,
                              ORB_POSE_OK, ORB_VERIFY_MINIMAL, ORB_VERIFY_OK, POINT_DTYPE, POSE_DTYPE)

F = np.float32
MIN_INLIERS = 8  # RP-6: fewer epipolar inliers than the eight-point sample that made F


def defaults(fx, fy, cx, cy, max_reproj_px=0.0, max_cos_parallax=0.0, min_good=0, ambiguity_permille=0):
    """OrbPoseParams with its zero fields replaced by the defaults."""
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), max_reproj_px=F(max_reproj_px) if max_reproj_px else F(2.0),
                max_cos_parallax=F(max_cos_parallax) if max_cos_parallax else F(0.99998), min_good=min_good or 8,
                ambiguity_permille=ambiguity_permille or 700)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _cof(m):
    """Cofactor matrix of a row-major 3 x 3 (list of 9): rows m1 x m2, m2 x m0, m0 x m1."""
    r0, r1, r2 = m[0:3], m[3:6], m[6:9]
    return _cross(r1, r2) + _cross(r2, r0) + _cross(r0, r1)


def essential_raw(f, fx, fy, cx, cy):
    """RP-2 before the division: (E = K^T (F K) entry by entry, n = sqrt(0.5 sum E^2) (row-major sum))."""
    f = [F(v) for v in f]
    g = []
    for r in range(3):
        g += [f[3 * r] * fx, f[3 * r + 1] * fy, (f[3 * r] * cx + f[3 * r + 1] * cy) + f[3 * r + 2]]
    e = [fx * g[c] for c in range(3)] + [fy * g[3 + c] for c in range(3)] + [(cx * g[c] + cy * g[3 + c]) + g[6 + c] for c in range(3)]
    s = e[0] * e[0]
    for v in e[1:]:
        s = s + v * v
    return e, np.sqrt(F(0.5) * s)


def essential(f, fx, fy, cx, cy):
    """RP-2: essential_raw's E divided by its n.  None: n not finite or not > 0."""
    e, n = essential_raw(f, fx, fy, cx, cy)
    if not (np.isfinite(n) and n > F(0)):
        return None
    return [v / n for v in e]


def baseline_row(e):
    """RP-3: T = I - E E^T (list of 9) and i, the first index of the largest T[i][i]."""
    T = []
    for i in range(3):
        for j in range(3):
            p = (e[3 * i] * e[3 * j] + e[3 * i + 1] * e[3 * j + 1]) + e[3 * i + 2] * e[3 * j + 2]
            T.append((F(1) if i == j else F(0)) - p)
    i, best = 0, T[0]
    if T[4] > best:
        i, best = 1, T[4]
    if T[8] > best:
        i, best = 2, T[8]
    return T, i


def baseline(e):
    """RP-3: t = T[i] / sqrt(T[i][i]) for baseline_row's T and i.  None: that entry is not > 0."""
    T, i = baseline_row(e)
    best = T[4 * i]
    if not best > F(0):
        return None
    q = np.sqrt(best)
    return [T[3 * i + c] / q for c in range(3)]


def polar(r):
    """RP-4: three steps R <- 0.5 (R + Cof(R) / det R), det = (r00 c00 + r01 c01) + r02 c02.  (R, valid)."""
    ok = True
    for _ in range(3):
        c = _cof(r)
        det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2]
        ok = ok and bool(np.isfinite(det) and det > F(0))
        r = [F(0.5) * (r[k] + c[k] / det) for k in range(9)]
    return r, ok


def rotations_raw(e, t):
    """RP-4 before the polar steps: (Ra, Rb) = Cof(E) -+ [t]x E, lists of 9."""
    c = _cof(e)
    s = [None] * 9
    for col in range(3):  # S = [t]x E: column by column t x E[:, col]
        x = _cross(t, [e[col], e[3 + col], e[6 + col]])
        s[col], s[3 + col], s[6 + col] = x
    return [c[k] - s[k] for k in range(9)], [c[k] + s[k] for k in range(9)]


def candidates(f, fx, fy, cx, cy):
    """RP-2..RP-4: None (no model), or (Ra, Rb, t, valid_a, valid_b) with the rotations as lists of 9 and t of 3 np.float32."""
    with np.errstate(all="ignore"):
        e = essential(f, fx, fy, cx, cy)
        if e is None:
            return None
        t = baseline(e)
        if t is None:
            return None
        ra0, rb0 = rotations_raw(e, t)
        ra, va = polar(ra0)
        rb, vb = polar(rb0)
        if not (va or vb):
            return None
        return ra, rb, t, va, vb


def triangulate(r, t, u1, v1, u2, v2, p):
    """RP-5 for one candidate (R, t) on arrays of correspondences: (X (n, 3), good, parallax)."""
    fx, fy, cx, cy = p["fx"], p["fy"], p["cx"], p["cy"]
    r2 = p["max_reproj_px"] * p["max_reproj_px"]
    c2 = p["max_cos_parallax"] * p["max_cos_parallax"]
    with np.errstate(all="ignore"):
        d1x, d1y = (u1 - cx) / fx, (v1 - cy) / fy
        d2x, d2y = (u2 - cx) / fx, (v2 - cy) / fy
        ax = (r[0] * d1x + r[1] * d1y) + r[2]
        ay = (r[3] * d1x + r[4] * d1y) + r[5]
        az = (r[6] * d1x + r[7] * d1y) + r[8]
        aa = (ax * ax + ay * ay) + az * az
        bb = (d2x * d2x + d2y * d2y) + F(1)
        ab = (ax * d2x + ay * d2y) + az
        at = (ax * t[0] + ay * t[1]) + az * t[2]
        bt = (d2x * t[0] + d2y * t[1]) + t[2]
        det = aa * bb - ab * ab
        z1 = (ab * bt - at * bb) / det
        z2 = (aa * bt - ab * at) / det
        X = np.stack([z1 * d1x, z1 * d1y, z1], 1).astype(F)
        yx = ((r[0] * X[:, 0] + r[1] * X[:, 1]) + r[2] * X[:, 2]) + t[0]
        yy = ((r[3] * X[:, 0] + r[4] * X[:, 1]) + r[5] * X[:, 2]) + t[1]
        yz = ((r[6] * X[:, 0] + r[7] * X[:, 1]) + r[8] * X[:, 2]) + t[2]
        ex = (fx * (yx / yz) + cx) - u2
        ey = (fy * (yy / yz) + cy) - v2
        err2 = ex * ex + ey * ey
        good = np.isfinite(z1) & np.isfinite(z2) & (z1 > F(0)) & (z2 > F(0)) & (err2 <= r2)
        par = (ab <= F(0)) | (ab * ab < c2 * (aa * bb))
    return X, good, par


def pose_points(f, status, u1, v1, u2, v2, **params):
    """RP-1..RP-7 on the epipolar inliers of one pair: f the record's nine entries, status its status, (u1, v1) -> (u2, v2) the
    inliers' level-0 coordinates (float32, in query order).  Returns (record of POSE_DTYPE, POINT_DTYPE per inlier)."""
    p = defaults(**params)
    u1, v1, u2, v2 = (np.asarray(a, dtype=F) for a in (u1, v1, u2, v2))
    n = len(u1)
    out = np.zeros((), dtype=POSE_DTYPE)
    pts = np.zeros(n, dtype=POINT_DTYPE)
    out["status"] = ORB_POSE_NOMODEL
    if int(status) not in (ORB_VERIFY_OK, ORB_VERIFY_MINIMAL):
        return out, pts
    cand = candidates(f, p["fx"], p["fy"], p["cx"], p["cy"])
    if cand is None:
        return out, pts
    if n < MIN_INLIERS:
        out["status"] = ORB_POSE_FEW
        return out, pts
    ra, rb, t, va, vb = cand
    nt = [-v for v in t]
    res, good, par = [], [], []
    for r, tk, valid in ((ra, t, va), (ra, nt, va), (rb, t, vb), (rb, nt, vb)):
        X, g, q = triangulate(r, tk, u1, v1, u2, v2, p)
        res.append((r, tk, X, g, q))
        good.append(int(g.sum()) if valid else -1)  # RP-6: a candidate with an invalid rotation never wins
        par.append(int((g & q).sum()))
    k = int(np.argmax(good))  # the first of the largest
    best = good[k]
    second = max(max(g for i, g in enumerate(good) if i != k), 0)
    r, tk, X, g, q = res[k]
    out["r"], out["t"] = np.array(r, F), np.array(tk, F)
    out["inliers"], out["good"], out["second"] = n, best, second
    if best < p["min_good"]:
        out["status"] = ORB_POSE_FEW
    elif 1000 * second >= p["ambiguity_permille"] * best:
        out["status"] = ORB_POSE_AMBIGUOUS
    elif 2 * par[k] < best:
        out["status"] = ORB_POSE_LOW_PARALLAX
    else:
        out["status"] = ORB_POSE_OK
    pts["x"], pts["y"], pts["z"] = np.where(g, X[:, 0], F(0)), np.where(g, X[:, 1], F(0)), np.where(g, X[:, 2], F(0))
    pts["flags"] = np.where(g, ORB_POINT_GOOD | np.where(q, ORB_POINT_PARALLAX, 0), 0)
    return out, pts


def pose_pair(q_corners, t_corners, matches, model, mask, cap=None, **params):
    """RP-1..RP-7 for one pair from the stored records of frames f and f + 1, the matcher's records of frame f's stored queries,
    the epipolar record and its inlier bytes.  Returns (record, POINT_DTYPE per query: cap of them when cap is given)."""
    nq = len(q_corners)
    sel = np.nonzero(np.asarray(mask[:nq]) == 1)[0]
    u1, v1 = vr.level0(q_corners[sel])
    u2, v2 = vr.level0(t_corners[matches["index"][sel].astype(np.int64)])
    rec, pts = pose_points(model["h"], model["status"], u1, v1, u2, v2, **params)
    out = np.zeros(nq if cap is None else cap, dtype=POINT_DTYPE)
    out[sel] = pts
    return rec, out


# ---- yardsticks (float64) ----------------------------------------------------------------------------------------------------
def svd_pose(Fm, K):
    """The textbook decomposition: E = K^T F K = U diag(s1, s2, s3) V^T with det U = det V = 1, the rotations U W V^T and
    U W^T V^T, the baseline direction U[:, 2] up to sign.  Returns (R1, R2, t); the caller takes the candidate nearest its own."""
    E = np.asarray(K, np.float64).T @ np.asarray(Fm, np.float64).reshape(3, 3) @ np.asarray(K, np.float64)
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    Wm = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    return U @ Wm @ Vt, U @ Wm.T @ Vt, U[:, 2]


def rotation_angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3).T @ np.asarray(Rb, np.float64).reshape(3, 3)) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def direction_angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))
