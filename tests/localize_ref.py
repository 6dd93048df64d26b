"""CPU restatement of the localisation stage, LO-1..LO-7 of DESIGN.md section 21, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_localize.h
perform, in the same order: the OrbFrameFix and inlier bytes of orb_localize_consecutive must equal what this module returns, bit
for bit.  Hypotheses are vectorised (one row per hypothesis): the complete-pivoting elimination of LO-3 and the polar steps of LO-4
run on all of them at once.  The Gauss-Newton refit of LO-6 sums per candidate as vectors and solves on scalars, as one lane does;
its solver is verify_ref's GV-6 elimination at size 6 x 7.
"""
import numpy as np

import verify_ref as vr
from tinyslam_amd.orb import (FIX_DTYPE, ORB_LOCALIZE_DEGENERATE, ORB_LOCALIZE_FEW, ORB_LOCALIZE_MINIMAL, ORB_LOCALIZE_NOMAP, ORB_LOCALIZE_OK,
                              ORB_MATCH_NONE as _NONE, ORB_POINT_GOOD, ORB_POSE_OK)

F = np.float32
MAX_HYPOTHESES = vr.MAX_HYPOTHESES
SEED_SALT = 0x4C4F3031       # LO-2: the draw stream's seed is lowbias32(seed ^ SEED_SALT)
DRAWS = 32                   # LO-2: draws per hypothesis
SAMPLE = 6                   # LO-3: points of a minimal sample; a pair with fewer candidates is FEW
PIVOT_RATIO = F(2.0 ** -22)  # LO-3: degenerate when |last pivot| <= PIVOT_RATIO * |first pivot|
GN_STEPS = 4                 # LO-6
_IU, _JU = np.triu_indices(6)


def defaults(fx, fy, cx, cy, max_reproj_px=0.0, hypotheses=0, max_distance=0, ratio=0.0, seed=0):
    """OrbLocalizeParams with its zero fields replaced by the defaults."""
    return dict(fx=F(fx), fy=F(fy), cx=F(cx), cy=F(cy), max_reproj_px=F(max_reproj_px) if max_reproj_px else F(2.0),
                hypotheses=hypotheses or 512, max_distance=max_distance or 64, ratio=F(ratio) if ratio else F(0.8), seed=seed & 0xFFFFFFFF)


# ---- LO-1 --------------------------------------------------------------------------------------------------------------------
def correspondences(nq_prev, nq, nq_next, matches_prev, matches, pose_prev, points_prev, corners_next, p):
    """LO-1 for pair f: the stored counts of frames f - 1, f and f + 1, the matcher's records of frames f - 1 and f, pair f - 1's pose
    record and points, frame f + 1's records.  Returns (the slots i of frame f - 1 that are candidates, ascending; rec (M, 7) float32:
    Yx, Yy, Yz, u2, v2, dx, dy)."""
    nq_prev, nq, nq_next = int(nq_prev), int(nq), int(nq_next)
    i = slice(0, nq_prev)
    ok = (points_prev["flags"][i] & ORB_POINT_GOOD) != 0
    j = matches_prev["index"][i].astype(np.int64)
    ok &= j < nq
    jj = np.where(ok, j, 0)
    if nq == 0:
        sel = np.zeros(0, np.int64)
        return sel, np.zeros((0, 7), F)
    m2 = matches[:nq][jj]
    k = m2["index"].astype(np.int64)
    d, second = m2["distance"], m2["second"]
    ok &= (m2["index"] != _NONE) & (k < nq_next) & (d <= p["max_distance"]) & (d.astype(F) < p["ratio"] * second.astype(F))
    sel = np.nonzero(ok)[0]
    k = k[sel]
    r, t = pose_prev["r"].astype(F), pose_prev["t"].astype(F)
    X = points_prev[i][sel]
    with np.errstate(all="ignore"):
        Y = [((r[3 * c] * X["x"] + r[3 * c + 1] * X["y"]) + r[3 * c + 2] * X["z"]) + t[c] for c in range(3)]
        u2, v2 = vr.level0(corners_next[k])
        dx, dy = (u2 - p["cx"]) / p["fx"], (v2 - p["cy"]) / p["fy"]
    return sel, np.stack(Y + [u2, v2, dx, dy], 1).astype(F).reshape(-1, 7)


# ---- LO-2 --------------------------------------------------------------------------------------------------------------------
def sample(seed, pair, M, hyps):
    """LO-2: (hyps, 6) candidate indices in draw order and a validity flag per hypothesis."""
    mix = vr.lowbias32(vr.lowbias32(np.uint32((seed ^ SEED_SALT) & 0xFFFFFFFF)) ^ np.uint32(pair))
    h = np.arange(hyps, dtype=np.uint32)
    J = np.zeros((hyps, SAMPLE), dtype=np.int64)
    n = np.zeros(hyps, dtype=np.int64)
    rows = np.arange(hyps)
    for d in range(DRAWS):
        r = vr.lowbias32(mix ^ ((h << np.uint32(5)) | np.uint32(d)))
        j = ((r.astype(np.uint64) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
        dup = ((np.arange(SAMPLE)[None, :] < n[:, None]) & (J == j[:, None])).any(1)
        take = (n < SAMPLE) & ~dup
        J[rows[take], n[take]] = j[take]
        n += take
    return J, n == SAMPLE


# ---- LO-3 --------------------------------------------------------------------------------------------------------------------
def dlt_rows(S):
    """LO-3: the 11 x 12 systems of samples S (n, 6, 7): two rows per sample point in draw order, without the twelfth."""
    Yx, Yy, Yz, dx, dy = S[..., 0], S[..., 1], S[..., 2], S[..., 5], S[..., 6]
    one, zero = np.ones_like(Yx), np.zeros_like(Yx)
    r1 = np.stack([Yx, Yy, Yz, one, zero, zero, zero, zero, -(dx * Yx), -(dx * Yy), -(dx * Yz), -dx], -1)
    r2 = np.stack([zero, zero, zero, zero, Yx, Yy, Yz, one, -(dy * Yx), -(dy * Yy), -(dy * Yz), -dy], -1)
    A = np.stack([r1, r2], 2).reshape(len(S), 12, 12)
    return A[:, :11].astype(F)


def null_vectors(A, pivot_ratio=PIVOT_RATIO):
    """LO-3 on (n, 11, 12) systems: complete pivoting as EP-3 (the first maximal |a| of the remaining block in row-major order; its
    row and its column swapped into place), elimination `f = a[q][r] / a[r][r]`, `a[q][c] = a[q][c] - f a[r][c]` for c > r, the
    unpivoted column's unknown 1, back substitution `s = s - a[r][q] x[q]` over ascending q from s = 0, `x[r] = s / a[r][r]`, the
    columns put back.  Returns (P (n, 12), ok (n,), |last pivot| / |first pivot| (n,) float64, for the census of the threshold)."""
    A = np.array(A, dtype=F, copy=True)
    n = len(A)
    rows = np.arange(n)
    perm = np.tile(np.arange(12), (n, 1))
    ok = np.ones(n, dtype=bool)
    p0 = np.zeros(n, dtype=F)
    with np.errstate(all="ignore"):
        for r in range(11):
            sub = np.abs(A[:, r:, r:]).reshape(n, -1)
            k = np.argmax(sub, 1)
            pi, pj = r + k // (12 - r), r + k % (12 - r)
            pmax = sub[rows, k]
            ok &= pmax != F(0)
            if r == 0:
                p0 = pmax
            ri, rr = A[rows, pi].copy(), A[:, r].copy()  # row swap
            A[:, r], A[rows, pi] = ri, rr
            ci, cr = A[rows, :, pj].copy(), A[:, :, r].copy()  # column swap, every row
            A[:, :, r], A[rows, :, pj] = ci, cr
            qi, qr = perm[rows, pj].copy(), perm[:, r].copy()
            perm[:, r], perm[rows, pj] = qi, qr
            for q in range(r + 1, 11):
                f = A[:, q, r] / A[:, r, r]
                A[:, q, r + 1:] = A[:, q, r + 1:] - f[:, None] * A[:, r, r + 1:]
        last = np.abs(A[:, 10, 10])
        ok &= ~(last <= F(pivot_ratio) * p0)
        x = np.zeros((n, 12), dtype=F)
        x[:, 11] = F(1)
        for r in range(10, -1, -1):
            s = np.zeros(n, dtype=F)
            for q in range(r + 1, 12):
                s = s - A[:, r, q] * x[:, q]
            x[:, r] = s / A[:, r, r]
        ok &= np.isfinite(x).all(1)
        P = np.zeros((n, 12), dtype=F)
        P[rows[:, None], perm] = x
        ratio = last.astype(np.float64) / p0.astype(np.float64)
    return P, ok, ratio


# ---- LO-4 --------------------------------------------------------------------------------------------------------------------
def _cof(m):
    """pose_ref._cof on a list of nine arrays."""
    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    r0, r1, r2 = m[0:3], m[3:6], m[6:9]
    return cross(r1, r2) + cross(r2, r0) + cross(r0, r1)


def polar(r, steps):
    """RP-4's step `steps` times on a list of nine arrays (or scalars): (R, every det finite and > 0)."""
    ok = True
    for _ in range(steps):
        c = _cof(r)
        det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2]
        ok = ok & (np.isfinite(det) & (det > F(0)))
        r = [F(0.5) * (r[k] + c[k] / det) for k in range(9)]
    return r, ok


def pose_from_p(P):
    """LO-4 on (n, 12) row-major 3 x 4 matrices: (R (n, 9), t (n, 3), ok (n,))."""
    P = np.asarray(P, dtype=F).reshape(-1, 12)
    with np.errstate(all="ignore"):
        m = [P[:, 4 * (k // 3) + k % 3] for k in range(9)]
        c = _cof(m)
        det = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2]
        ok = np.isfinite(det) & (det != F(0))
        P = np.where((det < F(0))[:, None], -P, P)
        m = [P[:, 4 * (k // 3) + k % 3] for k in range(9)]
        s = m[0] * m[0]
        for k in range(1, 9):
            s = s + m[k] * m[k]
        n = np.sqrt(s / F(3))
        ok &= np.isfinite(n) & (n > F(0))
        r, okp = polar([v / n for v in m], 3)
        ok &= okp
        t = np.stack([P[:, 3] / n, P[:, 7] / n, P[:, 11] / n], 1)
    return np.stack(r, 1).astype(F), t.astype(F), ok


# ---- LO-5 --------------------------------------------------------------------------------------------------------------------
def transform(R, t, rec):
    """Y' = R Y + t in RP-5's order: models (n, 9), (n, 3) on candidates (M, 7) -> three (n, M) arrays."""
    R, t = np.atleast_2d(R), np.atleast_2d(t)
    Y = [rec[None, :, c] for c in range(3)]
    r = [R[:, e:e + 1] for e in range(9)]
    return [((r[3 * c] * Y[0] + r[3 * c + 1] * Y[1]) + r[3 * c + 2] * Y[2]) + t[:, c:c + 1] for c in range(3)]


def inliers(R, t, rec, p):
    """LO-5: (n_models, M) inlier flags, the reprojection test without a division."""
    r2 = p["max_reproj_px"] * p["max_reproj_px"]
    with np.errstate(all="ignore"):
        x, y, z = transform(R, t, rec)
        ex = p["fx"] * x + (p["cx"] - rec[None, :, 3]) * z
        ey = p["fy"] * y + (p["cy"] - rec[None, :, 4]) * z
        return (z > F(0)) & (ex * ex + ey * ey <= r2 * (z * z))


# ---- LO-6 --------------------------------------------------------------------------------------------------------------------
def solve(sums, n=6):
    """GV-6's solver (verify_ref.solve) at size n x (n + 1): None when it fails."""
    iu, ju = np.triu_indices(n)
    m = len(iu)
    A = np.zeros((n, n + 1), dtype=F)
    A[iu, ju] = sums[:m]
    A[ju, iu] = sums[:m]
    A[:, n] = sums[m:]
    with np.errstate(all="ignore"):
        for c in range(n):
            piv, pmax = c, abs(A[c, c])
            for r in range(c + 1, n):
                if abs(A[r, c]) > pmax:
                    pmax, piv = abs(A[r, c]), r
            if pmax == F(0):
                return None
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
            for r in range(c + 1, n):
                f = A[r, c] / A[c, c]
                A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
        x = np.zeros(n, dtype=F)
        ok = True
        for r in range(n - 1, -1, -1):
            s = A[r, n]
            for q in range(r + 1, n):
                s = s - A[r, q] * x[q]
            x[r] = s / A[r, r]
            ok = ok and bool(np.isfinite(x[r]))
    return x if ok else None


def normal_sums(R, t, rec, inl, p):
    """LO-6: the 27 sums of one Gauss-Newton step under (R, t) over the candidates flagged in `inl`, in GV-6's order and tree."""
    fx, fy, cx, cy = p["fx"], p["fy"], p["cx"], p["cy"]
    with np.errstate(all="ignore"):
        x, y, z = (v[0] for v in transform(np.array(R, F), np.array(t, F), rec))
        ex = (fx * (x / z) + cx) - rec[:, 3]
        ey = (fy * (y / z) + cy) - rec[:, 4]
        a, b = fx / z, -((fx * x / z) / z)
        c, d = fy / z, -((fy * y / z) / z)
        zero = np.zeros_like(x)
        J1 = np.stack([b * y, a * z - b * x, -(a * y), a, zero, b], 1)
        J2 = np.stack([d * y - c * z, -(d * x), c * x, zero, c, d], 1)
        T = np.concatenate([J1[:, _IU] * J1[:, _JU] + J2[:, _IU] * J2[:, _JU], -(J1 * ex[:, None] + J2 * ey[:, None])], 1).astype(F)
        T[~inl] = F(0)  # adding +0 leaves a partial sum as it is (it starts at +0 and never becomes -0)
        Pt = np.zeros((256, 27), dtype=F)
        for j0 in range(0, len(rec), 256):
            blk = T[j0:j0 + 256]
            Pt[:len(blk)] = Pt[:len(blk)] + blk
        s = 128
        while s >= 1:
            Pt[:s] = Pt[:s] + Pt[s:2 * s]
            s //= 2
    return Pt[0]


def gn_step(R, t, rec, inl, p):
    """LO-6: one step on lists of np.float32: (R, t), or None (a failed solve, a non-finite entry or an invalid polar det)."""
    x = solve(normal_sums(R, t, rec, inl, p))
    if x is None:
        return None
    w0, w1, w2 = x[0], x[1], x[2]
    one = F(1)
    W = [one, -w2, w1, w2, one, -w0, -w1, w0, one]
    with np.errstate(all="ignore"):
        Rn = [(W[3 * r] * R[c] + W[3 * r + 1] * R[3 + c]) + W[3 * r + 2] * R[6 + c] for r in range(3) for c in range(3)]
        tn = [((W[3 * r] * t[0] + W[3 * r + 1] * t[1]) + W[3 * r + 2] * t[2]) + x[3 + r] for r in range(3)]
        Rn, ok = polar(Rn, 2)
    if not (bool(ok) and all(np.isfinite(v) for v in Rn) and all(np.isfinite(v) for v in tn)):
        return None
    return Rn, tn


def refit(R, t, rec, inl, p):
    """LO-6: GN_STEPS steps from the minimal model over its (fixed) inliers; None as gn_step."""
    R, t = [F(v) for v in R], [F(v) for v in t]
    for _ in range(GN_STEPS):
        nxt = gn_step(R, t, rec, inl, p)
        if nxt is None:
            return None
        R, t = nxt
    return R, t


# ---- LO-2 .. LO-7 ------------------------------------------------------------------------------------------------------------
def hypotheses(rec, pair, p):
    """LO-2..LO-4 for every hypothesis: (R (hyps, 9), t (hyps, 3), ok (hyps,), J (hyps, 6), pivot ratios)."""
    J, ok = sample(p["seed"], pair, len(rec), p["hypotheses"])
    P, okn, ratio = null_vectors(dlt_rows(rec[J]))
    R, t, okp = pose_from_p(P)
    ok = ok & okn & okp
    R[~ok], t[~ok] = F(0), F(0)
    return R, t, ok, J, ratio


def localize_points(rec, pair, nomap=False, trace=None, **params):
    """LO-2..LO-7 on the candidates of pair `pair` (rec (M, 7) as `correspondences` returns them).  `trace`: a dict that receives
    n_min, whether the refit came through (fit) and its inlier count (n_fit), for tests that must tell a failed refit from a
    rejected one.  Returns (record of FIX_DTYPE, per-candidate inlier flags)."""
    p = defaults(**params)
    rec = np.asarray(rec, dtype=F).reshape(-1, 7)
    M = len(rec)
    out = np.zeros((), dtype=FIX_DTYPE)
    mask = np.zeros(M, dtype=bool)
    if nomap:
        out["status"] = ORB_LOCALIZE_NOMAP
        return out, mask
    if M < SAMPLE:
        out["status"] = ORB_LOCALIZE_FEW
        return out, mask
    hyps = p["hypotheses"]
    R, t, ok, _, _ = hypotheses(rec, pair, p)
    if not ok.any():
        out["status"] = ORB_LOCALIZE_DEGENERATE
        return out, mask
    counts = np.zeros(hyps, dtype=np.int64)
    for h0 in range(0, hyps, 256):  # chunks of hypotheses bound the memory
        counts[h0:h0 + 256] = inliers(R[h0:h0 + 256], t[h0:h0 + 256], rec, p).sum(1)
    keys = np.where(ok, ((counts + 1) << 12) | (MAX_HYPOTHESES - 1 - np.arange(hyps)), 0)
    h = int(np.argmax(keys))
    Rm, tm = R[h], t[h]
    inl_m = inliers(Rm, tm, rec, p)[0]
    n_min = int(inl_m.sum())
    assert n_min == counts[h]
    fit = refit(Rm, tm, rec, inl_m, p)
    keep = False
    if fit is not None:
        Rr, tr_ = np.array(fit[0], F), np.array(fit[1], F)
        inl_r = inliers(Rr, tr_, rec, p)[0]
        keep = 16 * int(inl_r.sum()) >= 15 * n_min
    if trace is not None:
        trace.update(n_min=n_min, fit=fit is not None, n_fit=int(inl_r.sum()) if fit is not None else 0)
    Rk, tk, mask = (Rr, tr_, inl_r) if keep else (Rm, tm, inl_m)
    out["r"], out["t"] = Rk, tk
    with np.errstate(all="ignore"):
        out["step"] = np.sqrt((tk[0] * tk[0] + tk[1] * tk[1]) + tk[2] * tk[2])
    out["candidates"], out["inliers"], out["hypothesis"] = M, int(mask.sum()), h
    out["status"] = ORB_LOCALIZE_OK if keep else ORB_LOCALIZE_MINIMAL
    return out, mask


def localize_pair(f, counts, corners_next, matches_prev, matches, pose_prev, points_prev, cap, **params):
    """LO-1..LO-7 for pair f >= 1 (pair 0: pass None for what pair f - 1 would give).  counts: the stored counts of the batch's frames.
    Returns (record, inlier bytes (cap,) of frame f - 1's slots)."""
    p = defaults(**params)
    mask = np.zeros(cap, dtype=np.uint8)
    if f == 0 or int(pose_prev["status"]) != ORB_POSE_OK:
        return localize_points(np.zeros((0, 7), F), f, nomap=True, **params)[0], mask
    sel, rec = correspondences(counts[f - 1], counts[f], counts[f + 1], matches_prev, matches, pose_prev, points_prev, corners_next, p)
    out, inl = localize_points(rec, f, **params)
    mask[sel[inl]] = 1
    return out, mask


def localize(counts, corners, matches, poses, points, cap, n_frames=None, **params):
    """LO-1..LO-7 for the pairs of a batch.  counts: the stored counts of the frames; corners[f]: frame f's stored records;
    matches[f]: the matcher's records of frame f's stored queries; poses[f], points[f]: pair f's pose record and points.
    Returns (FIX_DTYPE (n_frames - 1,), uint8 (n_frames - 1, cap))."""
    n = len(counts) if n_frames is None else n_frames
    recs, masks = np.zeros(n - 1, dtype=FIX_DTYPE), np.zeros((n - 1, cap), dtype=np.uint8)
    for f in range(n - 1):
        recs[f], masks[f] = localize_pair(f, counts, corners[f + 1], matches[f - 1] if f else None, matches[f], poses[f - 1] if f else None,
                                          points[f - 1] if f else None, cap, **params)
    return recs, masks
