"""CPU restatement of the geometric verifier, GV-1..GV-7 of DESIGN.md section 13, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_verify.h
perform, in the same order: the records and inlier bytes of orb_verify_consecutive must equal what this module returns, bit for bit.
Hypotheses are vectorised (one row per hypothesis); the elimination of GV-6 runs as scalar float32 operations.
"""
import numpy as np

from tinyslam_amd.orb import ORB_MATCH_NONE as _NONE, VERIFY_MODEL_DTYPE

F = np.float32
VERIFY_OK, VERIFY_FEW, VERIFY_DEGENERATE, VERIFY_MINIMAL = 0, 1, 2, 3
MAX_HYPOTHESES = 4096
_IU, _JU = np.triu_indices(8)  # GV-6: the 36 entries of the upper triangle, row by row


def defaults(hypotheses=0, max_distance=0, ratio=0.0, inlier_px=0.0, seed=0):
    """OrbVerifyParams with its zero fields replaced by the defaults."""
    return dict(hypotheses=hypotheses or 512, max_distance=max_distance or 64, ratio=F(ratio) if ratio else F(0.8),
                inlier_px=F(inlier_px) if inlier_px else F(3.0), seed=seed & 0xFFFFFFFF)


def lowbias32(x):
    x = np.asarray(x, dtype=np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * 0x7FEB352D & 0xFFFFFFFF).astype(np.uint32)
    x = x ^ (x >> np.uint32(15))
    x = (x.astype(np.uint64) * 0x846CA68B & 0xFFFFFFFF).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def candidates(matches, n_t, max_distance, ratio):
    """GV-1: indices of the queries whose match is a candidate, ascending."""
    idx = matches["index"]
    d, second = matches["distance"], matches["second"]
    keep = (idx != _NONE) & (idx < n_t) & (d <= max_distance) & (d.astype(F) < F(ratio) * second.astype(F))
    return np.nonzero(keep)[0]


def level0(corners):
    """orb_corner_level0_xy"""
    s = np.left_shift(1, corners["octave"].astype(np.int64) & 31).astype(F)
    return (corners["x"].astype(F) + F(0.5)) * s - F(0.5), (corners["y"].astype(F) + F(0.5)) * s - F(0.5)


def normalise(W, H):
    """GV-2: centre and scale"""
    return F(0.5) * F(W - 1), F(0.5) * F(H - 1), F(2.0) / F(max(W, H))


def sample(seed, pair, M, hyps):
    """GV-3: (hyps, 4) candidate indices and a validity flag per hypothesis."""
    mix = lowbias32(lowbias32(np.uint32(seed)) ^ np.uint32(pair))
    h = np.arange(hyps, dtype=np.uint32)
    J = np.zeros((hyps, 4), dtype=np.int64)
    n = np.zeros(hyps, dtype=np.int64)
    rows = np.arange(hyps)
    for d in range(16):
        r = lowbias32(mix ^ ((h << np.uint32(4)) | np.uint32(d)))
        j = ((r.astype(np.uint64) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
        take = (n < 4) & ~((n > 0) & (j == J[:, 0])) & ~((n > 1) & (j == J[:, 1])) & ~((n > 2) & (j == J[:, 2]))
        J[rows[take], n[take]] = j[take]
        n += take
    return J, n == 4


COLLINEAR = F(1.0 / 65536.0)


def _cross(ax, ay, bx, by, qx, qy):
    """GV-4: the cross product of (b - a, q - a) and the bound its magnitude must exceed."""
    dx1, dy1, dx2, dy2 = bx - ax, by - ay, qx - ax, qy - ay
    return dx1 * dy2 - dy1 * dx2, COLLINEAR * ((np.abs(dx1) + np.abs(dy1)) * (np.abs(dx2) + np.abs(dy2)))


def _sq2quad(x, y):
    """GV-4: Heckbert's square-to-quad matrix times its denominator; x, y: (n, 4).  Returns (n, 9) and den != 0."""
    x0, x1, x2, x3 = x.T
    y0, y1, y2, y3 = y.T
    sx, sy = ((x0 - x1) + x2) - x3, ((y0 - y1) + y2) - y3
    dx1, dx2, dy1, dy2 = x1 - x2, x3 - x2, y1 - y2, y3 - y2
    den = dx1 * dy2 - dx2 * dy1
    g, hh = sx * dy2 - dx2 * sy, dx1 * sy - sx * dy1
    S = np.stack([(x1 - x0) * den + g * x1, (x3 - x0) * den + hh * x3, x0 * den,
                  (y1 - y0) * den + g * y1, (y3 - y0) * den + hh * y3, y0 * den, g, hh, den], 1)
    return S, den != F(0)


def mat3(A, B):
    """(n, 9) x (n, 9) row-major 3 x 3 products, every entry (a0 b0 + a1 b1) + a2 b2."""
    A, B = np.atleast_2d(A), np.atleast_2d(B)
    R = np.empty(np.broadcast_shapes(A.shape, B.shape), dtype=F)
    for r in range(3):
        for c in range(3):
            R[:, 3 * r + c] = (A[:, 3 * r] * B[:, c] + A[:, 3 * r + 1] * B[:, 3 + c]) + A[:, 3 * r + 2] * B[:, 6 + c]
    return R


def minimal_models(rec, J, ok):
    """GV-4: H = S_dst * adj(S_src) per hypothesis (rows of zeros where invalid) and the final validity."""
    P = rec[J]  # (n, 4, 4): u, v, u2, v2
    for a, b, c in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        s, ms = _cross(P[:, a, 0], P[:, a, 1], P[:, b, 0], P[:, b, 1], P[:, c, 0], P[:, c, 1])
        d, md = _cross(P[:, a, 2], P[:, a, 3], P[:, b, 2], P[:, b, 3], P[:, c, 2], P[:, c, 3])
        ok = ok & (np.abs(s) > ms) & (np.abs(d) > md) & ((s > F(0)) == (d > F(0)))
    S, oks = _sq2quad(P[:, :, 0], P[:, :, 1])
    D, okd = _sq2quad(P[:, :, 2], P[:, :, 3])
    ok = ok & oks & okd
    A = np.stack([S[:, 4] * S[:, 8] - S[:, 5] * S[:, 7], S[:, 2] * S[:, 7] - S[:, 1] * S[:, 8], S[:, 1] * S[:, 5] - S[:, 2] * S[:, 4],
                  S[:, 5] * S[:, 6] - S[:, 3] * S[:, 8], S[:, 0] * S[:, 8] - S[:, 2] * S[:, 6], S[:, 2] * S[:, 3] - S[:, 0] * S[:, 5],
                  S[:, 3] * S[:, 7] - S[:, 4] * S[:, 6], S[:, 1] * S[:, 6] - S[:, 0] * S[:, 7], S[:, 0] * S[:, 4] - S[:, 1] * S[:, 3]], 1)
    H = mat3(D, A)
    H[~ok] = F(0)
    return H, ok


def inliers(H, rec, t2):
    """GV-5: (n_models, M) inlier flags of models H (n_models, 9)."""
    H = np.atleast_2d(H)
    u, v, u2, v2 = (rec[None, :, i] for i in range(4))
    h = [H[:, e:e + 1] for e in range(9)]
    xp = (h[0] * u + h[1] * v) + h[2]
    yp = (h[3] * u + h[4] * v) + h[5]
    wp = (h[6] * u + h[7] * v) + h[8]
    ex, ey = xp - u2 * wp, yp - v2 * wp
    return ex * ex + ey * ey < t2 * (wp * wp)


def normal_sums(rec, inl):
    """GV-6: the 44 sums, candidate j into partial sum j mod 256 (ascending j), then the pairwise tree 128, 64, ..., 1."""
    u, v, u2, v2 = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    one, zero = np.ones_like(u), np.zeros_like(u)
    r1 = np.stack([u, v, one, zero, zero, zero, -(u * u2), -(v * u2)], 1)
    r2 = np.stack([zero, zero, zero, u, v, one, -(u * v2), -(v * v2)], 1)
    T = np.concatenate([r1[:, _IU] * r1[:, _JU] + r2[:, _IU] * r2[:, _JU], r1 * u2[:, None] + r2 * v2[:, None]], 1)
    T[~inl] = F(0)  # adding +0 leaves a partial sum as it is (it starts at +0 and never becomes -0)
    P = np.zeros((256, 44), dtype=F)
    for j0 in range(0, len(rec), 256):
        blk = T[j0:j0 + 256]
        P[:len(blk)] = P[:len(blk)] + blk
    s = 128
    while s >= 1:
        P[:s] = P[:s] + P[s:2 * s]
        s //= 2
    return P[0]


def solve(sums):
    """GV-6: Gaussian elimination with partial pivoting (first maximal |pivot|) on the 8 x 9 system; None when it fails."""
    A = np.zeros((8, 9), dtype=F)
    A[_IU, _JU] = sums[:36]
    A[_JU, _IU] = sums[:36]
    A[:, 8] = sums[36:]
    with np.errstate(all="ignore"):
        for c in range(8):
            piv, pmax = c, abs(A[c, c])
            for r in range(c + 1, 8):
                if abs(A[r, c]) > pmax:
                    pmax, piv = abs(A[r, c]), r
            if pmax == F(0):
                return None
            if piv != c:
                A[[c, piv]] = A[[piv, c]]
            for r in range(c + 1, 8):
                f = A[r, c] / A[c, c]
                A[r, c + 1:] = A[r, c + 1:] - f * A[c, c + 1:]
        x = np.zeros(9, dtype=F)
        ok = True
        for r in range(7, -1, -1):
            s = A[r, 8]
            for q in range(r + 1, 8):
                s = s - A[r, q] * x[q]
            x[r] = s / A[r, r]
            ok = ok and bool(np.isfinite(x[r]))
    x[8] = F(1)
    return x if ok else None


def to_pixels(Hn, cx, cy, k):
    """GV-7: T^-1 * Hn * T divided by its [2][2] entry."""
    T = np.array([[k, 0, -(cx * k), 0, k, -(cy * k), 0, 0, 1]], dtype=F)
    ik = F(1) / k
    Ti = np.array([[ik, 0, cx, 0, ik, cy, 0, 0, 1]], dtype=F)
    Q = mat3(Ti, mat3(Hn[None], T))[0]
    with np.errstate(all="ignore"):
        return Q / Q[8]


def verify_points(x0, y0, x1, y1, W, H, pair=0, **params):
    """GV-2..GV-7 on candidate correspondences (level-0 pixel coordinates, float32, in candidate order).
    Returns (record of VERIFY_MODEL_DTYPE, per-candidate inlier flags)."""
    p = defaults(**params)
    cx, cy, k = normalise(W, H)
    t = p["inlier_px"] * k
    t2 = t * t
    x0, y0, x1, y1 = (np.asarray(a, dtype=F) for a in (x0, y0, x1, y1))
    rec = np.stack([(x0 - cx) * k, (y0 - cy) * k, (x1 - cx) * k, (y1 - cy) * k], 1).astype(F)
    M = len(rec)
    out = np.zeros((), dtype=VERIFY_MODEL_DTYPE)
    out["candidates"] = M
    out["hypothesis"] = _NONE
    mask = np.zeros(M, dtype=bool)
    if M < 4:
        out["status"] = VERIFY_FEW
        return out, mask
    hyps = p["hypotheses"]
    J, ok = sample(p["seed"], pair, M, hyps)
    Hs, ok = minimal_models(rec, J, ok)
    counts = np.zeros(hyps, dtype=np.int64)
    for h0 in range(0, hyps, 256):  # chunks of hypotheses bound the memory
        counts[h0:h0 + 256] = inliers(Hs[h0:h0 + 256], rec, t2).sum(1)
    if not ok.any():
        out["status"] = VERIFY_DEGENERATE
        return out, mask
    keys = np.where(ok, ((counts + 1) << 12) | (MAX_HYPOTHESES - 1 - np.arange(hyps)), 0)
    h = int(np.argmax(keys))
    Hm = Hs[h]
    inl_m = inliers(Hm, rec, t2)[0]
    n_min = int(inl_m.sum())
    assert n_min == counts[h]
    x = solve(normal_sums(rec, inl_m))
    keep = False
    if x is not None:
        inl_r = inliers(x, rec, t2)[0]
        keep = 16 * int(inl_r.sum()) >= 15 * n_min  # GV-6: at least 15/16 of the minimal model's inliers
    Hk, mask = (x, inl_r) if keep else (Hm, inl_m)
    out["h"] = to_pixels(Hk, cx, cy, k)
    out["inliers"] = int(mask.sum())
    out["hypothesis"] = h
    out["status"] = VERIFY_OK if keep else VERIFY_MINIMAL
    return out, mask


def verify_pair(q_corners, t_corners, matches, W, H, pair, cap=None, **params):
    """GV-1..GV-7 for one pair from the stored records of frames f and f + 1 and the matches of frame f's stored queries.
    Returns (record, inlier bytes of the queries: cap of them when cap is given, else len(matches))."""
    p = defaults(**params)
    sel = candidates(matches, len(t_corners), p["max_distance"], p["ratio"])
    x0, y0 = level0(q_corners[sel])
    x1, y1 = level0(t_corners[matches["index"][sel].astype(np.int64)])
    rec, inl = verify_points(x0, y0, x1, y1, W, H, pair=pair, **params)
    mask = np.zeros(len(matches) if cap is None else cap, dtype=np.uint8)
    mask[sel[inl]] = 1
    return rec, mask
