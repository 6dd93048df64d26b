"""CPU restatement of guided matching, GM-1..GM-4 of DESIGN.md section 14, in NumPy (test infrastructure, not a test file).

No grid: the window is the definition's test on the coordinates.  To keep the bench-size comparison short, the targets are
first narrowed to a strip |x_j - px| <= r + 1 + (|px| + r) 1e-6 in float64 (the binary32 test |fl(x_j - px)| <= r implies
|x_j - px| <= r (1 + 2^-23), well inside the strip), then every pair of the strip gets the exact binary32 test of GM-3.
Every binary32 operation of GM-2 is performed as np.float32, in the definition's order.
"""
import numpy as np

from tinyslam_amd.orb import MATCH_DTYPE, ORB_GUIDE_HOST, ORB_GUIDE_IDENTITY, ORB_GUIDE_VERIFIED, ORB_MATCH_NONE as NONE
from verify_ref import level0

F = np.float32
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint16)
IDENTITY = np.eye(3, dtype=F).reshape(9)


def model_of(source, pair, vmodels=None, host=None):
    """GM-1: the nine binary32 entries of pair's model, or None when the pair has none.  vmodels: the VERIFY_MODEL_DTYPE
    records of the last verification; host: (pairs, 9) floats."""
    if source == ORB_GUIDE_IDENTITY:
        return IDENTITY.copy()
    if source == ORB_GUIDE_HOST:
        return np.asarray(host, dtype=F).reshape(-1, 9)[pair].copy()
    assert source == ORB_GUIDE_VERIFIED
    rec = vmodels[pair]
    return np.asarray(rec["h"], dtype=F).reshape(9).copy() if int(rec["status"]) in (0, 3) else None  # OK, MINIMAL


def predict(m, x, y):
    """GM-2: (px, py, ok) for float32 coordinate arrays."""
    m = np.asarray(m, dtype=F).reshape(9)
    with np.errstate(all="ignore"):
        w = (m[6] * x + m[7] * y) + m[8]
        px = ((m[0] * x + m[1] * y) + m[2]) / w
        py = ((m[3] * x + m[4] * y) + m[5]) / w
    ok = (w > F(0)) & np.isfinite(px) & np.isfinite(py)
    return px, py, ok


def guided_pair(q_corners, q_desc, t_corners, t_desc, model, radius_px=0.0, octave_window=0, scale_radius=False, cap=None):
    """GM-1..GM-4 for one pair: q_* the stored records of frame f (n_q of them), t_* those of frame f+1 (n_t); model: nine
    floats or None.  Returns MATCH_DTYPE records for the n_q queries, or cap of them with NONE records past n_q."""
    nq, nt = len(q_corners), len(t_corners)
    out = np.zeros(nq if cap is None else cap, dtype=MATCH_DTYPE)
    out["index"] = NONE
    out["distance"] = out["second"] = 0xFFFF
    if model is None or nq == 0 or nt == 0:
        return out
    radius = F(radius_px) if radius_px else F(16.0)
    xq, yq = level0(q_corners)
    xt, yt = level0(t_corners)
    oq, ot = q_corners["octave"].astype(np.int64), t_corners["octave"].astype(np.int64)
    px, py, ok = predict(model, xq, yq)
    with np.errstate(over="ignore"):
        r = radius * np.left_shift(1, oq & 31).astype(F) if scale_radius else np.full(nq, radius, dtype=F)
    qi = np.nonzero(ok)[0]
    # strip by x in float64 (an over-approximation of the window), then the exact test
    order = np.argsort(xt, kind="stable")
    xs = xt[order].astype(np.float64)
    p64, r64 = px[qi].astype(np.float64), r[qi].astype(np.float64)
    with np.errstate(invalid="ignore"):
        marg = 1.0 + (np.abs(p64) + r64) * 1e-6
        lo = np.searchsorted(xs, p64 - r64 - marg, side="left")
        hi = np.searchsorted(xs, p64 + r64 + marg, side="right")
    n = np.maximum(hi - lo, 0)
    qq = np.repeat(qi, n)
    start = np.repeat(lo - np.cumsum(n) + n, n)
    tj = order[start + np.arange(int(n.sum()))] if len(qq) else np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        inw = (np.abs(xt[tj] - px[qq]) <= r[qq]) & (np.abs(yt[tj] - py[qq]) <= r[qq])
    if octave_window:
        inw &= np.abs(ot[tj] - oq[qq]) < octave_window
    qq, tj = qq[inw], tj[inw].astype(np.int64)
    if not len(qq):
        return out
    qd = q_desc.view(np.uint8).reshape(nq, 32)
    td = t_desc.view(np.uint8).reshape(nt, 32)
    d = _POP8[qd[qq] ^ td[tj]].sum(axis=1).astype(np.int64)
    key = (d << 23) | tj  # GM-4: distance first, then the smaller index
    srt = np.lexsort((key, qq))
    qs, ks = qq[srt], key[srt]
    first = np.nonzero(np.r_[True, qs[1:] != qs[:-1]])[0]
    bq, bk = qs[first], ks[first]
    out["index"][bq] = bk & 0x7FFFFF
    out["distance"][bq] = bk >> 23
    nxt = first + 1
    has2 = nxt < len(qs)
    has2[has2] = qs[nxt[has2]] == bq[has2]
    out["second"][bq[has2]] = ks[nxt[has2]] >> 23
    return out


def brute_force(q_desc, t_desc):
    """orb_match_consecutive's records by a dense argmin over every target."""
    nq, nt = len(q_desc), len(t_desc)
    out = np.zeros(nq, dtype=MATCH_DTYPE)
    out["index"] = NONE
    out["distance"] = out["second"] = 0xFFFF
    if nq == 0 or nt == 0:
        return out
    qd = q_desc.view(np.uint8).reshape(nq, 32)
    td = t_desc.view(np.uint8).reshape(nt, 32)
    D = _POP8[qd[:, None, :] ^ td[None, :, :]].sum(axis=2).astype(np.int64)
    best = np.argmin(D, axis=1)  # the first minimum: the smallest j
    out["index"] = best
    out["distance"] = D[np.arange(nq), best]
    if nt > 1:
        D[np.arange(nq), best] = 1 << 20
        out["second"] = D.min(axis=1)
    return out
