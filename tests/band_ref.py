"""CPU restatement of epipolar-band guided matching, EB-1..EB-4 of DESIGN.md section 18, in NumPy (test infrastructure, not a test
file).

No grid: membership is the definition's test on the coordinates, evaluated densely for every (query, target) pair in query
chunks.  Every binary32 operation of EB-2 and EB-3 is performed as np.float32, one rounding per product and per sum, in the
definition's order (NumPy's element-wise products and sums are separate operations: nothing is fused).
"""
import numpy as np

from tinyslam_amd.orb import MATCH_DTYPE, ORB_BAND_HOST, ORB_BAND_VERIFIED, ORB_MATCH_NONE as NONE
from verify_ref import level0

F = np.float32
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint16)
MIN_NORM2 = F(2.0 ** -64)
SIDEWAYS = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], dtype=F)  # a pure translation along x: the line of (x, y) is y' = y


def model_of(source, pair, vmodels=None, host=None):
    """EB-1: the nine binary32 entries of pair's F, or None when the pair has none.  vmodels: the VERIFY_MODEL_DTYPE records of
    the last epipolar verification; host: (pairs, 9) floats."""
    if source == ORB_BAND_HOST:
        return np.asarray(host, dtype=F).reshape(-1, 9)[pair].copy()
    assert source == ORB_BAND_VERIFIED
    rec = vmodels[pair]
    return np.asarray(rec["h"], dtype=F).reshape(9).copy() if int(rec["status"]) in (0, 3) else None  # OK, MINIMAL


def scaled(value, octave, scale):
    """value, or value * 2^octave per query (ORB_BAND_SCALE), as float32."""
    with np.errstate(over="ignore"):
        return F(value) * np.left_shift(1, octave & 31).astype(F) if scale else np.full(len(octave), F(value), dtype=F)


def lines(m, x, y, d):
    """EB-2: (a0, a1, a2, t, ok) for float32 coordinate arrays and the per-query band half-width d."""
    m = np.asarray(m, dtype=F).reshape(9)
    with np.errstate(all="ignore"):
        a0 = (m[0] * x + m[1] * y) + m[2]
        a1 = (m[3] * x + m[4] * y) + m[5]
        a2 = (m[6] * x + m[7] * y) + m[8]
        n2 = a0 * a0 + a1 * a1
        t = (d * d) * n2
        ok = np.isfinite(a0) & np.isfinite(a1) & np.isfinite(a2) & np.isfinite(t) & (n2 >= MIN_NORM2)
    return a0, a1, a2, t, ok


def members(q_corners, t_corners, model, band_px=0.0, radius_px=0.0, octave_window=0, scale=False, chunk=256):
    """EB-2 and EB-3: (query, target) index arrays of every candidate pair, queries ascending."""
    nq, nt = len(q_corners), len(t_corners)
    empty = np.zeros(0, np.int64)
    if model is None or nq == 0 or nt == 0:
        return empty, empty
    xq, yq = level0(q_corners)
    xt, yt = level0(t_corners)
    oq, ot = q_corners["octave"].astype(np.int64), t_corners["octave"].astype(np.int64)
    d = scaled(band_px if band_px else 2.0, oq, scale)
    R = scaled(radius_px, oq, scale)
    a0, a1, a2, t, ok = lines(model, xq, yq, d)
    qs, ts = [], []
    for i0 in range(0, nq, chunk):
        s = slice(i0, i0 + chunk)
        with np.errstate(all="ignore"):
            r = (a0[s, None] * xt[None, :] + a1[s, None] * yt[None, :]) + a2[s, None]
            assert r.dtype == F
            inb = ok[s, None] & (r * r <= t[s, None])
            inw = (np.abs(xt[None, :] - xq[s, None]) <= R[s, None]) & (np.abs(yt[None, :] - yq[s, None]) <= R[s, None])
        inb &= inw | ~(R[s, None] > 0)
        if octave_window:
            inb &= np.abs(ot[None, :] - oq[s, None]) < octave_window
        qi, tj = np.nonzero(inb)
        qs.append(qi + i0)
        ts.append(tj)
    return np.concatenate(qs).astype(np.int64), np.concatenate(ts).astype(np.int64)


def band_pair(q_corners, q_desc, t_corners, t_desc, model, band_px=0.0, radius_px=0.0, octave_window=0, scale=False, cap=None,
              candidates=None):
    """EB-1..EB-4 for one pair: q_* the stored records of frame f (n_q of them), t_* those of frame f+1 (n_t); model: nine floats
    or None.  Returns MATCH_DTYPE records for the n_q queries, or cap of them with NONE records past n_q.  candidates: the result
    of members() for the same arguments, when the caller has it already."""
    nq, nt = len(q_corners), len(t_corners)
    out = np.zeros(nq if cap is None else cap, dtype=MATCH_DTYPE)
    out["index"] = NONE
    out["distance"] = out["second"] = 0xFFFF
    qq, tj = candidates if candidates is not None else members(q_corners, t_corners, model, band_px, radius_px, octave_window, scale)
    if not len(qq):
        return out
    qd = np.ascontiguousarray(q_desc).view(np.uint8).reshape(nq, 32)
    td = np.ascontiguousarray(t_desc).view(np.uint8).reshape(nt, 32)
    key = np.empty(len(qq), np.int64)
    for k0 in range(0, len(qq), 1 << 20):
        k = slice(k0, k0 + (1 << 20))
        key[k] = (_POP8[qd[qq[k]] ^ td[tj[k]]].sum(axis=1).astype(np.int64) << 23) | tj[k]  # EB-4: distance first, then the smaller index
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
