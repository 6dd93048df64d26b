"""CPU restatement of feature tracks and keyframes, TK-1..TK-5 of DESIGN.md section 15, in NumPy (test infrastructure, not a test
file).

No pointer doubling: heads are a plain walk forward over the frames, tails a plain walk backward.  GV-1's candidate test is
verify_ref.candidates; everything else is integer arithmetic.
"""
import numpy as np

from tinyslam_amd.orb import ORB_MATCH_NONE as NONE, ORB_TRACK_VERIFIED, TRACK_DTYPE, TRACK_FRAME_DTYPE
from verify_ref import candidates


def defaults(source=ORB_TRACK_VERIFIED, max_distance=0, ratio=0.0, min_gap=0, max_gap=0, keep_permille=0, min_shared=0):
    """OrbTrackParams with its zero fields replaced by the defaults (max_distance and ratio only matter for GUIDED / MATCHED)."""
    return dict(source=source, max_distance=max_distance or 64, ratio=np.float32(ratio) if ratio else np.float32(0.8),
                min_gap=min_gap or 1, max_gap=max_gap, keep_permille=keep_permille or 900, min_shared=min_shared)


def pair_links(source, records, n_q, n_t, inlier=None, max_distance=0, ratio=0.0):
    """TK-1 for one pair: (target, distance) int64 arrays over the n_q queries, target -1 without a link.  records: MATCH_DTYPE of
    at least n_q queries (the matcher's for VERIFIED / MATCHED, the guided call's for GUIDED); inlier: the verification's bytes."""
    rec = np.asarray(records)[:n_q]
    j = np.full(n_q, -1, np.int64)
    if source == ORB_TRACK_VERIFIED:
        keep = np.nonzero((np.asarray(inlier)[:n_q] == 1) & (rec["index"] < n_t))[0]
    else:
        p = defaults(max_distance=max_distance, ratio=ratio)
        keep = candidates(rec, n_t, p["max_distance"], p["ratio"])
    j[keep] = rec["index"][keep]
    return j, rec["distance"].astype(np.int64)


def one_to_one(j, d, n_t):
    """TK-2: (next over the queries, prev over the n_t targets), -1 for NONE.  Of the links to one target the smallest key
    (distance << 23) | i survives."""
    nq = len(j)
    nxt = np.full(nq, -1, np.int64)
    prv = np.full(n_t, -1, np.int64)
    i = np.nonzero(j >= 0)[0]
    if not len(i):
        return nxt, prv
    key = (d[i] << 23) | i
    best = np.full(n_t, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(best, j[i], key)
    won = best[j[i]] == key
    nxt[i[won]] = j[i[won]]
    prv[j[i[won]]] = i[won]
    return nxt, prv


def track(counts, cap, links, **params):
    """TK-2..TK-5.  counts: the raw counters of the n_frames frames; links[f]: pair f's (target, distance) arrays from pair_links.
    Returns (per-frame TRACK_DTYPE arrays of cap entries, TRACK_FRAME_DTYPE array of n_frames records)."""
    p = defaults(**params)
    F = len(counts)
    n = [min(int(c), cap) for c in counts]
    prev = [np.full(n[f], -1, np.int64) for f in range(F)]
    next_ = [np.full(n[f], -1, np.int64) for f in range(F)]
    for f in range(F - 1):
        next_[f], prev[f + 1] = one_to_one(np.asarray(links[f][0])[:n[f]], np.asarray(links[f][1])[:n[f]], n[f + 1])
    # TK-3: heads forward, tails backward
    head_f = [np.arange(0) for _ in range(F)]
    head_i = [np.arange(0) for _ in range(F)]
    for f in range(F):
        head_f[f] = np.full(n[f], f, np.int64)
        head_i[f] = np.arange(n[f], dtype=np.int64)
        has = prev[f] >= 0
        if f and has.any():
            head_f[f][has] = head_f[f - 1][prev[f][has]]
            head_i[f][has] = head_i[f - 1][prev[f][has]]
    tail_f = [None] * F
    for f in range(F - 1, -1, -1):
        tail_f[f] = np.full(n[f], f, np.int64)
        has = next_[f] >= 0
        if f < F - 1 and has.any():
            tail_f[f][has] = tail_f[f + 1][next_[f][has]]
    tracks = []
    for f in range(F):
        t = np.zeros(cap, TRACK_DTYPE)
        t["prev"] = t["next"] = t["head_index"] = NONE
        t["head_frame"] = t["tail_frame"] = 0xFFFF
        nf = n[f]
        t["prev"][:nf] = np.where(prev[f] >= 0, prev[f], NONE)
        t["next"][:nf] = np.where(next_[f] >= 0, next_[f], NONE)
        t["head_index"][:nf] = head_i[f]
        t["head_frame"][:nf] = head_f[f]
        t["tail_frame"][:nf] = tail_f[f]
        tracks.append(t)

    def shared(k, f):  # TK-4
        return int(np.sum(head_f[f] <= k))

    base = [int(np.sum(next_[f] >= 0)) for f in range(F)]
    fr = np.zeros(F, TRACK_FRAME_DTYPE)
    fr["keypoints"] = n
    fr["links_in"] = [int(np.sum(prev[f] >= 0)) for f in range(F)]
    fr["links_out"] = base
    fr["keyframe"][0] = 1
    fr["shared"][0] = shared(0, 0)
    k = 0
    for f in range(1, F):  # TK-5
        g, s = f - k, shared(k, f)
        key = g >= p["min_gap"] and ((p["max_gap"] != 0 and g >= p["max_gap"]) or s == 0 or 1000 * s < p["keep_permille"] * base[k]
                                     or s < p["min_shared"])
        fr["keyframe"][f] = int(key)
        fr["ref_keyframe"][f] = k
        fr["shared"][f] = s
        if key:
            k = f
    return tracks, fr
