"""CPU restatement of orb_match_pairs and orb_verify_pairs (test infrastructure, not a test file).

Nothing here is new arithmetic: a row is constructed.match_ref of the two listed frames, a record and its inlier bytes are
verify_ref.verify_pair (model 0, GV-1..GV-7) or epipolar_ref.verify_pair (model 1, EP-1..EP-6) on that row and the two frames'
corners, with `pair` = the LIST INDEX -- the draw stream's seed never sees a frame.  What is the stage's own is the list and its
rules (MP-1), restated in `violation`."""
import numpy as np

import constructed as C
import epipolar_ref as er
import verify_ref as vr

PAIRS_PER_FRAME = 4            # ORB_PAIRS_PER_FRAME: place's default `top`
HOMOGRAPHY, EPIPOLAR = 0, 1    # ORB_PAIRS_HOMOGRAPHY, ORB_PAIRS_EPIPOLAR
FRAME_PAIR_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4")])
defaults = vr.defaults         # OrbVerifyParams' defaults are the consecutive verifiers'


def capacity(max_batch):
    """P: the pairs one call takes."""
    return PAIRS_PER_FRAME * max_batch


def as_list(pairs):
    """(n, 2) integers or (query, target) tuples as a FRAME_PAIR_DTYPE array."""
    a = np.asarray(pairs)
    if a.dtype == FRAME_PAIR_DTYPE:
        return a.reshape(-1)
    out = np.zeros(len(a), FRAME_PAIR_DTYPE)
    a = a.reshape(-1, 2)
    out["query"], out["target"] = a[:, 0], a[:, 1]
    return out


def violation(pairs, n_frames, max_batch):
    """MP-1: None for a list orb_match_pairs takes on a batch of n_frames frames, else what it refuses: "count" for a length
    outside 1 .. P, or the index of the first entry with a frame at or past n_frames or with query == target."""
    L = as_list(pairs)
    if not 1 <= len(L) <= capacity(max_batch):
        return "count"
    for i, (q, t) in enumerate(zip(L["query"].tolist(), L["target"].tolist())):
        if q >= n_frames or t >= n_frames or q == t:
            return i
    return None


def stored(counts, f, cap):
    return min(int(counts[f]), cap)


def match_pairs(counts, desc, cap, pairs):
    """MP-2: row i = match_ref of the first min(count, cap) records of frame query_i against those of frame target_i.  counts: the raw
    counters; desc[f]: uint32 (m_f, 8) with m_f >= min(counts[f], cap) (rows behind the stored count are stale and never read)."""
    return [C.match_ref(np.asarray(desc[q])[:stored(counts, q, cap)], np.asarray(desc[t])[:stored(counts, t, cap)])
            for q, t in as_list(pairs).tolist()]


def verify_pairs(counts, corners, rows, cap, pairs, W, H, model=HOMOGRAPHY, n_pairs=None, **params):
    """MP-3: [(record, cap inlier bytes)] of pairs 0 .. n_pairs - 1 (None: the whole list) from rows[i] (MATCH_DTYPE, at least the
    stored queries of frame query_i) and corners[f] (CORNER_DTYPE, at least the stored records of frame f)."""
    fn = {HOMOGRAPHY: vr.verify_pair, EPIPOLAR: er.verify_pair}[model]
    out = []
    for i, (q, t) in enumerate(as_list(pairs).tolist()[:n_pairs]):
        nq, nt = stored(counts, q, cap), stored(counts, t, cap)
        out.append(fn(np.asarray(corners[q])[:nq], np.asarray(corners[t])[:nt], np.asarray(rows[i])[:nq], W, H, i, cap=cap, **params))
    return out
