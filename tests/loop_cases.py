"""Hand-built inputs of the loop stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_loop_pairs reads the rows of orb_match_pairs, the matcher's consecutive records, the trajectory's frame
records, the landmark records, the stored keypoints and the raw counters.  `out_and_back` is a localize_cases.views batch whose
camera goes five steps out and the same steps back, so that frame 10 stands where frame 0 stood; `plant` gives every landmark a
descriptor and every stored keypoint its landmark's with a few bits flipped, so that the pairs matcher finds the true
correspondences (constructed.match_ref gives the same rows on the CPU); `set_candidates` rewrites a query frame's descriptors so
that a list entry has exactly M candidates.  `reference` runs the trajectory, landmark and loop restatements on a batch.
"""
import numpy as np

import constructed as C
import landmark_cases as L
import localize_cases as lc
import loop_ref as lpr
from tinyslam_amd import orb

OUT_STEPS = 5
LOOP_PAIRS = [(10, 0), (9, 1), (8, 2), (7, 3), (6, 4), (10, 1), (9, 0), (0, 10), (3, 2)]  # backward, forward and consecutive


def out_and_back(seed, nf=OUT_STEPS, n_land=200, cap=128, wrong=0.05, noise=0.001, **kw):
    """2 nf + 1 views of one cloud: nf of localize_cases.default_steps out and their inverses back."""
    fw = lc.default_steps(nf)
    back = [(R.T, -R.T @ t) for R, t in reversed(fw)]
    return lc.views(np.random.default_rng(seed), 2 * nf + 1, n_land, cap, steps=fw + back, wrong=wrong, noise=noise, **kw)


def cameras(b):
    """The true cameras of a views batch: [(R, t)] with X_k = R X_0 + t, in the cloud's unit."""
    cams = [(np.eye(3), np.zeros(3))]
    for R, t in b["steps"]:
        cams.append((R @ cams[-1][0], R @ cams[-1][1] + t))
    return cams


def true_relative(b, q, T, o):
    """Camera q relative to camera T, and camera q relative to camera o, both in the unit of the segment of origin o (the baseline
    of the pair (o, o + 1)): ((R, t), (R, t))."""
    cams = cameras(b)
    unit = np.linalg.norm(b["steps"][o][1])

    def rel(a, c):
        (Ra, ta), (Rc, tc_) = cams[a], cams[c]
        R = Ra @ Rc.T
        return R, (ta - R @ tc_) / unit

    return rel(q, T), rel(q, o)


def rotation_error_deg(R, Rtrue):
    return float(np.degrees(np.arccos(np.clip((np.trace(np.asarray(R, np.float64).reshape(3, 3) @ Rtrue.T) - 1) / 2, -1, 1))))


def plant(b, rng, max_flips=8):
    """desc[f] (stored count, 8) uint32: one random descriptor per landmark, and each stored keypoint its landmark's with at most
    `max_flips` bits flipped."""
    n_land = len(b["slots"][0])
    base = C.random_desc(rng, n_land)
    nq = lc.stored(b)
    out = []
    for f in range(b["n"]):
        d = C.random_desc(rng, int(nq[f]))
        for l in np.nonzero(b["slots"][f] >= 0)[0]:
            s = int(b["slots"][f][l])
            if s < nq[f]:
                d[s] = C.flip(base[l], int(rng.integers(0, max_flips + 1)), rng)
        out.append(d)
    return out


def rows_ref(desc, pairs):
    """The rows of orb_match_pairs on the CPU: constructed.match_ref of every listed pair."""
    return [C.match_ref(desc[q], desc[T]) for q, T in pairs]


def set_candidates(desc, q, T, own_T, M, rng, nq_q=None):
    """Rewrites desc[q] (a copy is returned) so that the entry (q, T) has exactly M candidates under the defaults: query slot a of the
    first M keeps its descriptor when its best match in T has an owner, else gets the descriptor of a random owned keypoint of T
    with at most 8 bits flipped (several slots may share one); every other slot gets a fresh random descriptor, about 128 bits from
    everything."""
    d = desc[q].copy()
    nq_q = len(d) if nq_q is None else nq_q
    assert M <= nq_q
    owned = np.nonzero(own_T[:len(desc[T])] != lpr.NONE)[0]
    assert len(owned) or M == 0
    row = C.match_ref(d, desc[T])
    for a in range(len(d)):
        r = row[a]
        is_cand = r["index"] != orb.ORB_MATCH_NONE and r["distance"] <= 64 and r["distance"] < 0.8 * r["second"] and own_T[int(r["index"])] != lpr.NONE
        if a < M and not is_cand:
            d[a] = C.flip(desc[T][int(rng.choice(owned))], int(rng.integers(0, 9)), rng)
        elif a >= M:
            d[a] = C.random_desc(rng, 1)[0]
    return d


def keep_only(b, desc, q, lands, rng):
    """A copy of desc[q] in which only the keypoints of the landmarks `lands` keep their descriptors; the others get fresh random
    ones, so that their records fail the filter."""
    d = desc[q].copy()
    keep = set(int(l) for l in lands)
    for l, s in enumerate(b["slots"][q]):
        if l not in keep and 0 <= s < len(d):
            d[s] = C.random_desc(rng, 1)[0]
    return d


# ---- the GPU tests' batches (64 x 48 frames) ---------------------------------------------------------------------------------
COUNT_CAP = 300
COUNTS = (0, 5, 6, 7, 255, 256, 257, 300)  # k_loc_score's 256-candidate tile, the refine's partials wrapping, the gather's second block


def count_batch(cap=COUNT_CAP):
    """Four views of 420 landmarks: every frame sees more than `cap` of them, stores `cap` and counts 11 more."""
    b = lc.views(np.random.default_rng(300), 4, 420, cap, noise=0.001, wrong=0.02, extra=11)
    assert (b["counts"] == cap + 11).all()
    return b


def lost_batch(cap=128):
    """The out-and-back path with the pose of pair 4 not OK: frame 5 is LOST and its own origin, frame 6 starts a segment there."""
    b = out_and_back(1, cap=cap)
    b["poses"]["status"][4] = orb.ORB_POSE_LOW_PARALLAX
    return b


def contention_batch(cap=128):
    """Six views in which a tenth of the matches point at a wrong slot: under a landmarks call that accepts any reprojection error
    (CONTENTION_LM) the chains that merge there are all GOOD, and the views behind the merge have several registered landmarks."""
    return lc.views(np.random.default_rng(17), 6, 150, cap, wrong=0.1, noise=0.001)


CONTENTION_LM = dict(max_reproj_px=1000.0)


def flat_batch(cap=128, n_land=100):
    """The rail camera (landmark_cases.rail: exact rays) and two query frames' worth of degenerate clouds: `plane` lists the
    landmarks at depth 8, `line` ten of them moved onto one image row in every view.  Returns (batch, plane, line)."""
    b = L.rail(6, n_land, cap=cap, v_hi=L.V_HI)
    plane = np.nonzero(b["cloud"][:, 2] == 8.0)[0]
    line = plane[:10]
    for f in range(b["n"]):
        b["corners"][f]["y"][b["slots"][f][line]] = 20
    return b, plane, line


def reference(b, pairs, rows, traj=None, lm=None, L_frames=None, trace=None, **params):
    """A views batch through the trajectory, landmark and loop restatements.  Returns (frame records, landmark records, fixes,
    inlier bytes)."""
    n = b["n"] if L_frames is None else L_frames
    fr, lms, _ = L.reference(b, n, traj=traj, **(lm or {}))
    if n < b["n"]:  # the trajectory of the whole batch, the landmarks of its first n frames
        fr = L.tc.reference(b, b["n"], **(traj or {}))[0]
    nq = lc.stored(b)
    intr = lc.intrinsics(b["W"], b["H"], b["focal"])
    out, masks = lpr.loop_pairs(nq, [c[:nq[f]] for f, c in enumerate(b["corners"])], [b["matches"][f][:nq[f]] for f in range(n - 1)], rows, pairs, fr,
                                list(lms), b["cap"], L=n, trace=trace, **{**intr, **params})
    return fr, lms, out, masks
