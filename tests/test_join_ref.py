"""The join stage's restatement (tests/join_ref.py) on the CPU: each clause of SJ-3..SJ-6 on hand-built
records of the rail camera (tests/join_cases.py, tests/landmark_cases.py), and the accuracy of the joined path on the out-and-back
batches with a LOST frame in the middle (tests/loop_cases.py) against the true cameras and a float64 join."""
import numpy as np

import join_cases as J
import join_ref as jr
import landmark_cases as L
import loop_cases as K
import loop_ref as lpr
from tinyslam_amd import orb

F = np.float32
NONE = 0xFFFFFFFF
T = orb
V = dict(HOLDS=T.ORB_JOIN_LINK_HOLDS, STATUS=T.ORB_JOIN_LINK_STATUS, FEW=T.ORB_JOIN_LINK_FEW, RANGE=T.ORB_JOIN_LINK_RANGE, SAME=T.ORB_JOIN_LINK_SAME,
         FORWARD=T.ORB_JOIN_LINK_FORWARD, NONFINITE=T.ORB_JOIN_LINK_NONFINITE, RATIO_FEW=T.ORB_JOIN_LINK_RATIO_FEW,
         RATIO_SPREAD=T.ORB_JOIN_LINK_RATIO_SPREAD)
LANDS = 12


def _exact(b, lms, depth):
    """Every landmark's z set by hand: depth[o] (a number or LANDS numbers, by landmark) for the segment of origin o.  With the
    rail's identity rotations Z_A and Z_B are these numbers exactly, so a ratio is their quotient."""
    lms = [lm.copy() for lm in lms]
    for o, z in depth.items():
        lms[o]["z"][b["slots"][o]] = z
    return lms


# ---- SJ-3: the verdicts --------------------------------------------------------------------------------------------------------
def test_every_verdict_in_order():
    b, lms = J.rail()
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 3, 3, 3]
    base = J.fix(b, 5, 0)
    assert (base["origin"], base["query_origin"]) == (0, 3)

    def verdict(q=5, T_=0, n=None, frames=None, flags=0, min_inliers=0, **edit):
        fx = J.fix(b, q if q < 6 else 5, T_ if T_ < 6 else 0)
        for k, v in edit.items():
            fx[k] = v
        rows, masks = [J.row(b, min(q, 5), min(T_, 5))], [J.mask(b, min(q, 5))]
        lk = J.run(b, lms, [(q, T_)], rows=rows, fx=np.array([fx]), masks=masks, n=n, frames=frames, flags=flags, min_inliers=min_inliers)[2][0]
        assert (lk["origin"], lk["query_origin"]) == (fx["origin"], fx["query_origin"])  # copied as read, whatever the verdict
        if lk["verdict"] not in (V["HOLDS"], V["RATIO_FEW"], V["RATIO_SPREAD"]):
            assert lk["shared"] == 0 and lk["consistent"] == 0 and lk["gamma"] == 0 and lk["chosen"] == 0
        return int(lk["verdict"])

    assert verdict() == V["HOLDS"]
    # 1 STATUS
    assert verdict(status=J.FEW_FIX) == V["STATUS"] and verdict(status=J.MINIMAL) == V["STATUS"]
    assert verdict(status=J.MINIMAL, flags=T.ORB_JOIN_USE_MINIMAL) == V["HOLDS"] and verdict(status=J.FEW_FIX, flags=T.ORB_JOIN_USE_MINIMAL) == V["STATUS"]
    # 2 FEW
    assert verdict(inliers=11) == V["FEW"] and verdict(inliers=12) == V["HOLDS"] and verdict(inliers=12, min_inliers=13) == V["FEW"]
    assert verdict(inliers=1, min_inliers=1) == V["HOLDS"]
    # 3 RANGE: q >= F, T >= F, q >= L, no origin, an origin word outside the frames
    assert verdict(q=6) == V["RANGE"] and verdict(T_=6) == V["RANGE"] and verdict(query_origin=NONE) == V["RANGE"] and verdict(query_origin=6) == V["RANGE"]
    # L = 5 < F = 6: q = 4 is past RANGE, and has no ratios, because segment 3's landmarks reach frame 5 and take no part (LC-2)
    assert verdict(q=5, n=5) == V["RANGE"] and verdict(q=4, n=5) == V["RATIO_FEW"]
    # 4 SAME, 5 FORWARD
    assert verdict(q=4, T_=3) == V["SAME"] and verdict(q=1, T_=2) == V["SAME"] and verdict(q=0, T_=5) == V["FORWARD"] and verdict(q=2, T_=3) == V["FORWARD"]
    # 6 NONFINITE: the fix's pose in the map, camera q's record
    for bad in (np.nan, np.inf, -np.inf):
        pr, pt = base["pose_r"].copy(), base["pose_t"].copy()
        pr[5], pt[1] = bad, bad
        assert verdict(pose_r=pr) == V["NONFINITE"] and verdict(pose_t=pt) == V["NONFINITE"]
        for field, k in (("r", 2), ("t", 0)):
            fr = b["frames"].copy()
            fr[field][5][k] = bad
            assert verdict(frames=fr) == V["NONFINITE"] and verdict(q=4, frames=fr) == V["HOLDS"]
    r = base["r"].copy()
    r[0] = np.nan
    assert verdict(r=r, t=(np.nan, 0, 0), step=np.nan) == V["HOLDS"]  # the relative pose is not read
    # two at once: the first in the order
    pt = base["pose_t"].copy()
    pt[0] = np.nan
    assert verdict(status=J.FEW_FIX, inliers=0) == V["STATUS"] and verdict(q=6, status=J.FEW_FIX) == V["STATUS"]
    assert verdict(q=6, inliers=3) == V["FEW"] and verdict(q=4, T_=3, inliers=3) == V["FEW"]
    assert verdict(q=4, T_=3, query_origin=NONE) == V["RANGE"] and verdict(q=0, T_=5, query_origin=NONE) == V["RANGE"]
    assert verdict(q=4, T_=3, pose_t=pt) == V["SAME"] and verdict(q=0, T_=5, pose_t=pt) == V["FORWARD"] and verdict(q=6, pose_t=pt) == V["RANGE"]


def test_identity_camera_and_an_origin_record_that_is_never_read():
    # q = b: camera(q, b) is the identity whatever the record holds (LM-2), taken through the same arithmetic
    b, lms = J.rail(scales={3: 2})
    fr = b["frames"].copy()
    fr["r"][3], fr["t"][3], fr["scale"][3] = np.nan, np.inf, np.nan
    t = {}
    out, seg, links = J.run(b, lms, [(3, 1)], trace=t)
    out2, seg2, links2 = J.run(b, lms, [(3, 1)], frames=fr)
    assert links[0]["verdict"] == V["HOLDS"] and links2.tobytes() == links.tobytes() and seg2.tobytes() == seg.tobytes()
    assert len(t[0]) == LANDS and abs(float(links[0]["gamma"]) - 0.5) < 1e-4
    # a = I^T (p - gamma 0): the fix's translation itself; A = I after the polar step
    assert seg[3]["t"].tobytes() == J.fix(b, 3, 1)["pose_t"].tobytes() and seg[3]["r"].tolist() == np.eye(3).ravel().tolist()
    # the LOST origin itself is MOVED through the identity: its pose is the segment's similarity
    assert out[3]["status"] == T.ORB_JOIN_MOVED and out[3]["r"].tobytes() == seg[3]["r"].tobytes() and out[3]["t"].tobytes() == seg[3]["t"].tobytes()
    assert out[3]["scale"] == 0 and out[3]["gain"] == seg[3]["sigma"]
    assert np.isnan(out2[3]["scale"]) and out2[3]["t"].tobytes() == out[3]["t"].tobytes()  # sigma * NaN: the record's scale word is read


# ---- SJ-3: the ratios ----------------------------------------------------------------------------------------------------------
def test_ratios_each_clause():
    b, lms0 = J.rail()
    s, cap = b["slots"], b["cap"]
    lms = _exact(b, lms0, {0: 8.0, 3: 4.0})
    q, T_ = 5, 1
    t = {}
    lk = J.run(b, lms, [(q, T_)], trace=t)[2][0]
    assert t[0].tolist() == [2.0] * LANDS and (lk["verdict"], lk["shared"], lk["consistent"], lk["gamma"]) == (V["HOLDS"], LANDS, LANDS, 2.0)

    def count(lms=lms, row=None, mask=None, counts=None):
        t = {}
        J.run(b, lms, [(q, T_)], rows=[J.row(b, q, T_) if row is None else row], masks=[J.mask(b, q) if mask is None else mask], trace=t, counts=counts)
        return t[0].tolist()

    # the inlier byte must be 1
    m = J.mask(b, q)
    m[s[q][0]], m[s[q][1]] = 0, 2
    assert len(count(mask=m)) == LANDS - 2
    # a slot missing either owner: the landmark of T's segment, then the landmark of q's
    for o in (0, 3):
        bad = [lm.copy() for lm in lms]
        bad[o]["flags"][s[o][4]] = 0
        assert len(count(lms=bad)) == LANDS - 1
    # k = n_q(T) gives none, k = n_q(T) - 1 does; NONE gives none
    a = int(s[q][2])
    for k, n in ((LANDS, LANDS - 1), (LANDS - 1, LANDS), (orb.ORB_MATCH_NONE, LANDS - 1)):
        r = J.row(b, q, T_)
        r["index"][a] = k
        assert len(count(row=r)) == n, k
    # stale bytes and records at and above n_q(q) are not read; a counter cut below a slot takes its ratio
    m, r = J.mask(b, q), J.row(b, q, T_)
    m[LANDS:], r[LANDS:] = 1, r[s[q][0]]
    assert len(count(mask=m, row=r)) == LANDS
    counts = np.full(b["n"], LANDS, np.int64)
    counts[q] = LANDS - 1
    assert len(count(counts=counts)) == LANDS - 1
    # rho <= 0 and rho not finite do not count
    for o, l, z in ((3, 0, -4.0), (0, 1, 0.0), (3, 2, 0.0), (3, 3, np.nan), (0, 4, np.inf), (0, 5, -8.0)):
        zs = np.full(LANDS, 8.0 if o == 0 else 4.0)
        zs[l] = z
        assert count(lms=_exact(b, lms, {o: zs})) == [2.0] * (LANDS - 1), (o, l, z)
    both = _exact(b, lms, {0: np.r_[-8.0, [8.0] * (LANDS - 1)], 3: np.r_[-4.0, [4.0] * (LANDS - 1)]})
    assert count(lms=both) == [2.0] * LANDS  # a positive quotient of two negative depths counts: only rho is tested
    # a target at or above L has no owners
    out, seg, links = J.run(b, lms, [(4, 5)], fx=np.array([J.fix(b, 4, 1)]), n=5)
    assert (links[0]["verdict"], links[0]["shared"]) == (V["RATIO_FEW"], 0)


def test_counts_median_and_permille():
    b, lms0 = J.rail()
    q, T_ = 4, 2

    def link(m, depth3=4.0, **kw):
        lms = _exact(b, lms0, {0: 8.0, 3: depth3})
        lk = J.run(b, lms, [(q, T_)], masks=[J.mask(b, q, range(m))], **kw)[2][0]
        return int(lk["verdict"]), int(lk["shared"]), int(lk["consistent"]), float(lk["gamma"])

    # m = 0, 1, min_shared - 1, min_shared
    assert link(0) == (V["RATIO_FEW"], 0, 0, 0.0) and link(1) == (V["RATIO_FEW"], 1, 1, 2.0) and link(7) == (V["RATIO_FEW"], 7, 7, 2.0)
    assert link(8) == (V["HOLDS"], 8, 8, 2.0) and link(4, min_shared=5) == (V["RATIO_FEW"], 4, 4, 2.0) and link(5, min_shared=5) == (V["HOLDS"], 5, 5, 2.0)
    # the lower median of half 1.0 and half 2.0: rank (m - 1) / 2
    half = np.r_[[8.0] * 5, [4.0] * 7]  # landmarks 0-4 give 1.0, the others 2.0
    assert link(10, half) == (V["HOLDS"], 10, 5, 1.0)           # rank 4 of 1 1 1 1 1 2 2 2 2 2
    assert link(11, half) == (V["HOLDS"], 11, 6, 2.0)           # rank 5 of 1 1 1 1 1 2 2 2 2 2 2
    assert link(11, np.r_[[8.0] * 6, [4.0] * 6]) == (V["HOLDS"], 11, 6, 1.0)
    # the permille rule at its boundary: HOLDS iff 1000 consistent >= permille m
    assert link(10, half, consistent_permille=500)[0] == V["HOLDS"] and link(10, half, consistent_permille=501)[0] == V["RATIO_SPREAD"]
    assert link(11, half, consistent_permille=545)[0] == V["HOLDS"] and link(11, half, consistent_permille=546)[0] == V["RATIO_SPREAD"]
    assert link(10, half, consistent_permille=1000)[0] == V["RATIO_SPREAD"] and link(8, consistent_permille=1000)[0] == V["HOLDS"]
    # the tolerance: 1.0 and 1.0625 are consistent within 0.1 of the median, not within 0.05
    near = np.r_[[8.0] * 5, [8.0 / 1.0625] * 7]
    assert link(10, near)[2] == 10 and link(10, near, scale_tolerance=0.05)[2] == 5 and link(10, near, scale_tolerance=0.0625)[2] == 10
    d = jr.defaults()
    assert (d["min_inliers"], d["min_shared"], d["consistent_permille"], d["flags"]) == (12, 8, 500, 0) and d["scale_tolerance"] == F(0.1)


# ---- SJ-4 ----------------------------------------------------------------------------------------------------------------------
def test_similarity_values_and_nonfinite():
    # v = p - gamma t_q, a = R_q^T v, A = R_q^T P after one polar step
    Rz = [F(v) for v in (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)]
    I = [F(v) for v in np.eye(3).ravel()]
    A, a, fin = jr.similarity(I, [F(10), F(20), F(30)], Rz, [F(1), F(2), F(3)], F(2))
    assert fin and [float(v) for v in a] == [16.0, -8.0, 24.0] and [float(v) for v in A] == [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    # a HOLDS entry whose similarity overflows becomes NONFINITE, its counts and gamma zero
    b, lms0 = J.rail()
    lms = _exact(b, lms0, {0: 8.0, 3: 8.0})
    fx = J.fix(b, 5, 0)
    fx["pose_t"][0] = 3e38
    fr = b["frames"].copy()
    fr["t"][5][0] = -3e38
    lk = J.run(b, lms, [(5, 0)], fx=np.array([fx]), frames=fr)[2][0]
    assert lk["verdict"] == V["NONFINITE"] and lk["shared"] == 0 and lk["consistent"] == 0 and lk["gamma"] == 0 and lk["origin"] == 0 and lk["query_origin"] == 3
    fr["t"][5][0] = -3e37
    lk = J.run(b, lms, [(5, 0)], fx=np.array([fx]), frames=fr)[2][0]
    assert lk["verdict"] == V["HOLDS"] and lk["gamma"] == 1.0


# ---- SJ-5 ----------------------------------------------------------------------------------------------------------------------
def test_choice_tie_and_more_consistent():
    b, lms = J.rail(scales={3: 2})
    pairs = [(5, 0), (4, 1), (5, 0), (3, 2)]
    out, seg, links = J.run(b, lms, pairs)
    assert links["verdict"].tolist() == [V["HOLDS"]] * 4 and links["consistent"].tolist() == [LANDS] * 4
    assert links["chosen"].tolist() == [1, 0, 0, 0] and seg[3]["link"] == 0 and seg[3]["status"] == T.ORB_JOIN_SEGMENT_LINKED
    # a later entry with more consistent ratios wins; the duplicate behind it loses the tie
    masks = [J.mask(b, 5, range(10)), J.mask(b, 4), J.mask(b, 5, range(11)), J.mask(b, 3)]
    out, seg, links = J.run(b, lms, pairs, masks=masks)
    assert links["consistent"].tolist() == [10, 12, 11, 12] and links["chosen"].tolist() == [0, 1, 0, 0] and seg[3]["link"] == 1
    # an entry that does not hold is no candidate, however many ratios it has
    out, seg, links = J.run(b, lms, pairs, masks=masks, min_shared=12)
    assert links["verdict"].tolist() == [V["RATIO_FEW"], V["HOLDS"], V["RATIO_FEW"], V["HOLDS"]] and seg[3]["link"] == 1
    out, seg, links = J.run(b, lms, pairs, masks=masks, min_shared=13)
    assert not links["chosen"].any() and seg[3]["status"] == T.ORB_JOIN_SEGMENT_ROOT and seg[3]["link"] == NONE


# ---- SJ-6 ----------------------------------------------------------------------------------------------------------------------
def test_chain_of_three_segments():
    b, lms = J.rail(J.THREE, scales={2: 2, 4: 8})
    assert b["frames"]["origin"].tolist() == [0, 0, 2, 2, 4, 4]
    pairs = [(5, 3), (3, 0), (4, 1)]  # 4 -> 2, 2 -> 0, and 4 -> 0 directly with fewer ratios
    masks = [J.mask(b, 5), J.mask(b, 3), J.mask(b, 4, range(9))]
    out, seg, links = J.run(b, lms, pairs, masks=masks)
    assert links["verdict"].tolist() == [V["HOLDS"]] * 3 and links["chosen"].tolist() == [1, 1, 0]
    g42, g20 = F(links["gamma"][0]), F(links["gamma"][1])
    assert abs(g42 - 0.25) < 1e-4 and abs(g20 - 0.5) < 1e-4 and abs(float(links["gamma"][2]) - 0.125) < 1e-4
    assert seg["status"].tolist() == [1, 0, 2, 0, 2, 0] and seg["root"].tolist() == [0, 1, 0, 3, 0, 5] and seg["link"].tolist() == [NONE, NONE, 1, NONE, 0, NONE]
    assert seg[2]["sigma"] == g20 and seg[4]["sigma"] == g20 * g42  # sigma' = sigma_o * gamma
    # every frame in segment 0's frame and unit: the rail camera at x = 0.5 f
    assert out["status"].tolist() == [0, 0, 1, 1, 1, 1] and out["root"].tolist() == [0] * 6
    assert np.allclose(out["t"][:, 0], [-0.5 * f for f in range(6)], atol=1e-4) and np.allclose(out["r"], np.eye(3).ravel(), atol=1e-6)
    assert out["gain"].tolist() == [1, 1, seg[2]["sigma"], seg[2]["sigma"], seg[4]["sigma"], seg[4]["sigma"]]
    assert out["scale"].tolist() == [0, 1, 0, seg[2]["sigma"], 0, seg[4]["sigma"]]
    # the direct link alone: the same place, one step
    out1, seg1, _ = J.run(b, lms, pairs[2:], masks=masks[2:])
    assert seg1["root"].tolist() == [0, 1, 2, 3, 0, 5] and np.allclose(out1["t"][4:, 0], [-2.0, -2.5], atol=1e-4) and out1["status"].tolist() == [0] * 4 + [1, 1]


def test_a_composed_similarity_that_is_not_finite_leaves_a_root():
    b, lms0 = J.rail(J.THREE)
    lms = _exact(b, lms0, {0: 8.0 * 2.0 ** 60, 2: 8.0, 4: 8.0 * 2.0 ** -70})
    pairs = [(5, 3), (3, 0)]
    out, seg, links = J.run(b, lms, pairs)
    assert links["verdict"].tolist() == [V["HOLDS"]] * 2 and links["gamma"].tolist() == [2.0 ** 70, 2.0 ** 60]
    assert links["chosen"].tolist() == [0, 1]  # sigma' = 2^60 * 2^70 overflows: segment 4 stays a root
    assert seg["status"].tolist() == [1, 0, 2, 0, 1, 0] and seg[4]["root"] == 4 and seg[4]["link"] == NONE and seg[4]["sigma"] == 1
    assert seg[4]["r"].tolist() == np.eye(3).ravel().tolist() and not seg[4]["t"].any()
    assert out["status"].tolist() == [0, 0, 1, 1, 0, 0] and out[5].tobytes()[:52] == b["frames"][5].tobytes()[:52]


def test_chained_and_origin_frame_moves_with_the_old_segment():
    b, lms = J.rail(J.RESTART, scales={2: 4})
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 2, 2, 2] and b["frames"]["status"][2] == L.CHAINED
    # segment 2 hangs under an origin 1 of its own making: frame 2, whose record names origin 0, stays with segment 0
    fr = b["frames"].copy()
    fr["origin"][:2], fr["origin"][2] = 0, 0
    out, seg, links = J.run(b, lms, [(4, 1), (2, 4)])
    assert links["verdict"].tolist() == [V["HOLDS"], V["FORWARD"]] and abs(float(links["gamma"][0]) - 0.25) < 1e-4
    assert seg["status"].tolist() == [1, 0, 2, 0, 0, 0] and seg[2]["root"] == 0
    assert out["status"].tolist() == [0, 0, 0, 1, 1, 1] and out["root"].tolist() == [0] * 6
    assert out[2].tobytes()[:52] == b["frames"][2].tobytes()[:52] and out[2]["gain"] == 1  # COPIED: the old segment is a root
    assert np.allclose(out["t"][:, 0], [-0.5 * f for f in range(6)], atol=1e-4)
    # ... and when the old segment itself is moved, frame 2 moves with it, by the old segment's similarity
    segs3 = [L.ORIGIN, L.LOST, L.START, L.FEW, L.CHAINED, L.CHAINED]
    b, lms = J.rail(segs3, scales={1: 2, 2: 4})
    assert b["frames"]["origin"].tolist() == [0, 1, 1, 2, 2, 2] and b["frames"]["status"][2] == L.START
    out, seg, links = J.run(b, lms, [(4, 1), (2, 1)])  # segment 2 -> 1; (2, 1) lies in segment 1
    assert links["verdict"].tolist() == [V["HOLDS"], V["SAME"]] and seg["root"].tolist() == [0, 1, 1, 3, 4, 5]
    assert out["status"].tolist() == [0, 0, 0, 1, 1, 1] and out["root"].tolist() == [0, 1, 1, 1, 1, 1]


def test_no_chosen_link_is_the_trajectory_byte_for_byte():
    b, lms = J.rail(scales={3: 2})
    fr = b["frames"].copy()
    fr["t"][4][1], fr["scale"][5] = np.nan, -0.0
    for pairs, kw in (([(4, 3), (0, 5), (1, 2)], {}), ([(5, 0)], dict(min_shared=13)), ([(5, 0)], dict(min_inliers=51))):
        out, seg, links = J.run(b, lms, pairs, frames=fr, **kw)
        assert not links["chosen"].any() and (out["status"] == T.ORB_JOIN_COPIED).all()
        for f in range(b["n"]):
            assert out[f].tobytes()[:52] == fr[f].tobytes()[:52] and out[f]["gain"] == 1 and out[f]["root"] == fr[f]["origin"]
        assert seg["status"].tolist() == [1, 0, 0, 1, 0, 0] and (seg["root"] == np.arange(6)).all() and (seg["sigma"] == 1).all() and (seg["link"] == NONE).all()


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
# The yardstick is a float64 join of the same records: the same ratios in float64, the same choice, the nearest rotation (SVD) in
# place of the polar step.  Measured (deterministic) over seeds 0-3, worst of all: gamma 3.7798e-3 relative for both; rotation
# 0.0962 (restatement) and 0.0941 (float64) degrees; position 0.043264 units of segment 0 for both.
def _nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt


def _join64(nq, rows, pairs, frames, lms, fixes, masks, own, cap, L_frames, p):
    """gamma, (R, t) of every frame in its root's frame, float64.  Two segments at most are linked in these batches, so the chain is
    one step."""
    best = {}
    for i, (q, T_) in enumerate(pairs):
        fx = fixes[i]
        if jr.first_verdict(frames, q, T_, fx, L_frames, p) is not None:
            continue
        b = int(fx["query_origin"])
        P, pt = np.asarray(fx["pose_r"], np.float64).reshape(3, 3), np.asarray(fx["pose_t"], np.float64)
        Rq, tq = (np.asarray(v, np.float64) for v in jr.camera(frames, q, b))
        Rq = Rq.reshape(3, 3)
        rho = []
        for a in range(int(nq[q])):
            k = int(rows[i]["index"][a])
            if masks[i][a] != 1 or k >= nq[T_] or own[T_][k] == NONE or own[q][a] == NONE:
                continue
            XA, XB = (lms[key // cap][key % cap] for key in (int(own[T_][k]), int(own[q][a])))
            za = P[2] @ np.array([XA["x"], XA["y"], XA["z"]], np.float64) + pt[2]
            zb = Rq[2] @ np.array([XB["x"], XB["y"], XB["z"]], np.float64) + tq[2]
            if np.isfinite(za / zb) and za / zb > 0:
                rho.append(za / zb)
        rho = np.sort(rho)
        m = len(rho)
        if m < p["min_shared"]:
            continue
        g = rho[(m - 1) // 2]
        c = int((np.abs(rho - g) <= float(p["scale_tolerance"]) * g).sum())
        if 1000 * c < p["consistent_permille"] * m:
            continue
        if b not in best or (c, -i) > best[b][0]:
            best[b] = ((c, -i), g, _nearest_rotation(Rq.T @ P), Rq.T @ (pt - g * tq))
    cams, gam = {}, {}
    for f in range(len(frames)):
        b = int(frames["origin"][f])
        R, t = (np.asarray(v, np.float64) for v in jr.camera(frames, f, b))
        R = R.reshape(3, 3)
        if b in best:
            _, g, A, a = best[b]
            R, t = _nearest_rotation(R @ A), R @ a + g * t
            gam[b] = g
        cams[f] = (R, t)
    return gam, cams


def _errors(b, cams, frames_moved):
    e_t, e_r = 0.0, 0.0
    for f in frames_moved:
        _, (Rt, tt) = K.true_relative(b, f, 0, 0)
        R, t = cams[f]
        e_r = max(e_r, K.rotation_error_deg(R, Rt))
        e_t = max(e_t, float(np.linalg.norm(np.asarray(t, np.float64) - tt)))
    return e_r, e_t


def accuracy(seeds=range(4), verbose=True):
    """Worst errors over the seeds: (gamma relative, rotation degrees, position units of segment 0) of the restatement and of the
    float64 yardstick."""
    worst32, worst64 = np.zeros(3), np.zeros(3)
    p = jr.defaults()
    for seed in seeds:
        b = J.lost_batch(seed)
        desc = K.plant(b, np.random.default_rng(100 + seed))
        rows = K.rows_ref(desc, K.LOOP_PAIRS)
        fr, lms, fx, masks = K.reference(b, K.LOOP_PAIRS, rows, traj=L.FULL_TRAJ)
        assert fr["origin"].tolist() == [0] * 5 + [5] * 6 and fr["status"][5] == L.LOST and (fx["status"] == T.ORB_LOCALIZE_OK).all()
        nq = [min(int(c), b["cap"]) for c in b["counts"]]
        matches = [b["matches"][f][:nq[f]] for f in range(b["n"] - 1)]
        out, seg, links = jr.join_pairs(nq, matches, rows, K.LOOP_PAIRS, fr, list(lms), fx, masks, b["cap"])
        # the conditions the batches were chosen for
        want = {(0, 10): V["FORWARD"], (3, 2): V["SAME"]}
        assert [int(v) for v in links["verdict"]] == [want.get(pr, V["HOLDS"]) for pr in K.LOOP_PAIRS], (seed, links["verdict"])
        assert seg[5]["status"] == T.ORB_JOIN_SEGMENT_LINKED and seg[5]["root"] == 0 and out["status"].tolist() == [0] * 5 + [1] * 6
        true = J.true_gamma(b, 0, 5)
        own = lpr.owners(nq, matches, fr, list(lms), b["cap"], b["n"])
        gam64, cams64 = _join64(nq, rows, K.LOOP_PAIRS, fr, list(lms), fx, masks, own, b["cap"], b["n"], p)
        holds = links["verdict"] == V["HOLDS"]
        e32 = np.array([np.abs(links["gamma"][holds].astype(np.float64) / true - 1).max(),
                        *_errors(b, {f: (out[f]["r"], out[f]["t"]) for f in range(5, 11)}, range(5, 11))])
        # the yardstick's gamma error over the same entries: each entry's own float64 median
        g64 = []
        for i in np.nonzero(holds)[0]:
            g, _ = _join64(nq, rows[i:i + 1], [K.LOOP_PAIRS[i]], fr, list(lms), fx[i:i + 1], masks[i:i + 1], own, b["cap"], b["n"], p)
            g64.append(g[5])
        e64 = np.array([np.abs(np.array(g64) / true - 1).max(), *_errors(b, cams64, range(5, 11))])
        if verbose:
            print("seed %d: true gamma %.4f; restatement gamma %.3e, %.4f deg, %.4f units; float64 %.3e, %.4f deg, %.4f units; shared %s" %
                  (seed, true, *e32, *e64, links["shared"][holds].tolist()))
        worst32, worst64 = np.maximum(worst32, e32), np.maximum(worst64, e64)
    if verbose:
        print("worst: restatement %s, float64 %s" % (worst32, worst64))
    return worst32, worst64


def test_accuracy_on_the_out_and_back_path_with_a_lost_frame():
    """Measured over seeds 0-3 (deterministic; printed by this test): see DESIGN.md section 30 for the figures.  The restatement's
    worst errors are asserted at twice the float64 yardstick's worst; the factor covers a change of seeds only."""
    w32, w64 = accuracy()
    assert (w32 <= 2 * w64).all(), (w32, w64)
    assert np.allclose(J.BOUNDS, 2 * w64, rtol=1e-3), (J.BOUNDS, 2 * w64)  # the figures the GPU test holds the device to
