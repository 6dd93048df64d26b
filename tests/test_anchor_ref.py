"""The anchor stage's restatement (tests/anchor_ref.py) on the CPU: each clause of AN-3..AN-7 on hand-built
records of the rail camera with its frames in a store (tests/anchor_cases.py), and the accuracy of a real second batch anchored in
the map of the first (tests/keyframes_cases.py) against the true cameras and a float64 anchor."""
import numpy as np

import anchor_cases as A
import anchor_ref as ar
import join_ref as jr
import keyframes_cases as KC
import keyframes_ref as kfr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import loop_ref as lpr
from tinyslam_amd import orb

F = np.float32
NONE = 0xFFFFFFFF
T = orb
V = A.V
LANDS = 12


def _exact(case, store_z=None, seg_z=None):
    """(store, lms) with depths set by hand: store_z[s] (a number or one per landmark) is the z of slot s's stored points, seg_z[o]
    the z of the landmarks of the segment of origin o.  With the rail's identity rotations Z_A and Z_B are these numbers exactly,
    so a ratio is their quotient."""
    b, lms, _, _, store = case
    store = {s: dict(kf, points=kf["points"].copy()) for s, kf in store.items()}
    lms = [lm.copy() for lm in lms]
    for s, z in (store_z or {}).items():
        store[s]["points"]["z"][b["slots"][s]] = z
    for o, z in (seg_z or {}).items():
        lms[o]["z"][b["slots"][o]] = z
    return store, lms


# ---- AN-3: the verdicts --------------------------------------------------------------------------------------------------------
def test_every_verdict_in_order():
    case = A.rail()
    b = case[0]
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 3, 3, 3]
    assert all(case[4][s]["head"]["status"] == T.ORB_KEYFRAME_STORED and case[4][s]["head"]["points"] == LANDS for s in range(6))
    base = A.fix(b, 5, 0)
    assert (base["origin"], base["slot"]) == (0, 0)

    def verdict(q=5, s=0, n=None, frames=None, flags=0, min_inliers=0, **edit):
        fx = A.fix(b, min(q, 5), s)
        for k, v in edit.items():
            fx[k] = v
        fr = b["frames"] if frames is None else frames
        lk = A.run(case, [(q, s)], fx=np.array([fx]), n=n, frames=frames, flags=flags, min_inliers=min_inliers)[2][0]
        assert (lk["query_origin"], lk["slot"]) == (fr["origin"][q] if q < 6 else 0, s)  # as read, whatever the verdict
        if lk["verdict"] not in (V["HOLDS"], V["RATIO_FEW"], V["RATIO_SPREAD"]):
            assert lk["shared"] == 0 and lk["consistent"] == 0 and lk["gamma"] == 0 and lk["chosen"] == 0
        return int(lk["verdict"])

    assert verdict() == V["HOLDS"]
    # 1 STATUS: not OK; MINIMAL with and without the flag; a NOMAP keyframe's fix
    assert verdict(status=A.FEW_FIX) == V["STATUS"] and verdict(status=A.MINIMAL) == V["STATUS"] and verdict(status=A.NOMAP_FIX) == V["STATUS"]
    assert verdict(status=A.MINIMAL, flags=T.ORB_ANCHOR_USE_MINIMAL) == V["HOLDS"] and verdict(status=A.FEW_FIX, flags=T.ORB_ANCHOR_USE_MINIMAL) == V["STATUS"]
    assert verdict(status=T.ORB_LOCALIZE_DEGENERATE, flags=T.ORB_ANCHOR_USE_MINIMAL) == V["STATUS"]
    # 2 FEW
    assert verdict(inliers=11) == V["FEW"] and verdict(inliers=12) == V["HOLDS"] and verdict(inliers=12, min_inliers=13) == V["FEW"]
    assert verdict(inliers=1, min_inliers=1) == V["HOLDS"]
    # 3 RANGE: q >= F, q >= L, no origin, an origin word outside the frames
    fr_none, fr_out = b["frames"].copy(), b["frames"].copy()
    fr_none["origin"][5], fr_out["origin"][5] = NONE, 6
    assert verdict(q=6) == V["RANGE"] and verdict(frames=fr_none) == V["RANGE"] and verdict(frames=fr_out) == V["RANGE"]
    # L = 5 < F = 6: q = 4 is past RANGE, and has no ratios, because segment 3's landmarks reach frame 5 and take no part (LC-2)
    assert verdict(q=5, n=5) == V["RANGE"] and verdict(q=4, n=5) == V["RATIO_FEW"]
    # the keyframe's segment and the query's are compared nowhere: a query of the keyframe's own segment, before or behind it, holds
    assert verdict(q=1, s=2) == V["HOLDS"] and verdict(q=2, s=0) == V["HOLDS"] and verdict(q=4, s=3) == V["HOLDS"] and verdict(q=0, s=5) == V["HOLDS"]
    # 4 NONFINITE: the fix's relative pose, its pose in the map, camera q's record
    for bad in (np.nan, np.inf, -np.inf):
        for field, k in (("r", 7), ("t", 2), ("pose_r", 5), ("pose_t", 1)):
            v = base[field].copy()
            v[k] = bad
            assert verdict(**{field: v}) == V["NONFINITE"], (field, bad)
        for field, k in (("r", 2), ("t", 0)):
            fr = b["frames"].copy()
            fr[field][5][k] = bad
            assert verdict(frames=fr) == V["NONFINITE"] and verdict(q=4, frames=fr) == V["HOLDS"]
    assert verdict(step=np.nan) == V["HOLDS"]  # |t| is not read
    fr = b["frames"].copy()
    fr["r"][3], fr["t"][3] = np.nan, np.inf
    assert verdict(q=3, frames=fr) == V["HOLDS"]  # q = b: the identity, whatever the record holds (LM-2)
    # two at once: the first in the order
    pt = base["pose_t"].copy()
    pt[0] = np.nan
    assert verdict(status=A.FEW_FIX, inliers=0) == V["STATUS"] and verdict(q=6, status=A.FEW_FIX) == V["STATUS"]
    assert verdict(q=6, inliers=3) == V["FEW"] and verdict(frames=fr_none, inliers=3) == V["FEW"]
    assert verdict(q=6, pose_t=pt) == V["RANGE"] and verdict(frames=fr_out, pose_t=pt) == V["RANGE"] and verdict(q=5, n=5, pose_t=pt) == V["RANGE"]


# ---- AN-3: the ratios ----------------------------------------------------------------------------------------------------------
def test_ratios_each_clause():
    case = A.rail()
    b = case[0]
    s, cap = b["slots"], b["cap"]
    q, kf = 5, 1
    store, lms = _exact(case, {kf: 8.0}, {3: 4.0})
    t = {}
    lk = A.run(case, [(q, kf)], store=store, lms=lms, trace=t)[2][0]
    assert t[0].tolist() == [2.0] * LANDS and (lk["verdict"], lk["shared"], lk["consistent"], lk["gamma"]) == (V["HOLDS"], LANDS, LANDS, 2.0)

    def count(store=store, lms=lms, row=None, mask=None, counts=None):
        t = {}
        A.run(case, [(q, kf)], rows=[A.row(b, q, kf) if row is None else row], masks=[A.mask(b, q) if mask is None else mask], store=store, lms=lms,
              trace=t, counts=counts)
        return t[0].tolist()

    # the inlier byte must be 1
    m = A.mask(b, q)
    m[s[q][0]], m[s[q][1]] = 0, 2
    assert len(count(mask=m)) == LANDS - 2
    # the stored point must have a key; the query's slot must have an owner
    st = {kf: dict(store[kf], points=store[kf]["points"].copy())}
    st[kf]["points"]["key"][s[kf][4]] = NONE
    assert len(count(store=st)) == LANDS - 1
    bad = [lm.copy() for lm in lms]
    bad[3]["flags"][s[3][4]] = 0
    assert len(count(lms=bad)) == LANDS - 1
    bad = [lm.copy() for lm in lms]
    bad[0]["flags"][s[0][4]] = 0  # the keyframe segment's landmark records are not read: the store holds its points
    assert len(count(lms=bad)) == LANDS
    # k = keypoints gives none, k = keypoints - 1 does; NONE gives none
    a = int(s[q][2])
    for k, n in ((LANDS, LANDS - 1), (LANDS - 1, LANDS), (orb.ORB_MATCH_NONE, LANDS - 1)):
        r = A.row(b, q, kf)
        r["index"][a] = k
        assert len(count(row=r)) == n, k
    short = {kf: dict(store[kf], head=store[kf]["head"].copy())}
    short[kf]["head"]["keypoints"] = 5
    assert len(count(store=short)) == int((s[kf] < 5).sum())
    # stale bytes and records at and above n_q(q) are not read; a counter cut below a slot takes its ratio
    m, r = A.mask(b, q), A.row(b, q, kf)
    m[LANDS:], r[LANDS:] = 1, r[s[q][0]]
    assert len(count(mask=m, row=r)) == LANDS
    counts = np.full(b["n"], LANDS, np.int64)
    counts[q] = LANDS - 1
    assert len(count(counts=counts)) == LANDS - 1
    # rho <= 0 and rho not finite do not count
    for side, l, z in (("seg", 0, -4.0), ("store", 1, 0.0), ("seg", 2, 0.0), ("seg", 3, np.nan), ("store", 4, np.inf), ("store", 5, -8.0)):
        zs = np.full(LANDS, 8.0 if side == "store" else 4.0)
        zs[l] = z
        st2, lm2 = _exact(case, {kf: zs if side == "store" else 8.0}, {3: zs if side == "seg" else 4.0})
        assert count(store=st2, lms=lm2) == [2.0] * (LANDS - 1), (side, l, z)
    st2, lm2 = _exact(case, {kf: np.r_[-8.0, [8.0] * (LANDS - 1)]}, {3: np.r_[-4.0, [4.0] * (LANDS - 1)]})
    assert count(store=st2, lms=lm2) == [2.0] * LANDS  # a positive quotient of two negative depths counts: only rho is tested
    # Z_A goes through the fix's relative pose: r[6..8] and t[2]
    fx = A.fix(b, q, kf)
    fx["t"][2] = 8.0
    t = {}
    A.run(case, [(q, kf)], fx=np.array([fx]), store=store, lms=lms, trace=t)
    assert t[0].tolist() == [4.0] * LANDS
    # a NOMAP keyframe under a fix written as OK: every key is NONE
    nomap = {kf: dict(store[kf], points=store[kf]["points"].copy())}
    nomap[kf]["points"]["key"] = NONE
    lk = A.run(case, [(q, kf)], store=nomap, lms=lms)[2][0]
    assert (lk["verdict"], lk["shared"]) == (V["RATIO_FEW"], 0)


def test_ratio_counts_at_the_radix_selects_edges():
    """0, 1, 7, 8, 255, 256, 257 and 300 ratios at capacity 300, with ratios that differ: the lower median is rank (m - 1) / 2."""
    case = A.rail(K_=300, cap=300)
    b = case[0]
    q, kf = 4, 2
    factor = 1.0 + (np.arange(300) % 7) / 64.0  # exact in binary32
    store, lms = _exact(case, {kf: 8.0 * factor}, {3: 4.0})
    for m in (0, 1, 7, 8, 255, 256, 257, 300):
        t = {}
        out, seg, links, rows, land = A.run(case, [(q, kf)], masks=[A.mask(b, q, range(m))], store=store, lms=lms, trace=t)
        lk = links[0]
        assert len(t[0]) == m == lk["shared"] and lk["verdict"] == (V["RATIO_FEW"] if m < 8 else V["HOLDS"]), (m, lk)
        if m:
            g = np.sort(t[0])[(m - 1) // 2]
            assert lk["gamma"] == g and lk["consistent"] == int((np.abs(t[0] - g) <= F(0.1) * g).sum())
        assert seg[3]["status"] == (A.SEG_ANCHORED if m >= 8 else A.SEG_FREE)


def test_counts_median_and_permille():
    case = A.rail()
    b = case[0]
    q, kf = 4, 2

    def link(m, depth3=4.0, **kw):
        store, lms = _exact(case, {kf: 8.0}, {3: depth3})
        lk = A.run(case, [(q, kf)], masks=[A.mask(b, q, range(m))], store=store, lms=lms, **kw)[2][0]
        return int(lk["verdict"]), int(lk["shared"]), int(lk["consistent"]), float(lk["gamma"])

    assert link(0) == (V["RATIO_FEW"], 0, 0, 0.0) and link(1) == (V["RATIO_FEW"], 1, 1, 2.0) and link(7) == (V["RATIO_FEW"], 7, 7, 2.0)
    assert link(8) == (V["HOLDS"], 8, 8, 2.0) and link(4, min_shared=5) == (V["RATIO_FEW"], 4, 4, 2.0) and link(5, min_shared=5) == (V["HOLDS"], 5, 5, 2.0)
    half = np.r_[[8.0] * 5, [4.0] * 7]  # landmarks 0-4 give 1.0, the others 2.0
    assert link(10, half) == (V["HOLDS"], 10, 5, 1.0) and link(11, half) == (V["HOLDS"], 11, 6, 2.0)
    assert link(10, half, consistent_permille=500)[0] == V["HOLDS"] and link(10, half, consistent_permille=501)[0] == V["RATIO_SPREAD"]
    assert link(10, half, consistent_permille=1000)[0] == V["RATIO_SPREAD"] and link(8, consistent_permille=1000)[0] == V["HOLDS"]
    near = np.r_[[8.0] * 5, [8.0 / 1.0625] * 7]
    assert link(10, near)[2] == 10 and link(10, near, scale_tolerance=0.05)[2] == 5 and link(10, near, scale_tolerance=0.0625)[2] == 10
    d = ar.defaults()
    assert (d["min_inliers"], d["min_shared"], d["consistent_permille"], d["flags"]) == (12, 8, 500, 0) and d["scale_tolerance"] == F(0.1)


# ---- AN-4 ----------------------------------------------------------------------------------------------------------------------
def test_similarity_overflow_is_nonfinite():
    case = A.rail()
    b = case[0]
    store, lms = _exact(case, {0: 8.0}, {3: 8.0})
    fx = A.fix(b, 5, 0)
    fx["pose_t"][0] = 3e38
    fr = b["frames"].copy()
    fr["t"][5][0] = -3e38
    out, seg, links, rows, land = A.run(case, [(5, 0)], fx=np.array([fx]), frames=fr, store=store, lms=lms)
    lk = links[0]
    assert lk["verdict"] == V["NONFINITE"] and lk["shared"] == 0 and lk["consistent"] == 0 and lk["gamma"] == 0 and (lk["query_origin"], lk["slot"]) == (3, 0)
    assert seg[3]["status"] == A.SEG_FREE and (out["status"] == A.FREE).all()
    fr["t"][5][0] = -3e37
    lk = A.run(case, [(5, 0)], fx=np.array([fx]), frames=fr, store=store, lms=lms)[2][0]
    assert lk["verdict"] == V["HOLDS"] and lk["gamma"] == 1.0


# ---- AN-5, AN-6 ----------------------------------------------------------------------------------------------------------------
def test_choice_tie_duplicate_and_the_segment_record():
    case = A.rail(scales={3: 2})
    b, lms, lrows, _, store = case
    pairs = [(5, 0), (4, 1), (5, 0), (3, 2)]
    out, seg, links, rows, land = A.run(case, pairs)
    assert links["verdict"].tolist() == [V["HOLDS"]] * 4 and links["consistent"].tolist() == [LANDS] * 4
    assert links["chosen"].tolist() == [1, 0, 0, 0]  # the tie and the duplicate: the lowest index
    S = seg[3]
    assert (S["status"], S["link"], S["slot"], S["map_origin"], S["map_frame"], S["user"].tolist()) == (A.SEG_ANCHORED, 0, 0, 0, 0, [1, 1000])
    assert abs(float(S["gamma"]) - 0.5) < 1e-4 and S["gamma"] == links["gamma"][0] and not S["reserved"].any()
    # segment 0 is named and has no entry of its own: FREE, the identity; the other slots are no origin
    assert seg["status"].tolist() == [A.SEG_FREE, 0, 0, A.SEG_ANCHORED, 0, 0]
    for k in (0, 1, 2, 4, 5):
        assert seg[k]["r"].tolist() == np.eye(3).ravel().tolist() and not seg[k]["t"].any() and seg[k]["gamma"] == 1 and not seg[k]["user"].any()
        assert (seg[k]["slot"], seg[k]["link"], seg[k]["map_origin"], seg[k]["map_frame"]) == (NONE,) * 4
    # frames 3-5 in segment 0's frame and unit -- the rail camera at x = 0.5 f --, frames 0-2 the trajectory byte for byte
    assert out["status"].tolist() == [A.FREE] * 3 + [A.ANCHORED] * 3 and out["slot"].tolist() == [NONE] * 3 + [0] * 3
    assert np.allclose(out["t"][3:, 0], [-1.5, -2.0, -2.5], atol=1e-4) and np.allclose(out["r"][3:], np.eye(3).ravel(), atol=1e-6)
    assert out["gain"].tolist() == [1, 1, 1] + [S["gamma"]] * 3 and out["scale"].tolist() == [0, 1, 1, 0, S["gamma"], S["gamma"]]
    for f in range(3):
        assert out[f].tobytes()[:52] == b["frames"][f].tobytes()[:52]
    # a later entry with more consistent ratios wins; the duplicate behind it loses the tie
    masks = [A.mask(b, 5, range(10)), A.mask(b, 4), A.mask(b, 5, range(11)), A.mask(b, 3)]
    out, seg, links, rows, land = A.run(case, pairs, masks=masks)
    assert links["consistent"].tolist() == [10, 12, 11, 12] and links["chosen"].tolist() == [0, 1, 0, 0]
    assert (seg[3]["link"], seg[3]["slot"], seg[3]["map_frame"], seg[3]["user"].tolist()) == (1, 1, 1, [8, 1001])
    # an entry that does not hold is no candidate, however many ratios it has
    out, seg, links, rows, land = A.run(case, pairs, masks=masks, min_shared=12)
    assert links["verdict"].tolist() == [V["RATIO_FEW"], V["HOLDS"], V["RATIO_FEW"], V["HOLDS"]] and seg[3]["link"] == 1
    # two segments, each through an entry of its own: segment 0 under its own keyframe (gamma 1), segment 3 under another
    out, seg, links, rows, land = A.run(case, [(1, 2), (4, 0)])
    assert links["chosen"].tolist() == [1, 1] and seg["status"].tolist() == [A.SEG_ANCHORED, 0, 0, A.SEG_ANCHORED, 0, 0]
    assert seg["link"][[0, 3]].tolist() == [0, 1] and seg["slot"][[0, 3]].tolist() == [2, 0] and (out["status"] == A.ANCHORED).all()
    assert seg[0]["gamma"] == 1 and np.allclose(out["t"][:, 0], [-0.5 * f for f in range(6)], atol=1e-4)


def test_a_frame_whose_origin_is_outside_the_frames_is_free():
    case = A.rail(scales={3: 2})
    b = case[0]
    fr = b["frames"].copy()
    fr["origin"][4] = 9
    out, seg, links, rows, land = A.run(case, [(5, 0)], frames=fr)
    assert links[0]["verdict"] == V["HOLDS"] and out["status"].tolist() == [A.FREE] * 3 + [A.ANCHORED, A.FREE, A.ANCHORED]
    assert out[4].tobytes()[:52] == fr[4].tobytes()[:52] and out[4]["gain"] == 1 and out[4]["slot"] == NONE


# ---- AN-7 ----------------------------------------------------------------------------------------------------------------------
def test_landmarks_in_the_maps_frame():
    case = A.rail(scales={3: 2})
    b, lms, lrows, _, store = case
    s = b["slots"]
    assert lrows["origin"].tolist() == [0, 0, NONE, 3, 3]  # pair 2 ends at the LOST frame: no landmark starts there
    # a landmark lives in the row of the pair it starts in: the rail's start in pairs 0 (segment 0) and 3 (segment 3)
    assert [int((lm["flags"] & T.ORB_POINT_GOOD != 0).sum()) for lm in lms] == [LANDS, 0, 0, LANDS, 0]
    wild = [lm.copy() for lm in lms]
    wild[3]["x"][s[3][6]] = np.inf        # gamma x is not finite: dropped
    wild[3]["views"][s[3][7]] = 0          # no view: copied
    wild[3]["origin"][s[3][8]] = 0         # another origin word than the row's: copied
    wild[3]["flags"][s[3][9]] = 0          # not GOOD: copied
    t = {}
    out, seg, links, rows, land = A.run(case, [(4, 0)], lms=wild, trace=t)
    assert links[0]["verdict"] == V["HOLDS"] and links[0]["shared"] == len(t[0]) >= 8 and abs(float(links[0]["gamma"]) - 0.5) < 1e-4
    assert rows["origin"].tolist() == [0, 0, NONE, 3, 3] and rows["slot"].tolist() == [NONE] * 3 + [0, 0] and rows["map_origin"].tolist() == [NONE] * 3 + [0, 0]
    assert rows["good"].tolist() == [LANDS, 0, 0, LANDS - 1, 0] and rows["moved"].tolist() == [0, 0, 0, LANDS - 4, 0]
    assert rows["dropped"].tolist() == [0, 0, 0, 1, 0] and not rows["reserved"].any()
    for p in (0, 1, 2, 4):
        assert land[p].tobytes() == wild[p].tobytes()  # segment 0 is FREE, pair 2 has no origin, pair 4 no landmark
    # the same physical landmark in segment 0's coordinates: lms[0] holds it at its slot of frame 0
    moved = [l for l in range(LANDS) if l not in (6, 7, 8, 9)]
    got, want = land[3][s[3][moved]], lms[0][s[0][moved]]
    for k in "xyz":
        assert np.allclose(got[k], want[k], atol=2e-3), k
    assert (got["origin"] == 3).all() and got["flags"].tobytes() == wild[3]["flags"][s[3][moved]].tobytes()  # the origin word is left alone
    d = land[3][s[3][6]]
    assert (d["x"], d["y"], d["z"], d["flags"]) == (0, 0, 0, 0) and d.tobytes()[16:] == wild[3][s[3][6]].tobytes()[16:]
    for l in (7, 8, 9):
        assert land[3][s[3][l]].tobytes() == wild[3][s[3][l]].tobytes()
    # slots without a landmark are copied
    free = np.setdiff1d(np.arange(b["cap"]), s[3])
    assert land[3][free].tobytes() == wild[3][free].tobytes()


def test_no_holds_is_the_trajectory_and_the_landmarks_byte_for_byte():
    case = A.rail(scales={3: 2})
    b, lms, lrows, _, store = case
    fr = b["frames"].copy()
    fr["t"][4][1], fr["scale"][5] = np.nan, -0.0
    for pairs, kw in (([(5, 0)], dict(min_shared=13)), ([(5, 0), (4, 2)], dict(min_inliers=51)), ([(6, 0)], {})):
        out, seg, links, rows, land = A.run(case, pairs, frames=fr, **kw)
        assert not links["chosen"].any() and (links["verdict"] != V["HOLDS"]).all() and (out["status"] == A.FREE).all()
        for f in range(b["n"]):
            assert out[f].tobytes()[:52] == fr[f].tobytes()[:52] and out[f]["gain"] == 1 and out[f]["slot"] == NONE
        assert seg["status"].tolist() == [A.SEG_FREE, 0, 0, A.SEG_FREE, 0, 0] and (seg["gamma"] == 1).all() and (seg["link"] == NONE).all()
        assert all(land[p].tobytes() == lms[p].tobytes() for p in range(b["n"] - 1))
        assert not rows["moved"].any() and not rows["dropped"].any() and (rows["slot"] == NONE).all() and rows["origin"].tolist() == lrows["origin"].tolist()
        assert rows["good"].tolist() == [int((lm["flags"] & T.ORB_POINT_GOOD != 0).sum()) for lm in lms]


# ---- accuracy ------------------------------------------------------------------------------------------------------------------
# The yardstick is a float64 anchor of the same records: the same ratios in float64, the same choice, the nearest rotation (SVD) in
# place of the polar step.  Measured (deterministic; printed by the test) over seeds 0-3, keyframes_cases.second_batch against all
# eleven keyframes of loop_cases.out_and_back, keyframes_cases.SECOND_PAIRS, worst of all:
#                 gamma (relative)   rotation (degrees)   position (store units)
#   restatement   0.027034           0.16234              0.089591
#   yardstick     0.027034           0.16139              0.089592
# gamma over all forty entries against |b2 step 0| / |b1 step 0|, rotation and position over the five anchored frames against the
# true cameras.  The two agree closely: the error is that of the chosen entry's fix and of the data -- keypoints at integer pixels,
# landmarks with 0.1 % noise --, which both take as they are.
RESTATED = (0.027034, 0.16234, 0.089591)
YARDSTICK = (0.027034, 0.16139, 0.089592)


def _nearest_rotation(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt


def _anchor64(c, own, p, only=None):
    """gamma of every segment and (R, t) of every frame in the map's frame, float64.  only: that entry alone."""
    frames, cap = c["frames"], c["cap"]
    best = {}
    for i, (q, s) in enumerate(c["pairs"]):
        fx = c["fixes"][i]
        if (only is not None and i != only) or ar.first_verdict(frames, q, fx, len(c["lms"]) + 1, p) is not None:
            continue
        b = int(frames["origin"][q])
        r, t = np.asarray(fx["r"], np.float64).reshape(3, 3), np.asarray(fx["t"], np.float64)
        P, pt = np.asarray(fx["pose_r"], np.float64).reshape(3, 3), np.asarray(fx["pose_t"], np.float64)
        Rq, tq = (np.asarray(v, np.float64) for v in jr.camera(frames, q, b))
        Rq = Rq.reshape(3, 3)
        kf = c["store"][s]
        rho = []
        for a in range(int(c["nq"][q])):
            k = int(c["rows"][i]["index"][a])
            if c["masks"][i][a] != 1 or k >= int(kf["head"]["keypoints"]) or kf["points"]["key"][k] == NONE or own[q][a] == NONE:
                continue
            Y = kf["points"][k]
            key = int(own[q][a])
            XB = c["lms"][key // cap][key % cap]
            za = r[2] @ np.array([Y["x"], Y["y"], Y["z"]], np.float64) + t[2]
            zb = Rq[2] @ np.array([XB["x"], XB["y"], XB["z"]], np.float64) + tq[2]
            if np.isfinite(za / zb) and za / zb > 0:
                rho.append(za / zb)
        rho = np.sort(rho)
        m = len(rho)
        if m < p["min_shared"]:
            continue
        g = rho[(m - 1) // 2]
        n_in = int((np.abs(rho - g) <= float(p["scale_tolerance"]) * g).sum())
        if 1000 * n_in < p["consistent_permille"] * m:
            continue
        if b not in best or (n_in, -i) > best[b][0]:
            best[b] = ((n_in, -i), g, _nearest_rotation(Rq.T @ P), Rq.T @ (pt - g * tq))
    cams, gam = {}, {}
    for f in range(len(frames)):
        b = int(frames["origin"][f])
        R, t = (np.asarray(v, np.float64) for v in jr.camera(frames, f, b))
        R = R.reshape(3, 3)
        if b in best:
            _, g, A_, a = best[b]
            R, t = _nearest_rotation(R @ A_), R @ a + g * t
            gam[b] = g
            cams[f] = (R, t)
    return gam, cams


def _pose_errors(c, cams):
    e_r, e_t = 0.0, 0.0
    for f, (R, t) in cams.items():
        _, (Rt, tt) = KC.true_relative(c["b1"], c["b2"], f, 0, 0)
        e_r = max(e_r, K.rotation_error_deg(R, Rt))
        e_t = max(e_t, float(np.linalg.norm(np.asarray(t, np.float64) - tt)))
    return e_r, e_t


def _owners(c):
    return lpr.owners(c["nq"], c["matches"], c["frames"], c["lms"], c["cap"], len(c["lms"]) + 1)


def accuracy(seeds=range(4), verbose=True):
    """Worst errors over the seeds: (gamma relative, rotation degrees, position store units) of the restatement and of the float64
    yardstick."""
    worst32, worst64 = np.zeros(3), np.zeros(3)
    p = ar.defaults()
    for seed in seeds:
        c = A.two_batches(seed)
        assert c["fr1"]["status"].tolist() == [L.ORIGIN, L.START] + [L.CHAINED] * 9 and (c["frames"]["origin"] == 0).all()
        assert (c["fixes"]["status"] == T.ORB_LOCALIZE_OK).all()
        out, seg, links, rows, land = A.anchor(c)
        # the conditions the batches were chosen for: every entry HOLDS, segment 0 ANCHORED
        assert (links["verdict"] == V["HOLDS"]).all(), (seed, links["verdict"])
        assert seg[0]["status"] == A.SEG_ANCHORED and (out["status"] == A.ANCHORED).all() and links["chosen"].sum() == 1
        true = A.true_gamma(c["b1"], c["b2"])
        own = _owners(c)
        gam64, cams64 = _anchor64(c, own, p)
        assert sorted(cams64) == list(range(5))
        e32 = np.array([np.abs(links["gamma"].astype(np.float64) / true - 1).max(), *_pose_errors(c, {f: (out[f]["r"], out[f]["t"]) for f in range(5)})])
        g64 = [_anchor64(c, own, p, only=i)[0][0] for i in range(len(c["pairs"]))]  # each entry's own float64 median
        e64 = np.array([np.abs(np.array(g64) / true - 1).max(), *_pose_errors(c, cams64)])
        if verbose:
            print("seed %d: true gamma %.4f; restatement gamma %.4e, %.4f deg, %.5f units; float64 %.4e, %.4f deg, %.5f units; shared %d..%d, consistent %d..%d, link %d" %
                  (seed, true, *e32, *e64, links["shared"].min(), links["shared"].max(), links["consistent"].min(), links["consistent"].max(), seg[0]["link"]))
        worst32, worst64 = np.maximum(worst32, e32), np.maximum(worst64, e64)
    if verbose:
        print("worst: restatement %s, float64 %s" % (worst32, worst64))
    return worst32, worst64


def test_accuracy_of_a_second_batch_in_the_stored_map():
    """Measured over seeds 0-3 (deterministic; printed by this test): the table above and in DESIGN.md section 33.  The restatement's
    worst errors are asserted at twice the float64 yardstick's worst; the factor covers a change of seeds only."""
    w32, w64 = accuracy()
    assert (w32 <= 2 * w64).all(), (w32, w64)
    assert np.allclose(w32, RESTATED, rtol=2e-4) and np.allclose(w64, YARDSTICK, rtol=2e-4), (w32, w64)  # the table above is what was measured
    assert np.allclose(A.BOUNDS, 2 * w64, rtol=1e-3), (A.BOUNDS, 2 * w64)  # the figures the other tests hold the stage to


def test_two_segments_each_through_an_entry_of_its_own():
    """Pair 2 of the second batch LOW_PARALLAX: frames 0-2 are segment 0, frame 3 is LOST and the origin of frames 3-4, whose unit is
    the step of pair 3 (0.25) where segment 0's is that of pair 0 (0.35)."""
    for seed in range(2):
        c = A.two_batches(seed, lost_pair=2)
        assert c["frames"]["origin"].tolist() == [0, 0, 0, 3, 3] and c["frames"]["status"][3] == L.LOST
        out, seg, links, rows, land = A.anchor(c)
        assert (links["verdict"] == V["HOLDS"]).all(), (seed, links["verdict"])
        assert seg["status"].tolist() == [A.SEG_ANCHORED, 0, 0, A.SEG_ANCHORED, 0] and (out["status"] == A.ANCHORED).all()
        i0, i3 = int(seg[0]["link"]), int(seg[3]["link"])
        assert i0 != i3 and c["pairs"][i0][0] < 3 <= c["pairs"][i3][0] and links["chosen"].sum() == 2
        true0 = A.true_gamma(c["b1"], c["b2"])
        g0, g3 = float(seg[0]["gamma"]) / true0, float(seg[3]["gamma"]) / true0
        print("seed %d: gamma of segment 0 %.4f and of segment 3 %.4f of segment 0's true one (1.0 and %.4f)" % (seed, g0, g3, 0.25 / 0.35))
        assert abs(g0 - 1.0) <= A.BOUNDS[0] and abs(g3 / (0.25 / 0.35) - 1.0) <= A.BOUNDS[0], (seed, g0, g3)
        assert rows["origin"].tolist() == [0, 0, NONE, 3]  # pair 2 ends at the LOST frame
        assert rows["slot"].tolist() == [seg[0]["slot"]] * 2 + [NONE, seg[3]["slot"]] and rows["moved"][0] > 0 and rows["moved"][3] > 0 and rows["moved"][2] == 0


def test_self_anchor_agrees_with_the_trajectory():
    """Frames of a batch inserted into a store, and entries (q, slot of T) with q in T's segment: the map is the batch's own frame,
    so gamma is 1 and the anchored poses are the trajectory's, to the accuracy bound measured above."""
    b = K.out_and_back(0)
    desc = K.plant(b, np.random.default_rng(100))
    fr, lms, store = KC.reference(b, desc, [(f, f) for f in range(b["n"])], traj=L.FULL_TRAJ)
    _, _, lrows = L.reference(b, b["n"], traj=L.FULL_TRAJ)
    assert (fr["origin"] == 0).all()
    intr = lc.intrinsics(b["W"], b["H"], b["focal"])
    nq, corners, descs, matches = KC.batch_inputs(b, desc)
    pairs = K.LOOP_PAIRS
    rows = kfr.match_keyframes(nq, descs, store, pairs, b["cap"])
    fx, masks = kfr.localize_keyframes(nq, corners, rows, pairs, store, b["cap"], **intr)
    out, seg, links, arows, land = ar.anchor_frames(nq, matches, rows, pairs, fr, np.array(lrows), list(lms), fx, masks, store, b["cap"])
    holds = links["verdict"] == V["HOLDS"]
    assert holds.sum() >= 8 and seg[0]["status"] == A.SEG_ANCHORED and (out["status"] == A.ANCHORED).all()
    assert np.abs(links["gamma"][holds].astype(np.float64) - 1).max() <= A.BOUNDS[0]
    e_r = max(K.rotation_error_deg(out[f]["r"], np.asarray(fr[f]["r"], np.float64).reshape(3, 3)) for f in range(1, b["n"]))
    e_t = max(float(np.linalg.norm(out[f]["t"].astype(np.float64) - fr[f]["t"])) for f in range(1, b["n"]))
    print("self-anchor: gamma %.5f, %.4f deg, %.5f units off the trajectory" % (float(seg[0]["gamma"]), e_r, e_t))
    assert e_r <= A.BOUNDS[1] and e_t <= A.BOUNDS[2]
    # the landmarks likewise: moved within the bound of where they were
    for p in range(b["n"] - 1):
        good = (land[p]["flags"] & T.ORB_POINT_GOOD != 0) & (lms[p]["views"] != 0)
        X = np.stack([lms[p][k][good].astype(np.float64) for k in "xyz"], 1)
        d = np.stack([land[p][k][good].astype(np.float64) for k in "xyz"], 1) - X
        # X' - X = (A^T - I) gamma X + (gamma - 1) X - A^T a: the translation's bound plus the scale's and the rotation's times |X|
        assert (np.linalg.norm(d, axis=1) <= A.BOUNDS[2] + (A.BOUNDS[0] + np.radians(A.BOUNDS[1])) * np.linalg.norm(X, axis=1)).all()
