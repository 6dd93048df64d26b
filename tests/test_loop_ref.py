"""The loop stage's restatement (tests/loop_ref.py) on the CPU: each clause of LC-2 and LC-3 on hand-built
records of the rail camera (tests/landmark_cases.py), the salt and the list index in the draws, and the accuracy of the fixes on
the out-and-back batches (tests/loop_cases.py) with planted descriptors against the true cameras."""
import numpy as np

import epipolar_ref as er
import bridge_ref as brr
import landmark_cases as L
import localize_cases as lc
import localize_ref as lr
import loop_cases as K
import loop_ref as lpr
import verify_ref as vr
from tinyslam_amd import orb

F = np.float32
NONE = orb.ORB_MATCH_NONE
GOOD = orb.ORB_POINT_GOOD
OK, NOMAP, FEW = orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_NOMAP, orb.ORB_LOCALIZE_FEW
CAP, LANDS = 16, 12


def _rail(n=5, plan=None, K_=LANDS, cap=CAP):
    b = L.rail(n, K_, cap=cap, plan=plan, v_hi=L.V_HI)
    lms, _ = L.run(b)
    return b, [lm.copy() for lm in lms]


def _owners(b, lms, n=None, frames=None, counts=None):
    n = b["n"] if n is None else n
    nq = lc.stored(b) if counts is None else counts
    return lpr.owners(nq, [b["matches"][f] for f in range(n - 1)], b["frames"] if frames is None else frames, lms, b["cap"], n)


def _row(b, q, T, distance=10, second=100):
    """The true row of the entry (q, T): landmark l's slot in q points at its slot in T."""
    row = np.zeros(b["cap"], orb.MATCH_DTYPE)
    row["index"], row["distance"], row["second"] = NONE, 0xFFFF, 0xFFFF
    row["index"][b["slots"][q]], row["distance"][b["slots"][q]], row["second"][b["slots"][q]] = b["slots"][T], distance, second
    return row


def _run(b, lms, pairs, rows, n=None, frames=None, trace=None, **params):
    nq = lc.stored(b)
    n = b["n"] if n is None else n
    return lpr.loop_pairs(nq, [c[:nq[f]] for f, c in enumerate(b["corners"])], [b["matches"][f] for f in range(n - 1)], rows, pairs,
                          b["frames"] if frames is None else frames, lms[:n - 1], b["cap"], L=n, trace=trace, **{**L.RAIL, **params})


# ---- LC-2 --------------------------------------------------------------------------------------------------------------------
def test_owners_participation_walk_and_key():
    b, lms = _rail()
    s, n, cap = b["slots"], b["n"], b["cap"]
    own = _owners(b, lms)
    for g in range(n):  # every landmark starts at pair 0 and is seen in all five views
        assert own[g][s[g]].tolist() == s[0].tolist() and (own[g][LANDS:] == lpr.NONE).all()
    # the GOOD flag
    bad = [lm.copy() for lm in lms]
    bad[0]["flags"][s[0][3]] &= ~np.uint32(GOOD)
    o2 = _owners(b, bad)
    assert all(o2[g][s[g][3]] == lpr.NONE for g in range(n)) and (o2 != lpr.NONE).sum() == (LANDS - 1) * n
    # p + views = L takes part, p + views = L + 1 does not
    assert (lms[0]["views"][s[0]] == n).all()
    assert (_owners(b, lms, n=n - 1) == lpr.NONE).all()
    short = [lm.copy() for lm in lms]
    short[0]["views"][s[0][:4]] = n - 1
    o3 = _owners(b, short, n=n - 1)
    assert (o3 != lpr.NONE).sum() == 4 * (n - 1) and o3[n - 2][s[n - 2][:4]].tolist() == s[0][:4].tolist()
    # a walk that stops early: the keypoint of the third view is not stored
    counts = lc.stored(b).copy()
    counts[2] = LANDS - 1
    cut = int(np.nonzero(s[2] == LANDS - 1)[0][0])
    o4 = _owners(b, lms, counts=counts)
    assert [o4[g][s[g][cut]] != lpr.NONE for g in range(n)] == [True, True, False, False, False]
    assert (o4 != lpr.NONE).sum() == LANDS * n - 3
    # two landmarks on one view: the smaller key wins, whatever the order
    two = [lm.copy() for lm in lms]
    l = 5
    two[1][s[1][l]] = lms[0][s[0][l]]
    two[1]["views"][s[1][l]] = 2  # views (1, s1[l]) and (2, s2[l]), which landmark l of pair 0 sees too
    o5 = _owners(b, two)
    assert o5.tolist() == own.tolist()
    two[0]["flags"][s[0][l]] = 0
    o6 = _owners(b, two)
    assert [int(o6[g][s[g][l]]) for g in range(n)] == [lpr.NONE, cap + s[1][l], cap + s[1][l], lpr.NONE, lpr.NONE]
    assert lpr.refused(1 << 16, 1 << 16) and not lpr.refused((1 << 16) - 1, 1 << 16) and lpr.refused(4096, (1 << 20) + 1)


def test_owners_register_by_origin_whatever_the_status():
    # frame 2 is CHAINED in segment 0 and the origin of the segment that a RESTART begins: it takes the old segment's landmarks only
    b, lms = _rail(6, plan=[L.ORIGIN, L.START, L.CHAINED, L.FEW, L.CHAINED, L.CHAINED])
    s, cap = b["slots"], b["cap"]
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 2, 2, 2]
    assert (lms[0]["origin"][s[0]] == 0).all() and (lms[2]["origin"][s[2]] == 2).all() and (lms[2]["views"][s[2]] == 4).all()
    own = _owners(b, lms)
    assert own[2][s[2]].tolist() == s[0].tolist()  # keys of pair 0, not 2 * cap + ...
    assert own[3][s[3]].tolist() == (2 * cap + s[2]).tolist() and own[5][s[5]].tolist() == (2 * cap + s[2]).tolist()
    # a LOST frame is its own origin and takes the landmarks that start in it
    b, lms = _rail(6, plan=[L.ORIGIN, L.START, L.CHAINED, L.LOST, L.START, L.CHAINED])
    s = b["slots"]
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 3, 3, 3] and b["frames"]["status"][3] == L.LOST
    own = _owners(b, lms)
    assert own[3][s[3]].tolist() == (3 * cap + s[3]).tolist() and own[2][s[2]].tolist() == s[0].tolist()
    pairs = [(5, 3), (0, 3), (1, 2)]
    out, masks = _run(b, lms, pairs, [_row(b, q, T) for q, T in pairs])
    assert out["status"].tolist() == [OK, OK, OK] and out["origin"].tolist() == [3, 3, 0] and out["query_origin"].tolist() == [3, 0, 0]
    assert out["candidates"].tolist() == [LANDS] * 3
    # the LOST target's camera is the identity: the pose in the map is the fix itself after a polar step
    assert np.allclose(out["pose_r"][0], out["r"][0], atol=1e-6) and out["pose_t"][0].tobytes() == out["t"][0].tobytes()
    # the rail: camera q relative to camera T is a shift of 0.5 (q - T) along -x
    for i, (q, T) in enumerate(pairs):
        assert np.allclose(out["r"][i], np.eye(3).ravel(), atol=2e-3) and np.allclose(out["t"][i], (-L.RAIL_BASE * (q - T), 0, 0), atol=2e-2), out[i]


# ---- LC-3 --------------------------------------------------------------------------------------------------------------------
def test_candidates_each_clause_of_the_filter():
    b, lms = _rail()
    s, n = b["slots"], b["n"]
    q, T = 4, 0

    def count(row, **kw):
        t = {}
        out, masks = _run(b, lms, [(q, T)], [row], trace=t, **kw)
        return t[0]["slots"].tolist(), out, masks

    full, out, masks = count(_row(b, q, T))
    assert full == sorted(s[q].tolist()) and out["candidates"][0] == LANDS and out["status"][0] == OK and masks[0].sum() == out["inliers"][0]
    a = int(s[q][2])
    for field, value, keeps in (("index", NONE, False), ("index", LANDS, False), ("index", LANDS - 1, True), ("distance", 64, True),
                                ("distance", 65, False)):
        row = _row(b, q, T)
        row[field][a] = value
        assert (a in count(row)[0]) == keeps, (field, value)
    for second, keeps in ((80, False), (81, True)):  # 64 < 0.8f * 80 = 64 fails in binary32, 64 < 0.8f * 81 holds
        row = _row(b, q, T)
        row["distance"][a], row["second"][a] = 64, second
        assert (a in count(row)[0]) == keeps, second
    assert F(0.8) * F(80) == F(64) and F(64) < F(0.8) * F(81)
    row = _row(b, q, T)
    row["distance"][a] = 20
    assert a not in count(row, max_distance=19)[0] and a in count(row, max_distance=20)[0]
    assert a not in count(row, ratio=0.2)[0] and a in count(row, ratio=0.21)[0]
    # a keypoint of T without an owner
    bad = [lm.copy() for lm in lms]
    bad[0]["flags"][s[0][2]] = 0
    assert a not in _trace_slots(b, bad, q, T) and len(_trace_slots(b, bad, q, T)) == LANDS - 1
    # two query slots on one k each count; stale records at and above n_q(q) are not read
    row = _row(b, q, T)
    row["index"][s[q][3]] = row["index"][s[q][4]]
    row[LANDS:] = row[s[q][0]]
    slots, out, _ = count(row)
    assert slots == full and out["candidates"][0] == LANDS


def _trace_slots(b, lms, q, T):
    t = {}
    _run(b, lms, [(q, T)], [_row(b, q, T)], trace=t)
    return t[0]["slots"].tolist()


def test_targets_and_queries_at_the_edge_of_the_map():
    b, lms = _rail()
    n = b["n"]
    short = [lm.copy() for lm in lms]
    for p in range(len(short)):
        short[p]["views"] = np.minimum(short[p]["views"], n - 1 - p)  # the landmarks of a call over n - 1 frames
    pairs = [(0, n - 2), (0, n - 1), (n - 1, 0), (n - 1, n - 2)]
    rows = [_row(b, q, T) for q, T in pairs]
    out, masks = _run(b, short, pairs, rows, n=n - 1)
    # T = L - 1 is the last frame of the map, T = L is outside it; a query at or above L is read like any other
    assert out["status"].tolist() == [OK, NOMAP, OK, OK] and out["query_origin"].tolist() == [0, 0, 0, 0]
    assert not out[1].tobytes().replace(np.uint32(NOMAP).tobytes(), b"").strip(b"\0") and not masks[1].any()
    # a query above the trajectory call's frames has no origin
    out2, _ = _run(b, short, pairs, rows, n=n - 1, frames=b["frames"][:n - 1])
    assert out2["query_origin"].tolist() == [0, 0, lpr.NONE, lpr.NONE] and out2["r"].tobytes() == out["r"].tobytes()
    # FEW: five candidates; the record is zero but for the status
    row = _row(b, 0, 1)
    row["index"][b["slots"][0][5:]] = NONE
    few, fm = _run(b, lms, [(0, 1)], [row])
    assert few["status"][0] == FEW and not few[0]["r"].any() and few["candidates"][0] == 0 and few["origin"][0] == 0 and not fm.any()
    # a frame record of T that is not finite: NOMAP
    fr = b["frames"].copy()
    fr["t"][2][1] = np.nan
    nan, _ = _run(b, lms, [(0, 2), (0, 1)], [_row(b, 0, 2), _row(b, 0, 1)], frames=fr)
    assert nan["status"].tolist() == [NOMAP, OK]
    fr = b["frames"].copy()
    fr["r"][0], fr["t"][0] = np.nan, np.inf  # the origin's own record is never read (LM-2)
    assert _run(b, lms, [(3, 0)], [_row(b, 3, 0)], frames=fr)[0]["status"][0] == OK


def test_pose_in_map_is_the_trajectory_compose():
    R = [F(v) for v in (0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0)]
    Rp, tp = lpr.pose_in_map(R, [F(1), F(2), F(3)], R, [F(10), F(20), F(30)])
    assert [float(v) for v in Rp] == [-1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0] and [float(v) for v in tp] == [-19.0, 12.0, 33.0]
    Rz, tz = lpr.pose_in_map(R, [F(1), F(2), F(np.inf)], R, [F(10), F(20), F(30)])
    assert not any(Rz) and not any(tz)


# ---- LC-4 --------------------------------------------------------------------------------------------------------------------
def test_salt_list_index_and_duplicates():
    assert lpr.SEED_SALT == 0x4C433031 == int.from_bytes(b"LC01", "big")
    assert lpr.SEED_SALT not in (0, er.SEED_SALT, lr.SEED_SALT, brr.SEED_SALT)
    b, lms = _rail()
    pairs = [(4, 0), (3, 1), (4, 0)]
    rows = [_row(b, q, T) for q, T in pairs]
    t = {}
    out, masks = _run(b, lms, pairs, rows, trace=t, seed=99, hypotheses=8)
    M = len(t[1]["rec"])
    mix = vr.lowbias32(vr.lowbias32(np.uint32(99 ^ 0x4C433031)) ^ np.uint32(1))  # lowbias32(lowbias32(seed ^ salt) ^ list index)
    h = np.arange(8, dtype=np.uint32)
    first = ((vr.lowbias32(mix ^ (h << np.uint32(5))).astype(np.uint64) * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
    J, ok = lr.sample(99 ^ lr.SEED_SALT ^ lpr.SEED_SALT, 1, M, 8)
    assert J[:, 0].tolist() == first.tolist() and ok.all() and lr.sample(99, 1, M, 8)[0].tolist() != J.tolist()
    X, inl = lpr.fix(t[1]["rec"], 1, lpr.defaults(**L.RAIL, seed=99, hypotheses=8))
    assert X["hypothesis"] == out["hypothesis"][1] and X["r"].tobytes() == out["r"][1].tobytes()
    # the same two frames at list positions 0 and 2: the same candidates, other draws
    assert t[0]["rec"].tobytes() == t[2]["rec"].tobytes() and t[0]["slots"].tolist() == t[2]["slots"].tolist()
    M = len(t[0]["rec"])
    assert lr.sample(99 ^ lr.SEED_SALT ^ lpr.SEED_SALT, 0, M, 8)[0].tolist() != lr.sample(99 ^ lr.SEED_SALT ^ lpr.SEED_SALT, 2, M, 8)[0].tolist()
    d = lpr.defaults(1, 1, 0, 0)
    assert (d["max_reproj_px"], d["hypotheses"], d["max_distance"], d["seed"]) == (2.0, 512, 64, 0) and d["ratio"] == F(0.8)


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
# Measured on this restatement (deterministic): over seeds 0-3 and the nine listed pairs the worst errors are 0.300 degrees and 0.0630
# segment units for the relative pose, 0.300 degrees and 0.0520 units for the pose in the map.  Asserted with a factor 2, which
# covers a change of seeds only.  At 64 x 48 and focal 60 one pixel is about 0.95 degrees.
ROT_DEG, T_UNITS, POSE_ROT_DEG, POSE_T_UNITS = 2 * 0.300, 2 * 0.0630, 2 * 0.300, 2 * 0.0520


def test_accuracy_on_the_out_and_back_path():
    worst = np.zeros(4)
    for seed in range(4):
        b = K.out_and_back(seed)
        desc = K.plant(b, np.random.default_rng(100 + seed))
        rows = K.rows_ref(desc, K.LOOP_PAIRS)
        fr, lms, out, masks = K.reference(b, K.LOOP_PAIRS, rows, traj=L.FULL_TRAJ)
        assert fr["status"].tolist() == [L.ORIGIN, L.START] + [L.CHAINED] * 9 and (out["status"] == OK).all(), (seed, out["status"])
        for i, (q, T) in enumerate(K.LOOP_PAIRS):
            rec = out[i]
            assert rec["origin"] == 0 and rec["query_origin"] == 0 and 40 <= rec["candidates"] <= 128 and rec["inliers"] >= rec["candidates"] - 2
            assert masks[i].sum() == rec["inliers"] and rec["step"] == np.sqrt((rec["t"][0] * rec["t"][0] + rec["t"][1] * rec["t"][1]) + rec["t"][2] * rec["t"][2])
            (Rr, tr_), (Rp, tp) = K.true_relative(b, q, T, 0)
            e = np.array([K.rotation_error_deg(rec["r"], Rr), np.linalg.norm(rec["t"] - tr_), K.rotation_error_deg(rec["pose_r"], Rp),
                          np.linalg.norm(rec["pose_t"] - tp)])
            worst = np.maximum(worst, e)
            assert e[0] <= ROT_DEG and e[1] <= T_UNITS and e[2] <= POSE_ROT_DEG and e[3] <= POSE_T_UNITS, (seed, q, T, e)
        (Rr, tr_), _ = K.true_relative(b, 10, 0, 0)  # the trajectory's own record of frame 10, beside the loop's: printed, not bounded
        print("seed %d: trajectory at frame 10: %.4f deg, %.4f units; loop (10, 0): %.4f deg, %.4f units" %
              (seed, K.rotation_error_deg(fr["r"][10], Rr), np.linalg.norm(fr["t"][10] - tr_), K.rotation_error_deg(out["pose_r"][0], Rr),
               np.linalg.norm(out["pose_t"][0] - tr_)))
    print("worst: relative %.4f deg %.4f units; in the map %.4f deg %.4f units" % tuple(worst))
