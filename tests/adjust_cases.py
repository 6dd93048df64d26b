"""Hand-built inputs of the adjustment stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_adjust_consecutive reads the raw counters, the stored records, the matcher's records, the frame records of
the trajectory stage and the records of the landmark stage.  The batches are landmark_cases' (`rail`, `cross`, `restart_batch`) and
localize_cases.views; a case runs the landmark stage on a batch under one set of frame records and then the adjustment under the
same set or another one (`adjust_frames`: what a test writes over the records between the two calls, so that a landmark that was
GOOD meets a pose that is not finite, or rays that have become parallel).

`cases` holds the constructions that pin BA-2..BA-7 as data -- the calls of each case and the outcome its construction implies -- so
that tests/test_adjust_ref.py runs them on the restatement and tests/test_gpu_adjust.py on the device.
"""
import numpy as np

import adjust_ref as ar
import landmark_cases as L
import localize_cases as lc
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = L.CHAINED, L.START, L.FEW, L.SPREAD, L.LOST, L.ORIGIN
HELD, REFINED, A_FEW, FAILED = orb.ORB_ADJUST_HELD, orb.ORB_ADJUST_REFINED, orb.ORB_ADJUST_FEW, orb.ORB_ADJUST_FAILED
RAIL = L.RAIL
NONE = ar.NONE
WIDE = dict(max_reproj_px=1000.0)  # a landmarks call that keeps every solved landmark in front of its cameras GOOD


def inputs(b, n=None):
    """What both stages read of a batch: (stored counts, records, matches) of its first n frames."""
    n = b["n"] if n is None else n
    nq = lc.stored(b)
    return nq[:n], [c[:nq[f]] for f, c in enumerate(b["corners"][:n])], [b["matches"][f][:nq[f]] for f in range(n - 1)]


def call(b, frames=None, adjust_frames=None, n_frames=None, intr=None, lm=None, **params):
    """One adjust call of a case: the batch; the frame records of the landmarks call (default: the batch's own) and those of the
    adjust call (default: the same); the adjust call's extent (default: the whole batch; the landmarks call always covers it);
    the intrinsics (default: RAIL); the landmarks call's other parameters `lm`; the adjust call's other parameters."""
    frames = b["frames"] if frames is None else frames
    return dict(batch=b, frames=frames, adjust_frames=frames if adjust_frames is None else adjust_frames,
                n_frames=b["n"] if n_frames is None else n_frames, intr=RAIL if intr is None else intr, lm=lm or {}, params=params)


def run_call(c, trace=None):
    """A call of a case on the restatements: dict(poses (n_frames,), recs (n_frames - 1, cap), lms: the landmark stage's records,
    frames: the records the adjust call read)."""
    b, n = c["batch"], c["n_frames"]
    lms = L.run(b, frames=c["frames"], intr=c["intr"], **c["lm"])[0]
    nq, corners, matches = inputs(b)
    poses, recs = ar.adjust(nq, corners, matches, c["adjust_frames"], lms, b["cap"], n_frames=n, trace=trace, **c["intr"], **c["params"])
    return dict(poses=poses, recs=recs, lms=lms, frames=c["adjust_frames"])


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def held_is_copied(res, frames=None):
    """BA-7: every HELD record is the trajectory's r and t bit for bit and zeros behind them."""
    fr = res["frames"] if frames is None else frames
    for g, rec in enumerate(res["poses"]):
        if rec["status"] == HELD:
            assert same_bits(rec["r"], fr["r"][g]) and same_bits(rec["t"], fr["t"][g]), g
            assert rec["cost_before"].tobytes() == rec["cost_after"].tobytes() == b"\0" * 4 and rec["observations"] == 0, g


def all_finite(res, frames):
    """BA-7: no non-finite byte in the record of a free frame or of a participating landmark."""
    for g, rec in enumerate(res["poses"]):
        if int(frames["status"][g]) == CHAINED:
            assert all(np.isfinite(rec[k]).all() for k in ("r", "t", "cost_before", "cost_after")), (g, rec)
    for k in "xyz":
        assert np.isfinite(res["recs"][k]).all()


def rotation_angle_deg(Ra, Rb):
    Ra, Rb = (np.asarray(a, np.float64).reshape(3, 3) for a in (Ra, Rb))
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra @ Rb.T) - 1.0) / 2.0, -1.0, 1.0))))


def turned(b, g, deg):
    """The batch with the keypoints of frame g replaced by the projections (rounded to pixels) of the cloud into a camera at the
    rail's position turned by `deg` degrees about its optical axis; returns (batch, the true R of camera g)."""
    out = L.copy_batch(b)
    R = tr.rot("z", deg)
    Q = (b["cloud"] - np.array([L.RAIL_BASE * g, 0.0, 0.0])) @ R.T
    u, v = 64.0 * Q[:, 0] / Q[:, 2] + 32.0, 64.0 * Q[:, 1] / Q[:, 2] + 32.0
    out["corners"][g]["x"][b["slots"][g]], out["corners"][g]["y"][b["slots"][g]] = np.rint(u).astype(np.int64), np.rint(v).astype(np.int64)
    assert (np.rint(u) >= 0).all() and (np.rint(v) >= 0).all()
    return out, R


def recount_owners(views, lms, frames, cap):
    """BA-3 slot by slot in plain Python: {(frame, keypoint slot): key} from the views of every participating landmark."""
    own = {}
    for (p, i), vs in views.items():
        for g, k in vs:
            if int(frames["status"][g]) == CHAINED and int(lms[p][i]["origin"]) == int(frames["origin"][g]):
                own[g, k] = min(own.get((g, k), NONE), p * cap + i)
    return own


# ---- the hand-built cases, as data (tests/test_adjust_ref.py, tests/test_gpu_adjust.py) ---------------------------------------
SMALL = L.SMALL
FAR = 4096  # `exact`: the keypoints and the principal point moved this far out


def exact(n=6, K=8, cap=SMALL):
    """A rail batch whose residuals are exactly 0: every keypoint and the principal point moved FAR pixels out in x and y, so that
    `fx (x / z) + cx` is rounded at a size where a binary32 step (2^-11 px) is a hundred times what LM-4's rounding leaves of
    error in the landmark stage's points (some 1e-5 px, measured at the rail's own cx = 32, where a step is 4e-6 px).  Every
    normal equation then has a right side of zeros, every step is zero, and the points of round r are those of round r - 1.
    Returns (batch, intrinsics)."""
    b = L.copy_batch(L.rail(n, K, cap=cap, v_hi=L.V_HI))
    for c in b["corners"]:
        c["x"][:], c["y"][:] = c["x"] + FAR, c["y"] + FAR
    return b, dict(fx=64.0, fy=64.0, cx=32.0 + FAR, cy=32.0 + FAR)


def fields(r, *names):
    return tuple(r[k].item() for k in names)


def cases():
    """The hand-built cases of BA-2..BA-7: a list of dict(name, calls, expect, cap).  `calls` are the adjust calls of the case, in
    order, on one program (`call`).  `expect(results)` asserts the outcome the construction implies on results[k] = dict(poses,
    recs, lms, frames) of call k -- the restatement's (tests/test_adjust_ref.py) or the device's (tests/test_gpu_adjust.py).  A
    case's capacity is that of its batches: SMALL, 64, 257 (a second block of one thread in the per-slot kernels) or 300 (more
    than 256 owned slots in a frame, so that the partial sums wrap)."""
    out = []

    def add(name, calls, expect):
        assert len({c["batch"]["cap"] for c in calls}) == 1
        out.append(dict(name=name, calls=calls, expect=expect, cap=calls[0]["batch"]["cap"]))

    # ---- exact data: a fixed point to the bit ----
    b, intr = exact()

    def fixed_point(res, b=b):
        for r in res:
            assert r["poses"]["status"].tolist() == [HELD, HELD] + [REFINED] * 4 and r["poses"]["observations"].tolist() == [0, 0, 8, 8, 8, 8]
            assert not r["poses"]["cost_before"].tobytes().strip(b"\0") and not r["poses"]["cost_after"].tobytes().strip(b"\0")
            assert same_bits(r["poses"]["r"], b["frames"]["r"]) and same_bits(r["poses"]["t"], b["frames"]["t"])
            assert same_bits(r["recs"], r["lms"]) and (r["lms"][0]["flags"] == GOOD | PAR).all() and (r["lms"][0]["views"] == 6).all()
            held_is_copied(r)

    add("exact data: rounds 1, 4, 16", [call(b, intr=intr, rounds=k) for k in (1, 4, 16)], fixed_point)

    # ---- BA-4: one free frame's keypoints turned about the optical axis ----
    K, g, deg = 40, 3, 5.0
    b, truth = turned(L.rail(5, K, cap=64, v_hi=L.V_HI), g, deg)

    def moved(res, b=b, g=g, truth=truth, deg=deg, K=K):
        for r, rounds in zip(res, (1, 4, 16)):
            po = r["poses"]
            assert po["status"].tolist() == [HELD, HELD, REFINED, REFINED, REFINED] and po["observations"].tolist() == [0, 0, K, K, K]
            assert 0 < po["cost_after"][g] < po["cost_before"][g], (rounds, po[g])
            before, after = rotation_angle_deg(b["frames"]["r"][g], truth), rotation_angle_deg(po["r"][g], truth)
            assert abs(before - deg) < 1e-3 and after < 0.5 * before, (rounds, before, after)
            held_is_copied(r)
            all_finite(r, r["frames"])

    add("frame 3 turned by 5 degrees: rounds 1, 4, 16", [call(b, lm=WIDE, rounds=k) for k in (1, 4, 16)], moved)

    # ---- BA-3: owners ----
    n, K = 5, 7
    b = L.rail(n, K, cap=SMALL, v_hi=L.V_HI)
    s = b["slots"]
    b["matches"]["index"][0, s[0][0]] = s[1][1]  # landmark 0's first slot continues into landmark 1's chain

    def shared(res, s=s, n=n, K=K):
        r = res[0]
        a, c = r["lms"][0][s[0][0]], r["lms"][0][s[0][1]]
        assert a["flags"] & GOOD and c["flags"] & GOOD and a["views"] == c["views"] == n and a["tail_index"] == c["tail_index"]
        assert r["poses"]["status"].tolist() == [HELD, HELD] + [REFINED] * 3 and r["poses"]["observations"].tolist() == [0, 0, K, K, K]
        for q in (a, c):
            assert fields(r["recs"][0][s[0][int(q is c)]], "views", "origin", "tail_index") == fields(q, "views", "origin", "tail_index")
        all_finite(r, r["frames"])

    add("two landmarks share their later views", [call(b, lm=WIDE)], shared)
    b = L.cross()
    b["corners"][0]["x"][4], b["corners"][0]["y"][4] = 32, 32  # a second landmark on the first one's pixels, into the same slot of frame 1
    b["matches"]["index"][0, 4] = 5
    b["points"][0, 4] = (0.0, 0.0, 8.0, GOOD | PAR)

    def crossed(res):
        r = res[0]
        for i in (3, 4):
            assert fields(r["lms"][0][i], "x", "y", "z", "flags", "views", "inliers") == (0.0, 0.0, 8.0, GOOD | PAR, 3, 3)
        assert same_bits(r["recs"], r["lms"])  # LM-4 again under the same poses
        assert fields(r["poses"][2], "status", "observations", "cost_before", "cost_after") == (A_FEW, 1, 0.0, 0.0)
        assert same_bits(r["poses"]["r"], r["frames"]["r"]) and same_bits(r["poses"]["t"], r["frames"]["t"])
        held_is_copied(r)

    add("cross: two landmarks on one view, one owned slot", [call(b, intr=L.CROSS)], crossed)
    # a frame that is CHAINED in segment 0 and the origin of segment 2; landmark 0 of segment 0 is not GOOD (a keypoint 6 px off),
    # so slot s[2][0] of frame 2 is seen by a GOOD landmark of segment 2 only
    n, K = 6, 7
    b = L.rail(n, K, cap=SMALL, plan=[ORIGIN, START, CHAINED, SPREAD, CHAINED, CHAINED], v_hi=L.V_HI)
    s = b["slots"]
    b["corners"][1]["y"][s[1][0]] += 6

    def two_segments(res, s=s, K=K):
        r = res[0]
        lm = r["lms"]
        assert r["frames"]["origin"].tolist() == [0, 0, 0, 2, 2, 2]
        assert lm[0][s[0][0]]["views"] == 3 and lm[0][s[0][0]]["flags"] == 0 and lm[0][s[0][0]]["z"] != 0  # solved, not GOOD
        assert all(lm[2][s[2][l]]["flags"] & GOOD and lm[2][s[2][l]]["origin"] == 2 and lm[2][s[2][l]]["views"] == 4 for l in range(K))
        po = r["poses"]
        assert po["status"].tolist() == [HELD, HELD, REFINED, HELD, REFINED, REFINED] and po["observations"].tolist() == [0, 0, K - 1, 0, K, K]
        assert same_bits(r["recs"][0][s[0][0]], lm[0][s[0][0]])  # BA-7: byte for byte
        held_is_copied(r)
        all_finite(r, r["frames"])

    add("a CHAINED frame that is the next segment's origin; a landmark that is not GOOD", [call(b)], two_segments)

    # ---- BA-4: observation counts ----
    five, six = L.rail(4, 5, cap=SMALL, v_hi=L.V_HI), L.rail(4, 6, cap=SMALL, v_hi=L.V_HI)

    def few(res, five=five):
        r5, r6 = res
        assert r5["poses"]["status"].tolist() == [HELD, HELD, A_FEW, A_FEW] and r5["poses"]["observations"].tolist() == [0, 0, 5, 5]
        assert not r5["poses"]["cost_before"].tobytes().strip(b"\0") and not r5["poses"]["cost_after"].tobytes().strip(b"\0")
        assert same_bits(r5["poses"]["r"], five["frames"]["r"]) and same_bits(r5["poses"]["t"], five["frames"]["t"])
        assert same_bits(r5["recs"], r5["lms"])  # no pose moved: LM-4 and LM-5 again under the same poses
        assert r6["poses"]["status"].tolist() == [HELD, HELD, REFINED, REFINED] and r6["poses"]["observations"].tolist() == [0, 0, 6, 6]

    add("5 owned slots FEW, 6 REFINED", [call(five), call(six)], few)

    # ---- BA-4, BA-5, BA-7: records that are not finite, unsolved landmarks ----
    n, K = 5, 7
    b = L.rail(n, K, cap=SMALL, v_hi=L.V_HI)
    s = b["slots"]
    calls, labels = [], []
    for g in (3, 1):  # a free frame, a held one
        for bad in (np.nan, np.inf, -np.inf):
            for field, k in (("t", 0), ("r", 4)):
                fr = b["frames"].copy()
                fr[field][g][k] = bad
                calls.append(call(b, adjust_frames=fr))
                labels.append((g, bad, field, k))

    def not_finite(res, b=b, s=s, n=n, K=K, labels=labels):
        assert len(res) == 12
        for r, (g, bad, field, k) in zip(res, labels):
            po = r["poses"]
            assert (r["lms"][0]["flags"][s[0]] == GOOD | PAR).all()
            if g == 3:
                assert po["status"].tolist() == [HELD, HELD, REFINED, FAILED, REFINED], (labels, po)
                assert not po[3].tobytes()[:56].strip(b"\0") and po[3]["observations"] == K
                all_finite(r, r["frames"])
            else:
                assert po["status"].tolist() == [HELD, HELD, REFINED, REFINED, REFINED]
                assert same_bits(po[field][1], r["frames"][field][1]) and not np.isfinite(po[field][1][k])
            held_is_copied(r)
            for l in range(K):  # every landmark sees the frame: unsolved in every round, X kept, no view of that frame an inlier
                got, was = r["recs"][0][s[0][l]], r["lms"][0][s[0][l]]
                assert fields(got, "x", "y", "z", "views") == fields(was, "x", "y", "z", "views") and got["flags"] == 0 and got["inliers"] < n

    add("NaN, +inf, -inf in t[0], r[4] of a free and of a held frame", calls, not_finite)
    # landmark 0 has two views, frames 0 and 1, both at the principal point; the landmarks call sees camera 1 turned so that the
    # rays meet near z = 8, the adjust call sees it unturned: parallel rays, A = diag(2, 2, 0), det = 0
    b = L.rail(4, K, cap=SMALL, v_hi=L.V_HI)
    s = b["slots"]
    b["points"]["flags"][1, s[1][0]] = 0
    for f in (0, 1):
        b["corners"][f]["x"][s[f][0]], b["corners"][f]["y"][s[f][0]] = 32, 32
    fr_lm = b["frames"].copy()
    fr_lm["r"][1] = tr.rot("y", np.degrees(np.arctan(1.0 / 16.0))).astype(F).ravel()

    def parallel(res, s=s):
        r = res[0]
        was, got = r["lms"][0][s[0][0]], r["recs"][0][s[0][0]]
        assert fields(was, "views", "inliers", "flags") == (2, 2, GOOD | PAR) and abs(was["z"] - 8.0) < 0.1
        assert fields(got, "x", "y", "z") == fields(was, "x", "y", "z")  # BA-5: unsolved, X kept
        assert fields(got, "views", "inliers", "flags", "origin", "tail_index") == (2, 1, 0) + fields(was, "origin", "tail_index")
        held_is_copied(r)

    add("parallel rays after a pose is set so: the landmark keeps its X", [call(b, frames=fr_lm, adjust_frames=b["frames"])], parallel)

    # ---- extents, no free frame, empty frames ----
    b = L.rail(5, K, cap=SMALL, v_hi=L.V_HI)
    island = L.rail(3, K, cap=SMALL, plan=[ORIGIN, LOST, START], v_hi=L.V_HI)

    def extents(res, K=K):
        two, three, isl = res
        for r, m in ((two, 2), (three, 3)):
            assert len(r["poses"]) == m and len(r["recs"]) == m - 1 and same_bits(r["recs"], r["lms"][:m - 1])
            assert same_bits(r["poses"]["r"], r["frames"]["r"][:m]) and same_bits(r["poses"]["t"], r["frames"]["t"][:m])
        assert two["poses"]["status"].tolist() == [HELD, HELD]
        # no landmark of the five-frame call lies inside three frames: frame 2 is free and owns nothing
        assert three["poses"]["status"].tolist() == [HELD, HELD, A_FEW] and three["poses"]["observations"].tolist() == [0, 0, 0]
        assert isl["poses"]["status"].tolist() == [HELD] * 3 and (isl["lms"][1]["views"][:K] == 2).all() and same_bits(isl["recs"], isl["lms"])
        for r in res:
            held_is_copied(r)

    add("n_frames 2 and 3; three frames without a free one", [call(b, n_frames=2), call(b, n_frames=3), call(island)], extents)
    lost = L.rail(5, K, cap=SMALL, plan=[ORIGIN] + [LOST] * 4, v_hi=L.V_HI)
    empty = L.rail(5, K, cap=SMALL, v_hi=L.V_HI)
    empty["counts"][:] = 0

    def nothing(res):
        for r, st in zip(res, ([HELD] * 5, [HELD, HELD] + [A_FEW] * 3)):
            assert r["poses"]["status"].tolist() == st and not r["recs"].tobytes().strip(b"\0") and (r["poses"]["observations"] == 0).all()
            assert same_bits(r["poses"]["r"], r["frames"]["r"]) and same_bits(r["poses"]["t"], r["frames"]["t"])
            held_is_copied(r)

    add("every frame LOST; every counter 0", [call(lost), call(empty)], nothing)
    b = L.rail(6, 8, cap=SMALL, octaves=2, v_hi=L.V_HI)

    def octaves(res):
        r = res[0]
        assert r["poses"]["status"].tolist() == [HELD, HELD] + [REFINED] * 4 and (r["recs"][0]["flags"] == GOOD | PAR).all()
        assert np.abs(r["poses"]["t"] - r["frames"]["t"]).max() < 1e-4 and (r["poses"]["cost_after"] < 1e-6).all()

    add("octaves 0, 1, 2", [call(b)], octaves)

    # ---- the block edges: every slot a landmark ----
    for K, n in ((257, 6), (300, 4)):
        b = L.rail(n, K, v_hi=L.V_HI)

        def full(res, K=K, n=n):
            for r in res:
                assert r["poses"]["status"].tolist() == [HELD, HELD] + [REFINED] * (n - 2) and r["poses"]["observations"].tolist() == [0, 0] + [K] * (n - 2)
                assert (r["recs"][0]["flags"] == GOOD | PAR).all() and (r["recs"][0]["inliers"] == n).all()
                assert (r["poses"]["cost_after"][2:] < 1e-4).all() and np.abs(r["poses"]["t"] - r["frames"]["t"]).max() < 1e-3
                all_finite(r, r["frames"])

        add("capacity %d, every slot a landmark: rounds 1, 4, 16" % K, [call(b, rounds=k) for k in (1, 4, 16)], full)
    return out
