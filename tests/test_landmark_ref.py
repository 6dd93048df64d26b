"""The landmark stage's definition on the CPU restatement tests/landmark_ref.py: hand-built arrays
(tests/landmark_cases.py) that pin each clause, and the accuracy of the fused point against the trajectory's two-view point on the
constructed camera paths of section 20."""
import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import landmark_cases as L
import landmark_ref as lmr
import localize_cases as lc
import pose_ref as pr
import trajectory_ref as tr
import verify_ref as vr
from tinyslam_amd import orb

F = np.float32
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = L.CHAINED, L.START, L.FEW, L.SPREAD, L.LOST, L.ORIGIN
NO_ORIGIN = orb.ORB_LANDMARK_NO_ORIGIN


def _zero(rec):
    return rec.tobytes() == np.zeros((), orb.LANDMARK_DTYPE).tobytes()


def _rows_from(out, origin):
    """LM-6's row of each pair, counted from its records."""
    rows = np.zeros(len(out), orb.LANDMARK_ROW_DTYPE)
    for p, o in enumerate(out):
        s = o["views"] != 0
        rows[p] = (int(s.sum()), int(((o["flags"] & GOOD) != 0).sum()), int(o["views"].max(initial=0)), origin[p])
    return rows


def _near(rec, X, tol=1e-4):
    got = np.array([rec["x"], rec["y"], rec["z"]], np.float64)
    return np.abs(got - X).max() <= tol * np.abs(X).max()


# ---- LM-3 --------------------------------------------------------------------------------------------------------------------
def test_chains_of_one_two_and_every_live_slot():
    """All K landmarks chain through the batch: one start each in pair 0, n_frames views, nothing in the later pairs.  A point that
    is not GOOD stops the link into it and the slot behind it starts again; the tail is the keypoint of the last view."""
    n, K = 5, 7
    b = L.rail(n, K)
    s = b["slots"]
    out, rows = L.run(b)
    assert rows.tolist() == [(K, K, n, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    for l in range(K):
        r = out[0][s[0][l]]
        assert (r["views"], r["inliers"], r["flags"], r["origin"], r["tail_index"]) == (n, n, GOOD | PAR, 0, s[n - 1][l]) and _near(r, b["cloud"][l])
    assert all(_zero(r) for p in range(1, n - 1) for r in out[p])
    # landmark 0 is not GOOD in pair 1: a chain of one live slot (two views), then one of two (three views) from pair 2
    # landmark 1 is not GOOD in pair 2: a chain of two live slots (three views), then one of one from pair 3
    b["points"]["flags"][1, s[1][0]] = PAR
    b["points"]["flags"][2, s[2][1]] = 0
    out, rows = L.run(b)
    a0, a2, b0, b3 = out[0][s[0][0]], out[2][s[2][0]], out[0][s[0][1]], out[3][s[3][1]]
    assert (a0["views"], a0["tail_index"], a2["views"], a2["tail_index"]) == (2, s[1][0], 3, s[4][0])
    assert (b0["views"], b0["tail_index"], b3["views"], b3["tail_index"]) == (3, s[2][1], 2, s[4][1])
    assert _zero(out[1][s[1][0]]) and _zero(out[2][s[2][1]])
    # a start at p != o(p): camera p's pose is its frame record, and the point is still in the origin's frame
    for r, l in ((a0, 0), (a2, 0), (b0, 1), (b3, 1)):
        assert r["flags"] == GOOD | PAR and r["origin"] == 0 and r["inliers"] == r["views"] and _near(r, b["cloud"][l]), (r, l)
    assert rows.tolist() == [(K, K, n, 0), (0, 0, 0, 0), (1, 1, 3, 0), (1, 1, 2, 0)]
    assert rows.tobytes() == _rows_from(out, [0] * 4).tobytes()
    # PARALLAX: GOOD and some live slot of the chain carries it
    b["points"]["flags"][:, :] &= ~np.uint32(PAR)
    b["points"]["flags"][3, s[3][2]] |= PAR
    out, _ = L.run(b)
    assert out[0][s[0][2]]["flags"] == GOOD | PAR and out[0][s[0][3]]["flags"] == GOOD and out[0][s[0][0]]["flags"] == GOOD


def test_no_successor_gives_a_one_view_start():
    """ORB_MATCH_NONE, an index at the stored count and one above it end the chain at its first view; the landmark's slot in the
    next pair starts again.  Stale GOOD points at and above the counter are no starts and no successors."""
    n, K = 4, 6
    b = L.rail(n, K, cap=K + 2)
    s = b["slots"]
    for f in range(n - 1):  # stale records above the counters: GOOD points with matches among themselves
        b["points"][f, K:] = (1.0, 1.0, 8.0, GOOD | PAR)
        b["matches"]["index"][f, K:] = K, K + 1
    b["matches"]["index"][0, s[0][0]] = orb.ORB_MATCH_NONE
    b["matches"]["index"][0, s[0][1]] = K
    b["matches"]["index"][0, s[0][2]] = K + 1
    out, rows = L.run(b)
    for l in (0, 1, 2):
        r, nxt = out[0][s[0][l]], out[1][s[1][l]]
        assert (r["views"], r["inliers"], r["flags"], r["tail_index"], r["origin"]) == (1, 0, 0, s[0][l], 0) and (r["x"], r["y"], r["z"]) == (0, 0, 0)
        assert (nxt["views"], nxt["flags"], nxt["tail_index"]) == (n - 1, GOOD | PAR, s[n - 1][l]) and _near(nxt, b["cloud"][l])
    assert all(_zero(r) for p in range(n - 1) for r in out[p][K:])
    assert rows.tolist() == [(K, K - 3, n, 0), (3, 3, n - 1, 0), (0, 0, 0, 0)]
    # the counter of frame 1 cut to K - 1: the landmark stored there last loses its successor in pair 0 and its slot in pair 1
    last = int(np.nonzero(s[1] == K - 1)[0][0])
    b = L.rail(n, K, cap=K + 2)
    b["counts"][1] = K - 1
    out, rows = L.run(b)
    assert out[0][s[0][last]]["views"] == 1 and _zero(out[1][K - 1]) and rows["landmarks"].tolist() == [K, 0, 1]
    assert out[2][s[2][last]]["views"] == 2  # frames 2 and 3: the slot of pair 2 has no live predecessor


@pytest.mark.parametrize("status", [START, FEW, SPREAD, LOST])
def test_a_new_segment_cuts_the_chain_and_starts_another(status):
    """Frame 3 is START, RESTART_FEW, RESTART_SPREAD (origin 2) or LOST (pair 2 unmapped, frame 4 START with origin 3): the chains of
    segment 0 end with frame 2's view, and the next mapped pair starts every landmark again in its own origin's frame, where the
    origin's camera is the identity whatever its frame record holds."""
    n, K = 6, 5
    plan = [ORIGIN, START, CHAINED, status, START if status == LOST else CHAINED, CHAINED]
    b = L.rail(n, K, plan=plan)
    s = b["slots"]
    out, rows = L.run(b)
    first = 3 if status == LOST else 2  # the pair that starts again, also its origin
    assert b["frames"]["origin"].tolist() == [0, 0, 0, 3 if status == LOST else 2, first, first]
    want = [(K, K, 3, 0), (0, 0, 0, 0), (0, 0, 0, NO_ORIGIN), (K, K, 3, 3), (0, 0, 0, 3)] if status == LOST else \
           [(K, K, 3, 0), (0, 0, 0, 0), (K, K, 4, 2), (0, 0, 0, 2), (0, 0, 0, 2)]
    assert rows.tolist() == want and rows.tobytes() == _rows_from(out, [w[3] for w in want]).tobytes()
    for l in range(K):
        a, c = out[0][s[0][l]], out[first][s[first][l]]
        assert (a["views"], a["origin"], a["tail_index"]) == (3, 0, s[2][l]) and _near(a, b["cloud"][l])
        assert (c["views"], c["origin"], c["tail_index"], c["flags"]) == (n - first, first, s[n - 1][l], GOOD | PAR)
        assert _near(c, b["cloud"][l] - np.array([L.RAIL_BASE * first, 0, 0]))
    if status == LOST:
        assert all(_zero(r) for r in out[2])
    assert not np.array_equal(b["frames"]["t"][2], np.zeros(3))  # frame 2's own record belongs to segment 0


def test_two_slots_share_one_successor():
    """Landmarks 0 and 1 both match landmark 1's keypoint in frame 1: both are starts and share every later view; landmark 0's
    own slot in pair 1 has no predecessor and starts again."""
    n, K = 5, 6
    b = L.rail(n, K)
    s = b["slots"]
    b["matches"]["index"][0, s[0][0]] = s[1][1]
    out, rows, views = L.run(b, return_views=True)
    v0, v1 = views[0, s[0][0]], views[0, s[0][1]]
    assert v0[0] == (0, s[0][0]) and v0[1:] == v1[1:] and len(v0) == len(v1) == n
    assert rows.tolist()[:2] == [(K, K - 1, n, 0), (1, 1, n - 1, 0)]
    shared = out[0][s[0][0]]
    assert shared["views"] == n and shared["inliers"] < n and shared["flags"] == 0 and shared["z"] != 0  # solved, kept, not GOOD
    assert out[0][s[0][1]]["flags"] == GOOD | PAR and out[1][s[1][0]]["views"] == n - 1 and _zero(out[1][s[1][1]])


# ---- LM-4, LM-5, LM-6 --------------------------------------------------------------------------------------------------------
def test_min_views_and_the_reprojection_bound():
    n, K = 3, 4
    b = L.rail(n, K)
    s = b["slots"]
    b["points"]["flags"][1, s[1][0]] = 0  # landmark 0: two views
    two, _ = L.run(b)
    three, rows3 = L.run(b, min_views=3)
    r2, r3 = two[0][s[0][0]], three[0][s[0][0]]
    assert (r2["views"], r2["inliers"], r2["flags"]) == (2, 2, GOOD | PAR) and (r3["views"], r3["inliers"], r3["flags"]) == (2, 2, 0)
    assert (r2["x"], r2["y"], r2["z"]) == (r3["x"], r3["y"], r3["z"]) and r3["z"] > 0  # solved but not GOOD: kept
    assert rows3["good"].tolist() == [K - 1, 0] and three[0][s[0][1]]["flags"] == GOOD | PAR
    assert L.run(b, min_views=4)[1]["good"].tolist() == [0, 0]
    # a keypoint moved by 6 px: the point is pulled off the other rays; solved, kept, not GOOD; 1000 px accept it
    b = L.rail(n, K)
    b["corners"][1]["y"][s[1][1]] += 6
    out, _ = L.run(b)
    r = out[0][s[0][1]]
    assert r["views"] == 3 and r["inliers"] < 3 and r["flags"] == 0 and r["z"] > 0
    assert L.run(b, max_reproj_px=1000.0)[0][0][s[0][1]]["flags"] == GOOD | PAR
    assert L.run(b, max_reproj_px=1e-6)[1]["good"].sum() <= K  # nothing but exact reprojections
    # LM-5 at its edge, on one view of the identity camera: a keypoint exactly 2 px from the projection is in, one binary32 step
    # further is out; a NaN fails; a point behind the camera fails
    p = lmr.defaults(**L.RAIL)
    eye, zero = np.eye(3, dtype=F).ravel(), np.zeros(3, F)

    def inl(X, u, v=32.0, R=eye, t=zero, p=p):
        step = dict(rows=np.arange(1), g=0, k=np.zeros(1, np.int64), R=R, t=t, u=np.array([u], F), v=np.array([v], F))
        return int(lmr.check([step], np.array(X, F).reshape(3, 1), 1, p)[0])

    X = [1.0, 0.0, 8.0]  # projects to u = 64 / 8 + 32 = 40
    assert inl(X, 40.0) == 1 and inl(X, 42.0) == 1 and inl(X, 38.0) == 1 and inl(X, float(np.nextafter(F(42), F(43)))) == 0
    assert inl(X, 40.0, 34.0) == 1 and inl(X, 41.0, 34.0) == 0  # sqrt(5) px
    assert inl(X, 42.0, p=lmr.defaults(**L.RAIL, max_reproj_px=2.001)) == 1 and inl(X, 42.002, p=lmr.defaults(**L.RAIL, max_reproj_px=2.001)) == 0
    assert inl([1.0, 0.0, -8.0], 24.0) == 0 and inl([1.0, 0.0, 0.0], 40.0) == 0
    assert inl([np.nan, 0.0, 8.0], 40.0) == 0 and inl(X, 40.0, t=np.array([0, np.nan, 0], F)) == 0


def test_behind_the_camera_parallel_rays_and_poses_that_are_not_finite():
    n, K = 5, 6
    b = L.rail(n, K)
    s = b["slots"]
    u0 = int(b["corners"][0]["x"][s[0][0]])
    for f in range(n):  # landmark 0's keypoint moves the wrong way: the rays meet behind the cameras
        b["corners"][f]["x"][s[f][0]] = u0 + 4 * f
        b["corners"][f]["x"][s[f][1]], b["corners"][f]["y"][s[f][1]] = 32, 32  # landmark 1: the same ray in every view
    out, rows = L.run(b)
    behind, par = out[0][s[0][0]], out[0][s[0][1]]
    assert (behind["views"], behind["inliers"], behind["flags"]) == (n, 0, 0) and behind["z"] < 0
    # parallel rays through the principal point: A = diag(n, n, 0) exactly, det = 0: unsolved
    assert (par["views"], par["inliers"], par["flags"], par["origin"], par["tail_index"]) == (n, 0, 0, 0, s[n - 1][1])
    assert (par["x"], par["y"], par["z"]) == (0, 0, 0)
    assert rows[0].tolist() == (K, K - 2, n, 0)
    for bad in (np.nan, np.inf, -np.inf):
        for field, k in (("t", 0), ("r", 4), ("r", 2)):
            fr = b["frames"].copy()
            fr[field][3][k] = bad
            out, rows = L.run(b, frames=fr)
            for l in range(K):
                r = out[0][s[0][l]]
                assert (r["views"], r["inliers"], r["flags"], r["x"], r["y"], r["z"]) == (n, 0, 0, 0, 0, 0), (bad, field, k, r)
            assert rows[0].tolist() == (K, 0, n, 0) and np.isfinite(out["x"]).all()
    fr = b["frames"].copy()
    fr["t"][4] = (3e38, 3e38, 3e38)  # finite sums A, b overflows: X is not finite, the landmark unsolved
    out, _ = L.run(b, frames=fr)
    assert np.isfinite(out["x"]).all() and np.isfinite(out["z"]).all()


def test_extents_and_unmapped_pairs():
    """n_frames = 2 and 3 give the leading rows of shorter chains; a batch whose every frame is LOST has no landmark."""
    n, K = 5, 6
    b = L.rail(n, K)
    s = b["slots"]
    for m in (2, 3, 4):
        out, rows = L.run(b, n_frames=m)
        assert len(out) == m - 1 and rows.tolist() == [(K, K, m, 0)] + [(0, 0, 0, 0)] * (m - 2)
        assert all(out[0][s[0][l]]["tail_index"] == s[m - 1][l] for l in range(K))
    lost = L.rail(n, K, plan=[ORIGIN] + [LOST] * (n - 1))
    out, rows = L.run(lost)
    assert not out.view(np.uint8).any() and rows.tolist() == [(0, 0, 0, NO_ORIGIN)] * (n - 1)
    empty = L.rail(n, K)
    empty["counts"][:] = 0
    out, rows = L.run(empty)
    assert not out.view(np.uint8).any() and rows.tolist() == [(0, 0, 0, 0)] * (n - 1)


def test_the_point_is_the_least_squares_point():
    """A turning camera (localize_cases.views without noise, through the trajectory restatement): X of every GOOD landmark with
    three or more views against a float64 least-squares solution over the same views and frame records.  The bound is 64 binary32
    roundings times the condition number of the landmark's own A."""
    rng = np.random.default_rng(5)
    b = lc.views(rng, 6, 120, 160, W=640, H=480, focal=500.0)
    intr = lc.intrinsics(640, 480, 500.0)
    fr, out, rows, views = L.reference(b, return_views=True)
    assert fr["status"].tolist() == [ORIGIN, START] + [CHAINED] * 4
    cams = [(np.eye(3), np.zeros(3))] + [(fr["r"][f].reshape(3, 3), fr["t"][f]) for f in range(1, 6)]
    worst, n = 0.0, 0
    for (p, i), v in views.items():
        r = out[p][i]
        if len(v) < 3 or not r["flags"] & GOOD:
            continue
        obs = [(float(u[0]), float(w[0]), g) for g, k in v for u, w in [vr.level0(b["corners"][g][k:k + 1])]]
        X = L.least_squares(obs, cams, intr)
        A = np.zeros((3, 3))
        for u, w, g in obs:
            R = np.asarray(cams[g][0], np.float64)
            d = R.T @ np.array([(u - intr["cx"]) / 500.0, (w - intr["cy"]) / 500.0, 1.0])
            A += np.eye(3) - np.outer(d, d) / (d @ d)
        err = np.abs(np.array([r["x"], r["y"], r["z"]], np.float64) - X).max() / np.abs(X).max()
        bound = 64 * 2.0 ** -24 * np.linalg.cond(A)
        worst, n = max(worst, err / bound), n + 1
        assert err <= bound, (p, i, err, bound)
    print("least squares: %d landmarks, worst error / bound %.3f" % (n, worst))
    assert n > 60


# ---- accuracy on constructed paths -------------------------------------------------------------------------------------------
W, H, FOCAL = 640, 480, 500.0
INTR = dict(fx=FOCAL, fy=FOCAL, cx=(W - 1) / 2, cy=(H - 1) / 2)
PATHS, SEEDS = ("sideways", "forward"), (0, 1, 2)
# Measured on the binary32 restatement over the six scenes: the worst median relative error of the fused point
# of the planted landmarks with three or more views that are GOOD.  The test's bound is twice it.
FUSED_ERR = 0.0117
_CACHE = {}


def _run(path, seed):
    if (path, seed) not in _CACHE:
        steps = tr.path_steps(path)
        s = tr.path_scene(np.random.default_rng(seed), steps, W, H, FOCAL)
        V = len(s["corners"])
        m = [C.match_ref(s["desc"][f], s["desc"][f + 1]) for f in range(V - 1)]
        ep = [er.verify_pair(s["corners"][f], s["corners"][f + 1], m[f], W, H, f, inlier_px=2.0) for f in range(V - 1)]
        po = [pr.pose_pair(s["corners"][f], s["corners"][f + 1], m[f], ep[f][0], ep[f][1], **INTR) for f in range(V - 1)]
        counts = [len(c) for c in s["corners"]]
        cap = max(counts)
        fr, world = tr.trajectory(counts, m, [q[0] for q in po], [q[1] for q in po], cap)
        out, rows, views = lmr.landmarks(counts, s["corners"], m, [q[1] for q in po], fr, cap, return_views=True, **INTR)
        _CACHE[path, seed] = dict(scene=s, steps=steps, matches=m, poses=po, frames=fr, world=world, out=out, rows=rows, views=views)
    return _CACHE[path, seed]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("path", PATHS)
def test_fused_point_beats_the_two_view_point(path, seed):
    r = _run(path, seed)
    s, fr, out, views, world = r["scene"], r["frames"], r["out"], r["views"], r["world"]
    nl, ids = s["n_landmarks"], s["ids"]
    assert (fr["status"][2:] == CHAINED).all() and (fr["origin"] == 0).all()
    base = np.linalg.norm(r["steps"][0][1])  # the segment's unit: the baseline of pair 0, whose camera 0 is the origin
    fused, two, planted3, good3 = [], [], 0, 0
    for (p, i), v in views.items():
        lid = int(ids[p][i])
        if lid >= nl or len(v) < 3 or any(int(ids[g][k]) != lid for g, k in v):
            continue
        planted3 += 1
        rec = out[p][i]
        if not rec["flags"] & GOOD:
            continue
        good3 += 1
        truth = s["cloud"][lid] / base
        fused.append(np.linalg.norm(np.array([rec["x"], rec["y"], rec["z"]], np.float64) - truth) / np.linalg.norm(truth))
        w = world[p][i]
        assert w["flags"] & GOOD
        two.append(np.linalg.norm(np.array([w["x"], w["y"], w["z"]], np.float64) - truth) / np.linalg.norm(truth))
    # the caps: the comparison cannot pass by dropping cases
    live = {(p, i) for p in range(len(out)) for i in np.nonzero((r["poses"][p][1]["flags"][:len(ids[p])] & GOOD) != 0)[0] if ids[p][i] < nl}
    in_a_view = {(g, k) for v in views.values() for g, k in v}
    assert live <= in_a_view
    seen = {int(ids[p][i]) for p, i in live}
    starts = sum(1 for (p, i) in views if ids[p][i] < nl)
    shared = sum(1 for p in range(len(out) - 1) for j, c in zip(*np.unique(r_next(r, p), return_counts=True)) if c > 1)
    fm, tm = float(np.median(fused)), float(np.median(two))
    print("%s %d: %d planted landmarks with >= 3 views, %d GOOD (%.1f %%); median relative error fused %.4f, two-view %.4f, ratio %.2f; "
          "%d starts on %d planted landmarks seen; %d successors shared by several live slots; longest %d" %
          (path, seed, planted3, good3, 100.0 * good3 / planted3, fm, tm, fm / tm, starts, len(seen), shared, int(r["rows"]["longest"].max())))
    assert good3 >= 0.85 * planted3
    assert abs(starts - len(seen)) <= 0.02 * len(seen)
    assert fm < tm
    assert fm <= 2 * FUSED_ERR


def r_next(r, p):
    """The successors of pair p's live slots whose link continues (LM-3): a value that occurs twice is a shared successor."""
    po, fr = r["poses"], r["frames"]
    n = len(po) + 1
    nq = [len(c) for c in r["scene"]["corners"]]
    mapped, origin = lmr.segments(fr, n)
    live = lmr.live_flags(nq, [q[1] for q in po], mapped, max(nq))
    if not lmr.continues(p, n, mapped, origin):
        return np.zeros(0, np.int64)
    i = np.nonzero(live[p])[0]
    j = r["matches"][p]["index"][i].astype(np.int64)
    j = j[j < nq[p + 1]]
    return j[live[p + 1][j] != 0]
