"""Hand-built inputs of the landmark stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_landmarks_consecutive reads the raw counters, the stored records, the matcher's records, the flags of the
pairs' points and the frame records of the trajectory stage.  `rail` builds all of them directly for a camera that slides along x
without turning, with a focal length of 64 and depths of 8 and 16, so that every projection is an integer pixel and every ray meets
its landmark exactly: a test then changes one flag, index, counter, keypoint or frame record and sees what that alone does.  The
batches of tests/localize_cases.py (`views`, `join`) serve the cases that need a turning camera, and the GPU tests; `reference`
runs the trajectory restatement and then the landmark restatement on such a batch.

`cases` holds the constructions that pin LM-2..LM-6 as data -- the calls of each case and the outcome its construction implies --
so that tests/test_landmark_cases_ref.py runs them on the restatement and tests/test_gpu_landmark_cases.py on the device, where
`inject_frames` writes the frame records (orb_debug_frame_buffer) that only a trajectory call could write before.
"""
import numpy as np

import constructed as C
import landmark_ref as lmr
import localize_cases as lc
import trajectory_cases as tc
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
U = np.uint32
NONE = orb.ORB_MATCH_NONE
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = tc.CHAINED, tc.START, tc.FEW, tc.SPREAD, tc.LOST, tc.ORIGIN
RAIL = dict(fx=64.0, fy=64.0, cx=32.0, cy=32.0)
RAIL_BASE = 0.5  # the rail camera's step along x


def frame_records(plan, base=RAIL_BASE):
    """The OrbFramePose records of a camera at x = base * f without rotation, under a plan of statuses (plan[0] is ORIGIN): LOST is
    the identity with its own origin and scale 0, START and the two RESTARTs begin a segment at the frame before, CHAINED goes on."""
    fr = np.zeros(len(plan), orb.FRAME_POSE_DTYPE)
    origin = 0
    for f, st in enumerate(plan):
        if st == LOST:
            origin = f
        elif st in (START, FEW, SPREAD):
            origin = f - 1
        lost = st in (LOST, ORIGIN)
        fr[f]["r"] = tc.IDENTITY
        fr[f]["t"] = (0, 0, 0) if lost else (-base * (f - origin), 0, 0)
        fr[f]["scale"] = 0 if lost else 1
        fr[f]["origin"], fr[f]["status"] = origin, st
    return fr


def rail(n_frames, K, cap=None, plan=None, seed=0, octaves=0, v_hi=60):
    """K landmarks seen in all n_frames (at most 6) views of the rail camera.  Landmark l sits at slot slots[f][l] of frame f (a
    permutation per frame), matched to its slot in the next frame, GOOD | PARALLAX in every pair; its keypoint in frame f is
    (u0 - shift * f, v0) with a shift of 4 px (depth 8) or 2 px (depth 16), v0 below v_hi.  With `octaves` (1 or 2) every landmark
    has an octave of its own, 0 .. octaves (at most 1 at depth 16; landmarks 0, 1, 2 have 2, 1, 0), the same in all its views: the
    stored x, y are those of that level, its level-0 keypoint (orb_corner_level0_xy) is 2^o x + (2^o - 1) / 2 and still moves by
    the whole shift, and `cloud` is computed from the level-0 keypoint, so every ray still meets its landmark exactly.  Returns a
    batch dict as localize_cases.views does, with `frames` (the records under `plan`, default ORIGIN, START, CHAINED ...), `slots`,
    `cloud` (K, 3) in camera 0's frame, `octave` (K,)."""
    assert 2 <= n_frames <= 6 and 0 <= octaves <= 2
    rng = np.random.default_rng(seed)
    cap = K if cap is None else cap
    plan = [ORIGIN, START] + [CHAINED] * (n_frames - 2) if plan is None else plan
    u0, v0 = rng.integers(24, 60, K), rng.integers(4, v_hi, K)
    z = np.where(rng.random(K) < 0.5, 8.0, 16.0)
    z[:2] = 8.0, 16.0
    shift = (64.0 * RAIL_BASE / z).astype(np.int64)
    slots = [rng.permutation(K) for _ in range(n_frames)]
    o = np.zeros(K, np.int64)
    if octaves:  # a generator of its own: the draws above are those of octaves = 0
        o = np.minimum(np.random.default_rng(seed + 7919).integers(0, octaves + 1, K), np.where(z == 8.0, 2, 1))
        o[:3] = np.minimum((2, 1, 0), octaves)[:K]
    x0, y0, step = u0 >> o, v0 >> o, shift >> o  # at the landmark's own level
    half = ((1 << o) - 1) / 2.0
    ul, vl = x0 * (1 << o) + half, y0 * (1 << o) + half  # level 0, frame 0
    cloud = np.stack([(ul - 32.0) * z / 64.0, (vl - 32.0) * z / 64.0, z], 1)
    corners = []
    for f in range(n_frames):
        c = C.corners(np.zeros(cap, np.int64), np.zeros(cap, np.int64), 0)
        c["x"][slots[f]], c["y"][slots[f]], c["octave"][slots[f]] = x0 - step * f, y0, o
        corners.append(c)
    M = np.zeros((n_frames - 1, cap), orb.MATCH_DTYPE)
    M["index"], M["distance"], M["second"] = NONE, 0xFFFF, 0xFFFF
    P = np.zeros((n_frames - 1, cap), orb.POINT_DTYPE)
    for f in range(n_frames - 1):
        M["index"][f, slots[f]] = slots[f + 1]
        P["x"][f, slots[f]], P["y"][f, slots[f]], P["z"][f, slots[f]] = cloud[:, 0] - RAIL_BASE * f, cloud[:, 1], cloud[:, 2]
        P["flags"][f, slots[f]] = GOOD | PAR
    return dict(counts=np.full(n_frames, K, U), corners=corners, matches=M, points=P, cap=cap, n=n_frames, frames=frame_records(plan),
                slots=slots, cloud=cloud, octave=o)


def run(b, n_frames=None, frames=None, return_views=False, intr=None, **params):
    """landmark_ref.landmarks on a batch's arrays (the counts clipped to the capacity) under the frame records `frames` (default:
    the batch's own `frames`)."""
    n = b["n"] if n_frames is None else n_frames
    nq = lc.stored(b)
    fr = b["frames"] if frames is None else frames
    intr = RAIL if intr is None else intr
    return lmr.landmarks(nq[:n], [c[:nq[f]] for f, c in enumerate(b["corners"][:n])], [b["matches"][f][:nq[f]] for f in range(n - 1)],
                         list(b["points"][:n - 1]), fr[:n], b["cap"], n_frames=n, return_views=return_views, **{**intr, **params})


def reference(b, n_frames=None, traj=None, return_views=False, **params):
    """A localize_cases batch through trajectory_ref.trajectory (parameters `traj`) and then landmark_ref.landmarks.  Returns the
    frame records in front of what `run` returns."""
    n = b["n"] if n_frames is None else n_frames
    fr = tc.reference(b, n, **(traj or {}))[0]
    return (fr,) + tuple(run(b, n, frames=fr, return_views=return_views, intr=lc.intrinsics(b["W"], b["H"], b["focal"]), **params))


def slow_steps(n, length=0.004):
    """n small camera steps for a long chain inside a 64 x 48 frame: a twentieth of a degree of yaw, sideways, lengths that vary by
    a factor of two."""
    return [(tr.rot("y", -0.05) @ tr.rot("x", 0.01), np.array([-length * (1.0 + 0.5 * np.sin(k)), 0.1 * length, 0.2 * length])) for k in range(n)]


def least_squares(views, cams, intr):
    """The point nearest to the rays of `views` [(u, v, camera index)] in float64, by numpy.linalg.lstsq on the stacked
    (I - w w^T / w.w) X = (I - w w^T / w.w) c; cams[k] = (R, t) with X_k = R X + t."""
    rows, rhs = [], []
    for u, v, k in views:
        R, t = (np.asarray(a, np.float64) for a in cams[k])
        w = R.T @ np.array([(u - intr["cx"]) / intr["fx"], (v - intr["cy"]) / intr["fy"], 1.0])
        c = -R.T @ t
        Q = np.eye(3) - np.outer(w, w) / (w @ w)
        rows.append(Q)
        rhs.append(Q @ c)
    return np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]


# ---- the GPU tests' batches (64 x 48 frames) ---------------------------------------------------------------------------------
def status_batch(cap):
    """Twelve frames: a five-view path with wrong, far and lost matches and points without flags; a plane (three views); a cloud
    whose matches are all wrong (three views); an empty frame.  The pairs between the runs are not OK (LOST frames, a new origin
    behind each) and carry the matches of unrelated scenes."""
    rng = np.random.default_rng(2027)
    runs = [lc.views(rng, 5, 500, cap, wrong=0.1, far=0.05, lost=0.05, bad_points=0.05, noise=0.002),
            lc.views(rng, 3, 200, cap, shape="plane"), lc.views(rng, 3, 150, cap, wrong=1.0), lc.views(rng, 1, 0, cap)]
    return lc.join(runs, bridge=True)


FULL_TRAJ = dict(min_shared=4)


def full_batch(cap=64, n=6, extra=11):
    """Every frame stores `cap` of 90 landmarks and its raw counter lies `extra` above the capacity."""
    return lc.views(np.random.default_rng(64), n, 90, cap, noise=0.001, extra=extra, wrong=0.05)


LONG_FRAMES, LONG_CAP = 70, 8
LONG_TRAJ = dict(min_shared=4)


def long_batch():
    """Seventy frames at capacity 8: eight landmarks that stay in view along 69 small steps, so chains of 70 views that cross any
    64-frame staging of the frame records."""
    return lc.views(np.random.default_rng(7), LONG_FRAMES, LONG_CAP, LONG_CAP, steps=slow_steps(LONG_FRAMES - 1))


RESTART_TRAJ = dict(scale_tolerance=2e-4, consistent_permille=280)


def restart_batch(cap=300):
    """Eight views of one cloud with noisy points: under RESTART_TRAJ some joints are RESTART_SPREAD and some hold, under a
    min_shared above the capacity every joint is RESTART_FEW -- chains cut and started again in the same frame."""
    return lc.views(np.random.default_rng(11), 8, 260, cap, noise=0.0004, wrong=0.05)


# ---- the hand-built cases, as data (tests/test_landmark_cases_ref.py, tests/test_gpu_landmark_cases.py) ---------------------------
# The GPU test holds 64 x 48 programs; the stage reads no image, but the rail cases keep their keypoints inside such a frame all the
# same: v0 below 40 (a case moves a keypoint 6 px down), u below 60.
V_HI = 40
SMALL = 8  # the capacity of the cases that need no particular one
CROSS = dict(fx=16.0, fy=16.0, cx=32.0, cy=32.0)
NO_ORIGIN = orb.ORB_LANDMARK_NO_ORIGIN


def inject_frames(prog, frames, first=0):
    """Overwrites the frame records first .. of the last trajectory call (orb_debug_frame_buffer) with FRAME_POSE_DTYPE rows: what
    orb_trajectory_read, the landmark stage and the bridge stage read.  Ordered as trajectory_cases.inject_pose: everything queued is
    finished before the copy starts, and the copy before this returns.  No stage's freshness changes."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    B = cfg.max_batch
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    a = np.ascontiguousarray(frames, dtype=orb.FRAME_POSE_DTYPE)
    n = len(a)
    assert a.ndim == 1 and first + n <= B, (a.shape, first, B)
    node.as_tensor(prog.debug_frame_buffer(), (B, 20), "<i4", dev)[first:first + n].copy_(torch.from_numpy(a.view(np.int32).reshape(n, 20)))
    torch.cuda.synchronize(dev)


def copy_batch(b):
    """A batch whose arrays can be edited without touching b's."""
    out = dict(b)
    out.update(counts=b["counts"].copy(), corners=[c.copy() for c in b["corners"]], matches=b["matches"].copy(), points=b["points"].copy(),
               frames=b["frames"].copy())
    return out


def cross(cap=SMALL):
    """Three views whose every operation of LM-4 and LM-5 is exact, under the intrinsics CROSS: the landmark (0, 0, 8) seen by the
    origin's camera on its axis and by cameras at x = +8 and x = -8 at 45 degrees (keypoints (32, 32), (16, 32), (48, 32)), so every
    n is 1 or 2, A = diag(2, 3, 1), b = (0, 0, 8), det = 6, X = (0, 0, 8) and every residual of LM-5 is 0 exactly."""
    b = rail(3, 2, cap=cap)
    slot = (3, 5, 1)
    xs = (32, 16, 48)
    for f in range(3):
        b["corners"][f][:] = 0
        b["corners"][f]["x"][slot[f]], b["corners"][f]["y"][slot[f]] = xs[f], 32
    b["matches"]["index"][:], b["points"][:] = NONE, 0
    for f in range(2):
        b["matches"]["index"][f, slot[f]] = slot[f + 1]
        b["points"][f, slot[f]] = (0.0, 0.0, 8.0, GOOD | PAR)
    b["counts"][:] = 6
    b["frames"]["t"][1], b["frames"]["t"][2] = (-8.0, 0.0, 0.0), (8.0, 0.0, 0.0)
    b.update(slots=[np.array([s]) for s in slot], cloud=np.array([[0.0, 0.0, 8.0]]))
    return b


def smallest_good(b, pair, slot, lo=2.0, hi=1000.0):
    """(below, at): the smallest binary32 max_reproj_px at which the restatement makes the landmark (pair, slot) of b GOOD, and the
    binary32 value just below it, by bisection over the bit patterns between lo (not GOOD) and hi (GOOD).  r2 = r * r and the
    comparison of LM-5 do not decrease with r, so there is one such step."""
    def good(bits):
        return bool(run(b, max_reproj_px=float(tc.floats([bits])[0]))[0][pair][slot]["flags"] & GOOD)

    lo, hi = int(tc.bits(lo)), int(tc.bits(hi))
    assert not good(lo) and good(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if good(mid) else (mid, hi)
    return float(tc.floats([lo])[0]), float(tc.floats([hi])[0])


def raw_points(b, frames, pair, intr=None):
    """LM-4 of pair `pair`'s starts before anything is masked, from the restatement's own steps: (starts (m,), X (3, m) as the division
    leaves it, whether all of b is finite (m,)).  The cases use it to state what their records were built to reach."""
    n, cap = b["n"], b["cap"]
    nq = lc.stored(b)
    p = lmr.defaults(**(RAIL if intr is None else intr))
    mapped, origin = lmr.segments(frames, n)
    live = lmr.live_flags(nq, list(b["points"]), mapped, cap)
    pred = lmr.predecessors(nq, [b["matches"][f][:nq[f]] for f in range(n - 1)], live, mapped, origin, n, cap)
    starts = np.nonzero((live[pair] != 0) & (pred[pair] == 0))[0]
    steps, _ = lmr.walk(pair, starts, nq, [c[:nq[f]] for f, c in enumerate(b["corners"])], [b["matches"][f][:nq[f]] for f in range(n - 1)], live,
                        mapped, origin, frames, n)
    A, rhs = lmr.accumulate(steps, len(starts), p)
    return starts, lmr.solve(A, rhs)[0], np.isfinite(rhs).all(0)


def call(b, frames=None, n_frames=None, intr=None, **params):
    """One landmarks call of a case: the batch, the frame records to call under (default: the batch's own), the extent (default:
    the whole batch), the intrinsics (default: RAIL) and the other parameters."""
    return dict(batch=b, frames=b["frames"] if frames is None else frames, n_frames=b["n"] if n_frames is None else n_frames,
                intr=RAIL if intr is None else intr, params=params)


def run_call(c):
    """A call of a case on the restatement: (LANDMARK_DTYPE (n_frames - 1, cap), LANDMARK_ROW_DTYPE (n_frames - 1,))."""
    return run(c["batch"], n_frames=c["n_frames"], frames=c["frames"], intr=c["intr"], **c["params"])


def is_zero(rec):
    return not np.asarray(rec).tobytes().strip(b"\0")


def near(rec, X, tol=1e-4):
    got = np.array([rec["x"], rec["y"], rec["z"]], np.float64)
    return np.abs(got - X).max() <= tol * np.abs(X).max()


def rows_from(out, origin):
    """LM-6's row of each pair, counted from its records."""
    rows = np.zeros(len(out), orb.LANDMARK_ROW_DTYPE)
    for p, o in enumerate(out):
        s = o["views"] != 0
        rows[p] = (int(s.sum()), int(((o["flags"] & GOOD) != 0).sum()), int(o["views"].max(initial=0)), origin[p])
    return rows


def fields(r, *names):
    return tuple(r[k].item() for k in names)


def cases():
    """The hand-built cases of LM-2..LM-6: a list of dict(name, calls, expect).  `calls` are the landmarks calls of the case, in
    order, on one program (`call`): one batch under several parameter sets, extents or frame records, or several batches in turn.
    `expect(results)` asserts the outcome the construction implies on results[k] = (records (n_frames - 1, cap), rows (n_frames - 1,))
    of call k -- the restatement's (tests/test_landmark_cases_ref.py) or the device's (tests/test_gpu_landmark_cases.py).  A case's
    capacity is that of its batches: SMALL, or 64, 256, 257 and 1100 for the block edges of k_lm_fuse."""
    out = []

    def add(name, calls, expect):
        assert len({c["batch"]["cap"] for c in calls}) == 1
        out.append(dict(name=name, calls=calls, expect=expect, cap=calls[0]["batch"]["cap"]))

    # ---- LM-3: chains ----
    n, K = 5, 7
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]

    def every_slot(res, b=b, s=s, n=n, K=K):
        o, rows = res[0]
        assert rows.tolist() == [(K, K, n, 0), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
        for l in range(K):
            r = o[0][s[0][l]]
            assert fields(r, "views", "inliers", "flags", "origin", "tail_index") == (n, n, GOOD | PAR, 0, s[n - 1][l]) and near(r, b["cloud"][l])
        assert is_zero(o[1:]) and is_zero(o[0][K:])

    add("chains of every live slot", [call(b)], every_slot)
    # landmark 0 is not GOOD in pair 1: a chain of one live slot (two views), then one of two (three views) from pair 2
    # landmark 1 is not GOOD in pair 2: a chain of two live slots (three views), then one of one from pair 3
    b1 = copy_batch(b)
    b1["points"]["flags"][1, s[1][0]] = PAR
    b1["points"]["flags"][2, s[2][1]] = 0

    def one_and_two(res, b=b1, s=s, n=n, K=K):
        o, rows = res[0]
        a0, a2, b0, b3 = o[0][s[0][0]], o[2][s[2][0]], o[0][s[0][1]], o[3][s[3][1]]
        assert fields(a0, "views", "tail_index") + fields(a2, "views", "tail_index") == (2, s[1][0], 3, s[4][0])
        assert fields(b0, "views", "tail_index") + fields(b3, "views", "tail_index") == (3, s[2][1], 2, s[4][1])
        assert is_zero(o[1][s[1][0]]) and is_zero(o[2][s[2][1]])
        # a start at p != o(p): camera p's pose is its frame record, and the point is still in the origin's frame
        for r, l in ((a0, 0), (a2, 0), (b0, 1), (b3, 1)):
            assert r["flags"] == GOOD | PAR and r["origin"] == 0 and r["inliers"] == r["views"] and near(r, b["cloud"][l]), (r, l)
        assert rows.tolist() == [(K, K, n, 0), (0, 0, 0, 0), (1, 1, 3, 0), (1, 1, 2, 0)]
        assert rows.tobytes() == rows_from(o, [0] * 4).tobytes()

    add("chains of one and two live slots, starts at p != o(p)", [call(b1)], one_and_two)
    b2 = copy_batch(b1)
    b2["points"]["flags"][:, :] &= ~U(PAR)
    b2["points"]["flags"][3, s[3][2]] |= PAR

    def parallax(res, s=s):
        o, _ = res[0]
        assert o[0][s[0][2]]["flags"] == GOOD | PAR and o[0][s[0][3]]["flags"] == GOOD and o[0][s[0][0]]["flags"] == GOOD

    add("PARALLAX from one live slot of the chain", [call(b2)], parallax)
    # stale predecessor bytes: the full batch, a mid-chain point without flags (its successor becomes a start), the full batch again
    b3 = copy_batch(b)
    b3["points"]["flags"][1, s[1][2]] = 0

    def stale_pred(res, s=s, n=n, K=K):
        (o0, r0), (o1, r1), (o2, r2) = res
        assert o2.tobytes() == o0.tobytes() and r2.tobytes() == r0.tobytes()
        assert r0.tolist() == [(K, K, n, 0)] + [(0, 0, 0, 0)] * 3 and r1.tolist() == [(K, K, n, 0), (0, 0, 0, 0), (1, 1, 3, 0), (0, 0, 0, 0)]
        assert fields(o1[0][s[0][2]], "views", "tail_index") == (2, s[1][2]) and fields(o1[2][s[2][2]], "views", "tail_index") == (3, s[4][2])
        assert is_zero(o0[2][s[2][2]])

    add("stale predecessor bytes", [call(b), call(b3), call(copy_batch(b))], stale_pred)

    # ---- LM-3: no successor ----
    n, K = 4, 6
    b = rail(n, K, cap=K + 2, v_hi=V_HI)
    assert b["cap"] == SMALL
    s = b["slots"]
    stale = copy_batch(b)
    for f in range(n - 1):  # stale records above the counters: GOOD points with matches among themselves
        stale["points"][f, K:] = (1.0, 1.0, 8.0, GOOD | PAR)
        stale["matches"]["index"][f, K:] = K, K + 1
    b1 = copy_batch(stale)
    b1["matches"]["index"][0, s[0][0]] = NONE
    b1["matches"]["index"][0, s[0][1]] = K
    b1["matches"]["index"][0, s[0][2]] = K + 1

    def no_successor(res, b=b1, s=s, n=n, K=K):
        o, rows = res[0]
        for l in (0, 1, 2):
            r, nxt = o[0][s[0][l]], o[1][s[1][l]]
            assert fields(r, "views", "inliers", "flags", "tail_index", "origin", "x", "y", "z") == (1, 0, 0, s[0][l], 0, 0, 0, 0)
            assert fields(nxt, "views", "flags", "tail_index") == (n - 1, GOOD | PAR, s[n - 1][l]) and near(nxt, b["cloud"][l])
        assert is_zero(o[:, K:])
        assert rows.tolist() == [(K, K - 3, n, 0), (3, 3, n - 1, 0), (0, 0, 0, 0)]

    add("no successor: NONE, n_q, n_q + 1; stale GOOD points above the counters", [call(b1)], no_successor)
    # the counter of frame 1 cut to K - 1: the landmark stored there last loses its successor in pair 0 and its slot in pair 1
    last = int(np.nonzero(s[1] == K - 1)[0][0])
    b2 = copy_batch(stale)
    b2["counts"][1] = K - 1

    def counter_cut(res, s=s, K=K, last=last):
        o, rows = res[0]
        assert o[0][s[0][last]]["views"] == 1 and is_zero(o[1][K - 1]) and rows["landmarks"].tolist() == [K, 0, 1]
        assert o[2][s[2][last]]["views"] == 2  # frames 2 and 3: the slot of pair 2 has no live predecessor
        assert is_zero(o[:, K:])

    add("a counter cut below a stored successor", [call(b2)], counter_cut)
    # every counter at the capacity: the index n_q is the capacity itself, the first slot of the next row
    n, K = 4, SMALL
    b = rail(n, K, v_hi=V_HI)
    s = b["slots"]
    b["matches"]["index"][0, s[0][0]] = K

    def at_capacity(res, b=b, s=s, n=n, K=K):
        o, rows = res[0]
        assert fields(o[0][s[0][0]], "views", "inliers", "flags", "tail_index", "x", "y", "z") == (1, 0, 0, s[0][0], 0, 0, 0)
        assert fields(o[1][s[1][0]], "views", "flags", "tail_index") == (n - 1, GOOD | PAR, s[n - 1][0]) and near(o[1][s[1][0]], b["cloud"][0])
        assert rows.tolist() == [(K, K - 1, n, 0), (1, 1, n - 1, 0), (0, 0, 0, 0)]

    add("the index n_q where n_q is the capacity", [call(b)], at_capacity)

    # ---- LM-2, LM-3: a new segment ----
    n, K = 6, 5
    for status, label in ((START, "START"), (FEW, "RESTART_FEW"), (SPREAD, "RESTART_SPREAD"), (LOST, "LOST")):
        plan = [ORIGIN, START, CHAINED, status, START if status == LOST else CHAINED, CHAINED]
        b = rail(n, K, cap=SMALL, plan=plan, v_hi=V_HI)
        first = 3 if status == LOST else 2  # the pair that starts again, also its origin
        # LM-2: the origin's own record is never read: frame 0's, and frame 3's when it is LOST (frame 2's, the origin of the
        # segment that a START or RESTART begins, is segment 0's record of its last view)
        nan = b["frames"].copy()
        for f in ((0, 3) if status == LOST else (0,)):
            nan["r"][f], nan["t"][f], nan["scale"][f] = np.nan, np.nan, np.nan

        def segment(res, b=b, K=K, n=n, status=status, first=first):
            o, rows = res[0]
            s = b["slots"]
            assert b["frames"]["origin"].tolist() == [0, 0, 0, 3 if status == LOST else 2, first, first]
            want = ([(K, K, 3, 0), (0, 0, 0, 0), (0, 0, 0, NO_ORIGIN), (K, K, 3, 3), (0, 0, 0, 3)] if status == LOST else
                    [(K, K, 3, 0), (0, 0, 0, 0), (K, K, 4, 2), (0, 0, 0, 2), (0, 0, 0, 2)])
            assert rows.tolist() == want and rows.tobytes() == rows_from(o, [w[3] for w in want]).tobytes()
            for l in range(K):
                a, c = o[0][s[0][l]], o[first][s[first][l]]
                assert fields(a, "views", "origin", "tail_index") == (3, 0, s[2][l]) and near(a, b["cloud"][l])
                assert fields(c, "views", "origin", "tail_index", "flags") == (n - first, first, s[n - 1][l], GOOD | PAR)
                assert near(c, b["cloud"][l] - np.array([RAIL_BASE * first, 0, 0]))
            if status == LOST:
                assert is_zero(o[2])
            else:
                assert not np.array_equal(b["frames"]["t"][2], np.zeros(3))  # frame 2's own record belongs to segment 0
            assert res[1][0].tobytes() == o.tobytes() and res[1][1].tobytes() == rows.tobytes()  # NaN where LM-2 says identity

        add("frame 3 %s; the origins' records NaN" % label, [call(b), call(b, frames=nan)], segment)

    # ---- LM-3: a shared successor ----
    n, K = 5, 6
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]
    b["matches"]["index"][0, s[0][0]] = s[1][1]

    def shared(res, s=s, n=n, K=K):
        o, rows = res[0]
        assert rows.tolist()[:2] == [(K, K - 1, n, 0), (1, 1, n - 1, 0)]
        sh = o[0][s[0][0]]
        assert sh["views"] == n and sh["inliers"] < n and sh["flags"] == 0 and sh["z"] != 0  # solved, kept, not GOOD
        assert sh["tail_index"] == s[n - 1][1] == o[0][s[0][1]]["tail_index"]  # the later views are landmark 1's
        assert o[0][s[0][1]]["flags"] == GOOD | PAR and o[1][s[1][0]]["views"] == n - 1 and is_zero(o[1][s[1][1]])

    add("two slots share one successor", [call(b)], shared)

    # ---- LM-4, LM-5, LM-6 ----
    n, K = 3, 4
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]
    b["points"]["flags"][1, s[1][0]] = 0  # landmark 0: two views

    def min_views(res, s=s, K=K):
        (two, _), (three, rows3), (_, rows4) = res
        r2, r3 = two[0][s[0][0]], three[0][s[0][0]]
        assert fields(r2, "views", "inliers", "flags") == (2, 2, GOOD | PAR) and fields(r3, "views", "inliers", "flags") == (2, 2, 0)
        assert fields(r2, "x", "y", "z") == fields(r3, "x", "y", "z") and r3["z"] > 0  # solved but not GOOD: kept
        assert rows3["good"].tolist() == [K - 1, 0] and three[0][s[0][1]]["flags"] == GOOD | PAR
        assert rows4["good"].tolist() == [0, 0] and rows4["landmarks"].tolist() == [K, 0]

    add("min_views 2, 3, 4", [call(b), call(b, min_views=3), call(b, min_views=4)], min_views)
    # a keypoint moved by 6 px: the point is pulled off the other rays; solved, kept, not GOOD; 1000 px accept it
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]
    b["corners"][1]["y"][s[1][1]] += 6
    below, at = smallest_good(b, 0, s[0][1])

    def moved(res, s=s, K=K):
        (o, rows), (wide, wrows), (tiny, trows) = res
        r = o[0][s[0][1]]
        assert r["views"] == 3 and r["inliers"] < 3 and r["flags"] == 0 and r["z"] > 0 and rows["good"].tolist() == [K - 1, 0]
        assert wide[0][s[0][1]]["flags"] == GOOD | PAR and wrows["good"].tolist() == [K, 0]
        t = tiny[0][s[0][1]]
        assert t["flags"] == 0 and fields(t, "x", "y", "z") == fields(r, "x", "y", "z") and trows["landmarks"].tolist() == [K, 0]

    add("a keypoint moved 6 px: 2 px, 1000 px, 1e-6 px", [call(b), call(b, max_reproj_px=1000.0), call(b, max_reproj_px=1e-6)], moved)

    def last_bit(res, s=s, K=K):
        (lo, lrows), (hi, hrows) = res
        assert fields(hi[0][s[0][1]], "views", "inliers", "flags") == (3, 3, GOOD | PAR) and hrows["good"].tolist() == [K, 0]
        assert lo[0][s[0][1]]["flags"] == 0 and lo[0][s[0][1]]["inliers"] < 3 and lrows["good"].tolist() == [K - 1, 0]
        assert fields(lo[0][s[0][1]], "x", "y", "z") == fields(hi[0][s[0][1]], "x", "y", "z")

    assert 2.0 < below < at < 1000.0 and tc.bits(at) - tc.bits(below) == 1
    add("LM-5 at its last bit: max_reproj_px %r and %r" % (below, at), [call(b, max_reproj_px=below), call(b, max_reproj_px=at)], last_bit)
    # every operation exact and every residual 0: r2 = (1e-30)^2 underflows to 0 and `0 <= 0` holds
    b = cross()

    def exact(res, b=b):
        for o, rows in res:
            r = o[0][b["slots"][0][0]]
            assert fields(r, "x", "y", "z", "flags", "views", "inliers", "origin", "tail_index") == (0.0, 0.0, 8.0, GOOD | PAR, 3, 3, 0, b["slots"][2][0])
            assert rows.tolist() == [(1, 1, 3, 0), (0, 0, 0, 0)]

    add("exact rays: residual 0 against r2 = 0", [call(b, intr=CROSS), call(b, intr=CROSS, max_reproj_px=1e-30)], exact)

    # ---- behind the camera, det == 0, records that are not finite ----
    n, K = 5, 6
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]
    u0 = min(int(b["corners"][0]["x"][s[0][0]]), 40)  # the last view stays inside a 64-pixel row
    for f in range(n):  # landmark 0's keypoint moves the wrong way: the rays meet behind the cameras
        b["corners"][f]["x"][s[f][0]] = u0 + 4 * f
        b["corners"][f]["x"][s[f][1]], b["corners"][f]["y"][s[f][1]] = 32, 32  # landmark 1: the same ray in every view

    def behind(res, s=s, n=n, K=K):
        o, rows = res[0]
        back, par = o[0][s[0][0]], o[0][s[0][1]]
        assert fields(back, "views", "inliers", "flags") == (n, 0, 0) and back["z"] < 0
        # parallel rays through the principal point: A = diag(n, n, 0) exactly, det = 0: unsolved
        assert fields(par, "views", "inliers", "flags", "origin", "tail_index", "x", "y", "z") == (n, 0, 0, 0, s[n - 1][1], 0, 0, 0)
        assert rows[0].tolist() == (K, K - 2, n, 0)

    add("rays that meet behind the cameras; parallel rays, det == 0", [call(b)], behind)
    calls, labels = [], []
    for bad in (np.nan, np.inf, -np.inf):
        for field, k in (("t", 0), ("r", 4), ("r", 2)):
            fr = b["frames"].copy()
            fr[field][3][k] = bad
            calls.append(call(b, frames=fr))
            labels.append((bad, field, k))

    def not_finite(res, s=s, n=n, K=K, labels=labels):
        assert len(res) == 9
        for (o, rows), label in zip(res, labels):
            for l in range(K):
                assert fields(o[0][s[0][l]], "views", "inliers", "flags", "x", "y", "z") == (n, 0, 0, 0, 0, 0), (label, l)
            assert rows[0].tolist() == (K, 0, n, 0) and is_zero(o[1:]), label

    add("NaN, +inf, -inf in t[0], r[4], r[2] of frame 3", calls, not_finite)
    fr = b["frames"].copy()
    fr["t"][4] = (3e38, 3e38, 3e38)  # finite sums A, b overflows: X is not finite, the landmark unsolved

    def huge(res, n=n, K=K):
        o, rows = res[0]
        assert all(np.isfinite(o[k]).all() for k in "xyz") and fields(rows[0], "landmarks", "longest") == (K, n)

    add("t = 3e38 in frame 4", [call(b, frames=fr)], huge)
    # Cameras 1 .. 4 turned by a cyclic permutation P of the axes (a rotation; the records hold R = P and the rail's t, so the map is
    # P^T times the rail's): the chains start at pair 1, where no view is the origin's, and the depth, the coordinate that the nearly
    # parallel rays determine worst, is X0, X1 or X2.  1e38 added to frame 3's t leaves A and b finite and takes that one coordinate
    # of X, and no other, past FLT_MAX in most landmarks: each isfinite(X_r) of LM-4 decides alone.
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]
    b["points"]["flags"][0] = 0
    for r, (label, P) in enumerate((("X0", [0, 1, 0, 0, 0, 1, 1, 0, 0]), ("X1", [0, 0, 1, 1, 0, 0, 0, 1, 0]), ("X2", tc.IDENTITY))):
        turned = b["frames"].copy()
        turned["r"][1:] = P
        big = turned.copy()
        big["t"][3] += F(1e38)
        starts, X, finite_b = raw_points(b, big, 1)
        only = [int(i) for i, x, fb in zip(starts, X.T, finite_b) if fb and not np.isfinite(x[r]) and np.isfinite(np.delete(x, r)).all()]
        assert len(only) >= 4, (label, only)

        def one_coordinate(res, b=b, s=s, n=n, K=K, P=np.array(P, np.float64).reshape(3, 3), only=only):
            (o, rows), (obig, rbig) = res
            assert rows.tolist() == [(0, 0, 0, 0), (K, K, n - 1, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
            for l in range(K):  # w = R^T d and c = -R^T t: the map is P^T times the rail's
                assert fields(o[1][s[1][l]], "views", "inliers", "flags", "tail_index") == (n - 1, n - 1, GOOD | PAR, s[n - 1][l])
                assert near(o[1][s[1][l]], P.T @ b["cloud"][l])
            for i in only:
                assert fields(obig[1][i], "views", "inliers", "flags", "origin", "x", "y", "z") == (n - 1, 0, 0, 0, 0, 0, 0), (i, obig[1][i])
            assert fields(rbig[1], "landmarks", "longest") == (K, n - 1) and rbig[1]["good"] <= K - len(only)

        add("cameras turned by a permutation; only %s overflows" % label, [call(b, frames=turned), call(b, frames=big)], one_coordinate)

    # ---- extents, unmapped pairs, empty frames ----
    b = rail(n, K, cap=SMALL, v_hi=V_HI)
    s = b["slots"]

    def extents(res, s=s, K=K):
        for (o, rows), m in zip(res, (2, 3, 4)):
            assert len(o) == m - 1 and rows.tolist() == [(K, K, m, 0)] + [(0, 0, 0, 0)] * (m - 2)
            assert all(o[0][s[0][l]]["tail_index"] == s[m - 1][l] for l in range(K))

    add("n_frames 2, 3, 4", [call(b, n_frames=m) for m in (2, 3, 4)], extents)
    lost = rail(n, K, cap=SMALL, plan=[ORIGIN] + [LOST] * (n - 1), v_hi=V_HI)

    def nothing(origin, n=n):
        def expect(res):
            assert is_zero(res[0][0]) and res[0][1].tolist() == [(0, 0, 0, origin)] * (n - 1)
        return expect

    add("every frame LOST", [call(lost)], nothing(NO_ORIGIN))
    empty = rail(n, K, cap=SMALL, v_hi=V_HI)
    empty["counts"][:] = 0
    add("every counter 0", [call(empty)], nothing(0))

    # ---- octaves ----
    n, K = 6, 8
    b = rail(n, K, cap=SMALL, octaves=2, v_hi=V_HI)
    assert set(b["octave"].tolist()) == {0, 1, 2} and all((c["octave"][:K] <= 2).all() for c in b["corners"])

    def octaves(res, b=b, n=n, K=K):
        o, rows = res[0]
        s = b["slots"]
        for l in range(K):
            r = o[0][s[0][l]]
            assert fields(r, "views", "inliers", "flags", "tail_index") == (n, n, GOOD | PAR, s[n - 1][l]) and near(r, b["cloud"][l]), (l, r, b["cloud"][l])
        assert rows.tolist() == [(K, K, n, 0)] + [(0, 0, 0, 0)] * (n - 2)

    add("octaves 0, 1, 2", [call(b)], octaves)

    # ---- the block edges of k_lm_fuse: every slot a start ----
    for K in (64, 256, 257, 1100):
        b = rail(6, K, v_hi=V_HI)

        def full(res, K=K):
            o, rows = res[0]
            assert rows.tolist() == [(K, K, 6, 0)] + [(0, 0, 0, 0)] * 4
            assert (o[0]["views"] == 6).all() and (o[0]["inliers"] == 6).all() and (o[0]["flags"] == GOOD | PAR).all() and is_zero(o[1:])

        add("capacity %d, every slot a start" % K, [call(b)], full)
    return out
