"""Hand-built inputs of the landmark stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_landmarks_consecutive reads the raw counters, the stored records, the matcher's records, the flags of the
pairs' points and the frame records of the trajectory stage.  `rail` builds all of them directly for a camera that slides along x
without turning, with a focal length of 64 and depths of 8 and 16, so that every projection is an integer pixel and every ray meets
its landmark exactly: a test then changes one flag, index, counter, keypoint or frame record and sees what that alone does.  The
batches of tests/localize_cases.py (`views`, `join`) serve the cases that need a turning camera, and the GPU tests; `reference`
runs the trajectory restatement and then the landmark restatement on such a batch.
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


def rail(n_frames, K, cap=None, plan=None, seed=0):
    """K landmarks seen in all n_frames (at most 6) views of the rail camera.  Landmark l sits at slot slots[f][l] of frame f (a
    permutation per frame), matched to its slot in the next frame, GOOD | PARALLAX in every pair; its keypoint in frame f is
    (u0 - shift * f, v0) with a shift of 4 px (depth 8) or 2 px (depth 16).  Returns a batch dict as localize_cases.views does, with
    `frames` (the records under `plan`, default ORIGIN, START, CHAINED ...), `slots`, `cloud` (K, 3) in camera 0's frame."""
    assert 2 <= n_frames <= 6
    rng = np.random.default_rng(seed)
    cap = K if cap is None else cap
    plan = [ORIGIN, START] + [CHAINED] * (n_frames - 2) if plan is None else plan
    u0, v0 = rng.integers(24, 60, K), rng.integers(4, 60, K)
    z = np.where(rng.random(K) < 0.5, 8.0, 16.0)
    z[:2] = 8.0, 16.0
    cloud = np.stack([(u0 - 32.0) * z / 64.0, (v0 - 32.0) * z / 64.0, z], 1)
    shift = (64.0 * RAIL_BASE / z).astype(np.int64)
    slots = [rng.permutation(K) for _ in range(n_frames)]
    corners = []
    for f in range(n_frames):
        c = C.corners(np.zeros(cap, np.int64), np.zeros(cap, np.int64), 0)
        c["x"][slots[f]], c["y"][slots[f]] = u0 - shift * f, v0
        corners.append(c)
    M = np.zeros((n_frames - 1, cap), orb.MATCH_DTYPE)
    M["index"], M["distance"], M["second"] = NONE, 0xFFFF, 0xFFFF
    P = np.zeros((n_frames - 1, cap), orb.POINT_DTYPE)
    for f in range(n_frames - 1):
        M["index"][f, slots[f]] = slots[f + 1]
        P["x"][f, slots[f]], P["y"][f, slots[f]], P["z"][f, slots[f]] = cloud[:, 0] - RAIL_BASE * f, cloud[:, 1], cloud[:, 2]
        P["flags"][f, slots[f]] = GOOD | PAR
    return dict(counts=np.full(n_frames, K, U), corners=corners, matches=M, points=P, cap=cap, n=n_frames, frames=frame_records(plan),
                slots=slots, cloud=cloud)


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
