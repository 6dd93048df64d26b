"""Hand-built inputs of the bridge stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_bridge_consecutive reads the raw counters, the stored records, the matcher's records, the pairs' points,
the frame records of the trajectory stage and the landmark records.  `gapped` builds a localize_cases.views batch -- 64 x 48
frames, one cloud along one path -- in which some steps are a pure rotation or a pause: such a pair's pose record is set to a
status that is not OK and its points lose their flags, as the pose stage leaves a pair without parallax, and its matches are
kept, because the matcher still pairs the keypoints.  That is what differs from localize_cases.join's unrelated runs, whose
bridging matches are all wrong.  `reference` runs the trajectory, landmark and bridge restatements on a batch; `trim` leaves a
gap end an exact number of candidates.
"""
import numpy as np

import bridge_ref as br
import landmark_ref as lmr
import localize_cases as lc
import trajectory_cases as tc
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
U = np.uint32
NONE = orb.ORB_MATCH_NONE
GOOD = orb.ORB_POINT_GOOD
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = tc.CHAINED, tc.START, tc.FEW, tc.SPREAD, tc.LOST, tc.ORIGIN
COPIED, MOVED, FIXED, JOINED, UNFIXED = (orb.ORB_BRIDGE_COPIED, orb.ORB_BRIDGE_MOVED, orb.ORB_BRIDGE_FIXED, orb.ORB_BRIDGE_JOINED,
                                         orb.ORB_BRIDGE_UNFIXED)
L_OK, L_NOMAP, L_FEW, L_DEGENERATE, L_MINIMAL = (orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_NOMAP, orb.ORB_LOCALIZE_FEW,
                                                 orb.ORB_LOCALIZE_DEGENERATE, orb.ORB_LOCALIZE_MINIMAL)
ROTATION, PAUSE = "rotation", "pause"


def small_steps(n, gaps=None):
    """n camera steps that keep a cloud inside a 64 x 48 frame (a third of a degree of yaw, sideways and slightly forward, lengths
    that change by up to 2); step k of `gaps` {k: ROTATION | PAUSE} is a pure rotation of 1.5 degrees or no motion at all."""
    lengths = [0.12, 0.2, 0.1, 0.16, 0.08, 0.14, 0.12, 0.18, 0.1, 0.16, 0.12, 0.15, 0.09]
    steps = []
    for k in range(n):
        kind = (gaps or {}).get(k)
        if kind == ROTATION:
            steps.append((tr.rot("y", 1.5) @ tr.rot("x", -0.4), np.zeros(3)))
        elif kind == PAUSE:
            steps.append((np.eye(3), np.zeros(3)))
        else:
            l = lengths[k % len(lengths)]
            steps.append((tr.rot("y", 0.35) @ tr.rot("x", 0.15), np.array([-l, 0.1 * l, 0.3 * l])))
    return steps


def lose(b, pairs):
    """The pose records of `pairs` set to statuses that are not OK (arbitrary bits elsewhere) and their points' flags cleared; the
    matches stay."""
    rng = np.random.default_rng(len(pairs))
    for c, k in enumerate(pairs):
        q = rng.integers(0, 1 << 32, 16, dtype=U).view(orb.POSE_DTYPE)
        q["status"] = tc.NOT_OK[(c + 2) % 4]
        b["poses"][k] = q[0]
        b["points"][k] = np.zeros(b["cap"], orb.POINT_DTYPE)
    return b


def gapped(rng, n_frames, n_land, cap, gaps, **kw):
    """localize_cases.views along small_steps with the pairs of `gaps` lost."""
    with np.errstate(all="ignore"):  # a step without translation has no unit baseline: its pose and points are replaced below
        b = lc.views(rng, n_frames, n_land, cap, steps=small_steps(n_frames - 1, gaps), **kw)
    b["gaps"] = dict(gaps)
    return lose(b, sorted(gaps))


def inputs(b, n=None):
    n = b["n"] if n is None else n
    nq = lc.stored(b)
    return nq[:n], [c[:nq[f]] for f, c in enumerate(b["corners"][:n])], [b["matches"][f][:nq[f]] for f in range(n - 1)], list(b["points"][:n - 1])


def maps(b, n_frames=None, traj=None, lm=None):
    """The frame records and landmark records of a batch by the trajectory and landmark restatements."""
    n = b["n"] if n_frames is None else n_frames
    intr = lc.intrinsics(b["W"], b["H"], b["focal"])
    fr = tc.reference(b, n, **(traj or {}))[0]
    nq, corners, matches, points = inputs(b, n)
    lms = lmr.landmarks(nq, corners, matches, points, fr, b["cap"], n_frames=n, **{**intr, **(lm or {})})[0]
    return fr, lms


def run(b, fr, lms, n_frames=None, trace=None, **params):
    """bridge_ref.bridge on a batch's arrays under the frame records `fr` and landmark records `lms`."""
    n = b["n"] if n_frames is None else n_frames
    nq, corners, matches, points = inputs(b, n)
    return br.bridge(nq, corners, matches, points, fr[:n], lms, b["cap"], n_frames=n, trace=trace,
                     **{**lc.intrinsics(b["W"], b["H"], b["focal"]), **params})


def reference(b, n_frames=None, traj=None, lm=None, trace=None, **params):
    """A batch through the three restatements.  Returns (frame records, landmark records, OrbBridgePose records, inlier bytes)."""
    fr, lms = maps(b, n_frames, traj, lm)
    return (fr, lms) + tuple(run(b, fr, lms, n_frames, trace=trace, **params))


def trim(b, g, M, traj=None, lm=None, **params):
    """Leaves gap end g exactly M candidates: the first-hop matches of the tails behind the others become ORB_MATCH_NONE.  Fails
    when it has fewer, or when landmarks that share a tail make M unreachable."""
    trace = {}
    fr, lms, out, _ = reference(b, traj=traj, lm=lm, trace=trace, **params)
    T = int(out[g]["anchor"])
    src = trace[g]["src"]
    assert len(src) >= M, (len(src), M)
    for q, i in src[M:]:
        b["matches"]["index"][T, int(lms[q][i]["tail_index"])] = NONE
    trace = {}
    reference(b, traj=traj, lm=lm, trace=trace, **params)
    assert trace[g]["total"] == M, (trace[g]["total"], M)
    return b


def true_step(b, T, g):
    """(R, t) with X_g = R X_T + t in metres, from the batch's steps."""
    R, t = np.eye(3), np.zeros(3)
    for k in range(T, g):
        Rk, tk = b["steps"][k]
        R, t = Rk @ R, Rk @ t + tk
    return R, t


def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ---- the GPU tests' batches (64 x 48 frames) ---------------------------------------------------------------------------------
MAIN_GAPS = {0: PAUSE, 3: ROTATION, 6: PAUSE, 7: ROTATION}


def main_batch(cap):
    """Twelve frames.  A nine-view path: pair 0 lost (frame 1 LOST behind ORIGIN: NOMAP), a one-frame gap (frame 4, a rotation), a
    two-frame gap (frames 7 and 8, a pause and a rotation); then the first frame of a plane's three views, LOST behind unrelated
    matches (all wrong) and the third LOST frame of its run; the plane's last pair lost, so the last frame is a gap end whose
    candidates are coplanar."""
    rng = np.random.default_rng(2031)
    a = gapped(rng, 9, 420, cap, MAIN_GAPS, wrong=0.08, far=0.04, lost=0.04, bad_points=0.04, noise=0.002)
    p = gapped(rng, 3, 220, cap, {1: ROTATION}, shape="plane")
    b = lc.join([a, p], bridge=True)
    b["steps"] = a["steps"]
    return b


def empty_batch(cap):
    """Seven frames of one path; frame 4 is a gap end and stores nothing, so no hop reaches it (FEW); frame 5 starts again."""
    rng = np.random.default_rng(5)
    b = gapped(rng, 7, 200, cap, {3: PAUSE}, noise=0.001)
    b["counts"][4] = 0
    return b


def repeated_batch(cap):
    """Five frames of a cloud of two points, each repeated twenty times; frame 3 is a gap end whose forty candidates are two points:
    no six of them give a model (DEGENERATE)."""
    return gapped(np.random.default_rng(1), 5, 40, cap, {2: ROTATION}, shape="two", unique=False)


def count_batch(cap, M, n_land=90, extra=0, seed=64):
    """Six frames, a gap at frame 4 with exactly M candidates; with `extra`, raw counters above the capacity."""
    b = gapped(np.random.default_rng(seed), 6, n_land, cap, {3: ROTATION}, noise=0.001, extra=extra)
    return trim(b, 4, M, traj=dict(min_shared=4))


SHARED_LM = dict(max_reproj_px=1000.0)


def shared_batch(cap=8):
    """Capacity 8, five frames, a gap at frame 4: two slots of pair 0 match one keypoint of frame 1, so two landmarks share their
    later views and their tail, and the orphaned keypoint starts a landmark of its own in pair 1: nine candidates for eight places
    (the landmarks call at 1000 px, so that the landmark through the wrong keypoints is GOOD)."""
    b = gapped(np.random.default_rng(8), 5, cap, cap, {3: PAUSE}, unique=False)
    assert (lc.stored(b) == cap).all()
    first = b["matches"]["index"][0].copy()
    for i in range(1, cap):  # the first slot whose landmark through slot 0's keypoints comes out in front of every camera
        b["matches"]["index"][0] = first
        b["matches"]["index"][0, i] = first[0]
        trace = {}
        reference(b, traj=dict(min_shared=4), lm=SHARED_LM, trace=trace)
        if trace[4]["total"] == cap + 1:
            return b
    raise AssertionError("no pair of slots shares a tail with both landmarks GOOD")


def plain_batch(cap):
    """Six views without a gap."""
    return lc.views(np.random.default_rng(3), 6, 200, cap, steps=small_steps(5), noise=0.001, wrong=0.05)
