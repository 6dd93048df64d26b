"""orb_adjust_consecutive on the GPU: every OrbAdjustedPose and every one of the capacity's OrbLandmark
records of every pair against the CPU restatement (tests/adjust_ref.py) fed with what the device holds -- the counters, keypoint
records, match records, the frame records of orb_trajectory_read and the landmark records of orb_landmarks_read -- byte for byte,
and then the outcome each construction of tests/adjust_cases.py implies on the device's own records.  No tolerance anywhere.

The programs are 64 x 48 with two levels and zero images, as in tests/test_gpu_landmark_cases.py: the match, epipolar and pose stages
run once on empty frames and the trajectory stage once on what they left, only to be fresh; what the landmarks and adjust calls read
is then written over their buffers (constructed.inject, trajectory_cases.inject_pose, landmark_cases.inject_frames).  The landmarks
call runs on the device under one set of frame records, and where a case says so another set is written before the adjust call."""
import time

import numpy as np
import pytest

import adjust_cases as A
import adjust_ref as ar
import constructed as C
import landmark_cases as L
import localize_cases as lc
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48
MAX_BATCH = 8
CASES = A.cases()
CAPS = sorted({c["cap"] for c in CASES})
assert CAPS == [A.SMALL, 64, 257, 300]


def _program(tinyorb, cap, max_batch=MAX_BATCH, **kw):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=max_batch, **kw)
    return tinyorb.OrbProgram(cfg).init()


def _load(prog, b):
    """The batch over the program's buffers, with every stage the landmarks and adjust calls need fresh."""
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], [c[:b["cap"]] for c in b["corners"]])
    tc.inject_pose(prog, matches=b["matches"], poses=b.get("poses"), points_=b["points"])
    prog.trajectory_consecutive(n)


def _inputs(prog, n, cap):
    """What the adjust call reads, as the device holds it: (counts, records, matches, frame records, landmark records)."""
    counts = np.minimum(prog.batch_counts(n), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n)])
    lms = np.stack([prog.landmarks_read(p, cap)[1] for p in range(n - 1)])
    return counts, corners, matches, frames, lms


def _read(prog, n, cap):
    got = [prog.adjust_read(f, cap) for f in range(n)]
    return np.array([g[0] for g in got]), np.stack([g[1] for g in got])


def _check(prog, n, cap, inputs, intr, call=True, stream=None, **params):
    """One adjust call (unless call=False) and every byte of its read-backs against the restatement of `inputs`.  Returns the
    device's (poses (n,), records (n - 1, cap))."""
    counts, corners, matches, frames, lms = inputs
    if call:
        prog.adjust_consecutive(n, stream=stream, **intr, **params)
    want_p, want_l = ar.adjust(counts, corners, matches, frames, lms, cap, n_frames=n, **intr, **params)
    poses, recs = _read(prog, n, cap)
    for f in range(n):
        assert poses[f].tobytes() == want_p[f].tobytes(), (f, params, poses[f], want_p[f])
    assert not recs[n - 1].tobytes().strip(b"\0")  # the last frame starts no pair
    for p in range(n - 1):
        if recs[p].tobytes() != want_l[p].tobytes():
            bad = np.nonzero((recs[p].view(np.uint32).reshape(cap, 8) != want_l[p].view(np.uint32).reshape(cap, 8)).any(1))[0]
            raise AssertionError((p, params, bad[:8], recs[p][bad[:8]], want_l[p][bad[:8]]))
    return poses, recs[:n - 1]


def _call(prog, k, cap):
    """One call of a case: the frame records in, the landmarks call, the adjust call's own frame records in, the adjust call."""
    b, n = k["batch"], k["n_frames"]
    L.inject_frames(prog, k["frames"])
    prog.landmarks_consecutive(b["n"], **k["intr"], **k["lm"])
    if k["adjust_frames"] is not k["frames"]:
        L.inject_frames(prog, k["adjust_frames"])  # no stage's freshness changes
    inputs = _inputs(prog, b["n"], cap)
    assert inputs[3].tobytes() == np.ascontiguousarray(k["adjust_frames"]).tobytes()
    poses, recs = _check(prog, n, cap, inputs, k["intr"], **k["params"])
    return dict(poses=poses, recs=recs, lms=inputs[4], frames=inputs[3])


@pytest.mark.parametrize("cap", CAPS)
def test_cases(tinyorb, cap):
    """Capacity 8: the cases of BA-2..BA-7.  64: a frame whose keypoints were turned.  257: every slot a landmark, a second block of
    one thread in the per-slot kernels.  300: 300 owned slots in a frame, so slots 256 .. 299 wrap into partial sums 0 .. 43.
    Rounds 1, 4 and 16 where the case says so."""
    t0 = time.perf_counter()
    cases = [c for c in CASES if c["cap"] == cap]
    checked = calls = 0
    with _program(tinyorb, cap) as prog:
        held = None
        for c in cases:
            res = []
            for k in c["calls"]:
                if k["batch"] is not held:
                    held = k["batch"]
                    _load(prog, held)
                res.append(_call(prog, k, cap))
                calls += 1
            try:
                c["expect"](res)
            except AssertionError as e:
                raise AssertionError("case %r: %s" % (c["name"], e)) from e
            checked += 1
    assert checked == len(cases) and checked > 0
    print("capacity %d: %d cases, %d calls, %.2f s" % (cap, checked, calls, time.perf_counter() - t0))


def test_a_turning_camera(tinyorb):
    """One localize_cases.views batch of 6 frames and landmark_cases.restart_batch (8 frames, capacity 300, some joints
    RESTART_SPREAD), each through the device's own trajectory and landmarks calls, at rounds 1, 4 and 16."""
    t0 = time.perf_counter()
    for b, traj, cap in ((lc.views(np.random.default_rng(24), 6, 90, 64, W=W0, H=H0, noise=0.001, wrong=0.05), L.FULL_TRAJ, 64),
                         (L.restart_batch(), L.RESTART_TRAJ, 300)):
        n, intr = b["n"], lc.intrinsics(b["W"], b["H"], b["focal"])
        with _program(tinyorb, cap) as prog:
            lc.inject(prog, b)
            prog.trajectory_consecutive(n, **traj)
            prog.landmarks_consecutive(n, **intr)
            inputs = _inputs(prog, n, cap)
            status = inputs[3]["status"].tolist()
            assert status.count(tc.CHAINED) >= 2, status
            for rounds in (1, 4, 16):
                poses, recs = _check(prog, n, cap, inputs, intr, rounds=rounds)
                refined = poses["status"] == A.REFINED
                assert refined.sum() >= 2 and (poses["observations"][refined] >= 6).all(), (rounds, poses["status"], poses["observations"])
                print("%d frames at capacity %d, %d rounds: statuses %s, adjusted %s, observations %s, cost %.4f -> %.4f" %
                      (n, cap, rounds, status, poses["status"].tolist(), poses["observations"].tolist(),
                       float(poses["cost_before"][refined].sum()), float(poses["cost_after"][refined].sum())))
    print("turning camera: %.2f s" % (time.perf_counter() - t0))


def test_state_arguments_and_ordering(tinyorb):
    """ORB_ESTATE before the landmarks call and after a new batch; every argument rule; two calls on one program with different
    `rounds`, the second one's bytes its own; a call on another stream ordered behind the landmark stage's, and the landmark,
    trajectory and match stages behind it."""
    import torch
    t0 = time.perf_counter()
    T = tinyorb
    cap = 64
    b = lc.views(np.random.default_rng(5), 5, 90, cap, W=W0, H=H0, noise=0.001)
    n, intr = b["n"], lc.intrinsics(W0, H0, b["focal"])
    lib = T.load_library()
    with _program(T, cap, max_batch=5) as prog:

        def code(n_frames=n, **kw):
            try:
                prog.adjust_consecutive(n_frames, **{**intr, **kw})
            except T.OrbError as e:
                return e.code
            return T.ORB_OK

        with pytest.raises(T.OrbError) as e:
            prog.adjust_read(0, 0)
        assert e.value.code == T.ORB_ESTATE
        lc.inject(prog, b)
        assert code() == T.ORB_ESTATE  # neither the trajectory nor the landmarks
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        assert code() == T.ORB_ESTATE  # before the landmarks call
        prog.landmarks_consecutive(n, **intr)
        nan, inf = float("nan"), float("inf")
        for kw in (dict(n_frames=1), dict(n_frames=n + 1), dict(rounds=17), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(fx=0.0),
                   dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf), dict(max_reproj_px=-1.0), dict(max_reproj_px=nan)):
            assert code(**kw) == T.ORB_EINVAL, kw
        assert lib.orb_adjust_consecutive(prog._handle(), n, None, None) == T.ORB_EINVAL
        assert lib.orb_adjust_consecutive(prog._handle(), n, T.OrbAdjustParams(), None) == T.ORB_EINVAL  # a zero-initialised struct is not valid
        prog.landmarks_consecutive(3, **intr)
        assert code(n_frames=4) == T.ORB_EINVAL  # four frames asked for, the landmarks of three
        prog.landmarks_consecutive(n, **intr)
        inputs = _inputs(prog, n, cap)
        assert inputs[3]["status"].tolist() == [tc.ORIGIN, tc.START, tc.CHAINED, tc.CHAINED, tc.CHAINED]
        # two calls with different rounds: each one's bytes are those of its own inputs
        one = _check(prog, n, cap, inputs, intr, rounds=1)
        four = _check(prog, n, cap, inputs, intr)  # the default
        assert _check(prog, n, cap, inputs, intr, rounds=4)[0].tobytes() == four[0].tobytes() != one[0].tobytes()
        assert _check(prog, n, cap, inputs, intr, rounds=1)[0].tobytes() == one[0].tobytes()
        _check(prog, 3, cap, inputs, intr)
        blob = [a.tobytes() for a in _check(prog, n, cap, inputs, intr)]
        # read errors
        with pytest.raises(T.OrbError) as e:
            prog.adjust_read(n, cap)
        assert e.value.code == T.ORB_EINVAL
        assert lib.orb_adjust_read(prog._handle(), n - 1, None, None, 5) == T.ORB_EINVAL  # landmarks NULL with n > 0
        assert lib.orb_adjust_read(prog._handle(), n - 1, None, None, 0) == T.ORB_OK
        assert len(prog.adjust_read(1, cap + 100)[1]) == cap and len(prog.adjust_read(1)[1]) == cap and len(prog.adjust_read(1, 7)[1]) == 7
        # isolation: what the stages it reads hold, before and after
        def others():
            return [prog.match_read(f, cap).tobytes() + prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() +
                    prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() + prog.pose_read(f, cap)[1].tobytes()
                    for f in range(n - 1)]

        before = others()
        _check(prog, n, cap, inputs, intr, rounds=2)
        assert others() == before
        # ordering: the landmarks call on a second stream and the adjust call on the first, which waits for it
        s = torch.cuda.Stream(device=0)
        prog.landmarks_consecutive(n, stream=s.cuda_stream, **intr)
        assert [a.tobytes() for a in _check(prog, n, cap, inputs, intr)] == blob
        # the adjust call on the second stream, then the stages it reads on the first: each waits before it overwrites
        prog.adjust_consecutive(n, stream=s.cuda_stream, **intr)
        prog.landmarks_consecutive(n, max_reproj_px=1e-6, **intr)  # no landmark GOOD
        prog.trajectory_consecutive(n, min_shared=10000)            # every joint RESTART_FEW
        prog.match_consecutive(n)
        assert [a.tobytes() for a in _check(prog, n, cap, inputs, intr, call=False)] == blob
        # a new batch: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
    print("state: %.2f s" % (time.perf_counter() - t0))
