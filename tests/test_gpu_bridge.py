"""The bridge stage on the GPU (orb_bridge_consecutive): every OrbBridgePose byte and inlier byte against the
CPU restatement (tests/bridge_ref.py) fed with the device's own counts, records, matches, points, orb_trajectory_read and
orb_landmarks_read output, on hand-built batches (tests/bridge_cases.py) of 64 x 48 frames written over the stages' buffers, with
the trajectory and landmarks calls on the device behind the injection: gaps of one and two frames, NOMAP behind ORIGIN, a gap at
the last frame, unrelated matches, coplanar candidates, an empty frame, two points repeated, each parameter, 5 to 7 and 255 to 257 candidates, raw
counters above the capacity, shared tails beyond the capacity, a batch without a gap; the other stages' results untouched; the
call's state, argument and stream rules."""
import numpy as np
import pytest

import bridge_cases as B
import constructed as C
import bridge_ref as brr
import localize_cases as lc

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)
COPIED, MOVED, FIXED, JOINED, UNFIXED = B.COPIED, B.MOVED, B.FIXED, B.JOINED, B.UNFIXED
CHAINED, START, LOST, ORIGIN = B.CHAINED, B.START, B.LOST, B.ORIGIN


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _setup(prog, b, traj=None, lm=None):
    """The batch over the program's buffers, then the trajectory and landmarks calls on the device."""
    lc.inject(prog, b)
    prog.trajectory_consecutive(b["n"], **(traj or {}))
    prog.landmarks_consecutive(b["n"], **INTR, **(lm or {}))
    return _inputs(prog, b["n"], b["cap"])


def _inputs(prog, n_frames, cap):
    """What the call reads, as the device holds it."""
    counts = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    points = [prog.pose_read(f, cap)[1] for f in range(n_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames)])
    lms = [prog.landmarks_read(p, cap)[1] for p in range(n_frames - 1)]
    return counts, corners, matches, points, frames, lms


def _check(prog, n_frames, cap, inputs, stream=None, call=True, **params):
    """Bridge call, then every frame's record and cap inlier bytes against the restatement, byte for byte.  Returns the device's
    records (BRIDGE_POSE_DTYPE (n_frames,)), its inlier bytes and the bytes of everything read."""
    counts, corners, matches, points, frames, lms = inputs
    if call:
        prog.bridge_consecutive(n_frames, stream=stream, **INTR, **params)
    want, wmask = brr.bridge(counts, corners, matches, points, frames[:n_frames], lms, cap, n_frames=n_frames, **INTR, **params)
    recs, masks, blob = [], [], b""
    for f in range(n_frames):
        rec, mask = prog.bridge_read(f, cap)
        assert rec.tobytes() == want[f].tobytes(), (f, params, rec, want[f])
        assert mask.tobytes() == wmask[f].tobytes(), (f, params, np.nonzero(mask != wmask[f])[0][:8])
        recs.append(rec)
        masks.append(mask)
        blob += rec.tobytes() + mask.tobytes()
    return np.array(recs), np.array(masks), blob


def test_gaps_parameters_and_extents(tinyorb):
    """Capacity 1100 (no multiple of 64, 256 or 1024), twelve frames (bridge_cases.main_batch), then each parameter and
    n_frames 2, 3 and 12."""
    T = tinyorb
    cap = 1100
    b = B.main_batch(cap)
    n = b["n"]
    with _program(T, cap, 12) as prog:
        inputs = _setup(prog, b)
        assert n == 12 and inputs[4]["status"].tolist() == [ORIGIN, LOST, START, CHAINED, LOST, START, CHAINED, LOST, LOST, LOST, START, LOST]
        recs, masks, blob = _check(prog, n, cap, inputs)
        print("status", recs["status"].tolist(), "fix", recs["fix"].tolist(), "candidates", recs["candidates"].tolist(), "inliers", recs["inliers"].tolist())
        # what the restatement gives on these arrays (tests/test_bridge_ref.py checks the fixes against the true steps)
        assert recs["status"].tolist() == [COPIED, UNFIXED, COPIED, COPIED, JOINED, MOVED, MOVED, FIXED, FIXED, FIXED, COPIED, FIXED]
        assert recs["root"].tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 9, 9] and recs["anchor"].tolist() == [0, 0, 0, 0, 3, 0, 0, 6, 6, 6, 0, 10]
        assert recs["fix"][1] == T.ORB_LOCALIZE_NOMAP and not masks[1].any()
        for f in range(n):
            gap = inputs[4]["status"][f] == LOST
            assert int(masks[f].sum()) <= int(recs["inliers"][f]) and (gap or not masks[f].any())
            assert not masks[f][inputs[0][f]:].any()
        for kw in (dict(seed=12345), dict(max_reproj_px=0.5), dict(max_reproj_px=1000.0), dict(max_reproj_px=1e-6), dict(hypotheses=1),
                   dict(hypotheses=64), dict(hypotheses=65), dict(hypotheses=512), dict(window=1), dict(max_distance=20, ratio=0.2)):
            got, _, _ = _check(prog, n, cap, inputs, **kw)
            print(kw, "status", got["status"].tolist(), "fix", got["fix"].tolist(), "inliers", got["inliers"].tolist())
        one, _, _ = _check(prog, n, cap, inputs, max_hops=1)
        assert one["status"].tolist()[7:10] == [FIXED, UNFIXED, UNFIXED] and one["fix"].tolist()[8:10] == [T.ORB_LOCALIZE_NOMAP] * 2
        few, _, _ = _check(prog, n, cap, inputs, min_shared=1000)
        assert few["status"][4] == FIXED and few["shared"][4] == recs["shared"][4] and few["status"].tolist()[5:7] == [COPIED, COPIED]
        spread, _, _ = _check(prog, n, cap, inputs, scale_tolerance=1e-5)
        assert spread["status"][4] == FIXED and spread["consistent"][4] < recs["consistent"][4] and spread["root"].tolist()[5:7] == [4, 4]
        two, _, _ = _check(prog, 2, cap, inputs)
        assert two["status"].tolist() == [COPIED, UNFIXED]
        _check(prog, 3, cap, inputs)
        five, _, _ = _check(prog, 5, cap, inputs)  # the gap end is the last frame: no join
        assert five["status"][4] == FIXED
        with pytest.raises(T.OrbError) as e:
            prog.bridge_read(5, cap)
        assert e.value.code == T.ORB_EINVAL
        assert _check(prog, n, cap, inputs)[2] == blob  # stale candidates, keys, ratios or inlier bytes of the calls between would show


def test_an_empty_gap_end_and_repeated_points(tinyorb):
    T = tinyorb
    cap = 300
    b = B.empty_batch(cap)
    with _program(T, cap, b["n"]) as prog:
        inputs = _setup(prog, b)
        assert inputs[0][4] == 0 and inputs[4]["status"].tolist()[3:6] == [CHAINED, LOST, START]
        recs, masks, _ = _check(prog, b["n"], cap, inputs)
        assert recs["fix"][4] == T.ORB_LOCALIZE_FEW and recs["status"][4] == UNFIXED and not masks.any()
    b = B.repeated_batch(cap)  # two points repeated: DEGENERATE
    with _program(T, cap, b["n"]) as prog:
        inputs = _setup(prog, b, traj=dict(min_shared=4))
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, LOST, START]
        recs, masks, _ = _check(prog, b["n"], cap, inputs)
        assert recs["fix"][3] == T.ORB_LOCALIZE_DEGENERATE and recs["status"].tolist() == [COPIED, COPIED, COPIED, UNFIXED, COPIED] and not masks.any()
        assert recs["candidates"][3] == 0 and recs["root"].tolist() == [0, 0, 0, 3, 3]


@pytest.mark.parametrize("cap,n_land,extra,counts", [(64, 90, 11, (5, 6, 7)), (1100, 900, 0, (255, 256, 257))])
def test_candidate_counts_at_the_edges(tinyorb, cap, n_land, extra, counts):
    """Capacity 64 with raw counters above it: 5 (FEW), 6 and 7 candidates.  Capacity 1100: 255, 256 and 257, the score kernel's tile."""
    T = tinyorb
    with _program(T, cap, 6) as prog:
        for M in counts:
            b = B.count_batch(cap, M, n_land=n_land, extra=extra)
            inputs = _setup(prog, b, traj=dict(min_shared=4))
            if extra:
                assert (prog.batch_counts(6) == cap + extra).all() and (inputs[0] == cap).all()
            assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, LOST, START]
            recs, _, _ = _check(prog, 6, cap, inputs, min_shared=4)
            print(M, recs[4])
            if M < 6:
                assert recs["fix"][4] == T.ORB_LOCALIZE_FEW and recs["candidates"][4] == 0
            else:
                assert recs["fix"][4] in (T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_MINIMAL) and recs["candidates"][4] == M
            _check(prog, 6, cap, inputs, hypotheses=65, seed=7)


def test_shared_tails_beyond_the_capacity(tinyorb):
    T = tinyorb
    cap = 8
    b = B.shared_batch(cap)
    with _program(T, cap, b["n"]) as prog:
        inputs = _setup(prog, b, traj=dict(min_shared=4), lm=B.SHARED_LM)
        trace = {}
        counts, corners, matches, points, frames, lms = inputs
        brr.bridge(counts, corners, matches, points, frames, lms, cap, trace=trace, **INTR)
        assert trace[4]["total"] == 9 and len(trace[4]["k"]) == 8  # nine candidates, the first eight kept
        recs, _, _ = _check(prog, b["n"], cap, inputs)
        assert recs["candidates"][4] in (0, 8)
        _check(prog, b["n"], cap, inputs, max_reproj_px=1000.0, min_shared=1)


def test_a_batch_without_a_lost_frame_is_the_trajectory(tinyorb):
    T = tinyorb
    cap = 300
    b = B.plain_batch(cap)
    n = b["n"]
    with _program(T, cap, n) as prog:
        inputs = _setup(prog, b)
        assert inputs[4]["status"].tolist() == [ORIGIN, START] + [CHAINED] * (n - 2)
        recs, masks, _ = _check(prog, n, cap, inputs)
        for f in range(n):
            tj = prog.trajectory_read(f, 0)[0]
            assert recs[f]["r"].tobytes() == tj["r"].tobytes() and recs[f]["t"].tobytes() == tj["t"].tobytes()
            assert recs[f]["scale"].tobytes() == tj["scale"].tobytes()
        assert (recs["status"] == COPIED).all() and (recs["gain"] == 1).all() and not recs["root"].any() and not masks.any()


def test_isolation_state_arguments_and_ordering(tinyorb):
    import torch
    T = tinyorb
    cap, n = 300, 5
    b = B.gapped(np.random.default_rng(77), n, 250, cap, {2: B.ROTATION}, wrong=0.1, noise=0.002)

    def code(n_frames=n, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.bridge_consecutive(n_frames, **{**INTR, **kw})
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.bridge_read(0, cap)  # no bridge call yet
        assert e.value.code == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # no match
        lc.inject(prog, b)  # match -> verify_epipolar -> pose on a new batch, then the arrays
        assert code() == T.ORB_ESTATE  # no trajectory
        prog.trajectory_consecutive(n)
        assert code() == T.ORB_ESTATE  # no landmarks
        prog.landmarks_consecutive(n, **INTR)
        inf, nan = float("inf"), float("nan")
        for kw in (dict(n_frames=1), dict(n_frames=0), dict(n_frames=n + 1), dict(reserved=(1, 0)), dict(reserved=(0, 7)), dict(fx=0.0), dict(fy=-1.0),
                   dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf), dict(max_reproj_px=-1.0), dict(max_reproj_px=nan), dict(max_reproj_px=inf),
                   dict(ratio=-0.5), dict(ratio=nan), dict(scale_tolerance=-1.0), dict(scale_tolerance=inf), dict(hypotheses=4097),
                   dict(max_distance=257), dict(max_hops=17), dict(window=4096), dict(consistent_permille=1001)):
            assert code(**kw) == T.ORB_EINVAL, kw
        lib = T.load_library()
        assert lib.orb_bridge_consecutive(prog._handle(), n, None, None) == T.ORB_EINVAL  # NULL params: the intrinsics have no default
        assert lib.orb_bridge_consecutive(prog._handle(), n, T.OrbBridgeParams(), None) == T.ORB_EINVAL  # a zero-initialised struct is not valid
        prog.landmarks_consecutive(3, **INTR)
        assert code(n_frames=4) == T.ORB_EINVAL  # four frames asked for, landmarks of three
        _check(prog, 3, cap, _inputs(prog, 3, cap))
        prog.landmarks_consecutive(n, **INTR)
        inputs = _inputs(prog, n, cap)
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, LOST, START]
        recs, _, blob = _check(prog, n, cap, inputs, hypotheses=64)
        assert recs["status"].tolist()[:3] == [COPIED] * 3 and recs["fix"][3] == T.ORB_LOCALIZE_OK
        # read errors
        with pytest.raises(T.OrbError) as e:
            prog.bridge_read(n, cap)
        assert e.value.code == T.ORB_EINVAL
        assert lib.orb_bridge_read(prog._handle(), 0, None, None, 5) == T.ORB_EINVAL  # inliers NULL with n > 0
        assert lib.orb_bridge_read(prog._handle(), 0, None, None, 0) == T.ORB_OK
        assert len(prog.bridge_read(1, cap + 100)[1]) == cap and len(prog.bridge_read(1)[1]) == cap and len(prog.bridge_read(1, 7)[1]) == 7
        C.check_read_arguments(T, prog, lib.orb_bridge_read, n, 1, head=True)
        # isolation: the other stages' read-backs before and after bridge calls
        prog.verify_consecutive(n, inlier_px=2.0)
        prog.localize_consecutive(n, **INTR)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                    prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() +
                    prog.localize_read(f, cap)[0].tobytes() + prog.localize_read(f, cap)[1].tobytes() +
                    prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]

        before = others()
        _check(prog, n, cap, inputs, hypotheses=64)
        _check(prog, 4, cap, inputs, max_reproj_px=1.0, hypotheses=32)
        assert others() == before
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.bridge_consecutive(n, stream=s.cuda_stream, hypotheses=64, **INTR)
        assert _check(prog, n, cap, inputs, call=False, hypotheses=64)[2] == blob
        assert _check(prog, n, cap, inputs, hypotheses=64)[2] == blob
        assert _check(prog, n, cap, inputs, stream=s.cuda_stream, hypotheses=64)[2] == blob
        # a call on the second stream, then the four stages it reads on the first, which overwrite what it reads: each waits for it
        import trajectory_cases as tc
        prog.bridge_consecutive(n, stream=s.cuda_stream, hypotheses=64, **INTR)
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        assert _check(prog, n, cap, inputs, call=False, hypotheses=64)[2] == blob
        tc.inject_pose(prog, b["matches"], b["poses"], b["points"])  # the calls above wrote their own
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        assert _check(prog, n, cap, inputs, hypotheses=64)[2] == blob
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        assert code() == T.ORB_ESTATE  # match, pose and trajectory are fresh, the landmarks are not
        prog.landmarks_consecutive(n, **INTR)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, n, cap, _inputs(prog, n, cap))  # fresh again: parity on the new batch's own (empty) records
