"""The landmark stage on the GPU (orb_landmarks_consecutive): every OrbLandmark and OrbLandmarkRow byte against
the CPU restatement (tests/landmark_ref.py) fed with the device's own counts, records, matches, points and orb_trajectory_read
records, on hand-built batches (tests/landmark_cases.py, tests/localize_cases.py) of 64 x 48 frames written over the stages' buffers,
with a trajectory call on the device behind the injection: LOST frames and new origins, an empty frame, each parameter, every
extent, raw counters above the capacity, a 70-frame chain, chains cut and restarted in one frame; the other stages' results
untouched; the call's state, argument and stream rules."""
import numpy as np
import pytest

import constructed as C
import landmark_cases as L
import landmark_ref as lmr
import localize_cases as lc

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = L.CHAINED, L.START, L.FEW, L.SPREAD, L.LOST, L.ORIGIN
NO = 0xFFFFFFFF


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _inputs(prog, n_frames, cap):
    """What the call reads, as the device holds it: stored counts and records, the matcher's records, the pairs' points, the frame
    records of the last trajectory call."""
    counts = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    points = [prog.pose_read(f, cap)[1] for f in range(n_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames)])
    return counts, corners, matches, points, frames


def _check(prog, n_frames, cap, inputs, stream=None, call=True, **params):
    """Landmarks call, then every pair's row and cap records against the restatement, byte for byte.  Returns the device's rows
    (LANDMARK_ROW_DTYPE (n_frames - 1,)), its records and the bytes of everything read."""
    counts, corners, matches, points, frames = inputs
    if call:
        prog.landmarks_consecutive(n_frames, stream=stream, **INTR, **params)
    want, wrows = lmr.landmarks(counts, corners, matches, points, frames[:n_frames], cap, n_frames=n_frames, **INTR, **params)
    rows, recs, blob = [], [], b""
    for p in range(n_frames - 1):
        row, got = prog.landmarks_read(p, cap)
        assert row.tobytes() == wrows[p].tobytes(), (p, params, row, wrows[p])
        if got.tobytes() != want[p].tobytes():
            bad = np.nonzero(got.view(np.uint32).reshape(cap, 8) != want[p].view(np.uint32).reshape(cap, 8))[0]
            raise AssertionError((p, params, bad[:8], got[bad[:8]], want[p][bad[:8]]))
        rows.append(row)
        recs.append(got)
        blob += row.tobytes() + got.tobytes()
    return np.array(rows), np.array(recs), blob


def test_segments_parameters_and_extents(tinyorb):
    """Capacity 1100 (no multiple of 64, 256 or 1024), twelve frames: a five-view path, LOST frames with a new origin behind each,
    a RESTART_SPREAD, an empty frame; each parameter; n_frames 2, 3 and the whole batch."""
    T = tinyorb
    cap = 1100
    b = L.status_batch(cap)
    B = b["n"]
    with _program(T, cap, 12) as prog:
        lc.inject(prog, b)
        prog.trajectory_consecutive(B)
        inputs = _inputs(prog, B, cap)
        assert B == 12 and inputs[0].tolist() == lc.stored(b).tolist() and inputs[0][11] == 0
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, CHAINED, LOST, START, CHAINED, LOST, START, SPREAD, LOST]
        rows, recs, blob = _check(prog, B, cap, inputs)
        print("rows", rows.tolist())
        # what the restatement gives on these arrays (tests/landmark_cases.py): the counts of the path, the plane, the wrong matches
        assert rows.tolist() == [(342, 250, 5, 0), (79, 63, 4, 0), (80, 62, 3, 0), (74, 67, 2, 0), (0, 0, 0, NO), (158, 158, 3, 5), (7, 7, 2, 5),
                                 (0, 0, 0, NO), (138, 21, 2, 8), (131, 19, 2, 9), (0, 0, 0, NO)]
        for p in (4, 7, 10):
            assert not recs[p].view(np.uint8).any()
        for p in range(B - 1):  # LM-6: the rows count the records; every start carries its origin; no record at or above n_q(p)
            s = recs[p]["views"] != 0
            assert (int(s.sum()), int(((recs[p]["flags"] & T.ORB_POINT_GOOD) != 0).sum()), int(recs[p]["views"].max())) == tuple(rows[p].tolist()[:3])
            assert (recs[p]["origin"][s] == rows[p]["origin"]).all() and not recs[p][inputs[0][p]:].view(np.uint8).any()
        # each parameter, against the restatement; what it moves
        tight, _, _ = _check(prog, B, cap, inputs, max_reproj_px=0.5)
        assert tight["good"].tolist() == [196, 59, 55, 67, 0, 140, 7, 0, 6, 5, 0] and tight["landmarks"].tolist() == rows["landmarks"].tolist()
        wide, _, _ = _check(prog, B, cap, inputs, max_reproj_px=1000.0)
        assert wide["good"].tolist() == [313, 75, 73, 69, 0, 158, 7, 0, 82, 88, 0]
        tiny, trec, _ = _check(prog, B, cap, inputs, max_reproj_px=1e-6)
        assert not tiny["good"].any() and (trec["z"][0] != 0).sum() > 300  # solved but not GOOD: the coordinates are kept
        three, _, _ = _check(prog, B, cap, inputs, min_views=3)
        assert three["good"].tolist() == [177, 47, 37, 0, 0, 154, 0, 0, 0, 0, 0]
        many, _, _ = _check(prog, B, cap, inputs, min_views=100)
        assert not many["good"].any() and many["longest"].tolist() == rows["longest"].tolist()
        # n_frames 2 and 3: shorter chains from the same starts; a pair beyond the call is an error
        two, _, _ = _check(prog, 2, cap, inputs)
        assert two.tolist() == [(342, 300, 2, 0)]
        part, _, _ = _check(prog, 3, cap, inputs)
        assert part.tolist() == [(342, 277, 3, 0), (79, 72, 2, 0)]
        with pytest.raises(T.OrbError) as e:
            prog.landmarks_read(2, cap)
        assert e.value.code == T.ORB_EINVAL
        assert _check(prog, B, cap, inputs)[2] == blob  # stale predecessor bytes, rows or records of the calls between would show


def test_raw_counters_above_the_capacity(tinyorb):
    T = tinyorb
    cap = 64
    b = L.full_batch(cap)
    with _program(T, cap, b["n"]) as prog:
        lc.inject(prog, b)
        prog.trajectory_consecutive(b["n"], **L.FULL_TRAJ)
        raw = prog.batch_counts(b["n"])
        inputs = _inputs(prog, b["n"], cap)
        assert (raw == cap + 11).all() and (inputs[0] == cap).all()
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, CHAINED, CHAINED]
        rows, _, _ = _check(prog, b["n"], cap, inputs)
        assert rows.tolist() == [(44, 39, 6, 0), (17, 11, 5, 0), (16, 15, 4, 0), (12, 10, 3, 0), (17, 16, 2, 0)]
        _check(prog, b["n"], cap, inputs, min_views=4, max_reproj_px=1.0)


def test_a_chain_of_seventy_frames(tinyorb):
    T = tinyorb
    n, cap = L.LONG_FRAMES, L.LONG_CAP
    b = L.long_batch()
    with _program(T, cap, n) as prog:
        lc.inject(prog, b)
        prog.trajectory_consecutive(n, **L.LONG_TRAJ)
        inputs = _inputs(prog, n, cap)
        assert inputs[4]["status"].tolist() == [ORIGIN, START] + [CHAINED] * (n - 2)
        rows, recs, _ = _check(prog, n, cap, inputs)
        assert rows[0].tolist() == (8, 7, 70, 0) and sorted(recs[0]["views"].tolist()) == [5] + [70] * 7
        assert ((recs[0]["flags"] & T.ORB_POINT_GOOD) != 0).sum() == 7 and (recs[0]["inliers"][recs[0]["views"] == 70] == 70).all()
        part, _, _ = _check(prog, 66, cap, inputs, min_views=66)
        assert part[0].tolist() == (8, 7, 66, 0)


def test_chains_cut_and_restarted_in_the_same_frame(tinyorb):
    """Trajectory parameters that make RESTART_SPREAD on some joints of one path and RESTART_FEW on all of them: frame p + 2 is a
    RESTART, so pair p's chains end with frame p + 1 and pair p + 1 starts every landmark again with a new origin."""
    T = tinyorb
    cap = 300
    b = L.restart_batch(cap)
    n = b["n"]
    with _program(T, cap, n) as prog:
        lc.inject(prog, b)
        prog.trajectory_consecutive(n, **L.RESTART_TRAJ)
        inputs = _inputs(prog, n, cap)
        assert inputs[4]["status"].tolist() == [ORIGIN, START, SPREAD, SPREAD, CHAINED, SPREAD, SPREAD, CHAINED]
        assert inputs[4]["origin"].tolist() == [0, 0, 1, 2, 2, 4, 5, 5]
        rows, _, _ = _check(prog, n, cap, inputs)
        assert rows["longest"].tolist() == [2, 2, 3, 2, 2, 3, 2] and rows["origin"].tolist() == [0, 1, 2, 2, 4, 5, 5]
        prog.trajectory_consecutive(n, min_shared=10000)
        inputs = _inputs(prog, n, cap)
        assert inputs[4]["status"].tolist() == [ORIGIN, START] + [FEW] * (n - 2)
        rows, _, _ = _check(prog, n, cap, inputs)
        assert rows.tolist() == [(220, 212, 2, 0), (202, 192, 2, 1), (191, 184, 2, 2), (164, 158, 2, 3), (166, 158, 2, 4), (148, 143, 2, 5), (134, 126, 2, 6)]


def test_isolation_state_arguments_and_ordering(tinyorb):
    import torch
    T = tinyorb
    cap, n = 300, 5
    b = lc.views(np.random.default_rng(77), n, 250, cap, wrong=0.1, noise=0.002)

    def code(n_frames=n, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.landmarks_consecutive(n_frames, **{**INTR, **kw})
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.landmarks_read(0, cap)  # no landmarks call yet
        assert e.value.code == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # no match
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        assert code() == T.ORB_ESTATE  # no pose
        lc.inject(prog, b)  # match -> verify_epipolar -> pose on a new batch, then the arrays
        assert code() == T.ORB_ESTATE  # no trajectory
        prog.trajectory_consecutive(n)
        inf, nan = float("inf"), float("nan")
        for kw in (dict(n_frames=1), dict(n_frames=0), dict(n_frames=n + 1), dict(reserved=(1, 0)), dict(reserved=(0, 7)), dict(fx=0.0), dict(fy=-1.0),
                   dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf), dict(max_reproj_px=-1.0), dict(max_reproj_px=nan), dict(max_reproj_px=inf)):
            assert code(**kw) == T.ORB_EINVAL, kw
        lib = T.load_library()
        assert lib.orb_landmarks_consecutive(prog._handle(), n, None, None) == T.ORB_EINVAL  # NULL params: the intrinsics have no default
        zero = T.OrbLandmarkParams()
        assert lib.orb_landmarks_consecutive(prog._handle(), n, zero, None) == T.ORB_EINVAL  # a zero-initialised struct is not valid
        prog.trajectory_consecutive(3)
        assert code(n_frames=4) == T.ORB_EINVAL  # four frames asked for, three chained
        inputs3 = _inputs(prog, 3, cap)
        _check(prog, 3, cap, inputs3)
        _check(prog, 2, cap, inputs3)
        prog.trajectory_consecutive(n)
        inputs = _inputs(prog, n, cap)
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, CHAINED]
        rows, _, blob = _check(prog, n, cap, inputs)
        assert rows["longest"].tolist() == [5, 4, 3, 2] and (rows["good"] > 0).all()
        # read errors
        with pytest.raises(T.OrbError) as e:
            prog.landmarks_read(n - 1, cap)
        assert e.value.code == T.ORB_EINVAL
        assert lib.orb_landmarks_read(prog._handle(), 0, None, None, 5) == T.ORB_EINVAL  # landmarks NULL with n > 0
        assert lib.orb_landmarks_read(prog._handle(), 0, None, None, 0) == T.ORB_OK
        assert len(prog.landmarks_read(1, cap + 100)[1]) == cap and len(prog.landmarks_read(1)[1]) == cap and len(prog.landmarks_read(1, 7)[1]) == 7
        C.check_read_arguments(T, prog, lib.orb_landmarks_read, n - 1, 32, head=True)
        # isolation: the other stages' read-backs before and after landmarks calls
        prog.verify_consecutive(n, inlier_px=2.0)
        prog.localize_consecutive(n, **INTR)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                    prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() +
                    prog.localize_read(f, cap)[0].tobytes() + prog.localize_read(f, cap)[1].tobytes() for f in range(n - 1)]

        before = others()
        _check(prog, n, cap, inputs)
        _check(prog, 3, cap, inputs, max_reproj_px=1.0, min_views=3)
        assert others() == before
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.landmarks_consecutive(n, stream=s.cuda_stream, **INTR)
        assert _check(prog, n, cap, inputs, call=False)[2] == blob
        assert _check(prog, n, cap, inputs)[2] == blob
        assert _check(prog, n, cap, inputs, stream=s.cuda_stream)[2] == blob
        # a call on the second stream, then the matcher, a pose call and a trajectory call on the first, which overwrite what it
        # reads: each waits for it
        import trajectory_cases as tc
        prog.landmarks_consecutive(n, stream=s.cuda_stream, **INTR)
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        assert _check(prog, n, cap, inputs, call=False)[2] == blob
        tc.inject_pose(prog, b["matches"], b["poses"], b["points"])  # the calls above wrote their own
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, stream=s.cuda_stream, **INTR)
        prog.trajectory_consecutive(n, min_shared=10000)  # every joint RESTART_FEW: other frame records
        assert _check(prog, n, cap, inputs, call=False)[2] == blob
        few = _inputs(prog, n, cap)
        assert few[4]["status"].tolist() == [ORIGIN, START, FEW, FEW, FEW]
        assert _check(prog, n, cap, few)[0]["longest"].tolist() == [2, 2, 2, 2]
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        assert code() == T.ORB_ESTATE  # match and pose are fresh, the trajectory is not
        prog.trajectory_consecutive(n)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, n, cap, _inputs(prog, n, cap))  # fresh again: parity on the new batch's own (empty) records
