"""The localisation stage on the GPU (orb_localize_consecutive): every OrbFrameFix byte and every inlier byte
against the CPU restatement (tests/localize_ref.py) fed with the device's own counts, records, matches, pose records and points, on
hand-built batches (tests/localize_cases.py) of 64 x 48 frames: every status, the sample-size and tile edges of the number of
correspondences, the block edges of the number of hypotheses, each parameter, raw counters above the capacity; the other stages'
results untouched; the call's state, argument and stream rules."""
import numpy as np
import pytest

import constructed as C
import localize_cases as lc
import localize_ref as lr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _inputs(prog, n_frames, cap):
    """What the call reads, as the device holds it: stored counts and records, the matcher's records, the pose records and points."""
    counts = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    poses = [prog.pose_read(f, cap) for f in range(n_frames - 1)]
    return counts, corners, matches, [p[0] for p in poses], [p[1] for p in poses]


def _check(prog, n_frames, cap, inputs, stream=None, call=True, **params):
    """Localize call, then every pair's record and cap inlier bytes against the restatement, byte for byte.  Returns the device's
    records (FIX_DTYPE (n_frames - 1,)) and the bytes of everything read."""
    counts, corners, matches, poses, points = inputs
    if call:
        prog.localize_consecutive(n_frames, stream=stream, **INTR, **params)
    want, wmask = lr.localize(counts, corners, matches, poses, points, cap, n_frames=n_frames, **INTR, **params)
    recs, blob = [], b""
    for f in range(n_frames - 1):
        got, mask = prog.localize_read(f, cap)
        assert got.tobytes() == want[f].tobytes(), (f, params, got, want[f])
        if mask.tobytes() != wmask[f].tobytes():
            bad = np.nonzero(mask != wmask[f])[0]
            raise AssertionError((f, params, bad[:8], mask[bad[:8]], wmask[f][bad[:8]]))
        assert int(mask.sum()) == int(got["inliers"])
        recs.append(got)
        blob += got.tobytes() + mask.tobytes()
    return np.array(recs), blob


def _status_batch(cap):
    """Twelve frames: a five-view path with wrong, far, close and lost matches and points without flags; a plane (three views); a
    cloud whose matches are all wrong (three views); an empty frame.  The pairs between the runs carry the matches of unrelated
    scenes."""
    rng = np.random.default_rng(2026)
    runs = [lc.views(rng, 5, 500, cap, wrong=0.1, far=0.05, close=0.05, lost=0.05, bad_points=0.05, noise=0.002),
            lc.views(rng, 3, 200, cap, shape="plane"), lc.views(rng, 3, 150, cap, wrong=1.0), lc.views(rng, 1, 0, cap)]
    return lc.join(runs, bridge=True)


def test_every_status_parameters_and_extents(tinyorb):
    """Capacity 1100 (no multiple of 64 or 256), twelve frames, every status; NOMAP behind a call that wrote the same pair; each
    parameter and a second seed; hypotheses at the block edges; n_frames 3 and the whole batch."""
    T = tinyorb
    cap = 1100
    b = _status_batch(cap)
    B = b["n"]
    OK, NOMAP, FEW, DEG, MIN = T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_NOMAP, T.ORB_LOCALIZE_FEW, T.ORB_LOCALIZE_DEGENERATE, T.ORB_LOCALIZE_MINIMAL
    with _program(T, cap, 12) as prog:
        lc.inject(prog, b)
        inputs = _inputs(prog, B, cap)
        assert B == 12 and inputs[0].tolist() == lc.stored(b).tolist()
        base, blob = _check(prog, B, cap, inputs)
        print("statuses", base["status"].tolist(), "candidates", base["candidates"].tolist(), "inliers", base["inliers"].tolist(),
              "step", base["step"].tolist())
        st = base["status"].tolist()
        assert st[:4] == [NOMAP, OK, OK, OK] and st[5] == NOMAP and st[6] == DEG and st[8] == NOMAP and st[10] == FEW
        assert base["candidates"][4] > 100 and base["candidates"][9] > 50  # the unrelated scenes, the wrong matches: a RANSAC ran
        assert (base["candidates"][1:4] > 150).all() and (2 * base["inliers"][1:4] > base["candidates"][1:4]).all()
        true = [np.linalg.norm(b["steps"][f][1]) / np.linalg.norm(b["steps"][f - 1][1]) for f in range(1, 4)]
        assert np.allclose(base["step"][1:4], true, rtol=0.2)
        for f in (0, 5, 6, 8, 10):  # NOMAP, DEGENERATE and FEW write zeros and the status
            z = np.zeros((), T.FIX_DTYPE)
            z["status"] = st[f]
            assert base[f].tobytes() == z.tobytes()
        # each parameter, against the restatement; what it moves
        seed2, _ = _check(prog, B, cap, inputs, seed=12345)
        assert (seed2["hypothesis"][1:4] != base["hypothesis"][1:4]).any() and seed2["status"].tolist()[:4] == st[:4]
        tight, _ = _check(prog, B, cap, inputs, max_reproj_px=0.5)
        assert (tight["inliers"][1:4] < base["inliers"][1:4]).all()
        wide, _ = _check(prog, B, cap, inputs, max_reproj_px=1000.0, seed=3)
        assert MIN in wide["status"].tolist()  # a refit over everything in front of the camera
        tiny, _ = _check(prog, B, cap, inputs, max_reproj_px=1e-6)
        assert (tiny["status"][1:4] == MIN).all() and not tiny["inliers"][1:4].any()  # no inlier: the solve fails
        near, _ = _check(prog, B, cap, inputs, max_distance=10)
        assert (near["candidates"][1:4] < base["candidates"][1:4]).all()
        far, _ = _check(prog, B, cap, inputs, max_distance=256, ratio=10.0)
        assert (far["candidates"][1:4] > base["candidates"][1:4]).all()
        ratio, _ = _check(prog, B, cap, inputs, ratio=0.1)
        assert (ratio["candidates"][1:4] < base["candidates"][1:4]).all()
        for hyps in (1, 64, 65, 512):
            res, _ = _check(prog, B, cap, inputs, hypotheses=hyps, seed=9)
            assert (res["hypothesis"] < hyps).all()
        # n_frames 3: the same leading records; a pair beyond the call is an error
        part, pblob = _check(prog, 3, cap, inputs)
        assert part.tobytes() == base[:2].tobytes() and pblob == blob[:len(pblob)]
        with pytest.raises(T.OrbError) as e:
            prog.localize_read(2, cap)
        assert e.value.code == T.ORB_EINVAL
        again, ablob = _check(prog, B, cap, inputs)
        assert ablob == blob
        # NOMAP behind a call that wrote the same pair: pair 1's pose stops being OK; stale records, bytes or keys would show
        import trajectory_cases as tc
        poses = b["poses"].copy()
        poses["status"][0] = T.ORB_POSE_LOW_PARALLAX
        tc.inject_pose(prog, poses=poses)
        lost, _ = _check(prog, B, cap, _inputs(prog, B, cap))
        assert lost["status"].tolist() == [NOMAP, NOMAP] + st[2:] and lost[2:].tobytes() == base[2:].tobytes()


@pytest.mark.parametrize("cap,land,sizes", [(64, 90, (5, 6, 7)), (1100, 450, (255, 256, 257))])
def test_sample_size_and_tile_edges(tinyorb, cap, land, sizes):
    """Capacity 64 with 5, 6 and 7 correspondences (FEW, the first sample, one to spare) and raw counters above the capacity;
    capacity 1100 with 255, 256 and 257 (the edges of the 256-candidate tiles and of the 256 partial sums)."""
    T = tinyorb
    rng = np.random.default_rng(100 + cap)
    runs = [lc.trim(lc.views(rng, 3, land, cap, noise=0.002, extra=9 + M), 1, M, rng) for M in sizes]
    b = lc.join(runs)
    with _program(T, cap, 9) as prog:
        lc.inject(prog, b)
        inputs = _inputs(prog, b["n"], cap)
        raw = prog.batch_counts(b["n"])
        if cap == 64:
            assert (raw > cap).all() and (inputs[0] == cap).all()
        res, _ = _check(prog, b["n"], cap, inputs)
        print(cap, "statuses", res["status"].tolist(), "candidates", res["candidates"].tolist(), "inliers", res["inliers"].tolist())
        for c, M in enumerate(sizes):
            r = res[3 * c + 1]
            if M < 6:
                assert r["status"] == T.ORB_LOCALIZE_FEW and r["candidates"] == 0
            else:
                assert r["status"] in (T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_MINIMAL) and r["candidates"] == M
        _check(prog, b["n"], cap, inputs, hypotheses=65, seed=7, max_reproj_px=3.0)
        if cap > 64:
            assert (res["status"][[1, 4, 7]] == T.ORB_LOCALIZE_OK).all() and (res["inliers"][[1, 4, 7]] > 200).all()


def test_isolation_state_arguments_and_ordering(tinyorb):
    import torch
    T = tinyorb
    cap, n = 300, 5
    b = lc.views(np.random.default_rng(77), n, 250, cap, wrong=0.1, noise=0.002)

    def code(n_frames=n, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.localize_consecutive(n_frames, **{**INTR, **kw})
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.localize_read(0, cap)  # no localize call yet
        assert e.value.code == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # no match
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        assert code() == T.ORB_ESTATE  # before a pose call
        lc.inject(prog, b)  # match -> verify_epipolar -> pose on a new batch, then the arrays
        inf, nan = float("inf"), float("nan")
        for kw in (dict(n_frames=2), dict(n_frames=0), dict(n_frames=n + 1), dict(reserved=(0, 0, 1, 0, 0, 0, 0)), dict(reserved=(1, 0, 0, 0, 0, 0, 0)),
                   dict(reserved=(0, 0, 0, 0, 0, 0, 7)), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf), dict(cx=nan), dict(cy=inf),
                   dict(max_reproj_px=-1.0), dict(max_reproj_px=nan), dict(max_reproj_px=inf), dict(hypotheses=4097), dict(max_distance=257),
                   dict(ratio=-0.5), dict(ratio=nan), dict(ratio=inf)):
            assert code(**kw) == T.ORB_EINVAL, kw
        L = T.load_library()
        assert L.orb_localize_consecutive(prog._handle(), n, None, None) == T.ORB_EINVAL  # NULL params: the intrinsics have no default
        zero = T.OrbLocalizeParams()
        assert L.orb_localize_consecutive(prog._handle(), n, zero, None) == T.ORB_EINVAL  # a zero-initialised struct is not valid
        prog.pose_consecutive(3, **INTR)
        assert code(n_frames=4) == T.ORB_EINVAL  # three pairs asked for, two posed
        prog.pose_consecutive(n, **INTR)
        import trajectory_cases as tc
        tc.inject_pose(prog, b["matches"], b["poses"], b["points"])  # the pose calls above wrote their own
        inputs = _inputs(prog, n, cap)
        one, blob = _check(prog, n, cap, inputs, hypotheses=4096)
        one, blob = _check(prog, n, cap, inputs)
        assert one["status"].tolist() == [T.ORB_LOCALIZE_NOMAP] + [T.ORB_LOCALIZE_OK] * 3
        # read errors
        with pytest.raises(T.OrbError) as e:
            prog.localize_read(n - 1, cap)
        assert e.value.code == T.ORB_EINVAL
        import ctypes
        assert L.orb_localize_read(prog._handle(), 0, None, None, 5) == T.ORB_EINVAL  # inliers NULL with n > 0
        assert L.orb_localize_read(prog._handle(), 0, None, None, 0) == T.ORB_OK
        assert len(prog.localize_read(1, cap + 100)[1]) == cap and len(prog.localize_read(1)[1]) == cap and len(prog.localize_read(1, 7)[1]) == 7
        C.check_read_arguments(T, prog, L.orb_localize_read, n - 1, 1, head=True)
        # isolation: the other stages' read-backs before and after localize calls
        prog.verify_consecutive(n, inlier_px=2.0)
        prog.trajectory_consecutive(n)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                    prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() for f in range(n - 1)]

        before = others()
        _check(prog, n, cap, inputs)
        _check(prog, 3, cap, inputs, max_reproj_px=1.0, hypotheses=100, seed=5)
        assert others() == before
        # ordering: a call on a second stream, then the trajectory stage on the first (another reader: no wait), then a call on the
        # first stream again, which waits for the one on the second before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.localize_consecutive(n, stream=s.cuda_stream, **INTR)
        prog.trajectory_consecutive(n)
        assert _check(prog, n, cap, inputs, call=False)[1] == blob
        assert _check(prog, n, cap, inputs)[1] == blob
        assert _check(prog, n, cap, inputs, stream=s.cuda_stream)[1] == blob
        # a call on the second stream, then the matcher and a pose call on the first, which overwrite what it read: they wait
        prog.localize_consecutive(n, stream=s.cuda_stream, **INTR)
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        assert _check(prog, n, cap, inputs, call=False)[1] == blob
        # a new batch, or another output set: the pose call is stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        assert code() == T.ORB_ESTATE  # the match is fresh, the pose call is not
        prog.pose_consecutive(n, **INTR)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, n, cap, _inputs(prog, n, cap))  # fresh again: parity on the new batch's own (empty) records
