"""The trajectory stage on the GPU (orb_trajectory_consecutive): every OrbFramePose and every map OrbPoint byte
against the CPU restatement (tests/trajectory_ref.py) fed with the device's own counts, matches, pose records and points, on
constructed camera paths at two capacities; parameters that move the verdicts; the other stages' results untouched; the call's state,
argument and stream rules."""
import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import trajectory_ref as tr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 640, 480, 500.0
INTR0 = dict(fx=FOCAL, fy=FOCAL, cx=(W0 - 1) / 2, cy=(H0 - 1) / 2)


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _inject(prog, scenes, cap, extra=None):
    """The scenes' frames one after the other; `extra`: {frame: raw counter above the stored records}.  Returns the frames."""
    cor = [c[:cap] for s in scenes for c in s["corners"]]
    desc = [d[:cap] for s in scenes for d in s["desc"]]
    counts = np.array([len(c) for s in scenes for c in s["corners"]], np.uint32)
    for f, e in (extra or {}).items():
        counts[f] += e
    prog.extract_batch_host(np.zeros((len(counts), H0, W0, 4), np.uint8))
    C.inject(prog, counts, cor, desc)
    return len(counts)


def _pipeline(prog, B):
    prog.match_consecutive(B)
    prog.verify_epipolar(B, inlier_px=2.0)
    prog.pose_consecutive(B, **INTR0)


def _inputs(prog, n_frames, cap):
    """What the call reads, as the device holds it: stored counts, the matcher's records, the pose records and points."""
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    poses = [prog.pose_read(f, cap) for f in range(n_frames - 1)]
    return counts, matches, [p[0] for p in poses], [p[1] for p in poses]


def _check(prog, n_frames, cap, inputs, stream=None, call=True, **params):
    """Trajectory call, then every frame's record and cap map points against the restatement, byte for byte.  Returns the device's
    records (FRAME_POSE_DTYPE (n_frames,)) and the bytes of everything read."""
    counts, matches, poses, points = inputs
    if call:
        prog.trajectory_consecutive(n_frames, stream=stream, **params)
    want, wmap = tr.trajectory(counts[:n_frames], matches[:n_frames - 1], poses[:n_frames - 1], points[:n_frames - 1], cap, **params)
    recs, blob = [], b""
    for f in range(n_frames):
        got, pts = prog.trajectory_read(f, cap)
        assert got.tobytes() == want[f].tobytes(), (f, params, got, want[f])
        if pts.tobytes() != wmap[f].tobytes():
            bad = np.nonzero(pts != wmap[f])[0]
            raise AssertionError((f, params, bad[:5], pts[bad[:5]], wmap[f][bad[:5]]))
        recs.append(got)
        blob += got.tobytes() + pts.tobytes()
    return np.array(recs), blob


def _big_batch(cap):
    """Ten frames: a 6-frame sideways path, an unrelated two-view scene with `cap` stored records and raw counters above the capacity,
    and an outliers-only pair."""
    rng = np.random.default_rng(2026)
    scenes = [tr.path_scene(rng, tr.path_steps("sideways"), W0, H0, FOCAL), er.scene(rng, "forward", n=1400, count=cap),
              er.scene(rng, "sideways", outlier_share=1.0, n=300)]
    return scenes, {6: 37, 7: 5}


def test_parity_constructed_and_parameters(tinyorb):
    """640 x 480, capacity 1100 (no multiple of 64 or 1024; two map workgroups per pair), ten frames: ORIGIN, START, four CHAINED, LOST
    where the path ends, START on the two-view scene, LOST twice.  Then the parameters, each against the restatement."""
    T = tinyorb
    cap = 1100
    scenes, extra = _big_batch(cap)
    with _program(T, cap, 10) as prog:
        B = _inject(prog, scenes, cap, extra)
        assert B == 10
        _pipeline(prog, B)
        inputs = _inputs(prog, B, cap)
        assert prog.batch_counts(B)[6] == cap + 37 and inputs[0][6] == cap
        base, blob = _check(prog, B, cap, inputs)
        print("statuses", base["status"].tolist(), "shared", base["shared"].tolist(), "consistent", base["consistent"].tolist(), "step", base["step"].tolist())
        assert base["status"].tolist() == [T.ORB_TRAJ_ORIGIN, T.ORB_TRAJ_START] + [T.ORB_TRAJ_CHAINED] * 4 + \
            [T.ORB_TRAJ_LOST, T.ORB_TRAJ_START, T.ORB_TRAJ_LOST, T.ORB_TRAJ_LOST]
        assert base["origin"].tolist() == [0, 0, 0, 0, 0, 0, 6, 6, 8, 9]
        assert (base["shared"][2:6] > 100).all()
        joints = slice(2, 6)  # the frames behind an evaluated joint
        few, _ = _check(prog, B, cap, inputs, min_shared=5000)
        assert (few["status"][joints] == T.ORB_TRAJ_RESTART_FEW).all() and (few["shared"] == base["shared"]).all() and not few["step"].any()
        assert few["origin"].tolist() == [0, 0, 1, 2, 3, 4, 6, 6, 8, 9]
        spread, _ = _check(prog, B, cap, inputs, scale_tolerance=1e-7)
        assert (spread["status"][joints] == T.ORB_TRAJ_RESTART_SPREAD).all() and (spread["step"] == base["step"]).all()
        assert (spread["consistent"][joints] < 10).all()
        strict, _ = _check(prog, B, cap, inputs, consistent_permille=1000)
        for r in strict[joints]:
            assert r["status"] == (T.ORB_TRAJ_CHAINED if r["consistent"] == r["shared"] else T.ORB_TRAJ_RESTART_SPREAD)
        lax, _ = _check(prog, B, cap, inputs, consistent_permille=1, scale_tolerance=0.001)
        assert (lax["status"][joints] == T.ORB_TRAJ_CHAINED).all() and (lax["consistent"][joints] < base["consistent"][joints]).all()
        par, _ = _check(prog, B, cap, inputs, flags=T.ORB_TRAJ_NEED_PARALLAX)
        assert (par["shared"] <= base["shared"]).all()
        # n_frames = 2, 3 and the whole batch: the same leading records and map rows, except the row that is now the last frame's
        for n in (2, 3):
            part, pblob = _check(prog, n, cap, inputs)
            assert part.tobytes() == base[:n].tobytes()
            row = len(blob) // B
            assert pblob[:row * (n - 1)] == blob[:row * (n - 1)]
            with pytest.raises(T.OrbError) as e:
                prog.trajectory_read(n, cap)
            assert e.value.code == T.ORB_EINVAL
        again, ablob = _check(prog, B, cap, inputs)
        assert ablob == blob


@pytest.mark.parametrize("count", [8, 63, 64, 65])
def test_parity_wave_and_workgroup_edges(tinyorb, count):
    """Capacity 64 and paths cut to 8, 63, 64 and 65 records (65: the raw counter above the capacity, 64 records stored): the edges
    of the ballot counts, and histograms with very few entries."""
    cap = 64
    rng = np.random.default_rng(500 + count)
    scene = tr.path_scene(rng, tr.path_steps("sideways"), W0, H0, FOCAL, count=count, outlier_share=0.1)
    with _program(tinyorb, cap, 6) as prog:
        B = _inject(prog, [scene], cap)
        _pipeline(prog, B)
        inputs = _inputs(prog, B, cap)
        res, _ = _check(prog, B, cap, inputs)
        print(count, "statuses", res["status"].tolist(), "shared", res["shared"].tolist(), "consistent", res["consistent"].tolist())
        _check(prog, B, cap, inputs, min_shared=1, consistent_permille=1)
        if count >= 63:
            assert (res["shared"] > 0).any()
        # a pose stage that accepts nearly anything: joints of a handful of ratios (eight records give no OK pose otherwise)
        prog.pose_consecutive(B, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **INTR0)
        inputs = _inputs(prog, B, cap)
        _check(prog, B, cap, inputs)
        loose, _ = _check(prog, B, cap, inputs, min_shared=1, consistent_permille=1)
        print(count, "loose pose: statuses", loose["status"].tolist(), "shared", loose["shared"].tolist(), "consistent", loose["consistent"].tolist())
        assert (loose["shared"] > 0).any()


def test_isolation_state_arguments_and_ordering(tinyorb):
    import torch
    T = tinyorb
    cap = 700
    rng = np.random.default_rng(77)
    scene = tr.path_scene(rng, tr.path_steps("sideways")[:3], W0, H0, FOCAL, n=700)
    n = 4

    def code(n_frames=n, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.trajectory_consecutive(n_frames, **kw)
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.trajectory_read(0, cap)  # no trajectory call yet
        assert e.value.code == T.ORB_ESTATE
        B = _inject(prog, [scene], cap)
        assert B == n and code() == T.ORB_ESTATE  # no match
        prog.match_consecutive(n)
        prog.verify_epipolar(n, inlier_px=2.0)
        assert code() == T.ORB_ESTATE  # before a pose call
        prog.pose_consecutive(n, **INTR0)
        inf, nan = float("inf"), float("nan")
        for kw in (dict(n_frames=1), dict(n_frames=0), dict(n_frames=n + 1), dict(reserved=(0, 0, 1, 0)), dict(reserved=(1, 0, 0, 0)),
                   dict(reserved=(0, 0, 0, 7)), dict(flags=2), dict(flags=0x80000001), dict(scale_tolerance=nan), dict(scale_tolerance=inf),
                   dict(scale_tolerance=-0.5), dict(consistent_permille=1001)):
            assert code(**kw) == T.ORB_EINVAL, kw
        prog.pose_consecutive(3, **INTR0)
        assert code(n_frames=4) == T.ORB_EINVAL  # three pairs asked for, two posed
        prog.pose_consecutive(n, **INTR0)
        L = T.load_library()
        assert L.orb_trajectory_consecutive(prog._handle(), n, None, None) == T.ORB_OK  # NULL params: the defaults
        inputs = _inputs(prog, n, cap)
        one, blob = _check(prog, n, cap, inputs, call=False)
        assert one["status"].tolist() == [T.ORB_TRAJ_ORIGIN, T.ORB_TRAJ_START, T.ORB_TRAJ_CHAINED, T.ORB_TRAJ_CHAINED]
        # read errors
        for args in ((n, cap),):
            with pytest.raises(T.OrbError) as e:
                prog.trajectory_read(*args)
            assert e.value.code == T.ORB_EINVAL
        assert L.orb_trajectory_read(prog._handle(), 0, None, None, 5) == T.ORB_EINVAL  # points NULL with n > 0
        assert L.orb_trajectory_read(prog._handle(), 0, None, None, 0) == T.ORB_OK
        assert len(prog.trajectory_read(0, cap + 100)[1]) == cap and len(prog.trajectory_read(0)[1]) == cap
        C.check_read_arguments(T, prog, L.orb_trajectory_read, n, 16, head=True)
        # isolation: the other stages' read-backs before and after trajectory calls
        prog.verify_consecutive(n, inlier_px=2.0)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() for f in range(n - 1)]

        before = others()
        _check(prog, n, cap, inputs)
        _check(prog, 3, cap, inputs, scale_tolerance=0.01, min_shared=3)
        assert others() == before
        # ordering: a call on a second stream, then a pose call and the matcher on the first, which overwrite what it read: they wait
        s = torch.cuda.Stream(device=0)
        prog.trajectory_consecutive(n, stream=s.cuda_stream)
        prog.pose_consecutive(n, **INTR0)
        prog.match_consecutive(n)
        assert _check(prog, n, cap, inputs, call=False)[1] == blob
        assert _check(prog, n, cap, _inputs(prog, n, cap), stream=s.cuda_stream)[1] == blob  # behind them, on the other stream
        # a new batch, or another output set: the pose call is stale
        B = _inject(prog, [scene], cap)
        assert code() == T.ORB_ESTATE
        prog.match_consecutive(n)
        prog.verify_epipolar(n, inlier_px=2.0)
        assert code() == T.ORB_ESTATE  # the match is fresh, the pose call is not
        prog.pose_consecutive(n, **INTR0)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, n, cap, _inputs(prog, n, cap))  # fresh again: parity on the new batch's own records
