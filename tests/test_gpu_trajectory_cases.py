"""The hand-built cases of tests/trajectory_cases.py on the GPU: orb_trajectory_consecutive fed through orb_debug_pose_buffers, every
OrbFramePose and every map OrbPoint byte against the CPU restatement (tests/trajectory_ref.py) of the same arrays, and the outcome
each construction implies on the device's own records.  No tolerance anywhere.

The images are zeros at 64 x 48 with two levels, the smallest extent the GPU suite extracts at elsewhere (tests/golden/g64x48_d2):
the match, epipolar and pose stages run once on empty frames, only to be fresh; what the trajectory call reads is then written over
their buffers."""
import time

import numpy as np
import pytest

import trajectory_cases as tc

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48


def _program(tinyorb, cap, max_batch):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=max_batch)
    return tinyorb.OrbProgram(cfg).init()


def _compare(prog, b, n_frames=None, call=True, **params):
    """A trajectory call on the batch the program holds; every frame's record and every map point against the restatement of b's
    arrays, byte for byte.  Returns the device's records (FRAME_POSE_DTYPE (n,)) and map (POINT_DTYPE (n, cap))."""
    n, cap = b["n"] if n_frames is None else n_frames, b["cap"]
    if call:
        prog.trajectory_consecutive(n, **params)
    want, wmap = tc.reference(b, n, **params)
    got = [prog.trajectory_read(f, cap) for f in range(n)]
    recs, world = np.array([g[0] for g in got]), np.stack([g[1] for g in got])
    if recs.tobytes() != want.tobytes():
        f = next(f for f in range(n) if recs[f].tobytes() != want[f].tobytes())
        raise AssertionError(("frame record", f, params, recs[f], want[f]))
    if world.tobytes() != wmap.tobytes():
        f = next(f for f in range(n) if world[f].tobytes() != wmap[f].tobytes())
        bad = np.nonzero(world[f].view(np.uint32).reshape(cap, 4) != wmap[f].view(np.uint32).reshape(cap, 4))[0]
        raise AssertionError(("map row", f, params, bad[:5], world[f][bad[:5]], wmap[f][bad[:5]]))
    return recs, world


@pytest.mark.parametrize("cap", [64, 1100, 2049])
def test_packed_joints(tinyorb, cap):
    """Every joint case that fits the capacity in one batch of 3 k + 1 frames (trajectory_cases.pack), one call per parameter set
    of the cases.  64: one wave's worth of slots; 1100: two strided passes of the 1024 threads and a tail that is no multiple of
    64; 2049: three passes and a tail of one."""
    t0 = time.perf_counter()
    cases = tc.joint_cases(cap)
    b = tc.pack(cases, cap)
    with _program(tinyorb, cap, b["n"]) as prog:
        tc.prepare(prog, b["n"], W0, H0)
        tc.inject_batch(prog, b)
        assert list(prog.batch_counts(b["n"])) == list(b["counts"])
        checked = 0
        for ps in tc.param_sets(cases):
            recs, _ = _compare(prog, b, **ps)
            for c, f in zip(cases, b["joint"]):
                if c["params"] == ps:
                    tc.check_expect(c, recs[f])
                    checked += 1
        assert checked == len(cases)
    print("capacity %d: %d cases, %d frames, %d parameter sets, %.2f s" % (cap, len(cases), b["n"], len(tc.param_sets(cases)), time.perf_counter() - t0))


def test_chain_of_260_frames(tinyorb):
    """Five chunks of k_traj_chain's staging, the last of three frames: CHAINED runs across every chunk edge with the scale running
    to inf and to 0 and the compositions whose det is 0, < 0 and not finite in between, then LOST, START and both RESTARTs on the
    frames next to the edges; and calls that end one frame behind an edge and one before."""
    t0 = time.perf_counter()
    runs, plan, notes = tc.chain_runs()
    edges, eplan = tc.chain_edges()
    with _program(tinyorb, tc.CHAIN_CAP, tc.CHAIN_FRAMES) as prog:
        tc.prepare(prog, tc.CHAIN_FRAMES, W0, H0)
        tc.inject_batch(prog, runs)
        recs, world = _compare(prog, runs)
        assert recs["status"].tolist() == plan
        assert recs["scale"][notes["scale inf"]] == np.inf and np.isinf(world[notes["scale inf"] - 1]["x"][:12]).all()
        s0 = notes["scale 0"]
        assert recs["scale"][s0] == 0 and 0 < recs["scale"][s0 - 1] < np.float32(1.2e-38) and recs["scale"][s0 + 1] == 0
        assert not recs["r"][notes["det 0"]].any()
        assert np.linalg.det(recs["r"][notes["det < 0"]].astype(np.float64).reshape(3, 3)) < -0.99
        assert np.abs(recs["r"][notes["det not finite"]]).max() > 1e19
        for n in (65, 66, 129, 2):
            part, _ = _compare(prog, runs, n_frames=n)
            assert part.tobytes() == recs[:n].tobytes()
        tc.inject_batch(prog, edges)
        recs, world = _compare(prog, edges)
        assert recs["status"].tolist() == eplan
        assert recs["shared"][192] == 3 and recs["shared"][193] == 12 and recs["shared"][257] == 3
        assert not world[63].tobytes().strip(b"\0") and world[64].tobytes() == edges["points"][64].tobytes()
    print("260 frames: %.2f s" % (time.perf_counter() - t0))


def test_chain_of_4096_frames(tinyorb):
    """The longest batch the call accepts, at capacity 8 (64 chunks): one small rotation, every frame from the third on CHAINED."""
    t0 = time.perf_counter()
    n = 4096
    b, _ = tc.long_chain(n)
    with _program(tinyorb, b["cap"], n) as prog:
        tc.prepare(prog, n, W0, H0)
        tc.inject_batch(prog, b)
        recs, _ = _compare(prog, b)
        assert (recs["status"][2:] == tc.CHAINED).all() and (recs["origin"] == 0).all() and (recs["shared"][2:] == 8).all()
        with pytest.raises(tinyorb.OrbError) as e:
            prog.trajectory_consecutive(n + 1)
        assert e.value.code == tinyorb.ORB_EINVAL
    print("4096 frames: %.2f s" % (time.perf_counter() - t0))


def test_stale_joints_and_map_rows(tinyorb):
    """Three calls on one program.  Every pair OK; then three poses overwritten to not OK: the joints next to them are not evaluated
    and keep the first call's HOLDS rows, which the chain must not use (START with no counts), and the map rows of the LOST frames,
    which held transformed points, must be zeros; then fewer frames: the row of what is now the last frame is zeros."""
    t0 = time.perf_counter()
    T = tinyorb
    n = 14
    b, plan = tc.steady_chain(n)
    with _program(T, tc.CHAIN_CAP, n) as prog:
        with pytest.raises(T.OrbError) as e:
            prog.debug_pose_buffers()
        assert e.value.code == T.ORB_ESTATE  # nothing allocated yet
        tc.prepare(prog, n, W0, H0)
        assert all(prog.debug_pose_buffers())
        L = T.load_library()
        assert L.orb_debug_pose_buffers(prog._handle(), None, None, None) == T.ORB_OK  # every out-pointer may be NULL
        tc.inject_batch(prog, b)
        first, fmap = _compare(prog, b)
        assert first["status"].tolist() == plan and (first["shared"][2:] == 12).all()
        assert all(fmap[f].tobytes().strip(b"\0") for f in range(1, n - 1))
        lost = dict(b, poses=b["poses"].copy())
        for p, status in ((4, T.ORB_POSE_FEW), (5, T.ORB_POSE_AMBIGUOUS), (9, T.ORB_POSE_NOMODEL)):
            lost["poses"][p]["status"] = status
        tc.inject_pose(prog, poses=lost["poses"])
        second, smap = _compare(prog, lost)
        want = list(plan)
        want[5], want[6], want[7], want[10], want[11] = tc.LOST, tc.LOST, tc.START, tc.LOST, tc.START
        assert second["status"].tolist() == want
        assert not second["shared"][[5, 6, 7, 10, 11]].any() and not second["consistent"][[5, 6, 7, 10, 11]].any()
        assert second["origin"].tolist() == [0] * 5 + [5, 6, 6, 6, 6, 10, 10, 10, 10]
        for f in (4, 5, 9):
            assert not smap[f].tobytes().strip(b"\0")
        third, tmap = _compare(prog, lost, n_frames=4)
        assert third.tobytes() == second[:4].tobytes() and tmap[:3].tobytes() == smap[:3].tobytes() and not tmap[3].tobytes().strip(b"\0")
        with pytest.raises(T.OrbError) as e:
            prog.trajectory_read(4, tc.CHAIN_CAP)
        assert e.value.code == T.ORB_EINVAL
        tc.inject_pose(prog, poses=b["poses"])
        again, amap = _compare(prog, b)
        assert again.tobytes() == first.tobytes() and amap.tobytes() == fmap.tobytes()
    print("stale state: %.2f s" % (time.perf_counter() - t0))
