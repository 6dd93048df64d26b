"""Relative pose recovery and triangulation on the GPU (orb_pose_consecutive): every OrbPairPose and OrbPoint
byte against the CPU restatement (tests/pose_ref.py) on constructed two-view scenes at two capacities and on extracted two-layer
views; parameters that move the status; the other stages' results untouched; the call's state, argument and stream rules."""
import ctypes

import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import pose_ref as pr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 640, 480, 500.0
INTR0 = dict(fx=FOCAL, fy=FOCAL, cx=(W0 - 1) / 2, cy=(H0 - 1) / 2)
W1, H1 = 320, 240
INTR1 = dict(fx=300.0, fy=310.0, cx=158.0, cy=121.5)
SHIFT_FAR, SHIFT_NEAR = np.array([2.0, 1.0]), np.array([12.0, 6.0])  # per frame, along one direction: a sideways camera


def _program(tinyorb, W, H, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch,
                            flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


def _two_layer_views(oracle, W, H, n):
    """test_gpu_epipolar's views of two textured planes from a camera that translates along (2, 1): the far plane (rows < H / 2)
    moves by SHIFT_FAR px per frame, the near one by SHIFT_NEAR."""
    pad = 8 + int(SHIFT_NEAR.max()) * n
    far, near = oracle.synth_frame(W + pad, H + pad, 4001), oracle.synth_frame(W + pad, H + pad, 4002)
    views = np.empty((n, H, W, 4), np.uint8)
    for i in range(n):
        for tex, s, rows in ((far, SHIFT_FAR, slice(0, H // 2)), (near, SHIFT_NEAR, slice(H // 2, H))):
            ox, oy = (s * i).astype(int)
            views[i, rows] = tex[oy:oy + H, ox:ox + W][rows]
    return views


def _inputs(prog, n_frames, cap):
    """What the pose call reads, as the device holds it: stored corners, the matcher's records, the epipolar records and bytes."""
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(counts[f])) for f in range(n_frames - 1)]
    epi = [prog.verify_epipolar_read(f, cap) for f in range(n_frames - 1)]
    return corners, matches, epi


def _check(prog, n_frames, cap, inputs, intr, stream=None, call=True, **params):
    """Pose call, then every pair's record and cap points against the restatement, byte for byte.  Returns the device's records."""
    corners, matches, epi = inputs
    if call:
        prog.pose_consecutive(n_frames, stream=stream, **intr, **params)
    out = []
    for f in range(n_frames - 1):
        got, pts = prog.pose_read(f, cap)
        want, wpts = pr.pose_pair(corners[f], corners[f + 1], matches[f], epi[f][0], epi[f][1], cap=cap, **intr, **params)
        assert got.tobytes() == want.tobytes(), (f, params, got, want)
        if pts.tobytes() != wpts.tobytes():
            bad = np.nonzero(pts != wpts)[0]
            raise AssertionError((f, params, bad[:5], pts[bad[:5]], wpts[bad[:5]]))
        out.append((got, pts))
    return out


def _inject_scenes(prog, scenes, cap, extra=None):
    """Scene i in frames (2i, 2i + 1): the pairs between two scenes have no candidates.  `extra`: {frame: raw counter above the
    stored records}."""
    cor, desc, counts = [], [], []
    for s in scenes:
        cor += [c[:cap] for c in s["corners"]]
        desc += [d[:cap] for d in s["desc"]]
        counts += [len(s["corners"][0])] * 2
    counts = np.array(counts, np.uint32)
    for f, e in (extra or {}).items():
        counts[f] += e
    B = len(counts)
    prog.extract_batch_host(np.zeros((B, H0, W0, 4), np.uint8))
    C.inject(prog, counts, cor, desc)
    return B


def test_parity_constructed(tinyorb):
    """640 x 480, capacity 1100 (no multiple of 64 or 1024; two workgroups per pair): the three motions -- the forward one with 1100
    stored records and raw counters above the capacity -- a pair with 7 candidates and an outliers-only pair, each scene in two
    frames of its own (five scenes cannot share five frames: ten frames, the pairs between two scenes have no candidates)."""
    cap = 1100
    rng = np.random.default_rng(2025)
    scenes = [er.scene(rng, "sideways"), er.scene(rng, "yaw"), er.scene(rng, "forward", n=1400, count=cap),
              er.scene(rng, "forward", count=7), er.scene(rng, "sideways", outlier_share=1.0, n=300)]
    with _program(tinyorb, W0, H0, cap, 10) as prog:
        B = _inject_scenes(prog, scenes, cap, extra={4: 37, 5: 5})
        prog.match_consecutive(B)
        prog.verify_epipolar(B, inlier_px=2.0)
        inputs = _inputs(prog, B, cap)
        assert [int(e[0]["status"]) for e in inputs[2][0:6:2]] == [tinyorb.ORB_VERIFY_OK] * 3 and inputs[2][6][0]["status"] == tinyorb.ORB_VERIFY_FEW
        res = _check(prog, B, cap, inputs, INTR0)
        st = [int(r[0]["status"]) for r in res]
        print("statuses", st, "good", [int(r[0]["good"]) for r in res], "second", [int(r[0]["second"]) for r in res])
        assert st[0:6:2] == [tinyorb.ORB_POSE_OK] * 3 and all(s == tinyorb.ORB_POSE_NOMODEL for s in st[1::2]) and st[6] == tinyorb.ORB_POSE_NOMODEL
        assert all(r[0]["good"] > 500 for r in res[0:6:2]) and res[4][0]["inliers"] > 700
        for r, pts in res:
            assert int((pts["flags"] & tinyorb.ORB_POINT_GOOD != 0).sum()) == r["good"]
        # other parameters, other intrinsics (a principal point off the centre, fx != fy)
        _check(prog, B, cap, inputs, dict(fx=480.0, fy=510.0, cx=300.25, cy=250.5), max_reproj_px=0.75, max_cos_parallax=0.9999, min_good=30)


@pytest.mark.parametrize("count", [8, 63, 64, 65])
def test_parity_wave_and_workgroup_edges(tinyorb, count):
    """Capacity 64 and scenes cut to 8, 63, 64 and 65 correspondences (65: the raw counter above the capacity, 64 records stored)."""
    cap = 64
    rng = np.random.default_rng(300 + count)
    scenes = [er.scene(rng, m, count=count, outlier_share=0.1) for m in ("sideways", "yaw", "forward")]
    with _program(tinyorb, W0, H0, cap, 6) as prog:
        B = _inject_scenes(prog, scenes, cap)
        prog.match_consecutive(B)
        prog.verify_epipolar(B, inlier_px=2.0)
        inputs = _inputs(prog, B, cap)
        res = _check(prog, B, cap, inputs, INTR0)
        print(count, "statuses", [int(r[0]["status"]) for r in res], "inliers", [int(r[0]["inliers"]) for r in res])
        assert any(r[0]["status"] != tinyorb.ORB_POSE_NOMODEL for r in res)


def test_parity_extracted_and_parameters(tinyorb, oracle):
    """Intended mode, the two-layer views at 320 x 240, n_frames 3 and 2; then max_reproj_px and ambiguity_permille at their extremes
    move the status as the restatement says."""
    cap, n = 1500, 3
    frames = _two_layer_views(oracle, W1, H1, n)
    with _program(tinyorb, W1, H1, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(n)
        prog.verify_epipolar(n, inlier_px=2.0)
        inputs = _inputs(prog, n, cap)
        assert all(e[0]["status"] in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL) and e[0]["inliers"] > 100 for e in inputs[2])
        base = _check(prog, n, cap, inputs, INTR1)  # n_frames = the epipolar call's pairs + 1
        print("extracted", [(int(r["status"]), int(r["inliers"]), int(r["good"]), int(r["second"])) for r, _ in base])
        assert all(r["status"] != tinyorb.ORB_POSE_NOMODEL and r["good"] > 50 for r, _ in base)
        two = _check(prog, 2, cap, inputs, INTR1)  # n_frames 2: pair 0 alone, the same record
        assert two[0][0].tobytes() == base[0][0].tobytes() and two[0][1].tobytes() == base[0][1].tobytes()
        with pytest.raises(tinyorb.OrbError) as e:
            prog.pose_read(1, cap)  # one pair only
        assert e.value.code == tinyorb.ORB_EINVAL
        tiny = _check(prog, n, cap, inputs, INTR1, max_reproj_px=1e-6)
        assert all(r["status"] == tinyorb.ORB_POSE_FEW and r["good"] < 8 and r["inliers"] == b[0]["inliers"] for (r, _), b in zip(tiny, base))
        wide = _check(prog, n, cap, inputs, INTR1, max_reproj_px=1e6)
        assert all(r["good"] >= b[0]["good"] for (r, _), b in zip(wide, base))
        amb = _check(prog, n, cap, inputs, INTR1, ambiguity_permille=1)
        for (r, _), b in zip(amb, base):
            assert r["status"] == (tinyorb.ORB_POSE_AMBIGUOUS if 1000 * int(r["second"]) >= int(r["good"]) else b[0]["status"])
            assert r["r"].tobytes() == b[0]["r"].tobytes() and r["good"] == b[0]["good"]
        sure = _check(prog, n, cap, inputs, INTR1, ambiguity_permille=1000)
        assert all(r["status"] != tinyorb.ORB_POSE_AMBIGUOUS or r["second"] == r["good"] for r, _ in sure)
        flat = _check(prog, n, cap, inputs, INTR1, max_cos_parallax=0.5, ambiguity_permille=1000)
        assert all(r["status"] in (tinyorb.ORB_POSE_LOW_PARALLAX, tinyorb.ORB_POSE_AMBIGUOUS) for r, _ in flat)


def test_isolation_state_arguments_and_ordering(tinyorb, oracle):
    import torch
    cap, n = 800, 3
    frames = _two_layer_views(oracle, W1, H1, n)
    L = tinyorb.load_library()

    def code(n_frames=3, **kw):
        with pytest.raises(tinyorb.OrbError) as e:
            prog.pose_consecutive(n_frames, **{**INTR1, **kw})
        return e.value.code

    with _program(tinyorb, W1, H1, cap, n, tinyorb.ORB_FLAG_INTENDED | tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(tinyorb.OrbError) as e:
            prog.pose_read(0, cap)  # no pose call yet
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.extract_batch_host(frames)
        assert code() == tinyorb.ORB_ESTATE  # no match
        prog.match_consecutive(n)
        prog.verify_consecutive(n, inlier_px=2.0)
        assert code() == tinyorb.ORB_ESTATE  # before any epipolar call: the homography verifier is not the source
        prog.verify_epipolar(n, inlier_px=2.0, seed=3)
        inf, nan = float("inf"), float("nan")
        for kw in (dict(n_frames=1), dict(n_frames=4), dict(fx=0.0), dict(fx=-1.0), dict(fx=nan), dict(fx=inf), dict(fy=0.0), dict(fy=-300.0),
                   dict(fy=nan), dict(fy=inf), dict(cx=nan), dict(cx=inf), dict(cy=nan), dict(cy=-inf), dict(max_reproj_px=-1.0),
                   dict(max_reproj_px=nan), dict(max_reproj_px=inf), dict(max_cos_parallax=1.5), dict(max_cos_parallax=-0.5),
                   dict(max_cos_parallax=nan), dict(ambiguity_permille=1001)):
            assert code(**kw) == tinyorb.ORB_EINVAL, kw
        assert L.orb_pose_consecutive(prog._handle(), 3, None, None) == tinyorb.ORB_EINVAL  # NULL params
        prog.verify_epipolar(2, inlier_px=2.0, seed=3)
        assert code(n_frames=3) == tinyorb.ORB_EINVAL  # two pairs asked for, one verified
        prog.verify_epipolar(n, inlier_px=2.0, seed=3)
        # isolation: the other stages' read-backs before and after pose calls
        prog.match_guided(n, source=tinyorb.ORB_GUIDE_VERIFIED, radius_px=3.0)
        prog.match_epipolar(n, band_px=2.0, radius_px=24.0)
        prog.track_consecutive(n)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.match_guided_read(f, cap).tobytes() + prog.match_epipolar_read(f, cap).tobytes() + prog.track_read(f, cap).tobytes()
                    for f in range(n - 1)] + [prog.track_read(n - 1, cap).tobytes(), prog.track_frames(n).tobytes()]

        before = others()
        inputs = _inputs(prog, n, cap)
        one = [r.tobytes() + p.tobytes() for r, p in _check(prog, n, cap, inputs, INTR1)]
        C.check_read_arguments(tinyorb, prog, L.orb_pose_read, n - 1, 16, head=True)
        _check(prog, 2, cap, inputs, INTR1, max_reproj_px=0.5)
        assert others() == before
        # ordering: a pose call on a second stream, then an epipolar verification on the first that overwrites what it read: it waits
        s = torch.cuda.Stream(device=0)
        prog.pose_consecutive(n, stream=s.cuda_stream, **INTR1)
        prog.verify_epipolar(n, seed=5, hypotheses=64)
        prog.match_consecutive(n)  # and the matcher, whose records it pairs the inliers by
        assert [r.tobytes() + p.tobytes() for r, p in _check(prog, n, cap, inputs, INTR1, call=False)] == one
        _check(prog, n, cap, _inputs(prog, n, cap), INTR1, stream=s.cuda_stream)  # behind that verification, on the other stream
        # a new batch, or another output set: the verification is stale
        prog.extract_batch_host(frames)
        assert code() == tinyorb.ORB_ESTATE
        prog.match_consecutive(n)
        assert code() == tinyorb.ORB_ESTATE  # the match is fresh, the epipolar call is not
        prog.verify_epipolar(n, inlier_px=2.0, seed=3)
        prog.batch_select_output(1)
        assert code() == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, n, cap, _inputs(prog, n, cap), INTR1)  # fresh again: parity on the new batch's own records
