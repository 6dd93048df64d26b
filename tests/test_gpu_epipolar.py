"""Epipolar verification of consecutive-frame matches on the GPU (orb_verify_epipolar): every record and inlier
byte against the CPU restatement (tests/epipolar_ref.py) on extracted frames, on constructed two-view scenes with depth and at the
bench size; more correct matches kept than the homography verifier on two-layer parallax views; the homography verifier's results,
guided matching and tracks untouched; the call's state, argument and stream rules."""
import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
from test_gpu_verify import _parity_frames, _program, _view, _warp

pytestmark = pytest.mark.gpu


def _check_parity(prog, n_frames, W, H, cap, **params):
    """Epipolar verification of the first n_frames of the last match; every pair's record and cap inlier bytes against the
    restatement."""
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    prog.verify_epipolar(n_frames, **params)
    recs = []
    for f in range(n_frames - 1):
        matches = prog.match_read(f, int(counts[f]))
        rec, mask = prog.verify_epipolar_read(f, cap)
        ref, rmask = er.verify_pair(corners[f], corners[f + 1], matches, W, H, f, cap=cap, **params)
        assert rec.tobytes() == ref.tobytes(), (f, params, rec, ref)
        assert np.array_equal(mask, rmask), (f, params, np.nonzero(mask != rmask)[0][:8])
        recs.append(rec)
    return recs


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_parity_extracted(tinyorb, oracle, intended):
    """test_gpu_verify's parity frames (shifted and warped views, a blank frame, tiny frames) at two capacities."""
    W, H = 320, 240
    frames = _parity_frames(oracle, W, H)
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    statuses = set()
    for cap in (1200, 150):
        with _program(tinyorb, W, H, cap, len(frames), flags) as prog:
            prog.extract_batch_host(frames)
            prog.match_consecutive(len(frames))
            for hyps, seed in ((1, 0), (100, 0x9E3779B9), (512, 0), (4096, 7)):
                recs = _check_parity(prog, len(frames), W, H, cap, hypotheses=hyps, seed=seed)
                statuses |= {int(r["status"]) for r in recs}
            recs = _check_parity(prog, len(frames), W, H, cap, ratio=1.0, max_distance=256, inlier_px=1.5, seed=5)
            statuses |= {int(r["status"]) for r in recs}
            if cap == 1200 and intended:
                assert recs[0]["status"] in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL) and recs[0]["inliers"] > 50
    assert tinyorb.ORB_VERIFY_FEW in statuses and tinyorb.ORB_VERIFY_OK in statuses


def _constructed_batch(tinyorb, cap):
    """Pairs (0, 1) ... of constructed scenes, each in frames (2i, 2i + 1): the three motions in full (about 810 candidates:
    several 256-candidate tiles), M = 8, M = 257 and 255 (either side of a tile boundary), M = cap with raw counters above the
    capacity, outliers only, and collinear correspondences.  The pairs between two scenes have no candidates (FEW)."""
    W, H = 640, 480
    rng = np.random.default_rng(2024)
    scenes = [er.scene(rng, "sideways"), er.scene(rng, "yaw"), er.scene(rng, "forward"), er.scene(rng, "forward", count=8),
              er.scene(rng, "yaw", count=257), er.scene(rng, "sideways", count=255), er.scene(rng, "forward", n=1400, count=cap),
              er.scene(rng, "sideways", outlier_share=1.0, n=300)]
    cor, desc, counts = [], [], []
    for s in scenes:
        cor += s["corners"]
        desc += s["desc"]
        counts += [len(s["corners"][0])] * 2
    counts[12] += 37  # the M = cap scene: raw counters above the capacity
    counts[13] += 5
    cc, dc = C.collinear(rng, 60, W, H)
    cor += list(cc)
    desc += list(dc)
    counts += [60, 60]
    return W, H, cor, desc, np.array(counts, np.uint32), scenes


def test_parity_constructed(tinyorb):
    cap = 1024
    W, H, cor, desc, counts, scenes = _constructed_batch(tinyorb, cap)
    B = len(counts)
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B)
    with tinyorb.OrbProgram(cfg) as prog:
        prog.extract_batch_host(np.zeros((B, H, W, 4), np.uint8))
        C.inject(prog, counts, cor, desc)
        prog.match_consecutive(B)
        for params in (dict(inlier_px=2.0), dict(hypotheses=4096, inlier_px=2.0, seed=11), dict(hypotheses=64, seed=3)):
            recs = _check_parity(prog, B, W, H, cap, **params)
            got = [(int(r["candidates"]), int(r["status"])) for r in recs[0::2]]
            assert [g[0] for g in got] == [len(s["corners"][0]) for s in scenes[:6]] + [cap, 300, 60], got
            assert all(s == tinyorb.ORB_VERIFY_OK for _, s in got[:7]), (params, got)
            assert got[8][1] == tinyorb.ORB_VERIFY_DEGENERATE, got
            assert all(int(r["status"]) == tinyorb.ORB_VERIFY_FEW for r in recs[1::2]), params
            if params.get("inlier_px") == 2.0:
                for i in range(3):  # the full scenes: the kept share of the correct correspondences
                    _, mask = prog.verify_epipolar_read(2 * i, cap)
                    correct = scenes[i]["correct"]
                    assert mask[:len(correct)][correct].mean() >= 0.95, (i, params)


def test_bench_size_parity(tinyorb, oracle):
    """1280 x 720 at capacity 8192, the intended mode: related views of one scene (shifts, +-3 % scale, mild perspective)."""
    W, H, cap, B = 1280, 720, 8192, 6
    rng = np.random.default_rng(12)
    scene = oracle.synth_frame(W + 160, H + 160, 905)
    frames = np.stack([_view(scene, _warp(rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(0.97, 1.03), 0, rng.uniform(-2e-5, 2e-5),
                                          rng.uniform(-2e-5, 2e-5), W=W, H=H), W, H) for _ in range(B)])
    with _program(tinyorb, W, H, cap, B, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(B)
        recs = _check_parity(prog, B, W, H, cap)
    assert all(int(r["status"]) == tinyorb.ORB_VERIFY_OK and r["candidates"] > 1000 for r in recs), recs


SHIFT_FAR, SHIFT_NEAR = np.array([2.0, 1.0]), np.array([12.0, 6.0])  # per frame, along one direction: a sideways camera


def _two_layer_views(oracle, W, H, n):
    """Views of two textured planes from a camera that translates along (2, 1): the far plane (rows < H / 2 of the view) moves by
    SHIFT_FAR px per frame, the near one (the other rows) by SHIFT_NEAR: 13.4 - 2.2 = 11.2 px apart, each half of the view."""
    pad = 8 + int(SHIFT_NEAR.max()) * n
    far, near = oracle.synth_frame(W + pad, H + pad, 4001), oracle.synth_frame(W + pad, H + pad, 4002)
    views = np.empty((n, H, W, 4), np.uint8)
    for i in range(n):
        for tex, s, rows in ((far, SHIFT_FAR, slice(0, H // 2)), (near, SHIFT_NEAR, slice(H // 2, H))):
            ox, oy = (s * i).astype(int)
            views[i, rows] = tex[oy:oy + H, ox:ox + W][rows]
    return views


def test_two_layer_parallax(tinyorb, oracle):
    """Intended mode.  A correct match lies within 2 px of its layer's motion (the layer of the query's row); on every pair the
    epipolar verifier keeps more of them than orb_verify_consecutive, which can follow one layer only."""
    W, H, cap, n = 640, 480, 4096, 5
    frames = _two_layer_views(oracle, W, H, n)
    shares = []
    with _program(tinyorb, W, H, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(n)
        prog.verify_consecutive(n, inlier_px=2.0)
        prog.verify_epipolar(n, inlier_px=2.0)
        counts = np.minimum(prog.batch_counts(n), cap)
        for f in range(n - 1):
            q = prog.batch_read(f, int(counts[f]))[0]
            t = prog.batch_read(f + 1, int(counts[f + 1]))[0]
            m = prog.match_read(f, int(counts[f]))
            _, hmask = prog.verify_read(f, int(counts[f]))
            _, emask = prog.verify_epipolar_read(f, int(counts[f]))
            qx, qy = er.vr.level0(q)
            ok = (m["index"] != tinyorb.ORB_MATCH_NONE) & (m["index"] < len(t))
            tx, ty = er.vr.level0(t[np.where(ok, m["index"], 0).astype(np.int64)])
            s = np.where((qy < H // 2)[:, None], -SHIFT_FAR, -SHIFT_NEAR)
            correct = ok & (np.hypot(tx - (qx + s[:, 0]), ty - (qy + s[:, 1])) <= 2.0)
            near = correct & (qy >= H // 2)
            h_keep, e_keep = int((hmask.astype(bool) & correct).sum()), int((emask.astype(bool) & correct).sum())
            shares.append((int(correct.sum()), int(near.sum()), h_keep, e_keep))
            print("pair %d: correct %d (near layer %d), homography keeps %d (%.3f), epipolar %d (%.3f)" %
                  (f, correct.sum(), near.sum(), h_keep, h_keep / max(correct.sum(), 1), e_keep, e_keep / max(correct.sum(), 1)))
    for c, nr, hk, ek in shares:
        assert nr >= c / 4 and c - nr >= c / 4, shares  # both layers hold correct matches
        assert ek > hk, shares


def test_isolation_from_the_homography_path(tinyorb, oracle):
    """An epipolar call between orb_verify_consecutive and its readers leaves the homography records and inlier bytes,
    orb_match_guided(VERIFIED) and orb_track_consecutive(VERIFIED) byte for byte as they are without it."""
    W, H, cap = 320, 240, 1200
    frames = _parity_frames(oracle, W, H)
    n = len(frames)

    def run(with_epi):
        prog.match_consecutive(n)
        prog.verify_consecutive(n, inlier_px=2.0, seed=9)
        if with_epi:
            prog.verify_epipolar(n, hypotheses=4096, inlier_px=1.0, seed=9)
        prog.match_guided(n, source=tinyorb.ORB_GUIDE_VERIFIED, radius_px=3.0)
        prog.track_consecutive(n)
        out = [prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() for f in range(n - 1)]
        out += [prog.match_guided_read(f, cap).tobytes() for f in range(n - 1)]
        out += [prog.track_read(f, cap).tobytes() for f in range(n)] + [prog.track_frames(n).tobytes()]
        return out

    with _program(tinyorb, W, H, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        a = run(False)
        b = run(True)
        assert prog.verify_epipolar_read(0, cap)[0]["status"] in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL)
    assert a == b


def test_state_and_ordering(tinyorb, oracle):
    import torch
    W, H, cap = 320, 240, 800
    frames = _parity_frames(oracle, W, H)[:4]
    with _program(tinyorb, W, H, cap, 4, tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        prog.extract_batch_host(frames)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_epipolar(4)  # no match yet
        assert e.value.code == tinyorb.ORB_ESTATE
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_epipolar_read(0, cap)  # nothing verified
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.match_consecutive(3)
        for kw in (dict(n_frames=4), dict(n_frames=1), dict(n_frames=3, hypotheses=4097), dict(n_frames=3, max_distance=257),
                   dict(n_frames=3, reserved=(0, 1, 0)), dict(n_frames=3, reserved=(0, 0, 2)), dict(n_frames=3, ratio=-1.0),
                   dict(n_frames=3, ratio=float("inf")), dict(n_frames=3, inlier_px=float("nan")), dict(n_frames=3, inlier_px=-0.5)):
            with pytest.raises(tinyorb.OrbError) as e:
                prog.verify_epipolar(**kw)
            assert e.value.code == tinyorb.ORB_EINVAL, kw
        one = _check_parity(prog, 3, W, H, cap, seed=3)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_epipolar_read(2, cap)  # two pairs only
        assert e.value.code == tinyorb.ORB_EINVAL
        C.check_read_arguments(tinyorb, prog, tinyorb.load_library().orb_verify_epipolar_read, 2, 1, head=True)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_read(0, cap)  # the homography verifier has run nowhere
        assert e.value.code == tinyorb.ORB_ESTATE
        # on another stream than the match's: ordered behind it, the same records; then the match on its own stream waits for it
        s = torch.cuda.Stream(device=0)
        prog.match_consecutive(4)
        prog.verify_epipolar(3, seed=3, hypotheses=4096, stream=s.cuda_stream)
        prog.match_consecutive(4, stream=prog._lib.orb_program_stream(prog._handle()))
        many = _check_parity(prog, 3, W, H, cap, seed=3, hypotheses=4096)
        prog.verify_epipolar(3, seed=3, stream=s.cuda_stream)
        for f in range(2):
            assert prog.verify_epipolar_read(f, cap)[0].tobytes() == one[f].tobytes()
        prog.verify_epipolar(3, seed=3, hypotheses=4096)  # back on the last stream, behind the one before
        for f in range(2):
            assert prog.verify_epipolar_read(f, cap)[0].tobytes() == many[f].tobytes()
        # a new batch without a new match, or another output set
        prog.extract_batch_host(frames)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_epipolar(3)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.match_consecutive(4)
        prog.batch_select_output(1)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_epipolar(3)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        prog.verify_epipolar(3, seed=3)
        assert prog.verify_epipolar_read(0, cap)[0].tobytes() == one[0].tobytes()
