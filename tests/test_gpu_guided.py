"""Guided matching of consecutive frames on the GPU (orb_match_guided): GM-6 equivalence with the brute-force
matcher, every record against the CPU restatement (tests/guided_ref.py) for every model source and window option, verified
models on ground-truth views, the bench size, the call's state and stream rules, and records that do not depend on the grid's
cell size."""
import numpy as np
import pytest

import constructed as C
import guided_ref as gr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
NONE = 0xFFFFFFFF


def _program(tinyorb, W, H, cap, max_batch, flags=0, depth=2):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR,
                            max_batch=max_batch, flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


def _view(scene, G, W, H):
    """Nearest-neighbour inverse mapping: view pixel (x, y) shows scene pixel round(G (x, y, 1)) of the view-sized window at the
    scene's centre (image rows, row 0 at the top)."""
    Hs, Ws = scene.shape[:2]
    G = np.array([[1, 0, (Ws - W) / 2], [0, 1, (Hs - H) / 2], [0, 0, 1]]) @ G
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    p = np.einsum("ij,jhw->ihw", G, np.stack([x, y, np.ones_like(x)]))
    sx = np.floor(p[0] / p[2] + 0.5).astype(np.int64)
    sy = np.floor(p[1] / p[2] + 0.5).astype(np.int64)
    ok = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
    out = np.zeros((H, W, 4), np.uint8)
    out[ok] = scene[sy[ok], sx[ok]]
    out[..., 3] = 255
    return out


def _warp(dx=0.0, dy=0.0, scale=1.0, angle_deg=0.0, px=0.0, py=0.0, W=640, H=480):
    """View-to-scene map: a similarity about the view's centre followed by a mild perspective term, then a shift."""
    c, s = np.cos(np.radians(angle_deg)) * scale, np.sin(np.radians(angle_deg)) * scale
    C = np.array([[1, 0, W / 2], [0, 1, H / 2], [0, 0, 1]])
    Ci = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]])
    A = np.array([[c, -s, dx], [s, c, dy], [px, py, 1.0]])
    return C @ A @ Ci


def _frames(oracle, W, H):
    """Related views of one scene, an all-black frame, two small blobs."""
    scene = oracle.synth_frame(W + 40, H + 40, 300)
    views = [_view(scene, _warp(W=W, H=H), W, H), _view(scene, _warp(3, 2, W=W, H=H), W, H),
             _view(scene, _warp(8, 6, 1.04, 0, 4e-5, -3e-5, W=W, H=H), W, H), np.zeros((H, W, 4), np.uint8)]
    blob = np.zeros((H, W, 4), np.uint8)
    blob[100:103, 150:153] = 255
    blob2 = np.zeros((H, W, 4), np.uint8)
    blob2[101:104, 152:155] = 255
    return np.stack(views + [blob, blob2])


def _records(prog, n_frames, cap):
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    return counts, [prog.batch_read(f, int(counts[f])) for f in range(n_frames)]


def _check(prog, n_frames, cap, recs, source, vmodels=None, host=None, **kw):
    """Guided call, then every record of every pair (cap of them) against the restatement."""
    prog.match_guided(n_frames, source=source, models=host, **kw)
    for f in range(n_frames - 1):
        got = prog.match_guided_read(f, cap)
        m = gr.model_of(source, f, vmodels=vmodels, host=host)
        want = gr.guided_pair(recs[f][0], recs[f][1], recs[f + 1][0], recs[f + 1][1], m, kw.get("radius_px", 0.0),
                              kw.get("octave_window", 0), kw.get("scale_radius", False), cap=cap)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            raise AssertionError((f, source, kw, bad[:5], got[bad[:5]], want[bad[:5]]))


def _homographies(rng, pairs, W, H):
    """Mild random homographies about the frame centre."""
    out = np.empty((pairs, 9), np.float32)
    for f in range(pairs):
        A = _warp(rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(0.97, 1.03), rng.uniform(-3, 3), rng.uniform(-5e-5, 5e-5),
                  rng.uniform(-5e-5, 5e-5), W=W, H=H)
        out[f] = (A / A[2, 2]).reshape(9)
    return out


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_identity_full_window_equals_matcher(tinyorb, oracle, intended):
    """GM-6: identity model, any octave, radius over the whole frame: orb_match_consecutive's records, bit for bit."""
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    W, H = 320, 240
    frames = _frames(oracle, W, H)
    for cap in (1200, 150):
        with _program(tinyorb, W, H, cap, len(frames), flags) as prog:
            prog.extract_batch_host(frames)
            prog.match_consecutive(len(frames))
            prog.match_guided(len(frames), source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=1e6)
            counts = np.minimum(prog.batch_counts(len(frames)), cap)
            for f in range(len(frames) - 1):
                g = prog.match_guided_read(f, cap)
                assert g[:counts[f]].tobytes() == prog.match_read(f, int(counts[f])).tobytes(), (cap, f)
                assert np.all(g["index"][counts[f]:] == NONE) and np.all(g["distance"][counts[f]:] == 0xFFFF)
    W, H, cap = 1280, 720, 8192
    rng = np.random.default_rng(4)
    scene = oracle.synth_frame(W + 160, H + 160, 901)
    frames = np.stack([_view(scene, _warp(rng.uniform(-8, 8), rng.uniform(-8, 8), W=W, H=H), W, H) for _ in range(3)])
    with _program(tinyorb, W, H, cap, 3, flags) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(3)
        prog.match_guided(3, source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=1e6)
        counts = np.minimum(prog.batch_counts(3), cap)
        assert counts.min() > 1000
        for f in range(2):
            assert prog.match_guided_read(f, cap)[:counts[f]].tobytes() == prog.match_read(f, int(counts[f])).tobytes(), f


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_records_against_restatement(tinyorb, oracle, intended):
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    W, H = 320, 240
    frames = _frames(oracle, W, H)
    n = len(frames)
    rng = np.random.default_rng(21)
    I = tinyorb.ORB_GUIDE_IDENTITY
    for cap in (1200, 150):
        with _program(tinyorb, W, H, cap, n, flags) as prog:
            prog.extract_batch_host(frames)
            counts, recs = _records(prog, n, cap)
            assert counts[3] == 0  # the black frame
            for r in (0.0, 0.5, 3.0, 16.0):
                _check(prog, n, cap, recs, I, radius_px=r)
            _check(prog, n, cap, recs, I, radius_px=6.0, octave_window=1)
            _check(prog, n, cap, recs, I, radius_px=6.0, octave_window=2)
            _check(prog, n, cap, recs, I, radius_px=3.0, scale_radius=True)
            _check(prog, n, cap, recs, I, radius_px=2.5, octave_window=1, scale_radius=True)
            host = _homographies(rng, n - 1, W, H)
            host[0] = np.array([1, 0, 5000, 0, 1, -3000, 0, 0, 1], np.float32)  # every window outside the frame
            host[1] = np.array([1, 0, 0, 0, 1, 0, -1.0 / 200, 0, 1], np.float32)  # w <= 0 for x >= 200
            host[2][4] = np.nan
            for r in (3.0, 16.0):
                _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_HOST, host=host, radius_px=r)
                assert counts[0] > 0 and np.all(prog.match_guided_read(0, cap)["index"] == NONE)
                assert np.all(prog.match_guided_read(2, cap)["index"] == NONE)
            _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_HOST, host=host, radius_px=4.0, octave_window=1, scale_radius=True)


def test_verified_models_on_ground_truth_views(tinyorb, oracle):
    """Intended mode: the device's OrbPairModels feed the restatement; with radius inlier_px + 1 every verify inlier of a pair with a
    finite h is matched to the brute-force target (the global best is in the window, and the window is a subset)."""
    W, H, cap = 640, 480, 4096
    scene = oracle.synth_frame(W + 120, H + 120, 77)
    motions = [dict(), dict(dx=6, dy=-4), dict(dx=-5, dy=3, scale=1.05), dict(dx=2, dy=2, scale=0.97, px=3e-5, py=-2e-5),
               dict(dx=-3, dy=5, px=-4e-5, py=3e-5), dict(angle_deg=10), dict(angle_deg=-10, dx=4)]
    frames = np.stack([_view(scene, _warp(W=W, H=H, **m), W, H) for m in motions])
    n, inlier_px = len(frames), 2.0
    with _program(tinyorb, W, H, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        counts, recs = _records(prog, n, cap)
        prog.match_consecutive(n)
        prog.verify_consecutive(n, inlier_px=inlier_px)
        vm = [prog.verify_read(f, cap) for f in range(n - 1)]
        vmodels = np.array([v[0] for v in vm])
        assert np.all(vmodels["status"] == tinyorb.ORB_VERIFY_OK)
        _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_VERIFIED, vmodels=vmodels)
        _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_VERIFIED, vmodels=vmodels, radius_px=3.0, octave_window=2)
        _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_VERIFIED, vmodels=vmodels, radius_px=inlier_px + 1.0)
        matched = 0
        for f in range(n - 1):
            assert np.all(np.isfinite(vmodels[f]["h"]))
            g = prog.match_guided_read(f, cap)
            bf = prog.match_read(f, int(counts[f]))
            inl = vm[f][1][:counts[f]] == 1
            assert np.array_equal(g["index"][:counts[f]][inl], bf["index"][inl]), f
            assert np.all(g["distance"][:counts[f]][inl] == bf["distance"][inl])
            matched += int(inl.sum())
        assert matched > 1000


def test_bench_size_verified(tinyorb, oracle):
    """256 related 1280x720 frames at capacity 8192, matched, verified and guided by the verified models: every pair."""
    W, H, cap, B = 1280, 720, 8192, 256
    rng = np.random.default_rng(11)
    scenes = [oracle.synth_frame(W + 160, H + 160, 900 + s) for s in range(4)]
    frames = np.empty((B, H, W, 4), np.uint8)
    for i in range(B):
        G = _warp(rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(0.97, 1.03), 0, rng.uniform(-2e-5, 2e-5),
                  rng.uniform(-2e-5, 2e-5), W=W, H=H)
        frames[i] = _view(scenes[i // 64], G, W, H)
    with _program(tinyorb, W, H, cap, B) as prog:
        prog.extract_batch_host(frames)
        counts, recs = _records(prog, B, cap)
        prog.match_consecutive(B)
        prog.verify_consecutive(B)
        vmodels = np.array([prog.verify_read(f, 0)[0] for f in range(B - 1)])
        assert np.sum(vmodels["status"] == tinyorb.ORB_VERIFY_OK) > 200
        _check(prog, B, cap, recs, tinyorb.ORB_GUIDE_VERIFIED, vmodels=vmodels, radius_px=3.0)


def test_state_and_ordering(tinyorb, oracle):
    import torch
    W, H, cap = 320, 240, 800
    frames = _frames(oracle, W, H)[:4]
    V, I, HM = tinyorb.ORB_GUIDE_VERIFIED, tinyorb.ORB_GUIDE_IDENTITY, tinyorb.ORB_GUIDE_HOST
    host = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (3, 1))

    def code(**kw):
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_guided(**kw)
        return e.value.code

    with _program(tinyorb, W, H, cap, 4, tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_guided_read(0, cap)  # nothing guided yet
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.extract_batch_host(frames)
        assert code(n_frames=4) == tinyorb.ORB_ESTATE  # verified source without a verification
        for kw in (dict(n_frames=5, source=I), dict(n_frames=1, source=I), dict(n_frames=4, source=HM),
                   dict(n_frames=4, source=I, models=host), dict(n_frames=4, source=3), dict(n_frames=4, source=I, flags=2),
                   dict(n_frames=4, source=I, reserved=(0, 0, 0, 1)), dict(n_frames=4, source=I, radius_px=-1.0),
                   dict(n_frames=4, source=I, radius_px=float("nan")), dict(n_frames=4, source=I, radius_px=float("inf"))):
            assert code(**kw) == tinyorb.ORB_EINVAL, kw
        prog.match_consecutive(4)
        prog.verify_consecutive(3)
        assert code(n_frames=4) == tinyorb.ORB_EINVAL  # three pairs, two verified
        assert code(n_frames=3, models=host) == tinyorb.ORB_EINVAL
        prog.match_guided(3)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_guided_read(2, cap)  # two pairs only
        assert e.value.code == tinyorb.ORB_EINVAL
        C.check_read_arguments(tinyorb, prog, tinyorb.load_library().orb_match_guided_read, 2, 8, head=False)
        # the matcher's and the verifier's results are untouched by a guided call
        before = [(prog.match_read(f, cap).tobytes(), prog.verify_read(f, cap)[0].tobytes(), prog.verify_read(f, cap)[1].tobytes())
                  for f in range(2)]
        one = [prog.match_guided_read(f, cap).tobytes() for f in range(2)]
        prog.match_guided(4, source=I)
        prog.match_guided(4, source=HM, models=host, radius_px=3.0)
        after = [(prog.match_read(f, cap).tobytes(), prog.verify_read(f, cap)[0].tobytes(), prog.verify_read(f, cap)[1].tobytes())
                 for f in range(2)]
        assert before == after
        # the same call on another stream, behind the one before; then back on the batch's stream
        s = torch.cuda.Stream(device=0)
        prog.match_guided(3, stream=s.cuda_stream)
        assert [prog.match_guided_read(f, cap).tobytes() for f in range(2)] == one
        prog.verify_consecutive(3, stream=s.cuda_stream)
        prog.match_guided(3, source=I, radius_px=3.0, stream=s.cuda_stream)
        ident = [prog.match_guided_read(f, cap).tobytes() for f in range(2)]
        prog.match_guided(3)
        assert [prog.match_guided_read(f, cap).tobytes() for f in range(2)] == one
        prog.match_guided(4, source=I, radius_px=3.0)
        assert [prog.match_guided_read(f, cap).tobytes() for f in range(2)] == ident
        # a new batch, or another output set: the verification is stale
        prog.extract_batch_host(frames)
        assert code(n_frames=3) == tinyorb.ORB_ESTATE
        prog.match_guided(4, source=I, radius_px=3.0)  # the other sources need no verification
        prog.match_consecutive(4)
        prog.verify_consecutive(4)
        prog.batch_select_output(1)
        assert code(n_frames=3) == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        counts, recs = _records(prog, 4, cap)  # (a new extraction may store the keypoints in another order)
        vmodels = np.array([prog.verify_read(f, 0)[0] for f in range(3)])
        _check(prog, 4, cap, recs, V, vmodels=vmodels)


def _canonical(recs, out, n_frames):
    """(distance, second) of every query keyed by keypoint (x, y, octave) instead of storage order: two extractions of the same
    frames may store the keypoints in different orders, and with them the target a tie goes to; the distances do not change."""
    rows = []
    for f in range(n_frames - 1):
        qc = recs[f][0]
        g = out[f][:len(qc)]
        r = np.c_[np.full(len(qc), f), qc["x"], qc["y"], qc["octave"], g["distance"], g["second"]].astype(np.int64)
        rows.append(r[np.lexsort(r[:, 3::-1].T)])
    return np.concatenate(rows)


def test_cell_size_changes_no_record(tinyorb, oracle, monkeypatch):
    """GM-5: the grid is an acceleration structure only -- with TINYORB_GUIDE_CELL=8 and =64 (read once per program) every record
    equals the restatement's (which has no grid), and the two programs' distances agree keypoint by keypoint."""
    W, H, cap = 320, 240, 1200
    frames = _frames(oracle, W, H)
    n = len(frames)
    host = _homographies(np.random.default_rng(2), n - 1, W, H)
    res = []
    for cell in ("8", "64"):
        monkeypatch.setenv("TINYORB_GUIDE_CELL", cell)
        with _program(tinyorb, W, H, cap, n) as prog:
            prog.extract_batch_host(frames)
            _, recs = _records(prog, n, cap)
            out = []
            for kw in (dict(radius_px=3.0), dict(radius_px=16.0), dict(radius_px=7.5, octave_window=1, scale_radius=True)):
                _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_IDENTITY, **kw)
                out.append(_canonical(recs, [prog.match_guided_read(f, cap) for f in range(n - 1)], n))
            _check(prog, n, cap, recs, tinyorb.ORB_GUIDE_HOST, host=host, radius_px=40.0)
            out.append(_canonical(recs, [prog.match_guided_read(f, cap) for f in range(n - 1)], n))
        res.append(np.concatenate(out))
    assert np.array_equal(res[0], res[1])
    assert np.sum(res[0][:, 4] != 0xFFFF) > 500
