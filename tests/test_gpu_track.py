"""Feature tracks and keyframes on the GPU (orb_track_consecutive): every OrbTrack of every frame and every
OrbTrackFrame against the CPU restatement (tests/track_ref.py) for the three link sources in both modes, with capacity cuts, blank
frames and fewer frames than the batch, at the bench size and with both forms of k_track_link; the call's argument, state and
stream rules; and the links' correctness on views with a known motion."""
import numpy as np
import pytest

import constructed as C
import track_ref as tr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
NONE = 0xFFFFFFFF


def _program(tinyorb, W, H, cap, max_batch, flags=0, depth=2):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR,
                            max_batch=max_batch, flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


def _view(scene, G, W, H):
    """Nearest-neighbour inverse mapping: view pixel (x, y) shows scene pixel round(G (x, y, 1)) of the view-sized window at the
    scene's centre (image rows, row 0 at the top).  (As in tests/test_gpu_guided.py.)"""
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
    """Eight related views of one scene, an all-black frame, two small blobs, then three more views: tracks that run, break at the
    blank frame and start again."""
    scene = oracle.synth_frame(W + 40, H + 40, 300)
    rng = np.random.default_rng(5)
    views = [_view(scene, _warp(*rng.uniform(-8, 8, 2), rng.uniform(0.98, 1.02), W=W, H=H), W, H) for _ in range(11)]
    blob = np.zeros((H, W, 4), np.uint8)
    blob[100:103, 150:153] = 255
    blob2 = np.zeros((H, W, 4), np.uint8)
    blob2[101:104, 152:155] = 255
    return np.stack(views[:8] + [np.zeros((H, W, 4), np.uint8), blob, blob2] + views[8:])


def _links(prog, source, n_frames, cap, counts, **kw):
    """TK-1 links of every pair from the device's own source records."""
    out = []
    for f in range(n_frames - 1):
        nq, nt = int(counts[f]), int(counts[f + 1])
        if source == 0:  # ORB_TRACK_VERIFIED
            out.append(tr.pair_links(source, prog.match_read(f, cap), nq, nt, inlier=prog.verify_read(f, cap)[1]))
        elif source == 1:
            out.append(tr.pair_links(source, prog.match_guided_read(f, cap), nq, nt, **kw))
        else:
            out.append(tr.pair_links(source, prog.match_read(f, cap), nq, nt, **kw))
    return out


def _check(prog, n_frames, cap, source, **kw):
    """Track call, then every OrbTrack of every frame (cap of them) and every OrbTrackFrame against the restatement."""
    prog.track_consecutive(n_frames, source=source, **kw)
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    lk = {k: kw[k] for k in ("max_distance", "ratio") if k in kw}
    want_t, want_f = tr.track(counts, cap, _links(prog, source, n_frames, cap, counts, **lk), source=source, **kw)
    for f in range(n_frames):
        got = prog.track_read(f, cap)
        if got.tobytes() != want_t[f].tobytes():
            bad = np.nonzero(got != want_t[f])[0]
            raise AssertionError((f, source, kw, bad[:5], got[bad[:5]], want_t[f][bad[:5]]))
    got = prog.track_frames(n_frames)
    assert got.tobytes() == want_f.tobytes(), (source, kw, got, want_f)
    return want_t, want_f


def _sources(tinyorb, prog, n, gsource=None):
    """match, verify and guided calls over n frames of the last batch."""
    prog.match_consecutive(n)
    prog.verify_consecutive(n)
    if gsource is None:
        prog.match_guided(n, source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=16.0)
    else:
        prog.match_guided(n, source=gsource, radius_px=3.0)


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_all_sources_against_restatement(tinyorb, oracle, intended):
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    W, H = 320, 240
    frames = _frames(oracle, W, H)
    n = len(frames)
    V, G, M = tinyorb.ORB_TRACK_VERIFIED, tinyorb.ORB_TRACK_GUIDED, tinyorb.ORB_TRACK_MATCHED
    for cap in (1200, 150):
        with _program(tinyorb, W, H, cap, n + 2, flags) as prog:
            prog.extract_batch_host(frames)
            counts = prog.batch_counts(n)
            assert counts[8] == 0 and (cap == 1200 or counts.max() > cap)  # the blank frame; a capacity cut
            _sources(tinyorb, prog, n)
            total = 0
            for src in (V, G, M):
                t, fr = _check(prog, n, cap, src)
                total += int(fr["links_out"].sum())
                _check(prog, n, cap, src, keep_permille=1000, min_gap=2, max_gap=5)
                _check(prog, n, cap, src, keep_permille=1, min_shared=40)
                _check(prog, 5, cap, src, keep_permille=500)  # fewer frames than the batch and than the source's pairs
                _check(prog, 2, cap, src)
            assert total > 100  # links over the three sources at the defaults (literal mode: about 200)
            for kw in (dict(max_distance=40, ratio=0.7), dict(max_distance=256, ratio=1.5), dict(max_distance=1, ratio=1e-3)):
                _check(prog, n, cap, G, **kw)
                _check(prog, n, cap, M, **kw)
            # a source over fewer pairs than the batch
            prog.match_consecutive(7)
            _check(prog, 7, cap, M)


def test_global_keys_change_nothing(tinyorb, oracle, monkeypatch):
    """k_track_link with its keys in global memory -- TINYORB_TRACK_GLOBAL_KEYS=1 (read once per program), or a capacity past the LDS
    form -- gives the restatement's bytes."""
    W, H = 320, 240
    frames = _frames(oracle, W, H)
    n = len(frames)
    monkeypatch.setenv("TINYORB_TRACK_GLOBAL_KEYS", "1")
    with _program(tinyorb, W, H, 1200, n) as prog:
        prog.extract_batch_host(frames)
        _sources(tinyorb, prog, n)
        for src in (0, 1, 2):
            _check(prog, n, 1200, src)
    monkeypatch.delenv("TINYORB_TRACK_GLOBAL_KEYS")
    with _program(tinyorb, W, H, 20000, n) as prog:  # 4 * cap past the LDS form's 64 KB
        prog.extract_batch_host(frames)
        _sources(tinyorb, prog, n)
        for src in (0, 1, 2):
            _check(prog, n, 20000, src, keep_permille=950)


def test_bench_size(tinyorb, oracle):
    """256 related 1280x720 frames at capacity 8192 (four scenes of 64 views): matched, verified, guided by the verified models at
    r = 3, then tracked from every source -- every entry of every frame."""
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
        _sources(tinyorb, prog, B, gsource=tinyorb.ORB_GUIDE_VERIFIED)
        for src in (0, 1, 2):
            _, fr = _check(prog, B, cap, src)
            assert fr["keyframe"].sum() >= 4  # at least the scene changes
        _check(prog, 200, cap, 1, max_gap=16, min_shared=100)


def test_state_and_ordering(tinyorb, oracle):
    import torch
    W, H, cap = 320, 240, 800
    frames = _frames(oracle, W, H)[:5]
    V, G, M = tinyorb.ORB_TRACK_VERIFIED, tinyorb.ORB_TRACK_GUIDED, tinyorb.ORB_TRACK_MATCHED

    def code(*a, **kw):
        with pytest.raises(tinyorb.OrbError) as e:
            prog.track_consecutive(*a, **kw)
        return e.value.code

    with _program(tinyorb, W, H, cap, 5, tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        for fn in (lambda: prog.track_read(0, cap), lambda: prog.track_frames(5)):
            with pytest.raises(tinyorb.OrbError) as e:
                fn()  # nothing tracked yet
            assert e.value.code == tinyorb.ORB_ESTATE
        prog.extract_batch_host(frames)
        for src in (V, G, M):
            assert code(5, source=src) == tinyorb.ORB_ESTATE  # no source call
        for kw in (dict(n_frames=6), dict(n_frames=1), dict(n_frames=5, source=3), dict(n_frames=5, reserved=1),
                   dict(n_frames=5, max_distance=10), dict(n_frames=5, ratio=0.5), dict(n_frames=5, source=M, max_distance=257),
                   dict(n_frames=5, source=M, ratio=-0.1), dict(n_frames=5, source=G, ratio=float("nan")),
                   dict(n_frames=5, source=G, ratio=float("inf")), dict(n_frames=5, keep_permille=1001),
                   dict(n_frames=5, min_gap=4, max_gap=3), dict(n_frames=5, max_gap=1, min_gap=0, keep_permille=2000)):
            assert code(**kw) == tinyorb.ORB_EINVAL, kw
        prog.match_consecutive(5)
        prog.verify_consecutive(4)
        prog.match_guided(3)
        assert code(5) == tinyorb.ORB_EINVAL  # four pairs, three verified
        assert code(5, source=G) == tinyorb.ORB_EINVAL  # two guided
        _check(prog, 4, cap, V)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.track_read(4, cap)  # four frames only
        assert e.value.code == tinyorb.ORB_EINVAL
        C.check_read_arguments(tinyorb, prog, tinyorb.load_library().orb_track_read, 4, 16, head=False)
        assert len(prog.track_frames(10)) == 4
        # the matcher's, the verifier's and the guided call's results are untouched by a track call
        prog.match_guided(5, source=tinyorb.ORB_GUIDE_IDENTITY)

        def sources():
            return [(prog.match_read(f, cap).tobytes(), prog.verify_read(f, cap)[0].tobytes(), prog.verify_read(f, cap)[1].tobytes(),
                     prog.match_guided_read(f, cap).tobytes()) for f in range(3)]

        before = sources()
        for src in (V, G, M):
            prog.track_consecutive(4, source=src)
        assert sources() == before
        # match, verify, guided and track calls alternating between two streams give the single-stream results
        single = {}
        for src in (V, G, M):
            prog.track_consecutive(5 if src != V else 4, source=src)
            single[src] = ([prog.track_read(f, cap).tobytes() for f in range(4)], prog.track_frames(5).tobytes())

        def epipolar():
            return [tuple(r.tobytes() for r in prog.verify_epipolar_read(f, cap)) for f in range(3)]

        prog.verify_epipolar(4)
        single_epi = epipolar()
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        for rep in range(2):
            a, b = (s1, s2) if rep == 0 else (s2, s1)
            prog.match_consecutive(5, stream=a.cuda_stream)
            prog.verify_epipolar(4, stream=b.cuda_stream)  # waits for the match on a, whose results it reads
            prog.track_consecutive(5, source=M, stream=b.cuda_stream)
            prog.verify_consecutive(4, stream=a.cuda_stream)
            prog.track_consecutive(4, source=V, stream=b.cuda_stream)
            prog.match_guided(5, source=tinyorb.ORB_GUIDE_IDENTITY, stream=a.cuda_stream)
            prog.track_consecutive(5, source=G, stream=b.cuda_stream)
            got_g = ([prog.track_read(f, cap).tobytes() for f in range(4)], prog.track_frames(5).tobytes())
            assert got_g == single[G]
            prog.track_consecutive(4, source=V, stream=a.cuda_stream)
            assert epipolar() == single_epi
            prog.match_consecutive(5, stream=b.cuda_stream)  # waits for the track call on a before it overwrites the matches
            assert ([prog.track_read(f, cap).tobytes() for f in range(4)], prog.track_frames(5).tobytes()) == single[V]
            prog.track_consecutive(5, source=M, stream=a.cuda_stream)
            assert ([prog.track_read(f, cap).tobytes() for f in range(4)], prog.track_frames(5).tobytes()) == single[M]
        # a new batch makes every source stale; so does another output set
        prog.extract_batch_host(frames)
        for src in (V, G, M):
            assert code(4, source=src) == tinyorb.ORB_ESTATE
        prog.match_consecutive(5)
        assert code(4, source=V) == tinyorb.ORB_ESTATE  # the verification is of the batch before
        prog.verify_consecutive(5)
        prog.match_guided(5)
        prog.batch_select_output(1)
        for src in (V, G, M):
            assert code(4, source=src) == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        for src in (V, G, M):
            _check(prog, 5, cap, src)


def test_links_follow_ground_truth(tinyorb, oracle):
    """Intended mode, 24 views of one scene with known motions, match -> verify -> guided by the verified models at r = 3 -> track
    (GUIDED): every keypoint whose track started in an earlier frame is compared with its head keypoint sent through the composed
    ground-truth warp.  Floors set from the first measured run with margin: within 2 px 0.987 measured, floor 0.9; mean length of
    the tracks with a link 5.18 frames measured, floor 3.5."""
    W, H, cap, n = 640, 480, 4096, 24
    rng = np.random.default_rng(3)
    scene = oracle.synth_frame(W + 160, H + 160, 41)
    Gs = [_warp(rng.uniform(-6, 6), rng.uniform(-6, 6), rng.uniform(0.98, 1.02), rng.uniform(-2, 2), W=W, H=H) for _ in range(n)]
    frames = np.stack([_view(scene, G, W, H) for G in Gs])
    with _program(tinyorb, W, H, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        counts = np.minimum(prog.batch_counts(n), cap)
        recs = [prog.batch_read(f, int(counts[f]))[0] for f in range(n)]
        prog.match_consecutive(n)
        prog.verify_consecutive(n)
        prog.match_guided(n, source=tinyorb.ORB_GUIDE_VERIFIED, radius_px=3.0)
        t, fr = _check(prog, n, cap, tinyorb.ORB_TRACK_GUIDED)
    near = far = 0
    lengths = []
    for f in range(n):
        tf = t[f][:counts[f]]
        x, y = (v.astype(np.float64) for v in tinyorb.level0_xy(recs[f]))
        starts = tf["prev"] == NONE
        lengths += list(tf["tail_frame"][starts].astype(int) - f + 1)
        old = np.nonzero(tf["head_frame"] < f)[0]
        for h in np.unique(tf["head_frame"][old]):
            sel = old[tf["head_frame"][old] == h]
            hx, hy = (v.astype(np.float64) for v in tinyorb.level0_xy(recs[h][tf["head_index"][sel]]))
            T = np.linalg.inv(Gs[f]) @ Gs[h]  # view h -> scene -> view f
            p = T @ np.stack([hx, hy, np.ones_like(hx)])
            d = np.hypot(p[0] / p[2] - x[sel], p[1] / p[2] - y[sel])
            near += int(np.sum(d <= 2.0))
            far += int(np.sum(d > 2.0))
    lengths = np.array(lengths)
    frac, mean_len = near / max(near + far, 1), float(lengths[lengths > 1].mean())
    print("track quality: %d linked keypoints, %.4f within 2 px, mean length %.2f (tracks with a link), %.2f (all), %d keyframes"
          % (near + far, frac, mean_len, lengths.mean(), fr["keyframe"].sum()))
    assert near + far > 20000
    assert frac > 0.9, frac
    assert mean_len > 3.5, mean_len
