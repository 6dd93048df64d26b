"""Epipolar-band guided matching on the GPU (orb_match_epipolar): every record against the CPU restatement
(tests/band_ref.py) on constructed records for every kind of line, band, window and octave option, at two capacities and two cell
sizes; EB-6 (a) against the brute-force matcher on extracted frames; the verified fundamental matrices of a two-layer parallax scene
with EB-6 (c); and the call's state, argument, stream and buffer rules."""
import numpy as np
import pytest

import band_ref as br
import constructed as C

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
NONE = 0xFFFFFFFF
W0, H0, DEPTH, FRAMES = 160, 120, 3, 6
EPIPOLE = (80, 60)


def _program(tinyorb, W, H, cap, max_batch, flags=0, depth=2):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR,
                            max_batch=max_batch, flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


# ---- models ------------------------------------------------------------------------------------------------------------------
def _cross(e):
    """[e]_x row-major: the line of x1 joins it to the epipole e."""
    return np.array([0, -e[2], e[1], e[2], 0, -e[0], -e[1], e[0], 0], np.float32)


HORIZONTAL = br.SIDEWAYS                                              # a0 = 0: y' = y
VERTICAL = np.array([0, 0, -1, 0, 0, 0, 1, 0, 0], np.float32)         # a1 = 0: x' = x
DIAGONAL = _cross((1, 1, 0))                                          # x' - y' = x - y
STEEP = _cross((1, 40, 0))                                            # 40 x' - y' = c: nearly vertical
SHALLOW = _cross((40, 1, 0))                                          # x' - 40 y' = c: nearly horizontal
MISSES = np.array([0, 0, 0, 0, 0, -1, 0, 1, 1000], np.float32)        # y' = y + 1000
CORNER = _cross((0, 0, 1))                                            # every line through the corner (0, 0)
FAR_CORNER = _cross((W0 - 1, H0 - 1, 1))                              # ... through the corner (159, 119)
INSIDE = _cross(EPIPOLE + (1,))                                       # the epipole inside the frame: one query lies on it
ZERO = np.zeros(9, np.float32)


def _general(rng):
    A = rng.normal(size=(3, 3))
    t = rng.normal(size=3)
    K = np.array([[150.0, 0, W0 / 2], [0, 150.0, H0 / 2], [0, 0, 1]])
    Fm = np.linalg.inv(K).T @ _cross(t).reshape(3, 3).astype(np.float64) @ (np.eye(3) + 0.1 * A) @ np.linalg.inv(K)
    return (Fm / np.abs(Fm).max()).astype(np.float32).reshape(9)


def _with(m, e, v):
    m = m.copy()
    m[e] = v
    return m


def _model_sets():
    """Five models per set; the frames below make pairs 0..2 full against full, pair 3 an empty target frame, pair 4 an empty query
    frame."""
    rng = np.random.default_rng(77)
    g = [_general(rng) for _ in range(4)]
    return [
        np.stack([HORIZONTAL, VERTICAL, DIAGONAL, DIAGONAL, HORIZONTAL]),
        np.stack([STEEP, SHALLOW, g[0], g[1], g[1]]),
        np.stack([MISSES, CORNER, INSIDE, INSIDE, INSIDE]),
        np.stack([FAR_CORNER, g[2] * np.float32(2.0 ** -20), g[3] * np.float32(2.0 ** 20), HORIZONTAL, HORIZONTAL]),
    ]


# ---- constructed records -----------------------------------------------------------------------------------------------------
def _frame(rng, n, planted=()):
    """n distinct records inside a 160 x 120, depth-3 pyramid in a random order, the planted (x, y, octave) among them; descriptors
    with few distinct bytes, so that equal distances (ties to the smaller index) are the rule."""
    seen = dict.fromkeys(tuple(p) for p in planted)
    while len(seen) < n:
        o = int(rng.integers(0, DEPTH))
        seen.setdefault((int(rng.integers(0, W0 >> o)), int(rng.integers(0, H0 >> o)), o))
    rec = np.array(list(seen), np.int64).reshape(-1, 3)[rng.permutation(n)]
    d = np.ascontiguousarray(rng.integers(0, 4, (n, 32)).astype(np.uint8)).view(np.uint32).reshape(n, 8)
    return C.corners(rec[:, 0], rec[:, 1], rec[:, 2], rng=rng), d


def _batch(cap):
    """(counts, corners, descriptors, the stored records per frame).  cap 256: 190..230 records per frame (NONE tails); cap 48: raw
    counters above the capacity, one frame below it.  Frame 4 is empty.  Every query frame holds a keypoint exactly on EPIPOLE, and
    frame f + 1 holds targets at offsets of exactly 0.5, 2, 8 (band and window edges for d, R in {0.5, 2, 8}) and one more pixel
    from keypoints of frame f."""
    rng = np.random.default_rng(1000 + cap)
    sizes = [200, 230, 190, 215, 0, 205] if cap == 256 else [48, 48, 30, 48, 0, 48]
    extra = [0] * FRAMES if cap == 256 else [17, 1, 0, 300, 0, 5]
    cor, desc, prev = [], [], None
    for f, n in enumerate(sizes):
        planted = [EPIPOLE + (0,)] if n else []
        if prev is not None and n:
            for x, y, _, o in prev[:6].tolist():
                if o == 0 and 12 <= x < W0 - 12 and 12 <= y < H0 - 12:
                    planted += [(x + 8, y + 2, 0), (x - 9, y - 2, 0), (x + 3, y - 8, 0), (x - 2, y + 9, 0), (x + 2, y + 3, 0)]
                elif o == 1 and 6 <= x < (W0 >> 1) - 6 and 6 <= y < (H0 >> 1) - 6:  # level-0 centre (2x + 0.5, 2y + 0.5)
                    planted += [(2 * x + 1, 2 * y, 0), (2 * x, 2 * y + 2, 0), (2 * x + 9, 2 * y + 1, 0), (x + 4, y - 1, 1)]
        c, d = _frame(rng, n, planted[:max(n - 1, 0)])
        cor.append(c)
        desc.append(d)
        prev = np.stack([c["x"], c["y"], c["angle"], c["octave"]], 1).astype(np.int64) if n else None
    counts = np.array(sizes, np.uint32) + np.array(extra, np.uint32)
    return counts, cor, desc, list(zip(cor, desc))


def _check(prog, n_frames, cap, recs, source, vmodels=None, host=None, **kw):
    """Band call, then every record of every pair (cap of them) against the restatement.  Returns the device's records."""
    prog.match_epipolar(n_frames, source=source, models=host, **kw)
    got_all = []
    for f in range(n_frames - 1):
        got = prog.match_epipolar_read(f, cap)
        m = br.model_of(source, f, vmodels=vmodels, host=host)
        want = br.band_pair(recs[f][0], recs[f][1], recs[f + 1][0], recs[f + 1][1], m, kw.get("band_px", 0.0), kw.get("radius_px", 0.0),
                            kw.get("octave_window", 0), kw.get("scale", False), cap=cap)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            raise AssertionError((f, source, kw, bad[:5], got[bad[:5]], want[bad[:5]]))
        got_all.append(got)
    return got_all


def _options():
    for R in (0.0, 0.5, 8.0):
        for d in (0.0, 0.5, 2.0, 1e6):
            for ow in (0, 1, 2):
                for sc in (False, True):
                    yield dict(band_px=d, radius_px=R, octave_window=ow, scale=sc)


def _constructed_checks(tinyorb, cap, options):
    """Every model set under `options` on the constructed batch; returns the bytes of every record read."""
    H = tinyorb.ORB_BAND_HOST
    counts, cor, desc, recs = _batch(cap)
    out = []
    with _program(tinyorb, W0, H0, cap, FRAMES, depth=DEPTH) as prog:
        prog.extract_batch_host(np.zeros((FRAMES, H0, W0, 4), np.uint8))
        C.inject(prog, counts, cor, desc)
        matched = 0
        for kw in options:
            for ms, host in enumerate(_model_sets()):
                got = _check(prog, FRAMES, cap, recs, H, host=host, **kw)
                out += [g.tobytes() for g in got]
                assert np.all(got[3]["index"] == NONE) and np.all(got[4]["index"] == NONE)  # empty target frame, empty query frame
                if ms == 0:
                    matched += sum(int(np.sum(g["index"] != NONE)) for g in got)
                if ms == 2:
                    assert kw["band_px"] == 1e6 or np.all(got[0]["index"] == NONE), kw  # the line misses the frame
                    on = np.nonzero((cor[2]["x"] == EPIPOLE[0]) & (cor[2]["y"] == EPIPOLE[1]) & (cor[2]["octave"] == 0))[0]
                    assert len(on) == 1 and got[2]["index"][on[0]] == NONE, kw  # the query on the epipole has no line
                    if kw["band_px"] == 1e6 and kw["radius_px"] == 0.0 and kw["octave_window"] == 0:
                        assert np.sum(got[2]["index"][:len(cor[2])] == NONE) == 1  # ... and it is the only one
        assert matched > 5 * len(options)
        # F with an infinite or a NaN entry, and the zero matrix: no query has a line
        g = _general(np.random.default_rng(3))
        bad = np.stack([_with(HORIZONTAL, 5, np.inf), _with(DIAGONAL, 0, np.nan), ZERO, _with(g, 8, -np.inf), _with(g, 4, np.nan)])
        for kw in (dict(band_px=1e6), dict(band_px=2.0, radius_px=8.0, scale=True)):
            got = _check(prog, FRAMES, cap, recs, H, host=bad, **kw)
            out += [g.tobytes() for g in got]
            assert all(np.all(g["index"] == NONE) and np.all(g["distance"] == 0xFFFF) and np.all(g["second"] == 0xFFFF) for g in got)
    return out


@pytest.mark.parametrize("cap", [256, 48])
def test_constructed_records_against_restatement(tinyorb, cap):
    _constructed_checks(tinyorb, cap, list(_options()))


def test_cell_size_changes_no_record(tinyorb, monkeypatch):
    """EB-5: with TINYORB_GUIDE_CELL = 8 and = 64 (read once per program) every record equals the restatement's, which has no grid,
    and therefore the other program's."""
    options = [kw for kw in _options() if kw["octave_window"] == 0 and kw["band_px"] != 0.0]
    res = []
    for cell in ("8", "64"):
        monkeypatch.setenv("TINYORB_GUIDE_CELL", cell)
        res.append(_constructed_checks(tinyorb, 256, options))
    assert res[0] == res[1] and len(res[0]) == len(options) * 4 * (FRAMES - 1) + 2 * (FRAMES - 1)


# ---- extracted frames --------------------------------------------------------------------------------------------------------
def _view(scene, G, W, H):
    """Nearest-neighbour inverse mapping: view pixel (x, y) shows scene pixel round(G (x, y, 1)) of the view-sized window at the
    scene's centre."""
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


def _shift(dx, dy):
    return np.array([[1, 0, dx], [0, 1, dy], [0, 0, 1.0]])


def _frames(oracle, W, H):
    """Shifted views of one scene, an all-black frame, a small blob."""
    scene = oracle.synth_frame(W + 40, H + 40, 300)
    blob = np.zeros((H, W, 4), np.uint8)
    blob[100:103, 150:153] = 255
    return np.stack([_view(scene, _shift(0, 0), W, H), _view(scene, _shift(3, 2), W, H), _view(scene, _shift(8, 6), W, H),
                     np.zeros((H, W, 4), np.uint8), blob])


def _records(prog, n_frames, cap):
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    return counts, [prog.batch_read(f, int(counts[f])) for f in range(n_frames)]


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_covering_band_equals_matcher(tinyorb, oracle, intended):
    """EB-6 (a): host models, a band over the whole frame, no window: orb_match_consecutive's record for every query with a line."""
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    W, H = 320, 240
    frames = _frames(oracle, W, H)
    n = len(frames)
    rng = np.random.default_rng(9)
    host = np.stack([DIAGONAL, _general(rng), _cross((100.0, 80.0, 1.0)), HORIZONTAL])
    for cap in (1200, 150):
        with _program(tinyorb, W, H, cap, n, flags) as prog:
            prog.extract_batch_host(frames)
            prog.match_consecutive(n)
            counts, recs = _records(prog, n, cap)
            prog.match_epipolar(n, source=tinyorb.ORB_BAND_HOST, models=host, band_px=1e6)
            lined = 0
            for f in range(n - 1):
                g = prog.match_epipolar_read(f, cap)
                bf = prog.match_read(f, int(counts[f]))
                ok = br.lines(host[f], *br.level0(recs[f][0]), np.full(int(counts[f]), 1e6, np.float32))[4]
                assert g[:counts[f]][ok].tobytes() == bf[ok].tobytes(), (cap, f)
                assert np.all(g["index"][:counts[f]][~ok] == NONE) and np.all(g["index"][counts[f]:] == NONE)
                assert int(ok.sum()) >= int(counts[f]) - 1
                lined += int(ok.sum())
            assert lined > 100
            _check(prog, n, cap, recs, tinyorb.ORB_BAND_HOST, host=host, band_px=2.0)
            _check(prog, n, cap, recs, tinyorb.ORB_BAND_HOST, host=host, band_px=1.5, radius_px=24.0, octave_window=2, scale=True)


SHIFT_FAR, SHIFT_NEAR = np.array([2.0, 1.0]), np.array([12.0, 6.0])  # per frame, along one direction: a sideways camera


def _two_layer_views(oracle, W, H, n):
    """Views of two textured planes from a camera that translates along (2, 1): the far plane (rows < H / 2 of the view) moves by
    SHIFT_FAR px per frame, the near one (the other rows) by SHIFT_NEAR."""
    pad = 8 + int(SHIFT_NEAR.max()) * n
    far, near = oracle.synth_frame(W + pad, H + pad, 4001), oracle.synth_frame(W + pad, H + pad, 4002)
    views = np.empty((n, H, W, 4), np.uint8)
    for i in range(n):
        for tex, s, rows in ((far, SHIFT_FAR, slice(0, H // 2)), (near, SHIFT_NEAR, slice(H // 2, H))):
            ox, oy = (s * i).astype(int)
            views[i, rows] = tex[oy:oy + H, ox:ox + W][rows]
    return views


def test_verified_models_on_two_layer_parallax(tinyorb, oracle):
    """Intended mode, 640 x 480: match -> verify_epipolar -> match_epipolar with the verified F; every record against the
    restatement, and EB-6 (c): where the brute-force best lies in the band, the band record keeps its index and distance."""
    W, H, cap, n = 640, 480, 4096, 4
    frames = _two_layer_views(oracle, W, H, n)
    V = tinyorb.ORB_BAND_VERIFIED
    with _program(tinyorb, W, H, cap, n, tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        counts, recs = _records(prog, n, cap)
        prog.match_consecutive(n)
        prog.verify_epipolar(n, inlier_px=2.0)
        vm = [prog.verify_epipolar_read(f, cap) for f in range(n - 1)]
        vmodels = np.array([v[0] for v in vm])
        assert all(int(s) in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL) for s in vmodels["status"])
        prog.match_epipolar(n, source=V, band_px=2.0)
        kept = inliers = 0
        for f in range(n - 1):
            got = prog.match_epipolar_read(f, cap)
            cand = br.members(recs[f][0], recs[f + 1][0], vmodels[f]["h"], band_px=2.0)
            want = br.band_pair(recs[f][0], recs[f][1], recs[f + 1][0], recs[f + 1][1], vmodels[f]["h"], band_px=2.0, cap=cap, candidates=cand)
            assert got.tobytes() == want.tobytes(), (f, np.nonzero(got != want)[0][:5])
            bf = prog.match_read(f, int(counts[f]))
            qq, tj = cand
            inside = np.zeros(int(counts[f]), bool)
            inside[qq[tj == bf["index"][qq]]] = True
            g = got[:counts[f]]
            assert np.array_equal(g["index"][inside], bf["index"][inside]) and np.array_equal(g["distance"][inside], bf["distance"][inside])
            assert np.all(g["second"][inside] >= bf["second"][inside])
            kept += int(inside.sum())
            inliers += int(vm[f][1][:counts[f]].sum())
        # about 3 500 correct matches per pair, 98 % of them inliers of F at inlier_px 2: most lie in the band
        assert kept > 1500 and inliers > 1500, (kept, inliers)
        _check(prog, 3, cap, recs, V, vmodels=vmodels, band_px=2.0, radius_px=32.0)
        _check(prog, 2, cap, recs, V, vmodels=vmodels, band_px=1.0, radius_px=16.0, octave_window=1, scale=True)


# ---- state, arguments, streams, buffers --------------------------------------------------------------------------------------
def test_state_arguments_and_ordering(tinyorb, oracle):
    import torch
    W, H, cap = 320, 240, 800
    frames = _frames(oracle, W, H)[:4]
    V, HM = tinyorb.ORB_BAND_VERIFIED, tinyorb.ORB_BAND_HOST
    host = np.tile(DIAGONAL.reshape(1, 9), (4, 1))  # one more than the pairs, for the call that asks for five frames

    def code(**kw):
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_epipolar(**kw)
        return e.value.code

    with _program(tinyorb, W, H, cap, 4, tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_epipolar_read(0, cap)  # no band call yet
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.extract_batch_host(frames)
        assert code(n_frames=4) == tinyorb.ORB_ESTATE  # verified source before any epipolar verification
        prog.match_consecutive(4)
        prog.verify_consecutive(4)
        assert code(n_frames=4) == tinyorb.ORB_ESTATE  # the homography verifier is not the source
        for kw in (dict(n_frames=5, source=HM, models=host), dict(n_frames=1, source=HM, models=host), dict(n_frames=4, source=HM),
                   dict(n_frames=4, source=V, models=host), dict(n_frames=4, source=2, models=host), dict(n_frames=4, source=2),
                   dict(n_frames=4, source=HM, models=host, flags=2), dict(n_frames=4, source=HM, models=host, reserved=(0, 0, 1)),
                   dict(n_frames=4, source=HM, models=host, reserved=(1, 0, 0)), dict(n_frames=4, source=HM, models=host, band_px=-1.0),
                   dict(n_frames=4, source=HM, models=host, band_px=float("nan")), dict(n_frames=4, source=HM, models=host, band_px=float("inf")),
                   dict(n_frames=4, source=HM, models=host, radius_px=-0.5), dict(n_frames=4, source=HM, models=host, radius_px=float("nan")),
                   dict(n_frames=4, source=HM, models=host, radius_px=float("inf"))):
            assert code(**kw) == tinyorb.ORB_EINVAL, kw
        prog.verify_epipolar(3, seed=3)
        assert code(n_frames=4) == tinyorb.ORB_EINVAL  # three pairs, two verified
        assert code(n_frames=3, models=host) == tinyorb.ORB_EINVAL
        counts, recs = _records(prog, 4, cap)
        vmodels = np.array([prog.verify_epipolar_read(f, 0)[0] for f in range(2)])
        one = [g.tobytes() for g in _check(prog, 3, cap, recs, V, vmodels=vmodels)]
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_epipolar_read(2, cap)  # two pairs only
        assert e.value.code == tinyorb.ORB_EINVAL
        C.check_read_arguments(tinyorb, prog, tinyorb.load_library().orb_match_epipolar_read, 2, 8, head=False)
        # the other stages' results are untouched by band calls
        prog.match_guided(4, source=tinyorb.ORB_GUIDE_VERIFIED, radius_px=3.0)
        prog.track_consecutive(4)

        def others():
            return [prog.match_read(f, cap).tobytes() + prog.verify_read(f, cap)[0].tobytes() + prog.verify_read(f, cap)[1].tobytes() +
                    prog.verify_epipolar_read(f, cap)[0].tobytes() + prog.verify_epipolar_read(f, cap)[1].tobytes() +
                    prog.match_guided_read(f, cap).tobytes() + prog.track_read(f, cap).tobytes() for f in range(2)] + [prog.track_frames(4).tobytes()]

        before = others()
        prog.match_epipolar(3)
        prog.match_epipolar(4, source=HM, models=host, band_px=3.0, radius_px=20.0)
        assert others() == before
        # a band call on a second stream, then an epipolar verification on the first that overwrites the models: it waits
        s = torch.cuda.Stream(device=0)
        prog.match_epipolar(3, stream=s.cuda_stream)
        prog.verify_epipolar(3, seed=5, hypotheses=64)
        assert [prog.match_epipolar_read(f, cap).tobytes() for f in range(2)] == one
        v2 = np.array([prog.verify_epipolar_read(f, 0)[0] for f in range(2)])
        _check(prog, 3, cap, recs, V, vmodels=v2, stream=s.cuda_stream)  # behind that verification, on the other stream
        hostrec = [g.tobytes() for g in _check(prog, 4, cap, recs, HM, host=host, band_px=3.0, stream=s.cuda_stream)]
        assert [g.tobytes() for g in _check(prog, 4, cap, recs, HM, host=host, band_px=3.0)] == hostrec  # back on the batch's stream
        # a new batch, or another output set: the verification is stale; host models need none
        prog.extract_batch_host(frames)
        assert code(n_frames=3) == tinyorb.ORB_ESTATE
        prog.match_epipolar(4, source=HM, models=host)
        prog.match_consecutive(4)
        prog.verify_epipolar(4)
        prog.batch_select_output(1)
        assert code(n_frames=3) == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        counts, recs = _records(prog, 4, cap)
        vmodels = np.array([prog.verify_epipolar_read(f, 0)[0] for f in range(3)])
        _check(prog, 4, cap, recs, V, vmodels=vmodels)
        # guided and track sources stay as they were
        with pytest.raises(tinyorb.OrbError) as e:
            prog.match_guided(4, source=3)
        assert e.value.code == tinyorb.ORB_EINVAL
