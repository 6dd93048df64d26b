"""The matcher, the verifier, guided matching and tracks on constructed records (tests/constructed.py): a batch of blank frames is
extracted, its slabs are overwritten with records built for the edges the kernels were written around, and every record each stage
writes is compared byte for byte with the restatement and with the outcome the construction implies -- ties across the matcher's
tile, chunk and workgroup boundaries, a unique best in the last partial tile, capacity edges of the three matcher forms, chains
that need every pointer-doubling round, many links to one target in both forms of k_track_link, the keyframe walk across its
63-frame chunks, the verifier's FEW / DEGENERATE / MINIMAL outcomes and refit sums around 256 candidates, and windows that end
exactly on a target."""
import numpy as np
import pytest

import constructed as C
import guided_ref as gr
import track_ref as tr
import verify_ref as vr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
NONE = 0xFFFFFFFF
_MATCH_FORMS = {"fp4": {}, "i8": {"TINYORB_MATCH_I8": "1"}, "valu": {"TINYORB_MATCH_VALU": "1"}}


def _match_form(monkeypatch, form):
    """As tests/test_gpu_parity.py: fp4 the default, i8 the int8 matrix-core form, valu the vector-unit kernel (read once per program)."""
    for k in ("TINYORB_MATCH_I8", "TINYORB_MATCH_VALU"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _MATCH_FORMS[form].items():
        monkeypatch.setenv(k, v)


def _program(tinyorb, W, H, cap, B, depth=2):
    """A program holding a batch of B blank frames: the slabs the constructions overwrite."""
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR, max_batch=B)
    prog = tinyorb.OrbProgram(cfg).init()
    prog.extract_batch_host(np.zeros((B, H, W, 4), np.uint8))
    return prog


def _corners_for(rng, descs, W, H):
    return [C.distinct_corners(rng, len(d), W, H) for d in descs]


def _check_matches(prog, counts, descs, cap):
    """orb_match_consecutive over the injected frames: every pair's records against the dense argmin."""
    n = len(counts)
    prog.match_consecutive(n)
    out = []
    for f in range(n - 1):
        na, nb = min(int(counts[f]), cap), min(int(counts[f + 1]), cap)
        got = prog.match_read(f, na)
        want = C.match_ref(descs[f][:na], descs[f + 1][:nb])
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            raise AssertionError((f, na, nb, bad[:5], got[bad[:5]], want[bad[:5]]))
        out.append(got)
    return out


def _agree(got, exp):
    """Construction's records: index and distance exact; second exact where the construction knows it (two planted copies or more),
    otherwise only bounded by it (0xFFFF in exp: second > distance + 40)."""
    assert np.array_equal(got["index"], exp["index"]), (got, exp)
    assert np.array_equal(got["distance"], exp["distance"]), (got, exp)
    known = exp["second"] != 0xFFFF
    assert np.array_equal(got["second"][known], exp["second"][known]), (got, exp)
    assert np.all(got["second"][~known].astype(int) > got["distance"][~known].astype(int) + 40), got


# ---- matcher -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(_MATCH_FORMS))
def test_matcher_edges(tinyorb, monkeypatch, form):
    """Ties planted on both sides of the 16-, 64- and 256-index boundaries (the smallest index wins, second == distance), more than
    one workgroup row of queries, a unique best at candidate nb - 1 for nb = 1, 15, 17, 63, 65, 129, 207 (the partial tile's mask),
    distance 0 and 256, all-zero and all-one descriptors, empty frames on either side, and a raw counter above the capacity."""
    _match_form(monkeypatch, form)
    rng = np.random.default_rng(100)
    W = H = 256
    cap = 700
    pairs = []  # (qd, td, expected records of the first len(exp) queries, raw target counter or None)
    groups = [[15, 16], [63, 64], [255, 256], [31, 32, 47], [127, 128], [0, 599], [511, 512], [79, 80, 96, 257], [300]]
    qd, td, exp = C.planted_ties(rng, 300, 600, groups)
    pairs.append((qd, td, exp, None))
    for nb in (1, 15, 17, 63, 65, 129, 207):
        pairs.append(C.last_is_best(rng, 70, nb) + (None,))
    pairs.append(C.extremes(rng, 40) + (None,))
    pairs.append(C.all_at_256(3, 5) + (None,))
    pairs.append(C.all_at_256(3, 1) + (None,))
    e = np.zeros(0, tinyorb.MATCH_DTYPE)
    pairs.append((C.random_desc(rng, 5), C.random_desc(rng, 0), e, None))   # nb = 0
    pairs.append((C.random_desc(rng, 0), C.random_desc(rng, 5), e, None))   # na = 0
    qd, td, exp = C.last_is_best(rng, 70, cap)
    pairs.append((qd, td, exp, cap + 500))  # the raw counter of the target frame above the capacity: its first cap records count
    descs, counts = [], []
    for qd, td, _, raw in pairs:
        descs += [qd, td]
        counts += [len(qd), len(td) if raw is None else raw]
    with _program(tinyorb, W, H, cap, len(descs)) as prog:
        C.inject(prog, counts, _corners_for(rng, descs, W, H), descs)
        recs = _check_matches(prog, counts, descs, cap)
    for k, (qd, td, exp, _) in enumerate(pairs):
        got = recs[2 * k][:len(exp)]
        if len(exp):
            _agree(got, exp)
        if k == 0:
            assert got["second"][0] == got["distance"][0]
    # nb = 1: no runner-up at all
    assert np.all(recs[2]["second"] == 0xFFFF) and np.all(recs[2]["index"] == 0)
    assert np.all(recs[2 * 11]["index"] == NONE) and np.all(recs[2 * 11]["distance"] == 0xFFFF)  # nb = 0


@pytest.mark.parametrize("form,cap", [("fp4", 16383), ("i8", 16128), ("i8", 16129), ("i8", 16383), ("valu", 16383)])
def test_matcher_capacity_edges(tinyorb, monkeypatch, form, cap):
    """A full target frame at the matrix-core key's edges: fp4 at 16 383 (candidate 16 382's key is 1 at distance 256); int8 at
    16 128 (its largest), 16 129 and 16 383 (past its key: the vector unit).  Candidate cap - 1 is the only one at distance 256 for
    half of the queries and the best of the others; every form gives the dense argmin's records."""
    _match_form(monkeypatch, form)
    rng = np.random.default_rng(cap)
    td = C.random_desc(rng, cap)
    Z = td[cap - 1]
    qd = np.concatenate([np.tile(~Z, (128, 1)), np.stack([C.flip(Z, int(k), rng) for k in rng.integers(0, 30, 128)])])
    with _program(tinyorb, 128, 128, cap, 2) as prog:
        descs = [qd, td]
        C.inject(prog, [len(qd), cap], _corners_for(rng, descs, 128, 128), descs)
        got = _check_matches(prog, [len(qd), cap], descs, cap)[0]
    assert np.all(got["index"][:128] != cap - 1) and np.all(got["distance"][:128] < 256)
    assert np.all(got["index"][128:] == cap - 1) and np.all(got["second"][128:] > got["distance"][128:])


def test_matcher_vector_unit_at_2_pow_23(tinyorb):
    """The vector-unit key (d << 23) | j at its limit: cap 2^23, 64 queries against 2^23 candidates, the best at j = 2^23 - 1 and
    the runner-up at 2^22 -- from the construction alone (constructed.last_of_huge)."""
    cap = 1 << 23
    rng = np.random.default_rng(23)
    qd, td, exp = C.last_of_huge(rng, 64, cap)
    W, H = 4096, 2048  # 2^23 pixels: every target at its own octave-0 pixel
    j = np.arange(cap)
    tc = C.corners(j % W, j // W, 0)
    with _program(tinyorb, W, H, cap, 2) as prog:
        C.inject(prog, [64, cap], [C.distinct_corners(rng, 64, W, H), tc], [qd, td])
        del td, tc
        prog.match_consecutive(2)
        got = prog.match_read(0, 64)
    assert got.tobytes() == exp.tobytes(), (got[:4], exp[:4])


# ---- tracks ------------------------------------------------------------------------------------------------------------------
def _sources(tinyorb, prog, n):
    prog.match_consecutive(n)
    prog.verify_consecutive(n)
    prog.match_guided(n, source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=4.0)


def _links(prog, source, n_frames, cap, counts):
    out = []
    for f in range(n_frames - 1):
        nq, nt = int(counts[f]), int(counts[f + 1])
        if source == 0:
            out.append(tr.pair_links(source, prog.match_read(f, cap), nq, nt, inlier=prog.verify_read(f, cap)[1]))
        elif source == 1:
            out.append(tr.pair_links(source, prog.match_guided_read(f, cap), nq, nt))
        else:
            out.append(tr.pair_links(source, prog.match_read(f, cap), nq, nt))
    return out


def _check_tracks(prog, n_frames, cap, source, want_tracks=None, want_frames=None, **kw):
    """Track call, then every OrbTrack (cap of each frame) and OrbTrackFrame against the restatement over the device's own source
    records, and the stored keypoints' entries against the construction's tracks; want_frames: (keyframe, ref_keyframe, shared)."""
    prog.track_consecutive(n_frames, source=source, **kw)
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    want_t, want_f = tr.track(counts, cap, _links(prog, source, n_frames, cap, counts), source=source, **kw)
    for f in range(n_frames):
        got = prog.track_read(f, cap)
        if got.tobytes() != want_t[f].tobytes():
            bad = np.nonzero(got != want_t[f])[0]
            raise AssertionError((f, source, kw, bad[:5], got[bad[:5]], want_t[f][bad[:5]]))
        if want_tracks is not None:
            assert got[:counts[f]].tobytes() == want_tracks[f].tobytes(), (f, source, kw)
    got = prog.track_frames(n_frames)
    assert got.tobytes() == want_f.tobytes(), (source, kw, got, want_f)
    if want_frames is not None:
        key, ref, shared = want_frames
        assert np.array_equal(got["keyframe"], key) and np.array_equal(got["ref_keyframe"], ref), (source, kw, got)
        assert np.array_equal(got["shared"], shared), (source, kw, got)
    return got


def _inject_chains(prog, ch):
    C.inject(prog, ch["counts"], list(ch["corners"]), list(ch["desc"]))


def test_whole_batch_chains(tinyorb):
    """Permutation chains through the whole batch for n_frames from 2 to 257: every head is (0, the composed permutation), every
    tail the last frame, only frame 0 a keyframe (shared = n_0) -- and the chain needs every doubling round."""
    rng = np.random.default_rng(200)
    W = H = 128
    n = 24
    with _program(tinyorb, W, H, 32, 257) as prog:
        for F in (2, 3, 4, 5, 9, 17, 33, 65, 129, 256, 257):
            starts = np.zeros((F, n), bool)
            starts[0] = True
            ch = C.chains(rng, starts, W, H)
            _inject_chains(prog, ch)
            _sources(tinyorb, prog, F)
            for src in (0, 1, 2):
                fr = _check_tracks(prog, F, 32, src, ch["tracks"], C.steady_keyframes(F, n, n))
                assert fr["keyframe"].sum() == 1 and np.all(fr["shared"] == n)
            t = prog.track_read(F - 1, n)
            assert np.all(t["head_frame"] == 0) and np.array_equal(t["head_index"][ch["perm"][F - 1]], ch["perm"][0])


def test_chains_of_4096_frames(tinyorb):
    """4 096 frames of 64 x 64 (the largest n_frames), 16 keypoints each, one permutation chain per keypoint through all of them:
    12 doubling rounds, 66 chunks of the keyframe walk."""
    rng = np.random.default_rng(201)
    F, n = 4096, 16
    starts = np.zeros((F, n), bool)
    starts[0] = True
    ch = C.chains(rng, starts, 64, 64)
    with _program(tinyorb, 64, 64, 64, F) as prog:
        _inject_chains(prog, ch)
        prog.match_consecutive(F)
        prog.verify_consecutive(F)
        for src in (0, 2):
            _check_tracks(prog, F, 64, src, ch["tracks"], C.steady_keyframes(F, n, n))
        _check_tracks(prog, F, 64, 2, ch["tracks"], C.steady_keyframes(F, n, n, max_gap=63), max_gap=63)


def test_exact_track_lengths(tinyorb):
    """Tracks of exactly 2^k and 2^k + 1 links, k = 0 .. 7, inside one 256-frame batch, next to chains through the whole batch."""
    rng = np.random.default_rng(202)
    lengths = sorted({1 << k for k in range(8)} | {(1 << k) + 1 for k in range(8)})
    starts, spans = C.exact_lengths(256, lengths, 8)
    ch = C.chains(rng, starts, 128, 128)
    with _program(tinyorb, 128, 128, 32, 256) as prog:
        _inject_chains(prog, ch)
        _sources(tinyorb, prog, 256)
        for src in (0, 1, 2):
            _check_tracks(prog, 256, 32, src, ch["tracks"])
        for s, a, L in spans:
            t = prog.track_read(a + L, 32)[ch["perm"][a + L, s]]
            assert (t["head_frame"], t["head_index"], t["tail_frame"]) == (a, ch["perm"][a, s], a + L), (s, a, L)


@pytest.mark.parametrize("cap,global_keys", [(16320, False), (16321, False), (16320, True)], ids=["lds", "global", "forced-global"])
def test_link_contention(tinyorb, monkeypatch, cap, global_keys):
    """Many queries whose best target is one j near cap - 1: at equal distance the smallest i wins; at different distances the
    smallest distance wins even when its i is the largest.  k_track_link's LDS form at cap 16 320, its global form at 16 321 and
    with TINYORB_TRACK_GLOBAL_KEYS=1."""
    monkeypatch.delenv("TINYORB_TRACK_GLOBAL_KEYS", raising=False)
    if global_keys:
        monkeypatch.setenv("TINYORB_TRACK_GLOBAL_KEYS", "1")
    rng = np.random.default_rng(cap)
    groups = [(cap - 1, [(3, 5), (4000, 5), (cap - 2, 5)]), (cap - 2, [(7, 9), (120, 7), (cap - 1, 3)]),
              (cap - 3, [(8, 4), (9, 4), (10, 4), (11, 4)]), (cap - 17, [(12, 2), (cap - 3, 1)]), (0, [(13, 0), (14, 0)])]
    qd, td, win, planted = C.contention(rng, cap, cap, groups)
    pos = C.distinct_corners(rng, cap, 128, 128)
    with _program(tinyorb, 128, 128, cap, 2) as prog:
        C.inject(prog, [cap, cap], [pos, pos], [qd, td])
        prog.match_consecutive(2)
        prog.match_guided(2, source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=1e6)
        for src in (1, 2):
            _check_tracks(prog, 2, cap, src)
            t0, t1 = prog.track_read(0, cap), prog.track_read(1, cap)
            for j, i in win.items():
                assert t1["prev"][j] == i and t0["next"][i] == j, (src, j, i, t1["prev"][j])
            assert np.count_nonzero(t0["next"] != NONE) == len(groups)


def test_keyframe_walk_across_chunks(tinyorb):
    """TK-5 where k_track_key's 63-frame chunks meet: max_gap 62 .. 65 on perfect chains, and a steady loss of one track per frame
    whose permille clause first fires at gaps 62 .. 65 (keyframes on both sides of 63 and 126), with min_gap and min_shared."""
    rng = np.random.default_rng(203)
    F, n = 200, 256
    with _program(tinyorb, 64, 64, n, F) as prog:
        starts = np.zeros((F, 32), bool)
        starts[0] = True
        ch = C.chains(rng, starts, 64, 64)
        _inject_chains(prog, ch)
        prog.match_consecutive(F)
        for g in (62, 63, 64, 65):
            _check_tracks(prog, F, n, 2, ch["tracks"], C.steady_keyframes(F, 32, 32, max_gap=g), max_gap=g)
        ch = C.chains(rng, C.steady_loss(F, n), 64, 64)
        _inject_chains(prog, ch)
        _sources(tinyorb, prog, F)
        for G in (62, 63, 64, 65):
            p = C.permille_for_gap(n, G)
            for kw in (dict(keep_permille=p), dict(keep_permille=p, min_gap=G + 3), dict(keep_permille=1, min_shared=n - G + 1)):
                for src in ((0, 1, 2) if G == 63 else (2,)):
                    fr = _check_tracks(prog, F, n, src, ch["tracks"], C.steady_keyframes(F, n, n - 1, **kw), **kw)
            assert fr["keyframe"][G] == 1 and fr["keyframe"][2 * G] == 1 and fr["keyframe"][1:G].sum() == 0


# ---- verification ------------------------------------------------------------------------------------------------------------
def _verify(prog, c, d, W, H, cap, **params):
    C.inject(prog, [len(c[0]), len(c[1])], list(c), list(d))
    prog.match_consecutive(2)
    prog.verify_consecutive(2, **params)
    m = prog.match_read(0, len(c[0]))
    rec, mask = prog.verify_read(0, cap)
    ref, rmask = vr.verify_pair(c[0], c[1], m, W, H, 0, cap=cap, **params)
    assert rec.tobytes() == ref.tobytes(), (params, rec, ref)
    assert np.array_equal(mask, rmask), params
    return rec, mask


def test_verification_outcomes(tinyorb):
    """FEW at 3 candidates; DEGENERATE with an all-zero mask on 40 collinear ones; 4 and 5 in general position; M = 255, 256, 257,
    511 and 4 097 exact inliers of a translation plus 30 % outliers around the refit's 256 partial sums (status OK, at least the
    planted inliers); two equal-size motions; 1 and 4 096 hypotheses; a seeded construction the restatement calls MINIMAL."""
    W = H = 256
    cap = 8192
    rng = np.random.default_rng(300)
    with _program(tinyorb, W, H, cap, 2) as prog:
        for M in (3, 4, 5):
            c, d, _ = C.correspondences(rng, M, 0, W, H)
            rec, mask = _verify(prog, c, d, W, H, cap)
            assert rec["candidates"] == M and int(rec["status"]) == (vr.VERIFY_FEW if M == 3 else vr.VERIFY_OK)
            assert mask.sum() == (0 if M == 3 else M)
        c, d = C.collinear(rng, 40, W, H)
        rec, mask = _verify(prog, c, d, W, H, cap)
        assert int(rec["status"]) == vr.VERIFY_DEGENERATE and not mask.any() and rec["candidates"] == 40
        for M in (255, 256, 257, 511, 4097):
            c, d, inl = C.correspondences(rng, M, int(0.3 * M), W, H)
            rec, mask = _verify(prog, c, d, W, H, cap)
            assert int(rec["status"]) == vr.VERIFY_OK and rec["inliers"] >= M and np.all(mask[:len(inl)][inl] == 1), (M, rec)
            if M == 257:
                for hyps in (1, 4096):
                    _verify(prog, c, d, W, H, cap, hypotheses=hyps, seed=hyps)
        c, d = C.two_motions(rng, 50, W, H)
        rec, mask = _verify(prog, c, d, W, H, cap)
        assert int(rec["status"]) == vr.VERIFY_OK and rec["inliers"] == 50 and (mask[:50].all() or mask[50:100].all())
        c, d = C.jittered(np.random.default_rng(C.MINIMAL_SEED), 40, W, H)
        rec, _ = _verify(prog, c, d, W, H, cap, **C.MINIMAL_PARAMS)
        assert int(rec["status"]) == vr.VERIFY_MINIMAL


# ---- guided matching ---------------------------------------------------------------------------------------------------------
def _guided(tinyorb, prog, qc, qd, tc, td, cap, radius, raw_t=None, **kw):
    """Inject one pair (the target frame's raw counter raw_t, default its record count), run the guided call with the identity
    and compare with the restatement; returns the records of the stored queries."""
    C.inject(prog, [len(qc), len(tc) if raw_t is None else raw_t], [qc, tc], [qd, td])
    prog.match_guided(2, source=tinyorb.ORB_GUIDE_IDENTITY, radius_px=radius, **kw)
    nt = min(len(tc) if raw_t is None else raw_t, cap)
    got = prog.match_guided_read(0, cap)
    want = gr.guided_pair(qc, qd, tc[:nt], td[:nt], gr.IDENTITY, radius, kw.get("octave_window", 0), kw.get("scale_radius", False),
                          cap=cap)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        raise AssertionError((radius, kw, bad[:5], got[bad[:5]], want[bad[:5]]))
    return got[:len(qc)]


def test_guided_window_edges(tinyorb):
    """GM-3's inclusive edge: a target at exactly |x - px| = r or |y - py| = r is in the window, one pixel beyond or with r one ulp
    smaller it is not -- integer r on octave-0 coordinates, r = 2.5 on the half-pixel centres of octave-1 queries."""
    rng = np.random.default_rng(400)
    with _program(tinyorb, 256, 256, 256, 2) as prog:
        for octave, r in ((0, 3.0), (0, 1.0), (1, 2.5)):
            qc, qd, tc, td, cases = C.window_edges(rng, r, octave)
            below = float(np.nextafter(np.float32(r), np.float32(0)))
            on = _guided(tinyorb, prog, qc, qd, tc, td, 256, r)
            off = _guided(tinyorb, prog, qc, qd, tc, td, 256, below)
            for q, e, c in cases:
                assert (on["index"][q], on["distance"][q], on["second"][q]) == (e, 1, 10), (octave, r, q, on[q])
                assert (off["index"][q], off["distance"][q], off["second"][q]) == (c, 10, 0xFFFF), (octave, r, q, off[q])


def test_guided_cells(tinyorb):
    """Ties between targets in different grid cells stored in the opposite order to their indices (the smaller index wins), a cell
    with a target at every pixel under a capacity cut and a raw counter above the capacity, windows at the frame's corners and
    outside it, and the GM-6 equivalence with the matcher on the same constructed frames."""
    rng = np.random.default_rng(401)
    cap = 256
    with _program(tinyorb, 256, 256, cap, 2) as prog:
        qc, qd, tc, td, exp = C.cell_ties(rng)
        got = _guided(tinyorb, prog, qc, qd, tc, td, cap, 16.0)
        assert got.tobytes() == exp.tobytes()
        qc, qd, tc, td = C.dense_cell(rng, 96, 96, 300)
        for raw in (None, 364):  # 364 records: with the raw counter, the capacity cuts the frame at 256
            g = _guided(tinyorb, prog, qc, qd, tc[:cap], td[:cap], cap, 16.0, raw_t=raw)
            assert np.array_equal(g["index"], np.arange(64)) and np.all(g["distance"] == 3)
        # GM-6 on these frames: identity, radius over the frame = the matcher
        g = _guided(tinyorb, prog, qc, qd, tc[:cap], td[:cap], cap, 1e6)
        prog.match_consecutive(2)
        assert g.tobytes() == prog.match_read(0, 64).tobytes()
        # windows at the four corners of the frame: each query's own pixel holds its best (2 bits); a model moving every
        # prediction out of the frame leaves every query without a target
        xs, ys = np.array([0, 255, 0, 255, 1]), np.array([0, 0, 255, 255, 254])
        qd = C.random_desc(rng, 5)
        qc = C.corners(xs, ys, rng=rng)
        tc = np.concatenate([C.corners(xs, ys, rng=rng), C.distinct_corners(rng, 40, 256, 256, 20)])
        td = np.concatenate([C.flip(qd, 2, rng), C.random_desc(rng, 40)])
        g = _guided(tinyorb, prog, qc, qd, tc, td, cap, 3.0)
        assert np.array_equal(g["index"], np.arange(5)) and np.all(g["distance"] == 2)
        prog.match_guided(2, source=tinyorb.ORB_GUIDE_HOST, radius_px=3.0, models=np.array([[1, 0, 5000, 0, 1, -3000, 0, 0, 1]]))
        assert np.all(prog.match_guided_read(0, cap)["index"] == NONE)


def test_guided_octaves(tinyorb):
    """octave_window 1 and 2 and scale_radius at the top octave of depth 4: a query at octave 3 (level-0 centre 83.5, 83.5) with
    targets at octaves 3 (8 px away, 6 bits), 2 (2 px, 2 bits), 1 (1 px, 4 bits) and 0 (0.5 px, 1 bit)."""
    rng = np.random.default_rng(402)
    qd = C.random_desc(rng, 1)
    qc = C.corners([10], [10], 3, rng=rng)
    tc = C.corners([11, 21, 41, 84], [10, 20, 41, 84], [3, 2, 1, 0], rng=rng)
    td = np.stack([C.flip(qd[0], k, rng) for k in (6, 2, 4, 1)])
    with _program(tinyorb, 256, 256, 64, 2, depth=4) as prog:
        assert prog.level_size(3) == (32, 32)
        cases = [(2.0, True, 0, 3, 1), (2.0, True, 1, 0, 6), (2.0, True, 2, 1, 2), (2.0, False, 0, 3, 1), (2.0, False, 1, NONE, 0xFFFF),
                 (2.0, False, 2, 1, 2)]
        for r, scale, ow, idx, dist in cases:
            g = _guided(tinyorb, prog, qc, qd, tc, td, 64, r, octave_window=ow, scale_radius=scale)
            assert (g["index"][0], g["distance"][0]) == (idx, dist), (r, scale, ow, g)
