"""orb_match_pairs and orb_verify_pairs on the GPU: every row, record and inlier byte against the CPU
restatement (tests/pairs_ref.py) fed with the records the device holds.  No tolerance anywhere.

The programs are 64 x 48 (160 x 120 for the extracted scene) with zero images; counters, corners and descriptors are then written
over the batch (constructed.inject).

Shapes.  The matchers work on 16-candidate tiles (the last one masked), 64-candidate LDS chunks in two buffers, 256-query
workgroups (fp4) or 128-query waves (vector unit): at capacity 300 the query counts 0, 1, 15 .. 17, 63 .. 65, 255 .. 257, 300 and
a raw counter above the capacity meet the candidate counts 0, 1, 15 .. 17, 63 .. 65, 127 .. 129 and 300 in one list, on both matcher
forms.  The gather compacts 256 queries per pass: the verifier's query counts are 0, 3, 4, 7, 8, 255 .. 257 and 600
at capacity 600, between frames ten apart, forward and backward; the score kernels take 64 hypotheses per workgroup: 1, 64, 65
and 512."""
import numpy as np
import pytest

import constructed as C
import pairs_ref as pf
import place_ref as pr
import place_scene
import verify_ref as vr
from test_pairs_ref import check_scene_relations

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48
THR = 20.0 / 255.0
_MATCH_FORMS = {"fp4": {}, "valu": {"TINYORB_MATCH_VALU": "1"}}


def _match_form(monkeypatch, form):
    """As tests/test_gpu_constructed.py: fp4 the default, valu the vector-unit kernel (read once per program)."""
    for k in ("TINYORB_MATCH_I8", "TINYORB_MATCH_VALU"):
        monkeypatch.delenv(k, raising=False)
    for k, v in _MATCH_FORMS[form].items():
        monkeypatch.setenv(k, v)


def _program(tinyorb, cap, B, W=W0, H=H0, flags=0, blank=True):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=B, flags=flags,
                            fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    prog = tinyorb.OrbProgram(cfg).init()
    if blank:
        prog.extract_batch_host(np.zeros((B, H, W, 4), np.uint8))
    return prog


def _code(tinyorb, fn, *a, **kw):
    with pytest.raises(tinyorb.OrbError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def _check_rows(prog, counts, descs, cap, pairs, want=None, stream=None, call=True):
    """One orb_match_pairs call (call=False: the last one's rows) and the stored queries' records of every row against the
    restatement.  Returns the rows."""
    if call:
        prog.match_pairs(pairs, stream=stream)
    want = pf.match_pairs(counts, descs, cap, pairs) if want is None else want
    rows = []
    for i, w in enumerate(want):
        got = prog.match_pairs_read(i, len(w))
        if got.tobytes() != w.tobytes():
            bad = np.nonzero(got != w)[0]
            raise AssertionError((i, tuple(pf.as_list(pairs)[i]), len(w), bad[:5], got[bad[:5]], w[bad[:5]]))
        rows.append(got)
    return rows


def _check_verify(prog, counts, corners, rows, cap, pairs, W, H, model, n_pairs=None, want=None, stream=None, call=True, **params):
    """One orb_verify_pairs call (call=False: the last one's results) and every record and inlier byte against the restatement on
    `rows`.  Returns the records."""
    n = len(pairs) if n_pairs is None else n_pairs
    if call:
        prog.verify_pairs(n, model=model, stream=stream, **params)
    want = pf.verify_pairs(counts, corners, rows, cap, pairs, W, H, model=model, n_pairs=n, **params) if want is None else want
    recs = []
    for i, (wr, wm) in enumerate(want):
        rec, mask = prog.verify_pairs_read(i, cap)
        assert rec.tobytes() == wr.tobytes(), (model, params, i, tuple(pf.as_list(pairs)[i]), rec, wr)
        assert mask.tobytes() == wm.tobytes(), (model, params, i, np.nonzero(mask != wm)[0][:8])
        recs.append(rec)
    return recs


# ---- the matcher ---------------------------------------------------------------------------------------------------------------
MCAP = 300
TARGET_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)
QUERY_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300, MCAP + 77)  # the last: a raw counter above the capacity
_matcher_cache = []


def _matcher_batch():
    """The frames of the matcher tests, built once: one target frame per candidate count (frames 0 .. 11), one query frame per query
    count (12 .. 24), then the constructed pairs, every other one with its target frame stored first.  Every frame holds stale
    records behind its count.  Returns (counts, descs, constructed: [(query frame, target frame, expected records)])."""
    if _matcher_cache:
        return _matcher_cache[0]
    rng = np.random.default_rng(27)
    counts, descs = [], []

    def frame(raw, d=None):
        stored = min(raw, MCAP)
        d = C.random_desc(rng, stored) if d is None else d
        assert len(d) == stored
        counts.append(raw)
        descs.append(np.concatenate([d, C.random_desc(rng, min(9, MCAP - stored))]))  # stale rows behind the count
        return len(counts) - 1

    for n in TARGET_COUNTS + QUERY_COUNTS:
        frame(n)
    groups = [[15, 16], [63, 64], [255, 256], [31, 32, 47], [127, 128], [0, 299], [79, 80, 96, 257], [290]]
    built = [C.planted_ties(rng, 300, 300, groups)] + [C.last_is_best(rng, 70, nb) for nb in (1, 17, 65, 129)]
    built += [C.extremes(rng, 40), C.all_at_256(3, 5), C.all_at_256(3, 1)]
    constructed = []
    for k, (qd, td, exp) in enumerate(built):
        if k & 1:
            t = frame(len(td), td)
            q = frame(len(qd), qd)
        else:
            q = frame(len(qd), qd)
            t = frame(len(td), td)
        constructed.append((q, t, exp))
    _matcher_cache.append((np.array(counts, np.uint32), descs, constructed))
    return _matcher_cache[0]


def _agree(got, exp):
    """As tests/test_gpu_constructed.py: index and distance exact; second exact where the construction knows it, else only bounded."""
    assert np.array_equal(got["index"], exp["index"]), (got, exp)
    assert np.array_equal(got["distance"], exp["distance"]), (got, exp)
    known = exp["second"] != 0xFFFF
    assert np.array_equal(got["second"][known], exp["second"][known]), (got, exp)
    assert np.all(got["second"][~known].astype(int) > got["distance"][~known].astype(int) + 40), got


@pytest.mark.parametrize("form", list(_MATCH_FORMS))
def test_matcher_counts_and_constructed_records(tinyorb, monkeypatch, form):
    """Every query count against every candidate count in one list of 156 pairs, all of them backward; then the constructed
    records (ties across the tile, chunk and workgroup boundaries, a unique best at the last candidate, distances 0 and 256) with
    the outcome the construction implies."""
    _match_form(monkeypatch, form)
    counts, descs, constructed = _matcher_batch()
    B = len(counts)
    nt = len(TARGET_COUNTS)
    cross = [(nt + q, t) for q in range(len(QUERY_COUNTS)) for t in range(nt)]
    assert len(cross) == 156 <= pf.capacity(B) == tinyorb.ORB_PAIRS_PER_FRAME * B  # (a list of exactly P: test_matcher_lists)
    with _program(tinyorb, MCAP, B) as prog:
        C.inject(prog, counts, None, descs)
        rows = _check_rows(prog, counts, descs, MCAP, cross)
        assert [len(r) for r in rows[-nt:]] == [MCAP] * nt  # the raw counter above the capacity: its first 300 records
        assert np.all(rows[nt]["index"] == 0xFFFFFFFF) and np.all(rows[nt]["distance"] == 0xFFFF)  # one query, no candidate
        assert np.all(rows[nt + 1]["second"] == 0xFFFF) and np.all(rows[nt + 1]["index"] == 0)     # one candidate: no runner-up
        rows = _check_rows(prog, counts, descs, MCAP, [(q, t) for q, t, _ in constructed])
        for got, (_, _, exp) in zip(rows, constructed):
            _agree(got[:len(exp)], exp)
        assert rows[0]["second"][0] == rows[0]["distance"][0]


@pytest.mark.parametrize("form", list(_MATCH_FORMS))
def test_matcher_lists(tinyorb, monkeypatch, form):
    """Backward, distant and consecutive pairs in one list with a shared target and a duplicate; lists of 1 and of P; every refusal
    of MP-1; a second, shorter call; and the consecutive matcher's own pairs, listed."""
    _match_form(monkeypatch, form)
    counts, descs, _ = _matcher_batch()
    B = len(counts)
    P = pf.capacity(B)
    E = tinyorb.ORB_EINVAL
    with _program(tinyorb, MCAP, B, blank=False) as prog:
        assert _code(tinyorb, prog.match_pairs, [(0, 1)])[0] == tinyorb.ORB_ESTATE  # no batch
        assert _code(tinyorb, prog.match_pairs_read, 0, 1)[0] == tinyorb.ORB_ESTATE
        prog.extract_batch_host(np.zeros((B - 2, H0, W0, 4), np.uint8))  # a batch of B - 2 frames in a program of B
        C.inject(prog, counts[:B - 2], None, descs[:B - 2])
        n = B - 2
        assert _code(tinyorb, prog.match_pairs_read, 0, 1)[0] == tinyorb.ORB_ESTATE  # a batch, no call yet
        mixed = [(24, 3), (3, 24), (20, 21), (21, 20), (0, n - 1), (19, 11), (22, 11), (23, 11), (n - 1, 11), (19, 11), (24, 3)]
        rows = _check_rows(prog, counts, descs, MCAP, mixed)
        assert rows[5].tobytes() == rows[9].tobytes() and rows[0].tobytes() == rows[10].tobytes()  # the duplicates
        _check_rows(prog, counts, descs, MCAP, [(n - 1, 0)])
        full = [(i % n, (i % n + 1 + i // n) % n) for i in range(P)]
        assert pf.violation(full, n, B) is None
        full_rows = _check_rows(prog, counts, descs, MCAP, full)
        # MP-1: none of these calls counts, and the message names the first offending entry
        for bad in ([], full + [(0, 1)], [(0, 1), (n, 0)], [(0, n)], [(0, 1), (2, 3), (5, 5), (n, n)], [(0xFFFFFFFF, 0)], [(B - 1, 0)]):
            code, msg = _code(tinyorb, prog.match_pairs, bad)
            v = pf.violation(bad, n, B)
            assert code == E and v is not None and (v == "count" or "entry %d " % v in msg), (bad[:4], msg)
        _check_rows(prog, counts, descs, MCAP, full, want=full_rows, call=False)
        # a second, shorter call: rows at or past its n_pairs are refused, whatever the first call left there
        _check_rows(prog, counts, descs, MCAP, mixed[:3])
        assert _code(tinyorb, prog.match_pairs_read, 3, 1)[0] == E and _code(tinyorb, prog.match_pairs_read, P, 1)[0] == E
        # a listed (f, f + 1) is orb_match_read(f), byte for byte
        prog.match_consecutive(n)
        rows = _check_rows(prog, counts, descs, MCAP, [(f, f + 1) for f in range(n - 1)])
        for f, r in enumerate(rows):
            assert prog.match_read(f, len(r)).tobytes() == r.tobytes(), f


# ---- the verifier --------------------------------------------------------------------------------------------------------------
VCAP = 600
VERIFY_COUNTS = (0, 3, 4, 7, 8, 255, 256, 257, 600)
_verifier_cache = []


def _verifier_batch():
    """20 frames: the query frame of count n at frame k, its partner at frame 10 + k; a collinear pair at frames 9 and 19.  Counts from
    255 up hold a fifth of outliers and six queries with random descriptors, candidates only under ratio = 1 and max_distance = 256.
    Returns (counts, corners, descs, pairs): every pair forward and backward, and the pair (5, 15) at a second list position."""
    if _verifier_cache:
        return _verifier_cache[0]
    rng = np.random.default_rng(31)
    F = 20
    counts = np.zeros(F, np.uint32)
    corners = [np.zeros(0, C.CORNER_DTYPE)] * F
    descs = [np.zeros((0, 8), np.uint32)] * F
    for k, n in enumerate(VERIFY_COUNTS):
        noise = 6 if n >= 255 else 0
        outliers = n // 5 if n >= 255 else 0
        c, d, _ = C.correspondences(rng, n - noise - outliers, outliers, W0, H0)
        used = set(zip(c[0]["x"].tolist(), c[0]["y"].tolist()))
        free = [(x, y) for y in range(H0) for x in range(W0) if (x, y) not in used]
        pick = [free[i] for i in rng.choice(len(free), noise, replace=False)] if noise else []
        extra = C.corners(np.array([p[0] for p in pick], np.int64), np.array([p[1] for p in pick], np.int64), 0, rng=rng)
        corners[k], descs[k] = np.concatenate([c[0], extra]), np.concatenate([d[0], C.random_desc(rng, noise)])
        corners[10 + k], descs[10 + k] = c[1], d[1]
        counts[k], counts[10 + k] = n, n - noise
    c, d = C.collinear(rng, 12, W0, H0)
    corners[9], descs[9], corners[19], descs[19] = c[0], d[0], c[1], d[1]
    counts[9] = counts[19] = 12
    pairs = [p for k in range(len(VERIFY_COUNTS)) for p in ((k, 10 + k), (10 + k, k))] + [(9, 19), (19, 9), (5, 15)]
    _verifier_cache.append((counts, corners, descs, pairs))
    return _verifier_cache[0]


@pytest.mark.parametrize("hypotheses", [1, 64, 65, 512])
@pytest.mark.parametrize("model", [pf.HOMOGRAPHY, pf.EPIPOLAR])
def test_verifier(tinyorb, model, hypotheses):
    counts, corners, descs, pairs = _verifier_batch()
    with _program(tinyorb, VCAP, len(counts)) as prog:
        C.inject(prog, counts, corners, descs)
        rows = _check_rows(prog, counts, descs, VCAP, pairs)
        status = set()
        for kw in (dict(seed=0), dict(seed=0x9E3779B9), dict(seed=0, ratio=1.0, max_distance=256)):
            recs = _check_verify(prog, counts, corners, rows, VCAP, pairs, W0, H0, model, hypotheses=hypotheses, **kw)
            status |= {int(r["status"]) for r in recs}
            # (5, 15) at list positions 10 and 20: the same candidates -- 249 planted ones, and under the lax filter those of the six
            # random queries whose best is closer than their runner-up -- whatever the two draw streams make of them
            assert recs[10]["candidates"] == recs[20]["candidates"] and (249 < recs[10]["candidates"] <= 255 if "ratio" in kw else recs[10]["candidates"] == 249)
            assert [int(r["candidates"]) for r in recs[:4]] == [0, 0, 3, 3] and recs[18]["candidates"] == 12
            few = 4 if model == pf.HOMOGRAPHY else 8
            assert all((r["status"] == vr.VERIFY_FEW) == (r["candidates"] < few) for r in recs)
            assert recs[18]["status"] == recs[19]["status"] == vr.VERIFY_DEGENERATE  # the collinear pair, both ways
        assert {vr.VERIFY_FEW, vr.VERIFY_DEGENERATE} <= status and (hypotheses < 64 or vr.VERIFY_OK in status)


# ---- state and ordering --------------------------------------------------------------------------------------------------------
def test_state_streams_and_the_other_stages(tinyorb):
    import torch
    counts, corners, descs, pairs = _verifier_batch()
    n, cap = len(counts), VCAP
    L = tinyorb.load_library()
    S, E = tinyorb.ORB_ESTATE, tinyorb.ORB_EINVAL
    with _program(tinyorb, cap, n, flags=tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        C.inject(prog, counts, corners, descs)
        h = prog._handle()
        assert _code(tinyorb, prog.verify_pairs, 1)[0] == S           # before any orb_match_pairs
        assert _code(tinyorb, prog.verify_pairs_read, 0, 1)[0] == S
        rows = _check_rows(prog, counts, descs, cap, pairs)
        assert _code(tinyorb, prog.verify_pairs_read, 0, 1)[0] == S   # matched, not verified
        for kw in (dict(n_pairs=0), dict(n_pairs=len(pairs) + 1), dict(n_pairs=3, model=2), dict(n_pairs=3, hypotheses=4097),
                   dict(n_pairs=3, max_distance=257), dict(n_pairs=3, ratio=-1.0), dict(n_pairs=3, ratio=float("nan")),
                   dict(n_pairs=3, inlier_px=-1.0), dict(n_pairs=3, inlier_px=float("inf")), dict(n_pairs=3, reserved=(0, 1, 0))):
            assert _code(tinyorb, prog.verify_pairs, **kw)[0] == E, kw
        assert _code(tinyorb, prog.verify_pairs_read, 0, 1)[0] == S   # none of those calls counted
        for model in (pf.HOMOGRAPHY, pf.EPIPOLAR):                    # params NULL: the defaults
            assert L.orb_verify_pairs(h, len(pairs), model, None, None) == tinyorb.ORB_OK
            _check_verify(prog, counts, corners, rows, cap, pairs, W0, H0, model, call=False)
        # fewer pairs than matched; the read refuses a pair at or past them
        _check_verify(prog, counts, corners, rows, cap, pairs, W0, H0, pf.HOMOGRAPHY, n_pairs=5, hypotheses=64)
        assert _code(tinyorb, prog.verify_pairs_read, 5, 1)[0] == E
        # the reads' arguments and clipping
        C.check_read_arguments(tinyorb, prog, L.orb_match_pairs_read, len(pairs), 8, head=False)
        C.check_read_arguments(tinyorb, prog, L.orb_verify_pairs_read, 5, 1, head=True)
        # a caller's stream, and the caller's list overwritten as soon as the call returns
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        mine = pf.as_list(pairs).copy()
        prog.match_pairs(mine, stream=s1.cuda_stream)
        mine[:] = (0xFFFFFFFF, 0xFFFFFFFF)
        _check_rows(prog, counts, descs, cap, pairs, want=rows, call=False)
        epi = _check_verify(prog, counts, corners, rows, cap, pairs, W0, H0, pf.EPIPOLAR, stream=s1.cuda_stream, seed=3)
        # orb_match_pairs on another stream right behind orb_verify_pairs: the records are those of the list the verifier read
        other = [(t, q) for q, t in pairs][:7]
        big_want = pf.verify_pairs(counts, corners, rows, cap, pairs, W0, H0, model=pf.EPIPOLAR, seed=3, hypotheses=4096)
        for a, b in ((s1, s2), (s2, s1)):
            prog.match_pairs(pairs, stream=a.cuda_stream)
            prog.verify_pairs(len(pairs), model=pf.EPIPOLAR, seed=3, hypotheses=4096, stream=b.cuda_stream)
            prog.match_pairs(other, stream=a.cuda_stream)
            big = _check_verify(prog, counts, corners, rows, cap, pairs, W0, H0, pf.EPIPOLAR, want=big_want, call=False)
            assert [int(r["candidates"]) for r in big] == [int(r["candidates"]) for r in epi]
            _check_rows(prog, counts, descs, cap, other, call=False)
            assert _code(tinyorb, prog.verify_pairs, len(other) + 1)[0] == E  # the matched extent is the second list's now
        # the consecutive stages keep their results through pairs calls, and the pairs stages theirs through consecutive calls
        prog.match_consecutive(n)
        prog.verify_consecutive(n, hypotheses=64)
        prog.verify_epipolar(n, hypotheses=64)

        def consecutive():
            return [(prog.match_read(f, cap).tobytes(), [a.tobytes() for a in prog.verify_read(f, cap)],
                     [a.tobytes() for a in prog.verify_epipolar_read(f, cap)]) for f in range(n - 1)]

        before = consecutive()
        prows = _check_rows(prog, counts, descs, cap, pairs)
        _check_verify(prog, counts, corners, prows, cap, pairs, W0, H0, pf.HOMOGRAPHY, hypotheses=64, seed=5)
        assert consecutive() == before
        prog.match_consecutive(n)
        prog.verify_consecutive(n, hypotheses=64)
        prog.verify_epipolar(n, hypotheses=64)
        assert consecutive() == before
        _check_rows(prog, counts, descs, cap, pairs, want=prows, call=False)
        _check_verify(prog, counts, corners, prows, cap, pairs, W0, H0, pf.HOMOGRAPHY, call=False, hypotheses=64, seed=5)
        prog.verify_pairs(3)  # the pairs matcher is still fresh: neither consecutive call made it stale
        # orb_batch_select_output and a new batch make it stale
        prog.batch_select_output(1)
        assert _code(tinyorb, prog.verify_pairs, 3)[0] == S
        prog.batch_select_output(0)
        prog.verify_pairs(3)
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert _code(tinyorb, prog.verify_pairs, 3)[0] == S
        C.inject(prog, counts, corners, descs)
        _check_rows(prog, counts, descs, cap, pairs[:4])
        _check_verify(prog, counts, corners, rows, cap, pairs[:4], W0, H0, pf.HOMOGRAPHY)


# ---- the scene -----------------------------------------------------------------------------------------------------------------
def test_the_scene_closes_places_candidates(tinyorb, oracle):
    """place_scene.REDUCED extracted on the device in the intended mode: orb_place_frames proposes, the list is every revisit's two
    best candidates and the revisit against each filler; every byte against the restatement on the device's records, and the three
    relations tests/test_pairs_ref.py shows for the oracle's records."""
    S = place_scene.REDUCED
    frames, twin = place_scene.frames(oracle, **S)
    n, cap = len(frames), S["cap"]
    fillers = list(range(S["places"], S["places"] + S["fillers"]))
    flags = tinyorb.ORB_FLAG_INTENDED | tinyorb.ORB_FLAG_NMS
    with _program(tinyorb, cap, n, S["W"], S["H"], flags, blank=False) as prog:
        prog.extract_batch_host(frames)
        counts = prog.batch_counts(n)
        rec = [prog.batch_read(f, min(int(counts[f]), cap)) for f in range(n)]
        corners, descs = [r[0] for r in rec], [r[1] for r in rec]
        prog.place_frames(n, min_gap=S["min_gap"])
        prow = prog.place_read(0, n)
        assert prow.tobytes() == pr.place(counts, descs, cap, min_gap=S["min_gap"])[1].tobytes()
        pairs, kind = [], []
        for f, g in twin.items():
            assert prow[f]["n"] >= 2 and prow[f]["best"][0]["frame"] == g
            pairs += [(f, g), (f, int(prow[f]["best"][1]["frame"]))] + [(f, x) for x in fillers]
            kind += ["twin", "second"] + ["filler"] * len(fillers)
        rows = _check_rows(prog, counts, descs, cap, pairs)
        for model in (pf.HOMOGRAPHY, pf.EPIPOLAR):
            recs = _check_verify(prog, counts, corners, rows, cap, pairs, S["W"], S["H"], model)
            for (q, t), k, r in zip(pairs, kind, recs):
                print("model %d  %2d -> %2d  %-6s candidates %3d inliers %3d status %d" % (model, q, t, k, r["candidates"], r["inliers"], r["status"]))
            check_scene_relations(pairs, kind, recs)
