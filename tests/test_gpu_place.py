"""orb_place_frames on the GPU: every byte of every signature and of every OrbPlaceRow against the CPU
restatement (tests/place_ref.py) fed with the records the device holds.  No tolerance anywhere.

The programs are 64 x 48 (160 x 120 for the extracted scene) with zero images; the counters and descriptors are then written
over the batch (constructed.inject).  Descriptors are drawn from a small pool, so that frames share keys and the rows hold
candidates, many of them with equal scores.

Tile sizes: k_place_score works on tiles of 32 query frames x 32 ids (kPlaceTile; ids are the database entries, then the batch's
frames), in chunks of 64 words of a signature; k_place_sign walks a frame's records 256 at a time and k_place_select the ids 64
at a time.  So the frame counts 31, 32, 33 (and 1, 2, 17, 65) with 0 and 5 database entries put both sides of a tile below, at and
above 32 and 64; the record counts 63, 64, 65 and the capacity lie around a wave; and signatures of 8 words (bits 8, one table)
to 16384 (bits 16, 8 tables) lie below, at and above a chunk."""
import numpy as np
import pytest

import constructed as C
import place_ref as pr
import place_scene

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48
NONE = 0xFFFFFFFF


def _program(tinyorb, cap, max_batch, W=W0, H=H0, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0,
                            max_batch=max_batch, flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


def _hold(prog, n, counts, desc):
    """A batch of n empty frames, then the counters and descriptors over it."""
    prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
    C.inject(prog, counts, None, desc)


def _pool_frames(rng, n, cap, pool=300, lo=20):
    """n frames of lo .. cap descriptors drawn from one pool of `pool`."""
    P = C.random_desc(rng, pool)
    counts = rng.integers(lo, cap + 1, n).astype(np.uint32)
    return counts, [P[rng.choice(pool, int(c), replace=False)] for c in counts]


def _keyed(keys):
    """Descriptors whose 16 halves all hold the record's key: with bits 16 a shared key is one shared bit in every table."""
    k = np.asarray(keys, np.uint32)
    return np.repeat((k | (k << np.uint32(16)))[:, None], 8, 1)


def _check(prog, counts, desc, cap, n=None, db=None, keyframes=None, stream=None, **params):
    """One place call and every byte it leaves against the restatement.  Returns the rows."""
    n = len(counts) if n is None else n
    prog.place_frames(n, db=db, stream=stream, **params)
    sigs, want = pr.place(counts, desc, cap, n_frames=n, db=db, keyframes=keyframes, **params)
    got = prog.place_read(0, n)
    if got.tobytes() != want.tobytes():
        bad = [f for f in range(n) if got[f].tobytes() != want[f].tobytes()]
        raise AssertionError((params, n, bad[:4], got[bad[:4]], want[bad[:4]]))
    for f in range(n):
        s = prog.place_signature(f)
        assert s.shape == sigs[f].shape and s.tobytes() == sigs[f].tobytes(), (params, f, np.nonzero(s != sigs[f])[0][:8])
    return got


def _signature_batch(rng, cap):
    """Counts 0, 1, 63, 64, 65, the capacity, a raw counter above it, and a frame with stale descriptors behind its count; frame
    5 holds every descriptor of its first half twice."""
    P = C.random_desc(rng, 200)
    counts = np.array([0, 1, 63, 64, 65, cap, cap + 77, 100], np.uint32)
    desc = [P[rng.choice(200, min(int(c), cap), replace=False)] for c in counts]
    desc[5] = np.concatenate([desc[5][:cap // 2], desc[5][:cap - cap // 2]])
    desc[7] = np.concatenate([desc[7], C.random_desc(rng, cap - 100)])  # stale: stored 100, the rest never read
    return counts, desc


@pytest.mark.parametrize("bits,tables", [(8, 1), (8, 8), (8, 16), (13, 1), (13, 8), (13, 16), (16, 1), (16, 8)])
def test_signatures(tinyorb, bits, tables):
    cap = 128
    counts, desc = _signature_batch(np.random.default_rng(bits * 100 + tables), cap)
    with _program(tinyorb, cap, 8) as prog:
        _hold(prog, 8, counts, desc)
        rows = _check(prog, counts, desc, cap, bits=bits, tables=tables, min_gap=1, top=8)
        assert rows["keypoints"].tolist() == [0, 1, 63, 64, 65, cap, cap, 100]
        assert rows["bits_set"][0] == 0 and rows["bits_set"][1] == tables and rows["bits_set"][5] <= tables * (cap // 2)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.place_frames(8, bits=16, tables=16)
        assert e.value.code == tinyorb.ORB_EINVAL


def test_a_second_call_with_other_bits_leaves_nothing_behind(tinyorb):
    cap = 128
    counts, desc = _signature_batch(np.random.default_rng(7), cap)
    with _program(tinyorb, cap, 8) as prog:
        _hold(prog, 8, counts, desc)
        # (9, 5) and (10, 9): 80 and 288 words, a last slice of k_place_score that ends inside a chunk of 64
        for bits, tables in ((16, 8), (8, 8), (13, 16), (8, 1), (9, 5), (16, 1), (10, 9), (9, 3)):
            _check(prog, counts, desc, cap, bits=bits, tables=tables, min_gap=2)
        # other records under the same parameters: every word is written again
        counts2, desc2 = _signature_batch(np.random.default_rng(8), cap)
        C.inject(prog, counts2, None, desc2)
        _check(prog, counts2, desc2, cap, bits=9, tables=3, min_gap=2)


@pytest.mark.parametrize("n_frames", [1, 2, 17, 31, 32, 33, 65])
def test_rows(tinyorb, n_frames):
    cap = 128
    rng = np.random.default_rng(n_frames)
    counts, desc = _pool_frames(rng, 65, cap)
    counts[3] = 0  # a frame without keypoints, as a query and as a candidate
    desc[3] = desc[3][:0]
    with _program(tinyorb, cap, 70) as prog:
        _hold(prog, 65, counts, desc)
        db5 = pr.place(counts[60:65], desc[60:65], cap, bits=10, tables=4)[0]
        for top in (1, 4, 8):
            rows = _check(prog, counts, desc, cap, n=n_frames, bits=10, tables=4, min_gap=1, top=top)
            _check(prog, counts, desc, cap, n=n_frames, db=db5, bits=10, tables=4, min_gap=2, top=top)
        if n_frames >= 17:
            assert (rows["candidates"][3], rows["bits_set"][3], rows["eligible"][3]) == (0, 0, 3) and rows["n"].max() == 8
            ties = sum(int(np.sum(r["best"]["score"][1:int(r["n"])] == r["best"]["score"][:max(int(r["n"]) - 1, 0)])) for r in rows)
            assert ties > 0  # equal scores in the rows, ordered by id
        _check(prog, counts, desc, cap, n=n_frames, min_gap=1)          # the default signature: 16 bits, 8 tables
        _check(prog, counts, desc, cap, n=n_frames, min_gap=n_frames)   # nothing eligible
        for min_gap, kw in ((7, {}), (31, {}), (32, {}), (33, {}), (3, dict(min_score=40)), (3, dict(min_permille=120)),
                            (3, dict(min_score=1 << 31, min_permille=1000))):
            _check(prog, counts, desc, cap, n=n_frames, bits=10, tables=4, min_gap=min_gap, **kw)


def test_planted_ties_gaps_and_boundaries(tinyorb):
    """The restatement's hand-built cases on the device, with the answers the constructions imply."""
    cap, T = 8, 8
    q = list(range(100, 108))
    frames = [[100, 101, 9, 10], [102, 103, 11, 12], [100, 13, 14, 15], [], [100, 101, 102] + list(range(300, 305)), q, q]
    desc = [_keyed(k) for k in frames]
    counts = np.array([len(k) for k in frames], np.uint32)
    with _program(tinyorb, cap, 8) as prog:
        _hold(prog, 7, counts, desc)
        rows = _check(prog, counts, desc, cap, min_gap=1, top=8)
        assert rows["bits_set"].tolist() == [4 * T, 4 * T, 4 * T, 0, 8 * T, 8 * T, 8 * T]
        assert [tuple(b) for b in rows[5]["best"]] == [(4, 3 * T), (0, 2 * T), (1, 2 * T), (2, T)] + [(NONE, 0)] * 4
        assert (rows[5]["eligible"], rows[5]["candidates"], rows[5]["n"]) == (5, 4, 4)  # the empty frame is eligible, and no candidate
        assert (rows[3]["eligible"], rows[3]["candidates"], rows[3]["n"]) == (3, 0, 0)
        assert tuple(rows[6]["best"][0]) == (5, 8 * T)
        rows = _check(prog, counts, desc, cap, min_gap=1, top=2)
        assert [tuple(b) for b in rows[5]["best"][:3]] == [(4, 3 * T), (0, 2 * T), (NONE, 0)] and rows[5]["candidates"] == 4
        # g + min_gap == f is eligible, one less is not
        rows = _check(prog, counts, desc, cap, min_gap=4)
        assert rows["eligible"].tolist() == [0, 0, 0, 0, 1, 2, 3] and [tuple(b) for b in rows[5]["best"][:3]] == [(0, 2 * T), (1, 2 * T), (NONE, 0)]
        # 1000 * 16 == 250 * 64: a candidate at the exact boundary, none one past it; min_score likewise
        assert _check(prog, counts, desc, cap, min_gap=1, min_permille=250)[5]["candidates"] == 3
        assert _check(prog, counts, desc, cap, min_gap=1, min_permille=251)[5]["candidates"] == 1
        assert _check(prog, counts, desc, cap, min_gap=1, min_score=2 * T)[5]["candidates"] == 3
        assert _check(prog, counts, desc, cap, min_gap=1, min_score=2 * T + 1)[5]["candidates"] == 1
        # a database entry beats a batch frame on a tie
        db = pr.place(counts, desc, cap)[0][[1, 0]]
        rows = _check(prog, counts, desc, cap, db=db, min_gap=1, top=8)
        D = tinyorb.ORB_PLACE_DB
        assert [tuple(b) for b in rows[5]["best"][:6]] == [(4, 3 * T), (D | 0, 2 * T), (D | 1, 2 * T), (0, 2 * T), (1, 2 * T), (2, T)]


@pytest.mark.parametrize("n_db", [1, 5, 1024])
def test_database(tinyorb, n_db):
    """Signatures of 32 bytes (bits 8, one table), so that ORB_PLACE_DB_MAX of them stay small."""
    cap = 64
    rng = np.random.default_rng(n_db)
    counts, desc = _pool_frames(rng, 9, cap, pool=80, lo=5)
    db = (rng.integers(0, 256, (n_db, 32)) & rng.integers(0, 256, (n_db, 32))).astype(np.uint8)
    with _program(tinyorb, cap, 9) as prog:
        _hold(prog, 9, counts, desc)
        rows = _check(prog, counts, desc, cap, db=db, bits=8, tables=1, min_gap=2, top=8)
        assert rows["eligible"].tolist() == [n_db + max(f - 1, 0) for f in range(9)]
        marked = rows["best"]["frame"][(rows["best"]["frame"] != NONE) & (rows["best"]["frame"] >= tinyorb.ORB_PLACE_DB)]
        assert len(marked) and (marked & 0x7FFFFFFF).max() < n_db
        # the caller's rows are the caller's again when the call returns
        mine = db.copy()
        prog.place_frames(9, db=mine, bits=8, tables=1, min_gap=2, top=8)
        mine[:] = 0xFF
        assert prog.place_read(0, 9).tobytes() == rows.tobytes()


def test_round_trip_through_the_database(tinyorb):
    cap = 128
    counts, desc = _pool_frames(np.random.default_rng(3), 12, cap)
    with _program(tinyorb, cap, 12) as prog:
        _hold(prog, 12, counts, desc)
        _check(prog, counts, desc, cap, bits=12, tables=6)
        kept = np.stack([prog.place_signature(f) for f in range(12)])
        assert kept.shape == (12, 6 * 4096 // 8)
        _hold(prog, 12, counts, desc)  # the next batch shows the same places
        rows = _check(prog, counts, desc, cap, db=kept, bits=12, tables=6, top=1)
        for f in range(12):
            assert tuple(rows[f]["best"][0]) == (tinyorb.ORB_PLACE_DB | f, rows[f]["bits_set"])


def test_keyframes_and_the_track_stage(tinyorb):
    import torch
    cap, F = 40, 12
    ch = C.chains(np.random.default_rng(5), C.steady_loss(F, cap), W0, H0)
    counts, desc = ch["counts"], list(ch["desc"])
    K = tinyorb.ORB_PLACE_KEYFRAMES
    with _program(tinyorb, cap, F) as prog:
        prog.extract_batch_host(np.zeros((F, H0, W0, 4), np.uint8))
        C.inject(prog, counts, ch["corners"], desc)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.place_frames(F, flags=K)  # no track call yet
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.match_consecutive(F)
        prog.track_consecutive(F, source=tinyorb.ORB_TRACK_MATCHED, keep_permille=950)
        key = prog.track_frames(F)["keyframe"]
        assert 2 < key.sum() < F
        rows = _check(prog, counts, desc, cap, keyframes=key, flags=K, bits=12, tables=4, min_gap=1, top=8)
        plain = _check(prog, counts, desc, cap, bits=12, tables=4, min_gap=1, top=8)
        assert rows["eligible"].tolist() == [int(key[:f].sum()) for f in range(F)] and plain["eligible"].tolist() == list(range(F))
        assert all(key[b["frame"]] for r in rows for b in r["best"][:r["n"]])
        # fewer frames tracked than placed
        prog.track_consecutive(5, source=tinyorb.ORB_TRACK_MATCHED)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.place_frames(6, flags=K)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.place_frames(5, flags=K)
        # the ordering rule: a track call on another stream right behind the place call waits before it overwrites the keyframes
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        for a, b in ((s1, s2), (s2, s1)):
            prog.track_consecutive(F, source=tinyorb.ORB_TRACK_MATCHED, keep_permille=950, stream=a.cuda_stream)
            prog.place_frames(F, flags=K, bits=12, tables=4, min_gap=1, top=8, stream=b.cuda_stream)
            prog.track_consecutive(F, source=tinyorb.ORB_TRACK_MATCHED, keep_permille=1000, min_gap=1, max_gap=1, stream=a.cuda_stream)
            assert prog.place_read(0, F).tobytes() == rows.tobytes()
            assert prog.track_frames(F)["keyframe"].all()  # every frame a keyframe now
            _check(prog, counts, desc, cap, keyframes=np.ones(F), flags=K, bits=12, tables=4, min_gap=1, top=8, stream=b.cuda_stream)
        # a new batch makes the track stage stale
        prog.extract_batch_host(np.zeros((F, H0, W0, 4), np.uint8))
        with pytest.raises(tinyorb.OrbError) as e:
            prog.place_frames(F, flags=K)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.place_frames(F)


def test_extracted_frames(tinyorb, oracle):
    """The recognition scene cut down to 6 places, 2 fillers and 6 revisits at 160 x 120, extracted on the device in the intended
    mode: the rows equal the restatement's on the device's own records, and every revisit's first candidate is its twin -- as the
    restatement on the oracle's records shows for this scene (checked here as well, on the CPU)."""
    S = place_scene.REDUCED
    frames, twin = place_scene.frames(oracle, **S)
    n, cap = len(frames), S["cap"]
    totals, _, odesc = oracle.extract_intended_batch(frames, depth=2, max_features=cap, arc=9, nms=True)
    _, orows = pr.place(totals, odesc, cap, min_gap=S["min_gap"])
    assert all(orows[f]["best"][0]["frame"] == g for f, g in twin.items())
    flags = tinyorb.ORB_FLAG_INTENDED | tinyorb.ORB_FLAG_NMS
    with _program(tinyorb, cap, n, S["W"], S["H"], flags) as prog:
        prog.extract_batch_host(frames)
        counts = prog.batch_counts(n)
        desc = [prog.batch_read(f, min(int(counts[f]), cap))[1] for f in range(n)]
        assert counts.min() > 40
        rows = _check(prog, counts, desc, cap, min_gap=S["min_gap"])
        for f, g in twin.items():
            assert rows[f]["best"][0]["frame"] == g, (f, g, rows[f])
        _check(prog, counts, desc, cap, min_gap=S["min_gap"], bits=11, tables=16, min_permille=20)


def test_arguments_and_state(tinyorb):
    import torch
    cap = 32
    counts, desc = _pool_frames(np.random.default_rng(1), 5, cap, pool=60, lo=10)
    L = tinyorb.load_library()

    def code(fn, *a, **kw):
        with pytest.raises(tinyorb.OrbError) as e:
            fn(*a, **kw)
        return e.value.code

    with _program(tinyorb, cap, 6, flags=tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        assert code(prog.place_frames, 1) == tinyorb.ORB_ESTATE  # no batch
        assert code(prog.place_read, 0, 1) == tinyorb.ORB_ESTATE
        assert code(prog.place_signature, 0) == tinyorb.ORB_ESTATE
        _hold(prog, 5, counts, desc)
        assert code(prog.place_read, 0, 1) == tinyorb.ORB_ESTATE  # a batch, no call yet
        for kw in (dict(n_frames=0), dict(n_frames=6), dict(n_frames=5, bits=7), dict(n_frames=5, bits=17), dict(n_frames=5, tables=17),
                   dict(n_frames=5, bits=16, tables=9), dict(n_frames=5, bits=16, tables=16), dict(n_frames=5, top=9),
                   dict(n_frames=5, min_permille=1001), dict(n_frames=5, flags=2), dict(n_frames=5, flags=3), dict(n_frames=5, reserved=1),
                   dict(n_frames=5, db=np.zeros((tinyorb.ORB_PLACE_DB_MAX + 1, 32), np.uint8), bits=8, tables=1)):
            assert code(prog.place_frames, **kw) == tinyorb.ORB_EINVAL, kw
        h = prog._handle()
        prm = tinyorb.OrbPlaceParams(bits=8, tables=1)
        one = np.zeros(32, np.uint8)
        import ctypes
        assert L.orb_place_frames(h, 5, ctypes.byref(prm), one.ctypes.data, 0, None) == tinyorb.ORB_EINVAL  # rows and n_db 0
        assert L.orb_place_frames(h, 5, ctypes.byref(prm), None, 1, None) == tinyorb.ORB_EINVAL             # n_db and no rows
        assert code(prog.place_read, 0, 1) == tinyorb.ORB_ESTATE  # none of those calls counted
        assert L.orb_place_frames(h, 5, None, None, 0, None) == tinyorb.ORB_OK  # params NULL: the defaults
        prog._place = (5, pr.sig_bytes())
        want = pr.place(counts, desc, cap)
        assert prog.place_read(0, 5).tobytes() == want[1].tobytes() and prog.place_signature(4).tobytes() == want[0][4].tobytes()
        # the reads: clipped to the frames placed, a frame at or past them refused, NULL only with nothing asked for
        _check(prog, counts, desc, cap, n=4, bits=9, tables=2, min_gap=1)
        rows = np.zeros(8, tinyorb.PLACE_ROW_DTYPE)
        rows["n"] = 77
        assert L.orb_place_read(h, 2, rows.ctypes.data, 8) == tinyorb.ORB_OK
        assert (rows["n"][2:] == 77).all() and rows[:2].tobytes() == prog.place_read(2, 2).tobytes()
        assert L.orb_place_read(h, 4, rows.ctypes.data, 1) == tinyorb.ORB_EINVAL
        assert L.orb_place_read(h, 3, None, 0) == tinyorb.ORB_OK and L.orb_place_read(h, 3, None, 1) == tinyorb.ORB_EINVAL
        sig = np.full(2 * 64 + 40, 0xA5, np.uint8)
        assert L.orb_place_signature(h, 3, sig.ctypes.data, len(sig)) == tinyorb.ORB_OK
        assert (sig[128:] == 0xA5).all() and sig[:128].tobytes() == prog.place_signature(3).tobytes()  # sig_bytes copied, no more
        part = np.full(64, 0xA5, np.uint8)
        assert L.orb_place_signature(h, 3, part.ctypes.data, 10) == tinyorb.ORB_OK and part[:10].tobytes() == sig[:10].tobytes() and (part[10:] == 0xA5).all()
        assert L.orb_place_signature(h, 4, sig.ctypes.data, 1) == tinyorb.ORB_EINVAL
        assert L.orb_place_signature(h, 0, None, 0) == tinyorb.ORB_OK and L.orb_place_signature(h, 0, None, 1) == tinyorb.ORB_EINVAL
        # a call on a caller's stream followed by a read
        s = torch.cuda.Stream(device=0)
        _check(prog, counts, desc, cap, bits=14, tables=5, min_gap=1, stream=s.cuda_stream)
        # the other output set holds other records: the call reads the current one
        prog.batch_select_output(1)
        c2, d2 = _pool_frames(np.random.default_rng(2), 5, cap, pool=60, lo=10)
        C.inject(prog, c2, None, d2)
        _check(prog, c2, d2, cap, bits=14, tables=5, min_gap=1)
        prog.batch_select_output(0)
        _check(prog, counts, desc, cap, bits=14, tables=5, min_gap=1)
