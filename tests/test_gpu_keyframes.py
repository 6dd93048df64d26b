"""The keyframe store on the GPU (orb_keyframes_*, orb_match_keyframes, orb_localize_keyframes): every byte
of a slot, of a row, of an OrbKeyframeFix and of the inlier bytes against the CPU restatement (tests/keyframes_ref.py) fed with
what the device holds -- its counts, records, orb_match_read, orb_trajectory_read, orb_landmarks_read, orb_keyframes_read and
orb_match_keyframes_read output.  No tolerance anywhere.

The programs are 64 x 48.  A batch (tests/loop_cases.py) is written over the stages' buffers with descriptors; the trajectory and
landmarks calls run on the device behind the injection, as in tests/test_gpu_loop.py.

Shapes.  The matchers take 256 (fp4) or 64 x kMatchQ (vector unit) queries per workgroup, candidates in tiles of 16 and chunks of
64: query counts 0, 1, 15 .. 17, 63 .. 65, 255 .. 257, 300 against stored counts 0, 1, 15 .. 17, 63 .. 65, 127 .. 129, 300.
k_loc_score takes the candidates in tiles of 256, k_kf_gather compacts 256 query slots per pass: 0, 5, 6, 7, 255, 256, 257 and 300
candidates at capacity 300 under raw counters above it; 1, 64, 65 and 512 hypotheses; k_lc_index and k_kf_insert run 256 slots per
block: capacity 257 with every slot a landmark."""
import collections

import numpy as np
import pytest

import constructed as C
import keyframes_ref as kfr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import loop_ref as lpr
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)
Inputs = collections.namedtuple("Inputs", "nq corners descs matches frames lms L cap")


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _load(prog, b, desc, traj=None, L_frames=None):
    """A views batch over the program's buffers with its descriptors, then the trajectory and landmarks calls on the device."""
    lc.inject(prog, b)
    C.inject(prog, b["counts"], None, desc)
    prog.trajectory_consecutive(b["n"], **(traj or {}))
    Lf = b["n"] if L_frames is None else L_frames
    prog.landmarks_consecutive(Lf, **INTR)
    return _inputs(prog, b["n"], Lf, b["cap"])


def _load_rail(prog, b, desc):
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], b["corners"], desc)
    tc.inject_pose(prog, matches=b["matches"], points_=b["points"])
    prog.trajectory_consecutive(n)
    L.inject_frames(prog, b["frames"])
    prog.landmarks_consecutive(n, **L.RAIL)
    return _inputs(prog, n, n, b["cap"])


def _batch(prog, n_frames, cap):
    """(stored counts, corners, descriptors) of the batch as the device holds them."""
    nq = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    recs = [prog.batch_read(f, int(nq[f])) for f in range(n_frames)]
    return nq, [r[0] for r in recs], [kfr.desc_words(r[1]) for r in recs]


def _inputs(prog, n_frames, L_frames, cap):
    """What an insert reads, as the device holds it."""
    nq, corners, descs = _batch(prog, n_frames, cap)
    matches = [prog.match_read(f, int(nq[f])) for f in range(L_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames)])
    lms = [prog.landmarks_read(p, cap)[1] for p in range(L_frames - 1)]
    return Inputs(nq, corners, descs, matches, frames, lms, L_frames, cap)


def _slot_bytes(prog, slot, cap):
    """Every byte of a slot: the header and all `cap` records of the three arrays."""
    return b"".join(np.ascontiguousarray(a).tobytes() for a in prog.keyframes_read(slot, cap))


def _padded(kf, cap):
    out = kf["head"].tobytes()
    for a in (kf["corners"], np.ascontiguousarray(kf["desc"], np.uint32), kf["points"]):
        out += a.tobytes() + bytes((cap - len(a)) * a[:1].itemsize * (8 if a.ndim == 2 else 1)) if len(a) else bytes(cap * a.dtype.itemsize * (8 if a.ndim == 2 else 1))
    return out


def _insert(prog, inp, entries, model, stream=None):
    """orb_keyframes_insert, then every byte of the named slots against KF-2 on what the device holds.  `model` (slot -> Keyframe) is
    updated."""
    prog.keyframes_insert(entries, stream=stream)
    kfr.insert(model, entries, inp.nq, inp.corners, inp.descs, inp.matches, inp.frames, inp.lms, inp.cap, L=inp.L)
    for e in entries:
        got, want = _slot_bytes(prog, e[1], inp.cap), _padded(model[e[1]], inp.cap)
        assert got == want, (e, prog.keyframes_read(e[1])[0], model[e[1]]["head"])


def _device_store(prog, slots):
    """The listed slots as orb_keyframes_read gives them."""
    out = {}
    for s in slots:
        head, corners, desc, points = prog.keyframes_read(s)
        out[s] = dict(head=head, corners=corners, desc=kfr.desc_words(desc), points=points)
    return out


def _check(prog, nq, corners, descs, pairs, n=None, stream=None, match=True, call=True, intr=INTR, **params):
    """match_keyframes (match=False: the last one's rows), localize_keyframes (call=False: the last one's results), then every row,
    record and inlier byte against the restatement on the device's store.  Returns (records, inlier bytes, rows, all the bytes)."""
    cap = prog.config.max_features
    if match:
        prog.match_keyframes(pairs, stream=stream)
    store = _device_store(prog, sorted(set(s for q, s in pairs)))
    n = len(pairs) if n is None else n
    rows = [prog.match_keyframes_read(i, int(nq[q])) for i, (q, s) in enumerate(pairs)]
    want_rows = kfr.match_keyframes(nq, descs, store, pairs, cap)
    for i in range(len(pairs)):
        assert rows[i].tobytes() == want_rows[i].tobytes(), (i, pairs[i], np.nonzero(rows[i] != want_rows[i])[0][:8])
    if call:
        prog.localize_keyframes(n, stream=stream, **intr, **params)
    want, wmask = kfr.localize_keyframes(nq, corners, rows, pairs, store, cap, n=n, **intr, **params)
    recs, masks, blob = [], [], b"".join(r.tobytes() for r in rows)
    for i in range(n):
        rec, mask = prog.localize_keyframes_read(i, cap)
        assert rec.tobytes() == want[i].tobytes(), (i, pairs[i], params, rec, want[i])
        assert mask.tobytes() == wmask[i].tobytes(), (i, pairs[i], params, np.nonzero(mask != wmask[i])[0][:8])
        assert not mask[nq[pairs[i][0]]:].any() and int(mask.sum()) == int(rec["inliers"])
        recs.append(rec)
        masks.append(mask)
        blob += rec.tobytes() + mask.tobytes()
    return np.array(recs), np.array(masks), rows, blob


def _loop_words(rec):
    """An OrbLoopFix or OrbKeyframeFix without the word that differs (query_origin / slot)."""
    w = np.frombuffer(rec.tobytes(), np.uint32).copy()
    w[26] = 0
    return w.tobytes()


SLOTS = [(3 * f + 5) % 11 for f in range(11)]  # a permutation: the slot is not the frame
LIST = K.LOOP_PAIRS + [(5, 10)]                # ... and an entry whose target is frame L: NOMAP on both sides


def _first_batch(T, prog):
    """out_and_back(0) at capacity 128 with the landmarks of ten frames; every frame inserted; the loop stage's rows, fixes and
    inlier bytes of LIST.  Returns (inputs, loop rows, loop fixes, loop masks)."""
    b = K.out_and_back(0)
    desc = K.plant(b, np.random.default_rng(100))
    inp = _load(prog, b, desc, traj=L.FULL_TRAJ, L_frames=b["n"] - 1)
    prog.keyframes_reserve(len(SLOTS))
    _insert(prog, inp, [(f, SLOTS[f], 7 * f, 1000 + f) for f in range(b["n"])], {})
    prog.match_pairs(LIST)
    prog.loop_pairs(len(LIST), **INTR)
    rows = [prog.match_pairs_read(i, int(inp.nq[q])) for i, (q, t) in enumerate(LIST)]
    fixes = [prog.loop_pairs_read(i, inp.cap) for i in range(len(LIST))]
    return inp, rows, [f[0] for f in fixes], [f[1] for f in fixes]


@pytest.mark.parametrize("valu", ["", "1"])
def test_identity_with_the_loop_stage(tinyorb, monkeypatch, valu):
    """A frame T inserted into slot s: the entry (q, s) gives the bytes the loop stage gives (q, T), on both matcher forms."""
    T = tinyorb
    monkeypatch.setenv("TINYORB_MATCH_VALU", valu) if valu else monkeypatch.delenv("TINYORB_MATCH_VALU", raising=False)
    with _program(T, 128, 11) as prog:
        inp, rows, fixes, lmasks = _first_batch(T, prog)
        assert [int(f["status"]) for f in fixes] == [T.ORB_LOCALIZE_NOMAP if t == 10 else T.ORB_LOCALIZE_OK for q, t in LIST]  # (0, 10) and (5, 10)
        pairs = [(q, SLOTS[t]) for q, t in LIST]
        recs, masks, krows, _ = _check(prog, inp.nq, inp.corners, inp.descs, pairs)
        for i, (q, t) in enumerate(LIST):
            assert krows[i].tobytes() == rows[i].tobytes(), (i, q, t)
            assert _loop_words(recs[i]) == _loop_words(fixes[i]) and masks[i].tobytes() == lmasks[i].tobytes(), (i, q, t, recs[i], fixes[i])
            assert recs[i]["slot"] == (SLOTS[t] if t < 10 else 0)
        head = prog.keyframes_read(SLOTS[10])[0]
        assert head["status"] == T.ORB_KEYFRAME_NOMAP and head["origin"] == T.ORB_KEYFRAME_NONE and head["keypoints"] == inp.nq[10] and head["points"] == 0
        head = prog.keyframes_read(SLOTS[3])[0]
        assert head["status"] == T.ORB_KEYFRAME_STORED and head["frame"] == 3 and head["user"].tolist() == [21, 1003] and head["points"] > 40


def test_across_batches_in_one_program(tinyorb):
    """The store outlives the batch: a second batch over the program -- the first one's frames 10 .. 6, by their records only -- is
    matched and localised against the stored slots with the first batch's OrbLoopFix words."""
    T = tinyorb
    with _program(T, 128, 11) as prog:
        inp, rows, fixes, lmasks = _first_batch(T, prog)
        cap = inp.cap
        kept = [_slot_bytes(prog, s, cap) for s in range(len(SLOTS))]
        order = [10, 9, 8, 7, 6]
        prog.extract_batch_host(np.zeros((5, H0, W0, 4), np.uint8))
        C.inject(prog, [int(inp.nq[f]) for f in order], [inp.corners[f] for f in order], [inp.descs[f] for f in order])
        with pytest.raises(T.OrbError) as e:
            prog.keyframes_insert([(0, 0)])  # nothing of this batch has run
        assert e.value.code == T.ORB_ESTATE
        prog.match_consecutive(5)
        prog.verify_epipolar(5)
        prog.pose_consecutive(5, **INTR)
        prog.trajectory_consecutive(5)
        prog.landmarks_consecutive(5, **INTR)
        assert [_slot_bytes(prog, s, cap) for s in range(len(SLOTS))] == kept
        nq, corners, descs = _batch(prog, 5, cap)
        assert all(descs[i].tobytes() == inp.descs[f].tobytes() for i, f in enumerate(order))
        pairs = [(i, SLOTS[t]) for i, (q, t) in enumerate(K.LOOP_PAIRS[:5])]  # (10, 0), (9, 1), (8, 2), (7, 3), (6, 4) of the first batch
        assert [q for q, t in K.LOOP_PAIRS[:5]] == order
        recs, masks, krows, _ = _check(prog, nq, corners, descs, pairs)
        for i in range(5):
            assert krows[i].tobytes() == rows[i].tobytes()
            assert _loop_words(recs[i]) == _loop_words(fixes[i]) and masks[i].tobytes() == lmasks[i].tobytes(), (i, recs[i], fixes[i])
        assert (recs["status"] == T.ORB_LOCALIZE_OK).all() and recs["slot"].tolist() == [SLOTS[t] for q, t in K.LOOP_PAIRS[:5]]
        assert [_slot_bytes(prog, s, cap) for s in range(len(SLOTS))] == kept


def test_candidate_counts_hypotheses_and_seeds(tinyorb):
    """Capacity 300, raw counters 311, slots 0 and slots - 1 of a store of 3: 0 .. 300 candidates of one entry, then each hypothesis
    count under two seeds, and the first call again."""
    T = tinyorb
    cap = K.COUNT_CAP
    b = K.count_batch(cap)
    rng = np.random.default_rng(301)
    desc = K.plant(b, rng)
    with _program(T, cap, b["n"]) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ)
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all()
        prog.keyframes_reserve(3)
        _insert(prog, inp, [(0, 2), (3, 0)], {})
        pairs = [(3, 2), (0, 0), (3, 2)]
        own = lpr.owners(inp.nq, inp.matches, inp.frames, inp.lms, cap, inp.L)
        for M in K.COUNTS:
            d = K.set_candidates(desc, 3, 0, own[0], M, rng)
            C.inject(prog, b["counts"], None, desc[:3] + [d])
            nq, corners, descs = _batch(prog, b["n"], cap)
            recs, _, _, _ = _check(prog, nq, corners, descs, pairs)
            print(M, recs["status"].tolist(), recs["candidates"].tolist(), recs["inliers"].tolist())
            if M < 6:
                assert recs["status"][0] == T.ORB_LOCALIZE_FEW and recs["candidates"][0] == 0 and recs["status"][2] == T.ORB_LOCALIZE_FEW
            else:
                assert recs["status"][0] != T.ORB_LOCALIZE_FEW and recs["candidates"][0] in (M, 0) and recs["candidates"][2] in (M, 0)
        C.inject(prog, b["counts"], None, desc)
        nq, corners, descs = _batch(prog, b["n"], cap)
        first = None
        for hyps in (1, 64, 65, 512):
            for seed in (0, 0x9E3779B9):
                recs, _, _, blob = _check(prog, nq, corners, descs, pairs, match=first is None, hypotheses=hyps, seed=seed)
                first = blob if first is None else first
                assert recs["hypothesis"].max() < hyps
        _check(prog, nq, corners, descs, [(1, 0)])  # a list of one entry in between
        assert _check(prog, nq, corners, descs, pairs, hypotheses=1, seed=0)[3] == first  # stale rows, keys or bytes of the calls between would show


QUERY_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
STORED_COUNTS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300)


def _hand_built(rng, n, cap, status, keys=None):
    """A keyframe of n random records; keys: MAP_POINT keys (default: none has a landmark)."""
    from tinyslam_amd import orb
    head = np.zeros((), orb.KEYFRAME_DTYPE)
    pts = np.zeros(n, orb.MAP_POINT_DTYPE)
    pts["key"] = kfr.NONE if keys is None else keys
    if status == orb.ORB_KEYFRAME_STORED:
        head["r"], head["scale"], head["origin"] = np.eye(3, dtype=np.float32).ravel(), 1.0, 0
    else:
        head["origin"] = kfr.NONE
    head["keypoints"], head["points"], head["frame"], head["status"] = n, int((pts["key"] != kfr.NONE).sum()), 3, status
    return dict(head=head, corners=C.distinct_corners(rng, n, W0, H0) if n else np.zeros(0, orb.CORNER_DTYPE), desc=C.random_desc(rng, n), points=pts)


def _load_kf(prog, slot, kf):
    from tinyslam_amd import orb
    prog.keyframes_load(slot, kf["head"], kf["corners"], np.ascontiguousarray(kf["desc"], np.uint32).view(orb.DESCRIPTOR_DTYPE).reshape(-1), kf["points"])


@pytest.mark.parametrize("valu", ["", "1"])
def test_query_and_stored_counts_at_the_matchers_tiles(tinyorb, monkeypatch, valu):
    """Every query count against stored counts in one list of P entries with duplicates, at capacity 300 with raw counters above it."""
    T = tinyorb
    monkeypatch.setenv("TINYORB_MATCH_VALU", valu) if valu else monkeypatch.delenv("TINYORB_MATCH_VALU", raising=False)
    cap, n = 300, len(QUERY_COUNTS)
    rng = np.random.default_rng(77)
    with _program(T, cap, n) as prog:
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        counts = [c + (11 if c == cap else 0) for c in QUERY_COUNTS]
        C.inject(prog, counts, [C.distinct_corners(rng, c, W0, H0) for c in QUERY_COUNTS], [C.random_desc(rng, c) for c in QUERY_COUNTS])
        nq, corners, descs = _batch(prog, n, cap)
        assert nq.tolist() == list(QUERY_COUNTS) and prog.batch_counts(n)[-1] == cap + 11
        prog.keyframes_reserve(len(STORED_COUNTS))
        model = {}
        for s, c in enumerate(STORED_COUNTS):
            model[s] = _hand_built(rng, c, cap, T.ORB_KEYFRAME_NOMAP if s % 2 else T.ORB_KEYFRAME_STORED)
            _load_kf(prog, s, model[s])
            assert _slot_bytes(prog, s, cap) == _padded(model[s], cap)
        P = T.ORB_PAIRS_PER_FRAME * n
        pairs = [(q, (q + k) % n) for k in (0, 5, 9, 0) for q in range(n)]  # the last n entries repeat the first n
        assert len(pairs) == P == 48
        recs, _, rows, _ = _check(prog, nq, corners, descs, pairs, hypotheses=8)
        assert all((int(r["status"]) == T.ORB_LOCALIZE_NOMAP) == bool(s % 2) for r, (q, s) in zip(recs, pairs))
        assert all(int(r["status"]) in (T.ORB_LOCALIZE_NOMAP, T.ORB_LOCALIZE_FEW) for r in recs) and not recs["r"].any()
        i = pairs.index((n - 1, n - 1))  # 300 queries against 300 stored records: a best match for every one
        assert (rows[i]["index"] != T.ORB_MATCH_NONE).all() and (rows[pairs.index((7, 0))]["index"] == T.ORB_MATCH_NONE).all()
        with pytest.raises(T.OrbError) as e:
            prog.match_keyframes(pairs + [(0, 0)])
        assert e.value.code == T.ORB_EINVAL


def test_insert_at_capacity_257_with_every_slot_a_landmark(tinyorb):
    """k_lc_index's and k_kf_insert's one-thread second block."""
    T = tinyorb
    b = L.rail(6, 257, v_hi=L.V_HI)
    desc = K.plant(b, np.random.default_rng(22))
    with _program(T, 257, 6) as prog:
        inp = _load_rail(prog, b, desc)
        prog.keyframes_reserve(6)
        _insert(prog, inp, [(f, 5 - f) for f in range(6)], {})
        assert all(prog.keyframes_read(s)[0]["points"] == 257 for s in range(6))
        recs, masks, _, _ = _check(prog, inp.nq, inp.corners, inp.descs, [(5, 5), (0, 0), (3, 3)], intr=L.RAIL)
        assert recs["candidates"].tolist() == [257] * 3 and (recs["status"] == T.ORB_LOCALIZE_OK).all() and masks[:, 256].all()
        assert np.allclose(recs["t"][:, 0], [-2.5, 2.5, -0.5], atol=1e-3)


def test_store_life_save_and_load(tinyorb):
    T = tinyorb
    b = K.out_and_back(2, nf=2, n_land=150)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    rng = np.random.default_rng(32)
    pairs = [(4, 0), (3, 1), (0, 2)]

    def code(fn, *a, **kw):
        with pytest.raises(T.OrbError) as e:
            fn(*a, **kw)
        return e.value.code

    with _program(T, cap, n) as prog, _program(T, cap, n) as other:
        assert code(prog.keyframes_read, 0) == T.ORB_ESTATE and code(prog.keyframes_insert, [(0, 0)]) == T.ORB_ESTATE  # before reserve
        assert code(prog.keyframes_reserve, 0) == T.ORB_EINVAL and code(prog.keyframes_reserve, T.ORB_KEYFRAME_SLOTS_MAX + 1) == T.ORB_EINVAL
        prog.keyframes_reserve(4)
        prog.keyframes_reserve(4)
        assert code(prog.keyframes_reserve, 5) == T.ORB_ESTATE
        assert not _slot_bytes(prog, 3, cap).strip(b"\0")  # an empty slot is all zero
        assert code(prog.keyframes_insert, [(0, 0)]) == T.ORB_ESTATE and code(prog.match_keyframes, [(0, 0)]) == T.ORB_ESTATE  # before a batch
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ)
        for bad in ([], [(n, 0)], [(0, 4)], [(0, 1), (1, 1)], [(f % n, f % 4) for f in range(n + 1)]):
            assert code(prog.keyframes_insert, bad) == T.ORB_EINVAL, bad
        assert code(prog.match_keyframes, [(0, 0)]) == T.ORB_EINVAL  # every slot is empty
        model = {}
        _insert(prog, inp, [(0, 0), (1, 2)], model)
        with pytest.raises(T.OrbError) as e:  # the message names the first empty one: entry 2, slot 1 -- not entry 3's slot 3
            prog.match_keyframes([(0, 0), (1, 2), (2, 1), (3, 3), (4, 1)])
        assert e.value.code == T.ORB_EINVAL and "entry 2 names slot 1," in str(e.value), str(e.value)
        _insert(prog, inp, [(1, 1), (2, 2)], model)
        assert code(prog.match_keyframes, [(0, 0), (1, 3)]) == T.ORB_EINVAL and code(prog.match_keyframes, [(n, 0)]) == T.ORB_EINVAL  # slot 3 is empty
        assert code(prog.localize_keyframes, 1, **INTR) == T.ORB_ESTATE  # no match yet
        recs, masks, rows, blob = _check(prog, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)
        assert (recs["status"] == T.ORB_LOCALIZE_OK).all()
        for kw in (dict(fx=0.0), dict(cy=float("nan")), dict(max_reproj_px=-1.0), dict(hypotheses=4097), dict(max_distance=257), dict(ratio=-1.0),
                   dict(reserved=(0, 0, 0, 0, 0, 0, 1))):
            assert code(prog.localize_keyframes, 1, **{**INTR, **kw}) == T.ORB_EINVAL, kw
        assert code(prog.localize_keyframes, 0, **INTR) == T.ORB_EINVAL and code(prog.localize_keyframes, 4, **INTR) == T.ORB_EINVAL
        assert code(prog.localize_keyframes_read, 3) == T.ORB_EINVAL and code(prog.match_keyframes_read, 3, cap) == T.ORB_EINVAL
        # an insert after a match: the rows are of another store
        _insert(prog, inp, [(3, 3)], model)
        assert code(prog.localize_keyframes, 3, **INTR) == T.ORB_ESTATE
        assert _check(prog, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)[3] == blob
        # overwrite a slot with a shorter frame: the tail reads back as zeros
        short = b["counts"].copy()
        short[1] = 40
        C.inject(prog, short)
        inp2 = _inputs(prog, n, n, cap)
        assert inp2.nq[1] == 40 and model[3]["head"]["keypoints"] > 40
        _insert(prog, inp2, [(1, 3)], model)
        head, corners, descs, points = prog.keyframes_read(3, cap)
        assert head["keypoints"] == 40 and not corners[40:].tobytes().strip(b"\0") and not descs[40:].tobytes().strip(b"\0") and not points[40:].tobytes().strip(b"\0")
        C.inject(prog, b["counts"])
        # remove, then list the slot
        prog.keyframes_remove(3)
        assert not _slot_bytes(prog, 3, cap).strip(b"\0")
        assert code(prog.match_keyframes, [(0, 3)]) == T.ORB_EINVAL and code(prog.localize_keyframes, 3, **INTR) == T.ORB_ESTATE
        assert code(prog.keyframes_remove, 4) == T.ORB_EINVAL and code(prog.keyframes_read, 4) == T.ORB_EINVAL
        # read, then load into another slot and into a second program: the rows and fixes are identical
        saved = _device_store(prog, [0, 1, 2])
        for s in (0, 1, 2):
            assert saved[s]["head"].tobytes() == model[s]["head"].tobytes()
        _load_kf(prog, 3, saved[0])
        assert _slot_bytes(prog, 3, cap) == _slot_bytes(prog, 0, cap)
        moved = [(4, 3), (3, 1), (0, 2)]
        r2, m2, rows2, _ = _check(prog, inp.nq, inp.corners, inp.descs, moved, hypotheses=64)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(rows2, rows)) and m2.tobytes() == masks.tobytes()
        assert [_loop_words(a) for a in r2] == [_loop_words(c) for c in recs] and r2["slot"].tolist() == [3, 1, 2]
        other.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        C.inject(other, b["counts"], inp.corners, inp.descs)
        other.keyframes_reserve(3)
        for s in (0, 1, 2):
            _load_kf(other, s, saved[s])
            assert _slot_bytes(other, s, cap) == _slot_bytes(prog, s, cap)
        r3, m3, rows3, blob3 = _check(other, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)
        assert blob3 == blob
        # what load refuses
        kf = saved[1]
        for field, value in (("keypoints", int(kf["head"]["keypoints"]) - 1), ("status", 0), ("status", 3), ("points", 0), ("reserved", (0, 0, 0, 1))):
            bad = dict(kf, head=kf["head"].copy())
            bad["head"][field] = value
            assert code(_load_kf, prog, 1, bad) == T.ORB_EINVAL, field
        assert code(_load_kf, prog, 4, kf) == T.ORB_EINVAL and _slot_bytes(prog, 1, cap) == _padded(model[1], cap)
        # hand-built keyframes through load: a point that is not finite, every key NONE (FEW), a NOMAP header
        wild = dict(saved[1], points=saved[1]["points"].copy())
        has = np.nonzero(wild["points"]["key"] != kfr.NONE)[0]
        wild["points"]["x"][has[0]], wild["points"]["z"][has[1]] = np.inf, np.nan
        bare = dict(saved[2], points=saved[2]["points"].copy(), head=saved[2]["head"].copy())
        bare["points"]["key"], bare["head"]["points"] = kfr.NONE, 0
        nomap = _hand_built(rng, 50, cap, T.ORB_KEYFRAME_NOMAP, keys=np.arange(50))
        for s, kf in ((1, wild), (2, bare), (3, nomap)):
            _load_kf(prog, s, kf)
            assert _slot_bytes(prog, s, cap) == _padded(kf, cap)
        recs, _, _, _ = _check(prog, inp.nq, inp.corners, inp.descs, [(3, 1), (0, 2), (4, 3), (4, 0)], hypotheses=64)
        assert recs["status"].tolist() == [T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_FEW, T.ORB_LOCALIZE_NOMAP, T.ORB_LOCALIZE_OK]


def test_streams_and_repeated_calls(tinyorb):
    """Insert on one stream, match and localise on another: the bytes of a single-stream run.  The first call again after calls with
    other lists: the first bytes."""
    import torch
    T = tinyorb
    b = K.out_and_back(2, nf=2, n_land=150)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs, others = [(4, 0), (3, 1), (0, 2), (4, 0)], [(1, 2), (2, 0), (0, 1)]
    entries = [(0, 0), (1, 1), (2, 2)]
    with _program(T, cap, n) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ)
        prog.keyframes_reserve(3)
        _insert(prog, inp, entries, {})
        want = _check(prog, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)[3]
        kept = [_slot_bytes(prog, s, cap) for s in range(3)]
        for s in range(3):
            prog.keyframes_remove(s)
        s1, s2 = torch.cuda.Stream(device=0), torch.cuda.Stream(device=0)
        prog.keyframes_insert(entries, stream=s1.cuda_stream)
        prog.match_keyframes(pairs, stream=s2.cuda_stream)
        prog.localize_keyframes(len(pairs), stream=s2.cuda_stream, hypotheses=64, **INTR)
        assert _check(prog, inp.nq, inp.corners, inp.descs, pairs, match=False, call=False, hypotheses=64)[3] == want
        assert [_slot_bytes(prog, s, cap) for s in range(3)] == kept
        # a localize of 4096 hypotheses on the second stream, an insert of other frames behind it on the first: it waits for the reader
        prog.localize_keyframes(len(pairs), stream=s2.cuda_stream, hypotheses=4096, **INTR)
        prog.keyframes_insert([(3, 0), (4, 1)], stream=s1.cuda_stream)
        got = b"".join(prog.localize_keyframes_read(i, cap)[0].tobytes() for i in range(len(pairs)))
        prog.keyframes_insert(entries, stream=s1.cuda_stream)
        prog.match_keyframes(pairs, stream=s2.cuda_stream)
        prog.localize_keyframes(len(pairs), stream=s1.cuda_stream, hypotheses=4096, **INTR)
        assert b"".join(prog.localize_keyframes_read(i, cap)[0].tobytes() for i in range(len(pairs))) == got
        # other lists in between, then the first call again
        _check(prog, inp.nq, inp.corners, inp.descs, others, hypotheses=512, seed=5)
        _check(prog, inp.nq, inp.corners, inp.descs, pairs[:2], max_reproj_px=1.0)
        assert _check(prog, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)[3] == want
        # the other stages' results before and after keyframe calls
        before = [prog.match_read(f, cap).tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)] + \
                 [prog.trajectory_read(f, cap)[0].tobytes() for f in range(n)]
        prog.keyframes_insert(entries)
        _check(prog, inp.nq, inp.corners, inp.descs, pairs, hypotheses=64)
        assert before == [prog.match_read(f, cap).tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)] + \
            [prog.trajectory_read(f, cap)[0].tobytes() for f in range(n)]
