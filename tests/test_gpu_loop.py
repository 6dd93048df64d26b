"""The loop stage on the GPU (orb_loop_pairs): every OrbLoopFix byte and inlier byte against the CPU
restatement (tests/loop_ref.py) fed with what the device holds -- its counts, records, orb_match_read, orb_match_pairs_read,
orb_trajectory_read and orb_landmarks_read output.  No tolerance anywhere.

The programs are 64 x 48.  A batch (tests/loop_cases.py) is written over the stages' buffers with descriptors
(constructed.inject, trajectory_cases.inject_pose, landmark_cases.inject_frames); the trajectory, landmarks and match_pairs calls
run on the device behind the injection.

Shapes.  k_loc_score takes the candidates in tiles of 256, k_lc_refine adds candidate j to partial j mod 256, k_lc_gather compacts
256 query slots per pass: at capacity 300 the candidate counts are 0, 5, 6, 7, 255, 256, 257 and 300 under raw counters above the
capacity; the score kernel takes 64 hypotheses per workgroup: 1, 64, 65 and 512; k_lc_index runs 256 landmark slots per block:
capacity 257 with every slot a landmark."""
import collections

import numpy as np
import pytest

import constructed as C
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import loop_ref as lpr
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)
Inputs = collections.namedtuple("Inputs", "nq corners matches frames lms L cap intr")


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _descriptors(prog, b, desc):
    C.inject(prog, b["counts"], None, desc)


def _load(prog, b, desc, traj=None, lm=None, L_frames=None):
    """A views batch over the program's buffers with its descriptors, then the trajectory and landmarks calls on the device."""
    lc.inject(prog, b)
    _descriptors(prog, b, desc)
    prog.trajectory_consecutive(b["n"], **(traj or {}))
    prog.landmarks_consecutive(b["n"] if L_frames is None else L_frames, **INTR, **(lm or {}))
    return _inputs(prog, b["n"], b["n"] if L_frames is None else L_frames, b["cap"], INTR)


def _load_rail(prog, b, desc):
    """A rail batch (no pose records; its frame records are written over the trajectory call's), then the landmarks call."""
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], b["corners"], desc)
    tc.inject_pose(prog, matches=b["matches"], points_=b["points"])
    prog.trajectory_consecutive(n)
    L.inject_frames(prog, b["frames"])
    prog.landmarks_consecutive(n, **L.RAIL)
    return _inputs(prog, n, n, b["cap"], L.RAIL)


def _inputs(prog, n_frames, L_frames, cap, intr, traj_frames=None):
    """What the call reads besides the rows, as the device holds it."""
    nq = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(nq[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(nq[f])) for f in range(L_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames if traj_frames is None else traj_frames)])
    lms = [prog.landmarks_read(p, cap)[1] for p in range(L_frames - 1)]
    return Inputs(nq, corners, matches, frames, lms, L_frames, cap, intr)


def _check(prog, inp, pairs, n_pairs=None, stream=None, match=True, call=True, **params):
    """match_pairs (match=False: the last one's rows), loop_pairs (call=False: the last one's results), then every entry's record and
    cap inlier bytes against the restatement, byte for byte.  Returns the device's records (LOOP_FIX_DTYPE (n_pairs,)), its inlier
    bytes and the bytes of everything read."""
    if match:
        prog.match_pairs(pairs)
    n = len(pairs) if n_pairs is None else n_pairs
    rows = [prog.match_pairs_read(i, int(inp.nq[q])) for i, (q, T) in enumerate(pairs)]
    if call:
        prog.loop_pairs(n, stream=stream, **inp.intr, **params)
    want, wmask = lpr.loop_pairs(inp.nq, inp.corners, inp.matches, rows, pairs, inp.frames, inp.lms, inp.cap, L=inp.L, n_pairs=n, **inp.intr, **params)
    recs, masks, blob = [], [], b""
    for i in range(n):
        rec, mask = prog.loop_pairs_read(i, inp.cap)
        assert rec.tobytes() == want[i].tobytes(), (i, pairs[i], params, rec, want[i])
        assert mask.tobytes() == wmask[i].tobytes(), (i, pairs[i], params, np.nonzero(mask != wmask[i])[0][:8])
        assert not mask[inp.nq[pairs[i][0]]:].any() and int(mask.sum()) == int(rec["inliers"])
        recs.append(rec)
        masks.append(mask)
        blob += rec.tobytes() + mask.tobytes()
    return np.array(recs), np.array(masks), blob


def _owners(inp):
    return lpr.owners(inp.nq, inp.matches, inp.frames, inp.lms, inp.cap, inp.L)


def test_candidate_counts_hypotheses_and_seeds(tinyorb):
    """Capacity 300, raw counters 311: 0 .. 300 candidates of one entry, then each hypothesis count under two seeds."""
    T = tinyorb
    cap = K.COUNT_CAP
    b = K.count_batch(cap)
    rng = np.random.default_rng(301)
    desc = K.plant(b, rng)
    pairs = [(3, 0), (0, 3), (3, 0)]
    with _program(T, cap, b["n"]) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ)
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all()
        assert inp.frames["status"].tolist() == [L.ORIGIN, L.START, L.CHAINED, L.CHAINED]
        own = _owners(inp)
        for M in K.COUNTS:
            d = K.set_candidates(desc, 3, 0, own[0], M, rng)
            _descriptors(prog, b, desc[:3] + [d])
            recs, _, _ = _check(prog, inp, pairs)
            print(M, recs["status"].tolist(), recs["candidates"].tolist(), recs["inliers"].tolist())
            if M < 6:
                assert recs["status"][0] == T.ORB_LOCALIZE_FEW and recs["candidates"][0] == 0 and recs["status"][2] == T.ORB_LOCALIZE_FEW
            else:
                assert recs["status"][0] != T.ORB_LOCALIZE_FEW and recs["candidates"][0] in (M, 0) and recs["candidates"][2] in (M, 0)
        _descriptors(prog, b, desc)
        first = None
        for hyps in (1, 64, 65, 512):
            for seed in (0, 0x9E3779B9):
                recs, _, blob = _check(prog, inp, pairs, match=first is None, hypotheses=hyps, seed=seed)
                first = blob if first is None else first
                assert recs["hypothesis"].max() < hyps
        assert _check(prog, inp, pairs, match=False, hypotheses=1, seed=0)[2] == first  # stale keys or bytes of the calls between would show


def test_lists_directions_and_the_edge_of_the_map(tinyorb):
    """Eleven frames out and back, landmarks of ten: lists of 1 and of P = 44 entries; backward, forward, consecutive and duplicate
    entries; T = L - 1, T = L (NOMAP), q >= L."""
    T = tinyorb
    b = K.out_and_back(0)
    n, cap, Lf = b["n"], b["cap"], b["n"] - 1
    desc = K.plant(b, np.random.default_rng(100))
    with _program(T, cap, n) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ, L_frames=Lf)
        assert inp.frames["status"].tolist() == [L.ORIGIN, L.START] + [L.CHAINED] * 9
        recs, masks, _ = _check(prog, inp, [(9, 1)])
        assert recs["status"][0] == T.ORB_LOCALIZE_OK and recs["origin"][0] == 0 and recs["query_origin"][0] == 0
        P = T.ORB_PAIRS_PER_FRAME * n
        pairs = (K.LOOP_PAIRS + [(9, 1), (0, 9), (10, 9), (9, 10), (1, 10), (10, 8), (3, 4), (4, 3)] + [(q, t) for q in range(n) for t in range(n) if q != t])[:P]
        assert len(pairs) == P == 44
        recs, masks, _ = _check(prog, inp, pairs)
        st = dict(zip(pairs, recs["status"].tolist()))
        assert all((s == T.ORB_LOCALIZE_NOMAP) == (t == 10) for (q, t), s in st.items())
        assert st[(0, 9)] == st[(10, 9)] == st[(10, 8)] == T.ORB_LOCALIZE_OK  # T = L - 1; q = 10 >= L
        i, j = pairs.index((9, 1)), len(K.LOOP_PAIRS)
        assert pairs[j] == (9, 1) and recs["candidates"][i] == recs["candidates"][j] and recs[i].tobytes() != recs[j].tobytes()  # other draws
        for k, (q, t) in enumerate(K.LOOP_PAIRS):  # the listed loop pairs against the true cameras, within tests/test_loop_ref.py's bounds
            if t < Lf:
                assert recs["status"][k] == T.ORB_LOCALIZE_OK
                (Rr, tr_), _ = K.true_relative(b, q, t, 0)
                assert K.rotation_error_deg(recs["r"][k], Rr) <= 0.6 and np.linalg.norm(recs["t"][k] - tr_) <= 0.126, (q, t, recs[k])
        with pytest.raises(T.OrbError) as e:
            prog.loop_pairs(P + 1, **INTR)
        assert e.value.code == T.ORB_EINVAL
        _check(prog, inp, pairs, n_pairs=5, match=False)


def test_restart_lost_and_contended_batches(tinyorb):
    T = tinyorb
    # both origins in one frame: a frame that ends a segment and is the origin of the next takes the old segment's landmarks
    b = L.restart_batch(300)
    desc = K.plant(b, np.random.default_rng(11))
    pairs = [(q, t) for q in range(8) for t in range(8) if q != t][:32]
    with _program(T, 300, 8) as prog:
        inp = _load(prog, b, desc, traj=L.RESTART_TRAJ)
        st = inp.frames["status"].tolist()
        print("restart", st, inp.frames["origin"].tolist())
        assert T.ORB_TRAJ_RESTART_SPREAD in st and T.ORB_TRAJ_CHAINED in st[2:]
        recs, _, _ = _check(prog, inp, pairs)
        ok = recs["status"] == T.ORB_LOCALIZE_OK
        assert len(set(recs["origin"][ok].tolist())) > 1 and (recs["origin"][ok] != recs["query_origin"][ok]).any()
        assert all(recs["origin"][k] == inp.frames["origin"][t] for k, (q, t) in enumerate(pairs) if ok[k])
    # a LOST target is its own origin and takes the landmarks that start in it
    b = K.lost_batch()
    desc = K.plant(b, np.random.default_rng(12))
    pairs = [(6, 5), (7, 5), (10, 5), (5, 6), (0, 5), (5, 0), (10, 0), (4, 6)]
    with _program(T, b["cap"], b["n"]) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ)
        assert inp.frames["status"].tolist()[4:7] == [L.CHAINED, L.LOST, L.START] and inp.frames["origin"].tolist()[4:8] == [0, 5, 5, 5]
        recs, _, _ = _check(prog, inp, pairs)
        print("lost", recs["status"].tolist(), recs["candidates"].tolist(), recs["origin"].tolist(), recs["query_origin"].tolist())
        assert recs["status"][0] == T.ORB_LOCALIZE_OK and recs["origin"][:3].tolist() == [5, 5, 5] and recs["query_origin"][:3].tolist() == [5, 5, 5]
        assert recs["pose_t"][0].tobytes() == recs["t"][0].tobytes()  # the identity goes through the same arithmetic
    # owner contention: merged chains that are all GOOD
    b = K.contention_batch()
    desc = K.plant(b, np.random.default_rng(13))
    pairs = [(5, 2), (5, 3), (0, 4), (1, 5), (4, 3)]
    with _program(T, b["cap"], b["n"]) as prog:
        inp = _load(prog, b, desc, traj=L.FULL_TRAJ, lm=K.CONTENTION_LM)
        reg = np.zeros((inp.L, inp.cap), np.int64)
        lpr.owners(inp.nq, inp.matches, inp.frames, inp.lms, inp.cap, inp.L, registered=reg)
        print("contended views", int((reg > 1).sum()), "of", int((reg > 0).sum()))
        assert (reg > 1).sum() >= 8
        _check(prog, inp, pairs)


def test_degenerate_clouds_nan_target_and_one_thread_blocks(tinyorb):
    T = tinyorb
    b, plane, line = K.flat_batch()
    rng = np.random.default_rng(21)
    desc = K.plant(b, rng)
    with _program(T, b["cap"], b["n"]) as prog:
        inp = _load_rail(prog, b, desc)
        assert inp.frames.tobytes() == np.ascontiguousarray(b["frames"]).tobytes()
        recs, _, _ = _check(prog, inp, [(5, 0), (0, 5), (3, 2)])
        assert (recs["status"] == T.ORB_LOCALIZE_OK).all() and np.allclose(recs["t"][:, 0], [-2.5, 2.5, -0.5], atol=1e-3)
        for lands in (plane, line):  # only the keypoints of a plane, then of a line, keep their descriptors in the query frame
            _descriptors(prog, b, desc[:5] + [K.keep_only(b, desc, 5, lands, rng)])
            recs, masks, _ = _check(prog, inp, [(5, 0), (0, 4), (5, 3)])
            assert recs["status"].tolist() == [T.ORB_LOCALIZE_DEGENERATE, T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_DEGENERATE]
            assert not masks[0].any() and not recs[0]["r"].any() and recs["candidates"].tolist()[::2] == [0, 0]
        _descriptors(prog, b, desc)
        # a NaN in the frame record of T: NOMAP for that target, and only there
        fr = b["frames"].copy()
        fr["t"][2][1] = np.nan
        L.inject_frames(prog, fr)
        inp = _inputs(prog, b["n"], b["n"], b["cap"], L.RAIL)
        assert np.isnan(inp.frames["t"][2][1])
        recs, masks, _ = _check(prog, inp, [(5, 2), (5, 0), (2, 5), (0, 2)])
        assert recs["status"].tolist() == [T.ORB_LOCALIZE_NOMAP, T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_OK, T.ORB_LOCALIZE_NOMAP] and not masks[0].any()
    # capacity 257, every slot a landmark: k_lc_index's and k_lc_gather's one-thread second block
    b = L.rail(6, 257, v_hi=L.V_HI)
    desc = K.plant(b, np.random.default_rng(22))
    with _program(T, 257, 6) as prog:
        inp = _load_rail(prog, b, desc)
        assert (_owners(inp) != lpr.NONE).all()
        recs, masks, _ = _check(prog, inp, [(5, 0), (0, 5), (3, 2)])
        assert recs["candidates"].tolist() == [257] * 3 and (recs["status"] == T.ORB_LOCALIZE_OK).all() and masks[:, 256].all()


def test_state_arguments_isolation_and_ordering(tinyorb):
    import torch
    T = tinyorb
    b = K.out_and_back(2, nf=2, n_land=150)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs, other = [(4, 0), (3, 1), (0, 4)], [(1, 3), (2, 0), (4, 1), (0, 2)]

    def code(n_pairs=len(pairs), **kw):
        with pytest.raises(T.OrbError) as e:
            prog.loop_pairs(n_pairs, **{**INTR, **kw})
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        lib = T.load_library()
        with pytest.raises(T.OrbError) as e:
            prog.loop_pairs_read(0, cap)  # no loop call yet
        assert e.value.code == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # nothing has run
        lc.inject(prog, b)
        _descriptors(prog, b, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        assert code() == T.ORB_ESTATE  # before match_pairs
        prog.match_pairs(pairs)
        inf, nan = float("inf"), float("nan")
        for kw in (dict(reserved=(1, 0, 0, 0, 0, 0, 0)), dict(reserved=(0, 0, 0, 0, 0, 0, 7)), dict(fx=0.0), dict(fy=-1.0), dict(fx=nan), dict(fy=inf),
                   dict(cx=nan), dict(cy=inf), dict(max_reproj_px=-1.0), dict(max_reproj_px=nan), dict(max_reproj_px=inf), dict(ratio=-0.5),
                   dict(ratio=nan), dict(hypotheses=4097), dict(max_distance=257), dict(n_pairs=0), dict(n_pairs=len(pairs) + 1)):
            assert code(**kw) == T.ORB_EINVAL, kw
        assert lib.orb_loop_pairs(prog._handle(), 1, None, None) == T.ORB_EINVAL  # NULL params: the intrinsics have no default
        assert lib.orb_loop_pairs(prog._handle(), 1, T.OrbLoopParams(), None) == T.ORB_EINVAL  # a zero-initialised struct is not valid
        with pytest.raises(T.OrbError) as e:
            prog.loop_pairs_read(0, cap)  # none of them counts as a call
        assert e.value.code == T.ORB_ESTATE
        inp = _inputs(prog, n, n, cap, INTR)
        recs, _, blob = _check(prog, inp, pairs, match=False, hypotheses=64)
        assert (recs["status"] == T.ORB_LOCALIZE_OK).all()
        # read errors
        with pytest.raises(T.OrbError) as e:
            prog.loop_pairs_read(len(pairs), cap)
        assert e.value.code == T.ORB_EINVAL
        assert lib.orb_loop_pairs_read(prog._handle(), 0, None, None, 5) == T.ORB_EINVAL  # inliers NULL with n > 0
        assert lib.orb_loop_pairs_read(prog._handle(), 0, None, None, 0) == T.ORB_OK
        assert len(prog.loop_pairs_read(1, cap + 100)[1]) == cap and len(prog.loop_pairs_read(1)[1]) == cap and len(prog.loop_pairs_read(1, 7)[1]) == 7
        C.check_read_arguments(T, prog, lib.orb_loop_pairs_read, len(pairs), 1, head=True)
        # isolation: the other stages' read-backs before and after loop calls
        prog.bridge_consecutive(n, **INTR)
        prog.adjust_consecutive(n, **INTR)
        prog.verify_pairs(len(pairs))

        def others():
            out = [prog.match_read(f, cap).tobytes() + prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                   prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]
            out += [prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() + prog.bridge_read(f, cap)[0].tobytes() +
                    prog.bridge_read(f, cap)[1].tobytes() + prog.adjust_read(f, cap)[0].tobytes() + prog.adjust_read(f, cap)[1].tobytes() for f in range(n)]
            out += [prog.match_pairs_read(i, cap).tobytes() + prog.verify_pairs_read(i, cap)[0].tobytes() + prog.verify_pairs_read(i, cap)[1].tobytes()
                    for i in range(len(pairs))]
            return out

        before = others()
        _check(prog, inp, pairs, match=False, hypotheses=64)
        _check(prog, inp, pairs, n_pairs=2, match=False, max_reproj_px=1.0, hypotheses=32)
        assert others() == before
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.loop_pairs(len(pairs), stream=s.cuda_stream, hypotheses=64, **INTR)
        assert _check(prog, inp, pairs, match=False, call=False, hypotheses=64)[2] == blob
        assert _check(prog, inp, pairs, match=False, hypotheses=64)[2] == blob
        assert _check(prog, inp, pairs, match=False, stream=s.cuda_stream, hypotheses=64)[2] == blob
        # match_pairs with another list right behind a 4096-hypothesis call on another stream: it waits, and the records are those of
        # the list the call read
        rows = [prog.match_pairs_read(i, int(inp.nq[q])) for i, (q, t) in enumerate(pairs)]
        want, wmask = lpr.loop_pairs(inp.nq, inp.corners, inp.matches, rows, pairs, inp.frames, inp.lms, cap, L=n, **INTR, hypotheses=4096)
        prog.loop_pairs(len(pairs), stream=s.cuda_stream, hypotheses=4096, **INTR)
        prog.match_pairs(other)
        for i in range(len(pairs)):
            rec, mask = prog.loop_pairs_read(i, cap)
            assert rec.tobytes() == want[i].tobytes() and mask.tobytes() == wmask[i].tobytes(), (i, rec, want[i])
        _check(prog, inp, other, match=False, hypotheses=64)  # and the next call reads the new list
        # the stages it reads on the first stream right behind a call on the second: each waits for it
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), stream=s.cuda_stream, hypotheses=64, **INTR)
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        assert _check(prog, inp, pairs, match=False, call=False, hypotheses=64)[2] == blob
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        assert code(fx=0.0) == T.ORB_EINVAL and code(n_pairs=0) == T.ORB_ESTATE  # a parameter error comes before the state, the state before n_pairs
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.match_pairs(pairs)
        assert code() == T.ORB_ESTATE  # the landmarks are not fresh
        prog.landmarks_consecutive(n, **INTR)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, _inputs(prog, n, n, cap, INTR), pairs, match=False)  # fresh again: parity on the new batch's own (empty) records
