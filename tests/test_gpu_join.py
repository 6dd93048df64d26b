"""The join stage on the GPU (orb_join_pairs): every OrbJoinPose, OrbJoinSegment and OrbJoinLink byte against
the CPU restatement (tests/join_ref.py) fed with what the device holds -- its counts, orb_match_read, orb_match_pairs_read,
orb_trajectory_read, orb_landmarks_read and orb_loop_pairs_read output.  No tolerance anywhere.

The programs are 64 x 48.  A batch (tests/join_cases.py, tests/loop_cases.py) is written over the stages' buffers with descriptors
(constructed.inject, trajectory_cases.inject_pose, landmark_cases.inject_frames); fixes and inlier bytes are written over the loop
stage's where a case needs its own (graph_cases.inject_fixes, join_cases.inject_masks).

Shapes.  k_sj_ratio strides 256 threads over the capacity and selects the median through 256-bin histograms: at capacity 300 under
raw counters of 311 an entry has 0, 1, 7, 8, 255, 256, 257 and every reachable ratio; capacities 128 and 16 elsewhere."""
import numpy as np
import pytest

import constructed as C
import graph_cases as G
import join_cases as J
import join_ref as jr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K

pytestmark = pytest.mark.gpu

H0, W0, INTR = J.H0, J.W0, J.INTR
NONE = 0xFFFFFFFF


def _verdicts(T):
    return dict(HOLDS=T.ORB_JOIN_LINK_HOLDS, SAME=T.ORB_JOIN_LINK_SAME, FORWARD=T.ORB_JOIN_LINK_FORWARD, NONFINITE=T.ORB_JOIN_LINK_NONFINITE,
                RATIO_FEW=T.ORB_JOIN_LINK_RATIO_FEW, STATUS=T.ORB_JOIN_LINK_STATUS, RANGE=T.ORB_JOIN_LINK_RANGE)


def test_out_and_back_with_a_lost_frame(tinyorb):
    """Eleven frames out and back, frame 5 LOST: lists of 1, 9 and P = 44 entries with duplicates; segment 5 joined to segment 0
    within the CPU test's bounds."""
    T, V = tinyorb, _verdicts(tinyorb)
    b = J.lost_batch(1)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(101))
    P = T.ORB_PAIRS_PER_FRAME * n
    pairs = (K.LOOP_PAIRS + [(10, 0), (9, 1), (6, 5), (5, 4), (5, 0), (10, 5)] + [(q, t) for q in range(n) for t in range(n) if q != t])[:P]
    assert len(pairs) == P == 44
    with J.program(T, cap, n) as prog:
        inp = J.load(prog, b, desc, traj=L.FULL_TRAJ)
        assert inp.frames["origin"].tolist() == [0] * 5 + [5] * 6 and inp.frames["status"][5] == L.LOST
        prog.match_pairs(pairs)
        prog.loop_pairs(P, **INTR)
        for k in (1, 9, P):
            poses, segs, links, _ = J.check(prog, inp, pairs, n_pairs=k)
            assert links["verdict"][0] == V["HOLDS"] and segs[5]["status"] == T.ORB_JOIN_SEGMENT_LINKED and segs[5]["root"] == 0
            assert poses["status"].tolist() == [0] * 5 + [1] * 6 and (poses["root"] == 0).all()
        want = {(0, 10): V["FORWARD"], (3, 2): V["SAME"]}
        assert links["verdict"][:9].tolist() == [want.get(pr, V["HOLDS"]) for pr in K.LOOP_PAIRS]
        i, j = pairs.index((10, 0)), len(K.LOOP_PAIRS)
        assert (i, pairs[j]) == (0, (10, 0)) and links[j]["verdict"] == V["HOLDS"] and links[j]["shared"] > 0  # a duplicate: other draws, its own fix
        chosen = np.nonzero(links["chosen"])[0]
        assert len(chosen) == 1 and segs[5]["link"] == chosen[0] and links["consistent"][chosen[0]] == links["consistent"][links["verdict"] == 0].max()
        true = J.true_gamma(b, 0, 5)
        holds = links["verdict"][:9] == V["HOLDS"]
        assert np.abs(links["gamma"][:9][holds].astype(np.float64) / true - 1).max() <= J.BOUNDS[0]
        for f in range(5, 11):
            _, (Rt, tt) = K.true_relative(b, f, 0, 0)
            assert K.rotation_error_deg(poses[f]["r"], Rt) <= J.BOUNDS[1] and np.linalg.norm(poses[f]["t"] - tt) <= J.BOUNDS[2], (f, poses[f])
        with pytest.raises(T.OrbError) as e:
            prog.join_pairs(P + 1)
        assert e.value.code == T.ORB_EINVAL


def _counts(T, prog, inp, pairs, wanted, cap):
    """Entry 0's inlier bytes rewritten so that it has exactly m ratios, for every m of `wanted` (None: every reachable one)."""
    V = _verdicts(T)
    rows, fx, masks = J.hold(prog, inp, pairs, len(pairs))
    eligible = _eligible(inp, rows[0], pairs[0], fx[0], cap)
    top = len(eligible)
    print("reachable ratios of entry 0:", top, "of", cap)
    for m in wanted:
        m = top if m is None else m
        assert m <= top
        mk = masks.copy()
        mk[0] = 0
        mk[0][eligible[:m]] = 1
        J.inject_masks(prog, mk)
        held = J.hold(prog, inp, pairs, len(pairs))
        assert held[2].tobytes() == mk.tobytes() and held[1].tobytes() == fx.tobytes()
        t = {}
        jr.join_pairs(inp.nq, inp.matches, rows, pairs, inp.frames, inp.lms, fx, mk, cap, L=inp.L, trace=t)
        assert len(t[0]) == m  # the m this builder produced, on the CPU
        poses, segs, links, _ = J.check(prog, inp, pairs, held=held)
        assert links["shared"][0] == m and (links["verdict"][0] == V["RATIO_FEW"]) == (m < 8)
        print(m, links["verdict"].tolist(), links["consistent"].tolist(), links["gamma"].tolist(), segs["link"].tolist())
    return top


def test_ratio_counts(tinyorb):
    """Capacity 300, raw counters 311, two segments: the inlier bytes of one entry rewritten so that it has exactly m ratios.
    count_batch reaches 152 ratios at most (a landmark must be stored in all four frames, and a frame stores 300 of the 340 it
    sees), so 255, 256, 257 and 300 are taken on the rail camera at the same capacity and counters, where every slot owns on both
    sides."""
    T = tinyorb
    cap = K.COUNT_CAP
    b = K.count_batch(cap)
    b["poses"]["status"][1] = T.ORB_POSE_LOW_PARALLAX  # frame 2 is LOST: segments 0 (frames 0, 1) and 2 (frames 2, 3)
    desc = K.plant(b, np.random.default_rng(301))
    pairs = [(3, 0), (2, 1), (3, 1)]
    with J.program(T, cap, b["n"]) as prog:
        inp = J.load(prog, b, desc, traj=L.FULL_TRAJ)
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all() and inp.frames["origin"].tolist() == [0, 0, 2, 2]
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **INTR)
        fx = J.hold(prog, inp, pairs, len(pairs))[1]
        assert (fx["status"] == T.ORB_LOCALIZE_OK).all() and (fx["origin"] == 0).all() and (fx["query_origin"] == 2).all()
        assert 64 < _counts(T, prog, inp, pairs, (0, 1, 7, 8, 64, None), cap) < 255
    b, lms = J.rail(K_=cap, cap=cap, scales={3: 2})
    b["counts"][:] = cap + 11
    desc = K.plant(b, np.random.default_rng(302))
    pairs = [(5, 0), (4, 2), (5, 0)]
    with J.program(T, cap, b["n"]) as prog:
        inp = J.load_rail(prog, b, desc)
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all()
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **L.RAIL)
        G.inject_fixes(prog, J.fixes(b, pairs))
        J.inject_masks(prog, np.array([J.mask(b, q) for q, t in pairs]))
        assert _counts(T, prog, inp, pairs, (0, 1, 7, 8, 255, 256, 257, None), cap) == cap


def _eligible(inp, row, pair, fx, cap):
    """The query slots of an entry that give a ratio under an inlier byte of 1, ascending."""
    import loop_ref as lpr
    q, T_ = pair
    own = lpr.owners(inp.nq, inp.matches, inp.frames, inp.lms, cap, inp.L)
    out = []
    one = np.zeros(cap, np.uint8)
    P, pt = [np.float32(x) for x in fx["pose_r"]], [np.float32(x) for x in fx["pose_t"]]
    Rq, tq = jr.camera(inp.frames, q, int(fx["query_origin"]))
    for a in range(int(inp.nq[q])):
        one[:] = 0
        one[a] = 1
        if len(jr.ratios(inp.nq[q], inp.nq[T_], row, one, own[T_], own[q], inp.lms, cap, P, pt, Rq, tq)):
            out.append(a)
    return np.array(out, np.int64)


def test_rail_chain_tie_gamma_and_nan(tinyorb):
    """The rail camera, hand-built fixes and inlier bytes: three chained segments and a two-way tie; gamma to the bit; a NaN in a
    fix and in q's record."""
    T, V = tinyorb, _verdicts(tinyorb)
    # three segments, 4 -> 2 -> 0, a direct link with fewer ratios, and a duplicate of the first entry
    b, lms = J.rail(J.THREE, scales={2: 2, 4: 8})
    desc = K.plant(b, np.random.default_rng(41))
    pairs = [(5, 3), (3, 0), (4, 1), (5, 3)]
    with J.program(T, b["cap"], b["n"]) as prog:
        inp = J.load_rail(prog, b, desc)
        assert inp.frames.tobytes() == np.ascontiguousarray(b["frames"]).tobytes()
        assert all(inp.lms[p].tobytes() == lms[p].tobytes() for p in range(b["n"] - 1))
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **L.RAIL)
        for i, (q, t) in enumerate(pairs):
            assert prog.match_pairs_read(i, 12)["index"].tolist() == J.row(b, q, t)["index"][:12].tolist()
        G.inject_fixes(prog, J.fixes(b, pairs))
        masks = np.array([J.mask(b, 5), J.mask(b, 3), J.mask(b, 4, range(9)), J.mask(b, 5)])
        J.inject_masks(prog, masks)
        poses, segs, links, _ = J.check(prog, inp, pairs)
        want = J.run(b, lms, pairs, masks=list(masks))  # the CPU's own batch, landmarks and rows: the same bytes
        assert poses.tobytes() == want[0].tobytes() and segs.tobytes() == want[1].tobytes() and links.tobytes() == want[2].tobytes()
        assert links["verdict"].tolist() == [V["HOLDS"]] * 4 and links["consistent"].tolist() == [12, 12, 9, 12] and links["chosen"].tolist() == [1, 1, 0, 0]
        assert segs["status"].tolist() == [1, 0, 2, 0, 2, 0] and segs["root"].tolist() == [0, 1, 0, 3, 0, 5] and segs["link"].tolist() == [NONE, NONE, 1, NONE, 0, NONE]
        assert segs[4]["sigma"] == np.float32(links["gamma"][1]) * np.float32(links["gamma"][0]) and abs(float(segs[4]["sigma"]) - 0.125) < 1e-4
        assert poses["status"].tolist() == [0, 0, 1, 1, 1, 1] and np.allclose(poses["t"][:, 0], [-0.5 * f for f in range(6)], atol=1e-4)
        poses, segs, links, _ = J.check(prog, inp, pairs, n_pairs=1)  # only 4 -> 2
        assert segs["root"].tolist() == [0, 1, 2, 3, 2, 5] and poses["root"].tolist() == [0, 0, 2, 2, 2, 2]
    # two segments: gamma to the bit, then the NaNs
    b, lms = J.rail(scales={3: 2})
    desc = K.plant(b, np.random.default_rng(42))
    pairs = [(5, 0), (4, 1), (3, 2), (5, 2), (4, 3), (0, 5)]
    with J.program(T, b["cap"], b["n"]) as prog:
        inp = J.load_rail(prog, b, desc)
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **L.RAIL)
        fx = J.fixes(b, pairs)
        masks = np.array([J.mask(b, q) for q, t in pairs])
        G.inject_fixes(prog, fx)
        J.inject_masks(prog, masks)
        poses, segs, links, blob = J.check(prog, inp, pairs)
        want = J.run(b, lms, pairs)
        assert links.tobytes() == want[2].tobytes() and abs(float(links["gamma"][0]) - 0.5) < 1e-4
        assert links["verdict"].tolist() == [V["HOLDS"]] * 4 + [V["SAME"], V["FORWARD"]] and links["chosen"].tolist() == [1, 0, 0, 0, 0, 0]
        # a NaN in the fix of entry 1 and in the record of frame 5: NONFINITE there and only there
        bad = fx.copy()
        bad["pose_t"][1][2] = np.nan
        G.inject_fixes(prog, bad)
        fr = b["frames"].copy()
        fr["r"][5][4] = np.nan
        L.inject_frames(prog, fr)
        inp2 = J.inputs(prog, b["n"], b["n"], b["cap"], L.RAIL)
        assert np.isnan(inp2.frames["r"][5][4]) and all(inp2.lms[p].tobytes() == inp.lms[p].tobytes() for p in range(5))
        poses, segs, links, _ = J.check(prog, inp2, pairs)
        assert links["verdict"].tolist() == [V["NONFINITE"], V["NONFINITE"], V["HOLDS"], V["NONFINITE"], V["SAME"], V["FORWARD"]]
        assert links["chosen"].tolist() == [0, 0, 1, 0, 0, 0] and poses["status"].tolist() == [0, 0, 0, 1, 1, 1] and np.isnan(poses[5]["r"]).any()
        G.inject_fixes(prog, fx)
        L.inject_frames(prog, b["frames"])
        assert J.check(prog, inp, pairs)[3] == blob  # nothing of the calls between is left


def test_state_arguments_isolation_and_ordering(tinyorb):
    import torch
    T, V = tinyorb, _verdicts(tinyorb)
    b = J.lost_batch(1)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs, other = [(10, 0), (9, 1), (3, 2), (0, 10), (7, 3)], [(1, 3), (8, 2), (4, 1), (0, 2)]
    np_ = len(pairs)

    def code(n_pairs=np_, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.join_pairs(n_pairs, **kw)
        return e.value.code

    def read_code(fn, *args):
        with pytest.raises(T.OrbError) as e:
            fn(*args)
        return e.value.code

    with J.program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        lib = T.load_library()
        h = prog._handle()
        assert read_code(prog.join_read, 0) == T.ORB_ESTATE and read_code(prog.join_segments, 1) == T.ORB_ESTATE and read_code(prog.join_links, 1) == T.ORB_ESTATE
        assert read_code(prog.debug_loop_mask_buffer) == T.ORB_ESTATE  # no loop call yet
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # nothing has run
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        assert code() == T.ORB_ESTATE and read_code(prog.debug_loop_mask_buffer) == T.ORB_ESTATE  # before loop_pairs
        prog.loop_pairs(np_, hypotheses=64, **INTR)
        assert prog.debug_loop_mask_buffer() and prog.debug_loop_buffer()
        inf, nan = float("inf"), float("nan")
        for kw in (dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 7)), dict(consistent_permille=1001), dict(flags=2), dict(flags=3),
                   dict(scale_tolerance=-1.0), dict(scale_tolerance=nan), dict(scale_tolerance=inf), dict(n_pairs=0), dict(n_pairs=np_ + 1)):
            assert code(**kw) == T.ORB_EINVAL, kw
        assert read_code(prog.join_read, 0) == T.ORB_ESTATE  # none of them counts as a call
        inp = J.inputs(prog, n, n, cap, INTR)
        held = J.hold(prog, inp, pairs, np_)
        assert lib.orb_join_pairs(h, np_, None, None) == T.ORB_OK  # NULL params: the defaults
        poses, segs, links, blob = J.check(prog, inp, pairs, call=False, held=held)
        assert links["verdict"].tolist() == [V["HOLDS"], V["HOLDS"], V["SAME"], V["FORWARD"], V["HOLDS"]] and segs[5]["root"] == 0
        # read errors
        assert read_code(prog.join_read, n) == T.ORB_EINVAL and read_code(prog.join_segments, n + 1) == T.ORB_EINVAL
        assert read_code(prog.join_links, np_ + 1) == T.ORB_EINVAL
        assert lib.orb_join_read(h, 0, None) == T.ORB_EINVAL and lib.orb_join_segments(h, None, 1) == T.ORB_EINVAL and lib.orb_join_links(h, None, 1) == T.ORB_EINVAL
        assert lib.orb_join_segments(h, None, 0) == T.ORB_OK and lib.orb_join_links(h, None, 0) == T.ORB_OK
        assert len(prog.join_links(2)) == 2 and len(prog.join_segments(n)) == n
        # constructed.check_read_arguments on the frame read: its "rows" argument stands for the record (64 bytes, below max_features)
        scratch = np.zeros((), T.JOIN_POSE_DTYPE)
        C.check_read_arguments(T, prog, lambda hh, i, rows, k: lib.orb_join_read(hh, i, rows if rows or k else scratch.ctypes.data), n, 1, head=False)
        # isolation: the other stages' read-backs before and after join calls
        prog.bridge_consecutive(n, **INTR)
        prog.adjust_consecutive(n, **INTR)
        prog.verify_pairs(np_)
        prog.graph_pairs(np_)

        def others():
            out = [prog.match_read(f, cap).tobytes() + prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                   prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]
            out += [prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() + prog.bridge_read(f, cap)[0].tobytes() +
                    prog.bridge_read(f, cap)[1].tobytes() + prog.adjust_read(f, cap)[0].tobytes() + prog.adjust_read(f, cap)[1].tobytes() +
                    prog.graph_read(f).tobytes() for f in range(n)]
            out += [prog.match_pairs_read(i, cap).tobytes() + prog.verify_pairs_read(i, cap)[0].tobytes() + prog.verify_pairs_read(i, cap)[1].tobytes() +
                    prog.loop_pairs_read(i, cap)[0].tobytes() + prog.loop_pairs_read(i, cap)[1].tobytes() for i in range(np_)]
            return out + [prog.graph_edges(np_).tobytes()]

        before = others()
        assert J.check(prog, inp, pairs)[3] == blob
        J.check(prog, inp, pairs, n_pairs=2, min_shared=30, scale_tolerance=0.01, consistent_permille=100, min_inliers=20)
        assert others() == before
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.join_pairs(np_, stream=s.cuda_stream)
        assert J.check(prog, inp, pairs, call=False)[3] == blob
        assert J.check(prog, inp, pairs)[3] == blob
        assert J.check(prog, inp, pairs, stream=s.cuda_stream)[3] == blob
        # the five stages it reads, re-run on the first stream right behind a call on the second: each waits for it, and the
        # records are those of what the call read
        held = J.hold(prog, inp, pairs, np_)
        prog.join_pairs(np_, stream=s.cuda_stream)
        prog.match_consecutive(n)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(other)
        prog.loop_pairs(len(other), hypotheses=32, seed=5, **INTR)
        assert J.check(prog, inp, pairs, call=False, held=held)[3] == blob
        # put the batch back; a landmarks call between the loop call and the join call: the owners follow the new landmarks
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        prog.loop_pairs(np_, hypotheses=64, **INTR)
        inp = J.inputs(prog, n, n, cap, INTR)
        assert J.check(prog, inp, pairs)[3] == blob
        prog.landmarks_consecutive(n, min_views=4, **INTR)  # fewer GOOD landmarks: fewer owners, on both sides of a ratio
        inp4 = J.inputs(prog, n, n, cap, INTR)
        assert sum(int((a["flags"] != c["flags"]).sum()) for a, c in zip(inp.lms, inp4.lms)) > 0
        poses, segs, links4, blob4 = J.check(prog, inp4, pairs)
        assert blob4 != blob and (links4["shared"] < links["shared"]).any() and (links4["shared"] <= links["shared"]).all()
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        assert code(flags=2) == T.ORB_EINVAL and code(n_pairs=0) == T.ORB_ESTATE  # a parameter error comes before the state, the state before n_pairs
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        assert code() == T.ORB_ESTATE  # the loop stage is not fresh
        prog.loop_pairs(np_, **INTR)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        J.check(prog, J.inputs(prog, n, n, cap, INTR), pairs)  # fresh again: parity on the new batch's own (empty) records
