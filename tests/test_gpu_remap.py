"""The remap stage on the GPU (orb_remap_frames): every OrbRemapPose, OrbRemapRow and OrbLandmark byte against the
CPU restatement (tests/remap_ref.py) fed with what the device holds -- orb_trajectory_read, orb_landmarks_read, orb_graph_read and
orb_join_segments output.  No tolerance anywhere.

The programs are 64 x 48 with at most 12 frames.  A batch (tests/join_cases.py, tests/remap_cases.py) is written over the stages'
buffers as tests/test_gpu_join.py does.

Shapes.  k_rm_land runs 256 threads over a row of `cap` records, one or two slots per thread (two unless TINYORB_REMAP_SLOTS=1), a
wave's ballots giving the counts: capacities 16 (a quarter of one wave), 255, 256, 257 (the edges of a round of 256 slots: a second
round, or with one slot per thread a second workgroup, of one lane), 300, and 513 (a second workgroup at two slots per thread)."""
import numpy as np
import pytest

import constructed as C
import graph_cases as G
import join_cases as J
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import remap_cases as M
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

H0, W0, INTR = J.H0, J.W0, J.INTR
NONE = 0xFFFFFFFF


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_out_and_back_with_a_lost_frame(tinyorb):
    """Eleven frames out and back, frame 5 LOST: the graph refines segment 0, the join links segment 5 to it; all three flag
    settings, and the pose identities against orb_join_read, orb_graph_read and orb_trajectory_read."""
    T = tinyorb
    b = J.lost_batch(1)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(101))
    pairs = K.LOOP_PAIRS
    with M.program(T, cap, n) as prog:
        inp = M.load(prog, b, desc, traj=L.FULL_TRAJ)
        assert inp.frames["origin"].tolist() == [0] * 5 + [5] * 6
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **INTR)
        prog.graph_pairs(len(pairs))
        prog.join_pairs(len(pairs))
        gp = np.array([prog.graph_read(f) for f in range(n)])
        jp = np.array([prog.join_read(f) for f in range(n)])
        moved = np.isin(gp["status"], (T.ORB_GRAPH_REFINED, T.ORB_GRAPH_STALLED, T.ORB_GRAPH_FAILED))
        assert moved.any() and jp["status"].tolist() == [0] * 5 + [1] * 6
        blobs = {}
        for flags in M.FLAGS:
            poses, rows, lms, blobs[flags] = M.check(prog, inp, flags)
            if flags == M.JOIN:
                for k in ("r", "t", "scale", "gain", "root"):
                    assert _same(poses[k], jp[k]), k
                assert (poses["status"] == 2 * jp["status"]).all() and rows["moved"][:5].tolist() == [0] * 5 and (rows["moved"][5:] == rows["good"][5:]).all()
            elif flags == M.GRAPH:
                assert _same(poses["r"], gp["r"]) and _same(poses["t"], gp["t"]) and _same(poses["scale"], inp.frames["scale"])
                assert (poses["status"] == moved).all() and (poses["root"] == inp.frames["origin"]).all()
            else:
                assert (poses["status"] == moved + 2 * jp["status"]).all() and (poses["root"] == 0).all()
                assert rows["root"].tolist() == [0] * 4 + [NONE] + [0] * 5 and (rows["dropped"] == 0).all() and rows["moved"].sum() > 100
        assert blobs[0] == blobs[3] and len({blobs[1], blobs[2], blobs[3]}) == 3
        # no USED edge and no LINKED segment: the trajectory's words, the landmark records
        prog.graph_pairs(1, min_inliers=100000)
        prog.join_pairs(1, min_inliers=100000)
        poses, rows, lms, _ = M.check(prog, inp)
        assert _same(poses["r"], inp.frames["r"]) and _same(poses["t"], inp.frames["t"]) and _same(poses["scale"], inp.frames["scale"])
        assert (poses["status"] == 0).all() and (rows["moved"] == 0).all() and all(_same(lms[p], prog.landmarks_read(p, cap)[1]) for p in range(n - 1))


RAILS = {"two": (J.TWO, {3: 2}, [(5, 0), (4, 2)], {3: 0}), "three": (J.THREE, {2: 2, 4: 8}, [(5, 3), (3, 0), (4, 1)], {2: 0, 4: 0})}


@pytest.mark.parametrize("cap", (16, 255, 256, 257, 300, 513))
@pytest.mark.parametrize("which", sorted(RAILS))
def test_rail_capacities(tinyorb, which, cap):
    _rail(tinyorb, which, cap)


@pytest.mark.parametrize("cap", (257, 300))
def test_rail_capacities_one_slot_per_thread(tinyorb, monkeypatch, cap):
    """The other form of k_rm_land, which a program takes when TINYORB_REMAP_SLOTS=1 at its first remap call."""
    monkeypatch.setenv("TINYORB_REMAP_SLOTS", "1")
    _rail(tinyorb, "two", cap)


def _rail(tinyorb, which, cap):
    """The rail camera with every slot a landmark, raw counters of cap + 11, injected fixes and inlier bytes: every byte and the row
    counts are NumPy's; a remapped landmark of a linked segment is RM-5 evaluated in float64 on the same record; on three-frame
    segments it and the root segment's landmark of the same point both lie within 1e-4 of the point, and at capacity 16 within 1e-4
    of each other (DESIGN.md section 31 has why the larger rails and the two-frame segments are held to the former)."""
    T = tinyorb
    plan, scales, pairs, first = RAILS[which]
    b, _ = J.rail(plan, K_=cap, cap=cap, scales=scales)
    b["counts"][:] = cap + 11
    desc = K.plant(b, np.random.default_rng(300 + cap))
    with M.program(T, cap, b["n"]) as prog:
        inp = M.load_rail(prog, b, desc)
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all()
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **L.RAIL)
        G.inject_fixes(prog, J.fixes(b, pairs))
        J.inject_masks(prog, np.array([J.mask(b, q) for q, t in pairs]))
        prog.graph_pairs(len(pairs))
        prog.join_pairs(len(pairs))
        segs = prog.join_segments(b["n"])
        poses, rows, lms, blob = M.check(prog, inp)
        assert M.check(prog, inp, M.JOIN)[3] == blob and (poses["root"] == 0).all()
        src = [prog.landmarks_read(p, cap)[1] for p in range(b["n"] - 1)]
        for o, root in first.items():
            assert segs[o]["status"] == T.ORB_JOIN_SEGMENT_LINKED and tuple(rows[o]) == (cap, cap, 0, root)
            s, r = b["slots"][o], b["slots"][root]
            got = np.stack([lms[o][k][s].astype(np.float64) for k in "xyz"], 1)
            ref = np.stack([src[root][k][r].astype(np.float64) for k in "xyz"], 1)
            A, a = segs[o]["r"].astype(np.float64).reshape(3, 3), segs[o]["t"].astype(np.float64)
            X = np.stack([src[o][k][s].astype(np.float64) for k in "xyz"], 1)
            assert np.allclose(got, (float(segs[o]["sigma"]) * X - a) @ A, rtol=0, atol=1e-6 * np.abs(X).max())  # a few units in the last place of the terms
            assert (lms[o]["origin"][s] == root).all() and (src[o]["origin"][s] == o).all()
            print(which, cap, o, "remapped - root's own landmark, worst relative:", (np.abs(got - ref).max(1) / np.abs(ref).max(1)).max())
            if which == "two":  # three-frame segments: both landmarks of a point lie within 1e-4 of it (landmark_cases.near's measure)
                for X in (got, ref):
                    assert (np.abs(X - b["cloud"]).max(1) <= 1e-4 * np.abs(b["cloud"]).max(1)).all()
                if cap == 16:  # the twelve-landmark rail of the CPU test: within 1e-4 of each other as well
                    assert (np.abs(got - ref).max(1) <= 1e-4 * np.abs(ref).max(1)).all()
        for p in range(b["n"] - 1):
            if p not in first:
                assert _same(lms[p], src[p]) and rows[p]["moved"] == 0


def _load_anchored(prog, b, desc):
    """join_cases.load_rail with the landmarks call's parameters of the case."""
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], b["corners"], desc)
    tc.inject_pose(prog, matches=b["matches"], points_=b["points"])
    prog.trajectory_consecutive(n)
    L.inject_frames(prog, b["frames"])
    prog.landmarks_consecutive(n, **L.RAIL, **M.ANCHOR_LM)
    return J.inputs(prog, n, n, b["cap"], L.RAIL)


def test_graph_anchoring(tinyorb):
    """remap_cases.anchored: segment 2 refined by the graph and linked to segment 0; first views at the root's origin, at a HELD
    frame and at a moved frame.  Then a NaN in a frame record the graph reads (INVALID: everything is copied), and a frame record
    so large that C overflows (the records anchored there are dropped, no others)."""
    T = tinyorb
    b, pairs, fixes, masks = M.anchored()
    cap = b["cap"]
    desc = K.plant(b, np.random.default_rng(77))
    with M.program(T, cap, b["n"]) as prog:
        inp = _load_anchored(prog, b, desc)
        assert _same(inp.frames, np.ascontiguousarray(b["frames"]))
        prog.match_pairs(pairs)
        prog.loop_pairs(len(pairs), **L.RAIL)
        G.inject_fixes(prog, fixes)
        J.inject_masks(prog, masks)
        prog.graph_pairs(len(pairs))
        prog.join_pairs(len(pairs))
        gp = np.array([prog.graph_read(f) for f in range(6)])
        assert gp["status"].tolist()[:3] == [0, 1, 0] and np.isin(gp["status"][3:], (2, 3)).all() and (gp["loops"][3:] == 2).all()
        assert prog.join_segments(6)[2]["status"] == T.ORB_JOIN_SEGMENT_LINKED
        poses, rows, lms, blob = M.check(prog, inp)
        src = [prog.landmarks_read(p, cap)[1] for p in range(5)]
        assert poses["status"].tolist() == [0, 0, M.MOVED] + [M.MOVED | M.FROM_GRAPH] * 3 and (poses["root"] == 0).all()
        assert [tuple(r) for r in rows] == [(12, 0, 0, 0), (0, 0, 0, NONE), (9, 9, 0, 0), (3, 3, 0, 0), (0, 0, 0, 0)]
        assert _same(lms[0], src[0]) and not _same(lms[2], src[2]) and not _same(lms[3], src[3])
        only_graph = M.check(prog, inp, M.GRAPH)
        assert [int(r["moved"]) for r in only_graph[1]] == [0, 0, 0, 3, 0] and _same(only_graph[2][2], src[2]) and not _same(only_graph[2][3], src[3])
        only_join = M.check(prog, inp, M.JOIN)
        assert [int(r["moved"]) for r in only_join[1]] == [0, 0, 9, 3, 0] and _same(only_join[2][2], lms[2]) and not _same(only_join[2][3], lms[3])
        # a NaN in a free camera of segment 2: INVALID, nothing starts from the graph
        bad = b["frames"].copy()
        bad["t"][4][1] = np.nan
        L.inject_frames(prog, bad)
        prog.graph_pairs(len(pairs))
        inp2 = J.inputs(prog, 6, 6, cap, L.RAIL)
        assert np.array([prog.graph_read(f)["status"] for f in range(3, 6)]).tolist() == [T.ORB_GRAPH_INVALID] * 3
        poses, rows, lms2, _ = M.check(prog, inp2, M.GRAPH)
        assert _same(poses["r"], bad["r"]) and _same(poses["t"], bad["t"]) and (poses["status"] == 0).all() and (rows["moved"] == 0).all()
        assert all(_same(lms2[p], src[p]) for p in range(5))
        # frame 3's record of the trajectory out of range (the graph's, of the call before the NaN, stays): C overflows there
        L.inject_frames(prog, b["frames"])
        prog.graph_pairs(len(pairs))
        big = b["frames"].copy()
        big["r"][3][[0, 4, 8]] = 3e38
        big["t"][3] = 3e38
        L.inject_frames(prog, big)
        inp3 = J.inputs(prog, 6, 6, cap, L.RAIL)
        poses, rows, lms3, _ = M.check(prog, inp3)
        assert [tuple(r) for r in rows] == [(12, 0, 0, 0), (0, 0, 0, NONE), (9, 9, 0, 0), (3, 0, 3, 0), (0, 0, 0, 0)]
        late = b["slots"][3][list(M.ANCHOR_LATE)]
        d = lms3[3][late]
        assert (d["x"] == 0).all() and (d["y"] == 0).all() and (d["z"] == 0).all() and (d["flags"] == 0).all() and _same(d["views"], src[3][late]["views"])
        assert _same(lms3[2], lms[2]) and _same(np.delete(lms3[3], late), np.delete(src[3], late))
        L.inject_frames(prog, b["frames"])
        assert M.check(prog, J.inputs(prog, 6, 6, cap, L.RAIL))[3] == blob  # nothing of the calls between is left


def test_state_arguments_isolation_and_ordering(tinyorb):
    import torch
    T = tinyorb
    b = J.lost_batch(1)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs, other = [(10, 0), (9, 1), (3, 2), (0, 10), (7, 3)], [(1, 3), (8, 2), (4, 1), (0, 2)]
    np_ = len(pairs)

    def code(flags=0, **kw):
        with pytest.raises(T.OrbError) as e:
            prog.remap_frames(flags, **kw)
        return e.value.code

    def read_code(fn, *args):
        with pytest.raises(T.OrbError) as e:
            fn(*args)
        return e.value.code

    with M.program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        lib = T.load_library()
        h = prog._handle()
        assert read_code(prog.remap_read, 0) == T.ORB_ESTATE and read_code(prog.remap_landmarks, 0) == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # nothing has run
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        assert code(M.GRAPH) == T.ORB_ESTATE  # before the landmarks call
        prog.landmarks_consecutive(n, **INTR)
        for flags in M.FLAGS:
            assert code(flags) == T.ORB_ESTATE  # before any source
        prog.match_pairs(pairs)
        prog.loop_pairs(np_, hypotheses=64, **INTR)
        prog.graph_pairs(np_)
        assert code() == T.ORB_ESTATE and code(M.JOIN) == T.ORB_ESTATE and code(3) == T.ORB_ESTATE  # before the join call
        assert read_code(prog.remap_read, 0) == T.ORB_ESTATE  # none of them counts as a call
        inp = J.inputs(prog, n, n, cap, INTR)
        only_graph = M.check(prog, inp, M.GRAPH)[3]  # the graph alone is a whole call
        prog.join_pairs(np_)
        for kw in (dict(flags=4), dict(flags=7), dict(flags=0x80000000), dict(reserved=(1, 0, 0, 0, 0, 0, 0)), dict(reserved=(0, 0, 0, 0, 0, 0, 9))):
            assert code(**kw) == T.ORB_EINVAL, kw
        held = M.sources(prog, inp)
        assert lib.orb_remap_frames(h, None, None) == T.ORB_OK  # NULL params: the defaults
        poses, rows, lms, blob = M.check(prog, inp, call=False, held=held)
        assert blob != only_graph and (poses["root"] == 0).all()
        # read errors
        assert read_code(prog.remap_read, n) == T.ORB_EINVAL and read_code(prog.remap_landmarks, n - 1) == T.ORB_EINVAL
        assert lib.orb_remap_read(h, 0, None) == T.ORB_EINVAL and lib.orb_remap_landmarks(h, 0, None, None, 1) == T.ORB_EINVAL
        assert lib.orb_remap_landmarks(h, n - 2, None, None, 0) == T.ORB_OK and len(prog.remap_landmarks(0, 5)[1]) == 5
        C.check_read_arguments(T, prog, lambda hh, i, rws, k: lib.orb_remap_landmarks(hh, i, None, rws, k), n - 1, 32, head=False)
        # isolation: the other stages' read-backs before and after remap calls
        def others():
            out = [prog.match_read(f, cap).tobytes() + prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                   prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]
            out += [prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() + prog.graph_read(f).tobytes() +
                    prog.join_read(f).tobytes() for f in range(n)]
            out += [prog.match_pairs_read(i, cap).tobytes() + prog.loop_pairs_read(i, cap)[0].tobytes() + prog.loop_pairs_read(i, cap)[1].tobytes()
                    for i in range(np_)]
            return out + [prog.graph_edges(np_).tobytes(), prog.join_segments(n).tobytes(), prog.join_links(np_).tobytes()]

        before = others()
        for flags in M.FLAGS:
            M.check(prog, inp, flags)
        assert others() == before and M.check(prog, inp)[3] == blob
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.remap_frames(stream=s.cuda_stream)
        assert M.check(prog, inp, call=False)[3] == blob
        assert M.check(prog, inp, M.GRAPH)[3] == only_graph
        assert M.check(prog, inp, stream=s.cuda_stream)[3] == blob
        # the stages it reads, re-run on the first stream right behind a call on the second: each waits for it, and the records are
        # those of what the call read
        held = M.sources(prog, inp)
        prog.remap_frames(stream=s.cuda_stream)
        prog.graph_pairs(1, min_inliers=100000)
        prog.join_pairs(1, min_inliers=100000)
        prog.landmarks_consecutive(n, min_views=4, **INTR)
        prog.trajectory_consecutive(n)
        assert M.check(prog, inp, call=False, held=held)[3] == blob
        # put the batch back; a trajectory call of another frame count behind the graph and join calls: their extents are not F
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        prog.loop_pairs(np_, hypotheses=64, **INTR)
        prog.graph_pairs(np_)
        prog.join_pairs(np_)
        assert M.check(prog, J.inputs(prog, n, n, cap, INTR))[3] == blob
        prog.trajectory_consecutive(n - 1, **L.FULL_TRAJ)
        assert [code(f) for f in M.FLAGS] == [T.ORB_ESTATE] * 4 and code(4) == T.ORB_EINVAL
        prog.graph_pairs(np_)  # (10, 0) and (0, 10) are out of range now
        short = J.inputs(prog, n - 1, n, cap, INTR)
        poses, rows, lms, _ = M.check(prog, short, M.GRAPH)  # F = n - 1, and the landmarks call's n - 1 pairs cut to F - 1
        assert len(poses) == n - 1 and len(rows) == n - 2 and read_code(prog.remap_landmarks, n - 2) == T.ORB_EINVAL and read_code(prog.remap_read, n - 1) == T.ORB_EINVAL
        assert code(M.JOIN) == T.ORB_ESTATE and code() == T.ORB_ESTATE  # the join call is still of the trajectory of n frames
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE and code(M.GRAPH) == T.ORB_ESTATE
        assert code(8) == T.ORB_EINVAL  # a parameter error comes before the state
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        prog.loop_pairs(np_, **INTR)
        prog.graph_pairs(np_)
        assert code() == T.ORB_ESTATE  # the join stage is not fresh
        prog.join_pairs(np_)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        M.check(prog, J.inputs(prog, n, n, cap, INTR))  # fresh again: parity on the new batch's own (empty) records
