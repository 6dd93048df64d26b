"""The graph stage on the GPU (orb_graph_pairs): every OrbGraphPose and OrbGraphEdge byte against the CPU
restatement (tests/graph_ref.py) fed with what the device holds -- orb_trajectory_read's records, the list, orb_loop_pairs_read's
fixes.  No tolerance anywhere.

The programs are 64 x 48.  The out-and-back batch (tests/loop_cases.py) goes through the real chain, match_pairs and loop_pairs on
the device, with drift written over the frame records behind the loop call.  The hand-built cases (tests/graph_cases.py) run the
chain on empty frames and write their frame records and fixes over the stages' buffers.

Shapes.  k_pg_solve strides 256 threads over a segment's free nodes and adds node j to partial j mod 256: segments of 1, 2, 255, 256
and 257 free nodes; it keeps a segment of at most 512 free nodes in LDS and a longer one in global memory: 512, 513 and 600."""
import collections

import numpy as np
import pytest

import constructed as C
import graph_cases as G
import graph_ref as gr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import trajectory_cases as tc

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0
W0, H0, FOCAL = 64, 48, 60.0
INTR = lc.intrinsics(W0, H0, FOCAL)
Held = collections.namedtuple("Held", "frames pairs fixes")


def _program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def _empty_chain(prog, n_batch, n_traj, pairs):
    """Every stage the graph call needs, fresh on a batch of empty frames: the records and fixes are written over afterwards."""
    tc.prepare(prog, n_batch, W0, H0)
    prog.trajectory_consecutive(n_traj)
    prog.landmarks_consecutive(n_traj, **INTR)
    prog.match_pairs(pairs)
    prog.loop_pairs(len(pairs), **INTR)


def _held(prog, n_traj, pairs):
    """What the call reads, as the device holds it."""
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_traj)])
    fixes = np.array([prog.loop_pairs_read(i, 0)[0] for i in range(len(pairs))])
    return Held(frames, list(pairs), fixes)


def _check(prog, held, n_pairs=None, call=True, stream=None, **params):
    """graph_pairs (call=False: the last one's results), then every frame's record and every entry's verdict against the
    restatement, byte for byte.  Returns (records, verdicts, the bytes of both)."""
    n = len(held.pairs) if n_pairs is None else n_pairs
    if call:
        prog.graph_pairs(n, stream=stream, **params)
    want, wedges = gr.graph_pairs(held.frames, held.pairs, held.fixes, n_pairs=n, **params)
    recs = np.array([prog.graph_read(f) for f in range(len(held.frames))])
    edges = prog.graph_edges(n)
    assert edges.tobytes() == wedges.tobytes(), (params, np.nonzero(edges != wedges)[0][:8], edges[:8], wedges[:8])
    bad = np.nonzero(recs != want)[0]
    assert recs.tobytes() == want.tobytes(), (params, bad[:8], recs[bad[:2]], want[bad[:2]])
    return recs, edges, recs.tobytes() + edges.tobytes()


def _bytes(prog, n_frames, n_pairs):
    return np.array([prog.graph_read(f) for f in range(n_frames)]).tobytes() + prog.graph_edges(n_pairs).tobytes()


def test_the_real_chain_with_drift(tinyorb):
    """Eleven frames out and back through match_pairs and loop_pairs on the device; every chain step of the trajectory's records
    turned and scaled before the call.  Lists of 1 and of P = 44 entries, a second call with another n_pairs, the same call twice."""
    T = tinyorb
    b = K.out_and_back(0)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(100))
    P = T.ORB_PAIRS_PER_FRAME * n
    pairs = (K.LOOP_PAIRS + [(q, t) for q in range(n) for t in range(n) if q != t])[:P]
    with _program(T, cap, n) as prog:
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        prog.loop_pairs(P, **INTR)
        fr = np.array([prog.trajectory_read(f, 0)[0] for f in range(n)])
        assert fr["status"].tolist() == [L.ORIGIN, L.START] + [L.CHAINED] * 9
        cams = [(np.eye(3), np.zeros(3))] + [(np.asarray(f["r"], np.float64).reshape(3, 3), np.asarray(f["t"], np.float64)) for f in fr[1:]]
        for k, (R, t) in enumerate(G.drifted(cams, bias=0.004, scale=1.01)):
            fr[k]["r"], fr[k]["t"] = R.reshape(9), t
        L.inject_frames(prog, fr)
        held = _held(prog, n, pairs)
        assert held.frames.tobytes() == fr.tobytes() and (held.fixes["status"][:9] == T.ORB_LOCALIZE_OK).all()
        recs, edges, _ = _check(prog, held, n_pairs=1)
        assert edges["verdict"][0] == T.ORB_GRAPH_EDGE_USED and (recs["status"][1:] == T.ORB_GRAPH_REFINED).all() and recs["loops"][1] == 1
        recs, edges, blob = _check(prog, held)
        used = int((edges["verdict"] == T.ORB_GRAPH_EDGE_USED).sum())
        print("P = %d entries: %d USED, cost %.6g -> %.6g, status %s" % (P, used, recs["cost_before"][1], recs["cost_after"][1], set(recs["status"].tolist())))
        assert used >= 9 and recs["loops"][1] == used and recs["cost_after"][1] < recs["cost_before"][1] and recs["status"][0] == T.ORB_GRAPH_HELD
        unit = np.linalg.norm(b["steps"][0][1])
        true = [(R, t / unit) for R, t in K.cameras(b)]
        assert G.worst_position_error(recs["r"], recs["t"], true) < G.worst_position_error(fr["r"], fr["t"], true)
        _check(prog, held, n_pairs=9)  # a second call with another n_pairs, then the first again, twice: byte-identical
        for _ in range(2):
            prog.graph_pairs(P)
            assert _bytes(prog, n, P) == blob
        with pytest.raises(T.OrbError) as e:
            prog.graph_pairs(P + 1)
        assert e.value.code == T.ORB_EINVAL


def _hand_built(prog, n_batch, frames, pairs, fixes):
    _empty_chain(prog, n_batch, len(frames), pairs)
    L.inject_frames(prog, frames)
    G.inject_fixes(prog, fixes)
    held = _held(prog, len(frames), pairs)
    assert held.frames.tobytes() == np.ascontiguousarray(frames).tobytes() and held.fixes.tobytes() == np.ascontiguousarray(fixes).tobytes()
    return held


def test_every_verdict_and_a_batch_of_segments(tinyorb):
    T = tinyorb
    a, b, fr = G.two_segments()
    nF = len(fr)
    cases = G.verdict_cases(a, nF)
    pairs = [c[0] for c in cases]
    fixes = np.array([c[1] for c in cases], T.LOOP_FIX_DTYPE)
    with _program(T, 32, nF + 1) as prog:
        held = _hand_built(prog, nF + 1, fr, pairs, fixes)
        recs, edges, _ = _check(prog, held)
        assert edges["verdict"].tolist() == [c[2] for c in cases]
        assert recs["loops"][[1, 7, 11, 0, 10]].tolist() == [5, 3, 1, 0, 0]
        _check(prog, held, flags=T.ORB_GRAPH_USE_MINIMAL)
        _check(prog, held, min_inliers=11, loop_weight=4.0, rotation_weight=0.25)
        # one REFINED, one UNCHANGED, one INVALID: segment 6 loses its loops with the list's tail, segment 10 gets a NaN
        bad = fr.copy()
        bad["t"][11][2] = np.nan
        L.inject_frames(prog, bad)
        held = _held(prog, nF, pairs)
        recs, edges, _ = _check(prog, held, n_pairs=6)
        assert edges["verdict"].tolist()[5] == T.ORB_GRAPH_EDGE_SEGMENT_INVALID
        assert recs["status"].tolist() == [T.ORB_GRAPH_HELD] + [T.ORB_GRAPH_REFINED] * 6 + [T.ORB_GRAPH_UNCHANGED] * 3 + [T.ORB_GRAPH_HELD, T.ORB_GRAPH_INVALID]
        assert np.isnan(recs["t"][11][2]) and recs["r"][7:].tobytes() == bad["r"][7:].tobytes()
        # a NaN in an origin's own record is never read
        bad = fr.copy()
        bad["r"][0][:] = np.nan
        L.inject_frames(prog, bad)
        recs, edges, _ = _check(prog, _held(prog, nF, pairs))
        assert edges["verdict"][0] == T.ORB_GRAPH_EDGE_USED and recs["status"][1] == T.ORB_GRAPH_REFINED and np.isnan(recs["r"][0]).all()


def test_segment_sizes_around_the_block(tinyorb):
    """Segments of 1, 2, 255, 256 and 257 free nodes in one batch; rounds 1 and 16; cg_iterations 1, 0 and 512."""
    T = tinyorb
    fr, pairs, fixes = G.segments_batch((1, 2, 255, 256, 257))
    with _program(T, 32, len(fr)) as prog:
        held = _hand_built(prog, len(fr), fr, pairs, fixes)
        recs, edges, _ = _check(prog, held)
        assert (edges["verdict"] == T.ORB_GRAPH_EDGE_USED).all() and set(recs["status"].tolist()) <= {T.ORB_GRAPH_HELD, T.ORB_GRAPH_REFINED, T.ORB_GRAPH_STALLED}
        assert (recs["cost_after"][recs["loops"] > 0] < recs["cost_before"][recs["loops"] > 0]).all()
        _check(prog, held, rounds=1)
        _check(prog, held, cg_iterations=1)
    fr, pairs, fixes = G.segments_batch((1, 2, 31))
    with _program(T, 32, len(fr)) as prog:
        held = _hand_built(prog, len(fr), fr, pairs, fixes)
        _check(prog, held, rounds=16)
        _check(prog, held, rounds=2, cg_iterations=512)


def test_segments_across_the_lds_bound(tinyorb):
    """512 free nodes are solved in LDS, 513 and 600 in the stage's workspace: the same arithmetic."""
    T = tinyorb
    assert gr.LDS_NODES == 512
    fr, pairs, fixes = G.segments_batch((512, 513, 600))
    with _program(T, 32, len(fr)) as prog:
        held = _hand_built(prog, len(fr), fr, pairs, fixes)
        recs, edges, _ = _check(prog, held, rounds=2)
        assert (edges["verdict"] == T.ORB_GRAPH_EDGE_USED).all() and (recs["cost_after"][recs["loops"] > 0] < recs["cost_before"][recs["loops"] > 0]).all()
        assert recs["status"][[0, 513, 1027]].tolist() == [T.ORB_GRAPH_HELD] * 3 and recs["loops"][[1, 514, 1028]].tolist() == [2, 2, 2]


def test_the_undo_on_the_device(tinyorb):
    T = tinyorb
    fr, pairs, fixes = G.stall_case()
    with _program(T, 32, len(fr)) as prog:
        held = _hand_built(prog, len(fr), fr, pairs, fixes)
        one, _, _ = _check(prog, held, rounds=1)
        two, _, _ = _check(prog, held)
        assert (one["status"][1:] == T.ORB_GRAPH_REFINED).all() and (two["status"][1:] == T.ORB_GRAPH_STALLED).all()
        assert two["r"].tobytes() == one["r"].tobytes() and two["t"].tobytes() == one["t"].tobytes() and two["cost_after"][1] == one["cost_after"][1]


def test_state_arguments_isolation_and_ordering(tinyorb):
    import torch
    T = tinyorb
    b = K.out_and_back(2, nf=2, n_land=150)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs, other = [(4, 0), (3, 1), (0, 4)], [(1, 3), (2, 0), (4, 1), (0, 2)]

    def code(n_pairs=len(pairs), **kw):
        with pytest.raises(T.OrbError) as e:
            prog.graph_pairs(n_pairs, **kw)
        return e.value.code

    def read_code(fn, *args):
        with pytest.raises(T.OrbError) as e:
            fn(*args)
        return e.value.code

    with _program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        lib = T.load_library()
        assert read_code(prog.graph_read, 0) == T.ORB_ESTATE and read_code(prog.graph_edges, 1) == T.ORB_ESTATE  # no graph call yet
        assert read_code(prog.debug_loop_buffer) == T.ORB_ESTATE  # no loop call yet
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE  # nothing has run
        lc.inject(prog, b)
        C.inject(prog, b["counts"], None, desc)
        prog.trajectory_consecutive(n, **L.FULL_TRAJ)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        assert code() == T.ORB_ESTATE  # before loop_pairs
        assert read_code(prog.debug_loop_buffer) == T.ORB_ESTATE
        prog.loop_pairs(len(pairs), hypotheses=64, **INTR)
        assert prog.debug_loop_buffer()
        inf, nan = float("inf"), float("nan")
        for kw in (dict(reserved=(1, 0)), dict(reserved=(0, 7)), dict(rounds=17), dict(cg_iterations=513), dict(flags=2), dict(flags=3),
                   dict(loop_weight=-1.0), dict(loop_weight=nan), dict(loop_weight=inf), dict(rotation_weight=-0.5), dict(rotation_weight=nan),
                   dict(rotation_weight=inf), dict(n_pairs=0), dict(n_pairs=len(pairs) + 1)):
            assert code(**kw) == T.ORB_EINVAL, kw
        assert read_code(prog.graph_read, 0) == T.ORB_ESTATE  # none of them counts as a call
        held = _held(prog, n, pairs)
        assert (held.fixes["status"] == T.ORB_LOCALIZE_OK).all()
        assert lib.orb_graph_pairs(prog._handle(), len(pairs), None, None) == T.ORB_OK  # NULL params: the defaults
        recs, edges, blob = _check(prog, held, call=False)
        assert (edges["verdict"] == T.ORB_GRAPH_EDGE_USED).all() and recs["loops"][1] == 3
        # read errors
        assert read_code(prog.graph_read, n) == T.ORB_EINVAL and read_code(prog.graph_edges, len(pairs) + 1) == T.ORB_EINVAL
        assert lib.orb_graph_read(prog._handle(), 0, None) == T.ORB_EINVAL and lib.orb_graph_edges(prog._handle(), None, 1) == T.ORB_EINVAL
        assert lib.orb_graph_edges(prog._handle(), None, 0) == T.ORB_OK and len(prog.graph_edges(2)) == 2
        # isolation: the other stages' read-backs before and after graph calls
        prog.bridge_consecutive(n, **INTR)
        prog.adjust_consecutive(n, **INTR)
        prog.verify_pairs(len(pairs))

        def others():
            out = [prog.match_read(f, cap).tobytes() + prog.pose_read(f, cap)[0].tobytes() + prog.pose_read(f, cap)[1].tobytes() +
                   prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]
            out += [prog.trajectory_read(f, cap)[0].tobytes() + prog.trajectory_read(f, cap)[1].tobytes() + prog.bridge_read(f, cap)[0].tobytes() +
                    prog.bridge_read(f, cap)[1].tobytes() + prog.adjust_read(f, cap)[0].tobytes() + prog.adjust_read(f, cap)[1].tobytes() for f in range(n)]
            out += [prog.match_pairs_read(i, cap).tobytes() + prog.verify_pairs_read(i, cap)[0].tobytes() + prog.verify_pairs_read(i, cap)[1].tobytes() +
                    prog.loop_pairs_read(i, cap)[0].tobytes() + prog.loop_pairs_read(i, cap)[1].tobytes() for i in range(len(pairs))]
            return out

        before = others()
        assert _check(prog, held)[2] == blob
        _check(prog, held, n_pairs=2, rounds=2, cg_iterations=3, loop_weight=2.0)
        assert others() == before
        # ordering: a call on a second stream, then a call on the first, which waits for it before it overwrites the stage's buffers
        s = torch.cuda.Stream(device=0)
        prog.graph_pairs(len(pairs), stream=s.cuda_stream)
        assert _check(prog, held, call=False)[2] == blob
        assert _check(prog, held)[2] == blob
        assert _check(prog, held, stream=s.cuda_stream)[2] == blob
        # loop_pairs and the trajectory re-run on the first stream right behind a call on the second: each waits for it, and the
        # records are those of what the call read
        prog.graph_pairs(len(pairs), stream=s.cuda_stream, rounds=16, cg_iterations=512)
        prog.loop_pairs(len(pairs), hypotheses=32, seed=5, **INTR)
        prog.trajectory_consecutive(n)
        want, wedges = gr.graph_pairs(held.frames, held.pairs, held.fixes, rounds=16, cg_iterations=512)
        assert np.array([prog.graph_read(f) for f in range(n)]).tobytes() == want.tobytes() and prog.graph_edges(len(pairs)).tobytes() == wedges.tobytes()
        held2 = _held(prog, n, pairs)
        blob2 = _check(prog, held2)[2]  # and the next call reads the new records and fixes
        # match_pairs with another list right behind a call on another stream: it waits, and the verdicts are those of the list read
        prog.graph_pairs(len(pairs), stream=s.cuda_stream)
        prog.match_pairs(other)
        assert _check(prog, held2, call=False)[2] == blob2
        # a new batch, or another output set: the stages before are stale
        prog.extract_batch_host(np.zeros((n, H0, W0, 4), np.uint8))
        assert code() == T.ORB_ESTATE
        assert code(rounds=17) == T.ORB_EINVAL and code(n_pairs=0) == T.ORB_ESTATE  # a parameter error comes before the state, the state before n_pairs
        prog.match_consecutive(n)
        prog.verify_epipolar(n)
        prog.pose_consecutive(n, **INTR)
        prog.trajectory_consecutive(n)
        prog.landmarks_consecutive(n, **INTR)
        prog.match_pairs(pairs)
        assert code() == T.ORB_ESTATE  # the loop stage is not fresh
        prog.loop_pairs(len(pairs), **INTR)
        prog.batch_select_output(1)
        assert code() == T.ORB_ESTATE
        prog.batch_select_output(0)
        _check(prog, _held(prog, n, pairs))  # fresh again: parity on the new batch's own (empty) records
