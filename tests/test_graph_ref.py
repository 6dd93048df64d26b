"""The graph stage's restatement (tests/graph_ref.py) on hand-built records: each clause of PG-2 and PG-4 at
its boundary, PG-7's undo, the pieces of PG-5 / PG-6 against float64, and the accuracy of the whole against a float64 Gauss-Newton
written here."""
import numpy as np

import graph_cases as G
import graph_ref as gr
import localize_ref as lr
from tinyslam_amd import orb

F = np.float32
USED, STATUS, FEW, RANGE, SEGMENT, NONFINITE, SEG_INVALID = (orb.ORB_GRAPH_EDGE_USED, orb.ORB_GRAPH_EDGE_STATUS, orb.ORB_GRAPH_EDGE_FEW,
                                                             orb.ORB_GRAPH_EDGE_RANGE, orb.ORB_GRAPH_EDGE_SEGMENT, orb.ORB_GRAPH_EDGE_NONFINITE,
                                                             orb.ORB_GRAPH_EDGE_SEGMENT_INVALID)
HELD, UNCHANGED, REFINED, STALLED, FAILED, INVALID = (orb.ORB_GRAPH_HELD, orb.ORB_GRAPH_UNCHANGED, orb.ORB_GRAPH_REFINED, orb.ORB_GRAPH_STALLED,
                                                      orb.ORB_GRAPH_FAILED, orb.ORB_GRAPH_INVALID)


def test_nodes_of_a_segment():
    a, b, fr = G.two_segments()
    assert [gr.free_origin(fr, g) for g in range(12)] == [gr.NONE, 0, 0, 0, 0, 0, 0, 6, 6, 6, gr.NONE, 10] and gr.free_origin(fr, 12) == gr.NONE
    assert [gr.segment_nodes(fr, o) for o in (0, 6, 10, 3, 11)] == [6, 3, 1, 0, 0]
    assert gr.is_node(fr, 6, 0) and gr.is_node(fr, 6, 6) and not gr.is_node(fr, 7, 0) and not gr.is_node(fr, 10, 6)
    # a LOST or ORIGIN status inside a run ends it, whatever the origin word says
    cut = fr.copy()
    cut["status"][3] = G.LOST
    assert gr.segment_nodes(cut, 0) == 2 and gr.free_origin(cut, 4) == gr.NONE
    out, _ = gr.graph_pairs(cut, [(2, 0)], np.array([G.fix(np.eye(3), np.zeros(3), 0, status=G.FEW_FIX)]))
    assert out["status"].tolist() == [HELD, UNCHANGED, UNCHANGED] + [HELD] * 4 + [UNCHANGED] * 3 + [HELD, UNCHANGED]


def test_every_verdict_at_its_boundary():
    a, b, fr = G.two_segments()
    nF = len(fr)
    cases = G.verdict_cases(a, nF)
    pairs = [c[0] for c in cases]
    fixes = np.array([c[1] for c in cases], orb.LOOP_FIX_DTYPE)
    out, edges = gr.graph_pairs(fr, pairs, fixes)
    assert edges["verdict"].tolist() == [c[2] for c in cases]
    assert edges["origin"].tolist() == fixes["origin"].tolist()
    used = edges["verdict"] == USED
    assert (edges["cost_before"][~used] == 0).all() and (edges["cost_after"][~used] == 0).all() and (edges["cost_before"][0] > 0)
    assert out["loops"][1] == 5 and out["loops"][7] == 3 and out["loops"][11] == 1 and out["loops"][0] == out["loops"][10] == 0
    assert out["status"][[0, 10]].tolist() == [HELD, HELD] and out["status"][6] in (REFINED, STALLED) and (out["status"][1:7] == out["status"][6]).all()
    # ORB_GRAPH_USE_MINIMAL admits the MINIMAL fix and nothing else
    _, e2 = gr.graph_pairs(fr, pairs, fixes, flags=orb.ORB_GRAPH_USE_MINIMAL)
    assert e2["verdict"][2] == USED and e2["verdict"][1] == STATUS
    # min_inliers moves FEW's boundary
    _, e3 = gr.graph_pairs(fr, pairs, fixes, min_inliers=11)
    assert e3["verdict"][3] == USED
    # n_pairs cuts the list
    out4, e4 = gr.graph_pairs(fr, pairs, fixes, n_pairs=1)
    assert len(e4) == 1 and out4["loops"][1] == 1 and (out4["status"][7:10] == UNCHANGED).all()


def test_duplicates_and_reversed_entries_each_count():
    true = G.circle(12)
    fr = G.frames_of(G.drifted(true, bias=0.01))
    one = G.fixes_of(true, [(11, 0)])
    rev = G.fixes_of(true, [(0, 11)])
    o1, e1 = gr.graph_pairs(fr, [(11, 0)], one)
    o2, e2 = gr.graph_pairs(fr, [(11, 0), (11, 0)], np.concatenate([one, one]))
    o3, e3 = gr.graph_pairs(fr, [(11, 0), (0, 11)], np.concatenate([one, rev]))
    assert o1["loops"][1] == 1 and o2["loops"][1] == 2 and o3["loops"][1] == 2
    assert e2["cost_before"][0] == e2["cost_before"][1] == e1["cost_before"][0] and o2["cost_before"][1] > o1["cost_before"][1]
    assert o2["r"].tobytes() != o1["r"].tobytes() and e3["verdict"].tolist() == [USED, USED]
    # a doubled entry is a doubled weight, up to rounding
    o4, _ = gr.graph_pairs(fr, [(11, 0)], one, loop_weight=2.0)
    assert np.allclose(o4["t"], o2["t"], atol=1e-4) and np.isclose(o4["cost_before"][1], o2["cost_before"][1], rtol=1e-6)


def test_invalid_unchanged_and_the_origins_own_record():
    a, b, fr = G.two_segments()
    pairs = [(5, 0), (9, 6)]
    fixes = np.array([G.fix(*G.relative(a, 5, 0), 0), G.fix(*G.relative(b, 3, 0), 6)], orb.LOOP_FIX_DTYPE)
    base, e0 = gr.graph_pairs(fr, pairs, fixes)
    assert e0["verdict"].tolist() == [USED, USED]
    # a NaN in a free node's record: the whole segment INVALID, poses copied bit for bit; the other segment as before
    bad = fr.copy()
    bad["r"][3][4] = np.nan
    out, e = gr.graph_pairs(bad, pairs, fixes)
    assert e["verdict"].tolist() == [SEG_INVALID, USED] and (out["status"][1:7] == INVALID).all() and out["status"][0] == HELD
    assert out["r"][:7].tobytes() == bad["r"][:7].tobytes() and out["t"][:7].tobytes() == bad["t"][:7].tobytes()
    assert not out["cost_before"][:7].any() and not out["loops"][:7].any() and out[7:].tobytes() == base[7:].tobytes()
    # frame 6 is a free node of segment 0 (INVALID when its record is not finite) ...
    bad = fr.copy()
    bad["t"][6][0] = np.inf
    out, e = gr.graph_pairs(bad, pairs, fixes)
    assert e["verdict"].tolist() == [SEG_INVALID, USED] and out[7:].tobytes() == base[7:].tobytes()  # ... and as segment 6's origin never read
    # the origin's own record is never read
    bad = fr.copy()
    bad["r"][0][:] = np.nan
    bad["t"][10][:] = np.nan
    out, e = gr.graph_pairs(bad, pairs, fixes)
    assert e["verdict"].tolist() == [USED, USED] and out[1:10].tobytes() == base[1:10].tobytes() and out["status"][0] == HELD
    assert out["r"][0].tobytes() == bad["r"][0].tobytes()
    # a segment without USED edges
    out, e = gr.graph_pairs(fr, pairs[:1], fixes[:1])
    assert (out["status"][7:10] == UNCHANGED).all() and out["r"][7:10].tobytes() == fr["r"][7:10].tobytes() and out["t"][7:].tobytes() == fr["t"][7:].tobytes()
    assert not out["cost_before"][7:].any() and out["status"][11] == UNCHANGED


def test_chain_edges_start_at_zero_cost():
    """PG-3: the measurement of a chain edge is the relative pose of the records, so the cost before is the loop edges' alone."""
    true = G.circle(20)
    fr = G.frames_of(G.drifted(true))
    out, e = gr.graph_pairs(fr, [(19, 0), (10, 1)], G.fixes_of(true, [(19, 0), (10, 1)]))
    assert out["cost_before"][1] == F(e["cost_before"][0]) + F(e["cost_before"][1])
    assert out["cost_after"][1] > e["cost_after"].sum() > 0  # the chain edges carry the rest


def test_the_undo_of_a_round_that_raises_the_cost():
    fr, pairs, fixes = G.stall_case()
    one, _ = gr.graph_pairs(fr, pairs, fixes, rounds=1)
    two, _ = gr.graph_pairs(fr, pairs, fixes, rounds=2)
    dflt, _ = gr.graph_pairs(fr, pairs, fixes)
    assert (one["status"][1:] == REFINED).all() and (two["status"][1:] == STALLED).all() and one["cost_after"][1] < one["cost_before"][1]
    assert two["r"].tobytes() == one["r"].tobytes() and two["t"].tobytes() == one["t"].tobytes() and two["cost_after"][1] == one["cost_after"][1]
    assert dflt.tobytes() == two.tobytes()
    # the round that was undone did raise the cost
    tr = {}
    gr.graph_pairs(fr, pairs, fixes, rounds=1, trace=tr)
    seg = tr[0]
    with np.errstate(all="ignore"):
        seg.update(seg.solve_round())
        assert not seg.cost()[0] < one["cost_after"][1]


def test_the_block_solver_is_section_21s():
    rng = np.random.default_rng(5)
    D = rng.normal(size=(7, 6, 6)).astype(F)
    D = np.einsum("nij,nkj->nik", D, D).astype(F)
    D[3] = 0          # fails: a zero pivot
    D[5][2, :] = D[5][:, 2] = 0
    X, ok = gr.invert_blocks([[D[:, r, c] for c in range(6)] for r in range(6)])
    iu = np.triu_indices(6)
    for n in range(7):
        cols = [lr.solve(np.concatenate([D[n][iu], np.eye(6, dtype=F)[k]]), 6) for k in range(6)]
        assert ok[n] == all(c is not None for c in cols)
        if ok[n]:
            assert X[n].tobytes() == np.stack(cols, 1).astype(F).tobytes()
    assert ok.tolist() == [True, True, True, False, True, False, True]


def test_the_operator_is_the_jacobians_product():
    """H p applied edge by edge, the gradient and the diagonal blocks against a dense float64 J of PG-5's Jacobians."""
    true = G.circle(9)
    fr = G.frames_of(G.drifted(true, bias=0.02))
    pairs = [(8, 0), (0, 5), (6, 2), (6, 2)]
    fx = G.fixes_of(true, pairs)
    p = gr.defaults(loop_weight=3.0, rotation_weight=0.5)
    loops = [(i, q, T, [np.full(1, v, F) for v in fx[i]["r"]], [np.full(1, v, F) for v in fx[i]["t"]]) for i, (q, T) in enumerate(pairs)]
    seg = gr.Segment(fr, 0, 8, loops, p)
    J, e = _system(fr, pairs, fx, rho=0.5, lw=3.0)
    H = J.T @ J
    g, D = seg.gradient_and_blocks()
    assert np.allclose(g.T.reshape(-1), J.T @ e, atol=2e-4)
    for j in range(8):
        blk = np.array([[D[r][c][j] for c in range(6)] for r in range(6)])
        assert np.allclose(blk, H[6 * j:6 * j + 6, 6 * j:6 * j + 6], atol=2e-4)
    v = np.random.default_rng(1).normal(size=(6, 8)).astype(F)
    assert np.allclose(seg.apply(v).T.reshape(-1), H @ v.T.reshape(-1).astype(np.float64), atol=5e-4)
    assert np.isclose(seg.cost()[0], e @ e, rtol=1e-5)


# ---- the yardstick: a float64 Gauss-Newton on the same graph ------------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def _orth(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ np.diag([1, 1, np.linalg.det(U @ Vt)]) @ Vt


def _edges64(frames, pairs, fixes, lw):
    n = len(frames)
    R = [np.eye(3)] + [np.asarray(f["r"], np.float64).reshape(3, 3) for f in frames[1:]]
    t = [np.zeros(3)] + [np.asarray(f["t"], np.float64) for f in frames[1:]]
    edges = []
    for g in range(1, n):
        Rz = R[g] @ R[g - 1].T
        edges.append((g - 1, g, Rz, t[g] - Rz @ t[g - 1], 1.0))
    for (q, T), fx in zip(pairs, fixes):
        edges.append((T, q, np.asarray(fx["r"], np.float64).reshape(3, 3), np.asarray(fx["t"], np.float64), lw))
    return R, t, edges


def _stack(R, t, edges, rho):
    n = len(R)
    J, e = np.zeros((6 * len(edges), 6 * n)), np.zeros(6 * len(edges))
    for k, (a, b, Rz, tz, w) in enumerate(edges):
        Rh = R[b] @ R[a].T
        E = Rh @ Rz.T
        sw = np.sqrt(w) * np.array([np.sqrt(rho)] * 3 + [1.0] * 3)
        e[6 * k:6 * k + 6] = sw * np.concatenate([0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]), t[b] - Rh @ t[a] - tz])
        J[6 * k:6 * k + 6, 6 * b:6 * b + 6] = sw[:, None] * np.block([[np.eye(3), np.zeros((3, 3))], [_skew(Rh @ t[a]), np.eye(3)]])
        J[6 * k:6 * k + 6, 6 * a:6 * a + 6] = sw[:, None] * np.block([[-Rh, np.zeros((3, 3))], [-Rh @ _skew(t[a]), -Rh]])
    return J[:, 6:], e


def _system(frames, pairs, fixes, rho=1.0, lw=1.0):
    R, t, edges = _edges64(frames, pairs, fixes, lw)
    return _stack(R, t, edges, rho)


def gn64(frames, pairs, fixes, rho=1.0, lw=1.0, iters=200):
    """A dense float64 Gauss-Newton on segment 0's graph -- PG-3..PG-5's edges, residual, Jacobians and update, with the nearest
    rotation in place of the polar step --, solved by numpy.linalg.solve and run until the cost stops falling.  Not the code under
    test: its own residuals, its own Jacobian matrix, its own solver.  Returns (r (n, 9), t (n, 3), cost before, cost)."""
    R, t, edges = _edges64(frames, pairs, fixes, lw)
    n = len(R)
    J, e = _stack(R, t, edges, rho)
    cost0 = cost = float(e @ e)
    for _ in range(iters):
        x = np.linalg.solve(J.T @ J, -J.T @ e).reshape(n - 1, 6)
        R2 = [R[0]] + [_orth((np.eye(3) + _skew(x[g - 1][:3])) @ R[g]) for g in range(1, n)]
        t2 = [t[0]] + [t[g] + x[g - 1][3:] for g in range(1, n)]
        J2, e2 = _stack(R2, t2, edges, rho)
        c2 = float(e2 @ e2)
        if not c2 < cost:
            break
        done = cost - c2 <= 1e-12 * cost
        R, t, J, e, cost = R2, t2, J2, e2, c2
        if done:
            break
    return np.array([r.reshape(9) for r in R]), np.array(t), cost0, cost


# Measured (this file prints them): the restatement's cost_after and largest camera-position error over the float64 result's.  The
# restatement is deterministic, so a margin covers a change of seeds only: twice the worst ratio measured over seeds 0-3.
OUT_AND_BACK_COST_RATIO, OUT_AND_BACK_ERR_RATIO = 2 * 1.0003, 2 * 0.9995
# One circle, one case: four rounds of 63 CG iterations stop short of the float64 minimum (sixteen rounds: cost 1.23, error 1.80 times)
CIRCLE_COST_RATIO, CIRCLE_ERR_RATIO = 2 * 2.3762, 2 * 3.2447
BIAS, SCALE = 0.004, 1.01


def _accuracy(fr, pairs, fixes, true_cams, cost_ratio, err_ratio, tag):
    out, edges = gr.graph_pairs(fr, pairs, fixes)
    r64, t64, c0, c64 = gn64(fr, pairs, fixes[:len(pairs)])
    before = G.worst_position_error(fr["r"], fr["t"], true_cams)
    after = G.worst_position_error(out["r"], out["t"], true_cams)
    e64 = G.worst_position_error(r64, t64, true_cams)
    cb, ca = float(out["cost_before"][1]), float(out["cost_after"][1])
    print("%s: cost %.6g -> %.6g (float64 %.6g -> %.6g, ratio %.4f); position error %.4f -> %.4f (float64 %.4f, ratio %.4f); used %d" %
          (tag, cb, ca, c0, c64, ca / c64, before, after, e64, after / e64, int((edges["verdict"] == USED).sum())))
    assert (out["status"][1:] == REFINED).all() and np.isclose(cb, c0, rtol=1e-4)
    assert ca < cb and after < before
    assert ca <= cost_ratio * c64 and after <= err_ratio * e64, (tag, ca / c64, after / e64)
    return ca / c64, after / e64


def test_accuracy_on_the_out_and_back_path():
    """Section 28's out-and-back path with its nine loop entries, seeds 0-3; every chain step of the trajectory's records turned by
    BIAS radians and its translation scaled by SCALE."""
    import landmark_cases as L
    import loop_cases as K
    worst = np.zeros(2)
    for seed in range(4):
        b = K.out_and_back(seed)
        desc = K.plant(b, np.random.default_rng(100 + seed))
        rows = K.rows_ref(desc, K.LOOP_PAIRS)
        fr, lms, fixes, masks = K.reference(b, K.LOOP_PAIRS, rows, traj=L.FULL_TRAJ)
        cams = [(np.eye(3), np.zeros(3))] + [(np.asarray(f["r"], np.float64).reshape(3, 3), np.asarray(f["t"], np.float64)) for f in fr[1:]]
        drift = fr.copy()
        for k, (R, t) in enumerate(G.drifted(cams, bias=BIAS, scale=SCALE)):
            drift[k]["r"], drift[k]["t"] = R.reshape(9), t
        unit = np.linalg.norm(b["steps"][0][1])
        true = [(R, t / unit) for R, t in K.cameras(b)]
        worst = np.maximum(worst, _accuracy(drift, K.LOOP_PAIRS, fixes, true, OUT_AND_BACK_COST_RATIO, OUT_AND_BACK_ERR_RATIO, "out-and-back seed %d" % seed))
    print("out-and-back worst ratios: cost %.4f, position error %.4f" % tuple(worst))


def test_accuracy_on_a_closed_circle():
    true = G.circle(64)
    fr = G.frames_of(G.drifted(true, bias=BIAS, scale=SCALE))
    r = _accuracy(fr, [(0, 63)], G.fixes_of(true, [(0, 63)]), true, CIRCLE_COST_RATIO, CIRCLE_ERR_RATIO, "circle of 64")
    print("circle ratios: cost %.4f, position error %.4f" % r)
