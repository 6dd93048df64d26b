"""The remap stage's definition on the CPU restatement (tests/remap_ref.py), without a device: the identities
RM-2..RM-5 give, RM-5 one clause at a time on the rail camera, and the accuracy of a remap into the root on the out-and-back path
with a LOST frame against a float64 remap of the same records."""
import numpy as np

import graph_ref as gr
import join_cases as J
import join_ref as jr
import landmark_cases as L
import loop_cases as K
import remap_cases as M
import remap_ref as rr
from tinyslam_amd import orb as T

F = np.float32
NONE = 0xFFFFFFFF
GOOD = T.ORB_POINT_GOOD


def _lost(seed):
    """join_cases.lost_batch through the restatements up to the remap stage's inputs."""
    b = J.lost_batch(seed)
    desc = K.plant(b, np.random.default_rng(100 + seed))
    pairs = K.LOOP_PAIRS
    rows = K.rows_ref(desc, pairs)
    fr, lms, fx, masks = K.reference(b, pairs, rows, traj=L.FULL_TRAJ)
    nq = [min(int(c), b["cap"]) for c in b["counts"]]
    matches = [b["matches"][f][:nq[f]] for f in range(b["n"] - 1)]
    jposes, segs, links = jr.join_pairs(nq, matches, rows, pairs, fr, list(lms), fx, masks, b["cap"])
    gposes, edges = gr.graph_pairs(fr, pairs, fx)
    lrows = L.rows_from(lms, [M.origin_of_pair(fr, p) for p in range(len(lms))])
    return b, fr, lrows, list(lms), gposes, edges, jposes, segs


def _same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_identities_on_the_out_and_back_path():
    b, fr, lrows, lms, gposes, edges, jposes, segs = _lost(1)
    assert segs[5]["status"] == T.ORB_JOIN_SEGMENT_LINKED and (edges["verdict"] == T.ORB_GRAPH_EDGE_USED).any()
    moved = np.isin(gposes["status"], (T.ORB_GRAPH_REFINED, T.ORB_GRAPH_STALLED, T.ORB_GRAPH_FAILED))
    assert moved.any() and not moved.all()
    # the join alone: orb_join_read's words
    poses, rows, out = rr.remap_frames(fr, lrows, lms, gposes, segs, flags=M.JOIN)
    for k in ("r", "t", "scale", "gain", "root"):
        assert _same(poses[k], jposes[k]), k
    assert (poses["status"] == np.where(jposes["status"] == T.ORB_JOIN_MOVED, M.MOVED, 0)).all()
    assert rows["root"].tolist() == [0] * 4 + [NONE] + [0] * 5 and rows["good"].tolist() == lrows["good"].tolist()
    for p in range(10):
        sel = (lms[p]["flags"] & GOOD) != 0
        assert rows[p]["dropped"] == 0 and rows[p]["moved"] == (sel.sum() if p >= 5 else 0)
        assert _same(out[p][~sel], lms[p][~sel]) and (p >= 5 or _same(out[p], lms[p]))
        assert p < 5 or ((out[p]["origin"][sel] == 0).all() and (lms[p]["origin"][sel] == 5).all())
    # the graph alone: orb_graph_read's r, t; the trajectory's scale; no root but the origin
    poses, rows, out = rr.remap_frames(fr, lrows, lms, gposes, segs, flags=M.GRAPH)
    assert _same(poses["r"], gposes["r"]) and _same(poses["t"], gposes["t"]) and _same(poses["scale"], fr["scale"])
    assert (poses["root"] == fr["origin"]).all() and (poses["gain"] == 1).all() and (poses["status"] == np.where(moved, M.FROM_GRAPH, 0)).all()
    assert (rows["moved"] > 0).any() and all((o["origin"] == l["origin"]).all() for o, l in zip(out, lms))
    # both: a frame the graph moved starts from the graph's words
    both = rr.remap_frames(fr, lrows, lms, gposes, segs)[0]
    assert (both["status"] == np.where(moved, M.FROM_GRAPH, 0) + np.where(jposes["status"] == T.ORB_JOIN_MOVED, M.MOVED, 0)).all()
    assert _same(both, rr.remap_frames(fr, lrows, lms, gposes, segs, flags=3)[0])
    # no USED edge and no LINKED segment: the trajectory's words and the landmark records
    g0, s0 = gr.graph_pairs(fr, [(0, 10)], np.zeros(1, T.LOOP_FIX_DTYPE))[0], np.zeros(len(fr), T.JOIN_SEGMENT_DTYPE)
    assert not np.isin(g0["status"], (2, 3, 4)).any()
    poses, rows, out = rr.remap_frames(fr, lrows, lms, g0, s0)
    assert _same(poses["r"], fr["r"]) and _same(poses["t"], fr["t"]) and _same(poses["scale"], fr["scale"]) and (poses["status"] == 0).all()
    assert all(_same(o, l) for o, l in zip(out, lms)) and (rows["moved"] == 0).all() and (rows["root"] == lrows["origin"]).all()


def test_rail_landmarks_meet_the_root_segments():
    """The segments' units are powers of two and every product is exact: a remapped landmark of a linked segment is the root
    segment's landmark of the same physical point."""
    for plan, scales, pairs, first in ((J.TWO, {3: 2}, [(5, 0), (4, 2)], {3: 0}), (J.THREE, {2: 2, 4: 8}, [(5, 3), (3, 0), (4, 1)], {2: 0, 4: 0})):
        b, lms = J.rail(plan, scales=scales)
        worst = 0.0
        gp, segs, links, (poses, rows, out) = M.reference(b, lms, pairs)
        assert (links["verdict"] == T.ORB_JOIN_LINK_HOLDS).all() and not np.isin(gp["status"], (2, 3, 4)).any()
        for o, root in first.items():
            assert segs[o]["status"] == T.ORB_JOIN_SEGMENT_LINKED and rows[o]["root"] == root and rows[o]["moved"] == rows[o]["good"] == 12
            for l in range(12):
                rec, ref = out[o][b["slots"][o][l]], lms[root][b["slots"][root][l]]
                assert rec["flags"] & GOOD and rec["origin"] == root and ref["origin"] == root
                src = lms[o][b["slots"][o][l]]
                # a handful of binary32 operations on exact products: the float64 value to a few units in the last place of the terms
                assert np.allclose(_xyz(rec), _float64_step(_xyz(src), S=segs[o]), rtol=0, atol=1e-6 * np.abs(_xyz(src)).max()) and not L.near(src, b["cloud"][l])
                # TWO's segments have three frames.  THREE's have two, and a two-view solve of a point at depth 16 is itself up to
                # 1.2e-4 from the point before any remap: there the difference is printed
                assert plan is not J.TWO or (L.near(rec, _xyz(ref)) and L.near(rec, b["cloud"][l]))
                worst = max(worst, np.abs(_xyz(rec) - _xyz(ref)).max() / np.abs(_xyz(ref)).max())
        print("remapped against the root's own landmark, worst relative difference: %.2e" % worst)
        assert np.allclose(poses["t"][:, 0], [-L.RAIL_BASE * f for f in range(6)], atol=1e-4) and (poses["root"] == 0).all()


def _float64_step(X, R=None, t=None, Rg=None, tg=None, S=None):
    X = np.asarray(X, np.float64)
    if R is not None:
        X = np.asarray(Rg, np.float64).reshape(3, 3).T @ (np.asarray(R, np.float64).reshape(3, 3) @ X + np.asarray(t, np.float64) - np.asarray(tg, np.float64))
    if S is not None:
        X = np.asarray(S["r"], np.float64).reshape(3, 3).T @ (float(S["sigma"]) * X - np.asarray(S["t"], np.float64))
    return X


def _xyz(rec):
    return np.array([rec["x"], rec["y"], rec["z"]], np.float64)


def test_rm5_one_clause_at_a_time():
    b, pairs, fixes, masks = M.anchored()
    lms = [lm.copy() for lm in L.run(b, **M.ANCHOR_LM)[0]]
    gp, segs, links, (poses, rows, out) = M.reference(b, lms, pairs, fixes=fixes, masks=list(masks))
    fr = b["frames"]
    lrows = L.rows_from(np.array(lms), [M.origin_of_pair(fr, p) for p in range(5)])
    assert gp["status"].tolist()[:3] == [0, 1, 0] and np.isin(gp["status"][3:], (2, 3)).all() and segs[2]["status"] == T.ORB_JOIN_SEGMENT_LINKED
    assert lrows["origin"].tolist() == [0, NONE, 2, 2, 2] and [int(r["landmarks"]) for r in lrows] == [12, 0, 9, 3, 0]
    assert (lrows["good"] == lrows["landmarks"]).all()
    assert poses["status"].tolist() == [0, 0, M.MOVED] + [M.MOVED | M.FROM_GRAPH] * 3 and rows["root"].tolist() == [0, NONE, 0, 0, 0]
    assert rows["moved"].tolist() == [0, 0, 9, 3, 0] and (rows["dropped"] == 0).all()
    # a root segment, first views at its origin: copied
    assert _same(out[0], lms[0]) and _same(out[1], lms[1]) and _same(out[4], lms[4])
    # p = o, a HELD frame: the root step alone
    late = b["slots"][3][list(M.ANCHOR_LATE)]
    early = np.setdiff1d(b["slots"][2], b["slots"][2][list(M.ANCHOR_LATE)])
    for s in early:
        assert np.allclose(_xyz(out[2][s]), _float64_step(_xyz(lms[2][s]), S=segs[2]), atol=1e-4) and out[2][s]["origin"] == 0
    # a moved frame: both steps, and the anchor step alone under ORB_REMAP_GRAPH
    alone = rr.remap_frames(fr, lrows, lms, gp, segs, flags=M.GRAPH)
    assert alone[1]["moved"].tolist() == [0, 0, 0, 3, 0] and alone[1]["root"].tolist() == [0, NONE, 2, 2, 2] and _same(alone[2][2], lms[2])
    for s in late:
        X = _xyz(lms[3][s])
        step = dict(R=fr[3]["r"], t=fr[3]["t"], Rg=gp[3]["r"], tg=gp[3]["t"])
        assert np.allclose(_xyz(out[3][s]), _float64_step(X, S=segs[2], **step), atol=1e-4) and out[3][s]["origin"] == 0
        assert np.allclose(_xyz(alone[2][3][s]), _float64_step(X, **step), atol=1e-4) and alone[2][3][s]["origin"] == 2
        assert np.abs(_xyz(alone[2][3][s]) - X).max() > 1e-4  # the graph did move the camera
        for k in ("flags", "views", "inliers", "tail_index", "reserved"):
            assert _same(out[3][s][k], lms[3][s][k])
    # an anchor frame without FROM_GRAPH: the root step alone
    g2 = gp.copy()
    g2["status"][3] = T.ORB_GRAPH_UNCHANGED
    o2 = rr.remap_frames(fr, lrows, lms, g2, segs)
    assert _same(o2[2][3], rr.remap_frames(fr, lrows, lms, None, segs, flags=M.JOIN)[2][3]) and not _same(o2[2][3], out[3]) and not o2[0]["status"][3] & M.FROM_GRAPH
    # frame p names another origin than the row's: no anchor step
    f2 = fr.copy()
    f2["origin"][3] = 0
    assert _same(rr.remap_frames(f2, lrows, lms, gp, segs, flags=M.GRAPH)[2][3], lms[3])
    # views 0, not GOOD, a foreign origin word: the record is copied; the counts follow
    s = int(late[0])
    for field, value, good in (("views", 0, 3), ("flags", T.ORB_POINT_PARALLAX, 2), ("origin", 0, 3)):
        l2 = [lm.copy() for lm in lms]
        l2[3][s][field] = value
        _, r2, o2 = rr.remap_frames(fr, lrows, l2, gp, segs)
        assert _same(o2[3][s], l2[3][s]) and (int(r2[3]["good"]), int(r2[3]["moved"])) == (good, 2), field
        assert _same(np.delete(o2[3], s), np.delete(out[3], s))
    # o >= F: everything of the row is copied
    r3 = lrows.copy()
    r3["origin"][3] = 6
    l3 = [lm.copy() for lm in lms]
    l3[3]["origin"][late] = 6
    _, r2, o2 = rr.remap_frames(fr, r3, l3, gp, segs)
    assert _same(o2[3], l3[3]) and (int(r2[3]["moved"]), int(r2[3]["root"])) == (0, 6)
    # an overflow: dropped, there only
    s2 = segs.copy()
    s2["sigma"][2] = F(3e38)
    _, r2, o2 = rr.remap_frames(fr, lrows, lms, gp, s2)
    assert r2["dropped"].tolist() == [0, 0, 9, 3, 0] and (r2["moved"] == 0).all() and r2["good"].tolist() == rows["good"].tolist()
    for p in (2, 3):
        sel = (lms[p]["flags"] & GOOD) != 0
        d = o2[p][sel]
        assert (d["x"] == 0).all() and (d["y"] == 0).all() and (d["z"] == 0).all() and (d["flags"] == 0).all() and (d["origin"] == 0).all()
        assert _same(d["views"], lms[p][sel]["views"]) and _same(d["tail_index"], lms[p][sel]["tail_index"]) and _same(o2[p][~sel], lms[p][~sel])
    assert _same(o2[0], lms[0])


def _nearest_rotation(M_):
    U, _, Vt = np.linalg.svd(M_)
    return U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt


def accuracy(seeds=range(4), verbose=True):
    """Over the seeds: the restatement's worst pose difference (degrees, units of segment 0) and median landmark displacement from a
    float64 remap of the same records, and that float64 remap's own worst pose error against the true cameras."""
    diff, own = np.zeros(3), np.zeros(2)
    for seed in seeds:
        b, fr, lrows, lms, gposes, edges, jposes, segs = _lost(seed)
        assert segs[5]["status"] == T.ORB_JOIN_SEGMENT_LINKED and segs[5]["root"] == 0
        poses, rows, out = rr.remap_frames(fr, lrows, lms, gposes, segs)
        S = segs[5]
        A, a, sigma = np.asarray(S["r"], np.float64).reshape(3, 3), np.asarray(S["t"], np.float64), float(S["sigma"])
        e = np.zeros(3)
        o64 = np.zeros(2)
        for f in range(5, 11):
            cam = rr.camera(fr, gposes, f)
            R, t = np.asarray(cam["r"], np.float64).reshape(3, 3), np.asarray(cam["t"], np.float64)
            R64, t64 = _nearest_rotation(R @ A), R @ a + sigma * t
            _, (Rt, tt) = K.true_relative(b, f, 0, 0)
            e[0] = max(e[0], K.rotation_error_deg(poses[f]["r"], R64))
            e[1] = max(e[1], float(np.linalg.norm(np.asarray(poses[f]["t"], np.float64) - t64)))
            o64 = np.maximum(o64, (K.rotation_error_deg(R64, Rt), float(np.linalg.norm(t64 - tt))))
            assert poses[f]["root"] == 0 and poses[f]["status"] & M.MOVED
        d = []
        for p in range(5, 10):
            anchor = p != 5 and rr.from_graph(gposes, p)
            for s in np.nonzero((lms[p]["flags"] & GOOD) != 0)[0]:
                step = dict(R=fr[p]["r"], t=fr[p]["t"], Rg=gposes[p]["r"], tg=gposes[p]["t"]) if anchor else {}
                d.append(np.linalg.norm(_xyz(out[p][s]) - _float64_step(_xyz(lms[p][s]), S=S, **step)))
                assert out[p][s]["origin"] == 0
        e[2] = float(np.median(d))
        if verbose:
            print("seed %d: %d landmarks; restatement - float64: %.3e deg, %.3e units, median landmark %.3e units; float64 - truth: %.4f deg, %.4f units"
                  % (seed, len(d), *e, *o64))
        diff, own = np.maximum(diff, e), np.maximum(own, o64)
    if verbose:
        print("worst: restatement - float64 %s; float64 - truth %s" % (diff, own))
    return diff, own


def test_accuracy_of_a_remap_into_the_root():
    """Measured over seeds 0-3 (deterministic; printed by this test): see DESIGN.md section 31 for the figures.  The restatement's
    worst pose difference and median landmark displacement from the float64 remap are asserted at twice that remap's own worst error
    against loop_cases.true_relative (the landmarks at twice its position error, the same unit); the factor covers a change of
    seeds only.  Measured: restatement - float64 0.0196 degrees, 4.8e-7 units,
    median landmark 5.4e-7 units; float64 - truth 0.0941 degrees, 0.0433 units."""
    diff, own = accuracy()
    assert diff[0] <= 2 * own[0] and diff[1] <= 2 * own[1] and diff[2] <= 2 * own[1], (diff, own)
