"""The later stages on extracted views, on the CPU: tests/layered_views.py's scenes through the oracle's intended-mode extraction and
the chained restatements (match -> verify_epipolar -> pose -> trajectory -> localize -> landmarks -> bridge -> adjust), once with
the records in the oracle's sorted order and once for each of 16 seeded orders of every frame's stored records.

tests/test_gpu_layered_chain.py runs the same chain on the device and requires, besides parity, that the device's records show
every one of the five later stages at work.  The device stores a band's records in the order of its LDS atomics and the RANSACs draw
by index, so what is required there must hold under any order: here every condition is asserted in all 17 runs of each scene, and
the weakest figures seen are printed (NOTEBOOK.md, "The later stages on extracted views", holds them).

Accuracy: only the `step` of the OK fixes is bounded, against the ratio of the true step lengths, in the sorted order.  Rotation and
direction of the two-view poses are printed, not bounded: two planes under a pure sideways step are close to degenerate for the
eight-point fit, and which F the verifier keeps depends on the draw.  With near shifts of 12 px a fifth of the poses went wrong
and 6 % of the orders lost a condition; the scenes move the near plane by 24 px, where none does (the notebook entry has the
singular values and the counts)."""
import numpy as np
import pytest

import layered_views as lv
import pose_ref as pr
from tinyslam_amd import orb as T

PERMUTATIONS = 16
# |step / true ratio - 1| of an OK fix: the worst over the 51 runs below was 0.01203 (the empty scene, order 10, the 2 : 1 step behind
# the gap; full 0.00167, roomy 0.00055); the bound is twice that, the project's usual margin
STEP_BOUND = 2 * 0.01203
_RUNS = {}


def runs(oracle, name):
    """The scene's 17 chains: [0] the sorted order, [k] the order of seed 1000 + k."""
    if name not in _RUNS:
        s = lv.scene(oracle, name)
        out = []
        for k in range(PERMUTATIONS + 1):
            b = s["batch"] if k == 0 else lv.permuted(*s["batch"], np.random.default_rng(1000 + k))
            out.append(lv.chain(*b, lv.W0, lv.H0, s["cap"], lv.INTR))
        _RUNS[name] = out
    return _RUNS[name]


def test_views_and_truth(oracle):
    frames, truth = lv.views(oracle, lv.STEPS_EMPTY, flat=(lv.EMPTY,))
    assert frames.shape == (9, lv.H0, lv.W0, 4) and frames.dtype == np.uint8
    assert (frames[lv.EMPTY, ..., :3] == lv.GREY).all()
    r = oracle.extract_intended(frames[lv.EMPTY], depth=2, threshold=lv.THR, arc=9, nms=True, max_features=lv.ROOMY)
    assert r["total"] == 0
    assert truth["ratio"].tolist() == [1, 2, 0.5, 1, 1, 2, 0.5] and truth["parallax"].tolist() == [True] * 3 + [False] * 2 + [True] * 3
    assert np.allclose(truth["direction"], [-2 / 5 ** 0.5, -1 / 5 ** 0.5, 0]) and np.array_equal(truth["r"], np.eye(3))
    plain, t2 = lv.views(oracle)
    assert t2["parallax"].tolist() == [True] * 4 + [False] + [True] * 3  # at the fifth step the camera stands still
    assert np.array_equal(plain[5], plain[4]) and not np.array_equal(plain[4], plain[3])
    # a step is a crop offset: the far rows of frame 1 are those of frame 0 moved by (2, 1), the near rows by (24, 12)
    h = lv.H0 // 2
    assert np.array_equal(plain[1][:h - 1, :-2], plain[0][1:h, 2:]) and np.array_equal(plain[1][h:-12, :-24], plain[0][h + 12:, 24:])
    with pytest.raises(AssertionError):
        lv.views(oracle, ((2, 12), (3, 12)))  # an odd shift is no integer offset along (2, 1)


def test_permuted_chain_pieces_and_differences(oracle):
    s = lv.scene(oracle, "roomy")
    counts, corners, desc = s["batch"]
    pc, pcor, pdesc = lv.permuted(counts, corners, desc, np.random.default_rng(3))
    assert pc is counts
    for f in range(len(counts)):
        assert not np.array_equal(pcor[f], corners[f])
        a, b = oracle.sort_keypoints(pcor[f], pdesc[f])
        assert np.array_equal(a, corners[f]) and np.array_equal(b, desc[f])
    base = runs(oracle, "roomy")[0]
    assert lv.differences(base, base) is None
    # the stages before `first` taken from an earlier result: the same bytes as one run; other parameters move later stages only
    again = lv.chain(*s["batch"], lv.W0, lv.H0, s["cap"], lv.INTR, first="trajectory", prior=base)
    assert lv.differences(again, base) is None and lv.blob(again) == lv.blob(base)
    other = lv.chain(*s["batch"], lv.W0, lv.H0, s["cap"], lv.INTR, first="localize", prior=base, adjust=dict(rounds=1), bridge=dict(hypotheses=1))
    d = lv.differences(other, base)
    assert d is not None and d.split(":")[0] in ("bridge", "adjust"), d
    assert other["adjusted"].tobytes() != base["adjusted"].tobytes()
    three = lv.chain(*s["batch"], lv.W0, lv.H0, s["cap"], lv.INTR, n_frames=3, first="trajectory", prior=base)
    assert three["n"] == 3 and len(three["pose"]) == 2 and len(three["bridge"]) == 3 and three["refined"].shape == (3, s["cap"])
    assert three["frames"].tobytes() == base["frames"][:3].tobytes()
    whole = lv.chain(*[x[:3] for x in s["batch"]], lv.W0, lv.H0, s["cap"], lv.INTR)
    assert lv.differences(three, whole) is None
    # one byte flipped in a late stage is reported at that stage, pair and slot
    bad = dict(base)
    bad["landmarks"] = base["landmarks"].copy()
    bad["landmarks"]["tail_index"][2, 17] ^= 1
    d = lv.differences(bad, base)
    assert d.startswith("landmarks: landmarks of pair 2 differs in 1 slots, the first [17]"), d
    bad = dict(base)
    bad["pose"] = base["pose"].copy()
    bad["pose"]["good"][5] += 1
    assert lv.differences(bad, base).startswith("pose: pose of pair 5"), lv.differences(bad, base)


def _report(name, res, truth):
    weakest = dict(ok_fixes=min(len(lv.ok_fixes(r)) for r in res), longest=min(int(r["rows"]["longest"].max()) for r in res),
                   good_three_views=min(lv.summary(r)["good_three_views"] for r in res),
                   pose_ok=min(int((r["pose"]["status"] == T.ORB_POSE_OK).sum()) for r in res),
                   chained=min(r["frames"]["status"].tolist().count(T.ORB_TRAJ_CHAINED) for r in res),
                   joined=min(r["bridge"]["status"].tolist().count(T.ORB_BRIDGE_JOINED) for r in res),
                   refined_better=min(int(((r["adjusted"]["status"] == T.ORB_ADJUST_REFINED) &
                                           (r["adjusted"]["cost_after"] < r["adjusted"]["cost_before"])).sum()) for r in res),
                   fix_inlier_share=min(min([r["fix"][p]["inliers"] / r["fix"][p]["candidates"] for p in lv.ok_fixes(r)] or [1.0]) for r in res))
    dev = [max(lv.step_deviations(r, truth).values() or [0.0]) for r in res]
    print("%s: weakest over %d orders %s; worst step deviation %.5f (order %d), sorted order %.5f" %
          (name, len(res), weakest, max(dev), int(np.argmax(dev)), dev[0]))
    return weakest, dev


def _print_sorted(name, res, truth):
    for k, v in lv.summary(res).items():
        print("  %s %s: %s" % (name, k, v))
    for p, q in enumerate(res["pose"]):  # printed, not bounded
        if q["status"] == T.ORB_POSE_OK and truth["parallax"][p]:
            print("  %s pair %d: rotation off by %.3f deg, direction off by %.3f deg, good %d" %
                  (name, p, pr.rotation_angle_deg(q["r"], truth["r"]), pr.direction_angle_deg(q["t"], truth["direction"]), int(q["good"])))


def test_roomy_conditions_in_every_order(oracle):
    """Capacity 1500, nine frames, the camera standing still at the fifth step."""
    s, res = lv.scene(oracle, "roomy"), runs(oracle, "roomy")
    counts = s["batch"][0]
    assert (counts < s["cap"]).all() and len(set(counts.tolist())) > 4 and all(c % 64 for c in counts), counts  # whatever the images give
    _print_sorted("roomy", res[0], s["truth"])
    for k, r in enumerate(res):
        try:
            lv.check_roomy(r)
        except AssertionError as e:
            raise AssertionError("order %d: %s" % (k, e)) from e
    weakest, dev = _report("roomy", res, s["truth"])
    st = res[0]["frames"]["status"].tolist()
    assert st == [T.ORB_TRAJ_ORIGIN, T.ORB_TRAJ_START] + [T.ORB_TRAJ_CHAINED] * 3 + [T.ORB_TRAJ_LOST, T.ORB_TRAJ_START] + [T.ORB_TRAJ_CHAINED] * 2
    assert res[0]["bridge"]["status"].tolist() == [T.ORB_BRIDGE_COPIED] * 5 + [T.ORB_BRIDGE_JOINED] + [T.ORB_BRIDGE_MOVED] * 3
    d = lv.step_deviations(res[0], s["truth"])
    assert sorted(d) == [1, 2, 3, 7] and max(d.values()) <= STEP_BOUND, d  # pair 6's fix is MINIMAL: pair 5's pose has 43 good points
    still = res[0]["fix"][4]  # the camera that stands still, against the map of the pair before
    assert still["status"] == T.ORB_LOCALIZE_OK and 2 * int(still["inliers"]) >= int(still["candidates"])
    print("roomy: step of the pair that stands still %.6f" % float(still["step"]))


def test_full_conditions_in_every_order(oracle):
    """Capacity 512: every frame's raw counter is above it."""
    s, res = lv.scene(oracle, "full"), runs(oracle, "full")
    counts, corners, desc = s["batch"]
    assert (counts > s["cap"]).all() and all(len(c) == s["cap"] for c in corners), counts
    for f in range(len(counts)):  # IM-8: the cut keeps a subset of the uncut records, descriptors and all
        wc, wd = s["whole"][1][f], s["whole"][2][f]
        have = {c.tobytes() + d.tobytes() for c, d in zip(wc, wd)}
        assert all(c.tobytes() + d.tobytes() in have for c, d in zip(corners[f], desc[f]))
    _print_sorted("full", res[0], s["truth"])
    for k, r in enumerate(res):
        assert (r["nq"] == s["cap"]).all()
        try:
            lv.check_full(r)
        except AssertionError as e:
            raise AssertionError("order %d: %s" % (k, e)) from e
    _report("full", res, s["truth"])
    d = lv.step_deviations(res[0], s["truth"])
    assert len(d) >= 2 and max(d.values()) <= STEP_BOUND, d


def test_empty_frame_conditions_in_every_order(oracle):
    """Capacity 1500, nine frames, frame 4 a constant grey: a raw counter of 0 inside the batch."""
    s, res = lv.scene(oracle, "empty"), runs(oracle, "empty")
    assert s["batch"][0][lv.EMPTY] == 0 and (np.delete(s["batch"][0], lv.EMPTY) > 400).all()
    _print_sorted("empty", res[0], s["truth"])
    for k, r in enumerate(res):
        try:
            lv.check_empty(r, lv.EMPTY)
        except AssertionError as e:
            raise AssertionError("order %d: %s" % (k, e)) from e
        assert r["bridge"]["status"][lv.EMPTY] == T.ORB_BRIDGE_UNFIXED and r["adjusted"]["status"][lv.EMPTY] == T.ORB_ADJUST_HELD
    _report("empty", res, s["truth"])
    d = lv.step_deviations(res[0], s["truth"])
    assert len(d) >= 2 and max(d.values()) <= STEP_BOUND, d
