"""The restatement of orb_match_pairs and orb_verify_pairs (tests/pairs_ref.py) on the CPU: that a listed
consecutive pair is the consecutive matcher's problem, that (a, b) and (b, a) are each other's transposed problem, that the draw
stream follows the list index and not the frames, every refusal of MP-1, and -- on the recognition scene of the place stage with
the oracle's intended-mode records -- that the two stages separate a true loop from a false one."""
import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import pairs_ref as pf
import place_ref as pr
import place_scene
import verify_ref as vr

W0, H0 = 64, 48


def test_a_listed_consecutive_pair_is_the_consecutive_matchers(numpy_ref):
    rng = np.random.default_rng(1)
    counts = np.array([40, 70, 0, 33, 500], np.uint32)  # the last raw counter exceeds the capacity
    cap = 64
    desc = [C.random_desc(rng, min(int(c), cap) + 5) for c in counts]  # five stale records behind every count
    pairs = [(f, f + 1) for f in range(4)]
    rows = pf.match_pairs(counts, desc, cap, pairs)
    for f, row in enumerate(rows):
        na, nb = min(int(counts[f]), cap), min(int(counts[f + 1]), cap)
        want = C.match_ref(desc[f][:na], desc[f + 1][:nb])
        assert row.tobytes() == want.tobytes() and len(row) == na
        idx, dist, second = numpy_ref.match(desc[f][:na], desc[f + 1][:nb])
        assert np.array_equal(row["index"], idx) and np.array_equal(row["distance"], dist) and np.array_equal(row["second"], second)


def test_backward_is_the_transposed_problem():
    """Frame b holds frame a's descriptors permuted, each with a few bits flipped: a's record i points at perm[i] and b's record
    perm[i] at i, at the same distance."""
    rng = np.random.default_rng(2)
    n = 90
    da = C.random_desc(rng, n)
    k = rng.integers(0, 20, n)
    perm = rng.permutation(n)
    db = np.zeros_like(da)
    db[perm] = np.stack([C.flip(da[i], int(k[i]), rng) for i in range(n)])
    counts = np.array([n, 7, n], np.uint32)
    fwd, bwd = pf.match_pairs(counts, [da, C.random_desc(rng, 7), db], 128, [(0, 2), (2, 0)])
    assert np.array_equal(fwd["index"], perm) and np.array_equal(fwd["distance"], k)
    assert np.array_equal(bwd["index"][perm], np.arange(n)) and np.array_equal(bwd["distance"][perm], k)
    assert np.all(fwd["second"] > 64) and np.all(bwd["second"] > 64)


@pytest.mark.parametrize("model", [pf.HOMOGRAPHY, pf.EPIPOLAR])
def test_the_draw_stream_follows_the_list_index(model):
    rng = np.random.default_rng(3)
    cor, desc, _ = C.correspondences(rng, 60, 15, W0, H0, shift=(3, -2), margin=4)
    filler = C.distinct_corners(rng, 10, W0, H0)
    counts = np.array([75, 10, 75], np.uint32)
    corners = [cor[0], filler, cor[1]]
    descs = [desc[0], C.random_desc(rng, 10), desc[1]]
    pairs = [(0, 2), (2, 0), (0, 1), (0, 2)]
    rows = pf.match_pairs(counts, descs, 128, pairs)
    out = pf.verify_pairs(counts, corners, rows, 128, pairs, W0, H0, model=model, hypotheses=64, seed=9)
    a, b = out[0][0], out[3][0]
    assert a["candidates"] == b["candidates"] == 75 and rows[0].tobytes() == rows[3].tobytes()
    sample = {pf.HOMOGRAPHY: vr.sample, pf.EPIPOLAR: er.sample}[model]
    J0, J3 = sample(9, 0, 75, 64)[0], sample(9, 3, 75, 64)[0]
    assert not np.array_equal(J0, J3)  # other draws at list position 3 than at 0, for the same two frames
    # position 3 is the verifier's pair 3 on frames (0, 2), whatever those frames are
    fn = {pf.HOMOGRAPHY: vr.verify_pair, pf.EPIPOLAR: er.verify_pair}[model]
    want, mask = fn(cor[0], cor[1], rows[3], W0, H0, 3, cap=128, hypotheses=64, seed=9)
    assert b.tobytes() == want.tobytes() and out[3][1].tobytes() == mask.tobytes()
    assert a["status"] in (vr.VERIFY_OK, vr.VERIFY_MINIMAL) and b["status"] in (vr.VERIFY_OK, vr.VERIFY_MINIMAL)
    assert a["inliers"] >= 55 and b["inliers"] >= 55
    assert out[2][0]["status"] == vr.VERIFY_FEW  # the filler


def test_every_refusal_of_the_list():
    B, n = 5, 4  # max_batch 5: P = 20; the batch holds 4 frames
    assert pf.capacity(B) == 20 and pf.PAIRS_PER_FRAME == pr.TOP_DEFAULT
    ok = [(0, 1), (3, 0), (1, 0), (0, 1), (2, 3)]  # consecutive, backward, duplicate
    assert pf.violation(ok, n, B) is None
    assert pf.violation([(0, 1)], n, B) is None and pf.violation([(0, 1)] * 20, n, B) is None
    assert pf.violation([], n, B) == "count" and pf.violation([(0, 1)] * 21, n, B) == "count"
    assert pf.violation(ok + [(4, 0)], n, B) == 5          # a query at the frame count
    assert pf.violation([(0, 4)] + ok, n, B) == 0          # a target at the frame count
    assert pf.violation(ok[:2] + [(2, 2)] + ok, n, B) == 2  # query == target
    assert pf.violation([(0, 1), (7, 7), (9, 0)], n, B) == 1  # the first of several
    assert pf.violation([(0xFFFFFFFF, 0)], n, B) == 0
    L = pf.as_list(ok)
    assert L.dtype == pf.FRAME_PAIR_DTYPE and L.itemsize == 8 and L["query"].tolist() == [0, 3, 1, 0, 2] and pf.violation(L, n, B) is None


def test_the_scene_separates_true_loops_from_false(oracle):
    """place_scene.REDUCED with the oracle's intended-mode records (FAST-9, NMS, capacity 256), both models at their defaults: every
    (revisit, twin) pair is OK or MINIMAL with more inliers than the same revisit against either filler and against the place
    stage's second candidate, and every filler pair is FEW or DEGENERATE."""
    S = place_scene.REDUCED
    frames, twin = place_scene.frames(oracle, **S)
    cap = S["cap"]
    totals, ocor, odesc = oracle.extract_intended_batch(frames, depth=2, max_features=cap, arc=9, nms=True)
    _, prow = pr.place(totals, odesc, cap, min_gap=S["min_gap"])
    fillers = list(range(S["places"], S["places"] + S["fillers"]))
    pairs, kind = [], []
    for f, g in twin.items():
        assert prow[f]["n"] >= 2 and prow[f]["best"][0]["frame"] == g
        pairs += [(f, g), (f, int(prow[f]["best"][1]["frame"]))] + [(f, x) for x in fillers]
        kind += ["twin", "second"] + ["filler"] * len(fillers)
    assert pf.violation(pairs, len(frames), len(frames)) is None
    rows = pf.match_pairs(totals, odesc, cap, pairs)
    for model in (pf.HOMOGRAPHY, pf.EPIPOLAR):
        out = pf.verify_pairs(totals, ocor, rows, cap, pairs, S["W"], S["H"], model=model)
        for i, ((q, t), k) in enumerate(zip(pairs, kind)):
            r = out[i][0]
            print("model %d  %2d -> %2d  %-6s candidates %3d inliers %3d status %d" % (model, q, t, k, r["candidates"], r["inliers"], r["status"]))
        check_scene_relations(pairs, kind, [o[0] for o in out])


def check_scene_relations(pairs, kind, records):
    """The three relations of the scene (tests/test_gpu_pairs.py asserts the same on the device's records)."""
    by_query = {}
    for (q, _), k, r in zip(pairs, kind, records):
        by_query.setdefault(q, {}).setdefault(k, []).append(r)
    assert by_query
    for q, d in by_query.items():
        (t,) = d["twin"]
        assert t["status"] in (vr.VERIFY_OK, vr.VERIFY_MINIMAL), (q, t)
        for other in d["second"] + d["filler"]:
            assert t["inliers"] > other["inliers"], (q, t, other)
        for f in d["filler"]:
            assert f["status"] in (vr.VERIFY_FEW, vr.VERIFY_DEGENERATE), (q, f)
