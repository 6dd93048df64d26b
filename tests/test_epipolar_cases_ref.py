"""The census of tests/epipolar_cases.py on the CPU restatement (tests/epipolar_ref.py with its trace): every case's stated label is
what the restatement gives at the case's own pair and parameters, and the list as a whole reaches every branch it was built for.
tests/test_gpu_epipolar_cases.py replays the same list on the device, so what is shown here is what the device is held to there.

What the list reaches:
    the fixed entry m of EP-5: each of 0 .. 8 with status OK (cases m0 .. m8), and again transposed in the backward listings;
    the refit's partial sums at 255, 256 and 257 candidates with m = 2;
    ORB_VERIFY_MINIMAL by the 15/16 rule (fit, 16 n_fit < 15 n_min) and by a failed solve (no fit, no inlier);
    M = 8 and M = 9 with valid and invalid hypotheses in one 64-hypothesis workgroup, M = 8 decided by the lowest-h tie rule at h = 2;
    EP-3's unpivoted column: 0, 2, 3 and 7 among the cases m0 .. m8, 1, 4 and 6 among the others;
    EP-6's normalising index: 8, and 2 for the pure translation.

The whole module takes 2.2 s on one CPU core (the scenes are built once per process and every case is traced once).
"""
import numpy as np
import pytest

import epipolar_cases as ec
import epipolar_ref as er
import pairs_ref as pf
import verify_ref as vr

NAMES = [c["name"] for c in ec.CASES]
_traced = {}


def _trace(i, backward=False):
    if (i, backward) not in _traced:
        rec, mask, trace = ec.traced(i, backward)
        _traced[i, backward] = (rec, mask, ec.label_of(rec, trace))
    return _traced[i, backward]


@pytest.mark.parametrize("name", NAMES)
def test_label(name):
    """The stated label, key by key, and what its group promises."""
    i = NAMES.index(name)
    c = ec.CASES[i]
    want = {k: v for k, v in c["label"].items() if k != "m_back"}
    assert {"status", "m", "fit", "candidates", "inliers", "hypothesis", "pixel_m", "unpivoted", "n_min", "n_fit"} <= set(want)
    rec, mask, got = _trace(i)
    assert {k: got[k] for k in want} == want, (name, got)
    assert int(mask.sum()) == want["inliers"] and len(mask) == ec.CAP
    assert rec["h"][got["pixel_m"]] == 1.0 and np.abs(rec["h"]).max() == 1.0
    if c["params"] == "ok":
        assert want["status"] == ec.OK and want["fit"] and want["candidates"] > 8 * 8
    if c["count"] is not None:
        assert want["candidates"] == c["count"]
    if c["params"] == "rule":
        assert want["status"] == ec.MINIMAL and want["fit"] and want["n_min"] > 0 and 16 * want["n_fit"] < 15 * want["n_min"]
        assert want["inliers"] == want["n_min"]
    if c["params"] == "solve":
        assert want["status"] == ec.MINIMAL and not want["fit"] and want["n_min"] == want["inliers"] == 0
        p = vr.defaults(**ec.PARAMS["solve"])
        assert p["inlier_px"] > 0 and (p["inlier_px"] * vr.normalise(ec.W, ec.H)[2]) ** 2 == 0  # t2 underflows
        assert got["valid"] == p["hypotheses"] and want["hypothesis"] == 0  # every hypothesis ties at no inlier: the first wins
    if c["params"] == "tiny":
        p = ec.PARAMS["tiny"]
        _, ok = er.sample(p["seed"], 2 * i, want["candidates"], p["hypotheses"])
        assert want["sampled"] == want["valid"] == int(ok.sum())
        assert 0 < ok[:64].sum() < 64  # valid and invalid lanes in the first workgroup
        if want["candidates"] == 8:  # one set of eight candidates: every valid hypothesis has all 8 as inliers
            assert want["n_min"] == 8 and want["hypothesis"] == int(np.argmax(ok)) > 0


def test_census():
    labels = [c["label"] for c in ec.CASES]
    ok_m = {l["m"] for l in labels if l["status"] == ec.OK}
    assert ok_m == set(range(9))
    assert [c["label"]["m"] for c in ec.CASES[:9]] == list(range(9)) and all(c["params"] == "ok" for c in ec.CASES[:9])
    minimal = [l for l in labels if l["status"] == ec.MINIMAL]
    assert any(l["fit"] for l in minimal) and any(not l["fit"] for l in minimal)
    assert {l["unpivoted"] for l in labels[:9]} == {0, 2, 3, 7}
    assert {l["unpivoted"] for l in labels} == {0, 1, 2, 3, 4, 6, 7}
    assert {l["pixel_m"] for l in labels} == {2, 8}
    bound = {l["candidates"]: l["m"] for l in labels if l["candidates"] in (255, 256, 257)}
    assert bound == {255: 2, 256: 2, 257: 2}  # one m outside {3, 5}, either side of one pass over the 256 partial sums
    assert {c["label"]["candidates"] for c in ec.CASES if c["params"] == "tiny"} == {8, 9}
    assert len(ec.CASES) <= 17 and max(l["candidates"] for l in labels) <= ec.CAP
    assert set(c["params"] for c in ec.CASES) == set(ec.PARAMS)


def test_backward_listings_transpose_m():
    """The backward listing of a case whose motion decides m (m_back stated) fixes the transposed entry, with status OK, at list
    entry 2 i + 1; between them the two listings show each of 1 <-> 3, 2 <-> 6 and 5 <-> 7 in both directions."""
    seen = set()
    for i, c in enumerate(ec.CASES):
        if "m_back" not in c["label"]:
            continue
        rec, _, got = _trace(i, backward=True)
        m = c["label"]["m"]
        assert c["label"]["m_back"] == ec.TRANSPOSED[m] == got["m"] and rec["status"] == ec.OK, (c["name"], got)
        assert rec["candidates"] == c["label"]["candidates"]
        seen.add((m, got["m"]))
    assert {(1, 3), (3, 1), (2, 6), (6, 2), (5, 7), (7, 5), (0, 0), (4, 4), (8, 8)} <= seen
    assert all("m_back" in c["label"] for c in ec.CASES[:9])


def test_the_pairs_restatement_meets_the_same_cases():
    """orb_verify_pairs' restatement on `pairs()`: entry 2 i is case i at pair 2 i, byte for byte, under the case's parameters; and
    the failed-solve parameters end every pair that has a sample's worth of candidates in MINIMAL without an inlier, for the
    homography model as for the epipolar one."""
    counts, corners, desc = ec.batch()
    pairs = ec.pairs()
    assert len(counts) == 2 * len(ec.CASES) and len(pairs) == len(counts) <= pf.capacity(len(counts))
    rows = pf.match_pairs(counts, desc, ec.CAP, pairs)
    between = [(f, f + 1) for f in range(1, len(counts) - 1, 2)]  # the consecutive pairs between two cases: no candidate
    for (q, t), row in zip(between, pf.match_pairs(counts, desc, ec.CAP, between)):
        assert not len(vr.candidates(row, int(counts[t]), 64, 0.8)), (q, t)
    for name, params in ec.PARAMS.items():
        out = pf.verify_pairs(counts, corners, rows, ec.CAP, pairs, ec.W, ec.H, model=pf.EPIPOLAR, **params)
        for i, c in enumerate(ec.CASES):
            if c["params"] == name:
                rec, mask, _ = _trace(i)
                assert out[2 * i][0].tobytes() == rec.tobytes() and out[2 * i][1].tobytes() == mask.tobytes(), c["name"]
                rec, mask, _ = _trace(i, backward=True)
                assert out[2 * i + 1][0].tobytes() == rec.tobytes() and out[2 * i + 1][1].tobytes() == mask.tobytes(), c["name"]
        if name == "solve":
            hom = pf.verify_pairs(counts, corners, rows, ec.CAP, pairs, ec.W, ec.H, model=pf.HOMOGRAPHY, **params)
            for few, recs in ((8, out), (4, hom)):
                assert all(r["candidates"] >= few and r["status"] == ec.MINIMAL and r["inliers"] == 0 and not m.any() for r, m in recs)
