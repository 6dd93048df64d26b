"""The labelled cases of tests/epipolar_cases.py on the GPU: every fixed entry m of the epipolar refit (EP-5) with status OK, the
refit's partial sums at 255, 256 and 257 candidates, ORB_VERIFY_MINIMAL by the 15/16 rule and by a failed solve, and M = 8 and 9
with invalid hypotheses beside valid ones.  tests/test_epipolar_cases_ref.py shows on the CPU that the restatement takes these
branches; here every record and inlier byte of the device equals the restatement's, with no tolerance, so the device took them too.

One blank 640 x 480 program of 34 frames at capacity 1024, case i injected into frames 2 i and 2 i + 1.  A call's parameters hold for
the whole batch: each of the four parameter sets is one call over every pair, compared pair by pair, and a case's label (status,
candidates, inliers, hypothesis) is asserted under its own set only."""
import pytest

import constructed as C
import epipolar_cases as ec
import epipolar_ref as er
import pairs_ref as pf
from test_gpu_epipolar import _check_parity
from test_gpu_pairs import _check_rows, _check_verify, _program

pytestmark = pytest.mark.gpu

_LABEL = ("status", "candidates", "inliers", "hypothesis")


def _blank(tinyorb, counts):
    return _program(tinyorb, ec.CAP, len(counts), ec.W, ec.H)


def _check_labels(name, recs, step):
    """recs[step * i] is case i's record: under parameter set `name`, the label of every case of that set."""
    for i, c in enumerate(ec.CASES):
        if c["params"] == name:
            got = {k: int(recs[step * i][k]) for k in _LABEL}
            print("%-6s %-14s m %d  %s" % (name, c["name"], c["label"]["m"], got))
            assert got == {k: c["label"][k] for k in _LABEL}, (name, c["name"], got, c["label"])
            assert recs[step * i]["h"][c["label"]["pixel_m"]] == 1.0


def test_verify_epipolar_on_the_cases(tinyorb):
    """orb_verify_epipolar: case i is pair 2 i; the pairs between two cases have no candidate."""
    counts, corners, desc = ec.batch()
    with _blank(tinyorb, counts) as prog:
        C.inject(prog, counts, corners, desc)
        prog.match_consecutive(len(counts))
        for name, params in ec.PARAMS.items():
            recs = _check_parity(prog, len(counts), ec.W, ec.H, ec.CAP, **params)
            _check_labels(name, recs, 2)
            assert all(r["status"] == er.VERIFY_FEW and r["candidates"] == 0 for r in recs[1::2]), name
            for i, c in enumerate(ec.CASES):  # the record the CPU census traced, not merely one the restatement gives on device rows
                if c["params"] == name:
                    assert recs[2 * i].tobytes() == ec.traced(i)[0].tobytes(), c["name"]


def test_verify_pairs_on_the_cases(tinyorb):
    """orb_match_pairs and orb_verify_pairs(EPIPOLAR) with every case listed forward (entry 2 i, the same draw stream as above) and
    backward (entry 2 i + 1: the transposed F, so 1 <-> 3, 2 <-> 6, 5 <-> 7); the failed-solve parameters under HOMOGRAPHY too, where
    every listed pair ends MINIMAL without an inlier."""
    counts, corners, desc = ec.batch()
    pairs = ec.pairs()
    with _blank(tinyorb, counts) as prog:
        C.inject(prog, counts, corners, desc)
        rows =_check_rows(prog, counts, desc, ec.CAP, pairs)
        for name, params in ec.PARAMS.items():
            recs = _check_verify(prog, counts, corners, rows, ec.CAP, pairs, ec.W, ec.H, pf.EPIPOLAR, **params)
            _check_labels(name, recs, 2)
            for i, c in enumerate(ec.CASES):
                if c["params"] == name:
                    assert recs[2 * i + 1].tobytes() == ec.traced(i, backward=True)[0].tobytes(), c["name"]
        recs = _check_verify(prog, counts, corners, rows, ec.CAP, pairs, ec.W, ec.H, pf.HOMOGRAPHY, **ec.PARAMS["solve"])
        assert all(r["status"] == er.VERIFY_MINIMAL and r["inliers"] == 0 and r["candidates"] >= 8 for r in recs), recs
