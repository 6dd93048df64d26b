"""The hand-built cases of tests/landmark_cases.py (`cases`) on the CPU restatement (tests/landmark_ref.py): every call of every case
through `run_call`, then the outcome the case's construction implies.  tests/test_gpu_landmark_cases.py runs the same calls on the
device and the same `expect` on the device's records; this file is what proves the expectations themselves.  DESIGN.md section 22
lists which case fails under which one-line change of the restatement."""
import numpy as np

import landmark_cases as L
import verify_ref as vr
from tinyslam_amd import orb

F, U = np.float32, np.uint32
GOOD = orb.ORB_POINT_GOOD


def test_every_case_on_the_restatement():
    cases = L.cases()
    assert len(cases) == 30 and len({c["name"] for c in cases}) == len(cases)
    assert sorted({c["cap"] for c in cases}) == [L.SMALL, 64, 256, 257, 1100]
    checked = calls = 0
    for c in cases:
        res = [L.run_call(k) for k in c["calls"]]
        for k, (out, rows) in zip(c["calls"], res):
            # LM-6 whatever the case: no byte that is not finite, the rows count the records, nothing at or above the stored counts
            assert all(np.isfinite(out[x]).all() for x in "xyz"), c["name"]
            assert rows[["landmarks", "good", "longest"]].tolist() == L.rows_from(out, rows["origin"])[["landmarks", "good", "longest"]].tolist(), c["name"]
            for p in range(k["n_frames"] - 1):
                assert L.is_zero(out[p][min(int(k["batch"]["counts"][p]), c["cap"]):]), (c["name"], p)
            calls += 1
        c["expect"](res)
        checked += 1
    assert checked == len(cases)
    print("%d cases, %d calls" % (checked, calls))


def test_every_injected_index_is_guarded():
    """What the device test writes over the stages' buffers: every keypoint inside a 64 x 48 frame at level 0, and every match index
    either below the next frame's stored count or one that LM-3's `j < n_q` turns away before any row is read with it (`ORB_MATCH_NONE`,
    the count itself, the count + 1: all at most the capacity + 1, none used as an index)."""
    for c in L.cases():
        for k in c["calls"]:
            b = k["batch"]
            nq = np.minimum(b["counts"], b["cap"])
            for f in range(b["n"]):
                u, v = vr.level0(b["corners"][f][:nq[f]])
                assert len(b["corners"][f]) == b["cap"] and (u >= 0).all() and (u < 64).all() and (v >= 0).all() and (v < 48).all(), c["name"]
            for f in range(b["n"] - 1):
                j = b["matches"]["index"][f].astype(np.int64)
                assert ((j < nq[f + 1]) | (j == orb.ORB_MATCH_NONE) | ((j >= nq[f + 1]) & (j <= b["cap"] + 1))).all(), c["name"]
            assert b["matches"].shape == b["points"].shape == (b["n"] - 1, b["cap"]) and len(k["frames"]) == b["n"] <= 6


def test_rail_octaves():
    """A landmark keeps one octave in all its views, its level-0 keypoint moves by the rail's whole-pixel shift, and the draws of
    octaves = 0 are the ones the other tests use."""
    n, K = 6, 40
    b, plain = L.rail(n, K, octaves=2, v_hi=L.V_HI), L.rail(n, K, v_hi=L.V_HI)
    s, o = b["slots"], b["octave"]
    assert np.bincount(o, minlength=3).min() >= 5 and all(np.array_equal(a, c) for a, c in zip(s, plain["slots"]))
    shift = (64.0 * L.RAIL_BASE / b["cloud"][:, 2])
    assert set(shift.tolist()) == {2.0, 4.0} and (o[shift == 2.0] <= 1).all()
    u0, v0 = vr.level0(b["corners"][0][s[0]])
    assert np.array_equal(u0, ((b["corners"][0]["x"][s[0]] << o) + ((1 << o) - 1) / 2.0).astype(F))
    for f in range(n):
        c = b["corners"][f][s[f]]
        u, v = vr.level0(c)
        assert np.array_equal(c["octave"], o) and np.array_equal(u, u0 - F(f) * shift.astype(F)) and np.array_equal(v, v0)
        assert np.array_equal(b["cloud"][:, 0], (u0.astype(np.float64) - 32.0) * b["cloud"][:, 2] / 64.0)
    assert not plain["octave"].any() and np.array_equal(plain["corners"][3]["x"], L.rail(n, K, v_hi=L.V_HI)["corners"][3]["x"])
    # without the octave the same records are other rays, which meet elsewhere: no landmark of octave 1 or 2 is near its point
    flat = L.copy_batch(b)
    for c in flat["corners"]:
        c["octave"] = 0
    out, _ = L.run(flat)
    at = np.array([L.near(out[0][s[0][l]], b["cloud"][l]) for l in range(K)])
    assert at[o == 0].all() and not at[o > 0].any()


def test_the_last_bit_of_lm5():
    """smallest_good's two values are neighbours in binary32 and the landmark flips between them, with r2 formed in binary32."""
    b = L.rail(3, 4, cap=L.SMALL, v_hi=L.V_HI)
    slot = b["slots"][0][1]
    b["corners"][1]["y"][b["slots"][1][1]] += 6
    below, at = L.smallest_good(b, 0, slot)
    assert int(F(at).view(U)) - int(F(below).view(U)) == 1 and F(below) * F(below) < F(at) * F(at)
    lo, hi = L.run(b, max_reproj_px=below)[0][0][slot], L.run(b, max_reproj_px=at)[0][0][slot]
    assert (lo["flags"], hi["flags"], hi["inliers"]) == (0, GOOD | orb.ORB_POINT_PARALLAX, 3) and lo["inliers"] < 3
    assert F(1e-30) * F(1e-30) == 0  # the exact case's r2
