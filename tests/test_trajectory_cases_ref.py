"""The hand-built cases of tests/trajectory_cases.py on the CPU restatement (tests/trajectory_ref.py): every case alone and packed
with the others, with the outcome its construction implies; the census of the paths the selection cases take through TJ-3's radix
select, from select_trace; the two 260-frame chains against their plans.  tests/test_gpu_trajectory_cases.py runs the same batches
on the device."""
import numpy as np
import pytest

import trajectory_cases as tc
import trajectory_ref as tr

F, U = np.float32, np.uint32
CAPS = (64, 1100)


@pytest.mark.parametrize("cap", CAPS)
def test_every_joint_case_alone_and_packed(cap):
    cases = tc.joint_cases(cap)
    assert len(cases) > 90 and len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        fr, _ = tc.run_case(c, **c["params"])
        assert fr["status"].tolist()[:2] == [tc.ORIGIN, tc.START]
        tc.check_expect(c, fr[2])
    b = tc.pack(cases, cap)
    assert b["n"] == 3 * len(cases) + 1
    # the scatter: the last slot, and at capacity 1100 both sides of 1024, hold GOOD points; arbitrary bits elsewhere
    good = (b["points"]["flags"] & tc.GOOD) != 0
    assert good[:, cap - 1].any() and (cap < 1024 or (good[:, 1023].any() and good[:, 1024].any()))
    sets = tc.param_sets(cases)
    assert {} in sets and len(sets) >= 10
    for ps in sets:
        fr, world = tc.reference(b, **ps)
        assert not tc.stored_nans(b, fr, world), (ps, tc.stored_nans(b, fr, world))
        for k, (c, f) in enumerate(zip(cases, b["joint"])):
            assert fr["status"][f - 1] == tc.START and fr["status"][f + 1] == tc.LOST and fr["origin"][f + 1] == f + 1
            if c["params"] == ps:
                tc.check_expect(c, fr[f])
            # the map: pair 3 k copied whole (arbitrary bits included), pair 3 k + 1 transformed or copied, pair 3 k + 2 zeros
            assert world[f - 2].tobytes() == b["points"][f - 2].tobytes() and not world[f].tobytes().strip(b"\0")
            if fr["status"][f] != tc.CHAINED:
                assert world[f - 1].tobytes() == b["points"][f - 1].tobytes()
            else:
                src = b["points"][f - 1]
                assert not world[f - 1][(src["flags"] & tc.GOOD) == 0].tobytes().strip(b"\0")
                assert (world[f - 1]["flags"] == np.where(src["flags"] & tc.GOOD, src["flags"], 0)).all()


def test_the_order_of_the_sum_shows():
    """The random-pose cases tell ((r0 x + r1 y) + r2 z) + t2 from two other orders of the same sum, and from a float64 sum rounded
    once: each gives other bits for some ratio."""
    other = {"right": 0, "t first": 0, "float64": 0}
    for c in tc.ratio_cases():
        if not c["name"].startswith("random pose"):
            continue
        X, r, t2 = c["pa"], c["pose_a"]["r"], c["pose_a"]["t"][2]
        want = (r[6] * X["x"] + r[7] * X["y"]) + r[8] * X["z"] + t2
        other["right"] += int((want != r[6] * X["x"] + (r[7] * X["y"] + r[8] * X["z"]) + t2).sum())
        other["t first"] += int((want != (t2 + r[6] * X["x"]) + r[7] * X["y"] + r[8] * X["z"]).sum())
        wide = (np.float64(r[6]) * X["x"] + np.float64(r[7]) * X["y"] + np.float64(r[8]) * X["z"] + np.float64(t2)).astype(F)
        other["float64"] += int((want != wide).sum())
    print(other)
    assert min(other.values()) >= 20


def test_selection_census():
    """What the selection cases reach, by select_trace: every (pass, byte mod 4) with lower byte values of the same group of four
    populated (the lane's `past` loop), byte values 0 and 255 (lanes 0 and 63) in passes 1..3 and 0 and 0x7f in pass 0, a first pass
    with two populated byte values and the rank in the second, a rank carried on above 0 from every pass, duplicates at the median,
    m = 1, 2 and the capacity."""
    for cap in CAPS:
        cases = tc.selection_cases(cap)
        cells, ends, carried, populated_first, dup, ms = set(), set(), set(), [], 0, set()
        for c in cases:
            rb = tc.case_ratio_bits(c, **c["params"])
            assert len(rb) == c["expect"]["shared"]
            t = tc.select_trace(rb)
            assert t["g"] == c["expect"]["step_bits"], c["name"]
            ms.add(len(rb))
            dup = max(dup, t["duplicates"] if len(set(rb.tolist())) > 1 else 0)
            for p, q in enumerate(t["passes"]):
                if q["below"] == (q["bin"] & 3) and q["populated"] > 1:
                    cells.add((p, q["bin"] & 3))
                if q["bin"] in (0, 255, 0x7F):
                    ends.add((p, q["bin"]))
                if q["carried"] > 0:
                    carried.add(p)
            populated_first.append((t["passes"][0]["populated"], t["passes"][0]["carried"], t["passes"][0]["below"]))
        assert cells == {(p, q) for p in range(4) for q in range(4)}, sorted(cells)
        assert ends >= {(0, 0), (0, 0x7F)} | {(p, b) for p in (1, 2, 3) for b in (0, 255)}, sorted(ends)
        assert carried == {0, 1, 2, 3}
        assert (2, 1, 0) in populated_first  # straddling 2.0: byte values 0x3f and 0x40 (two lanes), the rank in the second, 1 carried
        assert dup >= 4 and {1, 2, cap} <= ms
        print(cap, len(cases), "cases; cells", len(cells), "ends", sorted(ends), "largest m", max(ms))


def test_select_trace_is_the_sort():
    rng = np.random.default_rng(5)
    for _ in range(200):
        v = rng.integers(1, tc.FLT_MAX_BITS + 1, int(rng.integers(1, 40))).astype(U)
        if rng.integers(0, 2):
            v &= U(0xFFFF00FF) if rng.integers(0, 2) else U(0x3F8000FF)  # shared bytes, duplicates
            v |= U(1)
        t = tc.select_trace(v)
        assert t["g"] == np.sort(v)[(len(v) - 1) // 2] and t["duplicates"] == int((v == U(t["g"])).sum())
        assert t["passes"][0]["rank"] == (len(v) - 1) // 2 and all(q["carried"] <= q["rank"] for q in t["passes"])


def test_chains_follow_their_plans():
    b, plan, notes = tc.chain_runs()
    fr, world = tc.reference(b)
    assert b["n"] == tc.CHAIN_FRAMES and fr["status"].tolist() == plan
    assert not tc.stored_nans(b, fr, world)
    for edge in (64, 128, 192, 256):  # a CHAINED run across every edge of the 64-frame chunks
        assert (fr["status"][edge - 3:edge + 4] == tc.CHAINED).all() and len(set(fr["origin"][edge - 3:edge + 4].tolist())) == 1
    assert fr["scale"][notes["scale inf"]] == np.inf and fr["scale"][notes["scale inf"] - 1] > F(1e30)
    assert np.isinf(world[notes["scale inf"] - 1]["x"][:12]).all()
    s0 = notes["scale 0"]
    assert fr["scale"][s0] == 0 and 0 < fr["scale"][s0 - 1] < F(1.2e-38) and fr["status"][s0 + 1] == tc.CHAINED and fr["scale"][s0 + 1] == 0
    assert not fr["r"][notes["det 0"]].any() and not fr["r"][notes["det 0"] + 1].any()
    for name in ("det < 0", "det not finite"):  # the composition itself, no polar step
        f = notes[name]
        M = [F(v) for v in tr.compose([F(v) for v in b["poses"][f - 1]["r"]], [F(0)] * 3, [F(v) for v in fr["r"][f - 1]], [F(0)] * 3, F(0))[0]]
        P, R1 = b["poses"][f - 1]["r"].reshape(3, 3), fr["r"][f - 1].reshape(3, 3)
        raw = np.array([[(P[r, 0] * R1[0, c] + P[r, 1] * R1[1, c]) + P[r, 2] * R1[2, c] for c in range(3)] for r in range(3)], F)
        assert fr["r"][f].tobytes() == raw.tobytes() == np.array(M, F).tobytes(), name
    assert np.linalg.det(fr["r"][notes["det < 0"]].astype(np.float64).reshape(3, 3)) < -0.99
    assert fr["status"][notes["det < 0"] + 1] == tc.CHAINED
    assert sorted(set(b["poses"]["status"].tolist())) == [0, 1, 2, 3, 4, 5, 0x80000000, 0xFFFFFFFF]
    b, plan = tc.chain_edges()
    fr, world = tc.reference(b)
    assert fr["status"].tolist() == plan and not tc.stored_nans(b, fr, world)
    assert [plan[f] for f in (64, 65, 128, 129, 192, 193, 194, 256, 257, 258)] == \
        [tc.LOST, tc.START, tc.START, tc.LOST, tc.FEW, tc.SPREAD, tc.CHAINED, tc.SPREAD, tc.FEW, tc.CHAINED]
    assert fr["shared"][192] == 3 and fr["shared"][193] == 12 and fr["consistent"][193] < 6
    # the map: a transformed row zeroes what is not GOOD and keeps the flags; a LOST frame's pair and the last row are zeros
    src = b["points"][100]
    assert fr["status"][101] == tc.CHAINED and not world[100][(src["flags"] & tc.GOOD) == 0].tobytes().strip(b"\0")
    assert world[100]["flags"][63] == tc.GOOD | tc.PAR and world[100]["x"][:12].any()
    assert not world[63].tobytes().strip(b"\0") and not world[259].tobytes().strip(b"\0")
    assert world[64].tobytes() == b["points"][64].tobytes() and np.isnan(world[64]["x"][42])  # copied whole, NaN payloads included
