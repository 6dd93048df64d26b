"""The bridge stage on the GPU where tests/test_gpu_bridge.py's batches (twelve frames, gaps of three, one join per path) cannot show
an error (orb_bridge_consecutive): k_br_chain's chunks of 64 frames on a batch of 327 (a join read back from
the chunk before, a gap end as a chunk's first frame that joins through it, a gap across a boundary, calls that end on either side
of one), BR-1's hop limit at 16, 15 and 4 hops behind a pause of seventeen frames, two joins on one path, and BR-5's join on ratios
decided to the bit: 1 to 439 of them, equal ones, the lower median, values that differ in one byte with the rank in a lane's fourth
or first bin, the tolerance's and the permille rule's equality, min_shared, depths that give no ratio.  Every OrbBridgePose byte and
inlier byte against the restatement (tests/bridge_ref.py) fed with the device's own read-backs, through test_gpu_bridge.py's
helpers, and against what each construction implies (tests/bridge_cases.py; tests/test_bridge_cases_ref.py checks the layouts on
the CPU).  No record of any case holds a NaN."""
import numpy as np
import pytest

import bridge_cases as B
import bridge_ref as brr
import trajectory_cases as tc
from test_gpu_bridge import INTR, _check, _inputs, _program, _setup

pytestmark = pytest.mark.gpu

F = np.float32
COPIED, MOVED, FIXED, JOINED, UNFIXED = B.COPIED, B.MOVED, B.FIXED, B.JOINED, B.UNFIXED
CHAINED, START, LOST, ORIGIN = B.CHAINED, B.START, B.LOST, B.ORIGIN


def _trace(inputs, n, cap, **params):
    """The restatement's trace on the device's read-backs."""
    counts, corners, matches, points, frames, lms = inputs
    trace = {}
    brr.bridge(counts, corners, matches, points, frames[:n], lms, cap, n_frames=n, trace=trace, **INTR, **params)
    return trace


def _product(a, b):
    return F(F(a) * F(b)).tobytes()


@pytest.fixture(scope="module")
def long_run(tinyorb):
    """long_batch on a program of its own, behind the trajectory and landmarks calls: (prog, batch, inputs)."""
    b = B.long_batch()
    with _program(tinyorb, b["cap"], b["n"]) as prog:
        yield prog, b, _setup(prog, b, traj=B.LONG_TRAJ)


def test_chunks_of_the_chain(tinyorb, long_run):
    """327 frames: what the layout implies on either side of the boundaries at 64, 128, 192, 256 and 320, then calls that end at
    63, 64, 65, 66, 128 and 129 frames."""
    prog, b, inputs = long_run
    n, cap = b["n"], b["cap"]
    recs, _, _ = _check(prog, n, cap, inputs, **B.LONG)
    st, ts = recs["status"].tolist(), inputs[4]["status"].tolist()
    trace = _trace(inputs, n, cap, **B.LONG)
    gamma = {g: trace[g]["join"][1] for g in trace}
    # a JOINED frame in one chunk, MOVED frames of the next through it
    assert st[190] == JOINED and st[191:195] == [MOVED] * 4 and recs["root"][190:195].tolist() == [186] * 5
    assert (recs["gain"][191:195] == recs["gain"][190]).all() and recs["gain"][190] == gamma[190]
    # frame 64: a gap end with anchor 63 that joins through S_60
    assert ts[63:66] == [CHAINED, LOST, START] and st[60:69] == [JOINED] + [MOVED] * 3 + [JOINED] + [MOVED] * 4
    assert recs["anchor"][64] == 63 and recs["root"][56:69].tolist() == [56] * 13 and recs["gain"][60] == gamma[60]
    assert recs["gain"][64].tobytes() == _product(gamma[60], gamma[64]) and (recs["gain"][65:69] == recs["gain"][64]).all()
    # a gap of two frames across 128 behind anchor 127
    assert ts[127:131] == [CHAINED, LOST, LOST, START] and recs["anchor"][128:130].tolist() == [127, 127]
    assert st[124:133] == [JOINED] + [MOVED] * 3 + [FIXED, JOINED] + [MOVED] * 3 and recs["root"][120:133].tolist() == [120] * 13
    assert recs["gain"][129].tobytes() == _product(gamma[124], gamma[129])
    # a run's first frame as the last frame of a chunk and as the first of one
    for f in (255, 320):
        assert ts[f:f + 2] == [LOST, START] and recs["candidates"][f] > 0 and recs["inliers"][f] <= 6 and recs["root"][f + 1] == f
    for c in range(0, n - 20, B.CHUNK):
        assert set(st[c:c + B.CHUNK]) == {COPIED, MOVED, FIXED, JOINED, UNFIXED}, c
    for k in (63, 64, 65, 66, 128, 129):
        got, _, _ = _check(prog, k, cap, inputs, **B.LONG)
        assert got["status"][:k - 1].tolist() == st[:k - 1], k
        assert got["status"][k - 1] == (FIXED if k in (65, 129) else st[k - 1]), k  # a gap end that is the last frame cannot join
        assert k != 66 or (got[64].tobytes() == recs[64].tobytes() and got["status"][65] == MOVED)
        with pytest.raises(tinyorb.OrbError):
            prog.bridge_read(k, cap)  # the call before had k frames


def test_chunks_under_each_parameter_and_again(long_run):
    """The whole batch with window 1, 2 and 3, one hop and a second seed, then the first call's bytes again."""
    prog, b, inputs = long_run
    n, cap = b["n"], b["cap"]
    recs, _, blob = _check(prog, n, cap, inputs, **B.LONG)
    for kw in (dict(window=1), dict(window=2), dict(window=3), dict(seed=12345)):
        got, _, _ = _check(prog, n, cap, inputs, **B.LONG, **kw)
        assert got["anchor"].tolist() == recs["anchor"].tolist(), kw
        print(kw, "candidates", int(got["candidates"].sum()), "of", int(recs["candidates"].sum()))
    one, _, _ = _check(prog, n, cap, inputs, **B.LONG, max_hops=1)
    assert one["status"][128:131].tolist() == [FIXED, UNFIXED, COPIED] and one["fix"][129] == B.L_NOMAP and one["root"][130] == 129
    assert one["status"][64] == JOINED and one[64].tobytes() == recs[64].tobytes()
    assert _check(prog, n, cap, inputs, **B.LONG)[2] == blob  # a stale record, key, ratio or inlier byte of the calls between would show


def test_hops_at_the_limit(tinyorb):
    """A pause of seventeen frames: the frames within max_hops of the anchor are FIXED, the next is NOMAP."""
    b = B.hop_batch()
    n, cap = b["n"], b["cap"]
    with _program(tinyorb, cap, n) as prog:
        inputs = _setup(prog, b, traj=B.LONG_TRAJ)
        assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED] + [LOST] * 17 + [START, CHAINED, CHAINED]
        for hops in (16, 15, 4):
            recs, masks, _ = _check(prog, n, cap, inputs, **B.LONG, max_hops=hops)
            assert recs["status"].tolist() == [COPIED] * 4 + [FIXED] * hops + [UNFIXED] * (17 - hops) + [COPIED] * 3
            assert (recs["fix"][4:4 + hops] == B.L_OK).all() and (recs["fix"][4 + hops:21] == B.L_NOMAP).all() and (recs["anchor"][4:21] == 3).all()
            assert recs["root"].tolist() == [0] * (4 + hops) + list(range(4 + hops, 21)) + [20] * 3
            cand = recs["candidates"][4:4 + hops].astype(int)
            print("max_hops", hops, "candidates", cand.tolist())
            assert (np.diff(cand) < 0).all() and cand[-1] >= 100 and not recs["candidates"][4 + hops:].any() and not masks[4 + hops:].any()


def test_two_joins_on_one_path(tinyorb):
    """Frame 8 joins through S_4: sigma != 1, a JOINED frame whose own segment is MOVED, the compose through S before a join."""
    b = B.double_batch()
    n, cap = b["n"], b["cap"]
    with _program(tinyorb, cap, n) as prog:
        inputs = _setup(prog, b, traj=B.LONG_TRAJ)
        recs, _, blob = _check(prog, n, cap, inputs, **B.LONG)
        trace = _trace(inputs, n, cap, **B.LONG)
        g4, g8 = trace[4]["join"][1], trace[8]["join"][1]
        assert recs["status"].tolist() == [COPIED] * 4 + [JOINED] + [MOVED] * 3 + [JOINED] + [MOVED] * 4 and not recs["root"].any()
        assert g4 != 1 and g8 != 1 and recs["gain"][4] == g4 and recs["gain"][8].tobytes() == _product(g4, g8)
        assert (recs["gain"][5:8] == g4).all() and (recs["gain"][9:] == recs["gain"][8]).all() and recs["anchor"][8] == 7
        assert recs["scale"][10].tobytes() == _product(recs["gain"][8], inputs[4]["scale"][10])
        spread, _, _ = _check(prog, n, cap, inputs, **B.LONG, scale_tolerance=1e-5)  # the first join refused: the second roots behind the first gap
        assert spread["status"].tolist() == [COPIED] * 4 + [FIXED] + [COPIED] * 3 + [FIXED] + [COPIED] * 4
        assert spread["root"].tolist() == [0] * 5 + [4] * 4 + [8] * 4
        none, _, _ = _check(prog, n, cap, inputs, **B.LONG, max_reproj_px=1e-6)
        assert none["status"].tolist() == [COPIED] * 4 + [UNFIXED] + [COPIED] * 3 + [UNFIXED] + [COPIED] * 4
        assert none["root"].tolist() == [0] * 4 + [4] * 4 + [8] * 5
        assert _check(prog, n, cap, inputs, **B.LONG)[2] == blob


def test_join_edges(tinyorb):
    """BR-5 on ratios decided to the bit (bridge_cases.edge_cases): capacity 1100, 493 candidates, points[4] rewritten per case, the
    trajectory and landmarks calls on the device again behind each."""
    b = B.edge_batch()
    n, cap, g = b["n"], b["cap"], B.EDGE_G
    cases = B.edge_cases(b)
    with _program(tinyorb, cap, n) as prog:
        _setup(prog, b, traj=B.EDGE_TRAJ)
        for c in cases:
            tc.inject_pose(prog, points_=c["b"]["points"])
            prog.trajectory_consecutive(n, **B.EDGE_TRAJ)
            prog.landmarks_consecutive(n, **INTR)
            inputs = _inputs(prog, n, cap)
            assert inputs[4]["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, LOST, START], c["name"]
            assert inputs[3][g]["z"].tobytes() == c["b"]["points"]["z"][g].tobytes()  # the case's depths, NaN included, are what the call reads
            recs, _, _ = _check(prog, n, cap, inputs, **c["params"])
            rec = recs[g]
            print(c["name"], "status", rec["status"], "shared", rec["shared"], "consistent", rec["consistent"], "gain", rec["gain"])
            assert rec["candidates"] == 493 and rec["fix"] == B.L_OK and rec["status"] in (FIXED, JOINED)
            assert recs["status"][5] == (MOVED if rec["status"] == JOINED else COPIED)
            B.check_expect(c, rec)
