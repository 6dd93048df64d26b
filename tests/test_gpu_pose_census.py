"""orb_pose_consecutive through every branch of RP-2..RP-6 on the GPU: the scenes and intrinsics of
tests/pose_census.py, every OrbPairPose and OrbPoint byte against the CPU restatement (tests/pose_ref.py) fed with the device's own
counts, corners, match records and epipolar records.  No tolerance anywhere.

The kernels take F from the device's epipolar record, so the branches are reached through the intrinsics (E = K^T F K): the same
verified F under other fx, fy, cx, cy gives every row of T, every winner, one or no valid rotation, an n that is 0 or not finite, and
subnormal intermediates.  Not asked for: RP-3's `best <= 0`, which no finite input reaches (after RP-2 the squares of E sum to 2, so
trace T = 1 and the largest diagonal entry is at least 1/3 up to rounding)."""
import numpy as np
import pytest

import constructed as C
import pose_census as pc
import pose_ref as pr
from test_gpu_pose import H0, W0, _check, _inject_scenes, _inputs, _program

pytestmark = pytest.mark.gpu

assert (W0, H0) == (pc.W, pc.H)


def _zeros(rec, pts):
    """RP-7's record of zeros and no point."""
    return (not rec["r"].any() and not rec["t"].any() and rec["inliers"] == rec["good"] == rec["second"] == 0 and
            not pts.tobytes().strip(b"\0"))


def _verifier_differences(inputs, scenes, cap):
    """The pairs whose device match records, epipolar record or inlier bytes differ from the restatements'."""
    corners, matches, epi = inputs
    _, rmatches, repi = pc.cpu_inputs(scenes, cap)
    return [f for f in range(len(epi)) if matches[f].tobytes() != rmatches[f].tobytes() or epi[f][0].tobytes() != repi[f][0].tobytes() or
            np.asarray(epi[f][1]).tobytes() != repi[f][1].tobytes()]


def test_every_branch_at_capacity_64(tinyorb):
    """SCENES in one batch (scene i in frames 2i and 2i + 1), one pose call per entry of SWEEP in the committed order on the same
    program, every pair's record and all 64 points against the restatement.  A pair that the verifier gave a model and this entry
    leaves without a record had a written record under the entry before (pose_census.check_census asserts the order), so a stale
    record, stale points or stale counters would show; its zeros are asserted.  Then the census of the device's own inputs must
    reach what the CPU census reaches."""
    cap = 64
    scenes = [pc.build_scene(m, s) for m, s in pc.SCENES]
    with _program(tinyorb, W0, H0, cap, 2 * len(scenes)) as prog:
        B = _inject_scenes(prog, scenes, cap)
        prog.match_consecutive(B)
        prog.verify_epipolar(B, inlier_px=pc.INLIER_PX)
        inputs = _inputs(prog, B, cap)
        model = [int(e[0]["status"]) in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL) for e in inputs[2]]
        before, cleared = None, 0
        for k, intr in enumerate(pc.SWEEP):
            res = _check(prog, B, cap, inputs, intr)
            for f, (rec, pts) in enumerate(res):
                if rec["status"] == tinyorb.ORB_POSE_NOMODEL:
                    assert _zeros(rec, pts), (k, f, rec)
                    if model[f]:
                        assert before[f]["status"] != tinyorb.ORB_POSE_NOMODEL and before[f]["r"].any(), (k, f, before[f])
                        cleared += 1
                else:
                    assert rec["inliers"] == int((np.asarray(inputs[2][f][1]) == 1).sum()) >= pr.MIN_INLIERS, (k, f, rec)
            before = [r for r, _ in res]
        assert cleared > 100  # records of zeros over a pair's written record (the CPU census: 494 of them)
        rows = pc.census(inputs)
        print("\n" + pc.table(rows))
        try:
            pc.check_census(rows)
        except AssertionError as e:
            raise AssertionError("the device's inputs do not reach the census (%s); the pairs whose match or epipolar records differ "
                                 "from the restatements': %s" % (e, _verifier_differences(inputs, scenes, cap) or "none")) from e
        assert not _verifier_differences(inputs, scenes, cap)


def test_few_by_inlier_count(tinyorb):
    """RP-6's first rule with a valid model: after an OK call the query frame's raw counter alone is overwritten so that exactly 9, 7,
    8 and 0 of the pair's inlier bytes lie below it (7 after a written record).  0 and 7: FEW, a record of zeros, no point.  8 and
    9: a written record with the restatement's status.  The restatement gets the query corners and matches cut to the new count;
    both kernels must leave out the inliers at i >= n_q."""
    cap = 64
    scene = pc.build_scene(*pc.SCENES[4])  # forward
    with _program(tinyorb, W0, H0, cap, 2) as prog:
        _inject_scenes(prog, [scene], cap)
        prog.match_consecutive(2)
        prog.verify_epipolar(2, inlier_px=pc.INLIER_PX)
        corners, matches, epi = _inputs(prog, 2, cap)
        full = _check(prog, 2, cap, (corners, matches, epi), pc.DEFAULT)[0][0]
        assert full["status"] == tinyorb.ORB_POSE_OK
        inl = np.nonzero(np.asarray(epi[0][1]) == 1)[0]
        assert len(inl) == full["inliers"] > 9
        counts = prog.batch_counts(2)
        for below in (9, 7, 8, 0):
            nq = int(inl[below])  # the inliers below it are inl[0 .. below - 1]
            C.inject(prog, np.array([nq, counts[1]], np.uint32))
            cut = ([corners[0][:nq], corners[1]], [matches[0][:nq]], epi)
            assert list(prog.batch_counts(2)) == [nq, counts[1]]
            rec, pts = _check(prog, 2, cap, cut, pc.DEFAULT)[0]
            print("inliers below the counter %d (counter %d): status %d, inliers %d, good %d" % (below, nq, rec["status"], rec["inliers"], rec["good"]))
            if below < pr.MIN_INLIERS:
                assert rec["status"] == tinyorb.ORB_POSE_FEW and _zeros(rec, pts), rec
            else:
                assert rec["inliers"] == below and rec["r"].any() and rec["t"].any(), rec
                assert not pts[nq:].tobytes().strip(b"\0")
        C.inject(prog, counts)
        again = _check(prog, 2, cap, (corners, matches, epi), pc.DEFAULT)[0][0]
        assert again.tobytes() == full.tobytes()


# entries of SWEEP under which, for the scenes below, one rotation (Ra / Rb) or none is valid for some pair: found on the CPU, and
# asserted below on the device's own inputs
VALID_1, VALID_2, VALID_0 = 27, 118, 11


def test_two_workgroups_with_other_winners(tinyorb):
    """Capacity 1100: two workgroups of 1024 threads per pair, which must take the same winner, rotation and sign.  Scenes down, left
    and back (winners 1, 3 and 1 at the default intrinsics), raw counters above the capacity on one; then one entry of SWEEP for
    each of valid 1, 2 and 0."""
    cap = 1100
    scenes = [pc.build_scene(m, s, count=cap, n=1400) for m, s in (("down", 221), ("left", 222), ("back", 223))]
    with _program(tinyorb, W0, H0, cap, 6) as prog:
        B = _inject_scenes(prog, scenes, cap, extra={2: 41, 3: 7})
        prog.match_consecutive(B)
        prog.verify_epipolar(B, inlier_px=pc.INLIER_PX)
        inputs = _inputs(prog, B, cap)
        assert [len(c) for c in inputs[0]] == [cap] * 6 and list(prog.batch_counts(B)[2:4]) == [cap + 41, cap + 7]
        res = _check(prog, B, cap, inputs, pc.DEFAULT)
        labels = [pc.trace_pair(inputs, f, pc.DEFAULT) for f in (0, 2, 4)]
        print("default", [(c["winner"], c["status"], int(res[f][0]["good"])) for c, f in zip(labels, (0, 2, 4))])
        assert all(c["status"] == tinyorb.ORB_POSE_OK for c in labels) and {c["winner"] for c in labels} == {1, 3}
        for f in (0, 2, 4):  # good points in both workgroups' halves
            good = res[f][1]["flags"] & tinyorb.ORB_POINT_GOOD != 0
            assert good[:1024].sum() > 500 and good[1024:].sum() > 20
        for k, valid in ((VALID_1, 1), (VALID_2, 2), (VALID_0, 0)):
            labels = [pc.trace_pair(inputs, f, pc.SWEEP[k]) for f in (0, 2, 4)]
            print("entry", k, [(c["e"], c["valid"], c["winner"], c["status"]) for c in labels])
            assert any(c["e"] == "ok" and c["valid"] == valid for c in labels), (k, labels)
            assert all(c["winner"] is None or c["valid"] >> (c["winner"] >> 1) & 1 for c in labels)
            res = _check(prog, B, cap, inputs, pc.SWEEP[k])
            for c, f in zip(labels, (0, 2, 4)):
                assert (c["winner"] is None) == (res[f][0]["status"] == tinyorb.ORB_POSE_NOMODEL)
                if c["winner"] is None:
                    assert _zeros(*res[f])
