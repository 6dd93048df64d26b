"""The census of tests/pose_census.py on the CPU: SCENES x SWEEP through scene -> brute-force matches -> the epipolar restatement ->
trace reaches every branch of RP-2..RP-6 that tests/test_gpu_pose_census.py compares on the device (so that test cannot pass on
inputs that stopped reaching a branch), and trace agrees with pose_ref.pose_points on every case.

Not asked for: RP-3's `best <= 0`, unreachable for finite input (after RP-2 the squares of E sum to 2, so trace T = 1 and the largest
diagonal entry is at least 1/3 up to rounding), and FEW by the inlier count with a valid model, which needs a raw counter overwritten
on the device (test_gpu_pose_census.test_few_by_inlier_count; trace's own label for it is checked here on cut inputs)."""
import numpy as np

import pose_census as pc
import pose_ref as pr


def test_census_reaches_every_branch():
    assert 150 <= len(pc.SWEEP) <= 300 and pc.SWEEP[0] == pc.DEFAULT and pc.SWEEP[1] == pc.OFF_CENTRE
    for intr in pc.SWEEP:  # what orb_pose_consecutive accepts, as binary32
        v = [np.float32(intr[k]) for k in ("fx", "fy", "cx", "cy")]
        assert np.isfinite(v).all() and v[0] > 0 and v[1] > 0
    inputs = pc.cpu_inputs([pc.build_scene(m, s) for m, s in pc.SCENES])
    corners, matches, epi = inputs
    rows = pc.census(inputs)
    print("\n" + pc.table(rows))
    pc.check_census(rows)
    # trace against pose_ref.pose_points: the status, and the record is candidate `winner`'s (zeros when there is none)
    for intr, row in zip(pc.SWEEP, rows):
        for f, c in enumerate(row):
            rec, mask = epi[f]
            pose, pts = pr.pose_points(rec["h"], rec["status"], *pc.inlier_coordinates(corners[f], corners[f + 1], matches[f], mask), **intr)
            assert pose["status"] == c["status"], (intr, f, c, pose)
            if c["winner"] is None:
                assert not pose.tobytes()[:60].strip(b"\0") and not pts.tobytes().strip(b"\0"), (intr, f, c, pose)
            else:
                r, t = pc.candidate(rec["h"], intr, c["winner"])
                assert pose["r"].tobytes() == r.tobytes() and pose["t"].tobytes() == t.tobytes() and pose["inliers"] == int(mask.sum()), (intr, f, c)


def test_trace_few_by_inlier_count():
    """Seven inliers of a pair with a model: FEW by the inlier count, no winner; eight: a winner."""
    inputs = pc.cpu_inputs([pc.build_scene(*pc.SCENES[4])])
    corners, matches, epi = inputs
    rec, mask = epi[0]
    u1, v1, u2, v2 = pc.inlier_coordinates(corners[0], corners[1], matches[0], mask)
    for n, few in ((7, "inliers"), (8, None)):
        c = pc.trace(rec["h"], rec["status"], pc.DEFAULT, u1[:n], v1[:n], u2[:n], v2[:n])
        pose, _ = pr.pose_points(rec["h"], rec["status"], u1[:n], v1[:n], u2[:n], v2[:n], **pc.DEFAULT)
        assert c["few_by"] == few and (c["winner"] is None) == (n == 7) and c["status"] == pose["status"] and c["valid"] == 3
        assert (c["status"] == pr.ORB_POSE_FEW) == (n == 7)
