"""The CPU restatement of relative pose recovery and triangulation (tests/pose_ref.py, RP-1..RP-7 of DESIGN.md section 19) on the
constructed two-view scenes of tests/epipolar_ref.py, against the scenes' true motion and a float64 SVD of the same F, its status
cases, and the checks of its C ABI that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import pose_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
W, H, FOCAL = 640, 480, 500.0
K = np.array([[FOCAL, 0, (W - 1) / 2], [0, FOCAL, (H - 1) / 2], [0, 0, 1.0]])  # level-0 (pixel-centre) coordinates, as scene()'s Kc
INTR = dict(fx=FOCAL, fy=FOCAL, cx=(W - 1) / 2, cy=(H - 1) / 2)
MOTIONS, SEEDS = ("sideways", "yaw", "forward"), (0, 1, 2)
# Measured over the nine scenes: the largest angle between the restatement's winner and the nearest
# candidate of pose_ref.svd_pose on the same F.  The tests' bounds are twice these; the factor 2 covers the pairs of other seeds.
SVD_ROTATION_DEG, SVD_DIRECTION_DEG = 0.0237, 0.0301
# Measured the same way: the smallest share of planted epipolar inliers that come out good is 0.9011 (sideways, seed 1, whose F
# puts t 5 degrees off; 1.0 on the eight other scenes); the smallest share of those good points whose depth is within 25 % of the
# true one is 0.985 (forward, seed 2; the median error there is 2 %).  Each bound leaves 0.02 / 0.015 below the measured value.
GOOD_SHARE, DEPTH_REL, DEPTH_SHARE = 0.88, 0.25, 0.97

_CACHE = {}


def _run(motion, seed):
    """scene -> brute-force matches -> epipolar restatement -> pose restatement, once per (motion, seed)."""
    if (motion, seed) not in _CACHE:
        s = er.scene(np.random.default_rng(seed), motion, W, H)
        m = C.match_ref(s["desc"][0], s["desc"][1])
        rec, mask = er.verify_pair(s["corners"][0], s["corners"][1], m, W, H, 0, inlier_px=2.0)
        pose, pts = pr.pose_pair(s["corners"][0], s["corners"][1], m, rec, mask, **INTR)
        _CACHE[motion, seed] = (s, m, rec, mask, pose, pts)
    return _CACHE[motion, seed]


def _four(rec):
    ra, rb, t, va, vb = pr.candidates(rec["h"], *(np.float32(INTR[k]) for k in ("fx", "fy", "cx", "cy")))
    t = np.array(t, np.float64)
    return [(np.array(ra, np.float64), t), (np.array(ra, np.float64), -t), (np.array(rb, np.float64), t), (np.array(rb, np.float64), -t)]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("motion", MOTIONS)
def test_ground_truth_scenes(motion, seed):
    """Status OK; the winner is, of the four candidates, the nearest the scene's true (R, t) and has t . t_true > 0; R is a rotation
    to max |R^T R - I| < 1e-6 (measured <= 1.2e-7 after three polar steps; the bound is a few ulp of accumulated rounding above)."""
    s, m, rec, mask, pose, pts = _run(motion, seed)
    Rt, tt = er.scene_motion(motion)
    assert pose["status"] == pr.ORB_POSE_OK, pose
    assert pose["inliers"] == int(mask.sum()) and pose["good"] == int((pts["flags"] & pr.ORB_POINT_GOOD != 0).sum())
    R, t = pose["r"].astype(np.float64).reshape(3, 3), pose["t"].astype(np.float64)
    dist = [pr.rotation_angle_deg(Rk, Rt) + pr.direction_angle_deg(tk, tt) for Rk, tk in _four(rec)]
    k = int(np.argmin(dist))
    Rk, tk = _four(rec)[k]
    assert np.array_equal(Rk.reshape(3, 3), R) and np.array_equal(tk, t), (k, dist)
    assert t @ tt > 0
    orth = np.abs(R.T @ R - np.eye(3)).max()
    print(motion, seed, "rotation error %.3f deg, direction error %.3f deg, orth %.2e, |t| - 1 = %.1e" %
          (pr.rotation_angle_deg(R, Rt), pr.direction_angle_deg(t, tt), orth, np.linalg.norm(t) - 1))
    assert orth < 1e-6


def test_closed_form_against_svd():
    """The yardstick is the float64 SVD of the same F, not the kernel: over the nine scenes the winner lies within twice the measured
    maxima of the nearest SVD candidate."""
    rot = direction = 0.0
    for motion in MOTIONS:
        for seed in SEEDS:
            _, _, rec, _, pose, _ = _run(motion, seed)
            R1, R2, ts = pr.svd_pose(rec["h"], K)
            rot = max(rot, min(pr.rotation_angle_deg(pose["r"], R1), pr.rotation_angle_deg(pose["r"], R2)))
            direction = max(direction, min(pr.direction_angle_deg(pose["t"], ts), pr.direction_angle_deg(pose["t"], -ts)))
    print("max rotation angle to the SVD's %.4f deg, max direction angle %.4f deg" % (rot, direction))
    assert rot <= 2 * SVD_ROTATION_DEG
    assert direction <= 2 * SVD_DIRECTION_DEG


def _true_depths(seed, n=600, zmin=2.0, zmax=12.0):
    """The first draws of epipolar_ref.scene: frame-0 pixel -> the depths of the scene points that fall into it."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    z = 1.0 / rng.uniform(1.0 / zmax, 1.0 / zmin, n)
    d = {}
    for a, b, c in zip(np.floor(x).astype(int).tolist(), np.floor(y).astype(int).tolist(), z.tolist()):
        d.setdefault((a, b), []).append(c)
    return d


def test_planted_points_and_depths():
    """Of the planted correspondences that are epipolar inliers (and whose frame-0 pixel holds one scene point, so that the true
    depth is known), the share that comes out good, and of those the share whose z, times the true baseline length, is within
    DEPTH_REL of the true depth."""
    worst_good, worst_depth = 1.0, 1.0
    for motion in MOTIONS:
        for seed in SEEDS:
            s, _, _, mask, _, pts = _run(motion, seed)
            depths = _true_depths(seed)
            c0 = s["corners"][0]
            sel = [i for i in np.nonzero(s["planted"] & (mask[:len(c0)] == 1))[0] if len(depths.get((int(c0["x"][i]), int(c0["y"][i])), ())) == 1]
            assert len(sel) > 500
            zt = np.array([depths[int(c0["x"][i]), int(c0["y"][i])][0] for i in sel])
            good = (pts["flags"][sel] & pr.ORB_POINT_GOOD) != 0
            rel = np.abs(pts["z"][sel][good].astype(np.float64) * np.linalg.norm(er.scene_motion(motion)[1]) / zt[good] - 1)
            print(motion, seed, "good %.4f, depth within %.0f %%: %.4f (median error %.3f)" % (good.mean(), 100 * DEPTH_REL, (rel < DEPTH_REL).mean(), np.median(rel)))
            worst_good, worst_depth = min(worst_good, good.mean()), min(worst_depth, (rel < DEPTH_REL).mean())
    assert worst_good >= GOOD_SHARE
    assert worst_depth >= DEPTH_SHARE


# ---- status cases ------------------------------------------------------------------------------------------------------------
def _inliers(motion="yaw", seed=0):
    s, m, rec, mask, _, _ = _run(motion, seed)
    sel = np.nonzero(mask[:len(m)] == 1)[0]
    u1, v1 = er.vr.level0(s["corners"][0][sel])
    u2, v2 = er.vr.level0(s["corners"][1][m["index"][sel].astype(np.int64)])
    return rec, u1, v1, u2, v2


def _all_zero(pose, pts):
    return not pose["r"].any() and not pose["t"].any() and pose["inliers"] == pose["good"] == pose["second"] == 0 and not pts.tobytes().strip(b"\0")


def test_seven_inliers_are_few():
    rec, u1, v1, u2, v2 = _inliers()
    pose, pts = pr.pose_points(rec["h"], rec["status"], u1[:7], v1[:7], u2[:7], v2[:7], **INTR)
    assert pose["status"] == pr.ORB_POSE_FEW and _all_zero(pose, pts)
    pose, pts = pr.pose_points(rec["h"], rec["status"], u1[:8], v1[:8], u2[:8], v2[:8], **INTR)
    assert pose["status"] == pr.ORB_POSE_OK and pose["inliers"] == 8 and pose["good"] == 8
    # eight inliers, nine asked for: FEW by RP-6's second rule, and the record and the points are written
    pose, pts = pr.pose_points(rec["h"], rec["status"], u1[:8], v1[:8], u2[:8], v2[:8], min_good=9, **INTR)
    assert pose["status"] == pr.ORB_POSE_FEW and pose["good"] == 8 and pose["r"].any() and (pts["flags"] & 1).all()


def test_no_model():
    rec, u1, v1, u2, v2 = _inliers()
    for status in (er.VERIFY_DEGENERATE, er.VERIFY_FEW):
        pose, pts = pr.pose_points(rec["h"], status, u1, v1, u2, v2, **INTR)
        assert pose["status"] == pr.ORB_POSE_NOMODEL and _all_zero(pose, pts)
    for f in (np.zeros(9, np.float32), np.full(9, np.nan, np.float32), np.array([np.inf] + [0] * 8, np.float32)):
        pose, pts = pr.pose_points(f, er.VERIFY_OK, u1, v1, u2, v2, **INTR)
        assert pose["status"] == pr.ORB_POSE_NOMODEL and _all_zero(pose, pts), f
    pose, _ = pr.pose_points(rec["h"], er.VERIFY_MINIMAL, u1, v1, u2, v2, **INTR)
    assert pose["status"] == pr.ORB_POSE_OK


def test_parameters_move_the_status():
    rec, u1, v1, u2, v2 = _inliers()
    base, _ = pr.pose_points(rec["h"], rec["status"], u1, v1, u2, v2, **INTR)
    assert base["status"] == pr.ORB_POSE_OK and 0 < 1000 * base["second"] < 700 * base["good"]
    tiny, _ = pr.pose_points(rec["h"], rec["status"], u1, v1, u2, v2, max_reproj_px=1e-6, **INTR)
    assert tiny["status"] == pr.ORB_POSE_FEW and tiny["good"] < 8 and tiny["inliers"] == base["inliers"]
    amb, _ = pr.pose_points(rec["h"], rec["status"], u1, v1, u2, v2, ambiguity_permille=1, **INTR)
    assert amb["status"] == pr.ORB_POSE_AMBIGUOUS and amb["r"].tobytes() == base["r"].tobytes()
    sure, _ = pr.pose_points(rec["h"], rec["status"], u1, v1, u2, v2, ambiguity_permille=1000, **INTR)
    assert sure["status"] == pr.ORB_POSE_OK
    flat, pts = pr.pose_points(rec["h"], rec["status"], u1, v1, u2, v2, max_cos_parallax=0.5, **INTR)
    assert flat["status"] == pr.ORB_POSE_LOW_PARALLAX and flat["good"] == base["good"] and not (pts["flags"] & pr.ORB_POINT_PARALLAX).any()


def test_baseline_length_is_unobservable():
    """A pure-forward scene, and the same with t doubled: the same R and the same unit t."""
    poses = []
    for scale in (1.0, 2.0):
        s = er.scene(np.random.default_rng(5), (np.eye(3), np.array([0.0, 0.0, 0.2 * scale])), W, H, outlier_share=0.0)
        m = C.match_ref(s["desc"][0], s["desc"][1])
        rec, mask = er.verify_pair(s["corners"][0], s["corners"][1], m, W, H, 0, inlier_px=2.0)
        pose, _ = pr.pose_pair(s["corners"][0], s["corners"][1], m, rec, mask, **INTR)
        assert pose["status"] == pr.ORB_POSE_OK, pose
        poses.append(pose)
    for pose in poses:
        # pixel rounding leaves F a fraction of a degree off: 1 degree is several times what the nine scenes above show
        assert pr.rotation_angle_deg(pose["r"], np.eye(3)) < 1.0 and pr.direction_angle_deg(pose["t"], [0, 0, 1]) < 3.0, pose
    assert pr.rotation_angle_deg(poses[0]["r"], poses[1]["r"]) < 1.0 and pr.direction_angle_deg(poses[0]["t"], poses[1]["t"]) < 3.0


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_structs_and_constants(tinyorb):
    text = open(HEADER).read()
    assert ctypes.sizeof(tinyorb._PoseParams) == 32 and tinyorb.POSE_DTYPE.itemsize == 64 and tinyorb.POINT_DTYPE.itemsize == 16
    assert [tinyorb.POSE_DTYPE.fields[k][1] for k in ("r", "t", "inliers", "good", "second", "status")] == [0, 36, 48, 52, 56, 60]
    assert [tinyorb.POINT_DTYPE.fields[k][1] for k in ("x", "y", "z", "flags")] == [0, 4, 8, 12]
    fields = re.search(r"typedef struct \{([^}]*)\} OrbPoseParams;", text, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [f[0] for f in tinyorb._PoseParams._fields_]
    consts = dict(re.findall(r"#define\s+(ORB_PO[A-Z_]+)\s+(\d+)u\b", text))
    assert len(consts) == 7
    for name, value in consts.items():
        assert int(value) == getattr(tinyorb, name), name
    sigs = dict(re.findall(r"^int (orb_pose_\w+)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_pose_consecutive": "OrbProgram *p, uint32_t n_frames, const OrbPoseParams *params, void *stream",
                    "orb_pose_read": "OrbProgram *p, uint32_t pair, OrbPairPose *pose, OrbPoint *points, size_t n"}
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_abi_exports_and_null_program(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_pose_consecutive", "orb_pose_read"):
        assert n in tinyorb.EXPORTS
        assert hasattr(L, n)
    prm = tinyorb._PoseParams(500.0, 500.0, 320.0, 240.0)
    assert L.orb_pose_consecutive(None, 2, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_pose_consecutive(None, 2, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_pose_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("pose" in n for n in names)
