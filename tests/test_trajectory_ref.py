"""The CPU restatement of the trajectory stage (tests/trajectory_ref.py, TJ-1..TJ-7 of DESIGN.md section 20): hand-built pose and point
arrays that pin the definition, and its accuracy on constructed camera paths through the project's own restatements: match_ref ->
epipolar_ref.verify_pair -> pose_ref.pose_pair -> trajectory."""
import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import pose_ref as pr
import trajectory_cases as tc
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
W, H, FOCAL = 640, 480, 500.0
INTR = dict(fx=FOCAL, fy=FOCAL, cx=(W - 1) / 2, cy=(H - 1) / 2)
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX
IDENTITY = np.eye(3, dtype=F).ravel()


# ---- hand-built inputs (the builders are tests/trajectory_cases.py's, which the GPU tests share) -------------------------------
_pose = tc.pose


def _joint_case(rho, index=None, flags_a=None, flags_b=None, zb=None, **params):
    """Three frames, both pairs OK with R = I and t = 0, so that Yz = Xz exactly; pair 0's point i is (0, 0, rho[i]) and pair 1's
    point j is (0, 0, zb[j]) (1 by default): the ratio of i is rho[i] / zb[index[i]], exactly rho[i] by default."""
    if index is not None:
        index = np.where(np.asarray(index) == orb.ORB_MATCH_NONE, tc.NONE, np.asarray(index))
    return tc.run_case(tc.joint_case("", rho, index=index, flags_a=flags_a, flags_b=flags_b, zb=zb), **params)


def test_verdicts_and_the_lower_median():
    # m odd: the middle; m even: the lower of the two middle ones
    fr, _ = _joint_case(F([1.02, 0.98, 1.0, 1.01, 0.99, 1.03, 0.97, 1.04, 0.96]))
    assert fr["status"].tolist() == [orb.ORB_TRAJ_ORIGIN, orb.ORB_TRAJ_START, orb.ORB_TRAJ_CHAINED]
    assert fr["step"][2] == F(1.0) and fr["shared"][2] == 9 and fr["consistent"][2] == 9 and fr["scale"][2] == F(1.0)
    fr, _ = _joint_case(F([1.02, 0.98, 1.0, 1.01, 0.99, 1.03, 0.97, 1.04]))
    assert fr["status"][2] == orb.ORB_TRAJ_CHAINED and fr["step"][2] == F(1.0) and fr["shared"][2] == 8
    # seven ratios: FEW (the record says how many there were; the step is 0), a restart from the pair's own pose
    fr, _ = _joint_case(F([1.02, 0.98, 1.0, 1.01, 0.99, 1.03, 0.97]))
    assert fr["status"][2] == orb.ORB_TRAJ_RESTART_FEW and fr["shared"][2] == 7 and fr["consistent"][2] == 7 and fr["step"][2] == 0
    assert fr["origin"].tolist() == [0, 0, 1] and fr["scale"][2] == F(1.0)
    fr, _ = _joint_case(F([1.02, 0.98, 1.0, 1.01, 0.99, 1.03, 0.97]), min_shared=7)
    assert fr["status"][2] == orb.ORB_TRAJ_CHAINED
    # ten ratios of which four lie within 10 % of the median 1.0: SPREAD at the default 500 permille, HOLDS at 400
    rho = F([0.5, 0.6, 0.7, 0.95, 1.0, 1.05, 1.08, 1.5, 2.0, 3.0])
    fr, _ = _joint_case(rho)
    assert fr["status"][2] == orb.ORB_TRAJ_RESTART_SPREAD and fr["step"][2] == F(1.0) and fr["shared"][2] == 10 and fr["consistent"][2] == 4
    fr, _ = _joint_case(rho, consistent_permille=400)
    assert fr["status"][2] == orb.ORB_TRAJ_CHAINED and fr["consistent"][2] == 4
    fr, _ = _joint_case(rho, consistent_permille=401)
    assert fr["status"][2] == orb.ORB_TRAJ_RESTART_SPREAD


def test_selection_is_exact_on_the_bits():
    # ratios that differ in their lowest byte only, in a scrambled order: ranks 0 .. 199 are bits base .. base + 199
    base = int(F(1.25).view(np.uint32)) & ~0xFF
    bits = (base + np.random.default_rng(0).permutation(200)).astype(np.uint32)
    fr, _ = _joint_case(bits.view(F))
    assert fr["step"][2].view(np.uint32) == base + 99 and fr["shared"][2] == 200 and fr["consistent"][2] == 200
    fr, _ = _joint_case(bits[:199].view(F))
    assert fr["step"][2].view(np.uint32) == np.sort(bits[:199])[99]
    # duplicates: 5 x a, 4 x b > a: rank 4 of 9 is a; 4 x a, 5 x b: rank 4 is b
    a, b = F(0.75), F(0.8)
    fr, _ = _joint_case(F([b, a, b, a, a, b, a, b, a]))
    assert fr["step"][2] == a and fr["consistent"][2] == 9
    fr, _ = _joint_case(F([b, a, b, a, b, b, a, b, a]))
    assert fr["step"][2] == b
    # ratios across exponents, denormals included: the bits order them
    rho = F([1e-40, 3e-39, 1e-20, 0.5, 1.0, 2.0, 1e20, 3e38, 1.5])
    fr, _ = _joint_case(rho, consistent_permille=1)
    assert fr["step"][2] == F(1.0) and fr["consistent"][2] == 1 and fr["status"][2] == orb.ORB_TRAJ_CHAINED


def test_what_counts_as_a_ratio():
    ones = np.ones(12, F)
    # a ratio that is not finite or not > 0 is ignored: z = 0 in pair 1 (inf, and nan for 0 / 0), negative depths
    rho = ones.copy()
    rho[0], rho[1] = -1.0, 0.0
    zb = ones.copy()
    zb[2], zb[1] = 0.0, 0.0
    fr, _ = _joint_case(rho, zb=zb)
    assert fr["shared"][2] == 9 and fr["status"][2] == orb.ORB_TRAJ_CHAINED
    # a point that is not GOOD in either pair; an index beyond frame 1's keypoints
    fa, fb = np.full(12, GOOD), np.full(12, GOOD)
    fa[3], fb[4] = 0, 0
    idx = np.arange(12)
    idx[5] = orb.ORB_MATCH_NONE
    fr, _ = _joint_case(ones, index=idx, flags_a=fa, flags_b=fb)
    assert fr["shared"][2] == 9  # i = 3 and i = 4 (its j is not good), i = 5
    # several i that share one j each count
    fr, _ = _joint_case(ones, index=np.zeros(12, np.int64))
    assert fr["shared"][2] == 12
    # NEED_PARALLAX: both points must carry the flag
    fa, fb = np.full(12, GOOD | PAR), np.full(12, GOOD | PAR)
    fa[:2], fb[2:5] = GOOD, GOOD
    assert _joint_case(ones, flags_a=fa, flags_b=fb)[0]["shared"][2] == 12
    fr, _ = _joint_case(ones, flags_a=fa, flags_b=fb, flags=orb.ORB_TRAJ_NEED_PARALLAX)
    assert fr["shared"][2] == 7 and fr["status"][2] == orb.ORB_TRAJ_RESTART_FEW


def test_lost_start_and_two_frames():
    n, cap = 10, 10
    pts = np.zeros(cap, orb.POINT_DTYPE)
    pts["x"], pts["y"], pts["z"], pts["flags"] = np.arange(cap), 1.0, 2.0, GOOD
    m = np.zeros(n, orb.MATCH_DTYPE)
    m["index"] = np.arange(n)
    Ry = tr.rot("y", 2.0).astype(F).ravel()
    poses = [_pose(r=Ry, t=(1, 0, 0)), _pose(orb.ORB_POSE_AMBIGUOUS, r=Ry, t=(1, 0, 0)), _pose(r=Ry, t=(0, 1, 0)), _pose(r=Ry, t=(0, 0, 1))]
    fr, world = tr.trajectory([n] * 5, [m] * 4, poses, [pts] * 4, cap)
    assert fr["status"].tolist() == [orb.ORB_TRAJ_ORIGIN, orb.ORB_TRAJ_START, orb.ORB_TRAJ_LOST, orb.ORB_TRAJ_START, orb.ORB_TRAJ_CHAINED]
    assert fr["origin"].tolist() == [0, 0, 2, 2, 2] and fr["scale"].tolist() == [0, 1, 0, 1, fr["step"][4]]
    assert np.array_equal(fr["r"][0], IDENTITY) and np.array_equal(fr["r"][2], IDENTITY) and not fr["t"][2].any()
    assert np.array_equal(fr["r"][1], Ry) and fr["t"][1].tolist() == [1, 0, 0] and fr["t"][3].tolist() == [0, 1, 0]
    assert fr["shared"].tolist() == [0, 0, 0, 0, 10] and not fr["reserved"].any()
    # the map: pair 0 copied (origin 0), pair 1 zeros (frame 2 is LOST), pair 2 copied (origin 2), pair 3 transformed, the last row zeros
    assert world[0].tobytes() == pts.tobytes() and world[2].tobytes() == pts.tobytes()
    assert not world[1].tobytes().strip(b"\0") and not world[4].tobytes().strip(b"\0")
    R3, t3, s = fr["r"][3].astype(np.float64).reshape(3, 3), fr["t"][3].astype(np.float64), float(fr["scale"][4])
    X = np.stack([pts[k] for k in "xyz"], 1).astype(np.float64)
    want = (R3.T @ (s * X - t3).T).T
    got = np.stack([world[3][k] for k in "xyz"], 1)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5) and (world[3]["flags"] == GOOD).all()
    # n_frames = 2: ORIGIN and START, pair 0 copied
    fr2, w2 = tr.trajectory([n, n], [m], poses[:1], [pts], cap)
    assert fr2.tobytes() == fr[:2].tobytes() and w2[0].tobytes() == pts.tobytes() and not w2[1].tobytes().strip(b"\0")
    fr2, w2 = tr.trajectory([n, n], [m], poses[1:2], [pts], cap)
    assert fr2["status"].tolist() == [orb.ORB_TRAJ_ORIGIN, orb.ORB_TRAJ_LOST] and not w2.tobytes().strip(b"\0")


# Measured on the restatement: max |R^T R - I| over the 4096 frames of the chain below is 2.23e-7 -- one polar
# step per composition holds the product at a few ulp however long the chain.  The bound is twice that.
CHAIN_ORTH = 2.23e-7


def test_a_4096_frame_chain_stays_orthonormal():
    n = 4096
    b, Rs = tc.long_chain(n)
    fr, _ = tc.reference(b)
    assert (fr["status"][2:] == orb.ORB_TRAJ_CHAINED).all() and (fr["origin"] == 0).all() and np.isfinite(fr["scale"]).all()
    R = fr["r"].astype(np.float64).reshape(n, 3, 3)
    orth = np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max()
    # the rotation itself: frame f has turned f times the step's angle
    angle = pr.rotation_angle_deg(fr["r"][n - 1], np.linalg.matrix_power(Rs.astype(np.float64).reshape(3, 3), n - 1))
    print("4096 frames: max |R^T R - I| = %.3e, angle to the float64 power %.4f deg" % (orth, angle))
    assert orth <= 2 * CHAIN_ORTH
    assert angle < 0.5


# ---- accuracy on constructed paths -------------------------------------------------------------------------------------------
PATHS, SEEDS = ("sideways", "forward"), (0, 1, 2)
# Measured on the restatement over the six scenes, each the worst over scenes, frames and joints: the relative
# error of `step` against the true ratio of step lengths; the distance of the camera centre -R^T t from the true one over the true
# centre's distance from the origin, in units of the first step; the median over a pair's GOOD planted map points of the distance
# from the true landmark over the landmark's distance from the origin, and the smallest share of them within MAP_REL.  The tests'
# bounds are twice the errors, and the share less twice what the measured one leaves to 1.
STEP_ERR, CENTRE_ERR, MAP_MEDIAN_ERR, MAP_REL, MAP_SHARE = 0.0305, 0.0519, 0.0350, 0.25, 0.972
ENTER_SHARE = 0.90  # a cap, not a measurement: planted landmarks GOOD in both pairs that enter the joint

_CACHE = {}


def _run(path, seed):
    if (path, seed) not in _CACHE:
        s = tr.path_scene(np.random.default_rng(seed), tr.path_steps(path), W, H, FOCAL)
        V = len(s["corners"])
        m = [C.match_ref(s["desc"][f], s["desc"][f + 1]) for f in range(V - 1)]
        ep = [er.verify_pair(s["corners"][f], s["corners"][f + 1], m[f], W, H, f, inlier_px=2.0) for f in range(V - 1)]
        po = [pr.pose_pair(s["corners"][f], s["corners"][f + 1], m[f], ep[f][0], ep[f][1], **INTR) for f in range(V - 1)]
        counts = [len(c) for c in s["corners"]]
        fr, world = tr.trajectory(counts, m, [p[0] for p in po], [p[1] for p in po], max(counts))
        _CACHE[path, seed] = (s, po, fr, world)
    return _CACHE[path, seed]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("path", PATHS)
def test_path_accuracy(path, seed):
    s, po, fr, world = _run(path, seed)
    L = [np.linalg.norm(t) for _, t in tr.path_steps(path)]
    V = len(fr)
    assert fr["status"].tolist() == [orb.ORB_TRAJ_ORIGIN, orb.ORB_TRAJ_START] + [orb.ORB_TRAJ_CHAINED] * (V - 2), fr["status"]
    assert (fr["origin"] == 0).all()
    step = max(abs(float(fr["step"][k + 1]) / (L[k] / L[k - 1]) - 1) for k in range(1, V - 1))
    centre = 0.0
    for k in range(1, V):
        R, t = fr["r"][k].astype(np.float64).reshape(3, 3), fr["t"][k].astype(np.float64)
        Rt, tt = s["poses"][k]
        Ct = -Rt.T @ tt / L[0]
        centre = max(centre, np.linalg.norm(-R.T @ t - Ct) / np.linalg.norm(Ct))
    med, share = 0.0, 1.0
    for f in range(V - 1):
        ids = s["ids"][f]
        sel = np.nonzero(((world["flags"][f][:len(ids)] & GOOD) != 0) & (ids < s["n_landmarks"]))[0]
        assert len(sel) > 150
        got = np.stack([world[k][f][sel] for k in "xyz"], 1).astype(np.float64)
        want = s["cloud"][ids[sel]] / L[0]
        rel = np.linalg.norm(got - want, axis=1) / np.linalg.norm(want, axis=1)
        med, share = max(med, float(np.median(rel))), min(share, float((rel < MAP_REL).mean()))
    enter = 1.0
    for f in range(1, V - 1):  # joint f: planted landmarks GOOD in pair f - 1 and in pair f
        ida, idb = s["ids"][f - 1], s["ids"][f]
        ga, gb = (po[f - 1][1]["flags"][:len(ida)] & GOOD) != 0, (po[f][1]["flags"][:len(idb)] & GOOD) != 0
        both = np.isin(ida[ga & (ida < s["n_landmarks"])], idb[gb])
        enter = min(enter, int(fr["shared"][f + 1]) / int(both.sum()))
    print("%s %d: step error %.4f, centre error %.4f, map median error %.4f, share within %.2f: %.4f, entering %.3f, shared %s, consistent %s"
          % (path, seed, step, centre, med, MAP_REL, share, enter, fr["shared"][2:].tolist(), fr["consistent"][2:].tolist()))
    assert step <= 2 * STEP_ERR
    assert centre <= 2 * CENTRE_ERR
    assert med <= 2 * MAP_MEDIAN_ERR
    assert share >= 1 - 2 * (1 - MAP_SHARE)
    assert enter >= ENTER_SHARE
