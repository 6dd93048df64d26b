"""Which branches of RP-2..RP-6 a pair reaches under one set of intrinsics, and the fixed scenes and
intrinsics that reach all of them (test infrastructure, not a test file).

The pose kernels take F from the epipolar record, so a test cannot hand them an F of its choice; but E = K^T F K and the caller
chooses K.  `trace` labels one (pair, intrinsics) case with pose_ref's own functions; SCENES and SWEEP are the committed inputs
over which tests/test_pose_census_ref.py (CPU) and tests/test_gpu_pose_census.py (device) assert that every label is reached.

Not asked for: RP-3's `best <= 0`.  After RP-2 the squares of E sum to 2, so trace T = 3 - 2 = 1 and the largest diagonal entry is
at least 1/3 up to rounding: no finite input reaches that branch.
"""
import numpy as np

import constructed as C
import epipolar_ref as er
import pose_ref as pr
import verify_ref as vr

F = np.float32
W, H, FOCAL = 640, 480, 500.0
DEFAULT = dict(fx=FOCAL, fy=FOCAL, cx=(W - 1) / 2, cy=(H - 1) / 2)
OFF_CENTRE = dict(fx=480.0, fy=510.0, cx=300.25, cy=250.5)
INLIER_PX = 2.0
TINY = F(2.0 ** -126)  # the smallest normal binary32

_I = np.eye(3)
_YAW = er.scene_motion("yaw")[0]
MOTIONS = {"sideways": er.scene_motion("sideways"), "left": (_I, np.array([-0.3, 0.0, 0.0])), "up": (_I, np.array([0.0, 0.3, 0.0])),
           "down": (_I, np.array([0.0, -0.3, 0.0])), "forward": er.scene_motion("forward"), "back": (_I, np.array([0.0, 0.0, -0.3])),
           "diagonal": (_I, np.array([0.2, 0.2, 0.2])), "yaw": er.scene_motion("yaw"), "rotation": (_YAW, np.zeros(3)),
           "outliers": er.scene_motion("sideways")}


# (motion, seed), scene i in frames (2i, 2i + 1) of one batch: chosen on the CPU so that at DEFAULT and the default parameters the winners
# are 0, 3, 0, 1, 2, 3, 0, 0 with status OK (rows 0, 0, 1, 1, 2, 2, 2, 0), the first pure rotation is AMBIGUOUS and the second
# LOW_PARALLAX.  The outliers-only scene's 64 chance correspondences leave the verifier a model with 13 inliers: FEW by min_good.  The
# seeds differ, so no descriptor is shared between two scenes and the ten pairs between them have no candidates: the verifier's FEW,
# NOMODEL by RP-1.
SCENES = [("sideways", 13), ("left", 11), ("up", 21), ("down", 31), ("forward", 41), ("back", 51), ("diagonal", 61), ("yaw", 71),
          ("rotation", 82), ("rotation", 91), ("outliers", 101)]


# (fx, fy, cx, cy), binary32 values in their shortest decimal form; the order is part of the test (see below).  The default, a principal
# point off the centre with fx != fy, then draws with fx, fy log-uniform in 10^[-24, 16] (a part of them in 10^[-12, 12]) and |cx|, |cy| in
# 10^[-3, 16] with a random sign, searched on the CPU over SCENES and cut down to: every draw found with one valid rotation (valid 1
# or 2; about one (pair, draw) case in 1500), draws with n = 0, with n not finite, with both rotations invalid and with a subnormal
# intermediate beside a model for some pair, and unselected draws.  A draw that leaves a pair of SCENES without a model follows an
# entry that wrote that pair's record (a draw that writes all eleven, or the default again, is put before it where needed), so that
# a record, points or counters left over from the call before would show.
_SWEEP = [
    (500.0, 500.0, 319.5, 239.5),
    (480.0, 510.0, 300.25, 250.5),
    (27706.71, 4.614292e-16, 125.469406, 4796.5884),
    (3288.2524, 7.6996e-24, -0.0042892923, -745399000000000.0),
    (590293100.0, 1.1358599e-14, -0.40059778, -5965.552),
    (0.1184711, 6.979719e-12, 20900219000000.0, 46410510000.0),
    (2.471486, 81288.87, -0.025051212, 3033548.5),
    (5.8260364e-22, 175906090000000.0, 6.153972, -243.59503),
    (500.0, 500.0, 319.5, 239.5),
    (3722.3447, 375317330000000.0, -29556560.0, -104489110.0),
    (5.1092877, 1085745.2, -68052850000.0, 8634548.0),
    (4.1304145e-21, 4.0661994e-18, -137.67555, -36537.637),
    (0.000567032, 21223658.0, 83630.83, 46.819633),
    (714829460000.0, 33811292.0, -3482990000000.0, 6815.052),
    (0.06883863, 5383085600.0, -77720.83, 84.67341),
    (8.9375815e-21, 3.528353e-16, 3533267000.0, -497676.12),
    (45162630.0, 3776.1118, -128783910.0, 52019024.0),
    (5.2254052e-23, 0.2134102, 1189385300000.0, 0.94549567),
    (12.493434, 1.7972559e-07, 0.028539268, -0.0747582),
    (8.2021834e-20, 1238127000.0, 6609295.0, 8038.1),
    (3.403307e-21, 1.6742094e-15, 29563768.0, 41.97631),
    (500.0, 500.0, 319.5, 239.5),
    (104331624000.0, 1.4507966e-10, 308718930000.0, -0.022145063),
    (3.1855606e-17, 3297300000.0, 37730800.0, 643.8941),
    (6.9086035e-16, 1.9128055e-24, -1375670.6, -847766400000000.0),
    (2.1043473e-20, 1.2735627, 1833.6926, -0.00503656),
    (180838780.0, 4.91084e-24, 0.0055170855, 5.6397653),
    (326130100000.0, 237136.61, -54616125000.0, 53287.246),
    (2.5184053e-15, 212.59023, -6574904.0, -4500776600000.0),
    (999.41473, 424626.8, 176688.81, 602460860.0),
    (5652164.0, 6.729693e-23, -797284240000.0, 111593740000000.0),
    (500.0, 500.0, 319.5, 239.5),
    (0.022257656, 1.3048042e-24, 454.35342, 0.010524054),
    (182197600000.0, 874.4765, 0.6557641, 165381010.0),
    (1.6417733e-13, 1.4339347e-16, -752019400.0, 2508892200.0),
    (0.009154957, 2.1487756e-05, 0.039370604, -27.459734),
    (4.096159e-06, 5053520000000000.0, 42.352184, 117399.445),
    (174444540.0, 2.8080187e-21, 0.05256493, -0.0095203025),
    (259508880.0, 375.96567, 295442900000.0, -0.05221903),
    (500.0, 500.0, 319.5, 239.5),
    (8906.76, 267760200000.0, -592981300000000.0, 4.679315),
    (3955.286, 4.9446204e-11, -61841.37, 6050.711),
    (20420.207, 2186158100000.0, -44493.906, -3615929.5),
    (0.4241694, 288.67435, -332828.16, -516.9518),
    (7.993302e-11, 3.963442e-08, 172.19507, -639207.75),
    (9.684676e-16, 17120770.0, -767152450.0, 3642175.5),
    (0.026326332, 7.797533e-20, -446221520000.0, 3626982.0),
    (500.0, 500.0, 319.5, 239.5),
    (4486831500000.0, 1187798500.0, 19979936000000.0, 0.47616693),
    (732.88513, 89626.164, -2287.658, -637.5679),
    (2918.0881, 7.296504e-13, 861199060000000.0, -0.0047016595),
    (2.0958704e-12, 0.6800368, 1.9008204, 315013.16),
    (100492360000000.0, 0.027571829, -129709.71, 5013986.5),
    (500.0, 500.0, 319.5, 239.5),
    (49064677000.0, 2259834400000000.0, -482952830.0, 50.406284),
    (3094.0427, 841529500.0, 4.0204296, 72722145000.0),
    (2025182.4, 5931478.5, -1728.9874, 24172388000.0),
    (2.0785252e-20, 0.047792863, -14.511646, 19214.807),
    (265469900000.0, 7.886023e-18, 61580.254, -921125.0),
    (702219.4, 7.236779e-07, 61598492.0, 1708455200.0),
    (7.561508e-09, 6.4996257e-09, -0.04401999, 691217500000.0),
    (13.592825, 2.7953768e-16, -1326.7817, -0.006102546),
    (5.2578525e-07, 6.6678375e-08, -0.008592832, -198832.33),
    (324.46414, 9.2057584e-05, -37574.617, 60.786713),
    (2.1294799e-16, 9.0702755e-13, -7498645000000.0, -3.20349),
    (223922200.0, 5.680935e-22, 38589.586, -167840.94),
    (1.5031043, 242191.95, 6022188400000000.0, 89655570000000.0),
    (92624870.0, 9782.632, -30149232.0, -2.3524647),
    (861714050.0, 5.037104e-06, -172.30241, 1485.2411),
    (4.375183e-13, 1.7760878e-09, -1257.5647, 809745750000000.0),
    (500.0, 500.0, 319.5, 239.5),
    (3.4137224e-23, 2.0562807e-24, -0.2632808, 1455316700000000.0),
    (1.0241646e-11, 0.00043795476, 2.430974, -0.00451858),
    (2.5637098e-24, 8.829145e-16, 171.98384, 711789900000.0),
    (23683286.0, 0.00027137218, -1576.9714, 113.04976),
    (3.7728137e-12, 6.4011516e-08, -2250797700000.0, -0.0015158078),
    (12067286.0, 1106299600.0, -0.07838335, -1552182000.0),
    (0.00023824393, 0.8310817, 3604919400000.0, -487558100.0),
    (500.0, 500.0, 319.5, 239.5),
    (9.2820876e-05, 9.380324e-12, 1294315000000.0, -0.16745745),
    (115668580000.0, 0.33381703, 51100670.0, -813159.75),
    (248.25912, 82970790.0, 0.32579866, 28809217000000.0),
    (127139160000.0, 3.9657082e-21, -7205078.0, -92912.305),
    (7.6135364, 0.3044092, 0.276335, 2783342200000.0),
    (2.7219873e-09, 1726.3832, -0.0015251308, 0.016747817),
    (4.162374e-17, 1595893700000.0, 50384496.0, 419093800.0),
    (2.5349475e-10, 13.886335, -4551.8506, 5562222.5),
    (1.2418871e-17, 1662241300000.0, -311.8884, -5763577.5),
    (5.014012e-18, 8.376538e-15, -80410485000.0, 4456613400.0),
    (500.0, 500.0, 319.5, 239.5),
    (3.475309e-08, 93870910000.0, 42822.496, 800328300.0),
    (0.00024998173, 509019.84, 50671.24, 0.26768833),
    (46.737896, 630250.44, 0.01418946, -1085428900.0),
    (193176320000.0, 797.63025, -3697243600.0, -12.699355),
    (93408.766, 2.5914949e-11, -310210.1, 177402950000000.0),
    (4.329093e-12, 2.3118741e-06, -0.17226234, -0.0011273004),
    (1162878800000.0, 28.194376, -498499.75, -152642780000.0),
    (0.0018235291, 70.56812, -0.00313337, -26164.76),
    (978478400000000.0, 1.4364641e-18, -19173272000.0, -314476.0),
    (500.0, 500.0, 319.5, 239.5),
    (840005950.0, 29908798.0, -9686531000000000.0, -3335583500000000.0),
    (268324850000.0, 74246.445, 529888250000.0, -3268.5173),
    (34316544.0, 4.945713, 7494640000.0, -247228220000000.0),
    (2.6676373, 1514006.1, -106879060000.0, 0.0049993335),
    (100830830000.0, 15042186000.0, 60.010765, 185403.2),
    (1267.1018, 117196990000000.0, 5.5441976, -189.92288),
    (2.6047569e-09, 0.38506752, 30004276.0, -0.05634952),
    (1656464500000000.0, 5.173705e-09, 412679.03, -162.70758),
    (63.572845, 5677.9375, -0.0032637462, 4212960.0),
    (7.0077165e-23, 6.1618007e-19, -651868.6, 0.0052000587),
    (369885.8, 1.225074e-07, 0.0032878127, -71908380.0),
    (51.687347, 43629007000.0, 337.12088, 10024952000.0),
    (500.0, 500.0, 319.5, 239.5),
    (0.086662695, 1.6773272e-05, -2359804.5, 0.74594283),
    (2.7277183e-10, 1531.0815, 9549709000.0, -0.031729683),
    (3.5131717e-18, 1.4720001e-14, -0.18132976, -1890451700.0),
    (467783680.0, 1.8795924e-06, -3244224.0, 0.046014685),
    (51035616.0, 1170916100.0, -2120345700000.0, -2325558.8),
    (20319064000.0, 6685.6387, -216274440000.0, -0.13802756),
    (4283504000.0, 105645.99, 1560979600.0, 496.8926),
    (2.5147604e-16, 0.20382854, 7304301.5, -78692106000000.0),
    (6.4490166e-16, 0.043847818, 0.0012844569, 30509.979),
    (0.007943906, 1.4946517e-16, -606461560000.0, 24149650.0),
    (500.0, 500.0, 319.5, 239.5),
    (2.1265691e-09, 0.001624438, -5337371600.0, -14086.155),
    (2.8655895e-06, 118848905000.0, 61968.97, -14792269.0),
    (0.00065152394, 0.00064185663, -0.016228627, 0.17140009),
    (12975662.0, 1.961527, -272952160.0, 2.0089843),
    (0.66863173, 2.5626866e-06, -31073290000000.0, 16291319000.0),
    (0.010242863, 3460.753, 1363238300000.0, -480.94946),
    (2.5645283e-10, 6705751000000.0, 63617.836, 91300086000.0),
    (1.2618327e-22, 123285360.0, -2834.0706, 860375940.0),
    (3.0391955e-24, 1.5163121e-10, -5.848701, 48987020000000.0),
    (6.6276975, 295725660000.0, -121.36098, -4282611000.0),
    (4190349600000.0, 1.2663245e-18, -10.317364, 771497.7),
    (1.2242373e-19, 2300076000.0, 0.00425364, 11767461.0),
    (176434510000.0, 60094583000.0, -258320660000.0, -45.412434),
    (0.00010601512, 20531.346, 701.02216, -0.5127774),
    (0.020560741, 119591920.0, 5.481908, -2435501200000000.0),
    (1.7156275e-19, 11834793.0, 555716700.0, 524849.25),
    (1.5367632e-07, 1.5154389e-09, 80934.086, 155.22638),
    (500.0, 500.0, 319.5, 239.5),
    (609476.6, 1902507000.0, 0.06403578, -2748828000000.0),
    (9767976.0, 5493.2837, 0.32105893, -37.091305),
    (0.00059660844, 4824011600000.0, 209169680000.0, -2454856400.0),
    (595553340.0, 3.0663434e-23, 0.8184887, -90671560.0),
    (164017000.0, 8.608085e-15, -4.048469, 4964963400000000.0),
    (500.0, 500.0, 319.5, 239.5),
    (1.0248864e-06, 22836259000.0, -0.3679597, -1871935900000000.0),
    (42148.27, 76.761406, 0.14074641, 583.89734),
    (4.379769e-17, 1.8273593e-13, -208905320000.0, 30322412.0),
    (2059350500.0, 3883809.0, -4824458000.0, 92.86168),
    (2079766700000.0, 2.5620523e-11, -0.7954775, -3054809300.0),
    (1465.2131, 371.51337, 198112900000.0, -121058230.0),
    (41910803000000.0, 93529.516, -18671693000000.0, -21978464.0),
    (0.000716852, 1.4245375, 886939.8, 7.272955),
    (9769082000.0, 10.583668, -228267.36, -358826.2),
    (3.382218e-10, 10.880467, -42.549942, -127052910000.0),
    (500.0, 500.0, 319.5, 239.5),
    (354.01993, 1.0110321e-09, -66131.52, 6635124000.0),
    (98.49153, 1.1497892e-19, 1093.0684, -705.468),
    (8.660264e-24, 208701.42, 3.0617537, 12263557000000.0),
    (4.8772433e-23, 2717694.0, 1299246.8, -2635655.5),
    (2.8708647e-19, 5.3501127e-11, 2678535700000.0, -0.6628054),
    (16055.253, 213362640.0, -342.5576, -1014554400000.0),
]
SWEEP = [dict(zip(("fx", "fy", "cx", "cy"), v)) for v in _SWEEP]


def build_scene(motion, seed, count=64, **kw):
    """epipolar_ref.scene of a named motion: count correspondences, a tenth of them outliers ('outliers': nothing else)."""
    if motion == "outliers":
        kw = dict(outlier_share=1.0, n=300, **kw)
    else:
        kw = dict(outlier_share=0.1, **kw)
    return er.scene(np.random.default_rng(seed), MOTIONS[motion], W, H, focal=FOCAL, count=count, **kw)


def _subnormal(values):
    return any(v != F(0) and abs(v) < TINY for v in values)


def trace(f, status, intr, u1, v1, u2, v2, **params):
    """The labels of one pair under the intrinsics `intr` (dict fx, fy, cx, cy): f the epipolar record's nine entries, status its
    status, (u1, v1) -> (u2, v2) the inliers' level-0 coordinates, as pose_ref.pose_points takes them.

    e: 'inf' | 'zero' | 'ok' (RP-2's n; 'inf' includes NaN), row: RP-3's i, valid: bit 0 Ra, bit 1 Rb (RP-4), winner: RP-6's k or
    None when no record is written, status: the pose status, few_by: 'inliers' | 'min_good' | None, subnormal: some entry of E
    before or after the division, of t, or of Ra / Rb before the polar steps is non-zero and below 2^-126.  The labels of a
    step that is not reached (and all of them but status when the verifier gave no model) are None; subnormal is False there."""
    p = pr.defaults(**intr, **params)
    out = dict(e=None, row=None, valid=None, winner=None, status=pr.ORB_POSE_NOMODEL, few_by=None, subnormal=False)
    if int(status) not in (pr.ORB_VERIFY_OK, pr.ORB_VERIFY_MINIMAL):
        return out
    k4 = (p["fx"], p["fy"], p["cx"], p["cy"])
    with np.errstate(all="ignore"):
        raw, n = pr.essential_raw(f, *k4)
        out["subnormal"] = _subnormal(raw)
        out["e"] = "inf" if not np.isfinite(n) else "zero" if not n > F(0) else "ok"
        if out["e"] != "ok":
            return out
        e = pr.essential(f, *k4)
        out["row"] = pr.baseline_row(e)[1]
        t = pr.baseline(e)
        out["subnormal"] = out["subnormal"] or _subnormal(e)
        if t is None:  # unreachable for finite input (the module's docstring)
            return out
        ra0, rb0 = pr.rotations_raw(e, t)
        out["subnormal"] = out["subnormal"] or _subnormal(t) or _subnormal(ra0) or _subnormal(rb0)
        (ra, va), (rb, vb) = pr.polar(ra0), pr.polar(rb0)
    out["valid"] = (1 if va else 0) | (2 if vb else 0)
    if not out["valid"]:
        return out
    u1, v1, u2, v2 = (np.asarray(a, dtype=F) for a in (u1, v1, u2, v2))
    if len(u1) < pr.MIN_INLIERS:
        out["status"], out["few_by"] = pr.ORB_POSE_FEW, "inliers"
        return out
    nt = [-v for v in t]
    good, par = [], []
    for r, tk, valid in ((ra, t, va), (ra, nt, va), (rb, t, vb), (rb, nt, vb)):
        _, g, q = pr.triangulate(r, tk, u1, v1, u2, v2, p)
        good.append(int(g.sum()) if valid else -1)
        par.append(int((g & q).sum()))
    k = max(range(4), key=lambda i: (good[i], -i))  # the first of the largest
    second = max([g for i, g in enumerate(good) if i != k] + [0])
    out["winner"] = k
    if good[k] < p["min_good"]:
        out["status"], out["few_by"] = pr.ORB_POSE_FEW, "min_good"
    elif 1000 * second >= p["ambiguity_permille"] * good[k]:
        out["status"] = pr.ORB_POSE_AMBIGUOUS
    elif 2 * par[k] < good[k]:
        out["status"] = pr.ORB_POSE_LOW_PARALLAX
    else:
        out["status"] = pr.ORB_POSE_OK
    return out


def candidate(f, intr, k):
    """Candidate k's (R, t) as float32 arrays, for comparing a written record with trace's winner."""
    with np.errstate(all="ignore"):
        ra, rb, t, _, _ = pr.candidates(f, *(F(intr[n]) for n in ("fx", "fy", "cx", "cy")))
    return np.array(rb if k >> 1 else ra, F), np.array([-v for v in t] if k & 1 else t, F)


def inlier_coordinates(q_corners, t_corners, matches, mask):
    """pose_ref.pose_pair's selection: the level-0 coordinates of the queries whose inlier byte is 1 and of their partners."""
    sel = np.nonzero(np.asarray(mask[:len(q_corners)]) == 1)[0]
    u1, v1 = vr.level0(q_corners[sel])
    u2, v2 = vr.level0(t_corners[matches["index"][sel].astype(np.int64)])
    return u1, v1, u2, v2


def cpu_inputs(scenes, cap=64):
    """What the device holds after injecting scene i into frames (2i, 2i + 1), matching and verify_epipolar(inlier_px=INLIER_PX), by
    the restatements: (corners per frame, matches per pair, (record, inlier bytes) per pair), as test_gpu_pose._inputs returns them.
    The verifier's draws depend on the pair's index, so scene i is verified as pair 2i."""
    corners = [c[:cap] for s in scenes for c in s["corners"]]
    desc = [d[:cap] for s in scenes for d in s["desc"]]
    matches = [C.match_ref(desc[f], desc[f + 1]) for f in range(len(corners) - 1)]
    epi = [er.verify_pair(corners[f], corners[f + 1], matches[f], W, H, f, cap=cap, inlier_px=INLIER_PX) for f in range(len(corners) - 1)]
    return corners, matches, epi


def trace_pair(inputs, pair, intr, **params):
    """trace on pair `pair` of cpu_inputs' (or the device's) inputs."""
    corners, matches, epi = inputs
    rec, mask = epi[pair]
    return trace(rec["h"], rec["status"], intr, *inlier_coordinates(corners[pair], corners[pair + 1], matches[pair], mask), **params)


# ---- the census --------------------------------------------------------------------------------------------------------------
STATUS_NAMES = {pr.ORB_POSE_OK: "OK", pr.ORB_POSE_NOMODEL: "NOMODEL", pr.ORB_POSE_FEW: "FEW", pr.ORB_POSE_AMBIGUOUS: "AMBIGUOUS",
                pr.ORB_POSE_LOW_PARALLAX: "LOW_PARALLAX"}
MIN_SUBNORMAL_MODELS = 8  # (pair, intrinsics) cases with a subnormal intermediate and at least one valid rotation


def census(inputs, sweep=None):
    """trace over every pair of `inputs` under every entry of the sweep: rows[k][f] = the labels of pair f under entry k, with
    `model`: the verifier gave the pair a model (RP-1)."""
    rows = []
    for intr in SWEEP if sweep is None else sweep:
        rows.append([dict(trace_pair(inputs, f, intr), model=int(inputs[2][f][0]["status"]) in (pr.ORB_VERIFY_OK, pr.ORB_VERIFY_MINIMAL))
                     for f in range(len(inputs[2]))])
    return rows


def table(rows):
    """The census as text: one line per label and value with the number of (pair, intrinsics) cases."""
    cases = [c for row in rows for c in row]
    lines = ["%d entries x %d pairs = %d cases" % (len(rows), len(rows[0]), len(cases))]

    def line(name, pred):
        lines.append("  %-34s %6d" % (name, sum(1 for c in cases if pred(c))))

    line("RP-1 no model from the verifier", lambda c: not c["model"])
    for e in ("inf", "zero", "ok"):
        line("RP-2 n " + {"inf": "not finite", "zero": "== 0", "ok": "finite and > 0"}[e], lambda c: c["e"] == e)
    for r in range(3):
        line("RP-3 row %d" % r, lambda c: c["row"] == r)
    for v in range(4):
        line("RP-4 valid %d (n ok)" % v, lambda c: c["e"] == "ok" and c["valid"] == v)
    for k in range(4):
        line("RP-6 winner %d" % k, lambda c: c["winner"] == k)
    for k in range(4):
        line("RP-6 winner %d with status OK" % k, lambda c: c["winner"] == k and c["status"] == pr.ORB_POSE_OK)
    line("RP-6 FEW by min_good", lambda c: c["few_by"] == "min_good")
    line("RP-6 FEW by the inlier count", lambda c: c["few_by"] == "inliers")
    for s, name in sorted(STATUS_NAMES.items()):
        line("status " + name, lambda c: c["status"] == s)
    line("subnormal intermediate", lambda c: c["subnormal"])
    line("subnormal and valid != 0", lambda c: c["subnormal"] and bool(c["valid"]))
    return "\n".join(lines)


def check_census(rows):
    """The coverage both census tests assert.  rows[0] is the default entry."""
    cases = [c for row in rows for c in row]

    def count(pred):
        return sum(1 for c in cases if pred(c))

    ok = pr.ORB_POSE_OK
    first = rows[0]  # DEFAULT and the default parameters
    assert {c["winner"] for c in first if c["status"] == ok} == {0, 1, 2, 3}, "winners with status OK at the default intrinsics"
    assert {c["row"] for c in first if c["model"]} == {0, 1, 2}, "rows of T at the default intrinsics"
    assert {pr.ORB_POSE_AMBIGUOUS, pr.ORB_POSE_LOW_PARALLAX} <= {c["status"] for c in first}, "AMBIGUOUS and LOW_PARALLAX at the default intrinsics"
    assert count(lambda c: not c["model"]) and count(lambda c: c["e"] == "inf") and count(lambda c: c["e"] == "zero")
    for v in range(4):
        assert count(lambda c: c["e"] == "ok" and c["valid"] == v), "valid %d with a finite n > 0" % v
    for k in range(4):
        assert count(lambda c: c["winner"] == k and c["status"] == ok), "winner %d" % k
    for r in range(3):
        assert count(lambda c: c["row"] == r), "row %d" % r
    assert count(lambda c: c["few_by"] == "min_good")
    assert count(lambda c: c["subnormal"] and bool(c["valid"])) >= MIN_SUBNORMAL_MODELS
    # the order: a pair with a model from the verifier and no record under entry k has a written record under entry k - 1
    stale = {"inf": 0, "zero": 0, "valid0": 0}
    for k in range(1, len(rows)):
        for f, c in enumerate(rows[k]):
            if c["model"] and c["winner"] is None:
                assert rows[k - 1][f]["winner"] is not None, "entry %d leaves pair %d without a record, and so does the entry before it" % (k, f)
                stale[c["e"] if c["e"] != "ok" else "valid0"] += 1
    assert all(stale.values()), stale
