"""Labelled inputs of the epipolar verifier, for the CPU restatement and for the device (test infrastructure, not a test file).

The refit of EP-5 fixes entry m of F at 1, m the minimal model's entry of largest magnitude, and the kernels depend on m in three
places (epi_accumulate, EpipolarModel::from_solution, epi_null).  The constructed scenes of tests/test_gpu_epipolar.py reach m = 5
and 3 only, and no test says which m its extracted frames reach.  Here every case is an epipolar_ref.scene whose camera motion decides which entry of the normalised F is the largest, so that the
nine entries, both causes of ORB_VERIFY_MINIMAL and the smallest candidate counts are each met by a case that says so.

Which entry is largest.  E = [t]x R, and GV-2's coordinates divide an entry by f' = 2 focal / max(W, H) = 1.5625 once for each of its
row and column below 2.  A motion and its reverse give transposed F, so a pure translation (or one with a rotation about its own
axis) ties an entry with its transpose; the motions below break each tie by a rotation that shortens one of the two:

    t along z, R = Ry(32):            F[1] = -tz / f'^2, F[3] = tz cos 32 / f'^2                       m = 1; reversed: 3
    t along z, R = Ry(32) Rz(90):     F[0] = -tz / f'^2, F[4] = -tz cos 32 / f'^2                      m = 0
    t along z, R = Rz(90) Ry(32):     F[0] = -tz cos 32 / f'^2, F[4] = -tz / f'^2                      m = 4
    t along y, R = Rz(40):            F[2] = ty / f', F[6] = -ty cos 40 / f', F[7] = ty sin 40 / f'    m = 2; reversed: 6
    t along x, R = Rz(40):            F[5] = -tx / f', F[7] = tx cos 40 / f', F[6] = tx sin 40 / f'    m = 5; reversed: 7
    t along x, R = Rx(40):            F[8] = -tx sin 40, -F[5] = F[7] = tx cos 40 / f'                 m = 8

The largest entry leads the next by 1 / cos 32 = 1.18 or more, which the minimal model of the best of 256 samples does not overturn
(12 scene seeds of every motion, forward and backward, gave the same m).  A reversed case stores the scene's second frame first.
The matcher's backward rows are the forward ones inverted (every descriptor sits once in each frame), so the backward listing of a
case is its reversed motion under another draw stream: m is transposed there (1 <-> 3, 2 <-> 6, 5 <-> 7; 0, 4 and 8 stay).

Case i lies in frames 2 i and 2 i + 1 of one batch, so its pair is 2 i for orb_verify_epipolar, and list entry 2 i (forward) and
2 i + 1 (backward) of `pairs()` for orb_verify_pairs: the draw stream of EP-2 takes the pair, and a label holds at that pair under
the case's own parameter set only.  Every label was read once from epipolar_ref's trace and written down here;
tests/test_epipolar_cases_ref.py holds the restatement to each of them, tests/test_gpu_epipolar_cases.py the device.
"""
import numpy as np

import constructed as C
import epipolar_ref as er

W, H, FOCAL, CAP = 640, 480, 500.0, 1024
OK, MINIMAL = er.VERIFY_OK, er.VERIFY_MINIMAL
TRANSPOSED = (0, 3, 6, 1, 4, 7, 2, 5, 8)  # entry e of F is entry TRANSPOSED[e] of its transpose

# A call's parameters are the whole batch's: the cases are grouped by these sets.
#   ok     the refit replaces the minimal model (DESIGN.md section 16's constructed scenes: 2 px)
#   rule   a tight threshold and 8 hypotheses: some winners' refits keep fewer than 15/16 of the minimal model's inliers
#   solve  t2 = (1e-30 k)^2 underflows to 0: no candidate is an inlier of anything, the winner is the first valid hypothesis, all 44
#          sums are 0 and GV-6's solver meets a zero pivot
#   tiny   512 hypotheses: at M = 8 and 9 many of them draw no eight distinct indices in 32 draws (EP-2), so valid and invalid
#          lanes share a 64-hypothesis workgroup; seed 21 makes hypotheses 0 and 1 of the M = 8 case's pair invalid ones
PARAMS = {
    "ok": dict(inlier_px=2.0, hypotheses=256, seed=0),
    "rule": dict(inlier_px=0.25, hypotheses=8, seed=0),
    "solve": dict(inlier_px=1e-30, hypotheses=64, seed=0),
    "tiny": dict(inlier_px=2.0, hypotheses=512, seed=21),
}

TZ, TY, TX = (0.0, 0.0, 0.3), (0.0, 0.25, 0.0), (0.25, 0.0, 0.0)


def _case(name, rot, t, params="ok", reverse=False, seed=None, n=300, count=None, motion=None, **label):
    return dict(name=name, rot=rot, t=t, motion=motion, params=params, reverse=reverse, seed=seed, n=n, count=count, label=label)


# rot: rotations about the named axes, multiplied left to right; seed: the scene's (None: 1 + i, so that no two scenes share a
# descriptor); label: what the trace gives at pair 2 i under PARAMS[params]
# (m_back: m of the backward listing at list entry 2 i + 1, where the construction implies it)
CASES = [
    # one case per fixed entry, status OK
    _case("m0", [("y", 32), ("z", 90)], TZ,
          status=OK, m=0, m_back=0, fit=True, candidates=191, n_min=137, n_fit=137, inliers=137, hypothesis=216, unpivoted=0, pixel_m=8),
    _case("m1", [("y", 32)], TZ,
          status=OK, m=1, m_back=3, fit=True, candidates=247, n_min=175, n_fit=176, inliers=176, hypothesis=193, unpivoted=3, pixel_m=8),
    _case("m2", [("z", 40)], TY,
          status=OK, m=2, m_back=6, fit=True, candidates=337, n_min=237, n_fit=237, inliers=237, hypothesis=71, unpivoted=2, pixel_m=8),
    _case("m3", [("y", 32)], TZ, reverse=True,
          status=OK, m=3, m_back=1, fit=True, candidates=206, n_min=145, n_fit=145, inliers=145, hypothesis=176, unpivoted=7, pixel_m=8),
    _case("m4", [("z", 90), ("y", 32)], TZ,
          status=OK, m=4, m_back=4, fit=True, candidates=197, n_min=140, n_fit=140, inliers=140, hypothesis=190, unpivoted=0, pixel_m=8),
    _case("m5", [("z", 40)], TX,
          status=OK, m=5, m_back=7, fit=True, candidates=331, n_min=233, n_fit=233, inliers=233, hypothesis=193, unpivoted=7, pixel_m=8),
    _case("m6", [("z", 40)], TY, reverse=True,
          status=OK, m=6, m_back=2, fit=True, candidates=359, n_min=254, n_fit=253, inliers=253, hypothesis=69, unpivoted=2, pixel_m=8),
    _case("m7", [("z", 40)], TX, reverse=True,
          status=OK, m=7, m_back=5, fit=True, candidates=363, n_min=254, n_fit=255, inliers=255, hypothesis=37, unpivoted=7, pixel_m=8),
    _case("m8", [("x", 40)], TX, n=600,  # 40 degrees of pitch leave a strip of the view: 600 points for 187 candidates
          status=OK, m=8, m_back=8, fit=True, candidates=187, n_min=132, n_fit=132, inliers=132, hypothesis=13, unpivoted=7, pixel_m=8),
    # a pure translation: F[2] and F[6] tie, so m is this seed's (no m_back); the pixel F has no dominant last entry: EP-6 divides by
    # entry 2
    _case("translation_y", [], TY,
          status=OK, m=2, fit=True, candidates=397, n_min=278, n_fit=278, inliers=278, hypothesis=34, unpivoted=6, pixel_m=2),
    # the refit's 256 partial sums one short of a pass, one pass, one past it
    _case("m2_255", [("z", 40)], TY, count=255,
          status=OK, m=2, m_back=6, fit=True, candidates=255, n_min=176, n_fit=176, inliers=176, hypothesis=218, unpivoted=6, pixel_m=8),
    _case("m2_256", [("z", 40)], TY, count=256,
          status=OK, m=2, m_back=6, fit=True, candidates=256, n_min=178, n_fit=177, inliers=177, hypothesis=186, unpivoted=6, pixel_m=8),
    _case("m2_257", [("z", 40)], TY, count=257,
          status=OK, m=2, m_back=6, fit=True, candidates=257, n_min=180, n_fit=180, inliers=180, hypothesis=111, unpivoted=2, pixel_m=8),
    # MINIMAL by the 15/16 rule: scene_motion("forward"), the first of the scene seeds 100 .. 179 that ends so at pair 26
    # (16 * 57 = 912 < 915 = 15 * 61; 7 of 240 draws over the three named motions did)
    _case("minimal_rule", None, None, motion="forward", params="rule", seed=146, n=200,
          status=MINIMAL, m=3, fit=True, candidates=276, n_min=61, n_fit=57, inliers=61, hypothesis=4, unpivoted=1, pixel_m=8),
    # MINIMAL by a failed solve
    _case("minimal_solve", [("y", 32)], TZ, params="solve", n=100,
          status=MINIMAL, m=3, fit=False, candidates=80, n_min=0, n_fit=0, inliers=0, hypothesis=0, unpivoted=3, pixel_m=8),
    # M = 8: every valid hypothesis is the same eight candidates, all of them its inliers, so the lowest valid h wins the tie: 2
    _case("tiny_8", [("z", 40)], TX, params="tiny", count=8,
          status=OK, m=4, fit=True, candidates=8, n_min=8, n_fit=8, inliers=8, hypothesis=2, unpivoted=4, pixel_m=8, sampled=454, valid=454),
    _case("tiny_9", [("z", 40)], TX, params="tiny", count=9,
          status=OK, m=4, fit=True, candidates=9, n_min=8, n_fit=8, inliers=8, hypothesis=0, unpivoted=4, pixel_m=8, sampled=507, valid=507),
]


def rotation(rot):
    R = np.eye(3)
    for ax, deg in rot:
        a = np.radians(deg)
        c, s = np.cos(a), np.sin(a)
        R = R @ {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
                 "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])}[ax]
    return R


_cache = {}


def frames(i):
    """(corners, descriptors) of case i's two frames, in batch order (a reversed case: the scene's second frame first)."""
    if i not in _cache:
        c = CASES[i]
        motion = c["motion"] or (rotation(c["rot"]), np.array(c["t"], np.float64))
        s = er.scene(np.random.default_rng(1 + i if c["seed"] is None else c["seed"]), motion, W, H, focal=FOCAL, n=c["n"], count=c["count"])
        o = slice(None, None, -1) if c["reverse"] else slice(None)
        _cache[i] = (s["corners"][o], s["desc"][o])
    return _cache[i]


def batch():
    """(raw counters, corners, descriptors) of the 2 len(CASES) frames."""
    corners, desc = [], []
    for i in range(len(CASES)):
        c, d = frames(i)
        corners += c
        desc += d
    return np.array([len(c) for c in corners], np.uint32), corners, desc


def pairs():
    """Every case forward and backward: entries 2 i and 2 i + 1."""
    return [p for i in range(len(CASES)) for p in ((2 * i, 2 * i + 1), (2 * i + 1, 2 * i))]


def traced(i, backward=False, params=None):
    """The restatement on case i at its own pair (backward: list entry 2 i + 1) under its own parameter set, or `params`.
    Returns (record, CAP inlier bytes, trace)."""
    c, d = frames(i)
    q, t = (1, 0) if backward else (0, 1)
    trace = {}
    rec, mask = er.verify_pair(c[q], c[t], C.match_ref(d[q], d[t]), W, H, 2 * i + int(backward), cap=CAP, trace=trace,
                               **(PARAMS[CASES[i]["params"]] if params is None else params))
    return rec, mask, trace


def label_of(rec, trace):
    """What a label may state, from a record and its trace."""
    out = {k: int(rec[k]) for k in ("status", "candidates", "inliers", "hypothesis")}
    out.update({k: trace[k] for k in ("m", "fit", "n_min", "n_fit", "sampled", "valid", "unpivoted", "pixel_m")})
    return out
