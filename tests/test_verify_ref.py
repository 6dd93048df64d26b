"""Known answers for the CPU restatement of the geometric verifier (tests/verify_ref.py, GV-1..GV-7 of DESIGN.md section 13), and the
checks of its C ABI that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import verify_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
W, H = 640, 480
H_TRUE = np.array([[1.04, 0.03, 12.0], [-0.02, 0.97, -7.5], [2e-5, -3e-5, 1.0]])


def _apply(Hm, x, y):
    p = Hm @ np.stack([x, y, np.ones_like(x)])
    return p[0] / p[2], p[1] / p[2]


def _scene(n=400, outliers=0.4, seed=1):
    """Noise-free correspondences of H_TRUE on a pixel grid, a share of them replaced by random outliers."""
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(20, W - 20, n).astype(np.float32)
    y0 = rng.uniform(20, H - 20, n).astype(np.float32)
    x1, y1 = _apply(H_TRUE, x0.astype(np.float64), y0.astype(np.float64))
    out = rng.random(n) < outliers
    x1[out] = rng.uniform(0, W, out.sum())
    y1[out] = rng.uniform(0, H, out.sum())
    return x0, y0, x1.astype(np.float32), y1.astype(np.float32), ~out


def _corners_err(Ha, Hb):
    cx = np.array([0.0, W - 1, W - 1, 0.0])
    cy = np.array([0.0, 0.0, H - 1, H - 1])
    ax, ay = _apply(Ha, cx, cy)
    bx, by = _apply(Hb, cx, cy)
    return float(np.max(np.hypot(ax - bx, ay - by)))


def test_known_homography_with_outliers():
    x0, y0, x1, y1, good = _scene()
    rec, inl = vr.verify_points(x0, y0, x1, y1, W, H, inlier_px=1.0)
    assert rec["status"] == vr.VERIFY_OK and rec["candidates"] == len(x0)
    assert rec["h"][8] == 1.0
    assert _corners_err(rec["h"].astype(np.float64).reshape(3, 3), H_TRUE) < 1e-2
    # the outliers are uniform over the frame: one in a few thousand lands within 1 px of its true image
    x1t, y1t = _apply(H_TRUE, x0.astype(np.float64), y0.astype(np.float64))
    near = np.hypot(x1 - x1t, y1 - y1t) < 0.5
    assert np.array_equal(inl, near) and good.sum() == near.sum() - (near & ~good).sum()
    assert rec["inliers"] == inl.sum()


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_refit_agrees_with_double_least_squares(seed):
    """Correspondences rounded to the pixel grid (up to 0.7 px off the model): the binary32 normal equations, summed and
    eliminated in GV-6's order, against a float64 least-squares solve of the same inlier set.  They agree to about 0.02 px at the
    image corners (the conditioning of binary32 normal equations); the model itself is 0.1-0.2 px off the true H."""
    x0, y0, x1, y1, good = _scene(seed=seed)
    x0, y0, x1, y1 = (np.round(a).astype(np.float32) for a in (x0, y0, x1, y1))
    rec, inl = vr.verify_points(x0, y0, x1, y1, W, H, inlier_px=2.0)
    assert rec["status"] == vr.VERIFY_OK and np.array_equal(inl, good)
    X, Y, U, V = (a[inl].astype(np.float64) for a in (x0, y0, x1, y1))
    A = np.zeros((2 * len(X), 8))
    A[0::2, 0], A[0::2, 1], A[0::2, 2], A[0::2, 6], A[0::2, 7] = X, Y, 1, -X * U, -Y * U
    A[1::2, 3], A[1::2, 4], A[1::2, 5], A[1::2, 6], A[1::2, 7] = X, Y, 1, -X * V, -Y * V
    b = np.empty(2 * len(X))
    b[0::2], b[1::2] = U, V
    h = np.linalg.lstsq(A, b, rcond=None)[0]
    ref = np.append(h, 1.0).reshape(3, 3)
    assert _corners_err(rec["h"].astype(np.float64).reshape(3, 3), ref) < 0.05
    assert _corners_err(rec["h"].astype(np.float64).reshape(3, 3), H_TRUE) < 0.5


def test_few_and_degenerate():
    x = np.array([10, 200, 300], np.float32)
    rec, inl = vr.verify_points(x, x, x, x, W, H)
    assert rec["status"] == vr.VERIFY_FEW and rec["hypothesis"] == 0xFFFFFFFF and not inl.any()
    assert rec["candidates"] == 3 and not rec["h"].any()
    t = np.arange(50, dtype=np.float32)
    rec, inl = vr.verify_points(10 + 5 * t, 20 + 3 * t, 14 + 5 * t, 25 + 3 * t, W, H)  # collinear
    assert rec["status"] == vr.VERIFY_DEGENERATE and rec["hypothesis"] == 0xFFFFFFFF and rec["inliers"] == 0 and not inl.any()
    same = np.full(50, 100, np.float32)
    rec, _ = vr.verify_points(same, same, same + 3, same, W, H)  # all identical
    assert rec["status"] == vr.VERIFY_DEGENERATE


def test_single_hypothesis():
    x0, y0, x1, y1, _ = _scene(n=60, seed=3)
    for seed in range(20):
        rec, _ = vr.verify_points(x0, y0, x1, y1, W, H, hypotheses=1, seed=seed)
        assert rec["hypothesis"] in (0, 0xFFFFFFFF)


def test_seed_changes_the_draws():
    J0, ok0 = vr.sample(7, 3, 500, 512)
    J1, ok1 = vr.sample(7, 3, 500, 512)
    J2, _ = vr.sample(8, 3, 500, 512)
    J3, _ = vr.sample(7, 4, 500, 512)
    assert np.array_equal(J0, J1) and np.array_equal(ok0, ok1)
    assert not np.array_equal(J0, J2) and not np.array_equal(J0, J3)
    assert ok0.all() and (J0 < 500).all()
    assert all(len(set(r)) == 4 for r in J0.tolist())
    _, ok = vr.sample(0, 0, 4, 4096)  # four candidates: some hypotheses do not find all four within 16 draws
    assert 0 < ok.sum() < 4096


def test_lowbias32_known_values():
    # lowbias32 by its definition, in Python integers
    def ref(x):
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = [0, 1, 2, 12345, 0xDEADBEEF, 0xFFFFFFFF]
    assert vr.lowbias32(np.array(xs, np.uint32)).tolist() == [ref(x) for x in xs]


def test_candidate_filter():
    from tinyslam_amd import orb
    m = np.zeros(6, dtype=orb.MATCH_DTYPE)
    m["index"] = [0, 1, orb.ORB_MATCH_NONE, 9, 2, 3]
    m["distance"] = [10, 65, 0, 5, 40, 50]
    m["second"] = [30, 200, 0xFFFF, 100, 50, 62]
    assert vr.candidates(m, 5, 64, np.float32(0.8)).tolist() == [0]  # 40 < 0.8 * 50 is false; 50 < 49.6 is false
    assert vr.candidates(m, 5, 256, np.float32(1.0)).tolist() == [0, 1, 4, 5]


def test_abi_without_device(tinyorb):
    L = tinyorb.load_library()
    prm = tinyorb._VerifyParams()
    assert L.orb_verify_consecutive(None, 2, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_consecutive(None, 2, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert ctypes.sizeof(tinyorb._VerifyParams) == 32 and tinyorb.VERIFY_MODEL_DTYPE.itemsize == 64
    assert [getattr(tinyorb._VerifyParams, k).offset for k in ("hypotheses", "max_distance", "ratio", "inlier_px", "seed", "reserved")] == \
        [0, 4, 8, 12, 16, 20]
    assert [tinyorb.VERIFY_MODEL_DTYPE.fields[k][1] for k in ("h", "candidates", "inliers", "hypothesis", "status", "reserved")] == \
        [0, 36, 40, 44, 48, 52]
    text = open(HEADER).read()
    fields = re.search(r"typedef struct \{([^}]*)\} OrbVerifyParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(?:u?int32_t|float)\s+(\w+)", fields, re.M) == ["hypotheses", "max_distance", "ratio", "inlier_px", "seed", "reserved"]
    fields = re.search(r"typedef struct \{([^}]*)\} OrbPairModel;", text, re.S).group(1)
    assert re.findall(r"^\s*(?:u?int32_t|float)\s+(\w+)", fields, re.M) == ["h", "candidates", "inliers", "hypothesis", "status", "reserved"]
    consts = dict(re.findall(r"#define\s+(ORB_VERIFY_[A-Z_]+)\s+(\d+)u?\b", text))
    for k in ("ORB_VERIFY_OK", "ORB_VERIFY_FEW", "ORB_VERIFY_DEGENERATE", "ORB_VERIFY_MINIMAL"):
        assert int(consts[k]) == getattr(tinyorb, k) == getattr(vr, k[4:])
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert names[-3:] == ["k_verify_gather", "k_verify_score", "k_verify_refine"] and L.orb_kernel_name(25) == b""
