"""The CPU restatement of the epipolar verifier (tests/epipolar_ref.py, EP-1..EP-6 of DESIGN.md section 16) on constructed two-view
scenes with depth, its status cases and sampling, and the checks of its C ABI that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import constructed as C
import epipolar_ref as er
import verify_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
W, H = 640, 480
SCENE_SEED = 1


def _run_scene(motion, seed=SCENE_SEED):
    s = er.scene(np.random.default_rng(seed), motion, W, H)
    m = C.match_ref(s["desc"][0], s["desc"][1])
    rec, mask = er.verify_pair(s["corners"][0], s["corners"][1], m, W, H, 0, inlier_px=2.0)
    hrec, hmask = vr.verify_pair(s["corners"][0], s["corners"][1], m, W, H, 0, inlier_px=2.0)
    return s, m, rec, mask.astype(bool), hmask.astype(bool)


@pytest.mark.parametrize("motion", ["sideways", "yaw", "forward"])
def test_ground_truth_scenes(motion):
    """f = 500 px, 640 x 480, depths inverse-uniform in [2, 12] m, about 600 points, 30 % outliers at random pixels, inlier_px = 2:
    the restatement keeps at least 0.95 of the correct correspondences (planted ones, and outliers within 2 px Sampson distance
    of the true F), accepts at most 5 % of the other outliers, and the homography restatement on the same records keeps fewer
    than half of the correct ones."""
    s, m, rec, mask, hmask = _run_scene(motion)
    # the construction: every planted query's brute-force match is its partner at distance 0, so every query is a candidate
    assert (m["distance"] == 0).all() and rec["candidates"] == len(m)
    correct = s["correct"]
    recall, false_share, h_recall = mask[correct].mean(), mask[~correct].mean(), hmask[correct].mean()
    print(motion, len(m), int(correct.sum()), "recall %.4f false %.4f homography %.4f" % (recall, false_share, h_recall))
    assert rec["status"] == er.VERIFY_OK, rec
    assert recall >= 0.95
    assert false_share <= 0.05
    assert h_recall < 0.5


def test_sideways_recovers_true_f():
    """Case (a), R = I and t along x: the normalised F33 is 0, so a model that fixed F33 = 1 could not represent it.  The record's
    F, taken to GV-2's normalised coordinates and scaled to unit Frobenius norm (sign aligned), lies within 0.1 of the true F.

    The bound: the records are the projections rounded to whole pixels (up to 0.5 px per coordinate) and the inliers include
    outliers that happen to lie within 2 px of the true epipolar lines, so even an exact solve is off the truth; a float64 SVD
    of the same scenes' accepted inliers (seeds 1-5) is 0.00-0.05 from it.  0.1 leaves twice that for binary32."""
    cx, cy, k = (float(v) for v in vr.normalise(W, H))
    T = np.array([[k, 0, -cx * k], [0, k, -cy * k], [0, 0, 1]])
    Ti = np.linalg.inv(T)

    def unit(Fm):
        Fn = Ti.T @ Fm @ Ti
        return Fn / np.linalg.norm(Fn)

    s, _, rec, _, _ = _run_scene("sideways")
    truth = unit(s["F"])
    assert abs(truth[2, 2]) < 1e-12
    got = unit(rec["h"].astype(np.float64).reshape(3, 3))
    err = min(np.linalg.norm(got - truth), np.linalg.norm(got + truth))
    print("relative error %.4f, normalised F33 %.2e" % (err, got[2, 2]))
    assert err < 0.1
    assert np.max(np.abs(rec["h"])) == 1.0 and rec["h"][np.argmax(np.abs(rec["h"]))] == 1.0


def test_seven_candidates_are_few():
    rng = np.random.default_rng(3)
    x0 = rng.uniform(0, W, 8).astype(np.float32)
    y0 = rng.uniform(0, H, 8).astype(np.float32)
    rec, mask = er.verify_points(x0[:7], y0[:7], x0[:7] + 3, y0[:7], W, H)
    assert rec["status"] == er.VERIFY_FEW and rec["candidates"] == 7 and rec["hypothesis"] == 0xFFFFFFFF
    assert not mask.any() and not rec["h"].any() and rec["inliers"] == 0
    rec, _ = er.verify_points(x0, y0, x0 + 3 + (x0 > 300), y0, W, H)
    assert rec["status"] != er.VERIFY_FEW and rec["candidates"] == 8


@pytest.mark.parametrize("kind", ["coincident", "collinear", "slanted", "two_points"])
def test_degenerate_correspondences(kind):
    """Eight or more coincident or collinear correspondences: every sample is degenerate (a zero pivot, or a last pivot at most
    2^-20 of the first)."""
    n = 40
    i = np.arange(n, dtype=np.float32)
    if kind == "coincident":
        x0, y0, x1, y1 = np.full(n, 100.0), np.full(n, 200.0), np.full(n, 105.0), np.full(n, 201.0)
    elif kind == "collinear":  # constructed.collinear's layout: one row, translated along it
        x0, y0 = 10 + 3 * i, np.full(n, H // 2)
        x1, y1 = x0 + 4, y0
    elif kind == "slanted":
        x0, y0 = 10 + 7 * i, 20 + 5 * i
        x1, y1 = x0 + 3, y0 - 2
    else:
        x0 = np.where(i < n // 2, 100.0, 300.0)
        y0 = np.where(i < n // 2, 200.0, 50.0)
        x1, y1 = x0 + 5, y0 + 1
    for hyps in (1, 512, 4096):
        rec, mask = er.verify_points(x0, y0, x1, y1, W, H, hypotheses=hyps)
        assert rec["status"] == er.VERIFY_DEGENERATE and rec["hypothesis"] == 0xFFFFFFFF, (kind, hyps, rec)
        assert not mask.any() and not rec["h"].any()


def test_sampling_is_deterministic_and_its_own():
    """EP-2: the same (seed, pair, h) draws the same eight distinct indices; the stream differs from GV-3's."""
    for seed, pair, M in ((0, 0, 100), (7, 3, 5000), (0x9E3779B9, 254, 8)):
        J, ok = er.sample(seed, pair, M, 4096)
        J2, ok2 = er.sample(seed, pair, M, 4096)
        assert np.array_equal(J, J2) and np.array_equal(ok, ok2)
        assert ok.mean() > (0.5 if M == 8 else 0.99)
        Jv = J[ok]
        assert (np.sort(Jv, 1)[:, 1:] != np.sort(Jv, 1)[:, :-1]).all() and Jv.max() < M
        G, gok = vr.sample(seed, pair, M, 4096)
        both = ok & gok
        same = (J[both][:, :4] == G[both]).all(1)
        assert same.mean() < (0.2 if M == 8 else 0.01), (seed, pair, M, same.mean())
    # other pairs and seeds give other samples
    a, _ = er.sample(5, 0, 1000, 64)
    assert (a != er.sample(5, 1, 1000, 64)[0]).any(1).mean() > 0.9
    assert (a != er.sample(6, 0, 1000, 64)[0]).any(1).mean() > 0.9


def test_null_vector_of_an_exact_sample():
    """EP-3 on an exact eight-point sample of a known F: the null vector is F divided by its largest entry."""
    s = er.scene(np.random.default_rng(11), "forward", W, H, outlier_share=0.0)
    cx, cy, k = vr.normalise(W, H)
    x0, y0 = vr.level0(s["corners"][0][:8])
    m = C.match_ref(s["desc"][0], s["desc"][1])
    x1, y1 = vr.level0(s["corners"][1][m["index"][:8].astype(np.int64)])
    rec = np.stack([(x0 - cx) * k, (y0 - cy) * k, (x1 - cx) * k, (y1 - cy) * k], 1).astype(np.float32)
    Fs, ms, ok = er.null_vectors(er.design_rows(rec)[None])
    assert ok[0] and Fs[0, ms[0]] == 1.0 and np.abs(Fs[0]).max() == 1.0
    A = er.design_rows(rec).astype(np.float64)
    assert np.abs(A @ Fs[0].astype(np.float64)).max() < 1e-4


# ---- C ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_reuses_the_verify_structs():
    text = open(HEADER).read()
    sigs = re.findall(r"^int (orb_verify_epipolar\w*)\(([^)]*)\);", text, re.M)
    assert dict(sigs) == {"orb_verify_epipolar": "OrbProgram *p, uint32_t n_frames, const OrbVerifyParams *params, void *stream",
                          "orb_verify_epipolar_read": "OrbProgram *p, uint32_t pair, OrbPairModel *model, uint8_t *inlier, size_t n"}
    assert not re.search(r"\}\s*Orb\w*Epi\w*;", text), "no struct of its own"
    assert int(re.search(r"#define TINYORB_ABI_VERSION (\d+)", text).group(1)) == 5
    assert int(re.search(r"#define ORB_KERNEL_COUNT (\d+)", text).group(1)) == 25


def test_abi_exports_and_null_program(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_verify_epipolar", "orb_verify_epipolar_read"):
        assert n in tinyorb.EXPORTS
        assert hasattr(L, n)
    prm = tinyorb._VerifyParams()
    assert L.orb_verify_epipolar(None, 2, ctypes.byref(prm), None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_epipolar(None, 2, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_verify_epipolar_read(None, 0, None, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("epi" in n for n in names)
