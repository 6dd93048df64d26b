"""Geometric verification of consecutive-frame matches on the GPU (orb_verify_consecutive): every record and
inlier byte against the CPU restatement (tests/verify_ref.py), the recovered homography against known warps, the call's state
rules and its stream ordering."""
import numpy as np
import pytest

import constructed as C
import verify_ref as vr

pytestmark = pytest.mark.gpu

THR = 20.0 / 255.0


def _program(tinyorb, W, H, cap, max_batch, flags=0, depth=2):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR,
                            max_batch=max_batch, flags=flags, fast_arc=9 if flags & tinyorb.ORB_FLAG_INTENDED else 0)
    return tinyorb.OrbProgram(cfg).init()


def _view(scene, G, W, H):
    """Nearest-neighbour inverse mapping: view pixel (x, y) shows scene pixel round(G (x, y, 1)) of the view-sized window at the
    scene's centre (image rows, row 0 at the top)."""
    Hs, Ws = scene.shape[:2]
    G = np.array([[1, 0, (Ws - W) / 2], [0, 1, (Hs - H) / 2], [0, 0, 1]]) @ G  # centred in the scene
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    p = np.einsum("ij,jhw->ihw", G, np.stack([x, y, np.ones_like(x)]))
    sx = np.floor(p[0] / p[2] + 0.5).astype(np.int64)
    sy = np.floor(p[1] / p[2] + 0.5).astype(np.int64)
    ok = (sx >= 0) & (sx < Ws) & (sy >= 0) & (sy < Hs)
    out = np.zeros((H, W, 4), np.uint8)
    out[ok] = scene[sy[ok], sx[ok]]
    out[..., 3] = 255
    return out


def _warp(dx=0.0, dy=0.0, scale=1.0, angle_deg=0.0, px=0.0, py=0.0, W=640, H=480):
    """View-to-scene map: a similarity about the view's centre followed by a mild perspective term, then a shift."""
    c, s = np.cos(np.radians(angle_deg)) * scale, np.sin(np.radians(angle_deg)) * scale
    C = np.array([[1, 0, W / 2], [0, 1, H / 2], [0, 0, 1]])
    Ci = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]])
    A = np.array([[c, -s, dx], [s, c, dy], [px, py, 1.0]])
    return C @ A @ Ci


def _truth(Ga, Gb, H, mirrored):
    """Keypoint coordinates of view a -> view b; the literal mode's keypoints live in the mirrored frame y -> H - 1 - y."""
    T = np.linalg.inv(Gb) @ Ga
    if mirrored:
        Fm = np.array([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]], dtype=np.float64)
        T = Fm @ T @ Fm
    return T / T[2, 2]


def _corner_err(Ha, Hb, W, H):
    cx = np.array([0.0, W - 1, W - 1, 0.0])
    cy = np.array([0.0, 0.0, H - 1, H - 1])
    pa = Ha @ np.stack([cx, cy, np.ones(4)])
    pb = Hb @ np.stack([cx, cy, np.ones(4)])
    return float(np.max(np.hypot(pa[0] / pa[2] - pb[0] / pb[2], pa[1] / pa[2] - pb[1] / pb[2])))


def _check_parity(prog, n_frames, W, H, cap, **params):
    """Verifies the first n_frames of the last match and compares every pair's record and cap inlier bytes with the restatement."""
    counts = np.minimum(prog.batch_counts(n_frames), cap)
    corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(n_frames)]
    prog.verify_consecutive(n_frames, **params)
    recs = []
    for f in range(n_frames - 1):
        matches = prog.match_read(f, int(counts[f]))
        rec, mask = prog.verify_read(f, cap)
        ref, rmask = vr.verify_pair(corners[f], corners[f + 1], matches, W, H, f, cap=cap, **params)
        assert rec.tobytes() == ref.tobytes(), (f, params, rec, ref)
        assert np.array_equal(mask, rmask), (f, params)
        recs.append(rec)
    return recs


def _parity_frames(oracle, W, H):
    scene = oracle.synth_frame(W + 40, H + 40, 300)
    G0 = _warp(W=W, H=H)
    views = [_view(scene, G0, W, H), _view(scene, _warp(3, 2, W=W, H=H), W, H),
             _view(scene, _warp(8, 6, 1.04, 0, 4e-5, -3e-5, W=W, H=H), W, H), np.zeros((H, W, 4), np.uint8)]
    blob = np.zeros((H, W, 4), np.uint8)
    blob[100:103, 150:153] = 255
    blob2 = np.zeros((H, W, 4), np.uint8)
    blob2[101:104, 152:155] = 255
    return np.stack(views + [blob, blob2])


@pytest.mark.parametrize("intended", [False, True], ids=["literal", "intended"])
def test_parity_bit_for_bit(tinyorb, oracle, intended):
    W, H = 320, 240
    frames = _parity_frames(oracle, W, H)
    flags = tinyorb.ORB_FLAG_INTENDED if intended else 0
    statuses = set()
    for cap in (1200, 150):  # the second cuts the frames at their capacity
        with _program(tinyorb, W, H, cap, len(frames), flags) as prog:
            prog.extract_batch_host(frames)
            prog.match_consecutive(len(frames))
            for hyps in (1, 100, 512, 4096):
                for seed in (0, 0x9E3779B9):
                    recs = _check_parity(prog, len(frames), W, H, cap, hypotheses=hyps, seed=seed)
                    statuses |= {int(r["status"]) for r in recs}
            recs = _check_parity(prog, len(frames), W, H, cap, ratio=1.0, max_distance=256, inlier_px=1.5, seed=5)
            statuses |= {int(r["status"]) for r in recs}
            if cap == 1200 and intended:  # (the literal descriptors change under translation: few true matches, see below)
                assert recs[0]["status"] in (tinyorb.ORB_VERIFY_OK, tinyorb.ORB_VERIFY_MINIMAL) and recs[0]["inliers"] > 50
    assert tinyorb.ORB_VERIFY_FEW in statuses and tinyorb.ORB_VERIFY_OK in statuses


def test_ground_truth_homography(tinyorb, oracle):
    """The intended mode (no vertical mirror, rotation-invariant descriptors): translations, +-5 % scale, mild perspective and
    rotations of +-10 degrees are recovered by the refit (status OK) within 1 px at the image corners.

    The stored keypoint order of the intended mode is the order of the detector's atomic appends, so it changes from run to run,
    and with it the candidate list, the samples and the winner.  The bound must hold for every order: besides the GPU's own
    order, the restatement verifies each pair again in shuffled orders.  Observed over 12 orders per pair on the CPU: status OK in
    all 72, worst corner error 0.30 px.  (The literal mode is checked for parity only: its descriptors change under translation on these frames --
    corresponding keypoints of two shifted views differ in a median 126 of 256 bits -- so its matches hold too few true
    correspondences to pin a model.)"""
    W, H, cap = 640, 480, 4096
    scene = oracle.synth_frame(W + 120, H + 120, 77)
    motions = [dict(), dict(dx=6, dy=-4), dict(dx=-5, dy=3, scale=1.05), dict(dx=2, dy=2, scale=0.97, px=3e-5, py=-2e-5),
               dict(dx=-3, dy=5, px=-4e-5, py=3e-5), dict(angle_deg=10), dict(angle_deg=-10, dx=4)]
    Gs = [_warp(W=W, H=H, **m) for m in motions]
    frames = np.stack([_view(scene, G, W, H) for G in Gs])
    rng = np.random.default_rng(5)

    def check(f, rec, order):
        assert rec["status"] == tinyorb.ORB_VERIFY_OK, (f, order, rec)
        truth = _truth(Gs[f], Gs[f + 1], H, mirrored=False)
        err = _corner_err(rec["h"].astype(np.float64).reshape(3, 3), truth, W, H)
        assert err < 1.0, (f, order, motions[f + 1], err, rec)
        assert rec["inliers"] >= 0.5 * rec["candidates"], (f, order, rec)

    with _program(tinyorb, W, H, cap, len(frames), tinyorb.ORB_FLAG_INTENDED) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(len(frames))
        recs = _check_parity(prog, len(frames), W, H, cap, inlier_px=2.0)
        counts = np.minimum(prog.batch_counts(len(frames)), cap)
        corners = [prog.batch_read(f, int(counts[f]))[0] for f in range(len(frames))]
        matches = [prog.match_read(f, int(counts[f])) for f in range(len(frames) - 1)]
    for f, rec in enumerate(recs):
        check(f, rec, "device")
        for trial in range(3):  # another storage order of both frames: permute the records, remap the match indices
            pq, pt = rng.permutation(len(corners[f])), rng.permutation(len(corners[f + 1]))
            m = matches[f][pq].copy()
            ok = m["index"] < len(pt)
            m["index"][ok] = np.argsort(pt)[m["index"][ok]]
            rec2, _ = vr.verify_pair(corners[f][pq], corners[f + 1][pt], m, W, H, f, inlier_px=2.0)
            check(f, rec2, trial)


def test_literal_shift_crops_parity(tinyorb, oracle):
    """Literal mode on the matcher test's shifted crops, with every filter open (ratio 1, distance 256) and 4096 hypotheses."""
    W, H, cap = 320, 240, 1200
    base = oracle.synth_frame(W + 8, H + 6, 300)
    frames = np.stack([np.ascontiguousarray(base[dy:dy + H, dx:dx + W]) for dx, dy in ((0, 0), (3, 2), (8, 6))])
    with _program(tinyorb, W, H, cap, 3) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(3)
        _check_parity(prog, 3, W, H, cap, ratio=1.0, max_distance=256, hypotheses=4096, inlier_px=1.0)


def test_bench_size_parity(tinyorb, oracle):
    """256 related 1280x720 frames (shifted, scaled, perspective views of a few scenes) at capacity 8192: every pair."""
    W, H, cap, B = 1280, 720, 8192, 256
    rng = np.random.default_rng(11)
    scenes = [oracle.synth_frame(W + 160, H + 160, 900 + s) for s in range(4)]
    frames = np.empty((B, H, W, 4), np.uint8)
    for i in range(B):
        G = _warp(rng.uniform(-8, 8), rng.uniform(-8, 8), rng.uniform(0.97, 1.03), 0, rng.uniform(-2e-5, 2e-5),
                  rng.uniform(-2e-5, 2e-5), W=W, H=H)
        frames[i] = _view(scenes[i // 64], G, W, H)
    with _program(tinyorb, W, H, cap, B) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(B)
        recs = _check_parity(prog, B, W, H, cap)
    ok = [r for r in recs if r["status"] == tinyorb.ORB_VERIFY_OK]
    assert len(ok) > 200


def test_state_and_ordering(tinyorb, oracle):
    import torch
    W, H, cap = 320, 240, 800
    frames = _parity_frames(oracle, W, H)[:4]
    with _program(tinyorb, W, H, cap, 4, tinyorb.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        prog.extract_batch_host(frames)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_consecutive(4)  # no match yet
        assert e.value.code == tinyorb.ORB_ESTATE
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_read(0, cap)  # nothing verified
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.match_consecutive(3)
        for kw in (dict(n_frames=4), dict(n_frames=1), dict(n_frames=3, hypotheses=4097), dict(n_frames=3, max_distance=257),
                   dict(n_frames=3, reserved=(0, 1, 0)), dict(n_frames=3, ratio=-1.0), dict(n_frames=3, inlier_px=float("nan"))):
            with pytest.raises(tinyorb.OrbError) as e:
                prog.verify_consecutive(**kw)
            assert e.value.code == tinyorb.ORB_EINVAL, kw
        one = _check_parity(prog, 3, W, H, cap, seed=3)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_read(2, cap)  # two pairs only
        assert e.value.code == tinyorb.ORB_EINVAL
        C.check_read_arguments(tinyorb, prog, tinyorb.load_library().orb_verify_read, 2, 1, head=True)
        # the same verification on another stream than the match's: ordered behind it, the same records
        s = torch.cuda.Stream(device=0)
        prog.match_consecutive(4)
        prog.verify_consecutive(3, seed=3, stream=s.cuda_stream)
        for f in range(2):
            assert prog.verify_read(f, cap)[0].tobytes() == one[f].tobytes()
        prog.verify_consecutive(3, seed=3)  # and back on the batch's stream, behind the one before
        for f in range(2):
            assert prog.verify_read(f, cap)[0].tobytes() == one[f].tobytes()
        # a new batch without a new match, or another output set
        prog.extract_batch_host(frames)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_consecutive(3)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.match_consecutive(4)
        prog.batch_select_output(1)
        with pytest.raises(tinyorb.OrbError) as e:
            prog.verify_consecutive(3)
        assert e.value.code == tinyorb.ORB_ESTATE
        prog.batch_select_output(0)
        prog.verify_consecutive(3, seed=3)
        assert prog.verify_read(0, cap)[0].tobytes() == one[0].tobytes()


def test_profile_names_the_kernels(tinyorb, oracle):
    W, H, cap = 320, 240, 600
    frames = _parity_frames(oracle, W, H)[:3]
    with _program(tinyorb, W, H, cap, 3) as prog:
        prog.extract_batch_host(frames)
        prog.match_consecutive(3)
        prog.profile_enable(True)
        prog.verify_consecutive(3)
        prof = prog.profile()
    for k in ("k_verify_gather", "k_verify_score", "k_verify_refine"):
        assert prof[k][1] == 1, prof
