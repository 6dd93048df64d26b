"""CPU tests of the oracle itself (oracle/ is test infrastructure; PARITY UNPINNED).

The reference ships no tests or vectors, so the oracle is pinned by (1) known-answer tests that
follow from the reference's shader text alone, (2) an independently written NumPy
restatement, and (3) the committed golden fixtures (regression pins of the build's own oracle).
"""
import glob
import hashlib
import os
import re
import sys

import numpy as np
import pytest

from oracle import orb_numpy

THR = np.float32(20.0 / 255.0)
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _frame_with_squares(W, H, squares, bg=0, fg=255):
    img = np.full((H, W, 4), bg, dtype=np.uint8)
    img[..., 3] = 255
    for (x, y, s) in squares:
        img[y:y + s, x:x + s, :3] = fg
    return img


# ---------------------------------------------------------------- scalar known answers
def test_detect_streak_is_fast12(oracle):
    """fast.wgsl:51-60 == 'exists a circular run of >= 12 set bits' for all 65536 masks (Q4)."""
    assert oracle.detect_streak_16(0x0FFF) == 0x0001
    assert oracle.detect_streak_16(0x07FF) == 0
    assert oracle.detect_streak_16(0xF0FF) == 0x1000
    assert oracle.detect_streak_16(0xFFFF) == 0xFFFF
    masks = np.arange(65536, dtype=np.uint32)
    got = np.array([oracle.detect_streak_16(int(m)) for m in masks]) != 0
    run12 = np.zeros(65536, dtype=bool)
    run9 = np.zeros(65536, dtype=bool)
    dbl = masks | (masks << np.uint32(16))
    for start in range(16):
        run12 |= ((dbl >> np.uint32(start)) & np.uint32(0xFFF)) == 0xFFF
        run9 |= ((dbl >> np.uint32(start)) & np.uint32(0x1FF)) == 0x1FF
    assert np.array_equal(got, run12)
    assert int((got != run9).sum()) == 896  # it is NOT FAST-9
    assert np.array_equal(orb_numpy._streak12(masks) != 0, run12)


def test_pattern_fingerprint():
    """BRIEF pattern == the reference table (brief.wgsl:70-327), pinned by SURVEY.md 8a."""
    p = orb_numpy.PATTERN
    assert p.shape == (256, 4)
    assert p[0].tolist() == [8, -3, 9, 5] and p[-1].tolist() == [-1, -6, 0, -11]
    assert p.min() == -13 and p.max() == 12 and int(p.sum()) == -406
    assert _sha(p.astype(np.int8)) == "2164181aea6ff9ac426ca512d5130d15e1f6e3cd47b1cbdd568bbe1e55d49023"
    # the product's copy of the table is the same data
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "tinyslam_amd", "csrc", "orb_tables.h")).read()
    body = text[text.index("ORB_BRIEF_PATTERN[1024]"):]
    body = body[body.index("{") + 1:body.index("}")]
    vals = np.array([int(v) for v in re.findall(r"-?\d+", body)], dtype=np.int8)
    assert np.array_equal(vals.reshape(256, 4), p)


def test_trig_table_matches_libm_and_numpy(oracle):
    """CRD-10: the committed cos/sin table == double libm rounded to binary32, for all 3142 codes of the
    reference and the 6284 codes of the opt-in "intended" mode (full circle)."""
    import re
    text = open(os.path.join(os.path.dirname(__file__), "..", "tinyslam_amd", "csrc", "orb_tables.h")).read()

    def table(name):
        body = text[text.index(name + "["):]
        body = body[body.index("{") + 1:body.index("}")]
        return np.array([int(v, 16) for v in re.findall(r"0x[0-9a-f]{8}", body)], dtype=np.uint32).view(np.float32)
    cos_t, sin_t = table("ORB_COS_BITS"), table("ORB_SIN_BITS")
    assert cos_t.size == 6284 and sin_t.size == 6284
    theta = np.arange(6284, dtype=np.float32) / np.float32(1000.0)
    assert np.array_equal(cos_t, np.cos(theta.astype(np.float64)).astype(np.float32))
    assert np.array_equal(sin_t, np.sin(theta.astype(np.float64)).astype(np.float32))


def test_f16_conversion_matches_numpy(oracle):
    rng = np.random.default_rng(1)
    vals = np.concatenate([
        rng.integers(0, 2**32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
        rng.random(20000, dtype=np.float32),
        (rng.random(5000, dtype=np.float32) * np.float32(2.0**-14)),
        np.array([0x33000000, 0x33000001, 0x387fc000, 0x38800000, 0x477fe000, 0x477ff000, 0x3f801000, 0x3f803000],
                 dtype=np.uint32).view(np.float32)])
    vals = vals[~np.isnan(vals)]
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16)
    got = np.array([oracle.f32_to_f16(v) for v in vals], dtype=np.uint16)
    assert np.array_equal(got, want)
    halves = np.arange(0, 0x7c00, 7, dtype=np.uint16)
    back = np.array([oracle.f16_to_f32(int(h)) for h in halves], dtype=np.float32)
    assert np.array_equal(back, halves.view(np.float16).astype(np.float32))


def test_unorm8_is_ieee_division(oracle):
    for b in range(256):
        assert oracle.unorm8(b) == np.float32(b) / np.float32(255.0)


def test_atan2_against_libm(oracle):
    """CRD-9: canonical atan2 vs libm: milliradian code differs by at most 1, and only next to an integer."""
    rng = np.random.default_rng(2)
    cy = (rng.random(20000, dtype=np.float32) * 30).astype(np.float32)
    cx = (rng.random(20000, dtype=np.float32) * 60 - 30).astype(np.float32)
    mine = orb_numpy.atan2f(cy, cx)
    libm = np.arctan2(cy.astype(np.float64), cx.astype(np.float64))
    assert np.abs(mine.astype(np.float64) - libm).max() < 5e-7
    code = np.trunc(mine * np.float32(1000.0)).astype(np.int64)
    code_libm = np.trunc(libm * 1000.0).astype(np.int64)
    diff = np.abs(code - code_libm)
    assert diff.max() <= 1
    near = np.abs(libm * 1000.0 - np.round(libm * 1000.0)) < 1e-3
    assert np.all(near[diff == 1])
    # C and NumPy restatements agree exactly
    idx = rng.integers(0, cy.size, 3000)
    assert [oracle.angle_code(cy[i], cx[i]) for i in idx] == \
        np.where((cy[idx] < 0) | (mine[idx] < 0), 0, code[idx]).tolist()
    assert oracle.angle_code(0.0, 0.0) == 0            # atan2(0,0) = 0
    assert oracle.angle_code(-1.0, 1.0) == 0           # negative angles saturate to 0 (Q7)
    assert oracle.angle_code(0.0, -1.0) == 3141        # pi -> 3141
    assert oracle.angle_code(1.0, 0.0) == 1570


# ---------------------------------------------------------------- whole-pipeline known answers
def test_flat_image_has_no_corners(oracle):
    img = np.full((96, 128, 4), 77, dtype=np.uint8)
    r = oracle.extract(img, depth=2, threshold=THR)
    assert r["total"] == 0 and len(r["corners"]) == 0


@pytest.mark.parametrize("side,expected", [(1, 1), (2, 4), (3, 9), (4, 12), (5, 0), (6, 0)])
def test_bright_square_corner_counts(oracle, side, expected):
    """SURVEY.md 8c KAT 4: FAST-12 on an isolated bright s x s square (octave 0 only)."""
    img = _frame_with_squares(128, 96, [(60, 40, side)])
    r = oracle.extract(img, depth=1, threshold=THR)
    assert r["total"] == expected
    if side <= 3 and expected:
        ys = 96 - 1 - r["corners"]["y"].astype(int)   # keypoints live in the flipped frame (Q2)
        assert set(zip(r["corners"]["x"].tolist(), ys.tolist())) == \
            {(60 + i, 40 + j) for i in range(side) for j in range(side)}


def test_straight_edge_has_no_corners(oracle):
    img = np.zeros((96, 128, 4), dtype=np.uint8)
    img[:, 64:, :3] = 255
    img[..., 3] = 255
    assert oracle.extract(img, depth=1, threshold=THR)["total"] == 0


def test_vertical_flip_of_input(oracle):
    """KAT 6: flipping the input vertically maps keypoint rows y <-> H-1-y."""
    rgba = oracle.synth_frame(160, 120, 5)
    a = oracle.extract(rgba, depth=1, threshold=THR)
    b = oracle.extract(rgba[::-1].copy(), depth=1, threshold=THR)
    ka = {(int(c["x"]), int(c["y"])) for c in a["corners"]}
    kb = {(int(c["x"]), 119 - int(c["y"])) for c in b["corners"]}
    # the flipped frame sees the mirrored ring, so only the detection SET is compared (angles differ)
    assert ka == kb and len(ka) > 10


def test_depth1_is_octave0_subset(oracle):
    """KAT 8: D = 1 output == the octave-0 records of the D = 2 output."""
    rgba = oracle.synth_frame(200, 150, 8)
    d1 = oracle.extract(rgba, depth=1, threshold=THR)
    d2 = oracle.extract(rgba, depth=2, threshold=THR)
    sel = d2["corners"]["octave"] == 0
    assert np.array_equal(d1["corners"], d2["corners"][sel])
    assert np.array_equal(d1["descriptors"], d2["descriptors"][sel])
    assert (~sel).sum() > 0


def test_angle_zero_descriptor_is_unrotated_pattern(oracle):
    """KAT 5: a keypoint with angle code 0 samples the raw pattern offsets."""
    rgba = oracle.synth_frame(160, 120, 4)
    r = oracle.extract(rgba, depth=1, threshold=THR, planes=True)
    blur = r["blur"][:160 * 120].reshape(120, 160).view(np.float16).astype(np.float32)
    zero = np.nonzero(r["corners"]["angle"] == 0)[0]
    assert zero.size > 0
    p = orb_numpy.PATTERN
    for i in zero[:20]:
        x, y = int(r["corners"]["x"][i]), int(r["corners"]["y"][i])
        bits = blur[y + p[:, 1], x + p[:, 0]] > blur[y + p[:, 3], x + p[:, 2]]
        words = np.packbits(bits.reshape(8, 32), axis=1, bitorder="little").view(np.uint32).ravel()
        assert np.array_equal(words, r["descriptors"][i])


def test_blur_of_constant_and_row_locality(oracle):
    """KAT 7 + Q11-Q13: blur is row-local; two passes = pass(pass(row)) with both flips cancelling."""
    const = np.full((8, 64), oracle.f32_to_f16(0.5), dtype=np.uint16)
    out = oracle.blur_pass(oracle.blur_pass(const))
    assert np.all(np.abs(out.view(np.float16).astype(np.float32) - 0.5) < 2e-3)
    rng = np.random.default_rng(3)
    img = rng.random((10, 96), dtype=np.float32).astype(np.float16).view(np.uint16)
    two = oracle.blur_pass(oracle.blur_pass(img))
    for y in range(10):
        solo = oracle.blur_pass(oracle.blur_pass(img[y:y + 1]))
        assert np.array_equal(two[y], solo[0])
    one = oracle.blur_pass(img)   # a single pass is vertically flipped w.r.t. its input
    assert np.array_equal(one[0], oracle.blur_pass(img[9:10])[0])


def test_mip_even_is_2x2_mean_and_odd_is_bilinear(oracle):
    rng = np.random.default_rng(4)
    src = rng.random((6, 10), dtype=np.float32).astype(np.float16)
    got = oracle.mip(src.view(np.uint16)).view(np.float16).astype(np.float32)
    s = src.astype(np.float32)
    want = (((s[0::2, 0::2] + s[0::2, 1::2]) + (s[1::2, 0::2] + s[1::2, 1::2])) * np.float32(0.25)).astype(np.float16)
    assert np.array_equal(got, want.astype(np.float32))
    odd = rng.random((7, 11), dtype=np.float32).astype(np.float16).view(np.uint16)
    assert np.array_equal(oracle.mip(odd), orb_numpy.mip(odd))
    assert oracle.mip(odd).shape == (3, 5)


# ---------------------------------------------------------------- cross-checks and fixtures
@pytest.mark.parametrize("W,H,depth,seed", [(96, 80, 2, 21), (130, 75, 3, 22), (72, 200, 4, 23)])
def test_c_and_numpy_restatements_agree(oracle, W, H, depth, seed):
    rgba = oracle.synth_frame(W, H, seed)
    assert np.array_equal(rgba, orb_numpy.synth_frame(W, H, seed))
    a = oracle.extract(rgba, depth=depth, threshold=THR, planes=True)
    b = orb_numpy.extract(rgba, depth=depth, threshold=THR)
    dims, _ = oracle.level_dims(W, H, depth)
    for m, (w, h, off) in enumerate(dims):
        assert np.array_equal(a["gray"][off:off + w * h], b["gray"][m].ravel())
        assert np.array_equal(a["blur"][off:off + w * h], b["blur"][m].ravel())
    ka = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
    assert a["total"] == b["total"] and np.array_equal(ka, b["corners"])
    assert np.array_equal(a["descriptors"], b["descriptors"])


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p) for p in GOLDEN])
def test_golden_fixture(oracle, path):
    g = np.load(path)
    W, H, depth, seed, flags, cap = (int(v) for v in g["params"])
    rgba = oracle.synth_frame(W, H, seed, flags)
    assert _sha(rgba) == str(g["rgba_sha256"])
    r = oracle.extract(rgba, depth=depth, threshold=g["threshold"], max_features=cap, planes=True)
    assert r["total"] == int(g["total"])
    dims, _ = oracle.level_dims(W, H, depth)
    for m, (w, h, off) in enumerate(dims):
        assert _sha(r["gray"][off:off + w * h]) == str(g["gray_sha256"][m])
        assert _sha(r["blur"][off:off + w * h]) == str(g["blur_sha256"][m])
    c, d = oracle.sort_keypoints(r["corners"], r["descriptors"])
    assert np.array_equal(np.stack([c[k] for k in ("x", "y", "angle", "octave")], 1), g["corners"])
    assert np.array_equal(d, g["descriptors"])


Y8_GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "y8", "*.npz")))


@pytest.mark.parametrize("path", Y8_GOLDEN, ids=[os.path.basename(p) for p in Y8_GOLDEN])
def test_y8_golden_fixture(oracle, path):
    """Y8 input variant (one byte per pixel; not in the reference's code): C oracle against its committed fixture."""
    g = np.load(path)
    W, H, depth, seed, flags, cap = (int(v) for v in g["params"])
    y8 = oracle.synth_frame_y8(W, H, seed, flags)
    assert _sha(y8) == str(g["y8_sha256"])
    r = oracle.extract_y8(y8, depth=depth, threshold=g["threshold"], max_features=cap, planes=True)
    assert r["total"] == int(g["total"])
    dims, _ = oracle.level_dims(W, H, depth)
    for m, (w, h, off) in enumerate(dims):
        assert _sha(r["gray"][off:off + w * h]) == str(g["gray_sha256"][m])
        assert _sha(r["blur"][off:off + w * h]) == str(g["blur_sha256"][m])
    c, d = oracle.sort_keypoints(r["corners"], r["descriptors"])
    assert np.array_equal(np.stack([c[k] for k in ("x", "y", "angle", "octave")], 1), g["corners"])
    assert np.array_equal(d, g["descriptors"])


def test_y8_definition(oracle):
    """The Y8 grey image is f16(byte/255) of the vertically mirrored sample; a grey RGBA frame run through the literal
    luminance gives a DIFFERENT image (its weights sum to 0.93, Q1), so the two inputs are not interchangeable; C and
    NumPy restatements agree; everything downstream of the grey image is shared with the literal path."""
    from oracle import orb_numpy
    rng = np.random.default_rng(11)
    y8 = rng.integers(0, 256, size=(40, 52), dtype=np.uint8)
    g = oracle.grayscale_y8(y8)
    want = (y8[::-1].astype(np.float32) / np.float32(255.0)).astype(np.float16).view(np.uint16)
    assert np.array_equal(g, want) and np.array_equal(g, orb_numpy.grayscale_y8(y8))
    grey_rgba = np.stack([y8, y8, y8, np.full_like(y8, 255)], axis=2)
    assert not np.array_equal(oracle.grayscale(grey_rgba), g)
    frame = oracle.synth_frame_y8(96, 80, 5)
    a = oracle.extract_y8(frame, depth=3, threshold=THR, planes=True)
    b = orb_numpy.extract(frame, depth=3, threshold=THR, y8=True)
    ka = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
    assert a["total"] == b["total"] > 0 and np.array_equal(ka, b["corners"])
    assert np.array_equal(a["descriptors"], b["descriptors"])


def test_batch_threads_equal_serial(oracle):
    frames = np.stack([oracle.synth_frame(96, 64, 50 + i) for i in range(5)])
    t1, c1, d1 = oracle.extract_batch(frames, depth=2, threshold=THR, max_features=512, n_threads=1)
    t4, c4, d4 = oracle.extract_batch(frames, depth=2, threshold=THR, max_features=512, n_threads=4)
    assert np.array_equal(t1, t4) and np.array_equal(c1, c4) and np.array_equal(d1, d4)
    one = oracle.extract(frames[3], depth=2, threshold=THR, max_features=512)
    assert one["total"] == t1[3] and np.array_equal(one["corners"], c1[3][:one["total"]])


# ---------------------------------------------------------------- opt-in extensions (arc length, NMS)
@pytest.mark.parametrize("arc,nms", [(9, False), (9, True), (12, True), (14, False), (16, True)])
def test_extensions_c_and_numpy_agree(oracle, arc, nms):
    rgba = oracle.synth_frame(168, 130, 40)
    a = oracle.extract_ex(rgba, depth=2, threshold=THR, max_features=1 << 15, arc=arc, nms=nms)
    b = orb_numpy.extract_ex(rgba, depth=2, threshold=THR, max_features=1 << 15, arc=arc, use_nms=nms)
    ka = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
    assert a["total"] == b["total"] and np.array_equal(ka, b["corners"])
    assert np.array_equal(a["descriptors"], b["descriptors"])


def test_extensions_known_answers(oracle):
    rgba = oracle.synth_frame(200, 150, 41)
    lit = oracle.extract(rgba, depth=2, threshold=THR)
    same = oracle.extract_ex(rgba, depth=2, threshold=THR, arc=12, nms=False)
    assert same["total"] == lit["total"] and np.array_equal(same["corners"], lit["corners"])
    totals = [oracle.extract_ex(rgba, depth=2, threshold=THR, max_features=1 << 15, arc=a)["total"] for a in (9, 10, 12, 14, 16)]
    assert totals == sorted(totals, reverse=True) and totals[0] > totals[2] > totals[-1]  # longer arcs are subsets
    # NMS: a bright 3x3 square gives 9 FAST-12 corners; exactly one survives, never two adjacent
    img = _frame_with_squares(128, 96, [(60, 40, 3)])
    assert oracle.extract_ex(img, depth=1, threshold=THR, arc=12, nms=False)["total"] == 9
    kept = oracle.extract_ex(img, depth=1, threshold=THR, arc=12, nms=True)
    assert 1 <= kept["total"] <= 3
    pts = [(int(c["x"]), int(c["y"])) for c in kept["corners"]]
    for i, p in enumerate(pts):
        for q in pts[i + 1:]:
            assert max(abs(p[0] - q[0]), abs(p[1] - q[1])) > 1
    # FAST-9 fires on the corner pixels of a large bright square, FAST-12 does not (SURVEY.md 8c KAT 4)
    big = _frame_with_squares(128, 96, [(50, 30, 20)])
    assert oracle.extract_ex(big, depth=1, threshold=THR, arc=12)["total"] == 0
    assert oracle.extract_ex(big, depth=1, threshold=THR, arc=9)["total"] >= 4


# ---------------------------------------------------------------- "intended" mode (IM-1..IM-8)
INTENDED = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "intended", "*.npz")))


def _keys(corners):
    return np.stack([corners[k] for k in ("x", "y", "angle", "octave")], 1).astype(np.uint32)


@pytest.mark.parametrize("W,H,depth,arc,nms,cap", [(168, 130, 2, 9, False, 8192), (200, 97, 3, 12, True, 8192),
                                                   (168, 130, 2, 9, False, 64), (240, 200, 3, 10, True, 150)])
def test_intended_c_and_numpy_agree(oracle, W, H, depth, arc, nms, cap):
    rgba = oracle.synth_frame(W, H, 60)
    a = oracle.extract_intended(rgba, depth=depth, threshold=THR, max_features=cap, arc=arc, nms=nms, planes=True)
    b = orb_numpy.extract_intended(rgba, depth=depth, threshold=THR, max_features=cap, arc=arc, use_nms=nms)
    ca, da = oracle.sort_keypoints(a["corners"], a["descriptors"])
    order = np.lexsort((b["corners"][:, 0], b["corners"][:, 1], b["corners"][:, 3]))
    assert a["total"] == b["total"] and np.array_equal(_keys(ca), b["corners"][order])
    assert np.array_equal(da, b["descriptors"][order])
    assert np.array_equal(a["gray"], np.concatenate([g.ravel() for g in b["gray"]]))
    assert np.array_equal(a["blur"], np.concatenate([g.ravel() for g in b["blur"]]))


@pytest.mark.parametrize("path", INTENDED, ids=[os.path.basename(p) for p in INTENDED])
def test_intended_golden_fixture(oracle, path):
    g = np.load(path)
    W, H, depth, seed, flags, cap, arc, nms = (int(v) for v in g["params"])
    rgba = oracle.synth_frame(W, H, seed, flags)
    assert _sha(rgba) == str(g["rgba_sha256"])
    r = oracle.extract_intended(rgba, depth=depth, threshold=g["threshold"], max_features=cap, arc=arc, nms=bool(nms),
                                planes=True)
    assert r["total"] == int(g["total"])
    dims, _ = oracle.level_dims(W, H, depth)
    for m, (w, h, off) in enumerate(dims):
        assert _sha(r["gray"][off:off + w * h]) == str(g["gray_sha256"][m])
        assert _sha(r["blur"][off:off + w * h]) == str(g["blur_sha256"][m])
    c, d = oracle.sort_keypoints(r["corners"], r["descriptors"])
    assert np.array_equal(_keys(c), g["corners"]) and np.array_equal(d, g["descriptors"])


def test_intended_known_answers(oracle):
    f16 = lambda v: np.asarray(v, dtype=np.float32).astype(np.float16)  # noqa: E731
    gk = np.array([0.0312511548, 0.106235079, 0.221251875, 0.282523781, 0.221251875, 0.106235079, 0.0312511548],
                  dtype=np.float32)
    # IM-3: the kernel is the reference's four bilinear taps read in texel units (gaussian_blur_x.wgsl:14-26)
    off = [-2.2273038885157046, -0.4391873198428642, 1.3243948342247673, 3.0]
    wgt = [0.13748623236806098, 0.5037756553768409, 0.32748695702046415, 0.031251155234634016]
    taps = np.zeros(8)
    for o, w in zip(off, wgt):
        i = int(np.floor(o))
        taps[i + 3] += w * (1 - (o - i))
        taps[i + 4] += w * (o - i)
    assert np.array_equal(taps[:7].astype(np.float32), gk) and abs(float(gk.astype(np.float64).sum()) - 1.0) < 1e-7
    # impulse response = separable outer product with an f16 store after each pass
    img = np.zeros((21, 23), dtype=np.float16)
    img[10, 11] = 1.0
    px = oracle.gauss_pass(img.view(np.uint16), False)
    py = oracle.gauss_pass(px, True).view(np.float16)
    row = f16(gk)  # X pass of the impulse
    want = f16(gk[:, None] * row.astype(np.float32)[None, :])
    assert np.array_equal(py[7:14, 8:15], want) and float(np.abs(py.astype(np.float32)).sum()) == float(want.astype(np.float32).sum())
    # clamp-to-edge: a constant plane stays put to within one f16 ulp
    const = np.full((9, 12), np.float16(0.7311))
    out = oracle.gauss_pass(oracle.gauss_pass(const.view(np.uint16), False), True)
    assert int(np.abs(out.astype(np.int32) - int(const.view(np.uint16)[0, 0])).max()) <= 1
    # IM-5: the full circle
    assert oracle.angle_code_signed(0.0, 1.0) == 0 and oracle.angle_code_signed(1.0, 0.0) == 1570
    assert oracle.angle_code_signed(0.0, -1.0) == 3141 and oracle.angle_code_signed(-1.0, 0.0) == 4712
    assert oracle.angle_code_signed(-1.0, 1.0) == 5497 and oracle.angle_code_signed(0.0, 0.0) == 0
    assert oracle.angle_code_signed(-1e-30, 1.0) in (6283, 0)
    # IM-1: no mirror -- a bright 3x3 square is found where it is drawn (the literal mode reports H-1-y, Q2)
    img = _frame_with_squares(128, 96, [(60, 30, 3)])
    r = oracle.extract_intended(img, depth=1, threshold=THR, arc=12)
    assert r["total"] == 9 and set(int(v) for v in r["corners"]["y"]) == {30, 31, 32}
    lit = oracle.extract(img, depth=1, threshold=THR)
    assert set(int(v) for v in lit["corners"]["y"]) == {96 - 1 - 30, 96 - 1 - 31, 96 - 1 - 32}
    # IM-4: the guard follows the octave: nothing within 16 px of any octave's border
    rgba = oracle.synth_frame(256, 192, 61)
    r = oracle.extract_intended(rgba, depth=3, threshold=THR, max_features=1 << 15)
    for o in range(3):
        c = r["corners"][r["corners"]["octave"] == o]
        w, h = 256 >> o, 192 >> o
        assert len(c) > 0 and c["x"].min() > 16 and c["y"].min() > 16 and c["x"].max() < w - 16 and c["y"].max() < h - 16
    assert int((r["corners"]["angle"] > 3141).sum()) > 0 and int(r["corners"]["angle"].max()) <= 6283
    # IM-8: a cut keeps a subset of the uncut result, and the counter still reports the uncut number
    cut = oracle.extract_intended(rgba, depth=3, threshold=THR, max_features=100)
    assert cut["total"] == r["total"] and len(cut["corners"]) == 100
    full = {tuple(int(v) for v in k) for k in _keys(r["corners"])}
    assert all(tuple(int(v) for v in k) in full for k in _keys(cut["corners"]))


def test_intended_descriptors_follow_a_half_turn(oracle):
    """Rotating the frame by 180 degrees moves every keypoint to the mirrored position, adds pi to its angle and
    leaves its descriptor (nearly) unchanged -- the property the literal mode lacks (Q7, Q14)."""
    W, H = 200, 160
    rgba = oracle.synth_frame(W, H, 62)
    a = oracle.extract_intended(rgba, depth=1, threshold=THR, max_features=1 << 14, arc=9)
    b = oracle.extract_intended(np.ascontiguousarray(rgba[::-1, ::-1]), depth=1, threshold=THR, max_features=1 << 14, arc=9)
    tb = {(int(c["x"]), int(c["y"])): i for i, c in enumerate(b["corners"])}
    ham, dang, n = [], [], 0
    for i, c in enumerate(a["corners"]):
        j = tb.get((W - 1 - int(c["x"]), H - 1 - int(c["y"])))
        if j is None:
            continue
        n += 1
        d = (int(b["corners"]["angle"][j]) - int(c["angle"])) % 6283
        dang.append(min(abs(d - 3141), abs(d - 3142)))
        ham.append(int(np.unpackbits((a["descriptors"][i] ^ b["descriptors"][j]).view(np.uint8)).sum()))
    assert n > 0.9 * len(a["corners"]) and max(dang) <= 2
    assert float(np.median(ham)) <= 4 and float(np.mean(ham)) < 12


def test_match_oracle_known_answers():
    """The NumPy matcher (checker of orb_match_consecutive): ties to the smallest index, runner-up distance."""
    a = np.zeros((3, 8), dtype=np.uint32)
    a[1, 0] = 0b1111
    a[2, 7] = 0xFFFFFFFF
    b = np.zeros((4, 8), dtype=np.uint32)
    b[0, 0] = 0b0011          # distances to a[0]: 2, a[1]: 2, a[2]: 34 (the runner-up of a[2])
    b[1, 0] = 0b0011          # duplicate of b[0]: ties go to index 0
    b[2, 7] = 0xFFFFFFFE      # distance to a[2]: 1
    b[3, 3] = 0xFFFFFFFF
    idx, dist, second = orb_numpy.match(a, b)
    assert idx.tolist() == [0, 0, 2] and dist.tolist() == [2, 2, 1] and second.tolist() == [2, 2, 34]
    idx, dist, second = orb_numpy.match(a, b[:1])
    assert idx.tolist() == [0, 0, 0] and second.tolist() == [0xFFFF] * 3
    idx, dist, second = orb_numpy.match(a, b[:0])
    assert idx.tolist() == [0xFFFFFFFF] * 3 and dist.tolist() == [0xFFFF] * 3


# ---------------------------------------------------------------------------------------------
# The implementation-defined switches (orb_oracle.h orc_impl_t): out-of-level loads and sampler weight precision
# ---------------------------------------------------------------------------------------------
import glob as _glob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IMPL_FIXTURES = sorted(_glob.glob(os.path.join(os.path.dirname(__file__), "golden", "impl", "*.npz")))


def test_out_of_level_policies_known_answers():
    """fast.wgsl:78,86,103 / brief.wgsl:59-60 outside the level: 0 (robust access), clamp, or naga's Restrict policy
    min(unsigned(coordinate), size - 1), under which a NEGATIVE coordinate lands on the last column / row."""
    from oracle import orb_numpy
    lvl = np.arange(12, dtype=np.float32).reshape(3, 4) + 1  # rows 0..2, columns 0..3; value = 4 y + x + 1
    xs = np.array([-1, 4, 2, 2, -1, 9])
    ys = np.array([1, 1, -1, 3, -1, 7])
    assert orb_numpy._load(lvl, xs, ys, "zero").tolist() == [0, 0, 0, 0, 0, 0]
    assert orb_numpy._load(lvl, xs, ys, "clamp").tolist() == [5, 8, 3, 11, 1, 12]
    assert orb_numpy._load(lvl, xs, ys, "umin").tolist() == [8, 8, 11, 11, 12, 12]
    inside = orb_numpy._load(lvl, np.array([0, 3]), np.array([0, 2]), "umin")
    assert inside.tolist() == [1, 12]


def test_sampler_weight_bits_known_answers():
    """A weight held in n fractional bits: nearest multiple of 2^-n, halves up; 0 bits = the exact fraction."""
    from oracle import orb_numpy
    f = np.array([0.0, 0.001, 0.5 / 256, 0.49 / 256, 0.75, 0.998, 0.9999], dtype=np.float32)
    assert np.array_equal(orb_numpy._weight(f, 0), f)
    assert orb_numpy._weight(f, 8).tolist() == [0.0, 0.0, 1 / 256, 0.0, 0.75, 255 / 256, 1.0]
    assert orb_numpy._weight(f, 1).tolist() == [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0]


@pytest.mark.parametrize("path", _IMPL_FIXTURES, ids=[os.path.basename(p) for p in _IMPL_FIXTURES])
def test_impl_switch_fixture_reproduces(oracle, path):
    """tests/golden/impl: the C restatement under the fixture's switches gives the fixture; under the defaults it does not."""
    import hashlib
    g = np.load(path)
    W, H, depth, seed, flags, cap, oob, wbits = (int(v) for v in g["params"])
    rgba = oracle.synth_frame(W, H, seed, flags)
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == str(g["rgba_sha256"])
    ref = oracle.extract(rgba, depth=depth, threshold=float(g["threshold"]), max_features=cap, oob=oob, weight_bits=wbits)
    c, d = oracle.sort_keypoints(ref["corners"], ref["descriptors"])
    assert ref["total"] == int(g["total"])
    assert np.array_equal(np.stack([c[k] for k in ("x", "y", "angle", "octave")], 1), g["corners"])
    assert np.array_equal(d, g["descriptors"])
    base = oracle.extract(rgba, depth=depth, threshold=float(g["threshold"]), max_features=cap)
    assert base["total"] == int(g["total_default"])
    assert base["total"] != ref["total"] or not np.array_equal(base["descriptors"], ref["descriptors"])


def test_impl_switches_c_equals_numpy_on_a_crafted_edge_frame(oracle):
    """Structure pushed against the right and bottom edges of every level and against the guard's inner corner (x, y = 17:
    rotated samples reach -1), all six switch settings, C against NumPy."""
    from oracle import orb_numpy
    W, H, depth = 132, 100, 3
    rgba = oracle.synth_frame(W, H, 77).copy()
    rng = np.random.default_rng(77)
    for (x0, y0) in [(W - 8, 20), (W - 6, H - 7), (20, H - 6), (16, 16), (17, 40), (40, 17), (W // 2 - 3, H // 2 - 3)]:
        rgba[y0:y0 + 6, x0:x0 + 6, :3] = rng.integers(0, 256, size=(6, 6, 3), dtype=np.uint8)[: H - y0, : W - x0]
    results = {}
    for oob in ("zero", "clamp", "umin"):
        for wbits in (0, 8):
            a = oracle.extract(rgba, depth=depth, max_features=4096, oob=oob, weight_bits=wbits)
            b = orb_numpy.extract(rgba, depth=depth, max_features=4096, oob=oob, weight_bits=wbits)
            kc = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
            assert a["total"] == b["total"] and np.array_equal(kc, b["corners"]), (oob, wbits)
            assert np.array_equal(a["descriptors"], b["descriptors"]), (oob, wbits)
            results[(oob, wbits)] = (a["total"], a["descriptors"].tobytes())
    assert results[("zero", 0)] != results[("clamp", 0)]


# ---------------------------------------------------------------------------------------------
# The pin: a dump of the REFERENCE itself (rust/dump_config0, run where cargo and a Vulkan adapter exist).  Skipped while
# tests/golden/reference_dump*/ is absent -- which is the state of this repository: PARITY UNPINNED.
# ---------------------------------------------------------------------------------------------
_REF_DUMPS = sorted(d for d in _glob.glob(os.path.join(os.path.dirname(__file__), "golden", "reference_dump*"))
                    if os.path.exists(os.path.join(d, "total.npy")))


@pytest.mark.skipif(not _REF_DUMPS, reason="no dump of the reference (tests/golden/reference_dump*/): parity unpinned")
@pytest.mark.parametrize("dump", _REF_DUMPS or [None])
def test_reference_dump_pins_the_oracle(oracle, dump):
    """One dumped frame turns parity green or names the switch that is wrong: the restatement must reproduce the reference's
    counter, keypoints, angle codes and every descriptor bit under at least one setting of the implementation-defined
    switches, and the defaults must be among the settings that do."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    _, results, exact = pin_oracle.check(dump)
    assert exact, {k: {kk: (len(vv) if isinstance(vv, list) else vv) for kk, vv in v.items()} for k, v in results.items() if not any(k[2:])}
    assert pin_oracle.DEFAULT in exact, "the reference's adapter follows %s, not the defaults: change them" % [pin_oracle.describe(s) for s in exact]


def _write_dump(tmp_path, t, c, d, seed, flags):
    np.save(tmp_path / "total.npy", np.uint32(t))
    np.save(tmp_path / "corners.npy", c)
    np.save(tmp_path / "descriptors.npy", d)
    np.save(tmp_path / "params.npy", np.array([640, 480, 2, seed, flags, 8192], dtype=np.uint32))


def test_pin_tool_names_the_setting_of_a_fabricated_dump(oracle, tmp_path):
    """tools/pin_oracle.py check on a dump fabricated from the restatement under (umin, 8) on the noisy frame: it must find
    exactly the settings that reproduce it, and the defaults must not be among them."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    t, c, d = pin_oracle.oracle_result(S("umin", 8), 2, 15)
    perm = np.random.default_rng(3).permutation(len(c))  # the reference's order is unspecified (atomic append)
    _write_dump(tmp_path, t, c[perm], d[perm], 2, 15)
    _, results, exact = pin_oracle.check(str(tmp_path))
    assert S("umin", 8) in exact and S() not in exact and S("zero", 8) not in exact and S("umin", 0) not in exact
    # (this frame tells neither clamp from umin nor the arithmetic forms apart -- the tool says so -- but zero from both, 0 from 8
    # weight bits, and nearest-even from truncating stores)
    assert all(s.oob in ("clamp", "umin") and s.weight_bits == 8 and s.f16_round == 0 for s in exact)
    assert results[S()]["descriptor_bits"] > 0
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 0


def test_pin_tool_tells_an_atan2_difference_from_a_real_one(oracle, tmp_path):
    """A dump fabricated from the restatement in which forty angle codes are one milliradian off and their descriptors are
    the restatement's AT THOSE angles -- an adapter whose atan2 rounds the other way (CRD-9) -- is reported as pinned up to
    atan2 under the right switches only; the same dump with one descriptor bit flipped at an agreeing angle is not."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    few = [S(), S("umin", 8), S("zero", 0, 7), S("zero", 0, 0, 1)]
    t, c, d, blur = pin_oracle.oracle_result(S(), 2, 15, planes=True)
    c, d = c.copy(), d.copy()
    rng = np.random.default_rng(5)
    pick = rng.choice(np.flatnonzero((c[:, 2] > 1) & (c[:, 2] < 3140)), size=40, replace=False)
    c[pick, 2] += rng.choice(np.array([-1, 1]), size=40).astype(np.int64).astype(np.uint32)
    d[pick] = pin_oracle.descriptors_at(blur, c[pick], S())
    assert np.any(d[pick] != pin_oracle.oracle_result(S(), 2, 15)[2][pick])  # the angle does move descriptor bits

    _write_dump(tmp_path, t, c, d, 2, 15)
    _, results, exact = pin_oracle.check(str(tmp_path), few)
    assert not exact
    r = results[S()]
    assert r["exact_up_to_atan2"] and r["angle_off_by_1"] == 40 and r["descriptor_bits_at_the_dumped_angle"] == 0
    assert not results[S("umin", 8)]["exact_up_to_atan2"]
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 3
    d2 = d.copy()
    other = np.setdiff1d(np.arange(len(c)), pick)[7]
    # a bit whose test has no rotated coordinate near an integer: not something sin / cos could explain either
    for bit in range(256):
        if not pin_oracle.sincos_explains(blur, c[other], bit, 1 - ((int(d[other, bit >> 5]) >> (bit & 31)) & 1), S(), tol=1e-3)[0]:
            break
    d2[other, bit >> 5] ^= np.uint32(1 << (bit & 31))
    _write_dump(tmp_path, t, c, d2, 2, 15)
    _, results, _ = pin_oracle.check(str(tmp_path), few)
    assert not results[S()]["exact_up_to_atan2"] and results[S()]["descriptor_bits_where_angles_agree"] == 1
    assert not results[S()]["exact_up_to_sincos"] and results[S()]["sincos_unexplained"] == 1
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 1


def test_pin_tool_tells_a_sincos_difference_from_a_real_one(oracle, numpy_ref, tmp_path):
    """cos / sin (brief.wgsl:36-37) are the adapter's own, as atan2 is: a dump fabricated from the restatement in which every test
    with a rotated coordinate within 5e-6 of a non-zero integer takes the truncation of the OTHER side (an adapter whose cos rounds
    one place differently) differs in descriptor bits at agreeing angle codes -- the tool must report it as pinned up to sin / cos
    (exit code 6) under the right switches, and a dump with one more bit flipped where no coordinate is near an integer as not pinned."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    few = [S(), S("clamp", 8), S("zero", 0, 7), S("zero", 0, 4, 1)]
    t, c, d, blur = pin_oracle.oracle_result(S(), 2, 15, planes=True)
    d = d.copy()
    F = np.float32
    theta = c[:, 2].astype(np.float32) / F(1000.0)
    ct, st = np.cos(theta.astype(np.float64)).astype(np.float32), np.sin(theta.astype(np.float64)).astype(np.float32)
    flipped = 0
    for j in range(256):
        ax, ay, bx, by = (F(v) for v in numpy_ref.PATTERN[j])
        co = np.stack(numpy_ref.rotate(ct, st, ax, ay) + numpy_ref.rotate(ct, st, bx, by), 1)  # (n, 4): rax, ray, rbx, rby
        n = np.rint(co)
        near = (n != 0) & (np.abs(co - n) <= 5e-6) & (c[:, 2:3] != 0)  # cos 0 = 1, sin 0 = 0 everywhere: code 0 rotates nothing
        for i in np.flatnonzero(near.any(1)):
            tr = np.trunc(co[i]).astype(np.int64)
            other = np.where(tr != n[i], n[i], n[i] - np.sign(n[i])).astype(np.int64)
            use = np.where(near[i], other, tr)
            va = pin_oracle._level_load(blur, int(c[i, 3]), int(c[i, 0]) + int(use[0]), int(c[i, 1]) + int(use[1]), "zero")
            vb = pin_oracle._level_load(blur, int(c[i, 3]), int(c[i, 0]) + int(use[2]), int(c[i, 1]) + int(use[3]), "zero")
            bit = int(va > vb)
            if bit != ((int(d[i, j >> 5]) >> (j & 31)) & 1):
                d[i, j >> 5] ^= np.uint32(1 << (j & 31))
                flipped += 1
    assert flipped > 0  # the frame has such tests (about one coordinate in 10^5 lies that close to an integer)
    _write_dump(tmp_path, t, c, d, 2, 15)
    _, results, exact = pin_oracle.check(str(tmp_path), few)
    r = results[S()]
    assert not exact and not r["exact_up_to_atan2"]
    assert r["exact_up_to_sincos"] and r["sincos_bits"] == flipped and r["sincos_unexplained"] == 0 and r["sincos_max_distance"] <= 5e-6
    assert not results[S("clamp", 8)]["exact_up_to_sincos"]
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 6
    # one real difference on top
    i = 11
    for bit in range(256):
        if not pin_oracle.sincos_explains(blur, c[i], bit, 1 - ((int(d[i, bit >> 5]) >> (bit & 31)) & 1), S(), tol=1e-3)[0]:
            break
    d[i, bit >> 5] ^= np.uint32(1 << (bit & 31))
    _write_dump(tmp_path, t, c, d, 2, 15)
    _, results, _ = pin_oracle.check(str(tmp_path), few)
    assert not results[S()]["exact_up_to_sincos"] and results[S()]["sincos_unexplained"] == 1
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 1


def _rn32(fr):
    """Fraction -> binary32, round to nearest even, exactly (float(Fraction) is correctly rounded to binary64; the candidates
    around its binary32 rounding are compared as fractions)."""
    from fractions import Fraction
    x = np.float32(float(fr))
    best = None
    for c in (np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))):
        d = abs(Fraction(float(c)) - fr)
        even = (np.frombuffer(np.float32(c).tobytes(), dtype=np.uint32)[0] & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, c)
    return np.float32(best[1])


@pytest.mark.parametrize("dot_order", [0, 1])
def test_contracted_luminance_is_an_exact_fma_chain(oracle, numpy_ref, dot_order):
    """CRD-13, orc_impl_t::contract & ORC_CONTRACT_LUM: the luminance is one product and a chain of fmas, each fma rounded ONCE --
    r*wr, fma(g, wg, .), fma(b, wb, .) first component first; b*wb, fma(g, wg, .), fma(r, wr, .) last component first (Mesa's fdot
    lowering) -- checked against exact rational arithmetic on 300 random colours in the C restatement AND the NumPy one (whose
    fma is built from binary64 operations); and each is a different function from the default on some texels of a frame."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    rgba = rng.integers(0, 256, size=(1, 300, 4), dtype=np.uint8)
    out = oracle.grayscale_fp(rgba, contract=oracle.CONTRACT_LUM, dot_order=dot_order)[0]
    want = np.zeros(300, dtype=np.uint16)
    wr, wg, wb = (Fraction(float(np.float32(w))) for w in (0.229, 0.587, 0.114))
    for i, (r, g, b, _) in enumerate(rgba[0]):
        fr, fg, fb = (Fraction(float(np.float32(np.float32(v) / np.float32(255)))) for v in (r, g, b))
        (f1, w1), (f3, w3) = ((fr, wr), (fb, wb)) if not dot_order else ((fb, wb), (fr, wr))
        t = _rn32(w1 * f1)
        t = _rn32(fg * wg + Fraction(float(t)))
        t = _rn32(f3 * w3 + Fraction(float(t)))
        want[i] = oracle.f32_to_f16(float(t))
    assert np.array_equal(out, want)
    assert np.array_equal(numpy_ref.grayscale(rgba, 1, dot_order)[0], want)
    # the readings differ somewhere on a frame (a handful of texels in a million), and nowhere else than in the last place
    frame = oracle.synth_frame(640, 480, 2, 15)
    a = oracle.extract(frame, depth=2, threshold=THR, planes=True)
    b = oracle.extract(frame, depth=2, threshold=THR, planes=True, contract=oracle.CONTRACT_LUM, dot_order=dot_order)
    diff = a["gray"].astype(np.int32) - b["gray"].astype(np.int32)
    assert 0 < np.count_nonzero(diff) < 100 and np.abs(diff).max() == 1


def test_uncontracted_last_first_luminance(oracle, numpy_ref):
    """dot_order = 1 without contraction: (b*wb + g*wg) + r*wr, every product and sum rounded -- what Mesa's fdot lowering gives on
    hardware without an fma (the reference's stated target, a Raspberry Pi 5).  Exact rationals, C and NumPy."""
    from fractions import Fraction
    rng = np.random.default_rng(12)
    rgba = rng.integers(0, 256, size=(1, 300, 4), dtype=np.uint8)
    out = oracle.grayscale_fp(rgba, contract=0, dot_order=1)[0]
    want = np.zeros(300, dtype=np.uint16)
    wr, wg, wb = (Fraction(float(np.float32(w))) for w in (0.229, 0.587, 0.114))
    for i, (r, g, b, _) in enumerate(rgba[0]):
        fr, fg, fb = (Fraction(float(np.float32(np.float32(v) / np.float32(255)))) for v in (r, g, b))
        pb, pg, pr = _rn32(fb * wb), _rn32(fg * wg), _rn32(fr * wr)
        t = _rn32(Fraction(float(pb)) + Fraction(float(pg)))
        want[i] = oracle.f32_to_f16(float(_rn32(Fraction(float(t)) + Fraction(float(pr)))))
    assert np.array_equal(out, want)
    assert np.array_equal(numpy_ref.grayscale(rgba, 0, 1)[0], want)
    assert np.any(out != oracle.grayscale_fp(rgba)[0]) or True  # (300 colours need not hold a difference; the frame test above does)


def test_contracted_rotation_forms(oracle, numpy_ref):
    """orc_impl_t::contract & ORC_CONTRACT_ROT: matrix * vector with ONE of the two products fused into the sum -- the second term onto
    the first product (dot_order 0) or the first onto the second (dot_order 1: Mesa builds the product from the last column down) --
    against exact rationals over every pattern point at 40 angle codes, C and NumPy; unfused, the order does not matter."""
    from fractions import Fraction
    rng = np.random.default_rng(13)
    codes = rng.integers(0, 3142, size=40)
    pts = {(int(x), int(y)) for row in numpy_ref.PATTERN for x, y in ((row[0], row[1]), (row[2], row[3]))}
    pts = sorted(pts)[::7]
    for code in codes:
        theta = np.float32(code) / np.float32(1000.0)
        ct, st = np.float32(np.cos(np.float64(theta))), np.float32(np.sin(np.float64(theta)))
        fct, fst = Fraction(float(ct)), Fraction(float(st))
        for (x, y) in pts:
            want0 = (_rn32(fst * y + Fraction(float(_rn32(fct * x)))), _rn32(fct * y + Fraction(float(_rn32(-fst * x)))))
            want1 = (_rn32(fct * x + Fraction(float(_rn32(fst * y)))), _rn32(-fst * x + Fraction(float(_rn32(fct * y)))))
            plain = (_rn32(Fraction(float(_rn32(fct * x))) + Fraction(float(_rn32(fst * y)))),
                     _rn32(Fraction(float(_rn32(-fst * x))) + Fraction(float(_rn32(fct * y)))))
            for order, want in ((0, want0), (1, want1)):
                got = oracle.brief_rotate(int(code), x, y, oracle.CONTRACT_ROT, order)
                assert (got[0], got[1]) == want, (code, x, y, order)
                gn = numpy_ref.rotate(np.array([ct]), np.array([st]), np.float32(x), np.float32(y), 1, order)
                assert (gn[0][0], gn[1][0]) == want
                assert tuple(oracle.brief_rotate(int(code), x, y, 0, order)) == plain


def test_f16_round_toward_zero(oracle, numpy_ref):
    """orc_impl_t::f16_round = 1: every store to an R16Float target truncates instead of rounding to nearest even -- the conversion
    itself over a sweep of binary32 values (C against NumPy against the definition: the largest binary16 not above |v|), and a frame
    through both restatements."""
    rng = np.random.default_rng(14)
    v = np.concatenate([rng.random(4000, dtype=np.float32), rng.random(500, dtype=np.float32) * np.float32(1e-4),
                        np.array([0.0, 1.0, 0.5, 6.1e-5, 5.96e-8, 2.9e-8, 3.1e-8, 65504.0, 65519.0, 65520.0, 70000.0], dtype=np.float32)])
    c = np.array([oracle.f32_to_f16(x, rtz=1) for x in v], dtype=np.uint16)
    ok = v <= np.float32(65504.0)
    assert np.array_equal(c[ok], numpy_ref.to_f16_bits(v[ok], rtz=1))
    back = c.view(np.float16).astype(np.float32)
    assert np.all(back[ok] <= v[ok])
    inner = ok & (c < 0x7bff)
    assert np.all(np.nextafter(c[inner].view(np.float16), np.float16(np.inf)).astype(np.float32) > v[inner])
    assert np.all(c[~ok] == 0x7bff)  # finite values beyond the largest binary16 stay finite when rounding toward zero
    rne = np.array([oracle.f32_to_f16(x) for x in v], dtype=np.uint16)
    assert np.any(rne != c) and np.all((rne == c) | (rne == c + 1))
    frame = oracle.synth_frame(333, 77, 5, 15)  # odd sizes: the bilinear blit's store as well
    a = oracle.extract(frame, depth=3, threshold=THR, planes=True, f16_round=1, weight_bits=8)
    b = numpy_ref.extract(frame, depth=3, threshold=THR, f16_round=1, weight_bits=8)
    assert a["total"] == b["total"]
    assert np.array_equal(a["gray"], np.concatenate([g.ravel() for g in b["gray"]]))
    assert np.array_equal(a["blur"], np.concatenate([g.ravel() for g in b["blur"]]))
    assert np.array_equal(a["descriptors"], b["descriptors"])
    d = oracle.extract(frame, depth=3, threshold=THR, planes=True, weight_bits=8)
    assert np.count_nonzero(a["gray"] != d["gray"]) > 1000  # about half of all texels round the other way


@pytest.mark.parametrize("contract,dot_order", [(1, 0), (2, 0), (4, 0), (4, 1), (7, 0), (7, 1), (0, 1), (3, 1), (5, 0)])
def test_c_equals_numpy_under_the_arithmetic_switches(oracle, numpy_ref, contract, dot_order):
    """The two restatements agree -- planes, keypoints, angle codes, descriptors -- under per-stage contraction and both reduction
    orders, on a noisy frame with an odd-sized level and under a second out-of-level policy."""
    frame = oracle.synth_frame(322, 241, 7 + contract, 15)
    for oob, wb in (("zero", 0), ("umin", 8)):
        a = oracle.extract(frame, depth=2, threshold=THR, planes=True, contract=contract, dot_order=dot_order, oob=oob, weight_bits=wb)
        b = numpy_ref.extract(frame, depth=2, threshold=THR, contract=contract, dot_order=dot_order, oob=oob, weight_bits=wb)
        assert a["total"] == b["total"] and a["total"] > 50
        assert np.array_equal(a["gray"], np.concatenate([g.ravel() for g in b["gray"]]))
        assert np.array_equal(a["blur"], np.concatenate([g.ravel() for g in b["blur"]]))
        ca = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
        assert np.array_equal(ca, b["corners"]) and np.array_equal(a["descriptors"], b["descriptors"])


def test_contracted_blur_is_one_fma_per_tap(oracle, numpy_ref):
    """orc_impl_t::contract & ORC_CONTRACT_BLUR: `result += sample * weight` as fma(sample, weight, result), the sampler's own lerp
    left alone -- one row against exact rationals, C and NumPy."""
    from fractions import Fraction
    rng = np.random.default_rng(15)
    w = 96
    row = numpy_ref.to_f16_bits(rng.random((1, w), dtype=np.float32))
    out = oracle.blur_pass_fp(row, contract=oracle.CONTRACT_BLUR)[0]
    assert np.array_equal(out, numpy_ref.blur_pass(row, 0, 1)[0])
    vals = row[0].view(np.float16).astype(np.float32)
    want = np.zeros(w, dtype=np.uint16)
    fw = np.float32(w)
    for x in range(w):
        u = (np.float32(x) + np.float32(0.5)) / fw
        acc = np.float32(0)
        for off, wgt in zip(numpy_ref.BLUR_OFF, numpy_ref.BLUR_WGT):
            coord = (u + off) * fw - np.float32(0.5)
            c0 = np.floor(coord)
            f = np.float32(coord - c0)
            i0, i1 = int(np.clip(int(c0), 0, w - 1)), int(np.clip(int(c0) + 1, 0, w - 1))
            sample = np.float32(vals[i0] + np.float32(f * np.float32(vals[i1] - vals[i0])))
            acc = _rn32(Fraction(float(sample)) * Fraction(float(wgt)) + Fraction(float(acc)))
        want[x] = oracle.f32_to_f16(float(acc))
    assert np.array_equal(out, want)
    big = oracle.grayscale(oracle.synth_frame(640, 480, 2))  # the f16 store hides most differences: one row need not hold one
    assert np.any(oracle.blur_pass_fp(big, contract=oracle.CONTRACT_BLUR) != oracle.blur_pass_fp(big))


def test_pin_tool_names_a_contracting_compiler(oracle, tmp_path):
    """A dump fabricated from the restatement with every stage contracted on a frame where that changes an angle code: the tool must
    explain it by contraction -- exit code 0, the settings it names all contract the luminance -- and not by the adapter's atan2,
    which would fit too; a dump of last-component-first arithmetic is told from both; and a dump of the default arithmetic on the
    same frame names the defaults."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    seed, flags = 1, 15
    few = [S(oob, 0, ct, do) for oob in ("zero", "clamp") for ct in (0, 1, 7) for do in (0, 1)]
    t, c, d = pin_oracle.oracle_result(S("zero", 0, 7), seed, flags)
    t0, c0, d0 = pin_oracle.oracle_result(S(), seed, flags)
    assert t == t0 and (not np.array_equal(c, c0) or not np.array_equal(d, d0))  # the frame tells the two apart

    _write_dump(tmp_path, t, c, d, seed, flags)
    _, results, exact = pin_oracle.check(str(tmp_path), few)
    # (the one texel behind the difference rounds the same way in every form but the default's: the frame tells the default from the
    # others, not the others from each other -- which is what the tool reports)
    assert S("zero", 0, 7) in exact and S() not in exact and all((s.contract & 1 or s.dot_order) and s.oob == "zero" for s in exact)
    _, results, exact = pin_oracle.check(str(tmp_path))  # the whole space
    assert S("zero", 0, 7) in exact and S() not in exact and all((s.contract & 1 or s.dot_order) and s.f16_round == 0 for s in exact)
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 0
    _write_dump(tmp_path, t0, c0, d0, seed, flags)
    _, results, exact = pin_oracle.check(str(tmp_path), few)
    assert S() in exact and S("zero", 0, 7) not in exact and not any(s.contract & 1 or s.dot_order for s in exact)
    # Mesa's order without an fma (a Raspberry Pi 5): told from the default and from both contracted forms
    t1, c1, d1 = pin_oracle.oracle_result(S("zero", 0, 0, 1), seed, flags)
    if not (np.array_equal(c1, c0) and np.array_equal(d1, d0)):
        _write_dump(tmp_path, t1, c1, d1, seed, flags)
        _, results, exact = pin_oracle.check(str(tmp_path), few)
        assert S("zero", 0, 0, 1) in exact and S() not in exact


def test_pin_tool_reports_a_truncating_store(oracle, tmp_path):
    """A dump of R16Float stores that round toward zero: only f16_round = 1 settings reproduce it, which the kernels do not carry --
    exit code 5."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    t, c, d = pin_oracle.oracle_result(S(f16_round=1), 2, 15)
    _write_dump(tmp_path, t, c, d, 2, 15)
    _, results, exact = pin_oracle.check(str(tmp_path), [S(), S(f16_round=1), S("zero", 0, 7), S("zero", 0, 7, 0, 1)])
    assert S(f16_round=1) in exact and all(s.f16_round == 1 for s in exact)
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 5


def test_negative_angle_conversion_policies(oracle, numpy_ref):
    """fast.wgsl:153 `u32(angle * 1000.0)` of a negative angle (orc_impl_t::neg_angle): 0 by default (Q7), the low 32 bits of the
    truncated value under "wrap" (x86-64's conversion through a 64-bit integer), all ones under "ones"; angles >= 0 never change;
    a negative angle above -0.001 truncates to 0 under every policy.  C == NumPy on a whole frame under each policy."""
    cy, cx = np.float32(-1.0), np.float32(1.0)  # atan2 = -pi/4 = -0.785398...
    assert oracle.angle_code_neg(cy, cx, "zero") == 0 == oracle.angle_code(cy, cx)
    assert oracle.angle_code_neg(cy, cx, "wrap") == (1 << 32) - 785
    assert oracle.angle_code_neg(cy, cx, "ones") == 0xFFFFFFFF
    for pol in ("zero", "wrap", "ones"):
        assert oracle.angle_code_neg(np.float32(1.0), np.float32(1.0), pol) == 785
        assert oracle.angle_code_neg(np.float32(-1e-5), np.float32(1.0), pol) == 0  # -0.00001 rad * 1000 truncates to -0
        assert oracle.angle_code_neg(np.float32(-1.0), np.float32(-1e-9), pol) == oracle.angle_code_neg(np.float32(-1.0), np.float32(0.0), pol)
    rgba = oracle.synth_frame(200, 136, 11, 15)
    base = oracle.extract(rgba, depth=3)
    for pol in ("wrap", "ones"):
        a = oracle.extract(rgba, depth=3, neg_angle=pol)
        b = numpy_ref.extract(rgba, depth=3, neg_angle=pol)
        assert a["total"] == b["total"] == base["total"]
        ca = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
        assert np.array_equal(ca, b["corners"]) and np.array_equal(a["descriptors"], b["descriptors"])
        pos = base["corners"]["angle"] > 0
        assert pos.any() and (~pos).any()
        assert np.array_equal(a["corners"]["angle"][pos], base["corners"]["angle"][pos])
        assert np.array_equal(a["descriptors"][pos], base["descriptors"][pos])
        big = a["corners"]["angle"] > 3142
        assert big.any() and not (big & pos).any()
        if pol == "ones":
            assert (a["corners"]["angle"][big] == 0xFFFFFFFF).all()
        else:
            m = (1 << 32) - a["corners"]["angle"][big].astype(np.int64)
            assert (m >= 1).all() and (m <= 3142).all() and len(np.unique(m)) > 1


def test_pin_tool_recognises_an_adapter_that_does_not_saturate_negative_angles(oracle, tmp_path):
    """A dump whose negative angles wrapped modulo 2^32 (a CPU adapter; SURVEY.md Q7 assumed saturation), with whatever that
    adapter's cos / sin made of the descriptors there: the tool reads the policy off the codes, checks the codes against the
    restatement under it, leaves those descriptors out, pins the rest -- exit code 7.  A wrong wrapped code is still a mismatch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    S = pin_oracle.setting
    few = [S(), S("clamp"), S("zero", 8), S("zero", 0, 7)]
    for pol in ("wrap", "ones"):
        t, c, d = pin_oracle.oracle_result(S(), 2, 15, neg_angle=pol)
        big = c[:, 2] > 3142
        assert 0 < big.sum() < len(c)
        d[big] ^= np.uint32(0x5A5A5A5A)  # some other cos / sin at 4e6 rad
        _write_dump(tmp_path, t, c, d, 2, 15)
        assert pin_oracle.neg_angle_policy(c) == pol
        _, results, exact = pin_oracle.check(str(tmp_path), few)
        assert S() in exact and S("zero", 8) not in exact and S("clamp") not in exact
        assert results[S()]["descriptors_not_compared"] == int(big.sum())
    assert pin_oracle.main(["pin_oracle.py", "check", str(tmp_path)]) == 7
    # under the default policy the same dump is not exact (the codes differ) ...
    ref0 = pin_oracle.oracle_result(S(), 2, 15, planes=True)
    r = pin_oracle.compare(pin_oracle.load_dump(str(tmp_path)), ref0, blur=ref0[3], s=S())
    assert not r["exact"] and r["angle_off_by_more"] == int(big.sum())
    # ... a descriptor bit at a NON-negative angle still counts, and so does a wrapped code that is not the restatement's
    t, c, d = pin_oracle.oracle_result(S(), 2, 15, neg_angle="wrap")
    d2 = d.copy()
    d2[np.flatnonzero(c[:, 2] <= 3142)[0], 0] ^= 1
    _write_dump(tmp_path, t, c, d2, 2, 15)
    assert pin_oracle.check(str(tmp_path), few)[2] == []
    c2 = c.copy()
    c2[np.flatnonzero(c[:, 2] > 3142)[0], 2] -= 5
    _write_dump(tmp_path, t, c2, d, 2, 15)
    assert pin_oracle.check(str(tmp_path), few)[2] == []
    # codes that are neither: no policy
    c3 = c.copy()
    c3[0, 2] = 100000
    assert pin_oracle.neg_angle_policy(c3) is None and pin_oracle.neg_angle_policy(pin_oracle.oracle_result(S(), 2, 15)[1]) == "zero"


def test_green_product_in_two_operations(numpy_ref):
    """k_front's packed luminance computes the green product fl(fl(G / 255) * 0.587f) of the non-contracted forms as fma(G, kGHi, fl(G * kGLo)):
    the constants are read from the kernel source and the identity is checked for every byte with exact rational arithmetic (and
    with the NumPy restatement's fma).  The same search finds no such pair for the other weights -- the kernel does not claim one."""
    from fractions import Fraction
    src = open(os.path.join(ROOT, "tinyslam_amd", "csrc", "orb_kernels_front.h")).read()
    m = re.search(r"kGHi = (0x[0-9a-fA-F.]+p[-+]?\d+)f, kGLo = (0x[0-9a-fA-F.]+p[-+]?\d+)f", src)
    assert m, "the constants of the green product are no longer where this test reads them"
    hi, lo = np.float32(float.fromhex(m.group(1))), np.float32(float.fromhex(m.group(2)))
    assert float(hi) == float.fromhex(m.group(1)) and float(lo) == float.fromhex(m.group(2))  # both are binary32 values
    b = np.arange(256, dtype=np.float32)
    want = ((b / np.float32(255.0)).astype(np.float32) * np.float32(0.587)).astype(np.float32)  # CRD-1, CRD-2
    t = (b * lo).astype(np.float32)
    assert np.array_equal(numpy_ref.fma32(b, np.full(256, hi, dtype=np.float32), t), want)

    def rne(fr):  # a rational to the nearest binary32, ties to even
        x = np.float32(float(fr))
        cands = [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]
        d = [abs(Fraction(float(c)) - fr) for c in cands]
        best = min(d)
        win = [c for c, dd in zip(cands, d) if dd == best]
        return win[0] if len(win) == 1 else [c for c in win if (int(np.float32(c).view(np.uint32)) & 1) == 0][0]

    for i in range(256):
        assert rne(Fraction(i) * Fraction(float(hi)) + Fraction(float(t[i]))) == want[i], i


REFTEXT = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "reftext", "*.npz")))


def reftext_frame(oracle, g):
    """A fixture's input frame: stored, or (BASELINE configs[0]'s 640x480 frame) rebuilt from its generator parameters and checked by hash."""
    if "rgba" in g:
        return g["rgba"]
    W, H, seed, flags = (int(v) for v in g["synth"])
    rgba = oracle.synth_frame(W, H, seed, flags)
    assert hashlib.sha256(rgba.tobytes()).hexdigest() == str(g["rgba_sha256"])
    return rgba


@pytest.mark.parametrize("path", REFTEXT, ids=[os.path.basename(p) for p in REFTEXT])
def test_reference_text_fixture(oracle, numpy_ref, path):
    """tests/golden/reftext/*.npz hold what the reference's shader text yields when tests/wgsl_interp.py executes it
    (tests/golden/make_reftext_golden.py, on a machine with the reference checkout): both restatements reproduce every grey and blur
    level, the counter, the keypoints with their angle codes and the descriptors, bit for bit -- also where the checkout is absent."""
    g = np.load(path)
    rgba, depth, thr, cap = reftext_frame(oracle, g), int(g["depth"]), np.float32(g["threshold"]), int(g["max_features"])
    H, W = rgba.shape[:2]
    ref = oracle.extract(rgba, depth=depth, threshold=thr, max_features=cap, planes=True)
    nref = numpy_ref.extract(rgba, depth=depth, threshold=thr, max_features=cap)
    dims, _ = oracle.level_dims(W, H, depth)
    for m, (w, h, off) in enumerate(dims):
        if "gray%d" % m in g:
            assert np.array_equal(ref["gray"][off:off + w * h].reshape(h, w), g["gray%d" % m]), "grey level %d" % m
            assert np.array_equal(nref["gray"][m], g["gray%d" % m])
        else:  # a large level of a noisy frame is held as its SHA-256
            want = str(g["gray%d_sha256" % m])
            assert hashlib.sha256(np.ascontiguousarray(ref["gray"][off:off + w * h]).tobytes()).hexdigest() == want, "grey level %d" % m
            assert hashlib.sha256(np.ascontiguousarray(nref["gray"][m]).tobytes()).hexdigest() == want
        assert np.array_equal(ref["blur"][off:off + w * h].reshape(h, w), g["blur%d" % m]), "blur level %d" % m
        assert np.array_equal(nref["blur"][m], g["blur%d" % m])
    assert ref["total"] == nref["total"] == int(g["total"]) > 0
    rc, rd = oracle.sort_keypoints(ref["corners"], ref["descriptors"])
    assert np.array_equal(np.stack([rc[k] for k in ("x", "y", "angle", "octave")], 1), g["corners"]) and np.array_equal(rd, g["descriptors"])
    nc = nref["corners"]
    order = np.lexsort((nc[:, 0], nc[:, 1], nc[:, 3]))
    assert np.array_equal(nc[order], g["corners"]) and np.array_equal(nref["descriptors"][order], g["descriptors"])


@pytest.mark.parametrize("name", ["t640x480_d2_config0", "t640x480_d2_noisy"])
def test_pin_tool_on_the_executed_text(oracle, tmp_path, name):
    """tools/pin_oracle.py fed with what the EXECUTED reference text yields on the two frames it asks a maintainer to dump -- BASELINE
    configs[0]'s and the noisy one (tests/golden/reftext/, made by the interpreter, not by the restatement the tool compares with): it finds
    the defaults among the exact settings, as it would for a dump of an adapter that follows CRD-1..13, and the noisy frame rules out what
    the smooth one cannot (the sampler's weight bits)."""
    path = os.path.join(ROOT, "tests", "golden", "reftext", name + ".npz")
    if not os.path.exists(path):
        pytest.skip("this fixture of the executed text is not in the tree")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pin_oracle
    g = np.load(path)
    W, H, seed, flags = (int(v) for v in g["synth"])
    assert (W, H, int(g["depth"]), int(g["max_features"])) == (640, 480, 2, 8192)
    _write_dump(tmp_path, int(g["total"]), g["corners"], g["descriptors"], seed, flags)
    S = pin_oracle.setting
    few = [S(), S("clamp"), S("umin"), S("zero", 8), S("zero", 0, 7), S(f16_round=1)]
    _, results, exact = pin_oracle.check(str(tmp_path), few)
    assert S() in exact and S("clamp") not in exact and S("umin") not in exact and S(f16_round=1) not in exact
    if name.endswith("noisy"):
        assert S("zero", 8) not in exact
    assert pin_oracle.neg_angle_policy(g["corners"]) == "zero"


@pytest.mark.parametrize("bins", [8, 30, 1024, 6284])
def test_intended_angle_bins(oracle, numpy_ref, bins):
    """IM-6b: bin = code * N / 6284, rotation by the bin's centre code (bin * 6284 + 3142) / N -- every code against the definition in
    Python integers, C against NumPy on a frame; the centre lies inside its bin, 6284 bins are the identity, and binning never moves a
    keypoint or its reported angle."""
    codes = np.arange(6284)
    want = np.array([((c * bins // 6284) * 6284 + 3142) // bins for c in codes])
    assert np.array_equal(numpy_ref.binned_angle_code(codes, bins), want)
    assert [oracle.binned_angle_code(int(c), bins) for c in codes[::37]] == want[::37].tolist()
    assert np.all(want * bins // 6284 == codes * bins // 6284) and want.max() <= 6283
    if bins == 6284:
        assert np.array_equal(want, codes)
    frame = oracle.synth_frame(320, 240, 5, 15)
    a = oracle.extract_intended(frame, depth=2, threshold=THR, arc=9, nms=True, angle_bins=bins)
    b = numpy_ref.extract_intended(frame, depth=2, threshold=THR, arc=9, use_nms=True, angle_bins=bins)
    ca = np.stack([a["corners"][k] for k in ("x", "y", "angle", "octave")], 1)
    assert a["total"] == b["total"] and np.array_equal(ca, b["corners"]) and np.array_equal(a["descriptors"], b["descriptors"])
    plain = oracle.extract_intended(frame, depth=2, threshold=THR, arc=9, nms=True)
    assert np.array_equal(plain["corners"], a["corners"])


# ---------------------------------------------------------------------------------------------
# The restatement's constants against the reference's TEXT: tests/golden/make_reftext_golden.py cases parses the numbers out of the shaders
# where the reference checkout is at hand and keeps them as digests (tests/golden/reftext_record/constants.json; nothing of the text is kept), which
# are compared here with the constants the two restatements and the kernels' generated tables hold.
# ---------------------------------------------------------------------------------------------
def test_constants_match_the_reference_text(oracle, numpy_ref):
    """Every numeric constant the restatements hold, against what was parsed from the shader text itself: the luminance weights
    (grayscale.wgsl:36), the blur's offsets and weights (gaussian_blur_x.wgsl:14-26), the 4-point and 16-point rings in order
    (fast.wgsl:25-49), the streak shifts (fast.wgsl:56-60), the guard (fast.wgsl:77), the milliradian factors (fast.wgsl:153,
    brief.wgsl:35), the workgroup shapes, and the BRIEF pattern row by row (brief.wgsl:70-327)."""
    import json
    from test_reference_text import CONSTANTS_JSON, digest
    text = json.load(open(CONSTANTS_JSON))
    coefs = [0.229, 0.587, 0.114, 0.0]
    assert text["luminance_weights"] == digest(np.array(coefs, dtype=np.float64))  # 0.229, sic (Q1)
    # ... and the restatement uses exactly their binary32 roundings: one white-red, white-green, white-blue texel each
    for ch, wgt in enumerate(coefs[:3]):
        px = np.zeros((1, 1, 4), dtype=np.uint8)
        px[0, 0, ch] = 255
        assert oracle.grayscale(px)[0, 0] == oracle.f32_to_f16(np.float32(wgt)) == numpy_ref.grayscale(px)[0, 0]
    assert text["blur_offsets"] == digest(np.array(numpy_ref.BLUR_OFF, dtype=np.float32))
    assert text["blur_weights"] == digest(np.array(numpy_ref.BLUR_WGT, dtype=np.float32))
    assert text["blur_sample_count"] == [4, 4]
    assert text["ring4"] == digest(np.array(numpy_ref.RING4, dtype=np.int32)) and text["ring16"] == digest(np.array(numpy_ref.RING16, dtype=np.int32))
    assert text["streak_shifts"] == digest(np.array([6, 3, 2, 1], dtype=np.int32))
    assert text["guard"] == digest(np.array([16, 16, 16, 16], dtype=np.int32))
    assert text["fast_milliradians"], "fast.wgsl: milliradians"
    assert text["brief_milliradians"], "brief.wgsl: milliradians back to radians"
    assert text["brief_pattern"] == digest(np.asarray(numpy_ref.PATTERN, dtype=np.int32))
    # the workgroup shapes the dispatch arithmetic of the restatement assumes (orb.rs:511-515 rounds to 8 x 8 groups; brief: 8 words per feature)
    assert text["workgroups"]
