"""k_front's blur column table of level 0, built once per program (k_blur_col_table, csrc/orb_kernels_front.h) and copied into LDS by
every full-width band of that level, instead of being rebuilt by every band.

* The device table's entries equal the NumPy restatement of the blur's tap positions (oracle/orb_numpy.py, blur_pass), field by
  field, the fractions by bit pattern.
* Extraction through every path that takes the table -- the two specialised 720p instances, the generic ones, 32-row bands in a batch
  that is not a multiple of 8, k_front_pair, Y8 -- equals the oracle's records and descriptors.  The table's only consumers are the
  descriptors of keypoints whose patch reaches the columns right of blur_q: every case first shows the oracle has such keypoints at
  every level.
* Two narrow shapes: a single 200x120 frame, whose 8-row bands have no load slot free for the table and copy it behind the staging
  of the rows, and a batch of 101-column frames (the general level-0 instance).
* A frame with one tiled level (whose bands still build the table themselves: no table pointer) and one that is not equals the oracle."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THR = 8.0 / 255.0  # the noise is faint: at this threshold it gives corners in every band up to the right edge, at every level
NOISE_WEDGES = 4 | 8  # orb_oracle.SYN_WEDGES | SYN_NOISE
SEED0 = 4100


def tap1(numpy_ref, x, w):
    """Tap 1 of the literal blur at columns x of a level w wide -> (i0, i1, fraction): the lines of orb_numpy.blur_pass."""
    F = numpy_ref.F
    fw = F(w)
    u = (np.asarray(x).astype(np.float32) + F(0.5)) / fw
    coord = (u + numpy_ref.BLUR_OFF[1]) * fw - F(0.5)
    c0 = np.floor(coord)
    frac = numpy_ref._weight((coord - c0).astype(np.float32), 0)
    i0 = np.clip(c0.astype(np.int64), 0, w - 1)
    i1 = np.clip(c0.astype(np.int64) + 1, 0, w - 1)
    return i0, i1, frac


def blur_stretches(numpy_ref, w):
    """(blur_p, blur_q): pass 1 is one value per row left of blur_p, the final blur left of blur_q (orb_front_body.inc, phase C)."""
    _, i1, _ = tap1(numpy_ref, np.arange(w), w)
    p = int(np.argmax(i1 != 0)) if np.any(i1 != 0) else w
    q = 0
    if p > 0:
        q = int(np.argmax(i1 >= p)) if np.any(i1 >= p) else w
    return p, q


def expected_table(numpy_ref, tinyorb, w):
    p, q = blur_stretches(numpy_ref, w)
    x = np.arange(q, w)
    j0, j1, f2 = tap1(numpy_ref, x, w)
    out = np.zeros(len(x), dtype=tinyorb.BLUR_COL_DTYPE)
    out["f2"] = f2.view(np.uint32)
    for j, (k0, k1, kf) in ((j0, ("a0", "a1", "fa")), (j1, ("b0", "b1", "fb"))):
        i0, i1, f = tap1(numpy_ref, j, w)
        const = j < p  # that pass-1 column lies in the stretch that is one constant per row
        out[k0] = np.where(const, 0xffff, i0)
        out[k1] = np.where(const, 0, i1)
        out[kf] = np.where(const, np.float32(0.0), f).astype(np.float32).view(np.uint32)
    return out, p, q


@pytest.mark.parametrize("W", [1280, 640, 752, 322, 101])
def test_table_entries(tinyorb, numpy_ref, W):
    """Every entry of the device table against the NumPy restatement, for the widths of the three levels of a depth-3 pyramid on W
    columns.  Only level 0 takes a ready-made table (the levels above build theirs in the band), and an entry depends on the
    level's width alone: each of the three widths is checked as the level 0 of a program of its own; the stretch bounds blur_p,
    blur_q of every level of the depth-3 program are checked against the restatement as well."""
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, 64), max_features=1024, hierarchy_depth=3, initial_threshold=THR, max_batch=2)
    with tinyorb.OrbProgram(cfg).init() as prog:
        assert prog.pipeline() == "fused", prog.pipeline()
        widths = [prog.level_size(lvl)[0] for lvl in range(3)]
        for lvl, w in enumerate(widths):
            got, p, q = prog.blur_col_table(lvl)
            assert (p, q) == blur_stretches(numpy_ref, w), (lvl, w)
            assert len(got) == (w - q if lvl == 0 else 0), (lvl, w, len(got))
    for w in widths:
        cfg = tinyorb.OrbConfig(tinyorb.Extent3d(w, 64), max_features=1024, hierarchy_depth=1, initial_threshold=THR, max_batch=2)
        with tinyorb.OrbProgram(cfg).init() as prog:
            assert prog.pipeline() == "fused", prog.pipeline()
            got, p, q = prog.blur_col_table(0)
        ref, rp, rq = expected_table(numpy_ref, tinyorb, w)
        assert (p, q) == (rp, rq), w
        assert len(got) == w - q and len(got) > 0, (w, len(got))
        for k in tinyorb.BLUR_COL_DTYPE.names:
            assert np.array_equal(got[k], ref[k]), "field %s at width %d" % (k, w)


_REF = {}


def reference(oracle, numpy_ref, W, H, depth, n, y8=False):
    """(frames, per frame the oracle's sorted records and descriptors); computed once per shape.  Shows that the oracle has, at every
    level, a keypoint whose patch reaches the columns the table describes (x > blur_q - 18)."""
    key = (W, H, depth, n, y8)
    if key not in _REF:
        synth = oracle.synth_frame_y8 if y8 else oracle.synth_frame
        frames = np.stack([synth(W, H, SEED0 + i, NOISE_WEDGES) for i in range(n)])
        cap = W * H // 2  # several times what these frames give (asserted below): no record is lost to the capacity
        refs = []
        for f in frames:
            r = (oracle.extract_y8 if y8 else oracle.extract)(f, depth=depth, threshold=THR, max_features=cap)
            assert r["total"] <= cap
            rc, rd = oracle.sort_keypoints(r["corners"], r["descriptors"])
            for m in range(depth):
                _, q = blur_stretches(numpy_ref, W >> m)
                assert np.any((rc["octave"] == m) & (rc["x"].astype(np.int64) > q - 18)), "no keypoint right of blur_q - 18 at level %d" % m
            refs.append((r["total"], rc, rd))
        _REF[key] = (frames, cap, refs)
    return _REF[key]


def assert_frame(got_total, corners, desc, ref, what):
    total, rc, rd = ref
    assert got_total == total, what
    order = np.lexsort((corners["x"], corners["y"], corners["octave"]))
    assert np.array_equal(corners[order], rc), "records of " + what
    assert np.array_equal(desc[order], rd), "descriptors of " + what


def run_batch(tinyorb, oracle, numpy_ref, W, H, depth, n, y8=False):
    frames, cap, refs = reference(oracle, numpy_ref, W, H, depth, n, y8)
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W, H), max_features=cap, hierarchy_depth=depth, initial_threshold=THR, max_batch=n,
                            flags=tinyorb.ORB_FLAG_INPUT_Y8 if y8 else 0)
    with tinyorb.OrbProgram(cfg).init() as prog:
        assert prog.pipeline() == "fused", prog.pipeline()
        tables = [len(prog.blur_col_table(m)[0]) for m in range(depth)]
        prog.extract_batch_host(frames)
        counts = prog.batch_counts(n)
        for i in range(n):
            corners, desc = prog.batch_read(i, int(counts[i]))
            assert_frame(int(counts[i]), corners, desc, refs[i], "frame %d" % i)
    return tables


def took(capfd, depth):
    """What each level's TINYORB_FRONT_TRACE line says the launch takes."""
    err = capfd.readouterr().err
    t = {int(m.group(1)): m.group(2) for m in re.finditer(r"tinyorb: k_front level (\d+) .* takes the (\S+)(?: \S+)? instance", err)}
    assert sorted(t) == list(range(depth)), err[-2000:]
    return t


@pytest.mark.parametrize("generic", [False, True])
def test_720p_batch(tinyorb, oracle, numpy_ref, monkeypatch, capfd, generic):
    """Eight 1280x720 frames: the two specialised instances, and the generic ones under TINYORB_FRONT_GENERIC=1."""
    monkeypatch.setenv("TINYORB_FRONT_TRACE", "1")
    monkeypatch.delenv("TINYORB_BAND_ROWS", raising=False)
    if generic:
        monkeypatch.setenv("TINYORB_FRONT_GENERIC", "1")
    else:
        monkeypatch.delenv("TINYORB_FRONT_GENERIC", raising=False)
    assert run_batch(tinyorb, oracle, numpy_ref, 1280, 720, 2, 8) == [1280 - 1125, 0]  # level 0 takes the ready-made table, level 1 builds its own
    want = "generic" if generic else "specialised"
    assert took(capfd, 2) == {0: want, 1: want}


def test_32_row_bands_odd_batch(tinyorb, oracle, numpy_ref):
    """Three 640x480 frames at depth 3: generic instances, 32-row bands, a batch that is not a multiple of 8."""
    tables = run_batch(tinyorb, oracle, numpy_ref, 640, 480, 3, 3)
    assert tables[0] > 0 and tables[1:] == [0, 0], tables


def test_y8_batch(tinyorb, oracle, numpy_ref):
    tables = run_batch(tinyorb, oracle, numpy_ref, 640, 480, 2, 8, y8=True)
    assert tables[0] > 0 and tables[1] == 0, tables


def test_single_frame_pair(tinyorb, oracle, numpy_ref):
    """One 1280x720 frame through extract_corners: k_front_pair, 8-row bands, level 1 staged from the frame."""
    frames, cap, refs = reference(oracle, numpy_ref, 1280, 720, 2, 8)
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(1280, 720), max_features=cap, hierarchy_depth=2, initial_threshold=THR)
    with tinyorb.OrbProgram(cfg).init() as prog:
        assert prog.pipeline() == "fused", prog.pipeline()
        total, corners, desc = prog.extract(frames[0])
    assert_frame(total, corners, desc, refs[0], "the frame")


def test_narrow_single_frame(tinyorb, oracle, numpy_ref):
    """One 200x120 frame through extract_corners: 8-row bands of 50 items a row, so the 14 staged rows are 700 items on 1024
    threads -- not every thread stages a row, no load slot is free by the rule the wide shapes use, and the band copies the table
    behind the staging instead.  25 entries: the last 16-byte piece is half entry, half zeros."""
    frames, cap, refs = reference(oracle, numpy_ref, 200, 120, 2, 1)
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(200, 120), max_features=cap, hierarchy_depth=2, initial_threshold=THR)
    with tinyorb.OrbProgram(cfg).init() as prog:
        assert prog.pipeline() == "fused", prog.pipeline()
        assert len(prog.blur_col_table(0)[0]) == 25
        total, corners, desc = prog.extract(frames[0])
    assert_frame(total, corners, desc, refs[0], "the frame")


def test_narrow_odd_width_batch(tinyorb, oracle, numpy_ref):
    """Two 101x80 frames: the general level-0 instance (a width that is no multiple of 4), which always copies the table behind
    the staging; 64-row bands, a table of 12 entries."""
    assert run_batch(tinyorb, oracle, numpy_ref, 101, 80, 1, 2) == [12]


def test_tiled_level_beside_full_width_level(tinyorb, oracle, numpy_ref):
    """2560x720: level 0 runs on column tiles and the program has no table at all -- the bands of both levels, the tiled one and the
    full-width one beside it, build theirs: the null-pointer path.  Still the oracle's records and descriptors."""
    assert run_batch(tinyorb, oracle, numpy_ref, 2560, 720, 2, 1) == [0, 0]
