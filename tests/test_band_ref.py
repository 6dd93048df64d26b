"""CPU checks of the epipolar-band restatement (tests/band_ref.py, EB-1..EB-4 of DESIGN.md section 18) and of the OrbBandParams
layout: hand-built known answers on the sideways-translation F, the scaled band, ties and `second`, queries without a line, and the
equivalences EB-6 (a), (b) and (c) against a dense brute-force argmin on random records."""
import ctypes
import os
import re

import numpy as np

import band_ref as br
import constructed as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
NONE = 0xFFFFFFFF
NOREC = (NONE, 0xFFFF, 0xFFFF)


def _desc(bits):
    """One descriptor per entry: the first `b` bits set."""
    d = np.zeros((len(bits), 8), np.uint32)
    for k, b in enumerate(bits):
        v = np.zeros(256, np.uint8)
        v[:b] = 1
        d[k] = np.packbits(v, bitorder="little").view(np.uint32)
    return d


def _rec(out, i):
    return int(out["index"][i]), int(out["distance"][i]), int(out["second"][i])


def _xy(points, octave=0):
    p = np.asarray(points, np.int64).reshape(-1, 2)
    return C.corners(p[:, 0], p[:, 1], octave)


def test_sideways_line_band_edges_ties_and_second():
    """F of a pure sideways translation: the line of (x, y) is y' = y, n2 = 1, so the test is (y_j - y)^2 <= d^2 exactly."""
    q = _xy([(50, 40), (10, 100)])
    qd = _desc([0, 0])
    #            |dy| 2     3         0         2 (tie with 0)  1, far in x
    t = _xy([(90, 42), (51, 43), (120, 40), (5, 38), (150, 41)])
    td = _desc([4, 1, 9, 4, 6])
    a0, a1, a2, tt, ok = br.lines(br.SIDEWAYS, *br.level0(q), np.float32([2, 2]))
    assert a0.tolist() == [0, 0] and a1.tolist() == [-1, -1] and a2.tolist() == [40, 100] and tt.tolist() == [4, 4] and ok.all()
    out = br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, cap=4)
    assert _rec(out, 0) == (0, 4, 4)  # |dy| = 2 is in, 3 (the closest descriptor) is out; the tie at 4 goes to the smaller j
    assert _rec(out, 1) == NOREC      # nothing near y = 100
    assert _rec(out, 2) == _rec(out, 3) == NOREC  # past n_q
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS), 0) == (0, 4, 4)  # band_px 0 is the default 2.0
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=3.0), 0) == (1, 1, 4)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=1.0), 0) == (4, 6, 9)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=0.5), 0) == (2, 9, 0xFFFF)  # one candidate
    # the window around the query's own position: inclusive edge (|dx| = 40 at j = 0), and the band still applies
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=40.0), 0) == (0, 4, 0xFFFF)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=39.0), 0) == NOREC
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=3.0, radius_px=39.0), 0) == (1, 1, 0xFFFF)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=45.0), 0) == (0, 4, 4)  # (5, 38) at |dx| = 45


def test_scaled_band_and_octave_window():
    """ORB_BAND_SCALE at octave 1: d = 2 * 2 = 4 around y = 2 * 20 + 0.5; octave-1 targets at level-0 |dy| = 4 (in) and 6 (out),
    an octave-0 target at |dy| = 4.5 (out) and one at 3.5 (in)."""
    q = C.corners([30], [20], 1)
    qd = _desc([0])
    t = C.corners([40, 41, 70, 71], [22, 23, 45, 44], [1, 1, 0, 0])  # y: 44.5, 46.5, 45, 44
    td = _desc([5, 1, 2, 7])
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0), 0) == NOREC  # unscaled: nothing within 2 of 40.5
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, scale=True), 0) == (0, 5, 7)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, scale=True, octave_window=1), 0) == (0, 5, 0xFFFF)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, scale=True, octave_window=2), 0) == (0, 5, 7)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=3.0, scale=True), 0) == (1, 1, 2)  # d = 6: |dy| = 6 and 4.5 come in
    # the window scales too: the query is at x = 60.5, j = 0 at 80.5 (|dx| = 20 = 10 * 2^1), j = 3 at 71
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=10.0, scale=True), 0) == (0, 5, 7)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=9.5, scale=True), 0) == (3, 7, 0xFFFF)
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=5.0, scale=True), 0) == NOREC
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, radius_px=20.0), 0) == NOREC  # unscaled, the band is 2 again


def test_scaled_band_on_integer_offsets():
    """The issue's second known answer: ORB_BAND_SCALE at octave 1 with d = 2 admits a level-0 offset of 4 and refuses 5."""
    q = C.corners([30], [20], 1)  # y = 40.5
    qd = _desc([0])
    t = C.corners([10, 11, 12, 13], [22, 18, 45, 11], [1, 1, 0, 2])  # y = 44.5 (|dy| = 4), 36.5 (4), 45 (4.5), 45.5 (5)
    td = _desc([3, 2, 1, 1])
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS, band_px=2.0, scale=True), 0) == (1, 2, 3)
    q0 = _xy([(30, 40)])
    t0 = _xy([(10, 44), (11, 45), (12, 36), (13, 35)])
    out = br.band_pair(q0, qd, t0, _desc([3, 1, 2, 1]), br.SIDEWAYS, band_px=4.0)
    assert _rec(out, 0) == (2, 2, 3)  # 4 in, 5 out, on both sides


def test_queries_without_a_line():
    q = _xy([(10, 10), (50, 10)])
    qd = _desc([0, 0])
    t = _xy([(10, 10), (50, 10)])
    td = _desc([1, 2])
    assert all(_rec(br.band_pair(q, qd, t, td, np.zeros(9, np.float32), band_px=1e6), i) == NOREC for i in range(2))  # EB-6 (b)
    assert all(_rec(br.band_pair(q, qd, t, td, None, band_px=1e6), i) == NOREC for i in range(2))  # a pair without a model
    for bad in (np.nan, np.inf, -np.inf):
        for e in range(9):
            m = br.SIDEWAYS.copy()
            m[e] = bad
            assert all(_rec(br.band_pair(q, qd, t, td, m, band_px=1e6), i) == NOREC for i in range(2)), (bad, e)
    # an epipole inside the frame: F = [e]_x with e = (50, 10, 1); the query at e has a0 = a1 = 0 (n2 < 2^-64), the other a line through e
    ex, ey = 50.0, 10.0
    epi = np.array([0, -1, ey, 1, 0, -ex, -ey, ex, 0], np.float32)
    out = br.band_pair(q, qd, t, td, epi, band_px=1.0)
    assert _rec(out, 1) == NOREC and _rec(out, 0) == (0, 1, 2)  # the line of (10, 10) is y = 10: both targets lie on it
    # the floor on n2 alone: a line with |(a0, a1)| = 2^-33 is refused, 2^-31 is kept
    for s, want in ((2.0 ** -33, NOREC), (2.0 ** -31, (0, 1, 2))):
        assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS * np.float32(s), band_px=1.0), 0) == want
    # t overflows although the line is finite: no line
    assert _rec(br.band_pair(q, qd, t, td, br.SIDEWAYS * np.float32(1e19), band_px=1e6), 0) == NOREC


def test_model_sources():
    from tinyslam_amd import orb
    v = np.zeros(3, dtype=orb.VERIFY_MODEL_DTYPE)
    v["h"] = np.arange(27, dtype=np.float32).reshape(3, 9)
    v["status"] = [orb.ORB_VERIFY_OK, orb.ORB_VERIFY_DEGENERATE, orb.ORB_VERIFY_MINIMAL]
    assert br.model_of(orb.ORB_BAND_VERIFIED, 0, vmodels=v).tolist() == list(range(9))
    assert br.model_of(orb.ORB_BAND_VERIFIED, 1, vmodels=v) is None
    assert br.model_of(orb.ORB_BAND_VERIFIED, 2, vmodels=v)[0] == 18
    assert br.model_of(orb.ORB_BAND_HOST, 1, host=np.arange(18, dtype=np.float32).reshape(2, 3, 3))[0] == 9


def _random_records(rng, n, W, H, depth, few_descriptors):
    o = rng.integers(0, depth, n)
    c = C.corners(rng.integers(0, W, n) >> o, rng.integers(0, H, n) >> o, o)
    d = rng.integers(0, 4, (n, 32)).astype(np.uint8).view(np.uint32) if few_descriptors else C.random_desc(rng, n)
    return c, np.ascontiguousarray(d).reshape(n, 8)


def _general_f(rng):
    """A fundamental matrix of a general motion, for coordinates of a few hundred pixels."""
    A = rng.normal(size=(3, 3))
    tx = rng.normal(size=3)
    T = np.array([[0, -tx[2], tx[1]], [tx[2], 0, -tx[0]], [-tx[1], tx[0], 0]])
    K = np.array([[300.0, 0, 160], [0, 300.0, 120], [0, 0, 1]])
    F = np.linalg.inv(K).T @ T @ (np.eye(3) + 0.1 * A) @ np.linalg.inv(K)
    return (F / np.abs(F).max()).astype(np.float32).reshape(9)


def test_eb6a_covering_band_equals_brute_force():
    rng = np.random.default_rng(5)
    for nq, nt in ((200, 300), (1, 1), (50, 1), (0, 10), (10, 0)):
        q, qd = _random_records(rng, nq, 320, 240, 3, True)  # few distinct descriptors: many ties
        t, td = _random_records(rng, nt, 320, 240, 3, True)
        for m in (br.SIDEWAYS, _general_f(rng)):
            out = br.band_pair(q, qd, t, td, m, band_px=1e6)
            a0, a1, a2, tt, ok = br.lines(m, *br.level0(q), np.full(nq, 1e6, np.float32))
            want = C.match_ref(qd, td)
            want[~ok] = NOREC
            assert out.tobytes() == want.tobytes(), (nq, nt)
            assert nq == 0 or ok.mean() > 0.9


def test_eb6c_best_in_band_keeps_index_and_distance():
    rng = np.random.default_rng(6)
    q, qd = _random_records(rng, 300, 320, 240, 2, False)
    t, td = _random_records(rng, 400, 320, 240, 2, False)
    bf = C.match_ref(qd, td)
    hits = 0
    for m, kw in ((br.SIDEWAYS, dict(band_px=30.0)), (_general_f(rng), dict(band_px=12.0)), (_general_f(rng), dict(band_px=30.0, radius_px=90.0))):
        out = br.band_pair(q, qd, t, td, m, **kw)
        qq, tj = br.members(q, t, m, **kw)
        inside = np.zeros(len(q), bool)
        inside[qq[tj == bf["index"][qq]]] = True
        hits += int(inside.sum())
        assert np.array_equal(out["index"][inside], bf["index"][inside]) and np.array_equal(out["distance"][inside], bf["distance"][inside])
        assert np.all(out["second"][inside] >= bf["second"][inside])
        # and every record is the restricted argmin, read literally from the candidate list
        for i in range(len(q)):
            js = tj[qq == i]
            d = sorted(zip(C.hamming(qd[i][None], td[js]).tolist(), js.tolist()))
            assert _rec(out, i) == (d[0][1] if d else NONE, d[0][0] if d else 0xFFFF, d[1][0] if len(d) > 1 else 0xFFFF), i
    assert hits > 20


def test_band_params_layout(tinyorb):
    assert ctypes.sizeof(tinyorb._BandParams) == 32
    names = ["source", "band_px", "radius_px", "octave_window", "flags", "reserved"]
    assert [getattr(tinyorb._BandParams, k).offset for k in names] == [0, 4, 8, 12, 16, 20]
    text = open(HEADER).read()
    fields = re.search(r"typedef struct \{([^}]*)\} OrbBandParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(?:u?int32_t|float)\s+(\w+)", fields, re.M) == names
    consts = dict(re.findall(r"#define\s+(ORB_BAND_[A-Z_]+)\s+(\d+)u?\b", text))
    assert sorted(consts) == ["ORB_BAND_HOST", "ORB_BAND_SCALE", "ORB_BAND_VERIFIED"]
    for k in consts:
        assert int(consts[k]) == getattr(tinyorb, k), k
    sigs = dict(re.findall(r"^int (orb_match_epipolar\w*)\(([^)]*)\);", text, re.M))
    assert sigs == {"orb_match_epipolar": "OrbProgram *p, uint32_t n_frames, const OrbBandParams *params, const float *models_host, void *stream",
                    "orb_match_epipolar_read": "OrbProgram *p, uint32_t frame, OrbMatch *dst, size_t n"}


def test_abi_without_device(tinyorb):
    L = tinyorb.load_library()
    for n in ("orb_match_epipolar", "orb_match_epipolar_read"):
        assert n in tinyorb.EXPORTS and hasattr(L, n)
    prm = tinyorb._BandParams()
    assert L.orb_match_epipolar(None, 2, ctypes.byref(prm), None, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_epipolar(None, 2, None, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_epipolar_read(None, 0, None, 0) == tinyorb.ORB_EINVAL
    assert L.orb_abi_version() == 5
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("band" in n for n in names)
