"""CPU checks of the guided-matching restatement (tests/guided_ref.py, GM-1..GM-4 of DESIGN.md section 14) and of the
OrbGuideParams layout: hand-built known answers, the octave window, the scaled radius, predictions without a window, and the
restatement with a window over the whole frame against a dense brute-force argmin."""
import ctypes
import os
import re

import numpy as np

import guided_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tinyorb.h")
NONE = 0xFFFFFFFF


def _corners(xy, octave=None):
    from tinyslam_amd import orb
    c = np.zeros(len(xy), dtype=orb.CORNER_DTYPE)
    if len(xy):
        c["x"], c["y"] = np.asarray(xy, dtype=np.uint32).T
    if octave is not None:
        c["octave"] = octave
    return c


def _desc(bits):
    """One descriptor per entry: the first `b` bits set."""
    from tinyslam_amd import orb
    d = np.zeros(len(bits), dtype=orb.DESCRIPTOR_DTYPE)
    for k, b in enumerate(bits):
        v = np.zeros(256, np.uint8)
        v[:b] = 1
        d["bits"][k] = np.packbits(v, bitorder="little")
    return d


def _rec(out, i):
    return int(out["index"][i]), int(out["distance"][i]), int(out["second"][i])


def test_known_answers_tie_second_empty_single():
    q = _corners([(10, 10), (100, 100), (300, 10)])
    qd = _desc([0, 0, 0])
    # targets near query 0: j=0 and j=2 both at distance 3 (tie -> 0), j=1 at 5; j=3 near query 1 alone; none near query 2
    t = _corners([(12, 9), (8, 11), (10, 13), (101, 99), (40, 40)])
    td = _desc([3, 5, 3, 7, 0])
    out = gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=4.0, cap=5)
    assert _rec(out, 0) == (0, 3, 3)          # tie to the smallest j, second = the other 3
    assert _rec(out, 1) == (3, 7, 0xFFFF)     # one candidate
    assert _rec(out, 2) == (NONE, 0xFFFF, 0xFFFF)  # empty window
    assert _rec(out, 3) == _rec(out, 4) == (NONE, 0xFFFF, 0xFFFF)  # past n_q
    # the window's edge is inclusive: |dx| = r is in, r + 1 is out
    out = gr.guided_pair(q[:1], qd[:1], t, td, gr.IDENTITY, radius_px=3.0)
    assert _rec(out, 0) == (0, 3, 3)
    out = gr.guided_pair(q[:1], qd[:1], t, td, gr.IDENTITY, radius_px=2.0)
    assert _rec(out, 0) == (0, 3, 5)  # (12, 9) and (8, 11) are within 2; (10, 13) is not
    # radius 0 means the default 16: the far target (40, 40) stays out, (101, 99) too
    out = gr.guided_pair(q[:1], qd[:1], t, td, gr.IDENTITY, radius_px=0.0)
    assert _rec(out, 0) == (0, 3, 3)


def test_octave_window_and_scaled_radius():
    # level-0 centres: octave 1 pixel (x, y) -> (2x + 0.5, 2y + 0.5)
    q = _corners([(20, 20)], octave=[1])   # (40.5, 40.5)
    qd = _desc([0])
    t = _corners([(40, 40), (20, 20), (10, 10), (22, 20)], octave=[0, 1, 2, 1])  # (40, 40), (40.5, 40.5), (41.5, 41.5), (44.5, 40.5)
    td = _desc([1, 2, 3, 4])
    assert _rec(gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=3.0), 0) == (0, 1, 2)
    assert _rec(gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=3.0, octave_window=1), 0) == (1, 2, 0xFFFF)
    assert _rec(gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=3.0, octave_window=2), 0) == (0, 1, 2)
    # scale_radius: r = 2 * 2^1 = 4 reaches (44.5, 40.5) at dx = 4; without it r = 2 does not
    assert _rec(gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=2.0, octave_window=1), 0) == (1, 2, 0xFFFF)
    assert _rec(gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=2.0, octave_window=1, scale_radius=True), 0) == (1, 2, 4)


def test_models_without_prediction():
    q = _corners([(10, 10), (50, 10)])
    qd = _desc([0, 0])
    t = _corners([(10, 10), (50, 10)])
    td = _desc([1, 2])
    # w = -x / 20 + 2: positive at x = 10, zero at x = 40, negative at 50
    m = np.array([1, 0, 0, 0, 1, 0, -0.05, 0, 2], np.float32)
    px, py, ok = gr.predict(m, np.float32([10, 40, 50]), np.float32([10, 10, 10]))
    assert ok.tolist() == [True, False, False]
    out = gr.guided_pair(q, qd, t, td, m, radius_px=1e6)
    assert _rec(out, 0)[0] in (0, 1) and _rec(out, 1) == (NONE, 0xFFFF, 0xFFFF)
    nan = gr.IDENTITY.copy()
    nan[4] = np.nan
    out = gr.guided_pair(q, qd, t, td, nan, radius_px=1e6)
    assert all(_rec(out, i) == (NONE, 0xFFFF, 0xFFFF) for i in range(2))
    inf = gr.IDENTITY.copy()
    inf[2] = np.inf
    assert all(_rec(gr.guided_pair(q, qd, t, td, inf, radius_px=1e6), i)[0] == NONE for i in range(2))
    assert all(_rec(gr.guided_pair(q, qd, t, td, None), i)[0] == NONE for i in range(2))  # a pair without a model


def test_model_sources():
    from tinyslam_amd import orb
    v = np.zeros(3, dtype=orb.VERIFY_MODEL_DTYPE)
    v["h"] = np.arange(27, dtype=np.float32).reshape(3, 9)
    v["status"] = [orb.ORB_VERIFY_OK, orb.ORB_VERIFY_FEW, orb.ORB_VERIFY_MINIMAL]
    assert gr.model_of(orb.ORB_GUIDE_VERIFIED, 0, vmodels=v).tolist() == list(range(9))
    assert gr.model_of(orb.ORB_GUIDE_VERIFIED, 1, vmodels=v) is None
    assert gr.model_of(orb.ORB_GUIDE_VERIFIED, 2, vmodels=v)[0] == 18
    assert gr.model_of(orb.ORB_GUIDE_IDENTITY, 7).tolist() == np.eye(3).reshape(9).tolist()
    host = np.arange(18, dtype=np.float32).reshape(2, 3, 3)
    assert gr.model_of(orb.ORB_GUIDE_HOST, 1, host=host)[0] == 9


def test_full_window_equals_brute_force():
    rng = np.random.default_rng(3)
    for nq, nt in ((200, 300), (1, 1), (50, 1), (0, 10), (10, 0)):
        q = _corners(np.c_[rng.integers(0, 320, nq), rng.integers(0, 240, nq)].reshape(-1, 2), octave=rng.integers(0, 3, nq))
        t = _corners(np.c_[rng.integers(0, 320, nt), rng.integers(0, 240, nt)].reshape(-1, 2), octave=rng.integers(0, 3, nt))
        from tinyslam_amd import orb
        qd = np.zeros(nq, dtype=orb.DESCRIPTOR_DTYPE)
        td = np.zeros(nt, dtype=orb.DESCRIPTOR_DTYPE)
        # few distinct descriptors: many ties
        qd["bits"] = rng.integers(0, 4, (nq, 32)).astype(np.uint8)
        td["bits"] = rng.integers(0, 4, (nt, 32)).astype(np.uint8)
        out = gr.guided_pair(q, qd, t, td, gr.IDENTITY, radius_px=1e6)
        assert out.tobytes() == gr.brute_force(qd, td).tobytes(), (nq, nt)


def test_small_window_is_the_restricted_argmin():
    """Every record against a per-query loop over the window (the definition read literally)."""
    from tinyslam_amd import orb
    rng = np.random.default_rng(8)
    nq, nt = 120, 150
    q = _corners(np.c_[rng.integers(0, 160, nq), rng.integers(0, 120, nq)], octave=rng.integers(0, 2, nq))
    t = _corners(np.c_[rng.integers(0, 160, nt), rng.integers(0, 120, nt)], octave=rng.integers(0, 2, nt))
    qd = np.zeros(nq, dtype=orb.DESCRIPTOR_DTYPE)
    td = np.zeros(nt, dtype=orb.DESCRIPTOR_DTYPE)
    qd["bits"] = rng.integers(0, 256, (nq, 32)).astype(np.uint8)
    td["bits"] = rng.integers(0, 256, (nt, 32)).astype(np.uint8)
    m = np.array([1.01, 0.02, 3.5, -0.01, 0.99, -2.0, 1e-4, -2e-4, 1.0], np.float32)
    for r, ow, sc in ((6.0, 0, False), (9.5, 1, False), (4.0, 2, True)):
        out = gr.guided_pair(q, qd, t, td, m, radius_px=r, octave_window=ow, scale_radius=sc)
        xq, yq = gr.level0(q)
        xt, yt = gr.level0(t)
        px, py, ok = gr.predict(m, xq, yq)
        for i in range(nq):
            rr = np.float32(r) * np.float32(2 ** int(q["octave"][i])) if sc else np.float32(r)
            win = [j for j in range(nt) if abs(xt[j] - px[i]) <= rr and abs(yt[j] - py[i]) <= rr
                   and (not ow or abs(int(t["octave"][j]) - int(q["octave"][i])) < ow)]
            d = sorted((int(np.unpackbits(qd["bits"][i] ^ td["bits"][j]).sum()), j) for j in win)
            want = (d[0][1] if d else NONE, d[0][0] if d else 0xFFFF, d[1][0] if len(d) > 1 else 0xFFFF)
            assert _rec(out, i) == want, (r, ow, sc, i)


def test_guide_params_layout(tinyorb):
    assert ctypes.sizeof(tinyorb._GuideParams) == 32
    assert [getattr(tinyorb._GuideParams, k).offset for k in ("source", "radius_px", "octave_window", "flags", "reserved")] == \
        [0, 4, 8, 12, 16]
    text = open(HEADER).read()
    fields = re.search(r"typedef struct \{([^}]*)\} OrbGuideParams;", text, re.S).group(1)
    assert re.findall(r"^\s*(?:u?int32_t|float)\s+(\w+)", fields, re.M) == ["source", "radius_px", "octave_window", "flags", "reserved"]
    consts = dict(re.findall(r"#define\s+(ORB_GUIDE_[A-Z_]+)\s+(\d+)u?\b", text))
    for k in ("ORB_GUIDE_VERIFIED", "ORB_GUIDE_IDENTITY", "ORB_GUIDE_HOST", "ORB_GUIDE_SCALE_RADIUS"):
        assert int(consts[k]) == getattr(tinyorb, k), k


def test_abi_without_device(tinyorb):
    L = tinyorb.load_library()
    prm = tinyorb._GuideParams()
    assert L.orb_match_guided(None, 2, ctypes.byref(prm), None, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_guided(None, 2, None, None, None) == tinyorb.ORB_EINVAL
    assert L.orb_match_guided_read(None, 0, None, 0) == tinyorb.ORB_EINVAL
    names = [L.orb_kernel_name(i).decode() for i in range(tinyorb.ORB_KERNEL_COUNT)]
    assert tinyorb.ORB_KERNEL_COUNT == 25 and not any("guide" in n for n in names)
