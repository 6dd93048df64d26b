"""The batches of tests/test_gpu_bridge_cases.py on the CPU (tests/bridge_cases.py through tests/bridge_ref.py):
that each is laid out as its docstring says -- where k_br_chain's chunks of 64 frames cut long_batch and what the restatement
gives on either side, the hop limit on hop_batch, the two joins of double_batch, BR-5's edges on edge_batch -- and that no record
of any of them holds a NaN (a NaN's sign and payload are undefined: such a case cannot be compared byte for byte)."""
import numpy as np

import bridge_cases as B
import trajectory_ref as tr

F = np.float32
U = np.uint32
CHAINED, START, LOST, ORIGIN = B.CHAINED, B.START, B.LOST, B.ORIGIN
COPIED, MOVED, FIXED, JOINED, UNFIXED = B.COPIED, B.MOVED, B.FIXED, B.JOINED, B.UNFIXED
NAMES = {COPIED: "COPIED", MOVED: "MOVED", FIXED: "FIXED", JOINED: "JOINED", UNFIXED: "UNFIXED"}
FIXES = {B.L_OK: "OK", B.L_NOMAP: "NOMAP", B.L_FEW: "FEW", B.L_DEGENERATE: "DEGENERATE", B.L_MINIMAL: "MINIMAL"}
_CACHE = {}


def _no_nan(fr, out):
    for rec in (fr, out):
        for k in ("r", "t", "scale") + (("gain",) if "gain" in rec.dtype.names else ("step",) if "step" in rec.dtype.names else ()):
            assert not np.isnan(rec[k]).any(), k


def _long():
    if "long" not in _CACHE:
        b = B.long_batch()
        trace = {}
        _CACHE["long"] = (b,) + B.reference(b, traj=B.LONG_TRAJ, trace=trace, **B.LONG) + (trace,)
    return _CACHE["long"]


def test_long_batch_layout_across_the_chunks():
    b, fr, lms, out, masks, trace = _long()
    n, st, ts = b["n"], out["status"].tolist(), fr["status"].tolist()
    assert n == 327 >= 131 and b["cap"] == 96 and (b["W"], b["H"]) == (64, 48)
    _no_nan(fr, out)
    # (a) a JOINED frame of one chunk, frames of the next MOVED through it: br_similarity reads a record of the chunk before
    assert st[190] == JOINED and st[191:195] == [MOVED] * 4 and fr["origin"][191:195].tolist() == [190] * 4
    assert out["root"][190:195].tolist() == [186] * 5 and (out["gain"][191:195] == out["gain"][190]).all()
    assert st[60] == JOINED and st[61:64] == [MOVED] * 3 and out["root"][56:69].tolist() == [56] * 13
    # (b) frame 64 is a gap end with anchor 63 and joins: RT, tT and oT were set in the chunk before, root != oT, the gain a product
    assert ts[63] == CHAINED and ts[64] == LOST and ts[65] == START and st[64] == JOINED and out["anchor"][64] == 63
    assert fr["origin"][63] == 60 and out["root"][64] == 56 and st[65:69] == [MOVED] * 4
    g60, g64 = trace[60]["join"][1], trace[64]["join"][1]
    assert out["gain"][60] == g60 and out["gain"][64].tobytes() == F(g60 * g64).tobytes() and g60 != 1 and g64 != 1
    assert out["gain"][68] == out["gain"][64] and out["scale"][66].tobytes() == F(out["gain"][64] * fr["scale"][66]).tobytes()
    # (c) a gap of two frames with its anchor in the chunk before 128 and its ends at 128 and behind it
    assert ts[127] == CHAINED and ts[128:131] == [LOST, LOST, START] and out["anchor"][128:130].tolist() == [127, 127]
    assert st[128:133] == [FIXED, JOINED] + [MOVED] * 3 and out["root"][120:133].tolist() == [120] * 13
    assert st[124] == JOINED and out["gain"][129].tobytes() == F(trace[124]["join"][1] * trace[129]["join"][1]).tobytes()
    # (d) a run's first frame, LOST behind unrelated matches, on each side of a boundary: the last frame of a chunk, the first of one
    first = set(b["first"].tolist())
    for f in (255, 320):
        assert f in first and ts[f] == LOST and ts[f + 1] == START and out["fix"][f] != B.L_NOMAP and out["candidates"][f] > 0
        assert out["inliers"][f] <= 6 and out["root"][f + 1] == f  # no model among wrong matches; the run is its own map
    assert 255 % B.CHUNK == B.CHUNK - 1 and 320 % B.CHUNK == 0
    # (e) every status in every chunk of 20 frames or more; the census
    for c in range(0, n, B.CHUNK):
        chunk = out[c:c + B.CHUNK]
        census = {NAMES[s]: int((chunk["status"] == s).sum()) for s in NAMES}
        fixes = {FIXES[s]: int(((chunk["fix"] == s) & (fr["status"][c:c + B.CHUNK] == LOST)).sum()) for s in FIXES}
        print("frames %d..%d" % (c, c + len(chunk) - 1), census, "fixes of LOST frames", fixes)
        if len(chunk) >= 20:
            assert all(census.values()), (c, census)
            assert fixes["OK"] >= 5 and fixes["MINIMAL"] >= 1, (c, fixes)
    assert [sum(1 for s in st if s == k) for k in (COPIED, MOVED, FIXED, JOINED, UNFIXED)] == [158, 81, 16, 32, 40]


def test_long_batch_cuts_at_the_boundaries():
    """The shorter calls the GPU test makes: at 65 frames frame 64 is the last and cannot join; at 66 it joins."""
    b, fr, lms, out, masks, trace = _long()
    for n in (63, 64, 65, 66, 128, 129):
        frn, _, o, _ = B.reference(b, n, traj=B.LONG_TRAJ, **B.LONG)
        _no_nan(frn, o)
        assert o[:n - 1]["status"].tolist() == out[:n - 1]["status"].tolist()
        assert o["status"][n - 1] == {65: FIXED, 129: FIXED}.get(n, out["status"][n - 1]), n
    o66 = B.reference(b, 66, traj=B.LONG_TRAJ, **B.LONG)[2]
    assert o66[64].tobytes() == out[64].tobytes() and o66["status"][65] == MOVED
    one = B.reference(b, traj=B.LONG_TRAJ, **B.LONG, max_hops=1)[2]
    assert one["status"][128:131].tolist() == [FIXED, UNFIXED, COPIED] and one["fix"][129] == B.L_NOMAP and one["root"][130] == 129


def test_hop_batch_at_the_hop_limit():
    b = B.hop_batch()
    assert b["n"] == 24 and b["cap"] == 256
    for hops, fixed in ((16, 16), (15, 15), (4, 4)):
        fr, lms, out, masks = B.reference(b, traj=B.LONG_TRAJ, max_hops=hops, **B.LONG)
        _no_nan(fr, out)
        assert fr["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED] + [LOST] * 17 + [START, CHAINED, CHAINED]
        assert out["status"].tolist() == [COPIED] * 4 + [FIXED] * fixed + [UNFIXED] * (17 - fixed) + [COPIED] * 3
        assert (out["anchor"][4:21] == 3).all() and (out["fix"][4:4 + fixed] == B.L_OK).all() and (out["fix"][4 + fixed:21] == B.L_NOMAP).all()
        assert out["root"].tolist() == [0] * (4 + fixed) + list(range(4 + fixed, 21)) + [20] * 3
        cand = out["candidates"][4:4 + fixed].astype(int)
        print("max_hops", hops, "candidates", cand.tolist())
        assert (np.diff(cand) < 0).all() and cand[-1] >= 100 and not out["candidates"][4 + fixed:].any()  # fewer at every hop


def test_double_batch_joins_twice_on_one_path():
    b = B.double_batch()
    trace = {}
    fr, lms, out, masks = B.reference(b, traj=B.LONG_TRAJ, trace=trace, **B.LONG)
    _no_nan(fr, out)
    assert out["status"].tolist() == [COPIED] * 4 + [JOINED] + [MOVED] * 3 + [JOINED] + [MOVED] * 4 and not out["root"].any()
    g4, g8 = trace[4]["join"][1], trace[8]["join"][1]
    assert out["gain"][4] == g4 != 1 and out["gain"][8].tobytes() == F(g4 * g8).tobytes() and g8 != 1
    assert (out["gain"][5:8] == g4).all() and (out["gain"][9:] == out["gain"][8]).all() and fr["origin"][7] == 4 and out["anchor"][8] == 7
    spread = B.reference(b, traj=B.LONG_TRAJ, **B.LONG, scale_tolerance=1e-5)[2]  # both refused: the second roots behind the first gap
    assert spread["status"].tolist() == [COPIED] * 4 + [FIXED] + [COPIED] * 3 + [FIXED] + [COPIED] * 4
    assert spread["root"].tolist() == [0] * 5 + [4] * 4 + [8] * 4
    none = B.reference(b, traj=B.LONG_TRAJ, **B.LONG, max_reproj_px=1e-6)[2]
    assert none["status"].tolist() == [COPIED] * 4 + [UNFIXED] + [COPIED] * 3 + [UNFIXED] + [COPIED] * 4
    assert none["root"].tolist() == [0] * 4 + [4] * 4 + [8] * 5
    _no_nan(fr, spread)
    _no_nan(fr, none)


def test_edge_cases_imply_their_outcomes():
    b = B.edge_batch()
    state = B.join_state(b, B.EDGE_G, traj=B.EDGE_TRAJ, **B.EDGE)
    assert b["cap"] == 1100 and len(state["slots"]) == 439
    cases = B.edge_cases(b, state)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) and ["shared_%d" % m for m in (1, 2, 3, 255, 256, 257, 439)] == names[:7]
    for c in cases:
        trace = {}
        fr, lms, out, masks = B.reference(c["b"], traj=B.EDGE_TRAJ, trace=trace, **c["params"])
        _no_nan(fr, out)
        rec = out[B.EDGE_G]
        m, gam, consistent, verdict = trace[B.EDGE_G]["join"]
        print(c["name"], NAMES[int(rec["status"])], "shared", m, "gamma", hex(int(F(gam).view(U))), "consistent", consistent)
        assert fr["status"].tolist() == [ORIGIN, START, CHAINED, CHAINED, LOST, START] and rec["candidates"] == 493
        assert rec["status"] == (JOINED if verdict == tr.HOLDS else FIXED) and (rec["shared"], rec["consistent"]) == (m, consistent)
        B.check_expect(c, rec)
    # the select on values of its own: the lower median for m even, the tolerance's edge as binary32 computes it
    edge = B.tolerance_edge(1.0, 0.1)
    assert abs(edge - F(1.0)) <= F(0.1) * F(1.0) and not abs(np.nextafter(edge, F(2)) - F(1.0)) <= F(0.1) * F(1.0)
    kept = B.ratios_of(next(c for c in cases if c["name"] == "depths")["b"], state)
    assert len(kept) == 433 and 0 < kept.min() < 1e-36  # of the seven depths only 3e38 gives a ratio: tiny, finite and > 0
