"""CPU checks of the constructed records (tests/constructed.py): for every builder at small sizes, the outcome the construction
implies equals the restatements' -- oracle/orb_numpy.match, tests/verify_ref.verify_pair, tests/guided_ref.guided_pair and
tests/track_ref.track -- so the fixtures of tests/test_gpu_constructed.py are right before any GPU runs them."""
import numpy as np
import pytest

import constructed as C
import guided_ref as gr
import track_ref as tr
import verify_ref as vr
from oracle import orb_numpy
from tinyslam_amd.orb import ORB_MATCH_NONE as NONE, ORB_TRACK_GUIDED, ORB_TRACK_MATCHED, ORB_TRACK_VERIFIED

W = H = 256


def _numpy_match(qd, td):
    idx, dist, second = orb_numpy.match(qd, td)
    out = np.zeros(len(idx), C.match_ref(qd[:0], td[:0]).dtype)
    out["index"], out["distance"], out["second"] = idx, dist, second
    return out


def _agree(got, exp, second_known=True):
    """got: the restatement's records of the planted queries; exp: the construction's.  Where the construction leaves second open
    (0xFFFF with a unique best), it only bounds it: second > distance + 40."""
    assert np.array_equal(got["index"], exp["index"]) and np.array_equal(got["distance"], exp["distance"])
    known = exp["second"] != 0xFFFF
    assert np.array_equal(got["second"][known], exp["second"][known])
    assert np.all(got["second"][~known].astype(int) > got["distance"][~known].astype(int) + 40)


def test_match_ref_equals_orb_numpy():
    rng = np.random.default_rng(1)
    for na, nb in ((0, 5), (5, 0), (1, 1), (70, 300), (300, 17)):
        qd, td = C.random_desc(rng, na), C.random_desc(rng, nb)
        assert C.match_ref(qd, td).tobytes() == _numpy_match(qd, td).tobytes()


def test_matcher_constructions():
    rng = np.random.default_rng(2)
    groups = [[15, 16], [63, 64], [255, 256], [31, 32, 47], [127, 128], [0, 599], [511, 512], [79, 80, 96, 257], [300]]
    qd, td, exp = C.planted_ties(rng, 300, 600, groups)
    got = C.match_ref(qd, td)
    assert got.tobytes() == _numpy_match(qd, td).tobytes()
    _agree(got[:len(groups)], exp)
    for nb in (1, 15, 17, 63, 65, 129, 207):
        qd, td, exp = C.last_is_best(rng, 70, nb)
        got = _numpy_match(qd, td)
        assert np.all(got["index"] == nb - 1) and np.array_equal(got["distance"], exp["distance"])
        assert nb == 1 or np.all(got["second"].astype(int) > got["distance"].astype(int) + 40)
        if nb == 1:
            assert np.all(got["second"] == 0xFFFF)
    qd, td, exp = C.extremes(rng, 40)
    got = _numpy_match(qd, td)
    _agree(got[:3], exp)
    assert C.hamming(qd[3], td[9]) == 256 and got["distance"][3] < 256
    for nb in (1, 5):
        qd, td, exp = C.all_at_256(3, nb)
        assert _numpy_match(qd, td).tobytes() == exp.tobytes()
    qd, td, exp = C.last_of_huge(rng, 64, 1000)
    assert _numpy_match(qd, td).tobytes() == exp.tobytes()


def _links_matched(d, counts):
    return [tr.pair_links(ORB_TRACK_MATCHED, C.match_ref(d[f][:counts[f]], d[f + 1][:counts[f + 1]]), counts[f], counts[f + 1])
            for f in range(len(counts) - 1)]


def _track_equals_construction(ch, cap, **kw):
    counts = [int(c) for c in ch["counts"]]
    links = _links_matched(ch["desc"], counts)
    t, fr = tr.track(counts, cap, links, **kw)
    for f in range(len(counts)):
        assert t[f][:counts[f]].tobytes() == ch["tracks"][f].tobytes(), f
    return t, fr, links


def test_chain_constructions():
    rng = np.random.default_rng(3)
    for F in (2, 3, 9, 17):
        ch = C.chains(rng, np.eye(F, 20, dtype=bool) | (np.arange(F)[:, None] == 0), W, H)
        counts = [int(c) for c in ch["counts"]]
        t, fr, links = _track_equals_construction(ch, 24)
        # the other sources give the same links: VERIFIED (identity inliers) and GUIDED (identity, radius 4)
        for f in range(F - 1):
            m = C.match_ref(ch["desc"][f], ch["desc"][f + 1])
            rec, mask = vr.verify_pair(ch["corners"][f], ch["corners"][f + 1], m, W, H, f)
            jv, _ = tr.pair_links(ORB_TRACK_VERIFIED, m, counts[f], counts[f + 1], inlier=mask)
            g = gr.guided_pair(ch["corners"][f], ch["desc"][f], ch["corners"][f + 1], ch["desc"][f + 1], gr.IDENTITY, 4.0)
            jg, _ = tr.pair_links(ORB_TRACK_GUIDED, g, counts[f], counts[f + 1])
            assert np.array_equal(jv, links[f][0]) and np.array_equal(jg, links[f][0]), f
    # whole-batch chains: heads (0, the composed permutation), tails F - 1, only frame 0 a keyframe
    F = 33
    ch = C.chains(rng, np.arange(F)[:, None] == np.zeros((1, 16)), W, H)
    t, fr, _ = _track_equals_construction(ch, 16)
    for f in range(F):
        assert np.all(t[f]["head_frame"][ch["perm"][f]] == 0) and np.array_equal(t[f]["head_index"][ch["perm"][f]], ch["perm"][0])
        assert np.all(t[f]["tail_frame"][:16] == F - 1)
    key, ref, shared = C.steady_keyframes(F, 16, 16)
    assert list(fr["keyframe"]) == list(key) == [1] + [0] * (F - 1)
    assert np.array_equal(fr["ref_keyframe"], ref) and np.array_equal(fr["shared"], shared) and np.all(shared == 16)
    for g in (5, 7):
        _, fr = tr.track(ch["counts"], 16, _links_matched(ch["desc"], [16] * F), max_gap=g)
        key, ref, shared = C.steady_keyframes(F, 16, 16, max_gap=g)
        assert np.array_equal(fr["keyframe"], key) and np.array_equal(fr["ref_keyframe"], ref) and np.array_equal(fr["shared"], shared)


def test_exact_lengths():
    rng = np.random.default_rng(4)
    F = 40
    lengths = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 39]
    starts, spans = C.exact_lengths(F, lengths, 4)
    ch = C.chains(rng, starts, W, H)
    t, _, _ = _track_equals_construction(ch, 20)
    for s, a, L in spans:
        r = ch["perm"][a + L, s]
        assert t[a + L]["head_frame"][r] == a and t[a]["tail_frame"][ch["perm"][a, s]] == a + L


@pytest.mark.parametrize("G", [4, 62, 63, 64, 65])
def test_steady_loss_keyframes(G):
    rng = np.random.default_rng(5)
    F, n = 140, 160
    ch = C.chains(rng, C.steady_loss(F, n), 64, 64)
    counts = [n] * F
    links = _links_matched(ch["desc"], counts)
    p = C.permille_for_gap(n, G)
    cases = [dict(keep_permille=p), dict(keep_permille=p, min_gap=G + 3), dict(keep_permille=1, min_shared=n - G + 1),
             dict(keep_permille=1, max_gap=G)]
    for kw in cases:
        _, fr = tr.track(counts, n, links, **kw)
        key, ref, shared = C.steady_keyframes(F, n, n - 1, **kw)
        assert np.array_equal(fr["keyframe"], key) and np.array_equal(fr["ref_keyframe"], ref), kw
        assert np.array_equal(fr["shared"], shared), kw
    if G == 63:
        assert list(np.nonzero(key)[0]) == [0, 63, 126]


def test_contention():
    rng = np.random.default_rng(6)
    nq = nt = 300
    groups = [(nt - 1, [(3, 5), (40, 5), (250, 5)]), (nt - 2, [(7, 9), (120, 7), (nq - 1, 3)]), (nt - 3, [(8, 4), (9, 4)]),
              (0, [(10, 0), (11, 1)])]
    qd, td, win, planted = C.contention(rng, nq, nt, groups)
    links = _links_matched([qd, td], [nq, nt])
    assert sorted(np.nonzero(links[0][0] >= 0)[0]) == sorted(planted)
    t, fr = tr.track([nq, nt], nq, links)
    for j, i in win.items():
        assert t[1]["prev"][j] == i and t[0]["next"][i] == j
    assert fr["links_out"][0] == len(groups)


def test_verification_constructions():
    rng = np.random.default_rng(7)
    for M in (3, 4, 5):
        c, d, _ = C.correspondences(rng, M, 0, W, H)
        rec, mask = vr.verify_pair(c[0], c[1], C.match_ref(d[0], d[1]), W, H, 0)
        assert int(rec["status"]) == (vr.VERIFY_FEW if M == 3 else vr.VERIFY_OK) and rec["candidates"] == M
        assert mask.sum() == (0 if M == 3 else M)
    c, d = C.collinear(rng, 40, W, H)
    rec, mask = vr.verify_pair(c[0], c[1], C.match_ref(d[0], d[1]), W, H, 0)
    assert int(rec["status"]) == vr.VERIFY_DEGENERATE and not mask.any() and rec["candidates"] == 40
    for M in (255, 257):
        c, d, inl = C.correspondences(rng, M, int(0.3 * M), W, H)
        for hyps in (1, 512):
            rec, mask = vr.verify_pair(c[0], c[1], C.match_ref(d[0], d[1]), W, H, 0, hypotheses=hyps)
            if hyps == 512:
                assert int(rec["status"]) == vr.VERIFY_OK and rec["inliers"] >= M and np.all(mask[inl] == 1)
    c, d = C.two_motions(rng, 50, W, H)
    rec, mask = vr.verify_pair(c[0], c[1], C.match_ref(d[0], d[1]), W, H, 0)
    assert int(rec["status"]) == vr.VERIFY_OK and rec["inliers"] == 50 and mask.sum() == 50 and (mask[:50].all() or mask[50:].all())
    c, d = C.jittered(np.random.default_rng(C.MINIMAL_SEED), 40, W, H)
    rec, _ = vr.verify_pair(c[0], c[1], C.match_ref(d[0], d[1]), W, H, 0, **C.MINIMAL_PARAMS)
    assert int(rec["status"]) == vr.VERIFY_MINIMAL


def _guided(qc, qd, tc, td, r, **kw):
    return gr.guided_pair(qc, qd, tc, td, gr.IDENTITY, r, **kw)


def test_guided_constructions():
    rng = np.random.default_rng(8)
    for octave, r in ((0, 3.0), (0, 1.0), (1, 2.5)):
        qc, qd, tc, td, cases = C.window_edges(rng, r, octave)
        below = float(np.nextafter(np.float32(r), np.float32(0)))
        on, off = _guided(qc, qd, tc, td, r), _guided(qc, qd, tc, td, below)
        for q, e, c in cases:
            assert (on["index"][q], on["distance"][q], on["second"][q]) == (e, 1, 10), (octave, r, q)
            assert (off["index"][q], off["distance"][q], off["second"][q]) == (c, 10, 0xFFFF), (octave, r, q)
    qc, qd, tc, td, exp = C.cell_ties(rng)
    assert _guided(qc, qd, tc, td, 16.0).tobytes() == exp.tobytes()
    qc, qd, tc, td = C.dense_cell(rng, 96, 96, 100)
    for nt in (len(tc), 64, 70):  # the whole frame and two capacity cuts
        g = _guided(qc, qd, tc[:nt], td[:nt], 16.0)
        assert np.array_equal(g["index"], np.arange(64)) and np.all(g["distance"] == 3)
    # the identity with a radius over the frame is the matcher (GM-6) on constructed frames too
    assert _guided(qc, qd, tc, td, 1e6).tobytes() == C.match_ref(qd, td).tobytes()
    assert np.all(gr.guided_pair(qc, qd, tc, td, np.array([1, 0, 5000, 0, 1, 0, 0, 0, 1], np.float32), 16.0)["index"] == NONE)
