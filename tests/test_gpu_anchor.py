"""The anchor stage on the GPU (orb_anchor_frames): every OrbAnchorPose, OrbAnchorSegment, OrbAnchorLink,
OrbAnchorRow and OrbLandmark byte against the CPU restatement (tests/anchor_ref.py) fed with what the device holds -- its counts,
orb_match_read, orb_trajectory_read, orb_landmarks_read, orb_keyframes_read, orb_match_keyframes_read and
orb_localize_keyframes_read output.  No tolerance anywhere but against the true cameras.

The programs are 64 x 48.  A batch (tests/anchor_cases.py, tests/keyframes_cases.py) is written over the stages' buffers with
descriptors; hand-built keyframes go in through orb_keyframes_load, hand-built rows, fixes and inlier bytes through
orb_debug_keyframe_buffers.

Shapes.  k_an_ratio strides 256 threads over the capacity and selects the median through 256-bin histograms: at capacity 300 under
raw counters of 311 an entry has 0, 1, 7, 8, 255, 256, 257 and 300 ratios; k_an_land takes 512 slots per workgroup: capacities 16,
128 and 300 are one partial workgroup per pair."""
import numpy as np
import pytest

import anchor_cases as A
import anchor_ref as ar
import keyframes_cases as KC
import join_cases as J
import landmark_cases as L
import loop_cases as K

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
V = A.V


def _two_batches(T, prog, seed, lost_pair=None):
    """out_and_back(seed) over the program, every frame inserted (slot = frame), then second_batch(seed) over the same program with
    its trajectory and landmarks, matched and localised against keyframes_cases.SECOND_PAIRS.  Returns (b1, b2, inputs)."""
    b1, b2 = K.out_and_back(seed), KC.second_batch(seed)
    if lost_pair is not None:
        b2["poses"]["status"][lost_pair] = T.ORB_POSE_LOW_PARALLAX
    d1, d2 = KC.plant_pair(b1, b2, 100 + seed)
    J.load(prog, b1, d1, traj=L.FULL_TRAJ)
    prog.keyframes_reserve(b1["n"])
    prog.keyframes_insert(A.entries(b1["n"]))
    i = J.load(prog, b2, d2, traj=L.FULL_TRAJ)
    inp = A.inputs(prog, b2["n"], b2["n"], b2["cap"])
    assert inp.frames.tobytes() == i.frames.tobytes()
    prog.match_keyframes(KC.SECOND_PAIRS)
    prog.localize_keyframes(len(KC.SECOND_PAIRS), **A.INTR)
    return b1, b2, inp


@pytest.mark.parametrize("valu", ["", "1"])
@pytest.mark.parametrize("seed", [0, 1])
def test_second_batch_in_the_stored_map(tinyorb, monkeypatch, seed, valu):
    """The real second batch against all eleven keyframes of the first, on both matcher forms: lists of 1, 5 and 10 entries; every
    entry HOLDS, segment 0 ANCHORED, gamma and the five anchored cameras within the CPU test's bounds of the truth."""
    T = tinyorb
    monkeypatch.setenv("TINYORB_MATCH_VALU", valu) if valu else monkeypatch.delenv("TINYORB_MATCH_VALU", raising=False)
    pairs = KC.SECOND_PAIRS
    with A.program(T, 128, 11) as prog:
        b1, b2, inp = _two_batches(T, prog, seed)
        assert (inp.frames["origin"] == 0).all()
        for n in (1, 5, len(pairs)):
            poses, segs, links, rows, land, _ = A.check(prog, inp, pairs, n=n)
            assert (links["verdict"] == V["HOLDS"]).all() and segs[0]["status"] == A.SEG_ANCHORED and (poses["status"] == A.ANCHORED).all()
        chosen = np.nonzero(links["chosen"])[0]
        assert len(chosen) == 1 and segs[0]["link"] == chosen[0] and links["consistent"][chosen[0]] == links["consistent"].max()
        slot = int(segs[0]["slot"])
        assert slot == pairs[chosen[0]][1] and (segs[0]["map_origin"], segs[0]["map_frame"], segs[0]["user"].tolist()) == (0, slot, [7 * slot + 1, 1000 + slot])
        assert (poses["slot"] == slot).all() and rows["slot"].tolist() == [slot] * 4 and rows["moved"][0] > 40 and not rows["dropped"].any()
        true = A.true_gamma(b1, b2)
        assert np.abs(links["gamma"].astype(np.float64) / true - 1).max() <= A.BOUNDS[0]
        for f in range(5):
            _, (Rt, tt) = KC.true_relative(b1, b2, f, 0, 0)
            assert K.rotation_error_deg(poses[f]["r"], Rt) <= A.BOUNDS[1] and np.linalg.norm(poses[f]["t"] - tt) <= A.BOUNDS[2], (f, poses[f])
        with pytest.raises(T.OrbError) as e:
            prog.anchor_frames(len(pairs) + 1)
        assert e.value.code == T.ORB_EINVAL


def test_two_segments_streams_and_a_call_without_holds(tinyorb):
    """Pair 2 of the second batch LOW_PARALLAX: both origins ANCHORED, each through an entry of its own; a second call on another
    stream; a call in which nothing holds is the trajectory and the landmark records byte for byte; an insert behind the localize
    call is ORB_ESTATE."""
    import torch
    T = tinyorb
    pairs = KC.SECOND_PAIRS
    with A.program(T, 128, 11) as prog:
        b1, b2, inp = _two_batches(T, prog, 0, lost_pair=2)
        assert inp.frames["origin"].tolist() == [0, 0, 0, 3, 3] and inp.lrows["origin"].tolist() == [0, 0, NONE, 3]
        poses, segs, links, rows, land, blob = A.check(prog, inp, pairs)
        assert (links["verdict"] == V["HOLDS"]).all() and segs["status"].tolist() == [A.SEG_ANCHORED, 0, 0, A.SEG_ANCHORED, 0]
        i0, i3 = int(segs[0]["link"]), int(segs[3]["link"])
        assert pairs[i0][0] < 3 <= pairs[i3][0] and links["chosen"].sum() == 2 and (poses["status"] == A.ANCHORED).all()
        true0 = A.true_gamma(b1, b2)
        g0, g3 = float(segs[0]["gamma"]) / true0, float(segs[3]["gamma"]) / true0
        assert abs(g0 - 1.0) <= A.BOUNDS[0] and abs(g3 / (0.25 / 0.35) - 1.0) <= A.BOUNDS[0], (g0, g3)
        assert rows["slot"].tolist() == [segs[0]["slot"]] * 2 + [NONE, segs[3]["slot"]] and rows["moved"][3] > 0 and rows["moved"][2] == 0
        # a second call on another stream, the first stream again, other parameters in between
        s = torch.cuda.Stream(device=0)
        prog.anchor_frames(len(pairs), stream=s.cuda_stream)
        assert A.check(prog, inp, pairs, call=False)[5] == blob
        A.check(prog, inp, pairs, n=3, min_shared=30, scale_tolerance=0.01, consistent_permille=100, min_inliers=20)
        assert A.check(prog, inp, pairs, stream=s.cuda_stream)[5] == blob
        assert A.check(prog, inp, pairs)[5] == blob
        # nothing holds: the trajectory and the landmark records
        poses, segs, links, rows, land, _ = A.check(prog, inp, pairs, min_inliers=100000)
        assert (links["verdict"] == V["FEW"]).all() and not links["chosen"].any() and segs["status"].tolist() == [A.SEG_FREE, 0, 0, A.SEG_FREE, 0]
        for f in range(5):
            assert poses[f].tobytes()[:52] == prog.trajectory_read(f, 0)[0].tobytes()[:52] and poses[f]["gain"] == 1 and poses[f]["slot"] == NONE
        for p in range(4):
            lrow, lm = prog.landmarks_read(p, inp.cap)
            assert land[p].tobytes() == lm.tobytes() and (rows[p]["good"], rows[p]["origin"]) == (lrow["good"], lrow["origin"])
        assert not rows["moved"].any() and (rows["slot"] == NONE).all()
        # the store changes behind the localize call: the rows and fixes are of another store
        prog.keyframes_insert([(0, 10)])
        with pytest.raises(T.OrbError) as e:
            prog.anchor_frames(len(pairs))
        assert e.value.code == T.ORB_ESTATE
        prog.match_keyframes(pairs)
        with pytest.raises(T.OrbError) as e:
            prog.anchor_frames(len(pairs))  # the fixes are of the rows before
        assert e.value.code == T.ORB_ESTATE
        prog.localize_keyframes(len(pairs), **A.INTR)
        A.check(prog, inp, pairs)


def _rail_program(T, case, counts=None):
    """The rail batch over a fresh program's buffers, its CPU-built keyframes through orb_keyframes_load (slot = frame)."""
    b, lms, lrows, desc, store = case
    if counts is not None:
        b["counts"][:] = counts
    prog = A.program(T, b["cap"], b["n"])
    J.load_rail(prog, b, desc)
    inp = A.inputs(prog, b["n"], b["n"], b["cap"])
    assert inp.frames.tobytes() == np.ascontiguousarray(b["frames"]).tobytes() and all(inp.lms[p].tobytes() == lms[p].tobytes() for p in range(b["n"] - 1))
    prog.keyframes_reserve(b["n"])
    return prog, inp


def _load_store(prog, store):
    for s, kf in store.items():
        A.load_kf(prog, s, kf)


def test_rail_verdicts_tie_and_nan(tinyorb):
    """The rail camera, hand-built keyframes, fixes and inlier bytes: every verdict in one list, MINIMAL with and without the flag,
    the tie and the duplicate, the landmarks in the map's frame; then RANGE through frame records without an origin."""
    T = tinyorb
    case = A.rail(scales={3: 2})
    b, lms, lrows, desc, store = case
    bare = dict(store[1], points=store[1]["points"].copy(), head=store[1]["head"].copy())  # slot 1: every key NONE
    bare["points"]["key"], bare["head"]["points"] = NONE, 0
    pairs = [(5, 0), (4, 2), (5, 0), (3, 2), (5, 0), (4, 2), (5, 0), (5, 2), (4, 0), (5, 1), (1, 2)]
    fx = A.fixes(b, pairs)
    fx["status"][4] = A.FEW_FIX                 # STATUS
    fx["status"][5] = A.MINIMAL                 # STATUS, HOLDS under the flag
    fx["inliers"][6] = 11                       # FEW
    fx["pose_t"][7][2] = np.nan                 # NONFINITE
    fx["r"][8][6] = np.inf                      # NONFINITE
    fx["status"][9], fx["inliers"][9] = A.NOMAP_FIX, 0  # STATUS before FEW
    masks = np.array([A.mask(b, q) for q, s in pairs])
    masks[9] = 1
    rows = np.array([A.row(b, q, s) for q, s in pairs])
    prog, inp = _rail_program(T, case)
    with prog:
        _load_store(prog, {**store, 1: bare})
        prog.match_keyframes(pairs)
        prog.localize_keyframes(len(pairs), **L.RAIL)
        for i, (q, s) in enumerate(pairs):
            assert prog.match_keyframes_read(i, 12)["index"].tolist() == A.row(b, q, s)["index"][:12].tolist()
        A.inject(prog, rows, fx, masks)
        poses, segs, links, arows, land, blob = A.check(prog, inp, pairs)
        want = A.run(case, pairs, fx=fx, masks=list(masks), store={**store, 1: bare})  # the CPU's own batch, landmarks and rows: the same bytes
        assert poses.tobytes() == want[0].tobytes() and segs.tobytes() == want[1].tobytes() and links.tobytes() == want[2].tobytes()
        assert links["verdict"].tolist() == [V[k] for k in ("HOLDS", "HOLDS", "HOLDS", "HOLDS", "STATUS", "STATUS", "FEW", "NONFINITE", "NONFINITE", "STATUS", "HOLDS")]
        assert links["chosen"].tolist() == [1] + [0] * 9 + [1] and links["consistent"][:4].tolist() == [12] * 4  # the tie and the duplicate: the lowest index
        assert segs["status"].tolist() == [A.SEG_ANCHORED, 0, 0, A.SEG_ANCHORED, 0, 0] and segs["link"][[0, 3]].tolist() == [10, 0]
        assert abs(float(segs[3]["gamma"]) - 0.5) < 1e-4 and segs[0]["gamma"] == 1 and np.allclose(poses["t"][:, 0], [-0.5 * f for f in range(6)], atol=1e-4)
        assert arows["moved"].tolist() == [12, 0, 0, 12, 0] and arows["slot"].tolist() == [2, 2, NONE, 0, 0]
        s = b["slots"]
        for k in "xyz":
            assert np.allclose(land[3][k][s[3]], inp.lms[0][k][s[0]], atol=2e-3)
        # MINIMAL under the flag; fewer inliers asked for
        _, _, links2, _, _, _ = A.check(prog, inp, pairs, flags=T.ORB_ANCHOR_USE_MINIMAL, min_inliers=11)
        assert links2["verdict"][[4, 5, 6, 9]].tolist() == [V["STATUS"], V["HOLDS"], V["HOLDS"], V["STATUS"]]
        # a later entry with more consistent ratios wins
        m2 = masks.copy()
        m2[0], m2[2] = A.mask(b, 5, range(10)), A.mask(b, 5, range(11))
        A.inject(prog, masks=m2)
        _, segs2, links2, _, _, _ = A.check(prog, inp, pairs)
        assert links2["consistent"][:4].tolist() == [10, 12, 11, 12] and segs2[3]["link"] == 1 and segs2[3]["slot"] == 2
        A.inject(prog, masks=masks)
        # frame records: frame 5 without an origin (RANGE), a NaN in frame 4's (NONFINITE there and only there)
        fr = b["frames"].copy()
        fr["origin"][5], fr["r"][4][4] = NONE, np.nan
        L.inject_frames(prog, fr)
        inp2 = A.inputs(prog, b["n"], b["n"], b["cap"])
        assert inp2.frames["origin"][5] == NONE and np.isnan(inp2.frames["r"][4][4])
        poses, segs, links, arows, land, _ = A.check(prog, inp2, pairs)
        assert links["verdict"][:4].tolist() == [V["RANGE"], V["NONFINITE"], V["RANGE"], V["HOLDS"]] and segs[3]["link"] == 3
        assert poses["status"].tolist() == [A.ANCHORED] * 3 + [A.ANCHORED, A.ANCHORED, A.FREE] and np.isnan(poses[4]["r"]).any()
        L.inject_frames(prog, b["frames"])
        assert A.check(prog, inp, pairs)[5] == blob  # nothing of the calls between is left


def test_ratio_counts(tinyorb):
    """Capacity 300, raw counters 311: the inlier bytes of one entry rewritten so that it has exactly m ratios, the ratios all
    different by multiples of 1/64."""
    T = tinyorb
    cap = 300
    case = A.rail(K_=cap, cap=cap)
    b, lms, lrows, desc, store = case
    factor = 1.0 + (np.arange(cap) % 7) / 64.0
    store = {s: dict(kf, points=kf["points"].copy()) for s, kf in store.items()}
    store[2]["points"]["z"][b["slots"][2]] *= factor.astype(np.float32)
    pairs = [(4, 2), (5, 0), (4, 2)]
    prog, inp = _rail_program(T, case, counts=cap + 11)
    with prog:
        assert (prog.batch_counts(b["n"]) == cap + 11).all() and (inp.nq == cap).all()
        _load_store(prog, store)
        prog.match_keyframes(pairs)
        prog.localize_keyframes(len(pairs), **L.RAIL)
        fx = A.fixes(b, pairs)
        rows = np.array([A.row(b, q, s) for q, s in pairs])
        for m in (0, 1, 7, 8, 255, 256, 257, 300):
            masks = np.array([A.mask(b, 4, range(m)), A.mask(b, 5), A.mask(b, 4)])
            A.inject(prog, rows, fx, masks)
            t = {}
            held = A.hold(prog, inp, pairs, len(pairs))
            assert held[2].tobytes() == masks.tobytes() and held[1].tobytes() == fx.tobytes()
            ar.anchor_frames(inp.nq, inp.matches, held[0], pairs, inp.frames, inp.lrows, inp.lms, fx, masks, A.device_store(prog, [0, 2]), cap, L=inp.L, trace=t)
            assert len(t[0]) == m and len(t[2]) == cap  # the m this builder produced, on the CPU
            poses, segs, links, arows, land, _ = A.check(prog, inp, pairs, held=held)
            assert links["shared"].tolist() == [m, cap, cap] and (links["verdict"][0] == V["RATIO_FEW"]) == (m < 8)
            if m:
                assert links["gamma"][0] == np.sort(t[0])[(m - 1) // 2]
            assert segs[3]["link"] == (0 if m == cap else 1) and arows["moved"].tolist() == [0, 0, 0, cap, 0]


def test_state_arguments_and_a_batch_that_replaces_the_first(tinyorb):
    T = tinyorb
    b = K.out_and_back(2, nf=2, n_land=150)
    n, cap = b["n"], b["cap"]
    desc = K.plant(b, np.random.default_rng(31))
    pairs = [(4, 0), (3, 1), (0, 2), (4, 0)]
    np_ = len(pairs)

    def code(fn, *a, **kw):
        with pytest.raises(T.OrbError) as e:
            fn(*a, **kw)
        return e.value.code

    with A.program(T, cap, n, T.ORB_FLAG_DOUBLE_OUTPUT) as prog:
        lib, h = T.load_library(), prog._handle()
        for fn, a in ((prog.anchor_read, (0,)), (prog.anchor_segments, (1,)), (prog.anchor_links, (1,)), (prog.anchor_landmarks, (0,)), (prog.debug_keyframe_buffers, ())):
            assert code(fn, *a) == T.ORB_ESTATE
        prog.extract_batch_host(np.zeros((n, A.H0, A.W0, 4), np.uint8))
        assert code(prog.anchor_frames, 1) == T.ORB_ESTATE  # nothing has run
        J.load(prog, b, desc, traj=L.FULL_TRAJ)
        prog.keyframes_reserve(3)
        prog.keyframes_insert([(0, 0), (1, 1), (2, 2)])
        prog.match_keyframes(pairs)
        assert code(prog.anchor_frames, 1) == T.ORB_ESTATE and code(prog.debug_keyframe_buffers) == T.ORB_ESTATE  # before localize_keyframes
        prog.localize_keyframes(np_, hypotheses=64, **A.INTR)
        assert all(prog.debug_keyframe_buffers())
        inf, nan = float("inf"), float("nan")
        for kw in (dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 7)), dict(consistent_permille=1001), dict(flags=2), dict(flags=3),
                   dict(scale_tolerance=-1.0), dict(scale_tolerance=nan), dict(scale_tolerance=inf)):
            assert code(prog.anchor_frames, np_, **kw) == T.ORB_EINVAL, kw
        assert code(prog.anchor_frames, 0) == T.ORB_EINVAL and code(prog.anchor_frames, np_ + 1) == T.ORB_EINVAL
        assert code(prog.anchor_read, 0) == T.ORB_ESTATE  # none of them counts as a call
        inp = A.inputs(prog, n, n, cap)
        held = A.hold(prog, inp, pairs, np_)
        assert lib.orb_anchor_frames(h, np_, None, None) == T.ORB_OK  # NULL params: the defaults
        poses, segs, links, rows, land, blob = A.check(prog, inp, pairs, call=False, held=held)
        assert links["verdict"][0] == V["HOLDS"] and segs[0]["status"] == A.SEG_ANCHORED  # a self-anchor: the map is the batch's own frame
        assert abs(float(segs[0]["gamma"]) - 1) <= A.BOUNDS[0]
        # read errors
        assert code(prog.anchor_read, n) == T.ORB_EINVAL and code(prog.anchor_segments, n + 1) == T.ORB_EINVAL and code(prog.anchor_links, np_ + 1) == T.ORB_EINVAL
        assert code(prog.anchor_landmarks, n - 1) == T.ORB_EINVAL
        assert lib.orb_anchor_read(h, 0, None) == T.ORB_EINVAL and lib.orb_anchor_segments(h, None, 1) == T.ORB_EINVAL and lib.orb_anchor_links(h, None, 1) == T.ORB_EINVAL
        assert lib.orb_anchor_landmarks(h, 0, None, None, 1) == T.ORB_EINVAL and lib.orb_anchor_landmarks(h, 0, None, None, 0) == T.ORB_OK
        assert lib.orb_anchor_segments(h, None, 0) == T.ORB_OK and lib.orb_anchor_links(h, None, 0) == T.ORB_OK
        # isolation: the stages it reads and the store, before and after
        def others():
            out = [prog.match_read(f, cap).tobytes() + prog.landmarks_read(f, cap)[0].tobytes() + prog.landmarks_read(f, cap)[1].tobytes() for f in range(n - 1)]
            out += [prog.trajectory_read(f, cap)[0].tobytes() for f in range(n)]
            out += [prog.match_keyframes_read(i, cap).tobytes() + prog.localize_keyframes_read(i, cap)[0].tobytes() + prog.localize_keyframes_read(i, cap)[1].tobytes()
                    for i in range(np_)]
            return out + [b"".join(np.ascontiguousarray(a).tobytes() for a in prog.keyframes_read(s, cap)) for s in range(3)]

        before = others()
        assert A.check(prog, inp, pairs)[5] == blob and others() == before
        # an insert, a load or a remove between the localize call and the anchor call: ORB_ESTATE, and a parameter error comes first
        prog.keyframes_insert([(3, 2)])
        assert code(prog.anchor_frames, np_) == T.ORB_ESTATE and code(prog.anchor_frames, np_, flags=2) == T.ORB_EINVAL and code(prog.anchor_frames, 0) == T.ORB_ESTATE
        prog.keyframes_insert([(2, 2)])
        prog.match_keyframes(pairs)
        assert code(prog.anchor_frames, np_) == T.ORB_ESTATE  # the fixes are of the rows before: localize_keyframes is behind match_keyframes
        prog.localize_keyframes(np_, hypotheses=64, **A.INTR)
        assert A.check(prog, inp, pairs)[5] == blob
        prog.keyframes_remove(1)
        assert code(prog.anchor_frames, np_) == T.ORB_ESTATE
        # a second batch replaces the first in the same program: the stages before are stale, the store stays
        b2 = K.out_and_back(3, nf=2, n_land=150)
        d2 = K.plant(b2, np.random.default_rng(31))
        prog.extract_batch_host(np.zeros((n, A.H0, A.W0, 4), np.uint8))
        assert code(prog.anchor_frames, np_) == T.ORB_ESTATE
        J.load(prog, b2, d2, traj=L.FULL_TRAJ)
        inp2 = A.inputs(prog, n, n, cap)
        other = [(4, 0), (1, 2), (2, 0)]
        assert code(prog.anchor_frames, 1) == T.ORB_ESTATE  # no keyframe call of this batch yet
        prog.match_keyframes(other)
        prog.localize_keyframes(len(other), **A.INTR)
        poses, segs, links, rows, land, blob2 = A.check(prog, inp2, other)
        assert blob2 != blob and (links["slot"] == [0, 2, 0]).all()
        prog.batch_select_output(1)
        assert code(prog.anchor_frames, 1) == T.ORB_ESTATE
        prog.batch_select_output(0)
        assert A.check(prog, inp2, other)[5] == blob2
