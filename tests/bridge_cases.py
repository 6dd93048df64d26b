"""Hand-built inputs of the bridge stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_bridge_consecutive reads the raw counters, the stored records, the matcher's records, the pairs' points,
the frame records of the trajectory stage and the landmark records.  `gapped` builds a localize_cases.views batch -- 64 x 48
frames, one cloud along one path -- in which some steps are a pure rotation or a pause: such a pair's pose record is set to a
status that is not OK and its points lose their flags, as the pose stage leaves a pair without parallax, and its matches are
kept, because the matcher still pairs the keypoints.  That is what differs from localize_cases.join's unrelated runs, whose
bridging matches are all wrong.  `reference` runs the trajectory, landmark and bridge restatements on a batch; `trim` leaves a
gap end an exact number of candidates.  `long_batch`, `hop_batch` and `double_batch` are laid out for k_br_chain's chunks of 64
frames, for BR-1's hop limit and for two joins on one path; `join_state`, `set_shared` and `set_ratios` decide BR-5's ratios of one
gap end to the bit.
"""
import numpy as np

import bridge_ref as br
import landmark_ref as lmr
import localize_cases as lc
import trajectory_cases as tc
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
U = np.uint32
NONE = orb.ORB_MATCH_NONE
GOOD = orb.ORB_POINT_GOOD
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = tc.CHAINED, tc.START, tc.FEW, tc.SPREAD, tc.LOST, tc.ORIGIN
COPIED, MOVED, FIXED, JOINED, UNFIXED = (orb.ORB_BRIDGE_COPIED, orb.ORB_BRIDGE_MOVED, orb.ORB_BRIDGE_FIXED, orb.ORB_BRIDGE_JOINED,
                                         orb.ORB_BRIDGE_UNFIXED)
L_OK, L_NOMAP, L_FEW, L_DEGENERATE, L_MINIMAL = (orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_NOMAP, orb.ORB_LOCALIZE_FEW,
                                                 orb.ORB_LOCALIZE_DEGENERATE, orb.ORB_LOCALIZE_MINIMAL)
ROTATION, PAUSE = "rotation", "pause"


def small_steps(n, gaps=None):
    """n camera steps that keep a cloud inside a 64 x 48 frame (a third of a degree of yaw, sideways and slightly forward, lengths
    that change by up to 2); step k of `gaps` {k: ROTATION | PAUSE} is a pure rotation of 1.5 degrees or no motion at all."""
    lengths = [0.12, 0.2, 0.1, 0.16, 0.08, 0.14, 0.12, 0.18, 0.1, 0.16, 0.12, 0.15, 0.09]
    steps = []
    for k in range(n):
        kind = (gaps or {}).get(k)
        if kind == ROTATION:
            steps.append((tr.rot("y", 1.5) @ tr.rot("x", -0.4), np.zeros(3)))
        elif kind == PAUSE:
            steps.append((np.eye(3), np.zeros(3)))
        else:
            l = lengths[k % len(lengths)]
            steps.append((tr.rot("y", 0.35) @ tr.rot("x", 0.15), np.array([-l, 0.1 * l, 0.3 * l])))
    return steps


def lose(b, pairs):
    """The pose records of `pairs` set to statuses that are not OK (arbitrary bits elsewhere) and their points' flags cleared; the
    matches stay."""
    rng = np.random.default_rng(len(pairs))
    for c, k in enumerate(pairs):
        q = rng.integers(0, 1 << 32, 16, dtype=U).view(orb.POSE_DTYPE)
        q["status"] = tc.NOT_OK[(c + 2) % 4]
        b["poses"][k] = q[0]
        b["points"][k] = np.zeros(b["cap"], orb.POINT_DTYPE)
    return b


def gapped(rng, n_frames, n_land, cap, gaps, **kw):
    """localize_cases.views along small_steps with the pairs of `gaps` lost."""
    with np.errstate(all="ignore"):  # a step without translation has no unit baseline: its pose and points are replaced below
        b = lc.views(rng, n_frames, n_land, cap, steps=small_steps(n_frames - 1, gaps), **kw)
    b["gaps"] = dict(gaps)
    return lose(b, sorted(gaps))


def inputs(b, n=None):
    n = b["n"] if n is None else n
    nq = lc.stored(b)
    return nq[:n], [c[:nq[f]] for f, c in enumerate(b["corners"][:n])], [b["matches"][f][:nq[f]] for f in range(n - 1)], list(b["points"][:n - 1])


def maps(b, n_frames=None, traj=None, lm=None):
    """The frame records and landmark records of a batch by the trajectory and landmark restatements."""
    n = b["n"] if n_frames is None else n_frames
    intr = lc.intrinsics(b["W"], b["H"], b["focal"])
    fr = tc.reference(b, n, **(traj or {}))[0]
    nq, corners, matches, points = inputs(b, n)
    lms = lmr.landmarks(nq, corners, matches, points, fr, b["cap"], n_frames=n, **{**intr, **(lm or {})})[0]
    return fr, lms


def run(b, fr, lms, n_frames=None, trace=None, **params):
    """bridge_ref.bridge on a batch's arrays under the frame records `fr` and landmark records `lms`."""
    n = b["n"] if n_frames is None else n_frames
    nq, corners, matches, points = inputs(b, n)
    return br.bridge(nq, corners, matches, points, fr[:n], lms, b["cap"], n_frames=n, trace=trace,
                     **{**lc.intrinsics(b["W"], b["H"], b["focal"]), **params})


def reference(b, n_frames=None, traj=None, lm=None, trace=None, **params):
    """A batch through the three restatements.  Returns (frame records, landmark records, OrbBridgePose records, inlier bytes)."""
    fr, lms = maps(b, n_frames, traj, lm)
    return (fr, lms) + tuple(run(b, fr, lms, n_frames, trace=trace, **params))


def trim(b, g, M, traj=None, lm=None, **params):
    """Leaves gap end g exactly M candidates: the first-hop matches of the tails behind the others become ORB_MATCH_NONE.  Fails
    when it has fewer, or when landmarks that share a tail make M unreachable."""
    trace = {}
    fr, lms, out, _ = reference(b, traj=traj, lm=lm, trace=trace, **params)
    T = int(out[g]["anchor"])
    src = trace[g]["src"]
    assert len(src) >= M, (len(src), M)
    for q, i in src[M:]:
        b["matches"]["index"][T, int(lms[q][i]["tail_index"])] = NONE
    trace = {}
    reference(b, traj=traj, lm=lm, trace=trace, **params)
    assert trace[g]["total"] == M, (trace[g]["total"], M)
    return b


def true_step(b, T, g):
    """(R, t) with X_g = R X_T + t in metres, from the batch's steps."""
    R, t = np.eye(3), np.zeros(3)
    for k in range(T, g):
        Rk, tk = b["steps"][k]
        R, t = Rk @ R, Rk @ t + tk
    return R, t


def angle_deg(Ra, Rb):
    c = (np.trace(np.asarray(Ra, np.float64).reshape(3, 3) @ np.asarray(Rb, np.float64).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ---- the GPU tests' batches (64 x 48 frames) ---------------------------------------------------------------------------------
MAIN_GAPS = {0: PAUSE, 3: ROTATION, 6: PAUSE, 7: ROTATION}


def main_batch(cap):
    """Twelve frames.  A nine-view path: pair 0 lost (frame 1 LOST behind ORIGIN: NOMAP), a one-frame gap (frame 4, a rotation), a
    two-frame gap (frames 7 and 8, a pause and a rotation); then the first frame of a plane's three views, LOST behind unrelated
    matches (all wrong) and the third LOST frame of its run; the plane's last pair lost, so the last frame is a gap end whose
    candidates are coplanar."""
    rng = np.random.default_rng(2031)
    a = gapped(rng, 9, 420, cap, MAIN_GAPS, wrong=0.08, far=0.04, lost=0.04, bad_points=0.04, noise=0.002)
    p = gapped(rng, 3, 220, cap, {1: ROTATION}, shape="plane")
    b = lc.join([a, p], bridge=True)
    b["steps"] = a["steps"]
    return b


def empty_batch(cap):
    """Seven frames of one path; frame 4 is a gap end and stores nothing, so no hop reaches it (FEW); frame 5 starts again."""
    rng = np.random.default_rng(5)
    b = gapped(rng, 7, 200, cap, {3: PAUSE}, noise=0.001)
    b["counts"][4] = 0
    return b


def repeated_batch(cap):
    """Five frames of a cloud of two points, each repeated twenty times; frame 3 is a gap end whose forty candidates are two points:
    no six of them give a model (DEGENERATE)."""
    return gapped(np.random.default_rng(1), 5, 40, cap, {2: ROTATION}, shape="two", unique=False)


def count_batch(cap, M, n_land=90, extra=0, seed=64):
    """Six frames, a gap at frame 4 with exactly M candidates; with `extra`, raw counters above the capacity."""
    b = gapped(np.random.default_rng(seed), 6, n_land, cap, {3: ROTATION}, noise=0.001, extra=extra)
    return trim(b, 4, M, traj=dict(min_shared=4))


SHARED_LM = dict(max_reproj_px=1000.0)


def shared_batch(cap=8):
    """Capacity 8, five frames, a gap at frame 4: two slots of pair 0 match one keypoint of frame 1, so two landmarks share their
    later views and their tail, and the orphaned keypoint starts a landmark of its own in pair 1: nine candidates for eight places
    (the landmarks call at 1000 px, so that the landmark through the wrong keypoints is GOOD)."""
    b = gapped(np.random.default_rng(8), 5, cap, cap, {3: PAUSE}, unique=False)
    assert (lc.stored(b) == cap).all()
    first = b["matches"]["index"][0].copy()
    for i in range(1, cap):  # the first slot whose landmark through slot 0's keypoints comes out in front of every camera
        b["matches"]["index"][0] = first
        b["matches"]["index"][0, i] = first[0]
        trace = {}
        reference(b, traj=dict(min_shared=4), lm=SHARED_LM, trace=trace)
        if trace[4]["total"] == cap + 1:
            return b
    raise AssertionError("no pair of slots shares a tail with both landmarks GOOD")


def plain_batch(cap):
    """Six views without a gap."""
    return lc.views(np.random.default_rng(3), 6, 200, cap, steps=small_steps(5), noise=0.001, wrong=0.05)


# ---- the chain's chunks, the hop limit, two joins on one path (tests/test_gpu_bridge_cases.py) -------------------------------------
CHUNK = 64  # frames k_br_chain stages at a time
LONG_TRAJ = dict(min_shared=4)
LONG = dict(min_shared=4, hypotheses=64)
_FILL = ((3, ROTATION), (2, PAUSE), (5, ROTATION), (1, PAUSE), (4, ROTATION), (3, PAUSE), (2, ROTATION), (5, PAUSE))


def long_batch(cap=96, seed=7):
    """327 frames, six chunks of k_br_chain, of runs of about 90 landmarks joined with unrelated matches between them (the first
    frame of every run but the first is LOST behind matches that are all wrong).  Fillers are runs of seven or nine frames with one
    gap each, the gap's place and kind taken in turn from _FILL (a gap at a run's last frame is FIXED: nothing behind it starts).
    Under the trajectory's LONG_TRAJ and the bridge's LONG:
      frames 56-68   a run with gaps at 60 and 64: JOINED at 60 (root 56), 61-63 MOVED, frame 64 -- the first of chunk 1 -- a gap end
                     with anchor 63 that joins through S_60 of chunk 0 (RT, tT, oT set in the chunk before, root != oT, the gain a
                     product of two), 65-68 MOVED;
      frames 120-132 a run with gaps at 124 and 128, 129: anchor 127 for the two gap ends of chunk 2; 128 FIXED, 129 JOINED;
      frames 186-194 a run with a gap at 190: JOINED there, 191-194 MOVED, so 192-194 read S_190 of the chunk before;
      frame 255      the last of chunk 3, and frame 320, the first of chunk 5: each a run's first frame.
    tests/test_bridge_cases_ref.py asserts all of it and the census of statuses per chunk."""
    rng = np.random.default_rng(seed)
    kw = dict(noise=0.002, wrong=0.05)
    runs, turn = [], [0]

    def fill(count):  # `count` frames: runs of seven, and as many of nine as make the count
        nines = count % 7 * 4 % 7
        while count:
            n = 9 if nines else 7
            nines -= n == 9
            k, kind = _FILL[turn[0] % len(_FILL)]
            turn[0] += 1
            runs.append(gapped(rng, n, 90, cap, {k: kind}, **kw))
            count -= n
        assert count == 0

    fill(56)  # 0 .. 55
    runs.append(gapped(rng, 13, 90, cap, {3: ROTATION, 7: PAUSE}, **kw))  # 56 .. 68
    fill(51)  # 69 .. 119
    runs.append(gapped(rng, 13, 90, cap, {3: ROTATION, 7: PAUSE, 8: PAUSE}, **kw))  # 120 .. 132
    fill(53)  # 133 .. 185
    runs.append(gapped(rng, 9, 90, cap, {3: ROTATION}, **kw))  # 186 .. 194
    fill(60)  # 195 .. 254
    fill(7)  # 255 .. 261
    fill(58)  # 262 .. 319
    fill(7)  # 320 .. 326
    b = lc.join(runs, bridge=True)
    assert b["n"] == 327 and {56, 120, 186, 255, 320} <= set(b["first"].tolist())
    return b


HOP_GAPS = {k: PAUSE for k in range(3, 20)}


def hop_batch(cap=256):
    """24 frames, seventeen LOST frames (4 to 20) behind anchor 3: a pause of seventeen steps.  Two hundredths of every hop's matches
    are ORB_MATCH_NONE, so each further hop has fewer candidates."""
    return gapped(np.random.default_rng(16), 24, 200, cap, HOP_GAPS, noise=0.002, lost=0.02)


def double_batch(cap=300):
    """13 frames, gaps at frames 4 and 8: both JOINED, so frame 8 joins through S_4 (sigma != 1, root 0 != oT = 4) and frames 5 to 7,
    the JOINED frame 8's own segment, are MOVED."""
    return gapped(np.random.default_rng(13), 13, 300, cap, {3: ROTATION, 7: PAUSE}, wrong=0.05, noise=0.002)


def edge_batch(cap=1100):
    """Six frames, a gap at frame 4 with 493 candidates of which 439 are shared (inliers of the fix whose point of pair 4 is GOOD);
    frame 5 is START whatever pair 4's points hold, so frame 4's join is evaluated."""
    return gapped(np.random.default_rng(64), 6, 900, cap, {3: ROTATION}, noise=0.001)


# ---- BR-5's inputs of one gap end, to the bit ------------------------------------------------------------------------------------
def join_state(b, g, traj=None, lm=None, **params):
    """What BR-5 of gap end g works on: the fix does not read points[g], so all of this holds for every points[g] the setters below
    write.  Returns dict(g, slots: the keypoint slots k_g of the candidates that are inliers of the fix and whose point is GOOD, in
    candidate order; z: Y'z of each (binary32, bridge_ref.join_ratios' expression); args: join_ratios' arguments before the points)."""
    trace = {}
    fr, lms, out, _ = reference(b, traj=traj, lm=lm, trace=trace, **params)
    t = trace[g]
    assert int(t["fix"]["status"]) == L_OK and g + 1 < b["n"] and fr["status"][g + 1] == START, (t["fix"], fr["status"])
    p = br.defaults(**{**lc.intrinsics(b["W"], b["H"], b["focal"]), **params})
    nq, corners, matches, _ = inputs(b)
    k, rec, _, _ = br.candidates(g, int(out[g]["anchor"]), nq, corners[g], matches, fr, lms, b["cap"], p)
    assert k.tolist() == t["k"].tolist()
    inl = t["inliers"]
    rx, tx = [F(v) for v in t["fix"]["r"]], [F(v) for v in t["fix"]["t"]]
    j, Y = k[inl], rec[inl]
    z = (((rx[6] * Y[:, 0] + rx[7] * Y[:, 1]) + rx[8] * Y[:, 2]) + tx[2]).astype(F)
    good = (b["points"]["flags"][g, j] & GOOD) != 0
    slots = j[good]
    assert len(set(slots.tolist())) == len(slots) and (z[good] > 0).all()  # one candidate per keypoint: a flag decides one ratio
    return dict(g=g, slots=slots, z=z[good], args=(rec, k, inl, rx, tx), shared=int(out[g]["shared"]))


def _with_points(b):
    out = dict(b)
    out["points"] = b["points"].copy()
    return out


def ratios_of(b, state):
    """BR-5's ratios of the state's gap end under b's points."""
    return br.join_ratios(*state["args"], b["points"][state["g"]])


def set_shared(b, g, m, state=None, **kw):
    """A copy of b in which gap end g's shared count is exactly m: the GOOD flag of points[g] is cleared at all but the first m of
    the slots of join_state(b, g, **kw) (`state`, when the caller has it already)."""
    state = join_state(b, g, **kw) if state is None else state
    assert state["g"] == g and 0 <= m <= len(state["slots"])
    out = _with_points(b)
    out["points"]["flags"][state["g"], state["slots"][m:]] = 0
    assert len(ratios_of(out, state)) == m
    return out


def _depth_for(z, rho):
    """A binary32 Z with z / Z == rho in binary32, or None: the quotient z / rho and its neighbours."""
    with np.errstate(all="ignore"):
        c = F(z) / F(rho)
        for cand in (c, np.nextafter(c, F(0)), np.nextafter(c, F(np.inf)), np.nextafter(np.nextafter(c, F(0)), F(0)),
                     np.nextafter(np.nextafter(c, F(np.inf)), F(np.inf))):
            if np.isfinite(cand) and cand > 0 and (F(z) / F(cand)).view(U) == F(rho).view(U):
                return F(cand)
    return None


def set_ratios(b, g, rhos, state=None, **kw):
    """A copy of b in which gap end g's ratios are exactly `rhos` (binary32 values, as a multiset: each goes to the first free
    slot whose Y'z has a binary32 Z with Y'z / Z == rho; a power of two always has one, Z = Y'z / 2^k, and 1.0 has Z = Y'z).
    The other shared slots lose their GOOD flag."""
    state = join_state(b, g, **kw) if state is None else state
    rhos = np.asarray(rhos, F)
    out = _with_points(b)
    slots, z = state["slots"], state["z"]
    assert state["g"] == g
    assert len(rhos) <= len(slots)
    free = list(range(len(slots)))
    for rho in rhos:
        for c in free:
            Z = _depth_for(z[c], rho)
            if Z is not None:
                out["points"]["z"][g, slots[c]] = Z
                free.remove(c)
                break
        else:
            raise AssertionError("no slot gives the ratio %r" % rho)
    out["points"]["flags"][g, slots[free]] = 0
    got = ratios_of(out, state)
    assert np.sort(got.view(U)).tolist() == np.sort(rhos.view(U)).tolist()
    return out


def set_depths(b, g, depths, state=None, **kw):
    """A copy of b with points[g].z of the first len(depths) shared slots set to `depths` as they are (any bits)."""
    state = join_state(b, g, **kw) if state is None else state
    out = _with_points(b)
    out["points"]["z"][g, state["slots"][:len(depths)]] = np.asarray(depths, F)
    return out


def tolerance_edge(gamma, tol):
    """The largest binary32 rho >= gamma with |rho - gamma| <= tol * gamma as binary32 computes both sides (TJ-3's test)."""
    gamma, tol = F(gamma), F(tol)
    tg = tol * gamma
    rho = gamma + tg
    while not (np.abs(rho - gamma) <= tg):
        rho = np.nextafter(rho, F(0))
    while np.abs(np.nextafter(rho, F(np.inf)) - gamma) <= tg:
        rho = np.nextafter(rho, F(np.inf))
    return rho


# ---- BR-5's edges on edge_batch's gap end (frame 4) ------------------------------------------------------------------------------
EDGE_G = 4
EDGE_TRAJ = dict(min_shared=4)
EDGE = dict(min_shared=1, hypotheses=64)
EDGE_SHARED = (1, 2, 3, 255, 256, 257, 439)  # one ratio, the ballots' and the select's 256 threads, every shared slot
EDGE_DEPTHS = (0.0, -0.0, -1.0, np.inf, np.nan, 1e-45, 3e38)  # rho: inf, -inf, < 0, 0, NaN, inf (a subnormal Z), about 1e-37


def _bits(values):
    return np.array(values, U).view(F)


def edge_cases(b=None, state=None):
    """[dict(name, b, params, expect)]: edge_batch with points[4] rewritten, the bridge parameters of the call and what the
    construction implies for frame 4's record -- status, shared, consistent and, where it is JOINED, the bits of its gain (gamma:
    the root segment's sigma is 1).  The select's passes take the bytes of a ratio's bits from the top; lane l of the scan owns
    bins 4l .. 4l + 3."""
    b = edge_batch() if b is None else b
    g = EDGE_G
    state = join_state(b, g, traj=EDGE_TRAJ, **EDGE) if state is None else state
    assert len(state["slots"]) == state["shared"] == EDGE_SHARED[-1]
    out = []

    def case(name, batch, status, shared, consistent=None, gain=None, **params):
        expect = dict(status=status, shared=shared)
        if consistent is not None:
            expect["consistent"] = consistent
        if gain is not None:
            expect["gain_bits"] = int(F(gain).view(U))
        out.append(dict(name=name, b=batch, params={**EDGE, **params}, expect=expect))

    def ratios(name, rhos, status, consistent, gain=None, **params):
        case(name, set_ratios(b, g, rhos, state), status, len(rhos), consistent, gain if status == JOINED else None, **params)

    for m in EDGE_SHARED:
        case("shared_%d" % m, set_shared(b, g, m, state), None, m)
    ratios("equal_300", [1.0] * 300, JOINED, 300, 1.0)  # every pass ends in one bin
    ratios("equal_1", [0.5], JOINED, 1, 0.5)
    ratios("half_even", [1.0] * 5 + [2.0] * 5, JOINED, 5, 1.0)  # the lower median; 1000 * 5 == 500 * 10
    ratios("half_odd", [1.0] * 5 + [2.0] * 6, JOINED, 6, 2.0)
    ratios("half_even_256", [1.0] * 128 + [2.0] * 128, JOINED, 128, 1.0)
    low = [0x3F800000 + j for j in range(256)]  # 257 values that differ in the lowest byte only: rank 128
    ratios("low_byte_7f", _bits(low + [0x3F800010]), JOINED, 257, _bits([0x3F80007F])[0])  # the fourth bin of lane 31
    ratios("low_byte_80", _bits(low + [0x3F8000F0]), JOINED, 257, _bits([0x3F800080])[0])  # the first bin of lane 32
    # values that differ in the top byte only (powers of four); one consistent, so 1 permille lets the join hold and show gamma
    ratios("top_byte_3f", _bits([t << 24 for t in range(0x30, 0x50)]), JOINED, 1, _bits([0x3F << 24])[0], consistent_permille=1)  # rank 15 of 32
    ratios("top_byte_40", _bits([t << 24 for t in range(0x31, 0x50)]), JOINED, 1, _bits([0x40 << 24])[0], consistent_permille=1)  # rank 15 of 31
    # the second pass: the rank in bin 0x7f (lane 31's fourth) and 0x80 (lane 32's first) of the second byte
    mid = [0x3F000000 | t << 16 for t in range(0x78, 0x88)]  # 0.96875 .. 1.0546875
    ratios("second_byte_7f", _bits(mid), JOINED, 16, _bits([0x3F7F0000])[0])  # rank 7 of 16
    ratios("second_byte_80", _bits(mid[1:]), JOINED, 15, _bits([0x3F800000])[0])  # rank 7 of 15
    # |rho - gamma| <= tol * gamma: equality holds, the next binary32 above does not
    up = lambda x: np.nextafter(F(x), F(np.inf))
    ratios("tol_1_at", [1.0, 1.0, 2.0], JOINED, 3, 1.0, scale_tolerance=1.0, consistent_permille=1000)
    ratios("tol_1_above", [1.0, 1.0, up(2.0)], FIXED, 2, scale_tolerance=1.0, consistent_permille=1000)
    ratios("tol_8th_at", [1.0, 1.0, 1.125], JOINED, 3, 1.0, scale_tolerance=0.125, consistent_permille=1000)
    ratios("tol_8th_above", [1.0, 1.0, up(1.125)], FIXED, 2, scale_tolerance=0.125, consistent_permille=1000)
    edge = tolerance_edge(1.0, 0.1)  # the default tolerance: gamma + tol * gamma is rounded, the edge is found by the test itself
    ratios("tol_default_at", [1.0, 1.0, edge], JOINED, 3, 1.0, consistent_permille=1000)
    ratios("tol_default_above", [1.0, 1.0, up(edge)], FIXED, 2, consistent_permille=1000)
    # 1000 * consistent >= permille * m
    ratios("permille_2_of_4", [1.0, 1.0, 4.0, 4.0], JOINED, 2, 1.0, consistent_permille=500)
    ratios("permille_1_of_3", [1.0, 2.0, 4.0], FIXED, 1, consistent_permille=500)
    ratios("min_shared_at", [1.0] * 10, JOINED, 10, 1.0, min_shared=10)
    ratios("min_shared_above", [1.0] * 10, FIXED, 10, min_shared=11)
    # Z that gives no ratio: six of the seven are dropped, the tiny quotient by 3e38 counts
    case("depths", set_depths(b, g, EDGE_DEPTHS, state), None, state["shared"] - 6)
    return out


def check_expect(case, rec):
    """The outcome the construction implies, on frame EDGE_G's record."""
    for k, v in case["expect"].items():
        if v is None:
            continue
        got = int(rec["gain"].view(U)) if k == "gain_bits" else int(rec[k])
        assert got == int(v), (case["name"], k, got, v, rec)
