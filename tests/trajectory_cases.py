"""Hand-built inputs of the trajectory stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_trajectory_consecutive reads the raw counters, the matcher's records, the pose records and the pairs'
points.  What match -> verify_epipolar -> pose produce from constructed camera paths never drives its kernels to the inputs they were
written around: a rank in the last bin of a lane's four, a ratio that is -0 or overflows, a tolerance met exactly, a second 64-frame
chunk of the chain.  The builders here make such inputs directly, as plain arrays together with the outcome the construction
implies; `pack` lays many independent joints into one batch, `inject_pose` writes a batch over a program's buffers
(orb_debug_pose_buffers), and `select_trace` labels a joint's ratios with the path the radix select of TJ-3 takes through them, from
the definition of the selection, so that a census can say which paths the committed cases reach.

A joint case (`joint_case`) is compact: n_a points of pair a with one match index each, n_b points of pair b, the two pose records;
by default R = I and t = 0 in pair a and z = 1 in pair b, so that point i's ratio is its own z exactly.  `pack` decides the slots.

No case lets the result of an operation on a NaN, of inf - inf or of 0 * inf reach an output byte: the definition fixes binary32
`+ - * /`, not the sign and payload of a NaN that they produce.  NaN and inf inputs are there, and reach the outputs by copies
(START, RESTART, a copied map row) and through `isfinite`; tests/test_trajectory_cases_ref.py asserts that nothing else stores one.
"""
import itertools

import numpy as np

import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
U = np.uint32
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX
OK = orb.ORB_POSE_OK
NOT_OK = (orb.ORB_POSE_NOMODEL, orb.ORB_POSE_FEW, orb.ORB_POSE_AMBIGUOUS, orb.ORB_POSE_LOW_PARALLAX)
IDENTITY = np.eye(3, dtype=F).ravel()
FLT_MAX_BITS = 0x7F7FFFFF
# index codes of a compact case (values >= 0 name a point of pair b)
NONE, AT_NQ = -1, -2  # ORB_MATCH_NONE; the stored count of frame b itself (the first index that is no keypoint)
CHAINED, START, FEW, SPREAD, LOST, ORIGIN = (orb.ORB_TRAJ_CHAINED, orb.ORB_TRAJ_START, orb.ORB_TRAJ_RESTART_FEW, orb.ORB_TRAJ_RESTART_SPREAD,
                                             orb.ORB_TRAJ_LOST, orb.ORB_TRAJ_ORIGIN)


def bits(x):
    return np.asarray(x, F).view(U)


def floats(b):
    return np.asarray(b, U).view(F)


def pose(status=OK, r=IDENTITY, t=(0, 0, 0)):
    p = np.zeros((), orb.POSE_DTYPE)
    p["r"], p["t"], p["status"] = r, t, status
    return p


def points(n, x=0.0, y=0.0, z=0.0, flags=GOOD):
    p = np.zeros(n, orb.POINT_DTYPE)
    p["x"], p["y"], p["z"], p["flags"] = x, y, z, flags
    return p


# ---- one joint ---------------------------------------------------------------------------------------------------------------
def joint_case(name, rho, index=None, flags_a=None, flags_b=None, zb=None, pose_a=None, pose_b=None, pa=None, pb=None, live_a=None,
               live_b=None, extra_a=0, extra_b=0, params=None, **expect):
    """A compact joint.  Pair a's point i is (0, 0, rho[i]) (or pa[i]) with flags_a[i] (GOOD) and match index index[i] (i); pair b's
    point j is (0, 0, zb[j]) (1) (or pb[j]) with flags_b[j] (GOOD).  live_a / live_b: how many of the points lie below the frame's raw
    counter (all); the others are stale records above it.  extra_a / extra_b: the raw counter exceeds the capacity by so much (needs
    every point live).  params: the OrbTrajectoryParams under which `expect` (shared, step_bits, consistent, status of the frame behind
    the joint) holds."""
    if pa is None:
        rho = np.asarray(rho, F)
        pa = points(len(rho), z=rho, flags=GOOD if flags_a is None else flags_a)
    n = len(pa)
    index = np.arange(n) if index is None else np.asarray(index, np.int64)
    if pb is None:
        nb = max(int(index.max()) + 1 if len(index) else 0, 0 if zb is None else len(np.atleast_1d(zb)), 0 if flags_b is None else len(np.atleast_1d(flags_b)))
        pb = points(nb, z=1.0 if zb is None else zb, flags=GOOD if flags_b is None else flags_b)
    assert len(index) == n and index.max(initial=-1) < len(pb)
    live_a, live_b = n if live_a is None else live_a, len(pb) if live_b is None else live_b
    assert (not extra_a or live_a == n) and (not extra_b or live_b == len(pb))
    return dict(name=name, pa=pa, index=index, pb=pb, pose_a=pose() if pose_a is None else pose_a, pose_b=pose() if pose_b is None else pose_b,
                live_a=live_a, live_b=live_b, extra_a=extra_a, extra_b=extra_b, params=dict(params or {}), expect=expect)


def size(case):
    """The smallest capacity that holds the case."""
    return max(len(case["pa"]), len(case["pb"]), 1)


def lay(case, cap, rng=None):
    """One case as the three frames of a batch of capacity cap: (counts (2,), matches (cap,), points a (cap,), points b (cap,)).
    rng None: point k in slot k.  Otherwise the live points go to random slots below the counter and the stale ones to random slots
    from the counter up, each group with its first and last slot taken (slot cap - 1 is always in use, and when cap > 1024 so
    are slots on both sides of 1024); every other slot holds a point that is not GOOD and a match record, both of arbitrary bits."""
    na, nb = len(case["pa"]), len(case["pb"])
    assert size(case) <= cap, (case["name"], cap)

    def slots(n, live):
        """-> (counter, slot of each point)"""
        if rng is None:
            return (cap if live == n else live), np.arange(n)
        c = cap if live == n else int(rng.integers(live, cap - (n - live) + 1))
        out = np.zeros(n, np.int64)
        for lo, hi, k0, k1 in ((0, c, 0, live), (c, cap, live, n)):
            k = k1 - k0
            if not k:
                continue
            must = [hi - 1, lo][:k] if k > 1 or hi == cap else [lo]  # one point: the last slot of the row, else the first of its range
            if lo < 1024 < hi and k >= 4:
                must += [s for s in (1023, 1024) if s not in must]
            rest = np.setdiff1d(np.arange(lo, hi), must)
            pick = np.concatenate([np.array(must, np.int64), rng.choice(rest, size=k - len(must), replace=False)])
            out[k0:k1] = rng.permutation(pick)
        return c, out

    ca, sa = slots(na, case["live_a"])
    cb, sb = slots(nb, case["live_b"])
    if rng is None:
        A, B, M = np.zeros(cap, orb.POINT_DTYPE), np.zeros(cap, orb.POINT_DTYPE), np.zeros(cap, orb.MATCH_DTYPE)
    else:
        A, B = (rng.integers(0, 1 << 32, (cap, 4), dtype=U).view(orb.POINT_DTYPE).ravel().copy() for _ in range(2))
        A["flags"] &= ~U(GOOD)
        B["flags"] &= ~U(GOOD)
        M = rng.integers(0, 1 << 32, (cap, 2), dtype=U).view(orb.MATCH_DTYPE).ravel().copy()
    A[sa], B[sb] = case["pa"], case["pb"]
    idx = case["index"]
    M["index"][sa] = np.where(idx >= 0, sb[np.maximum(idx, 0)] if nb else 0, np.where(idx == AT_NQ, min(cb, cap), orb.ORB_MATCH_NONE))
    return np.array([ca + case["extra_a"], cb + case["extra_b"]], U), M, A, B


def batch(counts, matches, poses, points_, cap):
    """A batch as dense arrays: counts (n,), matches (n - 1, cap), poses (n - 1,), points (n - 1, cap)."""
    n = len(poses) + 1
    return dict(counts=np.asarray(counts, U), matches=np.stack(matches).astype(orb.MATCH_DTYPE), poses=np.array(poses, orb.POSE_DTYPE),
                points=np.stack(points_).astype(orb.POINT_DTYPE), cap=cap, n=n)


def pack(cases, cap, seed=0):
    """Many independent joints in one batch of 3 k + 1 frames: case c is frames 3 c, 3 c + 1 and 3 c + 2 -- pair 3 c OK, pair 3 c + 1
    OK, pair 3 c + 2 not OK (every other status in turn, with a record and points of arbitrary bits) --, so joint 3 c + 1 is the
    case's, frame 3 c + 1 is START, frame 3 c + 2 carries the joint's outcome and frame 3 c + 3 is LOST.  Slots as `lay` scatters
    them.  Returns the batch with `joint`: the frame behind each case's joint."""
    rng = np.random.default_rng(seed)
    k = len(cases)
    counts = rng.integers(0, 2 * cap, 3 * k + 1).astype(U)
    M = rng.integers(0, 1 << 32, (3 * k, cap, 2), dtype=U).view(orb.MATCH_DTYPE).reshape(3 * k, cap)
    P = rng.integers(0, 1 << 32, (3 * k, cap, 4), dtype=U).view(orb.POINT_DTYPE).reshape(3 * k, cap)
    poses = rng.integers(0, 1 << 32, (3 * k, 16), dtype=U).view(orb.POSE_DTYPE).reshape(3 * k)
    for c, case in enumerate(cases):
        counts[3 * c:3 * c + 2], M[3 * c], P[3 * c], P[3 * c + 1] = lay(case, cap, rng)
        poses[3 * c], poses[3 * c + 1] = case["pose_a"], case["pose_b"]
        poses[3 * c + 2]["status"] = NOT_OK[c % len(NOT_OK)]
        if (case["index"] == AT_NQ).any():  # where the index points when frame b's stored count is the capacity: the row behind
            P[3 * c + 2][0] = (0.0, 0.0, 1.0, GOOD)
    b = batch(counts, M, poses, P, cap)
    b["joint"] = [3 * c + 2 for c in range(k)]
    return b


def reference(b, n_frames=None, **params):
    """trajectory_ref.trajectory on a batch's arrays (the counts clipped to the capacity, as TJ-1 stores them)."""
    n = b["n"] if n_frames is None else n_frames
    cap = b["cap"]
    nq = np.minimum(b["counts"], cap)
    return tr.trajectory(nq[:n], [b["matches"][f][:nq[f]] for f in range(n - 1)], list(b["poses"][:n - 1]), list(b["points"][:n - 1]), cap, **params)


def check_expect(case, rec):
    """The outcome the construction implies, on the record of the frame behind the case's joint."""
    assert rec["status"] != LOST and rec["status"] != START, (case["name"], rec)  # the joint was evaluated
    for k, v in case["expect"].items():
        got = int(rec["step"].view(U)) if k == "step_bits" else int(rec[k])
        assert got == int(v), (case["name"], k, got, v, rec)


def param_sets(cases):
    out = []
    for c in cases:
        if c["params"] not in out:
            out.append(c["params"])
    return out


# ---- injection ---------------------------------------------------------------------------------------------------------------
def prepare(prog, n_frames, width, height):
    """A program whose match and pose stages are fresh on a batch of n_frames empty frames: zero images, zero counters, then
    match -> verify_epipolar -> pose once.  The trajectory call reads the counters live: inject the case's own afterwards."""
    import constructed as C
    prog.extract_batch_host(np.zeros((n_frames, height, width, 4), np.uint8))
    C.inject(prog, np.zeros(n_frames, U))
    prog.match_consecutive(n_frames)
    prog.verify_epipolar(n_frames)
    prog.pose_consecutive(n_frames, fx=100.0, fy=100.0, cx=0.5 * (width - 1), cy=0.5 * (height - 1))
    prog.batch_sync()


def inject_pose(prog, matches=None, poses=None, points_=None, first=0):
    """Overwrites rows first .. of what the trajectory stage reads besides the counters: matches (n, cap) MATCH_DTYPE, poses (n,)
    POSE_DTYPE, points (n, cap) POINT_DTYPE, each optional.  The stages run on the program's streams, not torch's: everything queued
    is finished before the copies start, and the copies before this returns.  No stage's freshness changes."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    B, cap = cfg.max_batch, cfg.max_features
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    d_m, d_p, d_x = prog.debug_pose_buffers()
    for addr, arr, dtype, words in ((d_m, matches, orb.MATCH_DTYPE, 2), (d_p, poses, orb.POSE_DTYPE, 16), (d_x, points_, orb.POINT_DTYPE, 4)):
        if arr is None:
            continue
        a = np.ascontiguousarray(arr, dtype=dtype)
        n = len(a)
        assert first + n <= B and (words == 16 or a.shape == (n, cap)), (a.shape, B, cap)
        row = words if words == 16 else cap * words
        node.as_tensor(addr, (B, row), "<i4", dev)[first:first + n].copy_(torch.from_numpy(a.view(np.int32).reshape(n, row)))
    torch.cuda.synchronize(dev)


def inject_batch(prog, b):
    import constructed as C
    inject_pose(prog, b["matches"], b["poses"], b["points"])
    C.inject(prog, b["counts"])


# ---- the radix select, from its definition -------------------------------------------------------------------------------------
def select_trace(ratio_bits):
    """Labels of TJ-3's selection on the bits of a joint's ratios (non-empty, each in [1, 0x7f7fffff]): for each of the four passes,
    most significant byte first, over the ratios that share the bytes found so far: `bin` the byte value that holds the rank,
    `populated` how many byte values occur, `rank` the rank the pass starts with, `carried` the rank within the bin, `below` the
    populated byte values below `bin` in its aligned group of four.  Also `g` (the bits selected) and `duplicates` (ratios equal to
    it)."""
    cand = np.sort(np.asarray(ratio_bits, U))
    assert len(cand) and cand[0] >= 1 and cand[-1] <= FLT_MAX_BITS
    k = (len(cand) - 1) // 2
    passes = []
    for shift in (24, 16, 8, 0):
        byte = (cand >> U(shift)) & U(255)
        hist = np.bincount(byte, minlength=256)
        b = int(byte[k])  # the candidates are sorted: rank k's own byte
        lo = int(hist[:b].sum())
        passes.append(dict(bin=b, populated=int((hist > 0).sum()), rank=k, carried=k - lo, below=int((hist[b & ~3:b] > 0).sum())))
        k -= lo
        cand = cand[byte == b]
    return dict(passes=passes, g=int(cand[0]), duplicates=len(cand))


def case_ratio_bits(case, **params):
    """The ratio bits of a compact case, through trajectory_ref.ratios on its identity layout."""
    cap = size(case)
    counts, M, A, B = lay(case, cap)
    nq = np.minimum(counts, cap)
    need = bool(tr.defaults(**params)["flags"] & orb.ORB_TRAJ_NEED_PARALLAX)
    return tr.ratios(nq[0], nq[1], M[:nq[0]], case["pose_a"], A, B, need).view(U)


# ---- selection cases -------------------------------------------------------------------------------------------------------------
# The parameters of the selection cases: a joint of distinct ratios is SPREAD, whose record shows the step, and restarts -- a step near
# FLT_MAX is never multiplied into a scale or a map point.  All ratios equal: CHAINED with that step.
SELECT = dict(min_shared=1, scale_tolerance=1e-7, consistent_permille=1000)


def select_case(p, b, seed, decoys=3):
    """Ratios whose rank lands in byte value b of pass p with every lower byte value of b's aligned group of four populated.  In
    ascending order: for p > 0, `decoys` ratios whose bytes above pass p are smaller and whose byte at pass p is b (the histogram of a
    pass must leave them out); two ratios in each byte value of the group below b; five in b; as many above as below plus two -- in
    the byte values above b (the next three first) and, for p > 0, `decoys` of them (all, when b is 255) with larger bytes above pass
    p and b at pass p.  The rank (m - 1) / 2 is then the fourth of the five: `carried` is 3 at pass p.  The five share everything
    above pass p and differ below it (p = 3: they are equal).  Byte value 0x7f of pass 0 has nothing above it: one ratio in each of
    0x7c .. 0x7e and the five, rank 3, the first of them."""
    rng = np.random.default_rng(seed)
    shift = 24 - 8 * p
    top = 0x7F if p == 0 else 0xFF
    assert 0 <= b <= top

    def low():  # random bytes below pass p
        return int(rng.integers(0, 1 << shift)) if shift else 0

    prefix = 0 if p == 0 else int(rng.integers(0x20 << (8 * (p - 1)), 0x60 << (8 * (p - 1))))  # the bytes above pass p, the top one 0x20 .. 0x5f

    def make(byte, lo, pre=prefix):
        return (pre << (shift + 8)) | (byte << shift) | lo

    def other(k, sign):  # another prefix: the lowest or the highest of its bytes differs
        return prefix + sign * ((1 + k) if k % 2 == 0 else (1 << (8 * (p - 1))) + k)

    five = [make(b, low()) for _ in range(5)]
    if p == 0 and b == 0x7F:
        five = [FLT_MAX_BITS - int(rng.integers(0, 1 << 20)) for _ in range(4)] + [FLT_MAX_BITS]
        vals = [make(q, low()) for q in range(0x7C, 0x7F)] + five
    else:
        if p == 0 and b == 0:
            five = [1, 0x007FFFFF, 0x00800000] + [int(rng.integers(2, 1 << 24)) for _ in range(2)]  # subnormals, the smallest normal
        d = decoys if p else 0
        vals = [make(b, low(), other(k, -1)) for k in range(d)]
        vals += [make(q, low()) for q in range(b & ~3, b) for _ in range(2)]
        n_above = len(vals) + 2
        vals += five
        ups = list(range(b + 1, top + 1))
        n_far = (d if ups else n_above) if p else 0
        vals += [make(ups[k] if k < min(3, len(ups)) else int(rng.choice(ups)), low()) for k in range(n_above - n_far)]
        vals += [make(b, low(), other(k, +1)) for k in range(n_far)]
    vals = np.array(vals, np.uint64)
    assert vals.min() >= 1 and vals.max() <= FLT_MAX_BITS, (p, b)
    vals = vals.astype(U)[rng.permutation(len(vals))]
    g = int(np.sort(vals)[(len(vals) - 1) // 2])
    assert g == sorted(five)[0 if (p == 0 and b == 0x7F) else 3], (p, b)
    return joint_case("select pass %d byte %02x" % (p, b), floats(vals), params=SELECT, shared=len(vals), step_bits=g, status=SPREAD)


GROUPS = (0x3C, 0x84, 0x10, 0xF8)  # the aligned group of four of pass p in the (pass, byte mod 4) grid


def run_case(case, cap=None, **params):
    """A compact case alone, point k in slot k: (frames (3,), map (3, cap)) of trajectory_ref."""
    cap = size(case) + 3 if cap is None else cap
    counts, M, A, B = lay(case, cap)
    nq = np.minimum(counts, cap)
    return tr.trajectory([nq[0], nq[1], nq[1]], [M[:nq[0]], M[:nq[1]]], [case["pose_a"], case["pose_b"]], [A, B], cap, **params)


def selection_cases(cap):
    """The selection cases that fit a capacity (see the module's census in tests/test_trajectory_cases_ref.py)."""
    rng = np.random.default_rng(31)
    cases = [select_case(p, GROUPS[p] + q, 100 + 4 * p + q) for p in range(4) for q in range(4)]
    cases += [select_case(p, b, 200 + 2 * p + (b & 1)) for p in (1, 2, 3) for b in (0, 255)]
    cases += [select_case(0, 0, 220), select_case(0, 0x7F, 221)]
    # the first pass with two populated byte values (0x3f below 2.0, 0x40 from it), the rank in the second: 3 and 6
    cases.append(joint_case("straddling 2.0", F([1.5, 1.25, 1.75, 2.5, 3.0, 2.25, 3.5, 2.0, 3.75]), params=SELECT, shared=9,
                            step_bits=bits(2.25), status=SPREAD))
    # ratios that differ in their lowest byte only, in a scrambled order: ranks 0 .. 199 are bits base .. base + 199
    base = int(bits(1.25)) & ~0xFF
    perm = (base + np.random.default_rng(0).permutation(200)).astype(U)
    cases.append(joint_case("lowest byte, 200", floats(perm), shared=200, consistent=200, step_bits=base + 99, status=CHAINED))
    cases.append(joint_case("lowest byte, 199", floats(perm[:199]), shared=199, consistent=199, step_bits=sorted(perm[:199].tolist())[99], status=CHAINED))
    a, b = F(0.75), F(0.8)  # 5 x a, 4 x b > a: rank 4 of 9 is a; 4 x a, 5 x b: rank 4 is b
    cases.append(joint_case("duplicates 5a 4b", F([b, a, b, a, a, b, a, b, a]), shared=9, consistent=9, step_bits=bits(a), status=CHAINED))
    cases.append(joint_case("duplicates 4a 5b", F([b, a, b, a, b, b, a, b, a]), shared=9, consistent=9, step_bits=bits(b), status=CHAINED))
    cases.append(joint_case("all equal", np.full(9, 1.5, F), params=SELECT, shared=9, consistent=9, step_bits=bits(1.5), status=CHAINED))
    one = dict(min_shared=1)
    cases.append(joint_case("m = 1", F([3.0]), params=one, shared=1, consistent=1, step_bits=bits(3.0), status=CHAINED))
    # m = 2: the lower of the two; 1000 * 1 == 500 * 2 holds
    cases.append(joint_case("m = 2", F([3.0, 2.0]), params=one, shared=2, consistent=1, step_bits=bits(2.0), status=CHAINED))
    every = rng.integers(int(bits(0.5)), int(bits(2.0)), cap).astype(U)
    cases.append(joint_case("m = cap", floats(every), params=SELECT, shared=cap, step_bits=sorted(every.tolist())[(cap - 1) // 2], status=SPREAD))
    # ratios across exponents, subnormals included: the bits order them
    cases.append(joint_case("across exponents", F([1e-40, 3e-39, 1e-20, 0.5, 1.0, 2.0, 1e20, 3e38, 1.5]), params=dict(consistent_permille=1),
                            shared=9, consistent=1, step_bits=bits(1.0), status=CHAINED))
    for k in range(20):  # uniformly random bit patterns; m >= 2 distinct ratios are SPREAD under SELECT
        m = int(rng.integers(2, (min(cap, 64) if k % 2 else cap) + 1))
        v = rng.integers(1, FLT_MAX_BITS + 1, m).astype(U)
        cases.append(joint_case("random bits %d" % k, floats(v), params=SELECT, shared=m, step_bits=sorted(v.tolist())[(m - 1) // 2], status=SPREAD))
    return [c for c in cases if size(c) <= cap]


def ratio_cases():
    """What counts as a ratio (TJ-2).  Each case has nine plain ratios of 1 besides the ones in question, so that the joint holds under
    the default parameters and `shared` says how many counted."""
    rng = np.random.default_rng(32)
    ones = np.ones(12, F)
    cases = []
    rho = ones.copy()
    rho[:3] = -1.0, 0.0, -0.0
    cases.append(joint_case("negative, 0, -0", rho, shared=9, status=CHAINED))
    rho, zb = ones.copy(), ones.copy()
    rho[1], zb[1], zb[2], zb[0] = 0.0, 0.0, 0.0, -0.0  # 0 / 0, 1 / 0, 1 / -0
    cases.append(joint_case("z = 0 in pair b: nan, inf, -inf", rho, zb=zb, shared=9, status=CHAINED))
    fa, fb = np.full(12, GOOD, U), np.full(12, GOOD, U)
    fa[3], fb[4], fa[5], fb[6] = 0, 0, PAR, 0xFFFFFFFE
    cases.append(joint_case("not GOOD on either side", ones, flags_a=fa, flags_b=fb, shared=8, status=CHAINED))
    idx = np.arange(12)
    idx[5] = NONE
    cases.append(joint_case("ORB_MATCH_NONE", ones, index=idx, shared=11, status=CHAINED))
    cases.append(joint_case("every i on one j", ones, index=np.zeros(12, np.int64), shared=12, status=CHAINED))
    fa, fb = np.full(12, GOOD | PAR, U), np.full(12, GOOD | PAR, U)
    fa[:2], fb[2:5] = GOOD, GOOD
    cases.append(joint_case("parallax flags, not asked for", ones, flags_a=fa, flags_b=fb, shared=12, status=CHAINED))
    cases.append(joint_case("NEED_PARALLAX", ones, flags_a=fa, flags_b=fb, params=dict(flags=orb.ORB_TRAJ_NEED_PARALLAX), shared=7, status=FEW))
    rho, zb = ones.copy(), ones.copy()
    rho[:2], zb[:2] = (1e30, 3e38), (1e-30, 0.5)
    cases.append(joint_case("quotient overflows", rho, zb=zb, shared=10, status=CHAINED))
    rho, zb = ones.copy(), ones.copy()
    rho[:2], zb[:2] = (1e-30, 1e-45), (1e30, 4.0)
    cases.append(joint_case("quotient underflows to 0", rho, zb=zb, shared=10, status=CHAINED))
    rho, zb = ones.copy(), ones.copy()
    rho[:3], zb[:3] = (1e-20, 1e-38, 1e-45), (1e20, 2.0, 1.0)
    cases.append(joint_case("subnormal quotient", rho, zb=zb, shared=12, consistent=9, step_bits=bits(1.0), status=CHAINED))
    # frame b's counter below its stored points: index n_q - 1 (the last live slot, which some live point takes) counts, index n_q
    # (a stale GOOD point with z = 1) and a stale point's slot do not
    idx = np.arange(12)
    idx[10] = AT_NQ
    cases.append(joint_case("index n_q and n_q - 1", ones, index=idx, live_b=10, shared=10, status=CHAINED))
    cases.append(joint_case("frame b's counter below its points", ones, live_b=9, shared=9, status=CHAINED))
    cases.append(joint_case("frame a's counter below its points", ones, live_a=9, shared=9, status=CHAINED))
    cases.append(joint_case("frame a's counter above the capacity", ones, extra_a=37, shared=12, status=CHAINED))
    cases.append(joint_case("frame b's counter above the capacity", ones, index=idx, extra_b=5, shared=11, status=CHAINED))
    for k in range(20):  # random finite poses (no rotations) and points: the order of ((r0 x + r1 y) + r2 z) + t2 shows
        n = 24
        pa, pb = points(n), points(n)
        for q in (pa, pb):
            q["x"], q["y"], q["z"] = (rng.normal(0, 3, n).astype(F) for _ in range(3))
        cases.append(joint_case("random pose %d" % k, None, pa=pa, pb=pb, index=rng.integers(0, n, n), params=dict(min_shared=1),
                                pose_a=pose(r=rng.normal(0, 1, 9), t=rng.normal(0, 2, 3)), pose_b=pose(r=rng.normal(0, 1, 9), t=rng.normal(0, 2, 3))))
    # an OK pose of inf and nan (quiet, with a payload): no ratio is finite; START copies the record, RESTART_FEW the next pair's
    nan = floats([0x7FC01234])[0]
    bad = pose(r=[np.inf, 1, 0, 0, -np.inf, 0, nan, 0, 1], t=(1, -np.inf, nan))
    cases.append(joint_case("pose of inf and nan", ones, pose_a=bad, shared=0, consistent=0, step_bits=0, status=FEW))
    bad = pose(r=[1, 0, 0, 0, 1, 0, 0, 0, np.inf], t=(0, 0, -np.inf))  # inf - inf before the division
    cases.append(joint_case("pose row of inf", ones, pose_a=bad, shared=0, consistent=0, step_bits=0, status=FEW))
    return cases


def verdict_cases():
    """TJ-3's and TJ-4's comparisons met exactly and missed by one."""
    nine = F([1.02, 0.98, 1.0, 1.01, 0.99, 1.03, 0.97, 1.04, 0.96])
    ten = F([0.5, 0.6, 0.7, 0.95, 1.0, 1.05, 1.08, 1.5, 2.0, 3.0])  # four within 10 % of the median 1.0
    up = lambda v, to: np.nextafter(F(v), F(to))
    edge = F([0.875, 1.125, up(0.875, 0), up(1.125, 2), 1, 1, 1, 1, 1])  # |rho - 1| == 0.125 exactly (in), and one ulp further (exact too: out)
    sub = F([1, 1, 1, 1, 1, up(1, 0), up(1, 2), 0.5, 2])
    return [joint_case("min_shared == m", nine, params=dict(min_shared=9), shared=9, consistent=9, step_bits=bits(1.0), status=CHAINED),
            joint_case("min_shared == m + 1", nine, params=dict(min_shared=10), shared=9, consistent=9, step_bits=0, status=FEW),
            joint_case("default: 1000 c < 500 m", ten, shared=10, consistent=4, step_bits=bits(1.0), status=SPREAD),
            joint_case("1000 c == permille m", ten, params=dict(consistent_permille=400), shared=10, consistent=4, step_bits=bits(1.0), status=CHAINED),
            joint_case("permille + 1", ten, params=dict(consistent_permille=401), shared=10, consistent=4, step_bits=bits(1.0), status=SPREAD),
            joint_case("|rho - g| == tol g", edge, params=dict(scale_tolerance=0.125), shared=9, consistent=7, step_bits=bits(1.0), status=CHAINED),
            joint_case("subnormal tol", sub, params=dict(scale_tolerance=1e-40), shared=9, consistent=5, step_bits=bits(1.0), status=CHAINED)]


def joint_cases(cap):
    return selection_cases(cap) + ratio_cases() + verdict_cases()


# ---- the chain ---------------------------------------------------------------------------------------------------------------
CHAIN_FRAMES, CHAIN_CAP = 260, 64  # k_traj_chain stages 64 frames at a time: frames 1..64, 65..128, 129..192, 193..256, 257..259
_STEP = (tr.rot("y", 0.7) @ tr.rot("x", 0.2) @ tr.rot("z", 0.1)).astype(F).ravel()
_REGULAR, _WILD = np.arange(12), np.arange(20, 32)


def _chain_points(z0, rng, positive=False):
    """A pair's points at capacity 64: twelve regular GOOD points in slots 0..11 with depths within 2 % of z0, twelve wild ones in
    slots 20..31 (depths z0 * 2^-5 .. 2^6; no query is matched to them unless a joint is meant to be SPREAD, and their own match
    index is NONE), a GOOD | PARALLAX point in slot 63, and slots that are not GOOD, of arbitrary bits (NaN payloads among them)."""
    P = rng.integers(0, 1 << 32, (CHAIN_CAP, 4), dtype=U).view(orb.POINT_DTYPE).ravel().copy()
    P["flags"] &= ~U(GOOD)
    P[22 + 20]["x"] = floats([0x7FC00055])[0]  # a NaN payload in a slot that is not GOOD, whatever the draw
    for s, z in ((_REGULAR, F(z0) * (F(1) + F(0.002) * _REGULAR.astype(F))), (_WILD, F(z0) * F(2.0) ** (np.arange(12) - 5).astype(F)), ([63], F(z0))):
        P["x"][s], P["y"][s] = (np.abs(rng.normal(0, 0.3, len(s))) + 0.01 if positive else rng.normal(0, 0.3, len(s)) for _ in range(2))
        P["z"][s], P["flags"][s] = z, GOOD
    P["flags"][63] = GOOD | PAR
    return P


def _chain_matches(kind, rng):
    """holds: regular i -> regular i of the next pair; few: three of them; spread: regular i -> wild i."""
    M = rng.integers(0, 1 << 32, (CHAIN_CAP, 2), dtype=U).view(orb.MATCH_DTYPE).ravel().copy()
    M["index"][_WILD], M["index"][63] = orb.ORB_MATCH_NONE, orb.ORB_MATCH_NONE
    M["index"][_REGULAR] = _WILD if kind == "spread" else _REGULAR
    if kind == "few":
        M["index"][_REGULAR[3:]] = orb.ORB_MATCH_NONE
    return M


def _chain_base(seed, n=CHAIN_FRAMES):
    """Every pair OK with one small rotation and t = (0.6, 0, 0.8), depths at which r22 z + t2 = z up to rounding (every step is 1
    within 2 %), raw counters at and above the capacity: ORIGIN, START and CHAINED from there on."""
    rng = np.random.default_rng(seed)
    z0 = F(0.8) / (F(1) - _STEP[8])
    P = np.stack([_chain_points(z0, rng) for _ in range(n - 1)])
    M = np.stack([_chain_matches("holds", rng) for _ in range(n - 1)])
    poses = np.array([pose(r=_STEP, t=(0.6, 0.0, 0.8))] * (n - 1), orb.POSE_DTYPE)
    counts = (CHAIN_CAP + rng.integers(0, 3, n)).astype(U)
    return rng, counts, M, poses, P, [ORIGIN, START] + [CHAINED] * (n - 2)


def _lose(poses, plan, f, status):
    """Frame f LOST by pair f - 1's status (its record otherwise as it was); frame f + 1 then STARTs."""
    poses[f - 1]["status"] = status
    plan[f] = LOST
    if f + 1 < len(plan):
        plan[f + 1] = START


def chain_runs():
    """260 frames whose CHAINED runs cross every edge of the chain's 64-frame chunks, with the numeric sequences between LOST frames
    inside the chunks.  Returns (batch, plan: the status of every frame, notes: {name: frame})."""
    rng, counts, M, poses, P, plan = _chain_base(41)
    notes = {}
    lost = itertools.cycle(NOT_OK + (5, 0x80000000, 0xFFFFFFFF))  # every status that is not OK, and values that are no status at all

    def sequence(first, prs, zs, positive=False):
        """Frames first (LOST), first + 1 (START) .. : pair first + k has pose prs[k] and depths zs[k]; LOST again behind them."""
        _lose(poses, plan, first, next(lost))
        for k, (q, z) in enumerate(zip(prs, zs)):
            poses[first + k], P[first + k] = q, _chain_points(z, rng, positive)
        _lose(poses, plan, first + len(prs) + 1, next(lost))

    # steps of 2e30 and 1.5e30: scale 1, 2e30, inf.  Pose entries and coordinates are positive and the composition's det is 0 (kept
    # as it is), so inf meets no 0 and no -inf
    half = pose(r=np.full(9, 0.5, F), t=(0.5, 0.5, 0.5))
    sequence(19, [half] * 3, [1.0, 1e-30, 1e-30], positive=True)
    notes["scale inf"] = 22
    # steps of 1e-20 under a pose whose third row is 0 (Yz = t2 = 1): scale 1, 1e-20, 1e-40 (subnormal), 0, 0
    flat = pose(r=[1, 0, 0, 0, 1, 0, 0, 0, 0], t=(0.1, 0.2, 1.0))
    sequence(30, [flat] * 5, [1.0, 1e20, 1e20, 1e20, 1e20])
    notes["scale 0"] = 34
    turn = pose(r=_STEP, t=(0.6, 0.0, 0.8))
    z0 = F(0.8) / (F(1) - _STEP[8])
    sequence(40, [turn, pose(r=np.zeros(9, F), t=(1, 1, 1)), turn], [z0, z0, 1.0 / z0])  # det 0: the zero matrix, and a pose composed with it
    notes["det 0"] = 42
    sequence(50, [turn, pose(r=[1, 0, 0, 0, 1, 0, 0, 0, -1], t=(0.1, 0, 0.9)), turn], [z0, z0, -z0])  # det < 0 (Yz < 0 over depths < 0), and a pose composed with it
    notes["det < 0"] = 52
    sequence(100, [turn, pose(r=np.full(9, 1e20, F) * _STEP, t=(1, 2, 3))], [z0, z0])  # cofactors overflow: det not finite
    notes["det not finite"] = 102
    return batch(counts, M, poses, P, CHAIN_CAP), plan, notes


def chain_edges():
    """260 frames with LOST, START, RESTART_FEW and RESTART_SPREAD each on a frame just before and just after an edge of the 64-frame
    chunks (64|65, 128|129, 192|193, 256|257), and CHAINED behind each RESTART.  Returns (batch, plan)."""
    rng, counts, M, poses, P, plan = _chain_base(42)
    _lose(poses, plan, 64, orb.ORB_POSE_AMBIGUOUS)     # LOST before, START after
    _lose(poses, plan, 127, orb.ORB_POSE_NOMODEL)      # START at 128, before
    _lose(poses, plan, 129, orb.ORB_POSE_LOW_PARALLAX)  # LOST after; START at 130
    for f, kind in ((192, "few"), (193, "spread"), (256, "spread"), (257, "few")):  # the joint behind frame f is frame f - 1's
        M[f - 2] = _chain_matches(kind, rng)
        plan[f] = FEW if kind == "few" else SPREAD
    return batch(counts, M, poses, P, CHAIN_CAP), plan


def long_chain(n=4096, k=8):
    """The 4096-frame chain of one small rotation at capacity 8 (k = 8 points): every step is 1 within a few ulp."""
    pts = points(k, z=F(0.8) / (F(1) - _STEP[8]))
    m = np.zeros(k, orb.MATCH_DTYPE)
    m["index"] = np.arange(k)
    return batch([k] * n, [m] * (n - 1), [pose(r=_STEP, t=(0.6, 0.0, 0.8))] * (n - 1), [pts] * (n - 1), k), _STEP


def stored_nans(b, frames, world):
    """Where a reference output holds a NaN that is no copy of an input: frame records other than START / RESTART (copies of the pair's
    pose) and map rows other than copied ones.  The cases keep this empty (see the module's docstring)."""
    bad = []
    for f in range(len(frames)):
        if np.isnan(frames[f]["r"]).any() or np.isnan(frames[f]["t"]).any() or np.isnan(frames[f]["scale"]) or np.isnan(frames[f]["step"]):
            if frames[f]["status"] not in (START, FEW, SPREAD):
                bad.append(("frame", f))
        if f + 1 < len(frames) and frames[f + 1]["origin"] != f and any(np.isnan(world[f][c]).any() for c in "xyz"):
            bad.append(("map", f))
    return bad


def steady_chain(n, seed=43):
    """n frames at capacity 64, every pair OK and every joint holding: (batch, plan)."""
    _, counts, M, poses, P, plan = _chain_base(seed, n)
    return batch(counts, M, poses, P, CHAIN_CAP), plan
