"""Hand-built inputs of the join stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_join_pairs reads the trajectory's frame records, the landmark records, the matcher's consecutive records
(the owners' walk), the list and rows of orb_match_pairs, the fixes and inlier bytes of orb_loop_pairs and the raw counters.
`rail` is landmark_cases.rail under a plan with several segments, each segment's translations scaled by a power of two so that the
segments have different units and every ratio is exact; `fix` is the true OrbLoopFix of a rail entry, `row` its true row, `mask` its
inlier bytes.  `lost_batch` is the CPU probe's batch: loop_cases.out_and_back with pair 4 not OK.  The `load*`, `inputs`,
`inject_masks` and `check` helpers drive a device program.
"""
import collections

import numpy as np

import constructed as C
import graph_cases as G
import join_ref as jr
import landmark_cases as L
import localize_cases as lc
import loop_cases as K
import loop_ref as lpr
import trajectory_cases as tc
from tinyslam_amd import orb

F = np.float32
NONE = 0xFFFFFFFF
OK, MINIMAL, FEW_FIX = orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_MINIMAL, orb.ORB_LOCALIZE_FEW
TWO = [L.ORIGIN, L.START, L.CHAINED, L.LOST, L.START, L.CHAINED]   # segments 0 (frames 0-2) and 3 (frames 3-5)
THREE = [L.ORIGIN, L.START, L.LOST, L.START, L.LOST, L.START]      # segments 0, 2 and 4, two frames each
RESTART = [L.ORIGIN, L.START, L.CHAINED, L.FEW, L.CHAINED, L.CHAINED]  # frame 2 is CHAINED in segment 0 and the origin of segment 2


def scaled_frames(plan, scales=None):
    """landmark_cases.frame_records with the translations of segment o multiplied by scales[o] (a power of two): its unit is
    1 / scales[o] of the rail's."""
    fr = L.frame_records(plan)
    for o, k in (scales or {}).items():
        sel = (fr["origin"] == o) & (np.arange(len(fr)) != o)
        fr["t"][sel] *= F(k)
    return fr


def rail(plan=TWO, K_=12, cap=16, scales=None, seed=0):
    """(batch, landmark records) of the rail camera under `plan`: the landmarks are landmark_ref's under the scaled frame records,
    so segment o's landmarks are scales[o] times the rail's."""
    b = L.rail(len(plan), K_, cap=cap, plan=plan, v_hi=L.V_HI, seed=seed)
    b["frames"] = scaled_frames(plan, scales)
    b["scales"] = dict(scales or {})
    lms, _ = L.run(b)
    return b, [lm.copy() for lm in lms]


def row(b, q, T, distance=10, second=100):
    """The true row of the entry (q, T): landmark l's slot in q points at its slot in T."""
    r = np.zeros(b["cap"], orb.MATCH_DTYPE)
    r["index"], r["distance"], r["second"] = orb.ORB_MATCH_NONE, 0xFFFF, 0xFFFF
    r["index"][b["slots"][q]], r["distance"][b["slots"][q]], r["second"][b["slots"][q]] = b["slots"][T], distance, second
    return r


def fix(b, q, T, inliers=50, status=OK, frames=None):
    """The true OrbLoopFix of the rail entry (q, T): camera q in the frame and unit of T's segment."""
    fr = b["frames"] if frames is None else frames
    o = int(fr["origin"][T])
    k = b["scales"].get(o, 1)
    rec = G.fix(np.eye(3), (-L.RAIL_BASE * k * (q - T), 0, 0), o, int(fr["origin"][q]) if q < len(fr) else NONE, inliers=inliers, status=status)
    rec["pose_r"], rec["pose_t"] = tc.IDENTITY, (-L.RAIL_BASE * k * (q - o), 0, 0)
    return rec


def fixes(b, pairs, **kw):
    return np.array([fix(b, q, T, **kw) for q, T in pairs], orb.LOOP_FIX_DTYPE)


def mask(b, q, lands=None):
    """Inlier bytes of frame q: 1 at the slots of the landmarks `lands` (default: all)."""
    m = np.zeros(b["cap"], np.uint8)
    s = b["slots"][q]
    m[s if lands is None else s[np.asarray(lands, np.int64)]] = 1
    return m


def run(b, lms, pairs, rows=None, fx=None, masks=None, frames=None, n=None, trace=None, counts=None, **params):
    """join_ref.join_pairs on a rail batch; rows, fixes and masks default to the true ones of every entry."""
    nq = lc.stored(b) if counts is None else counts
    n = b["n"] if n is None else n
    rows = [row(b, q, T) for q, T in pairs] if rows is None else rows
    fx = fixes(b, pairs, frames=frames) if fx is None else fx
    masks = [mask(b, q) for q, T in pairs] if masks is None else masks
    return jr.join_pairs(nq, [b["matches"][f] for f in range(n - 1)], rows, pairs, b["frames"] if frames is None else frames, lms[:n - 1], fx, masks,
                         b["cap"], L=n, trace=trace, **params)


def lost_batch(seed, cap=128):
    """The out-and-back path with the pose of pair 4 not OK: frames 0-4 are segment 0, frame 5 is LOST and the origin of frames
    6-10.  The cloud's unit is the same everywhere; segment 0's unit is the step of pair 0, segment 5's that of pair 5."""
    b = K.out_and_back(seed, cap=cap)
    b["poses"]["status"][4] = orb.ORB_POSE_LOW_PARALLAX
    return b


def true_gamma(b, o, s):
    """Units of segment o per unit of segment s: a unit is the baseline of the segment's first pair."""
    return float(np.linalg.norm(b["steps"][s][1]) / np.linalg.norm(b["steps"][o][1]))


# ---- the device -------------------------------------------------------------------------------------------------------------
W0, H0, FOCAL = 64, 48, 60.0
THR = 20.0 / 255.0
INTR = lc.intrinsics(W0, H0, FOCAL)
Inputs = collections.namedtuple("Inputs", "nq corners matches frames lms L cap intr")


def program(tinyorb, cap, max_batch, flags=0):
    cfg = tinyorb.OrbConfig(tinyorb.Extent3d(W0, H0), max_features=cap, hierarchy_depth=2, initial_threshold=THR, max_batch=max_batch, flags=flags)
    return tinyorb.OrbProgram(cfg).init()


def inputs(prog, n_frames, L_frames, cap, intr):
    """What the loop and join calls read besides the rows, the fixes and the inlier bytes, as the device holds it."""
    nq = np.minimum(prog.batch_counts(n_frames), cap).astype(np.int64)
    corners = [prog.batch_read(f, int(nq[f]))[0] for f in range(n_frames)]
    matches = [prog.match_read(f, int(nq[f])) for f in range(L_frames - 1)]
    frames = np.array([prog.trajectory_read(f, 0)[0] for f in range(n_frames)])
    lms = [prog.landmarks_read(p, cap)[1] for p in range(L_frames - 1)]
    return Inputs(nq, corners, matches, frames, lms, L_frames, cap, intr)


def load(prog, b, desc, traj=None, lm=None, L_frames=None):
    """A views batch over the program's buffers with its descriptors, then the trajectory and landmarks calls on the device."""
    lc.inject(prog, b)
    C.inject(prog, b["counts"], None, desc)
    prog.trajectory_consecutive(b["n"], **(traj or {}))
    Lf = b["n"] if L_frames is None else L_frames
    prog.landmarks_consecutive(Lf, **INTR, **(lm or {}))
    return inputs(prog, b["n"], Lf, b["cap"], INTR)


def load_rail(prog, b, desc, frames=None):
    """A rail batch (no pose records; its frame records are written over the trajectory call's), then the landmarks call."""
    n = b["n"]
    tc.prepare(prog, n, W0, H0)
    C.inject(prog, b["counts"], b["corners"], desc)
    tc.inject_pose(prog, matches=b["matches"], points_=b["points"])
    prog.trajectory_consecutive(n)
    L.inject_frames(prog, b["frames"] if frames is None else frames)
    prog.landmarks_consecutive(n, **L.RAIL)
    return inputs(prog, n, n, b["cap"], L.RAIL)


def inject_masks(prog, masks, first=0):
    """Overwrites the inlier bytes of entries first .. of the last loop call (orb_debug_loop_mask_buffer) with rows of `cap`
    bytes.  Ordered as graph_cases.inject_fixes.  No stage's freshness changes."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    P, cap = orb.ORB_PAIRS_PER_FRAME * cfg.max_batch, cfg.max_features
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    a = np.ascontiguousarray(masks, dtype=np.uint8)
    n = len(a)
    assert a.ndim == 2 and a.shape[1] == cap and first + n <= P, (a.shape, first, P, cap)
    node.as_tensor(prog.debug_loop_mask_buffer(), (P, cap), "|u1", dev)[first:first + n].copy_(torch.from_numpy(a))
    torch.cuda.synchronize(dev)


def loop_state(prog, n, cap):
    """The fixes and inlier bytes of entries 0 .. n - 1 as the device holds them."""
    recs = [prog.loop_pairs_read(i, cap) for i in range(n)]
    return np.array([r for r, _ in recs]), np.array([m for _, m in recs])


def hold(prog, inp, pairs, n):
    """The rows, fixes and inlier bytes of entries 0 .. n - 1 as the device holds them now."""
    rows = [prog.match_pairs_read(i, int(inp.nq[q]) if q < len(inp.nq) else 0) for i, (q, T) in enumerate(pairs[:n])]
    return (rows,) + loop_state(prog, n, inp.cap)


def check(prog, inp, pairs, n_pairs=None, stream=None, call=True, held=None, **params):
    """join_pairs (call=False: the last one's results), then all three outputs against the restatement fed with what the device
    holds (`held`: what it held when the call was made), byte for byte.  Returns (poses, segments, links, the bytes of all three)."""
    n = len(pairs) if n_pairs is None else n_pairs
    nF = len(inp.frames)
    rows, fx, masks = hold(prog, inp, pairs, n) if held is None else held
    if call:
        prog.join_pairs(n, stream=stream, **params)
    want = jr.join_pairs(inp.nq, inp.matches, rows, pairs, inp.frames, inp.lms, fx, masks, inp.cap, L=inp.L, n_pairs=n, **params)
    poses = np.array([prog.join_read(f) for f in range(nF)])
    segs, links = prog.join_segments(nF), prog.join_links(n)
    for name, got, exp in (("links", links, want[2]), ("segments", segs, want[1]), ("poses", poses, want[0])):
        for k in range(len(exp)):
            assert got[k].tobytes() == exp[k].tobytes(), (name, k, params, got[k], exp[k])
    return poses, segs, links, poses.tobytes() + segs.tobytes() + links.tobytes()


# 2 x the float64 yardstick's worst over seeds 0-3 (tests/test_join_ref.py measures them and checks these figures): gamma relative to
# the true unit ratio, rotation in degrees, position in units of segment 0
BOUNDS = (2 * 0.0037798, 2 * 0.094150, 2 * 0.043264)
