"""Hand-built inputs of the graph stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_graph_pairs reads the trajectory's frame records, the list of orb_match_pairs and the fixes of
orb_loop_pairs, and nothing else: a case is a set of frame records, a list and a set of fix records.  `circle` and `line` give true
camera paths, `drifted` chains their steps again with a constant rotation bias and a scale on every step's translation, as a
trajectory with drift would, `fix` measures a pair of true cameras.  `inject_fixes` writes fix records over the loop stage's on the
device.
"""
import numpy as np

from tinyslam_amd import orb

F = np.float32
OK, MINIMAL, FEW_FIX = orb.ORB_LOCALIZE_OK, orb.ORB_LOCALIZE_MINIMAL, orb.ORB_LOCALIZE_FEW
CHAINED, START, LOST, ORIGIN, RESTART = orb.ORB_TRAJ_CHAINED, orb.ORB_TRAJ_START, orb.ORB_TRAJ_LOST, orb.ORB_TRAJ_ORIGIN, orb.ORB_TRAJ_RESTART_FEW
NONE = 0xFFFFFFFF


def rot(axis, angle):
    """Rodrigues: the rotation by `angle` radians about `axis` (float64)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def circle(n, radius=None):
    """n cameras on a circle in the x-z plane, one unit of arc apart, each turned along the tangent: [(R, t)] with
    X_k = R X_0 + t, camera 0 the identity."""
    radius = n / (2 * np.pi) if radius is None else radius
    cams = []
    for k in range(n):
        a = k / radius
        Rw = rot([0, 1, 0], a)                                     # camera-to-world
        c = np.array([radius * np.sin(a), 0.0, radius * (1 - np.cos(a))])  # centre in camera 0's frame
        cams.append((Rw.T, -Rw.T @ c))
    return cams


def line(n, step=(1.0, 0.0, 0.0), turn=0.01):
    """n cameras a step apart, each turned a little about y."""
    cams = [(np.eye(3), np.zeros(3))]
    S = rot([0, 1, 0], turn)
    for _ in range(n - 1):
        R, t = cams[-1]
        cams.append((S @ R, S @ t + np.asarray(step, np.float64)))
    return cams


def steps_of(cams):
    """The chain steps of a path: [(R, t)] with X_{k+1} = R X_k + t."""
    return [(Rb @ Ra.T, tb - Rb @ Ra.T @ ta) for (Ra, ta), (Rb, tb) in zip(cams[:-1], cams[1:])]


def drifted(cams, bias=0.004, scale=1.01, axis=(0.3, 1.0, 0.2)):
    """The path chained again with every step's rotation multiplied by a constant rotation of `bias` radians and its translation
    scaled."""
    B = rot(axis, bias)
    out = [cams[0]]
    for R, t in steps_of(cams):
        Rp, tp = out[-1]
        Rs = B @ R
        out.append((Rs @ Rp, Rs @ tp + scale * t))
    return out


def relative(cams, q, T):
    (Rq, tq), (RT, tT) = cams[q], cams[T]
    R = Rq @ RT.T
    return R, tq - R @ tT


def frames_of(cams, origin=0, first=0, status=None):
    """FRAME_POSE_DTYPE records of a path that is one segment: frame `first` + k holds cams[k]; cams[0] is the origin's (ORIGIN for
    frame 0, LOST otherwise: its own origin), the second START, the others CHAINED."""
    n = len(cams)
    fr = np.zeros(n, orb.FRAME_POSE_DTYPE)
    for k, (R, t) in enumerate(cams):
        fr[k]["r"], fr[k]["t"] = np.asarray(R, np.float64).reshape(9), t
        fr[k]["scale"], fr[k]["step"], fr[k]["origin"] = 1, 1, origin
        fr[k]["status"] = CHAINED if k > 1 else START
    fr[0]["status"], fr[0]["origin"] = (ORIGIN if first == 0 else LOST), first
    fr[0]["scale"] = fr[0]["step"] = 0
    if status is not None:
        fr["status"] = status
    return fr


def fix(R, t, origin, query_origin=None, inliers=50, status=OK):
    """A LOOP_FIX_DTYPE record: camera q relative to camera T is (R, t)."""
    rec = np.zeros((), orb.LOOP_FIX_DTYPE)
    rec["r"], rec["t"] = np.asarray(R, np.float64).reshape(9), t
    rec["step"] = np.linalg.norm(t)
    rec["origin"], rec["query_origin"] = origin, origin if query_origin is None else query_origin
    rec["candidates"], rec["inliers"], rec["status"] = inliers + 3, inliers, status
    return rec


def fixes_of(cams, pairs, origin=0, first=0, **kw):
    """The true fixes of the listed pairs (frame numbers; cams[k] is frame first + k)."""
    return np.array([fix(*relative(cams, q - first, T - first), origin, **kw) for q, T in pairs], orb.LOOP_FIX_DTYPE)


def positions(r, t):
    """Camera centres -R^T t of (n, 9), (n, 3) poses, float64."""
    R = np.asarray(r, np.float64).reshape(-1, 3, 3)
    return -np.einsum("nji,nj->ni", R, np.asarray(t, np.float64))


def worst_position_error(r, t, cams):
    true = positions(np.array([R.reshape(9) for R, _ in cams]), np.array([t_ for _, t_ in cams]))
    return float(np.linalg.norm(positions(r, t) - true, axis=1).max())


def two_segments():
    """Twelve frames: segment 0 holds frames 0 .. 6; frame 6 is CHAINED there and the origin of the segment that a RESTART begins at
    frame 7 (frames 7 .. 9); frame 10 is LOST, frame 11 starts segment 10.  Returns (true cameras of each segment, records)."""
    a, b = line(7), line(4, step=(0.0, 0.0, 1.0))
    fr = np.concatenate([frames_of(drifted(a)), frames_of(drifted(b), origin=6, first=6)[1:], frames_of(line(2), origin=10, first=10)])
    fr[7]["status"] = RESTART
    assert fr["origin"].tolist() == [0] * 7 + [6] * 3 + [10, 10] and fr["status"][10] == LOST
    return a, b, fr


def verdict_cases(a, nF):
    """((q, T), fix, verdict) of every clause of PG-4 at its boundary, on two_segments' records (a: segment 0's true cameras)."""
    I3, z = np.eye(3), np.zeros(3)
    nan_fix = fix(I3, z, 0)
    nan_fix["t"][1] = np.nan
    cases = [
        ((5, 0), fix(*relative(a, 5, 0), 0), orb.ORB_GRAPH_EDGE_USED),
        ((5, 0), fix(I3, z, 0, status=FEW_FIX), orb.ORB_GRAPH_EDGE_STATUS),
        ((5, 0), fix(I3, z, 0, status=MINIMAL), orb.ORB_GRAPH_EDGE_STATUS),
        ((5, 0), fix(I3, z, 0, inliers=11), orb.ORB_GRAPH_EDGE_FEW),
        ((5, 0), fix(I3, z, 0, inliers=12), orb.ORB_GRAPH_EDGE_USED),
        ((nF - 1, 10), fix(I3, z, 10), orb.ORB_GRAPH_EDGE_USED),                   # q = F - 1
        ((nF, 10), fix(I3, z, 10, query_origin=NONE), orb.ORB_GRAPH_EDGE_RANGE),  # q = F: loop_pairs gives it no origin
        ((nF, 10), fix(I3, z, 10), orb.ORB_GRAPH_EDGE_RANGE),
        ((10, nF), fix(I3, z, 10), orb.ORB_GRAPH_EDGE_RANGE),
        ((5, 1), fix(I3, z, 0, query_origin=NONE), orb.ORB_GRAPH_EDGE_RANGE),
        ((8, 5), fix(I3, z, 0, query_origin=6), orb.ORB_GRAPH_EDGE_SEGMENT),       # origins differ
        ((8, 7), fix(I3, z, 6), orb.ORB_GRAPH_EDGE_USED),                          # origins equal
        ((6, 2), fix(I3, z, 0), orb.ORB_GRAPH_EDGE_USED),                          # the frame that ends segment 0: a free node there ...
        ((8, 6), fix(I3, z, 6), orb.ORB_GRAPH_EDGE_USED),                          # ... and the held origin of segment 6
        ((6, 8), fix(I3, z, 6), orb.ORB_GRAPH_EDGE_USED),                          # q = o
        ((7, 2), fix(I3, z, 0), orb.ORB_GRAPH_EDGE_SEGMENT),                       # q is no node of the segment the fix names
        ((2, 7), fix(I3, z, 6), orb.ORB_GRAPH_EDGE_SEGMENT),
        ((0, 4), fix(I3, z, 0), orb.ORB_GRAPH_EDGE_USED),                          # q = o, T free
        ((4, 0), fix(I3, z, 0), orb.ORB_GRAPH_EDGE_USED),                          # T = o
        ((3, 10), fix(I3, z, 0), orb.ORB_GRAPH_EDGE_SEGMENT),                      # a LOST frame is a node of its own segment only
        ((5, 0), nan_fix, orb.ORB_GRAPH_EDGE_NONFINITE),
        ((5, 0), fix(I3, z, 0, inliers=11, status=FEW_FIX), orb.ORB_GRAPH_EDGE_STATUS),  # the first that applies
    ]
    return cases


def segments_batch(sizes, total=0.3, scale=1.01):
    """One segment per entry of `sizes`, laid end to end: a circle of n + 1 cameras with n free nodes whose chain has gathered
    `total` radians of drift, closed by a loop from its last camera to its origin and, from three free nodes on, one from its
    middle to its second camera.  The first origin is frame 0, the others LOST frames.  Returns (frame records, list, fixes)."""
    frames, pairs, fixes, o = [], [], [], 0
    for n in sizes:
        true = circle(n + 1)
        frames.append(frames_of(drifted(true, bias=total / n, scale=scale), origin=o, first=o))
        mine = [(o + n, o)] + ([(o + n // 2, o + 1)] if n >= 3 else [])
        pairs += mine
        fixes.append(fixes_of(true, mine, origin=o, first=o))
        o += n + 1
    return np.concatenate(frames), pairs, np.concatenate(fixes)


STALL_PAIRS = [(63, 0), (32, 1)]


def stall_case(n=64, total=2.0):
    """PG-7's undo: a circle whose chain has gathered `total` radians of rotation drift about the circle's own axis, closed by two
    loops.  Under the default parameters the first undamped round lowers the cost and the second raises it.  Returns (frame
    records, list, fixes)."""
    true = circle(n)
    cams = drifted(true, bias=total / n, scale=1.0, axis=(0.0, 1.0, 0.0))
    return frames_of(cams), list(STALL_PAIRS), fixes_of(true, STALL_PAIRS)


def inject_fixes(prog, fixes, first=0):
    """Overwrites the fix records first .. of the last loop call (orb_debug_loop_buffer) with LOOP_FIX_DTYPE rows: what
    orb_loop_pairs_read and the graph stage read.  Ordered as landmark_cases.inject_frames: everything queued is finished before
    the copy starts, and the copy before this returns.  No stage's freshness changes."""
    import torch
    from tinyslam_amd import node
    cfg = prog.config
    P = orb.ORB_PAIRS_PER_FRAME * cfg.max_batch
    dev = torch.device("cuda", cfg.device)
    prog.batch_sync()
    torch.cuda.synchronize(dev)
    a = np.ascontiguousarray(fixes, dtype=orb.LOOP_FIX_DTYPE)
    n = len(a)
    assert a.ndim == 1 and first + n <= P, (a.shape, first, P)
    node.as_tensor(prog.debug_loop_buffer(), (P, 32), "<i4", dev)[first:first + n].copy_(torch.from_numpy(a.view(np.int32).reshape(n, 32)))
    torch.cuda.synchronize(dev)
