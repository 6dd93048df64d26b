"""Hand-built inputs of the localisation stage, for the CPU restatement and for the device (test infrastructure, not a test file).

orb_localize_consecutive reads the raw counters, the stored records, the matcher's records, the pose records
and the pairs' points.  The builders here make all of them directly, as plain arrays, from a cloud of landmarks seen along a
camera path (`views`), so that a test decides the number of correspondences of a pair to the unit (`trim`), the shape of the cloud
(general, a plane, a line, two points repeated), which matches fail which clause of LO-1, and where raw counters exceed the
capacity.  `join` lays several such runs of frames one after the other in one batch; `reference` runs the restatement on a batch's
arrays; `inject` writes a batch over a program's buffers (constructed.inject, trajectory_cases.inject_pose).
"""
import numpy as np

import constructed as C
import localize_ref as lr
import trajectory_ref as tr
from tinyslam_amd import orb

F = np.float32
U = np.uint32
NONE = orb.ORB_MATCH_NONE
GOOD, PAR = orb.ORB_POINT_GOOD, orb.ORB_POINT_PARALLAX


def intrinsics(W, H, focal):
    """Pinhole intrinsics in level-0 (pixel-centre) coordinates of a camera whose principal point is the image centre."""
    return dict(fx=focal, fy=focal, cx=(W - 1) / 2, cy=(H - 1) / 2)


def default_steps(n):
    """n camera steps (X_{k+1} = R X_k + t): a little yaw and pitch, sideways and slightly forward, lengths that change by up to 2."""
    lengths = [0.3, 0.5, 0.25, 0.4, 0.2, 0.35, 0.3, 0.45, 0.25, 0.4, 0.3]
    return [(tr.rot("y", 0.7) @ tr.rot("x", 0.3), np.array([-l, 0.1 * l, 0.3 * l])) for l in lengths[:n]]


def cloud(rng, n, W, H, focal, shape="general"):
    """n landmarks in camera 0's frame, at random pixels with inverse-uniform depths in [2, 12]; `shape`: 'general', 'plane' (a
    tilted plane), 'line', 'two' (two points, each repeated)."""
    x, y = rng.uniform(0.15 * W, 0.85 * W, n), rng.uniform(0.15 * H, 0.85 * H, n)
    z = 1.0 / rng.uniform(1.0 / 12.0, 1.0 / 2.0, n)
    X = np.stack([(x - W / 2) / focal * z, (y - H / 2) / focal * z, z], 1)
    if shape == "plane":
        X[:, 2] = 6.0 + 0.4 * X[:, 0] - 0.3 * X[:, 1]
    elif shape == "line":
        s = rng.uniform(-1, 1, n)
        X = np.array([0.1, -0.1, 6.0]) + s[:, None] * np.array([1.0, 0.4, 2.0])
    elif shape == "two":
        X = np.where((np.arange(n) % 2 == 0)[:, None], np.array([0.5, -0.2, 6.0]), np.array([-0.8, 0.3, 4.0]))
    return X


def views(rng, n_frames, n_land, cap, W=64, H=48, focal=60.0, shape="general", steps=None, wrong=0.0, far=0.0, close=0.0, lost=0.0,
          bad_points=0.0, noise=0.0, unique=True, extra=0):
    """n_frames views of one cloud as the stages before localisation would leave them.  Frame k stores the landmarks it sees (in
    front, inside the image, one per pixel when `unique`) in a random order of its own, at most `cap` of them; `extra` is added to
    every raw counter whose frame stores `cap` records.  matches[k][i]: the slot in frame k + 1 of the landmark at slot i (distance
    below 30, second above 100), or ORB_MATCH_NONE when it is not stored there; of the matches, a share `wrong` points at a random
    other slot, `far` have a distance above 64, `close` a second distance that fails the ratio, `lost` are ORB_MATCH_NONE.
    poses[k]: the true step with a unit baseline, status OK.  points[k][i]: the landmark in camera k's frame and pair k's unit, GOOD
    (and PARALLAX) when both frames store it, plus `noise` (relative, Gaussian); a share `bad_points` loses its flags.
    Returns dict(counts, corners, matches (n - 1, cap), poses (n - 1,), points (n - 1, cap), cap, n, W, H, focal, steps, slots)."""
    steps = default_steps(n_frames - 1) if steps is None else steps
    X0 = cloud(rng, n_land, W, H, focal, shape)
    cams = [(np.eye(3), np.zeros(3))]
    for R, t in steps:
        Rk, tk = cams[-1]
        cams.append((R @ Rk, R @ tk + t))
    counts, corners, slots, Xc = np.zeros(n_frames, U), [], [], []
    for k in range(n_frames):
        Q = X0 @ cams[k][0].T + cams[k][1]
        with np.errstate(all="ignore"):
            u, v = focal * Q[:, 0] / Q[:, 2] + W / 2, focal * Q[:, 1] / Q[:, 2] + H / 2
        px, py = np.floor(u), np.floor(v)
        seen = (Q[:, 2] > 0) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
        if unique:
            taken = set()
            for l in np.nonzero(seen)[0]:
                if (px[l], py[l]) in taken:
                    seen[l] = False
                taken.add((px[l], py[l]))
        order = rng.permutation(np.nonzero(seen)[0])[:cap]
        slot = np.full(n_land, -1, np.int64)
        slot[order] = np.arange(len(order))
        counts[k] = len(order) + (extra if len(order) == cap else 0)
        corners.append(C.corners(px[order].astype(np.int64), py[order].astype(np.int64), 0, rng=rng))
        slots.append(slot)
        Xc.append(Q)
    M = np.zeros((n_frames - 1, cap), orb.MATCH_DTYPE)
    M["index"], M["distance"], M["second"] = NONE, 0xFFFF, 0xFFFF
    P = np.zeros((n_frames - 1, cap), orb.POINT_DTYPE)
    poses = np.zeros(n_frames - 1, orb.POSE_DTYPE)
    for k in range(n_frames - 1):
        R, t = steps[k]
        base = np.linalg.norm(t)
        poses[k]["r"], poses[k]["t"], poses[k]["status"] = R.ravel(), t / base, orb.ORB_POSE_OK
        here = np.nonzero(slots[k] >= 0)[0]
        i, j = slots[k][here], slots[k + 1][here]
        n = len(here)
        both = j >= 0
        idx = np.where(both, j, NONE).astype(np.int64)
        nxt = max(int(min(counts[k + 1], cap)), 1)
        idx = np.where(rng.random(n) < wrong, rng.integers(0, nxt, n), idx)
        idx = np.where(rng.random(n) < lost, NONE, idx)
        M["index"][k, i] = idx
        M["distance"][k, i] = np.where(rng.random(n) < far, rng.integers(65, 120, n), rng.integers(0, 30, n))
        M["second"][k, i] = np.where(rng.random(n) < close, M["distance"][k, i], rng.integers(100, 140, n))
        Xk = Xc[k][here] / base * (1.0 + noise * rng.standard_normal((n, 1)))
        P["x"][k, i], P["y"][k, i], P["z"][k, i] = Xk[:, 0], Xk[:, 1], Xk[:, 2]
        P["flags"][k, i] = np.where(both & ~(rng.random(n) < bad_points), GOOD | PAR, 0)
    return dict(counts=counts, corners=corners, matches=M, poses=poses, points=P, cap=cap, n=n_frames, W=W, H=H, focal=focal, steps=steps,
                slots=slots)


def stored(b):
    return np.minimum(b["counts"], b["cap"]).astype(np.int64)


def candidates(b, f, **params):
    """The slots of frame f - 1 that are pair f's correspondences (LO-1), ascending."""
    nq = stored(b)
    p = lr.defaults(**{**intrinsics(b["W"], b["H"], b["focal"]), **params})
    return lr.correspondences(nq[f - 1], nq[f], nq[f + 1], b["matches"][f - 1], b["matches"][f], b["poses"][f - 1], b["points"][f - 1],
                              b["corners"][f + 1][:nq[f + 1]], p)[0]


def trim(b, f, M, rng=None):
    """Leaves pair f exactly M correspondences: the flags of the points behind the others (random ones with `rng`, else the last) are
    cleared.  Fails when the pair has fewer."""
    sel = candidates(b, f)
    assert len(sel) >= M, (len(sel), M)
    drop = sel[M:] if rng is None else rng.choice(sel, len(sel) - M, replace=False)
    b["points"]["flags"][f - 1, drop] = 0
    assert len(candidates(b, f)) == M
    return b


def join(runs, bridge=False):
    """Several runs of frames, one after the other, in one batch.  The pair between two runs gets a pose that is not OK (every other
    status in turn, a record of arbitrary bits), points without flags and no matches: its own fix is FEW (no second hop) and the fix
    behind it NOMAP.  With `bridge`, the pair between two runs has matches, as the matcher pairs the keypoints of unrelated scenes:
    random stored keypoints of the next run's first frame at distances that pass, so its fix is a RANSAC over unrelated points."""
    cap = runs[0]["cap"]
    assert all(r["cap"] == cap and (r["W"], r["H"], r["focal"]) == (runs[0]["W"], runs[0]["H"], runs[0]["focal"]) for r in runs)
    rng = np.random.default_rng(len(runs))
    counts, corners, matches, poses, points = [], [], [], [], []
    for c, r in enumerate(runs):
        if c:
            m = np.zeros((1, cap), orb.MATCH_DTYPE)
            m["index"], m["distance"], m["second"] = NONE, 0xFFFF, 0xFFFF
            n_here, n_next = int(min(runs[c - 1]["counts"][-1], cap)), int(min(r["counts"][0], cap))
            if bridge and n_here and n_next:
                m["index"][0, :n_here] = rng.integers(0, n_next, n_here)
                m["distance"][0, :n_here], m["second"][0, :n_here] = rng.integers(0, 30, n_here), rng.integers(100, 140, n_here)
            q = rng.integers(0, 1 << 32, 16, dtype=U).view(orb.POSE_DTYPE)
            q["status"] = (orb.ORB_POSE_NOMODEL, orb.ORB_POSE_FEW, orb.ORB_POSE_AMBIGUOUS, orb.ORB_POSE_LOW_PARALLAX)[c % 4]
            matches.append(m)
            poses.append(q)
            points.append(np.zeros((1, cap), orb.POINT_DTYPE))
        counts.append(r["counts"])
        corners += r["corners"]
        matches.append(r["matches"])
        poses.append(r["poses"])
        points.append(r["points"])
    out = dict(runs[0])
    out.update(counts=np.concatenate(counts), corners=corners, matches=np.concatenate(matches), poses=np.concatenate(poses),
               points=np.concatenate(points), n=sum(r["n"] for r in runs), first=np.cumsum([0] + [r["n"] for r in runs])[:-1])
    return out


def reference(b, n_frames=None, **params):
    """localize_ref.localize on a batch's arrays (the counts clipped to the capacity).  Returns (FIX_DTYPE (n - 1,), uint8 (n - 1, cap))."""
    n = b["n"] if n_frames is None else n_frames
    nq = stored(b)
    return lr.localize(nq[:n], [c[:nq[f]] for f, c in enumerate(b["corners"][:n])], [b["matches"][f][:nq[f]] for f in range(n - 1)],
                       list(b["poses"][:n - 1]), list(b["points"][:n - 1]), b["cap"], **{**intrinsics(b["W"], b["H"], b["focal"]), **params})


def inject(prog, b):
    """A program whose match and pose stages are fresh on a batch of b['n'] frames (trajectory_cases.prepare: empty frames through
    match -> verify_epipolar -> pose), then the batch's records, counters, matches, pose records and points over its buffers."""
    import trajectory_cases as tc
    tc.prepare(prog, b["n"], b["W"], b["H"])
    C.inject(prog, b["counts"], [c[:b["cap"]] for c in b["corners"]])
    tc.inject_pose(prog, b["matches"], b["poses"], b["points"])
