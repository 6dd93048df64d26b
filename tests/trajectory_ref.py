"""CPU restatement of the trajectory stage, TJ-1..TJ-7 of DESIGN.md section 20, in NumPy (test infrastructure, not a test file).

Every intermediate is np.float32 and every binary32 operation is the one the kernels in tinyslam_amd/csrc/orb_kernels_traj.h
perform, in the same order: the OrbFramePose and OrbPoint bytes of orb_trajectory_consecutive must equal what this module returns,
bit for bit.  The ratios of a joint and the map are vectorised; the chain runs on scalars, as one lane runs it.  path_scene builds
several views of one point cloud along a camera path, with the true poses, for the accuracy tests and the GPU parity batches.
"""
import numpy as np

import pose_ref as pr
from tinyslam_amd.orb import (FRAME_POSE_DTYPE, ORB_POINT_GOOD, ORB_POINT_PARALLAX, ORB_POSE_OK, ORB_TRAJ_CHAINED, ORB_TRAJ_LOST,
                              ORB_TRAJ_NEED_PARALLAX, ORB_TRAJ_ORIGIN, ORB_TRAJ_RESTART_FEW, ORB_TRAJ_RESTART_SPREAD, ORB_TRAJ_START,
                              POINT_DTYPE)

F = np.float32
HOLDS, FEW, SPREAD = 0, 1, 2  # TJ-4
_IDENTITY = [F(1), F(0), F(0), F(0), F(1), F(0), F(0), F(0), F(1)]


def defaults(min_shared=0, scale_tolerance=0.0, consistent_permille=0, flags=0):
    """OrbTrajectoryParams with its zero fields replaced by the defaults."""
    return dict(min_shared=min_shared or 8, scale_tolerance=F(scale_tolerance) if scale_tolerance else F(0.1),
                consistent_permille=consistent_permille or 500, flags=flags)


def ratios(nq_prev, nq, matches_prev, pose_prev, points_prev, points, need_parallax=False):
    """TJ-2: the depth ratios of the joint between pair f - 1 (its stored queries' matches, its pose record, its points) and pair f
    (its points), in query order."""
    i = slice(0, int(nq_prev))
    fl = points_prev["flags"][i]
    j = matches_prev["index"][i].astype(np.int64)
    ok = ((fl & ORB_POINT_GOOD) != 0) & (j < int(nq))
    jj = np.where(ok, j, 0)
    fl2 = points["flags"][jj]
    ok &= (fl2 & ORB_POINT_GOOD) != 0
    if need_parallax:
        ok &= ((fl & ORB_POINT_PARALLAX) != 0) & ((fl2 & ORB_POINT_PARALLAX) != 0)
    r, t = pose_prev["r"].astype(F), pose_prev["t"].astype(F)
    with np.errstate(all="ignore"):
        yz = ((r[6] * points_prev["x"][i] + r[7] * points_prev["y"][i]) + r[8] * points_prev["z"][i]) + t[2]
        rho = (yz / points["z"][jj]).astype(F)
        ok &= np.isfinite(rho) & (rho > F(0))
    return rho[ok]


def joint(rho, p):
    """TJ-3, TJ-4: (m, g, consistent, verdict) of a joint's ratios."""
    m = len(rho)
    g, consistent = F(0), 0
    if m:
        g = np.sort(rho.view(np.uint32))[(m - 1) // 2:(m - 1) // 2 + 1].view(F)[0]  # positive binary32 order as their bits
        tg = p["scale_tolerance"] * g
        with np.errstate(all="ignore"):
            consistent = int((np.abs(rho - g) <= tg).sum())
    if m < p["min_shared"]:
        return m, g, consistent, FEW
    if 1000 * consistent < p["consistent_permille"] * m:
        return m, g, consistent, SPREAD
    return m, g, consistent, HOLDS


def polar_step(r):
    """One step of RP-4 (pose_ref.polar's arithmetic); r itself when the det is not finite or not > 0."""
    with np.errstate(all="ignore"):
        c = pr._cof(r)
        det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2]
        if not (np.isfinite(det) and det > F(0)):
            return r
        return [F(0.5) * (r[k] + c[k] / det) for k in range(9)]


def compose(pr_, pt, r1, t1, scale):
    """TJ-5: (P.r R', one polar step; P.r t' + scale P.t) on lists of np.float32."""
    with np.errstate(all="ignore"):
        m = [(pr_[3 * r] * r1[c] + pr_[3 * r + 1] * r1[3 + c]) + pr_[3 * r + 2] * r1[6 + c] for r in range(3) for c in range(3)]
        t = [((pr_[3 * r] * t1[0] + pr_[3 * r + 1] * t1[1]) + pr_[3 * r + 2] * t1[2]) + scale * pt[r] for r in range(3)]
        return polar_step(m), t


def trajectory(counts, matches, poses, points, cap, **params):
    """TJ-1..TJ-7.  counts: the stored counts n_q of the n_frames frames; matches[p]: MATCH_DTYPE of pair p's stored queries;
    poses[p]: POSE_DTYPE record; points[p]: POINT_DTYPE (cap,) of pair p, for the n_frames - 1 pairs.
    Returns (FRAME_POSE_DTYPE (n_frames,), POINT_DTYPE (n_frames, cap))."""
    p = defaults(**params)
    n = len(poses) + 1
    assert len(counts) >= n and len(matches) >= n - 1 and len(points) >= n - 1
    need = bool(p["flags"] & ORB_TRAJ_NEED_PARALLAX)
    okp = [int(q["status"]) == ORB_POSE_OK for q in poses]
    out = np.zeros(n, dtype=FRAME_POSE_DTYPE)
    world = np.zeros((n, cap), dtype=POINT_DTYPE)
    R, t, scale, origin = list(_IDENTITY), [F(0)] * 3, F(0), 0
    out[0]["r"], out[0]["status"] = R, ORB_TRAJ_ORIGIN
    for f in range(1, n):
        P = poses[f - 1]
        Pr, Pt = [F(v) for v in P["r"]], [F(v) for v in P["t"]]
        step, shared, consistent = F(0), 0, 0
        if not okp[f - 1]:
            status, R, t, scale, origin = ORB_TRAJ_LOST, list(_IDENTITY), [F(0)] * 3, F(0), f
        elif f == 1 or not okp[f - 2]:
            status, R, t, scale, origin = ORB_TRAJ_START, Pr, Pt, F(1), f - 1
        else:
            rho = ratios(counts[f - 2], counts[f - 1], matches[f - 2], poses[f - 2], points[f - 2], points[f - 1], need)
            shared, g, consistent, verdict = joint(rho, p)
            if verdict == HOLDS:
                status, step = ORB_TRAJ_CHAINED, g
                with np.errstate(all="ignore"):
                    scale = scale * g
                R, t = compose(Pr, Pt, R, t, scale)
            else:
                status = ORB_TRAJ_RESTART_FEW if verdict == FEW else ORB_TRAJ_RESTART_SPREAD
                step = g if verdict == SPREAD else F(0)
                R, t, scale, origin = Pr, Pt, F(1), f - 1
        o = out[f]
        o["r"], o["t"], o["scale"], o["step"] = R, t, scale, step
        o["origin"], o["shared"], o["consistent"], o["status"] = origin, shared, consistent, status
    for f in range(n - 1):  # TJ-6
        nxt = out[f + 1]
        if nxt["status"] == ORB_TRAJ_LOST:
            continue
        src = points[f][:cap]
        if nxt["origin"] == f:
            world[f, :len(src)] = src
            continue
        good = (src["flags"] & ORB_POINT_GOOD) != 0
        s, Rf, tf = nxt["scale"], out[f]["r"], out[f]["t"]
        with np.errstate(all="ignore"):
            v = [s * src[k] - tf[c] for c, k in enumerate("xyz")]
            for c, k in enumerate("xyz"):
                w = (Rf[c] * v[0] + Rf[3 + c] * v[1]) + Rf[6 + c] * v[2]
                world[k][f, :len(src)] = np.where(good, w, F(0))
        world["flags"][f, :len(src)] = np.where(good, src["flags"], 0)
    return out, world


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    return {"x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]]), "y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]),
            "z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])}[axis]


def path_steps(name):
    """The two constructed paths (X_{k+1} = R X_k + t in metres): 'sideways' (half a degree of yaw per step, sideways steps of
    lengths 0.25, 0.5, 0.16, 0.3, 0.12) and 'forward' (a little yaw and pitch, mostly forward; 0.5, 0.25, 0.45, 0.2, 0.4).  The
    lengths of consecutive steps differ by factors between 0.3 and 2."""
    if name == "sideways":
        return [(rot("y", 0.5), np.array([-l, 0.02 * l, 0.05 * l])) for l in (0.25, 0.5, 0.16, 0.3, 0.12)]
    return [(rot("y", 0.6) @ rot("x", 0.3), np.array([0.3 * l, 0.1 * l, -l])) for l in (0.5, 0.25, 0.45, 0.2, 0.4)]


def path_scene(rng, steps, W=640, H=480, focal=500.0, n=900, outlier_share=0.2, zmin=2.0, zmax=12.0, count=None):
    """Views 0 .. len(steps) of ONE point cloud: n points at random pixels of frame 0 with inverse-uniform depths in [zmin, zmax],
    seen from a pinhole camera (focal length `focal`, principal point at the image centre) that moves by steps[k] = (R, t) from
    view k to view k + 1.  The landmarks that stay in front of and inside every view, one per pixel in each, become octave-0 records
    at the floors of their projections, with one descriptor per landmark, repeated in every frame.  outlier_share of a frame's
    records are outliers: a random descriptor, repeated in every frame too, at a random free pixel of each -- the matcher pairs
    them and the geometry does not.  With `count`, a random subset of that many records (landmarks and outliers) is kept.  Every
    frame is stored in a random order of its own.

    Returns dict(corners, desc: one per frame; ids: per frame, the landmark of every record (>= n_landmarks: an outlier);
    n_landmarks; cloud (n_landmarks, 3) in camera 0's frame; poses: the true (R_k, t_k) with X_k = R_k X_0 + t_k, float64)."""
    import constructed as C
    Ke = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1.0]])  # pixel-edge coordinates
    x, y = rng.uniform(0, W, n), rng.uniform(0, H, n)
    z = 1.0 / rng.uniform(1.0 / zmax, 1.0 / zmin, n)
    X0 = np.linalg.inv(Ke) @ np.stack([x, y, np.ones(n)]) * z
    poses = [(np.eye(3), np.zeros(3))]
    for R, t in steps:
        Rk, tk = poses[-1]
        poses.append((R @ Rk, R @ tk + t))
    V = len(poses)
    pix = np.zeros((V, n, 2), np.int64)
    ok = np.ones(n, bool)
    for k, (Rk, tk) in enumerate(poses):
        Q = Rk @ X0 + tk[:, None]
        q = Ke @ Q
        u, v = q[0] / q[2], q[1] / q[2]
        ok &= (Q[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        pix[k] = np.stack([np.floor(np.where(ok, u, 0)), np.floor(np.where(ok, v, 0))], 1)
    seen = [set() for _ in range(V)]
    keep = []
    for i in np.nonzero(ok)[0]:  # one record per pixel in every frame
        px = [tuple(pix[k, i]) for k in range(V)]
        if all(px[k] not in seen[k] for k in range(V)):
            for k in range(V):
                seen[k].add(px[k])
            keep.append(i)
    pix, cloud = pix[:, keep], X0[:, keep].T
    n_in = len(keep)
    n_out = int(round(outlier_share / (1.0 - outlier_share) * n_in))
    out = np.zeros((V, n_out, 2), np.int64)
    for k in range(V):
        for o in range(n_out):
            while True:
                c = (int(rng.integers(0, W)), int(rng.integers(0, H)))
                if c not in seen[k]:
                    break
            seen[k].add(c)
            out[k, o] = c
    pix = np.concatenate([pix, out], 1)
    ids = np.arange(n_in + n_out)
    if count is not None:
        ids = np.sort(rng.choice(n_in + n_out, size=count, replace=False))
    d = C.random_desc(rng, n_in + n_out)
    corners, desc, idl = [], [], []
    for k in range(V):
        order = ids[rng.permutation(len(ids))]
        corners.append(C.corners(pix[k, order, 0], pix[k, order, 1], 0, rng=rng))
        desc.append(d[order])
        idl.append(order)
    return dict(corners=corners, desc=desc, ids=idl, n_landmarks=n_in, cloud=cloud, poses=poses)
