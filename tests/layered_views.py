"""Two textured planes seen by a camera that moves sideways, and every stage behind extraction run on what extraction gives for
them (test infrastructure, not a test file; no GPU and no torch at import).

`views` draws the frames of tests/test_gpu_epipolar.py's two-layer scene with a step of its own per frame, `chain` runs the CPU
restatements match -> verify_epipolar -> pose -> trajectory -> localize -> landmarks -> bridge -> adjust in order, each on the
restatements' own earlier outputs, `device_chain` makes the same calls on a program and reads every stage back, and `differences`
names the first stage, pair or frame and slots where two such results differ.  `permuted` reorders the stored records of every
frame: the device stores a band's records in the order of its LDS atomics, the RANSACs draw by index, and what a test requires of a
chain has to hold under every order (tests/test_layered_chain_ref.py)."""
import numpy as np

import adjust_ref as ar
import bridge_ref as brr
import constructed as C
import epipolar_ref as er
import landmark_ref as lmr
import localize_ref as lr
import pose_ref as pr
import trajectory_ref as tr
from tinyslam_amd import orb

THR = 20.0 / 255.0
W0, H0 = 320, 240
INTR = dict(fx=300.0, fy=300.0, cx=159.5, cy=119.5)
INTR_OFF = dict(fx=300.0, fy=310.0, cx=158.0, cy=121.5)  # a principal point off the centre, fx != fy
SEED_FAR, SEED_NEAR = 4001, 4002
# (far, near) shift in px of x per step; at the fifth step the camera stands still: two equal frames, a pair that has no model in
# any order of the records.  (With near shifts of 12 px and a fifth step of (4, 4), 6 % of the orders lose a condition of
# check_roomy: NOTEBOOK.md, "The later stages on extracted views".)
STEPS = ((2, 24), (2, 24), (4, 48), (2, 24), (0, 0), (2, 24), (2, 24), (2, 24))
# the scene with an empty frame in it: every step has parallax, so only the empty frame cuts the path
STEPS_EMPTY, EMPTY = ((2, 24), (2, 24), (4, 48), (2, 24), (2, 24), (2, 24), (4, 48), (2, 24)), 4
GREY = 128

STAGES = ("match", "epipolar", "pose", "trajectory", "localize", "landmarks", "bridge", "adjust")
# what each stage leaves, in the order it is compared: (key, indexed by)
FIELDS = {"match": (("match", "frame"),), "epipolar": (("epipolar", "pair"), ("epipolar_mask", "pair")),
          "pose": (("pose", "pair"), ("points", "pair")), "trajectory": (("frames", "frame"), ("map", "frame")),
          "localize": (("fix", "pair"), ("fix_mask", "pair")), "landmarks": (("rows", "pair"), ("landmarks", "pair")),
          "bridge": (("bridge", "frame"), ("bridge_mask", "frame")), "adjust": (("adjusted", "frame"), ("refined", "frame"))}
EPIPOLAR = dict(inlier_px=2.0)


# ---- the scene ---------------------------------------------------------------------------------------------------------------
def views(oracle, steps=STEPS, W=W0, H=H0, flat=()):
    """len(steps) + 1 frames (n, H, W, 4) uint8 and the truth.  Rows < H / 2 show texture synth_frame(., ., 4001), the far plane,
    the other rows 4002, the near one; step i moves the far plane by steps[i][0] px of x and the near one by steps[i][1], both along
    (2, 1), so every shift is even and every crop starts at an integer offset.  Frames listed in `flat` are a constant grey.
    The truth: `r` the rotation of every step (identity), `direction` the unit translation of the camera frame (x2 = x1 + t: the
    picture moves against the crop offset), `ratio[i]` the length of step i + 1 over that of step i (the near layer's shifts),
    `parallax[i]` whether step i moves the layers differently between two textured frames."""
    steps = np.asarray(steps, np.int64).reshape(-1, 2)
    assert not (steps % 2).any() and (steps >= 0).all(), steps
    n = len(steps) + 1
    off = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(steps, 0)])  # x offsets of (far, near) per frame
    pad = 8 + max(12 * n, int(off.max()))  # 8 + 12 n: the textures of the tests this scene comes from, at their steps
    tex = [oracle.synth_frame(W + pad, H + pad, s) for s in (SEED_FAR, SEED_NEAR)]
    frames = np.empty((n, H, W, 4), np.uint8)
    for i in range(n):
        for layer, rows in ((0, slice(0, H // 2)), (1, slice(H // 2, H))):
            ox, oy = int(off[i, layer]), int(off[i, layer]) // 2
            frames[i, rows] = tex[layer][oy:oy + H, ox:ox + W][rows]
    for f in flat:
        frames[f] = GREY
        frames[f, ..., 3] = 255
    d = -np.array([2.0, 1.0, 0.0]) / np.sqrt(5.0)
    parallax = np.array([s[0] != s[1] and i not in flat and i + 1 not in flat for i, s in enumerate(steps)])
    with np.errstate(all="ignore"):  # a step of zero: no ratio, and no parallax either
        ratio = steps[1:, 1].astype(np.float64) / steps[:-1, 1]
    truth = dict(r=np.eye(3), direction=d, ratio=ratio, parallax=parallax)
    return frames, truth


def step_deviations(res, truth):
    """{pair: |step / true ratio - 1|} of the fixes that are OK with at least half of their candidates inliers, at the pairs where
    the ratio means something: pair p and the pair before it both show parallax between two textured frames."""
    par, out = truth["parallax"], {}
    for p in ok_fixes(res):
        if p >= 1 and par[p - 1] and par[p]:
            out[p] = abs(float(res["fix"][p]["step"]) / float(truth["ratio"][p - 1]) - 1.0)
    return out


def extract_ref(oracle, frames, cap):
    """The oracle's intended-mode extraction of every frame at capacity `cap`, records in its sorted order:
    (raw counters uint32 (n,), [records], [descriptors])."""
    counts, corners, desc = [], [], []
    for f in frames:
        r = oracle.extract_intended(f, depth=2, threshold=THR, arc=9, nms=True, max_features=cap)
        c, d = oracle.sort_keypoints(r["corners"], r["descriptors"])
        counts.append(r["total"])
        corners.append(c)
        desc.append(d)
    return np.array(counts, np.uint32), corners, desc


# the batches of tests/test_layered_chain_ref.py and tests/test_gpu_layered_chain.py: steps, capacity, grey frames
ROOMY = 1500  # above every counter of these views
FULL = 512    # below every counter of these views
SCENES = {"roomy": (STEPS, ROOMY, ()), "full": (STEPS, FULL, ()), "empty": (STEPS_EMPTY, ROOMY, (EMPTY,))}
_SCENE = {}


def scene(oracle, name):
    """dict(frames, truth, cap, batch: extract_ref at the scene's capacity, whole: extract_ref at ROOMY), made once."""
    if name not in _SCENE:
        steps, cap, flat = SCENES[name]
        frames, truth = views(oracle, steps, flat=flat)
        whole = extract_ref(oracle, frames, ROOMY)
        assert (whole[0] <= ROOMY).all()
        _SCENE[name] = dict(frames=frames, truth=truth, cap=cap, whole=whole, batch=whole if cap == ROOMY else extract_ref(oracle, frames, cap))
    return _SCENE[name]


def permuted(counts, corners, desc, rng):
    """The same batch with the stored records of every frame in a random order."""
    perm = [rng.permutation(len(c)) for c in corners]
    return counts, [c[p] for c, p in zip(corners, perm)], [d[p] for d, p in zip(desc, perm)]


# ---- the restatements, chained -----------------------------------------------------------------------------------------------
def chain(counts, corners, desc, W, H, cap, intr, n_frames=None, first="match", prior=None, **stage):
    """Every stage's records for the first n_frames frames (None: all), in the dtypes of the device's read-backs.  counts: the raw
    counters; corners[f], desc[f]: frame f's stored records, min(counts[f], cap) of them.  stage: per-stage parameter dicts by the
    names of STAGES (`epipolar` defaults to inlier_px 2).  `prior`: a result of this function on the same batch; the stages before
    `first` are taken from it (cut to n_frames) instead of being run again."""
    n = len(counts) if n_frames is None else n_frames
    nq = np.minimum(np.asarray(counts[:n], np.int64), cap)
    assert all(len(corners[f]) == nq[f] and len(desc[f]) == nq[f] for f in range(n))
    P = {s: dict(stage.get(s) or {}) for s in STAGES}
    assert not set(stage) - set(STAGES), stage
    if "epipolar" not in stage:
        P["epipolar"] = dict(EPIPOLAR)
    start = STAGES.index(first)
    out = dict(n=n, nq=nq)

    def run(s):
        if STAGES.index(s) >= start:
            return True
        for key, by in FIELDS[s]:
            v = prior[key]
            out[key] = v[:n if by == "frame" and s != "match" else n - 1]  # the last frame has no match records
        return False

    if run("match"):
        out["match"] = [C.match_ref(desc[f], desc[f + 1]) for f in range(n - 1)]
    m = out["match"]
    if run("epipolar"):
        res = [er.verify_pair(corners[f], corners[f + 1], m[f], W, H, f, cap=cap, **P["epipolar"]) for f in range(n - 1)]
        out["epipolar"], out["epipolar_mask"] = np.array([r[0] for r in res]), np.stack([r[1] for r in res])
    if run("pose"):
        res = [pr.pose_pair(corners[f], corners[f + 1], m[f], out["epipolar"][f], out["epipolar_mask"][f], cap=cap, **intr, **P["pose"])
               for f in range(n - 1)]
        out["pose"], out["points"] = np.array([r[0] for r in res]), np.stack([r[1] for r in res])
    pose, points = list(out["pose"]), list(out["points"])
    if run("trajectory"):
        out["frames"], out["map"] = tr.trajectory(nq, m, pose, points, cap, **P["trajectory"])
    if run("localize"):
        out["fix"], out["fix_mask"] = lr.localize(nq, corners, m, pose, points, cap, n_frames=n, **intr, **P["localize"])
    if run("landmarks"):
        out["landmarks"], out["rows"] = lmr.landmarks(nq, corners, m, points, out["frames"], cap, n_frames=n, **intr, **P["landmarks"])
    if run("bridge"):
        out["bridge"], out["bridge_mask"] = brr.bridge(nq, corners, m, points, out["frames"], list(out["landmarks"]), cap, n_frames=n,
                                                       **intr, **P["bridge"])
    if run("adjust"):
        poses, recs = ar.adjust(nq, corners, m, out["frames"], out["landmarks"], cap, n_frames=n, **intr, **P["adjust"])
        out["adjusted"] = poses
        out["refined"] = np.concatenate([recs, np.zeros((1, cap), orb.LANDMARK_DTYPE)])  # the last frame starts no pair: zeros
    return out


# ---- the device --------------------------------------------------------------------------------------------------------------
def device_records(prog, n, cap):
    """(raw counters, [stored records], [stored descriptors]) of the program's batch."""
    counts = prog.batch_counts(n)
    got = [prog.batch_read(f, int(min(counts[f], cap))) for f in range(n)]
    return counts, [g[0] for g in got], [g[1] for g in got]


def device_chain(prog, n, intr, first="match", **stage):
    """The calls of `chain` from `first` on, on the program's batch with n_frames = n, and every stage's read-back of the first n
    frames as `chain` returns them."""
    cap = prog.config.max_features
    P = {s: dict(stage.get(s) or {}) for s in STAGES}
    assert not set(stage) - set(STAGES), stage
    if "epipolar" not in stage:
        P["epipolar"] = dict(EPIPOLAR)
    calls = (("match", lambda: prog.match_consecutive(n)), ("epipolar", lambda: prog.verify_epipolar(n, **P["epipolar"])),
             ("pose", lambda: prog.pose_consecutive(n, **intr, **P["pose"])),
             ("trajectory", lambda: prog.trajectory_consecutive(n, **P["trajectory"])),
             ("localize", lambda: prog.localize_consecutive(n, **intr, **P["localize"])),
             ("landmarks", lambda: prog.landmarks_consecutive(n, **intr, **P["landmarks"])),
             ("bridge", lambda: prog.bridge_consecutive(n, **intr, **P["bridge"])),
             ("adjust", lambda: prog.adjust_consecutive(n, **intr, **P["adjust"])))
    for s, call in calls[STAGES.index(first):]:
        call()
    nq = np.minimum(prog.batch_counts(n).astype(np.int64), cap)
    out = dict(n=n, nq=nq)
    out["match"] = [prog.match_read(f, int(nq[f])) for f in range(n - 1)]

    def both(read, count, a, b):
        got = [read(i, cap) for i in range(count)]
        out[a], out[b] = np.array([g[0] for g in got]), np.stack([g[1] for g in got])

    both(prog.verify_epipolar_read, n - 1, "epipolar", "epipolar_mask")
    both(prog.pose_read, n - 1, "pose", "points")
    both(prog.trajectory_read, n, "frames", "map")
    both(prog.localize_read, n - 1, "fix", "fix_mask")
    both(prog.landmarks_read, n - 1, "rows", "landmarks")
    both(prog.bridge_read, n, "bridge", "bridge_mask")
    both(prog.adjust_read, n, "adjusted", "refined")
    return out


def differences(got, want):
    """None when every read-back of `got` equals `want` byte for byte; otherwise a line that names the first stage that differs,
    the pair or frame and the first differing slots with both sides' values."""
    if got["n"] != want["n"] or got["nq"].tolist() != want["nq"].tolist():
        return "stored counts: %s against %s" % (got["nq"].tolist(), want["nq"].tolist())
    for s in STAGES:
        for key, by in FIELDS[s]:
            a, b = got[key], want[key]
            if len(a) != len(b):
                return "%s: %d rows of %s against %d" % (s, len(a), key, len(b))
            for i in range(len(a)):
                x, y = np.asarray(a[i]), np.asarray(b[i])
                if x.dtype != y.dtype or x.shape != y.shape:
                    return "%s: %s of %s %d is %s%s against %s%s" % (s, key, by, i, x.dtype, x.shape, y.dtype, y.shape)
                if x.tobytes() == y.tobytes():
                    continue
                if x.ndim == 0:
                    return "%s: %s of %s %d\n  got  %s\n  want %s" % (s, key, by, i, x, y)
                w = x.dtype.itemsize
                bad = np.nonzero((x.view(np.uint8).reshape(len(x), w) != y.view(np.uint8).reshape(len(y), w)).any(1))[0]
                return "%s: %s of %s %d differs in %d slots, the first %s\n  got  %s\n  want %s" % (
                    s, key, by, i, len(bad), bad[:8].tolist(), x[bad[:8]], y[bad[:8]])
    return None


def blob(res):
    """Every read-back of a result as one byte string."""
    return b"".join(np.ascontiguousarray(v).tobytes() for s in STAGES for key, _ in FIELDS[s] for v in res[key])


# ---- what a chain did ----------------------------------------------------------------------------------------------------------
def summary(res):
    """The figures the conditions are written in, as plain lists."""
    T = orb
    good = (res["landmarks"]["flags"] & T.ORB_POINT_GOOD) != 0
    return dict(
        counts=res["nq"].tolist(),
        epipolar=[(int(r["status"]), int(r["inliers"])) for r in res["epipolar"]],
        pose=[(int(r["status"]), int(r["good"])) for r in res["pose"]],
        trajectory=res["frames"]["status"].tolist(), origins=res["frames"]["origin"].tolist(),
        fix=[(int(r["status"]), int(r["inliers"]), int(r["candidates"])) for r in res["fix"]],
        step=[float(r["step"]) for r in res["fix"]],
        landmarks_good=good.sum(1).tolist(), longest=int(res["rows"]["longest"].max()),
        good_three_views=int((good & (res["landmarks"]["views"] >= 3)).sum()),
        bridge=res["bridge"]["status"].tolist(),
        adjusted=res["adjusted"]["status"].tolist(), observations=res["adjusted"]["observations"].tolist(),
        cost=[(float(r["cost_before"]), float(r["cost_after"])) for r in res["adjusted"]])


def ok_fixes(res):
    """The pairs whose fix is OK with at least half of its candidates inliers."""
    f = res["fix"]
    return [i for i in range(len(f)) if f[i]["status"] == orb.ORB_LOCALIZE_OK and 2 * int(f[i]["inliers"]) >= int(f[i]["candidates"])]


def check_roomy(res):
    """The conditions of the nine-frame scene at a capacity above every counter: what the device's records must show for the
    parity to have covered the five later stages at work.  The weakest figures over 17 orders of the records on the CPU and 160
    more orders tried once: 5 CHAINED frames, 5 OK fixes with at least 98.8 % of their candidates inliers, a longest chain of 5
    views, 909 GOOD landmarks with three views or more, one JOINED frame (the one behind the pair that stands still, in every order),
    5 REFINED frames with the cost falling: each requirement below is the smallest that still means the stage did its work, and the
    slack is the difference."""
    T = orb
    st = res["frames"]["status"].tolist()
    assert {T.ORB_TRAJ_CHAINED, T.ORB_TRAJ_LOST, T.ORB_TRAJ_START} <= set(st), st
    assert len(ok_fixes(res)) >= 2, res["fix"][["status", "inliers", "candidates"]]
    good = (res["landmarks"]["flags"] & T.ORB_POINT_GOOD) != 0
    assert int(res["rows"]["longest"].max()) >= 3 and (res["landmarks"]["views"] >= 3).any(), res["rows"]
    assert (good & (res["landmarks"]["views"] >= 3)).any()
    assert T.ORB_BRIDGE_JOINED in res["bridge"]["status"].tolist(), res["bridge"]["status"]
    a = res["adjusted"]
    better = (a["status"] == T.ORB_ADJUST_REFINED) & (a["cost_after"] < a["cost_before"])
    assert better.any(), a[["status", "cost_before", "cost_after"]]


def check_full(res):
    """The conditions of the batch whose every counter is above the capacity."""
    T = orb
    assert (res["pose"]["status"] == T.ORB_POSE_OK).any(), res["pose"]["status"]
    assert T.ORB_TRAJ_CHAINED in res["frames"]["status"].tolist(), res["frames"]["status"]


def check_empty(res, e):
    """The conditions of the batch whose frame e has no keypoint: both pairs at it FEW and NOMODEL, a new segment behind it, and
    zeros in every per-slot row of that frame."""
    T = orb
    assert res["nq"][e] == 0
    for p in (e - 1, e):
        assert res["epipolar"][p]["status"] == T.ORB_VERIFY_FEW and res["pose"][p]["status"] == T.ORB_POSE_NOMODEL, (p, res["epipolar"][p])
    fr = res["frames"]
    assert fr["status"][e] == T.ORB_TRAJ_LOST and fr["status"][e + 1] == T.ORB_TRAJ_LOST and fr["status"][e + 2] == T.ORB_TRAJ_START
    assert fr["origin"][e + 2] == e + 1 and (fr["origin"][e + 1:] >= e + 1).all() and (fr["origin"][:e + 1] <= e).all(), fr["origin"]
    assert len(res["match"][e]) == 0
    rows = [("epipolar_mask", e), ("points", e), ("map", e), ("fix_mask", e + 1), ("landmarks", e), ("bridge_mask", e), ("refined", e)]
    for key, i in rows:  # the fix of pair e + 1 marks frame e's slots
        assert not np.ascontiguousarray(res[key][i]).view(np.uint8).any(), key
