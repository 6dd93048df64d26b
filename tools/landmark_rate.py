"""Rate of the landmark stage (orb_landmarks_consecutive) next to the matcher, the epipolar verifier, the pose
stage and the trajectory stage of the same run, on the 256 related 1280x720 views of tools/pose_rate.py, extracted once; each call
timed alone with device events over warmed repeats.

    python tools/landmark_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--intended] [--json out.json]
    python tools/landmark_rate.py --alternating --frames 256 [--json out.json]

Prints ms per call of orb_match_consecutive, orb_verify_epipolar, orb_pose_consecutive, orb_trajectory_consecutive and
orb_landmarks_consecutive, the landmarks call's ratio to the trajectory call (the yardstick: there is no target figure) and its row
counts.  The views are near-planar warps, not a camera's motion: few of their pairs get an OK pose, most frames are LOST and most
pairs unmapped, so the call does little.  It is therefore timed a second time behind a pose call that accepts nearly anything
(max_reproj_px 1e6, min_good 1, ambiguity_permille 1000) and a trajectory call that chains whatever it gets (min_shared 1,
scale_tolerance 1e6, consistent_permille 1), where every pair with eight epipolar inliers is mapped and its chains are walked:
`loose` in the output, with the views walked per second (both walks counted once).  --alternating measures long chains instead: two
constructed 320x240 views of one cloud (tests/trajectory_ref.path_scene) injected alternately, so that every pair is OK, every
frame from the third on is CHAINED and a landmark's chain runs through the whole batch.  The counts say how the stage judges the
views, the times are what is measured.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--focal", type=float, default=1000.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--intended", action="store_true")
    ap.add_argument("--alternating", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    B = a.frames
    if a.alternating:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import constructed as C
        import trajectory_ref as tr
        W, H, cap, focal = 320, 240, 1024, 250.0
        scene = tr.path_scene(np.random.default_rng(a.seed), tr.path_steps("sideways")[:1], W, H, focal, n=700)
        frames = np.zeros((B, H, W, 4), np.uint8)
        flags = 0
    else:
        from verify_rate import synth_views
        W, H, cap, focal = a.width, a.height, a.cap, a.focal
        frames = synth_views(B, W, H, a.seed)
        flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if flags else 0)
    intr = dict(fx=focal, fy=focal, cx=(W - 1) / 2, cy=(H - 1) / 2)
    with orb.OrbProgram(cfg) as prog:
        prog.extract_batch_host(frames)
        prog.batch_sync()
        if a.alternating:
            C.inject(prog, np.array([len(scene["corners"][f & 1]) for f in range(B)], np.uint32),
                     [scene["corners"][f & 1] for f in range(B)], [scene["desc"][f & 1] for f in range(B)])
        stream = torch.cuda.Stream(device=0)
        sp = stream.cuda_stream

        def timed(fn):
            for _ in range(a.warmup):
                fn()
            stream.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(a.repeats):
                fn()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1) / a.repeats

        def summary():
            rows = np.array([prog.landmarks_read(p, 0)[0] for p in range(B - 1)])
            views = 0
            for p in np.nonzero(rows["landmarks"])[0]:
                views += int(prog.landmarks_read(int(p), cap)[1]["views"].astype(np.int64).sum())
            st = np.array([int(prog.trajectory_read(f, 0)[0]["status"]) for f in range(B)])
            return {"mapped_pairs": int((rows["origin"] != orb.ORB_LANDMARK_NO_ORIGIN).sum()), "landmarks": int(rows["landmarks"].sum()),
                    "good": int(rows["good"].sum()), "longest": int(rows["longest"].max()), "views": views,
                    "frames_chained": int((st == orb.ORB_TRAJ_CHAINED).sum()), "frames_lost": int((st == orb.ORB_TRAJ_LOST).sum())}

        ms_match = timed(lambda: prog.match_consecutive(B, stream=sp))
        ms_epi = timed(lambda: prog.verify_epipolar(B, stream=sp, inlier_px=2.0 if a.alternating else 0.0))
        ms_pose = timed(lambda: prog.pose_consecutive(B, stream=sp, **intr))
        ms_traj = timed(lambda: prog.trajectory_consecutive(B, stream=sp))
        ms_lm = timed(lambda: prog.landmarks_consecutive(B, stream=sp, **intr))
        strict = summary()
        res = {
            "frames": B, "size": [W, H], "cap": cap, "focal": focal, "intended": a.intended, "alternating": a.alternating, "repeats": a.repeats,
            "ms_match": round(ms_match, 4), "ms_verify_epipolar": round(ms_epi, 4), "ms_pose": round(ms_pose, 4),
            "ms_trajectory": round(ms_traj, 4), "ms_landmarks": round(ms_lm, 4),
            "landmarks_over_trajectory": round(ms_lm / ms_traj, 4), "landmarks_over_pose": round(ms_lm / ms_pose, 4),
            "landmarks_over_match": round(ms_lm / ms_match, 4), "strict": strict,
        }
        if not a.alternating:
            prog.pose_consecutive(B, stream=sp, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
            loose_traj = dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1)
            ms_traj2 = timed(lambda: prog.trajectory_consecutive(B, stream=sp, **loose_traj))
            ms_lm2 = timed(lambda: prog.landmarks_consecutive(B, stream=sp, max_reproj_px=1e6, **intr))
            loose = summary()
            res["loose"] = dict(loose, ms_trajectory=round(ms_traj2, 4), ms_landmarks=round(ms_lm2, 4),
                                landmarks_over_trajectory=round(ms_lm2 / ms_traj2, 4),
                                views_per_s=float("%.4g" % (loose["views"] / (ms_lm2 * 1e-3))))
        else:
            res["views_per_s"] = float("%.4g" % (strict["views"] / (ms_lm * 1e-3)))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
