"""Rate of the trajectory stage (orb_trajectory_consecutive) next to the matcher, the epipolar verifier and the
pose stage of the same run, on the 256 related 1280x720 views of tools/verify_rate.py, extracted once; each call timed alone with
device events over warmed repeats.

    python tools/trajectory_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--intended] [--json out.json]
    python tools/trajectory_rate.py --alternating --frames 4096 [--json out.json]

Prints ms per call of orb_match_consecutive, orb_verify_epipolar, orb_pose_consecutive and orb_trajectory_consecutive, the trajectory
call's ratio to the pose call and to the matcher, and the status counts.  The views are near-planar warps, not a camera's motion: few
pairs are OK and few joints are evaluated, so the serial chain does little there.  --alternating measures the chain at its most
expensive instead: two constructed 320x240 views of one cloud (tests/trajectory_ref.path_scene) injected alternately, so that every
pair is OK and every frame from the third on is CHAINED; only the trajectory call's time means anything in that mode.  Per-kernel
times come from a run of its own under rocprofv3 --kernel-trace --stats.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402

STATUS = ("chained", "start", "restart_few", "restart_spread", "lost", "origin")


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

        ms_match = timed(lambda: prog.match_consecutive(B, stream=sp))
        ms_epi = timed(lambda: prog.verify_epipolar(B, stream=sp, inlier_px=2.0 if a.alternating else 0.0))
        ms_pose = timed(lambda: prog.pose_consecutive(B, stream=sp, **intr))
        ms_traj = timed(lambda: prog.trajectory_consecutive(B, stream=sp))
        recs = np.array([prog.trajectory_read(f, 0)[0] for f in range(B)])
        poses = [prog.pose_read(f, 0)[0] for f in range(B - 1)]
    st = np.bincount(recs["status"], minlength=len(STATUS))
    ev = recs["shared"][recs["shared"] > 0]
    res = {
        "frames": B, "size": [W, H], "cap": cap, "focal": focal, "intended": a.intended, "alternating": a.alternating, "repeats": a.repeats,
        "ms_match": round(ms_match, 4), "ms_verify_epipolar": round(ms_epi, 4), "ms_pose": round(ms_pose, 4),
        "ms_trajectory": round(ms_traj, 4),
        "trajectory_over_pose": round(ms_traj / ms_pose, 4), "trajectory_over_match": round(ms_traj / ms_match, 4),
        "poses_ok": int(sum(int(r["status"]) == orb.ORB_POSE_OK for r in poses)),
        "joints_with_ratios": int(len(ev)), "mean_shared": round(float(ev.mean()), 1) if len(ev) else 0.0,
        "status_counts": {k: int(v) for k, v in zip(STATUS, st)},
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
