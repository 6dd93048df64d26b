"""Rate of the adjustment stage (orb_adjust_consecutive) next to the landmark stage of the same run, on the
batches of tools/landmark_rate.py, extracted once; each call timed alone with device events over warmed repeats.

    python tools/adjust_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--rounds 0] [--json out.json]
    python tools/adjust_rate.py --alternating --frames 256 [--json out.json]

Prints ms per call of orb_trajectory_consecutive, orb_landmarks_consecutive and orb_adjust_consecutive at rounds 1, 4 (or --rounds)
and 16, the adjust call's ratio to the landmarks call (the yardstick: there is no target figure), and how the call judged the frames:
free frames by status, observations, the summed cost before and after.  The default batch is 256 related 1280x720 views -- near-planar
warps, not a camera's motion: few pairs get an OK pose and few frames are CHAINED, so the call does little; it is timed again behind a
pose call and a trajectory call that accept nearly anything (`loose`, as in tools/landmark_rate.py), where most frames are free.
--alternating: two constructed 320x240 views of one cloud injected alternately, so that every frame from the third on is CHAINED and
a landmark's chain runs through the whole batch.  The counts say how the stage judges the views, the times are what is measured.
Needs the GPU (no fallback)."""
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
    ap.add_argument("--rounds", type=int, default=0)
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
    else:
        from verify_rate import synth_views
        W, H, cap, focal = a.width, a.height, a.cap, a.focal
        frames = synth_views(B, W, H, a.seed)
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B)
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

        def measure(traj, lm):
            ms_traj = timed(lambda: prog.trajectory_consecutive(B, stream=sp, **traj))
            ms_lm = timed(lambda: prog.landmarks_consecutive(B, stream=sp, **lm, **intr))
            out = {"ms_trajectory": round(ms_traj, 4), "ms_landmarks": round(ms_lm, 4)}
            for rounds in (1, a.rounds or 4, 16):
                ms = timed(lambda: prog.adjust_consecutive(B, stream=sp, rounds=rounds, **intr))
                po = np.array([prog.adjust_read(f, 0)[0] for f in range(B)])
                ref = po["status"] == orb.ORB_ADJUST_REFINED
                out["rounds_%d" % rounds] = {
                    "ms_adjust": round(ms, 4), "adjust_over_landmarks": round(ms / ms_lm, 4),
                    "refined": int(ref.sum()), "few": int((po["status"] == orb.ORB_ADJUST_FEW).sum()),
                    "failed": int((po["status"] == orb.ORB_ADJUST_FAILED).sum()), "held": int((po["status"] == orb.ORB_ADJUST_HELD).sum()),
                    "observations": int(po["observations"].astype(np.int64).sum()),
                    "cost_before": float("%.6g" % po["cost_before"][ref].astype(np.float64).sum()),
                    "cost_after": float("%.6g" % po["cost_after"][ref].astype(np.float64).sum()),
                    "observations_per_s": float("%.4g" % (rounds * int(po["observations"][ref].astype(np.int64).sum()) / (ms * 1e-3)))}
            return out

        prog.match_consecutive(B, stream=sp)
        prog.verify_epipolar(B, stream=sp, inlier_px=2.0 if a.alternating else 0.0)
        prog.pose_consecutive(B, stream=sp, **intr)
        res = {"frames": B, "size": [W, H], "cap": cap, "focal": focal, "alternating": a.alternating, "repeats": a.repeats,
               "strict": measure({}, {})}
        if not a.alternating:
            prog.pose_consecutive(B, stream=sp, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
            res["loose"] = measure(dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1), dict(max_reproj_px=1e6))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
