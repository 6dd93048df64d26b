"""Rate of relative pose recovery and triangulation (orb_pose_consecutive) next to the matcher and the
epipolar verifier, on the 256 related 1280x720 views of tools/verify_rate.py, extracted once; each call timed alone with device
events over warmed repeats.

    python tools/pose_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--intended] [--json out.json]

Prints ms per call (frames - 1 pairs) of orb_match_consecutive, orb_verify_epipolar and orb_pose_consecutive, the pose call's
ratio to the other two, triangulated (candidate, inlier) evaluations/s, and the status counts.  The views are near-planar warps, not
a camera's motion: the statuses say how the stage judges them, the times are what is measured.  Per-kernel times come from a run of
its own under rocprofv3 --kernel-trace --stats.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402
from verify_rate import synth_views  # noqa: E402

STATUS = ("ok", "nomodel", "few", "ambiguous", "low_parallax")


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
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    W, H, B = a.width, a.height, a.frames
    frames = synth_views(B, W, H, a.seed)
    flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if a.intended else 0)
    intr = dict(fx=a.focal, fy=a.focal, cx=(W - 1) / 2, cy=(H - 1) / 2)
    with orb.OrbProgram(cfg) as prog:
        prog.extract_batch_host(frames)
        prog.batch_sync()
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
        ms_epi = timed(lambda: prog.verify_epipolar(B, stream=sp))
        ms_pose = timed(lambda: prog.pose_consecutive(B, stream=sp, **intr))
        poses = [prog.pose_read(f, 0)[0] for f in range(B - 1)]
        erecs = [prog.verify_epipolar_read(f, 0)[0] for f in range(B - 1)]
    pairs = B - 1
    st = np.bincount([int(r["status"]) for r in poses], minlength=len(STATUS))
    inl = np.array([int(r["inliers"]) for r in poses], np.int64)
    good = np.array([int(r["good"]) for r in poses], np.int64)
    einl = np.array([int(r["inliers"]) for r in erecs], np.int64)
    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": a.intended, "repeats": a.repeats,
        "ms_match": round(ms_match, 4), "ms_verify_epipolar": round(ms_epi, 4), "ms_pose": round(ms_pose, 4),
        "pose_over_epipolar": round(ms_pose / ms_epi, 4), "pose_over_match": round(ms_pose / ms_match, 4),
        "pose_evaluations_per_s": float("%.4g" % (4 * int(einl.sum()) / (ms_pose * 1e-3))),
        "mean_epipolar_inliers": round(float(einl.mean()), 1), "mean_pose_inliers": round(float(inl.mean()), 1),
        "mean_good": round(float(good.mean()), 1),
        "status_counts": {k: int(v) for k, v in zip(STATUS, st)},
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
