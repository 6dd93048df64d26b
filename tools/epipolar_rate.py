"""Rate of the epipolar verifier (orb_verify_epipolar) next to the matcher and the homography verifier, on the
256 related 1280x720 views of tools/verify_rate.py, extracted once; each call timed alone with device events over warmed repeats.

    python tools/epipolar_rate.py [--frames 256] [--hypotheses 512] [--repeats 20] [--intended] [--json out.json]

Prints ms per call (frames - 1 pairs) of orb_match_consecutive, orb_verify_consecutive and orb_verify_epipolar, the epipolar call's
ratios to the other two, evaluated (hypothesis, candidate) pairs/s, the mean inlier ratio of both verifiers and the status counts.
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
from verify_rate import synth_views  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--hypotheses", type=int, default=512)
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
        ms_verify = timed(lambda: prog.verify_consecutive(B, hypotheses=a.hypotheses, stream=sp))
        ms_epi = timed(lambda: prog.verify_epipolar(B, hypotheses=a.hypotheses, stream=sp))
        hrecs = [prog.verify_read(f, 0)[0] for f in range(B - 1)]
        erecs = [prog.verify_epipolar_read(f, 0)[0] for f in range(B - 1)]
    pairs = B - 1

    def stats(recs):
        cand = np.array([int(r["candidates"]) for r in recs], np.int64)
        inl = np.array([int(r["inliers"]) for r in recs], np.int64)
        st = np.bincount([int(r["status"]) for r in recs], minlength=4)
        return cand, round(float(np.mean(inl[cand > 0] / cand[cand > 0])), 4), {
            "ok": int(st[0]), "few": int(st[1]), "degenerate": int(st[2]), "minimal": int(st[3])}

    cand, h_ratio, h_status = stats(hrecs)
    _, e_ratio, e_status = stats(erecs)
    evaluated = int(cand[cand >= 8].sum()) * a.hypotheses
    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "hypotheses": a.hypotheses, "intended": a.intended,
        "ms_match": round(ms_match, 4), "ms_verify": round(ms_verify, 4), "ms_epipolar": round(ms_epi, 4),
        "epipolar_over_match": round(ms_epi / ms_match, 4), "epipolar_over_verify": round(ms_epi / ms_verify, 3),
        "epipolar_evaluated_pairs_per_s": float("%.4g" % (evaluated / (ms_epi * 1e-3))),
        "mean_candidates": round(float(cand.mean()), 1),
        "mean_inlier_ratio": {"homography": h_ratio, "epipolar": e_ratio},
        "status_counts": {"homography": h_status, "epipolar": e_status},
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
