"""Rate of the matcher plus the geometric verifier (orb_match_consecutive + orb_verify_consecutive) on 256
related 1280x720 frames: shifted, scaled and perspective-warped views of synthetic scenes (nearest-neighbour inverse mapping,
seeded), extracted once, then match + verify timed with device events over warmed repeats.

    python tools/verify_rate.py [--frames 256] [--hypotheses 512] [--repeats 20] [--intended] [--json out.json]

Prints ms per call (frames - 1 pairs), pairs/s, evaluated (hypothesis, candidate) pairs/s and the mean inlier ratio, and the
matcher's and the verifier's times on their own.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tinyslam_amd import orb  # noqa: E402


def synth_views(n, W, H, seed):
    """n views: every 64 share a scene (synth_frame of a larger canvas), each a random shift / +-3 % scale / mild perspective."""
    from oracle import orb_oracle
    rng = np.random.default_rng(seed)
    pad = 160
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 4), np.uint8)
    scene = None
    for i in range(n):
        if i % 64 == 0:
            scene = orb_oracle.synth_frame(W + pad, H + pad, seed * 1000 + i // 64)
        s = rng.uniform(0.97, 1.03)
        px, py = rng.uniform(-2e-5, 2e-5, 2)
        A = np.array([[s, 0, rng.uniform(-8, 8)], [0, s, rng.uniform(-8, 8)], [px, py, 1.0]])
        C = np.array([[1, 0, W / 2 + pad / 2], [0, 1, H / 2 + pad / 2], [0, 0, 1]])
        Ci = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]])
        G = C @ A @ Ci
        p = np.einsum("ij,jhw->ihw", G, np.stack([x, y, np.ones_like(x)]))
        sx = np.clip(np.floor(p[0] / p[2] + 0.5).astype(np.int64), 0, W + pad - 1)
        sy = np.clip(np.floor(p[1] / p[2] + 0.5).astype(np.int64), 0, H + pad - 1)
        out[i] = scene[sy, sx]
    return out


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
        ms_both = timed(lambda: (prog.match_consecutive(B, stream=sp), prog.verify_consecutive(B, hypotheses=a.hypotheses, stream=sp)))
        recs = [prog.verify_read(f, 0)[0] for f in range(B - 1)]
    pairs = B - 1
    cand = np.array([int(r["candidates"]) for r in recs], np.int64)
    inl = np.array([int(r["inliers"]) for r in recs], np.int64)
    status = np.bincount([int(r["status"]) for r in recs], minlength=4)
    evaluated = int(cand[cand >= 4].sum()) * a.hypotheses
    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "hypotheses": a.hypotheses, "intended": a.intended,
        "ms_match_plus_verify": round(ms_both, 4), "ms_match": round(ms_match, 4), "ms_verify": round(ms_verify, 4),
        "pairs_per_s": round(pairs / (ms_both * 1e-3), 1),
        "evaluated_pairs_per_s": float("%.4g" % (evaluated / (ms_verify * 1e-3))),
        "mean_candidates": round(float(cand.mean()), 1),
        "mean_inlier_ratio": round(float(np.mean(inl[cand > 0] / cand[cand > 0])), 4),
        "status_counts": {"ok": int(status[0]), "few": int(status[1]), "degenerate": int(status[2]), "minimal": int(status[3])},
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
