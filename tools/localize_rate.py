"""Rate of the localisation stage (orb_localize_consecutive) next to the matcher, the epipolar verifier and the
pose stage, on the 256 related 1280x720 views of tools/verify_rate.py, extracted once; each call timed alone with device events over
warmed repeats.

    python tools/localize_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--intended] [--json out.json]

Prints ms per call (frames - 1 pairs) of orb_match_consecutive, orb_verify_epipolar, orb_pose_consecutive and
orb_localize_consecutive, the localize call's ratio to the other three, and its status counts.  The views are near-planar warps, not
a camera's motion: few of their pairs get an OK pose, so most fixes are NOMAP and the call does little.  The call is therefore timed
a second time behind a pose call that accepts nearly anything (max_reproj_px 1e6, min_good 1, ambiguity_permille 1000), where every
pair with eight epipolar inliers has a map and the kernels build and score every hypothesis (a planar map makes most of them
DEGENERATE, which costs the same build and the same scoring loop): `loose` in the output, with hypothesis x candidate evaluations/s.
The statuses say how the stage judges the views, the times are what is measured.  Needs the GPU (no fallback)."""
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

STATUS = ("ok", "nomap", "few", "degenerate", "minimal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--focal", type=float, default=1000.0)
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

        def fixes():
            return [prog.localize_read(f, 0)[0] for f in range(B - 1)]

        ms_match = timed(lambda: prog.match_consecutive(B, stream=sp))
        ms_epi = timed(lambda: prog.verify_epipolar(B, stream=sp))
        ms_pose = timed(lambda: prog.pose_consecutive(B, stream=sp, **intr))
        ms_loc = timed(lambda: prog.localize_consecutive(B, stream=sp, hypotheses=a.hypotheses, **intr))
        strict = fixes()
        prog.pose_consecutive(B, stream=sp, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
        ms_loose = timed(lambda: prog.localize_consecutive(B, stream=sp, hypotheses=a.hypotheses, **intr))
        loose = fixes()
        # the pairs' correspondences, whatever their status: counted on the host as LO-1 counts them
        nq = np.minimum(prog.batch_counts(B), a.cap).astype(np.int64)
        poses = [prog.pose_read(f, a.cap) for f in range(B - 1)]
        matches = [prog.match_read(f, int(nq[f])) for f in range(B - 1)]
    cand = np.zeros(B - 1, np.int64)
    for f in range(1, B - 1):
        if int(poses[f - 1][0]["status"]) != orb.ORB_POSE_OK:
            continue
        i = np.arange(nq[f - 1])
        ok = (poses[f - 1][1]["flags"][i] & orb.ORB_POINT_GOOD) != 0
        j = matches[f - 1]["index"][i].astype(np.int64)
        ok &= j < nq[f]
        m = matches[f][np.where(ok, j, 0)] if nq[f] else None
        if m is None:
            continue
        ok &= (m["index"].astype(np.int64) < nq[f + 1]) & (m["distance"] <= 64) & (m["distance"].astype(np.float32) < np.float32(0.8) * m["second"].astype(np.float32))
        cand[f] = int(ok.sum())
    pairs = B - 1

    def summary(recs):
        st = np.bincount([int(r["status"]) for r in recs], minlength=len(STATUS))
        return {"status_counts": {k: int(v) for k, v in zip(STATUS, st)},
                "mean_inliers": round(float(np.mean([int(r["inliers"]) for r in recs])), 1)}

    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": a.intended, "repeats": a.repeats,
        "hypotheses": a.hypotheses,
        "ms_match": round(ms_match, 4), "ms_verify_epipolar": round(ms_epi, 4), "ms_pose": round(ms_pose, 4), "ms_localize": round(ms_loc, 4),
        "localize_over_epipolar": round(ms_loc / ms_epi, 4), "localize_over_pose": round(ms_loc / ms_pose, 4),
        "localize_over_match": round(ms_loc / ms_match, 4), "strict": summary(strict),
        "loose": dict(summary(loose), ms_localize=round(ms_loose, 4), localize_over_epipolar=round(ms_loose / ms_epi, 4),
                      pairs_with_a_sample=int((cand >= 6).sum()), mean_candidates=round(float(cand.mean()), 1),
                      evaluations_per_s=float("%.4g" % (a.hypotheses * int(cand[cand >= 6].sum()) / (ms_loose * 1e-3)))),
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
