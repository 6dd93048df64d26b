"""Rate and quality of feature tracks and keyframes (orb_track_consecutive) on the frames of
tools/guided_rate.py: 256 related 1280x720 views of four synthetic scenes, extracted once, matched, verified and guided by the
verified models at r = 3 once, then timed with device events over warmed repeats:

  * the brute-force matcher alone (orb_match_consecutive), the yardstick;
  * the track call alone from each source (VERIFIED, GUIDED, MATCHED) at the default parameters.

It also reports, per source, the mean and median track length (tracks of two frames or more, and all tracks), the keyframes at the
defaults, and the fraction of links (next != NONE) whose target lies within 2 px of the ground-truth warp of the query.

    python tools/track_rate.py [--frames 256] [--repeats 20] [--intended] [--json out.json]

Per-kernel times come from a run of its own under rocprofv3 --kernel-trace --stats.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402
from guided_rate import synth_views, truth  # noqa: E402

NAMES = {orb.ORB_TRACK_VERIFIED: "verified", orb.ORB_TRACK_GUIDED: "guided", orb.ORB_TRACK_MATCHED: "matched"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--intended", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    W, H, B = a.width, a.height, a.frames
    frames, Gs = synth_views(B, W, H, a.seed)
    flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if a.intended else 0)
    res = {"frames": B, "pairs": B - 1, "size": [W, H], "cap": a.cap, "intended": a.intended, "repeats": a.repeats}
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
        prog.verify_consecutive(B, stream=sp)
        prog.match_guided(B, source=orb.ORB_GUIDE_VERIFIED, radius_px=3.0, stream=sp)
        res["ms_match"] = round(ms_match, 4)
        counts = np.minimum(prog.batch_counts(B), a.cap)
        res["mean_keypoints"] = round(float(counts.mean()), 1)
        recs = [prog.batch_read(f, int(counts[f]))[0] for f in range(B)]
        for src, name in NAMES.items():
            ms = timed(lambda: prog.track_consecutive(B, source=src, stream=sp))
            tracks = [prog.track_read(f, a.cap) for f in range(B)]
            fr = prog.track_frames(B)
            lengths, good, links = [], 0, 0
            for f in range(B):
                t = tracks[f][:counts[f]]
                starts = t["prev"] == orb.ORB_MATCH_NONE
                lengths.append(t["tail_frame"][starts].astype(np.int64) - f + 1)
                if f + 1 < B:
                    i = np.nonzero(t["next"] != orb.ORB_MATCH_NONE)[0]
                    if len(i):
                        T = truth(Gs[f], Gs[f + 1], H, mirrored=not a.intended)
                        xq, yq = (v.astype(np.float64) for v in orb.level0_xy(recs[f][i]))
                        xt, yt = (v.astype(np.float64) for v in orb.level0_xy(recs[f + 1][t["next"][i]]))
                        p = T @ np.stack([xq, yq, np.ones_like(xq)])
                        good += int(np.sum(np.hypot(p[0] / p[2] - xt, p[1] / p[2] - yt) <= 2.0))
                        links += len(i)
            L = np.concatenate(lengths)
            L2 = L[L > 1]
            res[name] = {"ms_track": round(ms, 4), "track_over_match": round(ms / ms_match, 4), "links_per_pair": round(links / (B - 1), 1),
                         "correct_links": round(good / max(links, 1), 4), "tracks": int(len(L)), "tracks_linked": int(len(L2)),
                         "mean_length_linked": round(float(L2.mean()) if len(L2) else 0.0, 3),
                         "median_length_linked": float(np.median(L2)) if len(L2) else 0.0,
                         "mean_length_all": round(float(L.mean()), 3), "keyframes": int(fr["keyframe"].sum()),
                         "keyframe_list": [int(k) for k in np.nonzero(fr["keyframe"])[0]]}
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
