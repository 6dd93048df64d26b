"""Rate of the place stage (orb_place_frames) next to the matcher of the same run, on the batch of
tools/verify_rate.py -- 256 related 1280x720 views, every 64 of one scene --, extracted once in the intended mode; each call timed
alone with device events over warmed repeats.

    python tools/place_rate.py [--frames 256] [--repeats 20] [--json out.json]

Prints ms per call of orb_match_consecutive (the yardstick: there is no target figure) and of orb_place_frames at the default
signature (16 bits, 8 tables) with min_gap 32 and 1, at a signature an eighth the size (13 bits), and with a database of
ORB_PLACE_DB_MAX entries (the batch's own signatures, repeated), which includes the copy of the database from host memory and the
host's wait for it; the AND/popcount word operations the scoring kernel does per second; and how the rows came out: candidates per
frame and how often a frame's first candidate is a frame of its own scene.  The counts say how the stage judges these views, the
times are what is measured.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402

TILE = 32  # kPlaceTile of csrc/orb_kernels_place.h


def scored_tiles(n_frames, n_db, min_gap):
    """Tiles k_place_score works on: those that hold a database entry or a pair g + min_gap <= f."""
    n = 0
    for q0 in range(0, n_frames, TILE):
        q_last = min(q0 + TILE, n_frames) - 1
        for i0 in range(0, n_db + n_frames, TILE):
            n += i0 < n_db or i0 - n_db + min_gap <= q_last
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from verify_rate import synth_views
    B, W, H = a.frames, a.width, a.height
    frames = synth_views(B, W, H, a.seed)
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=orb.ORB_FLAG_INTENDED, fast_arc=9)
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

        def measure(db=None, **kw):
            ms = timed(lambda: prog.place_frames(B, db=db, stream=sp, **kw))
            rows = prog.place_read(0, B)
            words = ((kw.get("tables", 0) or 8) << (kw.get("bits", 0) or 16)) // 32
            n_db = 0 if db is None else len(db)
            ops = scored_tiles(B, n_db, kw.get("min_gap", 0) or 32) * TILE * TILE * words
            has = rows["n"] > 0
            first = rows["best"]["frame"][:, 0]
            own = has & (first < orb.ORB_PLACE_DB) & (first // 64 == np.arange(B) // 64)
            return {"ms_place": round(ms, 4), "word_ops": int(ops), "word_ops_per_s": float("%.4g" % (ops / (ms * 1e-3))),
                    "frames_with_candidates": int(has.sum()), "mean_candidates": round(float(rows["candidates"].mean()), 2),
                    "first_candidate_of_own_scene": int(own.sum()), "mean_bits_set": round(float(rows["bits_set"].mean()), 1)}

        ms_match = timed(lambda: prog.match_consecutive(B, stream=sp))
        res = {"frames": B, "size": [W, H], "cap": a.cap, "intended": True, "repeats": a.repeats, "ms_match": round(ms_match, 4),
               "mean_keypoints": float(np.minimum(prog.batch_counts(B), a.cap).mean()),
               "default": measure(), "min_gap_1": measure(min_gap=1), "bits_13": measure(bits=13, min_gap=1)}
        prog.place_frames(B, stream=sp)
        own = np.stack([prog.place_signature(f) for f in range(B)])
        db = np.concatenate([own] * (-(-orb.ORB_PLACE_DB_MAX // B)))[:orb.ORB_PLACE_DB_MAX]
        res["database_%d" % len(db)] = measure(db=db)
        res["place_over_match"] = round(res["default"]["ms_place"] / ms_match, 4)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
