"""Rate of orb_anchor_frames next to orb_join_pairs on the in-batch equivalents of the same list and to a
device-to-device copy, all of the same process, on the batch and store of tools/keyframes_rate.py -- 256 related 1280x720 views,
extracted once in the intended mode at capacity 8192, every fourth frame a keyframe --; each call timed alone with device events
over warmed repeats.

    python tools/anchor_rate.py [--frames 256] [--keyframes 64] [--repeats 20] [--json out.json]

A list of P = 1024 entries (q, T) over the keyframes' source frames is matched and localised once as (q, T) by orb_match_pairs /
orb_loop_pairs, which orb_join_pairs reads, and once as (q, slot of T) by orb_match_keyframes / orb_localize_keyframes, which
orb_anchor_frames reads; the two calls are alternated over `--rounds` rounds, so the spread of a call's own repeats is in the
record.  The map is the `loose` one of tools/loop_rate.py (the views are near-planar warps, and the strict chain leaves hardly a
landmark).  The verdict census says what the entries were: the join refuses an entry as SAME or FORWARD before it computes a
ratio, the anchor has no such clauses.  The landmark pass streams: k_an_land reads 32 bytes and writes 32 bytes per keypoint slot
of every pair, whatever the records hold, so its yardstick is a device-to-device copy that moves the same bytes (section 31's).
The tool times the copy and a call of one entry, which runs the memsets, the owners' pass, one workgroup of k_an_ratio, the two
per-frame kernels and all of k_an_land; k_an_land alone is read from a kernel trace of this tool in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/anchor_rate.py --rounds 1).  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402

ANCHOR_VERDICTS = ("HOLDS", "STATUS", "FEW", "RANGE", "NONFINITE", "RATIO_FEW", "RATIO_SPREAD")
JOIN_VERDICTS = ("HOLDS", "STATUS", "FEW", "RANGE", "SAME", "FORWARD", "NONFINITE", "RATIO_FEW", "RATIO_SPREAD")


def census(verdicts, names):
    return {names[k]: int(c) for k, c in enumerate(np.bincount(verdicts, minlength=len(names))) if c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--keyframes", type=int, default=64)
    ap.add_argument("--focal", type=float, default=1000.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    from verify_rate import synth_views
    B, W, H, S = a.frames, a.width, a.height, a.keyframes
    frames = synth_views(B, W, H, a.seed)
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=orb.ORB_FLAG_INTENDED, fast_arc=9)
    intr = dict(fx=a.focal, fy=a.focal, cx=(W - 1) / 2, cy=(H - 1) / 2)
    with orb.OrbProgram(cfg) as prog:
        prog.extract_batch_host(frames)
        prog.batch_sync()
        stored = np.minimum(prog.batch_counts(B), a.cap).astype(np.int64)
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

        prog.match_consecutive(B, stream=sp)
        prog.verify_epipolar(B, stream=sp)
        prog.pose_consecutive(B, stream=sp, max_reproj_px=1e6, min_good=1, ambiguity_permille=1000, **intr)
        prog.trajectory_consecutive(B, stream=sp, min_shared=1, scale_tolerance=1e6, consistent_permille=1)
        prog.landmarks_consecutive(B, stream=sp, max_reproj_px=1e6, **intr)
        origins = np.array([prog.trajectory_read(f, 0)[0]["origin"] for f in range(B)])
        step = B // S
        kf_frames = [step * s for s in range(S)]
        entries = np.zeros(S, orb.KEYFRAME_ENTRY_DTYPE)
        entries["frame"], entries["slot"] = kf_frames, np.arange(S)
        P = orb.ORB_PAIRS_PER_FRAME * B
        pairs = []
        for i in range(P):
            q, s = i % B, (7 * i + i // B) % S
            if q == kf_frames[s]:
                s = (s + 1) % S
            pairs.append((q, s))
        qT = np.asarray([(q, kf_frames[s]) for q, s in pairs], dtype=np.uint32).view(orb.FRAME_PAIR_DTYPE).reshape(-1)
        qs = np.asarray(pairs, dtype=np.uint32).view(orb.KEYFRAME_PAIR_DTYPE).reshape(-1)
        prog.keyframes_reserve(S)
        prog.keyframes_insert(entries, stream=sp)
        fix_kw = dict(max_reproj_px=1e6)
        prog.match_pairs(qT, stream=sp)
        prog.loop_pairs(P, stream=sp, **fix_kw, **intr)
        prog.match_keyframes(qs, stream=sp)
        prog.localize_keyframes(P, stream=sp, **fix_kw, **intr)
        join_ms, anchor_ms = [], []
        for _ in range(a.rounds):
            join_ms.append(timed(lambda: prog.join_pairs(P, stream=sp)))
            anchor_ms.append(timed(lambda: prog.anchor_frames(P, stream=sp)))
        links = prog.anchor_links(P)
        segs = prog.anchor_segments(B)
        poses = np.array([prog.anchor_read(f) for f in range(B)])
        rows = np.array([prog.anchor_landmarks(p, 0)[0] for p in range(B - 1)])
        jlinks = prog.join_links(P)
        one_ms = [timed(lambda: prog.anchor_frames(1, stream=sp)) for _ in range(a.rounds)]
        # the yardstick: a copy of 32 bytes per keypoint slot of the B - 1 pairs, which reads and writes what k_an_land reads and writes
        n_copy = (B - 1) * a.cap * orb.LANDMARK_DTYPE.itemsize
        with torch.cuda.stream(stream):
            src = torch.zeros(n_copy, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)

        copy_ms = [timed(copy) for _ in range(a.rounds)]

        def r4(v):
            return [round(float(x), 4) for x in v]

        res = {"frames": B, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": True, "repeats": a.repeats, "warmup": a.warmup, "rounds": a.rounds,
               "mean_keypoints": float(stored.mean()), "keyframes": S, "entries": P, "segments_of_the_batch": int(len(set(origins.tolist()))),
               "anchor_frames_ms": r4(anchor_ms), "join_pairs_ms": r4(join_ms),
               "anchor_over_join": round(float(np.mean(anchor_ms) / np.mean(join_ms)), 4),
               "anchor_verdicts": census(links["verdict"], ANCHOR_VERDICTS), "join_verdicts": census(jlinks["verdict"], JOIN_VERDICTS),
               "anchor_mean_shared": round(float(links["shared"].mean()), 1), "join_mean_shared": round(float(jlinks["shared"].mean()), 1),
               "segments_anchored": int((segs["status"] == orb.ORB_ANCHOR_SEGMENT_ANCHORED).sum()),
               "frames_anchored": int((poses["status"] == orb.ORB_ANCHOR_ANCHORED).sum()),
               "landmarks_good": int(rows["good"].sum()), "landmarks_moved": int(rows["moved"].sum()), "landmarks_dropped": int(rows["dropped"].sum()),
               "anchor_frames_of_one_entry_ms": r4(one_ms),
               "note": "a call of one entry runs the memsets, the owners' pass, one workgroup of k_an_ratio, the per-frame kernels and all of k_an_land",
               "k_an_land_bytes": 2 * n_copy, "copy_bytes_moved": 2 * n_copy, "copy_ms": r4(copy_ms),
               "copy_gb_per_s": round(2 * n_copy / float(np.mean(copy_ms)) / 1e6, 1),
               "one_entry_over_copy": round(float(np.mean(one_ms) / np.mean(copy_ms)), 3)}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
