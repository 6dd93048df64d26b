"""Rate of the keyframe calls next to orb_match_pairs and orb_loop_pairs on the same (query, target) list
and to a device-to-device copy, all of the same process, on the batch of tools/join_rate.py -- 256 related 1280x720 views,
extracted once in the intended mode at capacity 8192 --; each call timed alone with device events over warmed repeats.

    python tools/keyframes_rate.py [--frames 256] [--keyframes 64] [--repeats 20] [--json out.json]

64 frames of the batch (every fourth) are inserted into slots 0 .. 63; a list of P = 1024 entries (q, T) over those frames is
matched and localised once as (q, T) by orb_match_pairs / orb_loop_pairs and once as (q, slot of T) by orb_match_keyframes /
orb_localize_keyframes, alternated over `--rounds` rounds, so the spread of a call's own repeats is in the record.  The map is the
`loose` one of tools/loop_rate.py (the views are near-planar warps, and the strict chain leaves hardly a landmark).  The insert is
timed next to a device-to-device copy of the bytes its copy kernel reads and writes; a call waits on the host for the call before
it, so that figure is a latency.  Needs the GPU (no fallback)."""
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
        ms_insert = timed(lambda: prog.keyframes_insert(entries, stream=sp))
        heads = np.array([prog.keyframes_read(s, 0)[0] for s in range(S)])
        # k_kf_insert writes a whole slot and reads, per stored record, a corner, a descriptor and an owner word, and per point half a
        # landmark record; the copy reads and writes the same bytes in all.  Not in the count: the insert's memset and index pass (LC-2)
        written = S * (96 + 64 * a.cap)
        read = int(heads["keypoints"].sum()) * (16 + 32 + 4) + int(heads["points"].sum()) * 16
        with torch.cuda.stream(stream):
            src = torch.zeros((read + written) // 2, dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src)

        ms_copy = timed(copy)
        fix_kw = dict(max_reproj_px=1e6)
        m_pairs, m_kf, l_loop, l_kf = [], [], [], []
        for _ in range(a.rounds):
            m_pairs.append(timed(lambda: prog.match_pairs(qT, stream=sp)))
            m_kf.append(timed(lambda: prog.match_keyframes(qs, stream=sp)))
        for _ in range(a.rounds):
            l_loop.append(timed(lambda: prog.loop_pairs(P, stream=sp, **fix_kw, **intr)))
            l_kf.append(timed(lambda: prog.localize_keyframes(P, stream=sp, **fix_kw, **intr)))
        loop = np.array([prog.loop_pairs_read(i, 0)[0] for i in range(P)])
        kf = np.array([prog.localize_keyframes_read(i, 0)[0] for i in range(P)])
        same_rows = all(prog.match_pairs_read(i, a.cap).tobytes() == prog.match_keyframes_read(i, a.cap).tobytes() for i in range(0, P, 37))
        lw, kw = loop.view(np.uint32).reshape(P, 32).copy(), kf.view(np.uint32).reshape(P, 32).copy()
        lw[:, 26] = kw[:, 26] = 0

        def r4(v):
            return [round(float(x), 4) for x in v]

        res = {"frames": B, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": True, "repeats": a.repeats, "rounds": a.rounds,
               "mean_keypoints": float(stored.mean()), "keyframes": S, "entries": P,
               "stored": int((heads["status"] == orb.ORB_KEYFRAME_STORED).sum()), "points": int(heads["points"].sum()),
               "insert": {"ms": round(ms_insert, 4), "bytes_written": written, "bytes_read": read, "copy_bytes": (read + written) // 2,
                          "note": "a call waits on the host for the call before it (the pinned list) and is a memset and three launches: latency, not throughput",
                          "copy_ms": round(ms_copy, 4), "over_copy": round(ms_insert / ms_copy, 3)},
               "match_pairs_ms": r4(m_pairs), "match_keyframes_ms": r4(m_kf),
               "match_keyframes_over_pairs": round(float(np.mean(m_kf) / np.mean(m_pairs)), 4),
               "loop_pairs_ms": r4(l_loop), "localize_keyframes_ms": r4(l_kf),
               "localize_keyframes_over_loop": round(float(np.mean(l_kf) / np.mean(l_loop)), 4),
               "rows_equal_sampled": bool(same_rows), "fix_words_equal": bool((lw == kw).all()),
               "ok": int((kf["status"] == orb.ORB_LOCALIZE_OK).sum()), "minimal": int((kf["status"] == orb.ORB_LOCALIZE_MINIMAL).sum()),
               "few": int((kf["status"] == orb.ORB_LOCALIZE_FEW).sum()), "nomap": int((kf["status"] == orb.ORB_LOCALIZE_NOMAP).sum()),
               "mean_candidates": round(float(kf["candidates"].mean()), 1)}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
