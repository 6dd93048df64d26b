"""Time of orb_remap_frames next to orb_graph_pairs and orb_join_pairs of the same run, on the batch of
tools/join_rate.py -- 256 related 1280x720 views, every 64 of one scene --, extracted once in the intended mode; each call timed
alone with device events over warmed repeats.

    python tools/remap_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--slots 2] [--json out.json]

The stage streams: k_rm_land reads 32 bytes and writes 32 bytes per keypoint slot of every pair, whatever the records hold, so the
yardstick is a device-to-device copy that moves the same bytes (32 bytes per slot copied: as many read, as many written), timed in
the same process on the same stream with the same events.  The tool reports both and their ratio and asserts nothing.  Two lists,
as tools/join_rate.py: what orb_place_frames proposes at its defaults, and P = ORB_PAIRS_PER_FRAME x frames backward pairs; each
under the strict defaults and behind the `loose` calls that accept nearly anything, so that the graph moves cameras and the join
links segments.  The counts -- frames from the graph, frames moved, landmarks GOOD, moved, dropped -- say what the stage had to do;
the bytes do not depend on them.  --slots 1 runs k_rm_land with one slot per thread instead of two (TINYORB_REMAP_SLOTS).  Needs
the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--cap", type=int, default=8192)
    ap.add_argument("--focal", type=float, default=1000.0)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--slots", type=int, default=2, choices=(1, 2))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.environ["TINYORB_REMAP_SLOTS"] = str(a.slots)  # read by a program's first remap call
    import torch
    from tinyslam_amd import orb
    from verify_rate import synth_views
    B, W, H = a.frames, a.width, a.height
    frames = synth_views(B, W, H, a.seed)
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=orb.ORB_FLAG_INTENDED, fast_arc=9)
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
            return round(t0.elapsed_time(t1) / a.repeats, 4)

        # the yardstick: a copy of 32 bytes per keypoint slot of the B - 1 pairs, which reads and writes what k_rm_land reads and writes
        pairs_l = B - 1
        n_copy = pairs_l * a.cap * orb.LANDMARK_DTYPE.itemsize
        src = torch.zeros(n_copy, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)

        def copy():
            with torch.cuda.stream(stream):
                dst.copy_(src, non_blocking=True)

        copy_ms = timed(copy)

        prog.match_consecutive(B, stream=sp)
        prog.verify_epipolar(B, stream=sp)
        prog.place_frames(B, stream=sp)
        rows = prog.place_read(0, B)
        P = orb.ORB_PAIRS_PER_FRAME * B
        proposed = [(f, int(g)) for f in range(B) for g in rows[f]["best"]["frame"][:int(rows[f]["n"])] if g < orb.ORB_PLACE_DB][:P]
        backward = [(1 + i % (B - 1), (i % (B - 1) - 7 * (i // (B - 1))) % (1 + i % (B - 1))) for i in range(P)]
        lists = (("place_list", proposed), ("backward_P", backward))

        def measure(pose_kw, traj_kw, lm_kw, fix_kw, graph_kw, join_kw):
            prog.pose_consecutive(B, stream=sp, **pose_kw, **intr)
            prog.trajectory_consecutive(B, stream=sp, **traj_kw)
            prog.landmarks_consecutive(B, stream=sp, **lm_kw, **intr)
            out = {}
            for name, pairs in lists:
                if not pairs:
                    out[name] = {"pairs": 0}
                    continue
                n = len(pairs)
                prog.match_pairs(np.asarray(pairs, dtype=np.uint32).view(orb.FRAME_PAIR_DTYPE).reshape(-1), stream=sp)
                prog.loop_pairs(n, stream=sp, **fix_kw, **intr)
                r = {"pairs": n, "graph_pairs_ms": timed(lambda: prog.graph_pairs(n, stream=sp, **graph_kw)),
                     "join_pairs_ms": timed(lambda: prog.join_pairs(n, stream=sp, **join_kw))}
                for key, flags in (("remap_frames_ms", 0), ("remap_frames_graph_only_ms", orb.ORB_REMAP_GRAPH), ("remap_frames_join_only_ms", orb.ORB_REMAP_JOIN)):
                    r[key] = timed(lambda: prog.remap_frames(flags, stream=sp))
                prog.remap_frames(stream=sp)
                poses = np.array([prog.remap_read(f) for f in range(B)])
                rws = np.array([prog.remap_landmarks(p, 0)[0] for p in range(pairs_l)])
                r.update(copy_ratio=round(r["remap_frames_ms"] / copy_ms, 3), frames_from_graph=int(((poses["status"] & orb.ORB_REMAP_FROM_GRAPH) != 0).sum()),
                         frames_moved=int(((poses["status"] & orb.ORB_REMAP_MOVED) != 0).sum()), roots=len(set(poses["root"].tolist())),
                         landmarks_good=int(rws["good"].sum()), landmarks_moved=int(rws["moved"].sum()), landmarks_dropped=int(rws["dropped"].sum()))
                out[name] = r
            return out

        res = {"frames": B, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": True, "repeats": a.repeats, "warmup": a.warmup,
               "slots_per_thread": a.slots, "pairs_of_landmarks": pairs_l, "k_rm_land_bytes": 2 * n_copy, "copy_bytes_moved": 2 * n_copy,
               "copy_ms": copy_ms, "copy_gb_per_s": round(2 * n_copy / copy_ms / 1e6, 1),
               "strict": measure({}, {}, {}, {}, {}, {}),
               "loose": measure(dict(max_reproj_px=1e6, min_good=1, ambiguity_permille=1000), dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1),
                                dict(max_reproj_px=1e6), dict(max_reproj_px=1e6), dict(min_inliers=1, flags=orb.ORB_GRAPH_USE_MINIMAL),
                                dict(min_inliers=1, min_shared=1, flags=orb.ORB_JOIN_USE_MINIMAL))}
        for mode in ("strict", "loose"):
            for name, _ in lists:
                if "remap_frames_ms" in res[mode][name]:
                    res[mode][name]["remap_gb_per_s"] = round(2 * n_copy / res[mode][name]["remap_frames_ms"] / 1e6, 1)
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
