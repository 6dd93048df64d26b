"""Time of orb_join_pairs next to orb_loop_pairs and orb_graph_pairs of the same run, on the batch of
tools/loop_rate.py and tools/graph_rate.py -- 256 related 1280x720 views, every 64 of one scene --, extracted once in the intended
mode; each call timed alone with device events over warmed repeats.

    python tools/join_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--json out.json]

There is no target figure: the yardsticks are the calls of the same run.  Two lists, as tools/graph_rate.py: what orb_place_frames
proposes at its defaults, and P = ORB_PAIRS_PER_FRAME x frames backward pairs; each under the strict defaults and behind the `loose`
pose, trajectory, landmarks and loop calls that accept nearly anything (there the join takes min_inliers 1, min_shared 1 and
ORB_JOIN_USE_MINIMAL, and keeps its tolerance: a link still needs half its ratios within a tenth of their median).  The counts --
verdicts, segments before the join, roots after it -- say what the stage had to do; the times are what is measured.  Needs the GPU
(no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from tinyslam_amd import orb  # noqa: E402

VERDICT = ("holds", "status", "few", "range", "same", "forward", "nonfinite", "ratio_few", "ratio_spread")


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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
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
            out = {"trajectory_consecutive_ms": timed(lambda: prog.trajectory_consecutive(B, stream=sp, **traj_kw))}
            prog.landmarks_consecutive(B, stream=sp, **lm_kw, **intr)
            fr = np.array([prog.trajectory_read(f, 0)[0] for f in range(B)])
            origins = sorted(set(fr["origin"].tolist()))
            out.update(segments=len(origins), frames_lost=int((fr["status"] == orb.ORB_TRAJ_LOST).sum()))
            for name, pairs in lists:
                if not pairs:
                    out[name] = {"pairs": 0}
                    continue
                n = len(pairs)
                prog.match_pairs(np.asarray(pairs, dtype=np.uint32).view(orb.FRAME_PAIR_DTYPE).reshape(-1), stream=sp)
                r = {"pairs": n, "loop_pairs_ms": timed(lambda: prog.loop_pairs(n, stream=sp, **fix_kw, **intr))}
                r["graph_pairs_ms"] = timed(lambda: prog.graph_pairs(n, stream=sp, **graph_kw))
                r["join_pairs_ms"] = timed(lambda: prog.join_pairs(n, stream=sp, **join_kw))
                poses, segs, links = np.array([prog.join_read(f) for f in range(B)]), prog.join_segments(B), prog.join_links(n)
                r["verdict"] = {k: int((links["verdict"] == i).sum()) for i, k in enumerate(VERDICT)}
                r["segments_linked"] = int((segs["status"] == orb.ORB_JOIN_SEGMENT_LINKED).sum())
                r["roots"] = int((segs["status"] == orb.ORB_JOIN_SEGMENT_ROOT).sum())
                r["frames_moved"] = int((poses["status"] == orb.ORB_JOIN_MOVED).sum())
                r["largest_joined_group"] = int(np.bincount(poses["root"], minlength=B).max())
                r["forest_consistent"] = bool(r["roots"] + r["segments_linked"] == out["segments"] and len(set(poses["root"].tolist())) == r["roots"])
                out[name] = r
            return out

        res = {"frames": B, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": True, "repeats": a.repeats, "warmup": a.warmup,
               "strict": measure({}, {}, {}, {}, {}, {}),
               "loose": measure(dict(max_reproj_px=1e6, min_good=1, ambiguity_permille=1000), dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1),
                                dict(max_reproj_px=1e6), dict(max_reproj_px=1e6), dict(min_inliers=1, flags=orb.ORB_GRAPH_USE_MINIMAL),
                                dict(min_inliers=1, min_shared=1, flags=orb.ORB_JOIN_USE_MINIMAL))}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
