"""Rate of orb_loop_pairs next to the RANSACs of orb_localize_consecutive and orb_bridge_consecutive and to
orb_verify_pairs on the same lists, all of the same run, on the batch of tools/pairs_rate.py -- 256 related 1280x720 views, every
64 of one scene --, extracted once in the intended mode; each call timed alone with device events over warmed repeats.

    python tools/loop_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--json out.json]

There is no target figure: the yardsticks are the calls of the same run, in ms and in pairs per second.  Two lists: what
orb_place_frames proposes at its defaults (up to 4 candidates a frame), and P = ORB_PAIRS_PER_FRAME x frames backward pairs.  The
views are near-planar warps, not a camera's motion: as they are, few pairs get an OK pose and there is hardly a map, so every
list is timed a second time behind a pose call that accepts nearly anything, a trajectory call that chains whatever it gets and a
landmarks call that accepts any reprojection error (`loose`, as tools/bridge_rate.py).  The counts say how the stage judges the
views, the times are what is measured.  Needs the GPU (no fallback)."""
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

        def rate(n, ms):
            return float("%.4g" % (n / (ms * 1e-3)))

        prog.match_consecutive(B, stream=sp)
        prog.verify_epipolar(B, stream=sp)
        prog.place_frames(B, stream=sp)
        rows = prog.place_read(0, B)
        P = orb.ORB_PAIRS_PER_FRAME * B
        proposed = [(f, int(g)) for f in range(B) for g in rows[f]["best"]["frame"][:int(rows[f]["n"])] if g < orb.ORB_PLACE_DB][:P]
        backward = [(1 + i % (B - 1), (i % (B - 1) - 7 * (i // (B - 1))) % (1 + i % (B - 1))) for i in range(P)]
        assert all(q > t for q, t in backward)
        lists = (("place_list", proposed), ("backward_P", backward))

        def measure(pose_kw, traj_kw, lm_kw, fix_kw):
            prog.pose_consecutive(B, stream=sp, **pose_kw, **intr)
            prog.trajectory_consecutive(B, stream=sp, **traj_kw)
            prog.landmarks_consecutive(B, stream=sp, **lm_kw, **intr)
            ms_loc = timed(lambda: prog.localize_consecutive(B, stream=sp, **fix_kw, **intr))
            ms_br = timed(lambda: prog.bridge_consecutive(B, stream=sp, **fix_kw, **intr))
            fr = np.array([prog.trajectory_read(f, 0)[0] for f in range(B)])
            good = int(sum(int(prog.landmarks_read(p, 0)[0]["good"]) for p in range(B - 1)))
            out = {"frames_lost": int((fr["status"] == orb.ORB_TRAJ_LOST).sum()), "good_landmarks": good,
                   "localize_consecutive": {"pairs": B - 1, "ms": round(ms_loc, 4), "pairs_per_s": rate(B - 1, ms_loc)},
                   "bridge_consecutive": {"frames": B, "ms": round(ms_br, 4), "frames_per_s": rate(B, ms_br)}}
            for name, pairs in lists:
                if not pairs:
                    out[name] = {"pairs": 0}
                    continue
                n = len(pairs)
                prog.match_pairs(np.asarray(pairs, dtype=np.uint32).view(orb.FRAME_PAIR_DTYPE).reshape(-1), stream=sp)
                r = {"pairs": n, "mean_query_keypoints": round(float(stored[[q for q, _ in pairs]].mean()), 1)}
                for key, model in (("verify_pairs_homography", orb.ORB_PAIRS_HOMOGRAPHY), ("verify_pairs_epipolar", orb.ORB_PAIRS_EPIPOLAR)):
                    ms = timed(lambda: prog.verify_pairs(n, model=model, stream=sp))
                    r[key] = {"ms": round(ms, 4), "pairs_per_s": rate(n, ms)}
                ms = timed(lambda: prog.loop_pairs(n, stream=sp, **fix_kw, **intr))
                recs = np.array([prog.loop_pairs_read(i, 0)[0] for i in range(n)])
                st = recs["status"]
                r["loop_pairs"] = {"ms": round(ms, 4), "pairs_per_s": rate(n, ms), "over_verify_pairs_epipolar": round(ms / r["verify_pairs_epipolar"]["ms"], 4),
                                   "over_localize_per_pair": round((ms / n) / (ms_loc / (B - 1)), 4),
                                   "ok": int((st == orb.ORB_LOCALIZE_OK).sum()), "minimal": int((st == orb.ORB_LOCALIZE_MINIMAL).sum()),
                                   "few": int((st == orb.ORB_LOCALIZE_FEW).sum()), "degenerate": int((st == orb.ORB_LOCALIZE_DEGENERATE).sum()),
                                   "nomap": int((st == orb.ORB_LOCALIZE_NOMAP).sum()), "mean_candidates": round(float(recs["candidates"].mean()), 1),
                                   "mean_inliers": round(float(recs["inliers"].mean()), 1)}
                out[name] = r
            return out

        res = {"frames": B, "size": [W, H], "cap": a.cap, "focal": a.focal, "intended": True, "repeats": a.repeats, "mean_keypoints": float(stored.mean()),
               "strict": measure({}, {}, {}, {}),
               "loose": measure(dict(max_reproj_px=1e6, min_good=1, ambiguity_permille=1000), dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1),
                                dict(max_reproj_px=1e6), dict(max_reproj_px=1e6))}
    print(json.dumps(res))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
