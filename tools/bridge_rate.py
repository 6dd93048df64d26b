"""Rate of the bridge stage (orb_bridge_consecutive) next to the trajectory, localisation and landmark calls of
the same run, on the 256 related 1280x720 views of tools/pose_rate.py, extracted once; each call timed alone with device events
over warmed repeats.

    python tools/bridge_rate.py [--frames 256] [--focal 1000] [--repeats 20] [--intended] [--json out.json]
    python tools/bridge_rate.py --gapped --frames 256 [--json out.json]

Prints ms per call of orb_trajectory_consecutive, orb_localize_consecutive, orb_landmarks_consecutive and orb_bridge_consecutive,
the bridge call's ratio to the localisation and trajectory calls (the yardsticks: there is no target figure) and how it judged the
frames.  The views are near-planar warps, not a camera's motion: as they are, few pairs get an OK pose and there is no map to
bridge from, so the call is timed a second time behind a pose call that accepts nearly anything and a trajectory call that chains
whatever it gets (`loose`, as tools/landmark_rate.py).  --gapped measures work instead: two constructed 320x240 views of one cloud
(tests/trajectory_ref.path_scene) injected alternately, except that every eighth frame repeats the view before it -- a pause, whose
pair has no parallax -- so that every eighth frame is LOST with the landmarks of the seven frames before it in view.  The counts
say how the stage judges the views, the times are what is measured.  Needs the GPU (no fallback)."""
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
    ap.add_argument("--intended", action="store_true")
    ap.add_argument("--gapped", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    B = a.frames
    if a.gapped:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import constructed as C
        import trajectory_ref as tr
        W, H, cap, focal = 320, 240, 1024, 250.0
        scene = tr.path_scene(np.random.default_rng(a.seed), tr.path_steps("sideways")[:1], W, H, focal, n=700)
        view, v = [], 0
        for f in range(B):
            if f and f % 8:
                v ^= 1  # every eighth frame repeats the view before it
            view.append(v)
        frames = np.zeros((B, H, W, 4), np.uint8)
        flags = 0
    else:
        from verify_rate import synth_views
        W, H, cap, focal = a.width, a.height, a.cap, a.focal
        frames = synth_views(B, W, H, a.seed)
        flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if flags else 0)
    intr = dict(fx=focal, fy=focal, cx=(W - 1) / 2, cy=(H - 1) / 2)
    with orb.OrbProgram(cfg) as prog:
        prog.extract_batch_host(frames)
        prog.batch_sync()
        if a.gapped:
            C.inject(prog, np.array([len(scene["corners"][v]) for v in view], np.uint32), [scene["corners"][v] for v in view],
                     [scene["desc"][v] for v in view])
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

        def summary():
            rec = np.array([prog.bridge_read(f, 0)[0] for f in range(B)])
            st, fx = rec["status"], rec["fix"]
            lost = st >= orb.ORB_BRIDGE_FIXED
            return {"frames_lost": int(lost.sum()), "copied": int((st == orb.ORB_BRIDGE_COPIED).sum()), "moved": int((st == orb.ORB_BRIDGE_MOVED).sum()),
                    "fixed": int((st == orb.ORB_BRIDGE_FIXED).sum()), "joined": int((st == orb.ORB_BRIDGE_JOINED).sum()),
                    "unfixed": int((st == orb.ORB_BRIDGE_UNFIXED).sum()),
                    "fix_ok": int((lost & (fx == orb.ORB_LOCALIZE_OK)).sum()), "fix_nomap": int((lost & (fx == orb.ORB_LOCALIZE_NOMAP)).sum()),
                    "fix_few": int((lost & (fx == orb.ORB_LOCALIZE_FEW)).sum()), "fix_degenerate": int((lost & (fx == orb.ORB_LOCALIZE_DEGENERATE)).sum()),
                    "fix_minimal": int((lost & (fx == orb.ORB_LOCALIZE_MINIMAL)).sum()),
                    "candidates": int(rec["candidates"].sum()), "inliers": int(rec["inliers"].sum()), "roots": int(len(np.unique(rec["root"])))}

        def measure(pose_kw, traj_kw, lm_kw, br_kw):
            prog.pose_consecutive(B, stream=sp, **pose_kw, **intr)
            ms_traj = timed(lambda: prog.trajectory_consecutive(B, stream=sp, **traj_kw))
            ms_loc = timed(lambda: prog.localize_consecutive(B, stream=sp, **intr))
            ms_lm = timed(lambda: prog.landmarks_consecutive(B, stream=sp, **lm_kw, **intr))
            ms_br = timed(lambda: prog.bridge_consecutive(B, stream=sp, **br_kw, **intr))
            return dict(summary(), ms_trajectory=round(ms_traj, 4), ms_localize=round(ms_loc, 4), ms_landmarks=round(ms_lm, 4),
                        ms_bridge=round(ms_br, 4), bridge_over_localize=round(ms_br / ms_loc, 4), bridge_over_trajectory=round(ms_br / ms_traj, 4))

        prog.match_consecutive(B, stream=sp)
        prog.verify_epipolar(B, stream=sp, inlier_px=2.0 if a.gapped else 0.0)
        res = {"frames": B, "size": [W, H], "cap": cap, "focal": focal, "intended": a.intended, "gapped": a.gapped, "repeats": a.repeats,
               "strict": measure({}, {}, {}, {})}
        if not a.gapped:
            res["loose"] = measure(dict(max_reproj_px=1e6, min_good=1, ambiguity_permille=1000),
                                   dict(min_shared=1, scale_tolerance=1e6, consistent_permille=1), dict(max_reproj_px=1e6),
                                   dict(max_reproj_px=1e6, min_shared=1, scale_tolerance=1e6, consistent_permille=1))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
