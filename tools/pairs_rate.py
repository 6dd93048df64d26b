"""Rate of orb_match_pairs and orb_verify_pairs next to orb_match_consecutive and the consecutive verifiers of
the same run, on the batch of tools/verify_rate.py -- 256 related 1280x720 views, every 64 of one scene --, extracted once in the
intended mode; each call timed alone with device events over warmed repeats.

    python tools/pairs_rate.py [--frames 256] [--repeats 20] [--json out.json]

There is no target figure: the yardsticks are the consecutive calls of the same run, in descriptor pairs per second (the sum over
the listed pairs of stored queries x stored candidates) and in pairs verified per second.  Three lists: the 255 consecutive pairs
(the same body as orb_match_consecutive on the same frames: the rates should agree); what orb_place_frames proposes at its
defaults (up to 4 candidates a frame); and P = ORB_PAIRS_PER_FRAME x frames backward pairs.  An orb_match_pairs call includes
the copy of its list and the expansion of the descriptors of frames 0 .. the largest listed one, as orb_match_consecutive's
includes its expansion.  Needs the GPU (no fallback)."""
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

        def dpairs(pairs):
            p = np.asarray(pairs, np.int64).reshape(-1, 2)
            return int((stored[p[:, 0]] * stored[p[:, 1]]).sum())

        consecutive = [(f, f + 1) for f in range(B - 1)]
        ms = timed(lambda: prog.match_consecutive(B, stream=sp))
        res = {"frames": B, "size": [W, H], "cap": a.cap, "intended": True, "repeats": a.repeats, "mean_keypoints": float(stored.mean()),
               "match_consecutive": {"pairs": B - 1, "ms": round(ms, 4), "descriptor_pairs": dpairs(consecutive),
                                     "descriptor_pairs_per_s": rate(dpairs(consecutive), ms)}}
        for name, fn in (("verify_consecutive", prog.verify_consecutive), ("verify_epipolar", prog.verify_epipolar)):
            ms = timed(lambda: fn(B, stream=sp))
            res[name] = {"pairs": B - 1, "ms": round(ms, 4), "pairs_per_s": rate(B - 1, ms)}

        prog.place_frames(B, stream=sp)
        rows = prog.place_read(0, B)
        proposed = [(f, int(g)) for f in range(B) for g in rows[f]["best"]["frame"][:int(rows[f]["n"])] if g < orb.ORB_PLACE_DB]
        P = orb.ORB_PAIRS_PER_FRAME * B
        backward = [(1 + i % (B - 1), (i % (B - 1) - 7 * (i // (B - 1))) % (1 + i % (B - 1))) for i in range(P)]
        assert all(q > t for q, t in backward)
        for name, pairs in (("consecutive_list", consecutive), ("place_list", proposed[:P]), ("backward_P", backward)):
            if not pairs:
                res[name] = {"pairs": 0}
                continue
            lst = np.asarray(pairs, dtype=np.uint32).view(orb.FRAME_PAIR_DTYPE).reshape(-1)
            ms = timed(lambda: prog.match_pairs(lst, stream=sp))
            r = {"pairs": len(pairs), "ms_match": round(ms, 4), "descriptor_pairs": dpairs(pairs), "descriptor_pairs_per_s": rate(dpairs(pairs), ms)}
            for key, model in (("homography", orb.ORB_PAIRS_HOMOGRAPHY), ("epipolar", orb.ORB_PAIRS_EPIPOLAR)):
                ms = timed(lambda: prog.verify_pairs(len(pairs), model=model, stream=sp))
                recs = [prog.verify_pairs_read(i, 0)[0] for i in range(len(pairs))]
                r[key] = {"ms": round(ms, 4), "pairs_per_s": rate(len(pairs), ms),
                          "ok_or_minimal": int(sum(int(x["status"]) in (0, 3) for x in recs)),
                          "mean_inliers": round(float(np.mean([int(x["inliers"]) for x in recs])), 1)}
            res[name] = r
        c, m = res["consecutive_list"], res["match_consecutive"]
        res["consecutive_list_over_match_consecutive"] = round(c["ms_match"] / m["ms"], 4)
        # the listed consecutive pairs are the consecutive matcher's problem: the same records
        prog.match_pairs(consecutive, stream=sp)
        prog.match_consecutive(B, stream=sp)
        n0 = int(stored[0])
        res["rows_equal_match_read"] = bool(prog.match_pairs_read(0, n0).tobytes() == prog.match_read(0, n0).tobytes())
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
