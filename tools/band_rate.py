"""Rate and recall of epipolar-band guided matching (orb_match_epipolar) on the frames of
tools/verify_rate.py: 256 related 1280x720 views (shifted, +-3 % scaled, mildly perspective views of four synthetic scenes), extracted
once, then timed with device events over warmed repeats:

  * the brute-force matcher (orb_match_consecutive) and guided matching with the identity model at r = 16: the yardsticks;
  * the epipolar verification (orb_verify_epipolar);
  * the band call with the verified fundamental matrices at (d = 2, R = 0) and (d = 2, R = 32) (binning + search).

It also counts the candidates per query of both band calls, and the correct correspondences per pair -- matches whose target lies
within 2 px of the ground-truth warp of the query -- for brute force, brute force restricted to the epipolar inliers, and both band
calls.

    python tools/band_rate.py [--frames 256] [--repeats 20] [--intended] [--json out.json]

Per-kernel times come from a run of its own under rocprofv3 --kernel-trace --stats.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tinyslam_amd import orb  # noqa: E402
from tools.guided_rate import correct, synth_views, truth  # noqa: E402


def band_counts(qc, tc, Fm, d, R):
    """Candidates of EB-3 (binary32, as the kernel) over the queries that have a line: (candidates, such queries)."""
    f32 = np.float32
    xq, yq = orb.level0_xy(qc)
    xt, yt = orb.level0_xy(tc)
    m = np.asarray(Fm, f32).reshape(9)
    with np.errstate(all="ignore"):
        a0 = (m[0] * xq + m[1] * yq) + m[2]
        a1 = (m[3] * xq + m[4] * yq) + m[5]
        a2 = (m[6] * xq + m[7] * yq) + m[8]
        n2 = a0 * a0 + a1 * a1
        t = (f32(d) * f32(d)) * n2
        ok = np.isfinite(a0) & np.isfinite(a1) & np.isfinite(a2) & np.isfinite(t) & (n2 >= f32(2.0 ** -64))
    total = 0
    for i0 in range(0, len(qc), 512):
        s = slice(i0, i0 + 512)
        with np.errstate(all="ignore"):
            r = (a0[s, None] * xt[None, :] + a1[s, None] * yt[None, :]) + a2[s, None]
            inb = ok[s, None] & (r * r <= t[s, None])
        if R:
            inb &= (np.abs(xt[None, :] - xq[s, None]) <= f32(R)) & (np.abs(yt[None, :] - yq[s, None]) <= f32(R))
        total += int(inb.sum())
    return total, int(ok.sum())


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
    ap.add_argument("--sample", type=int, default=16, help="pairs over which candidates and correct matches are counted")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    W, H, B = a.width, a.height, a.frames
    frames, Gs = synth_views(B, W, H, a.seed)
    flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if a.intended else 0)
    V = orb.ORB_BAND_VERIFIED
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
        ms_ident = timed(lambda: prog.match_guided(B, source=orb.ORB_GUIDE_IDENTITY, radius_px=16.0, stream=sp))
        ms_epi = timed(lambda: prog.verify_epipolar(B, stream=sp))
        ms_line = timed(lambda: prog.match_epipolar(B, source=V, band_px=2.0, stream=sp))
        ms_win = timed(lambda: prog.match_epipolar(B, source=V, band_px=2.0, radius_px=32.0, stream=sp))
        pairs = B - 1
        sample = np.unique(np.linspace(0, pairs - 1, min(a.sample, pairs)).astype(int)) if a.sample else np.zeros(0, int)
        counts = np.minimum(prog.batch_counts(B), a.cap)
        recs = {}
        for f in sample:
            for g in (f, f + 1):
                if g not in recs:
                    recs[g] = prog.batch_read(int(g), int(counts[g]))[0]
        erec = {int(f): prog.verify_epipolar_read(int(f), a.cap) for f in sample}
        status = np.array([int(prog.verify_epipolar_read(f, 0)[0]["status"]) for f in range(pairs)])
        bf = {int(f): prog.match_read(int(f), a.cap) for f in sample}
        bw = {int(f): prog.match_epipolar_read(int(f), a.cap) for f in sample}
        prog.match_epipolar(B, source=V, band_px=2.0, stream=sp)
        bl = {int(f): prog.match_epipolar_read(int(f), a.cap) for f in sample}
    cand_l, cand_w = [0, 0], [0, 0]
    c_bf, c_bfe, c_bl, c_bw = [], [], [], []
    for f in sample:
        f = int(f)
        qc, tc, nq = recs[f], recs[f + 1], int(counts[f])
        T = truth(Gs[f], Gs[f + 1], H, mirrored=not a.intended)
        if erec[f][0]["status"] in (0, 3):
            for acc, R in ((cand_l, 0.0), (cand_w, 32.0)):
                c, q = band_counts(qc, tc, erec[f][0]["h"], 2.0, R)
                acc[0] += c
                acc[1] += q
        idx = bf[f]["index"][:nq].copy()
        c_bf.append(correct(qc, tc, idx, T))
        idx[erec[f][1][:nq] != 1] = orb.ORB_MATCH_NONE
        c_bfe.append(correct(qc, tc, idx, T))
        c_bl.append(correct(qc, tc, bl[f]["index"][:nq], T))
        c_bw.append(correct(qc, tc, bw[f]["index"][:nq], T))
    mean = lambda v: round(float(np.mean(v)), 1) if len(v) else None  # noqa: E731
    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "intended": a.intended, "repeats": a.repeats,
        "ms_match": round(ms_match, 4), "ms_guided_identity_r16": round(ms_ident, 4), "ms_verify_epipolar": round(ms_epi, 4),
        "ms_band_d2": round(ms_line, 4), "ms_band_d2_r32": round(ms_win, 4),
        "band_d2_over_match": round(ms_line / ms_match, 4), "band_d2_r32_over_match": round(ms_win / ms_match, 4),
        "mean_keypoints": round(float(counts.mean()), 1),
        "pairs_with_model": int(np.sum((status == 0) | (status == 3))),
        "sampled_pairs": int(len(sample)),
        "candidates_per_query_d2": round(cand_l[0] / max(cand_l[1], 1), 2),
        "candidates_per_query_d2_r32": round(cand_w[0] / max(cand_w[1], 1), 2),
        "correct_per_pair_bruteforce": mean(c_bf),
        "correct_per_pair_bruteforce_epipolar_inliers": mean(c_bfe),
        "correct_per_pair_band_d2": mean(c_bl),
        "correct_per_pair_band_d2_r32": mean(c_bw),
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
