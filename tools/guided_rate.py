"""Rate and recall of guided matching (orb_match_guided) on the frames of tools/verify_rate.py: 256 related
1280x720 views (shifted, +-3 % scaled, mildly perspective views of four synthetic scenes), extracted once, then timed with device
events over warmed repeats:

  * the brute-force matcher alone (orb_match_consecutive);
  * guided matching with the identity model at r = 16 (binning + search);
  * match + verify + guided matching with the verified models at r = 3, and the guided call of that chain alone.

It also counts the window's targets per query, and the correct correspondences per pair -- matches whose target lies within 2 px
of the ground-truth warp of the query -- for brute force + verify inliers against guided-verified.

    python tools/guided_rate.py [--frames 256] [--repeats 20] [--intended] [--json out.json]

Per-kernel times come from a run of its own under rocprofv3 --kernel-trace --stats.  Needs the GPU (no fallback)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tinyslam_amd import orb  # noqa: E402


def synth_views(n, W, H, seed):
    """tools/verify_rate.py's views, with the view-to-scene map G of every frame (view pixel p shows scene pixel G p)."""
    from oracle import orb_oracle
    rng = np.random.default_rng(seed)
    pad = 160
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 4), np.uint8)
    Gs = []
    scene = None
    for i in range(n):
        if i % 64 == 0:
            scene = orb_oracle.synth_frame(W + pad, H + pad, seed * 1000 + i // 64)
        s = rng.uniform(0.97, 1.03)
        px, py = rng.uniform(-2e-5, 2e-5, 2)
        A = np.array([[s, 0, rng.uniform(-8, 8)], [0, s, rng.uniform(-8, 8)], [px, py, 1.0]])
        C = np.array([[1, 0, W / 2 + pad / 2], [0, 1, H / 2 + pad / 2], [0, 0, 1]])
        Ci = np.array([[1, 0, -W / 2], [0, 1, -H / 2], [0, 0, 1]])
        G = C @ A @ Ci
        p = np.einsum("ij,jhw->ihw", G, np.stack([x, y, np.ones_like(x)]))
        sx = np.clip(np.floor(p[0] / p[2] + 0.5).astype(np.int64), 0, W + pad - 1)
        sy = np.clip(np.floor(p[1] / p[2] + 0.5).astype(np.int64), 0, H + pad - 1)
        out[i] = scene[sy, sx]
        Gs.append(G)
    return out, Gs


def truth(Ga, Gb, H, mirrored):
    """Keypoint coordinates of view a -> view b (the literal mode's keypoints live in the mirrored frame y -> H - 1 - y)."""
    T = np.linalg.inv(Gb) @ Ga
    if mirrored:
        Fm = np.array([[1, 0, 0], [0, -1, H - 1], [0, 0, 1]], dtype=np.float64)
        T = Fm @ T @ Fm
    return T


def correct(qc, tc, index, T, tol=2.0):
    """Number of matches (index != NONE) whose target lies within tol px of T applied to the query."""
    ok = index != orb.ORB_MATCH_NONE
    if not ok.any():
        return 0
    xq, yq = (v.astype(np.float64) for v in orb.level0_xy(qc[ok]))
    xt, yt = (v.astype(np.float64) for v in orb.level0_xy(tc[index[ok]]))
    p = T @ np.stack([xq, yq, np.ones_like(xq)])
    return int(np.sum(np.hypot(p[0] / p[2] - xt, p[1] / p[2] - yt) <= tol))


def window_counts(qc, tc, M, r):
    """Targets in the GM-3 window of every query with a prediction (binary32, as the kernels)."""
    F = np.float32
    xq, yq = orb.level0_xy(qc)
    xt, yt = orb.level0_xy(tc)
    m = np.asarray(M, F).reshape(9)
    with np.errstate(all="ignore"):
        w = (m[6] * xq + m[7] * yq) + m[8]
        px = ((m[0] * xq + m[1] * yq) + m[2]) / w
        py = ((m[3] * xq + m[4] * yq) + m[5]) / w
    ok = (w > 0) & np.isfinite(px) & np.isfinite(py)
    order = np.argsort(xt)
    xs = xt[order]
    lo = np.searchsorted(xs, px[ok] - F(r) - F(1), "left")
    hi = np.searchsorted(xs, px[ok] + F(r) + F(1), "right")
    n = hi - lo
    qq = np.repeat(np.nonzero(ok)[0], n)
    tj = order[np.repeat(lo - np.cumsum(n) + n, n) + np.arange(int(n.sum()))]
    inw = (np.abs(xt[tj] - px[qq]) <= F(r)) & (np.abs(yt[tj] - py[qq]) <= F(r))
    return int(inw.sum()), int(ok.sum())


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
    ap.add_argument("--sample", type=int, default=32, help="pairs over which candidates and correct matches are counted")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    W, H, B = a.width, a.height, a.frames
    frames, Gs = synth_views(B, W, H, a.seed)
    flags = orb.ORB_FLAG_INTENDED if a.intended else 0
    cfg = orb.OrbConfig(orb.Extent3d(W, H), max_features=a.cap, hierarchy_depth=2, initial_threshold=20.0 / 255.0, max_batch=B,
                        flags=flags, fast_arc=9 if a.intended else 0)
    I, V = orb.ORB_GUIDE_IDENTITY, orb.ORB_GUIDE_VERIFIED
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
        ms_ident = timed(lambda: prog.match_guided(B, source=I, radius_px=16.0, stream=sp))
        ms_chain = timed(lambda: (prog.match_consecutive(B, stream=sp), prog.verify_consecutive(B, stream=sp),
                                  prog.match_guided(B, source=V, radius_px=3.0, stream=sp)))
        ms_gver = timed(lambda: prog.match_guided(B, source=V, radius_px=3.0, stream=sp))
        pairs = B - 1
        sample = np.unique(np.linspace(0, pairs - 1, min(a.sample, pairs)).astype(int))
        counts = np.minimum(prog.batch_counts(B), a.cap)
        recs = {}
        for f in sample:
            for g in (f, f + 1):
                if g not in recs:
                    recs[g] = prog.batch_read(int(g), int(counts[g]))[0]
        vrec = {int(f): prog.verify_read(int(f), a.cap) for f in sample}
        gv = {int(f): prog.match_guided_read(int(f), a.cap) for f in sample}
        bf = {int(f): prog.match_read(int(f), a.cap) for f in sample}
        prog.match_guided(B, source=I, radius_px=16.0, stream=sp)
        gi = {int(f): prog.match_guided_read(int(f), a.cap) for f in sample}
    cand_i = [0, 0]
    cand_v = [0, 0]
    c_bf, c_bfv, c_gv, c_gi = [], [], [], []
    for f in sample:
        f = int(f)
        qc, tc, nq = recs[f], recs[f + 1], int(counts[f])
        T = truth(Gs[f], Gs[f + 1], H, mirrored=not a.intended)
        for acc, M, r in ((cand_i, np.eye(3), 16.0), (cand_v, vrec[f][0]["h"] if vrec[f][0]["status"] in (0, 3) else None, 3.0)):
            if M is not None:
                c, q = window_counts(qc, tc, M, r)
                acc[0] += c
                acc[1] += q
        idx_bf = bf[f]["index"][:nq].copy()
        c_bf.append(correct(qc, tc, idx_bf, T))
        idx_bf[vrec[f][1][:nq] != 1] = orb.ORB_MATCH_NONE
        c_bfv.append(correct(qc, tc, idx_bf, T))
        c_gv.append(correct(qc, tc, gv[f]["index"][:nq], T))
        c_gi.append(correct(qc, tc, gi[f]["index"][:nq], T))
    res = {
        "frames": B, "pairs": pairs, "size": [W, H], "cap": a.cap, "intended": a.intended, "repeats": a.repeats,
        "ms_match": round(ms_match, 4), "ms_guided_identity_r16": round(ms_ident, 4),
        "guided_identity_over_match": round(ms_ident / ms_match, 4),
        "ms_match_verify_guided_r3": round(ms_chain, 4), "ms_guided_verified_r3": round(ms_gver, 4),
        "mean_keypoints": round(float(counts.mean()), 1),
        "sampled_pairs": int(len(sample)),
        "candidates_per_query_identity_r16": round(cand_i[0] / max(cand_i[1], 1), 2),
        "candidates_per_query_verified_r3": round(cand_v[0] / max(cand_v[1], 1), 2),
        "correct_per_pair_bruteforce": round(float(np.mean(c_bf)), 1),
        "correct_per_pair_bruteforce_verify_inliers": round(float(np.mean(c_bfv)), 1),
        "correct_per_pair_guided_verified_r3": round(float(np.mean(c_gv)), 1),
        "correct_per_pair_guided_identity_r16": round(float(np.mean(c_gi)), 1),
    }
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
