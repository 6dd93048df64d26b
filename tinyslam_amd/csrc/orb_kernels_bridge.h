// orb_kernels_bridge.h -- a trajectory carried across LOST frames (not in the reference; the definition is the build's own,
// BR-1..BR-7 in DESIGN.md section 23).  One pair with little translation ends the trajectory's segment although the landmarks built
// just before it (orb_landmarks_consecutive) are still in view.  Here the matcher's records carry the GOOD landmarks whose last
// view is the frame before the gap (the anchor T) hop by hop into the LOST frame g, section 21's six-point DLT RANSAC and
// Gauss-Newton refit give camera g relative to camera T in the unit of T's segment, and when a new segment starts behind g the
// lower median of depth ratios measures its unit against the old one.  A serial chain then writes every frame's pose in the frame
// and unit of the earliest origin it can be traced back to.  Every binary32 operation below is written out in the order the
// definition gives (-ffp-contract=off, correctly rounded division and square root), so the CPU restatement (tests/bridge_ref.py)
// reproduces every bit.
//
//   k_br_gather   one workgroup of 256 per frame: the anchor from the frame records (BR-1), the landmark rows of the window in
//                 order, the hops, the candidate (BR-2), compacted by k_loc_gather's step (loc_compact, loc_candidate) and
//                 clipped at the capacity; a frame that is no gap end leaves at once with a count of 0
//   k_loc_score   of orb_kernels_localize.h, as it is, on the bridge's buffers with grid.x = frames (BR-3)
//   k_br_refine   one workgroup per frame: k_loc_refine's fit (loc_fit of orb_kernels_localize.h), the inlier bytes
//                 by keypoint slot, then BR-5 on the candidates: traj_consensus and traj_verdict of orb_kernels_traj.h (integer
//                 atomics only: no result depends on an order), the per-frame fix record
//   k_br_chain    one wave, the arithmetic on lane 0 (BR-6 is sequential by definition; BR-4 is traj_compose); all 64 lanes stage
//                 the frame and fix records of the next 64 frames in LDS
#pragma once
#include "orb_kernels_localize.h"
#include "orb_kernels_traj.h"

namespace orb {

constexpr uint32_t kBrSeedSalt = 0x42523031u;  // BR-3: the draw stream's seed is lowbias32(seed ^ kBrSeedSalt)
constexpr uint32_t kBrFrameWords = 20u;        // OrbFramePose
constexpr uint32_t kBrFixWords = 24u;          // r[9], t[3], step, candidates, inliers, hypothesis, fix, shared, g, consistent, joined, 3 x 0
constexpr uint32_t kBrOutWords = 24u;          // OrbBridgePose
constexpr uint32_t kBrChunk = 64u;             // frames k_br_chain stages at a time
constexpr uint32_t kBrMaxHops = 16u;

struct BrArgs {
    LocArgs loc;             // k_loc_score's view of the stage's own buffers: rows per frame; fix: [frames][kBrFixWords]; cand_of unused
    const uint32_t* frames;  // [frames][kBrFrameWords] of the last orb_trajectory_consecutive
    const float4* lms;       // [pairs][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    uint32_t n_frames;
    uint32_t max_hops;       // BR-1
    uint32_t window;         // BR-2
    uint32_t min_shared;     // BR-5 (TJ-4)
    float tol;               // BR-5 (TJ-3)
    uint32_t permille;       // BR-5 (TJ-4)
    uint32_t* ratios;        // [frames][cap] the bits of a join's ratios by candidate (0: none)
    uint32_t* out;           // [frames][kBrOutWords] OrbBridgePose
};

// BR-1: 0: frame g is no gap end; 1: a gap end without a usable map (NOMAP); 2: a gap end whose anchor is T
__device__ __forceinline__ uint32_t br_anchor(const BrArgs& a, uint32_t g, uint32_t& T) {
    T = 0u;
    if (a.frames[(size_t)g * kBrFrameWords + 17u] != ORB_TRAJ_LOST) return 0u;
    for (uint32_t d = 1u; d <= a.max_hops && d <= g; d++) {
        const uint32_t st = a.frames[(size_t)(g - d) * kBrFrameWords + 17u];
        if (st != ORB_TRAJ_LOST) {
            T = g - d;
            return st == ORB_TRAJ_ORIGIN ? 1u : 2u;
        }
    }
    return 1u;  // g - T > max_hops
}

// grid (frames), block 256
__global__ __launch_bounds__(256) void k_br_gather(BrArgs a) {
    __shared__ uint32_t wave_n[4];
    const LocArgs& L = a.loc;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    uint32_t T;
    if (br_anchor(a, g, T) != 2u) {  // uniform
        if (tid == 0u) L.n_cand[g] = 0u;
        return;
    }
    const uint32_t* const recT = a.frames + (size_t)T * kBrFrameWords;
    const uint32_t o = recT[14];
    float R[9], t[3];
    traj_load_pose(recT, R, t);
    const CornerData* const cg = L.corners + (size_t)g * L.cap;
    const uint32_t first = T > a.window ? T - a.window : 0u;  // BR-2: p + window >= T
    uint32_t base = 0;
    for (uint32_t p = max(o, first); p < T; p++) {
        const uint32_t np = min(L.counts[p], L.cap);
        const float4* const lm = a.lms + (size_t)p * L.cap * 2u;
        for (uint32_t i0 = 0; i0 < np; i0 += 256u) {
            const uint32_t i = i0 + tid;
            bool keep = false;
            uint32_t k = 0;
            float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (i < np) {
                X = lm[2u * i];
                const float4 hi = lm[2u * i + 1u];
                const uint32_t views = __float_as_uint(hi.x) & 0xffffu;
                if (views != 0u && (__float_as_uint(X.w) & ORB_POINT_GOOD) != 0u && p + views - 1u == T) {
                    k = __float_as_uint(hi.z);  // tail_index
                    keep = true;
                    for (uint32_t s = T; s < g && keep; s++) {  // GV-1's filter on every hop; no row is read past its stored count
                        keep = k < min(L.counts[s], L.cap);
                        if (keep) {
                            const MatchRecord m = L.matches[(size_t)s * L.cap + k];
                            const uint32_t d = m.dist & 0xffffu, second = m.dist >> 16;
                            k = m.index;
                            keep = k != kVerifyNone && k < min(L.counts[s + 1u], L.cap) && d <= L.max_distance && (float)d < L.ratio * (float)second;
                        }
                    }
                }
            }
            uint32_t total;
            const uint32_t slot = loc_compact(keep, base, wave_n, total);
            if (keep && slot < L.cap) loc_candidate(L, g, slot, X, R, t, cg[k], __uint_as_float(k));  // the first `capacity` candidates
            base += total;
            __syncthreads();
        }
    }
    if (tid == 0u) L.n_cand[g] = min(base, L.cap);
}

// grid (frames), block 256; the inlier bytes are cleared by a memset before
__global__ __launch_bounds__(256) void k_br_refine(BrArgs a) {
    __shared__ TrajSelectLds lds;
    const LocArgs& L = a.loc;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    uint32_t T;
    const uint32_t kind = br_anchor(a, g, T);  // uniform
    const uint32_t M = kind == 2u ? L.n_cand[g] : 0u;
    const float4* const reca = L.reca + (size_t)g * L.cap;
    const float4* const recb = L.recb + (size_t)g * L.cap;
    const LocFit fit = loc_fit(L, g, M);
    const bool has_min = fit.has_min, keep = fit.keep;
    const float* const Rk = fit.R;
    const float* const tk = fit.t;
    // BR-7: an inlier byte per keypoint slot of frame g (same-value byte stores cannot race)
    uint8_t* const mask = L.mask + (size_t)g * L.cap;
    if (has_min)
        for (uint32_t j = tid; j < M; j += 256u) {
            const float4 Y = reca[j], k = recb[j];
            if (loc_inlier(Rk, tk, Y.x, Y.y, Y.z, k.x, k.y, L)) mask[__float_as_uint(Y.w)] = 1u;
        }
    // BR-5; join is the same in every thread, as traj_consensus's barriers need
    const bool join = keep && g + 2u <= a.n_frames && a.frames[(size_t)(g + 1u) * kBrFrameWords + 17u] == ORB_TRAJ_START;  // uniform
    TrajConsensus c = {0u, 0u, 0u};
    uint32_t verdict = kTrajFew;
    if (join) {
        const float4* const pts = L.points + (size_t)g * L.cap;
        // the ratio of candidate j: an inlier whose keypoint has a GOOD point of pair g, its depth after the fix over that point's
        c = traj_consensus<256u>(lds, a.ratios + (size_t)g * L.cap, M, a.tol, [&](uint32_t j) {
            const float4 Y = reca[j], k = recb[j];
            if (!loc_inlier(Rk, tk, Y.x, Y.y, Y.z, k.x, k.y, L)) return 0u;
            const float4 P = pts[__float_as_uint(Y.w)];
            if ((__float_as_uint(P.w) & ORB_POINT_GOOD) == 0u) return 0u;
            float x, y, z;
            loc_transform(Rk, tk, Y.x, Y.y, Y.z, x, y, z);
            const float rho = z / P.z;
            return isfinite(rho) && rho > 0.0f ? __float_as_uint(rho) : 0u;
        });
        verdict = traj_verdict(c.m, c.consistent, a.min_shared, a.permille);
    }
    if (tid == 0u) {  // the fix record
        uint32_t* const out = L.fix + (size_t)g * kBrFixWords;
        loc_put_pose(out, fit);
        out[13] = has_min ? M : 0u;
        out[14] = fit.inliers;
        out[15] = fit.h;
        out[16] = loc_status(kind != 2u, M, has_min, keep);
        out[17] = c.m;
        out[18] = c.g;
        out[19] = c.consistent;
        out[20] = join && verdict == kTrajHolds ? 1u : 0u;
        out[21] = out[22] = out[23] = 0u;
    }
}

// BR-6: S_o of origin o, read back from the record this lane wrote for frame o: the frame's own pose, gain and root when it is
// JOINED, else (I, 0, 1, o).  The records of the frames below f are written (frame 0 is its own origin and never JOINED).
__device__ __forceinline__ void br_similarity(const uint32_t* out, uint32_t o, uint32_t f, float A[9], float t[3], float& sigma, uint32_t& root) {
    const uint32_t* const rec = out + (size_t)o * kBrOutWords;
    const bool joined = o < f && rec[22] == ORB_BRIDGE_JOINED;
#pragma unroll
    for (int k = 0; k < 9; k++) A[k] = joined ? __uint_as_float(rec[k]) : ((k & 3) == 0 ? 1.0f : 0.0f);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = joined ? __uint_as_float(rec[9 + k]) : 0.0f;
    sigma = joined ? __uint_as_float(rec[13]) : 1.0f;
    root = joined ? rec[14] : o;
}

// grid 1, block 64
__global__ __launch_bounds__(64) void k_br_chain(BrArgs a) {
    __shared__ uint32_t s_frame[kBrChunk * kBrFrameWords];  // frame[base + k], k < 64
    __shared__ uint32_t s_fix[kBrChunk * kBrFixWords];      // fix[base + k]
    const uint32_t lane = threadIdx.x;
    float RT[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, tT[3] = {0.0f, 0.0f, 0.0f};  // the last frame that is not LOST
    uint32_t T = 0u, oT = 0u;
    for (uint32_t base = 0u; base < a.n_frames; base += kBrChunk) {
        __syncthreads();  // lane 0 is done with the chunk before
        {
            const uint32_t w0 = base * kBrFrameWords, wn = a.n_frames * kBrFrameWords;
#pragma unroll
            for (uint32_t k = 0u; k < kBrFrameWords; k++) {
                const uint32_t w = k * 64u + lane;
                s_frame[w] = w0 + w < wn ? a.frames[w0 + w] : 0u;
            }
            const uint32_t x0 = base * kBrFixWords, xn = a.n_frames * kBrFixWords;
#pragma unroll
            for (uint32_t k = 0u; k < kBrFixWords; k++) {
                const uint32_t w = k * 64u + lane;
                s_fix[w] = x0 + w < xn ? a.loc.fix[x0 + w] : 0u;
            }
        }
        __syncthreads();
        const uint32_t end = min(base + kBrChunk, a.n_frames);
#pragma unroll 1
        for (uint32_t f = base; lane == 0u && f < end; f++) {
            const uint32_t* const P = s_frame + (f - base) * kBrFrameWords;
            const uint32_t* const X = s_fix + (f - base) * kBrFixWords;
            float R[9], t[3];
            traj_load_pose(P, R, t);
            float scale = __uint_as_float(P[12]), gain = 0.0f;
            uint32_t root = f, status, anchor = 0u;
            if (P[17] != ORB_TRAJ_LOST) {
                const uint32_t o = P[14];
                float A[9], av[3], sigma;
                br_similarity(a.out, o, f, A, av, sigma, root);
#pragma unroll
                for (int k = 0; k < 9; k++) RT[k] = R[k];
#pragma unroll
                for (int k = 0; k < 3; k++) tT[k] = t[k];
                T = f;
                oT = o;
                if (f == 0u || root == o) {
                    status = ORB_BRIDGE_COPIED;
                    gain = 1.0f;
                    root = f == 0u ? 0u : o;
                } else {
                    status = ORB_BRIDGE_MOVED;
                    float Rn[9], tn[3];
                    traj_compose(R, t, sigma, A, av, Rn, tn);
#pragma unroll
                    for (int k = 0; k < 9; k++) R[k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) t[k] = tn[k];
                    scale = sigma * scale;
                    gain = sigma;
                }
            } else {
                status = ORB_BRIDGE_UNFIXED;
                anchor = T;
                if (X[16] == ORB_LOCALIZE_OK) {
                    float Rx[9], tx[3], Rg[9], tg[3], A[9], av[3], sigma;
                    uint32_t ro;
                    traj_load_pose(X, Rx, tx);
                    traj_compose(Rx, tx, 1.0f, RT, tT, Rg, tg);  // BR-4: camera g in segment oT
                    br_similarity(a.out, oT, f, A, av, sigma, ro);
                    if (ro != oT) {
                        float Rn[9], tn[3];
                        traj_compose(Rg, tg, sigma, A, av, Rn, tn);
#pragma unroll
                        for (int k = 0; k < 9; k++) Rg[k] = Rn[k];
#pragma unroll
                        for (int k = 0; k < 3; k++) tg[k] = tn[k];
                    }
                    const float sc = sigma * __uint_as_float(X[12]);
                    const bool joined = X[20] != 0u;
                    const float sg = joined ? sigma * __uint_as_float(X[18]) : 0.0f;
                    if (isfinite(sc) && isfinite(sg) && traj_pose_finite(Rg, tg)) {
                        status = joined ? ORB_BRIDGE_JOINED : ORB_BRIDGE_FIXED;
#pragma unroll
                        for (int k = 0; k < 9; k++) R[k] = Rg[k];
#pragma unroll
                        for (int k = 0; k < 3; k++) t[k] = tg[k];
                        scale = sc;
                        gain = sg;
                        root = ro;
                    }
                }
            }
            const bool gap = P[17] == ORB_TRAJ_LOST;
            uint32_t* const out = a.out + (size_t)f * kBrOutWords;
            traj_store_pose(out, R, t);
            out[12] = __float_as_uint(scale);
            out[13] = __float_as_uint(gain);
            out[14] = root;
            out[15] = anchor;
            out[16] = gap ? X[13] : 0u;
            out[17] = gap ? X[14] : 0u;
            out[18] = gap ? X[15] : 0u;
            out[19] = gap ? X[17] : 0u;
            out[20] = gap ? X[19] : 0u;
            out[21] = gap ? X[16] : (uint32_t)ORB_LOCALIZE_NOMAP;
            out[22] = status;
            out[23] = 0u;
        }
    }
}

}  // namespace orb
