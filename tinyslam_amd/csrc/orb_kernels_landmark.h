// orb_kernels_landmark.h -- one multi-view map point per landmark (not in the reference; the definition is the build's own,
// LM-1..LM-6 in DESIGN.md section 22).  The trajectory's map (TJ-6) holds a landmark once per pair that triangulated it, each copy
// with the error of one short baseline.  Here the matcher's records chain the GOOD points of consecutive pairs of one segment: a
// live slot that no live slot of the pair before continues into is a start, and each start is one landmark, placed by every view
// of its chain -- the point nearest to all rays (midpoint method) under the frame poses of orb_trajectory_consecutive -- and
// checked by reprojection into every view.  Every binary32 operation below is written out in the order the definition gives
// (-ffp-contract=off, correctly rounded division, no square root), so the CPU restatement (tests/landmark_ref.py) reproduces every
// bit.
//
//   k_lm_mark   grid (pairs, ceil(cap / 256)): a thread per slot; a live slot whose link continues stores a byte 1 at its successor
//               (same-value stores: no race; the bytes are cleared by a memset before); thread 0 of a pair's first block
//               initialises the pair's row
//   k_lm_fuse   the same grid: a thread per slot; a start walks its views twice (the nine sums and the 3 x 3 solve, then the
//               check), in registers; the threads of a workgroup step through the same frames, so the frame poses and counters
//               are uniform loads and the match, point and keypoint reads are the gathers; one 32-byte record per slot; the
//               row's counts through LDS and one integer atomic per block and counter: no result depends on an order
#pragma once
#include "orb_kernels_pose.h"

namespace orb {

constexpr uint32_t kLmThreads = 256u;
constexpr uint32_t kLmFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kLmRowWords = 4u;     // OrbLandmarkRow: landmarks, good, longest, origin
constexpr uint32_t kLmNoOrigin = 0xffffffffu;

struct LmArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    const CornerData* corners;   // [frames][cap]
    const MatchRecord* matches;  // [frames][cap]
    uint32_t cap;
    uint32_t n_frames;
    const float4* points;        // [pairs][cap] of the last orb_pose_consecutive
    const uint32_t* frames;      // [frames][kLmFrameWords] of the last orb_trajectory_consecutive
    float fx, fy, cx, cy;        // LM-1: intrinsics
    float r2;                    // LM-5: max_reproj_px squared
    uint32_t min_views;          // LM-6
    uint8_t* pred;               // [frames][cap] 1: a live slot of the pair before continues into this slot
    uint32_t* rows;              // [frames][kLmRowWords]
    float4* out;                 // [frames][cap][2] OrbLandmark
};

// LM-2: pair p is mapped (p <= n_frames - 2)
__device__ __forceinline__ bool lm_mapped(const LmArgs& a, uint32_t p) { return a.frames[(size_t)(p + 1u) * kLmFrameWords + 17u] != ORB_TRAJ_LOST; }
__device__ __forceinline__ uint32_t lm_origin(const LmArgs& a, uint32_t p) { return a.frames[(size_t)(p + 1u) * kLmFrameWords + 14u]; }

// LM-3: the flags of slot i of the mapped pair p when the slot is live, else 0
__device__ __forceinline__ uint32_t lm_live(const LmArgs& a, uint32_t p, uint32_t i) {
    if (i >= min(a.counts[p], a.cap)) return 0u;
    const uint32_t fl = __float_as_uint(a.points[(size_t)p * a.cap + i].w);
    return (fl & ORB_POINT_GOOD) ? fl : 0u;
}

// grid (n_frames - 1, ceil(cap / kLmThreads)), block kLmThreads
__global__ __launch_bounds__(kLmThreads) void k_lm_mark(LmArgs a) {
    const uint32_t p = blockIdx.x, i = blockIdx.y * kLmThreads + threadIdx.x;
    const bool mapped = lm_mapped(a, p);  // uniform
    const uint32_t o = lm_origin(a, p);
    if (blockIdx.y == 0u && threadIdx.x == 0u) {
        uint32_t* const row = a.rows + (size_t)p * kLmRowWords;
        row[0] = 0u;
        row[1] = 0u;
        row[2] = 0u;
        row[3] = mapped ? o : kLmNoOrigin;
    }
    if (!mapped || p + 2u >= a.n_frames) return;            // uniform: no pair behind this one
    if (!lm_mapped(a, p + 1u) || lm_origin(a, p + 1u) != o) return;  // uniform: frame p + 2 is not CHAINED
    if (i >= a.cap || !lm_live(a, p, i)) return;
    const uint32_t j = a.matches[(size_t)p * a.cap + i].index;
    if (j >= min(a.counts[p + 1u], a.cap)) return;
    if (lm_live(a, p + 1u, j)) a.pred[(size_t)(p + 1u) * a.cap + j] = 1u;
}

// A view of a chain: camera g's pose in the segment of origin o (LM-2) and keypoint k of frame g (orb_corner_level0_xy)
struct LmView {
    float R[9], t[3], u, v;
};

__device__ __forceinline__ void lm_view(const LmArgs& a, uint32_t g, uint32_t k, uint32_t o, LmView& w) {
    const uint32_t* const rec = a.frames + (size_t)g * kLmFrameWords;
    const bool own = g == o;  // uniform: the origin's own record belongs to the segment before it
#pragma unroll
    for (int q = 0; q < 9; q++) w.R[q] = own ? ((q & 3) == 0 ? 1.0f : 0.0f) : __uint_as_float(rec[q]);
#pragma unroll
    for (int q = 0; q < 3; q++) w.t[q] = own ? 0.0f : __uint_as_float(rec[9 + q]);
    const CornerData c = a.corners[(size_t)g * a.cap + k];
    const float s = (float)(1u << (c.octave & 31u));
    w.u = ((float)c.x + 0.5f) * s - 0.5f;
    w.v = ((float)c.y + 0.5f) * s - 0.5f;
}

// LM-3: the views of the start (p, i) of segment o in ascending frame order, `f(view)` on each.  Returns the number of views;
// `tail` is the keypoint slot of the last one, `par` the PARALLAX flag of the chain's live slots.
template <class Fn>
__device__ __forceinline__ uint32_t lm_walk(const LmArgs& a, uint32_t p, uint32_t i, uint32_t o, uint32_t flags, uint32_t& tail, uint32_t& par,
                                            Fn&& f) {
    uint32_t g = p, k = i, views = 0u, fl = flags;
    par = 0u;
    for (;;) {
        LmView w;
        lm_view(a, g, k, o, w);
        f(w);
        views++;
        tail = k;
        if (!fl) break;  // the view behind the chain's last live slot
        par |= fl & ORB_POINT_PARALLAX;
        const uint32_t j = a.matches[(size_t)g * a.cap + k].index;
        if (j >= min(a.counts[g + 1u], a.cap)) break;  // no successor
        g++;
        k = j;
        fl = (g + 1u < a.n_frames && lm_mapped(a, g) && lm_origin(a, g) == o) ? lm_live(a, g, k) : 0u;
    }
    return views;
}

// grid (n_frames - 1, ceil(cap / kLmThreads)), block kLmThreads
__global__ __launch_bounds__(kLmThreads) void k_lm_fuse(LmArgs a) {
    __shared__ uint32_t s_row[3];  // starts, good, longest
    const uint32_t p = blockIdx.x, i = blockIdx.y * kLmThreads + threadIdx.x;
    if (threadIdx.x < 3u) s_row[threadIdx.x] = 0u;
    __syncthreads();
    const bool mapped = lm_mapped(a, p);  // uniform
    const uint32_t o = lm_origin(a, p);
    float4 lo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t hi0 = 0u, hi1 = 0u, hi2 = 0u;
    const uint32_t flags = mapped && i < a.cap ? lm_live(a, p, i) : 0u;
    if (flags && !a.pred[(size_t)p * a.cap + i]) {  // LM-3: a start
        // LM-4
        float A00 = 0.0f, A01 = 0.0f, A02 = 0.0f, A11 = 0.0f, A12 = 0.0f, A22 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
        uint32_t tail = 0u, par = 0u;
        const uint32_t views = lm_walk(a, p, i, o, flags, tail, par, [&](const LmView& w) {
            const float d0 = (w.u - a.cx) / a.fx, d1 = (w.v - a.cy) / a.fy, d2 = 1.0f;
            const float w0 = (w.R[0] * d0 + w.R[3] * d1) + w.R[6] * d2;
            const float w1 = (w.R[1] * d0 + w.R[4] * d1) + w.R[7] * d2;
            const float w2 = (w.R[2] * d0 + w.R[5] * d1) + w.R[8] * d2;
            const float c0 = -((w.R[0] * w.t[0] + w.R[3] * w.t[1]) + w.R[6] * w.t[2]);
            const float c1 = -((w.R[1] * w.t[0] + w.R[4] * w.t[1]) + w.R[7] * w.t[2]);
            const float c2 = -((w.R[2] * w.t[0] + w.R[5] * w.t[1]) + w.R[8] * w.t[2]);
            const float n = (w0 * w0 + w1 * w1) + w2 * w2;
            const float q00 = 1.0f - (w0 * w0) / n, q01 = 0.0f - (w0 * w1) / n, q02 = 0.0f - (w0 * w2) / n;
            const float q11 = 1.0f - (w1 * w1) / n, q12 = 0.0f - (w1 * w2) / n, q22 = 1.0f - (w2 * w2) / n;
            const float e0 = (q00 * c0 + q01 * c1) + q02 * c2;
            const float e1 = (q01 * c0 + q11 * c1) + q12 * c2;
            const float e2 = (q02 * c0 + q12 * c1) + q22 * c2;
            A00 += q00;
            A01 += q01;
            A02 += q02;
            A11 += q11;
            A12 += q12;
            A22 += q22;
            b0 += e0;
            b1 += e1;
            b2 += e2;
        });
        const float m[9] = {A00, A01, A02, A01, A11, A12, A02, A12, A22};
        float C[9];
        pose_cof(m, C);
        const float det = (A00 * C[0] + A01 * C[1]) + A02 * C[2];
        const float X0 = ((C[0] * b0 + C[1] * b1) + C[2] * b2) / det;
        const float X1 = ((C[3] * b0 + C[4] * b1) + C[5] * b2) / det;
        const float X2 = ((C[6] * b0 + C[7] * b1) + C[8] * b2) / det;
        const bool solved = isfinite(det) && det > 0.0f && isfinite(X0) && isfinite(X1) && isfinite(X2);
        uint32_t inliers = 0u, out_flags = 0u;
        if (solved) {
            // LM-5
            uint32_t tail2, par2;
            lm_walk(a, p, i, o, flags, tail2, par2, [&](const LmView& w) {
                const float yx = ((w.R[0] * X0 + w.R[1] * X1) + w.R[2] * X2) + w.t[0];
                const float yy = ((w.R[3] * X0 + w.R[4] * X1) + w.R[5] * X2) + w.t[1];
                const float yz = ((w.R[6] * X0 + w.R[7] * X1) + w.R[8] * X2) + w.t[2];
                const float ex = a.fx * yx + (a.cx - w.u) * yz;
                const float ey = a.fy * yy + (a.cy - w.v) * yz;
                inliers += (yz > 0.0f && ex * ex + ey * ey <= a.r2 * (yz * yz)) ? 1u : 0u;
            });
            const bool good = views >= a.min_views && inliers == views;
            out_flags = good ? (ORB_POINT_GOOD | par) : 0u;
            lo = make_float4(X0, X1, X2, __uint_as_float(out_flags));
        }
        hi0 = views | inliers << 16;
        hi1 = o;
        hi2 = tail;
        atomicAdd(&s_row[0], 1u);
        if (out_flags & ORB_POINT_GOOD) atomicAdd(&s_row[1], 1u);
        atomicMax(&s_row[2], views);
    }
    if (i < a.cap) {
        float4* const out = a.out + ((size_t)p * a.cap + i) * 2u;
        out[0] = lo;
        out[1] = make_float4(__uint_as_float(hi0), __uint_as_float(hi1), __uint_as_float(hi2), 0.0f);
    }
    __syncthreads();
    if (threadIdx.x < 3u && s_row[threadIdx.x]) {
        uint32_t* const row = a.rows + (size_t)p * kLmRowWords + threadIdx.x;
        if (threadIdx.x == 2u)
            atomicMax(row, s_row[2]);
        else
            atomicAdd(row, s_row[threadIdx.x]);
    }
}

}  // namespace orb
