// orb_kernels_traj.h -- the pair poses of orb_pose_consecutive chained into one camera path and one point map with a common scale (not
// in the reference; the definition is the build's own, TJ-1..TJ-7 in DESIGN.md section 20).  Pair f - 1 triangulated a landmark from
// camera f - 1, pair f triangulated it again from camera f, and the matcher's index says which point is which: the landmark has two
// depths in camera f, one in units of each pair's baseline, and their ratio is the ratio of the baselines.  The lower median of a
// joint's ratios is its step; the chain multiplies the steps and composes the poses.  Every binary32 operation below is written out
// in the order the definition gives (-ffp-contract=off, correctly rounded division), so the CPU restatement
// (tests/trajectory_ref.py) reproduces every bit.
//
//   k_traj_joint   one workgroup of 1024 threads per joint f = 1 .. n_frames - 2 (it leaves at once unless both pairs are OK):
//                  traj_consensus over the queries of pair f - 1 (traj_ratio), then the joint record with traj_verdict
//   k_traj_chain   one wave, the arithmetic on lane 0 (TJ-5 is sequential by definition: traj_compose); all 64 lanes stage the pose
//                  and joint records of the next 64 frames in LDS
//   k_traj_map     grid (pairs, ceil(cap / 1024)): the points of pair f in the frame and unit of frame f + 1's origin, one
//                  16-byte store per slot
#pragma once
#include "orb_kernels_pose.h"

namespace orb {

constexpr uint32_t kTrajThreads = 1024u;
constexpr uint32_t kTrajFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kTrajJointWords = 4u;   // m, g, consistent, verdict
constexpr uint32_t kTrajHolds = 0u, kTrajFew = 1u, kTrajSpread = 2u;  // TJ-4
constexpr uint32_t kTrajChunk = 64u;       // frames k_traj_chain stages at a time

struct TrajArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    const MatchRecord* matches;  // [frames][cap]
    uint32_t cap;
    uint32_t n_frames;
    const uint32_t* poses;       // [pairs][kPoseWords] of the last orb_pose_consecutive
    const float4* points;        // [pairs][cap] its points
    uint32_t min_shared;         // TJ-4
    float tol;                   // TJ-3
    uint32_t permille;           // TJ-4
    uint32_t need_parallax;      // TJ-2
    uint32_t* ratios;            // [frames][cap] the bits of a joint's ratios (0: none), row f for joint f
    uint32_t* joints;            // [frames][kTrajJointWords], row f for joint f
    uint32_t* frames;            // [frames][kTrajFrameWords] OrbFramePose
    float4* map;                 // [frames][cap]
};

// TJ-2: the bits of query i's ratio at joint f, 0 when it has none
__device__ __forceinline__ uint32_t traj_ratio(const TrajArgs& a, uint32_t f, uint32_t i, uint32_t nq_prev, uint32_t nq, const float r[3], float t2) {
    if (i >= nq_prev) return 0u;
    const float4 X = a.points[(size_t)(f - 1u) * a.cap + i];
    const uint32_t fl = __float_as_uint(X.w);
    if (!(fl & ORB_POINT_GOOD)) return 0u;
    const uint32_t j = a.matches[(size_t)(f - 1u) * a.cap + i].index;
    if (j >= nq) return 0u;
    const float4 Y = a.points[(size_t)f * a.cap + j];
    const uint32_t fl2 = __float_as_uint(Y.w);
    if (!(fl2 & ORB_POINT_GOOD)) return 0u;
    if (a.need_parallax && !(fl & fl2 & ORB_POINT_PARALLAX)) return 0u;
    const float yz = ((r[0] * X.x + r[1] * X.y) + r[2] * X.z) + t2;
    const float rho = yz / Y.z;
    return isfinite(rho) && rho > 0.0f ? __float_as_uint(rho) : 0u;
}

// What the stages after this one take from it (bridge, loop, join): the consensus, the compose and the twelve pose words.

struct TrajSelectLds {  // declared __shared__ by the kernel
    uint32_t hist[256];
    uint32_t count[2];  // m, consistent
    uint32_t sel[2];    // the prefix found so far, the rank within it
};
struct TrajConsensus {
    uint32_t m, g, consistent;  // the ratios, the bits of their lower median (0: m == 0), the ratios within tol g of it
};

// TJ-3/TJ-4 on the n slots of `row`, by a workgroup of kThreads: ratio_bits(i), i < n, gives slot i's ratio as bits (0: none).
// Every thread of the workgroup must make the call (it holds barriers): call sites are workgroup-uniform.
//   A  a slot per thread, strided over n: the bits to global memory, their number through wave ballots and one LDS add per wave
//   B  the ratio of rank (m - 1) / 2 by a radix select from the most significant byte down: four passes, each a 256-bin LDS
//      histogram of the ratios that share the prefix found so far, and a prefix over the bins by one wave
//   C  the ratios within tol g of it, counted like A
// Integer atomics only: no result depends on an order.
template <uint32_t kThreads, class Ratio>
__device__ __forceinline__ TrajConsensus traj_consensus(TrajSelectLds& s, uint32_t* row, uint32_t n, float tol, Ratio ratio_bits) {
    static_assert(kThreads >= 256u && kThreads % 64u == 0u, "a thread per bin, whole waves");
    const uint32_t tid = threadIdx.x;
    const bool first = (tid & 63u) == 0u;
    if (tid < 2u) s.count[tid] = 0u;
    __syncthreads();
    // A
    for (uint32_t base = 0u; base < n; base += kThreads) {  // uniform trip count: the ballots see whole waves
        const uint32_t i = base + tid;
        const uint32_t bits = i < n ? ratio_bits(i) : 0u;
        if (i < n) row[i] = bits;
        const uint32_t c = (uint32_t)__popcll(__ballot(bits != 0u));
        if (first && c) atomicAdd(&s.count[0], c);
    }
    __syncthreads();  // every thread reads back its own stores only; the barrier publishes the count
    const uint32_t m = s.count[0];
    uint32_t g = 0u;
    if (m) {  // uniform
        // B: the element of rank (m - 1) / 2 in ascending order of the bits
        if (tid == 0u) {
            s.sel[0] = 0u;
            s.sel[1] = (m - 1u) / 2u;
        }
#pragma unroll 1
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (kThreads == 256u || tid < 256u) s.hist[tid] = 0u;
            __syncthreads();
            const uint32_t prefix = s.sel[0];
            for (uint32_t i = tid; i < n; i += kThreads) {
                const uint32_t bits = row[i];
                // shift 24: every ratio shares the empty prefix (a shift by 32 is not one)
                const bool in = bits != 0u && (shift == 24 || (bits >> (shift + 8)) == prefix);
                if (in) atomicAdd(&s.hist[bits >> shift & 255u], 1u);
            }
            __syncthreads();
            if (tid < 64u) {  // lane l owns bins 4 l .. 4 l + 3
                const uint32_t k = s.sel[1];
                const uint32_t h0 = s.hist[4u * tid], h1 = s.hist[4u * tid + 1u], h2 = s.hist[4u * tid + 2u], h3 = s.hist[4u * tid + 3u];
                const uint32_t sum = (h0 + h1) + (h2 + h3);
                uint32_t incl = sum;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d);
                    if ((int)tid >= d) incl += up;
                }
                uint32_t lo = incl - sum;  // ratios in the bins below this lane's
                if (k >= lo && k < incl) {  // one lane: 0 <= k < the ratios that share the prefix
                    uint32_t bin = 4u * tid;
                    const uint32_t h[3] = {h0, h1, h2};
                    bool past = true;  // k lies past every bin so far
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        past = past && k >= lo + h[q];
                        lo += past ? h[q] : 0u;
                        bin += past ? 1u : 0u;
                    }
                    s.sel[0] = prefix << 8 | bin;
                    s.sel[1] = k - lo;
                }
            }
            __syncthreads();
        }
        g = s.sel[0];
        // C
        const float gf = __uint_as_float(g), tg = tol * gf;
        for (uint32_t base = 0u; base < n; base += kThreads) {
            const uint32_t i = base + tid;
            const uint32_t bits = i < n ? row[i] : 0u;
            const bool in = bits != 0u && fabsf(__uint_as_float(bits) - gf) <= tg;
            const uint32_t c = (uint32_t)__popcll(__ballot(in));
            if (first && c) atomicAdd(&s.count[1], c);
        }
        __syncthreads();
    }
    return {m, g, s.count[1]};
}

// TJ-4
__device__ __forceinline__ uint32_t traj_verdict(uint32_t m, uint32_t consistent, uint32_t min_shared, uint32_t permille) {
    return m < min_shared ? kTrajFew : (1000ull * consistent < (unsigned long long)permille * m ? kTrajSpread : kTrajHolds);
}

// grid n_frames - 2 (joint f = blockIdx.x + 1), block kTrajThreads
__global__ __launch_bounds__(kTrajThreads) void k_traj_joint(TrajArgs a) {
    __shared__ TrajSelectLds lds;
    const uint32_t f = blockIdx.x + 1u;
    const uint32_t* const pa = a.poses + (size_t)(f - 1u) * kPoseWords;
    if (pa[15] != ORB_POSE_OK || a.poses[(size_t)f * kPoseWords + 15] != ORB_POSE_OK) return;  // uniform
    const uint32_t nq_prev = min(a.counts[f - 1u], a.cap), nq = min(a.counts[f], a.cap);
    const float r[3] = {__uint_as_float(pa[6]), __uint_as_float(pa[7]), __uint_as_float(pa[8])};
    const float t2 = __uint_as_float(pa[11]);
    const TrajConsensus c = traj_consensus<kTrajThreads>(lds, a.ratios + (size_t)f * a.cap, a.cap, a.tol,
                                                         [&](uint32_t i) { return traj_ratio(a, f, i, nq_prev, nq, r, t2); });
    if (threadIdx.x == 0u) {
        uint32_t* const out = a.joints + (size_t)f * kTrajJointWords;
        out[0] = c.m;
        out[1] = c.g;
        out[2] = c.consistent;
        out[3] = traj_verdict(c.m, c.consistent, a.min_shared, a.permille);
    }
}

// RP-4's step once; M itself when the det is not finite or not > 0
__device__ __forceinline__ void traj_polar_step(float r[9]) {
    float c[9];
    pose_cof(r, c);
    const float det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2];
    const bool ok = isfinite(det) && det > 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const float s = 0.5f * (r[k] + c[k] / det);
        r[k] = ok ? s : r[k];
    }
}

// TJ-5 / BR-4: R = Ra Rb after one polar step (the product itself when its det is not finite or not > 0), t = Ra tb + s ta
__device__ __forceinline__ void traj_compose(const float Ra[9], const float ta[3], float s, const float Rb[9], const float tb[3], float R[9],
                                             float t[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (Ra[3 * r] * Rb[c] + Ra[3 * r + 1] * Rb[3 + c]) + Ra[3 * r + 2] * Rb[6 + c];
        t[r] = ((Ra[3 * r] * tb[0] + Ra[3 * r + 1] * tb[1]) + Ra[3 * r + 2] * tb[2]) + s * ta[r];
    }
    traj_polar_step(R);
}

// the twelve pose words of a record: R[9], t[3]
__device__ __forceinline__ void traj_load_pose(const uint32_t* w, float R[9], float t[3]) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = __uint_as_float(w[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = __uint_as_float(w[9 + k]);
}

__device__ __forceinline__ void traj_store_pose(uint32_t* w, const float R[9], const float t[3]) {
#pragma unroll
    for (int k = 0; k < 9; k++) w[k] = __float_as_uint(R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) w[9 + k] = __float_as_uint(t[k]);
}

__device__ __forceinline__ bool traj_pose_finite(const float R[9], const float t[3]) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) fin = fin && isfinite(R[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && isfinite(t[k]);
    return fin;
}

// grid 1, block 64
__global__ __launch_bounds__(64) void k_traj_chain(TrajArgs a) {
    __shared__ uint32_t s_pose[kTrajChunk * kPoseWords];        // pose[base - 1 + k], k < 64
    __shared__ uint32_t s_joint[kTrajChunk * kTrajJointWords];  // joint[base - 1 + k]
    const uint32_t lane = threadIdx.x, pairs = a.n_frames - 1u;
    float R[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, t[3] = {0.0f, 0.0f, 0.0f};
    float scale = 0.0f;
    uint32_t origin = 0u;
    bool prev_ok = false;  // pose[f - 2] is OK
    if (lane == 0u) {      // frame 0: ORIGIN
        uint32_t* const out = a.frames;
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = __float_as_uint(R[k]);
#pragma unroll
        for (int k = 9; k < 20; k++) out[k] = 0u;
        out[17] = ORB_TRAJ_ORIGIN;
    }
    for (uint32_t base = 1u; base < a.n_frames; base += kTrajChunk) {
        __syncthreads();  // lane 0 is done with the chunk before
        {
            const uint32_t w0 = (base - 1u) * kPoseWords, wn = pairs * kPoseWords;
#pragma unroll
            for (uint32_t k = 0u; k < kPoseWords; k++) {
                const uint32_t w = k * 64u + lane;
                s_pose[w] = w0 + w < wn ? a.poses[w0 + w] : 0u;
            }
            // joint rows 1 .. n_frames - 2 are written (those that were evaluated); the others are never used
            const uint32_t j0 = (base - 1u) * kTrajJointWords, jn = pairs * kTrajJointWords;
#pragma unroll
            for (uint32_t k = 0u; k < kTrajJointWords; k++) {
                const uint32_t w = k * 64u + lane;
                s_joint[w] = j0 + w < jn ? a.joints[j0 + w] : 0u;
            }
        }
        __syncthreads();
        const uint32_t end = min(base + kTrajChunk, a.n_frames);
#pragma unroll 1
        for (uint32_t f = base; lane == 0u && f < end; f++) {
            const uint32_t* const P = s_pose + (f - base) * kPoseWords;
            const uint32_t* const J = s_joint + (f - base) * kTrajJointWords;
            float pr[9], pt[3];
            traj_load_pose(P, pr, pt);
            const bool ok = P[15] == ORB_POSE_OK;
            uint32_t status, shared = 0u, consistent = 0u;
            float step = 0.0f;
            if (!ok) {
                status = ORB_TRAJ_LOST;
            } else if (!prev_ok) {
                status = ORB_TRAJ_START;
            } else {
                shared = J[0];
                consistent = J[2];
                const float g = __uint_as_float(J[1]);
                status = J[3] == kTrajHolds ? ORB_TRAJ_CHAINED : (J[3] == kTrajFew ? ORB_TRAJ_RESTART_FEW : ORB_TRAJ_RESTART_SPREAD);
                step = J[3] == kTrajFew ? 0.0f : g;
            }
            if (status == ORB_TRAJ_CHAINED) {
                scale = scale * step;
                float M[9], u[3];
                traj_compose(pr, pt, scale, R, t, M, u);  // TJ-5
#pragma unroll
                for (int k = 0; k < 9; k++) R[k] = M[k];
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = u[k];
            } else {
                const bool lost = status == ORB_TRAJ_LOST;
#pragma unroll
                for (int k = 0; k < 9; k++) R[k] = lost ? ((k & 3) == 0 ? 1.0f : 0.0f) : pr[k];
#pragma unroll
                for (int k = 0; k < 3; k++) t[k] = lost ? 0.0f : pt[k];
                scale = lost ? 0.0f : 1.0f;
                origin = lost ? f : f - 1u;
            }
            prev_ok = ok;
            uint32_t* const out = a.frames + (size_t)f * kTrajFrameWords;
            traj_store_pose(out, R, t);
            out[12] = __float_as_uint(scale);
            out[13] = __float_as_uint(step);
            out[14] = origin;
            out[15] = shared;
            out[16] = consistent;
            out[17] = status;
            out[18] = 0u;
            out[19] = 0u;
        }
    }
}

// grid (n_frames - 1, ceil(cap / kTrajThreads)), block kTrajThreads
__global__ __launch_bounds__(kTrajThreads) void k_traj_map(TrajArgs a) {
    const uint32_t f = blockIdx.x, i = blockIdx.y * kTrajThreads + threadIdx.x;
    if (i >= a.cap) return;
    const uint32_t* const cur = a.frames + (size_t)f * kTrajFrameWords;
    const uint32_t* const nxt = cur + kTrajFrameWords;
    const uint32_t status = nxt[17];
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (status != ORB_TRAJ_LOST) {  // uniform
        const float4 X = a.points[(size_t)f * a.cap + i];
        if (nxt[14] == f) {
            out = X;
        } else if (__float_as_uint(X.w) & ORB_POINT_GOOD) {
            const float s = __uint_as_float(nxt[12]);
            float R[9];
#pragma unroll
            for (int k = 0; k < 9; k++) R[k] = __uint_as_float(cur[k]);
            const float v0 = s * X.x - __uint_as_float(cur[9]), v1 = s * X.y - __uint_as_float(cur[10]), v2 = s * X.z - __uint_as_float(cur[11]);
            out.x = (R[0] * v0 + R[3] * v1) + R[6] * v2;
            out.y = (R[1] * v0 + R[4] * v1) + R[7] * v2;
            out.z = (R[2] * v0 + R[5] * v1) + R[8] * v2;
            out.w = X.w;
        }
    }
    a.map[(size_t)f * a.cap + i] = out;
}

}  // namespace orb
