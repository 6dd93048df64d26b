// orb_kernels_adjust.h -- poses and landmarks refined by reprojection (not in the reference; the definition is the build's own,
// BA-1..BA-7 in DESIGN.md section 24).  Every frame pose of orb_trajectory_consecutive is a product of two-view poses, and
// orb_landmarks_consecutive places its points under those poses without moving one.  Here the two halves that exist already are
// alternated (resection-intersection, bundle adjustment by block coordinate descent): a Gauss-Newton step of section 21 on every
// free camera over the landmarks its keypoints own, then section 22's point nearest to all rays for every landmark under the new
// poses, `rounds` times; a closing pass evaluates the cost and checks every landmark again.  The first two cameras of a segment are
// held, which fixes the gauge.  Every binary32 operation below is written out in the order the definition gives
// (-ffp-contract=off, correctly rounded division, no square root), so the CPU restatement (tests/adjust_ref.py) reproduces every bit.
// LO-6's sums and update, GV-6's solver and RP-4's cofactors are the functions of orb_kernels_localize.h, orb_kernels_verify.h and
// orb_kernels_pose.h, and a view is section 22's LmView.  LM-4's sums and LM-5's check stay here as lambdas: in
// orb_kernels_landmark.h they are lambdas of k_lm_fuse, not functions, and made into functions there they change that kernel's code.
//
//   k_ba_index      grid (frames, ceil(cap / 256)): a thread per landmark slot; a GOOD landmark walks its views and puts its key
//                   p * cap + i on every registered one with an integer atomicMin (the owners are set to 0xffffffff by a memset
//                   before: no result depends on an order); the initial X of every slot; thread 0 of a frame's first block copies
//                   the frame's pose into its OrbAdjustedPose, which holds the current pose from then on
//   k_ba_motion     one workgroup of 256 per frame: slot k of a free frame into partial k mod 256 in ascending k, the 28 sums in
//                   LDS through GV-6's tree, the 6 x 7 solve, the update and two polar steps on one lane; mode 1 is round 1 (the
//                   observations, FEW, cost_before), mode 2 the closing pass (cost_after only)
//   k_ba_structure  grid (pairs, ceil(cap / 256)): a thread per slot; a participating landmark walks its views under the current
//                   poses (LM-4) and keeps its X when the result is unsolved; the threads of a workgroup step through the same
//                   frames, so the pose reads are uniform
//   k_ba_check      grid (frames, ceil(cap / 256)): LM-5 under the final poses and the OrbLandmark of every slot (a copy for a slot
//                   that does not take part, zeros in the last frame's row)
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_landmark.h"
#include "orb_kernels_localize.h"

namespace orb {

constexpr uint32_t kBaThreads = 256u;    // verify_solve_n reads the sums of [sum][256] partials
constexpr uint32_t kBaFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kBaPoseWords = 16u;   // OrbAdjustedPose: r[9], t[3], cost_before, cost_after, observations, status
constexpr uint32_t kBaSums = 28u;        // BA-4: LO-6's 27 and the cost
constexpr uint32_t kBaMinObs = 6u;       // BA-4: fewer owned slots give FEW
constexpr uint32_t kBaNone = 0xffffffffu;
constexpr uint32_t kBaDead = 4u;         // inside a call: a free frame whose record is not finite (FAILED in the output)
constexpr uint32_t kBaStep = 0u, kBaFirst = 1u, kBaClose = 2u;  // k_ba_motion's modes

struct BaArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    const CornerData* corners;   // [frames][cap]
    const MatchRecord* matches;  // [frames][cap]
    uint32_t cap;
    uint32_t n_frames;
    const uint32_t* frames;      // [frames][kBaFrameWords] of the last orb_trajectory_consecutive
    const float4* lms;           // [pairs][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    float fx, fy, cx, cy;        // BA-1: intrinsics
    float r2;                    // BA-6: max_reproj_px squared
    uint32_t* owner;             // [frames][cap] BA-3: the key p * cap + i of the slot's owner, kBaNone: none
    float4* X;                   // [pairs][cap] the current point of slot (p, i); w: 1 iff the landmark takes part
    uint32_t* pose;              // [frames][kBaPoseWords] OrbAdjustedPose, the current poses
    float4* out;                 // [frames][cap][2] OrbLandmark
};

__device__ __forceinline__ uint32_t ba_nq(const BaArgs& a, uint32_t g) { return min(a.counts[g], a.cap); }

// orb_corner_level0_xy of keypoint k of frame g
__device__ __forceinline__ void ba_keypoint(const BaArgs& a, uint32_t g, uint32_t k, float& u, float& v) {
    const CornerData c = a.corners[(size_t)g * a.cap + k];
    const float s = (float)(1u << (c.octave & 31u));
    u = ((float)c.x + 0.5f) * s - 0.5f;
    v = ((float)c.y + 0.5f) * s - 0.5f;
}

// grid (n_frames, ceil(cap / kBaThreads)), block kBaThreads; the owners are set to kBaNone by a memset before
__global__ __launch_bounds__(kBaThreads) void k_ba_index(BaArgs a) {
    const uint32_t p = blockIdx.x, i = blockIdx.y * kBaThreads + threadIdx.x;
    if (blockIdx.y == 0u && threadIdx.x == 0u) {  // BA-2, BA-7: frame p's record
        const uint32_t* const rec = a.frames + (size_t)p * kBaFrameWords;
        uint32_t* const out = a.pose + (size_t)p * kBaPoseWords;
        const bool is_free = rec[17] == ORB_TRAJ_CHAINED;
        bool fin = true;
#pragma unroll
        for (int q = 0; q < 12; q++) fin = fin && isfinite(__uint_as_float(rec[q]));
        const bool dead = is_free && !fin;
#pragma unroll
        for (int q = 0; q < 12; q++) out[q] = dead ? 0u : rec[q];
        out[12] = out[13] = out[14] = 0u;
        out[15] = !is_free ? (uint32_t)ORB_ADJUST_HELD : dead ? kBaDead : (uint32_t)ORB_ADJUST_REFINED;
    }
    if (p + 1u >= a.n_frames || i >= a.cap) return;
    const size_t slot = (size_t)p * a.cap + i;
    const float4 lo = a.lms[2u * slot], hi = a.lms[2u * slot + 1u];
    const uint32_t views = __float_as_uint(hi.x) & 0xffffu, o = __float_as_uint(hi.y);
    const bool part = views != 0u && (__float_as_uint(lo.w) & ORB_POINT_GOOD) != 0u && p + views <= a.n_frames;  // BA-3
    a.X[slot] = make_float4(lo.x, lo.y, lo.z, __uint_as_float(part ? 1u : 0u));
    if (!part) return;
    uint32_t k = i;
    for (uint32_t s = 0u; s < views; s++) {
        const uint32_t g = p + s;  // <= n_frames - 1
        if (k >= ba_nq(a, g)) break;
        const uint32_t* const rec = a.frames + (size_t)g * kBaFrameWords;
        if (rec[17] == ORB_TRAJ_CHAINED && rec[14] == o) atomicMin(&a.owner[(size_t)g * a.cap + k], (uint32_t)slot);
        if (s + 1u < views) k = a.matches[(size_t)g * a.cap + k].index;  // g <= n_frames - 2
    }
}

// BA-7: a cost as it is written
__device__ __forceinline__ uint32_t ba_cost_bits(float c) { return __float_as_uint(isfinite(c) ? c : 3.402823466e+38f); }

// grid (n_frames), block kBaThreads
__global__ __launch_bounds__(kBaThreads) void k_ba_motion(BaArgs a, uint32_t mode) {
    __shared__ float part[kBaSums][kBaThreads];  // [sum][thread]: conflict-free columns
    __shared__ float aug[6][7];
    __shared__ float sol[6];
    __shared__ uint32_t s_count;
    const uint32_t g = blockIdx.x, tid = threadIdx.x;
    uint32_t* const rec = a.pose + (size_t)g * kBaPoseWords;
    const uint32_t st = rec[15];
    const bool dead = st == kBaDead;
    if (!(st == ORB_ADJUST_REFINED || (mode == kBaClose && (st == ORB_ADJUST_FAILED || dead)))) return;  // uniform
    if (tid == 0u) s_count = 0u;
    float R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = __uint_as_float(rec[e]);
#pragma unroll
    for (int e = 0; e < 3; e++) t[e] = __uint_as_float(rec[9 + e]);
    __syncthreads();
    const uint32_t n = ba_nq(a, g);
    const uint32_t* const owner = a.owner + (size_t)g * a.cap;
    float acc[kBaSums];
#pragma unroll
    for (uint32_t e = 0; e < kBaSums; e++) acc[e] = 0.0f;
    uint32_t cnt = 0u;
    for (uint32_t k = tid; k < n; k += kBaThreads) {  // BA-4: slot k into partial sum k mod 256, ascending k
        const uint32_t key = owner[k];
        if (key == kBaNone) continue;
        cnt++;
        if (dead) continue;
        const float4 Y = a.X[key];
        float u2, v2;
        ba_keypoint(a, g, k, u2, v2);
        acc[27] = acc[27] + loc_accumulate(acc, R, t, Y, u2, v2, a);  // LO-6's 27 sums and the cost
    }
    if (cnt) atomicAdd(&s_count, cnt);
#pragma unroll
    for (uint32_t e = 0; e < kBaSums; e++) part[e][tid] = acc[e];
    __syncthreads();
    for (uint32_t s = 128u; s >= 1u; s >>= 1) {  // pairwise tree, strides 128 .. 1
        if (tid < s)
            for (uint32_t e = 0; e < kBaSums; e++) part[e][tid] = part[e][tid] + part[e][tid + s];
        __syncthreads();
    }
    if (tid != 0u) return;
    const uint32_t obs = s_count;
    if (mode == kBaClose) {
        if (dead) {
            rec[14] = obs;
            rec[15] = ORB_ADJUST_FAILED;
        } else {
            rec[13] = ba_cost_bits(part[27][0]);
        }
        return;
    }
    if (mode == kBaFirst) {
        rec[14] = obs;
        if (obs < kBaMinObs) {
            rec[15] = ORB_ADJUST_FEW;
            return;
        }
        rec[12] = ba_cost_bits(part[27][0]);
    }
    uint32_t ok = verify_solve_n<6>(part, aug, sol);
    if (ok) ok = loc_update(sol, R, t) ? 1u : 0u;
    if (ok) {
#pragma unroll
        for (int e = 0; e < 9; e++) rec[e] = __float_as_uint(R[e]);
#pragma unroll
        for (int e = 0; e < 3; e++) rec[9 + e] = __float_as_uint(t[e]);
    } else {
        rec[15] = ORB_ADJUST_FAILED;  // BA-4: the pose of before this step stays, and the frame is held from here on
    }
}

// BA-3: the views of the participating landmark (p, i) in ascending frame order, `f(view)` on each, as lm_walk's but under camera
// g's current pose in the segment of origin o (LM-2); p + views <= n_frames
template <class Fn>
__device__ __forceinline__ void ba_walk(const BaArgs& a, uint32_t p, uint32_t i, uint32_t views, uint32_t o, Fn&& f) {
    uint32_t k = i;
    for (uint32_t s = 0u; s < views; s++) {
        const uint32_t g = p + s;
        if (k >= ba_nq(a, g)) break;
        const uint32_t* const rec = a.pose + (size_t)g * kBaPoseWords;
        const bool own = g == o;  // the origin's own record belongs to the segment before it
        LmView w;
#pragma unroll
        for (int q = 0; q < 9; q++) w.R[q] = own ? ((q & 3) == 0 ? 1.0f : 0.0f) : __uint_as_float(rec[q]);
#pragma unroll
        for (int q = 0; q < 3; q++) w.t[q] = own ? 0.0f : __uint_as_float(rec[9 + q]);
        ba_keypoint(a, g, k, w.u, w.v);
        f(w);
        if (s + 1u < views) k = a.matches[(size_t)g * a.cap + k].index;  // g <= n_frames - 2
    }
}

// grid (n_frames - 1, ceil(cap / kBaThreads)), block kBaThreads
__global__ __launch_bounds__(kBaThreads) void k_ba_structure(BaArgs a) {
    const uint32_t p = blockIdx.x, i = blockIdx.y * kBaThreads + threadIdx.x;
    if (i >= a.cap) return;
    const size_t slot = (size_t)p * a.cap + i;
    const float4 X = a.X[slot];
    if (!(__float_as_uint(X.w) & 1u)) return;
    const float4 hi = a.lms[2u * slot + 1u];
    const uint32_t views = __float_as_uint(hi.x) & 0xffffu, o = __float_as_uint(hi.y);
    // LM-4
    float A00 = 0.0f, A01 = 0.0f, A02 = 0.0f, A11 = 0.0f, A12 = 0.0f, A22 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    ba_walk(a, p, i, views, o, [&](const LmView& w) {
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
    if (solved) a.X[slot] = make_float4(X0, X1, X2, X.w);  // BA-5: an unsolved landmark keeps its X
}

// grid (n_frames, ceil(cap / kBaThreads)), block kBaThreads
__global__ __launch_bounds__(kBaThreads) void k_ba_check(BaArgs a) {
    const uint32_t p = blockIdx.x, i = blockIdx.y * kBaThreads + threadIdx.x;
    if (i >= a.cap) return;
    const size_t slot = (size_t)p * a.cap + i;
    float4* const out = a.out + 2u * slot;
    if (p + 1u >= a.n_frames) {  // uniform: the last frame starts no pair
        out[0] = out[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 lo = a.lms[2u * slot], hi = a.lms[2u * slot + 1u];
    const float4 X = a.X[slot];
    if (!(__float_as_uint(X.w) & 1u)) {  // BA-7: byte for byte
        out[0] = lo;
        out[1] = hi;
        return;
    }
    const uint32_t views = __float_as_uint(hi.x) & 0xffffu, o = __float_as_uint(hi.y);
    uint32_t inliers = 0u;
    ba_walk(a, p, i, views, o, [&](const LmView& w) {  // LM-5
        const float yx = ((w.R[0] * X.x + w.R[1] * X.y) + w.R[2] * X.z) + w.t[0];
        const float yy = ((w.R[3] * X.x + w.R[4] * X.y) + w.R[5] * X.z) + w.t[1];
        const float yz = ((w.R[6] * X.x + w.R[7] * X.y) + w.R[8] * X.z) + w.t[2];
        const float ex = a.fx * yx + (a.cx - w.u) * yz;
        const float ey = a.fy * yy + (a.cy - w.v) * yz;
        inliers += (yz > 0.0f && ex * ex + ey * ey <= a.r2 * (yz * yz)) ? 1u : 0u;
    });
    const uint32_t flags = inliers == views ? (ORB_POINT_GOOD | (__float_as_uint(lo.w) & ORB_POINT_PARALLAX)) : 0u;
    out[0] = make_float4(X.x, X.y, X.z, __uint_as_float(flags));
    out[1] = make_float4(__uint_as_float(views | inliers << 16), hi.y, hi.z, hi.w);
}

}  // namespace orb
