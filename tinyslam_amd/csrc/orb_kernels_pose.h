// orb_kernels_pose.h -- relative pose and triangulation of the epipolar inliers of consecutive frames (not in the reference; the
// definition is the build's own, RP-1..RP-7 in DESIGN.md section 19): the pair's fundamental matrix from the last
// orb_verify_epipolar and the caller's pinhole intrinsics give the essential matrix; its baseline direction and its two rotations
// come in closed form (Horn 1990: t from I - E E^T, R = Cof(E) -+ [t]x E, three polar steps towards the nearest rotation; no SVD, no
// loop whose length depends on the data); every inlier is triangulated under the four (R, t) candidates and the one with the most
// points in front of both cameras and within the reprojection bound wins.  Every binary32 operation below is written out in the
// order the definition gives (-ffp-contract=off, correctly rounded division and square root), so the CPU restatement
// (tests/pose_ref.py) reproduces every bit.
//
//   k_pose_count    grid (pairs, ceil(cap / 1024)), 1024 threads: thread 0 rebuilds the candidates into LDS (about 300 operations:
//                   cheaper than a launch of its own and a round trip through memory), every thread takes one query and evaluates
//                   the four candidates on it, the counts go through wave ballots and one integer atomicAdd per wave and counter
//                   (integer sums do not depend on the order)
//   k_pose_points   the same grid: the candidates again (the same operations, the same bits), the winner and the status from the
//                   counters, the OrbPairPose by block 0 of the pair, an OrbPoint per query in one 16-byte store
#pragma once
#include "orb_kernels_verify.h"

namespace orb {

constexpr uint32_t kPoseThreads = 1024u;
constexpr uint32_t kPoseCounters = 12u;   // per pair: good[4], parallax[4] (good points that have it), inliers, three spare
constexpr uint32_t kPoseMinInliers = 8u;  // RP-6: fewer epipolar inliers than the eight-point sample that made F
constexpr uint32_t kPoseWords = 16u;      // OrbPairPose

struct PoseArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    const CornerData* corners;   // [frames][cap]
    const MatchRecord* matches;  // [frames][cap]
    uint32_t cap;
    const uint32_t* vmodel;      // [pairs][16] OrbPairModel of the last epipolar verification
    const uint8_t* vmask;        // [pairs][cap] its inlier bytes
    float fx, fy, cx, cy;        // RP-1: intrinsics
    float r2;                    // RP-5: max_reproj_px squared
    float c2;                    // RP-5: max_cos_parallax squared
    uint32_t min_good;           // RP-6
    uint32_t permille;           // RP-6
    uint32_t* counters;          // [pairs][kPoseCounters], zeroed before k_pose_count
    uint32_t* poses;             // [pairs][kPoseWords]
    float4* points;              // [pairs][cap]
};

// The candidates of a pair as one lane leaves them in LDS
struct PoseCandidates {
    float ra[9], rb[9], t[3];
    uint32_t valid;  // bit 0: Ra is a rotation, bit 1: Rb is; 0: no model (RP-1..RP-4)
};

// rows m1 x m2, m2 x m0, m0 x m1 of a row-major 3 x 3
__device__ __forceinline__ void pose_cof(const float m[9], float c[9]) {
    c[0] = m[4] * m[8] - m[5] * m[7];
    c[1] = m[5] * m[6] - m[3] * m[8];
    c[2] = m[3] * m[7] - m[4] * m[6];
    c[3] = m[7] * m[2] - m[8] * m[1];
    c[4] = m[8] * m[0] - m[6] * m[2];
    c[5] = m[6] * m[1] - m[7] * m[0];
    c[6] = m[1] * m[5] - m[2] * m[4];
    c[7] = m[2] * m[3] - m[0] * m[5];
    c[8] = m[0] * m[4] - m[1] * m[3];
}

// RP-4: three steps R <- 0.5 (R + Cof(R) / det R); false when a det is not finite or not > 0
__device__ __forceinline__ bool pose_polar(float r[9]) {
    bool ok = true;
#pragma unroll
    for (int s = 0; s < 3; s++) {
        float c[9];
        pose_cof(r, c);
        const float det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2];
        ok = ok && isfinite(det) && det > 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) r[k] = 0.5f * (r[k] + c[k] / det);
    }
    return ok;
}

// RP-1..RP-4 on one lane.  v: the pair's OrbPairModel.
__device__ __forceinline__ void pose_candidates(const uint32_t* __restrict__ v, const PoseArgs& a, PoseCandidates& out) {
    out.valid = 0u;
    const uint32_t st = v[12];
    if (!(st == ORB_VERIFY_OK || st == ORB_VERIFY_MINIMAL)) return;
    float f[9], g[9], e[9];
#pragma unroll
    for (int k = 0; k < 9; k++) f[k] = __uint_as_float(v[k]);
    // RP-2: G = F K, E = K^T G
#pragma unroll
    for (int r = 0; r < 3; r++) {
        g[3 * r] = f[3 * r] * a.fx;
        g[3 * r + 1] = f[3 * r + 1] * a.fy;
        g[3 * r + 2] = (f[3 * r] * a.cx + f[3 * r + 1] * a.cy) + f[3 * r + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        e[c] = a.fx * g[c];
        e[3 + c] = a.fy * g[3 + c];
        e[6 + c] = (a.cx * g[c] + a.cy * g[3 + c]) + g[6 + c];
    }
    float s = e[0] * e[0];
#pragma unroll
    for (int k = 1; k < 9; k++) s = s + e[k] * e[k];
    const float n = sqrtf(0.5f * s);
    if (!(isfinite(n) && n > 0.0f)) return;
#pragma unroll
    for (int k = 0; k < 9; k++) e[k] = e[k] / n;
    // RP-3: T = I - E E^T, the row of its largest diagonal entry
    float T[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            T[3 * i + j] = (i == j ? 1.0f : 0.0f) - ((e[3 * i] * e[3 * j] + e[3 * i + 1] * e[3 * j + 1]) + e[3 * i + 2] * e[3 * j + 2]);
    float best = T[0], t0 = T[0], t1 = T[1], t2 = T[2];
    const bool g1 = T[4] > best;
    best = g1 ? T[4] : best;
    t0 = g1 ? T[3] : t0;
    t1 = g1 ? T[4] : t1;
    t2 = g1 ? T[5] : t2;
    const bool g2 = T[8] > best;
    best = g2 ? T[8] : best;
    t0 = g2 ? T[6] : t0;
    t1 = g2 ? T[7] : t1;
    t2 = g2 ? T[8] : t2;
    if (!(best > 0.0f)) return;
    const float q = sqrtf(best);
    t0 = t0 / q;
    t1 = t1 / q;
    t2 = t2 / q;
    // RP-4: C = Cof(E), S = [t]x E (column by column t x E[:, c]), Ra = C - S, Rb = C + S
    float C[9], S[9];
    pose_cof(e, C);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        S[c] = t1 * e[6 + c] - t2 * e[3 + c];
        S[3 + c] = t2 * e[c] - t0 * e[6 + c];
        S[6 + c] = t0 * e[3 + c] - t1 * e[c];
    }
#pragma unroll
    for (int k = 0; k < 9; k++) {
        out.ra[k] = C[k] - S[k];
        out.rb[k] = C[k] + S[k];
    }
    const bool va = pose_polar(out.ra), vb = pose_polar(out.rb);
    out.t[0] = t0;
    out.t[1] = t1;
    out.t[2] = t2;
    out.valid = (va ? 1u : 0u) | (vb ? 2u : 0u);
}

// RP-5: a correspondence's rays, and what the two signs of t share under one rotation
struct PoseRay {
    float d1x, d1y, d2x, d2y, u2, v2, bb;
    float ax, ay, az, aa, ab, det;
};

__device__ __forceinline__ void pose_ray(const float r[9], PoseRay& p) {
    p.ax = (r[0] * p.d1x + r[1] * p.d1y) + r[2];
    p.ay = (r[3] * p.d1x + r[4] * p.d1y) + r[5];
    p.az = (r[6] * p.d1x + r[7] * p.d1y) + r[8];
    p.aa = (p.ax * p.ax + p.ay * p.ay) + p.az * p.az;
    p.ab = (p.ax * p.d2x + p.ay * p.d2y) + p.az;
    p.det = p.aa * p.bb - p.ab * p.ab;
}

// RP-5 under (R, t): Cramer's rule on the normal equations of z1 a - z2 d2 = -t, the point X = z1 d1, its reprojection into frame
// f + 1.  Returns good.
__device__ __forceinline__ bool pose_point(const float r[9], float t0, float t1, float t2, const PoseRay& p, const PoseArgs& a, float X[3]) {
    const float at = (p.ax * t0 + p.ay * t1) + p.az * t2;
    const float bt = (p.d2x * t0 + p.d2y * t1) + t2;
    const float z1 = (p.ab * bt - at * p.bb) / p.det;
    const float z2 = (p.aa * bt - p.ab * at) / p.det;
    X[0] = z1 * p.d1x;
    X[1] = z1 * p.d1y;
    X[2] = z1;
    const float yx = ((r[0] * X[0] + r[1] * X[1]) + r[2] * X[2]) + t0;
    const float yy = ((r[3] * X[0] + r[4] * X[1]) + r[5] * X[2]) + t1;
    const float yz = ((r[6] * X[0] + r[7] * X[1]) + r[8] * X[2]) + t2;
    const float ex = (a.fx * (yx / yz) + a.cx) - p.u2;
    const float ey = (a.fy * (yy / yz) + a.cy) - p.v2;
    const float err2 = ex * ex + ey * ey;
    return isfinite(z1) && isfinite(z2) && z1 > 0.0f && z2 > 0.0f && err2 <= a.r2;
}

// RP-5: the rays' angle is large enough to fix a depth
__device__ __forceinline__ bool pose_parallax(const PoseRay& p, const PoseArgs& a) {
    return p.ab <= 0.0f || p.ab * p.ab < a.c2 * (p.aa * p.bb);
}

// RP-1: query i of the pair is a correspondence iff its inlier byte is 1 (then the matcher's index is a stored keypoint of f + 1);
// its rays
__device__ __forceinline__ bool pose_correspondence(const PoseArgs& a, uint32_t pair, uint32_t i, PoseRay& p) {
    const uint32_t nq = min(a.counts[pair], a.cap), nt = min(a.counts[pair + 1u], a.cap);
    if (i >= nq || a.vmask[(size_t)pair * a.cap + i] != 1u) return false;
    const uint32_t j = a.matches[(size_t)pair * a.cap + i].index;
    if (j >= nt) return false;
    const CornerData c1 = a.corners[(size_t)pair * a.cap + i], c2 = a.corners[(size_t)(pair + 1u) * a.cap + j];
    const float s1 = (float)(1u << (c1.octave & 31u)), s2 = (float)(1u << (c2.octave & 31u));
    const float u1 = ((float)c1.x + 0.5f) * s1 - 0.5f, v1 = ((float)c1.y + 0.5f) * s1 - 0.5f;
    p.u2 = ((float)c2.x + 0.5f) * s2 - 0.5f;
    p.v2 = ((float)c2.y + 0.5f) * s2 - 0.5f;
    p.d1x = (u1 - a.cx) / a.fx;
    p.d1y = (v1 - a.cy) / a.fy;
    p.d2x = (p.u2 - a.cx) / a.fx;
    p.d2y = (p.v2 - a.cy) / a.fy;
    p.bb = (p.d2x * p.d2x + p.d2y * p.d2y) + 1.0f;
    return true;
}

// the candidates of the workgroup's pair, built by thread 0 and handed to every thread
__device__ __forceinline__ void pose_share(const PoseArgs& a, uint32_t pair, PoseCandidates& mine) {
    __shared__ PoseCandidates cand;
    if (threadIdx.x == 0u) pose_candidates(a.vmodel + (size_t)pair * kVerifyModelWords, a, cand);
    __syncthreads();
    mine = cand;
}

// grid (pairs, ceil(cap / kPoseThreads)), block kPoseThreads
__global__ __launch_bounds__(kPoseThreads) void k_pose_count(PoseArgs a) {
    const uint32_t pair = blockIdx.x, i = blockIdx.y * kPoseThreads + threadIdx.x;
    PoseCandidates c;
    pose_share(a, pair, c);
    if (c.valid == 0u) return;  // uniform: k_pose_points reads no counter of such a pair
    PoseRay p;
    const bool is = i < a.cap && pose_correspondence(a, pair, i, p);
    bool good[4] = {false, false, false, false}, par[4] = {false, false, false, false};
    if (is) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const float* const r = h ? c.rb : c.ra;
            pose_ray(r, p);
            const bool has = pose_parallax(p, a);
            const bool valid = (c.valid >> h & 1u) != 0u;
            float X[3];
            good[2 * h] = valid && pose_point(r, c.t[0], c.t[1], c.t[2], p, a, X);
            good[2 * h + 1] = valid && pose_point(r, -c.t[0], -c.t[1], -c.t[2], p, a, X);
            par[2 * h] = good[2 * h] && has;
            par[2 * h + 1] = good[2 * h + 1] && has;
        }
    }
    uint32_t* const out = a.counters + (size_t)pair * kPoseCounters;
    const bool first = (threadIdx.x & 63u) == 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t ng = (uint32_t)__popcll(__ballot(good[k])), np = (uint32_t)__popcll(__ballot(par[k]));
        if (first && ng) atomicAdd(out + k, ng);
        if (first && np) atomicAdd(out + 4 + k, np);
    }
    const uint32_t ni = (uint32_t)__popcll(__ballot(is));
    if (first && ni) atomicAdd(out + 8, ni);
}

// grid (pairs, ceil(cap / kPoseThreads)), block kPoseThreads
__global__ __launch_bounds__(kPoseThreads) void k_pose_points(PoseArgs a) {
    const uint32_t pair = blockIdx.x, i = blockIdx.y * kPoseThreads + threadIdx.x;
    PoseCandidates c;
    pose_share(a, pair, c);
    const uint32_t* const cnt = a.counters + (size_t)pair * kPoseCounters;
    // RP-6: the winner is the first of the largest good count among the candidates whose rotation is valid
    uint32_t status = ORB_POSE_NOMODEL, win = 0u, best = 0u, second = 0u, inliers = 0u;
    bool written = false;
    if (c.valid != 0u) {
        inliers = cnt[8];
        if (inliers < kPoseMinInliers) {
            status = ORB_POSE_FEW;
        } else {
            int bk = -1;
            uint32_t good[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                good[k] = cnt[k];  // 0 for a candidate whose rotation is invalid
                const bool valid = (c.valid >> (k >> 1) & 1u) != 0u;
                if (valid && (bk < 0 || good[k] > best)) {
                    bk = k;
                    best = good[k];
                }
            }
            win = (uint32_t)bk;
#pragma unroll
            for (int k = 0; k < 4; k++) second = (uint32_t)k != win && good[k] > second ? good[k] : second;
            const uint32_t wpar = cnt[4u + win];
            written = true;
            if (best < a.min_good)
                status = ORB_POSE_FEW;
            else if (1000ull * second >= (unsigned long long)a.permille * best)
                status = ORB_POSE_AMBIGUOUS;
            else if (2ull * wpar < best)
                status = ORB_POSE_LOW_PARALLAX;
            else
                status = ORB_POSE_OK;
        }
    }
    const bool second_rot = (win >> 1) != 0u;
    float r[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) r[k] = second_rot ? c.rb[k] : c.ra[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (win & 1u) ? -c.t[k] : c.t[k];
    if (blockIdx.y == 0u && threadIdx.x == 0u) {  // RP-7: the record
        uint32_t* const out = a.poses + (size_t)pair * kPoseWords;
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = written ? __float_as_uint(r[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) out[9 + k] = written ? __float_as_uint(t[k]) : 0u;
        out[12] = written ? inliers : 0u;
        out[13] = written ? best : 0u;
        out[14] = written ? second : 0u;
        out[15] = status;
    }
    if (i >= a.cap) return;
    float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    PoseRay p;
    if (written && pose_correspondence(a, pair, i, p)) {
        pose_ray(r, p);
        float X[3];
        if (pose_point(r, t[0], t[1], t[2], p, a, X)) {
            const bool has = pose_parallax(p, a);
            pt = make_float4(X[0], X[1], X[2], __uint_as_float(ORB_POINT_GOOD | (has ? ORB_POINT_PARALLAX : 0u)));
        }
    }
    a.points[(size_t)pair * a.cap + i] = pt;
}

}  // namespace orb
