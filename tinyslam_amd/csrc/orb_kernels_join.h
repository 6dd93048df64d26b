// orb_kernels_join.h -- trajectory segments joined through loop fixes (not in the reference; the definition is the build's own,
// SJ-1..SJ-7 in DESIGN.md section 30).  An OrbLoopFix whose query q lies in segment b and whose target T lies in segment o gives
// camera q in o's frame and unit; the trajectory gives camera q in b's.  An inlier keypoint of q that a landmark of o owns through
// T and a landmark of b owns directly has two depths in camera q, one in each unit: the lower median of their ratios is the scale
// between the segments, the two poses of camera q the rotation and translation.  Every segment takes its best link to an earlier
// one, the links are chained, and every frame is written in the frame and unit of its root.  Every binary32 operation below is
// written out in the order the definition gives (-ffp-contract=off, correctly rounded division), so the CPU restatement
// (tests/join_ref.py) reproduces every bit.
//
//   k_lc_index   of orb_kernels_loop.h, as it is, on an LcArgs of this stage's owner buffer (set to 0xffffffff by a memset) (SJ-2)
//   k_sj_ratio   one workgroup of 256 per list entry: SJ-3's verdict (uniform), then traj_consensus of orb_kernels_traj.h over the
//                query's slots (sj_ratio), then, on one lane, traj_verdict as a link verdict, SJ-4, the link record and SJ-5's
//                atomicMax on the segment's 64-bit key; integer atomics only, no result depends on an order
//   k_sj_chain   one wave: the lanes mark the origins, lane 0 walks the frame slots in ascending order and writes SJ-6's table
//                (traj_compose)
//   k_sj_write   a thread per frame: the OrbJoinPose records (traj_compose)
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_loop.h"

namespace orb {

constexpr uint32_t kSjThreads = 256u;
constexpr uint32_t kSjFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kSjFixWords = 32u;    // OrbLoopFix
constexpr uint32_t kSjPoseWords = 16u;   // OrbJoinPose
constexpr uint32_t kSjSegWords = 16u;    // OrbJoinSegment
constexpr uint32_t kSjLinkWords = 8u;    // OrbJoinLink
constexpr uint32_t kSjNone = 0xffffffffu;
// SJ-3's verdicts (ORB_JOIN_LINK_*)
constexpr uint32_t kSjHolds = 0u, kSjStatus = 1u, kSjFew = 2u, kSjRange = 3u, kSjSame = 4u, kSjForward = 5u, kSjNonfinite = 6u, kSjRatioFew = 7u,
                   kSjRatioSpread = 8u;
constexpr uint32_t kSjSegNone = 0u, kSjSegRoot = 1u, kSjSegLinked = 2u;  // OrbJoinSegment.status
constexpr uint32_t kSjCopied = 0u, kSjMoved = 1u;                        // OrbJoinPose.status

struct SjArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    uint32_t cap;
    const uint2* list;           // [entries] OrbFramePair of the last orb_match_pairs
    const MatchRecord* rows;     // [entries][cap] its rows
    const uint32_t* frames;      // [F][kSjFrameWords] of the last orb_trajectory_consecutive
    const float4* lms;           // [L - 1][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    const uint32_t* fixes;       // [entries][kSjFixWords] of the last orb_loop_pairs
    const uint8_t* mask;         // [entries][cap] its inlier bytes
    const uint32_t* owner;       // [F][cap] SJ-2 (rows L .. F - 1: no owner)
    uint32_t n_frames;           // F
    uint32_t map_frames;         // L
    uint32_t n_pairs;
    uint32_t min_inliers;
    uint32_t use_minimal;
    uint32_t min_shared;         // TJ-4
    float tol;                   // TJ-3
    uint32_t permille;           // TJ-4
    uint32_t* ratios;            // [entries][cap] the bits of an entry's ratios (0: none)
    uint32_t* links;             // [entries][kSjLinkWords] OrbJoinLink
    unsigned long long* keys;    // [F] SJ-5: consistent << 32 | ~index of the best HOLDS entry of the segment, 0: none (a memset before)
    uint32_t* segs;              // [F][kSjSegWords] OrbJoinSegment (a memset to 0 before)
    uint32_t* out;               // [F][kSjPoseWords] OrbJoinPose
};

// LM-2's camera(g, o) from frame g's record: the identity when g is its own origin; false when an entry is not finite
__device__ __forceinline__ bool sj_camera(const uint32_t* rec, bool own, float R[9], float t[3]) {
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 9; k++) {
        R[k] = own ? ((k & 3) == 0 ? 1.0f : 0.0f) : __uint_as_float(rec[k]);
        fin = fin && isfinite(R[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        t[k] = own ? 0.0f : __uint_as_float(rec[9 + k]);
        fin = fin && isfinite(t[k]);
    }
    return fin;
}

// SJ-4: coordinates of segment o -> camera b's frame, one unit of b = gamma units of o; false when an entry is not finite
__device__ __forceinline__ bool sj_similarity(const float P[9], const float p[3], const float Rq[9], const float tq[3], float gamma, float A[9], float a[3]) {
    const float v0 = p[0] - gamma * tq[0], v1 = p[1] - gamma * tq[1], v2 = p[2] - gamma * tq[2];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        a[r] = (Rq[r] * v0 + Rq[3 + r] * v1) + Rq[6 + r] * v2;
#pragma unroll
        for (int c = 0; c < 3; c++) A[3 * r + c] = (Rq[r] * P[c] + Rq[3 + r] * P[3 + c]) + Rq[6 + r] * P[6 + c];
    }
    traj_polar_step(A);
    return isfinite(gamma) && traj_pose_finite(A, a);
}

// SJ-3: the bits of slot a's ratio of entry e = (q, T), 0 when it has none
__device__ __forceinline__ uint32_t sj_ratio(const SjArgs& g, uint32_t e, uint32_t q, uint32_t T, uint32_t a, uint32_t nq, uint32_t nt, const float P[3], float p2,
                                             const float R[3], float t2) {
    if (a >= nq || g.mask[(size_t)e * g.cap + a] != 1u) return 0u;
    const uint32_t k = g.rows[(size_t)e * g.cap + a].index;
    if (k >= nt) return 0u;
    const uint32_t ka = g.owner[(size_t)T * g.cap + k], kb = g.owner[(size_t)q * g.cap + a];
    if (ka == kSjNone || kb == kSjNone) return 0u;
    const float4 XA = g.lms[2u * (size_t)ka], XB = g.lms[2u * (size_t)kb];
    const float za = ((P[0] * XA.x + P[1] * XA.y) + P[2] * XA.z) + p2;
    const float zb = ((R[0] * XB.x + R[1] * XB.y) + R[2] * XB.z) + t2;
    const float rho = za / zb;
    return isfinite(rho) && rho > 0.0f ? __float_as_uint(rho) : 0u;
}

// grid n_pairs, block kSjThreads
__global__ __launch_bounds__(kSjThreads) void k_sj_ratio(SjArgs g) {
    __shared__ TrajSelectLds lds;
    const uint32_t e = blockIdx.x, tid = threadIdx.x, cap = g.cap;
    const uint2 qt = g.list[e];
    const uint32_t q = qt.x, T = qt.y;
    const uint32_t* const fix = g.fixes + (size_t)e * kSjFixWords;
    const uint32_t o = fix[25], b = fix[26], st = fix[30];
    uint32_t* const link = g.links + (size_t)e * kSjLinkWords;
    // every thread takes the same way: the verdict depends on the entry only
    uint32_t verdict = kSjHolds;
    if (!(st == ORB_LOCALIZE_OK || (st == ORB_LOCALIZE_MINIMAL && g.use_minimal))) verdict = kSjStatus;
    else if (fix[28] < g.min_inliers) verdict = kSjFew;
    else if (q >= g.n_frames || T >= g.n_frames || q >= g.map_frames || b == kSjNone || b >= g.n_frames) verdict = kSjRange;
    else if (o == b) verdict = kSjSame;
    else if (o > b) verdict = kSjForward;
    float P[9], p[3], Rq[9], tq[3];
    if (verdict == kSjHolds) {
        const bool fin = sj_camera(g.frames + (size_t)q * kSjFrameWords, q == b, Rq, tq);
        traj_load_pose(fix + 13, P, p);  // OrbLoopFix's pose of camera q in segment o
        if (!fin || !traj_pose_finite(P, p)) verdict = kSjNonfinite;
    }
    if (verdict != kSjHolds) {
        if (tid < kSjLinkWords) link[tid] = tid == 0u ? verdict : (tid == 1u ? o : (tid == 2u ? b : 0u));
        return;
    }
    const uint32_t nq = min(g.counts[q], cap), nt = min(g.counts[T], cap);
    const TrajConsensus c = traj_consensus<kSjThreads>(lds, g.ratios + (size_t)e * cap, cap, g.tol, [&](uint32_t a) {
        return sj_ratio(g, e, q, T, a, nq, nt, P + 6, p[2], Rq + 6, tq[2]);
    });
    if (tid == 0u) {
        const uint32_t tv = traj_verdict(c.m, c.consistent, g.min_shared, g.permille);
        verdict = tv == kTrajFew ? kSjRatioFew : (tv == kTrajSpread ? kSjRatioSpread : kSjHolds);
        if (verdict == kSjHolds) {  // SJ-4; SJ-6 forms it again from the same words
            float A[9], a[3];
            if (!sj_similarity(P, p, Rq, tq, __uint_as_float(c.g), A, a)) verdict = kSjNonfinite;
        }
        const bool nf = verdict == kSjNonfinite;
        link[0] = verdict;
        link[1] = o;
        link[2] = b;
        link[3] = nf ? 0u : c.m;
        link[4] = nf ? 0u : c.consistent;
        link[5] = nf ? 0u : c.g;
        link[6] = 0u;
        link[7] = 0u;
        // SJ-5: the most consistent ratios, then the lowest index (b < F: RANGE otherwise)
        if (verdict == kSjHolds) atomicMax(&g.keys[b], (unsigned long long)c.consistent << 32 | (unsigned long long)(kSjNone - e));
    }
}

// grid 1, block 64; keys and segs are as k_sj_ratio and the memset left them
__global__ __launch_bounds__(64) void k_sj_chain(SjArgs g) {
    const uint32_t lane = threadIdx.x, F = g.n_frames;
    // a frame slot is an origin when a record names it
    for (uint32_t f = lane; f < F; f += 64u) {
        const uint32_t o = g.frames[(size_t)f * kSjFrameWords + 14u];
        if (o < F) atomicMax(&g.segs[(size_t)o * kSjSegWords + 15u], kSjSegRoot);
    }
    __threadfence();
    __syncthreads();
    if (lane != 0u) return;
#pragma unroll 1
    for (uint32_t b = 0u; b < F; b++) {  // SJ-6: a link's parent is an earlier slot, whose record this lane has written
        uint32_t* const S = g.segs + (size_t)b * kSjSegWords;
        const uint32_t status = __hip_atomic_load(&S[15], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long key = g.keys[b];
        float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, a[3] = {0.0f, 0.0f, 0.0f};
        float sigma = 1.0f;
        uint32_t root = b, linked = kSjNone;
        if (status != kSjSegNone && key != 0ull) {
            const uint32_t e = kSjNone - (uint32_t)key;
            const uint32_t* const fix = g.fixes + (size_t)e * kSjFixWords;
            const uint32_t q = g.list[e].x, o = fix[25];  // HOLDS: q < F, o < b
            const float gamma = __uint_as_float(g.links[(size_t)e * kSjLinkWords + 5u]);
            float P[9], p[3], Rq[9], tq[3], Al[9], al[3];
            sj_camera(g.frames + (size_t)q * kSjFrameWords, q == b, Rq, tq);
            traj_load_pose(fix + 13, P, p);
            sj_similarity(P, p, Rq, tq, gamma, Al, al);
            const uint32_t* const So = g.segs + (size_t)o * kSjSegWords;
            float Ao[9], ao[3];
            traj_load_pose(So, Ao, ao);
            const float so = __uint_as_float(So[12]);
            float An[9], an[3];
            traj_compose(Al, al, so, Ao, ao, An, an);
            const float sn = so * gamma;
            if (isfinite(sn) && traj_pose_finite(An, an)) {
#pragma unroll
                for (int k = 0; k < 9; k++) A[k] = An[k];
#pragma unroll
                for (int k = 0; k < 3; k++) a[k] = an[k];
                sigma = sn;
                root = So[13];
                linked = e;
                g.links[(size_t)e * kSjLinkWords + 6u] = 1u;
            }
        }
        traj_store_pose(S, A, a);
        S[12] = __float_as_uint(sigma);
        S[13] = root;
        S[14] = linked;
        S[15] = linked != kSjNone ? kSjSegLinked : status;
    }
}

// grid ceil(F / kSjThreads), block kSjThreads
__global__ __launch_bounds__(kSjThreads) void k_sj_write(SjArgs g) {
    const uint32_t f = blockIdx.x * kSjThreads + threadIdx.x;
    if (f >= g.n_frames) return;
    const uint32_t* const rec = g.frames + (size_t)f * kSjFrameWords;
    uint32_t* const out = g.out + (size_t)f * kSjPoseWords;
    const uint32_t b = rec[14];
    const uint32_t* const S = g.segs + (size_t)min(b, g.n_frames - 1u) * kSjSegWords;
    const uint32_t root = b < g.n_frames ? S[13] : b;
    if (root == b) {  // COPIED: the trajectory's words
#pragma unroll
        for (int k = 0; k < 13; k++) out[k] = rec[k];
        out[13] = __float_as_uint(1.0f);
        out[14] = b;
        out[15] = kSjCopied;
        return;
    }
    float R[9], t[3], A[9], a[3], Rn[9], tn[3];
    sj_camera(rec, f == b, R, t);
    traj_load_pose(S, A, a);
    const float sigma = __uint_as_float(S[12]);
    traj_compose(R, t, sigma, A, a, Rn, tn);
    traj_store_pose(out, Rn, tn);
    out[12] = __float_as_uint(sigma * __uint_as_float(rec[12]));
    out[13] = __float_as_uint(sigma);
    out[14] = root;
    out[15] = kSjMoved;
}

}  // namespace orb
