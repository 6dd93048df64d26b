// orb_kernels_loop.h -- a listed query's pose from its target's landmarks (not in the reference; the definition is the build's own,
// LC-1..LC-7 in DESIGN.md section 28).  A confirmed loop of orb_match_pairs / orb_verify_pairs says that two frames show the same
// place, not where the query camera is in the map.  Here a row of the last orb_match_pairs sends every keypoint of the query frame
// q to a keypoint of the target frame T, that keypoint is a view of a landmark of the last orb_landmarks_consecutive, and the
// landmark is a 3D point in T's segment: section 21's six-point DLT RANSAC and Gauss-Newton refit on those 3D-2D correspondences
// give camera q relative to camera T in the unit of T's segment, and, composed with T's pose, camera q in that segment's frame.
// Every binary32 operation below is written out in the order the definition gives (-ffp-contract=off, correctly rounded division
// and square root), so the CPU restatement (tests/loop_ref.py) reproduces every bit.
//
//   k_lc_index    grid (L - 1, ceil(cap / 256)): a thread per landmark slot; a GOOD landmark whose views lie inside the L frames
//                 walks them and puts its key p * cap + i on every registered one with an integer atomicMin (the owners are set to
//                 0xffffffff by a memset before: no result depends on an order) (LC-2)
//   k_lc_gather   one workgroup of 256 per list entry: the entry, its row, the owner of the matched keypoint, the landmark in
//                 camera T's frame, the query keypoint and its ray (LC-3), compacted in the order of the query's slots by
//                 k_loc_gather's step (loc_compact, loc_candidate), plus the candidate of every slot (or kVerifyNone)
//   k_loc_score   of orb_kernels_localize.h, as it is, on the stage's buffers with grid.x = list entries (LC-4)
//   k_lc_refine   one workgroup per list entry: k_loc_refine's fit (loc_fit of orb_kernels_localize.h), then LC-5's compose
//                 (traj_compose of orb_kernels_traj.h with s = 1), the inlier bytes by query slot (loc_slot_bytes) and the record (LC-6)
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_localize.h"
#include "orb_kernels_traj.h"

namespace orb {

constexpr uint32_t kLcSeedSalt = 0x4C433031u;  // LC-4: the draw stream's seed is lowbias32(seed ^ kLcSeedSalt)
constexpr uint32_t kLcThreads = 256u;
constexpr uint32_t kLcFrameWords = 20u;        // OrbFramePose
constexpr uint32_t kLcFixWords = 32u;          // OrbLoopFix
constexpr uint32_t kLcNone = 0xffffffffu;      // a keypoint without an owner; query_origin of a query above the trajectory's frames

struct LcArgs {
    LocArgs loc;             // k_loc_score's view of the stage's own buffers: rows per list entry; fix: [entries][kLcFixWords]; matches: the
                             // matcher's consecutive records (the walk); counts, corners: the batch's
    const uint2* list;       // [entries] OrbFramePair of the last orb_match_pairs: (query, target)
    const MatchRecord* rows; // [entries][cap] its rows: row i holds the queries of entry i's query frame
    const uint32_t* frames;  // [traj_frames][kLcFrameWords] of the last orb_trajectory_consecutive
    const float4* lms;       // [L - 1][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    uint32_t n_frames;       // L
    uint32_t traj_frames;    // frames of the last orb_trajectory_consecutive (>= L)
    uint32_t* owner;         // [L][cap] LC-2: the key p * cap + i of the keypoint's owner, kLcNone: none
};

__device__ __forceinline__ uint32_t lc_nq(const LcArgs& a, uint32_t g) { return min(a.loc.counts[g], a.loc.cap); }

// LC-3: camera T's pose in the segment of its origin o (LM-2: the identity when T is its own origin); false: T is outside the map,
// or an entry of the pose is not finite (NOMAP)
__device__ __forceinline__ bool lc_target(const LcArgs& a, uint32_t T, uint32_t& o, float R[9], float t[3]) {
    o = 0u;
    if (T >= a.n_frames) return false;
    const uint32_t* const rec = a.frames + (size_t)T * kLcFrameWords;
    o = rec[14];
    const bool own = T == o;
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

// grid (L - 1, ceil(cap / kLcThreads)), block kLcThreads; the owners are set to kLcNone by a memset before
__global__ __launch_bounds__(kLcThreads) void k_lc_index(LcArgs a) {
    const uint32_t cap = a.loc.cap;
    const uint32_t p = blockIdx.x, i = blockIdx.y * kLcThreads + threadIdx.x;
    if (p + 1u >= a.n_frames || i >= cap) return;
    const size_t slot = (size_t)p * cap + i;
    const float4 lo = a.lms[2u * slot], hi = a.lms[2u * slot + 1u];
    const uint32_t views = __float_as_uint(hi.x) & 0xffffu, o = __float_as_uint(hi.y);
    if (views == 0u || (__float_as_uint(lo.w) & ORB_POINT_GOOD) == 0u || p + views > a.n_frames) return;  // LC-2: takes no part
    uint32_t k = i;
    for (uint32_t s = 0u; s < views; s++) {
        const uint32_t g = p + s;  // <= L - 1
        if (k >= lc_nq(a, g)) break;
        if (a.frames[(size_t)g * kLcFrameWords + 14u] == o) atomicMin(&a.owner[(size_t)g * cap + k], (uint32_t)slot);
        if (s + 1u < views) k = a.loc.matches[(size_t)g * cap + k].index;  // g <= L - 2
    }
}

// grid (entries), block 256
__global__ __launch_bounds__(256) void k_lc_gather(LcArgs a) {
    __shared__ uint32_t wave_n[4];
    const LocArgs& L = a.loc;
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    const uint2 qt = a.list[e];
    const uint32_t q = qt.x, T = qt.y;
    uint32_t o;
    float R[9], t[3];
    if (!lc_target(a, T, o, R, t)) {  // uniform
        if (tid == 0u) L.n_cand[e] = 0u;
        return;
    }
    const uint32_t nq = lc_nq(a, q), nt = lc_nq(a, T);
    const MatchRecord* const row = a.rows + (size_t)e * L.cap;
    const uint32_t* const own = a.owner + (size_t)T * L.cap;
    const CornerData* const cq = L.corners + (size_t)q * L.cap;
    uint32_t* const cand_of = L.cand_of + (size_t)e * L.cap;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < nq; i0 += 256u) {
        const uint32_t i = i0 + tid;
        bool keep = false;
        uint32_t key = kLcNone;
        if (i < nq) {  // LC-3: GV-1's filter against n_q(T), then the owner of the matched keypoint
            const MatchRecord m = row[i];
            const uint32_t d = m.dist & 0xffffu, second = m.dist >> 16, k = m.index;
            if (k != kVerifyNone && k < nt && d <= L.max_distance && (float)d < L.ratio * (float)second) {
                key = own[k];
                keep = key != kLcNone;
            }
        }
        uint32_t total;
        const uint32_t slot = loc_compact(keep, base, wave_n, total);
        if (i < nq) cand_of[i] = keep ? slot : kVerifyNone;
        if (keep) loc_candidate(L, e, slot, a.lms[2u * (size_t)key], R, t, cq[i], 0.0f);  // slot < n_q(q) <= cap
        base += total;
        __syncthreads();
    }
    if (tid == 0u) L.n_cand[e] = base;
}

// grid (entries), block 256
__global__ __launch_bounds__(256) void k_lc_refine(LcArgs a) {
    const LocArgs& L = a.loc;
    const uint32_t e = blockIdx.x;
    const uint2 qt = a.list[e];
    const uint32_t q = qt.x, T = qt.y;
    uint32_t o;
    float RT[9], tT[3];
    const bool nomap = !lc_target(a, T, o, RT, tT);  // uniform
    const uint32_t M = nomap ? 0u : L.n_cand[e];
    const LocFit f = loc_fit(L, e, M);
    const bool has_min = f.has_min;
    // LC-6: an inlier byte per keypoint slot of frame q (cand_of is written below n_q(q) of an entry that is not NOMAP)
    loc_slot_bytes(L, e, has_min ? lc_nq(a, q) : 0u, f);
    if (threadIdx.x == 0u) {  // the record
        uint32_t* const out = L.fix + (size_t)e * kLcFixWords;
        // LC-5: camera q in segment o's frame, R Rt after one polar step and R tT + t; zeros when an entry is not finite
        float Rp[9], tp[3];
        traj_compose(f.R, f.t, 1.0f, RT, tT, Rp, tp);
        const bool fin = has_min && traj_pose_finite(Rp, tp);
        loc_put_pose(out, f);
#pragma unroll
        for (int k = 0; k < 9; k++) out[13 + k] = fin ? __float_as_uint(Rp[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) out[22 + k] = fin ? __float_as_uint(tp[k]) : 0u;
        out[25] = has_min ? o : 0u;
        out[26] = has_min ? (q < a.traj_frames ? a.frames[(size_t)q * kLcFrameWords + 14u] : kLcNone) : 0u;
        out[27] = has_min ? M : 0u;
        out[28] = f.inliers;
        out[29] = f.h;
        out[30] = loc_status(nomap, M, has_min, f.keep);
        out[31] = 0u;
    }
}

}  // namespace orb
