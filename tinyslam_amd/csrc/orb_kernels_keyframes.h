// orb_kernels_keyframes.h -- a keyframe store that outlives a batch (not in the reference; the definition is the build's own,
// KF-1..KF-5 in DESIGN.md section 32).  orb_match_pairs and orb_loop_pairs close a loop between two frames of the last batch; a
// database hit of orb_place_frames names a frame of an earlier one.  Here a slot of the store keeps what those two calls read of a
// target frame T -- its stored corners and descriptors, camera T in its segment and, per keypoint, the owner key of LC-2 with the
// landmark already under camera T (what loc_candidate puts into reca) -- so that a later batch is matched and localised against
// the slot with the bytes it would get against T.  Every binary32 operation is written out in the order the definition gives
// (-ffp-contract=off), so the CPU restatement (tests/keyframes_ref.py) reproduces every bit.
//
//   k_lc_index       of orb_kernels_loop.h, as it is, on the insert's own owner buffer (KF-2)
//   k_kf_head        a thread per list entry: the header with `points` at 0, the slot's counter for the matchers
//   k_kf_insert      grid (ceil(cap / 256), entries): a lane per record of the slot, consecutive lanes on consecutive records; a
//                    corner, a point and the two halves of a descriptor are one 16-byte load and store each.  What the row shares
//                    -- the entry, the frame's counter, its pose -- sits at addresses that depend on blockIdx only.  `points` is
//                    a wave ballot and one integer atomicAdd per wave
//   k_match_kf_fp4,  k_match_fp4's and k_match's bodies (orb_match_fp4_body.inc, orb_match_valu_body.inc) on a buffer that holds
//   k_match_kf       the batch's rows followed by the slots': the candidates' frame is max_batch + slot (KF-3)
//   k_kf_gather      one workgroup of 256 per list entry: k_lc_gather with the slot's keypoints, keys and points (KF-4)
//   k_loc_score      of orb_kernels_localize.h, as it is
//   k_kf_refine      k_lc_refine on the header's pose: loc_fit, traj_compose with s = 1, loc_slot_bytes, the record
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_loop.h"
#include "orb_kernels_pairs.h"

namespace orb {

constexpr uint32_t kKfThreads = 256u;
constexpr uint32_t kKfHeadWords = 24u;  // OrbKeyframe: r 0..8, t 9..11, scale 12, keypoints 13, points 14, frame 15, origin 16, user 17..18, status 19
constexpr uint32_t kKfStored = 1u, kKfNomap = 2u;  // ORB_KEYFRAME_STORED, ORB_KEYFRAME_NOMAP

struct KfInsertArgs {
    LcArgs lc;                 // LC-1..LC-3 on the insert's owner buffer: loc.counts, loc.matches, loc.cap, frames, lms, n_frames, owner
    const uint4* list;         // [entries] OrbKeyframeEntry: (frame, slot, user[0], user[1])
    const uint4* corners;      // [frames][cap] the batch's CornerData
    const uint4* desc;         // [frames][cap][2] the batch's CornerDescriptor
    uint32_t n_entries;
    uint32_t* heads;           // [slots][kKfHeadWords]
    uint32_t* slot_counts;     // [slots] the matchers' counter of a slot
    uint4* kcorners;           // [slots][cap]
    uint4* kdesc;              // [slots][cap][2]
    float4* kpoints;           // [slots][cap] OrbMapPoint
};

// grid ceil(entries / kKfThreads), block kKfThreads
__global__ __launch_bounds__(kKfThreads) void k_kf_head(KfInsertArgs a) {
    const uint32_t e = blockIdx.x * kKfThreads + threadIdx.x;
    if (e >= a.n_entries) return;
    const uint4 ent = a.list[e];
    const uint32_t g = ent.x, n = lc_nq(a.lc, g);
    uint32_t o;
    float R[9], t[3];
    const bool ok = lc_target(a.lc, g, o, R, t);
    uint32_t* const out = a.heads + (size_t)ent.y * kKfHeadWords;
#pragma unroll
    for (int k = 0; k < 9; k++) out[k] = ok ? __float_as_uint(R[k]) : 0u;
#pragma unroll
    for (int k = 0; k < 3; k++) out[9 + k] = ok ? __float_as_uint(t[k]) : 0u;
    out[12] = ok ? a.lc.frames[(size_t)g * kLcFrameWords + 12u] : 0u;
    out[13] = n;
    out[14] = 0u;  // k_kf_insert counts
    out[15] = g;
    out[16] = ok ? o : kLcNone;
    out[17] = ent.z;
    out[18] = ent.w;
    out[19] = ok ? kKfStored : kKfNomap;
#pragma unroll
    for (int k = 20; k < (int)kKfHeadWords; k++) out[k] = 0u;
    a.slot_counts[ent.y] = n;
}

// grid (ceil(cap / kKfThreads), entries), block kKfThreads; the headers as k_kf_head left them
__global__ __launch_bounds__(kKfThreads) void k_kf_insert(KfInsertArgs a) {
    const uint32_t cap = a.lc.loc.cap;
    // what the row shares
    const uint4 ent = a.list[blockIdx.y];
    const uint32_t g = ent.x, n = lc_nq(a.lc, g);
    uint32_t o;
    float R[9], t[3];
    const bool ok = lc_target(a.lc, g, o, R, t);
    const size_t src = (size_t)g * cap, dst = (size_t)ent.y * cap;
    const uint32_t i = blockIdx.x * kKfThreads + threadIdx.x;
    bool has = false;
    if (i < cap) {
        uint4 c = make_uint4(0u, 0u, 0u, 0u), d0 = c, d1 = c;  // the records at and above n: zeros
        float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n) {
            c = a.corners[src + i];
            d0 = a.desc[2u * (src + i)];
            d1 = a.desc[2u * (src + i) + 1u];
            const uint32_t key = ok ? a.lc.owner[src + i] : kLcNone;
            pt.w = __uint_as_float(key);
            if (key != kLcNone) {  // the landmark under camera g: loc_candidate's point
                const float4 X = a.lc.lms[2u * (size_t)key];
                loc_transform(R, t, X.x, X.y, X.z, pt.x, pt.y, pt.z);
                has = true;
            }
        }
        a.kcorners[dst + i] = c;
        a.kdesc[2u * (dst + i)] = d0;
        a.kdesc[2u * (dst + i) + 1u] = d1;
        a.kpoints[dst + i] = pt;
    }
    const uint32_t n_has = (uint32_t)__popcll(__ballot(has));
    if ((threadIdx.x & 63u) == 0u && n_has) atomicAdd(&a.heads[(size_t)ent.y * kKfHeadWords + 14u], n_has);  // an integer sum, in any order
}

// counts, desc4: [max_batch + slots] rows, the batch's first; list: (query, slot)
__global__ __launch_bounds__(64 * kMatchWaves, TINYORB_MATCH_MINWAVES) void k_match_kf_fp4(const uint2* __restrict__ list, uint32_t first_slot_row,
                                                                                             const uint32_t* __restrict__ counts,
                                                                                             const uint8_t* __restrict__ desc4, uint32_t cap,
                                                                                             MatchRecord* __restrict__ matches) {
    const uint32_t item = blockIdx.x, fq = list[item].x, ft = first_slot_row + list[item].y;
#define MATCH_FA fq
#define MATCH_FB ft
#define MATCH_ROW item
#include "orb_match_fp4_body.inc"
#undef MATCH_FA
#undef MATCH_FB
#undef MATCH_ROW
}

__global__ __launch_bounds__(64) void k_match_kf(const uint2* __restrict__ list, uint32_t first_slot_row, const uint32_t* __restrict__ counts,
                                                 const CornerDescriptor* __restrict__ descriptors, uint32_t cap, MatchRecord* __restrict__ matches) {
    const uint32_t item = blockIdx.x, fq = list[item].x, ft = first_slot_row + list[item].y;
#define MATCH_FA fq
#define MATCH_FB ft
#define MATCH_ROW item
#include "orb_match_valu_body.inc"
#undef MATCH_FA
#undef MATCH_FB
#undef MATCH_ROW
}

struct KfArgs {
    LocArgs loc;              // k_loc_score's view of the stage's own buffers: rows per list entry; fix: [entries][kLcFixWords]; counts,
                              // corners: the batch's
    const uint2* list;        // [entries] OrbKeyframePair of the last orb_match_keyframes: (query, slot)
    const MatchRecord* rows;  // [entries][cap] its rows
    const uint32_t* heads;    // [slots][kKfHeadWords]
    const float4* kpoints;    // [slots][cap] OrbMapPoint
};

__device__ __forceinline__ uint32_t kf_nq(const KfArgs& a, uint32_t q) { return min(a.loc.counts[q], a.loc.cap); }

// grid (entries), block 256
__global__ __launch_bounds__(256) void k_kf_gather(KfArgs a) {
    __shared__ uint32_t wave_n[4];
    const LocArgs& L = a.loc;
    const uint32_t e = blockIdx.x, tid = threadIdx.x;
    const uint2 qs = a.list[e];
    const uint32_t q = qs.x;
    const uint32_t* const head = a.heads + (size_t)qs.y * kKfHeadWords;
    if (head[19] != kKfStored) {  // uniform
        if (tid == 0u) L.n_cand[e] = 0u;
        return;
    }
    const uint32_t nq = kf_nq(a, q), nt = head[13];
    const MatchRecord* const row = a.rows + (size_t)e * L.cap;
    const float4* const pts = a.kpoints + (size_t)qs.y * L.cap;
    const CornerData* const cq = L.corners + (size_t)q * L.cap;
    uint32_t* const cand_of = L.cand_of + (size_t)e * L.cap;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < nq; i0 += 256u) {
        const uint32_t i = i0 + tid;
        bool keep = false;
        float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < nq) {  // KF-4: LC-3's filter against the slot's keypoints, then the key of the matched keypoint
            const MatchRecord m = row[i];
            const uint32_t d = m.dist & 0xffffu, second = m.dist >> 16, k = m.index;
            if (k != kVerifyNone && k < nt && d <= L.max_distance && (float)d < L.ratio * (float)second) {
                pt = pts[k];
                keep = __float_as_uint(pt.w) != kLcNone;
            }
        }
        uint32_t total;
        const uint32_t slot = loc_compact(keep, base, wave_n, total);
        if (i < nq) cand_of[i] = keep ? slot : kVerifyNone;
        if (keep) loc_record(L, e, slot, pt.x, pt.y, pt.z, cq[i], 0.0f);  // loc_candidate's records, the point as the slot holds it; slot < n_q(q) <= cap
        base += total;
        __syncthreads();
    }
    if (tid == 0u) L.n_cand[e] = base;
}

// grid (entries), block 256
__global__ __launch_bounds__(256) void k_kf_refine(KfArgs a) {
    const LocArgs& L = a.loc;
    const uint32_t e = blockIdx.x;
    const uint2 qs = a.list[e];
    const uint32_t* const head = a.heads + (size_t)qs.y * kKfHeadWords;
    const bool nomap = head[19] != kKfStored;  // uniform
    const uint32_t M = nomap ? 0u : L.n_cand[e];
    const LocFit f = loc_fit(L, e, M);
    const bool has_min = f.has_min;
    loc_slot_bytes(L, e, has_min ? kf_nq(a, qs.x) : 0u, f);
    if (threadIdx.x == 0u) {  // the record
        uint32_t* const out = L.fix + (size_t)e * kLcFixWords;
        float RT[9], tT[3], Rp[9], tp[3];
        traj_load_pose(head, RT, tT);
        traj_compose(f.R, f.t, 1.0f, RT, tT, Rp, tp);  // LC-5 on the header's pose
        const bool fin = has_min && traj_pose_finite(Rp, tp);
        loc_put_pose(out, f);
#pragma unroll
        for (int k = 0; k < 9; k++) out[13 + k] = fin ? __float_as_uint(Rp[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) out[22 + k] = fin ? __float_as_uint(tp[k]) : 0u;
        out[25] = has_min ? head[16] : 0u;
        out[26] = has_min ? qs.y : 0u;
        out[27] = has_min ? M : 0u;
        out[28] = f.inliers;
        out[29] = f.h;
        out[30] = loc_status(nomap, M, has_min, f.keep);
        out[31] = 0u;
    }
}

}  // namespace orb
