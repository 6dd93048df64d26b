// orb_kernels_anchor.h -- a batch's trajectory and landmarks in the stored map (not in the reference; the definition is the build's
// own, AN-1..AN-7 in DESIGN.md section 33).  An OrbKeyframeFix of entry (q, s) gives camera q of the batch in the frame and unit of
// the keyframe's segment; the trajectory gives camera q in its own segment b.  An inlier keypoint of q whose matched keypoint of
// the slot carries a stored point and which a landmark of b owns has two depths in camera q, one in each unit: the lower median of
// their ratios is the scale between segment b and the stored map, the two poses of camera q the rotation and translation.  This
// is the join stage (section 30) with a keyframe on the far side: every segment of the batch takes its best entry and hangs
// directly under that keyframe's segment -- there is no chain -- and every frame and every GOOD landmark of an anchored segment is
// written in the map's frame and unit.  Every binary32 operation below is written out in the order the definition gives
// (-ffp-contract=off, correctly rounded division), so the CPU restatement (tests/anchor_ref.py) reproduces every bit.
//
//   k_lc_index    of orb_kernels_loop.h, as it is, on an LcArgs of this stage's owner buffer (set to 0xffffffff by a memset) (AN-2)
//   k_an_ratio    one workgroup of 256 per list entry: AN-3's verdict (uniform), then traj_consensus of orb_kernels_traj.h over the
//                 query's slots (an_ratio: the stored point is one 16-byte load), then, on one lane, traj_verdict as a link verdict,
//                 AN-4 (sj_similarity), the link record and AN-5's atomicMax on the segment's 64-bit key.  What the entry shares --
//                 the fix, the slot's header, frame q's record -- sits at addresses that depend on blockIdx only
//   k_an_segment  a thread per frame slot: marks the origin its record names (an integer atomicMax on the status word), and writes
//                 the slot's own segment record from its chosen entry (AN-6)
//   k_an_write    a thread per frame: the OrbAnchorPose records (traj_compose), and the row of pair f with its counts at 0
//   k_an_land     grid (ceil(cap / (256 S)), pairs), S slots per thread: AN-7.  A record is two 16-byte loads and two 16-byte
//                 stores per lane, coalesced over the row; what a workgroup shares -- the row's origin and its segment record --
//                 sits at addresses that depend on blockIdx only; the counts are wave ballots and one integer atomicAdd per wave
//                 and count
// Integer atomics only: no result depends on an order.  Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_join.h"
#include "orb_kernels_keyframes.h"

namespace orb {

constexpr uint32_t kAnThreads = 256u;
constexpr uint32_t kAnLandSlots = 2u;    // slots per thread of k_an_land
constexpr uint32_t kAnFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kAnFixWords = 32u;    // OrbKeyframeFix
constexpr uint32_t kAnPoseWords = 16u;   // OrbAnchorPose: r 0..8, t 9..11, scale 12, gain 13, slot 14, status 15
constexpr uint32_t kAnSegWords = 24u;    // OrbAnchorSegment: r 0..8, t 9..11, gamma 12, slot 13, link 14, map_origin 15, map_frame 16, user 17..18, status 19
constexpr uint32_t kAnLinkWords = 8u;    // OrbAnchorLink: verdict, query_origin, slot, shared, consistent, gamma, chosen, reserved
constexpr uint32_t kAnRowWords = 8u;     // OrbAnchorRow: good, moved, dropped, origin, slot, map_origin, reserved[2]
constexpr uint32_t kAnLmRowWords = 4u;   // OrbLandmarkRow
constexpr uint32_t kAnNone = 0xffffffffu;
// AN-3's verdicts (ORB_ANCHOR_LINK_*)
constexpr uint32_t kAnHolds = 0u, kAnStatus = 1u, kAnFew = 2u, kAnRange = 3u, kAnNonfinite = 4u, kAnRatioFew = 5u, kAnRatioSpread = 6u;
constexpr uint32_t kAnSegNone = 0u, kAnSegFree = 1u, kAnSegAnchored = 2u;  // OrbAnchorSegment.status
constexpr uint32_t kAnFree = 0u, kAnAnchored = 1u;                         // OrbAnchorPose.status

struct AnArgs {
    const uint32_t* __restrict__ counts;    // [frames] raw counters of the batch
    uint32_t cap;
    const uint2* __restrict__ list;         // [entries] OrbKeyframePair of the last orb_match_keyframes: (query, slot)
    const MatchRecord* __restrict__ rows;   // [entries][cap] its rows
    const uint32_t* __restrict__ frames;    // [F][kAnFrameWords] of the last orb_trajectory_consecutive
    const float4* __restrict__ lms;         // [L - 1][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    const uint32_t* __restrict__ lrows;     // [L - 1][kAnLmRowWords] its rows
    const uint32_t* __restrict__ fixes;     // [entries][kAnFixWords] of the last orb_localize_keyframes
    const uint8_t* __restrict__ mask;       // [entries][cap] its inlier bytes
    const uint32_t* __restrict__ heads;     // [slots][kKfHeadWords] the store's headers
    const float4* __restrict__ kpoints;     // [slots][cap] OrbMapPoint
    const uint32_t* __restrict__ owner;     // [F][cap] AN-2 (rows L .. F - 1: no owner)
    uint32_t n_frames;                      // F
    uint32_t map_frames;                    // L
    uint32_t n_pairs;                       // L - 1: the pairs of AN-7
    uint32_t n_entries;
    uint32_t min_inliers;
    uint32_t use_minimal;
    uint32_t min_shared;                    // TJ-4
    float tol;                              // TJ-3
    uint32_t permille;                      // TJ-4
    uint32_t* ratios;                       // [entries][cap] the bits of an entry's ratios (0: none)
    uint32_t* links;                        // [entries][kAnLinkWords] OrbAnchorLink
    unsigned long long* keys;               // [F] AN-5: consistent << 32 | ~index of the best HOLDS entry of the segment, 0: none (a memset before)
    uint32_t* segs;                         // [F][kAnSegWords] OrbAnchorSegment (a memset to 0 before)
    uint32_t* poses;                        // [F][kAnPoseWords] OrbAnchorPose
    uint32_t* out_rows;                     // [L - 1][kAnRowWords] OrbAnchorRow
    float4* out;                            // [L - 1][cap][2] OrbLandmark
};

// AN-3: the bits of slot a's ratio of entry e = (q, s), 0 when it has none.  r, t2: the third row of the fix's relative pose;
// R, T2: the third row of camera(q, b)
__device__ __forceinline__ uint32_t an_ratio(const AnArgs& g, uint32_t e, uint32_t q, const float4* __restrict__ pts, uint32_t a, uint32_t nq, uint32_t nt,
                                             const float r[3], float t2, const float R[3], float T2) {
    if (a >= nq || g.mask[(size_t)e * g.cap + a] != 1u) return 0u;
    const uint32_t k = g.rows[(size_t)e * g.cap + a].index;
    if (k >= nt) return 0u;
    const float4 Y = pts[k];  // the stored point, in the keyframe camera's frame
    if (__float_as_uint(Y.w) == kAnNone) return 0u;
    const uint32_t kb = g.owner[(size_t)q * g.cap + a];
    if (kb == kAnNone) return 0u;
    const float4 XB = g.lms[2u * (size_t)kb];
    const float za = ((r[0] * Y.x + r[1] * Y.y) + r[2] * Y.z) + t2;
    const float zb = ((R[0] * XB.x + R[1] * XB.y) + R[2] * XB.z) + T2;
    const float rho = za / zb;
    return isfinite(rho) && rho > 0.0f ? __float_as_uint(rho) : 0u;
}

// grid n_entries, block kAnThreads
__global__ __launch_bounds__(kAnThreads) void k_an_ratio(AnArgs g) {
    __shared__ TrajSelectLds lds;
    const uint32_t e = blockIdx.x, tid = threadIdx.x, cap = g.cap, F = g.n_frames;
    const uint2 qs = g.list[e];
    const uint32_t q = qs.x, s = qs.y;
    const uint32_t* const fix = g.fixes + (size_t)e * kAnFixWords;
    const uint32_t* const head = g.heads + (size_t)s * kKfHeadWords;
    const uint32_t* const rec = g.frames + (size_t)min(q, F - 1u) * kAnFrameWords;
    const uint32_t st = fix[30];
    const uint32_t b = q < F ? rec[14] : 0u;  // the fix carries no origin of its query
    uint32_t* const link = g.links + (size_t)e * kAnLinkWords;
    // every thread takes the same way: the verdict depends on the entry only
    uint32_t verdict = kAnHolds;
    if (!(st == ORB_LOCALIZE_OK || (st == ORB_LOCALIZE_MINIMAL && g.use_minimal))) verdict = kAnStatus;
    else if (fix[28] < g.min_inliers) verdict = kAnFew;
    else if (q >= F || q >= g.map_frames || b == kAnNone || b >= F) verdict = kAnRange;
    float r[9], t[3], P[9], p[3], Rq[9], tq[3];
    if (verdict == kAnHolds) {
        const bool fin = sj_camera(rec, q == b, Rq, tq);
        traj_load_pose(fix, r, t);        // camera q relative to the keyframe camera
        traj_load_pose(fix + 13, P, p);   // camera q in the keyframe's segment
        if (!fin || !traj_pose_finite(r, t) || !traj_pose_finite(P, p)) verdict = kAnNonfinite;
    }
    if (verdict != kAnHolds) {
        if (tid < kAnLinkWords) link[tid] = tid == 0u ? verdict : (tid == 1u ? b : (tid == 2u ? s : 0u));
        return;
    }
    const uint32_t nq = min(g.counts[q], cap), nt = min(head[13], cap);
    const float4* const pts = g.kpoints + (size_t)s * cap;
    const TrajConsensus c = traj_consensus<kAnThreads>(lds, g.ratios + (size_t)e * cap, cap, g.tol, [&](uint32_t a) {
        return an_ratio(g, e, q, pts, a, nq, nt, r + 6, t[2], Rq + 6, tq[2]);
    });
    if (tid == 0u) {
        const uint32_t tv = traj_verdict(c.m, c.consistent, g.min_shared, g.permille);
        verdict = tv == kTrajFew ? kAnRatioFew : (tv == kTrajSpread ? kAnRatioSpread : kAnHolds);
        if (verdict == kAnHolds) {  // AN-4; AN-6 forms it again from the same words
            float A[9], a[3];
            if (!sj_similarity(P, p, Rq, tq, __uint_as_float(c.g), A, a)) verdict = kAnNonfinite;
        }
        const bool nf = verdict == kAnNonfinite;
        link[0] = verdict;
        link[1] = b;
        link[2] = s;
        link[3] = nf ? 0u : c.m;
        link[4] = nf ? 0u : c.consistent;
        link[5] = nf ? 0u : c.g;
        link[6] = 0u;
        link[7] = 0u;
        // AN-5: the most consistent ratios, then the lowest index (b < F: RANGE otherwise)
        if (verdict == kAnHolds) atomicMax(&g.keys[b], (unsigned long long)c.consistent << 32 | (unsigned long long)(kAnNone - e));
    }
}

// grid ceil(F / kAnThreads), block kAnThreads; keys as k_an_ratio left them, segs as the memset left them.  The status word of a slot
// is written by atomicMax only (FREE by whoever names the slot, ANCHORED by the slot's own thread), every other word by the
// slot's own thread.
__global__ __launch_bounds__(kAnThreads) void k_an_segment(AnArgs g) {
    const uint32_t b = blockIdx.x * kAnThreads + threadIdx.x, F = g.n_frames;
    if (b >= F) return;
    // a frame slot is an origin when a record names it
    const uint32_t named = g.frames[(size_t)b * kAnFrameWords + 14u];
    if (named < F) atomicMax(&g.segs[(size_t)named * kAnSegWords + 19u], kAnSegFree);
    uint32_t* const S = g.segs + (size_t)b * kAnSegWords;
    const unsigned long long key = g.keys[b];
    float A[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f}, a[3] = {0.0f, 0.0f, 0.0f};
    float gamma = 1.0f;
    uint32_t slot = kAnNone, linked = kAnNone, map_origin = kAnNone, map_frame = kAnNone, user0 = 0u, user1 = 0u;
    if (key != 0ull) {  // a HOLDS entry of segment b: frame q's record names b, q < F, and the similarity is finite
        const uint32_t e = kAnNone - (uint32_t)key;
        const uint32_t* const fix = g.fixes + (size_t)e * kAnFixWords;
        const uint2 qs = g.list[e];
        const uint32_t* const head = g.heads + (size_t)qs.y * kKfHeadWords;
        gamma = __uint_as_float(g.links[(size_t)e * kAnLinkWords + 5u]);
        float P[9], p[3], Rq[9], tq[3];
        sj_camera(g.frames + (size_t)qs.x * kAnFrameWords, qs.x == b, Rq, tq);
        traj_load_pose(fix + 13, P, p);
        sj_similarity(P, p, Rq, tq, gamma, A, a);
        slot = qs.y;
        linked = e;
        map_origin = head[16];
        map_frame = head[15];
        user0 = head[17];
        user1 = head[18];
        g.links[(size_t)e * kAnLinkWords + 6u] = 1u;
    }
    traj_store_pose(S, A, a);
    S[12] = __float_as_uint(gamma);
    S[13] = slot;
    S[14] = linked;
    S[15] = map_origin;
    S[16] = map_frame;
    S[17] = user0;
    S[18] = user1;
    if (linked != kAnNone) atomicMax(&S[19], kAnSegAnchored);
}

// the segment record of origin o when it is ANCHORED, else null
__device__ __forceinline__ const uint32_t* an_anchored(const AnArgs& g, uint32_t o) {
    if (o >= g.n_frames) return nullptr;
    const uint32_t* const S = g.segs + (size_t)o * kAnSegWords;
    return S[19] == kAnSegAnchored ? S : nullptr;
}

// grid ceil(F / kAnThreads), block kAnThreads; segs as k_an_segment left them
__global__ __launch_bounds__(kAnThreads) void k_an_write(AnArgs g) {
    const uint32_t f = blockIdx.x * kAnThreads + threadIdx.x;
    if (f >= g.n_frames) return;
    if (f < g.n_pairs) {  // AN-7: the counts at 0, where the row goes
        const uint32_t o = g.lrows[(size_t)f * kAnLmRowWords + 3u];
        const uint32_t* const S = an_anchored(g, o);
        uint32_t* const row = g.out_rows + (size_t)f * kAnRowWords;
        row[0] = 0u;
        row[1] = 0u;
        row[2] = 0u;
        row[3] = o;
        row[4] = S ? S[13] : kAnNone;
        row[5] = S ? S[15] : kAnNone;
        row[6] = 0u;
        row[7] = 0u;
    }
    const uint32_t* const rec = g.frames + (size_t)f * kAnFrameWords;
    uint32_t* const out = g.poses + (size_t)f * kAnPoseWords;
    const uint32_t b = rec[14];
    const uint32_t* const S = an_anchored(g, b);
    if (!S) {  // FREE: the trajectory's words
#pragma unroll
        for (int k = 0; k < 13; k++) out[k] = rec[k];
        out[13] = __float_as_uint(1.0f);
        out[14] = kAnNone;
        out[15] = kAnFree;
        return;
    }
    float R[9], t[3], A[9], a[3], Rn[9], tn[3];
    sj_camera(rec, f == b, R, t);
    traj_load_pose(S, A, a);
    const float gamma = __uint_as_float(S[12]);
    traj_compose(R, t, gamma, A, a, Rn, tn);
    traj_store_pose(out, Rn, tn);
    out[12] = __float_as_uint(gamma * __uint_as_float(rec[12]));
    out[13] = __float_as_uint(gamma);
    out[14] = S[13];
    out[15] = kAnAnchored;
}

// grid (ceil(cap / (kAnThreads * SLOTS)), L - 1), block kAnThreads; the rows as k_an_write left them
template <uint32_t SLOTS>
__global__ __launch_bounds__(kAnThreads) void k_an_land(AnArgs g) {
    const uint32_t p = blockIdx.y, cap = g.cap;
    // what the workgroup shares
    const uint32_t o = g.lrows[(size_t)p * kAnLmRowWords + 3u];
    const uint32_t* const S = an_anchored(g, o);
    float A[9], a[3];
    float gamma = 1.0f;
    if (S) {
        traj_load_pose(S, A, a);
        gamma = __uint_as_float(S[12]);
    }
    const float4* const src = g.lms + (size_t)p * cap * 2u;
    float4* const dst = g.out + (size_t)p * cap * 2u;
    uint32_t n_good = 0u, n_moved = 0u, n_dropped = 0u;  // of this wave, the same on every lane
#pragma unroll
    for (uint32_t k = 0u; k < SLOTS; k++) {
        const uint32_t s = (blockIdx.x * SLOTS + k) * kAnThreads + threadIdx.x;
        bool good = false, moved = false, dropped = false;
        if (s < cap) {
            float4 lo = src[2u * (size_t)s];
            const float4 hi = src[2u * (size_t)s + 1u];
            const uint32_t flags = __float_as_uint(lo.w);
            good = (flags & ORB_POINT_GOOD) != 0u;
            const uint32_t views = __float_as_uint(hi.x) & 0xffffu;
            if (S && good && views != 0u && __float_as_uint(hi.y) == o) {  // gamma X_o = A X_map + a, solved for X_map
                const float e0 = gamma * lo.x - a[0], e1 = gamma * lo.y - a[1], e2 = gamma * lo.z - a[2];
                const float x0 = (A[0] * e0 + A[3] * e1) + A[6] * e2;
                const float x1 = (A[1] * e0 + A[4] * e1) + A[7] * e2;
                const float x2 = (A[2] * e0 + A[5] * e1) + A[8] * e2;
                dropped = !(isfinite(x0) && isfinite(x1) && isfinite(x2));
                moved = !dropped;
                lo = dropped ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(x0, x1, x2, lo.w);
            }
            dst[2u * (size_t)s] = lo;
            dst[2u * (size_t)s + 1u] = hi;
        }
        n_good += (uint32_t)__popcll(__ballot(good));
        n_moved += (uint32_t)__popcll(__ballot(moved));
        n_dropped += (uint32_t)__popcll(__ballot(dropped));
    }
    if ((threadIdx.x & 63u) == 0u) {  // integer sums, in any order
        uint32_t* const row = g.out_rows + (size_t)p * kAnRowWords;
        if (n_good) atomicAdd(&row[0], n_good);
        if (n_moved) atomicAdd(&row[1], n_moved);
        if (n_dropped) atomicAdd(&row[2], n_dropped);
    }
}

}  // namespace orb
