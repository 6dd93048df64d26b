// orb_kernels_remap.h -- the corrected map in one root frame (not in the reference; the definition is the build's own, RM-1..RM-6 in
// DESIGN.md section 31).  orb_graph_pairs leaves corrected cameras per segment, orb_join_pairs every segment's similarity to its
// root; this stage puts the two together: every frame's camera, the graph's where the graph moved it, composed with its segment's
// similarity, and every GOOD landmark carried along -- first with the camera of its first view, from where the trajectory had that
// camera to where the graph put it, then through the similarity into the root's frame and unit.  Nothing is triangulated again.
// Every binary32 operation below is written out in the order the definition gives (-ffp-contract=off), so the CPU restatement
// (tests/remap_ref.py) reproduces every bit.
//
//   k_rm_pose   a thread per frame: RM-2..RM-4 (traj_compose of orb_kernels_traj.h), and the row of pair f with its counts at 0
//   k_rm_land   grid (ceil(cap / (256 S)), pairs), S slots per thread: RM-5.  A record is two 16-byte loads and two 16-byte stores
//               per lane, coalesced over the row; what a workgroup shares -- the two poses of frame p, the row's origin, its
//               similarity -- sits at addresses that depend on blockIdx only; the counts of RM-6 are wave ballots and one integer
//               atomicAdd per wave and count
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_traj.h"

namespace orb {

constexpr uint32_t kRmThreads = 256u;
constexpr uint32_t kRmFrameWords = 20u;  // OrbFramePose
constexpr uint32_t kRmGraphWords = 16u;  // OrbGraphPose
constexpr uint32_t kRmSegWords = 16u;    // OrbJoinSegment
constexpr uint32_t kRmPoseWords = 16u;   // OrbRemapPose
constexpr uint32_t kRmRowWords = 4u;     // OrbLandmarkRow, OrbRemapRow
constexpr uint32_t kRmNone = 0xffffffffu;
constexpr uint32_t kRmFromGraph = 1u, kRmMoved = 2u;  // OrbRemapPose.status (ORB_REMAP_FROM_GRAPH, ORB_REMAP_MOVED)
constexpr uint32_t kRmSegLinked = 2u;                 // ORB_JOIN_SEGMENT_LINKED
constexpr uint32_t kRmGraphRefined = 2u, kRmGraphFailed = 4u;  // ORB_GRAPH_REFINED .. ORB_GRAPH_FAILED: the statuses of a moved camera

struct RmArgs {
    const uint32_t* __restrict__ frames;  // [F][kRmFrameWords] of the last orb_trajectory_consecutive
    const uint32_t* __restrict__ gposes;  // [F][kRmGraphWords] of the last orb_graph_pairs; null: the graph is no source
    const uint32_t* __restrict__ segs;    // [F][kRmSegWords] of the last orb_join_pairs; null: the join is no source
    const float4* __restrict__ lms;       // [pairs][cap][2] OrbLandmark of the last orb_landmarks_consecutive
    const uint32_t* __restrict__ lrows;   // [pairs][kRmRowWords] its rows
    uint32_t cap;
    uint32_t n_frames;                    // F
    uint32_t n_pairs;                     // P_l
    uint32_t* __restrict__ poses;         // [F][kRmPoseWords] OrbRemapPose
    uint32_t* __restrict__ rows;          // [pairs][kRmRowWords] OrbRemapRow
    float4* __restrict__ out;             // [pairs][cap][2] OrbLandmark
};

// RM-2: the graph moved frame f
__device__ __forceinline__ bool rm_from_graph(const RmArgs& g, uint32_t f) {
    if (!g.gposes) return false;
    const uint32_t st = g.gposes[(size_t)f * kRmGraphWords + 15u];
    return st >= kRmGraphRefined && st <= kRmGraphFailed;
}

// RM-3: the segment record of origin b when it is LINKED, else null
__device__ __forceinline__ const uint32_t* rm_similarity(const RmArgs& g, uint32_t b) {
    if (!g.segs || b >= g.n_frames) return nullptr;
    const uint32_t* const S = g.segs + (size_t)b * kRmSegWords;
    return S[15] == kRmSegLinked ? S : nullptr;
}

// grid ceil(F / kRmThreads), block kRmThreads
__global__ __launch_bounds__(kRmThreads) void k_rm_pose(RmArgs g) {
    const uint32_t f = blockIdx.x * kRmThreads + threadIdx.x;
    if (f >= g.n_frames) return;
    if (f < g.n_pairs) {  // RM-6: the counts at 0, the row's root
        const uint32_t o = g.lrows[(size_t)f * kRmRowWords + 3u];
        const uint32_t* const S = rm_similarity(g, o);
        uint32_t* const row = g.rows + (size_t)f * kRmRowWords;
        row[0] = 0u;
        row[1] = 0u;
        row[2] = 0u;
        row[3] = S ? S[13] : o;
    }
    const uint32_t* const rec = g.frames + (size_t)f * kRmFrameWords;
    uint32_t* const out = g.poses + (size_t)f * kRmPoseWords;
    const bool fg = rm_from_graph(g, f);
    const uint32_t* const cam = fg ? g.gposes + (size_t)f * kRmGraphWords : rec;  // RM-2
    const uint32_t b = rec[14];
    const uint32_t* const S = rm_similarity(g, b);
    const uint32_t status = fg ? kRmFromGraph : 0u;
    if (!S) {
#pragma unroll
        for (int k = 0; k < 12; k++) out[k] = cam[k];
        out[12] = rec[12];
        out[13] = __float_as_uint(1.0f);
        out[14] = b;
        out[15] = status;
        return;
    }
    float R[9], t[3], A[9], a[3], Rn[9], tn[3];
    traj_load_pose(cam, R, t);
    traj_load_pose(S, A, a);
    const float sigma = __uint_as_float(S[12]);
    traj_compose(R, t, sigma, A, a, Rn, tn);
    traj_store_pose(out, Rn, tn);
    out[12] = __float_as_uint(sigma * __uint_as_float(rec[12]));
    out[13] = __float_as_uint(sigma);
    out[14] = S[13];
    out[15] = status | kRmMoved;
}

// grid (ceil(cap / (kRmThreads * SLOTS)), P_l), block kRmThreads; the rows as k_rm_pose left them
template <uint32_t SLOTS>
__global__ __launch_bounds__(kRmThreads) void k_rm_land(RmArgs g) {
    const uint32_t p = blockIdx.y, F = g.n_frames, cap = g.cap;
    // what the workgroup shares
    const uint32_t o = g.lrows[(size_t)p * kRmRowWords + 3u];
    const uint32_t* const rec = g.frames + (size_t)p * kRmFrameWords;  // p < P_l <= F - 1
    const bool anchor = o < F && p != o && rec[14] == o && rm_from_graph(g, p);
    const uint32_t* const S = o < F ? rm_similarity(g, o) : nullptr;
    float R[9], t[3], Rg[9], tg[3], A[9], a[3];
    float sigma = 1.0f;
    uint32_t root = o;
    if (anchor) {
        traj_load_pose(rec, R, t);
        traj_load_pose(g.gposes + (size_t)p * kRmGraphWords, Rg, tg);
    }
    if (S) {
        traj_load_pose(S, A, a);
        sigma = __uint_as_float(S[12]);
        root = S[13];
    }
    const bool steps = anchor || S != nullptr;
    const float4* const src = g.lms + (size_t)p * cap * 2u;
    float4* const dst = g.out + (size_t)p * cap * 2u;
    uint32_t n_good = 0u, n_moved = 0u, n_dropped = 0u;  // of this wave, the same on every lane
#pragma unroll
    for (uint32_t k = 0u; k < SLOTS; k++) {
        const uint32_t s = (blockIdx.x * SLOTS + k) * kRmThreads + threadIdx.x;
        bool good = false, moved = false, dropped = false;
        if (s < cap) {
            float4 lo = src[2u * (size_t)s], hi = src[2u * (size_t)s + 1u];
            const uint32_t flags = __float_as_uint(lo.w);
            good = (flags & ORB_POINT_GOOD) != 0u;
            const uint32_t views = __float_as_uint(hi.x) & 0xffffu;
            if (steps && good && views != 0u && __float_as_uint(hi.y) == o) {
                float x0 = lo.x, x1 = lo.y, x2 = lo.z;
                if (anchor) {  // into camera p as the trajectory has it, out of camera p as the graph has it
                    const float c0 = ((R[0] * x0 + R[1] * x1) + R[2] * x2) + t[0];
                    const float c1 = ((R[3] * x0 + R[4] * x1) + R[5] * x2) + t[1];
                    const float c2 = ((R[6] * x0 + R[7] * x1) + R[8] * x2) + t[2];
                    const float d0 = c0 - tg[0], d1 = c1 - tg[1], d2 = c2 - tg[2];
                    x0 = (Rg[0] * d0 + Rg[3] * d1) + Rg[6] * d2;
                    x1 = (Rg[1] * d0 + Rg[4] * d1) + Rg[7] * d2;
                    x2 = (Rg[2] * d0 + Rg[5] * d1) + Rg[8] * d2;
                }
                if (S) {  // sigma X_o = A X_root + a, solved for X_root
                    const float e0 = sigma * x0 - a[0], e1 = sigma * x1 - a[1], e2 = sigma * x2 - a[2];
                    x0 = (A[0] * e0 + A[3] * e1) + A[6] * e2;
                    x1 = (A[1] * e0 + A[4] * e1) + A[7] * e2;
                    x2 = (A[2] * e0 + A[5] * e1) + A[8] * e2;
                    hi.y = __uint_as_float(root);
                }
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
    if ((threadIdx.x & 63u) == 0u) {  // RM-6: integer sums, in any order
        uint32_t* const row = g.rows + (size_t)p * kRmRowWords;
        if (n_good) atomicAdd(&row[0], n_good);
        if (n_moved) atomicAdd(&row[1], n_moved);
        if (n_dropped) atomicAdd(&row[2], n_dropped);
    }
}

}  // namespace orb
