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
//                 camera T's frame, the query keypoint and its ray (LC-3), compacted in the order of the query's slots by a wave
//                 ballot and a workgroup prefix (as k_loc_gather), plus the candidate of every slot (or kVerifyNone)
//   k_loc_score   of orb_kernels_localize.h, as it is, on the stage's buffers with grid.x = list entries (LC-4)
//   k_lc_refine   one workgroup per list entry: k_loc_refine's steps through the loc_* functions and GV-6's solver at 6 x 7, then
//                 LC-5's compose, the inlier bytes by query slot and the record (LC-6)
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
    const uint32_t e = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
    float4* const reca = L.reca + (size_t)e * L.cap;
    float4* const recb = L.recb + (size_t)e * L.cap;
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
        const unsigned long long bal = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base;
        for (uint32_t w = 0; w < wave; w++) off += wave_n[w];
        const uint32_t total = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
        if (i < nq) cand_of[i] = keep ? off + before : kVerifyNone;
        if (keep) {  // off + before < n_q(q) <= cap
            const float4 X = a.lms[2u * (size_t)key];
            float x, y, z;
            loc_transform(R, t, X.x, X.y, X.z, x, y, z);
            const CornerData c = cq[i];
            const float s = (float)(1u << (c.octave & 31u));
            const float u2 = ((float)c.x + 0.5f) * s - 0.5f, v2 = ((float)c.y + 0.5f) * s - 0.5f;
            reca[off + before] = make_float4(x, y, z, 0.0f);
            recb[off + before] = make_float4(u2, v2, (u2 - L.cx) / L.fx, (v2 - L.cy) / L.fy);
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0u) L.n_cand[e] = base;
}

// GV-6's solver at 6 x 7, written out here: a second inlined copy of verify_solve_n<6> in this translation unit changes the register
// allocation of k_loc_refine, which must stay as it is
__device__ __forceinline__ uint32_t lc_solve6(const float (*part)[256], float (*aug)[7], float* sol) {
    constexpr int N = 6;
    for (int i = 0, e = 0; i < N; i++)
        for (int j = i; j < N; j++, e++) aug[i][j] = aug[j][i] = part[e][0];
    for (int i = 0; i < N; i++) aug[i][N] = part[N * (N + 1) / 2 + i][0];
    uint32_t ok = 1u;
    for (int c = 0; c < N && ok; c++) {
        int piv = c;
        float pmax = fabsf(aug[c][c]);
        for (int r = c + 1; r < N; r++)
            if (fabsf(aug[r][c]) > pmax) pmax = fabsf(aug[r][c]), piv = r;
        if (pmax == 0.0f) {
            ok = 0u;
            break;
        }
        if (piv != c)
            for (int q = 0; q < N + 1; q++) {
                const float tmp = aug[c][q];
                aug[c][q] = aug[piv][q];
                aug[piv][q] = tmp;
            }
        for (int r = c + 1; r < N; r++) {
            const float f = aug[r][c] / aug[c][c];
            for (int q = c + 1; q < N + 1; q++) aug[r][q] = aug[r][q] - f * aug[c][q];
        }
    }
    if (ok)
        for (int r = N - 1; r >= 0; r--) {
            float s = aug[r][N];
            for (int q = r + 1; q < N; q++) s = s - aug[r][q] * sol[q];
            sol[r] = s / aug[r][r];
            if (!isfinite(sol[r])) ok = 0u;
        }
    return ok;
}

// grid (entries), block 256
__global__ __launch_bounds__(256) void k_lc_refine(LcArgs a) {
    __shared__ float part[kLocSums][256];  // [sum][thread]: conflict-free columns
    __shared__ float aug[6][7];
    __shared__ float sol[6];
    __shared__ float rowbuf[kLocRow];
    __shared__ float cur[12];  // the model one lane made, for every thread: the winner, then each step's
    __shared__ unsigned long long wkey[4];
    __shared__ uint32_t s_ok, s_count;
    const LocArgs& L = a.loc;
    const uint32_t e = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint2 qt = a.list[e];
    const uint32_t q = qt.x, T = qt.y;
    uint32_t o;
    float RT[9], tT[3];
    const bool nomap = !lc_target(a, T, o, RT, tT);  // uniform
    const uint32_t M = nomap ? 0u : L.n_cand[e];
    const float4* const reca = L.reca + (size_t)e * L.cap;
    const float4* const recb = L.recb + (size_t)e * L.cap;
    unsigned long long best = 0ull;
    if (M >= kLocSample)
        for (uint32_t h = tid; h < L.hyps; h += 256u) best = max(best, L.keys[(size_t)e * kVerifyMaxHyp + h]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off));
    if (lane == 0u) wkey[wave] = best;
    if (tid == 0u) s_count = 0u;
    __syncthreads();
    best = max(max(wkey[0], wkey[1]), max(wkey[2], wkey[3]));
    const bool has_min = best != 0ull;  // uniform
    const uint32_t h = has_min ? (kVerifyMaxHyp - 1u) - (uint32_t)(best & (kVerifyMaxHyp - 1u)) : 0u;
    const uint32_t n_min = has_min ? (uint32_t)(best >> 12) - 1u : 0u;
    float Rm[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, tm[3] = {0.f, 0.f, 0.f};
    float Rc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, tc[3] = {0.f, 0.f, 0.f};
    bool keep = false;
    if (has_min) {
        if (tid == 0u) {  // the winner rebuilt on one lane through an LDS row (valid: it scored a key)
            float R[9], t[3];
            (void)loc_model(reca, recb, M, lowbias32(L.seed_mix ^ e), h, rowbuf, R, t);
#pragma unroll
            for (int k = 0; k < 9; k++) cur[k] = R[k];
#pragma unroll
            for (int k = 0; k < 3; k++) cur[9 + k] = t[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 9; k++) Rc[k] = Rm[k] = cur[k];
#pragma unroll
        for (int k = 0; k < 3; k++) tc[k] = tm[k] = cur[9 + k];
        bool fit = true;
        for (uint32_t step = 0; step < kLocSteps && fit; step++) {  // LO-6; `fit` is uniform
            float acc[kLocSums];
#pragma unroll
            for (uint32_t k = 0; k < kLocSums; k++) acc[k] = 0.0f;
            for (uint32_t j = tid; j < M; j += 256u) {  // candidate j into partial sum j mod 256, ascending j; the inlier set is the winner's
                const float4 Y = reca[j], k = recb[j];
                if (loc_inlier(Rm, tm, Y.x, Y.y, Y.z, k.x, k.y, L)) loc_accumulate(acc, Rc, tc, Y, k, L);
            }
#pragma unroll
            for (uint32_t k = 0; k < kLocSums; k++) part[k][tid] = acc[k];
            __syncthreads();
            for (uint32_t s = 128u; s >= 1u; s >>= 1) {  // pairwise tree, strides 128 .. 1
                if (tid < s)
                    for (uint32_t k = 0; k < kLocSums; k++) part[k][tid] = part[k][tid] + part[k][tid + s];
                __syncthreads();
            }
            if (tid == 0u) {
                uint32_t ok = lc_solve6(part, aug, sol);
                if (ok) {
                    float R[9], t[3];
#pragma unroll
                    for (int k = 0; k < 9; k++) R[k] = Rc[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) t[k] = tc[k];
                    ok = loc_update(sol, R, t) ? 1u : 0u;
#pragma unroll
                    for (int k = 0; k < 9; k++) cur[k] = R[k];
#pragma unroll
                    for (int k = 0; k < 3; k++) cur[9 + k] = t[k];
                }
                s_ok = ok;
            }
            __syncthreads();
            fit = s_ok != 0u;
            if (fit) {
#pragma unroll
                for (int k = 0; k < 9; k++) Rc[k] = cur[k];
#pragma unroll
                for (int k = 0; k < 3; k++) tc[k] = cur[9 + k];
            }
            __syncthreads();  // s_ok and cur are read before the next step's lane writes them
        }
        if (fit) {
            uint32_t n = 0;
            for (uint32_t j = tid; j < M; j += 256u) {
                const float4 Y = reca[j], k = recb[j];
                n += loc_inlier(Rc, tc, Y.x, Y.y, Y.z, k.x, k.y, L) ? 1u : 0u;
            }
            atomicAdd(&s_count, n);
        }
        __syncthreads();
        keep = fit && 16u * s_count >= 15u * n_min;  // GV-6's rule
    }
    float Rk[9], tk[3];
#pragma unroll
    for (int k = 0; k < 9; k++) Rk[k] = keep ? Rc[k] : Rm[k];
#pragma unroll
    for (int k = 0; k < 3; k++) tk[k] = keep ? tc[k] : tm[k];
    // LC-6: an inlier byte per keypoint slot of frame q: one write each (cand_of is written below n_q(q) of an entry that is not NOMAP)
    const uint32_t nq = has_min ? lc_nq(a, q) : 0u;
    const uint32_t* const cand_of = L.cand_of + (size_t)e * L.cap;
    uint8_t* const mask = L.mask + (size_t)e * L.cap;
    for (uint32_t i = tid; i < L.cap; i += 256u) {
        uint8_t b = 0;
        if (i < nq) {
            const uint32_t j = cand_of[i];
            if (j != kVerifyNone) {
                const float4 Y = reca[j], k = recb[j];
                b = loc_inlier(Rk, tk, Y.x, Y.y, Y.z, k.x, k.y, L) ? 1 : 0;
            }
        }
        mask[i] = b;
    }
    if (tid == 0u) {  // the record
        uint32_t* const out = L.fix + (size_t)e * kLcFixWords;
        // LC-5: camera q in segment o's frame, R Rt after one polar step and R tT + t; zeros when an entry is not finite
        float Rp[9], tp[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) Rp[3 * r + c] = (Rk[3 * r] * RT[c] + Rk[3 * r + 1] * RT[3 + c]) + Rk[3 * r + 2] * RT[6 + c];
            tp[r] = ((Rk[3 * r] * tT[0] + Rk[3 * r + 1] * tT[1]) + Rk[3 * r + 2] * tT[2]) + 1.0f * tk[r];
        }
        traj_polar_step(Rp);
        bool fin = has_min;
#pragma unroll
        for (int k = 0; k < 9; k++) fin = fin && isfinite(Rp[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) fin = fin && isfinite(tp[k]);
#pragma unroll
        for (int k = 0; k < 9; k++) out[k] = has_min ? __float_as_uint(Rk[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) out[9 + k] = has_min ? __float_as_uint(tk[k]) : 0u;
        out[12] = has_min ? __float_as_uint(sqrtf((tk[0] * tk[0] + tk[1] * tk[1]) + tk[2] * tk[2])) : 0u;
#pragma unroll
        for (int k = 0; k < 9; k++) out[13 + k] = fin ? __float_as_uint(Rp[k]) : 0u;
#pragma unroll
        for (int k = 0; k < 3; k++) out[22 + k] = fin ? __float_as_uint(tp[k]) : 0u;
        out[25] = has_min ? o : 0u;
        out[26] = has_min ? (q < a.traj_frames ? a.frames[(size_t)q * kLcFrameWords + 14u] : kLcNone) : 0u;
        out[27] = has_min ? M : 0u;
        out[28] = has_min ? (keep ? s_count : n_min) : 0u;
        out[29] = h;
        out[30] = nomap ? (uint32_t)ORB_LOCALIZE_NOMAP
                  : M < kLocSample ? (uint32_t)ORB_LOCALIZE_FEW
                  : !has_min ? (uint32_t)ORB_LOCALIZE_DEGENERATE
                  : keep ? (uint32_t)ORB_LOCALIZE_OK
                         : (uint32_t)ORB_LOCALIZE_MINIMAL;
        out[31] = 0u;
    }
}

}  // namespace orb
