// orb_kernels_localize.h -- absolute pose of camera f + 1 relative to camera f from the map points of the pair before (not in the
// reference; the definition is the build's own, LO-1..LO-7 in DESIGN.md section 21): pair f - 1 of the last orb_pose_consecutive
// triangulated landmarks from cameras f - 1 and f, the matcher's records carry each of them on to a keypoint of frame f + 1, and
// those 3D-2D correspondences give R and a metric t (in units of pair f - 1's baseline) by a RANSAC over six-point DLT samples and
// four Gauss-Newton steps on the winner's inliers.  Pair f's fundamental matrix is not used.  Every binary32 operation below is
// written out in the order the definition gives (-ffp-contract=off, correctly rounded division and square root), so the CPU
// restatement (tests/localize_ref.py) reproduces every bit.
//
//   k_loc_gather   one workgroup per pair: the two match hops, the landmark in camera f's frame, the keypoint and its ray (LO-1),
//                  compacted in the order of frame f - 1's slots by a wave ballot and a workgroup prefix (as k_verify_gather), plus
//                  the candidate of every slot (or kVerifyNone)
//   k_loc_score    grid (pair, 64-hypothesis block), 256 threads: wave 0 builds hypothesis 64 * block + l on lane l (LO-2..LO-4),
//                  eliminating the 11 x 12 system with complete pivoting in a padded LDS row of its own (pivots found at run time
//                  would send a private array to scratch; the column permutation is twelve nibbles of a register pair); the 64
//                  poses go through LDS to all four waves; the candidates pass through LDS in tiles of 256 and are read as
//                  broadcasts, each wave every fourth one; one packed key per hypothesis (LO-5)
//   k_loc_refine   one workgroup per pair: loc_fit -- the best key, the winner rebuilt on one lane, four rounds of the 27
//                  normal-equation sums in GV-6's order and tree with GV-6's solve at 6 x 7 and the update on one lane (LO-6), the
//                  refit scored and kept or not --, then the inlier bytes and the record (LO-7)
// The bridge, the loop stage and the adjustment fit poses to 3D-2D correspondences too, and call what is here: k_loc_score as it
// is, loc_fit, the gathers' loc_compact and loc_candidate, loc_accumulate and loc_update.  LO-6 is stated once.
#pragma once
#include "orb_kernels_pose.h"

namespace orb {

constexpr uint32_t kLocSeedSalt = 0x4C4F3031u;  // LO-2: the draw stream's seed is lowbias32(seed ^ kLocSeedSalt)
constexpr uint32_t kLocDraws = 32u;             // LO-2: draws per hypothesis
constexpr uint32_t kLocSample = 6u;             // LO-3: points of a minimal sample; a pair with fewer candidates is ORB_LOCALIZE_FEW
constexpr uint32_t kLocRow = 133u;              // words of one lane's 11 x 12 system in LDS: 132 + 1, an odd stride (no bank conflicts)
constexpr float kLocPivotRatio = 1.0f / 4194304.0f;  // LO-3: degenerate when |last pivot| <= 2^-22 |first pivot|
constexpr uint32_t kLocSums = 27u;              // LO-6: 21 entries of the upper triangle of the 6 x 6 normal matrix + 6 of the right side
constexpr uint32_t kLocSteps = 4u;              // LO-6: Gauss-Newton steps
constexpr uint32_t kLocFixWords = 20u;          // OrbFrameFix

struct LocArgs {
    const uint32_t* counts;      // [frames] raw counters of the batch
    const CornerData* corners;   // [frames][cap]
    const MatchRecord* matches;  // [frames][cap]
    uint32_t cap;
    const uint32_t* poses;       // [pairs][kPoseWords] OrbPairPose of the last pose call
    const float4* points;        // [pairs][cap] its OrbPoint
    uint32_t hyps;               // 1..kVerifyMaxHyp
    uint32_t max_distance;
    float ratio;
    float fx, fy, cx, cy;        // the intrinsics given to the pose call
    float r2;                    // LO-5: max_reproj_px squared
    uint32_t seed_mix;           // lowbias32(seed ^ kLocSeedSalt)
    float4* reca;                // [pairs][cap] candidates: (Yx, Yy, Yz, 0), the landmark in camera f's frame
    float4* recb;                // [pairs][cap] candidates: (u2, v2, dx, dy), the keypoint of frame f + 1 and its ray
    uint32_t* cand_of;           // [pairs][cap] candidate of slot i of frame f - 1 (kVerifyNone: not a candidate); i < n_q(f - 1) only
    uint32_t* n_cand;            // [pairs]
    unsigned long long* keys;    // [pairs][kVerifyMaxHyp]
    uint32_t* fix;               // [pairs][kLocFixWords] OrbFrameFix
    uint8_t* mask;               // [pairs][cap]
};

// LO-1: pair 0 has no earlier points, and a pose that is not OK gives none that can be used
__device__ __forceinline__ bool loc_nomap(const LocArgs& a, uint32_t pair) {
    return pair == 0u || a.poses[(size_t)(pair - 1u) * kPoseWords + 15u] != ORB_POSE_OK;
}

// LO-2: six distinct candidate indices of hypothesis h in draw order, or false after 32 draws (all 32 are evaluated; the ones after
// the sixth index change nothing)
__device__ __forceinline__ bool loc_sample(uint32_t pair_mix, uint32_t h, uint32_t M, uint32_t js[kLocSample]) {
    uint32_t n = 0;
#pragma unroll
    for (uint32_t s = 0; s < kLocSample; s++) js[s] = 0u;
#pragma unroll
    for (uint32_t d = 0; d < kLocDraws; d++) {
        const uint32_t j = (uint32_t)(((unsigned long long)lowbias32(pair_mix ^ ((h << 5) | d)) * M) >> 32);
        bool dup = false;
#pragma unroll
        for (uint32_t s = 0; s < kLocSample; s++) dup = dup || (s < n && js[s] == j);
        const bool take = n < kLocSample && !dup;
#pragma unroll
        for (uint32_t s = 0; s < kLocSample; s++) js[s] = take && n == s ? j : js[s];
        n += take ? 1u : 0u;
    }
    return n == kLocSample;
}

// RP-4's step `Steps` times; false when a det is not finite or not > 0
template <int Steps>
__device__ __forceinline__ bool loc_polar(float r[9]) {
    bool ok = true;
#pragma unroll
    for (int s = 0; s < Steps; s++) {
        float c[9];
        pose_cof(r, c);
        const float det = (r[0] * c[0] + r[1] * c[1]) + r[2] * c[2];
        ok = ok && isfinite(det) && det > 0.0f;
#pragma unroll
        for (int k = 0; k < 9; k++) r[k] = 0.5f * (r[k] + c[k] / det);
    }
    return ok;
}

// LO-3 on one lane's 11 x 12 system `a` (row-major, LDS): complete pivoting as EP-3 -- the first maximal |a| of the remaining block
// in row-major order, its row and column swapped into place (every row's column), the column permutation kept as nibbles --
// elimination, the unpivoted column's unknown 1, back substitution, the columns put back.  False: degenerate (a zero pivot, a last
// pivot at most 2^-22 of the first, or a non-finite entry).
__device__ __forceinline__ bool loc_null(float* a, float P[12]) {
    unsigned long long perm = 0xBA9876543210ull;  // nibble c: the original column now at c
    bool ok = true;
    float p0 = 0.0f;
#pragma unroll
    for (int r = 0; r < 11; r++) {
        float pmax = -1.0f;
        int pi = r, pj = r;
#pragma unroll
        for (int i = r; i < 11; i++)
#pragma unroll
            for (int j = r; j < 12; j++) {
                const float v = fabsf(a[i * 12 + j]);
                const bool gt = v > pmax;
                pmax = gt ? v : pmax;
                pi = gt ? i : pi;
                pj = gt ? j : pj;
            }
        ok = ok && pmax != 0.0f;
        if (r == 0) p0 = pmax;
#pragma unroll
        for (int c = 0; c < 12; c++) {  // rows r <-> pi
            const float t = a[r * 12 + c];
            a[r * 12 + c] = a[pi * 12 + c];
            a[pi * 12 + c] = t;
        }
#pragma unroll
        for (int i = 0; i < 11; i++) {  // columns r <-> pj
            const float t = a[i * 12 + r];
            a[i * 12 + r] = a[i * 12 + pj];
            a[i * 12 + pj] = t;
        }
        const unsigned long long nr = (perm >> (4 * r)) & 15ull, nj = (perm >> (4 * pj)) & 15ull;
        perm = (perm & ~(15ull << (4 * r)) & ~(15ull << (4 * pj))) | (nj << (4 * r)) | (nr << (4 * pj));
#pragma unroll
        for (int q = r + 1; q < 11; q++) {
            const float f = a[q * 12 + r] / a[r * 12 + r];
#pragma unroll
            for (int c = r + 1; c < 12; c++) a[q * 12 + c] = a[q * 12 + c] - f * a[r * 12 + c];
        }
    }
    ok = ok && !(fabsf(a[10 * 12 + 10]) <= kLocPivotRatio * p0);
    float x[12];
    x[11] = 1.0f;
#pragma unroll
    for (int r = 10; r >= 0; r--) {
        float s = 0.0f;
#pragma unroll
        for (int q = r + 1; q < 12; q++) s = s - a[r * 12 + q] * x[q];
        x[r] = s / a[r * 12 + r];
        ok = ok && isfinite(x[r]);
    }
    // the columns put back through the lane's own LDS row (its first twelve words are no longer needed)
#pragma unroll
    for (int c = 0; c < 12; c++) a[(perm >> (4 * c)) & 15ull] = x[c];
#pragma unroll
    for (int e = 0; e < 12; e++) P[e] = a[e];
    return ok;
}

// LO-4: the pose of a row-major 3 x 4 P = s [R | t], s of either sign: the sign from det of the left 3 x 3, the scale from its
// Frobenius norm, three polar steps towards the nearest rotation.  False: invalid.
__device__ __forceinline__ bool loc_pose(float P[12], float R[9], float t[3]) {
    float m[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]}, c[9];
    pose_cof(m, c);
    const float det = (m[0] * c[0] + m[1] * c[1]) + m[2] * c[2];
    bool ok = isfinite(det) && det != 0.0f;
    const bool neg = det < 0.0f;
#pragma unroll
    for (int e = 0; e < 12; e++) P[e] = neg ? -P[e] : P[e];
#pragma unroll
    for (int k = 0; k < 9; k++) m[k] = neg ? -m[k] : m[k];
    float s = m[0] * m[0];
#pragma unroll
    for (int k = 1; k < 9; k++) s = s + m[k] * m[k];
    const float n = sqrtf(s / 3.0f);
    ok = ok && isfinite(n) && n > 0.0f;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = m[k] / n;
    ok = loc_polar<3>(R) && ok;
    t[0] = P[3] / n;
    t[1] = P[7] / n;
    t[2] = P[11] / n;
    return ok;
}

// LO-2..LO-4: the minimal model of hypothesis h, through the LDS row `a` of the calling lane; false: invalid / degenerate
__device__ __forceinline__ bool loc_model(const float4* __restrict__ reca, const float4* __restrict__ recb, uint32_t M, uint32_t pair_mix,
                                          uint32_t h, float* a, float R[9], float t[3]) {
    uint32_t js[kLocSample];
    if (!loc_sample(pair_mix, h, M, js)) return false;
#pragma unroll
    for (int s = 0; s < (int)kLocSample; s++) {  // LO-3: two rows per sample point, without the twelfth
        const float4 Y = reca[js[s]], k = recb[js[s]];
        float* const r1 = a + 24 * s;
        r1[0] = Y.x;
        r1[1] = Y.y;
        r1[2] = Y.z;
        r1[3] = 1.0f;
        r1[4] = r1[5] = r1[6] = r1[7] = 0.0f;
        r1[8] = -(k.z * Y.x);
        r1[9] = -(k.z * Y.y);
        r1[10] = -(k.z * Y.z);
        r1[11] = -k.z;
        if (s < (int)kLocSample - 1) {
            float* const r2 = r1 + 12;
            r2[0] = r2[1] = r2[2] = r2[3] = 0.0f;
            r2[4] = Y.x;
            r2[5] = Y.y;
            r2[6] = Y.z;
            r2[7] = 1.0f;
            r2[8] = -(k.w * Y.x);
            r2[9] = -(k.w * Y.y);
            r2[10] = -(k.w * Y.z);
            r2[11] = -k.w;
        }
    }
    float P[12];
    const bool ok = loc_null(a, P);
    return loc_pose(P, R, t) && ok;
}

// Y' = R Y + t in RP-5's order
__device__ __forceinline__ void loc_transform(const float R[9], const float t[3], float Yx, float Yy, float Yz, float& x, float& y, float& z) {
    x = ((R[0] * Yx + R[1] * Yy) + R[2] * Yz) + t[0];
    y = ((R[3] * Yx + R[4] * Yy) + R[5] * Yz) + t[1];
    z = ((R[6] * Yx + R[7] * Yy) + R[8] * Yz) + t[2];
}

// LO-5: in front of camera f + 1 and within max_reproj_px of the keypoint, without a division; a NaN fails
__device__ __forceinline__ bool loc_inlier(const float R[9], const float t[3], float Yx, float Yy, float Yz, float u2, float v2, const LocArgs& a) {
    float x, y, z;
    loc_transform(R, t, Yx, Yy, Yz, x, y, z);
    const float ex = a.fx * x + (a.cx - u2) * z, ey = a.fy * y + (a.cy - v2) * z;
    return z > 0.0f && ex * ex + ey * ey <= a.r2 * (z * z);
}

// LO-6: the two Jacobian rows in (omega, delta t) of point Y seen at (u2, v2) under (R, t), added to the 27 sums in GV-6's order.
// `g` gives the intrinsics (LocArgs, or the adjustment's BaArgs); returns the squared residual, which only BA-4 sums.
template <class Intr>
__device__ __forceinline__ float loc_accumulate(float* acc, const float R[9], const float t[3], const float4& Y, float u2, float v2, const Intr& g) {
    float x, y, z;
    loc_transform(R, t, Y.x, Y.y, Y.z, x, y, z);
    const float ex = (g.fx * (x / z) + g.cx) - u2, ey = (g.fy * (y / z) + g.cy) - v2;
    const float a = g.fx / z, b = -((g.fx * x / z) / z), c = g.fy / z, d = -((g.fy * y / z) / z);
    const float J1[6] = {b * y, a * z - b * x, -(a * y), a, 0.0f, b};
    const float J2[6] = {d * y - c * z, -(d * x), c * x, 0.0f, c, d};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = i; j < 6; j++, e++) acc[e] = acc[e] + (J1[i] * J1[j] + J2[i] * J2[j]);
#pragma unroll
    for (int i = 0; i < 6; i++) acc[21 + i] = acc[21 + i] + -(J1[i] * ex + J2[i] * ey);
    return ex * ex + ey * ey;
}

// LO-6 on one lane: omega and delta t from the solution, R <- (I + [omega]x) R, t <- (I + [omega]x) t + delta t, two polar steps.
// False: a non-finite entry or an invalid polar det.
__device__ __forceinline__ bool loc_update(const float* sol, float R[9], float t[3]) {
    const float W[9] = {1.0f, -sol[2], sol[1], sol[2], 1.0f, -sol[0], -sol[1], sol[0], 1.0f};
    float Rn[9], tn[3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (W[3 * r] * R[c] + W[3 * r + 1] * R[3 + c]) + W[3 * r + 2] * R[6 + c];
        tn[r] = ((W[3 * r] * t[0] + W[3 * r + 1] * t[1]) + W[3 * r + 2] * t[2]) + sol[3 + r];
    }
    bool ok = loc_polar<2>(Rn);
#pragma unroll
    for (int k = 0; k < 9; k++) {
        ok = ok && isfinite(Rn[k]);
        R[k] = Rn[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ok = ok && isfinite(tn[k]);
        t[k] = tn[k];
    }
    return ok;
}

// The compaction step of the PnP gathers (k_loc_gather, k_br_gather, k_lc_gather), by all 256 threads on one tile of 256: the
// slot of a kept candidate -- `base`, the kept ones of the waves below, the kept lanes below in its own wave -- and the tile's
// total, by a wave ballot and a prefix over wave_n.  Its barrier publishes wave_n; the caller's barrier at the end of the tile
// keeps the next tile's writes behind these reads.
__device__ __forceinline__ uint32_t loc_compact(bool keep, uint32_t base, uint32_t wave_n[4], uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(keep);
    const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t off = base;
    for (uint32_t w = 0; w < wave; w++) off += wave_n[w];
    total = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
    return off + before;
}

// LO-1: the two records of candidate `slot` of row `row`: the landmark (x, y, z) in the earlier camera's frame with the word w, the
// keypoint c in level-0 pixels (orb_corner_level0_xy) and its ray
__device__ __forceinline__ void loc_record(const LocArgs& a, uint32_t row, uint32_t slot, float x, float y, float z, const CornerData& c, float w) {
    const float s = (float)(1u << (c.octave & 31u));
    const float u2 = ((float)c.x + 0.5f) * s - 0.5f, v2 = ((float)c.y + 0.5f) * s - 0.5f;
    a.reca[(size_t)row * a.cap + slot] = make_float4(x, y, z, w);
    a.recb[(size_t)row * a.cap + slot] = make_float4(u2, v2, (u2 - a.cx) / a.fx, (v2 - a.cy) / a.fy);
}

// LO-1: candidate `slot` of row `row`: the landmark X under (R, t) with the word w, and the keypoint c
__device__ __forceinline__ void loc_candidate(const LocArgs& a, uint32_t row, uint32_t slot, const float4& X, const float R[9], const float t[3],
                                              const CornerData& c, float w) {
    float x, y, z;
    loc_transform(R, t, X.x, X.y, X.z, x, y, z);
    loc_record(a, row, slot, x, y, z, c, w);
}

// grid (pairs), block 256
__global__ __launch_bounds__(256) void k_loc_gather(LocArgs a) {
    __shared__ uint32_t wave_n[4];
    const uint32_t pair = blockIdx.x, tid = threadIdx.x;
    if (loc_nomap(a, pair)) {  // uniform
        if (tid == 0u) a.n_cand[pair] = 0u;
        return;
    }
    const uint32_t n0 = min(a.counts[pair - 1u], a.cap), n1 = min(a.counts[pair], a.cap), n2 = min(a.counts[pair + 1u], a.cap);
    const MatchRecord* const m0 = a.matches + (size_t)(pair - 1u) * a.cap;
    const MatchRecord* const m1 = a.matches + (size_t)pair * a.cap;
    const float4* const pts = a.points + (size_t)(pair - 1u) * a.cap;
    const CornerData* const ct = a.corners + (size_t)(pair + 1u) * a.cap;
    const uint32_t* const pose = a.poses + (size_t)(pair - 1u) * kPoseWords;
    uint32_t* const cand_of = a.cand_of + (size_t)pair * a.cap;
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = __uint_as_float(pose[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = __uint_as_float(pose[9 + k]);
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < n0; i0 += 256u) {
        const uint32_t i = i0 + tid;
        bool keep = false;
        uint32_t k = 0;
        float4 X = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < n0) {  // LO-1: a GOOD point, its keypoint in frame f, that keypoint's match in frame f + 1 under GV-1's filter
            X = pts[i];
            const uint32_t j = m0[i].index;
            if ((__float_as_uint(X.w) & ORB_POINT_GOOD) != 0u && j < n1) {
                const MatchRecord m = m1[j];
                const uint32_t d = m.dist & 0xffffu, second = m.dist >> 16;
                k = m.index;
                keep = k != kVerifyNone && k < n2 && d <= a.max_distance && (float)d < a.ratio * (float)second;
            }
        }
        uint32_t total;
        const uint32_t slot = loc_compact(keep, base, wave_n, total);
        if (i < n0) cand_of[i] = keep ? slot : kVerifyNone;
        if (keep) loc_candidate(a, pair, slot, X, R, t, ct[k], 0.0f);
        base += total;
        __syncthreads();
    }
    if (tid == 0u) a.n_cand[pair] = base;
}

// grid (pairs, ceil(hyps / 64)), block 256
__global__ __launch_bounds__(256) void k_loc_score(LocArgs a) {
    __shared__ float mat[kVerifyHypPerWg * kLocRow];
    __shared__ float models[12][kVerifyHypPerWg];
    __shared__ uint32_t valid_mask[2];
    __shared__ float4 tile_y[256];
    __shared__ float2 tile_k[256];
    __shared__ uint32_t cnt[4][kVerifyHypPerWg];
    const uint32_t pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t M = a.n_cand[pair];
    if (M < kLocSample) return;  // uniform: k_loc_refine reads no key of such a pair
    const float4* const reca = a.reca + (size_t)pair * a.cap;
    const float4* const recb = a.recb + (size_t)pair * a.cap;
    const uint32_t h = blockIdx.y * kVerifyHypPerWg + lane;
    if (wave == 0u) {
        float R[9], t[3];
        const bool valid = h < a.hyps && loc_model(reca, recb, M, lowbias32(a.seed_mix ^ pair), h, mat + lane * kLocRow, R, t);
#pragma unroll
        for (int e = 0; e < 9; e++) models[e][lane] = valid ? R[e] : 0.0f;  // an invalid hypothesis: z' = 0, never an inlier
#pragma unroll
        for (int e = 0; e < 3; e++) models[9 + e][lane] = valid ? t[e] : 0.0f;
        const unsigned long long vb = __ballot(valid);
        if (lane == 0u) {
            valid_mask[0] = (uint32_t)vb;
            valid_mask[1] = (uint32_t)(vb >> 32);
        }
    }
    __syncthreads();
    float R[9], t[3];
#pragma unroll
    for (int e = 0; e < 9; e++) R[e] = models[e][lane];
#pragma unroll
    for (int e = 0; e < 3; e++) t[e] = models[9 + e][lane];
    const bool valid = ((valid_mask[lane >> 5] >> (lane & 31u)) & 1u) != 0u;
    uint32_t n = 0;
    for (uint32_t c0 = 0; c0 < M; c0 += 256u) {
        const uint32_t tn = min(M - c0, 256u);
        if (tid < tn) {
            const float4 k = recb[c0 + tid];
            tile_y[tid] = reca[c0 + tid];
            tile_k[tid] = make_float2(k.x, k.y);
        }
        __syncthreads();
#pragma unroll 4
        for (uint32_t q = wave; q < tn; q += 4u) {
            const float4 Y = tile_y[q];
            const float2 k = tile_k[q];
            n += loc_inlier(R, t, Y.x, Y.y, Y.z, k.x, k.y, a) ? 1u : 0u;
        }
        __syncthreads();
    }
    cnt[wave][lane] = n;
    __syncthreads();
    if (wave == 0u && h < a.hyps) {
        const uint32_t total = (cnt[0][lane] + cnt[1][lane]) + (cnt[2][lane] + cnt[3][lane]);
        a.keys[(size_t)pair * kVerifyMaxHyp + h] = valid ? (((unsigned long long)(total + 1u) << 12) | (kVerifyMaxHyp - 1u - h)) : 0ull;
    }
}

// What loc_fit found for one row, the same on every thread
struct LocFit {
    bool has_min, keep;   // a hypothesis scored a key; the refit replaced it
    uint32_t h, n_min;    // the winner and its inlier count (0, 0 without one)
    uint32_t inliers;     // of the kept model (0 without one)
    float R[9], t[3];     // the kept model (zeros without one)
};

// LO-7's status; the bridge and the loop stage write the same five-way choice
__device__ __forceinline__ uint32_t loc_status(bool nomap, uint32_t M, bool has_min, bool keep) {
    return nomap ? (uint32_t)ORB_LOCALIZE_NOMAP
           : M < kLocSample ? (uint32_t)ORB_LOCALIZE_FEW
           : !has_min ? (uint32_t)ORB_LOCALIZE_DEGENERATE
           : keep ? (uint32_t)ORB_LOCALIZE_OK
                  : (uint32_t)ORB_LOCALIZE_MINIMAL;
}

// The first thirteen words of a fix record: r, t and the step |t| of the kept model, zeros without one
__device__ __forceinline__ void loc_put_pose(uint32_t* out, const LocFit& f) {
#pragma unroll
    for (int e = 0; e < 9; e++) out[e] = f.has_min ? __float_as_uint(f.R[e]) : 0u;
#pragma unroll
    for (int e = 0; e < 3; e++) out[9 + e] = f.has_min ? __float_as_uint(f.t[e]) : 0u;
    out[12] = f.has_min ? __float_as_uint(sqrtf((f.t[0] * f.t[0] + f.t[1] * f.t[1]) + f.t[2] * f.t[2])) : 0u;
}

// The fit of row `row` with M candidates (0 for a row without a map), called by all 256 threads of the three refine kernels
// (k_loc_refine, k_br_refine, k_lc_refine) with the row's keys in place: the best key, the winner rebuilt on one lane, LO-6's four
// rounds -- the 27 sums in GV-6's order and tree, GV-6's solve at 6 x 7 and the update on one lane --, the refit scored and kept
// under GV-6's rule or not.  The draw stream is lowbias32(seed_mix ^ row), as k_loc_score's.  The shared arrays are the
// function's own, as verify_refine_body's; its first barrier is unconditional and also publishes what the caller wrote to LDS
// before the call.
__device__ __forceinline__ LocFit loc_fit(const LocArgs& a, uint32_t row, uint32_t M) {
    __shared__ float part[kLocSums][256];  // [sum][thread]: conflict-free columns
    __shared__ float aug[6][7];
    __shared__ float sol[6];
    __shared__ float rowbuf[kLocRow];
    __shared__ float cur[12];  // the model one lane made, for every thread: the winner, then each step's
    __shared__ unsigned long long wkey[4];
    __shared__ uint32_t s_ok, s_count;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float4* const reca = a.reca + (size_t)row * a.cap;
    const float4* const recb = a.recb + (size_t)row * a.cap;
    unsigned long long best = 0ull;
    if (M >= kLocSample)
        for (uint32_t h = tid; h < a.hyps; h += 256u) best = max(best, a.keys[(size_t)row * kVerifyMaxHyp + h]);
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
            (void)loc_model(reca, recb, M, lowbias32(a.seed_mix ^ row), h, rowbuf, R, t);
#pragma unroll
            for (int e = 0; e < 9; e++) cur[e] = R[e];
#pragma unroll
            for (int e = 0; e < 3; e++) cur[9 + e] = t[e];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 9; e++) Rc[e] = Rm[e] = cur[e];
#pragma unroll
        for (int e = 0; e < 3; e++) tc[e] = tm[e] = cur[9 + e];
        bool fit = true;
        for (uint32_t step = 0; step < kLocSteps && fit; step++) {  // LO-6; `fit` is uniform
            float acc[kLocSums];
#pragma unroll
            for (uint32_t e = 0; e < kLocSums; e++) acc[e] = 0.0f;
            for (uint32_t j = tid; j < M; j += 256u) {  // candidate j into partial sum j mod 256, ascending j; the inlier set is the winner's
                const float4 Y = reca[j], k = recb[j];
                if (loc_inlier(Rm, tm, Y.x, Y.y, Y.z, k.x, k.y, a)) (void)loc_accumulate(acc, Rc, tc, Y, k.x, k.y, a);
            }
#pragma unroll
            for (uint32_t e = 0; e < kLocSums; e++) part[e][tid] = acc[e];
            __syncthreads();
            for (uint32_t s = 128u; s >= 1u; s >>= 1) {  // pairwise tree, strides 128 .. 1
                if (tid < s)
                    for (uint32_t e = 0; e < kLocSums; e++) part[e][tid] = part[e][tid] + part[e][tid + s];
                __syncthreads();
            }
            if (tid == 0u) {
                uint32_t ok = verify_solve_n<6>(part, aug, sol);
                if (ok) {
                    float R[9], t[3];
#pragma unroll
                    for (int e = 0; e < 9; e++) R[e] = Rc[e];
#pragma unroll
                    for (int e = 0; e < 3; e++) t[e] = tc[e];
                    ok = loc_update(sol, R, t) ? 1u : 0u;
#pragma unroll
                    for (int e = 0; e < 9; e++) cur[e] = R[e];
#pragma unroll
                    for (int e = 0; e < 3; e++) cur[9 + e] = t[e];
                }
                s_ok = ok;
            }
            __syncthreads();
            fit = s_ok != 0u;
            if (fit) {
#pragma unroll
                for (int e = 0; e < 9; e++) Rc[e] = cur[e];
#pragma unroll
                for (int e = 0; e < 3; e++) tc[e] = cur[9 + e];
            }
            __syncthreads();  // s_ok and cur are read before the next step's lane writes them
        }
        if (fit) {
            uint32_t n = 0;
            for (uint32_t j = tid; j < M; j += 256u) {
                const float4 Y = reca[j], k = recb[j];
                n += loc_inlier(Rc, tc, Y.x, Y.y, Y.z, k.x, k.y, a) ? 1u : 0u;
            }
            atomicAdd(&s_count, n);
        }
        __syncthreads();
        keep = fit && 16u * s_count >= 15u * n_min;  // GV-6's rule: the refit may lose a few marginal inliers, not 1/16 of them
    }
    LocFit f;
    f.has_min = has_min;
    f.keep = keep;
    f.h = h;
    f.n_min = n_min;
    f.inliers = keep ? s_count : n_min;
#pragma unroll
    for (int e = 0; e < 9; e++) f.R[e] = keep ? Rc[e] : Rm[e];
#pragma unroll
    for (int e = 0; e < 3; e++) f.t[e] = keep ? tc[e] : tm[e];
    return f;
}

// An inlier byte per slot of row `row` under the kept model: one write each below the capacity, 0 at a slot that is no candidate
// and at every slot from n on (n: the slots cand_of was written for)
__device__ __forceinline__ void loc_slot_bytes(const LocArgs& a, uint32_t row, uint32_t n, const LocFit& f) {
    const float4* const reca = a.reca + (size_t)row * a.cap;
    const float4* const recb = a.recb + (size_t)row * a.cap;
    const uint32_t* const cand_of = a.cand_of + (size_t)row * a.cap;
    uint8_t* const mask = a.mask + (size_t)row * a.cap;
    for (uint32_t i = threadIdx.x; i < a.cap; i += 256u) {
        uint8_t b = 0;
        if (i < n) {
            const uint32_t j = cand_of[i];
            if (j != kVerifyNone) {
                const float4 Y = reca[j], k = recb[j];
                b = loc_inlier(f.R, f.t, Y.x, Y.y, Y.z, k.x, k.y, a) ? 1 : 0;
            }
        }
        mask[i] = b;
    }
}

// grid (pairs), block 256
__global__ __launch_bounds__(256) void k_loc_refine(LocArgs a) {
    const uint32_t pair = blockIdx.x;
    const bool nomap = loc_nomap(a, pair);
    const uint32_t M = nomap ? 0u : a.n_cand[pair];
    const LocFit f = loc_fit(a, pair, M);
    // LO-7: an inlier byte per slot of frame f - 1
    loc_slot_bytes(a, pair, f.has_min ? min(a.counts[pair - 1u], a.cap) : 0u, f);  // has_min: the pair is not the first
    if (threadIdx.x == 0u) {  // the record
        uint32_t* const out = a.fix + (size_t)pair * kLocFixWords;
        loc_put_pose(out, f);
        out[13] = f.has_min ? M : 0u;
        out[14] = f.inliers;
        out[15] = f.h;
        out[16] = loc_status(nomap, M, f.has_min, f.keep);
        out[17] = out[18] = out[19] = 0u;
    }
}

}  // namespace orb
