// orb_kernels_epipolar.h -- epipolar verification of the Hamming matches between consecutive frames (not in the reference; the
// definition is the build's own, EP-1..EP-6 in DESIGN.md section 16): a RANSAC fit of a fundamental matrix per pair from minimal
// eight-point samples, a least-squares refit over the winner's inliers, an inlier byte per query.  The candidates and their
// normalised coordinates are the homography verifier's (GV-1, GV-2: k_verify_gather, run into this call's own buffers).  Every
// binary32 operation below is written out in the order the definition gives (-ffp-contract=off, correctly rounded division), so the
// CPU restatement (tests/epipolar_ref.py) reproduces every bit.  F is not projected to rank 2 (that needs an SVD).
//
// This header holds what is the fundamental matrix's own: the sampling, the minimal solver, the inlier test, an inlier's share of the
// refit's sums, and EpipolarModel, which hands them to the skeleton both verifiers share (orb_kernels_verify.h: verify_score_tail,
// verify_refine_body).
//
//   k_epi_score    grid (pair, 64-hypothesis block), 256 threads: wave 0 builds hypothesis 64 * block + l on lane l (EP-2, EP-3),
//                  eliminating with complete pivoting in a padded LDS row of its own (pivots found at run time would send a
//                  private array to scratch); the 64 models go through LDS to all four waves; then the shared tail: the candidates
//                  in tiles of 256 read as broadcasts, each wave every fourth one, one packed key per hypothesis (EP-4)
//   k_epi_refine   the shared refine body: the best key, the winner rebuilt on one lane (EpipolarModel::winner), the 44
//                  normal-equation sums in GV-6's order and tree, GV-6's solve on one lane, the refit scored, the record (EP-6)
//                  and the inlier bytes written
#pragma once
#include "orb_kernels_verify.h"

namespace orb {

constexpr uint32_t kEpiSeedSalt = 0x45504931u;  // EP-2: the draw stream's seed is lowbias32(seed ^ kEpiSeedSalt)
constexpr uint32_t kEpiDraws = 32u;             // EP-2: draws per hypothesis
constexpr uint32_t kEpiRow = 73u;               // words of one lane's 8 x 9 matrix in LDS: 72 + 1, an odd stride (no bank conflicts)
constexpr float kEpiPivotRatio = 1.0f / 1048576.0f;  // EP-3: degenerate when |last pivot| <= 2^-20 |first pivot|

// EP-2: eight distinct candidate indices of hypothesis h in draw order, or false after 32 draws (all 32 are evaluated; the ones after
// the eighth index change nothing)
__device__ __forceinline__ bool epi_sample(uint32_t pair_mix, uint32_t h, uint32_t M, uint32_t js[8]) {
    uint32_t n = 0;
#pragma unroll
    for (int s = 0; s < 8; s++) js[s] = 0u;
#pragma unroll
    for (uint32_t d = 0; d < kEpiDraws; d++) {
        const uint32_t j = (uint32_t)(((unsigned long long)lowbias32(pair_mix ^ ((h << 5) | d)) * M) >> 32);
        bool dup = false;
#pragma unroll
        for (uint32_t s = 0; s < 8u; s++) dup = dup || (s < n && js[s] == j);
        const bool take = n < 8u && !dup;
#pragma unroll
        for (uint32_t s = 0; s < 8u; s++) js[s] = take && n == s ? j : js[s];
        n += take ? 1u : 0u;
    }
    return n == 8u;
}

// EP-3: the row [u2 u, u2 v, u2, v2 u, v2 v, v2, u, v, 1] of a candidate
__device__ __forceinline__ void epi_row(const float4& c, float* a) {
    a[0] = c.z * c.x;
    a[1] = c.z * c.y;
    a[2] = c.z;
    a[3] = c.w * c.x;
    a[4] = c.w * c.y;
    a[5] = c.w;
    a[6] = c.x;
    a[7] = c.y;
    a[8] = 1.0f;
}

// EP-3 on one lane's 8 x 9 matrix `a` (row-major, LDS): complete pivoting -- the first maximal |a| of the remaining block in
// row-major order, its row and column swapped into place (every row's column), a column permutation kept as nibbles -- elimination,
// the unpivoted column set to 1, back substitution, the columns put back, the result divided by its first entry of largest
// magnitude (index mi).  False: degenerate (a zero pivot, a last pivot at most 2^-20 of the first, or a non-finite entry).
__device__ __forceinline__ bool epi_null(float* a, float F[9], uint32_t& mi) {
    unsigned long long perm = 0x876543210ull;  // nibble c: the original column now at c
    bool ok = true;
    float p0 = 0.0f;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        float pmax = -1.0f;
        int pi = r, pj = r;
#pragma unroll
        for (int i = r; i < 8; i++)
#pragma unroll
            for (int j = r; j < 9; j++) {
                const float v = fabsf(a[i * 9 + j]);
                const bool gt = v > pmax;
                pmax = gt ? v : pmax;
                pi = gt ? i : pi;
                pj = gt ? j : pj;
            }
        ok = ok && pmax != 0.0f;
        if (r == 0) p0 = pmax;
#pragma unroll
        for (int c = 0; c < 9; c++) {  // rows r <-> pi
            const float t = a[r * 9 + c];
            a[r * 9 + c] = a[pi * 9 + c];
            a[pi * 9 + c] = t;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {  // columns r <-> pj
            const float t = a[i * 9 + r];
            a[i * 9 + r] = a[i * 9 + pj];
            a[i * 9 + pj] = t;
        }
        const unsigned long long nr = (perm >> (4 * r)) & 15ull, nj = (perm >> (4 * pj)) & 15ull;
        perm = (perm & ~(15ull << (4 * r)) & ~(15ull << (4 * pj))) | (nj << (4 * r)) | (nr << (4 * pj));
#pragma unroll
        for (int q = r + 1; q < 8; q++) {
            const float f = a[q * 9 + r] / a[r * 9 + r];
#pragma unroll
            for (int c = r + 1; c < 9; c++) a[q * 9 + c] = a[q * 9 + c] - f * a[r * 9 + c];
        }
    }
    ok = ok && !(fabsf(a[7 * 9 + 7]) <= kEpiPivotRatio * p0);
    float x[9];
    x[8] = 1.0f;
#pragma unroll
    for (int r = 7; r >= 0; r--) {
        float s = 0.0f;
#pragma unroll
        for (int q = r + 1; q < 9; q++) s = s - a[r * 9 + q] * x[q];
        x[r] = s / a[r * 9 + r];
        ok = ok && isfinite(x[r]);
    }
    // the columns put back through the lane's own LDS row (its first nine words are no longer needed)
#pragma unroll
    for (int c = 0; c < 9; c++) a[(perm >> (4 * c)) & 15ull] = x[c];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = a[e];
    float best = fabsf(F[0]), fm = F[0];
    uint32_t m = 0;
#pragma unroll
    for (int e = 1; e < 9; e++) {
        const bool gt = fabsf(F[e]) > best;
        best = gt ? fabsf(F[e]) : best;
        fm = gt ? F[e] : fm;
        m = gt ? (uint32_t)e : m;
    }
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = F[e] / fm;
    mi = m;
    return ok;
}

// EP-2 + EP-3: the minimal model of hypothesis h, through the LDS row `a` of the calling lane; false: invalid / degenerate
__device__ __forceinline__ bool epi_model(const float4* __restrict__ rec, uint32_t M, uint32_t pair_mix, uint32_t h, float* a, float F[9],
                                          uint32_t& mi) {
    uint32_t js[8];
    if (!epi_sample(pair_mix, h, M, js)) return false;
#pragma unroll
    for (int s = 0; s < 8; s++) epi_row(rec[js[s]], a + 9 * s);
    return epi_null(a, F, mi);
}

// EP-4: Sampson's test without a division: a = F x1, d = F^T x2, r = x2^T F x1; r^2 < t2 ((a0^2 + a1^2) + (d0^2 + d1^2))
__device__ __forceinline__ bool epi_inlier(const float F[9], const float4& c, float t2) {
    const float a0 = (F[0] * c.x + F[1] * c.y) + F[2];
    const float a1 = (F[3] * c.x + F[4] * c.y) + F[5];
    const float a2 = (F[6] * c.x + F[7] * c.y) + F[8];
    const float d0 = (F[0] * c.z + F[3] * c.w) + F[6];
    const float d1 = (F[1] * c.z + F[4] * c.w) + F[7];
    const float r = (c.z * a0 + c.w * a1) + a2;
    return r * r < t2 * ((a0 * a0 + a1 * a1) + (d0 * d0 + d1 * d1));
}

// EP-5: an inlier's row without entry m (b, 8 entries) and c = -(row[m]), added to the 44 sums in GV-6's order
__device__ __forceinline__ void epi_accumulate(float acc[kVerifySums], const float4& c, uint32_t m) {
    float r[9];
    epi_row(c, r);
    float b[8];
    float cm = r[0];
#pragma unroll
    for (int e = 1; e < 9; e++) cm = (uint32_t)e == m ? r[e] : cm;
    cm = -cm;
#pragma unroll
    for (int i = 0; i < 8; i++) b[i] = (uint32_t)i < m ? r[i] : r[i + 1];
    int e = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++, e++) acc[e] = acc[e] + b[i] * b[j];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[36 + i] = acc[36 + i] + b[i] * cm;
}

// What the shared skeleton (orb_kernels_verify.h) needs to know about the fundamental matrix.  `m` is the entry of largest
// magnitude of the minimal model, which the refit fixes to 1 (EP-5).
struct EpipolarModel {
    static constexpr uint32_t kSample = 8u;  // candidates of a minimal sample; a pair with fewer is ORB_VERIFY_FEW
    // the winner rebuilt on one lane through an LDS row (valid: it scored a key), then handed to every thread
    static __device__ __forceinline__ void winner(const float4* __restrict__ rec, uint32_t M, uint32_t pair_mix, uint32_t h, bool has_min,
                                                  float Fm[9], uint32_t& m) {
        __shared__ float rowbuf[kEpiRow];
        __shared__ float fmin[9];
        __shared__ uint32_t s_m;
        if (has_min && threadIdx.x == 0u) {
            float F[9];
            uint32_t mi = 0;
            (void)epi_model(rec, M, pair_mix, h, rowbuf, F, mi);
#pragma unroll
            for (int e = 0; e < 9; e++) fmin[e] = F[e];
            s_m = mi;
        }
        __syncthreads();
        if (has_min) {
#pragma unroll
            for (int e = 0; e < 9; e++) Fm[e] = fmin[e];
            m = s_m;
        }
    }
    static __device__ __forceinline__ bool inlier(const float F[9], const float4& c, float t2) { return epi_inlier(F, c, t2); }
    static __device__ __forceinline__ void accumulate(float acc[kVerifySums], const float4& c, uint32_t m) { epi_accumulate(acc, c, m); }
    // EP-5: F[m] = 1, the other entries the solution in ascending order
    static __device__ __forceinline__ void from_solution(const float* sol, uint32_t m, float F[9]) {
#pragma unroll
        for (int e = 0; e < 9; e++) F[e] = (uint32_t)e == m ? 1.0f : sol[(uint32_t)e > m ? e - 1 : e];
    }
    // EP-6: the model in level-0 pixels, T^T * (F * T) divided by its first entry of largest magnitude
    static __device__ __forceinline__ void to_pixels(const float Fk[9], const VerifyArgs& a, float P[9]) {
        const float T[9] = {a.k, 0.0f, -(a.cx * a.k), 0.0f, a.k, -(a.cy * a.k), 0.0f, 0.0f, 1.0f};
        const float Tt[9] = {a.k, 0.0f, 0.0f, 0.0f, a.k, 0.0f, -(a.cx * a.k), -(a.cy * a.k), 1.0f};
        float G[9], Q[9];
        verify_mat3(Fk, T, G);
        verify_mat3(Tt, G, Q);
        float bestq = fabsf(Q[0]), qm = Q[0];
#pragma unroll
        for (int e = 1; e < 9; e++) {
            const bool gt = fabsf(Q[e]) > bestq;
            bestq = gt ? fabsf(Q[e]) : bestq;
            qm = gt ? Q[e] : qm;
        }
#pragma unroll
        for (int e = 0; e < 9; e++) P[e] = Q[e] / qm;
    }
};

// grid (pairs, ceil(hyps / 64)), block 256; VerifyArgs.seed_mix = lowbias32(seed ^ kEpiSeedSalt)
__global__ __launch_bounds__(256) void k_epi_score(VerifyArgs a) {
    __shared__ float mat[kVerifyHypPerWg * kEpiRow];
    __shared__ float models[9][kVerifyHypPerWg];
    __shared__ uint32_t valid_mask[2];
    const uint32_t pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t M = a.n_cand[pair];
    if (M < EpipolarModel::kSample) return;  // uniform: k_epi_refine reads no key of such a pair
    const float4* const rec = a.rec + (size_t)pair * a.cap;
    const uint32_t h = blockIdx.y * kVerifyHypPerWg + lane;
    if (wave == 0u) {
        float F[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        uint32_t mi = 0;
        bool valid = h < a.hyps && epi_model(rec, M, lowbias32(a.seed_mix ^ pair), h, mat + lane * kEpiRow, F, mi);
#pragma unroll
        for (int e = 0; e < 9; e++) models[e][lane] = valid ? F[e] : 0.0f;  // an invalid hypothesis: F = 0, never an inlier
        const unsigned long long vb = __ballot(valid);
        if (lane == 0u) {
            valid_mask[0] = (uint32_t)vb;
            valid_mask[1] = (uint32_t)(vb >> 32);
        }
    }
    __syncthreads();
    float F[9];
#pragma unroll
    for (int e = 0; e < 9; e++) F[e] = models[e][lane];
    verify_score_tail<EpipolarModel>(a, rec, M, h, F, (valid_mask[lane >> 5] >> (lane & 31u)) & 1u);
}

// grid (pairs), block 256
__global__ __launch_bounds__(256) void k_epi_refine(VerifyArgs a) { verify_refine_body<EpipolarModel>(a); }

}  // namespace orb
