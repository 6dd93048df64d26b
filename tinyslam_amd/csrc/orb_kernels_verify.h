// orb_kernels_verify.h -- geometric verification of the Hamming matches between consecutive frames (not in the reference; the
// definition is the build's own, GV-1..GV-7 in DESIGN.md section 13): a RANSAC fit of a homography per pair, a least-squares
// refit over the winner's inliers, an inlier byte per query.  Every binary32 operation below is written out in the order the
// definition gives (the build compiles with -ffp-contract=off and correctly rounded division), so the CPU restatement
// (tests/verify_ref.py) reproduces every bit.
//
//   k_verify_gather   one workgroup per pair: the candidates (GV-1) compacted in query order by a wave ballot and a workgroup
//                     prefix, as normalised coordinates (GV-2) (u, v, u2, v2) in one 16-byte record, plus the candidate of
//                     every query (or kVerifyNone)
//   k_verify_score    grid (pair, 64-hypothesis block), 256 threads: lane l of every wave builds hypothesis 64 * block + l in
//                     registers (GV-3, GV-4), the candidates pass through LDS in tiles of 256 and are read as broadcasts, the
//                     four waves take every fourth one; one packed key per hypothesis (GV-5)
//   k_verify_refine   one workgroup per pair: the best key, the winner rebuilt, the normal equations summed in the order of
//                     GV-6 (thread t owns partial sum t), solved on one lane, the refit scored, the record (GV-7) and the
//                     inlier bytes written
//
// The score kernel behind its prologue and the whole refine kernel are a skeleton shared with the epipolar verifier
// (orb_kernels_epipolar.h): verify_score_tail, verify_solve and verify_refine_body below, templates over a model type --
// HomographyModel here, EpipolarModel there -- that supplies the minimal sample size, the winner's rebuild, the inlier test, an
// inlier's share of the 44 sums, the solution as nine entries and the model in pixels.  A change to the solver or to the keep
// rule is made once.
#pragma once
#include "../../include/tinyorb.h"
#include "orb_kernels_staged.h"

namespace orb {

constexpr uint32_t kVerifyMaxHyp = 4096u;   // hypotheses per pair (the key keeps 12 bits of index)
constexpr uint32_t kVerifyHypPerWg = 64u;   // hypotheses of one k_verify_score workgroup (one per lane)
constexpr uint32_t kVerifyNone = 0xffffffffu;
constexpr uint32_t kVerifySums = 44u;       // GV-6: 36 entries of the upper triangle of the 8 x 8 normal matrix + 8 of the right side
constexpr uint32_t kVerifyModelWords = 16u; // OrbPairModel

struct VerifyArgs {
    const uint32_t* counts;     // [frames] raw counters of the batch
    const CornerData* corners;  // [frames][cap]
    const MatchRecord* matches; // [frames][cap]
    uint32_t cap;
    uint32_t hyps;              // 1..kVerifyMaxHyp
    uint32_t max_distance;
    float ratio;
    float cx, cy, k, t2;        // GV-2: centre, scale, squared threshold in normalised units
    uint32_t seed_mix;          // lowbias32(seed)
    float4* rec;                // [pairs][cap] candidates (u, v, u2, v2)
    uint32_t* cand_of;          // [pairs][cap] candidate of query i (kVerifyNone: not a candidate); i < n_q only
    uint32_t* n_cand;           // [pairs]
    unsigned long long* keys;   // [pairs][kVerifyMaxHyp]
    uint32_t* model;            // [pairs][kVerifyModelWords] OrbPairModel
    uint8_t* mask;              // [pairs][cap]
};

__host__ __device__ inline uint32_t lowbias32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// GV-3: four distinct candidate indices of hypothesis h, or false after 16 draws (all 16 are evaluated; the ones after the
// fourth index change nothing)
__device__ inline bool verify_sample(uint32_t pair_mix, uint32_t h, uint32_t M, uint4& js) {
    uint32_t n = 0, j0 = 0, j1 = 0, j2 = 0, j3 = 0;
#pragma unroll
    for (uint32_t d = 0; d < 16u; d++) {
        const uint32_t j = (uint32_t)(((unsigned long long)lowbias32(pair_mix ^ ((h << 4) | d)) * M) >> 32);
        const bool take = n < 4u && !(n > 0u && j == j0) && !(n > 1u && j == j1) && !(n > 2u && j == j2);
        j0 = take && n == 0u ? j : j0;
        j1 = take && n == 1u ? j : j1;
        j2 = take && n == 2u ? j : j2;
        j3 = take && n == 3u ? j : j3;
        n += take ? 1u : 0u;
    }
    js = make_uint4(j0, j1, j2, j3);
    return n == 4u;
}

// GV-4: a triple (a, b, q) is degenerate when, in either frame, its cross product c = dx1 dy2 - dy1 dx2 (d1 = b - a, d2 = q - a) is
// not larger in magnitude than 2^-16 (|dx1| + |dy1|) (|dx2| + |dy2|) -- (nearly) collinear or coincident points; rounding of the
// normalised coordinates leaves exactly collinear pixels a few ulps off zero -- or when the two signs differ (a reflection)
constexpr float kVerifyCollinear = 1.0f / 65536.0f;
__device__ inline float verify_cross(float ax, float ay, float bx, float by, float qx, float qy, float& bound) {
    const float dx1 = bx - ax, dy1 = by - ay, dx2 = qx - ax, dy2 = qy - ay;
    bound = kVerifyCollinear * ((fabsf(dx1) + fabsf(dy1)) * (fabsf(dx2) + fabsf(dy2)));
    return dx1 * dy2 - dy1 * dx2;
}

__device__ inline bool verify_triple_ok(const float4& a, const float4& b, const float4& c) {
    float ms, md;
    const float s = verify_cross(a.x, a.y, b.x, b.y, c.x, c.y, ms);
    const float d = verify_cross(a.z, a.w, b.z, b.w, c.z, c.w, md);
    return fabsf(s) > ms && fabsf(d) > md && ((s > 0.0f) == (d > 0.0f));
}

// GV-4: Heckbert's square-to-quad matrix, multiplied through by its denominator (no division): (0,0), (1,0), (1,1), (0,1) -> p0..p3
__device__ inline bool verify_sq2quad(float x0, float y0, float x1, float y1, float x2, float y2, float x3, float y3, float S[9]) {
    const float sx = ((x0 - x1) + x2) - x3, sy = ((y0 - y1) + y2) - y3;
    const float dx1 = x1 - x2, dx2 = x3 - x2, dy1 = y1 - y2, dy2 = y3 - y2;
    const float den = dx1 * dy2 - dx2 * dy1;
    const float g = sx * dy2 - dx2 * sy, hh = dx1 * sy - sx * dy1;
    S[0] = (x1 - x0) * den + g * x1;
    S[1] = (x3 - x0) * den + hh * x3;
    S[2] = x0 * den;
    S[3] = (y1 - y0) * den + g * y1;
    S[4] = (y3 - y0) * den + hh * y3;
    S[5] = y0 * den;
    S[6] = g;
    S[7] = hh;
    S[8] = den;
    return den != 0.0f;
}

// R = A * B, 3 x 3 row-major, every entry (a0 b0 + a1 b1) + a2 b2
__device__ inline void verify_mat3(const float A[9], const float B[9], float R[9]) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}

// GV-3 + GV-4: the minimal model of hypothesis h in normalised coordinates, H = S_dst * adj(S_src); false: invalid / degenerate
__device__ inline bool verify_model(const float4* __restrict__ rec, uint32_t M, uint32_t pair_mix, uint32_t h, float H[9]) {
    uint4 js;
    if (!verify_sample(pair_mix, h, M, js)) return false;
    const float4 p0 = rec[js.x], p1 = rec[js.y], p2 = rec[js.z], p3 = rec[js.w];
    if (!(verify_triple_ok(p0, p1, p2) && verify_triple_ok(p0, p1, p3) && verify_triple_ok(p0, p2, p3) && verify_triple_ok(p1, p2, p3)))
        return false;
    float S[9], D[9];
    if (!verify_sq2quad(p0.x, p0.y, p1.x, p1.y, p2.x, p2.y, p3.x, p3.y, S)) return false;
    if (!verify_sq2quad(p0.z, p0.w, p1.z, p1.w, p2.z, p2.w, p3.z, p3.w, D)) return false;
    const float A[9] = {S[4] * S[8] - S[5] * S[7], S[2] * S[7] - S[1] * S[8], S[1] * S[5] - S[2] * S[4],
                        S[5] * S[6] - S[3] * S[8], S[0] * S[8] - S[2] * S[6], S[2] * S[3] - S[0] * S[5],
                        S[3] * S[7] - S[4] * S[6], S[1] * S[6] - S[0] * S[7], S[0] * S[4] - S[1] * S[3]};
    verify_mat3(D, A, H);
    return true;
}

// GV-5: one-way transfer error below t, without a division: |(x', y') - (u2, v2) w'|^2 < t^2 w'^2
__device__ inline bool verify_inlier(const float H[9], const float4& c, float t2) {
    const float xp = (H[0] * c.x + H[1] * c.y) + H[2];
    const float yp = (H[3] * c.x + H[4] * c.y) + H[5];
    const float wp = (H[6] * c.x + H[7] * c.y) + H[8];
    const float ex = xp - c.z * wp, ey = yp - c.w * wp;
    return ex * ex + ey * ey < t2 * (wp * wp);
}

// grid (pairs), block 256
__global__ __launch_bounds__(256) void k_verify_gather(VerifyArgs a) {
    const uint32_t pair = blockIdx.x;  // the pair (frame pair, frame pair + 1) at row pair
#define GATHER_FQ pair
#define GATHER_FT (pair + 1u)
#define GATHER_ROW pair
#include "orb_verify_gather_body.inc"
#undef GATHER_FQ
#undef GATHER_FT
#undef GATHER_ROW
}

// GV-6: the two rows of an inlier's equations (h33 = 1) added to the 44 sums
__device__ inline void verify_accumulate(float acc[kVerifySums], const float4& c) {
    const float r1[8] = {c.x, c.y, 1.0f, 0.0f, 0.0f, 0.0f, -(c.x * c.z), -(c.y * c.z)};
    const float r2[8] = {0.0f, 0.0f, 0.0f, c.x, c.y, 1.0f, -(c.x * c.w), -(c.y * c.w)};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = i; j < 8; j++, e++) acc[e] = acc[e] + (r1[i] * r1[j] + r2[i] * r2[j]);
#pragma unroll
    for (int i = 0; i < 8; i++) acc[36 + i] = acc[36 + i] + (r1[i] * c.z + r2[i] * c.w);
}

// What the skeleton below needs to know about the homography (the fundamental matrix's counterpart is EpipolarModel in
// orb_kernels_epipolar.h).  `m` is the entry a model fixes to 1 in its refit: always h33 here, so it is not used.
struct HomographyModel {
    static constexpr uint32_t kSample = 4u;  // candidates of a minimal sample; a pair with fewer is ORB_VERIFY_FEW
    // the winner rebuilt in registers, on every thread (valid: it scored a key)
    static __device__ __forceinline__ void winner(const float4* __restrict__ rec, uint32_t M, uint32_t pair_mix, uint32_t h, bool has_min,
                                                  float Hm[9], uint32_t&) {
        if (has_min) (void)verify_model(rec, M, pair_mix, h, Hm);
    }
    static __device__ __forceinline__ bool inlier(const float H[9], const float4& c, float t2) { return verify_inlier(H, c, t2); }
    static __device__ __forceinline__ void accumulate(float acc[kVerifySums], const float4& c, uint32_t) { verify_accumulate(acc, c); }
    // GV-6: the solution with h33 = 1 appended
    static __device__ __forceinline__ void from_solution(const float* sol, uint32_t, float H[9]) {
#pragma unroll
        for (int e = 0; e < 8; e++) H[e] = sol[e];
        H[8] = 1.0f;
    }
    // GV-7: the model in level-0 pixels, T^-1 * H * T divided by its [2][2] entry
    static __device__ __forceinline__ void to_pixels(const float Hk[9], const VerifyArgs& a, float P[9]) {
        const float T[9] = {a.k, 0.0f, -(a.cx * a.k), 0.0f, a.k, -(a.cy * a.k), 0.0f, 0.0f, 1.0f};
        const float ik = 1.0f / a.k;
        const float Ti[9] = {ik, 0.0f, a.cx, 0.0f, ik, a.cy, 0.0f, 0.0f, 1.0f};
        float G[9], Q[9];
        verify_mat3(Hk, T, G);
        verify_mat3(Ti, G, Q);
#pragma unroll
        for (int e = 0; e < 9; e++) P[e] = Q[e] / Q[8];
    }
};

// The skeleton both verifiers share: everything of their score and refine kernels that does not depend on the model.

// The score kernels behind their prologue (lane l of every wave holds model F of hypothesis h = 64 * block + l, all zeros when it
// is not `valid`): the candidates through LDS in tiles of 256, read as broadcasts, wave w takes every fourth one from w; the four
// waves' counts added as (0 + 1) + (2 + 3); the packed key (GV-5), written by wave 0
template <class Model>
__device__ __forceinline__ void verify_score_tail(const VerifyArgs& a, const float4* __restrict__ rec, uint32_t M, uint32_t h, const float F[9],
                                                  bool valid) {
    __shared__ float4 tile[256];
    __shared__ uint32_t cnt[4][kVerifyHypPerWg];
    const uint32_t pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t n = 0;
    for (uint32_t c0 = 0; c0 < M; c0 += 256u) {
        const uint32_t tn = min(M - c0, 256u);
        if (tid < tn) tile[tid] = rec[c0 + tid];
        __syncthreads();
#pragma unroll 4
        for (uint32_t q = wave; q < tn; q += 4u) n += Model::inlier(F, tile[q], a.t2) ? 1u : 0u;
        __syncthreads();
    }
    cnt[wave][lane] = n;
    __syncthreads();
    if (wave == 0u && h < a.hyps) {
        const uint32_t total = (cnt[0][lane] + cnt[1][lane]) + (cnt[2][lane] + cnt[3][lane]);
        a.keys[(size_t)pair * kVerifyMaxHyp + h] = valid ? (((unsigned long long)(total + 1u) << 12) | (kVerifyMaxHyp - 1u - h)) : 0ull;
    }
}

// GV-6's solver on one lane at size N x (N + 1): the N (N + 1) / 2 + N sums (column 0 of `part`) spread into the symmetric system
// `aug`, Gaussian elimination with partial pivoting (first maximal |pivot|), back substitution into sol[0..N-1].  0: a zero pivot or
// a non-finite entry.  The verifiers solve at N = 8 (verify_solve), the localisation's refit at N = 6.
template <int N>
__device__ __forceinline__ uint32_t verify_solve_n(const float (*part)[256], float (*aug)[N + 1], float* sol) {
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

__device__ __forceinline__ uint32_t verify_solve(const float (*part)[256], float (*aug)[9], float* sol) { return verify_solve_n<8>(part, aug, sol); }

// The refine kernels, one workgroup of 256 per pair: the best key and what it encodes, the winner rebuilt (Model::winner), the
// normal equations of its inliers summed in GV-6's order (thread t owns partial sum t, then the tree), solved on one lane, the
// refit scored and kept or not, the inlier bytes and the record (GV-7 / EP-6)
template <class Model>
__device__ __forceinline__ void verify_refine_body(const VerifyArgs& a) {
    __shared__ float part[kVerifySums][256];  // [sum][thread]: conflict-free columns
    __shared__ float aug[8][9];
    __shared__ float sol[8];
    __shared__ unsigned long long wkey[4];
    __shared__ uint32_t s_ok, s_count;
    const uint32_t pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t M = a.n_cand[pair];
    const float4* const rec = a.rec + (size_t)pair * a.cap;
    unsigned long long best = 0ull;
    if (M >= Model::kSample)
        for (uint32_t h = tid; h < a.hyps; h += 256u) best = max(best, a.keys[(size_t)pair * kVerifyMaxHyp + h]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) best = max(best, (unsigned long long)__shfl_xor(best, off));
    if (lane == 0u) wkey[wave] = best;
    if (tid == 0u) s_count = 0u;
    __syncthreads();
    best = max(max(wkey[0], wkey[1]), max(wkey[2], wkey[3]));
    const bool has_min = best != 0ull;  // uniform
    const uint32_t h = has_min ? (kVerifyMaxHyp - 1u) - (uint32_t)(best & (kVerifyMaxHyp - 1u)) : kVerifyNone;
    const uint32_t n_min = has_min ? (uint32_t)(best >> 12) - 1u : 0u;
    float Fm[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t m = 0;
    Model::winner(rec, M, lowbias32(a.seed_mix ^ pair), h, has_min, Fm, m);
    bool keep = false;
    float Fr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (has_min) {
        float acc[kVerifySums];
#pragma unroll
        for (uint32_t e = 0; e < kVerifySums; e++) acc[e] = 0.0f;
        for (uint32_t j = tid; j < M; j += 256u) {  // candidate j into partial sum j mod 256, ascending j
            const float4 c = rec[j];
            if (Model::inlier(Fm, c, a.t2)) Model::accumulate(acc, c, m);
        }
#pragma unroll
        for (uint32_t e = 0; e < kVerifySums; e++) part[e][tid] = acc[e];
        __syncthreads();
        for (uint32_t s = 128u; s >= 1u; s >>= 1) {  // pairwise tree, strides 128 .. 1
            if (tid < s)
                for (uint32_t e = 0; e < kVerifySums; e++) part[e][tid] = part[e][tid] + part[e][tid + s];
            __syncthreads();
        }
        if (tid == 0u) s_ok = verify_solve(part, aug, sol);
        __syncthreads();
        if (s_ok) {
            Model::from_solution(sol, m, Fr);
            uint32_t n = 0;
            for (uint32_t j = tid; j < M; j += 256u) n += Model::inlier(Fr, rec[j], a.t2) ? 1u : 0u;
            atomicAdd(&s_count, n);
        }
        __syncthreads();
        keep = s_ok && 16u * s_count >= 15u * n_min;  // GV-6: the refit may lose a few marginal inliers, not 1/16 of them
    }
    float Fk[9];
#pragma unroll
    for (int e = 0; e < 9; e++) Fk[e] = keep ? Fr[e] : Fm[e];
    // inlier bytes of every query slot of the pair: one write each
    const uint32_t nq = min(a.counts[pair], a.cap);
    const uint32_t* const cand_of = a.cand_of + (size_t)pair * a.cap;
    uint8_t* const mask = a.mask + (size_t)pair * a.cap;
    for (uint32_t i = tid; i < a.cap; i += 256u) {
        uint8_t b = 0;
        if (has_min && i < nq) {
            const uint32_t j = cand_of[i];
            if (j != kVerifyNone) b = Model::inlier(Fk, rec[j], a.t2) ? 1 : 0;
        }
        mask[i] = b;
    }
    if (tid == 0u) {  // the record, the model in level-0 pixels
        uint32_t* const out = a.model + (size_t)pair * kVerifyModelWords;
        float P[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (has_min) Model::to_pixels(Fk, a, P);
#pragma unroll
        for (int e = 0; e < 9; e++) out[e] = __float_as_uint(P[e]);
        out[9] = M;
        out[10] = has_min ? (keep ? s_count : n_min) : 0u;
        out[11] = h;
        out[12] = M < Model::kSample ? (uint32_t)ORB_VERIFY_FEW : !has_min ? (uint32_t)ORB_VERIFY_DEGENERATE : keep ? (uint32_t)ORB_VERIFY_OK : (uint32_t)ORB_VERIFY_MINIMAL;
        out[13] = out[14] = out[15] = 0u;
    }
}

// grid (pairs, ceil(hyps / 64)), block 256
__global__ __launch_bounds__(256) void k_verify_score(VerifyArgs a) {
    const uint32_t pair = blockIdx.x, lane = threadIdx.x & 63u;
    const uint32_t M = a.n_cand[pair];
    if (M < HomographyModel::kSample) return;  // uniform: k_verify_refine reads no key of such a pair
    const float4* const rec = a.rec + (size_t)pair * a.cap;
    const uint32_t h = blockIdx.y * kVerifyHypPerWg + lane;
    float H[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // an invalid hypothesis: w' = 0, never an inlier
    const bool valid = h < a.hyps && verify_model(rec, M, lowbias32(a.seed_mix ^ pair), h, H);
    if (!valid)
#pragma unroll
        for (int e = 0; e < 9; e++) H[e] = 0.f;
    verify_score_tail<HomographyModel>(a, rec, M, h, H, valid);
}

// grid (pairs), block 256
__global__ __launch_bounds__(256) void k_verify_refine(VerifyArgs a) { verify_refine_body<HomographyModel>(a); }

}  // namespace orb
