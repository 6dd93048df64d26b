// orb_kernels_guide.h -- guided matching of consecutive frames ("search by projection"; not in the reference, the definition is
// the build's own, GM-1..GM-6 in DESIGN.md section 14): every keypoint of frame f is sent into frame f + 1 by a 3 x 3 model and
// matched against the keypoints of f + 1 inside a square window around the prediction only.  The result is the OrbMatch record of
// the brute-force matcher restricted to the window; the binary32 operations are the definition's, in its order (the build compiles
// with -ffp-contract=off and correctly rounded division), so the CPU restatement (tests/guided_ref.py) gives the same records.
//
//   k_guide_bin      one workgroup per frame of the batch: an LDS histogram of the stored keypoints over a row-major grid of
//                    C x C level-0 pixel cells, its exclusive prefix (the cell starts), and a scatter of every record -- level-0
//                    coordinates, index, octave and descriptor -- into cell order ("bucket first"): one row of cells of a window
//                    is one contiguous range of records
//   k_guide_search   one thread per query, the queries of frame f visited in ITS cell order (the lanes of a wave look at
//                    neighbouring windows); the cell rows of the window in frame f + 1 are walked as ranges, the exact GM-3 test
//                    decides membership, and the two smallest keys distance << 23 | index are kept (GM-4); written at the
//                    query's original index
// The grid is an acceleration structure only (GM-5): the window test is on the coordinates, and the cell range derived from the
// prediction is widened by a margin that covers the rounding of the test, so no cell size changes a record.
#pragma once
#include "../../include/tinyorb.h"
#include "orb_kernels_staged.h"

namespace orb {

constexpr uint32_t kGuideMaxCells = 8192u;   // cells per frame (the LDS histogram: 32 KB)
constexpr uint32_t kGuideBinThreads = 1024u; // k_guide_bin workgroup
constexpr uint32_t kGuideCellsPerThread = kGuideMaxCells / kGuideBinThreads;
constexpr uint32_t kGuideSearchThreads = 256u;
constexpr uint32_t kGuideNone = 0xffffffffu;
constexpr uint32_t kGuideBatch = 4u;         // records of a window row whose loads k_guide_search issues together

struct GuideArgs {
    const uint32_t* counts;          // [frames] raw counters of the batch
    const CornerData* corners;       // [frames][cap]
    const CornerDescriptor* desc;    // [frames][cap]
    uint32_t cap;
    uint32_t gw, gh, shift;          // grid: cells per row and per column, log2 of the cell size C
    uint4* srec;                     // [frames][cap] in cell order: (x0 bits, y0 bits, stored index, octave)
    uint4* sdesc;                    // [frames][cap][2] descriptors in the same order
    uint32_t* cell_start;            // [frames][kGuideMaxCells + 1] first record of every cell, then the frame's count
    uint32_t pairs;
    uint32_t source;                 // ORB_GUIDE_*
    const uint32_t* vmodel;          // [pairs][16] OrbPairModel of the last verification (ORB_GUIDE_VERIFIED)
    const float* hmodel;             // [pairs][9] the caller's models (ORB_GUIDE_HOST)
    float radius;                    // level-0 pixels
    uint32_t octave_window;          // 0: any octave
    uint32_t scale_radius;           // radius * 2^octave of the query
    MatchRecord* out;                // [pairs][cap]
};

// orb_corner_level0_xy
__device__ __forceinline__ float guide_level0(uint32_t v, uint32_t octave) {
    const float s = (float)(1u << (octave & 31u));
    return ((float)v + 0.5f) * s - 0.5f;
}

// cell column (row) of a level-0 coordinate: floor(v / C), clamped to the grid (a stored keypoint lies inside the frame, v >= 0)
__device__ __forceinline__ uint32_t guide_cell_of(float v, uint32_t shift, uint32_t n) {
    const uint32_t vi = (uint32_t)fminf(fmaxf(v, 0.0f), 1073741824.0f);
    return min(vi >> shift, n - 1u);
}

// grid (frames), block 1024
__global__ __launch_bounds__(kGuideBinThreads) void k_guide_bin(GuideArgs a) {
    __shared__ uint32_t cnt[kGuideMaxCells];
    __shared__ uint32_t wave_sum[kGuideBinThreads / 64u];
    const uint32_t f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = min(a.counts[f], a.cap), ncell = a.gw * a.gh;
    const uint4* const cf = reinterpret_cast<const uint4*>(a.corners + (size_t)f * a.cap);  // (x, y, angle, octave)
    for (uint32_t c = tid; c < ncell; c += kGuideBinThreads) cnt[c] = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kGuideBinThreads) {
        const uint4 q = cf[i];
        atomicAdd(&cnt[guide_cell_of(guide_level0(q.y, q.w), a.shift, a.gh) * a.gw + guide_cell_of(guide_level0(q.x, q.w), a.shift, a.gw)], 1u);
    }
    __syncthreads();
    // exclusive prefix over the cells: thread t owns cells 8t .. 8t + 7; a wave scan of the thread sums, then the wave sums
    uint32_t v[kGuideCellsPerThread], s = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kGuideCellsPerThread; k++) {
        const uint32_t c = tid * kGuideCellsPerThread + k;
        v[k] = c < ncell ? cnt[c] : 0u;
        s += v[k];
    }
    uint32_t incl = s;
#pragma unroll
    for (uint32_t d = 1u; d < 64u; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t excl = incl - s;
    for (uint32_t w = 0; w < wave; w++) excl += wave_sum[w];
    uint32_t* const cs = a.cell_start + (size_t)f * (kGuideMaxCells + 1u);
#pragma unroll
    for (uint32_t k = 0; k < kGuideCellsPerThread; k++) {
        const uint32_t c = tid * kGuideCellsPerThread + k;
        if (c < ncell) {
            cnt[c] = excl;  // every thread reads only its own cells above: no barrier needed before the overwrite
            cs[c] = excl;
        }
        excl += v[k];
    }
    if (tid == 0u) cs[ncell] = n;
    __syncthreads();
    // scatter in cell order; the order inside a cell follows the LDS atomics and changes nothing (the keys are unique per record)
    uint4* const sr = a.srec + (size_t)f * a.cap;
    uint4* const sd = a.sdesc + (size_t)f * a.cap * 2u;
    const uint4* const df = reinterpret_cast<const uint4*>(a.desc + (size_t)f * a.cap);
    for (uint32_t i = tid; i < n; i += kGuideBinThreads) {
        const uint4 q = cf[i], d0 = df[2u * i], d1 = df[2u * i + 1u];
        const float x0 = guide_level0(q.x, q.w), y0 = guide_level0(q.y, q.w);
        const uint32_t pos = atomicAdd(&cnt[guide_cell_of(y0, a.shift, a.gh) * a.gw + guide_cell_of(x0, a.shift, a.gw)], 1u);
        sr[pos] = make_uint4(__float_as_uint(x0), __float_as_uint(y0), i, q.w);
        sd[2u * pos] = d0;
        sd[2u * pos + 1u] = d1;
    }
}

// inclusive cell range [lo, hi] of the window [p - r, p + r] on one axis.  A target in the window has |fl(v - p)| <= r, hence
// |v - p| <= r (1 + 2^-23); the bounds are widened by 1 + (|p| + r) 2^-20 pixels, which covers that and the rounding of the bounds
// themselves, then clamped to the grid in float before the conversion to int
__device__ __forceinline__ void guide_range(float p, float r, uint32_t shift, uint32_t n, uint32_t& lo, uint32_t& hi) {
    const float m = 1.0f + (fabsf(p) + r) * 9.5367431640625e-07f;
    const float ic = 1.0f / (float)(1u << shift);
    const float top = (float)(n - 1u);
    lo = (uint32_t)fminf(fmaxf(floorf(((p - r) - m) * ic), 0.0f), top);
    hi = (uint32_t)fminf(fmaxf(floorf(((p + r) + m) * ic), 0.0f), top);
}

// grid (pairs * ceil(cap / 256)), block 256.  Workgroup b is relabelled so that the workgroups of one pair share a group b % 8
// (the dispatcher's round robin over the eight XCDs puts such a group on one XCD: frame f + 1's records stay in one L2); the
// relabelling is a bijection, and only speed depends on the placement.
__global__ __launch_bounds__(kGuideSearchThreads) void k_guide_search(GuideArgs a) {
    const uint32_t nch = (a.cap + kGuideSearchThreads - 1u) / kGuideSearchThreads, nwg = a.pairs * nch;
    const uint32_t b = blockIdx.x, g = b & 7u, qn = nwg >> 3, rn = nwg & 7u;
    const uint32_t wg = (g < rn ? g * (qn + 1u) : rn * (qn + 1u) + (g - rn) * qn) + (b >> 3);
    const uint32_t pair = wg / nch, t = (wg - pair * nch) * kGuideSearchThreads + threadIdx.x;
    if (t >= a.cap) return;
    const uint32_t nq = min(a.counts[pair], a.cap);
    MatchRecord* const out = a.out + (size_t)pair * a.cap;
    if (t >= nq) {  // GM-4: the slots past the frame's stored keypoints
        out[t] = MatchRecord{kGuideNone, 0xffffffffu};
        return;
    }
    const uint4 q = a.srec[(size_t)pair * a.cap + t];
    const float x = __uint_as_float(q.x), y = __uint_as_float(q.y);
    // GM-1
    float m[9];
    bool has = true;
    if (a.source == ORB_GUIDE_IDENTITY) {
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = (e % 4 == 0) ? 1.0f : 0.0f;
    } else if (a.source == ORB_GUIDE_HOST) {
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = a.hmodel[(size_t)pair * 9u + e];
    } else {
        const uint32_t* const v = a.vmodel + (size_t)pair * 16u;
        const uint32_t st = v[12];
        has = st == ORB_VERIFY_OK || st == ORB_VERIFY_MINIMAL;
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = __uint_as_float(v[e]);
    }
    uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;
    if (has) {
        // GM-2
        const float w = (m[6] * x + m[7] * y) + m[8];
        const float px = ((m[0] * x + m[1] * y) + m[2]) / w;
        const float py = ((m[3] * x + m[4] * y) + m[5]) / w;
        if (w > 0.0f && isfinite(px) && isfinite(py)) {
            // GM-3
            const uint32_t oi = q.w;
            const float r = a.scale_radius ? a.radius * (float)(1u << (oi & 31u)) : a.radius;
            uint32_t cx0, cx1, cy0, cy1;
            guide_range(px, r, a.shift, a.gw, cx0, cx1);
            guide_range(py, r, a.shift, a.gh, cy0, cy1);
            const uint4* const qd = a.sdesc + (size_t)pair * a.cap * 2u;
            const uint4 a0 = qd[2u * t], a1 = qd[2u * t + 1u];
            const uint4* const tr = a.srec + (size_t)(pair + 1u) * a.cap;
            const uint4* const td = a.sdesc + (size_t)(pair + 1u) * a.cap * 2u;
            const uint32_t* const cs = a.cell_start + (size_t)(pair + 1u) * (kGuideMaxCells + 1u);
            // the walk is bound by load latency, not by issue: the next row's bounds are loaded while this row is scanned, and
            // kGuideBatch records of a row, descriptors included, are loaded together before any of them is tested (the loads
            // past the row's end repeat its last record and are not counted)
            uint32_t e0 = cs[cy0 * a.gw + cx0], e1 = cs[cy0 * a.gw + cx1 + 1u];
            for (uint32_t cy = cy0; cy <= cy1; cy++) {
                uint32_t n0 = 0u, n1 = 0u;
                if (cy < cy1) {
                    n0 = cs[(cy + 1u) * a.gw + cx0];
                    n1 = cs[(cy + 1u) * a.gw + cx1 + 1u];
                }
                for (uint32_t k = e0; k < e1; k += kGuideBatch) {
                    uint4 c[kGuideBatch], b0[kGuideBatch], b1[kGuideBatch];
#pragma unroll
                    for (uint32_t u = 0; u < kGuideBatch; u++) {
                        const uint32_t ku = min(k + u, e1 - 1u);
                        c[u] = tr[ku];
                        b0[u] = td[2u * ku];
                        b1[u] = td[2u * ku + 1u];
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kGuideBatch; u++) {
                        const int od = (int)c[u].w - (int)oi;
                        const bool in = k + u < e1 && fabsf(__uint_as_float(c[u].x) - px) <= r && fabsf(__uint_as_float(c[u].y) - py) <= r &&
                                        (a.octave_window == 0u || (uint32_t)(od < 0 ? -od : od) < a.octave_window);
                        uint32_t d = __builtin_popcount(a0.x ^ b0[u].x);
                        d += __builtin_popcount(a0.y ^ b0[u].y);
                        d += __builtin_popcount(a0.z ^ b0[u].z);
                        d += __builtin_popcount(a0.w ^ b0[u].w);
                        d += __builtin_popcount(a1.x ^ b1[u].x);
                        d += __builtin_popcount(a1.y ^ b1[u].y);
                        d += __builtin_popcount(a1.z ^ b1[u].z);
                        d += __builtin_popcount(a1.w ^ b1[u].w);
                        const uint32_t key = in ? (d << 23) | c[u].z : 0xffffffffu;  // GM-4: distance first, then the smaller index
                        k2 = min(k2, max(k1, key));
                        k1 = min(k1, key);
                    }
                }
                e0 = n0;
                e1 = n1;
            }
        }
    }
    MatchRecord rec;
    rec.index = k1 == 0xffffffffu ? kGuideNone : (k1 & 0x7fffffu);
    rec.dist = (k1 == 0xffffffffu ? 0xffffu : (k1 >> 23)) | ((k2 == 0xffffffffu ? 0xffffu : (k2 >> 23)) << 16);
    out[q.z] = rec;
}

}  // namespace orb
