// orb_kernels_band.h -- epipolar-band guided matching of consecutive frames ("search for triangulation"; not in the reference, the
// definition is the build's own, EB-1..EB-6 in DESIGN.md section 18): every keypoint of frame f is sent to its epipolar line in
// frame f + 1 by the pair's fundamental matrix and matched against the keypoints of f + 1 within band_px of that line only (and,
// with radius_px > 0, inside a square window around the keypoint's own position).  The result is the OrbMatch record of the
// brute-force matcher restricted to that set; the binary32 operations are the definition's, in its order (the build compiles with
// -ffp-contract=off), so the CPU restatement (tests/band_ref.py) gives the same records.
//
//   k_guide_bin      (orb_kernels_guide.h, unchanged) bins the frames into this stage's own cell-ordered buffers
//   k_band_search    one thread per query, the queries of frame f visited in ITS cell order (the lanes of a wave hold neighbouring
//                    keypoints, whose lines under one F neighbour each other too); the cell rows the band can cross are walked, in
//                    each row the contiguous record range of the cell columns the band can touch there is scanned with the exact
//                    EB-3 test, and the two smallest keys distance << 23 | index are kept (EB-4 = GM-4); written at the query's
//                    original index
// The grid is an acceleration structure only (EB-5): membership is decided on the coordinates, and the row and column intervals are
// derived without a square root from |a0 x + a1 y + a2| <= D (|a0| + |a1|), D = d + a margin, widened by what the roundings of the
// test and of the interval itself can amount to (band_cols), so no cell size changes a record.
#pragma once
#include "orb_kernels_guide.h"

namespace orb {

constexpr float kBandMinNorm2 = 5.421010862427522e-20f;  // 2^-64: EB-2's floor on a0^2 + a1^2
constexpr float kBandSlope = 32.0f;  // an axis is solved for (x from y, or y from x) only when the line's slope on it is at most this

struct BandArgs {
    const uint32_t* counts;          // [frames] raw counters of the batch
    uint32_t cap;
    uint32_t gw, gh, shift;          // grid: cells per row and per column, log2 of the cell size C
    float fw, fh;                    // level-0 frame size
    const uint4* srec;               // [frames][cap] in cell order: (x0 bits, y0 bits, stored index, octave) (k_guide_bin)
    const uint4* sdesc;              // [frames][cap][2] descriptors in the same order
    const uint32_t* cell_start;      // [frames][kGuideMaxCells + 1]
    uint32_t pairs;
    uint32_t source;                 // ORB_BAND_*
    const uint32_t* vmodel;          // [pairs][16] OrbPairModel of the last epipolar verification (ORB_BAND_VERIFIED)
    const float* hmodel;             // [pairs][9] the caller's models (ORB_BAND_HOST)
    float band;                      // d, level-0 pixels
    float radius;                    // R, level-0 pixels; 0: no window
    uint32_t octave_window;          // 0: any octave
    uint32_t scale;                  // d and R times 2^octave of the query
    MatchRecord* out;                // [pairs][cap]
};

// One axis of the band solved for the other: points (u, v) of the band, |au u + av v + a2| <= D (|au| + |av|), with v in [v0, v1] have
//   u in [min(c + s v0, c + s v1) - w, max(..) + w],  c = -a2 / au,  s = -av / au,  w = D (1 + |s|) + m.
// It is used only when |av| <= kBandSlope |au| and c is finite; m = 1 + (|c| + kBandSlope (2 span + 2 D) + span) 2^-20 covers the
// roundings of c, s, the products and sums here (each relative 2^-24 of terms bounded by |c| + kBandSlope span) and what EB-3's own
// roundings let in beyond D.  An infinite w only widens.
struct BandAxis {
    float c, s, w;
    bool solved;
};
__device__ __forceinline__ BandAxis band_axis(float au, float av, float a2, float D, float span) {
    BandAxis ax;
    ax.c = -a2 / au;
    ax.s = -av / au;
    ax.solved = fabsf(au) * kBandSlope >= fabsf(av) && isfinite(ax.c);
    const float m = 1.0f + (fabsf(ax.c) + kBandSlope * (2.0f * span + 2.0f * D) + span) * 9.5367431640625e-07f;
    ax.w = D * (1.0f + fabsf(ax.s)) + m;
    return ax;
}
// inclusive cell range [lo, hi] of u for v in [v0, v1]; false: the band misses [0, span) there
__device__ __forceinline__ bool band_cells(const BandAxis& ax, float v0, float v1, float span, uint32_t shift, uint32_t n, uint32_t& lo, uint32_t& hi) {
    const float ua = ax.c + ax.s * v0, ub = ax.c + ax.s * v1;
    const float ul = fminf(ua, ub) - ax.w, uh = fmaxf(ua, ub) + ax.w;
    if (uh < 0.0f || ul > span) return false;
    const float ic = 1.0f / (float)(1u << shift), top = (float)(n - 1u);
    lo = (uint32_t)fminf(fmaxf(floorf(ul * ic), 0.0f), top);  // clamped in float before the conversion
    hi = (uint32_t)fminf(fmaxf(floorf(uh * ic), 0.0f), top);
    return true;
}

// grid (pairs * ceil(cap / 256)), block 256; workgroups relabelled as in k_guide_search (the workgroups of one pair share an XCD)
__global__ __launch_bounds__(kGuideSearchThreads) void k_band_search(BandArgs a) {
    const uint32_t nch = (a.cap + kGuideSearchThreads - 1u) / kGuideSearchThreads, nwg = a.pairs * nch;
    const uint32_t b = blockIdx.x, g = b & 7u, qn = nwg >> 3, rn = nwg & 7u;
    const uint32_t wg = (g < rn ? g * (qn + 1u) : rn * (qn + 1u) + (g - rn) * qn) + (b >> 3);
    const uint32_t pair = wg / nch, t = (wg - pair * nch) * kGuideSearchThreads + threadIdx.x;
    if (t >= a.cap) return;
    const uint32_t nq = min(a.counts[pair], a.cap);
    MatchRecord* const out = a.out + (size_t)pair * a.cap;
    if (t >= nq) {  // EB-4: the slots past the frame's stored keypoints
        out[t] = MatchRecord{kGuideNone, 0xffffffffu};
        return;
    }
    const uint4 q = a.srec[(size_t)pair * a.cap + t];
    const float x = __uint_as_float(q.x), y = __uint_as_float(q.y);
    // EB-1
    float m[9];
    bool has = true;
    if (a.source == ORB_BAND_HOST) {
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = a.hmodel[(size_t)pair * 9u + e];
    } else {
        const uint32_t* const v = a.vmodel + (size_t)pair * 16u;
        const uint32_t st = v[12];
        has = st == ORB_VERIFY_OK || st == ORB_VERIFY_MINIMAL;
#pragma unroll
        for (int e = 0; e < 9; e++) m[e] = __uint_as_float(v[e]);
    }
    // EB-2
    const uint32_t oi = q.w;
    const float sc = a.scale ? (float)(1u << (oi & 31u)) : 1.0f;
    const float d = a.band * sc, R = a.radius * sc;
    const float a0 = (m[0] * x + m[1] * y) + m[2];
    const float a1 = (m[3] * x + m[4] * y) + m[5];
    const float a2 = (m[6] * x + m[7] * y) + m[8];
    const float n2 = a0 * a0 + a1 * a1;
    const float tt = (d * d) * n2;
    has = has && isfinite(a0) && isfinite(a1) && isfinite(a2) && isfinite(tt) && n2 >= kBandMinNorm2;
    uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;
    if (has) {
        const bool win = R > 0.0f;
        // the band's half-width for the walk: d, what EB-3's roundings admit beyond it, and the slack of band_axis
        const float D = d + (1.0f + ((a.fw + a.fh) + d) * 9.5367431640625e-07f);
        const BandAxis colx = band_axis(a0, a1, a2, D, a.fh);  // x from y: the columns of a cell row
        const BandAxis rowy = band_axis(a1, a0, a2, D, a.fw);  // y from x: the rows the band crosses over the frame's width
        uint32_t cy0 = 0u, cy1 = a.gh - 1u, wx0 = 0u, wx1 = a.gw - 1u;
        bool any = true;
        if (rowy.solved) any = band_cells(rowy, 0.0f, a.fw, a.fh, a.shift, a.gh, cy0, cy1);
        if (win) {  // the window's rows and columns (GM-3's range around the query's own position)
            uint32_t wy0, wy1;
            guide_range(x, R, a.shift, a.gw, wx0, wx1);
            guide_range(y, R, a.shift, a.gh, wy0, wy1);
            cy0 = max(cy0, wy0);
            cy1 = min(cy1, wy1);
        }
        if (any && cy0 <= cy1) {
            const float cell = (float)(1u << a.shift);
            const uint4* const qd = a.sdesc + (size_t)pair * a.cap * 2u;
            const uint4 q0 = qd[2u * t], q1 = qd[2u * t + 1u];
            const uint4* const tr = a.srec + (size_t)(pair + 1u) * a.cap;
            const uint4* const td = a.sdesc + (size_t)(pair + 1u) * a.cap * 2u;
            const uint32_t* const cs = a.cell_start + (size_t)(pair + 1u) * (kGuideMaxCells + 1u);
            // the record range of cell row cy: the columns the band can touch for y in the row, clipped to the window's; empty: 0, 0
            const auto row_bounds = [&](uint32_t cy, uint32_t& r0, uint32_t& r1) {
                uint32_t lo = 0u, hi = a.gw - 1u;
                bool ok = true;
                if (colx.solved) {
                    const float y0 = (float)cy * cell;
                    ok = band_cells(colx, y0, y0 + cell, a.fw, a.shift, a.gw, lo, hi);
                }
                lo = max(lo, wx0);
                hi = min(hi, wx1);
                ok = ok && lo <= hi;
                r0 = ok ? cs[cy * a.gw + lo] : 0u;
                r1 = ok ? cs[cy * a.gw + hi + 1u] : 0u;
            };
            // as k_guide_search: the next row's bounds are loaded while this row is scanned, and kGuideBatch records of a row,
            // descriptors included, are loaded together before any of them is tested
            uint32_t e0, e1;
            row_bounds(cy0, e0, e1);
            for (uint32_t cy = cy0; cy <= cy1; cy++) {
                uint32_t n0 = 0u, n1 = 0u;
                if (cy < cy1) row_bounds(cy + 1u, n0, n1);
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
                        // EB-3
                        const float xj = __uint_as_float(c[u].x), yj = __uint_as_float(c[u].y);
                        const float r = (a0 * xj + a1 * yj) + a2;
                        const int od = (int)c[u].w - (int)oi;
                        const bool in = k + u < e1 && r * r <= tt && (!win || (fabsf(xj - x) <= R && fabsf(yj - y) <= R)) &&
                                        (a.octave_window == 0u || (uint32_t)(od < 0 ? -od : od) < a.octave_window);
                        uint32_t dist = __builtin_popcount(q0.x ^ b0[u].x);
                        dist += __builtin_popcount(q0.y ^ b0[u].y);
                        dist += __builtin_popcount(q0.z ^ b0[u].z);
                        dist += __builtin_popcount(q0.w ^ b0[u].w);
                        dist += __builtin_popcount(q1.x ^ b1[u].x);
                        dist += __builtin_popcount(q1.y ^ b1[u].y);
                        dist += __builtin_popcount(q1.z ^ b1[u].z);
                        dist += __builtin_popcount(q1.w ^ b1[u].w);
                        const uint32_t key = in ? (dist << 23) | c[u].z : 0xffffffffu;  // EB-4: distance first, then the smaller index
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
