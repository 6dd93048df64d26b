// orb_kernels_graph.h -- pose-graph correction from the loop fixes (not in the reference; the definition is the build's own,
// PG-1..PG-8 in DESIGN.md section 29).  The trajectory chains pair poses, so its error grows along a segment; an OrbLoopFix of
// orb_loop_pairs measures camera q relative to camera T without passing through that chain.  Here every segment of the last
// orb_trajectory_consecutive is a graph: its cameras are the nodes, the relative poses of consecutive cameras the chain edges, the
// qualifying fixes the loop edges; Gauss-Newton rounds, each solved by preconditioned conjugate gradients, move every camera but
// the segment's origin.  Every binary32 operation below is written out in the order the definition gives (-ffp-contract=off,
// correctly rounded division), so the CPU restatement (tests/graph_ref.py) reproduces every bit.
//
//   k_pg_edges   a thread per list entry: the verdict of PG-4 and the zeroed OrbGraphEdge
//   k_pg_index   one workgroup: a thread per frame walks the USED entries in ascending list index (staged through LDS in tiles)
//                and writes the frame's incident ones as a CSR row -- count, scan, fill; the order within a row is the list's
//   k_pg_write   a thread per frame: the record of a frame whose segment is not solved (HELD, UNCHANGED, INVALID)
//   k_pg_solve   one workgroup of 256 per frame; a block whose frame is not an origin with at least one USED edge leaves at once.
//                Threads stride over the segment's free nodes.  A node's state is kPgNodeWords words -- the pose (12), the
//                gradient (6), the inverse of its diagonal block (36), the CG vectors x, r, p and H p / z (24) --, kept in LDS
//                while the segment has at most kPgLdsNodes free nodes: 512 * 78 * 4 = 159,744 bytes, with the 2 KiB of the
//                reductions' partials and two flags 161,800 of the CU's 163,840.  A longer segment keeps the same words in a workspace of the
//                stage in global memory; the arithmetic does not know which.  The whole solve is one launch ordered by
//                __syncthreads: three per CG iteration.
// Kernels are ordered by launch boundaries only.
#pragma once
#include "orb_kernels_localize.h"
#include "orb_kernels_traj.h"

namespace orb {

constexpr uint32_t kPgThreads = 256u;
constexpr uint32_t kPgFrameWords = 20u;   // OrbFramePose
constexpr uint32_t kPgFixWords = 32u;     // OrbLoopFix
constexpr uint32_t kPgPoseWords = 16u;    // OrbGraphPose: r[9], t[3], cost_before, cost_after, loops, status
constexpr uint32_t kPgEdgeWords = 4u;     // OrbGraphEdge: verdict, cost_before, cost_after, origin
constexpr uint32_t kPgNone = 0xffffffffu;
constexpr uint32_t kPgTile = 2048u;       // list entries k_pg_index stages at a time
constexpr uint32_t kPgPose = 0u, kPgGrad = 12u, kPgDinv = 18u, kPgX = 54u, kPgR = 60u, kPgP = 66u, kPgHp = 72u;  // words of a node
constexpr uint32_t kPgNodeWords = 78u;
constexpr uint32_t kPgLdsNodes = 512u;    // free nodes of a segment that is solved in LDS
constexpr uint32_t kPgLdsBytes = kPgNodeWords * kPgLdsNodes * 4u;
constexpr uint32_t kPgMaxCg = 512u;       // PG-6: cg_iterations 0 is the segment's free nodes, clipped to this
// the 27 x 256 sums verify_solve_n reads lie over the CG vectors, which are dead while the blocks are inverted
static_assert(kLocSums * 256u <= (kPgNodeWords - kPgX) * kPgLdsNodes, "the solver's sums fit the CG vectors");
static_assert(kPgLdsBytes + 2u * 256u * 4u + 64u <= 163840u, "LDS of a CU");

struct PgArgs {
    const uint32_t* frames;  // [F][kPgFrameWords] of the last orb_trajectory_consecutive
    const uint2* list;       // [entries] OrbFramePair of the last orb_match_pairs: (query, target)
    const uint32_t* fixes;   // [entries][kPgFixWords] of the last orb_loop_pairs
    uint32_t n_frames;       // F
    uint32_t n_pairs;
    uint32_t min_inliers, use_minimal, rounds, cg_iterations;
    float loop_weight, rotation_weight;
    uint32_t* edges;         // [entries][kPgEdgeWords]
    uint32_t* row;           // [F + 1] CSR row starts
    uint32_t* col;           // [2 * entries] list indices
    uint32_t* out;           // [F][kPgPoseWords]
    float* work;             // [max_batch][kPgNodeWords] the node words of the segments above kPgLdsNodes
};

__device__ __forceinline__ bool pg_bits_finite(uint32_t w) { return (w & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool pg_member(const uint32_t* rec, uint32_t o) {
    return rec[14] == o && rec[17] != ORB_TRAJ_LOST && rec[17] != ORB_TRAJ_ORIGIN;
}

// PG-2: the origin of the segment in which frame g is a free node, kPgNone when it is free in none
__device__ __forceinline__ uint32_t pg_free_origin(const PgArgs& a, uint32_t g) {
    if (g >= a.n_frames) return kPgNone;
    const uint32_t o = a.frames[(size_t)g * kPgFrameWords + 14u];
    if (o >= g) return kPgNone;
    for (uint32_t h = o + 1u; h <= g; h++)
        if (!pg_member(a.frames + (size_t)h * kPgFrameWords, o)) return kPgNone;
    return o;
}

// PG-2: the free nodes of segment o are frames o + 1 .. o + n
__device__ __forceinline__ uint32_t pg_segment_nodes(const PgArgs& a, uint32_t o) {
    uint32_t n = 0u;
    while (o + 1u + n < a.n_frames && pg_member(a.frames + (size_t)(o + 1u + n) * kPgFrameWords, o)) n++;
    return n;
}

__device__ __forceinline__ bool pg_segment_invalid(const PgArgs& a, uint32_t o, uint32_t n) {
    bool fin = true;
    for (uint32_t j = 0u; j < n; j++) {
        const uint32_t* const rec = a.frames + (size_t)(o + 1u + j) * kPgFrameWords;
#pragma unroll
        for (int k = 0; k < 12; k++) fin = fin && pg_bits_finite(rec[k]);
    }
    return !fin;
}

__device__ __forceinline__ bool pg_is_node(const PgArgs& a, uint32_t g, uint32_t o) { return g == o || pg_free_origin(a, g) == o; }

// grid ceil(n_pairs / kPgThreads), block kPgThreads
__global__ __launch_bounds__(kPgThreads) void k_pg_edges(PgArgs a) {
    const uint32_t i = blockIdx.x * kPgThreads + threadIdx.x;
    if (i >= a.n_pairs) return;
    const uint32_t* const fix = a.fixes + (size_t)i * kPgFixWords;
    const uint2 e = a.list[i];
    const uint32_t q = e.x, T = e.y, F = a.n_frames, st = fix[30], o = fix[25], qo = fix[26];
    uint32_t v;
    if (!(st == ORB_LOCALIZE_OK || (st == ORB_LOCALIZE_MINIMAL && a.use_minimal))) {
        v = ORB_GRAPH_EDGE_STATUS;
    } else if (fix[28] < a.min_inliers) {
        v = ORB_GRAPH_EDGE_FEW;
    } else if (q >= F || T >= F || qo == kPgNone) {
        v = ORB_GRAPH_EDGE_RANGE;
    } else if (o != qo || !pg_is_node(a, q, o) || !pg_is_node(a, T, o)) {
        v = ORB_GRAPH_EDGE_SEGMENT;
    } else {
        bool fin = true;
#pragma unroll
        for (int k = 0; k < 12; k++) fin = fin && pg_bits_finite(fix[k]);
        if (!fin)
            v = ORB_GRAPH_EDGE_NONFINITE;
        else
            v = pg_segment_invalid(a, o, pg_segment_nodes(a, o)) ? ORB_GRAPH_EDGE_SEGMENT_INVALID : ORB_GRAPH_EDGE_USED;
    }
    uint32_t* const out = a.edges + (size_t)i * kPgEdgeWords;
    out[0] = v;
    out[1] = 0u;
    out[2] = 0u;
    out[3] = o;
}

// grid 1, block kPgThreads: thread t owns the frames t * per .. t * per + per - 1
__global__ __launch_bounds__(kPgThreads) void k_pg_index(PgArgs a) {
    __shared__ uint2 s_e[kPgTile];
    __shared__ uint32_t s_sum[kPgThreads];
    const uint32_t tid = threadIdx.x, F = a.n_frames, per = (F + kPgThreads - 1u) / kPgThreads;
    uint32_t pos = 0u;
    for (uint32_t pass = 0u; pass < 2u; pass++) {  // count, then fill from the thread's start
        for (uint32_t c = 0u; c < per; c++) {
            const uint32_t f = tid * per + c;
            for (uint32_t t0 = 0u; t0 < a.n_pairs; t0 += kPgTile) {
                const uint32_t tn = min(a.n_pairs - t0, kPgTile);
                __syncthreads();
                for (uint32_t k = tid; k < tn; k += kPgThreads)
                    s_e[k] = a.edges[(size_t)(t0 + k) * kPgEdgeWords] == ORB_GRAPH_EDGE_USED ? a.list[t0 + k] : make_uint2(kPgNone, kPgNone);
                __syncthreads();
                if (f < F)
                    for (uint32_t k = 0u; k < tn; k++) {
                        const uint2 e = s_e[k];
                        if (e.x == f || e.y == f) {
                            if (pass) a.col[pos] = t0 + k;
                            pos++;
                        }
                    }
            }
            if (pass && f < F) a.row[f + 1u] = pos;
        }
        if (!pass) {
            s_sum[tid] = pos;
            __syncthreads();
            pos = 0u;
            for (uint32_t t = 0u; t < tid; t++) pos += s_sum[t];
            if (tid == 0u) a.row[0] = 0u;
        }
    }
}

// grid ceil(F / kPgThreads), block kPgThreads
__global__ __launch_bounds__(kPgThreads) void k_pg_write(PgArgs a) {
    const uint32_t g = blockIdx.x * kPgThreads + threadIdx.x;
    if (g >= a.n_frames) return;
    const uint32_t* const rec = a.frames + (size_t)g * kPgFrameWords;
    const uint32_t o = pg_free_origin(a, g);
    uint32_t status = ORB_GRAPH_HELD;
    if (o != kPgNone) status = pg_segment_invalid(a, o, pg_segment_nodes(a, o)) ? ORB_GRAPH_INVALID : ORB_GRAPH_UNCHANGED;
    uint32_t* const out = a.out + (size_t)g * kPgPoseWords;
#pragma unroll
    for (int k = 0; k < 12; k++) out[k] = rec[k];
    out[12] = 0u;
    out[13] = 0u;
    out[14] = 0u;
    out[15] = status;
}

// PG-5: what an edge (a -> b) is under the current poses
struct PgGeom {
    float Rh[9];  // R^ = R_b R_a^T
    float s[3];   // R^ t_a
    float th[3];  // t^ = t_b - R^ t_a
    float ta[3];
};

__device__ __forceinline__ void pg_matvec(const float M[9], const float v[3], float out[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = (M[3 * r] * v[0] + M[3 * r + 1] * v[1]) + M[3 * r + 2] * v[2];
}
__device__ __forceinline__ void pg_matvec_t(const float M[9], const float v[3], float out[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = (M[r] * v[0] + M[3 + r] * v[1]) + M[6 + r] * v[2];
}
__device__ __forceinline__ void pg_cross(const float x[3], const float y[3], float out[3]) {
    out[0] = x[1] * y[2] - x[2] * y[1];
    out[1] = x[2] * y[0] - x[0] * y[2];
    out[2] = x[0] * y[1] - x[1] * y[0];
}

// a_held: camera a is the segment's origin, the identity -- R^ = R_b and t^ = t_b exactly
__device__ __forceinline__ void pg_geom(const float Ra[9], const float ta[3], const float Rb[9], const float tb[3], bool a_held, PgGeom& G) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float v = (Rb[3 * r] * Ra[3 * c] + Rb[3 * r + 1] * Ra[3 * c + 1]) + Rb[3 * r + 2] * Ra[3 * c + 2];
            G.Rh[3 * r + c] = a_held ? Rb[3 * r + c] : v;
        }
    float s[3];
    pg_matvec(G.Rh, ta, s);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        G.ta[r] = a_held ? 0.0f : ta[r];
        G.s[r] = a_held ? 0.0f : s[r];
        G.th[r] = tb[r] - G.s[r];
    }
}

// PG-5: e = (e_R, e_t) against the measurement (R_z, t_z)
__device__ __forceinline__ void pg_residual(const PgGeom& G, const float Rz[9], const float tz[3], float e[6]) {
    float E[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) E[3 * r + c] = (G.Rh[3 * r] * Rz[3 * c] + G.Rh[3 * r + 1] * Rz[3 * c + 1]) + G.Rh[3 * r + 2] * Rz[3 * c + 2];
    e[0] = 0.5f * (E[7] - E[5]);
    e[1] = 0.5f * (E[2] - E[6]);
    e[2] = 0.5f * (E[3] - E[1]);
#pragma unroll
    for (int r = 0; r < 3; r++) e[3 + r] = G.th[r] - tz[r];
}

__device__ __forceinline__ float pg_edge_cost(const float e[6], float w, float rho) {
    return w * (rho * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]) + ((e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]));
}

// u = J_b p_b - (-J_a) p_a; a NULL end is held and has no columns
__device__ __forceinline__ void pg_forward(const PgGeom& G, const float* pa, const float* pb, float u[6]) {
    float vb[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, va[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (pb) {
        float c[3];
        pg_cross(G.s, pb, c);
#pragma unroll
        for (int r = 0; r < 3; r++) vb[r] = pb[r], vb[3 + r] = c[r] + pb[3 + r];
    }
    if (pa) {
        float c[3], d[3];
        pg_cross(G.ta, pa, c);
#pragma unroll
        for (int r = 0; r < 3; r++) d[r] = c[r] + pa[3 + r];
        pg_matvec(G.Rh, pa, va);
        pg_matvec(G.Rh, d, va + 3);
    }
#pragma unroll
    for (int k = 0; k < 6; k++) u[k] = vb[k] - va[k];
}

// the node's share J^T (w W u) of an edge: as its head b or as its tail a
__device__ __forceinline__ void pg_back(const PgGeom& G, bool head, float w, float rho, const float u[6], float c[6]) {
    float qR[3], qt[3];
#pragma unroll
    for (int r = 0; r < 3; r++) qR[r] = w * (rho * u[r]), qt[r] = w * u[3 + r];
    if (head) {
        float x[3];
        pg_cross(qt, G.s, x);
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = qR[r] + x[r], c[3 + r] = qt[r];
    } else {
        float x[3], y[3], z[3];
        pg_matvec_t(G.Rh, qR, x);
        pg_matvec_t(G.Rh, qt, y);
        pg_cross(G.ta, y, z);
#pragma unroll
        for (int r = 0; r < 3; r++) c[r] = z[r] - x[r], c[3 + r] = -y[r];
    }
}

// A segment in k_pg_solve: its node words W with stride S between the words of one node
struct PgSeg {
    float* W;
    uint32_t S, o, n;
};

template <int N>
__device__ __forceinline__ void pg_load(const PgSeg& g, uint32_t word, uint32_t j, float* dst) {
#pragma unroll
    for (int k = 0; k < N; k++) dst[k] = g.W[(size_t)(word + k) * g.S + j];
}
template <int N>
__device__ __forceinline__ void pg_store(const PgSeg& g, uint32_t word, uint32_t j, const float* src) {
#pragma unroll
    for (int k = 0; k < N; k++) g.W[(size_t)(word + k) * g.S + j] = src[k];
}

// the current pose of frame f of the segment: node f - o - 1, or the identity for the origin
__device__ __forceinline__ void pg_pose(const PgSeg& g, uint32_t f, float R[9], float t[3]) {
    if (f == g.o) {
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (k & 3) == 0 ? 1.0f : 0.0f;
        t[0] = t[1] = t[2] = 0.0f;
    } else {
        pg_load<9>(g, kPgPose, f - g.o - 1u, R);
        pg_load<3>(g, kPgPose + 9u, f - g.o - 1u, t);
    }
}

// the same from the trajectory's record
__device__ __forceinline__ void pg_record_pose(const PgArgs& a, uint32_t o, uint32_t f, float R[9], float t[3]) {
    const uint32_t* const rec = a.frames + (size_t)f * kPgFrameWords;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = f == o ? ((k & 3) == 0 ? 1.0f : 0.0f) : __uint_as_float(rec[k]);
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = f == o ? 0.0f : __uint_as_float(rec[9 + k]);
}

// PG-5's edge order for the node of frame f: the chain edge into it, the chain edge out of it, its loop edges in ascending list
// index.  fn(G, head, fa, fb, w, i): the edge's geometry, whether f is its head, its two frames, its weight and its list index
// (kPgNone for a chain edge).
template <class Fn>
__device__ __forceinline__ void pg_for_edges(const PgArgs& a, const PgSeg& g, uint32_t f, Fn&& fn) {
    float Rf[9], tf[3], Ro[9], to[3];
    PgGeom G;
    pg_pose(g, f, Rf, tf);
    pg_pose(g, f - 1u, Ro, to);
    pg_geom(Ro, to, Rf, tf, f - 1u == g.o, G);
    fn(G, true, f - 1u, f, 1.0f, kPgNone);
    if (f < g.o + g.n) {
        pg_pose(g, f + 1u, Ro, to);
        pg_geom(Rf, tf, Ro, to, false, G);
        fn(G, false, f, f + 1u, 1.0f, kPgNone);
    }
    for (uint32_t k = a.row[f]; k < a.row[f + 1u]; k++) {
        const uint32_t i = a.col[k];
        if (a.edges[(size_t)i * kPgEdgeWords + 3u] != g.o) continue;  // the frame that ends this segment begins another: that one's edge
        const uint2 e = a.list[i];  // (q, T): the edge T -> q
        const bool head = e.x == f;
        pg_pose(g, head ? e.y : e.x, Ro, to);
        if (head)
            pg_geom(Ro, to, Rf, tf, e.y == g.o, G);
        else
            pg_geom(Rf, tf, Ro, to, false, G);
        fn(G, head, e.y, e.x, a.loop_weight, i);
    }
}

// PG-3 / PG-4: the measurement of an edge: of a chain edge from the records as read, of a loop edge the fix
__device__ __forceinline__ void pg_measurement(const PgArgs& a, uint32_t o, uint32_t fa, uint32_t fb, uint32_t i, float Rz[9], float tz[3]) {
    if (i == kPgNone) {
        float Ra[9], ta[3], Rb[9], tb[3];
        PgGeom M;
        pg_record_pose(a, o, fa, Ra, ta);
        pg_record_pose(a, o, fb, Rb, tb);
        pg_geom(Ra, ta, Rb, tb, fa == o, M);
#pragma unroll
        for (int k = 0; k < 9; k++) Rz[k] = M.Rh[k];
#pragma unroll
        for (int k = 0; k < 3; k++) tz[k] = M.th[k];
    } else {
        const uint32_t* const fix = a.fixes + (size_t)i * kPgFixWords;
#pragma unroll
        for (int k = 0; k < 9; k++) Rz[k] = __uint_as_float(fix[k]);
#pragma unroll
        for (int k = 0; k < 3; k++) tz[k] = __uint_as_float(fix[9 + k]);
    }
}

// PG-6: the sum of one value per thread: the 256 partials, GV-6's tree s = 128 .. 1 (every wave runs it on its own), one barrier
__device__ __forceinline__ float pg_reduce(float v, float (*s_red)[kPgThreads], uint32_t& parity) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    s_red[parity][tid] = v;
    __syncthreads();
    const float* const q = s_red[parity];
    float x = (q[lane] + q[lane + 128u]) + (q[lane + 64u] + q[lane + 192u]);
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x = x + __shfl_down(x, s, 64);
    parity ^= 1u;
    return __shfl(x, 0, 64);
}

__device__ __forceinline__ float pg_dot6(const float x[6], const float y[6]) {
    return ((((x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]) + x[3] * y[3]) + x[4] * y[4]) + x[5] * y[5];
}

// PG-7: the segment's cost under the current poses, the edges indexed by their head (a loop edge onto the origin by its tail);
// which 1 / 2: the loop edges' own costs into cost_before / cost_after
__device__ __forceinline__ float pg_cost(const PgArgs& a, const PgSeg& g, uint32_t which, float (*s_red)[kPgThreads], uint32_t& parity) {
    float acc = 0.0f;
    for (uint32_t j = threadIdx.x; j < g.n; j += kPgThreads) {
        const uint32_t f = g.o + 1u + j;
        float c = 0.0f;
        pg_for_edges(a, g, f, [&](const PgGeom& G, bool head, uint32_t fa, uint32_t fb, float w, uint32_t i) {
            if (!(head || (i != kPgNone && fb == g.o))) return;
            float Rz[9], tz[3], e[6];
            pg_measurement(a, g.o, fa, fb, i, Rz, tz);
            pg_residual(G, Rz, tz, e);
            const float ec = pg_edge_cost(e, w, a.rotation_weight);
            c = i == kPgNone ? ec : c + ec;
            if (which && i != kPgNone) a.edges[(size_t)i * kPgEdgeWords + which] = __float_as_uint(ec);
        });
        acc = acc + c;
    }
    return pg_reduce(acc, s_red, parity);
}

// z = D^-1 r
__device__ __forceinline__ void pg_precondition(const float Dinv[36], const float r[6], float z[6]) {
#pragma unroll
    for (int i = 0; i < 6; i++) z[i] = pg_dot6(Dinv + 6 * i, r);
}

__device__ __forceinline__ void pg_solve_segment(const PgArgs& a, const PgSeg& g, uint32_t loops, float* part) {
    __shared__ float s_red[2][kPgThreads];
    __shared__ uint32_t s_fail;
    const uint32_t tid = threadIdx.x;
    const float rho = a.rotation_weight;
    uint32_t parity = 0u;
    for (uint32_t j = tid; j < g.n; j += kPgThreads) {
        float R[9], t[3];
        pg_record_pose(a, g.o, g.o + 1u + j, R, t);
        pg_store<9>(g, kPgPose, j, R);
        pg_store<3>(g, kPgPose + 9u, j, t);
    }
    if (tid == 0u) s_fail = 0u;
    __syncthreads();
    const float cost_before = pg_cost(a, g, 1u, s_red, parity);
    float cost = cost_before;
    uint32_t status = ORB_GRAPH_REFINED;
    const uint32_t iterations = a.cg_iterations ? a.cg_iterations : min(g.n, kPgMaxCg);
#pragma unroll 1
    for (uint32_t round = 0u; round < a.rounds; round++) {
        // the poses of before the round into the records; g, D and D^-1 of every node
        for (uint32_t j = tid; j < g.n; j += kPgThreads) {
            const uint32_t f = g.o + 1u + j;
            float pose[12], grad[6] = {}, D[36] = {};
            pg_load<12>(g, kPgPose, j, pose);
            uint32_t* const out = a.out + (size_t)f * kPgPoseWords;
#pragma unroll
            for (int k = 0; k < 12; k++) out[k] = __float_as_uint(pose[k]);
            pg_for_edges(a, g, f, [&](const PgGeom& G, bool head, uint32_t fa, uint32_t fb, float w, uint32_t i) {
                const bool first = i == kPgNone && head;
                float Rz[9], tz[3], e[6], c[6];
                pg_measurement(a, g.o, fa, fb, i, Rz, tz);
                pg_residual(G, Rz, tz, e);
                pg_back(G, head, w, rho, e, c);
#pragma unroll
                for (int k = 0; k < 6; k++) grad[k] = first ? c[k] : grad[k] + c[k];
#pragma unroll
                for (int col = 0; col < 6; col++) {
                    float unit[6], u[6];
#pragma unroll
                    for (int k = 0; k < 6; k++) unit[k] = k == col ? 1.0f : 0.0f;
                    pg_forward(G, head ? nullptr : unit, head ? unit : nullptr, u);
                    pg_back(G, head, w, rho, u, c);
#pragma unroll
                    for (int k = 0; k < 6; k++) D[6 * k + col] = first ? c[k] : D[6 * k + col] + c[k];
                }
            });
            pg_store<6>(g, kPgGrad, j, grad);
            // PG-6: D^-1 by section 21's solver on the six unit vectors; it reads the upper triangle of D
            float aug[6][7], sol[6], Dinv[36];
            bool ok = true;
            for (int r = 0, e = 0; r < 6; r++)
                for (int c = r; c < 6; c++, e++) part[e * 256 + tid] = D[6 * r + c];
            for (int col = 0; col < 6; col++) {
                for (int k = 0; k < 6; k++) part[(21 + k) * 256 + tid] = k == col ? 1.0f : 0.0f;
                ok = verify_solve_n<6>(reinterpret_cast<const float(*)[256]>(part + tid), aug, sol) != 0u && ok;
                for (int k = 0; k < 6; k++) Dinv[6 * k + col] = sol[k];
            }
            if (!ok) s_fail = 1u;
            pg_store<36>(g, kPgDinv, j, Dinv);
        }
        __syncthreads();
        if (s_fail) {
            status = ORB_GRAPH_FAILED;
            break;
        }
        // PG-6: x = 0, r = -g, z = D^-1 r, p = z
        float acc = 0.0f;
        for (uint32_t j = tid; j < g.n; j += kPgThreads) {
            float grad[6], Dinv[36], x[6], r[6], z[6];
            pg_load<6>(g, kPgGrad, j, grad);
            pg_load<36>(g, kPgDinv, j, Dinv);
#pragma unroll
            for (int k = 0; k < 6; k++) x[k] = 0.0f, r[k] = -grad[k];
            pg_precondition(Dinv, r, z);
            pg_store<6>(g, kPgX, j, x);
            pg_store<6>(g, kPgR, j, r);
            pg_store<6>(g, kPgP, j, z);
            acc = acc + pg_dot6(r, z);
        }
        float rz = pg_reduce(acc, s_red, parity);
#pragma unroll 1
        for (uint32_t it = 0u; it < iterations; it++) {
            acc = 0.0f;
            for (uint32_t j = tid; j < g.n; j += kPgThreads) {
                const uint32_t f = g.o + 1u + j;
                float hp[6] = {}, p[6];
                pg_for_edges(a, g, f, [&](const PgGeom& G, bool head, uint32_t fa, uint32_t fb, float w, uint32_t i) {
                    float pa[6], pb[6], u[6], c[6];
                    if (fa != g.o) pg_load<6>(g, kPgP, fa - g.o - 1u, pa);
                    if (fb != g.o) pg_load<6>(g, kPgP, fb - g.o - 1u, pb);
                    pg_forward(G, fa != g.o ? pa : nullptr, fb != g.o ? pb : nullptr, u);
                    pg_back(G, head, w, rho, u, c);
                    const bool first = i == kPgNone && head;
#pragma unroll
                    for (int k = 0; k < 6; k++) hp[k] = first ? c[k] : hp[k] + c[k];
                });
                pg_load<6>(g, kPgP, j, p);
                pg_store<6>(g, kPgHp, j, hp);
                acc = acc + pg_dot6(p, hp);
            }
            const float php = pg_reduce(acc, s_red, parity);
            if (!(isfinite(php) && php > 0.0f)) break;
            const float alpha = rz / php;
            acc = 0.0f;
            for (uint32_t j = tid; j < g.n; j += kPgThreads) {
                float Dinv[36], x[6], r[6], p[6], hp[6], z[6];
                pg_load<36>(g, kPgDinv, j, Dinv);
                pg_load<6>(g, kPgX, j, x);
                pg_load<6>(g, kPgR, j, r);
                pg_load<6>(g, kPgP, j, p);
                pg_load<6>(g, kPgHp, j, hp);
#pragma unroll
                for (int k = 0; k < 6; k++) x[k] = x[k] + alpha * p[k], r[k] = r[k] - alpha * hp[k];
                pg_precondition(Dinv, r, z);
                pg_store<6>(g, kPgX, j, x);
                pg_store<6>(g, kPgR, j, r);
                pg_store<6>(g, kPgHp, j, z);  // H p is spent: its words hold z until p is renewed
                acc = acc + pg_dot6(r, z);
            }
            const float rz_new = pg_reduce(acc, s_red, parity);
            const float beta = rz_new / rz;
            rz = rz_new;
            for (uint32_t j = tid; j < g.n; j += kPgThreads) {
                float p[6], z[6];
                pg_load<6>(g, kPgP, j, p);
                pg_load<6>(g, kPgHp, j, z);
#pragma unroll
                for (int k = 0; k < 6; k++) p[k] = z[k] + beta * p[k];
                pg_store<6>(g, kPgP, j, p);
            }
            __syncthreads();
        }
        // PG-5: R <- one polar step of (I + [w]x) R, t <- t + v
        for (uint32_t j = tid; j < g.n; j += kPgThreads) {
            float R[9], t[3], x[6], M[9];
            pg_load<9>(g, kPgPose, j, R);
            pg_load<3>(g, kPgPose + 9u, j, t);
            pg_load<6>(g, kPgX, j, x);
#pragma unroll
            for (int c = 0; c < 3; c++) {
                M[c] = R[c] + (x[1] * R[6 + c] - x[2] * R[3 + c]);
                M[3 + c] = R[3 + c] + (x[2] * R[c] - x[0] * R[6 + c]);
                M[6 + c] = R[6 + c] + (x[0] * R[3 + c] - x[1] * R[c]);
            }
            traj_polar_step(M);
#pragma unroll
            for (int k = 0; k < 3; k++) t[k] = t[k] + x[3 + k];
            pg_store<9>(g, kPgPose, j, M);
            pg_store<3>(g, kPgPose + 9u, j, t);
        }
        __syncthreads();
        // PG-7: a round that does not lower the cost is undone
        const float after = pg_cost(a, g, 0u, s_red, parity);
        if (!(isfinite(after) && after < cost)) {
            for (uint32_t j = tid; j < g.n; j += kPgThreads) {
                const uint32_t* const out = a.out + (size_t)(g.o + 1u + j) * kPgPoseWords;
                float pose[12];
#pragma unroll
                for (int k = 0; k < 12; k++) pose[k] = __uint_as_float(out[k]);
                pg_store<12>(g, kPgPose, j, pose);
            }
            status = ORB_GRAPH_STALLED;
            __syncthreads();
            break;
        }
        cost = after;
    }
    const float cost_after = pg_cost(a, g, 2u, s_red, parity);
    for (uint32_t j = tid; j < g.n; j += kPgThreads) {
        float pose[12];
        pg_load<12>(g, kPgPose, j, pose);
        uint32_t* const out = a.out + (size_t)(g.o + 1u + j) * kPgPoseWords;
#pragma unroll
        for (int k = 0; k < 12; k++) out[k] = __float_as_uint(pose[k]);
        out[12] = __float_as_uint(cost_before);
        out[13] = __float_as_uint(cost_after);
        out[14] = loops;
        out[15] = status;
    }
}

// grid F, block kPgThreads, kPgLdsBytes of dynamic LDS
__global__ __launch_bounds__(kPgThreads) void k_pg_solve(PgArgs a) {
    extern __shared__ __attribute__((aligned(16))) float pg_lds[];
    const uint32_t o = blockIdx.x;
    if (o + 1u >= a.n_frames || !pg_member(a.frames + (size_t)(o + 1u) * kPgFrameWords, o)) return;
    const uint32_t n = pg_segment_nodes(a, o);
    // a USED edge of the segment has both ends in the rows of its frames; an INVALID segment has none.  The rows of the first and the
    // last frame may hold edges of the segments that end and begin there.
    __shared__ uint32_t s_ends;
    if (threadIdx.x == 0u) s_ends = 0u;
    __syncthreads();
    uint32_t mine = 0u;
    for (uint32_t k = a.row[o] + threadIdx.x; k < a.row[o + n + 1u]; k += kPgThreads) mine += a.edges[(size_t)a.col[k] * kPgEdgeWords + 3u] == o ? 1u : 0u;
    if (mine) atomicAdd(&s_ends, mine);
    __syncthreads();
    const uint32_t ends = s_ends;
    if (!ends) return;
    float* const part = pg_lds + kPgX * kPgLdsNodes;
    if (n <= kPgLdsNodes)
        pg_solve_segment(a, PgSeg{pg_lds, kPgLdsNodes, o, n}, ends / 2u, part);
    else
        pg_solve_segment(a, PgSeg{a.work + (size_t)kPgNodeWords * (o + 1u), n, o, n}, ends / 2u, part);
}

}  // namespace orb
