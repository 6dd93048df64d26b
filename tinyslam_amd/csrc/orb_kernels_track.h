// orb_kernels_track.h -- feature tracks and keyframes over the consecutive-frame matches of a batch (not in the reference; the
// definition is the build's own, TK-1..TK-5 in DESIGN.md section 15).  Integer arithmetic throughout apart from GV-1's binary32
// ratio test, so the CPU restatement (tests/track_ref.py) gives the same bytes.
//
//   k_track_link   one workgroup per pair (f, f + 1): every query's link (TK-1) offers the key distance << 23 | i to its target with
//                  an atomicMin -- in LDS, or in a global key buffer when the targets do not fit (or TINYORB_TRACK_GLOBAL_KEYS=1) --
//                  and after a barrier a query whose key won keeps its link (TK-2): next[f][i], prev[f + 1][j]; the links are
//                  counted with wave ballots
//   k_track_jump   one thread per stored keypoint: one round of pointer doubling over prev (heads) and next (tails) at once,
//                  between two ping-pong buffers of (index, frame) pointers; the first round starts from the links themselves
//   k_track_hist   one workgroup per frame: the last doubling round, the OrbTrack records (TK-3), an LDS histogram of head_frame
//                  and its inclusive prefix: row f of shared(k, f), k <= f (TK-4)
//   k_track_key    one workgroup: TK-5's greedy keyframe walk, in chunks of 63 frames.  In a chunk the reference frame k is either
//                  the one the chunk started with or a frame of the chunk, so every decision the walk may ask for is computed
//                  beforehand in parallel -- one ballot per frame over those 64 candidate k -- and the walk itself is a scan over
//                  64-bit masks held in registers: one round of independent loads per chunk instead of a chain of dependent ones
#pragma once
#include "../../include/tinyorb.h"
#include "orb_kernels_staged.h"

namespace orb {

constexpr uint32_t kTrackNone = 0xffffffffu;
constexpr uint32_t kTrackMaxFrames = 4096u;     // n_frames bound: head_frame / tail_frame are 16 bits, the histogram 16 KB of LDS
constexpr uint32_t kTrackLinkThreads = 1024u;
constexpr uint32_t kTrackLdsKeys = 16320u;      // k_track_link keeps the keys in LDS up to this many targets (64 KB with its counter)
constexpr uint32_t kTrackJumpThreads = 256u;
constexpr uint32_t kTrackHistThreads = 1024u;
constexpr uint32_t kTrackBinsPerThread = kTrackMaxFrames / kTrackHistThreads;
constexpr uint32_t kTrackKeyThreads = 1024u;
constexpr uint32_t kTrackChunk = 63u;           // frames per step of k_track_key: 1 + 63 candidate reference frames = 64 ballot lanes

struct TrackArgs {
    const uint32_t* counts;          // [frames] raw counters of the batch
    uint32_t cap;
    uint32_t frames;                 // n_frames
    uint32_t stride;                 // row length of the shared table (max_batch)
    uint32_t source;                 // ORB_TRACK_*
    const MatchRecord* rec;          // [pairs][cap] the matcher's (VERIFIED, MATCHED) or the guided call's (GUIDED) records
    const uint8_t* mask;             // [pairs][cap] inlier bytes of the last verification (VERIFIED)
    uint32_t max_distance;           // GV-1 (GUIDED, MATCHED)
    float ratio;
    uint32_t* gkeys;                 // [pairs][cap] global keys (global form of k_track_link)
    uint32_t* prev;                  // [frames][cap]
    uint32_t* next;                  // [frames][cap]
    uint32_t* links;                 // [pairs] links of every pair
    uint4* ptr[2];                   // [frames][cap] ping-pong (head index, head frame, tail index, tail frame)
    uint32_t src;                    // which of ptr the round reads (not the first round)
    uint32_t first;                  // the round starts from prev / next
    uint4* out;                      // [frames][cap] OrbTrack
    uint32_t* shared;                // [frames][stride] shared(k, f) at [f][k], k <= f
    uint32_t min_gap, max_gap, keep_permille, min_shared;
    uint32_t* frame_out;             // [frames][8] OrbTrackFrame
};

// TK-1: the target of query i of pair f and the link's distance; false without a link.  Only called for i < n_f.
__device__ __forceinline__ bool track_link_of(const TrackArgs& a, uint32_t f, uint32_t i, uint32_t nt, uint32_t& j, uint32_t& d) {
    const size_t e = (size_t)f * a.cap + i;
    const MatchRecord r = a.rec[e];
    j = r.index;
    d = r.dist & 0xffffu;
    if (a.source == ORB_TRACK_VERIFIED) return a.mask[e] == 1u && j < nt;  // (an inlier byte of 1 implies j < nt)
    const uint32_t second = r.dist >> 16;
    return j != kTrackNone && j < nt && d <= a.max_distance && (float)d < a.ratio * (float)second;
}

// grid (pairs), block 1024; dynamic LDS 4 * cap bytes with kLds
template <bool kLds>
__global__ __launch_bounds__(kTrackLinkThreads) void k_track_link(TrackArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t track_lds[];
    __shared__ uint32_t n_links;
    const uint32_t f = blockIdx.x, tid = threadIdx.x, pairs = a.frames - 1u;
    const uint32_t nq = min(a.counts[f], a.cap), nt = min(a.counts[f + 1u], a.cap);
    uint32_t* const key = kLds ? track_lds : a.gkeys + (size_t)f * a.cap;
    for (uint32_t j = tid; j < nt; j += kTrackLinkThreads) key[j] = kTrackNone;
    if (tid == 0u) n_links = 0u;
    __syncthreads();
    for (uint32_t i = tid; i < nq; i += kTrackLinkThreads) {
        uint32_t j, d;
        if (track_link_of(a, f, i, nt, j, d)) atomicMin(&key[j], (d << 23) | i);
    }
    __syncthreads();
    uint32_t* const nx = a.next + (size_t)f * a.cap;
    uint32_t* const pv = a.prev + (size_t)(f + 1u) * a.cap;
    uint32_t won_count = 0u;
    for (uint32_t i0 = 0u; i0 < a.cap; i0 += kTrackLinkThreads) {
        const uint32_t i = i0 + tid;
        uint32_t j = kTrackNone, d, k = kTrackNone;
        bool won = false;
        if (i < nq && track_link_of(a, f, i, nt, j, d)) {
            k = kLds ? key[j] : __hip_atomic_load(&key[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            won = k == ((d << 23) | i);
        }
        won_count += (uint32_t)__popcll(__ballot(won));
        if (i < a.cap) nx[i] = won ? j : kTrackNone;
        if (i < a.cap) {
            uint32_t kj = kTrackNone;
            if (i < nt) kj = kLds ? key[i] : __hip_atomic_load(&key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            pv[i] = kj != kTrackNone ? (kj & 0x7fffffu) : kTrackNone;
        }
        if (f == 0u && i < a.cap) a.prev[i] = kTrackNone;  // frame 0 has no predecessor, the last frame no successor
        if (f + 1u == pairs && i < a.cap) a.next[(size_t)a.frames * a.cap - a.cap + i] = kTrackNone;
    }
    if ((tid & 63u) == 0u) atomicAdd(&n_links, won_count);
    __syncthreads();
    if (tid == 0u) a.links[f] = n_links;
}

// One doubling step of (f, i) < n_f: the head pointer h and the tail pointer t (x = index, y = frame) after the round.  The first
// round composes the links with themselves; later ones compose the pointers of the previous round (a chain's end points to itself).
__device__ __forceinline__ void track_jump_of(const TrackArgs& a, uint32_t f, uint32_t i, uint2& h, uint2& t) {
    const size_t cap = a.cap;
    if (a.first) {
        h = make_uint2(i, f);
        t = make_uint2(i, f);
        const uint32_t p = a.prev[(size_t)f * cap + i], n = a.next[(size_t)f * cap + i];
        if (p != kTrackNone) {
            const uint32_t pp = a.prev[(size_t)(f - 1u) * cap + p];
            h = pp != kTrackNone ? make_uint2(pp, f - 2u) : make_uint2(p, f - 1u);
        }
        if (n != kTrackNone) {
            const uint32_t nn = a.next[(size_t)(f + 1u) * cap + n];
            t = nn != kTrackNone ? make_uint2(nn, f + 2u) : make_uint2(n, f + 1u);
        }
    } else {
        const uint4* const src = a.ptr[a.src];
        const uint4 q = src[(size_t)f * cap + i];
        const uint4 qh = src[(size_t)q.y * cap + q.x], qt = src[(size_t)q.w * cap + q.z];
        h = make_uint2(qh.x, qh.y);
        t = make_uint2(qt.z, qt.w);
    }
}

// grid (ceil(cap / 256), frames), block 256
__global__ __launch_bounds__(kTrackJumpThreads) void k_track_jump(TrackArgs a) {
    const uint32_t f = blockIdx.y, i = blockIdx.x * kTrackJumpThreads + threadIdx.x;
    if (i >= min(a.counts[f], a.cap)) return;
    uint2 h, t;
    track_jump_of(a, f, i, h, t);
    a.ptr[a.src ^ 1u][(size_t)f * a.cap + i] = make_uint4(h.x, h.y, t.x, t.y);
}

// grid (frames), block 1024
__global__ __launch_bounds__(kTrackHistThreads) void k_track_hist(TrackArgs a) {
    __shared__ uint32_t hist[kTrackMaxFrames];
    __shared__ uint32_t wave_sum[kTrackHistThreads / 64u];
    const uint32_t f = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t n = min(a.counts[f], a.cap), nbins = f + 1u;
    for (uint32_t b = tid; b < nbins; b += kTrackHistThreads) hist[b] = 0u;
    __syncthreads();
    uint4* const out = a.out + (size_t)f * a.cap;
    for (uint32_t i = tid; i < a.cap; i += kTrackHistThreads) {
        if (i < n) {
            uint2 h, t;
            track_jump_of(a, f, i, h, t);
            const size_t e = (size_t)f * a.cap + i;
            out[i] = make_uint4(a.prev[e], a.next[e], h.x, h.y | (t.y << 16));
            atomicAdd(&hist[h.y], 1u);
        } else {
            out[i] = make_uint4(kTrackNone, kTrackNone, kTrackNone, 0xffffffffu);
        }
    }
    __syncthreads();
    // inclusive prefix over the bins 0..f: thread t owns bins 4t .. 4t + 3; a wave scan of the thread sums, then the wave sums
    uint32_t v[kTrackBinsPerThread], s = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kTrackBinsPerThread; k++) {
        const uint32_t b = tid * kTrackBinsPerThread + k;
        v[k] = b < nbins ? hist[b] : 0u;
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
    uint32_t run = incl - s;
    for (uint32_t w = 0; w < wave; w++) run += wave_sum[w];
    uint32_t* const row = a.shared + (size_t)f * a.stride;
#pragma unroll
    for (uint32_t k = 0; k < kTrackBinsPerThread; k++) {
        const uint32_t b = tid * kTrackBinsPerThread + k;
        run += v[k];
        if (b < nbins) row[b] = run;
    }
}

// TK-5 for reference frame k and frame f > k: is f a keyframe?
__device__ __forceinline__ bool track_is_key(const TrackArgs& a, uint32_t f, uint32_t k, uint32_t s, uint32_t base) {
    const uint32_t g = f - k;
    if (g < a.min_gap) return false;
    return (a.max_gap != 0u && g >= a.max_gap) || s == 0u ||
           (uint64_t)s * 1000u < (uint64_t)a.keep_permille * base || s < a.min_shared;
}

// grid (1), block 1024
__global__ __launch_bounds__(kTrackKeyThreads) void k_track_key(TrackArgs a) {
    __shared__ unsigned long long dec[kTrackChunk];        // bit c: the decision of frame f0 + r against candidate c
    __shared__ uint32_t sval[kTrackChunk][kTrackChunk + 1u];  // shared(candidate c, f0 + r)
    __shared__ uint32_t k_next;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t F = a.frames, pairs = F - 1u;
    auto links_out = [&](uint32_t k) { return k < pairs ? a.links[k] : 0u; };
    auto write_frame = [&](uint32_t f, uint32_t key, uint32_t ref, uint32_t s) {
        uint4* const o = reinterpret_cast<uint4*>(a.frame_out + (size_t)f * 8u);
        o[0] = make_uint4(min(a.counts[f], a.cap), f ? a.links[f - 1u] : 0u, links_out(f), key);
        o[1] = make_uint4(ref, s, 0u, 0u);
    };
    if (tid == 0u) write_frame(0u, 1u, 0u, a.shared[0]);
    uint32_t ks = 0u;  // the reference frame the chunk starts with
    for (uint32_t f0 = 1u; f0 < F; f0 += kTrackChunk) {
        const uint32_t rows = min(kTrackChunk, F - f0);
        // candidate c of row r: k = ks (c = 0) or k = f0 + c - 1 (1 <= c <= r); each wave decides rows r = wave, wave + 16, ...
        for (uint32_t r = wave; r < rows; r += kTrackKeyThreads / 64u) {
            const uint32_t f = f0 + r, c = lane;
            bool key = false;
            if (c <= r) {
                const uint32_t k = c ? f0 + c - 1u : ks;
                const uint32_t s = a.shared[(size_t)f * a.stride + k];
                sval[r][c] = s;
                key = track_is_key(a, f, k, s, links_out(k));
            }
            const unsigned long long m = __ballot(key);
            if (lane == 0u) dec[r] = m;
        }
        __syncthreads();
        if (wave == 0u) {  // the walk: kc is the candidate index of the current reference frame
            const unsigned long long m = lane < rows ? dec[lane] : 0ull;
            const uint32_t mlo = (uint32_t)m, mhi = (uint32_t)(m >> 32);
            uint32_t kc = 0u, mine = 0u;
            for (uint32_t r = 0u; r < rows; r++) {
                // (readlane returns an int: through uint32_t, or the low word's sign would spread into the high one)
                const unsigned long long mr = (unsigned long long)(uint32_t)__builtin_amdgcn_readlane(mlo, r) |
                                              ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane(mhi, r) << 32);
                if (lane == r) mine = kc;
                if ((mr >> kc) & 1ull) kc = r + 1u;
            }
            if (lane < rows) write_frame(f0 + lane, (uint32_t)((m >> mine) & 1ull), mine ? f0 + mine - 1u : ks, sval[lane][mine]);
            if (lane == 0u) k_next = kc ? f0 + kc - 1u : ks;
        }
        __syncthreads();
        ks = k_next;
        __syncthreads();
    }
}

}  // namespace orb
