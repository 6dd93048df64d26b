// orb_kernels_place.h -- loop candidates by descriptor-signature overlap over the frames of a batch and a database of earlier
// signatures (not in the reference; the definition is the build's own, PL-1..PL-6 in DESIGN.md section 25).  Integer arithmetic
// throughout, so the CPU restatement (tests/place_ref.py) gives the same bytes.
//
//   k_place_sign     one workgroup per (table, frame): the table's bitmap of 2^bits bits (at most 8 KB) is built in LDS with one
//                    atomicOr per stored record (PL-1, PL-2), stored with 16-byte stores -- every word of it, so a call leaves
//                    nothing of the call before -- and its set bits are counted into the frame's word of that table
//   k_place_score    one workgroup per tile of 32 query frames x 32 ids (PL-4: database entries, then the batch's frames): the
//                    signatures of both sides are staged in LDS 64 words at a time, each read from memory once per tile, and a
//                    thread keeps the popcount of the AND (PL-3) of 2 x 2 pairs.  A tile that holds no eligible pair is left out;
//                    the selection never reads its scores.  A batch has few tiles (256 frames: 8 x 8, about half of them left
//                    out), so the words of a signature are cut into up to 8 slices, one workgroup each, that write partial
//                    scores side by side -- plain stores, summed by the selection -- where the score buffer has the room
//   k_place_select   one wave per query frame: every lane keeps the 8 greatest keys score << 32 | ~id (PL-6) of the eligible ids
//                    it walks (PL-4, PL-5), and the row is the `top` greatest of the wave, taken one at a time by a wave-wide
//                    maximum.  The keys are distinct, so the row does not depend on any order of execution
#pragma once
#include "../../include/tinyorb.h"
#include "orb_kernels_staged.h"

namespace orb {

constexpr uint32_t kPlaceSignThreads = 256u;
constexpr uint32_t kPlaceMaxTableWords = 2048u;  // 2^16 bits
constexpr uint32_t kPlaceMaxTables = 16u;        // row length of the per-table bit counts
constexpr uint32_t kPlaceTile = 32u;             // queries and ids of a tile of k_place_score
constexpr uint32_t kPlaceChunk = 64u;            // words of a signature staged at a time
constexpr uint32_t kPlaceRowVec = kPlaceChunk / 4u + 1u;  // LDS row of a staged chunk in 16-byte pieces: one more than it holds,
                                                          // so that the 16 rows a wave reads at one k lie in 16 different slots
constexpr uint32_t kPlaceScoreThreads = 256u;
constexpr uint32_t kPlaceMaxSlices = 8u;         // of a signature's words, one workgroup of a tile each
constexpr uint32_t kPlaceWantedGroups = 1024u;   // slices are added while a call has fewer workgroups than this
constexpr uint32_t kPlaceSelectThreads = 64u;
constexpr uint32_t kPlaceRowWords = 24u;         // OrbPlaceRow
constexpr uint32_t kPlaceTop = 8u;
constexpr uint32_t kPlaceFrameWords = 8u;        // OrbTrackFrame
constexpr uint32_t kPlaceKeyframeWord = 3u;      // OrbTrackFrame::keyframe

struct PlaceArgs {
    const uint32_t* counts;          // [frames] raw counters of the batch
    const CornerDescriptor* desc;    // [frames][cap]
    uint32_t cap;
    uint32_t n_frames;
    uint32_t bits, tables;
    uint32_t words;                  // of a signature: tables << (bits - 5)
    uint32_t slices, slice_words;    // k_place_score: slice z scores words [z * slice_words, (z + 1) * slice_words), whole chunks
    uint32_t n_db;
    uint32_t min_gap, top, min_score, min_permille;
    const uint32_t* keyframe;        // the track stage's [frames][8] OrbTrackFrame with ORB_PLACE_KEYFRAMES, else null
    uint32_t* sig;                   // [n_frames][words]
    const uint32_t* db;              // [n_db][words]
    uint32_t* tbits;                 // [n_frames][kPlaceMaxTables] set bits per table
    uint32_t* score;                 // [slices][n_frames][n_db + n_frames] partial scores
    uint32_t* rows;                  // [n_frames][24] OrbPlaceRow
};

// grid (tables, n_frames), block 256
__global__ __launch_bounds__(kPlaceSignThreads) void k_place_sign(PlaceArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t bitmap[kPlaceMaxTableWords];
    __shared__ uint32_t wave_bits[kPlaceSignThreads / 64u];
    const uint32_t t = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const uint32_t tw = 1u << (a.bits - 5u);  // words of one table, 8..2048
    for (uint32_t w = tid; w < tw; w += kPlaceSignThreads) bitmap[w] = 0u;
    __syncthreads();
    const uint32_t n = min(a.counts[f], a.cap), mask = (1u << a.bits) - 1u, shift = 16u * (t & 1u);
    const uint32_t* const d = reinterpret_cast<const uint32_t*>(a.desc + (size_t)f * a.cap) + (t >> 1);
    for (uint32_t i = tid; i < n; i += kPlaceSignThreads) {
        const uint32_t key = (d[(size_t)i * 8u] >> shift) & mask;  // PL-1 (bits <= 16: the mask takes the half as well)
        atomicOr(&bitmap[key >> 5], 1u << (key & 31u));
    }
    __syncthreads();
    uint4* const out = reinterpret_cast<uint4*>(a.sig + (size_t)f * a.words + (size_t)t * tw);
    const uint4* const src = reinterpret_cast<const uint4*>(bitmap);
    uint32_t set = 0u;
    for (uint32_t v = tid; v < tw / 4u; v += kPlaceSignThreads) {
        const uint4 q = src[v];
        out[v] = q;
        set += __popc(q.x) + __popc(q.y) + __popc(q.z) + __popc(q.w);
    }
#pragma unroll
    for (uint32_t o = 32u; o; o >>= 1) set += __shfl_xor(set, o, 64);
    if ((tid & 63u) == 0u) wave_bits[tid >> 6] = set;
    __syncthreads();
    if (tid == 0u) a.tbits[f * kPlaceMaxTables + t] = wave_bits[0] + wave_bits[1] + wave_bits[2] + wave_bits[3];
}

// PL-4 for a batch frame g against query f, the keyframe test apart
__device__ __forceinline__ bool place_gap_ok(const PlaceArgs& a, uint32_t g, uint32_t f) { return (uint64_t)g + a.min_gap <= f; }

// grid (ceil((n_db + n_frames) / 32), ceil(n_frames / 32), slices), block 256: thread (ty, tx) owns queries q0 + ty, q0 + ty + 16
// and ids i0 + tx, i0 + tx + 16
__global__ __launch_bounds__(kPlaceScoreThreads) void k_place_score(PlaceArgs a) {
    __shared__ uint4 stage[2u * kPlaceTile * kPlaceRowVec];  // rows 0..31 the queries, 32..63 the ids
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * kPlaceTile, q0 = blockIdx.y * kPlaceTile, n_ids = a.n_db + a.n_frames;
    const uint32_t q_last = min(q0 + kPlaceTile, a.n_frames) - 1u;
    if (i0 >= a.n_db && !place_gap_ok(a, i0 - a.n_db, q_last)) return;  // batch frames only, none eligible for any query of the tile
    // the rows this thread stages: piece `vc` of rows vr, vr + 16, vr + 32, vr + 48
    const uint32_t vc = tid & 15u, vr = tid >> 4;
    const uint4* row[4];
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
        const uint32_t lr = vr + 16u * r;
        const uint32_t* base = nullptr;
        if (lr < kPlaceTile) {
            const uint32_t q = q0 + lr;
            if (q < a.n_frames) base = a.sig + (size_t)q * a.words;
        } else {
            const uint32_t id = i0 + lr - kPlaceTile;
            if (id < a.n_db)
                base = a.db + (size_t)id * a.words;
            else if (id < n_ids)
                base = a.sig + (size_t)(id - a.n_db) * a.words;
        }
        row[r] = reinterpret_cast<const uint4*>(base);
    }
    uint32_t acc[2][2] = {{0u, 0u}, {0u, 0u}};
    const uint32_t k_end = min(a.words, (blockIdx.z + 1u) * a.slice_words);
    for (uint32_t k0 = blockIdx.z * a.slice_words; k0 < k_end; k0 += kPlaceChunk) {
        const uint32_t kv = min(kPlaceChunk, k_end - k0) / 4u;  // pieces of this chunk (words is a multiple of 8)
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (row[r] && vc < kv) v = row[r][k0 / 4u + vc];
            stage[(vr + 16u * r) * kPlaceRowVec + vc] = v;
        }
        __syncthreads();
        const uint4* const qa = stage + ty * kPlaceRowVec;
        const uint4* const qb = stage + (ty + 16u) * kPlaceRowVec;
        const uint4* const ia = stage + (kPlaceTile + tx) * kPlaceRowVec;
        const uint4* const ib = stage + (kPlaceTile + tx + 16u) * kPlaceRowVec;
        for (uint32_t c = 0u; c < kv; c++) {
            const uint4 x0 = qa[c], x1 = qb[c], y0 = ia[c], y1 = ib[c];
            acc[0][0] += __popc(x0.x & y0.x) + __popc(x0.y & y0.y) + __popc(x0.z & y0.z) + __popc(x0.w & y0.w);
            acc[0][1] += __popc(x0.x & y1.x) + __popc(x0.y & y1.y) + __popc(x0.z & y1.z) + __popc(x0.w & y1.w);
            acc[1][0] += __popc(x1.x & y0.x) + __popc(x1.y & y0.y) + __popc(x1.z & y0.z) + __popc(x1.w & y0.w);
            acc[1][1] += __popc(x1.x & y1.x) + __popc(x1.y & y1.y) + __popc(x1.z & y1.z) + __popc(x1.w & y1.w);
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t j = 0; j < 2u; j++)
#pragma unroll
        for (uint32_t i = 0; i < 2u; i++) {
            const uint32_t q = q0 + ty + 16u * j, id = i0 + tx + 16u * i;
            if (q < a.n_frames && id < n_ids) a.score[((size_t)blockIdx.z * a.n_frames + q) * n_ids + id] = acc[j][i];
        }
}

// grid (n_frames), block 64
__global__ __launch_bounds__(kPlaceSelectThreads) void k_place_select(PlaceArgs a) {
    const uint32_t f = blockIdx.x, lane = threadIdx.x, n_ids = a.n_db + a.n_frames;
    uint32_t bits_f = 0u;
    for (uint32_t t = 0u; t < a.tables; t++) bits_f += a.tbits[f * kPlaceMaxTables + t];
    const uint32_t floor_score = max(a.min_score, 1u);
    const uint64_t floor_permille = (uint64_t)a.min_permille * bits_f;
    unsigned long long best[kPlaceTop];
#pragma unroll
    for (uint32_t j = 0; j < kPlaceTop; j++) best[j] = 0ull;  // a candidate's key is at least 1 << 32
    uint32_t eligible = 0u, candidates = 0u;
    const uint32_t* const srow = a.score + (size_t)f * n_ids;
    for (uint32_t id = lane; id < n_ids; id += kPlaceSelectThreads) {
        if (id >= a.n_db) {  // PL-4
            const uint32_t g = id - a.n_db;
            if (!place_gap_ok(a, g, f)) continue;
            if (a.keyframe && a.keyframe[(size_t)g * kPlaceFrameWords + kPlaceKeyframeWord] == 0u) continue;
        }
        eligible++;
        uint32_t s = 0u;
        for (uint32_t z = 0u; z < a.slices; z++) s += srow[(size_t)z * a.n_frames * n_ids + id];
        if (s < floor_score || (uint64_t)s * 1000u < floor_permille) continue;  // PL-5
        candidates++;
        unsigned long long k = ((unsigned long long)s << 32) | (0xffffffffu - id);  // PL-6
#pragma unroll
        for (uint32_t j = 0; j < kPlaceTop; j++) {
            const unsigned long long b = best[j];
            const bool up = k > b;
            best[j] = up ? k : b;
            k = up ? b : k;
        }
    }
#pragma unroll
    for (uint32_t o = 32u; o; o >>= 1) {
        eligible += __shfl_xor(eligible, o, 64);
        candidates += __shfl_xor(candidates, o, 64);
    }
    uint32_t out_frame[kPlaceTop], out_score[kPlaceTop];
#pragma unroll
    for (uint32_t r = 0; r < kPlaceTop; r++) {
        unsigned long long m = r < a.top ? best[0] : 0ull;
#pragma unroll
        for (uint32_t o = 32u; o; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o, 64);
            m = other > m ? other : m;
        }
        if (m != 0ull && best[0] == m) {  // the one lane that holds it moves on to its next
#pragma unroll
            for (uint32_t j = 0; j + 1u < kPlaceTop; j++) best[j] = best[j + 1u];
            best[kPlaceTop - 1u] = 0ull;
        }
        const uint32_t id = 0xffffffffu - (uint32_t)m;
        out_frame[r] = m == 0ull ? ORB_MATCH_NONE : (id < a.n_db ? (ORB_PLACE_DB | id) : id - a.n_db);
        out_score[r] = (uint32_t)(m >> 32);
    }
    if (lane == 0u) {
        uint4* const o = reinterpret_cast<uint4*>(a.rows + (size_t)f * kPlaceRowWords);
        o[0] = make_uint4(min(a.counts[f], a.cap), bits_f, eligible, candidates);
        o[1] = make_uint4(min(candidates, a.top), 0u, 0u, 0u);
#pragma unroll
        for (uint32_t r = 0; r < kPlaceTop; r += 2u) o[2u + r / 2u] = make_uint4(out_frame[r], out_score[r], out_frame[r + 1u], out_score[r + 1u]);
    }
}

}  // namespace orb
