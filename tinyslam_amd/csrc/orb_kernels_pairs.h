// orb_kernels_pairs.h -- the matcher and the verifiers' gather over caller-listed frame pairs (not in the reference; the definition
// is the build's own, MP-1..MP-5 in DESIGN.md section 27).  orb_match_consecutive and the two verifiers work on the pairs
// (f, f + 1); a loop candidate of orb_place_frames is a pair of frames far apart.  Here the pair of a workgroup comes from a list
// in device memory -- entry i = (query frame, target frame), validated on the host: both below the batch's frame count -- and
// everything the workgroup writes goes to row i.
//
//   k_match_pairs_fp4      grid (n_pairs, ceil(cap / 256)), block 64 * kMatchWaves: the block-scaled fp4 MFMA matcher, k_match_fp4's body
//                          (orb_match_fp4_body.inc) on the descriptors orb_match_pairs expanded into its own buffer
//   k_match_pairs          grid (n_pairs, ceil(cap / (64 * kMatchQ))), block 64: the vector-unit matcher, k_match's body
//                          (orb_match_valu_body.inc)
//   k_verify_gather_pairs  grid (n_pairs), block 256: k_verify_gather's body (orb_verify_gather_body.inc), and the query frame's raw
//                          counter into qcount[i] -- the score and refine kernels of both verifiers index everything by blockIdx.x,
//                          the counters included (the refine kernel's inlier bytes), so they run on a list unchanged with qcount
//                          as their counts
//
// One source per body: the consecutive kernels include the same text with (pair, pair + 1, pair), and their machine code is what it
// was before this header existed (tools/isa_compare.py).
#pragma once
#include "orb_kernels_match.h"
#include "orb_kernels_verify.h"

namespace orb {

static_assert(sizeof(OrbFramePair) == 8, "OrbFramePair layout");

__global__ __launch_bounds__(64 * kMatchWaves, TINYORB_MATCH_MINWAVES) void k_match_pairs_fp4(const OrbFramePair* __restrict__ list,
                                                                                                const uint32_t* __restrict__ counts,
                                                                                                const uint8_t* __restrict__ desc4, uint32_t cap,
                                                                                                MatchRecord* __restrict__ matches) {
    const uint32_t item = blockIdx.x, fq = list[item].query, ft = list[item].target;
#define MATCH_FA fq
#define MATCH_FB ft
#define MATCH_ROW item
#include "orb_match_fp4_body.inc"
#undef MATCH_FA
#undef MATCH_FB
#undef MATCH_ROW
}

__global__ __launch_bounds__(64) void k_match_pairs(const OrbFramePair* __restrict__ list, const uint32_t* __restrict__ counts,
                                                    const CornerDescriptor* __restrict__ descriptors, uint32_t cap,
                                                    MatchRecord* __restrict__ matches) {
    const uint32_t item = blockIdx.x, fq = list[item].query, ft = list[item].target;
#define MATCH_FA fq
#define MATCH_FB ft
#define MATCH_ROW item
#include "orb_match_valu_body.inc"
#undef MATCH_FA
#undef MATCH_FB
#undef MATCH_ROW
}

// a.matches: the rows of orb_match_pairs; a.counts: the batch's raw counters
__global__ __launch_bounds__(256) void k_verify_gather_pairs(VerifyArgs a, const OrbFramePair* __restrict__ list, uint32_t* __restrict__ qcount) {
    const uint32_t item = blockIdx.x, fq = list[item].query, ft = list[item].target;
    if (threadIdx.x == 0u) qcount[item] = a.counts[fq];
#define GATHER_FQ fq
#define GATHER_FT ft
#define GATHER_ROW item
#include "orb_verify_gather_body.inc"
#undef GATHER_FQ
#undef GATHER_FT
#undef GATHER_ROW
}

}  // namespace orb
