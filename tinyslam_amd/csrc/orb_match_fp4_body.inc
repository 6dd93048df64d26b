// orb_match_fp4_body.inc -- the body of the block-scaled fp4 matcher, included by k_match_fp4 (orb_kernels_match.h) and by
// k_match_pairs_fp4 (orb_kernels_pairs.h) inside their braces.  The including kernel defines MATCH_FA and MATCH_FB, the frames of the
// queries and of the candidates, and MATCH_ROW, the row of `matches` the records go to -- all uniform for the workgroup -- and has the
// parameters counts, desc4, cap and matches.  Included as text, like orb_front_body.inc: called as an inlined function the same
// body gave k_match_fp4 another schedule and register assignment (DESIGN.md section 27), and the kernel is kept as it was measured.
    __shared__ __attribute__((aligned(16))) uint8_t stage[2][kMatchChunk * kMatch4RowBytes];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t na = min(counts[MATCH_FA], cap), nb = min(counts[MATCH_FB], cap);
    const uint32_t qw = blockIdx.y * (uint32_t)kMatchQueriesPerWg;
    if (qw >= na) return;  // uniform for the workgroup
    const uint32_t q0 = qw + wave * (16u * kMatchRowTiles);
    const bool wave_live = q0 < na;
    const uint32_t rc = lane & 15u, g = lane >> 4;
    const uint8_t* const qa = desc4 + (size_t)MATCH_FA * cap * 128u + 16u * g;
    const uint8_t* const qb = desc4 + (size_t)MATCH_FB * cap * 128u;
    v4i_t a[kMatchRowTiles][2];
#pragma unroll
    for (int m = 0; m < kMatchRowTiles; m++) {
        const uint32_t row = min(q0 + 16u * (uint32_t)m + rc, na - 1u);
#pragma unroll
        for (int t = 0; t < 2; t++) a[m][t] = *reinterpret_cast<const v4i_t*>(qa + (size_t)row * 128u + 64u * (uint32_t)t);
    }
    // The keys are kept as the BIT PATTERNS of the (non-negative) binary32 results, which order like the values: on floats every
    // v_max_f32 / v_med3_f32 is preceded by a canonicalising v_max_f32 x, x, x of the MFMA result (hipcc cannot know it is no
    // signalling NaN) -- 158 v_max_f32 per 64 results instead of 64.
    uint32_t best[kMatchRowTiles][4], second[kMatchRowTiles][4];
#pragma unroll
    for (int m = 0; m < kMatchRowTiles; m++)
#pragma unroll
        for (int i = 0; i < 4; i++) best[m][i] = second[m][i] = 0u;  // +0.0 = nothing: a real key is >= 1.0

    // staging: a chunk is 64 rows x 8 pieces of 16 bytes = 512 pieces, piece p = bytes 16 (p & 7) .. of candidate row p >> 3
    constexpr uint32_t NT = 64u * (uint32_t)kMatchWaves, NP = (uint32_t)(kMatchChunk * 8) / NT;
    static_assert(NP >= 1u && NP <= 8u && NP * NT == (uint32_t)(kMatchChunk * 8), "staging: whole pieces per thread");
    const uint32_t prow = tid >> 3, pcol = 16u * (tid & 7u);
    uint8_t* const put0 = &stage[0][prow * (uint32_t)kMatch4RowBytes + pcol];
    constexpr uint32_t kRowStep = NT / 8u, kPutStep = kRowStep * (uint32_t)kMatch4RowBytes, kBufBytes = (uint32_t)(kMatchChunk * kMatch4RowBytes);
    uint4 p0 = make_uint4(0u, 0u, 0u, 0u), p1 = p0, p2 = p0, p3 = p0, p4 = p0, p5 = p0, p6 = p0, p7 = p0;  // (named registers: an array went through scratch memory)
#define MATCH4_FETCH(J0) \
    do { \
        const uint8_t* const fb_ = qb + pcol; \
        if (NP > 0u) p0 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 0u * kRowStep, nb - 1u) * 128u); \
        if (NP > 1u) p1 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 1u * kRowStep, nb - 1u) * 128u); \
        if (NP > 2u) p2 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 2u * kRowStep, nb - 1u) * 128u); \
        if (NP > 3u) p3 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 3u * kRowStep, nb - 1u) * 128u); \
        if (NP > 4u) p4 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 4u * kRowStep, nb - 1u) * 128u); \
        if (NP > 5u) p5 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 5u * kRowStep, nb - 1u) * 128u); \
        if (NP > 6u) p6 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 6u * kRowStep, nb - 1u) * 128u); \
        if (NP > 7u) p7 = *reinterpret_cast<const uint4*>(fb_ + (size_t)min((J0) + prow + 7u * kRowStep, nb - 1u) * 128u); \
    } while (0)
#define MATCH4_PUT(BUF) \
    do { \
        uint8_t* const pb_ = put0 + (uint32_t)(BUF) * kBufBytes; \
        if (NP > 0u) *reinterpret_cast<uint4*>(pb_ + 0u * kPutStep) = p0; \
        if (NP > 1u) *reinterpret_cast<uint4*>(pb_ + 1u * kPutStep) = p1; \
        if (NP > 2u) *reinterpret_cast<uint4*>(pb_ + 2u * kPutStep) = p2; \
        if (NP > 3u) *reinterpret_cast<uint4*>(pb_ + 3u * kPutStep) = p3; \
        if (NP > 4u) *reinterpret_cast<uint4*>(pb_ + 4u * kPutStep) = p4; \
        if (NP > 5u) *reinterpret_cast<uint4*>(pb_ + 5u * kPutStep) = p5; \
        if (NP > 6u) *reinterpret_cast<uint4*>(pb_ + 6u * kPutStep) = p6; \
        if (NP > 7u) *reinterpret_cast<uint4*>(pb_ + 7u * kPutStep) = p7; \
    } while (0)
    const int scale = 127 + 7;  // E8M0: 2^7 for every block of both operands
    auto tile = [&](auto mask_tag, const uint8_t* src, uint32_t jt) {
        constexpr bool MASK = decltype(mask_tag)::value;
        v8i_t b[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const v4i_t q = *reinterpret_cast<const v4i_t*>(src + 64 * t);
            b[t] = v8i_t{q[0], q[1], q[2], q[3], 0, 0, 0, 0};
        }
        const uint32_t col = jt + rc;
        const float c0 = (float)(256u * kMatch4K + (kMatch4K - 1u) - col);
        const v4f_t cin = {c0, c0, c0, c0};
        v4f_t acc[kMatchRowTiles];
#pragma unroll
        for (int m = 0; m < kMatchRowTiles; m++) acc[m] = cin;
#pragma unroll
        for (int t = 0; t < 2; t++)
#pragma unroll
            for (int m = 0; m < kMatchRowTiles; m++) {
                const v8i_t am = {a[m][t][0], a[m][t][1], a[m][t][2], a[m][t][3], 0, 0, 0, 0};
                acc[m] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(am, b[t], acc[m], 4, 4, 0, scale, 0, scale);
            }
#pragma unroll
        for (int m = 0; m < kMatchRowTiles; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                uint32_t key = __float_as_uint(acc[m][i]);
                if (MASK) key = col < nb ? key : 0u;
                const uint32_t b0 = best[m][i], s0 = second[m][i];
                second[m][i] = max(min(b0, key), min(max(b0, key), s0));  // = med3(b0, s0, key): hipcc emits v_med3_u32
                best[m][i] = max(b0, key);
            }
    };
    if (nb) {
        MATCH4_FETCH(0u);
        MATCH4_PUT(0);
    }
    __syncthreads();
    // The loop over whole chunks has NO branch around the tiles: a wave without queries (wave_live false: its rows repeat the frame's last
    // one, nothing of it is stored) multiplies like the others, and the frame's last, partial chunk is handled behind the loop.  With the
    // partial chunk and `if (wave_live)` inside the loop hipcc kept the 2 x 16 (best, runner-up) registers of the two paths in different
    // places and copied them back every iteration: 32 v_mov per chunk next to its 128 useful vector instructions (6.4 vector instructions
    // per MFMA in the counters where the tile's arithmetic needs 4; 5.3 without them, 0.623 -> 0.59 ms per 255 pairs).
    const uint8_t* const src_base = &stage[0][rc * (uint32_t)kMatch4RowBytes + 16u * g];
    const uint32_t n_whole = nb / (uint32_t)kMatchChunk, n_chunks = (nb + (uint32_t)kMatchChunk - 1u) / (uint32_t)kMatchChunk;
    uint32_t c = 0;
    for (; c < n_whole; c++) {
        const uint32_t j0 = c * (uint32_t)kMatchChunk;
        const bool more = c + 1u < n_chunks;
        if (more) MATCH4_FETCH(j0 + (uint32_t)kMatchChunk);
        const uint8_t* const src0 = src_base + (c & 1u) * kBufBytes;
#pragma unroll
        for (int tt = 0; tt < kMatchChunk / 16; tt++) tile(std::false_type{}, src0 + tt * 16 * kMatch4RowBytes, j0 + 16u * (uint32_t)tt);
        if (more) MATCH4_PUT((c & 1u) ^ 1u);
        __syncthreads();
    }
    if (c < n_chunks) {  // the partial chunk: whole tiles, then one masked tile
        const uint32_t j0 = c * (uint32_t)kMatchChunk;
        const uint8_t* const src0 = src_base + (c & 1u) * kBufBytes;
        for (uint32_t tt = 0; j0 + 16u * tt < nb; tt++) {
            const uint32_t jt = j0 + 16u * tt;
            if (jt + 16u <= nb)
                tile(std::false_type{}, src0 + tt * (uint32_t)(16 * kMatch4RowBytes), jt);
            else
                tile(std::true_type{}, src0 + tt * (uint32_t)(16 * kMatch4RowBytes), jt);
        }
    }
#undef MATCH4_FETCH
#undef MATCH4_PUT
    if (!wave_live) return;
#pragma unroll
    for (int m = 0; m < kMatchRowTiles; m++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t b1 = best[m][i], s1 = second[m][i];
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) {
                const uint32_t b2 = (uint32_t)__shfl_xor((int)b1, sh), s2 = (uint32_t)__shfl_xor((int)s1, sh);
                s1 = max(min(b1, b2), max(s1, s2));
                b1 = max(b1, b2);
            }
            const uint32_t q = q0 + 16u * (uint32_t)m + 4u * g + (uint32_t)i;
            if (rc == 0u && q < na) {
                MatchRecord r;
                const uint32_t k1 = (uint32_t)__uint_as_float(b1), k2 = (uint32_t)__uint_as_float(s1);  // exact: integers below 2^24
                const uint32_t v1 = k1 >> 14, v2 = k2 >> 14;           // 512 - 2 * distance
                r.index = k1 ? kMatch4K - 1u - (k1 & (kMatch4K - 1u)) : 0xffffffffu;
                const uint32_t d1 = k1 ? (512u - v1) >> 1 : 0xffffu;
                const uint32_t d2 = k2 ? (512u - v2) >> 1 : 0xffffu;
                r.dist = d1 | (d2 << 16);
                matches[(size_t)MATCH_ROW * cap + q] = r;
            }
        }
