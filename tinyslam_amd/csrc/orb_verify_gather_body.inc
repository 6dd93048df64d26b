// orb_verify_gather_body.inc -- the body of the verifiers' gather (GV-1, GV-2), included by k_verify_gather (orb_kernels_verify.h) and by
// k_verify_gather_pairs (orb_kernels_pairs.h) inside their braces.  The including kernel defines GATHER_FQ and GATHER_FT, the frames of
// the queries and of their matches' targets, and GATHER_ROW, the row of a.matches, a.rec, a.cand_of and a.n_cand -- all uniform for
// the workgroup -- and has the parameter VerifyArgs a.  Included as text for the reason orb_match_fp4_body.inc gives.
    __shared__ uint32_t wave_n[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nq = min(a.counts[GATHER_FQ], a.cap), nt = min(a.counts[GATHER_FT], a.cap);
    const CornerData* const cq = a.corners + (size_t)GATHER_FQ * a.cap;
    const CornerData* const ct = a.corners + (size_t)GATHER_FT * a.cap;
    const MatchRecord* const mr = a.matches + (size_t)GATHER_ROW * a.cap;
    float4* const rec = a.rec + (size_t)GATHER_ROW * a.cap;
    uint32_t* const cand_of = a.cand_of + (size_t)GATHER_ROW * a.cap;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < nq; i0 += 256u) {
        const uint32_t i = i0 + tid;
        bool keep = false;
        uint32_t t = 0;
        if (i < nq) {  // GV-1
            const MatchRecord m = mr[i];
            const uint32_t d = m.dist & 0xffffu, second = m.dist >> 16;
            t = m.index;
            keep = t != kVerifyNone && t < nt && d <= a.max_distance && (float)d < a.ratio * (float)second;
        }
        const unsigned long long bal = __ballot(keep);
        const uint32_t before = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0u) wave_n[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t off = base;
        for (uint32_t w = 0; w < wave; w++) off += wave_n[w];
        const uint32_t total = (wave_n[0] + wave_n[1]) + (wave_n[2] + wave_n[3]);
        if (i < nq) cand_of[i] = keep ? off + before : kVerifyNone;
        if (keep) {  // GV-2: level-0 pixel centres (orb_corner_level0_xy), then normalised
            const CornerData q = cq[i], r = ct[t];
            const float sq = (float)(1u << (q.octave & 31u)), sr = (float)(1u << (r.octave & 31u));
            const float xq = ((float)q.x + 0.5f) * sq - 0.5f, yq = ((float)q.y + 0.5f) * sq - 0.5f;
            const float xr = ((float)r.x + 0.5f) * sr - 0.5f, yr = ((float)r.y + 0.5f) * sr - 0.5f;
            rec[off + before] = make_float4((xq - a.cx) * a.k, (yq - a.cy) * a.k, (xr - a.cx) * a.k, (yr - a.cy) * a.k);
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0u) a.n_cand[GATHER_ROW] = base;
