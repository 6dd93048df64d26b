// orb_brief_nf_keypoint.inc -- one keypoint that is not flat, described by a whole wave: the body of the keypoint loops of
// brief_nf_body (the scanning form) and brief_nf_mask_body (orb_kernels_brief.h), included as text so that both run the same
// lines.  In scope: r (the record, wave-uniform), idx (the keypoint's place in the chunk), lvl, w, h, qa, rowc, plane (its level),
// lane, patch (the wave's LDS patch), out_desc, host_descriptors, k0, bg, tab and the template flag OOB.
        // this lane's eight rotated points (brief.wgsl:50-57), from the table of the keypoint's angle code: issued here, used
        // behind the patch fill
        const uint4 tt = tab.rot[(size_t)min(r.z, (uint32_t)(ORB_ANGLE_STEPS - 1)) * 64u + lane];
        const uint32_t tw[4] = {tt.x, tt.y, tt.z, tt.w};
        uint64_t bal[4];
        if ((w & 1) == 0) {
            // ---- patch in LDS: rows y-18..y+18, columns c0..c0+47 with c0 = (x - 18) rounded down to 8.  A piece
            //      (8 columns) lies entirely left of the level (zeros), below qa (the row constant) or in the stored
            //      tail (one 16-byte load); the four pieces of a lane are loaded back to back from addresses that are
            //      always valid (the plane's first texels where none is needed) and composed afterwards.
            const int c0 = ((int)r.x - kBriefHalo) & ~7;
            constexpr int kPiecesPerRow = kNfPatchCols / 8, kPieces = kNfPatchRows * kPiecesPerRow;
            constexpr int kRounds = (kPieces + 63) / 64;
            uint4 tv[kRounds];
            uint32_t rcv[kRounds];
            int kind[kRounds], where[kRounds];  // 0: zeros, 1: row constant, 2: loaded, 3: the level ends inside the piece
#pragma unroll
            for (int rr = 0; rr < kRounds; rr++) {
                const int p = (int)lane + 64 * rr;
                const int pr = (int)(((float)p + 0.5f) * (1.0f / (float)kPiecesPerRow));
                const int pc = p - pr * kPiecesPerRow;
                const int gy0 = (int)r.y - kBriefHalo + pr, cx = c0 + 8 * pc;
                const int gy = OOB ? oob_index(gy0, h, bg.oob) : gy0;  // OOB: a row outside the level reads a row of the level
                const bool in = p < kPieces && gy >= 0 && gy < h && cx >= 0 && cx < w;
                kind[rr] = !in ? 0 : (cx < qa ? 1 : (cx + 8 <= w ? 2 : 3));
                where[rr] = p < kPieces ? pr * kNfPatchCols + 8 * pc : -1;
                rcv[rr] = rowc[min(max(gy, 0), h - 1)];
                if (OOB && p < kPieces && !(cx >= 0 && cx < w)) {
                    // the whole piece lies left (cx <= -8) or right (cx >= w) of the level: one texel of row gy repeated -- its first
                    // (clamp, left) or its last one (right; umin: left as well); a column below qa is the row constant
                    const int xm = oob_index(cx, w, bg.oob);
                    if (xm >= qa) rcv[rr] = plane[(size_t)(uint32_t)(__mul24(gy, w) + xm)];
                    kind[rr] = 1;
                }
                // 4-byte aligned: even width, cx a multiple of 8
                tv[rr] = *reinterpret_cast<const uint4*>(plane + (kind[rr] == 2 ? (size_t)(uint32_t)(__mul24(gy, w) + cx) : (size_t)0));
            }
#pragma unroll
            for (int rr = 0; rr < kRounds; rr++) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (kind[rr] == 1) {
                    const uint32_t c2 = rcv[rr] | (rcv[rr] << 16);
                    v = make_uint4(c2, c2, c2, c2);
                } else if (kind[rr] == 2) {
                    v = tv[rr];
                } else if (kind[rr] == 3) {  // width not a multiple of 8: the last piece of a row, texel by texel
                    const int p = (int)lane + 64 * rr;
                    const int pr = (int)(((float)p + 0.5f) * (1.0f / (float)kPiecesPerRow));
                    const int gy0 = (int)r.y - kBriefHalo + pr, cx = c0 + 8 * (p - pr * kPiecesPerRow);
                    const int gy = OOB ? oob_index(gy0, h, bg.oob) : gy0;
                    const uint16_t* src = plane + (size_t)(uint32_t)(__mul24(gy, w) + cx);
                    uint32_t t[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) t[q] = cx + q < w ? (uint32_t)src[q] : (OOB ? (uint32_t)src[w - 1 - cx] : 0u);  // OOB: the row's last texel (cx >= qa here)
                    v = make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
                }
                if (where[rr] >= 0) *reinterpret_cast<uint4*>(&patch[where[rr]]) = v;
            }
            // the patch is filled with 16-byte stores and sampled as halfs by OTHER lanes of this wave: order the two
            // (LDS is in order within a wave; the fence keeps the compiler from moving the differently typed accesses)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int xo = (int)r.x - c0;  // 18..25
            const uint8_t* const centre = reinterpret_cast<const uint8_t*>(patch + kBriefHalo * kNfPatchCols + xo);  // the keypoint's texel
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const uint32_t va = *reinterpret_cast<const uint16_t*>(centre + rot_a(tw[e]));
                const uint32_t vb = *reinterpret_cast<const uint16_t*>(centre + rot_b(tw[e]));
                bal[e] = __ballot(va > vb);  // non-negative f16: bit patterns order like the values (brief.wgsl:62)
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the next keypoint's fill overwrites what was just sampled
            __builtin_amdgcn_wave_barrier();
        } else {
            // ---- odd width: rows of the plane are only 2-byte aligned; gather sample by sample
            const int gy = (int)r.y - kBriefHalo + (int)lane;  // lanes 0..36 are the patch rows
            const uint32_t rowv = (gy >= 0 && gy < h && lane < 37u) ? (uint32_t)rowc[gy] : 0u;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                // the table holds 2 * (dy * kNfPatchCols + dx) with |dx| < kNfPatchCols / 2: take it apart again
                const int oa = rot_a(tw[e]) >> 1, ob = rot_b(tw[e]) >> 1;
                const int dya = (oa + kNfPatchCols / 2 + 64 * kNfPatchCols) / kNfPatchCols - 64, dxa = oa - dya * kNfPatchCols;
                const int dyb = (ob + kNfPatchCols / 2 + 64 * kNfPatchCols) / kNfPatchCols - 64, dxb = ob - dyb * kNfPatchCols;
                const int xa = (int)r.x + dxa, ya = (int)r.y + dya;
                const int xb = (int)r.x + dxb, yb = (int)r.y + dyb;
                uint32_t va = (uint32_t)__shfl((int)rowv, dya + kBriefHalo);  // 0 when the row is outside the level
                uint32_t vb = (uint32_t)__shfl((int)rowv, dyb + kBriefHalo);
                const bool ina = xa >= 0 && xa < w && ya >= 0 && ya < h;
                const bool inb = xb >= 0 && xb < w && yb >= 0 && yb < h;
                if (!ina)
                    va = OOB ? blur_sample_mapped(plane, rowc, w, h, qa, xa, ya, bg.oob) : 0u;
                else if (xa >= qa)
                    va = plane[(size_t)(uint32_t)(__mul24(ya, w) + xa)];
                if (!inb)
                    vb = OOB ? blur_sample_mapped(plane, rowc, w, h, qa, xb, yb, bg.oob) : 0u;
                else if (xb >= qa)
                    vb = plane[(size_t)(uint32_t)(__mul24(yb, w) + xb)];
                bal[e] = __ballot(va > vb);
            }
        }
        if (lane < 8u) {
            const uint64_t src = lane < 2u ? bal[0] : (lane < 4u ? bal[1] : (lane < 6u ? bal[2] : bal[3]));
            out_desc[(size_t)idx * 8u + lane] = (uint32_t)(src >> ((lane & 1u) * 32u));
            if (host_descriptors) store_host_u32(reinterpret_cast<uint32_t*>(host_descriptors + k0) + (size_t)idx * 8u + lane, (uint32_t)(src >> ((lane & 1u) * 32u)));
        }
