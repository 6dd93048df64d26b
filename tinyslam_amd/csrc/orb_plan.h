// orb_plan.h -- what orb_program_create decides before it allocates: which pipeline a program takes and the geometry of each.
//
// Host arithmetic only: nothing here calls the HIP runtime, so the whole decision runs without a device (tests/plan_dump.cpp prints it,
// tests/test_plan.py pins it).  In: the configuration, the options, the device's LDS limit and the create-time switches (PlanEnv, the
// one place that reads them).  Out: a ProgramPlan, which orb_api.hip writes once into OrbProgram::plan and only reads afterwards.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/tinyorb.h"
#include "orb_front_launch.h"
#include "orb_kernels_fused.h"
#include "orb_kernels_brief.h"
#include "orb_kernels_intended.h"
#include "orb_kernels_staged.h"

namespace orb {

// Environment switches (experiments and cross-checks), read once when the program is created and nowhere on a per-call path.  The
// stages' own switches (TINYORB_MATCH_VALU, _MATCH_I8, _GUIDE_CELL, _TRACK_GLOBAL_KEYS) are read at a stage's first call instead.
struct PlanEnv {
    bool single_memcpy = false, single_split = false, single_serial = false, single_sync = false, single_block = false;
    bool no_swizzle = false, quiet = false;
    bool front_generic = false, front_trace = false;  // TINYORB_FRONT_GENERIC: no instance of k_front with a compile-time geometry; TINYORB_FRONT_TRACE: say which
    int phase_mask = -1, brief_i_mask = -1, lds_pad = 0;
    uint32_t band_rows = 0;         // TINYORB_BAND_ROWS (experiments): one band height for every level that can have it; 0: not forced
    bool tile_w_set = false;        // TINYORB_TILE_W, present at all: column tiles at every level ...
    uint32_t tile_w = 0;            // ... of about max(64, value) columns
    bool ln_512 = false;            // TINYORB_LN_512: the levels >= 1 stay on kFrontThreadsLN threads
    bool no_latency_bands = false;  // TINYORB_NO_LATENCY_BANDS: a program of one frame keeps the throughput bands
    bool i_gauss_kernel = false;    // TINYORB_I_GAUSS_KERNEL: fused_i blurs with k_gauss over the stored grey plane
    bool stamps = false;            // TINYORB_STAMPS: diagnostic builds only (tools/stamps.py)
    bool brief_rows = false;        // TINYORB_BRIEF_ROWS: A/B and cross-check, the wave-per-keypoint kernel instead of k_brief_t
};

inline PlanEnv read_plan_env(uint32_t flags) {
    const auto on = [](const char* name) { const char* e = getenv(name); return e && *e && atoi(e) != 0; };
    const auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e && *e ? atoi(e) : dflt; };
    const auto set = [](const char* name) { return getenv(name) != nullptr; };
    PlanEnv env;
    env.single_memcpy = on("TINYORB_SINGLE_MEMCPY");
    env.single_split = on("TINYORB_SINGLE_SPLIT");
    env.single_serial = on("TINYORB_SINGLE_SERIAL");
    env.single_sync = on("TINYORB_SINGLE_SYNC");
    {   // how orb_extract_corners waits: "poll" (default) spins on the completion word; "block" spins for kSingleSpinUs, then sleeps
        // in hipEventSynchronize on a blocking-sync event (an interrupt instead of a spin -- the reference blocks in device.poll(Wait),
        // orb.rs:547); ORB_FLAG_SINGLE_BLOCKING_WAIT asks for the same from code
        const char* w = getenv("TINYORB_SINGLE_WAIT");
        env.single_block = (w && !strcmp(w, "block")) || (flags & ORB_FLAG_SINGLE_BLOCKING_WAIT) != 0u;
    }
    env.no_swizzle = on("TINYORB_NO_SWIZZLE");
    env.quiet = set("TINYORB_QUIET");
    env.front_generic = on("TINYORB_FRONT_GENERIC");
    env.front_trace = on("TINYORB_FRONT_TRACE");
    env.phase_mask = num("TINYORB_PHASE_MASK", -1);
    env.brief_i_mask = num("TINYORB_BRIEF_I_MASK", -1);
    env.lds_pad = num("TINYORB_LDS_PAD", 0);
    if (const char* e = getenv("TINYORB_BAND_ROWS")) env.band_rows = (uint32_t)atoi(e);
    if (const char* e = getenv("TINYORB_TILE_W")) env.tile_w_set = true, env.tile_w = std::max(64u, (uint32_t)atoi(e));
    env.ln_512 = set("TINYORB_LN_512");
    env.no_latency_bands = set("TINYORB_NO_LATENCY_BANDS");
    env.i_gauss_kernel = set("TINYORB_I_GAUSS_KERNEL");
    env.stamps = set("TINYORB_STAMPS");
    env.brief_rows = set("TINYORB_BRIEF_ROWS");
    return env;
}

// The argument checks of orb_program_create: the message of the first one that fails, or null.  (options may be null: the defaults.)
inline const char* check_config(const OrbConfig* config, const OrbOptions* options) {
    if (!config) return "config is NULL";
    const uint32_t W = config->image_size.width, H = config->image_size.height;
    if (W == 0 || H == 0 || config->image_size.depth_or_array_layers != 1) return "image_size must be WxHx1 with W,H > 0";
    if ((uint64_t)W * H > (1ull << 28)) return "image too large";
    if (config->hierarchy_depth < 1 || config->hierarchy_depth > ORB_MAX_HIERARCHY_DEPTH) return "hierarchy_depth must be 1..=10 (orb.rs:66-67)";
    if (config->max_features == 0 || config->max_features > (1u << 24)) return "max_features must be 1..=2^24";
    if (!(config->initial_threshold >= 0.f)) return "initial_threshold must be >= 0";
    if (!options) return nullptr;
    const bool extended = (options->flags & (ORB_FLAG_INTENDED | ORB_FLAG_NMS)) || (options->fast_arc != 0 && options->fast_arc != 12);
    if (options->fast_arc != 0 && (options->fast_arc < 9 || options->fast_arc > 16)) return "fast_arc must be 0 (= 12) or 9..16";
    if ((options->flags & ORB_FLAG_INPUT_Y8) && extended)
        return "ORB_FLAG_INPUT_Y8 is defined for the reference's detector only (no "
               "ORB_FLAG_INTENDED, ORB_FLAG_NMS or fast_arc other than 12)";
    if (options->oob_policy > ORB_OOB_UMIN || options->sampler_weight_bits > 23u)
        return "oob_policy must be ORB_OOB_ZERO / _CLAMP / _UMIN and sampler_weight_bits 0..23";
    if ((options->oob_policy != ORB_OOB_ZERO || options->sampler_weight_bits != 0u) && extended)
        return "oob_policy / sampler_weight_bits follow the reference's adapter: they are defined for the "
               "reference's detector only (no ORB_FLAG_INTENDED, ORB_FLAG_NMS or fast_arc other than 12)";
    if (options->fp_contract > (ORB_FP_CONTRACT_ALL | ORB_FP_LAST_TERM_FIRST))
        return "fp_contract is a mask of ORB_FP_CONTRACT_LUMINANCE / _BLUR / _ROTATION and ORB_FP_LAST_TERM_FIRST";
    if (options->fp_contract && (extended || (options->flags & ORB_FLAG_INPUT_Y8)))
        return "fp_contract follows the reference's shader compiler: it is defined for the reference's detector on RGBA "
               "input only (no ORB_FLAG_INTENDED, ORB_FLAG_NMS, ORB_FLAG_INPUT_Y8 or fast_arc other than 12)";
    if (options->angle_bins && (!(options->flags & ORB_FLAG_INTENDED) || options->angle_bins < 8u || options->angle_bins > 6284u))
        return "angle_bins is an option of ORB_FLAG_INTENDED (IM-6b): 0, or 8..6284 bins of the full circle";
    if ((options->flags & ORB_FLAG_INTENDED) && (W > 16384u || H > 16384u))
        return "ORB_FLAG_INTENDED needs W, H <= 16384 (14-bit coordinates in the top-K key)";
    return nullptr;
}

struct ProgramPlan {
    uint32_t max_batch = 1;
    uint32_t arc = 12;        // FAST arc length (opt-in extension, 9..16)
    uint32_t oob = kOobZero;  // OrbOptions::oob_policy
    float wq = 0.0f;          // OrbOptions::sampler_weight_bits as 2^bits (0: exact weights)
    bool intended = false;    // "intended" mode: survivors of the NMS with their scores, input of the top-K cut
    bool input_y8 = false;    // ORB_FLAG_INPUT_Y8: frames are one byte per pixel
    size_t frame_bytes = 0;
    Pyramid pyr{};
    bool fused = false;    // the plain fused pipeline: one k_front launch per level + BRIEF
    bool fused_i = false;  // fused "intended" pipeline (orb_kernels_intended.h): tile slots, their segments (record + score), the cut
    bool fused_x = false;  // the reference's algorithm with the opt-in arc / NMS on the tile kernels
    uint32_t band_rows_lvl[kMaxLevels] = {0};  // band height of the plain fused path per level: one of kFrontBandHeights
    uint32_t ln_threads[kMaxLevels] = {0};     // levels >= 1: threads of a band's workgroup, kFrontThreadsLN or kFrontThreadsLNBig
    uint32_t tile_w_lvl[kMaxLevels] = {0};     // 0: full-width bands; else the level runs on column tiles of this width (k_front<..., TILED>)
    BandGeom bands{};
    RowsGeom rows{};
    RowsGeom xrows{};          // fused_x: the tile slots as launch_brief sees them
    uint32_t xband_slots = 0;  // fused_x: 16-row bands per frame over all levels (grid of the blur-only launches)
    IBriefGeom itiles{};       // fused_i and fused_x
    BriefTGeom brieft{};       // thread-per-keypoint BRIEF of the fused literal pipelines (plain and arc/NMS)
    bool use_brief_t = false;
    uint32_t seg_classes = 1;  // lists per band slot of the plain fused path: 2 with k_brief_t (angle code 0 / the rest)
    uint32_t blur_qa[kMaxLevels] = {0};  // fused paths: per level, columns [0, qa) of the blur plane live in d_blur_rowc
    bool igauss_fused = false;  // fused_i: k_front_i blurs its own tile (phase G); false: k_gauss over the stored grey plane (TINYORB_I_GAUSS_KERNEL=1)
    bool igrey_stored = false;  // fused_i: k_front_i<true> stores the level-0 grey plane (k_gauss or k_mip reads it)
    uint32_t ibrief_lds = 0;    // fused_i: dynamic LDS of k_brief_i
    // opt-in NMS / "intended" on the staged kernels: score planes and the capacity of the provisional list
    ScoreLayout score_layout{};
    uint32_t cap_prov = 0;
    std::string pipeline_note;  // why the staged kernels were chosen when nobody asked for them (else empty)
};

inline void layout_pyramid(uint32_t W, uint32_t H, uint32_t depth, Pyramid* pyr) {
    memset(pyr, 0, sizeof *pyr);
    pyr->depth = depth;
    uint32_t off = 0;
    for (uint32_t m = 0; m < depth; m++) {
        uint32_t w = W >> m, h = H >> m;  // wgpu mip chain: max(1, dim >> m)
        pyr->w[m] = w ? w : 1u;
        pyr->h[m] = h ? h : 1u;
        pyr->off[m] = off;
        off += pyr->w[m] * pyr->h[m];
        off = (off + 7u) & ~7u;  // keep every level 16-byte aligned
    }
    pyr->stride = (off + 63u) & ~63u;
    uint32_t rows = 0;
    for (uint32_t m = 0; m < depth; m++) {
        pyr->row_off[m] = rows;
        rows += pyr->h[m];
    }
    pyr->row_stride = (rows + 7u) & ~7u;
}

// Dispatch grid of octave `lvl` in the reference (orb.rs:501-519: halved and 8-rounded per octave).
inline void reference_grid(const Pyramid& pyr, uint32_t lvl, uint32_t* gw, uint32_t* gh) {
    uint32_t width = pyr.w[0], height = pyr.h[0];
    for (uint32_t m = 0; m < lvl; m++) {
        width /= 2u;
        height /= 2u;
    }
    *gw = ((width + 7u) / 8u) * 8u;
    *gh = ((height + 7u) / 8u) * 8u;
}

// Can the fused per-level kernels handle this configuration?  (Otherwise: staged pipeline.)
inline bool fused_eligible(const ProgramPlan& pl, uint32_t flags) {
    if (flags & (ORB_FLAG_STAGED | ORB_FLAG_NMS | ORB_FLAG_INTENDED)) return false;
    if (pl.arc != 12u) return false;  // the fused FAST phase is specialised for the reference's 12-run
    const Pyramid& pyr = pl.pyr;
    // index arithmetic: v_mul_i32_i24 takes 24-bit operands (rows, widths < 2^14 here) and returns 32 bits; RGBA byte
    // offsets inside a frame are 4 * W * H < 2^32
    if ((uint64_t)pyr.w[0] * pyr.h[0] > (1ull << 26) || pyr.h[0] > 16384u) return false;
    if (pyr.w[0] > (uint32_t)kFrontMaxWidthTiled || pyr.w[0] < 8u) return false;
    // rows of any width: k_front<..., UA> loads RGBA texel by texel (4-byte aligned) and Y8 byte by byte
    return true;  // a level 1 that is not an exact half is built by k_mip from the stored level-0 plane (FrontGeom::store_grey)
}

inline bool fused_i_eligible(const ProgramPlan& pl, uint32_t flags) {
    if (!pl.intended || (flags & ORB_FLAG_STAGED)) return false;
    const Pyramid& pyr = pl.pyr;
    if ((uint64_t)pyr.w[0] * pyr.h[0] > (1ull << 26)) return false;  // 32-bit byte offsets; W, H <= 16384 (check_config)
    if ((pyr.w[0] & 3u) != 0u || pyr.w[0] < 8u) return false;       // level 0 is read as RGBA quads
    return true;
}

inline bool fused_x_eligible(const ProgramPlan& pl, uint32_t flags) {
    if (pl.intended || pl.input_y8 || (flags & ORB_FLAG_STAGED)) return false;  // the tile kernel reads RGBA
    if (pl.arc == 12u && !(flags & ORB_FLAG_NMS)) return false;  // that is the plain fused pipeline
    const Pyramid& pyr = pl.pyr;
    if ((uint64_t)pyr.w[0] * pyr.h[0] > (1ull << 26) || pyr.h[0] > 16384u) return false;
    if ((pyr.w[0] & 3u) != 0u || pyr.w[0] > (uint32_t)kFrontMaxWidth || pyr.w[0] < 8u) return false;
    if (pyr.depth > 1 && !(pyr.w[0] == 2u * pyr.w[1] && pyr.h[0] == 2u * pyr.h[1])) return false;
    return true;
}

inline uint32_t front_bands(const Pyramid& pyr, uint32_t lvl, uint32_t band_rows) {
    const uint32_t gh = (((pyr.h[0] >> lvl) + 7u) / 8u) * 8u;  // orb.rs:513, 518
    const uint32_t rows = pyr.h[lvl] > gh ? pyr.h[lvl] : gh;
    return (rows + band_rows - 1) / band_rows;
}

// tile_w = 0: full-width bands; else column tiles of that width (rounded up to 8; FrontGeom::tiled)
inline FrontGeom front_geometry(const Pyramid& pyr, uint32_t lvl, uint32_t gw, uint32_t gh, uint32_t n_frames, uint32_t band_rows = kFrontRows,
                                uint32_t tile_w = 0, uint32_t threads = 0) {
    FrontGeom g{};
    g.lvl = lvl;
    g.rows = band_rows;
    g.gw = gw;
    g.gh = gh;
    const uint32_t w = pyr.w[lvl], h = pyr.h[lvl];
    const uint32_t rows = h > gh ? h : gh;
    g.n_bands = (rows + band_rows - 1) / band_rows;
    g.n_frames = n_frames;
    const uint32_t cols = (w > gw ? w : gw) + 4u;
    g.ls = kLdsPad + ((cols + 7u) & ~7u);
    g.ts = (w + 7u) & ~7u;
    g.write_mip = (lvl + 1 < pyr.depth && w == 2u * pyr.w[lvl + 1] && h == 2u * pyr.h[lvl + 1]) ? 1u : 0u;
    g.xcd_swizzle = (n_frames % 8u == 0u) ? 1u : 0u;
    {   // constant stretches of the literal blur (tap 1 is monotone in x): see k_front phase C
        uint32_t P = 0;
        while (P < w && blur_tap(P, w, kBlurOffHost).i1 == 0) P++;
        uint32_t Q = 0;
        if (P > 0) while (Q < w && (uint32_t)blur_tap(Q, w, kBlurOffHost).i1 < P) Q++;
        g.blur_p = P;
        g.blur_q = Q;
        g.n_var = w - Q;
    }
    if (tile_w) {
        const uint32_t dom = ((w > gw ? w : gw) + 7u) & ~7u;  // columns of the level / of its dispatch domain
        g.tiled = 1u;
        g.tw = std::min((tile_w + 7u) & ~7u, dom);
        g.n_ct = (dom + g.tw - 1u) / g.tw;
        g.xb = 3u;
        while ((1u << g.xb) < g.tw) g.xb++;
        g.ls = kLdsPad + ((g.tw + 4u + 7u) & ~7u);
        g.ts = std::min(g.tw, (w + 7u) & ~7u);
        const BlurTap t = blur_tap(w - 1u, w, kBlurOffHost);
        g.far_i0 = (uint32_t)t.i0;
        g.far_i1 = (uint32_t)t.i1;
        // queues B (3 ts entries) and C (ts), or the blur column table (24 bytes per column that varies), whichever is larger
        g.tmp_halfs = std::max<uint32_t>(2u * kFrontTmpRows * g.ts, (uint32_t)(sizeof(BlurCol) / 2u) * g.n_var);
        g.tmp_halfs = (g.tmp_halfs + 7u) & ~7u;
    }
    {   // pre-test items of a band (tile): rows x ceil(dispatch columns / 16) at level 0 and on 1024 threads, / 8 otherwise (orb_front_body.inc, B1)
        const uint32_t cols_t = g.tiled ? std::min(g.tw, gw) : gw, iw = (lvl == 0 || threads == (uint32_t)kFrontThreadsLNBig) ? 16u : 8u;
        g.ovf_words = (band_rows * ((cols_t + iw - 1u) / iw) + 31u) / 32u;
    }
    g.n_classes = 1u;
    g.phase_mask = 15u;  // plan_level_geometry applies the program's experiment switches (TINYORB_PHASE_MASK, TINYORB_NO_SWIZZLE)
    return g;
}

// Can tile 0 of a tiled level do the band's blur from its own columns?  The column table's grey texels lie in [0, ~0.12 w].
inline bool front_tile0_holds_blur(const FrontGeom& g, uint32_t w) {
    if (!g.tiled || g.n_ct == 1u) return true;
    uint32_t hi = 0;
    for (uint32_t x = g.blur_q; x < w; x++) {
        const BlurTap t2 = blur_tap(x, w, kBlurOffHost);
        for (int j : {t2.i0, t2.i1})
            if ((uint32_t)j >= g.blur_p) hi = std::max<uint32_t>(hi, (uint32_t)blur_tap((uint32_t)j, w, kBlurOffHost).i1);
    }
    return hi + 1u <= g.tw;
}

// Geometry of k_brief_t over the band (or tile) slots described by `rg`; false when the frame is too large for its LDS
// staging (then k_brief_rows does the work).
inline bool brieft_geometry(const Pyramid& pyr, uint32_t oob, const PlanEnv& env, const RowsGeom& rg, uint32_t n_classes, BriefTGeom* out) {
    BriefTGeom g{};
    g.n_slots = rg.n_slots;
    g.seg_cap = rg.seg_cap;
    g.n_classes = n_classes;
    uint32_t rows = 0;
    for (uint32_t m = 0; m < pyr.depth; m++) {
        g.flat_end[m] = rg.flat_end[m];
        g.qa[m] = rg.qa[m];
        // 18 zero rows in front of a level and 26 behind it: the patch reaches 18 rows past the keypoint, and at
        // octaves >= 1 a keypoint may sit up to 7 rows below the level's last row (8-rounded dispatch, Q8)
        g.row_base[m] = rows + (uint32_t)kBriefHalo;
        rows += pyr.h[m] + 2u * (uint32_t)kBriefHalo + 8u;
    }
    g.rows_padded = rows;
    g.oob = oob;
    *out = g;
    if (env.brief_rows) return false;
    return rg.n_slots >= 1u && rg.n_slots * n_classes <= kBriefTMaxSlots && rows <= kBriefTMaxRows;
}

// Tile width of a level for the fused "intended" pipeline.
inline uint32_t itile_width(uint32_t w) {
    const uint32_t w8 = (w + 7u) & ~7u;
    return w8 < (uint32_t)kITileW ? w8 : (uint32_t)kITileW;
}

// What the band picker gives one level: band height (0: nothing fits), the LDS a band then needs, the threads of its workgroup
// (levels >= 1), and the width of its column tiles (0: full-width bands).
struct BandPick {
    uint32_t rows = 0, lds = 0, threads = (uint32_t)kFrontThreadsLN, tile_w = 0;
};

// Full-width bands of level lvl on `threads` threads, from kFrontBandHeights (tallest first): the tallest of which two fit a CU's
// LDS, the tallest that fits at all, and the forced height if it fits (0: none such).
struct BandFit {
    uint32_t twice = 0, twice_lds = 0, once = 0, once_lds = 0, want = 0, want_lds = 0;
};
inline BandFit fit_bands(const Pyramid& pyr, uint32_t lvl, uint32_t gw, uint32_t gh, uint32_t threads, uint32_t forced, uint32_t max_lds) {
    BandFit f;
    const uint32_t w = pyr.w[lvl];
    for (int cand : kFrontBandHeights) {
        if (std::max(w, gw) > (1u << front_x_bits(cand)) || std::max(w, gw) > (uint32_t)kFrontMaxWidthWide) continue;
        // levels >= 1: beyond about 32 pixels per thread a band only gets longer (at 512 threads: 640 wide, 32 rows
        // 4 % slower than 16; 480 wide, 32 rows 16 % faster than 16)
        if (lvl > 0 && (uint32_t)cand * gw > 32u * threads && cand > kFrontRowsWide) continue;
        const uint32_t lds = front_lds_bytes(front_geometry(pyr, lvl, gw, gh, 1, (uint32_t)cand, 0u, threads));
        if (lds > max_lds) continue;
        if (forced == (uint32_t)cand) f.want = (uint32_t)cand, f.want_lds = lds;
        if (!f.once) f.once = (uint32_t)cand, f.once_lds = lds;
        if (!f.twice && 2u * lds <= max_lds) f.twice = (uint32_t)cand, f.twice_lds = lds;
    }
    return f;
}

// Rows, threads and tile width of level lvl of the plain fused pipeline; gw, gh: the octave's FAST dispatch domain.
// Band height from kFrontBandHeights (64, 32, 16, 8 rows: x of a queue entry in 9, 10, 11, 12 bits).  Two workgroups per CU matter
// more than the smaller halo share of a taller band (0.62 against 0.45 ms at 720p with one), and a band should hold about 20 k pixels
// (the 1024 threads then take 2.5 pre-test items each): a level takes the tallest band of which two fit the CU's LDS -- level 0: 64
// rows up to about 330 wide, 32 up to 700, 16 up to 1390, 8 up to 1980 --, else the tallest that fits at all (16 rows up to 2048, 8
// rows up to 4096).
inline BandPick pick_level_bands(const Pyramid& pyr, uint32_t lvl, uint32_t gw, uint32_t gh, uint32_t max_batch, uint32_t oob, uint32_t max_lds,
                                 const PlanEnv& env) {
    BandPick pick;
    const uint32_t w = pyr.w[lvl], forced = env.band_rows;
    // Levels >= 1 take level 0's shape -- 1024 threads, sixteen-pixel pre-test items -- where a band of which two fit
    // a CU holds about as many pixels as level 0's at 1280 columns (18 k and more: 640 columns x 32 rows, 320 x 64,
    // 1280 x 16; measured at 720p, 640x480, 2560x1440: 5 ... 21 % off k_front<false>), and 512 threads otherwise
    // (480 columns: the tallest band that fits twice is 32 x 480 = 15 k pixels, 13 % slower on 1024 threads; 160
    // columns: 27 % slower).  Not for programs of one frame (flat bands), forced heights, tiles or an out-of-level
    // policy (those instances exist for 512 threads only).
    BandFit f;
    if (lvl > 0 && max_batch > 1u && !forced && !env.tile_w_set && oob == kOobZero && !env.ln_512) {
        f = fit_bands(pyr, lvl, gw, gh, (uint32_t)kFrontThreadsLNBig, forced, max_lds);
        if (f.twice != 0u && f.twice * gw >= 18432u) pick.threads = (uint32_t)kFrontThreadsLNBig;
    }
    if (pick.threads != (uint32_t)kFrontThreadsLNBig)
        f = fit_bands(pyr, lvl, gw, gh, lvl == 0 ? (uint32_t)kFrontThreadsL0 : (uint32_t)kFrontThreadsLN, forced, max_lds);
    // the tallest band of which two fit a CU; else the tallest that fits at all
    const bool two_per_cu = f.twice != 0u;
    pick.rows = two_per_cu ? f.twice : f.once, pick.lds = two_per_cu ? f.twice_lds : f.once_lds;
    // A program for one frame at a time (the reference's call shape) is after latency, not throughput: its 45 + 23
    // bands cannot fill 256 CUs anyway, so it takes the flattest bands -- twice the workgroups, each with half
    // the work on its critical path (k_front<true> 16.3 -> 13.6 us at 720p).
    if (max_batch == 1u && two_per_cu && !f.want && !env.no_latency_bands) {
        const uint32_t flat = (uint32_t)kFrontRowsWide;
        const uint32_t lds = front_lds_bytes(front_geometry(pyr, lvl, gw, gh, 1, flat));
        if (std::max(w, gw) <= (1u << front_x_bits((int)flat)) && lds <= max_lds) pick.rows = flat, pick.lds = lds;
    }
    if (f.want) pick.rows = f.want, pick.lds = f.want_lds;
    // Too wide for two full-width bands per CU (one workgroup per CU costs a third of the rate: 0.62 against
    // 0.45 ms at 720p), or for any: column tiles of about kFrontTileW columns -- 16 rows x 1280 columns is the
    // shape the kernel is tuned on --, equal ones, wide enough for tile 0 to hold the columns the band's blur
    // reads (front_tile0_holds_blur); 8 rows where 16-row tiles of that width do not fit a CU twice.
    if ((!two_per_cu && !f.want) || env.tile_w_set) {
        const uint32_t dom = (std::max(w, gw) + 7u) & ~7u;
        uint32_t want_w = env.tile_w_set ? env.tile_w : (uint32_t)kFrontTileW, tw = dom, t_rows = 0, t_lds = 0;
        for (; tw >= dom || t_rows == 0u; want_w += 64u) {
            const uint32_t n_ct = std::max(1u, (dom + want_w - 1u) / want_w);
            tw = std::min(dom, (((dom + n_ct - 1u) / n_ct) + 7u) & ~7u);
            t_rows = 0;
            for (uint32_t cand : {16u, 8u}) {
                const FrontGeom tg = front_geometry(pyr, lvl, gw, gh, 1, cand, tw);
                const uint32_t lds = front_lds_bytes(tg);
                const uint32_t items = lvl == 0 ? (tg.tw + 12u) / 4u : (tg.tw + 20u) / 8u;  // staged items of a row <= threads
                if (!front_tile0_holds_blur(tg, w) || cand > (1u << (15u - tg.xb)) || lds > max_lds ||
                    items > (lvl == 0 ? (uint32_t)kFrontThreadsL0 : (uint32_t)kFrontThreadsLN))
                    continue;
                if (!t_rows || (2u * lds <= max_lds && 2u * t_lds > max_lds)) t_rows = cand, t_lds = lds;
                if (2u * t_lds <= max_lds) break;
            }
            if (t_rows || want_w >= dom) break;
        }
        if (t_rows) pick.rows = t_rows, pick.lds = t_lds, pick.tile_w = tw;
    }
    return pick;
}

// Why a program that did not ask for the staged kernels got them.
inline std::string staged_note(const ProgramPlan& pl, uint32_t flags, uint32_t max_lds) {
    const Pyramid& py = pl.pyr;
    char why[256];
    const bool plain = !pl.intended && !(flags & ORB_FLAG_NMS) && pl.arc == 12u;  // the reference's own algorithm
    if ((py.w[0] & 3u) != 0u && !plain)
        snprintf(why, sizeof why, "width %u is not a multiple of 4 (the tile kernels read RGBA quads)", py.w[0]);
    else if (py.w[0] < 8u)
        snprintf(why, sizeof why, "width %u is below 8", py.w[0]);
    else if (!pl.intended && py.w[0] > (uint32_t)kFrontMaxWidthTiled)
        snprintf(why, sizeof why, "width %u exceeds %d", py.w[0], kFrontMaxWidthTiled);
    else if ((uint64_t)py.w[0] * py.h[0] > (1ull << 26) || py.h[0] > 16384u)
        snprintf(why, sizeof why, "%ux%u exceeds the fused kernels' 2^26-pixel / 16384-row index range", py.w[0], py.h[0]);
    else if (!pl.intended && !plain && py.depth > 1 && !(py.w[0] == 2u * py.w[1] && py.h[0] == 2u * py.h[1]))
        snprintf(why, sizeof why, "level 0 (%ux%u) does not halve exactly and hierarchy_depth > 1", py.w[0], py.h[0]);
    else if (pl.input_y8 && ((flags & ORB_FLAG_NMS) || pl.arc != 12u))
        snprintf(why, sizeof why, "the tile kernels of the arc/NMS extensions read RGBA");
    else
        snprintf(why, sizeof why, "the band does not fit in %u bytes of LDS", max_lds);
    return std::string("staged pipeline (one kernel per reference stage, about 1/7 of the fused rate): ") + why;
}

// Everything orb_program_create decides before it allocates.  max_lds: the device's LDS per workgroup.  The three pipelines exclude
// each other by their eligibility; each falls back to `false` when a band of it needs more than max_lds.
inline ProgramPlan plan_program(const OrbConfig& config, const OrbOptions& opt, uint32_t max_lds, const PlanEnv& env) {
    ProgramPlan pl;
    const uint32_t W = config.image_size.width, H = config.image_size.height;
    pl.max_batch = opt.max_batch ? opt.max_batch : 1u;
    pl.intended = (opt.flags & ORB_FLAG_INTENDED) != 0u;
    pl.input_y8 = (opt.flags & ORB_FLAG_INPUT_Y8) != 0u;
    pl.arc = opt.fast_arc ? opt.fast_arc : (pl.intended ? 9u : 12u);
    pl.oob = opt.oob_policy;
    pl.wq = opt.sampler_weight_bits ? (float)(1u << opt.sampler_weight_bits) : 0.0f;
    pl.frame_bytes = (size_t)W * H * (pl.input_y8 ? 1u : 4u);
    layout_pyramid(W, H, config.hierarchy_depth, &pl.pyr);
    const Pyramid& pyr = pl.pyr;
    const uint32_t D = pyr.depth;

    pl.fused = fused_eligible(pl, opt.flags);
    if (pl.fused) {
        uint32_t need = 0;
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            uint32_t gw, gh;
            reference_grid(pyr, lvl, &gw, &gh);
            const BandPick pick = pick_level_bands(pyr, lvl, gw, gh, pl.max_batch, pl.oob, max_lds, env);
            pl.band_rows_lvl[lvl] = pick.rows;
            pl.ln_threads[lvl] = pick.threads;
            pl.tile_w_lvl[lvl] = pick.tile_w;
            need = pick.rows == 0 ? max_lds + 1u : std::max(need, pick.lds);
        }
        if (need > max_lds) pl.fused = false;
    }
    if (pl.fused) {
        BandGeom& bg = pl.bands;
        uint32_t slots = 0;
        uint64_t band_px = 0;  // pixels of the largest band (tile): no band can hold more corners
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            bg.slot_base[lvl] = slots;
            const uint64_t lvl_cols = ((uint64_t)(W >> lvl) + 7u) / 8u * 8u;
            uint32_t n_ct = 1;
            if (pl.tile_w_lvl[lvl]) n_ct = (uint32_t)((lvl_cols + pl.tile_w_lvl[lvl] - 1u) / pl.tile_w_lvl[lvl]);
            slots += front_bands(pyr, lvl, pl.band_rows_lvl[lvl]) * n_ct;
            band_px = std::max<uint64_t>(band_px, (uint64_t)pl.band_rows_lvl[lvl] * (pl.tile_w_lvl[lvl] ? pl.tile_w_lvl[lvl] : lvl_cols));
        }
        bg.slot_base[D] = slots;
        bg.n_slots = slots;
        bg.seg_cap = (uint32_t)(band_px < config.max_features ? band_px : config.max_features);
        RowsGeom& rg = pl.rows;
        rg.n_slots = bg.n_slots;
        rg.seg_cap = bg.seg_cap;
        for (uint32_t lvl = 0; lvl <= D; lvl++) rg.slot_base[lvl] = bg.slot_base[lvl];
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            // columns [0, qa) of the level's blur are kept as one constant per row (k_front, phase C)
            const uint32_t q = front_geometry(pyr, lvl, 8, 8, 1).blur_q, qa = q & ~7u;
            pl.blur_qa[lvl] = qa;
            rg.qa[lvl] = qa;
            // a keypoint is "flat" when every sample column lies below Q, not only below qa: the stored columns [qa, Q) hold
            // the row constant too
            rg.flat_end[lvl] = q > (uint32_t)kBriefHalo ? q - kBriefHalo : 0u;
        }
        pl.use_brief_t = brieft_geometry(pyr, pl.oob, env, rg, 2u, &pl.brieft);
        pl.seg_classes = pl.use_brief_t ? 2u : 1u;
    }

    pl.fused_i = fused_i_eligible(pl, opt.flags);
    if (pl.fused_i) {
        IBriefGeom& bg = pl.itiles;
        uint32_t slots = 0;
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            bg.tw[lvl] = itile_width(pyr.w[lvl]);
            bg.n_ct[lvl] = (pyr.w[lvl] + bg.tw[lvl] - 1u) / bg.tw[lvl];
            bg.slot_base[lvl] = slots;
            slots += ((pyr.h[lvl] + kFrontRows - 1) / kFrontRows) * bg.n_ct[lvl];
        }
        bg.slot_base[D] = slots;
        bg.n_slots = slots;
        uint32_t groups = 0, max_rows = 0;
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            bg.n_bands[lvl] = (pyr.h[lvl] + kFrontRows - 1) / kFrontRows;
            bg.group_base[lvl] = groups;
            groups += ((bg.n_bands[lvl] + kIBriefStack - 1) / kIBriefStack) * bg.n_ct[lvl];
            const uint32_t rows = std::min<uint32_t>(bg.n_bands[lvl], kIBriefStack) * kFrontRows + 2u * kBriefHalo;
            if (rows > max_rows) max_rows = rows;
        }
        bg.group_base[D] = groups;
        // The Gaussian (IM-3) inside k_front_i, straight from the tile; the level-0 grey plane is then only stored when a level
        // that is not an exact half needs it (k_mip reads planes).
        pl.igauss_fused = !env.i_gauss_kernel;
        for (uint32_t lvl = 0; lvl < D; lvl++) pl.igauss_fused = pl.igauss_fused && ifront_gauss_fits(bg.tw[lvl]);
        pl.igrey_stored = !pl.igauss_fused || (D > 1 && !(pyr.w[0] == 2u * pyr.w[1] && pyr.h[0] == 2u * pyr.h[1]));
        // a tile's segment holds every keypoint the tile can have (one per pixel), whatever max_features is: the
        // top-K cut (IM-8) must see all candidates, not the ones that happened to be appended first
        bg.seg_cap = (uint32_t)kFrontRows * bg.tw[0];
        bg.pitch = (uint32_t)kITileW + 2u * kIBriefApronX;
        pl.ibrief_lds = max_rows * bg.pitch * (uint32_t)sizeof(uint16_t);
    }

    pl.fused_x = fused_x_eligible(pl, opt.flags);
    if (pl.fused_x) {
        // tiles over the reference's dispatch grid of every octave; blur-only k_front launches over 16-row bands
        IBriefGeom& bg = pl.itiles;
        RowsGeom& rg = pl.xrows;
        uint32_t slots = 0, bands = 0, need = 0;
        for (uint32_t lvl = 0; lvl < D; lvl++) {
            uint32_t gw, gh;
            reference_grid(pyr, lvl, &gw, &gh);
            const uint32_t dw = std::max(pyr.w[lvl], gw), dh = std::max(pyr.h[lvl], gh);
            bg.tw[lvl] = itile_width(dw);
            bg.n_ct[lvl] = (dw + bg.tw[lvl] - 1u) / bg.tw[lvl];
            bg.n_bands[lvl] = (dh + kFrontRows - 1) / kFrontRows;
            bg.slot_base[lvl] = slots;
            rg.slot_base[lvl] = slots;
            slots += bg.n_bands[lvl] * bg.n_ct[lvl];
            const FrontGeom fg = front_geometry(pyr, lvl, gw ? gw : 8u, gh, 1);
            bands += fg.n_bands;
            need = std::max(need, front_lds_bytes(fg));
            const uint32_t qa = fg.blur_q & ~7u;
            pl.blur_qa[lvl] = qa;
            rg.qa[lvl] = qa;
            rg.flat_end[lvl] = fg.blur_q > (uint32_t)kBriefHalo ? fg.blur_q - kBriefHalo : 0u;
        }
        bg.slot_base[D] = slots;
        rg.slot_base[D] = slots;
        bg.n_slots = slots;
        bg.seg_cap = (uint32_t)kFrontRows * bg.tw[0];
        rg.n_slots = slots;
        rg.seg_cap = bg.seg_cap;
        pl.xband_slots = bands;
        if (need > max_lds)
            pl.fused_x = false;
        else
            pl.use_brief_t = brieft_geometry(pyr, pl.oob, env, rg, 1u, &pl.brieft);  // the tile kernels keep one list per tile
    }

    // A silent fall to the per-stage kernels is a 7x performance cliff: say why, once, and keep it readable.
    if (!(pl.fused || pl.fused_i || pl.fused_x) && !(opt.flags & ORB_FLAG_STAGED)) pl.pipeline_note = staged_note(pl, opt.flags, max_lds);

    if (!(pl.fused_i || pl.fused_x) && (opt.flags & (ORB_FLAG_NMS | ORB_FLAG_INTENDED))) {
        // score planes: one float per dispatch-grid pixel of every octave + a 1-px border; provisional list
        uint32_t off = 0;
        for (uint32_t m = 0; m < D; m++) {
            uint32_t gw, gh;
            reference_grid(pyr, m, &gw, &gh);
            pl.score_layout.off[m] = off;
            pl.score_layout.pitch[m] = gw + 2u;
            off += (gw + 2u) * (gh + 2u);
        }
        pl.score_layout.stride = (off + 63u) & ~63u;
        // The provisional list must hold every detection (the NMS and the top-K cut have to see all of them): one
        // slot per texel of the pyramid is the worst case and what is allocated (20 bytes per texel and frame).
        pl.cap_prov = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(pyr.stride, config.max_features), 1u << 24);
    }
    return pl;
}

// The geometry of level `lvl` of the plain fused pipeline for a batch of n frames, less the device pointers (orb_api.hip attaches
// them: fused_level_geometry); gw, gh: the octave's FAST dispatch domain (orb.rs:501-519).
inline FrontGeom plan_level_geometry(const ProgramPlan& pl, const OrbOptions& opt, const PlanEnv& env, uint32_t lvl, uint32_t gw, uint32_t gh, uint32_t n) {
    const Pyramid& pyr = pl.pyr;
    FrontGeom g = front_geometry(pyr, lvl, gw ? gw : 8u, gh, n, pl.band_rows_lvl[lvl], pl.tile_w_lvl[lvl], pl.ln_threads[lvl]);
    if (gw == 0) g.gh = 0;  // no FAST dispatch at this octave (orb.rs:511-515 with width 0)
    g.slot_base = pl.bands.slot_base[lvl];
    g.n_slots = pl.bands.n_slots;
    g.seg_cap = pl.bands.seg_cap;
    g.n_classes = pl.seg_classes;
    if (env.phase_mask >= 0) g.phase_mask = (uint32_t)env.phase_mask;
    if (env.no_swizzle) g.xcd_swizzle = 0u;
    g.oob = pl.oob;
    g.wq = pl.wq;
    g.fp = opt.fp_contract;
    g.store_grey = (lvl == 0 && pyr.depth > 1 && !(pyr.w[0] == 2u * pyr.w[1] && pyr.h[0] == 2u * pyr.h[1])) ? 1u : 0u;
    return g;
}

// Which instance of k_front a prepared launch takes: one with a compile-time geometry (orb_kernels_front.h) when the launch is of that
// instance's kind -- level, input, alignment, band height, threads, arithmetic form -- AND every field the geometry replaces holds the
// compiled-in value, compared one by one (the frame size alone does not decide: TINYORB_BAND_ROWS, a program of one frame, a batch that
// is not a multiple of 8, an out-of-level policy, another depth all change the geometry); the generic instance otherwise, and always
// under TINYORB_FRONT_GENERIC=1.  `why`: what ruled the specialised instance out.
inline FrontGeoId front_pick_geo(const PlanEnv& env, uint32_t fp_contract, const FrontLaunch& L, const char** why = nullptr) {
    const char* reason = nullptr;
    FrontGeoId id = kFrontGeoGeneric;
    const bool l0 = L.g.lvl == 0u;
    if (env.front_generic) reason = "TINYORB_FRONT_GENERIC";
    else if (L.g.lvl > 1u) reason = "lvl";
    else if (L.input_y8) reason = "input_y8";
    else if (L.general) reason = "general";
    else if (L.oob) reason = "oob";
    else if (L.from_plane) reason = "from_plane";
    else if (front_form(fp_contract, l0) != 0u) reason = "fp_contract";
    else if (L.band_rows != (l0 ? FrontGeo720pL0::rows : FrontGeo720pL1::rows)) reason = "band_rows";
    else if (!l0 && L.ln_threads != (uint32_t)kFrontThreadsLNBig) reason = "ln_threads";
    else reason = l0 ? front_geo_mismatch<FrontGeo720pL0>(L.g, L.pyr) : front_geo_mismatch<FrontGeo720pL1>(L.g, L.pyr);
    if (!reason) id = l0 ? kFrontGeo720pL0 : kFrontGeo720pL1;
    if (why) *why = reason;
    return id;
}

inline const char* front_geo_name(FrontGeoId id) {
    return id == kFrontGeoGeneric ? "generic" : (id == kFrontGeo720pL0 ? "specialised 720p-L0" : "specialised 720p-L1");
}

// Which instance a full batch (max_batch frames) takes at level lvl of the plain fused pipeline, and why not the specialised one
inline FrontGeoId front_pick_full_batch(const ProgramPlan& pl, const OrbOptions& opt, const PlanEnv& env, uint32_t lvl, const char** why) {
    uint32_t gw, gh;
    reference_grid(pl.pyr, lvl, &gw, &gh);
    FrontLaunch L{};
    L.pyr = pl.pyr, L.g = plan_level_geometry(pl, opt, env, lvl, gw, gh, pl.max_batch);
    L.band_rows = pl.band_rows_lvl[lvl], L.ln_threads = pl.ln_threads[lvl], L.input_y8 = pl.input_y8;
    L.general = lvl == 0 && ((pl.pyr.w[0] & 3u) || L.g.store_grey), L.oob = pl.oob != kOobZero;
    return front_pick_geo(env, opt.fp_contract, L, why);
}

// The lines of TINYORB_FRONT_TRACE=1: one per level of the plain fused pipeline (tests/test_gpu_front_specialised.py parses them)
inline std::string front_trace_text(const ProgramPlan& pl, const OrbOptions& opt, const PlanEnv& env) {
    std::string text;
    for (uint32_t lvl = 0; lvl < pl.pyr.depth; lvl++) {
        const char* why = nullptr;
        const FrontGeoId id = front_pick_full_batch(pl, opt, env, lvl, &why);
        char line[256];
        snprintf(line, sizeof line, "tinyorb: k_front level %u (%ux%u, %u-row bands, batch %u) takes the %s instance%s%s\n", lvl, pl.pyr.w[lvl], pl.pyr.h[lvl],
                 pl.band_rows_lvl[lvl], pl.max_batch, front_geo_name(id), why ? ": " : "", why ? why : "");
        text += line;
    }
    return text;
}

}  // namespace orb
