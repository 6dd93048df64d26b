// plan_dump.cpp -- prints what csrc/orb_plan.h decides, one JSON line per case, with no device (tests/test_plan.py compares the
// lines with tests/golden/plan/cases.json, which was recorded from the code before the plan had a header of its own: NOTEBOOK.md).
// stdin: lines of `W H depth max_batch flags fast_arc oob_policy max_features max_lds`; the create-time switches come from the environment.
#include "../tinyslam_amd/csrc/orb_plan.h"

using namespace orb;

// The kernel headers that orb_plan.h takes its structs and constants from define kernels, and a host-only object registers them when
// the program starts.  Nothing here launches one: the registration calls land in these stand-ins, so the program loads no device code.
extern "C" {
void** __hipRegisterFatBinary(const void*) {
    static void* handle;
    return &handle;
}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipUnregisterFatBinary(void**) {}
}

static std::string jstr(const char* s) {
    if (!s) return "null";
    std::string o = "\"";
    for (; *s; s++) {
        if (*s == '"' || *s == '\\') o += '\\';
        o += *s;
    }
    return o + "\"";
}
static const char* jb(bool b) { return b ? "true" : "false"; }
template <class A>
static std::string jarr(const A& a, uint32_t n) {
    std::string o = "[";
    for (uint32_t i = 0; i < n; i++) o += (i ? ", " : "") + std::to_string(a[i]);
    return o + "]";
}

int main() {
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        unsigned W, H, depth, mb, flags, arc, oob, cap, max_lds;
        if (sscanf(line, "%u %u %u %u %u %u %u %u %u", &W, &H, &depth, &mb, &flags, &arc, &oob, &cap, &max_lds) != 9) continue;
        OrbConfig cfg{};
        cfg.image_size = {W, H, 1u};
        cfg.max_features = cap;
        cfg.hierarchy_depth = depth;
        cfg.initial_threshold = 20.0f / 255.0f;
        OrbOptions opt{};
        opt.max_batch = mb;
        opt.flags = flags;
        opt.fast_arc = arc;
        opt.oob_policy = oob;
        if (const char* msg = check_config(&cfg, &opt)) {
            printf("{\"error\": %s}\n", jstr(msg).c_str());
            continue;
        }
        const PlanEnv env = read_plan_env(opt.flags);
        const ProgramPlan s = plan_program(cfg, opt, max_lds, env);
        const uint32_t D = s.pyr.depth;
        printf("{\"error\": null, \"fused\": %s, \"fused_i\": %s, \"fused_x\": %s, \"use_brief_t\": %s, \"seg_classes\": %u, ", jb(s.fused), jb(s.fused_i),
               jb(s.fused_x), jb(s.use_brief_t), s.seg_classes);
        printf("\"bands\": {\"n_slots\": %u, \"seg_cap\": %u, \"slot_base\": %s}, ", s.bands.n_slots, s.bands.seg_cap, jarr(s.bands.slot_base, D + 1).c_str());
        printf("\"itiles\": {\"n_slots\": %u, \"seg_cap\": %u, \"tw\": %s, \"n_ct\": %s}, ", s.itiles.n_slots, s.itiles.seg_cap, jarr(s.itiles.tw, D).c_str(),
               jarr(s.itiles.n_ct, D).c_str());
        printf("\"brieft_rows_padded\": %u, \"igauss_fused\": %s, \"igrey_stored\": %s, \"ibrief_lds\": %u, ", s.brieft.rows_padded, jb(s.igauss_fused),
               jb(s.igrey_stored), s.ibrief_lds);
        printf("\"score_stride\": %u, \"cap_prov\": %u, \"xband_slots\": %u, \"pipeline_note\": %s, \"levels\": [", s.score_layout.stride, s.cap_prov,
               s.xband_slots, jstr(s.pipeline_note.c_str()).c_str());
        for (uint32_t l = 0; l < D; l++) {
            const char *why = nullptr, *geo = nullptr;  // the instance of k_front a full batch takes: of the plain fused pipeline only
            if (s.fused) geo = front_geo_name(front_pick_full_batch(s, opt, env, l, &why));
            printf("%s{\"w\": %u, \"h\": %u, \"band_rows\": %u, \"ln_threads\": %u, \"tile_w\": %u, \"blur_qa\": %u, \"flat_end\": %u, \"xflat_end\": %u, "
                   "\"geo\": %s, \"why\": %s}",
                   l ? ", " : "", s.pyr.w[l], s.pyr.h[l], s.band_rows_lvl[l], s.ln_threads[l], s.tile_w_lvl[l], s.blur_qa[l], s.rows.flat_end[l],
                   s.xrows.flat_end[l], jstr(geo).c_str(), jstr(why).c_str());
        }
        printf("]}\n");
    }
    return 0;
}
