// CPU harness of csrc/launch_plan.h with the builds of algo=pssmlt over technique=bdpt named (tests/test_pssmlt_bdpt.py): the
// chain-kernel plan of one configuration, as tests/native/plan_harness.cpp prints it.
//   pssmlt_bdpt_plan_harness key=value ... [DRMLT_X=value ...]
// keys are the fields of PlanInputs; DRMLT_* arguments are put into the environment before read_knobs(). Prints one JSON object.
#include "launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static const char *const BUILD_NAMES[] = {
    "PSSMLT",
    "V5_F0_ROWS", "V5_F1_ROWS", "V5_F3_ROWS", "V5_F7_ROWS",
    "V5_F7_GLOBAL", "V5_F0_STAMPS", "V5_F0", "V5_F1", "V5_F3", "V5_F7",
    "V5_F8_S32_ROWS", "V5_F15_S32_ROWS", "V5_F8_OVF_ROWS", "V5_F15_OVF_ROWS", "V5_F8_ROWS", "V5_F15_ROWS",
    "V5_F8_S32", "V5_F15_S32", "V5_F8_OVF", "V5_F15_OVF", "V5_F8_STAMPS", "V5_F8", "V5_F15",
    "V4_F0_STAMPS", "V4_F0", "V4_F3_STAMPS", "V4_F3", "V4_F7", "V4_F15_S32", "V4_F15_OVF", "V4_F15",
    "V4_F7_GLOBAL", "V4_F8_S32_GLOBAL", "V4_F15_S32_GLOBAL", "V4_F15_OVF_GLOBAL", "V4_F15_STAMPS_GLOBAL", "V4_F8_GLOBAL", "V4_F15_GLOBAL",
    "V3_F0", "V3_F3", "V3_F7", "V3_F15", "V3_F15_GLOBAL",
    "MMLT_F7_TABLES", "MMLT_F15", "MMLT_F7",
    "BDPT_F15", "BDPT_F7_OCC2_TABLES", "BDPT_F7_OCC2", "BDPT_F7",
    "PSSMLT_BDPT_F15", "PSSMLT_BDPT_F7_OCC2_TABLES", "PSSMLT_BDPT_F7_OCC2", "PSSMLT_BDPT_F7",
};
static_assert(sizeof BUILD_NAMES / sizeof *BUILD_NAMES == (size_t) Build::PSSMLT_BDPT_F7 + 1, "one name per Build");

int main(int argc, char **argv) {
    PlanInputs in;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string key(argv[i], eq - argv[i]);
        const char *v = eq + 1;
        if (key.rfind("DRMLT_", 0) == 0) { setenv(key.c_str(), v, 1); continue; }
        const long long n = strtoll(v, nullptr, 0);
        if (key == "technique") in.technique = (int) n;
        else if (key == "algo") in.algo = (int) n;
        else if (key == "work_units") in.work_units = (int) n;
        else if (key == "work_units_rule") in.work_units_rule = (int) n;
        else if (key == "budget") in.budget = (uint64_t) n;
        else if (key == "features") in.features = (int) n;
        else if (key == "use_bvh") in.use_bvh = n != 0;
        else if (key == "bvh_stack16") in.bvh_stack16 = n != 0;
        else if (key == "bvh_overflow") in.bvh_overflow = n != 0;
        else if (key == "n_shade") in.n_shade = (uint32_t) n;
        else if (key == "n_bsdfs") in.n_bsdfs = (uint32_t) n;
        else if (key == "n_emitters") in.n_emitters = (uint32_t) n;
        else if (key == "scene_bytes") in.scene_bytes = (uint64_t) n;
        else if (key == "eff_dim") in.eff_dim = (int) n;
        else if (key == "max_depth") in.max_depth = (int) n;
        else if (key == "mmlt_S") in.mmlt_S = (int) n;
        else if (key == "mmlt_E") in.mmlt_E = (int) n;
        else if (key == "cus") in.cus = (int) n;
        else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const Knobs K = read_knobs();
    const uint32_t n = derive_chains(in, K);
    const ChainPlan p = plan_chains(in, n, K);
    printf("{\"build\": \"%s\", \"chains\": %u, \"grid\": %u, \"lds\": %zu, \"aux_lds\": %zu, \"kernel_variant\": %d, \"tables_in_lds\": %d, "
           "\"small_tables_lds\": %d, \"rows_mem\": %d, \"mh_batch\": %d, \"trace_yield\": %d, \"pool_refill\": %d, \"trace_vote\": %d, "
           "\"run_ahead\": %d, \"note\": \"%s\"}\n",
           BUILD_NAMES[(int) p.build], n, p.grid, p.lds, p.aux_lds, p.kernel_variant, p.tables_in_lds, p.small_tables_lds, (int) p.rows_mem,
           p.mh_batch, p.trace_yield, p.pool_refill, p.trace_vote, (int) p.run_ahead, p.note.c_str());
    return 0;
}
