// CPU harness of csrc/launch_plan.h's k_mutate_w2h selection (tests/test_w2h_plan.py).
//   w2h_plan_harness key=value ... [DRMLT_X=value ...]
// keys: the fields of PlanInputs the path plans read, the ray-record counts among them; DRMLT_* arguments are put into the
// environment before read_knobs(). Prints one JSON object: the plan's grid and LDS bytes, whether launch_mutate may run
// k_mutate_w2, and whether it then runs k_mutate_w2h.
#include "launch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

int main(int argc, char **argv) {
    PlanInputs in;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string key(argv[i], eq - argv[i]);
        const char *v = eq + 1;
        if (key.rfind("DRMLT_", 0) == 0) { setenv(key.c_str(), v, 1); continue; }
        const long long n = strtoll(v, nullptr, 0);
        if (key == "work_units") in.work_units = (int) n;
        else if (key == "budget") in.budget = (uint64_t) n;
        else if (key == "features") in.features = (int) n;
        else if (key == "n_shade") in.n_shade = (uint32_t) n;
        else if (key == "n_bsdfs") in.n_bsdfs = (uint32_t) n;
        else if (key == "n_emitters") in.n_emitters = (uint32_t) n;
        else if (key == "eff_dim") in.eff_dim = (int) n;
        else if (key == "max_depth") in.max_depth = (int) n;
        else if (key == "cus") in.cus = (int) n;
        else if (key == "n_box") in.n_box = (int) n;
        else if (key == "n_flat_rec") in.n_flat_rec = (int) n;
        else if (key == "has_plain_tri") in.has_plain_tri = n != 0;
        else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const Knobs K = read_knobs();
    const uint32_t n = derive_chains(in, K);
    const ChainPlan p = plan_chains(in, n, K);
    printf("{\"v4_f0\": %d, \"chains\": %u, \"grid\": %u, \"lds\": %zu, \"w2\": %d, \"w2_held\": %d, \"fits\": %d}\n", (int) (p.build == Build::V4_F0), n, p.grid,
           p.lds, (int) p.w2, (int) p.w2_held, (int) plan_detail::w2_held_launch(in.n_box, in.n_flat_rec, in.has_plain_tri));
    return 0;
}
