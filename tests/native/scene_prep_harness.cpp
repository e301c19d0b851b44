// CPU harness of csrc/scene_prep.h (tests/test_scene_prep.py): what drmlt_create prepares for one scene and configuration.
//   scene_prep_harness scene=FILE [tables=FILE] [params=FILE] key=value ... [DRMLT_X=value ...]
// scene: a file written by SceneData.save(); keys are the fields of drmlt_config (defaults: abi.make_config's); DRMLT_* arguments
// are put into the environment before read_knobs(). Prints one JSON object: the refusal (or ""), the scalar fields of DParams, the
// PlanInputs, bvh_depth, ovf_entries and the byte count of every table; the raw tables go to `tables`, one after the other, in
// the order of "tables".
#include "scene_prep.h"

#include "drmlt_integrator.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

int main(int argc, char **argv) {
    drmlt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.type = DRMLT_TYPE_ORBITAL; cfg.max_depth = -1; cfg.rr_depth = 5; cfg.direct_samples = 16; cfg.luminance_samples = 100000;
    cfg.work_units = -1; cfg.sample_count = 1; cfg.p_large = 0.3f; cfg.sigma = 1.0f / 64.0f; cfg.scale_second = 0.1f;
    cfg.average_luminance = -1.0f; cfg.kelemen_style_weights = 1; cfg.kelemen_style_mutation = 1;
    const struct { const char *name; int32_t *i; float *f; } fields[] = {
        {"algo", &cfg.algo, nullptr}, {"technique", &cfg.technique, nullptr}, {"type", &cfg.type, nullptr}, {"max_depth", &cfg.max_depth, nullptr},
        {"rr_depth", &cfg.rr_depth, nullptr}, {"direct_samples", &cfg.direct_samples, nullptr}, {"luminance_samples", &cfg.luminance_samples, nullptr},
        {"work_units", &cfg.work_units, nullptr}, {"sample_count", &cfg.sample_count, nullptr}, {"p_large", nullptr, &cfg.p_large},
        {"sigma", nullptr, &cfg.sigma}, {"scale_second", nullptr, &cfg.scale_second}, {"average_luminance", nullptr, &cfg.average_luminance},
        {"acceptance_map", &cfg.acceptance_map, nullptr}, {"timid_after_large", &cfg.timid_after_large, nullptr},
        {"fix_emitter_path", &cfg.fix_emitter_path, nullptr}, {"use_mixture", &cfg.use_mixture, nullptr},
        {"kelemen_style_weights", &cfg.kelemen_style_weights, nullptr}, {"kelemen_style_mutation", &cfg.kelemen_style_mutation, nullptr},
        {"no_light_image", &cfg.no_light_image, nullptr}, {"timeout_s", &cfg.timeout_s, nullptr}, {"no_direct_sampling", &cfg.no_direct_sampling, nullptr},
        {"seed_rule", &cfg.seed_rule, nullptr}, {"work_units_rule", &cfg.work_units_rule, nullptr}};
    std::string scene_path, tables_path, params_path;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string key(argv[i], eq - argv[i]);
        const char *v = eq + 1;
        if (key.rfind("DRMLT_", 0) == 0) { setenv(key.c_str(), v, 1); continue; }
        if (key == "scene") { scene_path = v; continue; }
        if (key == "tables") { tables_path = v; continue; }
        if (key == "params") { params_path = v; continue; }
        bool known = false;
        for (const auto &f : fields)
            if (key == f.name) {
                if (f.i) *f.i = (int32_t) strtol(v, nullptr, 0);
                else *f.f = strtof(v, nullptr);
                known = true;
            }
        if (!known) { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const drmlt_host::SceneFile sf = drmlt_host::SceneFile::load(scene_path);
    const drmlt_scene scene = sf.view();
    const Knobs K = read_knobs();
    PreparedScene S;
    const std::string refusal = prepare_scene(cfg, scene, K, S);
    if (!refusal.empty()) S = PreparedScene();

    const struct { const char *name; const void *p; size_t bytes; } tables[] = {
        {"prims", S.prims.data(), S.prims.size() * sizeof(DPrim)}, {"shade", S.shade.data(), S.shade.size() * sizeof(DShade)},
        {"bsdfs", S.bsdfs.data(), S.bsdfs.size() * sizeof(DBsdf)}, {"emitters", S.emitters.data(), S.emitters.size() * sizeof(DEmitter)},
        {"lut", S.lut.data(), sizeof S.lut}, {"bvh", S.bvh.data(), S.bvh.size() * sizeof(DBvh4Node)},
        {"flat", S.flat.data(), S.flat.size() * sizeof(DPrimFlat)}, {"boxes", S.boxes.data(), S.boxes.size() * sizeof(DPrimBox)}};
    if (!tables_path.empty()) {
        FILE *f = fopen(tables_path.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", tables_path.c_str()); return 2; }
        for (const auto &t : tables)
            if (t.bytes && fwrite(t.p, t.bytes, 1, f) != 1) { fprintf(stderr, "short write to %s\n", tables_path.c_str()); return 2; }
        fclose(f);
    }
    // The raw DParams block (its pointers are null), for tests/native/ray_probe.hip. A file of its own, not an entry of "tables": the JSON's
    // table list and the tables file are pinned by hashes in tests/test_scene_prep.py, which a further entry would change in every case.
    if (!params_path.empty()) {
        FILE *f = fopen(params_path.c_str(), "wb");
        if (!f || fwrite(&S.P, sizeof S.P, 1, f) != 1 || fclose(f) != 0) { fprintf(stderr, "cannot write %s\n", params_path.c_str()); return 2; }
    }

    const DParams &P = S.P;
    const PlanInputs &in = S.plan;
    printf("{\"refusal\": \"");
    for (char c : refusal) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    printf("\", \"tables\": [");
    for (const auto &t : tables) printf("%s[\"%s\", %zu]", &t == tables ? "" : ", ", t.name, t.bytes);
    printf("], \"params\": {");
#define I(f) printf("\"" #f "\": %d, ", (int) P.f)
#define F(f) printf("\"" #f "\": %.9g, ", (double) P.f)
    I(n_prims); I(n_shade); I(n_bsdfs); I(n_emitters); I(n_bvh_nodes); I(use_bvh); I(bvh_leaf_shift); I(bvh_stack16);
    I(n_flat); I(n_flat_rec); I(n_box); I(has_plain_tri);
    printf("\"cam\": [");
    for (int k = 0; k < 12; ++k) printf("%s%.9g", k ? ", " : "", (double) P.cam[k]);
    printf("], ");
    F(tan_half_fov); F(inv_aspect); F(near_clip); F(far_clip); I(width); I(height); F(filter_radius); F(filter_scale); F(box_weight);
    I(type); I(max_depth); I(rr_depth); I(exclude_direct); I(acceptance_map); I(timid_after_large); I(use_mixture);
    F(p_large); F(sigma2); I(kelemen_weights); I(kelemen_mutation); F(pss_sigma); F(luminance_b);
    I(technique); I(light_image); I(fix_emitter_path);
    I(max_dim); I(eff_dim); I(mmlt_S); I(mmlt_E); I(mmlt_dmax); I(bd_Dd); I(features); I(env_emitter);
#undef I
#undef F
    printf("\"debug\": %d}, \"plan\": {\"technique\": %d, \"algo\": %d, \"work_units\": %d, \"work_units_rule\": %d, \"budget\": %llu, \"features\": %d, "
           "\"use_bvh\": %d, \"bvh_stack16\": %d, \"bvh_overflow\": %d, \"n_shade\": %u, \"n_bsdfs\": %u, \"n_emitters\": %u, \"scene_bytes\": %llu, "
           "\"eff_dim\": %d, \"max_depth\": %d, \"mmlt_S\": %d, \"mmlt_E\": %d}, \"bvh_depth\": %d, \"ovf_entries\": %d}\n",
           (int) P.debug, in.technique, in.algo, in.work_units, in.work_units_rule, (unsigned long long) in.budget, in.features, (int) in.use_bvh,
           (int) in.bvh_stack16, (int) in.bvh_overflow, in.n_shade, in.n_bsdfs, in.n_emitters, (unsigned long long) in.scene_bytes, in.eff_dim,
           in.max_depth, in.mmlt_S, in.mmlt_E, S.bvh_depth, S.ovf_entries);
    return 0;
}
