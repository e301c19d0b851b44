// CPU harness of the first light's joined record (tests/test_scene_prep_one_light.py): csrc/scene_prep.h fills DParams::light and
// DParams::light_shade, csrc/device_types.h's scene_has_one_light decides whether k_mutate_v4 reads them.
//   one_light_harness scene=FILE [DRMLT_X=value ...]
// scene: a file written by SceneData.save(); DRMLT_* arguments are put into the environment before read_knobs(). The configuration
// is technique=path, type=orbital, maxDepth 8. Prints one JSON object: the refusal (or ""), n_emitters, the predicate, the debug
// mask, sizeof(DParams) % 8 and, in hex, the joined record's two parts beside the table entries they must copy.
#include "scene_prep.h"

#include "drmlt_integrator.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

static void hex(const char *name, const void *p, size_t n, const char *tail) {
    printf("\"%s\": \"", name);
    for (size_t i = 0; i < n; ++i) printf("%02x", ((const unsigned char *) p)[i]);
    printf("\"%s", tail);
}

int main(int argc, char **argv) {
    drmlt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.type = DRMLT_TYPE_ORBITAL; cfg.max_depth = 8; cfg.rr_depth = 5; cfg.direct_samples = -1; cfg.luminance_samples = 100000;
    cfg.work_units = -1; cfg.sample_count = 1; cfg.p_large = 0.3f; cfg.sigma = 1.0f / 64.0f; cfg.scale_second = 0.1f;
    cfg.average_luminance = -1.0f; cfg.kelemen_style_weights = 1; cfg.kelemen_style_mutation = 1;
    std::string scene_path;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string key(argv[i], eq - argv[i]);
        if (key.rfind("DRMLT_", 0) == 0) setenv(key.c_str(), eq + 1, 1);
        else if (key == "scene") scene_path = eq + 1;
        else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const drmlt_host::SceneFile sf = drmlt_host::SceneFile::load(scene_path);
    const drmlt_scene scene = sf.view();
    const Knobs K = read_knobs();
    PreparedScene S;
    const std::string refusal = prepare_scene(cfg, scene, K, S);
    if (!refusal.empty()) S = PreparedScene();
    const DParams &P = S.P;
    static_assert(sizeof(P.light) == 32 && sizeof(P.light_shade) == 64, "8 + 16 dwords");

    printf("{\"refusal\": \"");
    for (char c : refusal) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    printf("\", \"n_emitters\": %d, \"one_light\": %d, \"debug\": %d, \"features\": %d, \"sizeof_params_mod_8\": %d, ", (int) P.n_emitters,
           (int) scene_has_one_light(P), (int) P.debug, (int) P.features, (int) (sizeof(DParams) % 8));
    hex("light", &P.light, sizeof P.light, ", ");
    hex("light_shade", &P.light_shade, sizeof P.light_shade, ", ");
    if (!S.emitters.empty()) {
        hex("emitter0", &S.emitters[0], sizeof(DEmitter), ", ");
        hex("shade_of_emitter0", &S.shade[(size_t) S.emitters[0].prim], sizeof(DShade), ", ");
        printf("\"kind\": %d, ", (int) (S.shade[(size_t) S.emitters[0].prim].bsdf >> 24));
    }
    printf("\"n_shade\": %d}\n", (int) P.n_shade);
    return 0;
}
