// CPU harness of the vertex normals (tests/test_smooth_normals.py). Two programs from one file:
//
// (1) default build, over csrc/scene_prep.h and csrc/smooth_frame.h:
//       normals_harness scene=FILE [uv=FILE out=FILE] [technique=N] [DRMLT_X=value ...]
//     scene: a file written by SceneData.save(). Prints one JSON object: the refusal (or ""), the feature bits, the kind of every
//     intersection record and of every shading record, the counts of flat, cuboid and vertex-normal records. With uv (two float32
//     per shape) and out: for every shape whose shading record is PRIM_SMOOTH, the frame that the kernels' own routine
//     (smooth_frame) builds from the PREPARED tables at that shape's (u, v), t = n x s as path_step forms it; nine float32 per
//     shape to `out` (zeros for the other shapes).
//
// (2) -DNORMALS_ADAPTOR, over host/mitsuba_adaptor.cpp and the stand-in Mitsuba headers:
//       normals_adaptor_harness <technique> <facenormals: 0|1>
//     One diffuse two-triangle mesh and one emitting one-triangle mesh, both with vertex normals, go through the plugin; the
//     stand-in for drmlt_node_create prints "shape <type> <emitter> <normals>" per shape, "normals <nine floats>" per table
//     entry and "size <struct_size> <n_normals>"; the log follows as "log <level> <text>".
#ifndef NORMALS_ADAPTOR

#include "scene_prep.h"

#include "drmlt_integrator.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static std::vector<float> read_floats(const std::string &path) {
    std::vector<float> v;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return v;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize((size_t) n / sizeof(float));
    if (fread(v.data(), sizeof(float), v.size(), f) != v.size()) v.clear();
    fclose(f);
    return v;
}

int main(int argc, char **argv) {
    drmlt_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg;
    cfg.type = DRMLT_TYPE_ORBITAL; cfg.max_depth = 8; cfg.rr_depth = 5; cfg.direct_samples = -1; cfg.luminance_samples = 100000;
    cfg.work_units = 1024; cfg.sample_count = 1; cfg.p_large = 0.3f; cfg.sigma = 1.0f / 64.0f; cfg.scale_second = 0.1f;
    cfg.average_luminance = -1.0f; cfg.kelemen_style_weights = 1; cfg.kelemen_style_mutation = 1;
    std::string scene_path, uv_path, out_path;
    for (int i = 1; i < argc; ++i) {
        const char *eq = strchr(argv[i], '=');
        if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
        const std::string key(argv[i], eq - argv[i]);
        const char *v = eq + 1;
        if (key.rfind("DRMLT_", 0) == 0) setenv(key.c_str(), v, 1);
        else if (key == "scene") scene_path = v;
        else if (key == "uv") uv_path = v;
        else if (key == "out") out_path = v;
        else if (key == "technique") cfg.technique = atoi(v);
        else { fprintf(stderr, "unknown key %s\n", key.c_str()); return 2; }
    }
    const drmlt_host::SceneFile sf = drmlt_host::SceneFile::load(scene_path);
    const drmlt_scene scene = sf.view();
    const Knobs K = read_knobs();
    PreparedScene S;
    const std::string refusal = prepare_scene(cfg, scene, K, S);
    if (!refusal.empty()) S = PreparedScene();

    if (refusal.empty() && !uv_path.empty()) {
        const std::vector<float> uv = read_floats(uv_path);
        if (uv.size() != 2 * (size_t) scene.n_shapes) { fprintf(stderr, "uv: expected two floats per shape\n"); return 2; }
        std::vector<float> out(9 * (size_t) scene.n_shapes, 0.f);
        for (int i = 0; i < scene.n_shapes; ++i) { // shading record i belongs to shape i (scene_prep.h: build_scene)
            const DShade &sh = S.shade[(size_t) i];
            if ((sh.bsdf >> 24) != PRIM_SMOOTH) continue;
            uint32_t index;
            memcpy(&index, &sh.n[0], sizeof index);
            index -= SMOOTH_INDEX_BIAS;
            if (index >= S.normals.size()) { fprintf(stderr, "shape %d: entry %u outside the table\n", i, index); return 2; }
            const SmoothFrame F = smooth_frame(S.normals[index], sh.eu[0] * sh.inv_len_eu, sh.eu[1] * sh.inv_len_eu, sh.eu[2] * sh.inv_len_eu, uv[2 * i], uv[2 * i + 1]); // as path_step calls it
            float *o = &out[9 * (size_t) i];
            o[0] = F.nx; o[1] = F.ny; o[2] = F.nz; o[3] = F.sx; o[4] = F.sy; o[5] = F.sz;
            o[6] = F.ny * F.sz - F.nz * F.sy; o[7] = F.nz * F.sx - F.nx * F.sz; o[8] = F.nx * F.sy - F.ny * F.sx; // cross3(n, s)
        }
        FILE *f = fopen(out_path.c_str(), "wb");
        if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { fprintf(stderr, "cannot write %s\n", out_path.c_str()); return 2; }
        fclose(f);
    }

    printf("{\"refusal\": \"");
    for (char c : refusal) { if (c == '"' || c == '\\') putchar('\\'); putchar(c); }
    printf("\", \"features\": %d, \"use_bvh\": %d, \"n_flat_rec\": %d, \"n_box\": %d, \"n_normals\": %zu, \"lds_table_bytes\": %d, \"prim_kinds\": [",
           S.P.features, S.P.use_bvh, S.P.n_flat_rec, S.P.n_box, S.normals.size(), (int) (S.plan.n_shade * sizeof(DShade)));
    for (size_t i = 0; i < S.prims.size(); ++i) printf("%s%d", i ? ", " : "", S.prims[i].type);
    printf("], \"shade_kinds\": [");
    for (size_t i = 0; i < S.shade.size(); ++i) printf("%s%d", i ? ", " : "", S.shade[i].bsdf >> 24);
    printf("], \"one_light\": %d}\n", scene_has_one_light(S.P) ? 1 : 0);
    return 0;
}

#else // NORMALS_ADAPTOR

#include <mitsuba/render/scene.h>

#include <cstdint>
#include <cstring>

#include "drmlt_abi.h"

using namespace mitsuba;

extern "C" void *CreateInstance(const Properties &props);

struct drmlt_ctx { int w, h; };
struct drmlt_node { int w, h; };
extern "C" {
drmlt_ctx *drmlt_create(const drmlt_config *, const drmlt_scene *sc, int, char *, size_t) { return new drmlt_ctx{sc->camera.width, sc->camera.height}; }
int drmlt_seed(drmlt_ctx *, uint64_t, uint32_t, double *b) { if (b) *b = 0.5; return DRMLT_OK; }
int drmlt_run(drmlt_ctx *, uint64_t, volatile int *, drmlt_progress_cb, void *) { return DRMLT_OK; }
int drmlt_develop(drmlt_ctx *c, const float *, float *out) { for (int i = 0; i < c->w * c->h * 3; ++i) out[i] = 0.5f; return DRMLT_OK; }
void drmlt_destroy(drmlt_ctx *c) { delete c; }
int drmlt_luminance_map(const float *, int, int, int W, int H, float *out) { for (int i = 0; i < W * H; ++i) out[i] = 2.0f; return DRMLT_OK; }
drmlt_node *drmlt_node_create(const drmlt_config *, const drmlt_scene *sc, uint32_t, char *, size_t) {
    for (int i = 0; i < sc->n_shapes; ++i) printf("shape %d %d %d\n", sc->shapes[i].type, sc->shapes[i].emitter, sc->shapes[i].normals);
    for (int i = 0; i < sc->n_normals; ++i) {
        printf("normals");
        for (int k = 0; k < 9; ++k) printf(" %.9g", sc->normals[9 * i + k]);
        printf("\n");
    }
    printf("size %u %d\n", sc->struct_size, sc->n_normals);
    return new drmlt_node{sc->camera.width, sc->camera.height};
}
int drmlt_node_set_importance_map(drmlt_node *, const float *) { return DRMLT_OK; }
int drmlt_node_seed(drmlt_node *, uint64_t, double *b) { *b = 0.125; return DRMLT_OK; }
int drmlt_node_run(drmlt_node *, uint64_t total, volatile int *, drmlt_progress_cb cb, void *user) { if (cb) cb(total, total, user); return DRMLT_OK; }
int drmlt_node_develop(drmlt_node *n, const float *, float *out) { for (int i = 0; i < n->w * n->h * 3; ++i) out[i] = 1.0f; return DRMLT_OK; }
int drmlt_node_render_direct(drmlt_node *n, int32_t, int32_t, uint64_t, float *out) { for (int i = 0; i < n->w * n->h * 3; ++i) out[i] = 0.0f; return DRMLT_OK; }
int drmlt_node_stats_get(drmlt_node *, drmlt_stats *s) { memset(s, 0, sizeof *s); s->mutations = 1; s->kernel_ms = 1.0; return DRMLT_OK; }
const char *drmlt_node_last_error(drmlt_node *) { return ""; }
void drmlt_node_destroy(drmlt_node *n) { delete n; }
}

static Class *named(const char *name, const Class *super) { return new Class(name, super); }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string technique = argv[1];
    const bool face_normals = atoi(argv[2]) != 0;

    Properties dp;
    dp.setSpectrum("reflectance", Spectrum(0.5, 0.5, 0.5));
    BSDF *grey = new BSDF(dp);
    grey->m_class = named("SmoothDiffuse", BSDF::m_theClass);

    Properties mp;
    if (face_normals) mp.setBoolean("faceNormals", true);
    ref<Scene> scene = new Scene();
    // a quad as a two-triangle mesh, four unnormalised vertex normals
    TriMesh *quad = new TriMesh();
    *const_cast<Properties *>(&quad->getProperties()) = mp;
    quad->m_pos = {Point(-1, -1, 0), Point(1, -1, 0), Point(1, 1, 0), Point(-1, 1, 0)};
    quad->m_tris = {Triangle{{0, 1, 2}}, Triangle{{2, 3, 0}}};
    quad->m_normals = {Normal(0.125, 0, 1), Normal(0, 0.25, 2), Normal(-0.5, 0, 0.75), Normal(0, -0.375, 1.5)};
    quad->m_class = named("ObjMesh", TriMesh::m_theClass);
    quad->m_bsdf = grey;
    quad->m_name = "quad";
    scene->m_shapes.push_back(quad);
    // an emitting triangle with vertex normals
    TriMesh *lamp = new TriMesh();
    *const_cast<Properties *>(&lamp->getProperties()) = mp;
    lamp->m_pos = {Point(-0.5, -0.5, 2), Point(0.5, -0.5, 2), Point(0, 0.5, 2)};
    lamp->m_tris = {Triangle{{0, 2, 1}}};
    lamp->m_normals = {Normal(0, 0.0625, -1), Normal(0.03125, 0, -1), Normal(0, 0, -3)};
    lamp->m_class = named("ObjMesh", TriMesh::m_theClass);
    lamp->m_bsdf = grey;
    lamp->m_name = "lamp";
    Properties ep;
    ep.setSpectrum("radiance", Spectrum(1.0, 1.0, 1.0));
    Emitter *em = new Emitter(ep);
    em->m_class = named("AreaLight", ConfigurableObject::m_theClass);
    lamp->m_emitter = em;
    scene->m_shapes.push_back(lamp);

    ref<PerspectiveCamera> camera = new PerspectiveCamera();
    Matrix4x4 m;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = r == c ? 1.0 : 0.0;
    m(2, 3) = 5.0; m(2, 2) = -1.0; m(0, 0) = -1.0;
    camera->m_toWorld = Transform(m);
    camera->m_xfov = 40.0; camera->m_nearClip = 1e-2; camera->m_farClip = 1e4;
    ref<Film> film = new Film();
    film->m_cropSize = Vector2i(8, 8);
    ref<ReconstructionFilter> rf = new ReconstructionFilter();
    rf->m_radius = 0.5 + 1e-5f;
    rf->m_class = named("BoxFilter", ConfigurableObject::m_theClass);
    Properties fp;
    fp.setFloat("radius", 0.5);
    *const_cast<Properties *>(&rf->getProperties()) = fp;
    film->m_filter = rf;
    camera->m_film = film;
    ref<Sampler> sampler = new Sampler();
    sampler->m_sampleCount = 4;
    camera->m_sampler = sampler;
    scene->m_sensor = camera.get();

    Properties iprops;
    iprops.setString("technique", technique);
    iprops.setString("type", "orbital");
    iprops.setInteger("maxDepth", 6);
    iprops.setInteger("directSamples", -1);
    iprops.setInteger("sampleCount", 4);
    iprops.setInteger("workUnits", 64);
    iprops.setInteger("seed", 1);
    ref<RenderQueue> queue = new RenderQueue();
    ref<RenderJob> job = new RenderJob();
    int rc = 0;
    try {
        ref<Integrator> integrator = static_cast<Integrator *>(CreateInstance(iprops));
        integrator->preprocess(scene, queue, job, 0, 1, 2);
        integrator->render(scene, queue, job, 0, 1, 2);
    } catch (const std::exception &e) {
        rc = 1;
    }
    for (auto &l : FakeLog::lines()) printf("log %d %s\n", l.first, l.second.c_str());
    return rc;
}

#endif
