// The adaptor's mapping of Mitsuba's SmoothConductor (host/mitsuba_adaptor.cpp: bsdfIndex), without a GPU: one emitting
// rectangle and one rectangle that carries a fake SmoothConductor go through the plugin surface; the stand-in for
// drmlt_node_create prints every drmlt_bsdf the plugin hands over as "bsdf <type> <rgb x 3> <p x 8>".
//   conductor_harness none                         material = "none"
//   conductor_harness explicit                     eta = (0.2, 0.9, 1.1), k = (3.9, 2.4, 2.1), extEta = 2, reflectance (0.9, 0.6, 0.3)
//   conductor_harness material <name> <prefix>     a named material, read through the FileResolver prefix
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
    for (int i = 0; i < sc->n_bsdfs; ++i) {
        const drmlt_bsdf &b = sc->bsdfs[i];
        printf("bsdf %d %.9g %.9g %.9g", b.type, b.rgb[0], b.rgb[1], b.rgb[2]);
        for (int k = 0; k < 8; ++k) printf(" %.9g", b.p[k]);
        printf("\n");
    }
    return new drmlt_node{sc->camera.width, sc->camera.height};
}
int drmlt_node_set_importance_map(drmlt_node *, const float *) { return DRMLT_OK; }
int drmlt_node_seed(drmlt_node *, uint64_t, double *b) { *b = 0.125; return DRMLT_OK; }
int drmlt_node_run(drmlt_node *, uint64_t total, volatile int *, drmlt_progress_cb cb, void *user) { if (cb) cb(total, total, user); return DRMLT_OK; }
int drmlt_node_develop(drmlt_node *n, const float *, float *out) { for (int i = 0; i < n->w * n->h * 3; ++i) out[i] = 1.0f; return DRMLT_OK; }
int drmlt_node_stats_get(drmlt_node *, drmlt_stats *s) { memset(s, 0, sizeof *s); s->mutations = 1; s->kernel_ms = 1.0; return DRMLT_OK; }
const char *drmlt_node_last_error(drmlt_node *) { return ""; }
void drmlt_node_destroy(drmlt_node *n) { delete n; }
}

static Class *named(const char *name, const Class *super) { return new Class(name, super); }

static ref<Shape> rectangle(double y, BSDF *bsdf) {
    Properties p;
    Matrix4x4 m;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = r == c ? 1.0 : 0.0;
    m(1, 3) = y;
    p.setTransform("toWorld", Transform(m));
    ref<Shape> sh = new Shape(p);
    sh->m_class = named("Rectangle", Shape::m_theClass);
    sh->m_bsdf = bsdf;
    return sh;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    Properties cp;
    if (mode == "none") cp.setString("material", "none");
    else if (mode == "explicit") {
        cp.setSpectrum("eta", Spectrum(0.2, 0.9, 1.1));
        cp.setSpectrum("k", Spectrum(3.9, 2.4, 2.1));
        cp.setFloat("extEta", 2.0);
        cp.setSpectrum("specularReflectance", Spectrum(0.9, 0.6, 0.3));
    } else if (mode == "material" && argc >= 4) {
        cp.setString("material", argv[2]);
        cp.setFloat("extEta", 1.0);
        FileResolver::prefix() = argv[3];
    } else return 2;
    BSDF *mirror = new BSDF(cp);
    mirror->m_class = named("SmoothConductor", BSDF::m_theClass);
    Properties dp;
    dp.setSpectrum("reflectance", Spectrum(0.0, 0.0, 0.0));
    BSDF *black = new BSDF(dp);
    black->m_class = named("SmoothDiffuse", BSDF::m_theClass);

    ref<Scene> scene = new Scene();
    scene->m_shapes.push_back(rectangle(0.0, mirror));
    ref<Shape> light = rectangle(1.0, black);
    Properties ep;
    ep.setSpectrum("radiance", Spectrum(1.0, 1.0, 1.0));
    Emitter *em = new Emitter(ep);
    em->m_class = named("AreaLight", ConfigurableObject::m_theClass);
    light->m_emitter = em;
    scene->m_shapes.push_back(light);

    ref<PerspectiveCamera> camera = new PerspectiveCamera();
    Matrix4x4 m;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = r == c ? 1.0 : 0.0;
    m(2, 3) = -3.0;
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
    iprops.setString("technique", "path");
    iprops.setString("type", "orbital");
    iprops.setInteger("maxDepth", 6);
    iprops.setInteger("directSamples", -1);
    iprops.setInteger("sampleCount", 4);
    iprops.setInteger("workUnits", 64);
    iprops.setInteger("seed", 1);
    ref<RenderQueue> queue = new RenderQueue();
    ref<RenderJob> job = new RenderJob();
    try {
        ref<Integrator> integrator = static_cast<Integrator *>(CreateInstance(iprops));
        integrator->preprocess(scene, queue, job, 0, 1, 2);
        integrator->render(scene, queue, job, 0, 1, 2);
    } catch (const std::exception &e) {
        for (auto &l : FakeLog::lines()) fprintf(stderr, "%d\t%s\n", l.first, l.second.c_str());
        return 1;
    }
    return 0;
}
