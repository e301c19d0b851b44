// Drives drmlt-mitsuba_amd/host/mitsuba_adaptor.cpp (compiled against tests/native/fake_mitsuba_emitters/) on scenes whose emitters no
// shape carries -- Mitsuba's `point` and `constant` plugins, and one the backend refuses -- and on the directPass property.
// Modelled on adaptor_harness.cpp: the scene is rebuilt from a flat scene file (SceneData.save of scenes.py) as Mitsuba
// objects, and the plugin is driven CreateInstance(props) -> preprocess -> render.
//
//   adaptor_emitters_harness <scene.bin> <out prefix> [--free-first] [--spot] [--unserialize] [-D key=value ...]
//
// Scene::m_emitters is filled in the order of the file's emitters: an AreaLight knows its shape (Emitter::getShape), a point
// light becomes a PointEmitter, the environment a ConstantBackgroundEmitter.
//   --free-first   the emitters that no shape carries come first, in their own order: where Mitsuba's XML loader leaves them
//                  (scene.cpp:547-567 against :621-622)
//   --spot         one SpotEmitter is appended
//   --unserialize  the instance that renders is a second one, made from the first one's serialize() output (<prefix>.ser)
// <prefix>.tostring holds toString() of the instance that renders.
//
// The adaptor is part of this translation unit, so that DRMLT(Stream *, InstanceManager *) can be named. Built twice by
// drmlt-mitsuba_amd/host/Makefile:
//   -DMOCK_ABI  the drmlt_* entry points are defined HERE and record what the adaptor hands over, all in the scene-file format
//               that SceneFile::load and SceneData.load read (point and normal blocks included):
//                 <prefix>.scene        the drmlt_scene given to drmlt_node_create, <prefix>.meta its struct_size, sizeof(drmlt_scene),
//                                       n_points and n_normals, <prefix>.cfg the drmlt_config bytes
//                 <prefix>.first.scene  the one given to drmlt_create (the first stage of twoStage), with its .meta
//                 <prefix>.direct       one line per drmlt_node_render_direct call: direct_samples hide_emitters seed
//               drmlt_node_create answers with the library's own scene checks (csrc/scene_prep.h: prepare_scene, host code);
//   (default)   linked with libdrmlt_amd.so: a real render through the plugin surface (<prefix>.img = W*H*3 floats).
// Log lines go to <prefix>.log as "<level>\t<text>".
#include "../../drmlt-mitsuba_amd/host/mitsuba_adaptor.cpp"

#include <cstdint>
#include <cstdlib>

#include "drmlt_integrator.hpp"

static std::string g_prefix;

#ifdef MOCK_ABI
#include "scene_prep.h"

// ------------------------------------------------------------------ a recording stand-in for libdrmlt_amd.so
struct drmlt_ctx { int w, h; };
struct drmlt_node { int w, h; std::string err; };
static void dump_scene(const std::string &path, const drmlt_scene *sc) {
    FILE *f = fopen(path.c_str(), "wb");
    uint32_t hdr[8] = {0x4C4D5244u, DRMLT_ABI_VERSION, (uint32_t) sc->n_shapes, (uint32_t) sc->n_bsdfs, (uint32_t) sc->n_emitters,
                       (uint32_t) sizeof(drmlt_shape), (uint32_t) sizeof(drmlt_bsdf), (uint32_t) sizeof(drmlt_emitter)};
    fwrite(hdr, sizeof hdr, 1, f);
    fwrite(sc->shapes, sizeof(drmlt_shape), sc->n_shapes, f);
    fwrite(sc->bsdfs, sizeof(drmlt_bsdf), sc->n_bsdfs, f);
    fwrite(sc->emitters, sizeof(drmlt_emitter), sc->n_emitters, f);
    fwrite(&sc->camera, sizeof sc->camera, 1, f);
    if (sc->n_points > 0 && sc->points) {
        uint32_t blk[2] = {drmlt_host::SceneFile::POINTS_TAG, (uint32_t) sc->n_points};
        fwrite(blk, sizeof blk, 1, f);
        fwrite(sc->points, sizeof(float), (size_t) sc->n_points * 3, f);
    }
    if (sc->n_normals > 0 && sc->normals) {
        uint32_t blk[2] = {drmlt_host::SceneFile::NORMALS_TAG, (uint32_t) sc->n_normals};
        fwrite(blk, sizeof blk, 1, f);
        fwrite(sc->normals, sizeof(float), (size_t) sc->n_normals * 9, f);
    }
    fclose(f);
    f = fopen((path + ".meta").c_str(), "w");
    fprintf(f, "%u %zu %d %d\n", sc->struct_size, sizeof(drmlt_scene), sc->n_points, sc->n_normals);
    fclose(f);
}
extern "C" {
drmlt_ctx *drmlt_create(const drmlt_config *, const drmlt_scene *sc, int, char *, size_t) {
    dump_scene(g_prefix + ".first.scene", sc);
    return new drmlt_ctx{sc->camera.width, sc->camera.height};
}
int drmlt_seed(drmlt_ctx *, uint64_t, uint32_t, double *b) { if (b) *b = 0.5; return DRMLT_OK; }
int drmlt_run(drmlt_ctx *, uint64_t, volatile int *, drmlt_progress_cb, void *) { return DRMLT_OK; }
int drmlt_develop(drmlt_ctx *c, const float *, float *out) { for (int i = 0; i < c->w * c->h * 3; ++i) out[i] = 0.5f; return DRMLT_OK; }
void drmlt_destroy(drmlt_ctx *c) { delete c; }
int drmlt_luminance_map(const float *, int, int, int W, int H, float *out) { for (int i = 0; i < W * H; ++i) out[i] = 2.0f; return DRMLT_OK; }
drmlt_node *drmlt_node_create(const drmlt_config *cfg, const drmlt_scene *sc, uint32_t, char *err, size_t errlen) {
    dump_scene(g_prefix + ".scene", sc);
    FILE *f = fopen((g_prefix + ".cfg").c_str(), "wb");
    fwrite(cfg, sizeof *cfg, 1, f);
    fclose(f);
    PreparedScene prepared;
    const std::string refusal = prepare_scene(*cfg, *sc, read_knobs(), prepared);
    if (!refusal.empty()) { snprintf(err, errlen, "%s", refusal.c_str()); return nullptr; }
    return new drmlt_node{sc->camera.width, sc->camera.height, ""};
}
int drmlt_node_set_importance_map(drmlt_node *, const float *) { return DRMLT_OK; }
int drmlt_node_seed(drmlt_node *, uint64_t, double *b) { *b = 0.125; return DRMLT_OK; }
int drmlt_node_run(drmlt_node *, uint64_t total, volatile int *, drmlt_progress_cb cb, void *user) { if (cb) cb(total, total, user); return DRMLT_OK; }
int drmlt_node_render_direct(drmlt_node *n, int32_t direct_samples, int32_t hide_emitters, uint64_t seed, float *out) {
    FILE *f = fopen((g_prefix + ".direct").c_str(), "a");
    fprintf(f, "%d %d %llu\n", direct_samples, hide_emitters, (unsigned long long) seed);
    fclose(f);
    for (int i = 0; i < n->w * n->h * 3; ++i) out[i] = 0.375f; // the full frame; not the host pass's 0.25
    return DRMLT_OK;
}
int drmlt_node_develop(drmlt_node *n, const float *direct, float *out) {
    for (int i = 0; i < n->w * n->h * 3; ++i) out[i] = 1.0f + (direct ? direct[i] : 0.f);
    return DRMLT_OK;
}
int drmlt_node_stats_get(drmlt_node *, drmlt_stats *s) { memset(s, 0, sizeof *s); s->kernel_ms = 1.0; return DRMLT_OK; }
const char *drmlt_node_last_error(drmlt_node *n) { return n->err.c_str(); }
void drmlt_node_destroy(drmlt_node *n) { delete n; }
}
#endif

// ------------------------------------------------------------------ flat scene file -> Mitsuba objects
static mitsuba::Class *named(const char *name, const mitsuba::Class *super) { return new mitsuba::Class(name, super); }

int main(int argc, char **argv) {
    using namespace mitsuba;
    if (argc < 3) return 2;
    g_prefix = argv[2];
    bool free_first = false, spot = false, unserialize = false;
    Properties iprops;
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--free-first") free_first = true;
        else if (a == "--spot") spot = true;
        else if (a == "--unserialize") unserialize = true;
        else if (a == "-D" && i + 1 < argc) {
            std::string kv = argv[++i], k = kv.substr(0, kv.find('=')), v = kv.substr(kv.find('=') + 1);
            char *end = nullptr;
            long iv = strtol(v.c_str(), &end, 10);
            if (v == "true" || v == "false") iprops.setBoolean(k, v == "true");
            else if (*end == 0 && !v.empty()) iprops.setInteger(k, (int) iv);
            else { double dv = strtod(v.c_str(), &end); if (*end == 0 && !v.empty()) iprops.setFloat(k, dv); else iprops.setString(k, v); }
        } else return 2;
    }
    drmlt_host::SceneFile sf;
    try { sf = drmlt_host::SceneFile::load(argv[1]); }
    catch (const std::exception &e) { fprintf(stderr, "%s\n", e.what()); return 2; }

    ref<Scene> scene = new Scene();
    std::vector<size_t> shape_of(sf.shapes.size()); // file record -> Mitsuba shape
    for (size_t i = 0; i < sf.shapes.size(); ++i) {
        const drmlt_shape &s = sf.shapes[i];
        shape_of[i] = scene->m_shapes.size();
        // a run of plain triangles of one material is one mesh, as a `cube` or an .obj file is in Mitsuba: the plugin then
        // gives them one BSDF record, as scenes.py does
        if (i > 0 && s.type == DRMLT_SHAPE_TRIANGLE && sf.shapes[i - 1].type == DRMLT_SHAPE_TRIANGLE && s.bsdf == sf.shapes[i - 1].bsdf &&
            s.emitter < 0 && sf.shapes[i - 1].emitter < 0 && s.normals == 0 && sf.shapes[i - 1].normals == 0) {
            TriMesh *mesh = static_cast<TriMesh *>(scene->m_shapes.back().get());
            const uint32_t v0 = (uint32_t) mesh->m_pos.size();
            for (int v = 0; v < 3; ++v) mesh->m_pos.push_back(Point(s.data[3 * v], s.data[3 * v + 1], s.data[3 * v + 2]));
            mesh->m_tris.push_back(Triangle{{v0, v0 + 1, v0 + 2}});
            shape_of[i] = scene->m_shapes.size() - 1;
            continue;
        }
        ref<Shape> sh;
        if (s.normals != 0) { fprintf(stderr, "this harness builds no vertex normals\n"); return 2; }
        if (s.type == DRMLT_SHAPE_RECTANGLE) {
            Properties p;
            Matrix4x4 m;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m(r, c) = s.data[r * 4 + c];
            p.setTransform("toWorld", Transform(m));
            sh = new Shape(p);
            sh->m_class = named("Rectangle", Shape::m_theClass);
        } else if (s.type == DRMLT_SHAPE_SPHERE) {
            sh = new Shape(Properties());
            sh->m_class = named("Sphere", Shape::m_theClass);
            sh->m_aabb.min = Point(s.data[0] - s.data[3], s.data[1] - s.data[3], s.data[2] - s.data[3]);
            sh->m_aabb.max = Point(s.data[0] + s.data[3], s.data[1] + s.data[3], s.data[2] + s.data[3]);
        } else {
            TriMesh *mesh = new TriMesh();
            for (int v = 0; v < 3; ++v) mesh->m_pos.push_back(Point(s.data[3 * v], s.data[3 * v + 1], s.data[3 * v + 2]));
            mesh->m_tris.push_back(Triangle{{0, 1, 2}});
            mesh->m_class = named("ObjMesh", TriMesh::m_theClass);
            sh = mesh;
        }
        const drmlt_bsdf &b = sf.bsdfs[s.bsdf];
        Properties bp;
        if (b.type == DRMLT_BSDF_DIFFUSE) bp.setSpectrum("reflectance", Spectrum(b.rgb[0], b.rgb[1], b.rgb[2]));
        else if (b.type == DRMLT_BSDF_DIELECTRIC) { bp.setFloat("intIOR", b.p[0]); bp.setFloat("extIOR", b.p[1]); }
        else { fprintf(stderr, "this harness builds diffuse and dielectric materials only\n"); return 2; }
        sh->m_bsdf = new BSDF(bp);
        sh->m_bsdf->m_class = named(b.type == DRMLT_BSDF_DIFFUSE ? "SmoothDiffuse" : "SmoothDielectric", BSDF::m_theClass);
        scene->m_shapes.push_back(sh);
    }
    std::vector<ref<Emitter>> carried, freed; // in the file's order
    std::vector<bool> is_free;
    for (const drmlt_emitter &e : sf.emitters) {
        Properties p;
        p.setFloat("samplingWeight", e.sampling_weight);
        const Spectrum value(e.radiance[0], e.radiance[1], e.radiance[2]);
        is_free.push_back(e.type != DRMLT_EMITTER_AREA);
        if (e.type == DRMLT_EMITTER_AREA) {
            p.setSpectrum("radiance", value);
            ref<Emitter> o = new Emitter(p);
            o->m_class = named("AreaLight", ConfigurableObject::m_theClass);
            o->m_shape = scene->m_shapes[shape_of[e.shape]].get();
            o->m_shape->m_emitter = o;
            carried.push_back(o);
        } else if (e.type == DRMLT_EMITTER_POINT) {
            p.setSpectrum("intensity", value);
            Matrix4x4 m;
            for (int r = 0; r < 3; ++r) m(r, 3) = sf.points[3 * e.shape + r];
            p.setTransform("toWorld", Transform(m));
            freed.push_back(new PointEmitter(p));
        } else {
            p.setSpectrum("radiance", value);
            freed.push_back(new ConstantBackgroundEmitter(p));
        }
    }
    if (spot) { is_free.push_back(true); freed.push_back(new SpotEmitter(Properties())); }
    if (free_first) {
        for (auto &o : freed) scene->m_emitters.push_back(o);
        for (auto &o : carried) scene->m_emitters.push_back(o);
    } else {
        size_t c = 0, f = 0;
        for (bool fr : is_free) scene->m_emitters.push_back(fr ? freed[f++] : carried[c++]);
    }

    const drmlt_camera &cam = sf.camera;
    ref<PerspectiveCamera> camera = new PerspectiveCamera();
    Matrix4x4 m;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) m(r, c) = cam.to_world[r * 4 + c];
    camera->m_toWorld = Transform(m);
    camera->m_xfov = cam.fov_x_deg; camera->m_nearClip = cam.near_clip; camera->m_farClip = cam.far_clip;
    ref<Film> film = new Film();
    film->m_cropSize = Vector2i(cam.width, cam.height);
    Properties fp;
    ref<ReconstructionFilter> rf = new ReconstructionFilter();
    if (cam.filter == DRMLT_FILTER_BOX) { fp.setFloat("radius", cam.filter_param); rf->m_radius = cam.filter_param + 1e-5f; rf->m_class = named("BoxFilter", ConfigurableObject::m_theClass); }
    else { fp.setFloat("stddev", cam.filter_param); rf->m_radius = 4 * cam.filter_param; rf->m_class = named("GaussianFilter", ConfigurableObject::m_theClass); }
    *const_cast<Properties *>(&rf->getProperties()) = fp;
    film->m_filter = rf;
    camera->m_film = film;
    ref<Sampler> sampler = new Sampler();
    sampler->m_sampleCount = (size_t) iprops.getInteger("sampleCount", 4);
    camera->m_sampler = sampler;
    scene->m_sensor = camera.get();

    int rc = 0;
    ref<RenderQueue> queue = new RenderQueue();
    ref<RenderJob> job = new RenderJob();
    try {
        ref<Integrator> integrator = static_cast<Integrator *>(CreateInstance(iprops));
        if (unserialize) { // Integrator(Stream *, InstanceManager *) / serialize: what the scheduler does with remote workers
            Stream st;
            integrator->serialize(&st, nullptr);
            FILE *g = fopen((g_prefix + ".ser").c_str(), "wb"); fwrite(st.buf.data(), 1, st.buf.size(), g); fclose(g);
            integrator = new DRMLT(&st, nullptr);
        }
        FILE *g = fopen((g_prefix + ".tostring").c_str(), "w"); fputs(integrator->toString().c_str(), g); fclose(g);
        integrator->preprocess(scene, queue, job, 0, 1, 2);
        const bool done = integrator->render(scene, queue, job, 0, 1, 2);
        FakeLog::log(EInfo, "render returned %s, %d refresh signal(s), %d direct pass sample(s)", done ? "true" : "false", queue->refreshes, BidirectionalUtils::calls());
        if (done) {
            g = fopen((g_prefix + ".img").c_str(), "wb");
            fwrite(film->m_result.data(), sizeof(float), film->m_result.size(), g);
            fclose(g);
        }
    } catch (const std::exception &e) {
        rc = 1; // Log(EError) of the plugin
    }
    FILE *f = fopen((g_prefix + ".log").c_str(), "w");
    for (auto &l : FakeLog::lines()) fprintf(f, "%d\t%s\n", l.first, l.second.c_str());
    fclose(f);
    return rc;
}
