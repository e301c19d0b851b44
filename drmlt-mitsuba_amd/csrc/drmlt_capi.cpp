// C-ABI of the MI355X-native DRMLT hot path (include/drmlt_abi.h): context management,
// scene flattening, bootstrap/seeding host logic and kernel orchestration. Everything that
// touches path evaluation runs in the HIP kernels of kernels.hip; there is no CPU fallback.
#include "../../include/drmlt_abi.h"
#include "device_types.h"
#include "drmlt_ctx.h"
#include "scene_prep.h"
#include "bdpt_layers.h"
#include "pt_layers.h"
#include "seed_select.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// launchers defined in kernels.hip
void launch_bootstrap(const DParams &P, uint32_t n, float *lum_out, hipStream_t st);
void launch_init_chains(const DParams &P, const uint32_t *seed_index, const float *seed_lum, hipStream_t st);
void launch_mutate(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st); // technique=path, both algorithms
void launch_eval_paths(const DParams &P, const float *u, uint32_t n, uint32_t dim, float *out8, hipStream_t st);
// technique=mmlt (kernels_mmlt.hip)
// (`lds`: ChainPlan::aux_lds)
void launch_bootstrap_mmlt(const DParams &P, uint32_t n, float *lum_out, size_t lds, hipStream_t st);
void launch_init_chains_mmlt(const DParams &P, const uint32_t *seed_index, const float *seed_lum, size_t lds, hipStream_t st);
void launch_mutate_mmlt(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_eval_paths_mmlt(const DParams &P, const float *u, uint32_t n, uint32_t dim, float *out8, size_t lds, hipStream_t st);
// technique=mmlt's reference renders (kernels_render_mmlt.hip); `film` / `layers` are fp64
uint32_t render_mmlt_grid(uint32_t n);
void launch_render_mmlt(const DParams &P, uint32_t n, float scale, double *film, size_t lds, hipStream_t st);
void launch_layers_mmlt(const DParams &P, uint32_t n, float scale, double *layers, int unweighted, size_t lds, hipStream_t st);
void launch_regroup(const uint32_t *work, const int32_t *depth_or_null, uint32_t n, uint32_t n_mut, uint32_t md, uint32_t *order, uint32_t padded, uint32_t *scratch, hipStream_t st);
size_t regroup_scratch_words(uint32_t n, uint32_t md);
// technique=bdpt (kernels_bdpt.hip)
void launch_bootstrap_bdpt(const DParams &P, uint32_t n, float *lum_out, size_t lds, hipStream_t st);
void launch_init_chains_bdpt(const DParams &P, const uint32_t *seed_index, const float *seed_lum, size_t lds, hipStream_t st);
void launch_mutate_bdpt(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_eval_lists_bdpt(const DParams &P, const float *u, uint32_t n, uint32_t dim, float *out, uint32_t stride, size_t lds, hipStream_t st);
// algo=pssmlt over technique=bdpt (kernels_pssmlt_bdpt.hip); bootstrap, seed replay and evaluation are technique=bdpt's
void launch_mutate_pssmlt_bdpt(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_render_pt(const DParams &P, uint64_t n_samples, uint32_t stream, float scale, hipStream_t st);
// independent bidirectional samples into a film (kernels_render_bdpt.hip)
void launch_render_bdpt(const DParams &P, uint32_t n, float scale, size_t lds, hipStream_t st);
// ... split by path length and strategy into a layered film (kernels_layers_bdpt.hip)
void launch_layers_bdpt(const DParams &P, uint32_t n, float scale, float *layers, int unweighted, size_t lds, hipStream_t st);
// technique=path's independent samples split by path length and strategy (kernels_layers_pt.hip)
void launch_render_pt_layers(const DParams &P, uint32_t n, float scale, double *layers, int unweighted, hipStream_t st);
// the direct-illumination pass (kernels_direct.hip)
uint32_t direct_grid(const DirectJob &J, int width);
void launch_render_direct(const DParams &P, const DirectJob &J, float *out, hipStream_t st);
// seed selection on the device (kernels_seed.hip)
size_t seed_workspace_bytes(uint32_t n);
hipError_t launch_seed_select(const float *lum, const float *wts, uint32_t n, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t n_select, uint32_t slice_lo,
                              uint32_t slice_n, void *work, uint32_t *out_index, float *out_lum, const double **sums_out, hipStream_t st);

namespace {

constexpr uint32_t TAG_SEEDSEL = 1;

// host Philox4x32-10 (seed selection draws; same function as device_math.h)
void philox_host(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]) {
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t) p1, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t) p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

} // namespace

drmlt_ctx::~drmlt_ctx() {
    if (comm) drmlt_comm_release(comm);
    if (own_stream && stream) (void) hipStreamDestroy(stream);
}

namespace {

// Overflow area of the traversal stacks (deep trees only): [ovf_entries][lanes of the launch] ints. Grown on demand before a
// launch whose grid has more lanes than any before it; `P` is the parameter block the launch will use.
static hipError_t ensure_overflow(drmlt_ctx *ctx, DParams &P, size_t lanes) {
    if (ctx->ovf_entries == 0) { P.bvh_overflow = nullptr; P.bvh_ovf_lanes = 0; return hipSuccess; }
    lanes = (lanes + 63) / 64 * 64;
    if (lanes > ctx->ovf_lanes) {
        hipError_t e = hipStreamSynchronize(ctx->stream); // a launch in flight may still be using the old area
        if (e != hipSuccess) return e;
        e = ctx->d_ovf.alloc((size_t) ctx->ovf_entries * lanes * sizeof(int32_t));
        if (e != hipSuccess) { ctx->ovf_lanes = 0; return e; }
        ctx->ovf_lanes = lanes;
    }
    ctx->P.bvh_overflow = P.bvh_overflow = ctx->d_ovf.as<int32_t>();
    ctx->P.bvh_ovf_lanes = P.bvh_ovf_lanes = (uint32_t) ctx->ovf_lanes;
    return hipSuccess;
}

} // namespace

extern "C" {

uint32_t drmlt_abi_version(void) { return DRMLT_ABI_VERSION; }

const char *drmlt_last_error(drmlt_ctx *ctx) { return ctx ? ctx->error.c_str() : "null context"; }

drmlt_ctx *drmlt_create(const drmlt_config *cfg, const drmlt_scene *scene, int device, char *err, size_t errlen) {
    auto bail = [&](drmlt_ctx *c, const std::string &msg) -> drmlt_ctx * {
        if (err && errlen) snprintf(err, errlen, "%s", msg.c_str());
        delete c;
        return nullptr;
    };
    if (!cfg || !scene) return bail(nullptr, "null config or scene");
    if (cfg->struct_size != sizeof(drmlt_config) || (scene->struct_size != sizeof(drmlt_scene) && scene->struct_size != DRMLT_SCENE_SIZE_NO_NORMALS && scene->struct_size != DRMLT_SCENE_SIZE_NO_POINTS))
        return bail(nullptr, "struct_size mismatch (ABI version skew)");
    // a scene that ends at `camera` has no point lights: nothing behind `camera` is read (its tail padding is where n_points lies);
    // one that ends at `points` has no vertex normals, and neither reads drmlt_shape.normals: to those callers it is `reserved`
    drmlt_scene scene_in;
    memset(&scene_in, 0, sizeof scene_in);
    memcpy(&scene_in, scene, scene->struct_size == sizeof(drmlt_scene) ? sizeof(drmlt_scene) : scene->struct_size == DRMLT_SCENE_SIZE_NO_NORMALS ? (size_t) DRMLT_SCENE_SIZE_NO_NORMALS : offsetof(drmlt_scene, camera) + sizeof(drmlt_camera));
    std::vector<drmlt_shape> shapes_in;
    if (scene->struct_size != sizeof(drmlt_scene) && scene->shapes && scene->n_shapes > 0) {
        shapes_in.assign(scene->shapes, scene->shapes + scene->n_shapes);
        for (drmlt_shape &sh : shapes_in) sh.normals = 0;
        scene_in.shapes = shapes_in.data();
    }
    scene = &scene_in;
    // ---- parameter checks of the DRMLT ctor / PathSampler ctor (drmlt.cpp:193-349, pathsampler.cpp:57-71)
    if (cfg->algo != DRMLT_ALGO_DRMLT && cfg->algo != DRMLT_ALGO_PSSMLT) return bail(nullptr, "Unknown algorithm");
    if (cfg->algo == DRMLT_ALGO_PSSMLT && cfg->technique == DRMLT_TECH_MMLT)
        return bail(nullptr, "algo=pssmlt runs over technique=path (BASELINE config 1) and technique=bdpt on the device, not over technique=mmlt");
    if (cfg->technique != DRMLT_TECH_PATH && cfg->technique != DRMLT_TECH_BDPT && cfg->technique != DRMLT_TECH_MMLT)
        return bail(nullptr, "Unknown technique type");
    if (cfg->type < DRMLT_TYPE_GREEN || cfg->type > DRMLT_TYPE_ORBITAL) return bail(nullptr, "Unknown implementation type");
    if (cfg->technique == DRMLT_TECH_MMLT && cfg->max_depth == -1) return bail(nullptr, "Impossible to use MMLT with no max depth");
    if (cfg->fix_emitter_path && cfg->technique != DRMLT_TECH_MMLT) return bail(nullptr, "Impossible to use fixEmitterPath without MMLT");
    if (cfg->scale_second > 1.0f) return bail(nullptr, "scaleSecond is bigger than the first stage");
    if (cfg->seed_rule != DRMLT_SEED_TARGET && cfg->seed_rule != DRMLT_SEED_REFERENCE) return bail(nullptr, "Unknown seeding rule (firstStageSeeding: target | reference)");
    if (cfg->work_units_rule != DRMLT_WORK_UNITS_DEVICE && cfg->work_units_rule != DRMLT_WORK_UNITS_REFERENCE) return bail(nullptr, "Unknown work-unit rule (workUnitsRule: device | reference)");
    const bool mmlt = cfg->technique == DRMLT_TECH_MMLT, bdpt = cfg->technique == DRMLT_TECH_BDPT;
    // (timidAfterLarge under bdpt: the reference's code path with its debug assertions compiled out -- a rejected large step's second
    // stage draws uniforms again for all three samplers, drmlt_sampler.cpp:319-321 -- as for technique=path, DESIGN deviation 2)
    // a wave's sampler and density rows (device_bdpt.h) take 60.7 KB of LDS at maxDepth 24 and pass the 64 KB of a workgroup at 26
    if (bdpt && cfg->max_depth > BDPT_MAX_DEPTH) return bail(nullptr, "technique=bdpt: maxDepth above 24 is not supported on the device");
    // ... and a vertex record packs its bsdf and emitter numbers into one word (device_bdpt.h: BR_IDS)
    if (bdpt && (scene->n_bsdfs > 4096 || scene->n_emitters > 65534)) return bail(nullptr, "technique=bdpt: more than 4096 bsdfs or 65534 emitters are not supported on the device");
    if (cfg->max_depth <= 0) return bail(nullptr, "technique=path needs a finite maxDepth (pssmlt_utils.h:63)");
    if (mmlt && cfg->max_depth > 24) return bail(nullptr, "technique=mmlt: maxDepth above 24 is not supported on the device");
    // a rejected large step re-draws the strategy; its second stage would read an emitter state that may be
    // empty (drmlt_sampler.cpp:189-191 with an unused emitter sampler): undefined in the reference, refused here
    if (mmlt && cfg->timid_after_large) return bail(nullptr, "timidAfterLarge is not defined for technique=mmlt");
    if (cfg->sample_count <= 0) return bail(nullptr, "sample_count must be positive");
    if (!(cfg->p_large >= 0.f && cfg->p_large <= 1.f)) return bail(nullptr, "pLarge must be in [0,1]");

    // ---- everything the scene and the configuration decide without a device (scene_prep.h): a refusal returns before any HIP call
    const Knobs K = read_knobs();
    PreparedScene prep;
    const std::string refusal = prepare_scene(*cfg, *scene, K, prep);
    if (!refusal.empty()) return bail(nullptr, refusal);

    drmlt_ctx *ctx = new drmlt_ctx();
    ctx->cfg = *cfg;
    ctx->device = device;
    ctx->knobs = K;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return bail(ctx, "no HIP device available (the DRMLT kernels have no CPU fallback)");
    if (device < 0 || device >= ndev) return bail(ctx, "invalid device index");
    if (hipSetDevice(device) != hipSuccess) return bail(ctx, "hipSetDevice failed");
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return bail(ctx, "hipStreamCreate failed");
    ctx->own_stream = true;
    // ---- chain count (workUnits = -1: derive_chains) and the chain kernel's build (launch_plan.h), chosen once
    PlanInputs &in = prep.plan;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) in.cus = prop.multiProcessorCount;
    DParams &P = ctx->P = prep.P;
    ctx->bvh_depth = prep.bvh_depth;
    ctx->ovf_entries = prep.ovf_entries;
    ctx->n_chains = derive_chains(in, K);
    ctx->cfg.work_units = (int) ctx->n_chains;
    P.n_chains = ctx->n_chains;
    const ChainPlan &plan = ctx->plan = plan_chains(in, ctx->n_chains, K);
    P.kernel_variant = plan.kernel_variant; P.tables_in_lds = plan.tables_in_lds; P.small_tables_lds = plan.small_tables_lds;
    P.mh_batch = plan.mh_batch; P.trace_yield = plan.trace_yield; P.pool_refill = plan.pool_refill; P.trace_vote = plan.trace_vote;

    // ---- allocate, upload the prepared tables, point P at them
    auto up = [](DevBuf &b, const auto &v) { // an empty table (no BVH, no flat loop, no cuboids) keeps its null pointer
        const size_t bytes = v.size() * sizeof v[0];
        return v.empty() || (b.alloc(std::max<size_t>(bytes, 64)) == hipSuccess && hipMemcpy(b.p, v.data(), bytes, hipMemcpyHostToDevice) == hipSuccess);
    };
    bool ok = up(ctx->d_prims, prep.prims) && up(ctx->d_shade, prep.shade) && up(ctx->d_bsdfs, prep.bsdfs) && up(ctx->d_emitters, prep.emitters) &&
              up(ctx->d_lut, prep.lut) && up(ctx->d_bvh, prep.bvh) && up(ctx->d_prims_flat, prep.flat) && up(ctx->d_prims_box, prep.boxes) &&
              up(ctx->d_normals, prep.normals);
    if (!ok) return bail(ctx, "device allocation/upload of the scene failed");
    P.prims = ctx->d_prims.as<DPrim>(); P.shade = ctx->d_shade.as<DShade>(); P.bsdfs = ctx->d_bsdfs.as<DBsdf>();
    P.emitters = ctx->d_emitters.as<DEmitter>(); P.bvh = ctx->d_bvh.as<DBvh4Node>(); P.filter_lut = ctx->d_lut.as<float>();
    P.prims_flat = ctx->d_prims_flat.as<DPrimFlat>(); P.prims_box = ctx->d_prims_box.as<DPrimBox>(); // null where the table is empty
    P.normals = ctx->d_normals.as<DSmooth>();
    const drmlt_camera &cam = scene->camera;

    ctx->film_floats = (size_t) cam.width * cam.height * 3;
    const size_t film_bytes = film_alloc_floats(cam.width, cam.height) * sizeof(float); // zero rows behind the film: film_tiles.h
    ok = ctx->d_film.alloc(film_bytes) == hipSuccess && ctx->d_x.alloc((size_t) P.eff_dim * ctx->n_chains * sizeof(float)) == hipSuccess &&
         ctx->d_cur.alloc((size_t) 6 * ctx->n_chains * sizeof(float)) == hipSuccess && ctx->d_stats.alloc(32 * sizeof(unsigned long long)) == hipSuccess &&
         ctx->d_err.alloc(64) == hipSuccess && ctx->d_chain_i.alloc((size_t) 2 * ctx->n_chains * sizeof(int32_t)) == hipSuccess;
    if (!ok) return bail(ctx, "device allocation of chain state / film failed");
    if (hipMemset(ctx->d_chain_i.p, 0, (size_t) 2 * ctx->n_chains * sizeof(int32_t)) != hipSuccess) return bail(ctx, "hipMemset of the chain state failed");
    P.chain_depth = ctx->d_chain_i.as<int32_t>(); P.cur_t = P.chain_depth + ctx->n_chains;
    // run-ahead of k_mutate_v4 (drmlt_run): per-chain mutation counts + the launch's counter of waves short of the target
    if (ctx->d_done.alloc(((size_t) ctx->n_chains + 1) * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(ctx->d_done.p, 0, ((size_t) ctx->n_chains + 1) * sizeof(uint32_t)) != hipSuccess) return bail(ctx, "device allocation failed");
    P.chain_done = nullptr; P.waves_left = ctx->d_done.as<uint32_t>() + ctx->n_chains; P.run_limit = 0;
    P.importance = nullptr;
    P.bd_verts = nullptr; P.bd_lists = nullptr; P.n_chains_alloc = ctx->n_chains;
    if (bdpt) {
        const size_t nvs = (size_t) 2 * cfg->max_depth + 1, rows = (size_t) 7 + 5 * cfg->max_depth;
        if (ctx->d_bd_verts.alloc(((size_t) (20 + 2) * nvs + 2 * ((size_t) cfg->max_depth + 2)) * ctx->n_chains * sizeof(float)) /* records of BR_FLOATS, the fp64 MIS tails, the s = 1 emitter samples: device_bdpt.h */ != hipSuccess ||
            ctx->d_bd_lists.alloc((size_t) 3 * rows * ctx->n_chains * sizeof(float)) != hipSuccess)
            return bail(ctx, "device allocation of the bdpt workspace failed");
        if (hipMemset(ctx->d_bd_lists.p, 0, (size_t) 3 * rows * ctx->n_chains * sizeof(float)) != hipSuccess) return bail(ctx, "hipMemset of the bdpt workspace failed");
        P.bd_verts = ctx->d_bd_verts.as<float>(); P.bd_lists = ctx->d_bd_lists.as<float>();
    }
    if (hipMemset(ctx->d_film.p, 0, film_bytes) != hipSuccess || hipMemset(ctx->d_stats.p, 0, 32 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(ctx->d_err.p, 0, 64) != hipSuccess)
        return bail(ctx, "hipMemset of the film / counters failed");
    P.film = ctx->d_film.as<float>();
    P.x = ctx->d_x.as<float>();
    float *cur = ctx->d_cur.as<float>();
    P.cur_lum = cur; P.cur_px = cur + ctx->n_chains; P.cur_py = cur + 2 * (size_t) ctx->n_chains;
    P.cur_r = cur + 3 * (size_t) ctx->n_chains; P.cur_g = cur + 4 * (size_t) ctx->n_chains; P.cur_b = cur + 5 * (size_t) ctx->n_chains;
    P.stats = ctx->d_stats.as<unsigned long long>();
    P.error_flag = ctx->d_err.as<int32_t>();
    P.rows = nullptr;
    if (plan.rows_mem) {
        if (ctx->d_rows.alloc((size_t) P.eff_dim * ctx->n_chains * sizeof(float)) != hipSuccess) return bail(ctx, "device allocation of the proposal rows failed");
        P.rows = ctx->d_rows.as<float>();
    }
    P.bvh_overflow = nullptr; P.bvh_ovf_lanes = 0;
    P.exec_order = nullptr;
    P.boot_weighted = 0;
    if (hipDeviceSynchronize() != hipSuccess) return bail(ctx, "device synchronisation failed after setup");
    return ctx;
}

void drmlt_destroy(drmlt_ctx *ctx) {
    if (!ctx) return;
    (void) hipSetDevice(ctx->device);
    (void) hipStreamSynchronize(ctx->stream);
    delete ctx;
}

int drmlt_set_stream(drmlt_ctx *ctx, void *hip_stream) {
    if (!ctx) return DRMLT_E_INVALID;
    (void) hipStreamSynchronize(ctx->stream);
    if (ctx->own_stream && ctx->stream) (void) hipStreamDestroy(ctx->stream);
    ctx->stream = static_cast<hipStream_t>(hip_stream);
    ctx->own_stream = false;
    return DRMLT_OK;
}

// Bootstrap + seed selection + replay. `pool_chains` = 0: this context draws its own seeds from its own bootstrap stream
// (stream id = chain_offset; per-rank estimates of b are averaged by the caller, the reference's multi-threaded seeding,
// drmlt.cpp:531-546). `pool_chains` > 0: SURVEY 8(e)'s global pool -- the bootstrap stream 0 is sized for, and
// `pool_chains` seeds are drawn for, the whole job (every rank repeats this cheap step and gets the same list and the
// same b); this context then takes seeds [chain_offset, chain_offset + work_units) of the sorted list. A job split over
// several contexts runs exactly the chains one context with pool_chains work units would.
// `on_device`: the middle -- mean, table, picks, their ordering -- runs in kernels_seed.hip instead of on one host core.
static int seed_impl(drmlt_ctx *ctx, uint64_t seed, uint32_t chain_offset, uint32_t pool_chains, double *b_out, bool on_device) {
    if (!ctx) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DParams &P = ctx->P;
    const bool pool = pool_chains > 0;
    if (pool && (uint64_t) chain_offset + ctx->n_chains > pool_chains) return ctx->fail(DRMLT_E_INVALID, "seed pool of %u chains does not cover chains [%u, %u)", pool_chains, chain_offset, chain_offset + ctx->n_chains);
    const uint32_t n_select = pool ? pool_chains : ctx->n_chains;
    EventPair ev;
    HIP_TRY(ctx, ev.create());
    HIP_TRY(ctx, hipEventRecord(ev.a, ctx->stream));
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    P.chain_offset = chain_offset; P.boot_stream = pool ? 0u : chain_offset;
    ctx->chain_offset = chain_offset;
    // luminance sample floor: max(luminanceSamples, 10 * workUnits), drmlt.cpp:454-466
    // technique=mmlt: x50, and as many again per depth; b is scaled by maxDepth below (drmlt.cpp:456-473,
    // pathsampler.cpp:884-890,932-934). One bootstrap stream per GPU, as with nCores = 1 in the reference.
    const bool mmlt = ctx->cfg.technique == DRMLT_TECH_MMLT;
    uint64_t n64 = (uint64_t) std::max<int64_t>(ctx->cfg.luminance_samples, (int64_t) n_select * (mmlt ? 50 : 10));
    if (mmlt) n64 *= (uint64_t) ctx->cfg.max_depth;
    if (n64 > 0x7fffffffull) return ctx->fail(DRMLT_E_INVALID, "too many luminance samples");
    uint32_t n = (uint32_t) n64;
    // Two-stage MLT: the chains sample f / importance, so that is what their seeds are drawn from (each bootstrap sample's luminance under
    // the map, second half of the buffer). The reference draws them from f itself (pathsampler.cpp:903-905 takes the luminance BEFORE
    // SplatList::normalize(importanceMap)) -- chains then start outside their stationary distribution; over its work units of 1e5
    // mutations that start-up bias is nothing, over the device's short chains it is not (a map of contrast 100 on the Cornell box, 1024
    // mutations per chain: the bright half + 13 %, the dark half - 15 %; DESIGN section 5, deviation 19). b stays the mean of f.
    // drmlt_config.seed_rule = DRMLT_SEED_REFERENCE (adaptor: firstStageSeeding=reference) restores the reference's rule; the oracle
    // follows the same field, so the chain-tracking tests run under both.
    const bool weighted_seeds = P.importance != nullptr && ctx->cfg.seed_rule == DRMLT_SEED_TARGET;
    P.boot_weighted = weighted_seeds ? 1 : 0;
    DevBuf d_lum;
    HIP_TRY(ctx, d_lum.alloc((size_t) n * (weighted_seeds ? 2 : 1) * sizeof(float)));
    const bool bdpt = ctx->cfg.technique == DRMLT_TECH_BDPT;
    HIP_TRY(ctx, ensure_overflow(ctx, P, std::max<size_t>(n, 2 * (size_t) P.n_chains_alloc)));
    if (mmlt) launch_bootstrap_mmlt(P, n, d_lum.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else if (bdpt) launch_bootstrap_bdpt(P, n, d_lum.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else launch_bootstrap(P, n, d_lum.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    double mean = 0.0;
    std::vector<uint32_t> seed_index;
    DevBuf d_si, d_sl;
    if (!on_device) {
        std::vector<float> lum((size_t) n * (weighted_seeds ? 2 : 1));
        HIP_TRY(ctx, hipMemcpyAsync(lum.data(), d_lum.p, lum.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        P.boot_weighted = 0;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

        // generateSeeds, pathsampler.cpp:879-954: mean over non-NaN samples, CDF over the non-zero ones
        double sum = 0.0, tok = 0.0;
        std::vector<uint32_t> idx;
        std::vector<double> cdf;
        idx.reserve(n);
        cdf.reserve((size_t) n + 1); // (hundreds of millions of samples with technique=mmlt's derived chain count: no reallocation on the way)
        cdf.push_back(0.0);
        for (uint32_t i = 0; i < n; ++i) {
            float l = lum[i];
            if (std::isnan(l)) continue;
            tok += 1.0;
            sum += (double) l;
            const float lw = weighted_seeds ? lum[(size_t) n + i] : l; // what the seed is drawn in proportion to
            if (l != 0.f && lw > 0.f && std::isfinite(lw)) { idx.push_back(i); cdf.push_back(cdf.back() + (double) lw); }
        }
        mean = tok > 0 ? sum / tok : 0.0;
        if (mmlt) mean *= (double) ctx->cfg.max_depth; // "As we split the path by corresponding depth"
        if (!(mean > 0.0))
            return ctx->fail(DRMLT_E_ZERO_LUM, "The average image luminance appears to be zero! This could indicate a problem with the scene setup.");
        if (idx.empty()) // mean(f) > 0, yet no sample can seed a chain: every contribution lies where the importance map is zero (or not finite)
            return ctx->fail(DRMLT_E_ZERO_LUM, "No bootstrap sample has a finite positive luminance under the importance map (average luminance %g): "
                                               "the map is zero wherever the scene contributes; firstStageSeeding=reference seeds from the plain luminance", mean);
        const double norm = 1.0 / cdf.back();
        for (size_t i = 1; i < cdf.size(); ++i) cdf[i] *= norm;
        cdf.back() = 1.0;
        // One pick per chain: DiscreteDistribution::sample on the uniform of its own stream address. The picks are SORTED afterwards
        // (PathSeedSortPredicate), so the order in which they are made is free: the uniforms are sorted first and the table is walked once,
        // each lower_bound galloping on from the previous one -- the same entry as a search of the whole table, without a million cold binary
        // searches through gigabytes (technique=mmlt derives a million chains and 50 x maxDepth bootstrap samples for each).
        std::vector<double> xis(n_select);
        for (uint32_t j = 0; j < n_select; ++j) {
            uint32_t r[4];
            philox_host(P.key0, P.key1, 0u, j, P.boot_stream, TAG_SEEDSEL, r);
            xis[j] = (double) ((float) (r[0] >> 8) * (1.0f / 16777216.0f));
        }
        std::sort(xis.begin(), xis.end());
        seed_index.assign(n_select, 0u);
        size_t from = 0; // lower_bound of the previous (smaller or equal) uniform: the next one's is not before it
        for (uint32_t j = 0; j < n_select; ++j) {
            const double xi = xis[j];
            size_t step = 1, hi = from;
            while (hi < cdf.size() && cdf[hi] < xi) { from = hi + 1; hi += step; step *= 2; }
            auto entry = std::lower_bound(cdf.begin() + from, cdf.begin() + std::min(hi, cdf.size()), xi);
            from = (size_t) (entry - cdf.begin());
            size_t index = (size_t) std::max<ptrdiff_t>(0, (entry - cdf.begin()) - 1);
            index = std::min(cdf.size() - 2, index);
            while (cdf[index + 1] - cdf[index] == 0 && index < cdf.size() - 1) ++index;
            seed_index[j] = idx[index];
        }
        std::sort(seed_index.begin(), seed_index.end()); // PathSeedSortPredicate
        if (pool) { // this context's slice of the job's seed list
            std::vector<uint32_t> mine(seed_index.begin() + chain_offset, seed_index.begin() + chain_offset + ctx->n_chains);
            seed_index.swap(mine);
        }
        ctx->seed_indices = seed_index;
        std::vector<float> seed_lum(ctx->n_chains);
        for (uint32_t j = 0; j < ctx->n_chains; ++j) seed_lum[j] = lum[seed_index[j]];

        HIP_TRY(ctx, d_si.alloc(seed_index.size() * sizeof(uint32_t)));
        HIP_TRY(ctx, d_sl.alloc(seed_lum.size() * sizeof(float)));
        HIP_TRY(ctx, hipMemcpyAsync(d_si.p, seed_index.data(), seed_index.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(d_sl.p, seed_lum.data(), seed_lum.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    } else {
        // The same selection on the device (kernels_seed.hip; the rule, its summation order and the pick are seed_select.h's, cited there
        // against pathsampler.cpp:936-957): no luminance leaves the device, no host allocation grows with n. What comes back is three
        // doubles and this context's n_chains picks, which the bookkeeping below and drmlt_seed_indices read.
        P.boot_weighted = 0;
        const size_t work_bytes = seed_workspace_bytes(n);
        DevBuf d_work; // freed on every return path, and before the chains are initialised
        if (d_work.alloc(work_bytes) != hipSuccess)
            return ctx->fail(DRMLT_E_DEVICE, "seed selection on the device: allocation of %zu bytes of workspace failed (%u bootstrap samples)", work_bytes, n);
        if (ctx->knobs.verbose) fprintf(stderr, "[drmlt] seed selection on the device: %zu bytes of workspace beside %zu bytes of luminances (%u samples, %u picks)\n", work_bytes, d_lum.bytes, n, n_select);
        HIP_TRY(ctx, d_si.alloc((size_t) ctx->n_chains * sizeof(uint32_t)));
        HIP_TRY(ctx, d_sl.alloc((size_t) ctx->n_chains * sizeof(float)));
        const double *d_sums = nullptr;
        HIP_TRY(ctx, launch_seed_select(d_lum.as<float>(), weighted_seeds ? d_lum.as<float>() + n : nullptr, n, P.key0, P.key1, P.boot_stream, n_select,
                                        pool ? chain_offset : 0u, ctx->n_chains, d_work.p, d_si.as<uint32_t>(), d_sl.as<float>(), &d_sums, ctx->stream));
        double sums[3] = {0.0, 0.0, 0.0}; // total weight, sum, tok
        seed_index.assign(ctx->n_chains, 0u);
        HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(seed_index.data(), d_si.p, seed_index.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const int status = seed_status(sums[1], sums[2], sums[0], mmlt ? (double) ctx->cfg.max_depth : 1.0, &mean);
        if (status == SEED_SELECT_ZERO_MEAN)
            return ctx->fail(DRMLT_E_ZERO_LUM, "The average image luminance appears to be zero! This could indicate a problem with the scene setup.");
        if (status == SEED_SELECT_NO_WEIGHT)
            return ctx->fail(DRMLT_E_ZERO_LUM, "No bootstrap sample has a finite positive luminance under the importance map (average luminance %g): "
                                               "the map is zero wherever the scene contributes; firstStageSeeding=reference seeds from the plain luminance", mean);
        ctx->seed_indices = seed_index;
    }
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_err.p, 0, 64, ctx->stream));
    HIP_TRY(ctx, ensure_overflow(ctx, P, 2 * (size_t) P.n_chains_alloc));
    if (mmlt && !ctx->knobs.mmlt_no_sort) {
        // execution order of k_mutate_mmlt: chains sorted by their (fixed) path depth, deepest first, whole waves (kernels_mmlt.hip)
        const uint32_t n = ctx->n_chains, padded = (n + 63u) / 64u * 64u;
        std::vector<uint32_t> order(padded, n);
        for (uint32_t j = 0; j < n; ++j) order[j] = j;
        const uint32_t md = (uint32_t) ctx->cfg.max_depth;
        const auto t_sort = std::chrono::steady_clock::now();
        std::stable_sort(order.begin(), order.begin() + n, [&](uint32_t a, uint32_t b) { return seed_index[a] % md > seed_index[b] % md; });
        if (ctx->knobs.verbose) // (this ordering stays on the host under both seed passes: its share of seed_ms)
            fprintf(stderr, "[drmlt] seed: depth ordering of %u chains on the host, %.3f ms\n", n, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sort).count());
        HIP_TRY(ctx, ctx->d_order.alloc(order.size() * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // `order` is a local
        ctx->P.exec_order = P.exec_order = ctx->d_order.as<uint32_t>();
    }
    // (k_mutate_pssmlt_bdpt keeps exec_order NULL: one evaluation per mutation, nothing tells the chains' work apart)
    if (bdpt && ctx->cfg.algo != DRMLT_ALGO_PSSMLT && !ctx->knobs.no_regroup) { // execution order of k_mutate_bdpt: identity until the first launch has told the chains' work apart (regroup_chains)
        const uint32_t n = ctx->n_chains, padded = (n + 63u) / 64u * 64u;
        std::vector<uint32_t> order(padded, n);
        for (uint32_t j = 0; j < n; ++j) order[j] = j;
        HIP_TRY(ctx, ctx->d_order.alloc(order.size() * sizeof(uint32_t)));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // `order` is a local
        ctx->P.exec_order = P.exec_order = ctx->d_order.as<uint32_t>();
    }
    if (mmlt) launch_init_chains_mmlt(P, d_si.as<uint32_t>(), d_sl.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else if (bdpt) launch_init_chains_bdpt(P, d_si.as<uint32_t>(), d_sl.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else launch_init_chains(P, d_si.as<uint32_t>(), d_sl.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    int32_t flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, ctx->d_err.p, sizeof flag, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ev.b, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->seed_ms += ev.elapsed_ms();
    if (flag) return ctx->fail(DRMLT_E_REPLAY, "Error when reconstructing a seed path: luminance mismatch");

    ctx->b = mean;
    if (ctx->cfg.acceptance_map) ctx->b = 1.0;                                       // drmlt.cpp:550-552
    else if (ctx->cfg.average_luminance != -1.0f) ctx->b = ctx->cfg.average_luminance; // drmlt.cpp:555-558
    ctx->seeded = true;
    ctx->regrouped = false;
    ctx->mutation_base = 0;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_done.p, 0, ctx->d_done.bytes, ctx->stream));
    if (b_out) *b_out = ctx->b;
    return DRMLT_OK;
}

int drmlt_seed(drmlt_ctx *ctx, uint64_t seed, uint32_t chain_offset, double *b_out) { return seed_impl(ctx, seed, chain_offset, 0u, b_out, false); }
int drmlt_seed_device(drmlt_ctx *ctx, uint64_t seed, uint32_t chain_offset, double *b_out) { return seed_impl(ctx, seed, chain_offset, 0u, b_out, true); }

int drmlt_bootstrap_luminances(drmlt_ctx *ctx, uint64_t seed, uint32_t stream, uint32_t n, float *out) {
    if (!ctx || !out) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DParams P = ctx->P;
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    P.boot_stream = stream;
    P.boot_weighted = 0;
    DevBuf d_lum;
    HIP_TRY(ctx, d_lum.alloc((size_t) n * sizeof(float)));
    HIP_TRY(ctx, ensure_overflow(ctx, P, std::max<size_t>(n, 2 * (size_t) P.n_chains_alloc)));
    if (ctx->cfg.technique == DRMLT_TECH_MMLT) launch_bootstrap_mmlt(P, n, d_lum.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else if (ctx->cfg.technique == DRMLT_TECH_BDPT) launch_bootstrap_bdpt(P, n, d_lum.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else launch_bootstrap(P, n, d_lum.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, d_lum.p, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_seed_indices(drmlt_ctx *ctx, uint32_t *out) {
    if (!ctx || !out) return DRMLT_E_INVALID;
    if (!ctx->seeded) return ctx->fail(DRMLT_E_STATE, "drmlt_seed_indices before drmlt_seed");
    memcpy(out, ctx->seed_indices.data(), ctx->seed_indices.size() * sizeof(uint32_t));
    return DRMLT_OK;
}

int drmlt_seed_pool(drmlt_ctx *ctx, uint64_t seed, uint32_t first_chain, uint32_t pool_chains, double *b_out) {
    if (!ctx) return DRMLT_E_INVALID;
    if (pool_chains == 0) return ctx->fail(DRMLT_E_INVALID, "drmlt_seed_pool: pool_chains must be positive");
    return seed_impl(ctx, seed, first_chain, pool_chains, b_out, false);
}

int drmlt_seed_pool_device(drmlt_ctx *ctx, uint64_t seed, uint32_t first_chain, uint32_t pool_chains, double *b_out) {
    if (!ctx) return DRMLT_E_INVALID;
    if (pool_chains == 0) return ctx->fail(DRMLT_E_INVALID, "drmlt_seed_pool_device: pool_chains must be positive");
    return seed_impl(ctx, seed, first_chain, pool_chains, b_out, true);
}

// The selection alone on caller-supplied samples (test utilities, like drmlt_bootstrap_luminances): on the device ...
int drmlt_select_seeds_device(drmlt_ctx *ctx, const float *lum, const float *weights_or_null, uint32_t n, uint64_t seed, uint32_t stream, uint32_t n_select,
                              uint32_t *out_sorted, double *mean_out, double *total_out) {
    if (!ctx || !lum || !out_sorted) return DRMLT_E_INVALID;
    if (n == 0 || n > 0x7fffffffu || n_select == 0) return ctx->fail(DRMLT_E_INVALID, "drmlt_select_seeds_device: between 1 and 2^31 - 1 samples and at least one pick");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t work_bytes = seed_workspace_bytes(n);
    DevBuf d_lum, d_work, d_out;
    HIP_TRY(ctx, d_lum.alloc((size_t) n * (weights_or_null ? 2 : 1) * sizeof(float)));
    HIP_TRY(ctx, d_out.alloc((size_t) n_select * sizeof(uint32_t)));
    if (d_work.alloc(work_bytes) != hipSuccess)
        return ctx->fail(DRMLT_E_DEVICE, "seed selection on the device: allocation of %zu bytes of workspace failed (%u samples)", work_bytes, n);
    HIP_TRY(ctx, hipMemcpyAsync(d_lum.p, lum, (size_t) n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (weights_or_null) HIP_TRY(ctx, hipMemcpyAsync(d_lum.as<float>() + n, weights_or_null, (size_t) n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const double *d_sums = nullptr;
    HIP_TRY(ctx, launch_seed_select(d_lum.as<float>(), weights_or_null ? d_lum.as<float>() + n : nullptr, n, (uint32_t) seed, (uint32_t) (seed >> 32), stream, n_select, 0u,
                                    n_select, d_work.p, d_out.as<uint32_t>(), nullptr, &d_sums, ctx->stream));
    double sums[3] = {0.0, 0.0, 0.0};
    HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_sorted, d_out.p, (size_t) n_select * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double mean = 0.0;
    const int status = seed_status(sums[1], sums[2], sums[0], 1.0, &mean);
    if (mean_out) *mean_out = mean;
    if (total_out) *total_out = sums[0];
    if (status != SEED_SELECT_OK) return ctx->fail(DRMLT_E_ZERO_LUM, status == SEED_SELECT_ZERO_MEAN ? "the mean of the samples is not positive" : "no sample has a finite positive weight");
    return DRMLT_OK;
}

// ... and on the host, with no device: seed_select.h run serially
int drmlt_select_seeds_blocked(const float *lum, const float *weights_or_null, uint32_t n, uint64_t seed, uint32_t stream, uint32_t n_select, uint32_t *out_sorted,
                               double *mean_out, double *total_out) {
    if (!lum || !out_sorted || n == 0 || n > 0x7fffffffu || n_select == 0) return DRMLT_E_INVALID;
    const int status = seed_select_host(lum, weights_or_null, n, (uint32_t) seed, (uint32_t) (seed >> 32), stream, n_select, 1.0, out_sorted, mean_out, total_out);
    return status == SEED_SELECT_OK ? DRMLT_OK : DRMLT_E_ZERO_LUM;
}

// Two-stage MLT (drmlt.cpp:406-418): the luminance image of the first stage weights the second stage's splats.
// Must be set before drmlt_seed: the chains' current states are normalised with it (drmlt_proc.cpp:514).
int drmlt_set_importance_map(drmlt_ctx *ctx, const float *lum_map_or_null) {
    if (!ctx) return DRMLT_E_INVALID;
    if (ctx->seeded) return ctx->fail(DRMLT_E_STATE, "the importance map must be set before drmlt_seed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!lum_map_or_null) { ctx->P.importance = nullptr; return DRMLT_OK; }
    const size_t n = (size_t) ctx->P.width * ctx->P.height;
    // Zero entries are legal: a first-stage image with an unlit region has them (mltLuminancePass applies no floor,
    // util.cpp:190-196). SplatList::normalize then divides by zero, the list luminance becomes inf and the chain loop
    // rejects the proposal (isInvalid, drmlt_proc.cpp:428) -- the kernels do the same (normalize_splat, lum_invalid).
    for (size_t i = 0; i < n; ++i)
        if (!(lum_map_or_null[i] >= 0.f) || !std::isfinite(lum_map_or_null[i]))
            return ctx->fail(DRMLT_E_INVALID, "importance map must be non-negative and finite (pixel %zu)", i);
    HIP_TRY(ctx, ctx->d_importance.alloc(n * sizeof(float)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_importance.p, lum_map_or_null, n * sizeof(float), hipMemcpyHostToDevice));
    ctx->P.importance = ctx->d_importance.as<float>();
    return DRMLT_OK;
}

// Tail of BidirectionalUtils::mltLuminancePass (src/libbidir/util.cpp:179-196): luminance of the developed
// first-stage image, up-sampled with a Gaussian reconstruction filter (stddev 0.5, radius 2), clamped boundary
// lookups, results clamped to [0, inf). Separable Resampler of include/mitsuba/core/rfilter.h:123-198,232-290:
// horizontal pass, then vertical, as mitsuba::resample does (src/libcore/bitmap.cpp:2258-2330).
int drmlt_luminance_map(const float *rgb, int w, int h, int W, int H, float *out) {
    if (!rgb || !out || w <= 0 || h <= 0 || W <= 0 || H <= 0) return DRMLT_E_INVALID;
    std::vector<float> lum((size_t) w * h);
    for (size_t i = 0; i < lum.size(); ++i)
        lum[i] = rgb[3 * i] * 0.212671f + rgb[3 * i + 1] * 0.715160f + rgb[3 * i + 2] * 0.072169f;
    auto gauss = [](float x) {
        const float stddev = 0.5f, radius = 2.0f, alpha = -1.0f / (2.0f * stddev * stddev);
        return std::max(0.0f, std::exp(alpha * x * x) - std::exp(alpha * radius * radius));
    };
    // one 1-D pass: src (n_src samples, stride s_src) -> dst (n_dst samples, stride s_dst)
    auto pass = [&](const float *src, int n_src, size_t s_src, float *dst, int n_dst, size_t s_dst) {
        if (n_src == n_dst) { for (int i = 0; i < n_dst; ++i) dst[i * s_dst] = std::max(0.0f, src[i * s_src]); return; }
        float radius = 2.0f, scale = 1.0f, invScale = 1.0f;
        if (n_dst < n_src) { scale = (float) n_src / (float) n_dst; invScale = 1 / scale; radius *= scale; }
        const int taps = (int) std::ceil(radius * 2);
        for (int i = 0; i < n_dst; ++i) {
            const float center = (i + 0.5f) / n_dst * n_src;
            const int start = (int) std::floor(center - radius + 0.5f);
            float wsum = 0.f, wts[64];
            for (int j = 0; j < taps && j < 64; ++j) { wts[j] = gauss((start + j + 0.5f - center) * invScale); wsum += wts[j]; }
            const float norm = 1.0f / wsum;
            float r = 0.f;
            for (int j = 0; j < taps && j < 64; ++j) {
                const int k = std::min(std::max(start + j, 0), n_src - 1); // EClamp
                r += src[k * s_src] * (wts[j] * norm);
            }
            dst[i * s_dst] = std::max(0.0f, r);
        }
    };
    std::vector<float> tmp((size_t) W * h);
    for (int y = 0; y < h; ++y) pass(&lum[(size_t) y * w], w, 1, &tmp[(size_t) y * W], W, 1);
    for (int x = 0; x < W; ++x) pass(&tmp[x], h, (size_t) W, &out[x], H, (size_t) W);
    return DRMLT_OK;
}

int drmlt_set_luminance(drmlt_ctx *ctx, double b) {
    if (!ctx) return DRMLT_E_INVALID;
    if (!(b > 0)) return ctx->fail(DRMLT_E_INVALID, "luminance must be positive");
    ctx->b = b;
    return DRMLT_OK;
}

// k_mutate_mmlt's waves are made of chains of one depth (seed_impl); between the launches of a call they -- and k_mutate_bdpt's -- are
// ALSO regrouped by the work of the launch just done. Chains run free (one path evaluation per lane per pass), so a wave lasts as long as its slowest
// chain, and a chain parked on a glint or a caustic rejects nearly every first stage: two evaluations per mutation, launch after
// launch. Sorted by (depth, evaluations of the last launch), such chains share waves -- full ones, run first -- instead of holding
// sixty-three finished lanes each (config 5 with the E S* L paths counted: 2.33e9 -> see DESIGN 7a). Chain ids, states and
// streams are untouched: the same chains bit for bit, in other lanes. Counting sort, stable: deterministic.
static int regroup_chains(drmlt_ctx *ctx, uint32_t n_mut) {
    const uint32_t n = ctx->n_chains, padded = (n + 63u) / 64u * 64u, md = ctx->cfg.technique == DRMLT_TECH_MMLT ? (uint32_t) ctx->cfg.max_depth : 1u; // (bdpt: no depth classes)
    if (!ctx->knobs.regroup_on_host) {
        // on the device, enqueued behind the launch whose counts it reads (kernels_mmlt.hip: launch_regroup): no copy, no synchronisation
        const size_t words = regroup_scratch_words(n, md);
        if (ctx->d_regroup.bytes < words * sizeof(uint32_t)) HIP_TRY(ctx, ctx->d_regroup.alloc(words * sizeof(uint32_t)));
        launch_regroup(ctx->d_done.as<uint32_t>(), ctx->cfg.technique == DRMLT_TECH_MMLT ? ctx->P.chain_depth : nullptr, n, n_mut, md, ctx->d_order.as<uint32_t>(), padded,
                       ctx->d_regroup.as<uint32_t>(), ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        if (!ctx->knobs.regroup_check) return DRMLT_OK;
        // test hook: the device's permutation against the host's stable counting sort of the same counts
        std::vector<uint32_t> got(padded), work(n);
        HIP_TRY(ctx, hipMemcpyAsync(got.data(), ctx->d_order.p, (size_t) padded * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(work.data(), ctx->d_done.p, (size_t) n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint32_t> want(n);
        for (uint32_t j = 0; j < n; ++j) want[j] = j;
        auto key = [&](uint32_t j) {
            const uint32_t d = ctx->seed_indices[j] % md, extra = work[j] > n_mut ? work[j] - n_mut : 0u;
            return (md - 1u - d) * 16u + (15u - std::min<uint32_t>(15u, (uint32_t) ((uint64_t) extra * 16u / std::max(1u, n_mut))));
        };
        std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
        for (uint32_t j = 0; j < padded; ++j)
            if (got[j] != (j < n ? want[j] : n)) return ctx->fail(DRMLT_E_DEVICE, "regroup: the device's order differs from the host's stable sort at slot %u (%u instead of %u)", j, got[j], j < n ? want[j] : n);
        ctx->regroup_checks++;
        return DRMLT_OK;
    }
    // the same permutation on the host (round 3's path, kept as the cross-check: tests/test_gpu_node.py compares the two)
    const uint32_t B = 16u;
    std::vector<uint32_t> work(n);
    HIP_TRY(ctx, hipMemcpyAsync(work.data(), ctx->d_done.p, (size_t) n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> start(md * B + 1u, 0u), key(n), order(padded, n);
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t d = ctx->seed_indices[j] % md;                     // deepest first, as at seed time
        const uint32_t extra = work[j] > n_mut ? work[j] - n_mut : 0u;    // second stages and reverse moves
        const uint32_t b = std::min<uint32_t>(B - 1u, (uint32_t) ((uint64_t) extra * B / std::max(1u, n_mut)));
        key[j] = (md - 1u - d) * B + (B - 1u - b);
        ++start[key[j] + 1u];
    }
    for (uint32_t k = 0; k < md * B; ++k) start[k + 1u] += start[k];
    for (uint32_t j = 0; j < n; ++j) order[start[key[j]]++] = j;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_order.p, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); // `order` is a local
    return DRMLT_OK;
}

int drmlt_run(drmlt_ctx *ctx, uint64_t total_mutations, volatile int *stop, drmlt_progress_cb cb, void *user) {
    if (!ctx) return DRMLT_E_INVALID;
    if (!ctx->seeded) return ctx->fail(DRMLT_E_STATE, "drmlt_run called before drmlt_seed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t per_chain = total_mutations / ctx->n_chains; // nMutations, drmlt.cpp:475-476
    std::vector<EventPair> evs; // destroyed on every return path
    uint64_t done = 0;
    int rc = DRMLT_OK;
    // "timeout" (drmlt.cpp:296, drmlt_proc.cpp:519-521,868-877): equal-time mode. All chains run concurrently here,
    // so they all stop at the first launch boundary after the deadline (the reference stops handing out work units).
    const bool timed = ctx->cfg.timeout_s > 0;
    const auto t_start = std::chrono::steady_clock::now();
    // Run-ahead (k_mutate_v4, more than one launch to go): a launch ends when every chain has reached its target, and until then
    // chains that are there keep going -- towards the total of THIS call, at most 8192 mutations beyond the target (16-bit event
    // counters per chain and launch). The last launch has target = limit = total: every chain ends at exactly its count.
    // (A single launch has target = limit and is the plain fixed-count launch; the per-chain counts are kept either way.)
    const Knobs &K = ctx->knobs;
    const ChainPlan &plan = ctx->plan;
    const bool ahead = plan.run_ahead;
    const uint64_t call_base = ctx->mutation_base, call_end = call_base + per_chain;
    const bool regroup = (ctx->cfg.technique == DRMLT_TECH_MMLT || ctx->cfg.technique == DRMLT_TECH_BDPT) && ctx->cfg.algo != DRMLT_ALGO_PSSMLT && ctx->P.exec_order && !K.no_regroup;
    int since_regroup = 0;
    while (done < per_chain) {
        if (stop && *stop) { rc = DRMLT_E_CANCELLED; break; }
        if (timed && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count() >= (double) ctx->cfg.timeout_s) break;
        // shorter launches when somebody is watching (cancellation / progress / deadline latency ~ tens of ms)
        // (regrouping: a short first launch -- an eighth of the call, 32 to 256 mutations -- to learn which chains are parked;
        // DRMLT_REGROUP_FIRST overrides its length, clamped to [1, slice]: a launch beyond 32 768 mutations would overflow the
        // kernels' 16-bit event counters)
        const uint64_t first_len = K.regroup_first ? (uint64_t) K.regroup_first : std::max<uint64_t>(32, std::min<uint64_t>(256, per_chain / 8));
        const uint64_t slice = (stop || cb || timed) ? std::min(K.slice, 256) : (regroup && !ctx->regrouped ? std::min<uint64_t>(K.slice, first_len) : (uint64_t) K.slice);
        uint32_t n = (uint32_t) std::min<uint64_t>(slice, per_chain - done);
        evs.emplace_back();
        EventPair &ev = evs.back();
        HIP_TRY(ctx, ev.create());
        HIP_TRY(ctx, hipEventRecord(ev.a, ctx->stream));
        ctx->P.luminance_b = (float) ctx->b;
        HIP_TRY(ctx, ensure_overflow(ctx, ctx->P, 2 * (size_t) ctx->P.n_chains_alloc + 128));
        if (ctx->cfg.technique != DRMLT_TECH_PATH) {
            DParams Q = ctx->P;
            if (regroup) Q.chain_done = ctx->d_done.as<uint32_t>(); // per-chain evaluation counts of this launch
            if (ctx->cfg.technique == DRMLT_TECH_MMLT) launch_mutate_mmlt(plan, Q, n, ctx->mutation_base, ctx->stream);
            else if (ctx->cfg.algo == DRMLT_ALGO_PSSMLT) launch_mutate_pssmlt_bdpt(plan, Q, n, ctx->mutation_base, ctx->stream);
            else launch_mutate_bdpt(plan, Q, n, ctx->mutation_base, ctx->stream);
        }
        else if (ahead) {
            DParams Q = ctx->P;
            const uint64_t target = call_base + done + n;
            Q.chain_done = ctx->d_done.as<uint32_t>();
            Q.run_limit = (uint32_t) std::min<uint64_t>(call_end, target + (K.ahead_cap >= 0 ? (uint64_t) K.ahead_cap : std::min<uint64_t>(8 * slice, 8192))); // at most eight launches ahead (the per-chain event counters of a launch are 16 bits wide); measured on config 3: 1024 6.7e8, 4096 7.1e8, 8192 7.14e8
            launch_set_u32(Q.waves_left, plan.grid, ctx->stream);
            launch_mutate(plan, Q, (uint32_t) target, 0u, ctx->stream);
        } else launch_mutate(plan, ctx->P, n, ctx->mutation_base, ctx->stream);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipEventRecord(ev.b, ctx->stream));
        ctx->mutation_base += n;
        done += n;
        ctx->launches++;
        // Regrouping is three small kernels on the chains' stream (kernels_mmlt.hip: launch_regroup), after every launch. (Round 3
        // sorted on the host -- a D2H copy, an H2D copy and two stream synchronisations per launch; that path survives behind
        // DRMLT_REGROUP_ON_HOST as the cross-check and is thinned to every fourth launch when somebody is watching.) A failure
        // ends the loop through the normal exit below: counters and timings are kept.
        if (regroup && (!(stop || cb || timed) || !ctx->regrouped || !K.regroup_on_host || ++since_regroup >= 4)) {
            rc = regroup_chains(ctx, n);
            if (rc != DRMLT_OK) break;
            ctx->regrouped = true;
            since_regroup = 0;
        }
        if (stop || cb || timed) {
            const hipError_t se = hipStreamSynchronize(ctx->stream);
            if (se != hipSuccess) { rc = ctx->fail(DRMLT_E_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(se)); break; }
            if (cb) cb(done * ctx->n_chains, per_chain * ctx->n_chains, user);
        }
    }
    { const hipError_t se = hipStreamSynchronize(ctx->stream); if (se != hipSuccess && rc == DRMLT_OK) rc = ctx->fail(DRMLT_E_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(se)); }
    for (const EventPair &e : evs) {
        const float ms = e.elapsed_ms();
        ctx->kernel_ms += ms;
        ctx->kt_ms += ms;
        ctx->kt_launches++;
    }
    if (ahead && done < per_chain && done > 0 && (rc == DRMLT_OK || rc == DRMLT_E_CANCELLED)) {
        // stopped early (cancel / timeout): chains are at the last target or up to eight launches beyond it. One catch-up launch
        // brings everybody to the most advanced chain's count, so that a stopped render, too, has run every chain equally long.
        std::vector<uint32_t> h(ctx->n_chains);
        HIP_TRY(ctx, hipMemcpy(h.data(), ctx->d_done.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        const uint32_t top = *std::max_element(h.begin(), h.end());
        if (top > ctx->mutation_base) {
            DParams Q = ctx->P;
            Q.chain_done = ctx->d_done.as<uint32_t>();
            Q.run_limit = top;
            launch_set_u32(Q.waves_left, plan.grid, ctx->stream);
            launch_mutate(plan, Q, top, 0u, ctx->stream);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            done += top - ctx->mutation_base;
            ctx->mutation_base = top;
            ctx->launches++;
        }
    }
    ctx->mutations += done * ctx->n_chains; // whatever ended the loop: what was launched is counted
    if (rc == DRMLT_E_CANCELLED) return ctx->fail(rc, "cancelled");
    return rc;
}

int drmlt_kernel_time(drmlt_ctx *ctx, double *avg_ms, uint64_t *launches, int reset) {
    if (!ctx) return DRMLT_E_INVALID;
    if (avg_ms) *avg_ms = ctx->kt_launches ? ctx->kt_ms / (double) ctx->kt_launches : 0.0;
    if (launches) *launches = ctx->kt_launches;
    if (reset) { ctx->kt_ms = 0.0; ctx->kt_launches = 0; }
    return DRMLT_OK;
}

int drmlt_develop(drmlt_ctx *ctx, const float *direct_rgb_or_null, float *out_rgb) {
    if (!ctx || !out_rgb) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t npix = (uint32_t) ctx->P.width * ctx->P.height, n = npix * 3;
    DevBuf d_sum, d_out, d_direct;
    HIP_TRY(ctx, d_sum.alloc(sizeof(double)));
    HIP_TRY(ctx, d_out.alloc((size_t) n * sizeof(float)));
    HIP_TRY(ctx, hipMemsetAsync(d_sum.p, 0, sizeof(double), ctx->stream));
    launch_lum_sum(ctx->P.film, ctx->P.importance, npix, d_sum.as<double>(), ctx->stream);
    double sum = 0.0;
    HIP_TRY(ctx, hipMemcpyAsync(&sum, d_sum.p, sizeof sum, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    double avg = sum / (double) npix;
    double factor = ctx->cfg.acceptance_map ? 1.0 : ctx->b / avg; // drmlt_proc.cpp:834-839
    if (direct_rgb_or_null) {
        HIP_TRY(ctx, d_direct.alloc((size_t) n * sizeof(float)));
        HIP_TRY(ctx, hipMemcpyAsync(d_direct.p, direct_rgb_or_null, (size_t) n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    launch_develop(ctx->P.film, d_direct.as<float>(), ctx->P.importance, (float) factor, n, d_out.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, d_out.p, (size_t) n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_stats_get(drmlt_ctx *ctx, drmlt_stats *o) {
    if (!ctx || !o) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    unsigned long long v[32];
    HIP_TRY(ctx, hipMemcpyAsync(v, ctx->d_stats.p, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((ctx->P.debug & 128) && ctx->cfg.technique == DRMLT_TECH_BDPT) // diagnostic stamps of eval_bdpt / k_mutate_bdpt
        fprintf(stderr, "[drmlt stamps] bdpt cycles per wave, summed: walks %llu pair loop %llu whole chain loop %llu | evaluations %llu | stages (all evaluations) %llu, weights + splats %llu, counters + commit %llu\n",
                v[16], v[17], v[18], v[19], v[20], v[21], v[22]);
    else if ((ctx->P.debug & 128) && ctx->P.kernel_variant == 5) // diagnostic stamps of k_mutate_v5
        fprintf(stderr, "[drmlt v5] cycles per wave, summed: bookkeeping %llu step %llu trace %llu | outer iterations %llu, bookkeeping branches %llu (%.1f chains each), "
                        "stepping chains per iteration %.1f, trace phases %llu starting with %.1f lanes, refills %llu\n",
                v[16], v[18], v[17], v[19], v[23], v[23] ? (double) v[24] / v[23] : 0.0, v[19] ? (double) v[25] / v[19] : 0.0, v[20], v[20] ? (double) v[21] / v[20] : 0.0, v[22]);
    else if (ctx->P.debug & 128) // diagnostic stamps of k_mutate_v3 / v4
        fprintf(stderr, "[drmlt stamps] cycles: mh %llu trace %llu step %llu | iterations %llu mh-branches %llu tracing-lanes %llu\n",
                v[16], v[17], v[18], v[19], v[20], v[21]),
        fprintf(stderr, "[drmlt stamps] mh sections: decide+splat %llu commit %llu start %llu fill %llu\n", v[22], v[23], v[24], v[25]),
        fprintf(stderr, "[drmlt stamps] iterations by chains tracing (of 32): 0: %llu, 1-4: %llu, 5-8: %llu, 9-16: %llu, 17-24: %llu, 25-32: %llu\n", v[26], v[27], v[28], v[29], v[30], v[31]);
    if (ctx->knobs.verbose && v[12])
        fprintf(stderr, "[drmlt bvh] wave iterations: inner %llu (%.1f lanes each), leaf %llu (%.1f lanes each)\n", v[12], (double) v[10] / (double) v[12], v[13],
                v[13] ? (double) v[11] / (double) v[13] : 0.0);
    if (ctx->knobs.verbose && ctx->P.kernel_variant == 4)
        fprintf(stderr, "[drmlt v4] waves through the orbital rule body: %llu\n", v[14]),
        fprintf(stderr, "[drmlt v4] waves through a one-light build: %llu\n", v[15]);
    if (ctx->knobs.verbose && ctx->P.kernel_variant == 4 && !(ctx->P.debug & 128)) // (slot 16 is a cycle stamp of the stamps builds)
        fprintf(stderr, "[drmlt v4] waves through k_mutate_w2: %llu\n", v[16]),
        fprintf(stderr, "[drmlt v4] waves with the ray records held in registers: %llu\n", v[17]); // (k_mutate_w2h; they count in slot 16 too)
    if ((ctx->P.debug & 1024) && v[20] && ctx->P.kernel_variant != 5)
        fprintf(stderr, "[drmlt bvh] lanes at slice start, of 64: tracing %.1f, chain waiting for its partner %.1f, chain parked for bookkeeping %.1f, helper idle %.1f, flush %.1f (%llu slices)\n",
                (double) v[21] / v[20], (double) v[22] / v[20], (double) v[23] / v[20], (double) v[24] / v[20], (double) v[25] / v[20], v[20]);
    memset(o, 0, sizeof *o);
    const uint64_t M = ctx->mutations;
    const uint64_t n_large = v[0], acc1_l = v[1], acc1_b = v[2], sec_l = v[3], sec_b = v[4], acc2_l = v[5], acc2_b = v[6], n_rev = v[7];
    if (ctx->cfg.algo == DRMLT_ALGO_PSSMLT) { // pssmlt_proc.cpp:230-260: one acceptance test per mutation
        o->overall_base = M;               o->overall_acc = acc1_l + acc1_b;
        o->large_base = n_large;           o->large_acc = acc1_l;
        o->bold_base = M - n_large;        o->bold_acc = acc1_b;
    } else if (!ctx->cfg.use_mixture) { // drmlt_proc.cpp:715-768
        o->first_base = M;                 o->first_acc = acc1_l + acc1_b;
        o->large_base = n_large;           o->large_acc = acc1_l;
        o->bold_base = M - n_large;        o->bold_acc = acc1_b;
        o->second_base = sec_l + sec_b;    o->second_acc = acc2_l + acc2_b;
        o->second_large_base = sec_l;      o->second_large_acc = acc2_l;
        o->second_bold_base = sec_b;       o->second_bold_acc = acc2_b;
        o->overall_base = M + sec_l + sec_b;
        o->overall_acc = acc1_l + acc1_b + acc2_l + acc2_b;
    } else { // drmlt_proc.cpp:342-377
        o->second_base = sec_b;            o->second_acc = acc2_b;
        o->first_base = M - sec_b;         o->first_acc = acc1_l + acc1_b;
        o->large_base = n_large;           o->large_acc = acc1_l;
        o->bold_base = M - n_large - sec_b; o->bold_acc = acc1_b;
        o->overall_base = M;               o->overall_acc = acc1_l + acc1_b + acc2_b;
    }
    o->mutations = M;
    o->path_evals = M + sec_l + sec_b + n_rev;
    o->rays = v[8];
    o->accepted = acc1_l + acc1_b + acc2_l + acc2_b;
    o->kernel_ms = ctx->kernel_ms;
    o->seed_ms = ctx->seed_ms;
    o->n_chains = ctx->n_chains;
    o->max_dim = (uint32_t) ctx->P.max_dim;
    o->launches = ctx->launches;
    o->bvh_node_visits = v[10]; o->bvh_prim_tests = v[11]; o->bvh_node_iterations = v[12]; o->bvh_leaf_iterations = v[13];
    return DRMLT_OK;
}

int drmlt_eval_paths(drmlt_ctx *ctx, const float *u, uint32_t n, uint32_t dim, drmlt_splat *out) {
    if (!ctx || !u || !out) return DRMLT_E_INVALID;
    const bool mmlt = ctx->cfg.technique == DRMLT_TECH_MMLT;
    if (ctx->cfg.technique == DRMLT_TECH_BDPT) return ctx->fail(DRMLT_E_INVALID, "technique=bdpt evaluates to splat lists: use drmlt_eval_lists");
    const int need = ctx->P.eff_dim + (mmlt ? 1 : 0); // mmlt: [sensor S | emitter E | direct | depth]
    if ((int) dim < need) return ctx->fail(DRMLT_E_INVALID, "eval_paths: need at least %d PSS dimensions per point", need);
    if (n == 0) return DRMLT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d_u, d_o;
    HIP_TRY(ctx, d_u.alloc((size_t) n * dim * sizeof(float)));
    HIP_TRY(ctx, d_o.alloc((size_t) n * 8 * sizeof(float)));
    HIP_TRY(ctx, hipMemcpyAsync(d_u.p, u, (size_t) n * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, ensure_overflow(ctx, ctx->P, std::max<size_t>(n, (size_t) ctx->P.n_chains_alloc)));
    if (mmlt) launch_eval_paths_mmlt(ctx->P, d_u.as<float>(), n, dim, d_o.as<float>(), ctx->plan.aux_lds, ctx->stream);
    else launch_eval_paths(ctx->P, d_u.as<float>(), n, dim, d_o.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<float> h((size_t) n * 8);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), d_o.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (uint32_t i = 0; i < n; ++i) {
        const float *r = &h[(size_t) i * 8];
        out[i].luminance = r[0]; out[i].x = r[1]; out[i].y = r[2];
        out[i].rgb[0] = r[3]; out[i].rgb[1] = r[4]; out[i].rgb[2] = r[5];
        memcpy(&out[i].n_dims, &r[6], 4);
        memcpy(&out[i].n_rays, &r[7], 4);
    }
    return DRMLT_OK;
}

int drmlt_film_read(drmlt_ctx *ctx, float *out_rgb) {
    if (!ctx || !out_rgb) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, ctx->d_film.p, ctx->film_floats * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_film_clear(drmlt_ctx *ctx) {
    if (!ctx) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_film.p, 0, ctx->d_film.bytes, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

void *drmlt_film_device_ptr(drmlt_ctx *ctx) { return ctx ? ctx->d_film.p : nullptr; }

int drmlt_render_pt(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, float *out_rgb) {
    if (!ctx || !out_rgb || spp == 0) return DRMLT_E_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DParams P = ctx->P;
    DevBuf film;
    const size_t bytes = (size_t) P.width * P.height * 3 * sizeof(float);
    HIP_TRY(ctx, film.alloc(bytes));
    HIP_TRY(ctx, hipMemsetAsync(film.p, 0, bytes, ctx->stream));
    P.film = film.as<float>();
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    const uint64_t n = (uint64_t) spp * P.width * P.height;
    HIP_TRY(ctx, ensure_overflow(ctx, P, (size_t) 16384 * 64));
    launch_render_pt(P, n, 0u, 1.0f / (float) spp, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, film.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

// Independent samples of sampleSplats(EBidirectional) into a film of its own: sample i is bootstrap sample i of stream 0 under
// `seed` (drmlt_bootstrap_luminances reports its list luminance), every splat of its list goes through film_put with weight
// 1 / spp. Scratch is the bootstrap's -- the workspace columns and list slot 1, which every mutation writes before it reads
// (k_mutate_bdpt, k_mutate_pssmlt_bdpt: the first evaluation of a mutation targets slot 1; slot 2 is read only after its own
// second stage wrote it) -- so the context's film, b, chain states, current lists (slot 0) and counters stay as they were.
int drmlt_render_bdpt(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, float *out_rgb) {
    if (!ctx || !out_rgb || spp == 0) return DRMLT_E_INVALID;
    if (ctx->cfg.technique != DRMLT_TECH_BDPT)
        return ctx->fail(DRMLT_E_INVALID, "drmlt_render_bdpt needs a context with technique=bdpt (its workspace, list rows and LDS plan)");
    DParams P = ctx->P;
    const uint64_t n = (uint64_t) spp * (uint64_t) P.width * (uint64_t) P.height;
    if (n >= (1ull << 32))
        return ctx->fail(DRMLT_E_INVALID, "render_bdpt: %u spp on %d x %d pixels are %llu samples, the sample address has 32 bits: "
                                          "average several calls with different seeds", spp, P.width, P.height, (unsigned long long) n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf film;
    const size_t bytes = (size_t) P.width * P.height * 3 * sizeof(float);
    HIP_TRY(ctx, film.alloc(bytes));
    HIP_TRY(ctx, hipMemsetAsync(film.p, 0, bytes, ctx->stream));
    P.film = film.as<float>();
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    P.boot_stream = 0u;
    P.importance = nullptr; // the image is of f itself
    P.boot_weighted = 0;
    P.debug &= ~128; // (the evaluation's cycle stamps go to the context's counters)
    HIP_TRY(ctx, ensure_overflow(ctx, P, 2 * (size_t) P.n_chains_alloc)); // the grid's lanes: n_chains_alloc, as the bootstrap's
    launch_render_bdpt(P, (uint32_t) n, 1.0f / (float) spp, ctx->plan.aux_lds, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, film.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_bdpt_layer_count(int32_t max_depth) { return bdpt_layer_count(max_depth); }
int drmlt_bdpt_layer_index(int32_t depth, int32_t s) { return bdpt_layer_index(depth, s); }

// drmlt_render_bdpt's samples, cell by cell: every connection (s, t) that produced goes into layer (d = s + t - 1, s) of a layered
// film, which is an allocation of this call. Refusals, scratch and what is left alone are drmlt_render_bdpt's; the splat lists the
// evaluation writes into slot 1 on the way are not read.
int drmlt_render_bdpt_layers(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, int32_t mode, float *out_layers) {
    if (!ctx || !out_layers) return DRMLT_E_INVALID;
    if (spp == 0) return ctx->fail(DRMLT_E_INVALID, "render_bdpt_layers: spp is 0, a render takes at least one sample per pixel");
    if (ctx->cfg.technique != DRMLT_TECH_BDPT)
        return ctx->fail(DRMLT_E_INVALID, "drmlt_render_bdpt needs a context with technique=bdpt (its workspace, list rows and LDS plan)");
    if (mode != DRMLT_LAYERS_WEIGHTED && mode != DRMLT_LAYERS_UNWEIGHTED)
        return ctx->fail(DRMLT_E_INVALID, "render_bdpt_layers: unknown mode %d (DRMLT_LAYERS_WEIGHTED = %d, DRMLT_LAYERS_UNWEIGHTED = %d)",
                         (int) mode, (int) DRMLT_LAYERS_WEIGHTED, (int) DRMLT_LAYERS_UNWEIGHTED);
    DParams P = ctx->P;
    const uint64_t n = (uint64_t) spp * (uint64_t) P.width * (uint64_t) P.height;
    if (n >= (1ull << 32))
        return ctx->fail(DRMLT_E_INVALID, "render_bdpt: %u spp on %d x %d pixels are %llu samples, the sample address has 32 bits: "
                                          "average several calls with different seeds", spp, P.width, P.height, (unsigned long long) n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf layers;
    const size_t bytes = (size_t) bdpt_layer_count(P.max_depth) * P.width * P.height * 3 * sizeof(float);
    if (layers.alloc(bytes) != hipSuccess) {
        (void) hipGetLastError(); // (the failed allocation is reported here, not by the next call that asks for the last error)
        return ctx->fail(DRMLT_E_DEVICE, "render_bdpt_layers: cannot allocate the layered film, %llu bytes (%d layers of %d x %d pixels)",
                         (unsigned long long) bytes, bdpt_layer_count(P.max_depth), P.width, P.height);
    }
    HIP_TRY(ctx, hipMemsetAsync(layers.p, 0, bytes, ctx->stream));
    P.film = nullptr; // nothing here writes a film but the sink
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    P.boot_stream = 0u;
    P.importance = nullptr; // the layers are of f itself
    P.boot_weighted = 0;
    P.debug &= ~128; // (the evaluation's cycle stamps go to the context's counters)
    HIP_TRY(ctx, ensure_overflow(ctx, P, 2 * (size_t) P.n_chains_alloc)); // the grid's lanes, as drmlt_render_bdpt
    launch_layers_bdpt(P, (uint32_t) n, 1.0f / (float) spp, layers.as<float>(), mode == DRMLT_LAYERS_UNWEIGHTED, ctx->plan.aux_lds, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_layers, layers.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_pt_layer_count(int32_t max_depth) { return pt_layer_count(max_depth); }
int drmlt_pt_layer_index(int32_t depth, int32_t strategy) { return pt_layer_index(depth, strategy); }

// drmlt_render_pt's samples, term by term: what path_step adds to a sample's radiance goes into layer (d, strategy) of a layered
// film, which is an allocation of this call. Like drmlt_render_pt it writes nothing of the context but the traversal's overflow
// area (scratch of every launch): the film, b, chain states and counters stay as they were.
int drmlt_render_pt_layers(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, int32_t mode, float *out_layers) {
    if (!ctx || !out_layers) return DRMLT_E_INVALID;
    if (spp == 0) return ctx->fail(DRMLT_E_INVALID, "render_pt_layers: spp is 0, a render takes at least one sample per pixel");
    if (ctx->cfg.technique != DRMLT_TECH_PATH)
        return ctx->fail(DRMLT_E_INVALID, "drmlt_render_pt_layers needs a context with technique=path, this one has technique=%s "
                                          "(drmlt_render_bdpt_layers splits the bidirectional estimate)",
                         ctx->cfg.technique == DRMLT_TECH_BDPT ? "bdpt" : ctx->cfg.technique == DRMLT_TECH_MMLT ? "mmlt" : "?");
    if (mode != DRMLT_LAYERS_WEIGHTED && mode != DRMLT_LAYERS_UNWEIGHTED)
        return ctx->fail(DRMLT_E_INVALID, "render_pt_layers: unknown mode %d (DRMLT_LAYERS_WEIGHTED = %d, DRMLT_LAYERS_UNWEIGHTED = %d)",
                         (int) mode, (int) DRMLT_LAYERS_WEIGHTED, (int) DRMLT_LAYERS_UNWEIGHTED);
    DParams P = ctx->P;
    if (P.max_depth < 1 || P.max_depth > PT_LAYERS_MAX_DEPTH)
        return ctx->fail(DRMLT_E_INVALID, "render_pt_layers: maxDepth %d: the layers need a path length bounded by 1 <= maxDepth <= %d, "
                                          "technique=bdpt's bound (a sample's terms are held in LDS until it ends)", P.max_depth, PT_LAYERS_MAX_DEPTH);
    const uint64_t n = (uint64_t) spp * (uint64_t) P.width * (uint64_t) P.height;
    if (n >= (1ull << 32))
        return ctx->fail(DRMLT_E_INVALID, "render_pt_layers: %u spp on %d x %d pixels are %llu samples, the sample address has 32 bits: "
                                          "average several calls with different seeds", spp, P.width, P.height, (unsigned long long) n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf layers;
    // the layered film is fp64 on the device and rounded to fp32 here, layer by layer (layer_film.h: layer_put_f64)
    const size_t layer_floats = (size_t) P.width * P.height * 3, n_layers = (size_t) pt_layer_count(P.max_depth);
    const size_t bytes = n_layers * layer_floats * sizeof(double);
    if (layers.alloc(bytes) != hipSuccess) {
        (void) hipGetLastError(); // (the failed allocation is reported here, not by the next call that asks for the last error)
        return ctx->fail(DRMLT_E_DEVICE, "render_pt_layers: cannot allocate the layered film, %llu bytes (%d layers of %d x %d pixels in fp64)",
                         (unsigned long long) bytes, pt_layer_count(P.max_depth), P.width, P.height);
    }
    HIP_TRY(ctx, hipMemsetAsync(layers.p, 0, bytes, ctx->stream));
    P.film = nullptr; // nothing here writes a film but the kernel's own put
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    HIP_TRY(ctx, ensure_overflow(ctx, P, (size_t) 16384 * 64)); // the grid's lanes, as drmlt_render_pt
    launch_render_pt_layers(P, (uint32_t) n, 1.0f / (float) spp, layers.as<double>(), mode == DRMLT_LAYERS_UNWEIGHTED, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> one(layer_floats);
    for (size_t l = 0; l < n_layers; ++l) {
        HIP_TRY(ctx, hipMemcpyAsync(one.data(), layers.as<double>() + l * layer_floats, layer_floats * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float *const dst = out_layers + l * layer_floats;
        for (size_t i = 0; i < layer_floats; ++i) dst[i] = (float) one[i];
    }
    return DRMLT_OK;
}

// Independent samples of sampleSplats(EMMLT) into an fp64 film, or into one film per (depth, strategy), which are allocations of
// this call: sample i is bootstrap sample i of stream 0 under `seed`, depth (i % maxDepth) + 1, so every depth has spp * W * H
// samples and the scale is 1 / spp (include/drmlt_abi.h has the derivation). Scratch is LDS and the traversal's overflow area
// alone: the context's film, b, chain states and counters stay as they were. `layered`: drmlt_render_mmlt_layers, with `mode`.
static int render_mmlt(drmlt_ctx *ctx, const char *name, uint32_t spp, uint64_t seed, bool layered, int32_t mode, float *out) {
    if (!ctx || !out) return DRMLT_E_INVALID;
    if (spp == 0) return ctx->fail(DRMLT_E_INVALID, "%s: spp is 0, a render takes at least one sample per pixel and depth", name);
    if (ctx->cfg.technique != DRMLT_TECH_MMLT)
        return ctx->fail(DRMLT_E_INVALID, "drmlt_%s needs a context with technique=mmlt, this one has technique=%s (%s is its reference)", name,
                         ctx->cfg.technique == DRMLT_TECH_BDPT ? "bdpt" : ctx->cfg.technique == DRMLT_TECH_PATH ? "path" : "?",
                         ctx->cfg.technique == DRMLT_TECH_BDPT ? (layered ? "drmlt_render_bdpt_layers" : "drmlt_render_bdpt")
                                                               : (layered ? "drmlt_render_pt_layers" : "drmlt_render_pt"));
    if (layered && mode != DRMLT_LAYERS_WEIGHTED && mode != DRMLT_LAYERS_UNWEIGHTED)
        return ctx->fail(DRMLT_E_INVALID, "%s: unknown mode %d (DRMLT_LAYERS_WEIGHTED = %d, DRMLT_LAYERS_UNWEIGHTED = %d)", name,
                         (int) mode, (int) DRMLT_LAYERS_WEIGHTED, (int) DRMLT_LAYERS_UNWEIGHTED);
    DParams P = ctx->P;
    const int n_layers = layered ? bdpt_layer_count(P.max_depth) : 1;
    if (P.max_depth < 1 || n_layers < 1) return ctx->fail(DRMLT_E_INVALID, "%s: maxDepth %d has no layers", name, P.max_depth);
    const uint64_t per_depth = (uint64_t) spp * (uint64_t) P.width * (uint64_t) P.height;
    if (per_depth >= (1ull << 32) || per_depth * (uint64_t) P.max_depth >= (1ull << 32))
        return ctx->fail(DRMLT_E_INVALID, "%s: %u spp on %d x %d pixels and %d depths are %llu x %d samples, the sample address has 32 bits: "
                                          "average several calls with different seeds", name, spp, P.width, P.height, P.max_depth,
                         (unsigned long long) per_depth, P.max_depth);
    const uint32_t n = (uint32_t) (per_depth * (uint64_t) P.max_depth);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf films;
    // the films are fp64 on the device and rounded to fp32 here, film by film (layer_film.h: layer_put_f64)
    const size_t film_floats = (size_t) P.width * P.height * 3;
    const size_t bytes = (size_t) n_layers * film_floats * sizeof(double);
    if (films.alloc(bytes) != hipSuccess) {
        (void) hipGetLastError(); // (the failed allocation is reported here, not by the next call that asks for the last error)
        return ctx->fail(DRMLT_E_DEVICE, "%s: cannot allocate the film, %llu bytes (%d films of %d x %d pixels in fp64)", name,
                         (unsigned long long) bytes, n_layers, P.width, P.height);
    }
    HIP_TRY(ctx, hipMemsetAsync(films.p, 0, bytes, ctx->stream));
    P.film = nullptr; // nothing here writes a film but the kernel's own put
    P.key0 = (uint32_t) seed; P.key1 = (uint32_t) (seed >> 32);
    P.boot_stream = 0u;
    P.importance = nullptr; // the image is of f itself
    P.boot_weighted = 0;
    HIP_TRY(ctx, ensure_overflow(ctx, P, (size_t) render_mmlt_grid(n) * 64)); // the grid's lanes
    const float scale = 1.0f / (float) spp;
    if (layered) launch_layers_mmlt(P, n, scale, films.as<double>(), mode == DRMLT_LAYERS_UNWEIGHTED, ctx->plan.aux_lds, ctx->stream);
    else launch_render_mmlt(P, n, scale, films.as<double>(), ctx->plan.aux_lds, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<double> one(film_floats);
    for (size_t l = 0; l < (size_t) n_layers; ++l) {
        HIP_TRY(ctx, hipMemcpyAsync(one.data(), films.as<double>() + l * film_floats, film_floats * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        float *const dst = out + l * film_floats;
        for (size_t i = 0; i < film_floats; ++i) dst[i] = (float) one[i];
    }
    return DRMLT_OK;
}
int drmlt_render_mmlt(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, float *out_rgb) {
    return render_mmlt(ctx, "render_mmlt", spp, seed, false, DRMLT_LAYERS_WEIGHTED, out_rgb);
}
int drmlt_render_mmlt_layers(drmlt_ctx *ctx, uint32_t spp, uint64_t seed, int32_t mode, float *out_layers) {
    return render_mmlt(ctx, "render_mmlt_layers", spp, seed, true, mode, out_layers);
}

int drmlt_direct_split(int32_t direct_samples, int32_t *pixel_samples, int32_t *shading_samples) {
    int ps = 0, ss = 0;
    if (!pixel_samples || !shading_samples || !direct_split(direct_samples, ps, ss)) return DRMLT_E_INVALID;
    *pixel_samples = ps; *shading_samples = ss;
    return DRMLT_OK;
}

// BidirectionalUtils::renderDirectComponent (util.cpp:30-92) for rows [row_lo, row_hi). Under a filter wider than a pixel the rows
// just outside the range are sampled too (their footprints reach in); their random numbers are addressed by the pixel, so they are
// the very samples the neighbouring range draws. The context's film, chains and parameter block are left alone.
int drmlt_render_direct(drmlt_ctx *ctx, int32_t direct_samples, int32_t hide_emitters, uint64_t seed, int32_t row_lo, int32_t row_hi, float *out_rgb) {
    if (!ctx) return DRMLT_E_INVALID;
    if (!out_rgb) return ctx->fail(DRMLT_E_INVALID, "render_direct: out_rgb is NULL");
    DirectJob J{};
    if (!direct_split(direct_samples, J.pixel_samples, J.shading_samples))
        return ctx->fail(DRMLT_E_INVALID, "render_direct: directSamples must be positive (got %d); the chains carry the direct light when it is -1", (int) direct_samples);
    const DParams &P = ctx->P;
    if (row_lo < 0 || row_hi > P.height || row_lo >= row_hi)
        return ctx->fail(DRMLT_E_INVALID, "render_direct: rows [%d, %d) are not a non-empty range within the film's %d rows", (int) row_lo, (int) row_hi, P.height);
    while ((1 << J.group_log2) < J.pixel_samples) J.group_log2++;
    J.key0 = (uint32_t) seed; J.key1 = (uint32_t) (seed >> 32);
    J.hide_emitters = hide_emitters ? 1 : 0;
    J.row_lo = row_lo; J.row_hi = row_hi;
    J.margin = std::max(0, (int) std::ceil(P.filter_radius - 0.5f));
    J.samp_lo = std::max(0, row_lo - J.margin); J.samp_hi = std::min(P.height, row_hi + J.margin);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the workspace first: 4-channel film of the rows + the developed rows; nothing is allocated once the launches are enqueued
    const size_t n_out = (size_t) (row_hi - row_lo) * P.width;
    DevBuf acc, out;
    HIP_TRY(ctx, acc.alloc(n_out * 4 * sizeof(float)));
    HIP_TRY(ctx, out.alloc(n_out * 3 * sizeof(float)));
    DParams Pl = P;
    HIP_TRY(ctx, ensure_overflow(ctx, Pl, (size_t) direct_grid(J, P.width) * 64));
    J.acc = acc.as<float>();
    HIP_TRY(ctx, hipMemsetAsync(acc.p, 0, acc.bytes, ctx->stream));
    launch_render_direct(Pl, J, out.as<float>(), ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_rgb, out.p, out.bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_eval_lists(drmlt_ctx *ctx, const float *u, uint32_t n, uint32_t dim, float *out, uint32_t stride) {
    if (!ctx || !u || !out) return DRMLT_E_INVALID;
    if (ctx->cfg.technique != DRMLT_TECH_BDPT) return ctx->fail(DRMLT_E_INVALID, "drmlt_eval_lists is for technique=bdpt");
    if ((int) dim < ctx->P.eff_dim) return ctx->fail(DRMLT_E_INVALID, "eval_lists: need at least %d PSS dimensions per point", ctx->P.eff_dim);
    if (stride < 10) return ctx->fail(DRMLT_E_INVALID, "eval_lists: stride must be at least 10 floats");
    if (n == 0) return DRMLT_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf d_u, d_o;
    HIP_TRY(ctx, d_u.alloc((size_t) n * dim * sizeof(float)));
    HIP_TRY(ctx, d_o.alloc((size_t) n * stride * sizeof(float)));
    HIP_TRY(ctx, hipMemcpyAsync(d_u.p, u, (size_t) n * dim * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, ensure_overflow(ctx, ctx->P, (size_t) ctx->P.n_chains_alloc));
    launch_eval_lists_bdpt(ctx->P, d_u.as<float>(), n, dim, d_o.as<float>(), stride, ctx->plan.aux_lds, ctx->stream);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, d_o.p, (size_t) n * stride * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DRMLT_OK;
}

int drmlt_chain_state(drmlt_ctx *ctx, drmlt_splat *cur, float *u, uint32_t dim) {
    if (!ctx) return DRMLT_E_INVALID;
    if (!ctx->seeded) return ctx->fail(DRMLT_E_STATE, "chain_state before seed");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n = ctx->n_chains;
    if (cur && ctx->cfg.technique == DRMLT_TECH_BDPT) {
        // current splat list (slot 0, unnormalised): luminance, main splat; n_dims = has main splat, n_rays = light-image splats
        std::vector<float> h((size_t) 7 * n), l(n);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->d_bd_lists.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(l.data(), ctx->d_cur.p, l.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < n; ++i) {
            int32_t meta; memcpy(&meta, &h[(size_t) n + i], 4);
            const float inv = l[i] > 0.f ? 1.f / l[i] : 0.f;
            cur[i].luminance = l[i]; cur[i].x = h[2 * (size_t) n + i]; cur[i].y = h[3 * (size_t) n + i];
            cur[i].rgb[0] = h[4 * (size_t) n + i] * inv; cur[i].rgb[1] = h[5 * (size_t) n + i] * inv; cur[i].rgb[2] = h[6 * (size_t) n + i] * inv;
            cur[i].n_dims = meta & 1; cur[i].n_rays = meta >> 1;
        }
        cur = nullptr;
    }
    if (cur) {
        std::vector<float> h((size_t) 6 * n);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->d_cur.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < n; ++i) {
            cur[i].luminance = h[i]; cur[i].x = h[n + i]; cur[i].y = h[2 * (size_t) n + i];
            cur[i].rgb[0] = h[3 * (size_t) n + i]; cur[i].rgb[1] = h[4 * (size_t) n + i]; cur[i].rgb[2] = h[5 * (size_t) n + i];
            cur[i].n_dims = 0; cur[i].n_rays = 0;
        }
        if (ctx->cfg.technique == DRMLT_TECH_MMLT) { // n_dims: the chain's path depth, n_rays: t of the current state
            std::vector<int32_t> ci((size_t) 2 * n);
            HIP_TRY(ctx, hipMemcpyAsync(ci.data(), ctx->d_chain_i.p, ci.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            for (uint32_t i = 0; i < n; ++i) { cur[i].n_dims = ci[i]; cur[i].n_rays = ci[n + i]; }
        }
    }
    if (u) {
        std::vector<float> h((size_t) ctx->P.eff_dim * n);
        HIP_TRY(ctx, hipMemcpyAsync(h.data(), ctx->d_x.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 0; k < dim; ++k) u[(size_t) i * dim + k] = k < (uint32_t) ctx->P.eff_dim ? h[(size_t) k * n + i] : 0.f;
    }
    return DRMLT_OK;
}

} // extern "C"
