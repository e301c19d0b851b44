// HIP kernels of the DRMLT hot path for gfx950 (MI355X). One Markov chain per lane.
//
//   k_bootstrap     luminance samples of PathSampler::generateSeeds (pathsampler.cpp:879-920)
//   k_init_chains   seed replay + fillReplay + luminance sanity check (drmlt_proc.cpp:467-514)
//   k_mutate_pssmlt PSSMLTRenderer::process (pssmlt_proc.cpp:113-297)
//   k_eval_paths    PathSampler::sampleSplats on caller-supplied PSS points (pathsampler.cpp:529-567)
//   k_render_pt     independent samples of the same integrand (validation image)
//   k_lum_sum / k_develop   DRMLTProcess::develop (drmlt_proc.cpp:824-849)
// DRMLTRenderer::process / processMixture's chain loop (drmlt_proc.cpp:161-380,518-770) is in two more units: kernels_v4.hip
// (k_mutate_v4, k_mutate_w2, k_mutate_v5) and kernels_v3.hip (k_mutate_v3, their predecessor, kept as the bit-equality cross-check);
// launch_mutate below dispatches to their launchers.
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include "device_path.h"

#include "kernel_common.h"
#include "launch_plan.h" // the launcher below dispatches on its Build

// Bootstrap sample `index` of the replayable stream. ONE compiled body serves k_bootstrap and k_init_chains: the replay is
// checked for EQUALITY with the bootstrap luminance (drmlt_proc.cpp:509-512), and two inlined copies of the same source
// may be contracted / scheduled differently by the compiler -- a rounding difference that flips one discrete decision in
// one of 1e5 paths fails the seeding.
__device__ __attribute__((noinline)) DSplat eval_boot_sample(const DParams &P, uint32_t index, uint32_t &nd) {
    Sampler smp;
    smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = P.boot_stream; smp.major = index;
    smp.mode = SM_BOOT; smp.arr = nullptr;
    uint32_t nr;
    return eval_path(P, smp, nr, nd);
}

__global__ void __launch_bounds__(64) k_bootstrap(DParams P, uint32_t n, float *lum_out) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t nd;
    DSplat s = eval_boot_sample(P, i, nd);
    lum_out[i] = s.lum;
    if (P.boot_weighted) { normalize_splat(s, P); lum_out[(size_t) n + i] = s.lum; } // luminance of f / importance
}

__global__ void __launch_bounds__(64) k_init_chains(DParams P, const uint32_t *seed_index, const float *seed_lum) {
    uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= P.n_chains) return;
    Sampler smp;
    smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = P.boot_stream; smp.major = seed_index[c];
    smp.mode = SM_BOOT; smp.arr = nullptr;
    uint32_t nd;
    DSplat s = eval_boot_sample(P, smp.major, nd);
    // sanity check of drmlt_proc.cpp:509-512: same function, same inputs -> bit-equal on the device
    if (!(s.lum == seed_lum[c])) atomicExch(P.error_flag, 1);
    normalize_splat(s, P);
    P.cur_lum[c] = s.lum; P.cur_px[c] = s.px; P.cur_py[c] = s.py;
    P.cur_r[c] = s.r; P.cur_g[c] = s.g; P.cur_b[c] = s.b;
    P.chain_depth[c] = (int32_t) nd; // pssmlt: components that exist after the replay (no fillReplay there)
    // replayed components + fillReplay top-up: dimension k of bootstrap sample i is U(BOOT, i, k)
    smp.reset_caches();
    for (uint32_t k = 0; k < (uint32_t) P.eff_dim; ++k) P.x[(size_t) k * P.n_chains + c] = smp.u_boot(k, TAG_BOOT);
}

// ------------------------------------------------------------------------------------------
// k_mutate_pssmlt: PSSMLTRenderer::process (src/integrators/pssmlt/pssmlt_proc.cpp:113-297) over sampleSplats(path).
// One proposal per mutation, Kelemen-style weights (with b and pLarge) or Veach's expectations, and the deferred splat
// of the current state with its cumulative weight (:215-226,262-266). The cumulative weight is flushed at the end of
// every launch (the reference does it once per work unit; splatting is linear, so the film is the same).
__global__ void __launch_bounds__(CHAIN_BLOCK) k_mutate_pssmlt(DParams P, uint32_t n_mut, uint32_t mut_base) {
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x * CHAIN_BLOCK + lane;
    const bool live = c < P.n_chains;
    const uint32_t cc = live ? c : P.n_chains - 1;
    const int D = P.eff_dim;
    for (int k = 0; k < D; ++k) lds_x[k * 64 + lane] = P.x[(size_t) k * P.n_chains + cc];
    DSplat cur;
    cur.lum = P.cur_lum[cc]; cur.px = P.cur_px[cc]; cur.py = P.cur_py[cc];
    cur.r = P.cur_r[cc]; cur.g = P.cur_g[cc]; cur.b = P.cur_b[cc];
    PssmltSampler smp;
    smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = P.chain_offset + cc;
    smp.kelemen = P.kelemen_mutation != 0; smp.sigma = P.pss_sigma; smp.lane = lane;
    smp.n_exist = mut_base == 0u ? (uint32_t) min(P.chain_depth[cc], D) : (uint32_t) D;
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    float cumulative = 0.f;
    const float b = P.luminance_b, pLarge = P.p_large;

    if (live) for (uint32_t it = 0; it < n_mut; ++it) {
        const uint32_t m = mut_base + it;
        const u4 coins = philox4x32_10(P.key0, P.key1, 0u, m, smp.chain, TAG_COIN);
        const bool large = u32_to_unit(coins.x) < pLarge;
        smp.major = m; smp.large = large;
        smp.reset_caches();
        uint32_t nr, nd;
        DSplat y = eval_path(P, smp, nr, nd);
        ct.rays += nr;
        normalize_splat(y, P);
        float a = fminf(1.f, y.lum / cur.lum);
        if (isnan(y.lum) || y.lum < 0.f) a = 0.f; // :188-191
        bool accept = false;
        float wc, wp = 0.f;
        if (a > 0.f) {
            if (P.kelemen_weights && !P.importance) { // :197-203: "Kelemen-style weights don't work for 2-stage MLT" (the a <= 0 branch keeps them)
                wc = (1.f - a) * cur.lum / (cur.lum / b + pLarge);
                wp = (a + (large ? 1.f : 0.f)) * y.lum / (y.lum / b + pLarge);
            } else {
                wc = 1.f - a;
                wp = a;
            }
            accept = a == 1.f || u32_to_unit(coins.y) < a;
        } else {
            wc = P.kelemen_weights ? cur.lum / (cur.lum / b + pLarge) : 1.f;
        }
        cumulative += wc;
        mh_count(ct, large, accept, false, false);
        // the whole vector was rewritten by the proposal; components that did not exist yet stay even on rejection
        const uint32_t n_exist = smp.n_exist;
        if (accept) {
            film_put(P, cur.px, cur.py, mk3(cur.r * cumulative, cur.g * cumulative, cur.b * cumulative));
            cumulative = wp;
            for (int k = 0; k < D; ++k) lds_x[k * 64 + lane] = smp.next((uint32_t) k);
            cur = y;
        } else {
            film_put(P, y.px, y.py, mk3(y.r * wp, y.g * wp, y.b * wp));
            for (uint32_t k = n_exist; k < (uint32_t) D; ++k) lds_x[k * 64u + lane] = smp.next(k);
        }
        smp.n_exist = (uint32_t) D;
    }
    if (live) {
        film_put(P, cur.px, cur.py, mk3(cur.r * cumulative, cur.g * cumulative, cur.b * cumulative)); // "Perform the last splat"
        for (int k = 0; k < D; ++k) P.x[(size_t) k * P.n_chains + c] = lds_x[k * 64 + lane];
        P.cur_lum[c] = cur.lum; P.cur_px[c] = cur.px; P.cur_py[c] = cur.py;
        P.cur_r[c] = cur.r; P.cur_g[c] = cur.g; P.cur_b[c] = cur.b;
    }
    flush_counters(P, ct, lane);
}

__global__ void __launch_bounds__(64) k_eval_paths(DParams P, const float *u, uint32_t n, uint32_t dim, float *out8) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Sampler smp;
    smp.key0 = smp.key1 = smp.chain = smp.major = 0u;
    smp.mode = SM_ARRAY;
    smp.arr = u + (size_t) i * dim;
    uint32_t nr, nd;
    DSplat s = eval_path(P, smp, nr, nd);
    float *o = out8 + (size_t) i * 8;
    o[0] = s.lum; o[1] = s.px; o[2] = s.py; o[3] = s.r; o[4] = s.g; o[5] = s.b;
    o[6] = __int_as_float((int) nd); o[7] = __int_as_float((int) nr);
}

__global__ void __launch_bounds__(64) k_render_pt(DParams P, uint64_t n_samples, uint32_t stream, float scale) {
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (; i < n_samples; i += stride) {
        Sampler smp;
        smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = stream + (uint32_t) (i >> 32); smp.major = (uint32_t) i;
        smp.mode = SM_PT; smp.arr = nullptr;
        uint32_t nr, nd;
        DSplat s = eval_path(P, smp, nr, nd);
        if (s.lum > 0.f) film_put(P, s.px, s.py, mk3(s.r * scale, s.g * scale, s.b * scale));
    }
}

// sum of pixel luminances in double (one atomic per block)
__global__ void __launch_bounds__(256) k_lum_sum(const float *film, const float *importance, uint32_t n_pixels, double *sum) {
    __shared__ double part[256];
    double acc = 0.0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pixels; i += gridDim.x * blockDim.x)
        acc += ((double) film[3 * i] * 0.212671 + (double) film[3 * i + 1] * 0.715160 + (double) film[3 * i + 2] * 0.072169) *
               (importance ? (double) importance[i] : 1.0); // drmlt_proc.cpp:826-832
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int) threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(sum, part[0]);
}

__global__ void __launch_bounds__(256) k_develop(const float *film, const float *direct, const float *importance, float factor, uint32_t n,
                                                 float *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = film[i] * (importance ? factor * importance[i / 3u] : factor) + (direct ? direct[i] : 0.f); // :841-847
}

__global__ void k_set_u32(uint32_t *p, uint32_t v) { *p = v; }
void launch_set_u32(uint32_t *p, uint32_t v, hipStream_t st) { hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, st, p, v); }
__global__ void k_set2(double *p, double a, double b) { p[0] = a; p[1] = b; }
void launch_set2(double *p, double a, double b, hipStream_t st) { hipLaunchKernelGGL(k_set2, dim3(1), dim3(1), 0, st, p, a, b); }

// Grids of the film kernels are capped (grid-stride loops): a launch of MORE than 2048 workgroups in front of a chain kernel
// costs that kernel 14 % (k_mutate_v4 41.0 -> 47.0 ms after a 3072-block develop, whatever the develop reads or writes;
// 2048 blocks and fewer: no effect) -- the chain kernel's 2048 workgroups fill the device exactly, eight to a CU, two to a
// SIMD, and whatever the dispatcher still holds of the larger grid skews that placement.
#define AUX_GRID_CAP 1024u
// the same with the factor taken from device memory: scal = {sum of the film's luminance over all ranks, sum of the ranks' b}
// (drmlt_exchange_tiled without a host round trip: the exchange of a step is enqueued behind its chain kernel)
__global__ void __launch_bounds__(256) k_develop_dev(const float *film, const float *importance, const double *scal, float inv_world, float inv_pixels,
                                                     int acceptance_map, uint32_t n, float *out) {
    const float factor = acceptance_map ? 1.f : (float) ((scal[1] * (double) inv_world) / (scal[0] * (double) inv_pixels));
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = film[i] * (importance ? factor * importance[i / 3u] : factor);
}

// dst += src (film tiles of ranks that share a device: drmlt_node.cpp's loopback transport)
__global__ void __launch_bounds__(256) k_accumulate(float *dst, const float *src, size_t n) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) dst[i] += src[i];
}
void launch_accumulate(float *dst, const float *src, size_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_accumulate, dim3((unsigned) std::min<size_t>((n + 255) / 256, AUX_GRID_CAP)), dim3(256), 0, st, dst, src, n);
}

// ---- host-callable launchers (C++ linkage, used by drmlt_capi.cpp) --------------------------
void launch_bootstrap(const DParams &P, uint32_t n, float *lum_out, hipStream_t st) {
    hipLaunchKernelGGL(k_bootstrap, dim3((n + 63) / 64), dim3(64), 0, st, P, n, lum_out);
}
void launch_init_chains(const DParams &P, const uint32_t *seed_index, const float *seed_lum, hipStream_t st) {
    hipLaunchKernelGGL(k_init_chains, dim3((P.n_chains + 63) / 64), dim3(64), 0, st, P, seed_index, seed_lum);
}
// technique=path's chain kernels: the build drmlt_create chose (launch_plan.h: plan_chains), with its grid and LDS. The DRMLT
// families have a launcher each, beside their kernels (kernels_v3.hip, kernels_v4.hip); a build that is not of the
// plan's family -- the bidirectional ones, which drmlt_run never sends here -- ends in that launcher's abort.
void launch_mutate_v3(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_mutate_v4(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_mutate_v5(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st);
void launch_mutate(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st) {
    if (plan.verbose && !plan.note.empty()) fprintf(stderr, "%s\n", plan.note.c_str());
    switch (plan.build) {
    case Build::PSSMLT: hipLaunchKernelGGL(k_mutate_pssmlt, dim3(plan.grid), dim3(CHAIN_BLOCK), plan.lds, st, P, n_mut, mut_base); break;
    default:
        if (plan.kernel_variant == 5) launch_mutate_v5(plan, P, n_mut, mut_base, st);
        else if (plan.kernel_variant == 4) launch_mutate_v4(plan, P, n_mut, mut_base, st);
        else launch_mutate_v3(plan, P, n_mut, mut_base, st);
    }
}
void launch_eval_paths(const DParams &P, const float *u, uint32_t n, uint32_t dim, float *out8, hipStream_t st) {
    hipLaunchKernelGGL(k_eval_paths, dim3((n + 63) / 64), dim3(64), 0, st, P, u, n, dim, out8);
}
void launch_render_pt(const DParams &P, uint64_t n_samples, uint32_t stream, float scale, hipStream_t st) {
    hipLaunchKernelGGL(k_render_pt, dim3(16384), dim3(64), 0, st, P, n_samples, stream, scale);
}
void launch_lum_sum(const float *film, const float *importance, uint32_t n_pixels, double *sum, hipStream_t st) {
    hipLaunchKernelGGL(k_lum_sum, dim3(256), dim3(256), 0, st, film, importance, n_pixels, sum);
}
void launch_develop_dev(const float *film, const float *importance, const double *scal, float inv_world, float inv_pixels, int acceptance_map, uint32_t n,
                        float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_develop_dev, dim3(std::min((n + 255) / 256, AUX_GRID_CAP)), dim3(256), 0, st, film, importance, scal, inv_world, inv_pixels, acceptance_map, n, out);
}
void launch_develop(const float *film, const float *direct, const float *importance, float factor, uint32_t n, float *out, hipStream_t st) {
    hipLaunchKernelGGL(k_develop, dim3(std::min((n + 255) / 256, AUX_GRID_CAP)), dim3(256), 0, st, film, direct, importance, factor, n, out);
}
