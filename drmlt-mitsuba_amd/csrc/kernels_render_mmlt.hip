// Independent samples of the multiplexed estimator into a film (gfx950): technique=mmlt's own equal-expectation reference, whole
// and split by path length and strategy.
//
//   k_render_mmlt   sample i is bootstrap sample i of stream 0 -- depth (i % maxDepth) + 1 (pathsampler.cpp:889), one
//                   sampleSplats(EMMLT) (src/libbidir/pathsampler.cpp:84-320, eval_mmlt) each, the random numbers k_bootstrap_mmlt
//                   reads -- and its one splat goes through the scene's filter into an fp64 film, scaled by 1 / spp
//   k_layers_mmlt   the same samples, each into layer bdpt_layer_index(depth, s) of a layered fp64 film, s the strategy the sample
//                   drew: as eval_mmlt returns it (value x MIS weight x number of strategies) or, through eval_mmlt's sink, without
//                   the MIS weight
//
// Sampler setup, LDS rows (the MIS scratch behind mmlt_nx(P) rows), tables and feature set are k_bootstrap_mmlt's. The grid is fixed
// (launch_render_mmlt) and every lane strides over the samples: n is bounded by 2^32 only, and one workgroup per 64 samples would be
// 6.7e7 workgroups there, each paying the sampler setup and its kernel arguments for one evaluation; the traversal's overflow area
// is sized by the lanes of the grid, which stay 262 144 whatever n is.
#include <algorithm>
#include "device_bidir.h"
#include "kernel_common.h"
#include "layer_film.h"
#include "bdpt_layers.h"

#define RENDER_MMLT_GRID 4096u // workgroups of one wave: 16 per compute unit of an MI355X, two rounds at two waves per SIMD

// eval_mmlt's sink (device_bidir.h): keeps the sum of the MIS sweep for the sample's lane
struct MmltMisSink {
    double *sum;
    DEV void mis_sum(double w) const { *sum = w; }
};

// n < 2^32: the sample address is MSampler::major alone. films: one film (LAYERS false) or bdpt_layer_count(max_depth) of them.
template <bool LAYERS> DEV void render_mmlt_samples(const DParams &P, uint32_t n, float scale, double *films, bool unweighted) {
    const uint32_t lane = threadIdx.x;
    MSampler smp;
    msampler_setup(smp, P, lane, true);
    smp.chain = P.boot_stream; smp.mode = SM_BOOT;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    const size_t film_doubles = (size_t) P.width * P.height * 3;
    const uint64_t stride = (uint64_t) gridDim.x * CHAIN_BLOCK;
    for (uint64_t i = (uint64_t) blockIdx.x * CHAIN_BLOCK + lane; i < n; i += stride) {
        smp.major = (uint32_t) i;
        const int depth = (int) ((uint32_t) i % (uint32_t) P.max_depth) + 1;
        MmltResult R;
        f3 v;
        if (LAYERS) {
            double mis = 1.0;
            eval_mmlt(P, T, smp, depth, mmlt_nx(P), R, MmltMisSink{&mis});
            v = mk3(R.splat.r, R.splat.g, R.splat.b);
            // the splat is value x (1 / sum) x strategies, the division in fp32: times the sum it is the strategy used alone
            if (unweighted) v = mk3((float) ((double) v.x * mis), (float) ((double) v.y * mis), (float) ((double) v.z * mis));
        } else {
            eval_mmlt(P, T, smp, depth, mmlt_nx(P), R);
            v = mk3(R.splat.r, R.splat.g, R.splat.b);
        }
        if (is_zero3(v)) continue; // (depth 1, a failed walk, a blocked connection, a light-image position off the film)
        size_t film = 0;
        if (LAYERS) {
            const int layer = bdpt_layer_index(depth, R.s);
            if (layer < 0) continue; // (no sample lies outside the table: the film is never written past its end)
            film = (size_t) layer * film_doubles;
        }
        layer_put_f64(P, films + film, R.splat.px, R.splat.py, v * scale);
    }
}

__global__ void __launch_bounds__(CHAIN_BLOCK) k_render_mmlt(DParams P, uint32_t n, float scale, double *film) {
    render_mmlt_samples<false>(P, n, scale, film, false);
}
__global__ void __launch_bounds__(CHAIN_BLOCK) k_layers_mmlt(DParams P, uint32_t n, float scale, double *layers, int unweighted) {
    render_mmlt_samples<true>(P, n, scale, layers, unweighted != 0);
}

uint32_t render_mmlt_grid(uint32_t n) { return std::min<uint32_t>(RENDER_MMLT_GRID, (uint32_t) (((uint64_t) n + CHAIN_BLOCK - 1) / CHAIN_BLOCK)); }
void launch_render_mmlt(const DParams &P, uint32_t n, float scale, double *film, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_render_mmlt, dim3(render_mmlt_grid(n)), dim3(CHAIN_BLOCK), lds, st, P, n, scale, film);
}
void launch_layers_mmlt(const DParams &P, uint32_t n, float scale, double *layers, int unweighted, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_layers_mmlt, dim3(render_mmlt_grid(n)), dim3(CHAIN_BLOCK), lds, st, P, n, scale, layers, unweighted);
}
