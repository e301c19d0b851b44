// The bidirectional estimate split by path length and strategy (gfx950): Veach's "pyramid", one film per (depth d, s) with
// d = s + t - 1 edges. What the reference's BDPT writes only under a compile-time switch (BDPT_DEBUG, bdpt_wr.cpp:53-71).
//
//   k_layers_bdpt   k_render_bdpt's loop -- sample i is bootstrap sample i of stream 0, one sampleSplats(EBidirectional)
//                   (src/libbidir/pathsampler.cpp:369-521) each -- with a sink on eval_bdpt's cells: every produced cell goes
//                   through the scene's filter into layer bdpt_layer_index(d, s) of a layered film, with its MIS weight
//                   (Path::miWeight, src/libbidir/path.cpp:763-1028) or without it
//
// The splat list the evaluation writes (slot 1, the bootstrap's scratch) is not used: the cells reach the film one by one
// instead of summed into the list's main splat. Workspace, LDS rows and tables are k_render_bdpt's.
#include <cstdlib>
#include "bdpt_lists.h"
#include "bdpt_layers.h"

// film_put (kernel_common.h) into a film that is not P.film: the same validity test, footprint and weights
DEV void layer_put(const DParams &P, float *film, float px, float py, f3 v) {
    if (P.debug & 1) return;
    if (!(isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) || v.x < 0.f || v.y < 0.f || v.z < 0.f) return;
    const float posx = px - 0.5f, posy = py - 0.5f;
    const int minx = max((int) ceilf(posx - P.filter_radius), 0), miny = max((int) ceilf(posy - P.filter_radius), 0);
    const int maxx = min((int) floorf(posx + P.filter_radius), P.width - 1), maxy = min((int) floorf(posy + P.filter_radius), P.height - 1);
    const bool box = P.box_weight > 0.f;
    for (int y = miny; y <= maxy; ++y) {
        const int iy = min((int) fabsf(((float) y - posy) * P.filter_scale), 31);
        const float wy = box ? (iy < 31 ? P.box_weight : 0.f) : P.filter_lut[iy];
        for (int x = minx; x <= maxx; ++x) {
            const int ix = min((int) fabsf(((float) x - posx) * P.filter_scale), 31);
            const float w = (box ? (ix < 31 ? P.box_weight : 0.f) : P.filter_lut[ix]) * wy;
            float *dst = film + ((size_t) y * P.width + x) * 3;
            atomic_add_global_f32(dst + 0, w * v.x);
            atomic_add_global_f32(dst + 1, w * v.y);
            atomic_add_global_f32(dst + 2, w * v.z);
        }
    }
}

// eval_bdpt's sink (device_bdpt.h): called by the whole wave, once per cell. Nothing here is wave-cooperative -- the film position
// arrives already read from the chain's lane -- so a lane without a produced cell just leaves.
struct LayerSink {
    static constexpr bool enabled = true;
    const DParams &P;
    float *layers;      // bdpt_layer_count(max_depth) films of height x width x 3
    float scale;        // 1 / spp, the same for every chain of the grid
    bool unweighted;    // DRMLT_LAYERS_UNWEIGHTED: the value before the division by miWeight's sum
    DEV void operator()(int s, int t, float px, float py, f3 value, float weight, bool produced, uint32_t) const {
        if (!produced) return;
        const int layer = bdpt_layer_index(s + t - 1, s);
        if (layer < 0 || s + t - 1 > P.max_depth) return; // (no cell lies outside the table: the film is never written past its end)
        if (unweighted) value = value * weight;
        layer_put(P, layers + (size_t) layer * ((size_t) P.width * P.height * 3), px, py, value * scale);
    }
};

// n < 2^32, as for k_render_bdpt
__global__ void __launch_bounds__(CHAIN_BLOCK) k_layers_bdpt(DParams P, uint32_t n, float scale, float *layers, int unweighted) {
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x * CHAIN_BLOCK + lane; // workspace column
    const bool has_col = c < P.n_chains_alloc;
    const uint32_t cc = has_col ? c : P.n_chains_alloc - 1u;
    MSampler smp;
    msampler_setup(smp, P, lane, false);
    smp.chain = 0u; smp.mode = SM_BOOT;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    float *const L = list_col(P, 1, cc);
    const LayerSink sink{P, layers, scale, unweighted != 0};
    for (unsigned long long i0 = (unsigned long long) blockIdx.x * CHAIN_BLOCK; i0 < n; i0 += P.n_chains_alloc) { // the whole wave makes every call (eval_bdpt)
        const unsigned long long i = i0 + lane;
        const bool active = has_col && i < n;
        smp.major = (uint32_t) i;
        BdptResult R;
        eval_bdpt(P, T, smp, active, cc, bdpt_nx_lds(P), L, R, sink);
    }
}

void launch_layers_bdpt(const DParams &P, uint32_t n, float scale, float *layers, int unweighted, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_layers_bdpt, dim3((P.n_chains_alloc + CHAIN_BLOCK - 1) / CHAIN_BLOCK), dim3(CHAIN_BLOCK), lds, st, P, n, scale, layers, unweighted);
}
