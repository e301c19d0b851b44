// The unidirectional estimate split by path length and strategy (gfx950): one film per (depth d, strategy), d the number of edges
// from the camera to the emitter, strategy the way the emitter was found -- by the BSDF-sampled ray (DRMLT_PT_HIT: an area light it
// hits or the environment it escapes to, path.cpp:253-285) or by the light sample (DRMLT_PT_DIRECT, path.cpp:187-238).
//
//   k_render_pt_layers   k_render_pt's loop -- sample i reads the random numbers of render_pt's sample i -- with a sink on
//                        path_step's additions to Li (device_path.h: PathNoSink): every term goes through the scene's filter into
//                        layer pt_layer_index(d, strategy) of a layered film, with its power-heuristic weight or without it
//
// A sample that path_step voids (a vertex normal without direction: Li = 0) is in no layer, as it is not in render_pt's image, so a
// sample's terms wait in LDS until it ends: 6 maxDepth + 1 floats per lane, slot j of lane l at lds_x[j * 64 + l] (no bank
// conflicts, no barrier: a lane reads what it wrote itself). Slot 3 * layer + channel holds the layer's term -- a sample has at most
// one per layer -- and the last slot the voided mark. The flags are kernels.hip's: path_step must round here as in k_render_pt.
#include "kernel_common.h"
#include "layer_film.h"
#include "pt_layers.h"

// path_step's sink (device_path.h). `row`: this lane's column of the block's LDS rows. A depth outside 2 .. max_depth has no slot
// and is dropped (path_step produces none: the row is never written past its end).
struct PtLayerSink {
    static constexpr bool enabled = true;
    float *row;
    int max_depth;
    bool unweighted; // DRMLT_LAYERS_UNWEIGHTED: the term without its power-heuristic factor
    DEV void put(int d, int strategy, f3 v) const {
        if (d < 2 || d > max_depth) return;
        float *const s = row + (size_t) (3 * pt_layer_index(d, strategy)) * 64;
        s[0] = v.x; s[64] = v.y; s[128] = v.z;
    }
    DEV void hit(int d, f3 term, float weight) const { put(d, 0, unweighted ? term : term * weight); }
    // the light sample's term takes its slot when it is parked and leaves it again if the shadow ray is blocked
    DEV void park(int d, f3 term, float weight) const { put(d, 1, unweighted ? term : term * weight); }
    DEV void shadow(int d, bool clear) const { if (!clear) put(d, 1, mk3(0.f, 0.f, 0.f)); }
    DEV void voided() const { row[(size_t) (6 * max_depth) * 64] = 1.f; }
};

// n < 2^32: the sample address is Sampler::major alone, as for k_render_pt's first 2^32 samples. max_depth in 1 .. PT_LAYERS_MAX_DEPTH
// (drmlt_render_pt_layers refuses the rest); dynamic LDS: (6 max_depth + 1) * 64 floats.
__global__ void __launch_bounds__(64) k_render_pt_layers(DParams P, uint32_t n, float scale, double *layers, int unweighted) {
    float *const row = lds_x + threadIdx.x;
    const int n_slots = 6 * P.max_depth + 1;
    const size_t film_floats = (size_t) P.width * P.height * 3;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    const PtLayerSink sink{row, P.max_depth, unweighted != 0};
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        Sampler smp;
        smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = 0u; smp.major = (uint32_t) i;
        smp.mode = SM_PT; smp.arr = nullptr;
        for (int j = 0; j < n_slots; ++j) row[(size_t) j * 64] = 0.f;
        // eval_path's loop (device_path.h) with the sink
        PathState ps;
        smp.reset_caches();
        path_init(P, ps);
        Hit h{-1, 0.f, 0.f, 0.f};
        ShadowRay sr_unused;
        for (;;) {
            if (ps.phase != PH_BEGIN) h = trace(P, ps.o, ps.d, ps.tmin, ps.tmax, ps.phase == PH_SHADOW);
            path_step<false, 15>(P, T, ps, smp, h, false, sr_unused, sink);
            if (ps.phase == PH_DONE) break;
        }
        // a sample render_pt leaves out whole -- voided, or a sum that is not finite -- is left out whole here
        if (row[(size_t) (n_slots - 1) * 64] != 0.f || !(isfinite(ps.Li.x) && isfinite(ps.Li.y) && isfinite(ps.Li.z))) continue;
        for (int layer = 2; layer < 2 * P.max_depth; ++layer) { // (both d = 1 layers stay empty)
            const float *const s = row + (size_t) (3 * layer) * 64;
            const f3 v = mk3(s[0], s[64], s[128]);
            if (!is_zero3(v)) layer_put_f64(P, layers + (size_t) layer * film_floats, ps.px, ps.py, v * scale);
        }
    }
}

void launch_render_pt_layers(const DParams &P, uint32_t n, float scale, double *layers, int unweighted, hipStream_t st) {
    const size_t lds = (size_t) (6 * P.max_depth + 1) * 64 * sizeof(float);
    hipLaunchKernelGGL(k_render_pt_layers, dim3(16384), dim3(64), lds, st, P, n, scale, layers, unweighted);
}
