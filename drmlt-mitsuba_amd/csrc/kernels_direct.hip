// HIP kernels of the direct-illumination pass for gfx950 (MI355X): BidirectionalUtils::renderDirectComponent
// (src/libbidir/util.cpp:30-92) -- the image DRMLTProcess::develop adds to the chains' film when directSamples > 0.
//
//   k_render_direct<FEAT>   one work item = one pixel sample: camera ray, MIDirectIntegrator::Li with its shading-sample loop
//                           (device_direct.h), the scene's filter into a 4-channel film (rgb and weight)
//   k_direct_normalise      hdrfilm's develop of that film: rgb / weight
//
// Built, like the other utility kernels, for the widest feature set of flat scenes (7) and of traversed scenes (15); the tables are
// read from device memory (GlobalTables), as k_render_pt and k_bootstrap read them.
#include <algorithm>
#include "device_direct.h"

// A wave's 64 lanes hold 64 / G pixels with G = 2^group_log2 sample slots each (pixelSamples <= 8 after the split, so G <= 8; slots
// beyond pixelSamples idle). Pixels are numbered row-major over the rows [samp_lo, samp_hi); the grid strides over them. What a
// work item computes depends on (seed, pixel, sample) alone, and the film sums a pixel's samples in an order fixed by G: neither
// the grid nor the row range nor the lane a sample lands in changes a bit of the box-filtered image.
template <int FEAT>
__global__ void __launch_bounds__(64) k_render_direct(DParams P, DirectJob J) {
    const uint32_t lane = threadIdx.x;
    const uint32_t per_wave = 64u >> J.group_log2, slot = lane >> J.group_log2, sample = lane & ((1u << J.group_log2) - 1u);
    const uint32_t W = (uint32_t) P.width, n_pix = (uint32_t) (J.samp_hi - J.samp_lo) * W;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    for (uint32_t base = blockIdx.x * per_wave; base < n_pix; base += gridDim.x * per_wave) { // wave-uniform trip count
        const uint32_t q = base + slot;
        const bool have = q < n_pix, live = have && sample < (uint32_t) J.pixel_samples;
        const uint32_t qq = have ? q : n_pix - 1u;
        const int X = (int) (qq % W), Y = J.samp_lo + (int) (qq / W);
        float px = (float) X + 0.5f, py = (float) Y + 0.5f;
        f3 L = mk3(0.f, 0.f, 0.f);
        if (live) {
            const uint32_t pixel = (uint32_t) Y * W + (uint32_t) X;
            const u4 sc = philox4x32_10(J.key0, J.key1, 0u, pixel, DIRECT_PIXEL_STREAM, TAG_DIRECT); // the pixel's scramble
            px = (float) X + direct_vdc(sample, sc.x); py = (float) Y + direct_sobol2(sample, sc.y);
            PathState ps; // the camera ray of path_begin (perspective.cpp:271-286); nothing else of the state is used
            path_begin(P, ps, px / (float) P.width, py / (float) P.height);
            L = direct_li<FEAT>(P, T, J, ps.o, ps.d, ps.tmin, ps.tmax, pixel, sample);
        }
        direct_film_put(P, J, live, have, lane, X, Y, px, py, L);
    }
}

__global__ void __launch_bounds__(256) k_direct_normalise(const float *acc, uint32_t n_pix, float *out) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += gridDim.x * blockDim.x) {
        const float4 a = reinterpret_cast<const float4 *>(acc)[i];
        const float inv = a.w > 0.f ? 1.f / a.w : 0.f; // a pixel no sample reached stays black
        out[3 * i] = a.x * inv; out[3 * i + 1] = a.y * inv; out[3 * i + 2] = a.z * inv;
    }
}

// Grid cap (grid-stride above it), as AUX_GRID_CAP of the film kernels in kernels.hip and for its reason: 2048 one-wave workgroups
// fill the device eight to a CU, and no larger grid is left in the dispatcher in front of a chain kernel.
#define DIRECT_GRID_CAP 2048u
uint32_t direct_grid(const DirectJob &J, int width) {
    const uint64_t n_pix = (uint64_t) (J.samp_hi - J.samp_lo) * (uint64_t) width, per_wave = 64u >> J.group_log2;
    return (uint32_t) std::min<uint64_t>((n_pix + per_wave - 1) / per_wave, DIRECT_GRID_CAP);
}
// Enqueues the pass on `st`; allocates nothing (J.acc: zeroed by the caller, `out`: (row_hi - row_lo) * W * 3 floats, both device)
void launch_render_direct(const DParams &P, const DirectJob &J, float *out, hipStream_t st) {
    const uint32_t grid = direct_grid(J, P.width), n_out = (uint32_t) (J.row_hi - J.row_lo) * (uint32_t) P.width;
    if (P.use_bvh) hipLaunchKernelGGL(k_render_direct<15>, dim3(grid), dim3(64), 0, st, P, J);
    else hipLaunchKernelGGL(k_render_direct<7>, dim3(grid), dim3(64), 0, st, P, J);
    hipLaunchKernelGGL(k_direct_normalise, dim3(std::min((n_out + 255u) / 256u, 1024u)), dim3(256), 0, st, J.acc, n_out, out);
}
