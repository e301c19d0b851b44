// Independent samples of the bidirectional integrand into a film (gfx950): the reference image of technique=bdpt and
// technique=mmlt, as k_render_pt is technique=path's.
//
//   k_render_bdpt   for every sample one PathSampler::sampleSplats(EBidirectional) (src/libbidir/pathsampler.cpp:321-527) on fresh
//                   uniform random numbers -- eval_bdpt, as k_bootstrap_bdpt calls it -- and the WHOLE splat list, the sensor-side
//                   splat and every light-image splat, through the scene's filter into P.film
//
// Sample i reads the random numbers of bootstrap sample i of stream 0 (SM_BOOT, chain = 0, major = i): the list whose luminance
// drmlt_bootstrap_luminances(seed, 0, n) reports at index i is the list that reaches the film here. Workspace, LDS rows and
// scratch list (slot 1) are the bootstrap's (kernels_bdpt.hip); tables are read from device memory (GlobalTables) and the
// evaluation is built for the widest feature set (FEAT 15), as there.
#include <cstdlib>
#include "bdpt_lists.h"

// `scale`: 1 / spp. n < 2^32 (the sample's address is 32 bits); the round counter is 64 bits wide because the last round's
// i0 + n_chains_alloc may pass 2^32.
__global__ void __launch_bounds__(CHAIN_BLOCK) k_render_bdpt(DParams P, uint32_t n, float scale) {
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blockIdx.x * CHAIN_BLOCK + lane; // workspace column
    const bool has_col = c < P.n_chains_alloc;
    const uint32_t cc = has_col ? c : P.n_chains_alloc - 1u;
    MSampler smp;
    msampler_setup(smp, P, lane, false);
    smp.chain = 0u; smp.mode = SM_BOOT;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    float *const L = list_col(P, 1, cc);
    for (unsigned long long i0 = (unsigned long long) blockIdx.x * CHAIN_BLOCK; i0 < n; i0 += P.n_chains_alloc) { // the whole wave makes every call (eval_bdpt)
        const unsigned long long i = i0 + lane;
        const bool active = has_col && i < n;
        smp.major = (uint32_t) i;
        BdptResult R;
        eval_bdpt(P, T, smp, active, cc, bdpt_nx_lds(P), L, R);
        if (active) list_splat_scaled(P, L, scale);
    }
}

void launch_render_bdpt(const DParams &P, uint32_t n, float scale, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_render_bdpt, dim3((P.n_chains_alloc + CHAIN_BLOCK - 1) / CHAIN_BLOCK), dim3(CHAIN_BLOCK), lds, st, P, n, scale);
}
