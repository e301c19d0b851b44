// The fp64 film of the reference renders that are compared bit for bit (drmlt_render_pt_layers, drmlt_render_mmlt,
// drmlt_render_mmlt_layers): film_put (kernel_common.h) into a film of doubles that is not P.film. One copy for the units that
// render into such a film (kernels_layers_pt.hip, kernels_render_mmlt.hip).
#pragma once
#include "kernel_common.h"

// no-return double add on device memory (global_atomic_add_f64)
DEV void atomic_add_global_f64(double *p, double v) {
    (void) __hip_atomic_fetch_add((double __attribute__((address_space(1))) *) (uintptr_t) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// film_put (kernel_common.h) into a film that is not P.film: the same validity test, footprint and fp32 weights and products. The
// film is fp64 and the host rounds it to fp32 once, at the end: the order in which the atomics arrive moves a pixel's sum by some
// 2^-53 relative per add instead of 2^-24, so two launches of the same samples give the same fp32 bits unless a sum lies that
// close to a rounding boundary (about 1e-8 per pixel channel at 64 terms) -- what lets two renders, or the two modes of a layered
// one where the weight is 1 by construction, be compared bit for bit.
DEV void layer_put_f64(const DParams &P, double *film, float px, float py, f3 v) {
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
            double *dst = film + ((size_t) y * P.width + x) * 3;
            atomic_add_global_f64(dst + 0, (double) (w * v.x));
            atomic_add_global_f64(dst + 1, (double) (w * v.y));
            atomic_add_global_f64(dst + 2, (double) (w * v.z));
        }
    }
}
