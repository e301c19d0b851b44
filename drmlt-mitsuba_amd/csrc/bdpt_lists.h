// Splat lists of technique=bdpt as the chain kernels handle them (kernels_bdpt.hip: k_mutate_bdpt, kernels_pssmlt_bdpt.hip:
// k_mutate_pssmlt_bdpt): a chain's column of a list slot, SplatList::normalize under an importance map, splatting, copying.
// Lists live in HBM (`bd_lists`, slot 0 = current state), unnormalised next to their luminance.
#pragma once
#include "device_bdpt.h"
#include "kernel_common.h"

DEV uint32_t bdpt_nx(const DParams &P) { return (uint32_t) (P.mmlt_S + P.mmlt_E + P.bd_Dd); } // components of a chain's state
DEV uint32_t bdpt_nx_lds(const DParams &P) { return (uint32_t) (P.mmlt_S + P.mmlt_E); }        // ... of which LDS holds the two walks'

DEV float *list_col(const DParams &P, int slot, uint32_t chain) {
    return P.bd_lists + (size_t) slot * (size_t) bdpt_list_rows(P.max_depth) * P.n_chains_alloc + chain;
}

// SplatList::normalize with a two-stage importance map (pathsampler.cpp:1001-1020): weigh every splat, recompute the
// list luminance. Lists stay unnormalised otherwise; the 1 / luminance factor is applied when splatting.
DEV float list_finalize(const DParams &P, float *list, float lum) {
    if (!P.importance) return lum;
    const size_t n = P.n_chains_alloc;
    const int meta = __float_as_int(list[(size_t) BL_META * n]);
    const int cnt = meta >> 1;
    float total = 0.f;
    for (int k = -1; k < cnt; ++k) {
        if (k < 0 && !(meta & 1)) continue;
        const int r0 = k < 0 ? BL_MAIN : BL_MORE + 5 * k;
        float r = list[(size_t) (r0 + 2) * n], g = list[(size_t) (r0 + 3) * n], b = list[(size_t) (r0 + 4) * n];
        if (r == 0.f && g == 0.f && b == 0.f) continue;
        const int ix = min(max(0, (int) list[(size_t) r0 * n]), P.width - 1), iy = min(max(0, (int) list[(size_t) (r0 + 1) * n]), P.height - 1);
        const float lv = P.importance[ix + iy * P.width];
        r /= lv; g /= lv; b /= lv;
        list[(size_t) (r0 + 2) * n] = r; list[(size_t) (r0 + 3) * n] = g; list[(size_t) (r0 + 4) * n] = b;
        total += luminance3(mk3(r, g, b));
    }
    list[(size_t) BL_LUM * n] = total;
    return total;
}

// splat every entry of a list with weight w / luminance (the list is stored unnormalised)
DEV void list_splat(const DParams &P, const float *list, float lum, float w) {
    if (!(w > 0.f) || !(lum > 0.f)) return;
    const size_t n = P.n_chains_alloc;
    const float sc = w / lum;
    const int meta = __float_as_int(list[(size_t) BL_META * n]);
    if (meta & 1)
        film_put(P, list[(size_t) BL_MAIN * n], list[(size_t) (BL_MAIN + 1) * n],
                 mk3(list[(size_t) (BL_MAIN + 2) * n] * sc, list[(size_t) (BL_MAIN + 3) * n] * sc, list[(size_t) (BL_MAIN + 4) * n] * sc));
    const int cnt = meta >> 1;
    for (int k = 0; k < cnt; ++k) {
        const int r0 = BL_MORE + 5 * k;
        film_put(P, list[(size_t) r0 * n], list[(size_t) (r0 + 1) * n],
                 mk3(list[(size_t) (r0 + 2) * n] * sc, list[(size_t) (r0 + 3) * n] * sc, list[(size_t) (r0 + 4) * n] * sc));
    }
}
// ... with the plain factor sc, no division by the list luminance: an independent sample's contribution is f itself (k_render_bdpt)
DEV void list_splat_scaled(const DParams &P, const float *list, float sc) {
    const size_t n = P.n_chains_alloc;
    const int meta = __float_as_int(list[(size_t) BL_META * n]);
    if (meta & 1)
        film_put(P, list[(size_t) BL_MAIN * n], list[(size_t) (BL_MAIN + 1) * n],
                 mk3(list[(size_t) (BL_MAIN + 2) * n] * sc, list[(size_t) (BL_MAIN + 3) * n] * sc, list[(size_t) (BL_MAIN + 4) * n] * sc));
    const int cnt = meta >> 1;
    for (int k = 0; k < cnt; ++k) {
        const int r0 = BL_MORE + 5 * k;
        film_put(P, list[(size_t) r0 * n], list[(size_t) (r0 + 1) * n],
                 mk3(list[(size_t) (r0 + 2) * n] * sc, list[(size_t) (r0 + 3) * n] * sc, list[(size_t) (r0 + 4) * n] * sc));
    }
}
DEV void list_splat_const(const DParams &P, const float *list, f3 c) { // acceptance map: every splat position (:443-450)
    const size_t n = P.n_chains_alloc;
    const int meta = __float_as_int(list[(size_t) BL_META * n]);
    if (meta & 1) film_put(P, list[(size_t) BL_MAIN * n], list[(size_t) (BL_MAIN + 1) * n], c);
    for (int k = 0; k < (meta >> 1); ++k) film_put(P, list[(size_t) (BL_MORE + 5 * k) * n], list[(size_t) (BL_MORE + 5 * k + 1) * n], c);
}
DEV void list_copy(const DParams &P, float *dst, const float *src) {
    const size_t n = P.n_chains_alloc;
    const int rows = BL_MORE + 5 * (__float_as_int(src[(size_t) BL_META * n]) >> 1);
    for (int r = 0; r < rows; ++r) dst[(size_t) r * n] = src[(size_t) r * n];
}
