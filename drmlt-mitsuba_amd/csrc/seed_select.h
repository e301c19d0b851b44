// The seed-selection rule of PathSampler::generateSeeds (pathsampler.cpp:879-957), stated ONCE for the device kernels
// (kernels_seed.hip) and for a serial host restatement (seed_select_host below, drmlt_select_seeds_blocked): both include this
// header and run the same statements, so their results agree bit for bit. Plain C++: no HIP header is needed to compile it.
//
// Inclusion (drmlt_capi.cpp: seed_impl). A NaN luminance counts for nothing. Every other sample adds 1 to `tok` and its
// luminance to `sum`; it has the weight lw if l != 0 && lw > 0 && isfinite(lw), else 0, where lw is the luminance itself or,
// under the importance map with seed_rule = TARGET, the luminance under the map (second half of the bootstrap buffer).
//
// Order. All sums are fp64 and BLOCKED: samples are cut into blocks of SEED_BLOCK = 256 consecutive indices. Inside a block the
// inclusive prefix is sequential in index order, starting from zero; the block's total is its last prefix; the block offsets
// are the sequential exclusive scan of the totals in block order; incl[i] = offset[block] + inblock[i]; total = offset[nb].
// `sum` and `tok` follow the same order. The order depends on n and SEED_BLOCK alone -- never on a grid, a wave or an arrival
// order -- and every partial sum is one rounded add of non-negative terms, so incl[] never decreases: the searches below rely
// on that. (The unit that holds the kernels is compiled with -ffp-contract=off; there is no multiply next to these adds anyway.)
//
// Pick. Chain slot j draws xi = (float) (r[0] >> 8) * 2^-24 from philox(key0, key1, 0, j, stream, TAG_SEEDSEL) and takes the
// smallest i with incl[i] >= xi * total and incl[i] > incl[i - 1] (incl[-1] = 0); if there is none, the last i of positive
// width. That is DiscreteDistribution::sample (include/mitsuba/core/pmf.h:164-188) with the zero-width skip of
// pathsampler.cpp:936-957 whenever xi * total is not within rounding of a boundary of the table.
//
// Ordering (PathSeedSortPredicate). The picks are counted per sample with integer adds, the counts are scanned (integers: any
// order gives the same sums) and sample i writes itself to positions [start_i, start_i + count_i) of the sorted list.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define SEED_HD __host__ __device__ inline
#else
#define SEED_HD inline
#endif

constexpr uint32_t SEED_BLOCK = 256;
constexpr uint32_t SEED_TAG_SEEDSEL = 1; // device_math.h: TAG_SEEDSEL

struct SeedSums {
    double w, sum, tok; // admissible weight, luminance, count of non-NaN samples
};
struct alignas(16) SeedQuad {
    float v[4];
};

SEED_HD uint32_t seed_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
SEED_HD bool seed_isnan(float x) { return (seed_bits(x) & 0x7fffffffu) > 0x7f800000u; }
SEED_HD bool seed_isfinite(float x) { return (seed_bits(x) & 0x7f800000u) != 0x7f800000u; }
SEED_HD uint64_t seed_blocks(uint64_t n) { return (n + SEED_BLOCK - 1) / SEED_BLOCK; }

// what sample (l, lw) is drawn in proportion to
SEED_HD double seed_weight(float l, float lw) { return (!seed_isnan(l) && l != 0.f && lw > 0.f && seed_isfinite(lw)) ? (double) lw : 0.0; }

SEED_HD void seed_add(SeedSums &a, float l, float lw) {
    if (seed_isnan(l)) return;
    a.tok = a.tok + 1.0;
    a.sum = a.sum + (double) l;
    a.w = a.w + seed_weight(l, lw);
}

// Totals of block b, sequential in index order. (A full block whose rows are 16-byte aligned is read four samples at a time; the
// adds are the same adds in the same order.)
SEED_HD SeedSums seed_block_sums(const float *lum, const float *wts, uint64_t n, uint64_t b) {
    SeedSums a = {0.0, 0.0, 0.0};
    const uint64_t lo = b * SEED_BLOCK, hi = lo + SEED_BLOCK < n ? lo + SEED_BLOCK : n;
    uint64_t i = lo;
    if (hi - lo == SEED_BLOCK && ((uintptr_t) (lum + lo) & 15u) == 0 && (!wts || ((uintptr_t) (wts + lo) & 15u) == 0)) {
        for (; i < hi; i += 4) {
            const SeedQuad l = *reinterpret_cast<const SeedQuad *>(lum + i);
            const SeedQuad w = wts ? *reinterpret_cast<const SeedQuad *>(wts + i) : l;
            seed_add(a, l.v[0], w.v[0]);
            seed_add(a, l.v[1], w.v[1]);
            seed_add(a, l.v[2], w.v[2]);
            seed_add(a, l.v[3], w.v[3]);
        }
    }
    for (; i < hi; ++i) seed_add(a, lum[i], wts ? wts[i] : lum[i]);
    return a;
}

// Philox4x32-10, word 0 of the block (the same function as device_math.h's and drmlt_capi.cpp's)
SEED_HD uint32_t seed_philox0(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t) 0xD2511F53u * c0, p1 = (uint64_t) 0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t) (p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t) p1, n2 = (uint32_t) (p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t) p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

SEED_HD double seed_target(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t j, double total) {
    const float xi = (float) (seed_philox0(k0, k1, 0u, j, stream, SEED_TAG_SEEDSEL) >> 8) * (1.0f / 16777216.0f);
    const double t = (double) xi * total;
    return t > total ? total : t; // (xi < 1: never taken; the last entry of positive width is then the answer)
}

// incl has reached the target AND lies beyond the leading zero-width entries (target = 0 picks the first entry of positive width)
SEED_HD bool seed_reached(double incl, double target) { return incl >= target && incl > 0.0; }

// Smallest block whose last inclusive prefix, off[b + 1], has reached the target; off: nb + 1 entries, off[nb] = total > 0.
SEED_HD uint64_t seed_pick_block(const double *off, uint64_t nb, double target) {
    uint64_t lo = 0, hi = nb - 1; // seed_reached(off[nb], target) holds: target <= total, total > 0
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (seed_reached(off[mid + 1], target)) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// The pick inside block b: the block's prefix is formed again, by the adds of seed_block_sums in their order.
SEED_HD uint32_t seed_pick_in_block(const float *lum, const float *wts, uint64_t n, uint64_t b, double off_b, double target) {
    const uint64_t lo = b * SEED_BLOCK, hi = lo + SEED_BLOCK < n ? lo + SEED_BLOCK : n;
    double acc = 0.0, prev = off_b;
    uint64_t last = lo;
    for (uint64_t i = lo; i < hi; ++i) {
        acc = acc + seed_weight(lum[i], wts ? wts[i] : lum[i]);
        const double incl = off_b + acc;
        if (incl > prev) {
            if (incl >= target) return (uint32_t) i;
            last = i;
            prev = incl;
        }
    }
    return (uint32_t) last;
}

SEED_HD uint32_t seed_pick(const float *lum, const float *wts, uint64_t n, const double *off, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t j) {
    const uint64_t nb = seed_blocks(n);
    const double target = seed_target(k0, k1, stream, j, off[nb]);
    const uint64_t b = seed_pick_block(off, nb, target);
    return seed_pick_in_block(lum, wts, n, b, off[b], target);
}

// Block b of the sorted list: its samples, each count[i] times, go to positions [start, ...) of the job's list; what falls into
// this context's slice [slice_lo, slice_lo + slice_n) is written, with the sample's luminance beside it.
SEED_HD void seed_expand_block(const uint32_t *count, const float *lum, uint64_t n, uint64_t b, uint32_t start, uint32_t slice_lo, uint32_t slice_n,
                               uint32_t *out_index, float *out_lum) {
    const uint64_t lo = b * SEED_BLOCK, hi = lo + SEED_BLOCK < n ? lo + SEED_BLOCK : n;
    uint64_t pos = start;
    const uint64_t end = (uint64_t) slice_lo + slice_n;
    for (uint64_t i = lo; i < hi && pos < end; ++i) {
        const uint32_t c = count[i];
        for (uint32_t k = 0; k < c; ++k, ++pos)
            if (pos >= slice_lo && pos < end) {
                out_index[pos - slice_lo] = (uint32_t) i;
                if (out_lum) out_lum[pos - slice_lo] = lum[i];
            }
    }
}

enum { SEED_SELECT_OK = 0, SEED_SELECT_ZERO_MEAN = 1, SEED_SELECT_NO_WEIGHT = 2 };
SEED_HD int seed_status(double sum, double tok, double total, double scale, double *mean_out) {
    double mean = tok > 0 ? sum / tok : 0.0;
    mean = mean * scale; // technique=mmlt: maxDepth, "As we split the path by corresponding depth"
    *mean_out = mean;
    if (!(mean > 0.0)) return SEED_SELECT_ZERO_MEAN;
    if (!(total > 0.0)) return SEED_SELECT_NO_WEIGHT;
    return SEED_SELECT_OK;
}

// The whole selection, serially: the statements the kernels run, block after block, slot after slot. `out_sorted`: n_select sample
// indices in ascending order. sums_out: {total weight, sum, tok} as scanned.
inline int seed_select_host(const float *lum, const float *wts, uint32_t n, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t n_select, double scale,
                            uint32_t *out_sorted, double *mean_out, double *total_out) {
    const uint64_t nb = seed_blocks(n);
    std::vector<double> off(nb + 1);
    double o = 0.0, sum = 0.0, tok = 0.0;
    for (uint64_t b = 0; b < nb; ++b) {
        const SeedSums s = seed_block_sums(lum, wts, n, b);
        off[b] = o;
        o = o + s.w;
        sum = sum + s.sum;
        tok = tok + s.tok;
    }
    off[nb] = o;
    if (total_out) *total_out = o;
    double mean = 0.0;
    const int st = seed_status(sum, tok, o, scale, &mean);
    if (mean_out) *mean_out = mean;
    if (st != SEED_SELECT_OK) return st;
    std::vector<uint32_t> count(n, 0u), bstart(nb + 1, 0u);
    for (uint32_t j = 0; j < n_select; ++j) {
        const uint32_t i = seed_pick(lum, wts, n, off.data(), k0, k1, stream, j);
        ++count[i];
        ++bstart[i / SEED_BLOCK];
    }
    uint32_t run = 0;
    for (uint64_t b = 0; b <= nb; ++b) { const uint32_t c = bstart[b]; bstart[b] = run; run += c; }
    for (uint64_t b = 0; b < nb; ++b)
        if (bstart[b + 1] != bstart[b]) seed_expand_block(count.data(), lum, n, b, bstart[b], 0u, n_select, out_sorted, nullptr);
    return SEED_SELECT_OK;
}
