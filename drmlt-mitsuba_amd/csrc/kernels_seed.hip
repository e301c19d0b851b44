// Seed selection on the device (gfx950): the rule of seed_select.h over the bootstrap luminances where launch_bootstrap* left
// them. Five small kernels on one stream; a kernel boundary is the only thing one workgroup ever waits for another by -- no
// flags, no look-back, no cooperative launch. The arithmetic is seed_select.h's, statement for statement: what a kernel adds
// is WHO runs which block or slot, never in what order a sum is formed. One lane owns one block of SEED_BLOCK samples (its
// 1 KiB row is read 16 bytes at a time; neighbouring lanes' rows share no cache line, which costs bandwidth and is what keeps
// the in-block prefix sequential), one lane owns one chain slot, and the two scans over the per-block arrays run in a single
// workgroup that loops. Every index and byte offset is 64 bits wide: n reaches 2^31 - 1 and the weighted buffer holds 2 n floats.
//
// Compiled with -ffp-contract=off and without flushing denormals (Makefile): an fp64 sum here must round as the host's does.
#include "seed_select.h"

#include <hip/hip_runtime.h>

namespace {

constexpr uint32_t SEED_THREADS = 256;
constexpr uint32_t SEED_MAX_GRID = 2048; // 256 CUs x 8 workgroups; the rest is a grid-stride loop

// (1) block totals: weights, luminance, count
__global__ __launch_bounds__(SEED_THREADS) void k_seed_block_sums(const float *__restrict__ lum, const float *__restrict__ wts, uint64_t n, uint64_t nb,
                                                                    double *__restrict__ bw, double *__restrict__ bsum, double *__restrict__ btok) {
    for (uint64_t b = (uint64_t) blockIdx.x * SEED_THREADS + threadIdx.x; b < nb; b += (uint64_t) gridDim.x * SEED_THREADS) {
        const SeedSums s = seed_block_sums(lum, wts, n, b);
        bw[b] = s.w;
        bsum[b] = s.sum;
        btok[b] = s.tok;
    }
}

// (2) one workgroup: the sequential exclusive scan of the block totals in block order. A tile of 1024 totals per array is staged in
// LDS (the latency of its loads is paid once per tile); lane 0 of waves 0, 1 and 2 each walks one array's tile and carries its running
// sum to the next tile: the host's adds, one after the other. bw becomes the offsets (nb + 1 entries, bw[nb] = total); of the
// luminances and the counts only the totals are kept: sums[] = {total, sum, tok}.
constexpr uint32_t SEED_SCAN_TILE = 4 * SEED_THREADS;
template <bool OFFSETS> __device__ __forceinline__ double seed_walk(const double *row, double *offs, uint32_t cnt, double carry) {
    for (uint32_t k = 0; k < cnt; ++k) {
        if (OFFSETS) offs[k] = carry;
        carry = carry + row[k];
    }
    return carry;
}
__global__ __launch_bounds__(SEED_THREADS) void k_seed_scan_sums(double *__restrict__ bw, const double *__restrict__ bsum, const double *__restrict__ btok,
                                                                   uint64_t nb, double *__restrict__ sums) {
    __shared__ double tile[3][SEED_SCAN_TILE];
    __shared__ double offs[SEED_SCAN_TILE];
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const bool walker = (t & 63u) == 0 && wave < 3;
    double carry = 0.0;
    for (uint64_t base = 0; base < nb; base += SEED_SCAN_TILE) {
        const uint32_t cnt = nb - base < SEED_SCAN_TILE ? (uint32_t) (nb - base) : SEED_SCAN_TILE;
        for (uint32_t k = t; k < cnt; k += SEED_THREADS) {
            tile[0][k] = bw[base + k];
            tile[1][k] = bsum[base + k];
            tile[2][k] = btok[base + k];
        }
        __syncthreads();
        if (walker) carry = wave == 0 ? seed_walk<true>(tile[0], offs, cnt, carry) : seed_walk<false>(tile[wave], offs, cnt, carry);
        __syncthreads();
        for (uint32_t k = t; k < cnt; k += SEED_THREADS) bw[base + k] = offs[k];
        // (the next tile's loads refill tile[] only; offs[] is rewritten behind the next barrier, after every lane has read its entries here)
    }
    if (walker) {
        sums[wave] = carry;
        if (wave == 0) bw[nb] = carry;
    }
}

// (3) one pick per chain slot, counted per sample and per block (integer atomics: the counts do not depend on arrival order)
__global__ __launch_bounds__(SEED_THREADS) void k_seed_pick(const float *__restrict__ lum, const float *__restrict__ wts, uint64_t n, const double *__restrict__ off,
                                                              uint32_t k0, uint32_t k1, uint32_t stream, uint32_t n_select, uint32_t *__restrict__ count,
                                                              uint32_t *__restrict__ bcount) {
    const uint64_t nb = seed_blocks(n);
    if (!(off[nb] > 0.0)) return; // no admissible sample: the host reports it from sums[]
    for (uint64_t j = (uint64_t) blockIdx.x * SEED_THREADS + threadIdx.x; j < n_select; j += (uint64_t) gridDim.x * SEED_THREADS) {
        const uint32_t i = seed_pick(lum, wts, n, off, k0, k1, stream, (uint32_t) j);
        atomicAdd(&count[i], 1u);
        atomicAdd(&bcount[i / SEED_BLOCK], 1u);
    }
}

// (4) one workgroup: exclusive scan of the per-block pick counts, in place (nb + 1 entries, the last becomes n_select). Sixteen
// consecutive counts per lane and tile, the lanes' partial sums scanned through LDS.
constexpr uint32_t SEED_PER_LANE = 16;
__global__ __launch_bounds__(SEED_THREADS) void k_seed_scan_counts(uint32_t *__restrict__ bcount, uint64_t nb) {
    __shared__ uint32_t part[SEED_THREADS];
    const uint32_t t = threadIdx.x;
    uint32_t carry = 0;
    for (uint64_t base = 0; base < nb; base += (uint64_t) SEED_THREADS * SEED_PER_LANE) {
        const uint64_t i0 = base + (uint64_t) t * SEED_PER_LANE;
        uint32_t local[SEED_PER_LANE], s = 0;
#pragma unroll
        for (uint32_t k = 0; k < SEED_PER_LANE; ++k) {
            local[k] = s;
            s += i0 + k < nb ? bcount[i0 + k] : 0u;
        }
        part[t] = s;
        __syncthreads();
        for (uint32_t d = 1; d < SEED_THREADS; d <<= 1) {
            const uint32_t v = t >= d ? part[t - d] : 0u;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        const uint32_t before = carry + (t ? part[t - 1] : 0u);
        carry += part[SEED_THREADS - 1];
#pragma unroll
        for (uint32_t k = 0; k < SEED_PER_LANE; ++k)
            if (i0 + k < nb) bcount[i0 + k] = before + local[k];
        __syncthreads();
    }
    if (t == 0) bcount[nb] = carry;
}

// (5) the sorted list: block b's samples go to positions [bstart[b], bstart[b + 1]) of the job's list; this context keeps its slice
__global__ __launch_bounds__(SEED_THREADS) void k_seed_expand(const uint32_t *__restrict__ count, const uint32_t *__restrict__ bstart, const float *__restrict__ lum,
                                                                uint64_t n, uint64_t nb, uint32_t slice_lo, uint32_t slice_n, uint32_t *__restrict__ out_index,
                                                                float *__restrict__ out_lum) {
    const uint64_t end = (uint64_t) slice_lo + slice_n;
    for (uint64_t b = (uint64_t) blockIdx.x * SEED_THREADS + threadIdx.x; b < nb; b += (uint64_t) gridDim.x * SEED_THREADS) {
        const uint32_t s = bstart[b], e = bstart[b + 1];
        if (s == e || e <= slice_lo || s >= end) continue;
        seed_expand_block(count, lum, n, b, s, slice_lo, slice_n, out_index, out_lum);
    }
}

uint32_t seed_grid(uint64_t items) {
    const uint64_t g = (items + SEED_THREADS - 1) / SEED_THREADS;
    return (uint32_t) (g < 1 ? 1 : g > SEED_MAX_GRID ? SEED_MAX_GRID : g);
}

size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

} // namespace

// Workspace: count[n] and bcount[nb + 1] (uint32, zeroed per call), off[nb + 1], bsum[nb], btok[nb] and sums[3] (fp64).
size_t seed_workspace_bytes(uint32_t n) {
    const size_t nb = (size_t) seed_blocks(n);
    return pad256((size_t) n * sizeof(uint32_t)) + pad256((nb + 1) * sizeof(uint32_t)) + pad256((nb + 1) * sizeof(double)) + 2 * pad256(nb * sizeof(double)) + 256;
}

// lum: n luminances (wts: n weights or NULL), both on the device. Draws n_select picks, writes slots [slice_lo, slice_lo + slice_n) of
// their sorted list to out_index / out_lum (device, slice_n entries) and {total weight, sum, tok} to the three doubles that
// seed_sums_ptr(work, n) points at. Everything is enqueued on `st`; n > 0.
hipError_t launch_seed_select(const float *lum, const float *wts, uint32_t n, uint32_t k0, uint32_t k1, uint32_t stream, uint32_t n_select, uint32_t slice_lo,
                              uint32_t slice_n, void *work, uint32_t *out_index, float *out_lum, const double **sums_out, hipStream_t st) {
    const size_t nb = (size_t) seed_blocks(n);
    char *p = static_cast<char *>(work);
    uint32_t *count = reinterpret_cast<uint32_t *>(p); p += pad256((size_t) n * sizeof(uint32_t));
    uint32_t *bcount = reinterpret_cast<uint32_t *>(p); p += pad256((nb + 1) * sizeof(uint32_t));
    const size_t zeroed = (size_t) (p - static_cast<char *>(work));
    double *off = reinterpret_cast<double *>(p); p += pad256((nb + 1) * sizeof(double));
    double *bsum = reinterpret_cast<double *>(p); p += pad256(nb * sizeof(double));
    double *btok = reinterpret_cast<double *>(p); p += pad256(nb * sizeof(double));
    double *sums = reinterpret_cast<double *>(p);
    *sums_out = sums;
    hipError_t e = hipMemsetAsync(work, 0, zeroed, st);
    if (e != hipSuccess) return e;
    k_seed_block_sums<<<seed_grid(nb), SEED_THREADS, 0, st>>>(lum, wts, n, nb, off, bsum, btok);
    k_seed_scan_sums<<<1, SEED_THREADS, 0, st>>>(off, bsum, btok, nb, sums);
    k_seed_pick<<<seed_grid(n_select), SEED_THREADS, 0, st>>>(lum, wts, n, off, k0, k1, stream, n_select, count, bcount);
    k_seed_scan_counts<<<1, SEED_THREADS, 0, st>>>(bcount, nb);
    k_seed_expand<<<seed_grid(nb), SEED_THREADS, 0, st>>>(count, bcount, lum, n, nb, slice_lo, slice_n, out_index, out_lum);
    return hipGetLastError();
}
