// Primary-sample-space transitions and samplers of technique=path: the transition kernels, each written ONCE as a leaf
// routine, and the samplers of the chain-kernel generations (k_mutate_v3: LdsSampler, k_mutate_v4: RowSamplerT, k_mutate_v5:
// PoolRowSampler and the v5_fill routines, k_mutate_pssmlt: PssmltSampler; bootstrap, replay, evaluation and path tracing: Sampler),
// which only load operands, call the leaves and store results. The generations run the same chains bit for bit
// (tests/test_gpu_parity.py, test_gpu_raypool.py, test_gpu_v4_row_roles.py, test_gpu_v4_rule_builds.py) BECAUSE there is one copy
// of the arithmetic (tests/test_transition_one_copy.py). MSampler (device_bidir.h: mmlt, bdpt) keeps its own, see there.
//
// Reference behaviour restated here (paths relative to the reference checkout):
//   transition kernels       src/integrators/drmlt/tools/transition.h:54-190
//   fillSpace / wrap         src/integrators/drmlt/drmlt_sampler.cpp:313-394, drmlt_sampler.h:140-144
//   PSSMLTSampler            src/integrators/pssmlt/pssmlt_sampler.cpp:93-168, pssmlt_sampler.h:113-143
#pragma once
#include "device_math.h"
#include "device_types.h"

// Current PSS states of the 64 chains of this wave, [dim][lane]: lane-contiguous rows, so any
// per-lane dimension pattern is bank-conflict free (64 == 0 mod 32 banks). Addressed directly
// (ds_read), never through a generic pointer: LDS offset 0 casts to the flat null pointer.
extern __shared__ __attribute__((aligned(16))) float lds_x[];

// The leaf routines below are inlined into every sampler (per component in k_mutate_v3, for whole rows in k_mutate_v4 and
// k_mutate_v5, pair-wise at a commit): without this the compiler contracts a*b+c into an fma at some of the inlined sites and
// not at others, and the kernels' chains drift apart in the last bit. Explicit fmaf() calls stay fused everywhere.
#define FP_STRICT _Pragma("clang fp contract(off)")

DEV float load_global_f32(const float *p) { return *(const float __attribute__((address_space(1))) *) (uintptr_t) p; }

// ------------------------------------------------------------------ transition kernels
enum { SM_BOOT = 0, SM_ARRAY = 1, SM_STAGE1 = 2, SM_STAGE2 = 3, SM_REVERSE = 4, SM_PT = 5 };

// drmlt_sampler.h:140-144: y > 1 ? 2 - y : (y <= 0 ? |y| : y). For 0 < y <= 1, |y| = y, so two selects collapse into
// one select on an |.|-modified operand (the nested form compiled to two exec-mask branches per component).
DEV float wrap01(float y) { return y > 1.f ? 2.f - y : fabsf(y); }
// A value that wrap01 maps back onto v, bit for bit, for every v that wrap01 returns: v itself inside [0, 1] (and for a NaN),
// where wrap01 is the identity; outside -- perturbations of more than one, which no sane setting produces -- v > 1 came from -v,
// and v < 0 from 2 - v (an exact difference: y >= 2 is a multiple of 2^-22, and so is 2 - y). Checked over all 2^32 arguments
// of wrap01: one exception, y = 2^25 + 4, where 2 - y is a rounding tie. k_mutate_v4 keeps its current state unwrapped and
// wraps it where it is read; it loads a stored (wrapped) state through this.
DEV float unwrap01(float v) { return v < 0.f ? 2.f - v : (v > 1.f ? -v : v); }

#define KELEMEN_S1 (1.0f / 1024.0f)
#define KELEMEN_S2 (1.0f / 64.0f)
#define ORBITAL_SCALE 1.9f
#define LOG2_S1_OVER_S2 (-4.0f) // log2((1/1024)/(1/64))
// wrapped Cauchy: rho = exp(-1/4), dispersion c = 2 rho / (1 + rho^2)
#define WC_DISPERSION 0.96954361f

// Kelemen kernel (transition.h:97-111): sign * s2 * (s1/s2)^(1 - xi')
DEV float kelemen_sample(float xi, float s2) {
        FP_STRICT;
    float sign = 1.f;
    if (xi < 0.5f) { xi *= 2.f; } else { sign = -1.f; xi = 2.f * (xi - 0.5f); }
    return sign * s2 * fast_exp2((1.f - xi) * LOG2_S1_OVER_S2);
}
// Gaussian kernel (transition.h:61-66), Box-Muller cosine branch
DEV float gaussian_sample(float u1, float u2, float sigma) {
        FP_STRICT;
    float tmp = sqrtf(-1.3862943611198906f * fast_log2(1.f - u1)); // -2 ln(v) = -2 ln2 log2(v)
    return tmp * cos_rev(u2) * sigma;
}
// log pdf of the (unscaled) Kelemen kernel, transition.h:113-122
// (a select, not an early return: in an unrolled ratio loop every return was an exec mask kept in scalar registers)
DEV float kelemen_logpdf(float du) {
    float d = fabsf(du);
    const float l = -__logf(2.f * d * 2.772588722239781f); // ln(s2/s1) = ln 16
    return (d < KELEMEN_S1 || d > KELEMEN_S2) ? -INFINITY : l;
}

// One Philox block of an addressed stream as four uniforms in [0, 1)
struct Unit4 { float v[4]; };
DEV Unit4 philox_unit4(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    FP_STRICT;
    const u4 r = philox4x32_10(k0, k1, c0, c1, c2, c3);
    return Unit4{{u32_to_unit(r.x), u32_to_unit(r.y), u32_to_unit(r.z), u32_to_unit(r.w)}};
}

// Orbital first stage (drmlt_sampler.cpp:354-361), one component of the pair (x0, x1): y = x + d (cos, sin)(2 pi ua), the radius d
// from the Kelemen kernel (x 1.9) on ud, the angle uniform. sin(2 pi a) is cos(2 pi (a - 1/4)): one v_cos serves either component
// (v_sin and v_cos differ in the last bit, so EVERY sampler takes the sine this way).
DEV float orbital_first(float ud, float ua, bool odd, float x) {
    FP_STRICT;
    const float d = kelemen_sample(ud, KELEMEN_S2 * ORBITAL_SCALE);
    return fmaf(d, cos_rev(ua - (odd ? 0.25f : 0.f)), x);
}
// ... both components (a - 0.f is a for every float: the same definition, not a second formula)
DEV void orbital_first_pair(float ud, float ua, float x0, float x1, float &y0, float &y1) {
    FP_STRICT;
    y0 = orbital_first(ud, ua, false, x0);
    y1 = orbital_first(ud, ua, true, x1);
}
// theta ~ wrapped Cauchy by inverse CDF (transition.h:157-173): cos(theta) = A
DEV void wrapped_cauchy_rotation(float xi, float &ct, float &st) {
    FP_STRICT;
    float sign = 1.f;
    if (xi < 0.5f) { xi *= 2.f; } else { sign = -1.f; xi = 2.f * (xi - 0.5f); }
    const float V = cos_rev(xi);
    const float c = WC_DISPERSION;
    const float A = fminf(1.f, fmaxf(-1.f, (V + c) / (1.f + c * V)));
    ct = A; st = sign * sqrtf(fmaxf(0.f, 1.f - A * A));
}
// Orbital second stage of a pair: z = y + R(theta) (x - y). (x - y) rotated by theta about y is identical to
// y + |x-y| (cos, sin)(theta + mu), mu the polar angle of x - y (drmlt_sampler.cpp:374-391), without the acos round trip.
DEV void orbital_second_pair(float xi, float x0, float x1, float y0, float y1, float &z0, float &z1) {
    FP_STRICT;
    float ct, st;
    wrapped_cauchy_rotation(xi, ct, st);
    const float dx0 = x0 - y0, dx1 = x1 - y1;
    z0 = y0 + (ct * dx0 - st * dx1);
    z1 = y1 + (st * dx0 + ct * dx1);
}
// iid kernels (Green, Mira): first stage Kelemen, second stage Gaussian (g: the perturbation, where a sampler parks it)
DEV float iid_first(float u, float x) { FP_STRICT; return x + kelemen_sample(u, KELEMEN_S2); }
DEV float iid_second(float x, float g) { FP_STRICT; return x + g; }
DEV float iid_second(float u0, float u1, float sigma2, float x) { FP_STRICT; return iid_second(x, gaussian_sample(u0, u1, sigma2)); }
// Green's reverse move: y* = z - (y - x) (drmlt_proc.cpp:588-598)
DEV float green_reverse(float x, float y, float z) { FP_STRICT; return z - (y - x); }
// First-stage proposal of dimensions 4b .. 4b+3 from the four uniforms of Philox block b (fillSpace with isFirst = true);
// a large step: the uniforms themselves
DEV void first_stage_block(int type, bool large, const Unit4 &u, const float (&x)[4], float (&y)[4]) {
    FP_STRICT;
    if (type == 2) { // pairwise orbital
        orbital_first_pair(u.v[0], u.v[1], x[0], x[1], y[0], y[1]);
        orbital_first_pair(u.v[2], u.v[3], x[2], x[3], y[2], y[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = iid_first(u.v[i], x[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = large ? u.v[i] : y[i];
}

// ------------------------------------------------------------------ sampler of one evaluation
// Bootstrap samples and their replay (SM_BOOT), caller-supplied points (SM_ARRAY), independent path-tracing samples (SM_PT):
// component k of (major, chain) is draw k of the addressed stream, or arr[k]. No chain mutates through it.
struct Sampler {
    uint32_t key0, key1, chain, major; // major: sample index
    int mode;
    const float *arr; // SM_ARRAY: explicit PSS vector
    u4 b1;            // one-block cache
    uint32_t b1_idx;

    DEV void reset_caches() { b1_idx = 0xffffffffu; }
    DEV float u_boot(uint32_t k, uint32_t tag) {
        uint32_t blk = k >> 2;
        if (blk != b1_idx) { b1 = philox4x32_10(key0, key1, blk, major, chain, tag); b1_idx = blk; }
        return pick4(b1, k & 3u);
    }
    // value handed to the path code for PSS dimension k (primarySample)
    DEV float next(uint32_t k) {
        switch (mode) {
            case SM_BOOT: return u_boot(k, TAG_BOOT);
            case SM_PT: return u_boot(k, TAG_PT);
            default: return arr[k]; // SM_ARRAY
        }
    }
};

// ------------------------------------------------------------------ PSS sampler of k_mutate_v3
// The Philox draws of a mutation are produced up front, by all lanes that start an evaluation together (convergent code in
// the bookkeeping branch), and parked in LDS next to the chain state:
//   lds_x  [0 .. D)          current state x
//   lds_u1 = lds_x + D*32    first-stage uniforms, draw k of the TAG_S1 stream (row k, D rounded to 4)
//   lds_s2 = lds_u1 + D4*32  second-stage values: orbital: theta uniform of pair q in row q;
//                            iid: the Gaussian perturbation of dim k in row k; large: uniform k
// The per-dimension code below is then pure arithmetic on LDS operands -- no RNG, no caches, no
// divergent Philox in the ray loop (measured: an on-demand sampler was ~2/3 of the VALU work).
struct LdsSampler {
    uint32_t key0, key1, chain, major;
    int mode, type;
    bool large;
    float sigma2;
    uint32_t lane;
    uint32_t u1_off, s2_off; // row offsets (in floats) of lds_u1 / lds_s2
    uint32_t stride;         // floats per row (32: k_mutate_v3's waves hold 32 chains and their 32 helper lanes)

    DEV void reset_caches() {}
    DEV float x(uint32_t k) const { return lds_x[k * stride + lane]; }
    DEV float u1(uint32_t k) const { return lds_x[u1_off + k * stride + lane]; }
    DEV float s2(uint32_t k) const { return lds_x[s2_off + k * stride + lane]; }
    DEV void put4(uint32_t off, const Unit4 &u) const {
        float *dst = &lds_x[off + lane];
        dst[0] = u.v[0]; dst[stride] = u.v[1]; dst[2u * stride] = u.v[2]; dst[3u * stride] = u.v[3];
    }

    // first-stage draws of this mutation, Philox blocks [b0, b1): rows 4b .. 4b+3 of lds_u1
    DEV void fill_stage1(uint32_t b0, uint32_t b1) {
        for (uint32_t b = b0; b < b1; ++b) put4(u1_off + b * 4u * stride, philox_unit4(key0, key1, b, major, chain, TAG_S1));
    }
    // second-stage values (see layout above); blocks first, first + step, ... (step 2 = shared by two lanes)
    DEV void fill_stage2(uint32_t D4, uint32_t first, uint32_t step) {
        if (large || type == 2) {
            const uint32_t rows = large ? D4 : (D4 / 2u + 3u) & ~3u; // uniforms: one per dim, or one per pair
            for (uint32_t b = first; b < rows / 4u; b += step) put4(s2_off + b * 4u * stride, philox_unit4(key0, key1, b, major, chain, TAG_S2));
        } else {
            for (uint32_t b = first; b < D4 / 2u; b += step) { // draws (2k, 2k+1) -> Gaussian sample of dim k
                const Unit4 u = philox_unit4(key0, key1, b, major, chain, TAG_S2);
                float *dst = &lds_x[s2_off + b * 2u * stride + lane];
                dst[0] = gaussian_sample(u.v[0], u.v[1], sigma2);
                dst[stride] = gaussian_sample(u.v[2], u.v[3], sigma2);
            }
        }
    }

    // first- and second-stage proposal, unwrapped (Mira's ratio reads them)
    DEV float y_raw(uint32_t k) const {
        if (large) return u1(k);
        if (type != 2) return iid_first(u1(k), x(k));
        const uint32_t k0 = k & ~1u;
        return orbital_first(u1(k0), u1(k0 + 1u), (k & 1u) != 0u, x(k));
    }
    DEV float z_raw(uint32_t k) const {
        if (large) return s2(k);
        if (type != 2) return iid_second(x(k), s2(k));
        float z0, z1;
        orbital_pair(k & ~1u, true, z0, z1);
        return (k & 1u) ? z1 : z0;
    }
    DEV float next(uint32_t k) const {
        if (type == 2 && mode == SM_STAGE1) {
            // The common case (orbital, first stage) without divergent branches: unconditional LDS reads, the
            // large-step case as a select, one v_cos for either component.
            const uint32_t k0 = k & ~1u;
            const bool odd = (k & 1u) != 0u;
            const float ua = u1(k0), ub = u1(k0 + 1u);
            const float y = orbital_first(ua, ub, odd, x(k));
            return wrap01(large ? (odd ? ub : ua) : y);
        }
        if (type == 2) {
            // orbital second stage (the reverse mode belongs to Green and never gets here): the pair once, the
            // large-step case (timidAfterLarge) as a select on an unconditional read
            float z0, z1;
            orbital_pair(k & ~1u, true, z0, z1);
            const float zl = s2(k);
            return wrap01(large ? zl : ((k & 1u) ? z1 : z0));
        }
        // iid kernels (Green, Mira): all three modes from unconditional reads and selects
        const float xk = x(k), a = u1(k), g = s2(k);
        const float y = large ? a : iid_first(a, xk);
        const float z = large ? g : iid_second(xk, g);
        const float v = mode == SM_STAGE1 ? y : (mode == SM_STAGE2 ? z : green_reverse(xk, y, z));
        return wrap01(v);
    }
    // Orbital pair (k0, k0 + 1), both components of the first- or second-stage proposal at once (a commit: the
    // per-component form evaluates the shared radius / angle / rotation twice per pair).
    DEV void orbital_pair(uint32_t k0, bool second, float &o0, float &o1) const {
        const float x0 = x(k0), x1 = x(k0 + 1u);
        float y0, y1;
        orbital_first_pair(u1(k0), u1(k0 + 1u), x0, x1, y0, y1);
        if (!second) { o0 = y0; o1 = y1; return; }
        orbital_second_pair(s2(k0 >> 1), x0, x1, y0, y1, o0, o1);
    }
};

// ------------------------------------------------------------------ PSS sampler of k_mutate_v4
// The proposals themselves are parked in LDS, not the uniforms they are made of: the bookkeeping branch of k_mutate_v4
// evaluates the transition kernels for ALL dimensions of the chains that start an evaluation, flattened over the 64
// lanes of the wave (items = chain x Philox block, every lane busy), so that inside the divergent path step a PSS
// component is one LDS read and a reflection. Three row groups of D4 rows each (stride `stride` floats, column = chain),
// all three UNWRAPPED; which group plays which role is the chain's own business:
//   x   current state (wrapped where it is read)
//   y   first-stage proposal (a large step: the uniforms themselves)
//   z   second-stage proposal
// A chain adopts a proposal by exchanging the roles of two of its groups (DRMLTSampler::accept without the copy): x_off and y_off
// are PER LANE, the float offset of row 0 of the group with the chain's column folded in, each below 2^14 (64 KB of LDS); the z
// group is the third one (the three offsets add up to `xyz`). Between loop sections a chain keeps the pair in one word (roles()).
// RULE (device_types.h): under RULE_ORBITAL `type` is 2 at compile time -- the fill routines keep their orbital arm, and `mode` is
// SM_STAGE1 or SM_STAGE2 (the reverse move is Green's), so a component is ONE read, of y or of z.
template <int RULE = RULE_GENERIC> struct RowSamplerT {
    static constexpr bool orbital = RULE == RULE_ORBITAL;
    static constexpr bool batch_draws = true; // path_step: the (up to) five components of a step are read together, ahead of the hit's digestion
    uint32_t key0, key1;
    int mode, type;
    float sigma2;
    uint32_t stride, x_off, y_off, xyz;

    DEV void reset_caches() {}
    DEV float x(uint32_t k) const { return wrap01(lds_x[x_off + k * stride]); }
    DEV float y_raw(uint32_t k) const { return lds_x[y_off + k * stride]; }
    DEV uint32_t z_off() const { return xyz - x_off - y_off; }
    DEV float z_raw(uint32_t k) const { return lds_x[z_off() + k * stride]; }
    DEV float next(uint32_t k) const {
        if constexpr (orbital) return wrap01(lds_x[(mode == SM_STAGE1 ? y_off : z_off()) + k * stride]);
        float v = y_raw(k);
        if (mode != SM_STAGE1) {
            const float z = z_raw(k);
            v = mode == SM_STAGE2 ? z : green_reverse(x(k), v, z);
        }
        return wrap01(v);
    }
    // adopt the first- (SM_STAGE1) or second-stage (SM_STAGE2) proposal: its group becomes x, the old x group is free for the
    // next proposal of that stage (0: nothing adopted)
    DEV void adopt(int commit_mode) {
        const uint32_t xo = x_off, zo = z_off();
        x_off = commit_mode == SM_STAGE1 ? y_off : (commit_mode == SM_STAGE2 ? zo : xo);
        y_off = commit_mode == SM_STAGE1 ? xo : y_off;
    }
    // The two offsets in one word: what a chain lane keeps across loop sections, and what travels to the lanes that fill ANOTHER
    // chain's rows in the flattened passes (bit 0 is free for the large-step bit there). `col`: the chain's column.
    DEV uint32_t roles() const { return (x_off << 1) | (y_off << 16); }
    DEV void set_roles(uint32_t w, uint32_t group, uint32_t col) { x_off = (w >> 1) & 0x7fffu; y_off = w >> 16; xyz = 3u * (group + col); }
    DEV static uint32_t first_roles(uint32_t group, uint32_t col) { return (col << 1) | ((group + col) << 16); }
    // first-stage proposal of the chain whose offsets this sampler carries, dimensions 4b .. 4b+3, from Philox block b of (major, chain)
    DEV void fill_first(uint32_t b, uint32_t major, uint32_t chain, bool large) const {
        const Unit4 u = philox_unit4(key0, key1, b, major, chain, TAG_S1);
        const float *xs = &lds_x[x_off + 4u * b * stride];
        float *ys = &lds_x[y_off + 4u * b * stride];
        const float x4[4] = {wrap01(xs[0]), wrap01(xs[stride]), wrap01(xs[2u * stride]), wrap01(xs[3u * stride])};
        float y[4];
        first_stage_block(orbital ? 2 : type, large, u, x4, y);
        ys[0] = y[0]; ys[stride] = y[1]; ys[2u * stride] = y[2]; ys[3u * stride] = y[3];
    }
    // second-stage proposal of that chain from Philox block b of the TAG_S2 stream: a large step (timidAfterLarge)
    // -> dims 4b..4b+3 (uniforms); orbital -> the angles of pairs 4b..4b+3 = dims 8b..8b+7; iid kernels -> the Gaussian
    // perturbations of dims 2b, 2b+1 (draws 2k, 2k+1 belong to dim k). Blocks beyond the chain's kind of stage do nothing.
    DEV void fill_second(uint32_t b, uint32_t D4, uint32_t major, uint32_t chain, bool large) const {
        const uint32_t nblk = large ? D4 / 4u : ((orbital || type == 2) ? (D4 / 2u + 3u) / 4u : D4 / 2u);
        if (b >= nblk) return;
        const Unit4 u = philox_unit4(key0, key1, b, major, chain, TAG_S2);
        const uint32_t zo = z_off();
        if (large) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) lds_x[zo + (4u * b + i) * stride] = u.v[i];
        } else if (orbital || type == 2) {
            // (all reads first: the writes below are to LDS too and may alias them for the compiler -- pair after pair would wait for its
            // own reads behind the previous pair's writes)
            float xa[4], xb[4], ya[4], yb[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t k0 = 2u * (4u * b + i), kk = k0 + 1u < D4 ? k0 : 0u;
                xa[i] = x(kk); xb[i] = x(kk + 1u);
                ya[i] = y_raw(kk); yb[i] = y_raw(kk + 1u);
            }
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                const uint32_t k0 = 2u * (4u * b + i);
                if (k0 + 1u < D4) {
                    float z0, z1;
                    orbital_second_pair(u.v[i], xa[i], xb[i], ya[i], yb[i], z0, z1);
                    lds_x[zo + k0 * stride] = z0;
                    lds_x[zo + (k0 + 1u) * stride] = z1;
                }
            }
        } else {
            const uint32_t k = 2u * b;
            const float x0 = x(k), x1 = x(k + 1u);
            lds_x[zo + k * stride] = iid_second(u.v[0], u.v[1], sigma2, x0);
            lds_x[zo + (k + 1u) * stride] = iid_second(u.v[2], u.v[3], sigma2, x1);
        }
    }
};
typedef RowSamplerT<> RowSampler;
// RowSamplerT::fill_first with the block's uniforms drawn by the CALLER (k_mutate_w2: one Philox site serves proposal and coin
// items alike, and only this tail differs): the same reads, the same first_stage_block, the same writes.
template <int RULE> DEV void row_fill_first_drawn(const RowSamplerT<RULE> &s, uint32_t b, const Unit4 &u, bool large) {
    const float *xs = &lds_x[s.x_off + 4u * b * s.stride];
    float *ys = &lds_x[s.y_off + 4u * b * s.stride];
    const float x4[4] = {wrap01(xs[0]), wrap01(xs[s.stride]), wrap01(xs[2u * s.stride]), wrap01(xs[3u * s.stride])};
    float y[4];
    first_stage_block(RowSamplerT<RULE>::orbital ? 2 : s.type, large, u, x4, y);
    ys[0] = y[0]; ys[s.stride] = y[1]; ys[2u * s.stride] = y[2]; ys[3u * s.stride] = y[3];
}
// ONE PAIR of RowSamplerT::fill_second (orbital rule), the block's uniforms drawn by the CALLER (k_mutate_w2<true>: its one Philox
// site serves second-stage items too, and an item is (chain, block b, pair p of the block's four) -- the four items of a block draw
// the same block and each takes its own uniform): the same block rule, the same reads (row 0's for a pair beyond D4), the same
// orbital_second_pair on the same values, the same stores to the same rows. Straight-line code: four reads, ONE wait, the rotation
// on every lane that enters (a large step's item rotates whatever its rows hold), and only the stores are conditional -- a store
// for a pair beyond D4 is never issued: the rows behind a group are the next group's, or the coin rows. A large step
// (timidAfterLarge) stores the block's four uniforms to rows 4b .. 4b+3 through its pairs 0 and 1.
template <int RULE> DEV void row_fill_second_pair_drawn(const RowSamplerT<RULE> &s, uint32_t b, uint32_t p, uint32_t D4, const Unit4 &u, bool large) {
    static_assert(RowSamplerT<RULE>::orbital, "the orbital arm of fill_second");
    const uint32_t nblk = large ? D4 / 4u : (D4 / 2u + 3u) / 4u;
    const uint32_t k0 = 2u * (4u * b + p), kk = k0 + 1u < D4 ? k0 : 0u;
    float xa = lds_x[s.x_off + kk * s.stride], xb = lds_x[s.x_off + (kk + 1u) * s.stride];
    float ya = s.y_raw(kk), yb = s.y_raw(kk + 1u);
    asm volatile("" : "+v"(xa), "+v"(xb), "+v"(ya), "+v"(yb)); // (every read has arrived here)
    const bool hi = (p & 2u) != 0u, odd = (p & 1u) != 0u;
    // (values, not loads: a select between two loads of the struct's fields becomes a load through a selected ADDRESS, and the struct
    // then lives in scratch memory -- see PoolRowSampler::y_raw)
    float u0 = u.v[0], u1 = u.v[1], u2 = u.v[2], u3 = u.v[3];
    asm volatile("" : "+v"(u0), "+v"(u1), "+v"(u2), "+v"(u3));
    const float xi = hi ? (odd ? u3 : u2) : (odd ? u1 : u0); // the pair's angle: draw p
    const float la = odd ? u2 : u0, lb = odd ? u3 : u1;     // a large step's rows 4b + 2p, 4b + 2p + 1: draws 2p, 2p + 1 (p < 2)
    float z0, z1;
    orbital_second_pair(xi, wrap01(xa), wrap01(xb), ya, yb, z0, z1);
    asm volatile("" : "+v"(z0), "+v"(z1)); // (... and the rotation is done here, not behind the stores' exec mask)
    const bool put = b < nblk && (large ? !hi : k0 + 1u < D4);
    const uint32_t zo = s.z_off(), row = large ? 4u * b + 2u * p : k0;
    if (put) {
        lds_x[zo + row * s.stride] = large ? la : z0;
        lds_x[zo + (row + 1u) * s.stride] = large ? lb : z1;
    }
}

// ------------------------------------------------------------------ PSS sampler of k_mutate_v5
// Where a wave's proposal rows live. RowsLds: 64 columns of lds_x (one per chain of the wave). RowsMem: device memory, [dim][chain]
// beside the state -- the builds that give the rows' 8.7 KB of LDS (and a few registers) for a THIRD wave per SIMD on scenes that
// are traversed: there the wave is parked on node fetches more than half of its time, and what covers a fetch is another wave
// (1 -> 2 waves per SIMD: x 1.69 on 1 000 000 triangles, x 1.58 on 50 000). A path step reads its handful of components
// through the L2s instead of LDS: one more fetch beside the ~60 node fetches of the ray it follows.
struct RowsLds {
    DEV float get(uint32_t k, uint32_t col) const { return lds_x[k * 64u + col]; }
    DEV void put(uint32_t k, uint32_t col, float v) const { lds_x[k * 64u + col] = v; }
};
struct RowsMem {
    typedef float __attribute__((address_space(1))) *GPtr;
    GPtr base;       // column 0 of this wave: P.rows + wave_base
    uint32_t stride; // P.n_chains
    // (plain loads and stores: with the streaming hint -- nt, to keep the L2 lines for the BVH -- the row reads themselves miss:
    // 50 000 triangles 3.13e8 -> 2.79e8, 1 000 000 9.16e7 -> 8.52e7. The same hint on the STATE instead -- read once per mutation,
    // a whole mutation of every wave of the XCD apart: it does not survive in the L2 anyway -- loses as well: Cornell at 196 608
    // chains 2.54e9 -> 2.18e9, door 1.09e9 -> 1.05e9, 50 000 triangles 3.45e8 -> 3.26e8. nt bypasses more than the L2.)
    DEV float get(uint32_t k, uint32_t col) const { return base[(size_t) k * stride + col]; }
    DEV void put(uint32_t k, uint32_t col, float v) const { base[(size_t) k * stride + col] = v; }
};

// the proposal rows as the path step sees them: whatever stage is being evaluated sits in the one row group
template <class Rows> struct PoolRowSampler {
    static constexpr bool batch_draws = true; // (device_path.h: path_step reads a step's components together)
    uint32_t lane;
    Rows rows;
    // Mira's ratio alone looks behind the rows (they hold z by then): the state in device memory and the first-stage draws,
    // set by the kernel before a decision (mira_*), block cache of the TAG_S1 stream
    const float *mira_x = nullptr;
    size_t mira_stride = 0;
    uint32_t mira_k0 = 0u, mira_k1 = 0u, mira_major = 0u, mira_chain = 0u, cached = 0xffffffffu;
    u4 blk = {0u, 0u, 0u, 0u};
    DEV void reset_caches() { cached = 0xffffffffu; }
    DEV float row(uint32_t k) const { return rows.get(k, lane); }
    DEV float next(uint32_t k) const { return wrap01(row(k)); }
    DEV float x(uint32_t k) const { return load_global_f32(mira_x + (size_t) k * mira_stride); }
    DEV float y_raw(uint32_t k) { // iid Kelemen step, small (the only caller: mira_ratio)
        if (cached != (k >> 2)) { cached = k >> 2; blk = philox4x32_10(mira_k0, mira_k1, cached, mira_major, mira_chain, TAG_S1); }
        // (values, not loads: a select between two single-use loads of this struct's fields becomes a load through a selected
        // ADDRESS and the whole sampler -- 60 bytes per lane -- then lives in scratch memory: VERDICT r03 #8)
        uint32_t bx = blk.x, by = blk.y, bz = blk.z, bw = blk.w;
        asm volatile("" : "+v"(bx), "+v"(by), "+v"(bz), "+v"(bw));
        const uint32_t c = k & 3u, w = (c & 2u) ? ((c & 1u) ? bw : bz) : ((c & 1u) ? by : bx);
        return iid_first(u32_to_unit(w), x(k));
    }
    DEV float z_raw(uint32_t k) const { return row(k); }
};

// first-stage proposal of the chain in column `col` (state column `xcol` of P.x), dimensions 4b .. 4b+3, from Philox block b
// (the four state components of the block are read by the CALLER, one pass of the flattened loop ahead: v5_state4)
struct State4 { float x0, x1, x2, x3; };
DEV State4 v5_state4(const DParams &P, uint32_t D, size_t xcol, uint32_t b) {
    const bool hi = 4u * b + 2u < D; // D is even: a block holds two pairs or, at the end of the vector, one
    const float *xs = P.x + (size_t) (4u * b) * P.n_chains + xcol;
    State4 X;
    X.x0 = load_global_f32(xs); X.x1 = load_global_f32(xs + P.n_chains);
    X.x2 = load_global_f32(xs + (hi ? 2u : 0u) * (size_t) P.n_chains); X.x3 = load_global_f32(xs + (hi ? 3u : 1u) * (size_t) P.n_chains);
    return X;
}
// (On the pair / component leaves directly, not on first_stage_block: through the shared block k_mutate_v5<15, true, false> with its rows in
// LDS spills 73 scalar registers instead of 63, and four more builds one to six more. RowSamplerT::fill_first is the block's user.)
template <class Rows> DEV void v5_fill_first(const DParams &P, const Rows &rows, uint32_t D, uint32_t col, const State4 &X, uint32_t b, uint32_t major, uint32_t chain, bool large) {
    const Unit4 u = philox_unit4(P.key0, P.key1, b, major, chain, TAG_S1);
    const float u0 = u.v[0], u1 = u.v[1], u2 = u.v[2], u3 = u.v[3];
    const bool hi = 4u * b + 2u < D;
    const float x0 = X.x0, x1 = X.x1, x2 = X.x2, x3 = X.x3;
    float y0, y1, y2, y3;
    if (P.type == 2) {
        orbital_first_pair(u0, u1, x0, x1, y0, y1);
        orbital_first_pair(u2, u3, x2, x3, y2, y3);
    } else {
        y0 = iid_first(u0, x0); y1 = iid_first(u1, x1);
        y2 = iid_first(u2, x2); y3 = iid_first(u3, x3);
    }
    rows.put(4u * b, col, large ? u0 : y0); rows.put(4u * b + 1u, col, large ? u1 : y1);
    if (hi) { rows.put(4u * b + 2u, col, large ? u2 : y2); rows.put(4u * b + 3u, col, large ? u3 : y3); }
}
// second-stage proposal from Philox block b of the TAG_S2 stream, written OVER the first-stage rows: a large step
// (timidAfterLarge) -> dims 4b .. 4b+3 (uniforms); orbital -> the angles of pairs 4b .. 4b+3 = dims 8b .. 8b+7 (reads the y rows
// it replaces); iid kernels -> the Gaussian perturbations of dims 2b, 2b+1 (draws 2k, 2k+1 belong to dim k)
template <class Rows> DEV void v5_fill_second(const DParams &P, const Rows &rows, uint32_t D, uint32_t col, size_t xcol, uint32_t b, uint32_t major, uint32_t chain, bool large) {
    const Unit4 u = philox_unit4(P.key0, P.key1, b, major, chain, TAG_S2);
    if (large) {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i)
            if (4u * b + i < D) rows.put(4u * b + i, col, u.v[i]);
        return;
    }
    if (P.type != 2) {
        const uint32_t k = 2u * b; // (k + 1 < D: the caller's block count)
        const float x0 = load_global_f32(P.x + (size_t) k * P.n_chains + xcol), x1 = load_global_f32(P.x + (size_t) (k + 1u) * P.n_chains + xcol);
        rows.put(k, col, iid_second(u.v[0], u.v[1], P.sigma2, x0));
        rows.put(k + 1u, col, iid_second(u.v[2], u.v[3], P.sigma2, x1));
        return;
    }
    // (all loads first: the stores below may alias them for the compiler, and with the rows in device memory every pair would
    // otherwise wait for its own round trip behind the previous pair's stores)
    float xa[4], xb[4], ya[4], yb[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t k0 = 2u * (4u * b + i);
        const uint32_t kk = k0 + 1u < D ? k0 : 0u;
        xa[i] = load_global_f32(P.x + (size_t) kk * P.n_chains + xcol); xb[i] = load_global_f32(P.x + (size_t) (kk + 1u) * P.n_chains + xcol);
        ya[i] = rows.get(kk, col); yb[i] = rows.get(kk + 1u, col);
    }
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t k0 = 2u * (4u * b + i);
        if (k0 + 1u < D) {
            float z0, z1;
            orbital_second_pair(u.v[i], xa[i], xb[i], ya[i], yb[i], z0, z1);
            rows.put(k0, col, z0);
            rows.put(k0 + 1u, col, z1);
        }
    }
}
// Green & Mira's reverse move and the adoption of a second-stage proposal under Green, for the iid kernels: dims 2b, 2b+1
// from Philox block b of TAG_S2 (z = x + g), block b / 2 of TAG_S1 (y = x + kelemen) and the state in device memory.
//   reverse:  rows := y* = z - (y - x)   (the rows held z, which is recomputed, not read)
//   !reverse: state := wrap(z)            (the rows hold y* by then: DRMLTSampler::accept(second), drmlt_sampler.cpp:189-199)
// A large step (timidAfterLarge): y and z are the uniforms themselves, dims 4b .. 4b+3 of block b of either stream.
template <class Rows> DEV void v5_iid_second_again(const DParams &P, const Rows &rows, uint32_t D, uint32_t col, size_t xcol, uint32_t b, uint32_t major, uint32_t chain, bool large, bool reverse) {
    const Unit4 u2 = philox_unit4(P.key0, P.key1, b, major, chain, TAG_S2);
    if (large) {
        Unit4 u1 = u2;
        if (reverse) u1 = philox_unit4(P.key0, P.key1, b, major, chain, TAG_S1);
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) {
            const uint32_t k = 4u * b + i;
            if (k < D) {
                float *xg = P.x + (size_t) k * P.n_chains + xcol;
                if (reverse) rows.put(k, col, green_reverse(load_global_f32(xg), u1.v[i], u2.v[i]));
                else *xg = wrap01(u2.v[i]);
            }
        }
        return;
    }
    const uint32_t k = 2u * b;
    float *xg0 = P.x + (size_t) k * P.n_chains + xcol, *xg1 = xg0 + P.n_chains;
    const float x0 = load_global_f32(xg0), x1 = load_global_f32(xg1);
    const float z0 = iid_second(u2.v[0], u2.v[1], P.sigma2, x0), z1 = iid_second(u2.v[2], u2.v[3], P.sigma2, x1);
    if (!reverse) { *xg0 = wrap01(z0); *xg1 = wrap01(z1); return; }
    const u4 r1 = philox4x32_10(P.key0, P.key1, k >> 2, major, chain, TAG_S1); // (two of the block's four draws)
    const float ua = (k & 2u) ? u32_to_unit(r1.z) : u32_to_unit(r1.x), ub = (k & 2u) ? u32_to_unit(r1.w) : u32_to_unit(r1.y);
    const float y0 = iid_first(ua, x0), y1 = iid_first(ub, x1); // (both before the stores: 1 - 9 scalar spills in five builds otherwise)
    rows.put(k, col, green_reverse(x0, y0, z0));
    rows.put(k + 1u, col, green_reverse(x1, y1, z1));
}

// ------------------------------------------------------------------ PSS sampler of k_mutate_pssmlt
// PSSMLTSampler (src/integrators/pssmlt/pssmlt_sampler.cpp:93-168, pssmlt_sampler.h:113-143) as a pure function of the
// addressed stream: at the first primarySample of a mutation the reference rewrites the whole vector in order --
// components that already exist are mutated (Kelemen: one draw, toroidal wrap; Gaussian: two draws, modulo 1) or
// redrawn (large step: one draw), components that do not exist yet (beyond what the seed path consumed; only possible
// in a chain's first mutation) are appended as fresh uniforms (one draw) and survive a rejection.
struct PssmltSampler {
    uint32_t key0, key1, chain, major;
    bool large, kelemen;
    float sigma;
    uint32_t lane;
    uint32_t n_exist; // components that exist before this mutation
    u4 b1;
    uint32_t b1_idx;
    DEV void reset_caches() { b1_idx = 0xffffffffu; }
    DEV float u_s1(uint32_t idx) {
        uint32_t blk = idx >> 2;
        if (blk != b1_idx) { b1 = philox4x32_10(key0, key1, blk, major, chain, TAG_S1); b1_idx = blk; }
        return pick4(b1, idx & 3u);
    }
    DEV float x(uint32_t k) const { return lds_x[k * 64u + lane]; }
    DEV float next(uint32_t k) {
        const uint32_t per = (large || kelemen) ? 1u : 2u; // draws taken by an existing component
        if (k >= n_exist) return u_s1(per * n_exist + (k - n_exist));
        if (large) return u_s1(k);
        float value = x(k);
        if (kelemen) {
            float xi = u_s1(k);
            const bool add = xi < 0.5f;
            xi = add ? 2.f * xi : 2.f * (xi - 0.5f);
            const float dv = KELEMEN_S2 * fast_exp2(xi * LOG2_S1_OVER_S2);
            if (add) { value += dv; if (value > 1.f) value -= 1.f; }
            else { value -= dv; if (value < 0.f) value += 1.f; }
            return value;
        }
        const float v = value + gaussian_sample(u_s1(2u * k), u_s1(2u * k + 1u), sigma);
        return v - floorf(v); // math::modulo(v, 1)
    }
};
