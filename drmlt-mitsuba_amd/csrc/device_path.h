// Device code of the DRMLT hot path: ray queries, the scene tables, and the unidirectional estimator as a
// resumable state machine with exactly one ray query per step. (PSS transitions and samplers: device_sampler.h.)
//
// Reference behaviour restated here (paths relative to the reference checkout):
//   sampleSplats (path)      src/libbidir/pathsampler.cpp:529-567
//   MIPathTracer::Li         src/integrators/path/path.cpp:123-321
//   ray epsilons             src/librender/skdtree.cpp:125-129,213-218, scene.cpp:891-893
//   emitter sampling         src/librender/scene.cpp:879-904, shape.cpp:102-127, area.cpp:111-189
//   diffuse / dielectric     src/bsdfs/diffuse.cpp:110-149, dielectric.cpp:228-333
//   perspective sensor       src/sensors/perspective.cpp:271-300
#pragma once
#include "device_bsdf.h"
#include "device_math.h"
#include "device_sampler.h"
#include "device_types.h"

// ------------------------------------------------------------------ ray queries
struct Hit {
    int prim;
    float t, u, v;
};

// Records fetched per lane from device memory, read through a GLOBAL-address-space pointer whatever the origin of `p`:
// a pointer that passed through a copied parameter block (k_mutate_v4's per-section copies) is generic to the compiler,
// which then emits FLAT loads -- both wait counters, the LDS aperture check. T: 16-byte multiple in a 16-byte aligned array.
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
template <class T> DEV T load_global16(const T *p) {
    static_assert(sizeof(T) % 16 == 0, "records are read in 16-byte words");
    typedef const u32x4_t __attribute__((address_space(1))) *GQ;
    const GQ q = (GQ) (uintptr_t) p;
    union { T v; u32x4_t w[sizeof(T) / 16]; } u;
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16u; ++i) u.w[i] = q[i];
    return u.v;
}
// Shading frame of a PRIM_SMOOTH record at the barycentrics (u, v) of p1 and p2 (smooth_frame.h; the hit of path_step and direct_li,
// and -- for its normal alone -- the light samples and emitter hits of both). In: n.x = the record's `n[0]`, which holds the index of
// its table entry; s = a positive multiple of p1 - p0 (the flat primitives' tangent). Out: the frame, or n = s = 0 and false: the
// interpolated normal has no direction, the caller ends the path. The entry is fetched by the lanes that hold such a record from
// device memory in every build: a plain per-lane gather behind the caller's kind test, which a wave without a smooth triangle
// skips as a whole. The step's builds sit at their register limits, so the routine is written to need next to nothing beside
// what the step holds anyway: it takes the index where the flat normal lies, and the entry's three 16-byte words arrive and are
// consumed one after the other (the empty asm keeps the next load behind the sum).
DEV f3 smooth_record_sum(const DParams &P, float index_bits, float u, float v) {
    // a wave-uniform base and a 32-bit byte offset per lane (global_load ... v_off, s[base]): one address register, three dwords a word
    typedef float f32x3_t __attribute__((ext_vector_type(3)));
    typedef const char __attribute__((address_space(1))) *GB;
    typedef const f32x3_t __attribute__((address_space(1))) *GQ;
    const GB q = (GB) (uintptr_t) P.normals + (__float_as_uint(index_bits) - SMOOTH_INDEX_BIAS) * (uint32_t) sizeof(DSmooth);
    const f32x3_t w0 = *(GQ) q;
    f3 a = mk3(w0.x, w0.y, w0.z);
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z) : : "memory");
    const f32x3_t w1 = *(GQ) (q + 16);
    a = fma3(mk3(w1.x, w1.y, w1.z), u, a);
    asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z) : : "memory");
    const f32x3_t w2 = *(GQ) (q + 32);
    a = fma3(mk3(w2.x, w2.y, w2.z), v, a);
    return a;
}
DEV bool smooth_record_frame(const DParams &P, float u, float v, f3 &n, f3 &s) {
    const f3 a = smooth_record_sum(P, n.x, u, v);
    const SmoothFrame F = smooth_finish(a.x, a.y, a.z, s.x, s.y, s.z);
    n = mk3(F.nx, F.ny, F.nz);
    s = mk3(F.sx, F.sy, F.sz);
    return !is_zero3(n);
}
// The normal alone, for an area light's sample and an emitter hit: in n.x the index, out the unit normal, or 0 when it has no
// direction (the light sample's pdf is then 0, the hit's cosine 0). No tangent takes part.
DEV void smooth_record_normal(const DParams &P, float u, float v, f3 &n) {
    const f3 a = smooth_record_sum(P, n.x, u, v);
    const SmoothFrame F = smooth_finish_normal(a.x, a.y, a.z);
    n = mk3(F.nx, F.ny, F.nz);
}
// Samplers whose components are plain reads (proposal rows in LDS or in device memory) have the draws of a path step requested
// together: a loop over `need` reads, each waited for, was `need` LDS round trips per step even with the rows in LDS (round 4: config 2
// 2.11e9 -> 2.24e9, the 2000-triangle soup 5.82e8 -> 6.01e8; with the rows in device memory it is the difference between one and five
// trips through the L2). The lazy samplers (Philox inside next()) keep the loop: one copy of their code.
template <class S, class = void> struct draws_batched : std::false_type {};
template <class S> struct draws_batched<S, std::void_t<decltype(S::batch_draws)>> : std::integral_constant<bool, S::batch_draws> {};
DEV void atomic_add_global_f32(float *p, float v) { // no-return float add on device memory (global_atomic_add_f32)
    (void) __hip_atomic_fetch_add((float __attribute__((address_space(1))) *) (uintptr_t) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One primitive against one ray. `P` is wave-uniform in the brute-force loop (SGPR operands).
// Flat primitives are branch-free (selects only): no exec-mask traffic in the hot loop.
template <int FEAT = 15> DEV void intersect_prim(const DPrim &P, int idx, f3 o, f3 d, float tmin, Hit &h) {
    f3 lo = mk3(fmaf(P.m[0], o.x, fmaf(P.m[1], o.y, fmaf(P.m[2], o.z, P.m[3]))),
                fmaf(P.m[4], o.x, fmaf(P.m[5], o.y, fmaf(P.m[6], o.z, P.m[7]))),
                fmaf(P.m[8], o.x, fmaf(P.m[9], o.y, fmaf(P.m[10], o.z, P.m[11]))));
    f3 ld = mk3(fmaf(P.m[0], d.x, fmaf(P.m[1], d.y, P.m[2] * d.z)), fmaf(P.m[4], d.x, fmaf(P.m[5], d.y, P.m[6] * d.z)),
                fmaf(P.m[8], d.x, fmaf(P.m[9], d.y, P.m[10] * d.z)));
    if (!(FEAT & 4) || P.type != PRIM_SPHERE) { // wave-uniform branch (compiled out for sphere-free scenes)
        float t = -lo.z * fast_rcp(ld.z);
        float u = fmaf(t, ld.x, lo.x), v = fmaf(t, ld.y, lo.y);
        // triangle: u, v, 1-u-v >= 0; parallelogram (rectangle or merged triangle pair): u, v, 1-u, 1-v >= 0.
        // The kind is wave-uniform (SGPR), so this is selects on a scalar condition, no exec-mask traffic.
        const bool tri = P.type == PRIM_TRIANGLE;
        const float w = tri ? 1.f - (u + v) : fminf(1.f - u, 1.f - v);
        // (w >= 0 on its own: a ray parallel to the plane has t = +inf, which passes t <= h.t for a ray without a far end; where one of
        // the rows u, v is orthogonal to it too, that coordinate and a triangle's w are inf * 0 = NaN, and fminf skips a NaN)
        bool hit = fminf(fminf(u, v), w) >= 0.f && w >= 0.f && t >= tmin && t <= h.t;
        int id = idx;
        if (P.type == PRIM_QUAD2) { // sub-triangle (a,b,c) for v <= u, (a,c,d) otherwise; its own barycentrics
            const bool second = v > u;
            id = idx + (second ? 1 : 0);
            const float uu = second ? u : u - v, vv = second ? v - u : v;
            u = uu; v = vv;
        }
        h.prim = hit ? id : h.prim;
        h.t = hit ? t : h.t;
        h.u = hit ? u : h.u;
        h.v = hit ? v : h.v;
    } else {
        // unit sphere; discriminant from the closest-approach vector (stable in fp32)
        float A = dot3(ld, ld), invA = fast_rcp(A);
        float b = dot3(lo, ld);
        f3 l = fma3(ld, -b * invA, lo);
        float disc = A * (1.f - dot3(l, l));
        if (disc >= 0.f) {
            float sq = sqrtf(disc);
            float q = (b < 0.f) ? -(b - sq) : -(b + sq); // = -0.5 (B -/+ sqrt(discrim)) with B = 2b
            float c = dot3(lo, lo) - 1.f;
            float t0 = q * invA, t1 = c / q;
            float nearT = fminf(t0, t1), farT = fmaxf(t0, t1);
            // sphere.cpp:176-188
            if (nearT <= h.t && farT >= tmin) {
                float t = nearT;
                bool ok = true;
                if (nearT < tmin) { t = farT; ok = farT <= h.t; }
                if (ok) { h.prim = idx; h.t = t; h.u = 0.f; h.v = 0.f; }
            }
        }
    }
}

// The same test for one record PER LANE (a BVH leaf), as straight-line code: with the kind in a vector register the
// selects of intersect_prim become branches over the lane mask. `ok`: the lane holds a leaf (the others computed on zeros).
template <int FEAT = 15> DEV void intersect_leaf(const DPrim &P, bool ok, f3 o, f3 d, float tmin, Hit &h) {
    const f3 lo = mk3(fmaf(P.m[0], o.x, fmaf(P.m[1], o.y, fmaf(P.m[2], o.z, P.m[3]))),
                      fmaf(P.m[4], o.x, fmaf(P.m[5], o.y, fmaf(P.m[6], o.z, P.m[7]))),
                      fmaf(P.m[8], o.x, fmaf(P.m[9], o.y, fmaf(P.m[10], o.z, P.m[11]))));
    const f3 ld = mk3(fmaf(P.m[0], d.x, fmaf(P.m[1], d.y, P.m[2] * d.z)), fmaf(P.m[4], d.x, fmaf(P.m[5], d.y, P.m[6] * d.z)),
                      fmaf(P.m[8], d.x, fmaf(P.m[9], d.y, P.m[10] * d.z)));
    const int type = P.type;
    const float t = -lo.z * fast_rcp(ld.z);
    const float u = fmaf(t, ld.x, lo.x), v = fmaf(t, ld.y, lo.y);
    const float w_tri = 1.f - (u + v), w_par = fminf(1.f - u, 1.f - v);
    const float w = type == PRIM_TRIANGLE ? w_tri : w_par;
    bool hit = ok & (fminf(fminf(u, v), w) >= 0.f) & (w >= 0.f) & (t >= tmin) & (t <= h.t); // (w >= 0: intersect_prim has the reason)
    if (FEAT & 4) hit = hit & (type != PRIM_SPHERE);
    const bool quad2 = type == PRIM_QUAD2, second = quad2 & (v > u); // sub-triangle (a,b,c) for v <= u, (a,c,d) otherwise; its own barycentrics
    const float uq = second ? u : u - v, vq = second ? v - u : v;
    h.prim = hit ? P.shade + (second ? 1 : 0) : h.prim;
    h.t = hit ? t : h.t;
    h.u = hit ? (quad2 ? uq : u) : h.u;
    h.v = hit ? (quad2 ? vq : v) : h.v;
    if (FEAT & 4) {
        const bool sph = ok & (type == PRIM_SPHERE);
        if (__ballot(sph)) { // wave-uniform: scenes with spheres keep the general test for them
            if (sph) intersect_prim<FEAT>(P, P.shade, o, d, tmin, h);
        }
    }
}

// closest hit in [tmin, tmax] over all primitives. The loop index is wave-uniform, so the 64 B
// primitive record is fetched through the SCALAR cache (constant address space => s_load_dwordx16)
// and feeds the VALU ops as SGPR operands: no VGPRs, no vector-memory latency in the loop.
typedef const DPrim __attribute__((address_space(4))) *ScalarPrimPtr;

template <int FEAT = 15> DEV Hit trace_brute(const DParams &P, f3 o, f3 d, float tmin, float tmax) {
    Hit h{-1, tmax, 0.f, 0.f};
    const int n = P.n_prims;
    if (P.debug & 64) { // A/B: vector-memory path
        for (int i = 0; i < n; ++i) intersect_prim(P.prims[i], P.prims[i].shade, o, d, tmin, h);
        return h;
    }
    ScalarPrimPtr sp = (ScalarPrimPtr) (uintptr_t) P.prims;
    // ping-pong software pipeline: while primitive i is tested (~35 VALU ops) the record of
    // primitive i+1 is already in flight through the scalar cache, and vice versa
    auto load = [&](int i, DPrim &G) {
#pragma unroll
        for (int k = 0; k < 12; ++k) G.m[k] = sp[i].m[k];
        const int ks = sp[i].kind_shade; // one scalar dword: kind in the low byte, shading record index above
        G.type = ks & 0xff;
        G.shade = ks >> 8;
    };
    // SMEM returns out of order, so the only wait is lgkmcnt(0) = "everything outstanding". The
    // empty asm pins that wait on record X BEFORE the request for the other record is issued;
    // otherwise the compiler's wait for X (placed at X's first use) would also wait for the
    // record just requested and the pipeline would collapse to one load at a time.
#define PIN(G) asm volatile("" ::"s"(G.m[0]), "s"(G.m[4]), "s"(G.m[8]), "s"(G.type), "s"(G.shade))
    DPrim A, B;
    load(0, A);
    for (int i = 0; i < n; i += 2) {
        PIN(A);
        load(i + 1 < n ? i + 1 : i, B);
        intersect_prim<FEAT>(A, A.shade, o, d, tmin, h);
        PIN(B);
        load(i + 2 < n ? i + 2 : i, A);
        if (i + 1 < n) intersect_prim<FEAT>(B, B.shade, o, d, tmin, h);
    }
#undef PIN
    return h;
}

// 4-wide BVH traversal, one ray per lane, RESUMABLE: the traversal state of a lane (`Trav` + its column of the LDS stack)
// survives a return, so a caller whose lanes need very different numbers of node visits (k_mutate_v4 on BVH scenes: the
// rays of 32 unrelated paths and their shadow rays) can take the lanes that have finished out of the loop, let them
// shade and come back with new rays, while the long traversals simply continue -- the wave-level regrouping of live rays
// the lock-step form lacks (there a wave waits for its longest ray, lane utilisation ~10 %).
//   * node = 128 B, four child boxes (DBvh4Node); the hit children are ordered near-to-far by a 5-comparator network on
//     (entry distance | child slot) keys and the far ones pushed;
//   * per-lane stack in LDS, column layout [slot][lane]: a push or pop is one ds access without bank conflicts (a stack
//     in registers is indexed by a divergent sp: the compiler turns every push and pop into a compare-and-select over all
//     entries, ~100 VALU per node); the builder bounds the tree depth so that a push never overflows;
//   * leaf references and node indices share the stack entries (32 bit, or 16 bit for scenes that fit);
//   * "while-while" with a vote: per iteration the wave either advances the lanes that hold inner nodes or the lanes that
//     hold leaves, whichever are more.
struct Trav {
    f3 o, d, inv, oi;
    float tmin;
    Hit h;
    int cur, sp;      // cur >= 0 inner node, < 0 leaf reference
    int ovf;          // entries of this lane's stack that sit in the overflow area (0 for trees the LDS column holds)
    uint32_t rx, ry, rz; // 1 where the ray runs against the axis: the NEAR plane of a box is then its upper one (row lo/hi swapped at the load)
    bool active, any_hit;
    uint32_t n_nodes, n_prims; // fetched so far by this lane (k_mutate_v4 reports them: the scene part of the algorithmic bytes)
    uint32_t it_inner, it_leaf; // wave-uniform: traversal iterations of each kind (lane occupancy = n_nodes / (64 it_inner) ...)
};

DEV void trav_begin(Trav &T, f3 o, f3 d, float tmin, float tmax, bool any_hit) {
    T.o = o; T.d = d;
    T.inv = mk3(1.f / d.x, 1.f / d.y, 1.f / d.z);
    T.oi = mk3(-o.x * T.inv.x, -o.y * T.inv.y, -o.z * T.inv.z);
    T.tmin = tmin;
    T.h = Hit{-1, tmax, 0.f, 0.f};
    T.cur = 0; T.sp = 0; T.ovf = 0;
    T.rx = T.inv.x < 0.f ? 1u : 0u; T.ry = T.inv.y < 0.f ? 1u : 0u; T.rz = T.inv.z < 0.f ? 1u : 0u;
    T.active = true; T.any_hit = any_hit;
}
DEV void trav_reset_counters(Trav &T) { T.n_nodes = T.n_prims = T.it_inner = T.it_leaf = 0u; }

DEV unsigned umin2(unsigned a, unsigned b) { return a < b ? a : b; }
DEV unsigned umax2(unsigned a, unsigned b) { return a < b ? b : a; }

// One wave's traversal machinery: the LDS stack column of this lane, the buffer resources of the node / primitive arrays, and
// `step` = ONE iteration for the whole wave (nodes or leaves, by vote). Two loops drive it: trav_run (every lane keeps the
// ray it was given until a slice ends) and k_mutate_v5's pool loop (a lane that finishes a ray takes the next one from
// the wave's ray queue inside the loop).
template <class StackT, class PT, bool OVF = true, int CAP = BVH_STACK, int FEAT = 15> struct TravLoop {
    static constexpr int SPILL = CAP / 2; // entries moved at a time
    static constexpr unsigned TRAV_NO_FETCH = 0xfffff000u;
    const PT &P;
    StackT *const stk;
    const size_t ovf_col;
    const bool has_ovf;
    const __amdgpu_buffer_rsrc_t r_bvh, r_prm;
    // `column`: this lane's column of a (CAP + 3) x 64 array in LDS. The column holds CAP entries (+ 3 spare: the branch-free
    // pushes write up to three entries above the top; lanes that hold no node: all three, from row CAP). A tree deeper than
    // CAP / 3 levels can need more. Slow paths: before a node's pushes could run past the column its SPILL OLDEST entries move
    // to this lane's column of an overflow area in memory and the rest slides down; a pop that finds the column empty brings
    // the newest SPILL back. Node and primitive records are raw buffers (byte offsets; drmlt_create refuses arrays of 2 GiB
    // and more).
    DEV TravLoop(const PT &P_, StackT *column)
        : P(P_), stk(column), ovf_col((size_t) blockIdx.x * 64u + (threadIdx.x & 63u)), has_ovf(OVF && P_.bvh_overflow != nullptr),
          r_bvh(__builtin_amdgcn_make_buffer_rsrc((void *) (uintptr_t) P_.bvh, 0, 0x80000000u, 0x00020000)),
          r_prm(__builtin_amdgcn_make_buffer_rsrc((void *) (uintptr_t) P_.prims, 0, 0x80000000u, 0x00020000)) {}
    DEV void spill(Trav &T) const {
        for (int i = 0; i < SPILL; ++i) P.bvh_overflow[(size_t) (T.ovf + i) * P.bvh_ovf_lanes + ovf_col] = (int) stk[i * 64];
        for (int i = SPILL; i < T.sp; ++i) stk[(i - SPILL) * 64] = stk[i * 64];
        T.sp -= SPILL; T.ovf += SPILL;
    }
    DEV void refill(Trav &T) const {
        T.ovf -= SPILL;
        for (int i = 0; i < SPILL; ++i) stk[i * 64] = (StackT) P.bvh_overflow[(size_t) (T.ovf + i) * P.bvh_ovf_lanes + ovf_col];
        T.sp = SPILL;
    }
    // Advance the lanes with `mine` set by one iteration. Returns, per lane, whether its traversal FINISHED in this iteration;
    // `any` (wave-uniform): some lane still had a traversal to advance (false: nothing was done).
    DEV bool step(Trav &T, bool mine, bool &any) const {
        const bool run = mine && T.active;
        const unsigned long long m_inner = __ballot(run && T.cur >= 0), m_leaf = __ballot(run && T.cur < 0);
        any = (m_inner | m_leaf) != 0ull;
        if (!any) return false;
        bool done_now = false;
        // Both blocks below are STRAIGHT-LINE code for the whole wave: a lane that does not hold the kind being advanced
        // computes on whatever its registers hold and keeps nothing of it (its pushes land in the spare rows above the
        // column, every state update is a select on `ok`). Only the fetches sit under the lane mask. As per-lane branches
        // the same code cost ~30 register copies and ~50 scalar instructions per iteration at the merges of its nested
        // conditions -- about as much as the node test itself.
        if (__popcll(m_inner) * P.trace_vote >= __popcll(m_leaf) * 16) { // a leaf test costs about 0.4 node tests: see drmlt_capi.cpp
            T.it_inner++;
            const bool ok = run && T.cur >= 0;
            if (has_ovf) { if (ok && T.sp > CAP - 3) spill(T); }
            // The node's rows (16 bytes each: lox, hix, loy, hiy, loz, hiz, child) are fetched with the lo / hi rows of an
            // axis SWAPPED where the ray runs against it: the first of each pair then holds the four NEAR planes, the second
            // the four FAR ones, and the slab test needs no per-axis min / max (24 of ~110 vector instructions per node).
            // Fetched through a buffer resource: a lane that holds no node offers an offset beyond the resource's range, for which
            // the load returns zeros without a memory access -- no lane mask, no branch, no register to initialise.
            const unsigned nb = ok ? (unsigned) T.cur << 7 : TRAV_NO_FETCH;
            const u32x4_t nxr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + (T.rx << 4), 0, 0), fxr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + ((T.rx ^ 1u) << 4), 0, 0);
            const u32x4_t nyr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + 32u + (T.ry << 4), 0, 0), fyr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + 32u + ((T.ry ^ 1u) << 4), 0, 0);
            const u32x4_t nzr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + 64u + (T.rz << 4), 0, 0), fzr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + 64u + ((T.rz ^ 1u) << 4), 0, 0);
            const u32x4_t chr = __builtin_amdgcn_raw_buffer_load_b128(r_bvh, nb + 96u, 0, 0);
            T.n_nodes += ok ? 1u : 0u;
            typedef float f2 __attribute__((ext_vector_type(2)));
            const f2 ix = {T.inv.x, T.inv.x}, iy = {T.inv.y, T.inv.y}, iz = {T.inv.z, T.inv.z};
            const f2 ox = {T.oi.x, T.oi.x}, oy = {T.oi.y, T.oi.y}, oz = {T.oi.z, T.oi.z};
            float tn[4];
            bool hitc[4];
            const int childc[4] = {(int) chr.x, (int) chr.y, (int) chr.z, (int) chr.w};
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) { // children (0, 1), then (2, 3): v_pk_fma_f32
                auto pr = [&](const u32x4_t &r) { return h2 == 0 ? (f2){__uint_as_float(r.x), __uint_as_float(r.y)} : (f2){__uint_as_float(r.z), __uint_as_float(r.w)}; };
                const f2 t0x = __builtin_elementwise_fma(pr(nxr), ix, ox), t1x = __builtin_elementwise_fma(pr(fxr), ix, ox);
                const f2 t0y = __builtin_elementwise_fma(pr(nyr), iy, oy), t1y = __builtin_elementwise_fma(pr(fyr), iy, oy);
                const f2 t0z = __builtin_elementwise_fma(pr(nzr), iz, oz), t1z = __builtin_elementwise_fma(pr(fzr), iz, oz);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const float a = fmaxf(fmaxf(t0x[q], t0y[q]), fmaxf(t0z[q], T.tmin));
                    const float f = fminf(fminf(t1x[q], t1y[q]), fminf(t1z[q], T.h.t));
                    tn[2 * h2 + q] = a;
                    hitc[2 * h2 + q] = a <= f;
                }
            }
            // Sort keys, nearest first. 16-bit child references: the key carries the child itself -- entry distance in the
            // upper half (its bit pattern orders like an unsigned: tn >= tmin >= 0; 7 mantissa bits are plenty for an ORDER),
            // reference in the lower half. 32-bit references: the key carries the SLOT in its two low mantissa bits.
            unsigned key[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned kk = sizeof(StackT) == 2 ? ((__float_as_uint(tn[c]) & 0xffff0000u) | ((unsigned) childc[c] & 0xffffu))
                                                        : ((__float_as_uint(tn[c]) & 0x7ffffffcu) | (unsigned) c);
                key[c] = hitc[c] ? kk : 0xffffffffu;
            }
            // sorting network (0,1)(2,3)(0,2)(1,3)(1,2)
            const unsigned a0 = umin2(key[0], key[1]), a1 = umax2(key[0], key[1]), a2 = umin2(key[2], key[3]), a3 = umax2(key[2], key[3]);
            const unsigned b0 = umin2(a0, a2), b2 = umax2(a0, a2), b1 = umin2(a1, a3), b3 = umax2(a1, a3);
            const unsigned k0 = b0, k1 = umin2(b1, b2), k2 = umax2(b1, b2), k3 = b3;
            auto child_of = [&](unsigned k) -> int {
                if constexpr (sizeof(StackT) == 2) return (int) (short) (k & 0xffffu);
                else {
                    const int lo = (k & 1u) ? childc[1] : childc[0], hi = (k & 1u) ? childc[3] : childc[2];
                    return (k & 2u) ? hi : lo;
                }
            };
            // far ones first, so that the nearest pending child ends on top; a write above the top of the stack is harmless
            int sp = ok ? T.sp : CAP;
            stk[sp * 64] = (StackT) child_of(k3); sp += k3 != 0xffffffffu ? 1 : 0;
            stk[sp * 64] = (StackT) child_of(k2); sp += k2 != 0xffffffffu ? 1 : 0;
            stk[sp * 64] = (StackT) child_of(k1); sp += k1 != 0xffffffffu ? 1 : 0;
            const bool has0 = k0 != 0xffffffffu;
            const int below = sp > 0 ? sp - 1 : 0;
            const int top = stk[below * 64]; // the pop, should the node have no child to descend into
            bool fin = !has0 && sp == 0;
            T.cur = ok && !fin ? (has0 ? child_of(k0) : top) : T.cur;
            T.sp = ok ? (has0 ? sp : below) : T.sp;
            if (has_ovf) { if (ok && fin && T.ovf > 0) { refill(T); T.cur = stk[--T.sp * 64]; fin = false; } }
            done_now = ok && fin;
            T.active = T.active && !done_now;
        } else {
            T.it_leaf++;
            const bool ok = run && T.cur < 0;
            // leaf reference: ~(first << shift | count); shift = 0 when every leaf holds one primitive (the default build)
            const int first = ~T.cur >> P.bvh_leaf_shift, n = P.bvh_leaf_shift ? (~T.cur & 7) : 1;
            T.n_prims += ok ? (uint32_t) n : 0u;
            if (P.bvh_leaf_shift == 0) { // wave-uniform
                union { DPrim v; u32x4_t w[4]; } G;
                const unsigned pb = ok ? (unsigned) first << 6 : TRAV_NO_FETCH;
#pragma unroll
                for (unsigned k = 0; k < 4u; ++k) G.w[k] = __builtin_amdgcn_raw_buffer_load_b128(r_prm, pb + 16u * k, 0, 0);
                intersect_leaf<FEAT>(G.v, ok, T.o, T.d, T.tmin, T.h);
            } else if (ok) {
                for (int i = 0; i < n; ++i) {
                    const DPrim G = load_global16(P.prims + first + i);
                    intersect_prim(G, G.shade, T.o, T.d, T.tmin, T.h);
                }
            }
            const bool found = T.any_hit && T.h.prim >= 0;
            const int sp = ok ? T.sp : 0;
            const int below = sp > 0 ? sp - 1 : 0;
            const int top = stk[below * 64];
            bool fin = found || sp == 0;
            T.cur = ok && !fin ? top : T.cur;
            T.sp = ok ? below : T.sp;
            if (has_ovf) { if (ok && !found && sp == 0 && T.ovf > 0) { refill(T); T.cur = stk[--T.sp * 64]; fin = false; } }
            done_now = ok && fin;
            T.active = T.active && !done_now;
        }
        return done_now;
    }
};

// Advance the traversals of the lanes with `mine` set until all of them are done or, if yield_lanes > 0, at least that
// many lanes of the wave have finished during this call.
// StackT: int, or short when every node index and leaf reference of the scene fits 15 bits (drmlt_create decides): half
// the LDS, which is what lets k_mutate_v4 keep 8 waves per CU on BVH scenes (measured: 1.13e8 -> 2.0e8 mutations/s on the
// 2000-triangle soup, all of it occupancy).
// OVF: compile the spill / refill paths in (k_mutate_v4 has a build without them for trees that fit the column: they cost
// 4 % there even when never taken).
// CAP: entries of the LDS column (k_mutate_v4 gives its 32-bit stacks 12 instead of 24 -- with the overflow paths the column
// only has to hold the hot top of the stack, and 3.5 KB instead of 6.5 KB keep eight waves on a CU).
template <class StackT, class PT, bool OVF = true, int CAP = BVH_STACK, int FEAT = 15> DEV void trav_run(const PT &P, Trav &T, bool mine, int yield_lanes) {
    __shared__ StackT bvh_stack[(CAP + 3) * 64];
    const TravLoop<StackT, PT, OVF, CAP, FEAT> L(P, bvh_stack + (threadIdx.x & 63u)); // every kernel that traces runs one wave per workgroup
    int finished = 0;
    for (;;) {
        if (yield_lanes > 0 && finished >= yield_lanes) break;
        bool any;
        const bool done_now = L.step(T, mine, any);
        if (!any) break;
        finished += __popcll(__ballot(done_now));
    }
}

// closest (or any) hit in [tmin, tmax], traversal run to completion
template <class PT> DEV Hit trace_bvh(const PT &P, f3 o, f3 d, float tmin, float tmax, bool any_hit) {
    Trav T;
    trav_reset_counters(T);
    trav_begin(T, o, d, tmin, tmax, any_hit);
    trav_run<int>(P, T, true, 0);
    return T.h;
}

// Brute-force loop for scenes of flat primitives only (rectangles, triangles, merged pairs). Same tests as
// intersect_prim, restructured around the scalar unit, which was issuing almost as many instructions as the VALU:
//   * DPrimFlat: the (u, v) rows arrive as aligned SGPR pairs -> packed FMAs without scalar shuffles;
//   * two sentinel records end the array, so the software pipeline reads ahead without clamping its index and the
//     loads take immediate offsets from one running pointer;
//   * the sub-triangle of a merged pair is resolved once, for the final hit, not per record.
typedef float float2v __attribute__((ext_vector_type(2)));
typedef const DPrimFlat __attribute__((address_space(4))) *ScalarFlatPtr;

struct FlatRec {
    float2v cx, cy, cz, cw;
    float z0, z1, z2, z3;
    int ks;
};

// The (u, v) rows of a record applied to a point and to a direction. BY_COMPONENT (trace_held): each component as its own chain of
// fmaf / multiply in the nesting of the packed expression. A packed fused multiply-add is two independent fused multiply-adds, so
// every component rounds as in the packed form (the unit is built with -ffp-contract=on: the packed expression fuses exactly where
// the fmaf stands). Why: a v_pk_fma_f32 occupies the SIMD for two passes, and in k_mutate_w2h's loop, which is bound by VALU issue
// at two waves per SIMD, the ray pass's 32 packed instructions cost more than the 50-odd plain ones that replace them (DESIGN
// section 7a, r20: +0.5 %). The streaming loops keep the packed rows: their records arrive as aligned scalar register pairs.
template <bool BY_COMPONENT> DEV float2v rows_at_point(float2v cx, float2v cy, float2v cz, float2v cw, f3 o) {
    if constexpr (BY_COMPONENT) return float2v{fmaf(cx.x, o.x, fmaf(cy.x, o.y, fmaf(cz.x, o.z, cw.x))), fmaf(cx.y, o.x, fmaf(cy.y, o.y, fmaf(cz.y, o.z, cw.y)))};
    else return cx * o.x + (cy * o.y + (cz * o.z + cw));
}
template <bool BY_COMPONENT> DEV float2v rows_at_direction(float2v cx, float2v cy, float2v cz, f3 d) {
    if constexpr (BY_COMPONENT) return float2v{fmaf(cx.x, d.x, fmaf(cy.x, d.y, cz.x * d.z)), fmaf(cx.y, d.x, fmaf(cy.y, d.y, cz.y * d.z))};
    else return cx * d.x + (cy * d.y + cz * d.z);
}
template <bool BY_COMPONENT> DEV float2v rows_along(float2v ld, float t, float2v lo) {
    if constexpr (BY_COMPONENT) return float2v{fmaf(ld.x, t, lo.x), fmaf(ld.y, t, lo.y)};
    else return ld * t + lo;
}

template <bool TRI> DEV void test_flat(const FlatRec &G, f3 o, f3 d, float tmin, float &best_t, float2v &best_uv, int &best_ks) {
    const float ldz = fmaf(G.z0, d.x, fmaf(G.z1, d.y, G.z2 * d.z));
    const float loz = fmaf(G.z0, o.x, fmaf(G.z1, o.y, fmaf(G.z2, o.z, G.z3)));
    const float t = -loz * fast_rcp(ldz);
    const float2v lo = G.cx * o.x + (G.cy * o.y + (G.cz * o.z + G.cw));
    const float2v ld = G.cx * d.x + (G.cy * d.y + G.cz * d.z);
    const float2v uv = ld * t + lo;
    float w;
    if (TRI && (G.ks & 0xff) == PRIM_TRIANGLE) w = 1.f - (uv.x + uv.y);
    else { const float2v om = 1.f - uv; w = fminf(om.x, om.y); }
    bool hit = fminf(fminf(uv.x, uv.y), w) >= 0.f && t >= tmin && t <= best_t;
    // a triangle's w can be NaN behind a non-negative minimum (intersect_prim has the reason). A parallelogram's cannot: the rows u, v and the
    // normal's span space, so a direction orthogonal to the normal's row and to one of u, v is not orthogonal to the other; that coordinate is
    // +-inf at t = +inf, and it or its 1 - x fails the test
    if (TRI) hit = hit && w >= 0.f;
    best_t = hit ? t : best_t;
    best_uv.x = hit ? uv.x : best_uv.x;
    best_uv.y = hit ? uv.y : best_uv.y;
    best_ks = hit ? G.ks : best_ks;
}
// test_flat<false> with its rows component by component (trace_held: no plain triangle among the records it is given)
DEV void test_flat_held(const FlatRec &G, f3 o, f3 d, float tmin, float &best_t, float2v &best_uv, int &best_ks) {
    const float ldz = fmaf(G.z0, d.x, fmaf(G.z1, d.y, G.z2 * d.z));
    const float loz = fmaf(G.z0, o.x, fmaf(G.z1, o.y, fmaf(G.z2, o.z, G.z3)));
    const float t = -loz * fast_rcp(ldz);
    const float2v lo = rows_at_point<true>(G.cx, G.cy, G.cz, G.cw, o);
    const float2v ld = rows_at_direction<true>(G.cx, G.cy, G.cz, d);
    const float2v uv = rows_along<true>(ld, t, lo);
    const float w = fminf(1.f - uv.x, 1.f - uv.y);
    const bool hit = fminf(fminf(uv.x, uv.y), w) >= 0.f && t >= tmin && t <= best_t;
    best_t = hit ? t : best_t;
    best_uv.x = hit ? uv.x : best_uv.x;
    best_uv.y = hit ? uv.y : best_uv.y;
    best_ks = hit ? G.ks : best_ks;
}

// ---- cuboid records (host side and the argument why this equals the loop over the separate faces: box_merge.h)
// The ray in the cuboid's own coordinates b in [0, 1]^3 (the affine map of a flat record), the three slabs, then the face the
// ray ENTERS through (entry distance >= tmin) or, failing that -- the ray starts inside, or the scene has no face there: the
// open side of a room -- the face it LEAVES through. Which of the two is needed is mostly the same for a whole wave (rays start
// inside a room and outside a box), so each half sits behind a wave-uniform test. The hit is handed on as the face's half-word
// (exists | code << 1 | kind << 4 | shade << 6) and the in-face coordinates (p, q) = (b[j], b[k]), j < k the other two axes;
// trace_flat turns the winner's into the face's own (u, v) and record once, after the loops.
#define BOX_FACE_FLAG 0x40000000
typedef const DPrimBox __attribute__((address_space(4))) *ScalarBoxPtr;
struct BoxRec {
    float2v cx, cy, cz, cw;
    float z0, z1, z2, z3;
    uint32_t f0, f1, f2; // face words of axes 0, 1, 2: low half side 0 (b = 0), high half side 1 (b = 1)
};
// ONE candidate face for a lane: the face the ray enters through (`leave` false) or leaves through. Moving along +axis a ray
// enters through side 0 and leaves through side 1, along -axis the other way round: side = (ld[axis] < 0) != leave. Everything by
// value (arguments and result): through references the choice among the three face words compiles to a load through a selected
// address, and the words then live in scratch memory.
struct BoxCand { float t, p, q; uint32_t hc; };
template <bool BY_COMPONENT = false>
DEV BoxCand box_candidate(bool leave, float nx, float ny, float fx, float fy, float tnear, float tfar, float2v lo, float2v ld, float loz, float ldz,
                          uint32_t f0, uint32_t f1, uint32_t f2) {
    BoxCand c;
    c.t = leave ? tfar : tnear;
    const float cx = leave ? fx : nx, cy = leave ? fy : ny;
    const bool a0 = cx == c.t, a1 = cy == c.t;                        // the axis whose plane the ray crosses at t
    const float lda = a0 ? ld.x : (a1 ? ld.y : ldz);
    const uint32_t w = a0 ? f0 : (a1 ? f1 : f2);
    c.hc = ((lda < 0.f) != leave) ? w >> 16 : w & 0xffffu;
    const float2v bxy = rows_along<BY_COMPONENT>(ld, c.t, lo);
    const float bzz = fmaf(ldz, c.t, loz);
    c.p = a0 ? bxy.y : bxy.x; c.q = (a0 || a1) ? bzz : bxy.y;       // in-face coordinates: axis 0 (y, z), 1 (x, z), 2 (x, y)
    return c;
}
// test_box<true>'s `hole` as ONE compare of a word that is pinned to a register: the ballot of a compare is the compare's mask, while of
// an `and` of three masks the compiler makes a 0 / 1 integer and compares that again (two instructions a cuboid, and the pin keeps
// it from folding the word back into the three masks).
DEV bool held_hole(bool through_from_outside, uint32_t hc) {
    uint32_t entry_exists = through_from_outside ? hc & 1u : 1u;
    asm volatile("" : "+v"(entry_exists));
    return entry_exists == 0u;
}
// OPEN_KNOWN (trace_held): whether the cuboid lacks a face at all is a property of its three face words, and the caller knows it as a
// wave-uniform flag. A closed cuboid has every entry face, `hole` is false on every lane, and neither the per-lane test nor its
// ballot is computed: one scalar test in their place. An open cuboid runs the test and the block as they are.
// BY_COMPONENT (trace_held): the rows as scalar chains (rows_at_point).
template <bool OPEN_KNOWN = false, bool BY_COMPONENT = false>
DEV void test_box(const BoxRec &G, f3 o, f3 d, float tmin, float &best_t, float2v &best_uv, int &best_ks, bool open = true) {
    const uint32_t f0 = G.f0, f1 = G.f1, f2 = G.f2;
    const float ldz = fmaf(G.z0, d.x, fmaf(G.z1, d.y, G.z2 * d.z));
    const float loz = fmaf(G.z0, o.x, fmaf(G.z1, o.y, fmaf(G.z2, o.z, G.z3)));
    const float2v lo = rows_at_point<BY_COMPONENT>(G.cx, G.cy, G.cz, G.cw, o);
    const float2v ld = rows_at_direction<BY_COMPONENT>(G.cx, G.cy, G.cz, d);
    const float ix = fast_rcp(ld.x), iy = fast_rcp(ld.y), iz = fast_rcp(ldz);
    // slab distances. (1 - lo) * inv, not t0 + inv: a ray parallel to a slab (inv = inf) must see (-inf, +inf) inside it and
    // two equal infinities outside
    const float ax = -lo.x * ix, bx = (1.f - lo.x) * ix, ay = -lo.y * iy, by = (1.f - lo.y) * iy, az = -loz * iz, bz = (1.f - loz) * iz;
    const float nx = fminf(ax, bx), fx = fmaxf(ax, bx), ny = fminf(ay, by), fy = fmaxf(ay, by), nz = fminf(az, bz), fz = fmaxf(az, bz);
    const float tnear = fmaxf(fmaxf(nx, ny), nz), tfar = fminf(fminf(fx, fy), fz);
    // One candidate per lane: the entry face if the ray comes from outside (entry distance >= tmin), the exit face otherwise. All
    // selects on values (a flag that lives across a branch costs a v_cndmask and a v_cmp at every merge).
    const bool through = tnear <= tfar && tfar >= tmin && tnear <= best_t;
    const bool inside = !(tnear >= tmin);
    BoxCand c = box_candidate<BY_COMPONENT>(inside, nx, ny, fx, fy, tnear, tfar, lo, ld, loz, ldz, f0, f1, f2);
    // the scene has no face where the ray enters (the open side of a room seen from outside): the face it leaves through. Rare, and
    // then for many lanes at once: behind a wave-uniform test.
    if (!OPEN_KNOWN || open) {
        // (OPEN_KNOWN: held_hole makes `hole` ONE compare, whose mask is the ballot; __ballot goes through a 0 / 1 integer and a second compare)
        const bool hole = OPEN_KNOWN ? held_hole(through && !inside, c.hc) : through && !inside && (c.hc & 1u) == 0u;
        if (OPEN_KNOWN ? __builtin_amdgcn_ballot_w64(hole) != 0ull : __ballot(hole) != 0ull) {
            const BoxCand c2 = box_candidate<BY_COMPONENT>(true, nx, ny, fx, fy, tnear, tfar, lo, ld, loz, ldz, f0, f1, f2);
            c.t = hole ? c2.t : c.t; c.p = hole ? c2.p : c.p; c.q = hole ? c2.q : c.q; c.hc = hole ? c2.hc : c.hc;
        }
    }
    const bool hit = through && (c.hc & 1u) != 0u && c.t >= tmin && c.t <= best_t;
    best_t = hit ? c.t : best_t;
    best_uv.x = hit ? c.p : best_uv.x;
    best_uv.y = hit ? c.q : best_uv.y;
    best_ks = hit ? (int) (c.hc | BOX_FACE_FLAG) : best_ks;
}

template <bool TRI> DEV Hit trace_flat(const DParams &P, f3 o, f3 d, float tmin, float tmax) {
    ScalarFlatPtr p = (ScalarFlatPtr) (uintptr_t) P.prims_flat;
    // VOLATILE scalar loads (three per record: 8 + 4 + 1 dwords): they stay where the pipeline below puts them. Left to its
    // scheduler the compiler sinks the read-ahead of a record to just before its first use and the wave then waits out a
    // scalar-cache access per record.
    auto load = [](ScalarFlatPtr q, FlatRec &G) {
#ifdef DRMLT_FLAT_PLAIN_LOADS
        G.cx = float2v{q->c[0], q->c[1]}; G.cy = float2v{q->c[2], q->c[3]}; G.cz = float2v{q->c[4], q->c[5]}; G.cw = float2v{q->c[6], q->c[7]};
        G.z0 = q->rz[0]; G.z1 = q->rz[1]; G.z2 = q->rz[2]; G.z3 = q->rz[3];
        G.ks = q->kind_shade;
#else
        typedef float f8v __attribute__((ext_vector_type(8)));
        typedef float f4v __attribute__((ext_vector_type(4)));
        const f8v c = *(const volatile f8v __attribute__((address_space(4))) *) &q->c[0];
        const f4v z = *(const volatile f4v __attribute__((address_space(4))) *) &q->rz[0];
        G.ks = *(const volatile int __attribute__((address_space(4))) *) &q->kind_shade;
        G.cx = float2v{c[0], c[1]}; G.cy = float2v{c[2], c[3]}; G.cz = float2v{c[4], c[5]}; G.cw = float2v{c[6], c[7]};
        G.z0 = z[0]; G.z1 = z[1]; G.z2 = z[2]; G.z3 = z[3];
#endif
    };
#define PINF(G) asm volatile("" ::"s"(G.cx.x), "s"(G.cz.x), "s"(G.z0), "s"(G.ks))
    float best_t = tmax;
    float2v best_uv = {0.f, 0.f};
    int best_ks = -1;
    // ---- cuboids first (record n_box is a sentinel: the read-ahead needs no clamp)
    if (P.n_box > 0) {
        auto loadb = [](ScalarBoxPtr q, BoxRec &G) {
            typedef float f8v __attribute__((ext_vector_type(8)));
            typedef float f4v __attribute__((ext_vector_type(4)));
            const f8v c = *(const volatile f8v __attribute__((address_space(4))) *) &q->c[0];
            const f4v z = *(const volatile f4v __attribute__((address_space(4))) *) &q->rz[0];
            // (three separate scalar loads: as elements of one loaded vector the per-lane choice among them in test_box became an
            // indexed load from a copy of the vector in scratch memory)
            typedef const volatile uint32_t __attribute__((address_space(4))) *SU;
            G.f0 = *(SU) &q->fw[0]; G.f1 = *(SU) &q->fw[1]; G.f2 = *(SU) &q->fw[2];
            G.cx = float2v{c[0], c[1]}; G.cy = float2v{c[2], c[3]}; G.cz = float2v{c[4], c[5]}; G.cw = float2v{c[6], c[7]};
            G.z0 = z[0]; G.z1 = z[1]; G.z2 = z[2]; G.z3 = z[3];
        };
        ScalarBoxPtr pb = (ScalarBoxPtr) (uintptr_t) P.prims_box;
        BoxRec A, B;
        loadb(pb, A);
        for (int i = 0; i < P.n_box; i += 2, pb += 2) {
            asm volatile("" ::"s"(A.cx.x), "s"(A.z0), "s"(A.f0));
            loadb(pb + 1, B);
            test_box(A, o, d, tmin, best_t, best_uv, best_ks);
            if (i + 1 < P.n_box) {
                asm volatile("" ::"s"(B.cx.x), "s"(B.z0), "s"(B.f0));
                loadb(pb + 2, A);
                test_box(B, o, d, tmin, best_t, best_uv, best_ks);
            }
        }
    }
    const int n = P.n_flat_rec;
    if (n > 0) {
        FlatRec A, B;
        load(p, A);
        for (int i = 0; i < n; i += 2, p += 2) { // records n and n + 1 are sentinels: the read-ahead needs no clamp
            PINF(A);
            load(p + 1, B);
            test_flat<TRI>(A, o, d, tmin, best_t, best_uv, best_ks);
            if (i + 1 < n) { // (with the cuboids most flat scenes keep one or two flat records -- the light: an odd count no longer pays for testing a sentinel)
                PINF(B);
                load(p + 2, A);
                test_flat<TRI>(B, o, d, tmin, best_t, best_uv, best_ks);
            }
        }
    }
#undef PINF
    Hit h{-1, best_t, best_uv.x, best_uv.y};
    if (best_ks >= 0) {
        if (best_ks & BOX_FACE_FLAG) { // a cuboid's face: its own (u, v) from the in-face coordinates, its own record
            const uint32_t hc = (uint32_t) best_ks & 0xffffu;
            const float uu = (hc & 2u) ? h.v : h.u, vv = (hc & 2u) ? h.u : h.v;
            h.u = (hc & 4u) ? 1.f - uu : uu;
            h.v = (hc & 8u) ? 1.f - vv : vv;
            best_ks = (int) (((hc >> 4) & 3u) | ((hc >> 6) << 8));
        }
        h.prim = best_ks >> 8;
        if ((best_ks & 0xff) == PRIM_QUAD2) { // sub-triangle (a,b,c) for v <= u, (a,c,d) otherwise; its own barycentrics
            const bool second = h.v > h.u;
            const float uu = second ? h.u : h.u - h.v, vv = second ? h.v - h.u : h.v;
            h.prim += second ? 1 : 0;
            h.u = uu; h.v = vv;
        }
    }
    return h;
}

// trace_flat with the scene's records held by the caller, in vector registers across its loop (k_mutate_w2h, kernels_v4.hip): up to
// three cuboids and one flat record, tested in the streaming loops' order by the same routines on the same values. No memory is
// read. What the scene is comes as ONE wave-uniform word of flags (held_flags: the host-side layout of the records never changes
// during a launch), each a scalar bit test here:
//   HELD_BOX1, HELD_BOX2, HELD_FLAT   the slot is used. Slot 0 always is: launch_plan.h's w2_held_launch asks for n_box >= 1.
//   HELD_OPEN0..2                     the cuboid lacks a face (test_box<true>: a closed one skips the `hole` test and its ballot)
//   HELD_QUAD2                        some record's kind is PRIM_QUAD2 -- the flat record's or a cuboid face's. Only then can a hit
//                                     need the sub-triangle arm of the tail; without the flag the arm is skipped by the wave.
// The tail is trace_flat's on the same values, as selects: no lane-dependent branch and no saved exec mask (with `if`s it cost
// three masks and two branches an iteration, and the PRIM_QUAD2 arm ran under an empty mask on scenes of rectangles).
struct HeldScene {
    BoxRec box[3];
    FlatRec flat;
};
enum { HELD_BOX1 = 1, HELD_BOX2 = 2, HELD_FLAT = 4, HELD_OPEN0 = 8, HELD_OPEN1 = 16, HELD_OPEN2 = 32, HELD_QUAD2 = 64 };
// (a face half-word: exists | code << 1 | kind << 4 | shade << 6)
DEV bool held_half_missing(uint32_t half) { return (half & 1u) == 0u; }
DEV bool held_half_quad2(uint32_t half) { return (half & 1u) != 0u && ((half >> 4) & 3u) == (uint32_t) PRIM_QUAD2; }
DEV uint32_t held_box_flags(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t open_bit) {
    bool open = false, quad2 = false;
    const uint32_t w[3] = {f0, f1, f2};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        open = open || held_half_missing(w[a] & 0xffffu) || held_half_missing(w[a] >> 16);
        quad2 = quad2 || held_half_quad2(w[a] & 0xffffu) || held_half_quad2(w[a] >> 16);
    }
    return (open ? open_bit : 0u) | (quad2 ? (uint32_t) HELD_QUAD2 : 0u);
}
// the word of flags of a held scene with n_box cuboids and n_flat flat records (slots beyond the counts hold zeros and set nothing)
DEV uint32_t held_flags(const HeldScene &S, uint32_t n_box, uint32_t n_flat) {
    uint32_t flags = (n_box > 1u ? (uint32_t) HELD_BOX1 : 0u) | (n_box > 2u ? (uint32_t) HELD_BOX2 : 0u) | (n_flat > 0u ? (uint32_t) HELD_FLAT : 0u);
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i)
        if (i < n_box) flags |= held_box_flags(S.box[i].f0, S.box[i].f1, S.box[i].f2, (uint32_t) HELD_OPEN0 << i);
    if (n_flat > 0u && (S.flat.ks & 0xff) == PRIM_QUAD2) flags |= (uint32_t) HELD_QUAD2;
    return flags;
}
DEV Hit trace_held(const HeldScene &S, uint32_t flags, f3 o, f3 d, float tmin, float tmax) {
    float best_t = tmax;
    float2v best_uv = {0.f, 0.f};
    int best_ks = -1;
    test_box<true, true>(S.box[0], o, d, tmin, best_t, best_uv, best_ks, (flags & HELD_OPEN0) != 0u);
    // (expected: the blocks stand in source order, each behind a guard that falls through when the slot is used)
    if (__builtin_expect((flags & HELD_BOX1) != 0u, 1)) test_box<true, true>(S.box[1], o, d, tmin, best_t, best_uv, best_ks, (flags & HELD_OPEN1) != 0u);
    if (__builtin_expect((flags & HELD_BOX2) != 0u, 1)) test_box<true, true>(S.box[2], o, d, tmin, best_t, best_uv, best_ks, (flags & HELD_OPEN2) != 0u);
    if (__builtin_expect((flags & HELD_FLAT) != 0u, 1)) test_flat_held(S.flat, o, d, tmin, best_t, best_uv, best_ks);
    Hit h{-1, best_t, best_uv.x, best_uv.y};
    const bool any = best_ks >= 0;
    const bool face = any && (best_ks & BOX_FACE_FLAG) != 0; // a cuboid's face: its own (u, v) from the in-face coordinates, its own record
    const uint32_t hc = (uint32_t) best_ks & 0xffffu;
    const float uu = (hc & 2u) ? h.v : h.u, vv = (hc & 2u) ? h.u : h.v;
    const float fu = (hc & 4u) ? 1.f - uu : uu, fv = (hc & 8u) ? 1.f - vv : vv;
    h.u = face ? fu : h.u;
    h.v = face ? fv : h.v;
    const int ks = face ? (int) (((hc >> 4) & 3u) | ((hc >> 6) << 8)) : best_ks;
    h.prim = any ? ks >> 8 : -1;
    if (flags & HELD_QUAD2) { // sub-triangle (a,b,c) for v <= u, (a,c,d) otherwise; its own barycentrics
        const bool quad2 = any && (ks & 0xff) == PRIM_QUAD2;
        const bool second = h.v > h.u;
        const float qu = second ? h.u : h.u - h.v, qv = second ? h.v - h.u : h.v;
        h.prim += (quad2 && second) ? 1 : 0;
        h.u = quad2 ? qu : h.u; h.v = quad2 ? qv : h.v;
    }
    return h;
}
// ... by the scene's counts, for a caller that holds no word of flags (the ray probe of the tests: one call, the flags made on the spot)
DEV Hit trace_held(const HeldScene &S, uint32_t n_box, uint32_t n_flat, f3 o, f3 d, float tmin, float tmax) {
    return trace_held(S, held_flags(S, n_box, n_flat), o, d, tmin, tmax);
}

template <int FEAT = 15> DEV Hit trace(const DParams &P, f3 o, f3 d, float tmin, float tmax, bool any_hit) {
    if ((FEAT & 8) && P.use_bvh) return trace_bvh(P, o, d, tmin, tmax, any_hit);
    if (P.prims_flat) {
        Hit h = P.has_plain_tri ? trace_flat<true>(P, o, d, tmin, tmax) : trace_flat<false>(P, o, d, tmin, tmax);
        if (FEAT & 4) // the spheres of the scene follow the flat records; same wave-uniform scalar loads, one at a time
            for (int i = P.n_flat; i < P.n_prims; ++i) { // (P.prims: every record of the scene, flat ones first -- n_flat of them, cuboid faces included)
                ScalarPrimPtr sp = (ScalarPrimPtr) (uintptr_t) P.prims;
                DPrim G;
#pragma unroll
                for (int k = 0; k < 12; ++k) G.m[k] = sp[i].m[k];
                const int ks = sp[i].kind_shade;
                G.type = PRIM_SPHERE; G.shade = ks >> 8;
                intersect_prim<4>(G, G.shade, o, d, tmin, h);
            }
        return h;
    }
    return trace_brute<FEAT>(P, o, d, tmin, tmax);
}

// ------------------------------------------------------------------ scene tables
// Shading / BSDF / emitter records are read per lane after a hit. Small scenes stage them in LDS
// once per launch (a dependent chain of 3-4 global gathers per step was ~1/3 of the wave's time
// at one wave per SIMD); large scenes read them from HBM/L2.
struct GlobalTables {
    const DShade *sh; const DBsdf *bs; const DEmitter *em;
    DEV DShade shade(int i) const { return load_global16(sh + i); }
    DEV DBsdf bsdf(int i) const { return load_global16(bs + i); }
    DEV DEmitter emitter(int i) const { return load_global16(em + i); }
    DEV float emitter_cdf_lo(int i) const { return load_global_f32(&em[i].cdf_lo); }
    DEV DShade emitter_shade(int, const DEmitter &E) const { return shade(E.prim); } // the shading record of emitter ei's shape
};
struct LdsTables {
    uint32_t shade_off, bsdf_off, emit_off; // float offsets into lds_x, multiples of 4
    // explicit field assignment from four 16 B LDS reads: going through a float* view of the struct
    // would park the record in scratch memory
    DEV DShade shade(int i) const {
        const float4 *q = reinterpret_cast<const float4 *>(&lds_x[shade_off + (uint32_t) i * 16u]);
        const float4 a = q[0], b = q[1], c = q[2], d = q[3];
        DShade s;
        s.origin[0] = a.x; s.origin[1] = a.y; s.origin[2] = a.z; s.eu[0] = a.w;
        s.eu[1] = b.x; s.eu[2] = b.y; s.ev[0] = b.z; s.ev[1] = b.w;
        s.ev[2] = c.x; s.n[0] = c.y; s.n[1] = c.z; s.n[2] = c.w;
        s.inv_len_eu = d.x; s.bsdf = __float_as_int(d.y); s.emitter = __float_as_int(d.z); s.inv_area = d.w;
        return s;
    }
    DEV DBsdf bsdf(int i) const {
        const float4 *q = reinterpret_cast<const float4 *>(&lds_x[bsdf_off + (uint32_t) i * 12u]);
        const float4 a = q[0], b = q[1], c = q[2];
        DBsdf r;
        r.type = __float_as_int(a.x); r.rgb[0] = a.y; r.rgb[1] = a.z; r.rgb[2] = a.w;
        r.p[0] = b.x; r.p[1] = b.y; r.p[2] = b.z; r.p[3] = b.w;
        r.p[4] = c.x; r.p[5] = c.y; r.p[6] = c.z; r.p[7] = c.w;
        return r;
    }
    DEV DEmitter emitter(int i) const {
        const float4 *q = reinterpret_cast<const float4 *>(&lds_x[emit_off + (uint32_t) i * 8u]);
        const float4 a = q[0], b = q[1];
        DEmitter e;
        e.radiance[0] = a.x; e.radiance[1] = a.y; e.radiance[2] = a.z; e.prim = __float_as_int(a.w);
        e.cdf_lo = b.x; e.cdf_hi = b.y; e.pad[0] = b.z; e.pad[1] = b.w;
        return e;
    }
    DEV float emitter_cdf_lo(int i) const { return lds_x[emit_off + (uint32_t) i * 8u + 4u]; }
    DEV DShade emitter_shade(int, const DEmitter &E) const { return shade(E.prim); }
    DEV int n_emitters(const DParams &P) const { return P.n_emitters; } // bound of path_step_diffuse's light pick
};
// LdsTables for a scene with one light (device_types.h: scene_has_one_light): every emitter index is 0, so the emitter's record and
// its shape's are the parameter block's joined copy -- wave-uniform scalars of the section's own block, loaded on the wait the
// section pays anyway -- and the light pick is an empty loop at compile time. The hit's shading record and the BSDFs stay in LDS.
struct OneLightTables {
    LdsTables L;
    const DParams &P;
    DEV DShade shade(int i) const { return L.shade(i); }
    DEV DBsdf bsdf(int i) const { return L.bsdf(i); }
    DEV DEmitter emitter(int) const { return P.light; }
    DEV float emitter_cdf_lo(int) const { return P.light.cdf_lo; }
    // (inv_area is pinned where the record is asked for: its only use sits in a conditional block, and the compiler would sink the
    // scalar load into it -- a wait of its own in the middle of the step instead of the one at the section's head)
    DEV DShade emitter_shade(int, const DEmitter &) const { DShade s = P.light_shade; asm volatile("" : "+s"(s.inv_area)); return s; }
    DEV constexpr int n_emitters(const DParams &) const { return 1; }
};
// OneLightTables with the light's two records held by the caller, in vector registers across its loop (k_mutate_w2, compiled for two
// waves per SIMD, has them to spare): no scalar load at the head of the step. The shape tag steers a wave-uniform branch of the
// step and goes back to a scalar register (one v_readfirstlane); everything else is a VALU operand.
// RECT (k_mutate_w2h): the light is a rectangle, known at compile time. Every scene that launch_plan.h's w2_held_launch accepts has one:
// the launch is a one-light launch, so the light's shape is tagged PRIM_RECTANGLE or PRIM_TRIANGLE (device_types.h:
// scene_has_one_light; a triangle with vertex normals is tagged PRIM_SMOOTH and is no such light). A triangle that emits is never
// merged into a pair (scene_prep.h asks emitter < 0 of both halves), a cuboid takes rectangles and pairs only (scene_prep.h clears
// `usable` for every other record before find_boxes), so the triangle stays a PRIM_TRIANGLE flat record,
// has_plain_tri is set and w2_held_launch says no. The step then has
// no triangle arm to compute and select away (path_step_diffuse: light_is_rectangle), and the tag goes to no scalar register.
template <bool RECT> struct HeldLightTablesT {
    static constexpr bool rectangle_light = RECT;
    LdsTables L;
    const DEmitter &E;
    const DShade &S;
    DEV DShade shade(int i) const { return L.shade(i); }
    DEV DBsdf bsdf(int i) const { return L.bsdf(i); }
    DEV DEmitter emitter(int) const { return E; }
    DEV float emitter_cdf_lo(int) const { return E.cdf_lo; }
    DEV DShade emitter_shade(int, const DEmitter &) const {
        DShade s = S;
        if constexpr (!RECT) s.bsdf = __builtin_amdgcn_readfirstlane(s.bsdf);
        return s;
    }
    DEV constexpr int n_emitters(const DParams &) const { return 1; }
};
typedef HeldLightTablesT<false> HeldLightTables;
template <class T, class = void> struct light_is_rectangle : std::false_type {};
template <class T> struct light_is_rectangle<T, std::void_t<decltype(T::rectangle_light)>> : std::integral_constant<bool, T::rectangle_light> {};
// BSDF and emitter records in LDS, shading records in device memory: for kernels whose own rows leave less LDS than the shading table
// needs (k_mutate_bdpt at two waves per SIMD: 19.25 KB of rows; the Cornell scene's 30 shading records are 1.9 KB, its four BSDFs and one
// emitter 224 bytes)
// `L.shade_off` holds one shading record per EMITTER (the record of its shape, in emitter order): what a light sample needs after the
// emitter is picked -- otherwise a dependent round trip to memory behind the pick.
struct MixedTables {
    const DShade *sh;
    LdsTables L;
    DEV DShade shade(int i) const { return load_global16(sh + i); }
    DEV DBsdf bsdf(int i) const { return L.bsdf(i); }
    DEV DEmitter emitter(int i) const { return L.emitter(i); }
    DEV float emitter_cdf_lo(int i) const { return L.emitter_cdf_lo(i); }
    DEV DShade emitter_shade(int ei, const DEmitter &) const { return L.shade(ei); }
};
// The same with a fallback: scenes whose BSDF / emitter tables do not fit beside a kernel's rows read them from device memory
// (wave-uniform `lds`). The BVH builds of k_mutate_v5: a path step's chain of dependent gathers -- shading record -> BSDF, light pick
// -> emitter -> its shape's record -- shrinks to the shading record alone.
struct HybridTables {
    const DShade *sh; const DBsdf *bs; const DEmitter *em;
    LdsTables L;
    bool lds;
    DEV DShade shade(int i) const { return load_global16(sh + i); }
    DEV DBsdf bsdf(int i) const { if (lds) return L.bsdf(i); return load_global16(bs + i); }
    DEV DEmitter emitter(int i) const { if (lds) return L.emitter(i); return load_global16(em + i); }
    DEV float emitter_cdf_lo(int i) const { if (lds) return L.emitter_cdf_lo(i); return load_global_f32(&em[i].cdf_lo); }
    DEV DShade emitter_shade(int ei, const DEmitter &E) const { if (lds) return L.shade(ei); return load_global16(sh + E.prim); }
};
DEV uint32_t small_tables_floats(const DParams &P) { return (uint32_t) P.n_emitters * 16u + (uint32_t) P.n_bsdfs * 12u + (uint32_t) P.n_emitters * 8u; }
// emitter shape records at T.shade_off, BSDFs at T.bsdf_off, emitters at T.emit_off
DEV void stage_bsdfs_emitters(const DParams &P, const LdsTables &T, uint32_t lane) {
    const float *src = reinterpret_cast<const float *>(P.bsdfs);
    for (uint32_t i = lane; i < (uint32_t) P.n_bsdfs * 12u; i += 64u) lds_x[T.bsdf_off + i] = src[i];
    src = reinterpret_cast<const float *>(P.emitters);
    for (uint32_t i = lane; i < (uint32_t) P.n_emitters * 8u; i += 64u) lds_x[T.emit_off + i] = src[i];
    for (uint32_t i = lane; i < (uint32_t) P.n_emitters * 16u; i += 64u) {
        const int prim = P.emitters[i >> 4].prim;
        lds_x[T.shade_off + i] = reinterpret_cast<const float *>(P.shade + prim)[i & 15u];
    }
}
// cooperative copy of the three tables into LDS by one wave
DEV void stage_tables(const DParams &P, const LdsTables &T, uint32_t lane) {
    const float *src = reinterpret_cast<const float *>(P.shade);
    for (uint32_t i = lane; i < (uint32_t) P.n_shade * 16u; i += 64u) lds_x[T.shade_off + i] = src[i];
    src = reinterpret_cast<const float *>(P.bsdfs);
    for (uint32_t i = lane; i < (uint32_t) P.n_bsdfs * 12u; i += 64u) lds_x[T.bsdf_off + i] = src[i];
    src = reinterpret_cast<const float *>(P.emitters);
    for (uint32_t i = lane; i < (uint32_t) P.n_emitters * 8u; i += 64u) lds_x[T.emit_off + i] = src[i];
}

// ------------------------------------------------------------------ estimator state machine
// MIPathTracer::Li + the sampleSplats prologue as a resumable machine. One call of path_step
// consumes the result of the ray query issued by the previous call and issues the next one.
// All PSS components a step needs are drawn at ONE site (the `next` loop below): the sampler
// code (Philox + transition kernels) is the bulk of the instruction footprint, so it is
// instantiated once per kernel instead of once per consumer.
enum { PH_DONE = 0, PH_BEGIN = 1, PH_CLOSEST = 2, PH_SHADOW = 3, PH_IDLE = 4, PH_FLUSH = 5 };

struct PathState {
    f3 o, d;          // ray to trace next (o doubles as the current surface point)
    float tmin, tmax;
    f3 thr, Li;
    f3 n, s, wi;      // shading frame (t = n x s) and local incident direction at the current vertex
    f3 nee;           // NEE contribution pending on the shadow ray
    f3 bweight;       // BSDF sample weight pending on the bounce ray
    float bpdf, beta_eta, eta;
    float bx, by;     // BSDF sample components, drawn together with the NEE ones
    float px, py;     // film position of this sample
    int phase, depth, bsdf;
    uint32_t k;       // next PSS dimension
    uint32_t nrays;
    bool non_specular, direct_on, has_bounce, bdelta, refn_zero;
    bool shadow_pending; // dual-lane mode: ps.nee waits for the partner lane's occlusion result
};

// shadow ray handed to the partner lane (dual-lane mode)
struct ShadowRay {
    f3 o, d;
    float tmin, tmax;
    bool valid;
};

DEV float ray_eps_closest(f3 o) { // skdtree.cpp:125-129
    return EPSILON_F * fmaxf(fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)), EPSILON_F);
}
DEV float ray_eps_shadow(f3 o) { // skdtree.cpp:213-218
    return EPSILON_F * fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z));
}

// Sphere as an area light seen from `ref` (sphere.cpp:286-385): uniform sampling of the cone it subtends when the
// reference point is outside, uniform area sampling otherwise. Outputs direction, distance, surface normal, solid-angle pdf.
DEV void sphere_sample_direct(f3 c, float radius, float inv_area, f3 ref, float sx, float sy, f3 &d, float &dist, f3 &n, float &pdf) {
    const f3 rc = c - ref;
    const float refDist2 = dot3(rc, rc);
    const float invRefDist = rsqrtf(refDist2);
    const float sinAlpha = radius * invRefDist;
    if (sinAlpha < 1.f - EPSILON_F) {
        const float cosAlpha = sqrtf(fmaxf(0.f, 1.f - sinAlpha * sinAlpha));
        const float cosTheta = (1.f - sx) + sx * cosAlpha, sinTheta = sqrtf(fmaxf(0.f, 1.f - cosTheta * cosTheta));
        const f3 fn = rc * invRefDist;
        f3 fs, ft; // Frame(n): coordinateSystem (util.cpp:606-616)
        if (fabsf(fn.x) > fabsf(fn.y)) { float inv = rsqrtf(fn.x * fn.x + fn.z * fn.z); ft = mk3(fn.z * inv, 0.f, -fn.x * inv); }
        else { float inv = rsqrtf(fn.y * fn.y + fn.z * fn.z); ft = mk3(0.f, fn.z * inv, -fn.y * inv); }
        fs = cross3(ft, fn);
        d = fma3(fs, cos_rev(sy) * sinTheta, fma3(ft, sin_rev(sy) * sinTheta, fn * cosTheta));
        pdf = 0.15915494309189535f / (1.f - cosAlpha);
        const float projDist = dot3(rc, d);
        const float baseT = refDist2 / projDist;
        const f3 qc = c - fma3(d, baseT, ref);
        const float queryDist2 = dot3(qc, qc), queryProjDist = dot3(qc, d);
        // solveQuadratic(1, -2 queryProjDist, queryDist2 - r^2), util.cpp:447-485
        const float B = -2.f * queryProjDist, C = queryDist2 - radius * radius;
        const float discrim = B * B - 4.f * C;
        float nearT = queryProjDist;
        if (discrim >= 0.f) {
            const float sq = sqrtf(discrim);
            const float temp = B < 0.f ? -0.5f * (B - sq) : -0.5f * (B + sq);
            nearT = fminf(temp, C / temp);
        }
        dist = baseT + nearT;
        n = normalize3(d * nearT - qc);
    } else {
        const float z = 1.f - 2.f * sy, r = sqrtf(fmaxf(0.f, 1.f - z * z));
        n = mk3(r * cos_rev(sx), r * sin_rev(sx), z);
        const f3 dv = fma3(n, radius, c) - ref;
        const float dist2 = dot3(dv, dv);
        dist = sqrtf(dist2);
        d = dv * (1.f / dist);
        pdf = inv_area * dist2 / fabsf(dot3(d, n));
    }
}
DEV float sphere_pdf_direct(f3 c, float radius, float inv_area, f3 ref, float dist, float cos_light) { // sphere.cpp:357-385
    const f3 rc = c - ref;
    const float sinAlpha = radius * rsqrtf(dot3(rc, rc));
    if (sinAlpha < 1.f - EPSILON_F) return 0.15915494309189535f / (1.f - sqrtf(fmaxf(0.f, 1.f - sinAlpha * sinAlpha)));
    return inv_area * dist * dist / cos_light;
}

// warp.cpp:81-102 + :43-52 (angles expressed in revolutions for v_sin/v_cos)
DEV f3 square_to_cosine_hemisphere(float sx, float sy) {
    float r1 = 2.f * sx - 1.f, r2 = 2.f * sy - 1.f;
    // selects instead of the three-way branch: num / den = r2 / r1 or r1 / r2, whichever has the larger denominator
    const bool first = r1 * r1 > r2 * r2;
    const float num = first ? r2 : r1, den = first ? r1 : r2;
    const float q = den != 0.f ? 0.125f * (num / den) : 0.f; // den == 0 only for r1 == r2 == 0: r = 0, angle irrelevant
    const float r = den, rev = first ? q : 0.25f - q;
    float px = r * cos_rev(rev), py = r * sin_rev(rev);
    float z = sqrtf(fmaxf(0.f, 1.f - px * px - py * py));
    if (z == 0.f) z = 1e-10f;
    return mk3(px, py, z);
}

// Constant environment seen from `ref` (ConstantBackgroundEmitter::sampleDirect, constant.cpp:173-214; refN = the shading normal
// `n`): a cosine-weighted direction in Frame(n) (coordinateSystem, util.cpp:606-616), its solid-angle pdf cos / pi, and the
// distance to the far side of the scene's bounding sphere (BSphere::rayIntersect + solveQuadratic, util.cpp:447-485). pdf = 0
// (the sample is dropped) unless `ref` lies inside the sphere. The refN = 0 case (uniform sphere) has no caller: only the
// dielectric zeroes refN, and it draws no light sample.
DEV void env_sample_direct(f3 c, float radius, f3 ref, f3 n, float sx, float sy, f3 &d, float &dist, float &pdf) {
    const f3 w = square_to_cosine_hemisphere(sx, sy);
    f3 fs, ft;
    if (fabsf(n.x) > fabsf(n.y)) { float inv = rsqrtf(n.x * n.x + n.z * n.z); ft = mk3(n.z * inv, 0.f, -n.x * inv); }
    else { float inv = rsqrtf(n.y * n.y + n.z * n.z); ft = mk3(0.f, n.z * inv, -n.y * inv); }
    fs = cross3(ft, n);
    d = fma3(fs, w.x, fma3(ft, w.y, n * w.z));
    pdf = INV_PI_F * w.z;
    const f3 o = ref - c;
    const float A = dot3(d, d), B = 2.f * dot3(o, d), C = dot3(o, o) - radius * radius;
    const float discrim = B * B - 4.f * A * C;
    const float sq = sqrtf(fmaxf(discrim, 0.f));
    const float temp = B < 0.f ? -0.5f * (B - sq) : -0.5f * (B + sq);
    const float x0 = temp / A, x1 = C / temp;
    const float nearT = fminf(x0, x1), farT = fmaxf(x0, x1);
    dist = farT;
    if (!(discrim >= 0.f && nearT < 0.f && farT > 0.f)) pdf = 0.f;
}

// util.cpp:659-689
DEV float fresnel_dielectric_ext(float cosThetaI_, float &cosThetaT_, float eta) {
    if (eta == 1.f) { cosThetaT_ = -cosThetaI_; return 0.f; }
    float scale = (cosThetaI_ > 0.f) ? 1.f / eta : eta;
    float cosThetaTSqr = 1.f - (1.f - cosThetaI_ * cosThetaI_) * (scale * scale);
    if (cosThetaTSqr <= 0.f) { cosThetaT_ = 0.f; return 1.f; }
    float cosThetaI = fabsf(cosThetaI_), cosThetaT = sqrtf(cosThetaTSqr);
    float Rs = (cosThetaI - eta * cosThetaT) / (cosThetaI + eta * cosThetaT);
    float Rp = (eta * cosThetaI - cosThetaT) / (eta * cosThetaI + cosThetaT);
    cosThetaT_ = (cosThetaI_ > 0.f) ? -cosThetaT : cosThetaT;
    return 0.5f * (Rs * Rs + Rp * Rp);
}

DEV void path_init(const DParams &P, PathState &ps) {
    ps.phase = PH_BEGIN;
    ps.k = 0u;
    ps.nrays = 0u;
    ps.thr = mk3(1.f, 1.f, 1.f);
    ps.Li = mk3(0.f, 0.f, 0.f);
    ps.eta = 1.f;
    ps.depth = 1;
    ps.non_specular = false;
    ps.direct_on = P.exclude_direct == 0; // pathsampler.cpp:558-561
    ps.has_bounce = false;
    ps.refn_zero = false;
    ps.shadow_pending = false;
    ps.px = ps.py = 0.f;
}

// First step of every path: film position from the first two PSS components (pathsampler.cpp:538-543) and the
// camera ray (sampleRayDifferential, perspective.cpp:271-286). Leaves the path in PH_CLOSEST.
DEV void path_begin(const DParams &P, PathState &ps, float v0, float v1) {
    ps.k = 2u;
    ps.px = v0 * (float) P.width;
    ps.py = v1 * (float) P.height;
    f3 nearP = mk3((1.f - 2.f * v0) * P.tan_half_fov * P.near_clip, (1.f - 2.f * v1) * P.tan_half_fov * P.inv_aspect * P.near_clip,
                   P.near_clip);
    f3 dl = normalize3(nearP);
    float invZ = 1.f / dl.z;
    ps.tmin = P.near_clip * invZ;
    ps.tmax = P.far_clip * invZ;
    ps.o = mk3(P.cam[3], P.cam[7], P.cam[11]);
    ps.d = mk3(fmaf(P.cam[0], dl.x, fmaf(P.cam[1], dl.y, P.cam[2] * dl.z)), fmaf(P.cam[4], dl.x, fmaf(P.cam[5], dl.y, P.cam[6] * dl.z)),
               fmaf(P.cam[8], dl.x, fmaf(P.cam[9], dl.y, P.cam[10] * dl.z)));
    ps.phase = PH_CLOSEST;
    ps.nrays = 1u;
}

// Consume the result of the ray query issued for `ps` (none in PH_BEGIN) and either issue the
// next ray (PH_CLOSEST / PH_SHADOW) or finish the path (PH_DONE, radiance in ps.Li).
// DUAL = false: one lane per chain, shadow rays take a step of their own (PH_SHADOW).
// DUAL = true : two lanes per chain. This lane traces the camera/bounce rays, its partner traces
//   the shadow ray of the SAME vertex concurrently; `shadow_clear` is the partner's result for the
//   ray handed over in the previous step (`sr`), so a bounce costs one step instead of two. The
//   order of the radiance additions is the same in both modes (NEE of vertex i, then MIS of i+1).
// FEAT: scene features compiled in (bit 0 rough conductor, bit 1 delta BSDFs: dielectric, smooth conductor, bit 2 what is not a polygon: spheres, point
// lights and the environment, bit 3 BVH); kernels for
// plain diffuse polygon scenes (the Cornell configs) carry none of the other code or its registers.
// HAS_BEGIN = false: the caller starts every path with path_begin itself (k_mutate_v4: in its bookkeeping branch), the
// step never sees PH_BEGIN and carries none of its code.
// SinkT: told about every term the step adds to ps.Li, by the complete path's edge count d (camera to emitter) and its strategy.
// ps.depth counts the surface vertices reached so far, and at each of the three places that add to Li it is the index of the LAST
// surface vertex of the path: the light sample is taken there (parked, then added in PH_SHADOW with the depth unchanged), and the
// emitter hit or the escape to the environment is seen before `ps.depth++` counts the hit. So d = ps.depth + 1 at all three.
//   hit(d, term, weight)     the emitter found by the BSDF-sampled ray (area light or environment): Li += term * weight
//   park(d, term, weight)    a light sample waits for its shadow ray: ps.nee = term * weight (weight 1 for a point light)
//   shadow(d, clear)         that ray came back; clear: Li += ps.nee
//   voided()                 the sample is invalid, Li = 0 and nothing is added after it
// The default does nothing and costs nothing (every use is under `if constexpr (SinkT::enabled)`); k_render_pt_layers has the one
// that does (kernels_layers_pt.hip). The dual-lane additions and path_step_diffuse have no sink.
struct PathNoSink {
    static constexpr bool enabled = false;
    DEV void hit(int, f3, float) const {}
    DEV void park(int, f3, float) const {}
    DEV void shadow(int, bool) const {}
    DEV void voided() const {}
};

template <bool DUAL, int FEAT, class SamplerT, class TablesT, bool HAS_BEGIN = true, class SinkT = PathNoSink>
DEV void path_step(const DParams &P, const TablesT &T, PathState &ps, SamplerT &smp, const Hit &hit, bool shadow_clear,
                   ShadowRay &sr, SinkT sink = SinkT()) {
    static_assert(!SinkT::enabled || !DUAL, "the dual-lane additions have no sink");
    // (row samplers: the five components a step can draw are requested HERE, all together and ahead of the shading record's gather -- one
    // round trip beside it instead of `need` of them behind it; what the step does not draw is not used)
    float pre0 = 0.f, pre1 = 0.f, pre2 = 0.f, pre3 = 0.f, pre4 = 0.f;
    if constexpr (draws_batched<SamplerT>::value) {
        const uint32_t kmax = (uint32_t) P.eff_dim - 1u, k = ps.k;
        pre0 = smp.next(min(k, kmax)); pre1 = smp.next(min(k + 1u, kmax)); pre2 = smp.next(min(k + 2u, kmax));
        pre3 = smp.next(min(k + 3u, kmax)); pre4 = smp.next(min(k + 4u, kmax));
    }
    // ---------------- part 1: digest the ray query, decide which PSS components are needed
    bool want_rr = false, want_nee = false;
    int need = 0;
    float rr_q = 1.f;
    f3 p = ps.o, n = ps.n, s = ps.s;
    DBsdf B;
    if (DUAL) {
        sr.valid = false;
        if (ps.shadow_pending) {
            if (shadow_clear) ps.Li = ps.Li + ps.nee;
            ps.shadow_pending = false;
        }
        if (ps.phase == PH_FLUSH) { ps.phase = PH_DONE; return; }
    }
    if (HAS_BEGIN && ps.phase == PH_BEGIN) {
        need = 2; // film position, pathsampler.cpp:538-543
    } else if (!DUAL && ps.phase == PH_SHADOW) {
        if (hit.prim < 0) ps.Li = ps.Li + ps.nee; // unoccluded
        if constexpr (SinkT::enabled) sink.shadow(ps.depth + 1, hit.prim < 0);
        B = T.bsdf(ps.bsdf);
    } else {
        if (hit.prim < 0) { // the ray left the scene
            if ((FEAT & 4) && P.env_emitter >= 0 && ps.has_bounce) { // environment seen by a BSDF-sampled ray (path.cpp:253-262, 275-285)
                ps.thr = ps.thr * ps.bweight;
                // the emitter-hit branch's gates: directTracing = false, so a camera ray that misses (has_bounce) or an escape after
                // delta vertices only (non_specular) adds nothing
                if (ps.direct_on && ps.non_specular) {
                    const DEmitter E = T.emitter(P.env_emitter);
                    // pdfEmitterDirect with the previous vertex's refN (ps.n; only the dielectric zeroes it, and it is delta: lumPdf = 0)
                    const float lumPdf = ps.bdelta ? 0.f : INV_PI_F * fmaxf(0.f, dot3(ps.d, ps.n)) * (E.cdf_hi - E.cdf_lo);
                    float a = ps.bpdf * ps.bpdf, b = lumPdf * lumPdf;
                    ps.Li = fma3(ps.thr * ld3(E.radiance), a / (a + b), ps.Li);
                    if constexpr (SinkT::enabled) sink.hit(ps.depth + 1, ps.thr * ld3(E.radiance), a / (a + b));
                }
            }
            ps.phase = PH_DONE;
            return;
        }
        const DShade S = T.shade(hit.prim);
        const int ptype = S.bsdf >> 24; // primitive kind rides in the top byte
        // surface point + shading frame (skdtree.h:340-429, rectangle.cpp:155-168, sphere.cpp:207-255)
        if (!(FEAT & 4) || ptype != PRIM_SPHERE) {
            p = fma3(ld3(S.eu), hit.u, fma3(ld3(S.ev), hit.v, ld3(S.origin)));
            n = ld3(S.n);
            s = ld3(S.eu) * S.inv_len_eu;
            // vertex normals: the interpolated normal and computeShadingFrame's tangent replace both (skdtree.h:355-396,426); a normal
            // without a direction makes the sample invalid (f = 0)
            // (a normal without a direction comes back as n = s = 0 and ends the path below, where the BSDF is read: an exit of its own
            // here cost every build with bit 4 some ten registers)
            if ((FEAT & 4) && __builtin_expect(ptype == PRIM_SMOOTH, 0)) smooth_record_frame(P, hit.u, hit.v, n, s);
        } else {
            f3 c = ld3(S.origin);
            f3 local = normalize3(fma3(ps.d, hit.t, ps.o) - c);
            p = fma3(local, S.eu[0], c);
            n = local;
            float zrad2 = local.x * local.x + local.y * local.y;
            float inv = rsqrtf(zrad2);
            s = zrad2 > 0.f ? mk3(-local.y * inv, local.x * inv, 0.f) : mk3(1.f, 0.f, 0.f);
        }
        if (ps.has_bounce) {
            ps.thr = ps.thr * ps.bweight;
            ps.eta *= ps.beta_eta;
            // emitter hit by the BSDF-sampled ray: MIS against direct sampling (path.cpp:269-285)
            if (S.emitter >= 0 && ps.direct_on && ps.non_specular) {
                const DEmitter E = T.emitter(S.emitter);
                float dn = dot3(ps.d, n);
                if (dn < 0.f) { // AreaLight::eval: dot(n, -d) > 0
                    float lumPdf = 0.f;
                    if (!ps.bdelta) { // pdfEmitterDirect: refN belongs to the PREVIOUS vertex (ps.n) or is 0
                        float dr = ps.refn_zero ? 0.f : dot3(ps.d, ps.n);
                        if (dr >= 0.f) {
                            lumPdf = S.inv_area * hit.t * hit.t / fabsf(dn);
                            if ((FEAT & 4) && ptype == PRIM_SPHERE) lumPdf = sphere_pdf_direct(ld3(S.origin), S.eu[0], S.inv_area, ps.o, hit.t, fabsf(dn));
                            lumPdf *= E.cdf_hi - E.cdf_lo;
                        }
                    }
                    float a = ps.bpdf * ps.bpdf, b = lumPdf * lumPdf;
                    ps.Li = fma3(ps.thr * ld3(E.radiance), a / (a + b), ps.Li);
                    if constexpr (SinkT::enabled) sink.hit(ps.depth + 1, ps.thr * ld3(E.radiance), a / (a + b)); // (before ps.depth++ below)
                }
            }
            ps.direct_on = true;                   // rRec.type = ERadianceNoEmission
            want_rr = ps.depth++ >= P.rr_depth;    // russian roulette, path.cpp:297-307
        }
        // `depth >= maxDepth` ends the path whatever the roulette draw says, so test it first
        if (ps.depth >= P.max_depth && P.max_depth > 0) {
            if (want_rr) ps.k++;
            ps.phase = PH_DONE;
            return;
        }
        if (want_rr) rr_q = fminf(max3(ps.thr) * ps.eta * ps.eta, 0.95f);
        // adopt the new vertex
        f3 t = cross3(n, s);
        f3 md = -ps.d;
        ps.wi = mk3(dot3(md, s), dot3(md, t), dot3(md, n));
        ps.o = p; ps.n = n; ps.s = s;
        ps.bsdf = S.bsdf & 0xffffff;
        B = T.bsdf(ps.bsdf);
        // a smooth triangle whose interpolated normal has no direction: the sample is invalid (f = 0). wi = 0, no light sample passes
        // its wo.z > 0, and as a diffuse vertex the path ends at that branch's wi.z > 0 -- the exits the step already has
        if ((FEAT & 4) && is_zero3(n)) {
            B.type = 0;
            ps.Li = mk3(0.f, 0.f, 0.f);
            if constexpr (SinkT::enabled) sink.voided();
        }
        ps.refn_zero = (FEAT & 2) && B.type == 1; // transmissive / two-sided: DirectSamplingRecord(its) zeroes refN
        // no light sample at a delta vertex, dielectric or smooth conductor (path.cpp:187, the ESmooth gate)
        want_nee = ps.direct_on && (B.type == 0 || ((FEAT & 1) && B.type == 2));
        need = (want_rr ? 1 : 0) + (want_nee ? 2 : 0) + 2;
    }

    // ---------------- part 2: the one place PSS components are drawn
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
    if constexpr (draws_batched<SamplerT>::value) {
        v0 = pre0; v1 = pre1; v2 = pre2; v3 = pre3; v4 = pre4;
    } else {
#pragma nounroll
        for (int j = 0; j < need; ++j) {
            float v = smp.next(ps.k + (uint32_t) j);
            if (j == 0) v0 = v; else if (j == 1) v1 = v; else if (j == 2) v2 = v; else if (j == 3) v3 = v; else v4 = v;
        }
    }

    // ---------------- part 3: use them
    if (HAS_BEGIN && ps.phase == PH_BEGIN) {
        path_begin(P, ps, v0, v1);
        return;
    }
    if (ps.phase == PH_CLOSEST) {
        if (want_rr) {
            ps.k++;
            if (v0 >= rr_q) { ps.phase = PH_DONE; return; }
            ps.thr = ps.thr * (1.f / rr_q);
        }
        float sx = want_rr ? v1 : v0, sy = want_rr ? v2 : v1;
        const int bpos = (want_rr ? 1 : 0) + (want_nee ? 2 : 0);
        ps.bx = bpos == 0 ? v0 : (bpos == 1 ? v1 : (bpos == 2 ? v2 : v3));
        ps.by = bpos == 0 ? v1 : (bpos == 1 ? v2 : (bpos == 2 ? v3 : v4));
        // direct illumination sampling (path.cpp:187-218, scene.cpp:879-904)
        if (want_nee) {
            ps.k += 2u;
            f3 t = cross3(n, s);
            int ei = 0; // DiscreteDistribution::sample (lower_bound semantics)
            for (int i = 1; i < P.n_emitters; ++i)
                if (T.emitter_cdf_lo(i) < sx) ei = i;
            const DEmitter E = T.emitter(ei);
            float emPdf = E.cdf_hi - E.cdf_lo;
            sx = (sx - E.cdf_lo) / emPdf; // sampleReuse
            const DShade L = T.emitter_shade(ei, E);
            f3 lp;
            if ((L.bsdf >> 24) == PRIM_RECTANGLE) { // rectangle.cpp:210-216
                lp = fma3(ld3(L.eu), sx, fma3(ld3(L.ev), sy, ld3(L.origin))); // origin = corner (-1,-1), eu/ev = full edges
            } else if ((FEAT & 4) && (L.bsdf >> 24) == PRIM_POINT) { // point light: the sample is drawn, not read (point.cpp:131-151)
                lp = ld3(L.origin);
            } else { // single triangle: squareToUniformTriangle
                float a = sqrtf(fmaxf(0.f, 1.f - sx));
                lp = fma3(ld3(L.eu), 1.f - a, fma3(ld3(L.ev), a * sy, ld3(L.origin)));
            }
            f3 ln = ld3(L.n);
            if ((FEAT & 4) && __builtin_expect((L.bsdf >> 24) == PRIM_SMOOTH, 0)) { // Triangle::sample returns the interpolated normal (triangle.cpp:34-42); zero: pdf = 0 below
                const float a = sqrtf(fmaxf(0.f, 1.f - sx)); // the sample's barycentrics (1 - a, a sy), formed again: sx and sy live on anyway
                smooth_record_normal(P, 1.f - a, a * sy, ln);
            }
            f3 dv = lp - p;
            float dist2 = dot3(dv, dv), dist = sqrtf(dist2);
            f3 dd = dv * (1.f / dist);
            float dln = dot3(dd, ln);
            float pdf = dln != 0.f ? L.inv_area * dist2 / fabsf(dln) : 0.f; // Shape::sampleDirect
            if ((FEAT & 4) && (L.bsdf >> 24) == PRIM_SPHERE) // sphere light: cone sampling, sphere.cpp:286-355
                sphere_sample_direct(ld3(L.origin), L.eu[0], L.inv_area, p, sx, sy, dd, dist, ln, pdf), dln = dot3(dd, ln);
            // environment: cosine-weighted about n, pdf cos / pi in solid angle, no facing test; MIS (power heuristic) against the BSDF
            // as for area lights (path.cpp:203-211: the emitter is on a surface, the measure is solid angle)
            if ((FEAT & 4) && (L.bsdf >> 24) == PRIM_ENV)
                env_sample_direct(ld3(L.origin), L.eu[0], p, n, sx, sy, dd, dist, pdf), dln = -1.f;
            // point light: pdf 1 (discrete), value I / dist^2, no facing test (n = 0); with the pick, value = I / (dist^2 emPdf) and
            // the MIS weight is 1 (path.cpp:190-218: bsdfPdf = 0 for an emitter that is not on a surface)
            const bool point = (FEAT & 4) && (L.bsdf >> 24) == PRIM_POINT;
            if (point) pdf = dist2, dln = -1.f;
            float dr = ps.refn_zero ? 0.f : dot3(dd, n);
            if (dr >= 0.f && dln < 0.f && pdf != 0.f) { // AreaLight::sampleDirect
                f3 wo = mk3(dot3(dd, s), dot3(dd, t), dot3(dd, n));
                if (ps.wi.z > 0.f && wo.z > 0.f) {
                    f3 bsdfVal;
                    float bsdfPdf;
                    if (!(FEAT & 1) || B.type == 0) { // diffuse eval / pdf (diffuse.cpp:110-127)
                        bsdfVal = ld3(B.rgb) * (INV_PI_F * wo.z);
                        bsdfPdf = INV_PI_F * wo.z;
                    } else { // rough conductor (roughconductor.cpp:258-323)
                        const DRoughConductor rc{DMicrofacet{B.p[7] != 0.f, fmaxf(B.p[0], 1e-4f)}, mk3(B.p[1], B.p[2], B.p[3]),
                                                 mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
                        bsdfVal = rc.eval(ps.wi, wo);
                        bsdfPdf = rc.pdf(ps.wi, wo);
                    }
                    float lpdf = pdf * emPdf;
                    float a = lpdf * lpdf, b = bsdfPdf * bsdfPdf;
                    f3 value = ld3(E.radiance) * (1.f / lpdf);
                    f3 c = ps.thr * value * bsdfVal * (point ? 1.f : a / (a + b));
                    if (!is_zero3(c)) {
                        ps.nee = c;
                        if constexpr (SinkT::enabled) sink.park(ps.depth + 1, ps.thr * value * bsdfVal, point ? 1.f : a / (a + b));
                        ps.nrays++;
                        if (DUAL) { // partner lane traces it while this lane traces the bounce ray
                            sr.o = p; sr.d = dd;
                            sr.tmin = ray_eps_shadow(p);
                            sr.tmax = dist * (1.f - SHADOW_EPSILON_F);
                            sr.valid = true;
                            ps.shadow_pending = true;
                        } else {
                            ps.d = dd;
                            ps.tmin = ray_eps_shadow(p);
                            ps.tmax = dist * (1.f - SHADOW_EPSILON_F);
                            ps.phase = PH_SHADOW;
                            return;
                        }
                    }
                }
            }
        }
    }
    // ---------------- BSDF sampling (path.cpp:224-245), reached from PH_CLOSEST and PH_SHADOW
    ps.k += 2u;
    f3 wo;
    if (B.type == 0) { // diffuse.cpp:139-149
        if (!(ps.wi.z > 0.f)) { ps.phase = (DUAL && ps.shadow_pending) ? PH_FLUSH : PH_DONE; return; }
        wo = square_to_cosine_hemisphere(ps.bx, ps.by);
        ps.bpdf = INV_PI_F * wo.z;
        ps.bweight = ld3(B.rgb);
        ps.beta_eta = 1.f;
        ps.bdelta = false;
    } else if ((FEAT & 2) && B.type == 1) { // dielectric.cpp:270-306
        float eta = B.p[0], invEta = B.p[1];
        float cosThetaT;
        float F = fresnel_dielectric_ext(ps.wi.z, cosThetaT, eta);
        ps.bdelta = true;
        if (ps.bx <= F) {
            wo = mk3(-ps.wi.x, -ps.wi.y, ps.wi.z);
            ps.bpdf = F;
            ps.bweight = mk3(1.f, 1.f, 1.f);
            ps.beta_eta = 1.f;
        } else {
            float scale = -(cosThetaT < 0.f ? invEta : eta);
            wo = mk3(scale * ps.wi.x, scale * ps.wi.y, cosThetaT);
            ps.beta_eta = cosThetaT < 0.f ? eta : invEta;
            ps.bpdf = 1.f - F;
            float factor = cosThetaT < 0.f ? invEta : eta;
            ps.bweight = mk3(factor * factor, factor * factor, factor * factor);
        }
    } else if ((FEAT & 1) && B.type == 2) { // roughconductor.cpp:371-409
        const DRoughConductor rc{DMicrofacet{B.p[7] != 0.f, fmaxf(B.p[0], 1e-4f)}, mk3(B.p[1], B.p[2], B.p[3]),
                                 mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
        ps.bpdf = 0.f;
        ps.bweight = rc.sample(ps.wi, ps.bx, ps.by, wo, ps.bpdf);
        ps.beta_eta = 1.f;
        ps.bdelta = false;
    } else if ((FEAT & 2) && B.type == 3) { // conductor.cpp:254-290; eta and k from the record the step already holds
        const DConductor mc{mk3(B.p[1], B.p[2], B.p[3]), mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
        ps.bweight = mc.sample(ps.wi, wo); // zero from below the surface: the path ends at the test that follows
        ps.bpdf = 1.f;
        ps.beta_eta = 1.f;
        ps.bdelta = true;
    } else {
        ps.phase = (DUAL && ps.shadow_pending) ? PH_FLUSH : PH_DONE;
        return;
    }
    if (is_zero3(ps.bweight)) { ps.phase = (DUAL && ps.shadow_pending) ? PH_FLUSH : PH_DONE; return; }
    ps.non_specular = ps.non_specular || !ps.bdelta;
    f3 t = cross3(ps.n, ps.s);
    ps.d = fma3(ps.s, wo.x, fma3(t, wo.y, ps.n * wo.z));
    ps.tmin = ray_eps_closest(ps.o);
    ps.tmax = INFINITY;
    ps.has_bounce = true;
    ps.phase = PH_CLOSEST;
    ps.nrays++;
}

// path_step<true, 0, SamplerT, TablesT, false> without its control flow: scenes of diffuse polygons only, two lanes per chain,
// paths begun by the caller (k_mutate_v4). Every lane computes the hit's vertex, the emitter-hit MIS term, the roulette
// decision, the light sample and the bounce once, in one instruction stream; the step's outcome (phase, dimensions used,
// radiance, rays) is then selected. The operations and their order are those of path_step, so f(u) is bit for bit the
// same. A lane whose path ends may compute garbage (NaN, inf) in what it does not use; none of it reaches `ps` or `sr`:
// radiance, dimensions and rays are selected, the shadow ray is written only when it is handed over, and the vertex
// and bounce fields only when the path goes on (a path that ends, or waits for its shadow ray, never reads them again).
// MASKED = false (k_mutate_w2): that last sentence is used instead of guarded against. Only what the caller reads of a path that
// has ended stays selected -- sr.valid, ps.Li, ps.k, ps.nrays, ps.shadow_pending, ps.phase -- and every other field is written
// on every lane that steps, garbage included: the two `if` blocks cost a saved exec mask and a run of masked v_mov each, per loop
// iteration. What is written without its condition, who could read it afterwards, and where it is set anew:
//   ps.nee                         read by the next step under ps.shadow_pending only (selected here; path_init clears it)
//   ps.thr, eta, depth, direct_on,
//   non_specular, has_bounce       path_init
//   ps.n, bpdf, bweight, beta_eta,
//   bdelta                         read by the next step under ps.has_bounce only (path_init clears it); the step that follows
//                                  path_begin computes with stale values there in the masked form as well, and selects them away
//   ps.wi, s, bsdf                 written for path_step's sake; this routine reads none of them
//   ps.o, d, tmin, tmax            path_begin; what a ray pass finds is read only after a PH_CLOSEST, which is selected (k_mutate_w2
//                                  runs the pass on every lane: one without a ray traces this garbage and nobody reads its hit)
//   sr.o, d, tmin, tmax            the helper lane's hit counts only under sr.valid (selected)
// Between a path's end and its path_init the lane is parked: mh_decide reads ps.px, ps.py, ps.Li, ps.nrays (and ps.k outside the
// orbital rule), the hand-off passes sr on, and nothing else looks at `ps`. A PH_FLUSH step (the path ended with its last shadow
// ray pending) runs this routine once more: it reads ps.Li, ps.nee, ps.shadow_pending of what was written, all three as the masked
// form leaves them, and selects everything else away (live = false).
// RARE_EMITTER_HIT = true (k_mutate_w2h): the emitter-hit MIS block, two divisions among its instructions, runs only in an iteration in
// which some stepping lane of the wave could use its result -- its bounce ray hit an emitter: live && hb && S.emitter >= 0 &&
// ps.direct_on && ps.non_specular, a wave-uniform test like test_box's `hole` (in a Cornell box a percent or two of the rays, and
// about 25 lanes step). When the block runs it is the block below, on every lane, with dn < 0 selecting as before; when it does
// not, Li is what it was and dn, dr, lumPdf and Lm, which nothing else reads, are never computed -- not even as garbage.
// (Commit b65b601 last carried a switch that compiled the unconditional block into k_mutate_w2h for an A/B run.)
// light_is_rectangle<TablesT> (k_mutate_w2h's HeldLightTablesT<true>): the light point is the rectangle's; the triangle's form, a root
// among its instructions, is not compiled in. Every other table type computes both and selects by the shape's tag, as before.
template <class SamplerT, class TablesT, bool MASKED = true, bool RARE_EMITTER_HIT = false>
DEV void path_step_diffuse(const DParams &P, const TablesT &T, PathState &ps, SamplerT &smp, const Hit &hit, bool shadow_clear,
                           ShadowRay &sr) {
    static_assert(draws_batched<SamplerT>::value, "the five draws are requested together");
    const uint32_t kmax = (uint32_t) P.eff_dim - 1u, k0 = ps.k;
    const float v0 = smp.next(min(k0, kmax)), v1 = smp.next(min(k0 + 1u, kmax)), v2 = smp.next(min(k0 + 2u, kmax));
    const float v3 = smp.next(min(k0 + 3u, kmax)), v4 = smp.next(min(k0 + 4u, kmax));
    sr.valid = false;
    // the partner's verdict on the previous vertex's shadow ray
    f3 Li = ps.Li;
    if (ps.shadow_pending && shadow_clear) Li = Li + ps.nee;
    // live: a PH_CLOSEST step whose ray hit something (PH_FLUSH and misses end the path here)
    const bool live = ps.phase != PH_FLUSH && hit.prim >= 0;
    const DShade S = T.shade(hit.prim >= 0 ? hit.prim : 0);
    const f3 p = fma3(ld3(S.eu), hit.u, fma3(ld3(S.ev), hit.v, ld3(S.origin)));
    const f3 n = ld3(S.n);
    const f3 s = ld3(S.eu) * S.inv_len_eu;
    const bool hb = ps.has_bounce;
    const f3 thr_b = hb ? ps.thr * ps.bweight : ps.thr;
    const float eta = hb ? ps.eta * ps.beta_eta : ps.eta;
    // emitter hit by the BSDF-sampled ray: MIS against direct sampling (refN is never zeroed without dielectrics)
    if (!RARE_EMITTER_HIT || __ballot(live && hb && S.emitter >= 0 && ps.direct_on && ps.non_specular) != 0ull) {
        const DEmitter E = T.emitter(S.emitter >= 0 ? S.emitter : 0);
        const float dn = dot3(ps.d, n);
        const float dr = dot3(ps.d, ps.n);
        float lumPdf = S.inv_area * hit.t * hit.t / fabsf(dn);
        lumPdf *= E.cdf_hi - E.cdf_lo;
        lumPdf = (!ps.bdelta && dr >= 0.f) ? lumPdf : 0.f;
        const float a = ps.bpdf * ps.bpdf, b = lumPdf * lumPdf;
        const f3 Lm = fma3(thr_b * ld3(E.radiance), a / (a + b), Li);
        if constexpr (RARE_EMITTER_HIT) {
            // (the `if` below, behind the wave's test, is compiled to two nested exec-masked regions with the arithmetic above sunk
            // into them; as a select on a condition without short cuts the block stays the straight-line block it is without the test)
            const bool use = (live & hb & (S.emitter >= 0) & ps.direct_on & ps.non_specular) & (dn < 0.f);
            Li = mk3(use ? Lm.x : Li.x, use ? Lm.y : Li.y, use ? Lm.z : Li.z);
        } else
        if (live && hb && S.emitter >= 0 && ps.direct_on && ps.non_specular && dn < 0.f) Li = Lm;
    }
    const bool want_rr = hb && ps.depth >= P.rr_depth;
    const int depth = hb ? ps.depth + 1 : ps.depth;
    const bool direct_on = hb || ps.direct_on;
    const bool at_max = depth >= P.max_depth && P.max_depth > 0;
    const float rr_q = fminf(max3(thr_b) * eta * eta, 0.95f);
    const bool survives = !want_rr || !(v0 >= rr_q);
    const f3 thr = want_rr ? thr_b * (1.f / rr_q) : thr_b;
    // go: the vertex is adopted and samples a light and a bounce
    const bool go = live && !at_max && survives;
    const f3 t = cross3(n, s);
    const f3 md = -ps.d;
    const f3 wi = mk3(dot3(md, s), dot3(md, t), dot3(md, n));
    const int bsdf = S.bsdf & 0xffffff;
    const DBsdf B = T.bsdf(bsdf);
    const bool want_nee = direct_on && B.type == 0;
    const float sx0 = want_rr ? v1 : v0, sy = want_rr ? v2 : v1;
    const int bpos = (want_rr ? 1 : 0) + (want_nee ? 2 : 0);
    const float bx = bpos == 0 ? v0 : (bpos == 1 ? v1 : (bpos == 2 ? v2 : v3));
    const float by = bpos == 0 ? v1 : (bpos == 1 ? v2 : (bpos == 2 ? v3 : v4));
    // direct illumination sampling
    int ei = 0; // DiscreteDistribution::sample (lower_bound semantics); the loop is wave-uniform
    for (int i = 1; i < T.n_emitters(P); ++i)
        if (T.emitter_cdf_lo(i) < sx0) ei = i;
    const DEmitter E = T.emitter(ei);
    const float emPdf = E.cdf_hi - E.cdf_lo;
    const float sx = (sx0 - E.cdf_lo) / emPdf; // sampleReuse
    const DShade L = T.emitter_shade(ei, E);
    f3 lp;
    if (light_is_rectangle<TablesT>::value || (L.bsdf >> 24) == PRIM_RECTANGLE) lp = fma3(ld3(L.eu), sx, fma3(ld3(L.ev), sy, ld3(L.origin)));
    else { const float a = sqrtf(fmaxf(0.f, 1.f - sx)); lp = fma3(ld3(L.eu), 1.f - a, fma3(ld3(L.ev), a * sy, ld3(L.origin))); }
    const f3 ln = ld3(L.n);
    const f3 dv = lp - p;
    const float dist2 = dot3(dv, dv), dist = sqrtf(dist2);
    const f3 dd = dv * (1.f / dist);
    const float dln = dot3(dd, ln);
    const float pdf = dln != 0.f ? L.inv_area * dist2 / fabsf(dln) : 0.f;
    const float drl = dot3(dd, n);
    const f3 wo_l = mk3(dot3(dd, s), dot3(dd, t), dot3(dd, n));
    const f3 bsdfVal = ld3(B.rgb) * (INV_PI_F * wo_l.z);
    const float bsdfPdf = INV_PI_F * wo_l.z;
    const float lpdf = pdf * emPdf;
    const float a = lpdf * lpdf, b = bsdfPdf * bsdfPdf;
    const f3 value = ld3(E.radiance) * (1.f / lpdf);
    const f3 c = thr * value * bsdfVal * (a / (a + b));
    const bool nee = go && want_nee && drl >= 0.f && dln < 0.f && pdf != 0.f && wi.z > 0.f && wo_l.z > 0.f && !is_zero3(c);
    // BSDF sampling (diffuse.cpp:139-149)
    const f3 wo = square_to_cosine_hemisphere(bx, by);
    const f3 bweight = ld3(B.rgb);
    const bool bounce = go && B.type == 0 && wi.z > 0.f && !is_zero3(bweight);
    // outcome
    ps.Li = Li;
    ps.k = k0 + ((live && want_rr) ? 1u : 0u) + (go ? (want_nee ? 4u : 2u) : 0u);
    ps.nrays += (nee ? 1u : 0u) + (bounce ? 1u : 0u);
    ps.shadow_pending = nee;
    ps.phase = bounce ? PH_CLOSEST : (nee ? PH_FLUSH : PH_DONE);
    if (!MASKED || nee) {
        ps.nee = c;
        sr.o = p; sr.d = dd;
        sr.tmin = ray_eps_shadow(p);
        sr.tmax = dist * (1.f - SHADOW_EPSILON_F);
        sr.valid = MASKED || nee;
    }
    if (!MASKED || bounce) {
        ps.thr = thr; ps.eta = eta; ps.depth = depth; ps.direct_on = direct_on;
        ps.wi = wi;
        ps.o = p; ps.n = n; ps.s = s;
        ps.bsdf = bsdf;
        ps.bpdf = INV_PI_F * wo.z;
        ps.bweight = bweight;
        ps.beta_eta = 1.f;
        ps.bdelta = false;
        ps.non_specular = true;
        ps.d = fma3(s, wo.x, fma3(t, wo.y, n * wo.z));
        ps.tmin = ray_eps_closest(p);
        ps.tmax = INFINITY;
        ps.has_bounce = true;
    }
}

// Run one full PSS evaluation (one wave-divergent loop; every step issues at most one ray query).
template <class SamplerT> DEV DSplat eval_path(const DParams &P, SamplerT &smp, uint32_t &nrays, uint32_t &ndims) {
    PathState ps;
    smp.reset_caches();
    path_init(P, ps);
    Hit h{-1, 0.f, 0.f, 0.f};
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    ShadowRay sr_unused;
    for (;;) {
        if (ps.phase != PH_BEGIN) h = trace(P, ps.o, ps.d, ps.tmin, ps.tmax, ps.phase == PH_SHADOW);
        path_step<false, 15>(P, T, ps, smp, h, false, sr_unused);
        if (ps.phase == PH_DONE) break;
    }
    DSplat out;
    out.px = ps.px; out.py = ps.py;
    out.r = ps.Li.x; out.g = ps.Li.y; out.b = ps.Li.z;
    out.lum = luminance3(ps.Li);
    nrays = ps.nrays;
    ndims = ps.k;
    return out;
}
