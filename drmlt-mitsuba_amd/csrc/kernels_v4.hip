// k_mutate_v4, k_mutate_w2<HELD> and k_mutate_v5: DRMLTRenderer::process / processMixture's chain loop (drmlt_proc.cpp:161-380,518-770),
// two lanes per chain (v4, w2) or a ray pool under 64 chains per wave (v5). ONE unit for the three on purpose: which of their templates
// a unit instantiates changes the machine code of the others -- k_mutate_w2<false> apart from k_mutate_v4, every k_mutate_v4 build
// apart from k_mutate_v5, k_mutate_v5's 16-bit-stack traversals apart from k_mutate_v4 -- and one of the latter measured 0.9 % slower
// in a unit of its own. Together they are the machine code they have always been. What k_mutate_v3
// (kernels_v3.hip) shares with them: chain_path.h.
#include <cstdlib>
#include <cstdio>
#include <type_traits>
#include "chain_path.h"

// ------------------------------------------------------------------------------------------
// k_mutate_v4: k_mutate_v3's two lanes per chain, without its lock-step rounds.
//
// In v3 the bookkeeping branch fires when all 32 chains of a wave are parked: a round lasts as long as the longest of 32
// paths (9.6 loop iterations per mutation where the mean path needs 3.9), because the branch costs the wave the same
// whether 1 or 32 chains take it -- per lane it walks D_eff dimensions (commit) and ~10 Philox blocks (next draws).
// Here that per-chain work is FLATTENED over the wave: the parked chains are compacted into a list (ballot + prefix
// count -> LDS) and all 64 lanes share the (chain, dimension pair) commit items and the (chain, Philox block) draw
// items, so the branch costs in proportion to the number of chains that take it and chains can run free: a chain starts
// its next evaluation as soon as its last one is digested. What is left per lane is the decision itself.
//
// Film: splats are queued in LDS and flushed by whole waves with the three colour channels of a splat in three adjacent
// lanes (one 12-byte segment per splat at the memory side instead of three scattered dwords), and the current state is
// splatted with its CUMULATIVE weight when it is replaced (or the launch ends) instead of once per mutation -- the
// reference's own PSSMLT loop does the same (pssmlt_proc.cpp:215-226,262-266); splatting is linear, the film is the
// same sum. An accepted proposal's weight starts the cumulative weight of the new current state.
//
// Chains are the same as k_mutate_v3's (same addressed draws, and the one copy of the arithmetic: device_sampler.h).
// (V4_STRIDE, V4_QCAP, V4_QCAP_BVH: launch_plan.h)
#define V4_STACK32_CAP 11 // LDS entries of a 32-bit traversal stack (the rest spills): 11 + 3 spare rows of 256 B keep eight waves on a CU

// STAMPS: the diagnostic build (DRMLT_DEBUG bit 128) with s_memtime section stamps; a compile-time switch because its
// sixteen 64-bit wave-uniform accumulators would otherwise sit in (and spill from) the scalar registers of the real kernel.
// Everything wave-uniform that k_mutate_v4 derives from the parameter block: recomputed (a handful of scalar ops) by each
// loop section from its own copy of the block, so that none of it occupies scalar registers across sections.
template <int RULE> struct V4Layout {
    RowSamplerT<RULE> smp;  // uniform fields only; `mode` and the group offsets are per lane (set_roles)
    V4Lds L;
    LdsTables LT;
    uint32_t D, D4, nb1;
    uint32_t group; // floats of one row group; the groups are at 0, group, 2 * group
};
template <int RULE> DEV V4Layout<RULE> v4_layout(const DParams &P, uint32_t qcap) {
    V4Layout<RULE> Y;
    Y.L.qcap = qcap;
    Y.D = (uint32_t) P.eff_dim;
    Y.D4 = (Y.D + 3u) & ~3u;
    Y.nb1 = Y.D4 / 4u; // first-stage Philox blocks of a mutation; item nb1 of a chain = the coins of its NEXT mutation
    Y.smp.key0 = P.key0; Y.smp.key1 = P.key1;
    Y.smp.mode = SM_STAGE1; Y.smp.type = P.type; Y.smp.sigma2 = P.sigma2;
    Y.smp.stride = V4_STRIDE;
    Y.smp.x_off = Y.smp.y_off = Y.smp.xyz = 0u;
    Y.group = Y.D4 * V4_STRIDE;
    Y.L.coin_off = 3u * Y.group;
    Y.L.list_off = Y.L.coin_off + 4u * V4_STRIDE;
    Y.L.q_off = Y.L.list_off + 32u;
    // v4_lds_bytes counts D rows for one of the groups (the plan and the waves per CU are those of a D-row x group): the D4 - D
    // rows it lacks, at most 99 floats, come out of the five queue rows -- 140 entries at least (BVH scenes: 80), 64 of them free
    // at the head of every bookkeeping branch
    const uint32_t q_floats = 5u * qcap - (Y.D4 - Y.D) * V4_STRIDE;
    Y.L.qcap = q_floats / 5u;
    Y.LT.shade_off = (Y.L.q_off + q_floats + 3u) & ~3u;
    Y.LT.bsdf_off = Y.LT.shade_off + (uint32_t) P.n_shade * 16u;
    Y.LT.emit_off = Y.LT.bsdf_off + (uint32_t) P.n_bsdfs * 12u;
    return Y;
}

// BUILD = FEAT | V4_ORBITAL_BUILD * RULE (device_types.h). The rule is fixed for a context's lifetime, so the builds that flat scenes
// with their tables in LDS run (V4_F0, V4_F0_STAMPS, V4_F3, V4_F7) have a twin with the orbital rule compiled in, and
// launch_mutate_v4 selects it once per launch by rule_is_orbital(P): no Build enumerator of its own, the plan is the same. The generic
// kernels keep their names and their code. V4_F3_STAMPS, a diagnostic build, has none (its twin spills 54 scalar registers where
// it spills 52: its stamps are those of the generic build). The BVH builds and the builds with their tables in device memory have no twin: their
// time is in the traversal and in table fetches. stats[14] counts the waves that ran an orbital build (DRMLT_VERBOSE prints it with drmlt_stats_get).
// BUILD also carries V4_ONE_LIGHT_BUILD * ONE_LIGHT: V4_F0 and V4_F0_STAMPS, the builds with the straight-line step, have under both
// rules a twin whose step reads the scene's one light from the parameter block (device_path.h: OneLightTables); launch_mutate_v4 selects
// it by scene_has_one_light(P) (device_types.h), again without a Build enumerator. stats[15] counts the waves that ran a one-light build.
#define V4_ORBITAL_BUILD 16
#define V4_ONE_LIGHT_BUILD 32
// The F7 builds (flat scenes with spheres, point lights, the environment or vertex normals) are compiled for three waves per SIMD:
// 165 to 168 registers, no scratch (tests/test_kernel_resources_smooth.py pins the counts). Every other build keeps the default bound.
#define V4_MIN_WAVES(BUILD) ((((BUILD) & (V4_ORBITAL_BUILD - 1)) == 7) ? 3 : 1)
template <int BUILD, bool LDS_TABLES, bool STAMPS, bool STACK16 = false, bool OVF = false>
__global__ void __launch_bounds__(CHAIN_BLOCK, V4_MIN_WAVES(BUILD)) k_mutate_v4(DParams P, uint32_t n_mut, uint32_t mut_base) {
    constexpr int FEAT = BUILD & (V4_ORBITAL_BUILD - 1), RULE = (BUILD & V4_ORBITAL_BUILD) / V4_ORBITAL_BUILD;
    constexpr bool ONE_LIGHT = (BUILD & V4_ONE_LIGHT_BUILD) != 0;
    static_assert(!ONE_LIGHT || (FEAT == 0 && LDS_TABLES), "the one-light twins are those of the straight-line step");
    typedef RowSamplerT<RULE> RowSampler;
    typedef V4Layout<RULE> V4Layout;
    constexpr bool orbital = RULE == RULE_ORBITAL; // stage 2 (Green's reverse move, kind 3, SM_REVERSE) does not occur
    if (orbital && threadIdx.x == 0) atomicAdd(P.stats + 14, 1ull);
    if (ONE_LIGHT && threadIdx.x == 0) atomicAdd(P.stats + 15, 1ull);
    // The parameter block is ~80 dwords, most of it used by one loop section only. Left to itself the compiler loads every
    // field it will ever need before the loop and then spills scalar registers into vector lanes all through the loop
    // (a sixth of the kernel's VALU instructions were v_readlane / v_writelane). Each loop section therefore works on its
    // own copy of the block, read through a kernarg pointer the compiler cannot see through: the fields a section uses
    // are scalar loads at its head (scalar cache hits) and dead at its end (SECTION_PARAMS, kernel_common.h).
    const uint32_t lane = threadIdx.x;
    const uint32_t sub = lane & 31u;
    const bool helper = lane >= 32u;
    const uint32_t c = blockIdx.x * 32u + sub;
    const bool live = !helper && c < P.n_chains;
    const uint32_t cc = c < P.n_chains ? c : P.n_chains - 1;
    const uint32_t S = V4_STRIDE;
    constexpr uint32_t QCAP = (FEAT & 8) ? V4_QCAP_BVH : V4_QCAP;
    int smp_mode = SM_STAGE1; // per-lane part of the sampler: which proposal the path in flight reads ...
    uint32_t roles; // ... and which row groups of the chain hold x and y (RowSampler::roles); every launch starts from groups 0 and 1
    uint32_t qn = 0u;
    ChainState cs;
    float cum = 0.f; // cumulative weight of the current state since it was adopted
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    PathState ps;
    bool helper_has_ray = false;
    Hit h{-1, 0.f, 0.f, 0.f};
    int batch;
    uint32_t base = 0u, target = 0u, limit = 0u; // mutation index of this chain's first mutation of the launch; see run-ahead below
    bool reported = false;                       // this wave has told the grid that all its chains are at the target
    constexpr bool RESUMABLE = (FEAT & 8) != 0; // BVH scenes: traversals survive loop iterations (device_path.h: Trav)
    Trav T;
    T.active = false; T.cur = 0; T.sp = 0; T.ovf = 0; T.rx = T.ry = T.rz = 0u; T.any_hit = false; T.h = h; T.tmin = 0.f;
    T.o = T.d = T.inv = T.oi = mk3(0.f, 0.f, 0.f);
    trav_reset_counters(T);
    int rstate = 0; // ray of this lane: 0 none, 1 issued, 2 being traversed, 3 result waiting to be consumed
    {
        const V4Layout Y = v4_layout<RULE>(P, QCAP);
        roles = RowSampler::first_roles(Y.group, sub);
        if (!helper) {
            for (uint32_t k = 0; k < Y.D; ++k) lds_x[k * S + sub] = unwrap01(P.x[(size_t) k * P.n_chains + cc]);
            for (uint32_t k = Y.D; k < Y.D4; ++k) lds_x[k * S + sub] = 0.f; // padding rows: proposed and adopted with the rest, never consumed
        }
        cs.cur.lum = P.cur_lum[cc]; cs.cur.px = P.cur_px[cc]; cs.cur.py = P.cur_py[cc];
        cs.cur.r = P.cur_r[cc]; cs.cur.g = P.cur_g[cc]; cs.cur.b = P.cur_b[cc];
        cs.y = cs.cur; cs.z = cs.cur;
        cs.a1 = 0.f; cs.coin_acc1 = cs.coin_acc2 = cs.coin_mix = 0.f;
        cs.it = 0u; cs.nd1 = cs.nd2 = 0u; cs.stage = -1; cs.large = false;
        path_init(P, ps);
        // Run-ahead (P.chain_done): `n_mut` is then the TARGET every chain must have reached when the launch ends, counted from
        // the chain's seeding; a chain that is there keeps mutating -- up to P.run_limit, the render's total -- for as long as
        // some chain of the grid is still short of the target. Every mutation executed is one of the chain's fixed total (its
        // index, hence its random numbers, is the chain's own count), so lanes that would have idled until the slowest chain of
        // the slowest wave is done do useful work instead; the render ends with every chain at exactly its total.
        base = (P.chain_done && live) ? P.chain_done[cc] : mut_base;
        target = P.chain_done ? n_mut : mut_base + n_mut;
        limit = P.chain_done ? P.run_limit : target;
        ps.phase = (live && base < limit) ? PH_DONE : PH_IDLE; // helpers stay PH_IDLE for good
        ps.o = mk3(0.f, 0.f, 0.f); ps.d = mk3(0.f, 0.f, 1.f); ps.tmin = 0.f; ps.tmax = 0.f;
        batch = P.mh_batch > 32 ? 32 : P.mh_batch;
        if (LDS_TABLES) stage_tables(P, Y.LT, lane);
        // coins of every chain's first mutation of this launch (afterwards they are drawn one mutation ahead, beside the proposal)
        if (!helper) {
            const u4 coins = philox4x32_10(P.key0, P.key1, 0u, base, P.chain_offset + blockIdx.x * 32u + sub, TAG_COIN);
            float *dst = &lds_x[Y.L.coin_off + sub];
            dst[0] = u32_to_unit(coins.x); dst[S] = u32_to_unit(coins.y); dst[2u * S] = u32_to_unit(coins.z); dst[3u * S] = u32_to_unit(coins.w);
        }
    }

    constexpr bool prio = true; // wave priority by loop section (see k_mutate_v3)
    constexpr bool stamps = STAMPS;
    // The stamps builds keep sixteen wave-uniform accumulators in scalar registers across the loop. The one-light twins count their
    // EVENTS (iterations, branches, tracing lanes, the histogram) in 32 bits per wave and launch -- at most 40 960 mutations per
    // chain (a slice of 32 768 and the run-ahead cap), some six iterations each, times 64 lanes: far from 2^32 -- so that they
    // spill no more scalars than the builds they replace; cycle sums stay 64-bit. The other builds keep their code.
    typedef typename std::conditional<ONE_LIGHT, uint32_t, unsigned long long>::type StampCount;
    unsigned long long t_mh = 0, t_trace = 0, t_step = 0;
    StampCount n_iter = 0, n_mh = 0, n_busy = 0;
    unsigned long long t_decide = 0, t_commit = 0, t_start = 0, t_fill = 0;
    StampCount hist[6] = {0, 0, 0, 0, 0, 0};
    unsigned long long dg[6] = {0, 0, 0, 0, 0, 0};
#define STAMP() (stamps ? __builtin_amdgcn_s_memtime() : 0ull)
    for (;;) {
        const bool parked = ps.phase == PH_DONE;
        const unsigned long long pmask = __ballot(parked);
        const unsigned long long rmask = __ballot(ps.phase != PH_DONE && ps.phase != PH_IDLE);
        if (!pmask && !rmask) break;
        const unsigned long long s0 = STAMP();
        if (pmask && (__popcll(pmask) >= batch || !rmask)) {
            n_mh++;
            SECTION_PARAMS(Pm);
            const V4Layout Y = v4_layout<RULE>(Pm, QCAP);
            const V4Lds &L = Y.L;
            RowSampler smp = Y.smp;
            smp.set_roles(roles, Y.group, sub); smp.mode = smp_mode;
            const uint32_t nb1 = Y.nb1, D4 = Y.D4;
            int *const lds_list = reinterpret_cast<int *>(&lds_x[L.list_off]);
            if (prio) __builtin_amdgcn_s_setprio(2);
            if (qn + 64u > L.qcap) { SECTION_PARAMS(Pf); v4_flush(Pf, L, qn, lane); } // room for this branch's splats (at most 2 per chain)
            // ---- decide (parked chain lanes): weights, commit mode, what the chain does next
            int commit = 0, kind = 0; // kind: 0 nothing / finished, 1 next mutation, 2 second stage, 3 Green's reverse
            bool wantA = false, wantB = false;
            float eAx = 0.f, eAy = 0.f, eAr = 0.f, eAg = 0.f, eAb = 0.f;
            float eBx = 0.f, eBy = 0.f, eBr = 0.f, eBg = 0.f, eBb = 0.f;
            if (parked) {
                const MhDigest o = mh_decide<RULE>(Pm, cs, smp, ps, ct);
                if (o.decided) {
                    cum += o.w.w0;
                    const bool a1st = o.acc1, a2nd = o.acc2, adopt = a1st || a2nd;
                    // rejected proposals are splatted now, an adopted one carries its weight into `cum`
                    const DSplat sb = select_splat(a2nd, cs.y, cs.z);
                    const float wb = a2nd ? o.w.w1 : o.w.w2;
                    wantB = !a1st && wb > 0.f;
                    eBx = sb.px; eBy = sb.py; eBr = sb.r * wb; eBg = sb.g * wb; eBb = sb.b * wb;
                    const DSplat sa = select_splat(adopt, cs.cur, cs.y);
                    const float wa = adopt ? cum : o.w.w1;
                    wantA = wa > 0.f;
                    eAx = sa.px; eAy = sa.py; eAr = sa.r * wa; eAg = sa.g * wa; eAb = sa.b * wa;
                    if (adopt) {
                        cum = a1st ? o.w.w1 : o.w.w2;
                        cs.cur = select_splat(a1st, cs.y, cs.z);
                        if (o.amap) { // acceptance map: a mark at the pixel of the state that was LEFT (the weights are all zero)
                            const f3 mc = mh_amap_colour(o.amap);
                            wantB = true; eBx = eAx; eBy = eAy; eBr = mc.x; eBg = mc.y; eBb = mc.z;
                        }
                    }
                    commit = mh_commit_mode(o);
                }
                kind = cs.stage < 0 ? 4 : ((orbital || cs.stage == 1) ? 2 : 3); // 4: between mutations -- resolved below
            }
            kind = mh_resolve_kind(Pm, kind, live, base + cs.it, target, limit, reported, lane);
            v4_enqueue(L, qn, wantA, eAx, eAy, eAr, eAg, eAb);
            v4_enqueue(L, qn, wantB, eBx, eBy, eBr, eBg, eBb);
            const unsigned long long m1 = STAMP();

            // ---- commit (DRMLTSampler::accept: uCurrent = wrap(chosen proposal)): the chosen proposal's row group BECOMES the
            // chain's x group -- nothing is copied, and the wrap happens where x is read
            smp.adopt(commit);
            roles = smp.roles();
            const unsigned long long m2 = STAMP();

            // ---- start (parked chain lanes): the coins of the mutation that begins were drawn with the previous one
            if (parked && kind == 1) {
                const float *cn = &lds_x[L.coin_off + sub];
                cs.large = cn[0] < Pm.p_large;
                cs.coin_acc1 = cn[S]; cs.coin_acc2 = cn[2u * S]; cs.coin_mix = cn[3u * S];
                cs.stage = 0;
                cs.nd1 = cs.nd2 = 0u;
            }
            const unsigned long long m3 = STAMP();

            // ---- proposals of the chains that start a mutation, flattened: items (chain j, Philox block b) -> dimensions
            // 4b..4b+3 of y; block nb1 = the four coins (large step, first / second acceptance, mixture) of the NEXT mutation
            SECTION_PARAMS(Pg);
            const V4Layout Yg = v4_layout<RULE>(Pg, QCAP);
            RowSampler smg = Yg.smp;
            const uint32_t chain_base_g = Pg.chain_offset + blockIdx.x * 32u;
            const uint32_t maj_mine = base + cs.it; // the mutation in flight (cs.it counts the mutations decided in this launch)
            const unsigned info = roles | (cs.large ? 1u : 0u); // the chain's x and y offsets + its large-step bit, for the lanes that fill its rows
            const uint32_t f1mask = (uint32_t) __ballot(kind == 1);
            if (f1mask) {
                if (kind == 1) lds_list[__builtin_amdgcn_mbcnt_lo(f1mask, 0u)] = (int) sub;
                const uint32_t n = (uint32_t) __popc(f1mask), total = n * (nb1 + 1u);
                const float rcp_n = 1.f / (float) n;
                for (uint32_t base = 0u; base < total; base += 64u) {
                    const uint32_t i = base + lane;
                    const bool valid = i < total;
                    const uint32_t ii = valid ? i : 0u;
                    const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                    const uint32_t cj = (uint32_t) lds_list[j];
                    const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                    const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                    smg.set_roles(inf, Yg.group, cj);
                    if (valid) {
                        if (b < nb1) smg.fill_first(b, mj, chain_base_g + cj, (inf & 1u) != 0u);
                        else {
                            const u4 coins = philox4x32_10(Pg.key0, Pg.key1, 0u, mj + 1u, chain_base_g + cj, TAG_COIN);
                            float *dst = &lds_x[L.coin_off + cj];
                            dst[0] = u32_to_unit(coins.x); dst[S] = u32_to_unit(coins.y); dst[2u * S] = u32_to_unit(coins.z); dst[3u * S] = u32_to_unit(coins.w);
                        }
                    }
                }
            }
            const uint32_t f2mask = (uint32_t) __ballot(kind == 2);
            if (f2mask) { // second-stage proposals (rare: rejected bold steps)
                if (kind == 2) lds_list[__builtin_amdgcn_mbcnt_lo(f2mask, 0u)] = (int) sub;
                // blocks per chain: uniforms for a large step (one per dim), the orbital angles (one per pair), Gaussian pairs otherwise
                const uint32_t nb2 = (orbital || Pg.type == 2) ? (Pg.timid_after_large ? D4 / 4u : (D4 / 2u + 3u) / 4u) : D4 / 2u;
                const uint32_t n = (uint32_t) __popc(f2mask), total = n * nb2;
                const float rcp_n = 1.f / (float) n;
                for (uint32_t base = 0u; base < total; base += 64u) {
                    const uint32_t i = base + lane;
                    const bool valid = i < total;
                    const uint32_t ii = valid ? i : 0u;
                    const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                    const uint32_t cj = (uint32_t) lds_list[j];
                    const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                    const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                    smg.set_roles(inf, Yg.group, cj);
                    if (valid) smg.fill_second(b, D4, mj, chain_base_g + cj, (inf & 1u) != 0u);
                }
            }
            const unsigned long long m4 = STAMP();

            // ---- begin the evaluation (parked chain lanes): film position and camera ray from the first two components
            if (parked) {
                if (kind == 0) ps.phase = PH_IDLE;
                else {
                    SECTION_PARAMS(Pb);
                    smp_mode = smp.mode = cs.stage == 0 ? SM_STAGE1 : ((orbital || cs.stage == 1) ? SM_STAGE2 : SM_REVERSE);
                    path_init(Pb, ps);
                    const float v0 = smp.next(0u), v1 = smp.next(1u);
                    path_begin(Pb, ps, v0, v1);
                    if (RESUMABLE) rstate = 1;
                }
            }
            const unsigned long long m5 = STAMP();
            t_decide += m1 - s0; t_commit += m2 - m1; t_fill += m4 - m3; t_start += (m3 - m2) + (m5 - m4);
        }
        const unsigned long long s1 = STAMP();
        unsigned long long s2 = s1;
        if constexpr (!RESUMABLE) {
            // one ray per lane: chain lanes their camera / bounce ray, helpers the shadow ray they were handed
            const bool tracing = helper ? helper_has_ray : ps.phase == PH_CLOSEST;
            if (stamps) n_busy += __popcll(__ballot(tracing));
            if (stamps) { const int nl = __popcll(__ballot(tracing && !helper)); hist[nl == 0 ? 0 : (nl <= 4 ? 1 : (nl <= 8 ? 2 : (nl <= 16 ? 3 : (nl <= 24 ? 4 : 5))))]++; }
            if (prio) __builtin_amdgcn_s_setprio(0);
            {
                SECTION_PARAMS(Pt);
                if (tracing) h = trace<FEAT>(Pt, ps.o, ps.d, ps.tmin, ps.tmax, helper);
            }
            if (prio) __builtin_amdgcn_s_setprio(3);
            s2 = STAMP();
            const unsigned occluded = from_upper_u((helper_has_ray && h.prim >= 0) ? 1u : 0u);
            helper_has_ray = false;
            ShadowRay sr;
            sr.o = ps.o; sr.d = ps.d; sr.tmin = 0.f; sr.tmax = 0.f; sr.valid = false;
            {
                SECTION_PARAMS(Ps);
                if (!helper && ps.phase != PH_DONE && ps.phase != PH_IDLE) {
                    const V4Layout Y = v4_layout<RULE>(Ps, QCAP);
                    RowSampler smp = Y.smp;
                    smp.set_roles(roles, Y.group, sub); smp.mode = smp_mode;
                    if constexpr (ONE_LIGHT) path_step_diffuse(Ps, OneLightTables{Y.LT, Ps}, ps, smp, h, occluded == 0u, sr); // ... with the light in scalar registers
                    else if constexpr (FEAT == 0 && LDS_TABLES) path_step_diffuse(Ps, Y.LT, ps, smp, h, occluded == 0u, sr); // diffuse polygons: straight-line step
                    else if (LDS_TABLES) path_step<true, FEAT, RowSampler, LdsTables, false>(Ps, Y.LT, ps, smp, h, occluded == 0u, sr);
                    else path_step<true, FEAT, RowSampler, GlobalTables, false>(Ps, GlobalTables{Ps.shade, Ps.bsdfs, Ps.emitters}, ps, smp, h, occluded == 0u, sr);
                }
            }
            // hand the shadow ray of this vertex to the helper lane
            const float ox = from_lower(sr.o.x), oy = from_lower(sr.o.y), oz = from_lower(sr.o.z);
            const float dx = from_lower(sr.d.x), dy = from_lower(sr.d.y), dz = from_lower(sr.d.z);
            const float t0 = from_lower(sr.tmin), t1 = from_lower(sr.tmax);
            const float vf = from_lower(sr.valid ? 1.f : 0.f);
            if (helper) {
                ps.o = mk3(ox, oy, oz); ps.d = mk3(dx, dy, dz); ps.tmin = t0; ps.tmax = t1;
                helper_has_ray = vf != 0.f;
            }
        } else {
            // ---- BVH scenes. A lane's traversal continues across iterations; a slice ends when every traversal is done
            // or `trace_yield` lanes have finished theirs. A chain lane steps when its own ray AND its partner's shadow
            // ray (of the previous vertex) are both done; everybody else just keeps traversing next time round.
            if (prio) __builtin_amdgcn_s_setprio(0);
            if (P.debug & 1024) { // diagnostic: where the 64 lanes are when a traversal slice starts
                dg[0]++; dg[1] += __popcll(__ballot(rstate == 1 || rstate == 2)); dg[2] += __popcll(__ballot(!helper && rstate == 3));
                dg[3] += __popcll(__ballot(!helper && ps.phase == PH_DONE)); dg[4] += __popcll(__ballot(helper && rstate == 0));
                dg[5] += __popcll(__ballot(!helper && ps.phase == PH_FLUSH));
            }
            {
                SECTION_PARAMS(Pt);
                if (rstate == 1) { trav_begin(T, ps.o, ps.d, ps.tmin, ps.tmax, helper); rstate = 2; }
                if (STACK16) trav_run<short, DParams, OVF, BVH_STACK, FEAT>(Pt, T, rstate == 2, Pt.trace_yield);
                else trav_run<int, DParams, true, V4_STACK32_CAP, FEAT>(Pt, T, rstate == 2, Pt.trace_yield); // always with the overflow paths
                if (rstate == 2 && !T.active) rstate = 3;
            }
            if (prio) __builtin_amdgcn_s_setprio(3);
            s2 = STAMP();
            const unsigned partner_busy = from_upper_u((rstate == 1 || rstate == 2) ? 1u : 0u);
            const unsigned occluded = from_upper_u((rstate == 3 && T.h.prim >= 0) ? 1u : 0u);
            const bool ready = !helper && partner_busy == 0u && ((ps.phase == PH_CLOSEST && rstate == 3) || ps.phase == PH_FLUSH);
            ShadowRay sr;
            sr.o = ps.o; sr.d = ps.d; sr.tmin = 0.f; sr.tmax = 0.f; sr.valid = false;
            {
                SECTION_PARAMS(Ps);
                if (ready) {
                    h = T.h;
                    rstate = 0;
                    const V4Layout Y = v4_layout<RULE>(Ps, QCAP);
                    RowSampler smp = Y.smp;
                    smp.set_roles(roles, Y.group, sub); smp.mode = smp_mode;
                    if (LDS_TABLES) path_step<true, FEAT, RowSampler, LdsTables, false>(Ps, Y.LT, ps, smp, h, occluded == 0u, sr);
                    else path_step<true, FEAT, RowSampler, GlobalTables, false>(Ps, GlobalTables{Ps.shade, Ps.bsdfs, Ps.emitters}, ps, smp, h, occluded == 0u, sr);
                    if (ps.phase == PH_CLOSEST) rstate = 1;
                }
            }
            // the partner's result has been consumed; hand it the shadow ray of this vertex, if any
            const unsigned stepped = from_lower_u(ready ? 1u : 0u);
            const float ox = from_lower(sr.o.x), oy = from_lower(sr.o.y), oz = from_lower(sr.o.z);
            const float dx = from_lower(sr.d.x), dy = from_lower(sr.d.y), dz = from_lower(sr.d.z);
            const float t0 = from_lower(sr.tmin), t1 = from_lower(sr.tmax);
            const float vf = from_lower(sr.valid ? 1.f : 0.f);
            if (helper && stepped != 0u) {
                rstate = 0;
                if (vf != 0.f) { ps.o = mk3(ox, oy, oz); ps.d = mk3(dx, dy, dz); ps.tmin = t0; ps.tmax = t1; rstate = 1; }
            }
        }
        const unsigned long long s3 = STAMP();
        t_mh += s1 - s0; t_trace += s2 - s1; t_step += s3 - s2; n_iter++;
    }
#undef STAMP
    // the epilogue reads its own copy of the block too: otherwise the compiler keeps the pointers it shares with the prologue
    // (state rows, film, counters) in scalar registers -- spilled -- all through the loop
    SECTION_PARAMS(Pe);
    // "Perform the last splat": the current states with what they have accumulated since they were adopted
    const V4Layout Y = v4_layout<RULE>(Pe, QCAP);
    if (qn + 32u > Y.L.qcap) v4_flush(Pe, Y.L, qn, lane); // (the last branch may have left fewer than 32 entries free)
    v4_enqueue(Y.L, qn, live && cum > 0.f, cs.cur.px, cs.cur.py, cs.cur.r * cum, cs.cur.g * cum, cs.cur.b * cum);
    v4_flush(Pe, Y.L, qn, lane);
    if (stamps && lane == 0) {
        atomicAdd(Pe.stats + 16, t_mh); atomicAdd(Pe.stats + 17, t_trace); atomicAdd(Pe.stats + 18, t_step);
        atomicAdd(Pe.stats + 19, (unsigned long long) n_iter); atomicAdd(Pe.stats + 20, (unsigned long long) n_mh); atomicAdd(Pe.stats + 21, (unsigned long long) n_busy);
        for (int q = 0; q < 6; ++q) atomicAdd(Pe.stats + 26 + q, (unsigned long long) hist[q]);
        atomicAdd(Pe.stats + 22, t_decide); atomicAdd(Pe.stats + 23, t_commit); atomicAdd(Pe.stats + 24, t_start); atomicAdd(Pe.stats + 25, t_fill);
    }
    if (live) {
        RowSampler smp = Y.smp;
        smp.set_roles(roles, Y.group, sub);
        for (uint32_t k = 0; k < Y.D; ++k) Pe.x[(size_t) k * Pe.n_chains + c] = smp.x(k); // the wrap the commit used to do
        Pe.cur_lum[c] = cs.cur.lum; Pe.cur_px[c] = cs.cur.px; Pe.cur_py[c] = cs.cur.py;
        Pe.cur_r[c] = cs.cur.r; Pe.cur_g[c] = cs.cur.g; Pe.cur_b[c] = cs.cur.b;
        if (Pe.chain_done) Pe.chain_done[c] = base + cs.it;
    }
    if (Pe.chain_done && !reported && lane == 0) atomicSub(Pe.waves_left, 1u); // (a wave none of whose chains had anything to do)
    flush_counters(Pe, ct, lane);
    const unsigned long long decided = wave_sum((live && !helper) ? cs.it : 0u); // mutations decided in this launch (with run-ahead: not n_mut per chain)
    if (lane == 0) atomicAdd(Pe.stats + 9, decided);
    if (RESUMABLE) {
        const unsigned long long nn = wave_sum(T.n_nodes), np = wave_sum(T.n_prims);
        if (lane == 0) { atomicAdd(Pe.stats + 10, nn); atomicAdd(Pe.stats + 11, np); atomicAdd(Pe.stats + 12, (unsigned long long) T.it_inner); atomicAdd(Pe.stats + 13, (unsigned long long) T.it_leaf); }
        if ((Pe.debug & 1024) && lane == 0)
            for (int q = 0; q < 6; ++q) atomicAdd(Pe.stats + 20 + q, dg[q]);
    }
}

// ------------------------------------------------------------------------------------------
// k_mutate_w2<HELD>: k_mutate_v4<V4_ONE_LIGHT_BUILD | V4_ORBITAL_BUILD, true, false> -- flat scene, tables in LDS, orbital rule, one
// area light -- compiled for TWO waves per SIMD. launch_mutate_v4 runs it in place of that twin on launches that cannot have a third
// wave on a SIMD (launch_plan.h: w2_launch), bench.py's flagship line among them: there the twin's 168-register bound buys
// nothing, and a wave's rate is its own serial time, instructions plus the waits one partner cannot cover. A kernel of its own
// name because the v3 / v4 / v5 instantiations are pinned register by register (tests/test_kernel_resources_smooth.py).
// Same chains bit for bit: the LDS layout, the run-ahead protocol, the splat queue, the prologue and epilogue are k_mutate_v4's,
// every floating-point expression is a header routine it shares with the twin. What differs, ingredient by ingredient (DESIGN.md section 7a has the measurements; commit b65b601
// last carried a source switch for each, which compiled the twin's form back in for an A/B run):
//   held constants    the wave-uniform constants that are only ever VALU operands or LDS address terms -- layout offsets, the light's
//                     two records, the camera, p_large, the roulette depths -- are read ONCE, in the prologue, and stay in vector
//                     registers (W2Held); the step and the bookkeeping branch open without a scalar load or v4_layout. The step's wait
//                     chain is otherwise the twin's: five component reads, a wait, the hit's shading record, a wait, the BSDF record.
//   held scalars      what the bookkeeping branch needs in SCALAR registers (the importance map, chain_done, waves_left, the Philox
//                     keys, chain_offset, eff_dim, timid_after_large) waits in vector registers too and comes back with one
//                     v_readfirstlane each: thirteen VALU instructions for a scalar-cache round trip. The streaming ray pass reads
//                     its record pointers and counts as k_mutate_v4 does (holding them measured slower).
//   one Philox site   a fill item computes its counter and tag per lane and calls Philox ONCE; only the tail differs
//                     (row_fill_first_drawn for a proposal block, four writes for a coin block).
//   unmasked step     the step writes the vertex, the bounce, ps.nee and the shadow ray on every lane that steps and selects only what a
//                     path that has ended is still read for (path_step_diffuse<.., MASKED = false>, device_path.h, lists each field
//                     and where it is set anew); the twin's two masked copy-back blocks are gone.
//   swapped hand-off  the shadow ray reaches the helper lanes in ONE v_permlane32_swap per value (lower_keeps: a chain lane keeps its
//                     own ray, its helper receives the shadow ray) in place of a broadcast from the lower half and a block of masked
//                     moves on the helpers.
//   unmasked trace    when any lane has a ray the WHOLE wave runs the ray pass (a wave-uniform test, no saved exec mask and no masked
//                     merge of the hit), and the shadow ray of a lane that does not step is left undefined instead of being set to
//                     zeros and copies. The ray pass reads memory through scalar loads only (HELD: not at all), so a lane without a
//                     ray computes garbage and touches nothing; `h` is read by lanes that traced, and by a PH_FLUSH step, which uses
//                     hit.prim -- a record's index or -1 -- for an LDS address and selects everything else away.
//   own film flush    w2_flush (below): the box filter and the tabulated filters in separate loop nests, the table read from LDS, so
//                     that no wait inside a flush names vmcnt and the film's no-return atomics are never waited for (+1.0 % with the
//                     box filter, -0.9 % with the Gaussian, where the atomics are the bound). The twin's three sites call v4_flush.
// Not here: the step's component reads issued ahead of the ray pass, and components and shading record requested in one batch
// (both built and measured: no gain and a loss, section 7a). The splat path keeps
// film_put_channel's debug test (DRMLT_DEBUG bit 1 must go on working; one scalar compare per flushed splat).
// stats[16] counts the waves that ran it (no build without stamps writes that slot; drmlt_stats_get prints it under DRMLT_VERBOSE).
//
// HELD (w2h; k_mutate_w2<false> is w2): the RAY PASS OVER RECORDS HELD IN VECTOR REGISTERS. A scene of one to three cuboids and at
// most one flat record without plain triangles (bench.py's Cornell box: three cuboids and the light) has 58 dwords of records, which
// never change during a launch. w2 streams them through two software-pipelined scalar loops in every iteration: the block's
// pointers, then the records, counters, read-ahead and waits. w2h reads them once, in the prologue, pinned like W2Held, and the
// pass is straight-line code that reads no memory at all (device_path.h: trace_held -- test_box and test_flat's arithmetic, in the
// loops' order, on the same values, the rows component by component where the loops use packed f32 (r20: each component rounds
// alike): the same chains bit for bit). launch_mutate_v4 runs it where the plan says so (launch_plan.h:
// w2_held_launch; DRMLT_NO_W2_HELD keeps w2). Three more things are w2h's own, and nothing launches a mixed form, so the one parameter
// selects them too: the decide is w2h_decide, by selects (w2: mh_decide and the twin's digest); the step runs its emitter-hit block only when
// a bounce ray of the wave hit the light (RARE_EMITTER_HIT); and the proposals of both stages are filled in ONE flattened pass with one Philox
// site (w2: two loops). And the iteration carries less around its arithmetic: the scene's shape is one held
// word of flags, a scalar bit test per slot and per open cuboid (trace_held; the tail of the pass by selects); the step has no
// triangle-light arm (HeldLightTablesT<true>); the hand-off's three copies stand ahead of its swaps and the two flags cross
// the halves against whatever a register holds; the wave's ray test is the `or` of two compare masks. And w2h expects its
// bookkeeping branch to be skipped, so that the ray pass follows the loop head and the branch stands behind the hand-off (r20).
// stats[14..16] as w2, stats[17] counts w2h's waves. The loop stands in the kernel itself, not in a routine both call:
// the tests of the build (tests/test_w2_flush_isa.py, test_w2h_isa.py, test_w2h_decide_isa.py, test_w2h_fill_isa.py) count by the kernel's lines.

// k_mutate_w2<true>'s decide (w2h): mh_decide<RULE_ORBITAL> and the caller's digest of its outcome (cumulative weight, the two queued splats,
// adoption) WITHOUT ARMS. In the bookkeeping branch about 16 of 64 lanes are parked, and the arms of the state machine -- stage -1 /
// 0 / 1, decided or not, adopted or not -- each sat behind a saved exec mask with a run of masked v_mov where they merge: the wave
// paid every arm on every call. Here every lane of the branch, parked or not, computes the first-stage test, the orbital second-stage
// test, the weights, the counter increments and both splats on whatever its registers hold, and selects choose what is kept: by
// `parked`, by cs.stage and by the outcomes. A lane that is not parked, or parked with nothing evaluated (stage < 0: the first
// call of a launch), keeps every value it had: no counter, weight or cs.it moves, and its splats are not wanted. The operations
// that produce a kept value, and their order, are those of mh_decide / mh_digest / mh_first / mh_second_orbital / mh_weights /
// mh_count and of the digest written out in k_mutate_w2<false>: the same chains bit for bit (tests/test_gpu_w2h_decide.py).
//   * the luminance test lum_invalid(res.lum) serves both stages (mh_first tests y's luminance, mh_digest z's: at either stage it
//     is the evaluation just finished);
//   * w1 = a1, w2 = (1 - a1) * a2, w0 = 1 - w1 - w2, then w2 = 0 without a second stage: at stage 0, a2 is 0 and 0 <= a1 <= 1, so
//     w2 is +0 before it is cleared and w0 is 1 - a1 either way -- one expression serves both stages, in mh_weights' order;
//   * what stays behind a branch is wave-uniform: the importance-map arm of the normalisation (P.importance; inside it, only lanes
//     with an evaluation read the map -- another lane's pixel is stale or not yet set).
// (Commit b65b601 last carried a switch that compiled the other form into this instantiation for an A/B run.)
struct W2hQueued { bool want; float px, py, r, g, b; };
DEV void w2h_decide(const DParams &P, bool parked, ChainState &cs, const PathState &ps, Counters &ct, float &cum, int &commit, int &kind,
                    W2hQueued &A, W2hQueued &B) {
    const int stage = cs.stage;
    const bool evald = parked && stage >= 0, first = evald && stage == 0, second = evald && stage != 0;
    DSplat res;
    res.px = ps.px; res.py = ps.py; res.r = ps.Li.x; res.g = ps.Li.y; res.b = ps.Li.z;
    res.lum = luminance3(ps.Li);
    if (P.importance) { // normalize_splat's first half
        float lum = 0.f;
        if (evald && !(res.r == 0.f && res.g == 0.f && res.b == 0.f)) {
            const int ix = min(max(0, (int) res.px), P.width - 1), iy = min(max(0, (int) res.py), P.height - 1);
            const float lv = P.importance[ix + iy * P.width];
            res.r /= lv; res.g /= lv; res.b /= lv;
            lum = luminance3(mk3(res.r, res.g, res.b));
        }
        res.lum = lum;
    }
    { // ... and its second
        const float inv = 1.f / res.lum;
        const bool pos = res.lum > 0.f;
        res.r = pos ? res.r * inv : res.r; res.g = pos ? res.g * inv : res.g; res.b = pos ? res.b * inv : res.b;
    }
    ct.rays += evald ? ps.nrays : 0u;
    const bool invalid = lum_invalid(res.lum), large = cs.large;
    // first stage (mh_first, no mixture)
    const float a1f = invalid ? 0.f : fminf(1.f, res.lum / cs.cur.lum);
    const bool acc1f = a1f > 0.f && mh_flip(a1f, cs.coin_acc1);
    const bool go_on = first && !acc1f && (P.timid_after_large != 0 || !large); // not decided: the second stage follows
    // orbital second stage (mh_second_orbital on y's luminance, kept since stage 0)
    const float y_lum = cs.y.lum, cur_lum = cs.cur.lum;
    const bool reject = invalid || res.lum < y_lum, full = res.lum >= cur_lum;
    const float ratio = (res.lum - y_lum) / (cur_lum - y_lum);
    const float a2 = (!second || reject) ? 0.f : (full ? 1.f : ratio);
    const bool acc2 = second && !reject && (full || mh_flip(ratio, cs.coin_acc2));
    const bool acc1 = first && acc1f; // (an accepted first stage never goes on)
    const bool decided = evald && !go_on;
    cs.y = select_splat(first, res, cs.y);
    cs.z = select_splat(second, res, cs.z);
    const float a1 = first ? a1f : cs.a1;
    cs.a1 = a1;
    MhWeights w;
    w.w1 = a1; w.w2 = (1.f - a1) * a2; w.w0 = 1.f - w.w1 - w.w2;
    w.w2 = second ? w.w2 : 0.f;
    { // mh_count, its increments under `decided`
        const bool lg = decided && large, bold = decided && !large;
        ct.large_acc1l += (lg ? 1u : 0u) + ((lg && acc1) ? 1u << 16 : 0u);
        ct.acc1b_secl += ((bold && acc1) ? 1u : 0u) + ((lg && second) ? 1u << 16 : 0u);
        ct.secb_acc2l += ((bold && second) ? 1u : 0u) + ((lg && acc2) ? 1u << 16 : 0u);
        ct.acc2b_rev += (bold && acc2) ? 1u : 0u;
    }
    cs.it += decided ? 1u : 0u;
    cs.stage = decided ? -1 : (go_on ? 1 : stage);
    // the digest of k_mutate_w2<false>: the current state collects its weight, a replaced state and the proposals are queued
    cum = decided ? cum + w.w0 : cum;
    const bool adopt = acc1 || acc2;
    const float wb = acc2 ? w.w1 : w.w2;
    B.want = decided && !acc1 && wb > 0.f;
    B.px = acc2 ? cs.y.px : cs.z.px; B.py = acc2 ? cs.y.py : cs.z.py;
    B.r = (acc2 ? cs.y.r : cs.z.r) * wb; B.g = (acc2 ? cs.y.g : cs.z.g) * wb; B.b = (acc2 ? cs.y.b : cs.z.b) * wb;
    const float wa = adopt ? cum : w.w1;
    A.want = decided && wa > 0.f;
    A.px = adopt ? cs.cur.px : cs.y.px; A.py = adopt ? cs.cur.py : cs.y.py;
    A.r = (adopt ? cs.cur.r : cs.y.r) * wa; A.g = (adopt ? cs.cur.g : cs.y.g) * wa; A.b = (adopt ? cs.cur.b : cs.y.b) * wa;
    cum = adopt ? (acc1 ? w.w1 : w.w2) : cum;
    cs.cur = select_splat(adopt, select_splat(acc1, cs.y, cs.z), cs.cur);
    commit = acc1 ? SM_STAGE1 : (acc2 ? SM_STAGE2 : 0);
    kind = parked ? (cs.stage < 0 ? 4 : 2) : 0; // 4: between mutations -- resolved by mh_resolve_kind
}

// the hand-off in one v_permlane32_swap per value: lane i < 32 keeps `keep`, lane 32 + i receives lane i's `give`
DEV unsigned lower_keeps_u(unsigned keep, unsigned give) { return __builtin_amdgcn_permlane32_swap(keep, give, false, false)[0]; }
DEV float lower_keeps(float keep, float give) { return __uint_as_float(lower_keeps_u(__float_as_uint(keep), __float_as_uint(give))); }
template <class T> DEV void hold_v(T &x) { asm volatile("" : "+v"(x)); }
DEV uint32_t wave_uniform(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
template <class T> DEV T *uniform_ptr(uint32_t lo, uint32_t hi) { return reinterpret_cast<T *>((uintptr_t) wave_uniform(lo) | ((uintptr_t) wave_uniform(hi) << 32)); }

struct W2Held {
    uint32_t group, coin_off, list_off, q_off, qcap, shade_off, bsdf_off; // v4_layout
    int eff_dim, rr_depth, max_depth;                                     // path_step_diffuse
    int exclude_direct, width, height;                                    // path_init, path_begin
    float tan_half_fov, inv_aspect, near_clip, far_clip, cam[12];
    float p_large;
    DEmitter light;
    DShade light_shade;
};
DEV W2Held w2_held(const DParams &P) {
    const V4Layout<RULE_ORBITAL> Y = v4_layout<RULE_ORBITAL>(P, V4_QCAP);
    W2Held H;
    H.group = Y.group; H.coin_off = Y.L.coin_off; H.list_off = Y.L.list_off; H.q_off = Y.L.q_off; H.qcap = Y.L.qcap;
    H.shade_off = Y.LT.shade_off; H.bsdf_off = Y.LT.bsdf_off;
    H.eff_dim = P.eff_dim; H.rr_depth = P.rr_depth; H.max_depth = P.max_depth;
    H.exclude_direct = P.exclude_direct; H.width = P.width; H.height = P.height;
    H.tan_half_fov = P.tan_half_fov; H.inv_aspect = P.inv_aspect; H.near_clip = P.near_clip; H.far_clip = P.far_clip;
#pragma unroll
    for (int i = 0; i < 12; ++i) H.cam[i] = P.cam[i];
    H.p_large = P.p_large;
    H.light = P.light; H.light_shade = P.light_shade;
    return H;
}
// pin what the loop reads of it in vector registers: an opaque definition the compiler cannot rematerialise as a scalar load
DEV void w2_hold(W2Held &H) {
    hold_v(H.group); hold_v(H.coin_off); hold_v(H.list_off); hold_v(H.q_off); hold_v(H.qcap); hold_v(H.shade_off); hold_v(H.bsdf_off);
    hold_v(H.eff_dim); hold_v(H.rr_depth); hold_v(H.max_depth); hold_v(H.exclude_direct); hold_v(H.width); hold_v(H.height);
    hold_v(H.tan_half_fov); hold_v(H.inv_aspect); hold_v(H.near_clip); hold_v(H.far_clip); hold_v(H.p_large);
#pragma unroll
    for (int i = 0; i < 12; ++i) hold_v(H.cam[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        hold_v(H.light.radiance[i]); hold_v(H.light_shade.origin[i]); hold_v(H.light_shade.eu[i]); hold_v(H.light_shade.ev[i]); hold_v(H.light_shade.n[i]);
    }
    hold_v(H.light.cdf_lo); hold_v(H.light.cdf_hi); hold_v(H.light_shade.inv_area); hold_v(H.light_shade.bsdf);
}
DEV RowSamplerT<RULE_ORBITAL> w2_sampler(uint32_t key0, uint32_t key1) { // the uniform fields, as v4_layout sets them under the orbital rule
    RowSamplerT<RULE_ORBITAL> s;
    s.key0 = key0; s.key1 = key1;
    s.mode = SM_STAGE1; s.type = 2; s.sigma2 = 0.f;
    s.stride = V4_STRIDE;
    s.x_off = s.y_off = s.xyz = 0u;
    return s;
}
// k_mutate_w2's film flush: film_put_channel and v4_flush with the box filter and the tabulated filters in two loop nests of their
// own, chosen once per flush by a wave-uniform test. Same passes, lanes, addresses, values and order of the atomics. In the shared
// routine the weight is `box ? constant : P.filter_lut[i]`; the compiler merges the arms, and the wait in front of the table value
// stands on the box path too, where no load was issued: there it waits for the no-return atomics of the previous pass, which count
// in the same vmcnt. Here the box nest reads no memory at all, so nothing in it waits for an atomic, and the tabulated nest reads
// its table from LDS (lgkmcnt): `lut` is the wave's list area (V4Lds::list_off, the 32 words v4_layout leaves between the coins
// and the queue), staged anew by every flush because the fill passes of every bookkeeping branch overwrite it. The area is free
// whenever a flush runs: the branch's flush precedes the list writes of the same call and nothing between the staging and the last
// table read writes LDS but the flush itself (it reads the queue rows only); the epilogue's flushes run after the loop. One wave
// per workgroup: the ds_write and the ds_reads of other lanes need no barrier (as lds_list's).
template <bool BOX> DEV void w2_film_put_channel(const DParams &P, const float *lut, float px, float py, float v, int ch) {
    if (P.debug & 1) return;
    float posx = px - 0.5f, posy = py - 0.5f;
    int minx = max((int) ceilf(posx - P.filter_radius), 0), miny = max((int) ceilf(posy - P.filter_radius), 0);
    int maxx = min((int) floorf(posx + P.filter_radius), P.width - 1), maxy = min((int) floorf(posy + P.filter_radius), P.height - 1);
    for (int y = miny; y <= maxy; ++y) {
        const int iy = min((int) fabsf(((float) y - posy) * P.filter_scale), 31);
        float wy = BOX ? (iy < 31 ? P.box_weight : 0.f) : lut[iy];
        for (int x = minx; x <= maxx; ++x) {
            const int ix = min((int) fabsf(((float) x - posx) * P.filter_scale), 31);
            float w = (BOX ? (ix < 31 ? P.box_weight : 0.f) : lut[ix]) * wy;
            atomic_add_global_f32(P.film + ((size_t) y * P.width + x) * 3 + ch, w * v);
        }
    }
}
template <bool BOX> DEV void w2_flush_passes(const DParams &P, const V4Lds &L, const float *lut, uint32_t qn, uint32_t lane) {
    const uint32_t s = lane / 3u, ch = lane - 3u * s;
    for (uint32_t base = 0u; base < qn; base += 21u) {
        const uint32_t e = base + s;
        if (e < qn && s < 21u) {
            const float *q = &lds_x[L.q_off + e];
            w2_film_put_channel<BOX>(P, lut, q[0], q[L.qcap], q[(2u + ch) * L.qcap], (int) ch);
        }
    }
}
DEV void w2_flush(const DParams &P, const V4Lds &L, uint32_t &qn, uint32_t lane) {
    float *const lut = &lds_x[L.list_off];
    if (P.box_weight > 0.f) w2_flush_passes<true>(P, L, lut, qn, lane);
    else if (qn) {
        // the one vector-memory load of a flush, and its one wait. The wait also covers whatever atomics the previous flush left
        // outstanding: those are about six bookkeeping calls old.
        if (lane < 32u) lut[lane] = P.filter_lut[lane];
        w2_flush_passes<false>(P, L, lut, qn, lane);
    }
    qn = 0u;
}

// the scene's ray records of k_mutate_w2<true>; k_mutate_w2<false> holds none
struct W2HeldScene {
    HeldScene S;
    uint32_t flags; // HELD_* (device_path.h): which slots are used, which cuboids lack a face, whether any record is a triangle pair
};
struct W2StreamedScene {};
// the twelve floats of a record's rows, pinned one by one, then as the vector pairs the tests read
template <class Rec> DEV void w2_hold_rows(Rec &G, const float *c, const float *rz, bool have) {
    float v[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) v[k] = 0.f;
    if (have) {
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = c[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[8 + k] = rz[k];
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) hold_v(v[k]);
    G.cx = float2v{v[0], v[1]}; G.cy = float2v{v[2], v[3]}; G.cz = float2v{v[4], v[5]}; G.cw = float2v{v[6], v[7]};
    G.z0 = v[8]; G.z1 = v[9]; G.z2 = v[10]; G.z3 = v[11];
}
// (a slot beyond the scene's count keeps zeros and is never tested; nothing past record n_box - 1 / n_flat_rec - 1 is read)
DEV W2HeldScene w2_held_scene(const DParams &P) {
    W2HeldScene H;
    const uint32_t n_box = (uint32_t) min(max(P.n_box, 0), 3), n_flat = (uint32_t) min(max(P.n_flat_rec, 0), 1);
#pragma unroll
    for (uint32_t i = 0; i < 3u; ++i) {
        BoxRec &G = H.S.box[i];
        const DPrimBox *q = P.prims_box + i;
        w2_hold_rows(G, q->c, q->rz, i < n_box);
        uint32_t f0 = 0u, f1 = 0u, f2 = 0u;
        if (i < n_box) { f0 = q->fw[0]; f1 = q->fw[1]; f2 = q->fw[2]; }
        hold_v(f0); hold_v(f1); hold_v(f2);
        G.f0 = f0; G.f1 = f1; G.f2 = f2;
    }
    FlatRec &F = H.S.flat;
    w2_hold_rows(F, P.prims_flat->c, P.prims_flat->rz, n_flat > 0u);
    int ks = -1;
    if (n_flat > 0u) ks = P.prims_flat->kind_shade;
    hold_v(ks);
    F.ks = ks;
    H.flags = held_flags(H.S, n_box, n_flat);
    hold_v(H.flags);
    return H;
}

template <bool HELD> __global__ void __launch_bounds__(CHAIN_BLOCK, 2) k_mutate_w2(DParams P, uint32_t n_mut, uint32_t mut_base) {
    typedef RowSamplerT<RULE_ORBITAL> RowSampler;
    if (threadIdx.x == 0) {
        atomicAdd(P.stats + 14, 1ull); atomicAdd(P.stats + 15, 1ull); atomicAdd(P.stats + 16, 1ull);
        if constexpr (HELD) atomicAdd(P.stats + 17, 1ull);
    }
    const uint32_t lane = threadIdx.x;
    const uint32_t sub = lane & 31u;
    const bool helper = lane >= 32u;
    const uint32_t c = blockIdx.x * 32u + sub;
    const bool live = !helper && c < P.n_chains;
    const uint32_t cc = c < P.n_chains ? c : P.n_chains - 1;
    const uint32_t S = V4_STRIDE;
    int smp_mode = SM_STAGE1;
    uint32_t roles;
    uint32_t qn = 0u;
    ChainState cs;
    float cum = 0.f;
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    PathState ps;
    bool helper_has_ray = false;
    Hit h{-1, 0.f, 0.f, 0.f};
    int batch;
    uint32_t base = 0u, target = 0u, limit = 0u;
    bool reported = false;
    W2Held held = w2_held(P);
    w2_hold(held);
    typename std::conditional<HELD, W2HeldScene, W2StreamedScene>::type scene;
    if constexpr (HELD) scene = w2_held_scene(P);
    // (W2Held's companions: what the bookkeeping branch needs in SCALAR registers, one v_readfirstlane each where it opens)
    uint32_t imp_lo = (uint32_t) (uintptr_t) P.importance, imp_hi = (uint32_t) ((uintptr_t) P.importance >> 32);
    uint32_t done_lo = (uint32_t) (uintptr_t) P.chain_done, done_hi = (uint32_t) ((uintptr_t) P.chain_done >> 32);
    uint32_t left_lo = (uint32_t) (uintptr_t) P.waves_left, left_hi = (uint32_t) ((uintptr_t) P.waves_left >> 32);
    uint32_t key0_v = P.key0, key1_v = P.key1, chain_off_v = P.chain_offset, timid_v = (uint32_t) P.timid_after_large;
    hold_v(imp_lo); hold_v(imp_hi); hold_v(done_lo); hold_v(done_hi); hold_v(left_lo); hold_v(left_hi);
    hold_v(key0_v); hold_v(key1_v); hold_v(chain_off_v); hold_v(timid_v);
    { // the prologue of k_mutate_v4
        const V4Layout<RULE_ORBITAL> Y = v4_layout<RULE_ORBITAL>(P, V4_QCAP);
        roles = RowSampler::first_roles(Y.group, sub);
        if (!helper) {
            for (uint32_t k = 0; k < Y.D; ++k) lds_x[k * S + sub] = unwrap01(P.x[(size_t) k * P.n_chains + cc]);
            for (uint32_t k = Y.D; k < Y.D4; ++k) lds_x[k * S + sub] = 0.f;
        }
        cs.cur.lum = P.cur_lum[cc]; cs.cur.px = P.cur_px[cc]; cs.cur.py = P.cur_py[cc];
        cs.cur.r = P.cur_r[cc]; cs.cur.g = P.cur_g[cc]; cs.cur.b = P.cur_b[cc];
        cs.y = cs.cur; cs.z = cs.cur;
        cs.a1 = 0.f; cs.coin_acc1 = cs.coin_acc2 = cs.coin_mix = 0.f;
        cs.it = 0u; cs.nd1 = cs.nd2 = 0u; cs.stage = -1; cs.large = false;
        path_init(P, ps);
        base = (P.chain_done && live) ? P.chain_done[cc] : mut_base;
        target = P.chain_done ? n_mut : mut_base + n_mut;
        limit = P.chain_done ? P.run_limit : target;
        ps.phase = (live && base < limit) ? PH_DONE : PH_IDLE;
        ps.o = mk3(0.f, 0.f, 0.f); ps.d = mk3(0.f, 0.f, 1.f); ps.tmin = 0.f; ps.tmax = 0.f;
        batch = P.mh_batch > 32 ? 32 : P.mh_batch;
        stage_tables(P, Y.LT, lane);
        if (!helper) {
            const u4 coins = philox4x32_10(P.key0, P.key1, 0u, base, P.chain_offset + blockIdx.x * 32u + sub, TAG_COIN);
            float *dst = &lds_x[Y.L.coin_off + sub];
            dst[0] = u32_to_unit(coins.x); dst[S] = u32_to_unit(coins.y); dst[2u * S] = u32_to_unit(coins.z); dst[3u * S] = u32_to_unit(coins.w);
        }
    }

    for (;;) {
        const bool parked = ps.phase == PH_DONE;
        const unsigned long long pmask = __ballot(parked);
        const unsigned long long rmask = __ballot(ps.phase != PH_DONE && ps.phase != PH_IDLE);
        if (!pmask && !rmask) break;
        const bool book = pmask && (__popcll(pmask) >= batch || !rmask);
        // w2h expects the branch to be skipped -- about two iterations in three skip it --, and the compiler then lays the ray pass
        // directly behind the loop head and the branch's thousand instructions behind the hand-off: the common iteration falls through.
        // (k_mutate_w2 keeps the plain test, `if (pmask && (__popcll(pmask) >= batch || !rmask))`, and the layout it gives.)
        if (HELD ? __builtin_expect(book, 0) : book) {
            // the branch's scalars: what steers wave-uniform branches, loop bounds and scalar addresses (importance, timid_after_large,
            // eff_dim, chain_done, waves_left) and the Philox keys -- one block for the whole branch
            DParams Pm{};
            Pm.importance = uniform_ptr<const float>(imp_lo, imp_hi); Pm.width = (int) wave_uniform((uint32_t) held.width); Pm.height = (int) wave_uniform((uint32_t) held.height);
            Pm.chain_done = uniform_ptr<uint32_t>(done_lo, done_hi); Pm.waves_left = uniform_ptr<uint32_t>(left_lo, left_hi);
            Pm.key0 = wave_uniform(key0_v); Pm.key1 = wave_uniform(key1_v); Pm.chain_offset = wave_uniform(chain_off_v);
            Pm.eff_dim = (int) wave_uniform((uint32_t) held.eff_dim); Pm.timid_after_large = (int) wave_uniform(timid_v);
            Pm.use_mixture = 0; Pm.acceptance_map = 0; Pm.type = 2; // (the orbital rule: mh_decide<RULE_ORBITAL> reads none of them)
            const W2Held &C = held;
            const V4Lds L{C.coin_off, C.list_off, C.q_off, C.qcap};
            RowSampler smp = w2_sampler(Pm.key0, Pm.key1);
            smp.set_roles(roles, C.group, sub); smp.mode = smp_mode;
            const uint32_t D4 = ((uint32_t) Pm.eff_dim + 3u) & ~3u, nb1 = D4 / 4u;
            int *const lds_list = reinterpret_cast<int *>(&lds_x[L.list_off]);
            __builtin_amdgcn_s_setprio(2);
            if (qn + 64u > wave_uniform(L.qcap)) { SECTION_PARAMS(Pf); w2_flush(Pf, L, qn, lane); }
            // ---- decide (parked chain lanes). HELD: by selects, no arm behind a divergent branch (w2h_decide); else as k_mutate_v4
            int commit = 0, kind = 0; // kind: 0 nothing / finished, 1 next mutation, 2 second stage
            W2hQueued qa{false, 0.f, 0.f, 0.f, 0.f, 0.f}, qb{false, 0.f, 0.f, 0.f, 0.f, 0.f};
            if constexpr (HELD) w2h_decide(Pm, parked, cs, ps, ct, cum, commit, kind, qa, qb);
            else if (parked) { // as k_mutate_v4: slot A = the current state when it is left, else y; slot B = y when z is adopted, else z
                const MhDigest o = mh_decide<RULE_ORBITAL>(Pm, cs, smp, ps, ct);
                if (o.decided) {
                    cum += o.w.w0;
                    const bool a1st = o.acc1, a2nd = o.acc2, adopt = a1st || a2nd;
                    const DSplat sb = select_splat(a2nd, cs.y, cs.z);
                    const float wb = a2nd ? o.w.w1 : o.w.w2;
                    qb.want = !a1st && wb > 0.f;
                    qb.px = sb.px; qb.py = sb.py; qb.r = sb.r * wb; qb.g = sb.g * wb; qb.b = sb.b * wb;
                    const DSplat sa = select_splat(adopt, cs.cur, cs.y);
                    const float wa = adopt ? cum : o.w.w1;
                    qa.want = wa > 0.f;
                    qa.px = sa.px; qa.py = sa.py; qa.r = sa.r * wa; qa.g = sa.g * wa; qa.b = sa.b * wa;
                    if (adopt) {
                        cum = a1st ? o.w.w1 : o.w.w2;
                        cs.cur = select_splat(a1st, cs.y, cs.z);
                    }
                    commit = mh_commit_mode(o);
                }
                kind = cs.stage < 0 ? 4 : 2; // 4: between mutations -- resolved below
            }
            kind = mh_resolve_kind(Pm, kind, live, base + cs.it, target, limit, reported, lane);
            v4_enqueue(L, qn, qa.want, qa.px, qa.py, qa.r, qa.g, qa.b);
            v4_enqueue(L, qn, qb.want, qb.px, qb.py, qb.r, qb.g, qb.b);


            // ---- commit: the chosen proposal's row group becomes the chain's x group
            smp.adopt(commit);
            roles = smp.roles();

            // ---- start (parked chain lanes): the coins of the mutation that begins were drawn with the previous one
            if (parked && kind == 1) {
                const float *cn = &lds_x[L.coin_off + sub];
                cs.large = cn[0] < C.p_large;
                cs.coin_acc1 = cn[S]; cs.coin_acc2 = cn[2u * S]; cs.coin_mix = cn[3u * S];
                cs.stage = 0;
                cs.nd1 = cs.nd2 = 0u;
            }

            // ---- proposals of the chains that start a mutation, flattened; block nb1 = the four coins of the NEXT mutation
            RowSampler smg = w2_sampler(Pm.key0, Pm.key1);
            const uint32_t chain_base_g = Pm.chain_offset + blockIdx.x * 32u;
            const uint32_t maj_mine = base + cs.it;
            const unsigned info = roles | (cs.large ? 1u : 0u);
            const uint32_t f1mask = (uint32_t) __ballot(kind == 1);
            if constexpr (HELD) {
                // w2h: ONE flattened pass. Items [0, t1) are the first-stage and coin items of the n1 chains that start a mutation, in
                // k_mutate_w2's mapping (block b, chain j); behind them come the second-stage items of the n2 chains whose first stage
                // was rejected -- typically one chain --, ONE PAIR each: item q = 4 b + p of chain j is pair p of Philox block b, so that
                // they ride in the empty lanes of the last trip and the wave pays one rotation for them, not four. The list holds the
                // first kind's columns in [0, n1) and the second's behind them (a chain has one kind: n1 + n2 <= 32). An item draws
                // ONE Philox block at an address selected per lane (the four pairs of a block draw it four times: the lanes are
                // there); what it does with the uniforms is its tail, and the second-stage tail (row_fill_second_pair_drawn) is
                // entered only by a trip that holds such an item.
                const uint32_t f2mask = (uint32_t) __ballot(kind == 2);
                if (f1mask | f2mask) {
                    const uint32_t n1 = (uint32_t) __popc(f1mask), n2 = (uint32_t) __popc(f2mask);
                    if (kind == 1 || kind == 2) lds_list[kind == 1 ? __builtin_amdgcn_mbcnt_lo(f1mask, 0u) : n1 + __builtin_amdgcn_mbcnt_lo(f2mask, 0u)] = (int) sub;
                    const uint32_t nb2 = Pm.timid_after_large ? D4 / 4u : (D4 / 2u + 3u) / 4u;
                    const uint32_t t1 = n1 * (nb1 + 1u), total = t1 + n2 * 4u * nb2;
                    for (uint32_t fb = 0u; fb < total; fb += 64u) {
                        const uint32_t i = fb + lane;
                        const bool valid = i < total, second = valid && i >= t1;
                        const uint32_t ii = valid ? (second ? i - t1 : i) : 0u, n = second ? n2 : n1;
                        // (the reciprocal per lane, by v_rcp: (ii + 0.5) / n is at least 1/64 from a whole number, one ulp does not move its
                        // floor, and a select between two quotients made in front of the loop compiles to a full division in every trip.
                        // n == 0 only on lanes without an item)
                        const uint32_t q = (uint32_t) (((float) ii + 0.5f) * __builtin_amdgcn_rcpf((float) n)), j = ii - q * n;
                        const uint32_t b = second ? q >> 2 : q;
                        const uint32_t cj = (uint32_t) lds_list[second ? n1 + j : j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        smg.set_roles(inf, C.group, cj);
                        const bool coin = !second && b >= nb1;
                        Unit4 u{{0.f, 0.f, 0.f, 0.f}};
                        if (valid) {
                            const u4 r = philox4x32_10(Pm.key0, Pm.key1, coin ? 0u : b, coin ? mj + 1u : mj, chain_base_g + cj, coin ? TAG_COIN : (second ? TAG_S2 : TAG_S1));
                            u = Unit4{{u32_to_unit(r.x), u32_to_unit(r.y), u32_to_unit(r.z), u32_to_unit(r.w)}};
                            if (!second) {
                                if (!coin) row_fill_first_drawn(smg, b, u, (inf & 1u) != 0u);
                                else {
                                    float *dst = &lds_x[L.coin_off + cj];
                                    dst[0] = u.v[0]; dst[S] = u.v[1]; dst[2u * S] = u.v[2]; dst[3u * S] = u.v[3];
                                }
                            }
                        }
                        if (__ballot(second)) {
                            if (second) row_fill_second_pair_drawn(smg, b, q & 3u, D4, u, (inf & 1u) != 0u);
                        }
                    }
                }
            } else {
                if (f1mask) {
                    if (kind == 1) lds_list[__builtin_amdgcn_mbcnt_lo(f1mask, 0u)] = (int) sub;
                    const uint32_t n = (uint32_t) __popc(f1mask), total = n * (nb1 + 1u);
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t fb = 0u; fb < total; fb += 64u) {
                        const uint32_t i = fb + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        smg.set_roles(inf, C.group, cj);
                        const bool coin = b >= nb1;
                        if (valid) {
                            const u4 r = philox4x32_10(Pm.key0, Pm.key1, coin ? 0u : b, coin ? mj + 1u : mj, chain_base_g + cj, coin ? TAG_COIN : TAG_S1);
                            const Unit4 u{{u32_to_unit(r.x), u32_to_unit(r.y), u32_to_unit(r.z), u32_to_unit(r.w)}};
                            if (!coin) row_fill_first_drawn(smg, b, u, (inf & 1u) != 0u);
                            else {
                                float *dst = &lds_x[L.coin_off + cj];
                                dst[0] = u.v[0]; dst[S] = u.v[1]; dst[2u * S] = u.v[2]; dst[3u * S] = u.v[3];
                            }
                        }
                    }
                }
                const uint32_t f2mask = (uint32_t) __ballot(kind == 2);
                if (f2mask) { // second-stage proposals (rare: rejected bold steps)
                    if (kind == 2) lds_list[__builtin_amdgcn_mbcnt_lo(f2mask, 0u)] = (int) sub;
                    const uint32_t nb2 = Pm.timid_after_large ? D4 / 4u : (D4 / 2u + 3u) / 4u;
                    const uint32_t n = (uint32_t) __popc(f2mask), total = n * nb2;
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t fb = 0u; fb < total; fb += 64u) {
                        const uint32_t i = fb + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        smg.set_roles(inf, C.group, cj);
                        if (valid) smg.fill_second(b, D4, mj, chain_base_g + cj, (inf & 1u) != 0u);
                    }
                }
            }

            // ---- begin the evaluation (parked chain lanes): film position and camera ray from the first two components
            if (parked) {
                if (kind == 0) ps.phase = PH_IDLE;
                else {
                    DParams Vb{}; // what path_init and path_begin read of the block
                    Vb.exclude_direct = C.exclude_direct; Vb.width = C.width; Vb.height = C.height;
                    Vb.tan_half_fov = C.tan_half_fov; Vb.inv_aspect = C.inv_aspect; Vb.near_clip = C.near_clip; Vb.far_clip = C.far_clip;
#pragma unroll
                    for (int q = 0; q < 12; ++q) Vb.cam[q] = C.cam[q];
                    smp_mode = smp.mode = cs.stage == 0 ? SM_STAGE1 : SM_STAGE2;
                    path_init(Vb, ps);
                    const float v0 = smp.next(0u), v1 = smp.next(1u);
                    path_begin(Vb, ps, v0, v1);
                }
            }
        }
        // one ray per lane: chain lanes their camera / bounce ray, helpers the shadow ray they were handed. When any lane has a ray
        // the whole wave runs the pass, whatever its lanes hold: registers in, registers out, and only lanes that traced read `h`
        // (a PH_FLUSH step reads hit.prim, a record's index or -1, and selects everything else away).
        // (w2h forms the wave's test from the two compare masks: helper_has_ray is false on every chain lane, and a helper's phase
        // is PH_IDLE from the prologue on, so `or` is the select)
        const bool tracing = HELD ? (helper_has_ray || ps.phase == PH_CLOSEST) : (helper ? helper_has_ray : ps.phase == PH_CLOSEST);
        __builtin_amdgcn_s_setprio(0);
        if constexpr (HELD) {
            if (__builtin_amdgcn_ballot_w64(tracing) != 0ull) h = trace_held(scene.S, wave_uniform(scene.flags), ps.o, ps.d, ps.tmin, ps.tmax);
        } else {
            SECTION_PARAMS(Pt);
            if (__ballot(tracing)) h = trace<0>(Pt, ps.o, ps.d, ps.tmin, ps.tmax, helper);
        }
        __builtin_amdgcn_s_setprio(3);
        unsigned occluded;
        if constexpr (HELD) { // (only chain lanes read it: the swap's other operand is whatever a register holds, not a copy of the flag)
            unsigned any_v;
            asm volatile("" : "=v"(any_v));
            occluded = __builtin_amdgcn_permlane32_swap((helper_has_ray && h.prim >= 0) ? 1u : 0u, any_v, false, false)[1];
        } else occluded = from_upper_u((helper_has_ray && h.prim >= 0) ? 1u : 0u);
        helper_has_ray = false;
        ShadowRay sr;
        asm volatile("" : "=v"(sr.d.x), "=v"(sr.d.y), "=v"(sr.d.z), "=v"(sr.tmin), "=v"(sr.tmax)); // whatever the registers hold: read under sr.valid only
        sr.o = ps.o; sr.valid = false;
        {
            // no scalar load at the head of the step; its LDS reads still leave in three dependent trips (components, shading record, BSDF)
            const W2Held &Cs = held;
            if (!helper && ps.phase != PH_DONE && ps.phase != PH_IDLE) {
                RowSampler sms = w2_sampler(0u, 0u);
                sms.set_roles(roles, Cs.group, sub); sms.mode = smp_mode;
                DParams Vs{}; // what path_step_diffuse reads of the block
                Vs.eff_dim = Cs.eff_dim; Vs.rr_depth = Cs.rr_depth; Vs.max_depth = Cs.max_depth;
                const LdsTables LT{Cs.shade_off, Cs.bsdf_off, 0u}; // (the emitter table is not read: HeldLightTables)
                // (RARE_EMITTER_HIT = HELD: w2h runs the emitter-hit block only in an iteration in which a bounce ray hit the light)
                // (HeldLightTablesT<HELD>: every scene w2h is launched on has a rectangle light -- device_path.h has the argument)
                typedef HeldLightTablesT<HELD> LightTables;
                path_step_diffuse<RowSampler, LightTables, false, HELD>(Vs, LightTables{LT, Cs.light, Cs.light_shade}, ps, sms, h, occluded == 0u, sr);
            }
        }
        // hand the shadow ray of this vertex to the helper lane
        if constexpr (HELD) {
            // w2h: a swap writes both its operands, and the shadow ray starts where the bounce ray does -- one register, which needs a
            // copy to be swapped with itself. The three copies stand here, ahead of the block of swaps, and the origin's swaps come last,
            // behind the direction's and the interval's, so that no copy is followed at once by the swap that reads it (gfx950 then
            // wants two idle states in between). The helper's flag is made a 0 / 1 word ahead of the copies for the same reason.
            // (`kept`: what a chain lane keeps of the flag is never read, so the swap's other operand is whatever a register holds, no
            // zero made for it -- named here, so that it is no register a swap has just written)
            unsigned valid01 = sr.valid ? 1u : 0u, kept;
            hold_v(valid01);
            asm volatile("" : "=v"(kept));
            float gx = sr.o.x, gy = sr.o.y, gz = sr.o.z;
            hold_v(gx); hold_v(gy); hold_v(gz);
            ps.d.x = lower_keeps(ps.d.x, sr.d.x); ps.d.y = lower_keeps(ps.d.y, sr.d.y); ps.d.z = lower_keeps(ps.d.z, sr.d.z);
            ps.tmin = lower_keeps(ps.tmin, sr.tmin); ps.tmax = lower_keeps(ps.tmax, sr.tmax);
            ps.o.x = lower_keeps(ps.o.x, gx); ps.o.y = lower_keeps(ps.o.y, gy); ps.o.z = lower_keeps(ps.o.z, gz);
            // (`helper` selects the flag, a scalar `and` of two masks -- not `&&`, which would put the swap behind the helpers' exec mask)
            const bool handed = lower_keeps_u(kept, valid01) != 0u;
            helper_has_ray = helper & handed;
        } else {
        ps.o.x = lower_keeps(ps.o.x, sr.o.x); ps.o.y = lower_keeps(ps.o.y, sr.o.y); ps.o.z = lower_keeps(ps.o.z, sr.o.z);
        ps.d.x = lower_keeps(ps.d.x, sr.d.x); ps.d.y = lower_keeps(ps.d.y, sr.d.y); ps.d.z = lower_keeps(ps.d.z, sr.d.z);
        ps.tmin = lower_keeps(ps.tmin, sr.tmin); ps.tmax = lower_keeps(ps.tmax, sr.tmax);
        helper_has_ray = lower_keeps_u(0u, sr.valid ? 1u : 0u) != 0u; // (a chain lane keeps the `false` set above)
        }
    }
    // the epilogue of k_mutate_v4, on its own copy of the block; the last splat goes through this kernel's flush, called here by name
    // (the tests of the build find a flush's instructions by the kernel's line that called it)
    SECTION_PARAMS(Pe);
    const V4Layout<RULE_ORBITAL> Y = v4_layout<RULE_ORBITAL>(Pe, V4_QCAP);
    if (qn + 32u > Y.L.qcap) w2_flush(Pe, Y.L, qn, lane);
    v4_enqueue(Y.L, qn, live && cum > 0.f, cs.cur.px, cs.cur.py, cs.cur.r * cum, cs.cur.g * cum, cs.cur.b * cum);
    w2_flush(Pe, Y.L, qn, lane);
    if (live) {
        RowSampler smp = Y.smp;
        smp.set_roles(roles, Y.group, sub);
        for (uint32_t k = 0; k < Y.D; ++k) Pe.x[(size_t) k * Pe.n_chains + c] = smp.x(k);
        Pe.cur_lum[c] = cs.cur.lum; Pe.cur_px[c] = cs.cur.px; Pe.cur_py[c] = cs.cur.py;
        Pe.cur_r[c] = cs.cur.r; Pe.cur_g[c] = cs.cur.g; Pe.cur_b[c] = cs.cur.b;
        if (Pe.chain_done) Pe.chain_done[c] = base + cs.it;
    }
    if (Pe.chain_done && !reported && lane == 0) atomicSub(Pe.waves_left, 1u);
    flush_counters(Pe, ct, lane);
    const unsigned long long decided = wave_sum((live && !helper) ? cs.it : 0u);
    if (lane == 0) atomicAdd(Pe.stats + 9, decided);
}

// k_mutate_v4 <FEAT, LDS_TABLES, STAMPS, STACK16, OVF>: lane pairs, 32 chains per wave
// (LAUNCH_RULE: the orbital twin of the build when the context's rule is the orbital one; LAUNCH_LIGHT: of either, the
// one-light twin when the scene has one light)
void launch_mutate_v4(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st) {
#define LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(plan.grid), dim3(CHAIN_BLOCK), plan.lds, st, P, n_mut, mut_base); break
#define LAUNCH_RULE(FEAT, ...) if (orbital) { LAUNCH(k_mutate_v4<FEAT | V4_ORBITAL_BUILD, __VA_ARGS__>); } LAUNCH(k_mutate_v4<FEAT, __VA_ARGS__>)
#define LAUNCH_LIGHT(...) if (one_light) { LAUNCH_RULE(V4_ONE_LIGHT_BUILD, __VA_ARGS__); } LAUNCH_RULE(0, __VA_ARGS__)
    const bool orbital = rule_is_orbital(P), one_light = scene_has_one_light(P);
    switch (plan.build) {
    case Build::V4_F0_STAMPS: LAUNCH_LIGHT(true, true);
    case Build::V4_F0: // (k_mutate_w2: the orbital one-light twin for launches without a third wave per SIMD -- plan.w2, launch_plan.h)
        if (plan.w2_held && orbital && one_light) { LAUNCH(k_mutate_w2<true>); } // (its ray records in registers: plan.w2_held)
        if (plan.w2 && orbital && one_light) { LAUNCH(k_mutate_w2<false>); }
        LAUNCH_LIGHT(true, false);
    case Build::V4_F3_STAMPS: LAUNCH(k_mutate_v4<3, true, true>); case Build::V4_F3: LAUNCH_RULE(3, true, false); case Build::V4_F7: LAUNCH_RULE(7, true, false);
    case Build::V4_F15_S32: LAUNCH(k_mutate_v4<15, true, false, false, true>); case Build::V4_F15_OVF: LAUNCH(k_mutate_v4<15, true, false, true, true>);
    case Build::V4_F15: LAUNCH(k_mutate_v4<15, true, false, true>);            case Build::V4_F7_GLOBAL: LAUNCH(k_mutate_v4<7, false, false>);
    case Build::V4_F8_S32_GLOBAL: LAUNCH(k_mutate_v4<8, false, false, false, true>); case Build::V4_F15_S32_GLOBAL: LAUNCH(k_mutate_v4<15, false, false, false, true>);
    case Build::V4_F15_OVF_GLOBAL: LAUNCH(k_mutate_v4<15, false, false, true, true>); case Build::V4_F15_STAMPS_GLOBAL: LAUNCH(k_mutate_v4<15, false, true, true>);
    case Build::V4_F8_GLOBAL: LAUNCH(k_mutate_v4<8, false, false, true>);            case Build::V4_F15_GLOBAL: LAUNCH(k_mutate_v4<15, false, false, true>);
    default:
        fprintf(stderr, "[drmlt] launch_mutate_v4: build %d is not a k_mutate_v4 build\n", (int) plan.build);
        abort();
    }
#undef LAUNCH_LIGHT
#undef LAUNCH_RULE
#undef LAUNCH
}

// ------------------------------------------------------------------------------------------
// k_mutate_v5: the chain loop with MORE RAYS THAN LANES (all three types).
//
// In k_mutate_v4 a ray belongs to a lane: chain lane i traverses its camera / bounce ray, helper lane 32 + i the shadow ray
// of the same vertex. On a scene that is traversed (not looped over) the wave then advances ~22 of its 64 lanes per node
// iteration: helpers mostly have no ray (no NEE at a vertex, the path parked or in its bookkeeping), chains wait for their
// partner, and a slice drains towards its longest ray. Here rays and lanes are decoupled:
//   * 64 chains per wave, chain c = lane c for everything that is per chain (path state, acceptance logic);
//   * every ray a path step issues -- the bounce ray and, beside it, the shadow ray of the same vertex -- goes into a RAY POOL
//     in LDS (slot c: chain c's closest-hit ray, slot 64 + c: its shadow ray; origin, direction, interval; the result is
//     written over the record) and its slot number into a FIFO of pending rays, appended with ballot + prefix count
//     (wave-level compaction of the lanes that have something to add);
//   * the traversal loop runs over whatever rays the pool holds: a lane whose traversal finishes writes the result to the
//     slot, and the idle lanes take the next pending slots off the queue (ballot + prefix count again) INSIDE the loop; a
//     phase ends when the pool is dry or `trace_yield` closest-hit rays have finished -- their chains then step (any lane
//     whose chain has its results) and refill the pool.
// With 64 chains a wave holds ~75-80 rays, so the queue keeps the lanes fed until a phase is nearly over.
//
// LDS (20 KB per wave = eight waves per CU = two per SIMD with 131 072 chains): v4's three row groups (x, y, z: 3 x 9 KB for
// 64 chains) cannot sit beside the pool. The CURRENT STATE x therefore stays at home in device memory ([dim][chain], the
// layout it has between launches anyway): it is read when a mutation's proposal is made (flattened over the wave, chain-minor:
// partly coalesced 256 B rows) and written when a proposal is adopted -- SURVEY 8(d)'s B_state, now real traffic (~250 B per
// mutation, L2 / MALL resident). LDS holds ONE row group: the proposal under evaluation -- y, overwritten in place by z when a
// chain enters its second stage. The orbital rule needs only the luminances of y afterwards; Green's reverse move and Mira's
// ratio need x, y and z together and RECOMPUTE what the rows no longer hold from the state and the addressed stream (Green:
// v5_iid_second_again, flattened; Mira: PoolRowSampler::y_raw, per deciding lane -- a twentieth of the mutations get that far;
// the rows, the sampler and the fill routines: device_sampler.h).
// Bookkeeping is v4's: decide per lane, commit / proposals / coins flattened over the 64 lanes. Same addressed draws, same arithmetic per component: the same chains.
// (V5_QCAP, V5_QCAP_STACK32, V5_SLOTS, v5_lds_bytes: launch_plan.h)
#define V5_STACK32_CAP 25 // (no splat queue, coins drawn per lane instead of kept in four rows: 28 rows of 256 B for the column; measured on 50 000 /
                          // 1 000 000 triangles: 11 entries 2.23e8 / 5.65e7, 16 2.48e8 / 7.03e7, 20 2.69e8 / 7.62e7)
#ifndef V5_ROWS_MEM_WAVES
#define V5_ROWS_MEM_WAVES 3 // waves per SIMD the ROWS_MEM builds are compiled for (registers) and sized for (LDS)
#endif
#ifndef V5_ROWS_MEM_STACK32_CAP
#define V5_ROWS_MEM_STACK32_CAP 25 // as the rows-in-LDS build (larger columns cost the twelfth wave: LDS is granted in steps)
#endif
enum { RS_IDLE = 0, RS_BUSY = 1, RS_DONE = 2 };

struct V5Lds {
    uint32_t coin_off, list_off; // 4 rows of coins (one mutation ahead), the compacted chain list of the bookkeeping branch
    uint32_t q_off;              // splat queue: 5 rows of V5_QCAP floats
    uint32_t pool_off;           // ray pool: 8 rows of V5_SLOTS floats (ox oy oz dx dy dz tmin tmax; result over rows 0..3)
    uint32_t ring_off;           // pending slots, FIFO: V5_SLOTS bytes
    uint32_t status_off;         // RS_* per slot: V5_SLOTS bytes
};
DEV V5Lds v5_layout(uint32_t D, uint32_t qcap, bool coin_rows) {
    V5Lds L;
    L.coin_off = D * 64u;
    L.list_off = L.coin_off + (coin_rows ? 4u * 64u : 0u);
    L.q_off = L.list_off + 64u;
    L.pool_off = L.q_off + 5u * qcap;
    L.ring_off = L.pool_off + 8u * V5_SLOTS;
    L.status_off = L.ring_off + V5_SLOTS / 4u;
    return L;
}

// FEAT & 8 (BVH scenes): the traversal loop described above. Flat scenes (FEAT without bit 3; LDS_TABLES: their shading /
// BSDF / emitter tables staged in LDS) run the same kernel with the wave-uniform brute-force loop as their "trace phase":
// up to 64 rays off the queue per pass, every one of them done when the pass ends -- so nearly all 64 chains step together
// (k_mutate_v4 steps at most its 32 chain lanes; the helper lanes idle through the path step).
// ROWS_MEM (chains for more than two waves per SIMD; traversed scenes and flat ones with their tables in LDS): proposal rows in device
// memory (RowsMem), registers for three waves (the flat builds need 169 - 179 as they are: 0 - 4 spilled).
template <int FEAT, bool STACK16, bool OVF, bool STAMPS = false, bool LDS_TABLES = false, bool ROWS_MEM = false>
__global__ void __launch_bounds__(CHAIN_BLOCK, ROWS_MEM ? V5_ROWS_MEM_WAVES : 2) k_mutate_v5(DParams P, uint32_t n_mut, uint32_t mut_base) {
    constexpr bool FLAT = (FEAT & 8) == 0;
    typedef typename std::conditional<ROWS_MEM, RowsMem, RowsLds>::type RowsT;
    typedef PoolRowSampler<RowsT> SamplerT;
    constexpr uint32_t QCAP = (FLAT || STACK16) ? V5_QCAP : V5_QCAP_STACK32;
    constexpr bool COIN_ROWS = FLAT || STACK16; // coins drawn one mutation ahead by the flattened proposal pass (else: per lane, when a mutation starts)
    // per-section copies of the parameter block, read through a kernarg pointer the compiler cannot see through (see k_mutate_v4):
    // the fields a section uses are scalar loads at its head and dead at its end, instead of ~200 spilled scalar registers
    SECTION_PARAMS(P0);
    const uint32_t lane = threadIdx.x;
    const uint32_t wave_base = blockIdx.x * 64u;
    const uint32_t c = wave_base + lane;
    const bool live = c < P0.n_chains;
    const uint32_t cc = live ? c : P0.n_chains - 1;
    const uint32_t D = (uint32_t) P0.eff_dim, nb1 = (D + 3u) / 4u;
    const V5Lds L = v5_layout(ROWS_MEM ? 0u : D, QCAP, COIN_ROWS);
    const V4Lds Lq{0u, 0u, L.q_off, QCAP};
    unsigned char *const ring = reinterpret_cast<unsigned char *>(&lds_x[L.ring_off]);
    unsigned char *const status = reinterpret_cast<unsigned char *>(&lds_x[L.status_off]);
    int *const lds_list = reinterpret_cast<int *>(&lds_x[L.list_off]);
    float *const pool = &lds_x[L.pool_off];
    status[lane] = RS_IDLE; status[64u + lane] = RS_IDLE;
    LdsTables LT;
    LT.shade_off = L.status_off + V5_SLOTS / 4u;
    LT.bsdf_off = LT.shade_off + (uint32_t) P0.n_shade * 16u;
    LT.emit_off = LT.bsdf_off + (uint32_t) P0.n_bsdfs * 12u;
    if (LDS_TABLES) stage_tables(P0, LT, lane);
    // traversed scenes: BSDF / emitter records and the emitters' shape records behind the pool when the launcher found room for them
    HybridTables HT;
    HT.L.shade_off = L.status_off + V5_SLOTS / 4u;
    HT.L.bsdf_off = HT.L.shade_off + (uint32_t) P0.n_emitters * 16u;
    HT.L.emit_off = HT.L.bsdf_off + (uint32_t) P0.n_bsdfs * 12u;
    HT.lds = !FLAT && P0.small_tables_lds != 0;
    if (HT.lds) stage_bsdfs_emitters(P0, HT.L, lane);

    ChainState cs;
    cs.cur.lum = P0.cur_lum[cc]; cs.cur.px = P0.cur_px[cc]; cs.cur.py = P0.cur_py[cc];
    cs.cur.r = P0.cur_r[cc]; cs.cur.g = P0.cur_g[cc]; cs.cur.b = P0.cur_b[cc];
    cs.y = cs.cur; cs.z = cs.cur;
    cs.a1 = 0.f; cs.coin_acc1 = cs.coin_acc2 = cs.coin_mix = 0.f;
    cs.it = 0u; cs.nd1 = cs.nd2 = 0u; cs.stage = -1; cs.large = false;
    float cum = 0.f; // weight of the current state since it was adopted (one splat per residence, as k_mutate_v4)
    uint32_t qn = 0u;
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    RowsT rows;
    if constexpr (ROWS_MEM) { rows.base = (RowsMem::GPtr) (uintptr_t) (P0.rows + wave_base); rows.stride = P0.n_chains; }
    SamplerT smp{lane, rows};

    PathState ps;
    path_init(P0, ps);
    ps.o = mk3(0.f, 0.f, 0.f); ps.d = mk3(0.f, 0.f, 1.f); ps.tmin = 0.f; ps.tmax = 0.f;
    // run-ahead between the launches of a call: as k_mutate_v4 (chain_done / waves_left / run_limit)
    const uint32_t base = (P0.chain_done && live) ? P0.chain_done[cc] : mut_base;
    const uint32_t target = P0.chain_done ? n_mut : mut_base + n_mut;
    const uint32_t limit = P0.chain_done ? P0.run_limit : target;
    bool reported = false;
    ps.phase = (live && base < limit) ? PH_DONE : PH_IDLE;
    const int batch = P0.mh_batch > 64 ? 64 : P0.mh_batch;
    if (COIN_ROWS) { // coins of every chain's first mutation of this launch (afterwards they are drawn one mutation ahead, beside the proposal)
        const u4 coins = philox4x32_10(P0.key0, P0.key1, 0u, base, P0.chain_offset + cc, TAG_COIN);
        float *dst = &lds_x[L.coin_off + lane];
        dst[0] = u32_to_unit(coins.x); dst[64] = u32_to_unit(coins.y); dst[128] = u32_to_unit(coins.z); dst[192] = u32_to_unit(coins.w);
    }

    // traversal: this lane's column of the stack, the ray it is working on (`slot`), the FIFO of pending slots
    typedef typename std::conditional<STACK16, short, int>::type StackT;
    constexpr int CAP = STACK16 ? BVH_STACK : (ROWS_MEM ? V5_ROWS_MEM_STACK32_CAP : V5_STACK32_CAP);
    __shared__ StackT v5_stack[FLAT ? 1 : (CAP + 3) * 64];
    StackT *const my_stack = v5_stack + (FLAT ? 0u : lane);
    Trav T;
    T.active = false; T.cur = 0; T.sp = 0; T.ovf = 0; T.rx = T.ry = T.rz = 0u; T.any_hit = false; T.h = Hit{-1, 0.f, 0.f, 0.f}; T.tmin = 0.f;
    T.o = T.d = T.inv = T.oi = mk3(0.f, 0.f, 0.f);
    trav_reset_counters(T);
    uint32_t slot = 0u;
    uint32_t q_head = 0u, q_count = 0u; // wave-uniform
    unsigned long long n_phase = 0ull, n_refill = 0ull, n_lanes_at_start = 0ull;
    unsigned long long t_mh = 0ull, t_step = 0ull, t_trace = 0ull, n_outer = 0ull, n_mh = 0ull, n_stepping = 0ull, n_parked = 0ull;
#define STAMP5() (STAMPS ? __builtin_amdgcn_s_memtime() : 0ull)
    auto prefix = [](unsigned long long m) { return __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u)); };

    // a ray goes into the pool slot of its chain (slot c: closest hit, 64 + c: shadow) and the slot number into the FIFO: ray
    // compaction by ballot + prefix count over the lanes that issued one
    auto push_rays = [&](bool push_c, bool push_s, const ShadowRay &sr) {
        if (push_c) {
            float *r = pool + lane;
            r[0] = ps.o.x; r[V5_SLOTS] = ps.o.y; r[2u * V5_SLOTS] = ps.o.z; r[3u * V5_SLOTS] = ps.d.x; r[4u * V5_SLOTS] = ps.d.y; r[5u * V5_SLOTS] = ps.d.z;
            r[6u * V5_SLOTS] = ps.tmin; r[7u * V5_SLOTS] = ps.tmax;
            status[lane] = RS_BUSY;
        }
        if (push_s) {
            float *r = pool + 64u + lane;
            r[0] = sr.o.x; r[V5_SLOTS] = sr.o.y; r[2u * V5_SLOTS] = sr.o.z; r[3u * V5_SLOTS] = sr.d.x; r[4u * V5_SLOTS] = sr.d.y; r[5u * V5_SLOTS] = sr.d.z;
            r[6u * V5_SLOTS] = sr.tmin; r[7u * V5_SLOTS] = sr.tmax;
            status[64u + lane] = RS_BUSY;
        }
        // ray compaction: the lanes that issued a ray append its slot to the FIFO (ballot + prefix count)
        const unsigned long long mc = __ballot(push_c);
        if (push_c) ring[(q_head + q_count + prefix(mc)) & (V5_SLOTS - 1u)] = (unsigned char) lane;
        q_count += (uint32_t) __popcll(mc);
        const unsigned long long ms = __ballot(push_s);
        if (push_s) ring[(q_head + q_count + prefix(ms)) & (V5_SLOTS - 1u)] = (unsigned char) (64u + lane);
        q_count += (uint32_t) __popcll(ms);
    };

    for (;;) {
        {
            const unsigned long long pm = __ballot(ps.phase == PH_DONE), rm = __ballot(ps.phase != PH_DONE && ps.phase != PH_IDLE);
            if (!pm && !rm) break;
        }
        if (STAMPS) n_outer++;
        auto do_step = [&]() {
            const unsigned long long t0 = STAMP5();
            // ---------------------------------------------------------------- step: chains whose ray results are in
            {
                SECTION_PARAMS(Ps);
                const int st_c = status[lane], st_s = status[64u + lane];
                const bool ready = (ps.phase == PH_CLOSEST && st_c == RS_DONE && st_s != RS_BUSY) || (ps.phase == PH_FLUSH && st_s != RS_BUSY);
                bool push_c = false, push_s = false;
                if (STAMPS) n_stepping += (unsigned long long) __popcll(__ballot(ready));
                ShadowRay sr;
                sr.o = ps.o; sr.d = ps.d; sr.tmin = 0.f; sr.tmax = 0.f; sr.valid = false;
                if (ready) {
                    Hit h{-1, 0.f, 0.f, 0.f};
                    if (ps.phase == PH_CLOSEST) {
                        h.prim = __float_as_int(pool[lane]); h.t = pool[V5_SLOTS + lane]; h.u = pool[2u * V5_SLOTS + lane]; h.v = pool[3u * V5_SLOTS + lane];
                    }
                    const bool shadow_clear = st_s == RS_DONE ? pool[64u + lane] == 0.f : true;
                    status[lane] = RS_IDLE; status[64u + lane] = RS_IDLE;
                    if (LDS_TABLES) path_step<true, FEAT, SamplerT, LdsTables, false>(Ps, LT, ps, smp, h, shadow_clear, sr);
                    else { HT.sh = Ps.shade; HT.bs = Ps.bsdfs; HT.em = Ps.emitters; path_step<true, FEAT, SamplerT, HybridTables, false>(Ps, HT, ps, smp, h, shadow_clear, sr); }
                    push_c = ps.phase == PH_CLOSEST;
                    push_s = sr.valid;
                }
                push_rays(push_c, push_s, sr);
            }
            t_step += STAMP5() - t0;
        };
        auto do_bookkeeping = [&]() {
            const unsigned long long t0 = STAMP5();
            // ---------------------------------------------------------------- bookkeeping: decide, commit, proposals, start
            const bool parked = ps.phase == PH_DONE;
            const unsigned long long pmask = __ballot(parked);
            // (the step above has refilled the queue: "nothing in flight" means every chain that is not idle is parked)
            const bool rays_in_flight = q_count != 0u || __ballot(T.active) != 0ull;
            if (pmask && (__popcll(pmask) >= batch || !rays_in_flight)) {
                SECTION_PARAMS(Pm);
                if (STAMPS) { n_mh++; n_parked += (unsigned long long) __popcll(pmask); }
                if (QCAP != 0u && qn + 64u > QCAP) v4_flush(Pm, Lq, qn, lane);
                int commit = 0, kind = 0; // kind: 0 nothing / finished, 1 next mutation, 2 second stage (4: between mutations, resolved below)
                bool want0 = false, want1 = false, want2 = false;
                float e0x = 0.f, e0y = 0.f, e0r = 0.f, e0g = 0.f, e0b = 0.f;
                float e1x = 0.f, e1y = 0.f, e1r = 0.f, e1g = 0.f, e1b = 0.f;
                float e2x = 0.f, e2y = 0.f, e2r = 0.f, e2g = 0.f, e2b = 0.f;
                if (parked) {
                    if (Pm.type == 1) { // Mira: what its ratio reads (PoolRowSampler)
                        smp.mira_x = Pm.x + cc; smp.mira_stride = Pm.n_chains; smp.mira_k0 = Pm.key0; smp.mira_k1 = Pm.key1;
                        smp.mira_major = base + cs.it; smp.mira_chain = Pm.chain_offset + cc; smp.reset_caches();
                    }
                    const MhDigest o = mh_decide(Pm, cs, smp, ps, ct);
                    if (o.decided) {
                        cum += o.w.w0;
                        const bool a1st = o.acc1, a2nd = o.acc2;
                        want1 = !a1st && o.w.w1 > 0.f;
                        e1x = cs.y.px; e1y = cs.y.py; e1r = cs.y.r * o.w.w1; e1g = cs.y.g * o.w.w1; e1b = cs.y.b * o.w.w1;
                        want2 = !a2nd && o.w.w2 > 0.f;
                        e2x = cs.z.px; e2y = cs.z.py; e2r = cs.z.r * o.w.w2; e2g = cs.z.g * o.w.w2; e2b = cs.z.b * o.w.w2;
                        if (o.acc1 || o.acc2) {
                            want0 = cum > 0.f;
                            e0x = cs.cur.px; e0y = cs.cur.py; e0r = cs.cur.r * cum; e0g = cs.cur.g * cum; e0b = cs.cur.b * cum;
                            cum = a1st ? o.w.w1 : o.w.w2;
                            cs.cur = select_splat(a1st, cs.y, cs.z);
                            if (o.amap) { // acceptance map: the mark goes to the pixel of the state that was LEFT (device_mh.h)
                                const f3 mc = mh_amap_colour(o.amap);
                                want1 = true; e1x = e0x; e1y = e0y; e1r = mc.x; e1g = mc.y; e1b = mc.z;
                            }
                        }
                        commit = mh_commit_mode(o);
                    }
                    kind = cs.stage < 0 ? 4 : (cs.stage == 1 ? 2 : 3); // 3: Green's reverse move
                }
                kind = mh_resolve_kind(Pm, kind, live, base + cs.it, target, limit, reported, lane);
                if constexpr (QCAP != 0u) { // the queue holds QCAP entries, a round adds at most 64
                    v4_enqueue(Lq, qn, want0, e0x, e0y, e0r, e0g, e0b);
                    if (qn + 64u > QCAP) v4_flush(Pm, Lq, qn, lane);
                    v4_enqueue(Lq, qn, want1, e1x, e1y, e1r, e1g, e1b);
                    if (qn + 64u > QCAP) v4_flush(Pm, Lq, qn, lane);
                    v4_enqueue(Lq, qn, want2, e2x, e2y, e2r, e2g, e2b);
                } else { // no queue in this build: ImageBlock::put straight away (film_put applies the validity test)
                    if (want0) film_put(Pm, e0x, e0y, mk3(e0r, e0g, e0b));
                    if (want1) film_put(Pm, e1x, e1y, mk3(e1r, e1g, e1b));
                    if (want2) film_put(Pm, e2x, e2y, mk3(e2r, e2g, e2b));
                }

                // ---- commit (DRMLTSampler::accept: uCurrent = wrap(adopted proposal)) to the state's home in device memory,
                // flattened: items (accepted chain j, row quad q), chain-minor
                // Under Green an adopted SECOND stage finds the rows holding the reverse move y*, not z: those chains' commits
                // recompute z from the state and the stream (v5_iid_second_again); every other adoption copies the rows.
                const bool green = Pm.type == 0 && !Pm.use_mixture;
                const unsigned long long cmask = __ballot(commit != 0 && !(green && commit == SM_STAGE2));
                if (cmask) {
                    if (commit != 0 && !(green && commit == SM_STAGE2)) lds_list[prefix(cmask)] = (int) lane;
                    const uint32_t n = (uint32_t) __popcll(cmask), total = n * nb1;
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t ib = 0u; ib < total; ib += 64u) {
                        const uint32_t i = ib + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t q = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - q * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        if (valid) {
                            float *dst = Pm.x + (size_t) (4u * q) * Pm.n_chains + wave_base + cj;
                            float v[4]; // (loads first: see v5_fill_second)
#pragma unroll
                            for (uint32_t r = 0; r < 4u; ++r) v[r] = rows.get(4u * q + r < D ? 4u * q + r : 4u * q, cj);
#pragma unroll
                            for (uint32_t r = 0; r < 4u; ++r)
                                if (4u * q + r < D) dst[(size_t) r * Pm.n_chains] = wrap01(v[r]);
                        }
                    }
                }
                const uint32_t chain_base = Pm.chain_offset + wave_base;
                const uint32_t maj_done = base + cs.it - 1u; // the mutation just decided (cs.it was advanced by the decision)
                const unsigned large_done = cs.large ? 1u : 0u;
                const unsigned long long gmask = __ballot(green && commit == SM_STAGE2);
                if (gmask) {
                    if (green && commit == SM_STAGE2) lds_list[prefix(gmask)] = (int) lane;
                    const uint32_t nbz = Pm.timid_after_large ? max(nb1, D / 2u) : D / 2u;
                    const uint32_t n = (uint32_t) __popcll(gmask), total = n * nbz;
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t ib = 0u; ib < total; ib += 64u) {
                        const uint32_t i = ib + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t bq = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - bq * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_done, (int) cj, 64);
                        const unsigned lg = (unsigned) __shfl((int) large_done, (int) cj, 64);
                        if (valid && bq < (lg ? nb1 : D / 2u)) v5_iid_second_again(Pm, rows, D, cj, (size_t) wave_base + cj, bq, mj, chain_base + cj, lg != 0u, false);
                    }
                }
                // this wave's own stores to the state rows must have landed before the proposals below read them back (same CU: the
                // wait is all a workgroup-scope fence amounts to)
                if (cmask | gmask) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                // ---- start (parked chain lanes): the coins of the mutation that begins were drawn with the previous one
                if (parked && kind == 1) {
                    if (COIN_ROWS) {
                        const float *cn = &lds_x[L.coin_off + lane];
                        cs.large = cn[0] < Pm.p_large;
                        cs.coin_acc1 = cn[64]; cs.coin_acc2 = cn[128]; cs.coin_mix = cn[192];
                    } else {
                        const u4 coins = philox4x32_10(Pm.key0, Pm.key1, 0u, base + cs.it, Pm.chain_offset + cc, TAG_COIN);
                        cs.large = u32_to_unit(coins.x) < Pm.p_large;
                        cs.coin_acc1 = u32_to_unit(coins.y); cs.coin_acc2 = u32_to_unit(coins.z); cs.coin_mix = u32_to_unit(coins.w);
                    }
                    cs.stage = 0;
                    cs.nd1 = cs.nd2 = 0u;
                }
                // ---- proposals, flattened: items (chain j, Philox block b) -> dimensions 4b .. 4b+3 of y from the state in device
                // memory (the commits above are this wave's own stores: visible to its later loads); block nb1 = the four coins of
                // the NEXT mutation
                const uint32_t maj_mine = base + cs.it; // the mutation in flight
                const unsigned info = cs.large ? 1u : 0u;
                const unsigned long long f1mask = __ballot(kind == 1);
                if (f1mask) {
                    if (kind == 1) lds_list[prefix(f1mask)] = (int) lane;
                    const uint32_t n = (uint32_t) __popcll(f1mask), total = n * (nb1 + (COIN_ROWS ? 1u : 0u));
                    const float rcp_n = 1.f / (float) n;
                    // The state components an item perturbs come from device memory (past the L2s at three waves per SIMD): the reads of pass
                    // i + 1 are issued before pass i's arithmetic (Philox, the transition kernel) instead of behind its stores, which they could not
                    // pass for the compiler.
                    auto locate = [&](uint32_t ib, uint32_t &b_, uint32_t &cj_, bool &valid_) {
                        const uint32_t i = ib + lane;
                        valid_ = i < total;
                        const uint32_t ii = valid_ ? i : 0u;
                        b_ = (uint32_t) (((float) ii + 0.5f) * rcp_n);
                        cj_ = (uint32_t) lds_list[ii - b_ * n];
                    };
                    uint32_t b_n, cj_n; bool valid_n;
                    locate(0u, b_n, cj_n, valid_n);
                    State4 X_n = v5_state4(Pm, D, (size_t) wave_base + cj_n, valid_n && b_n < nb1 ? b_n : 0u);
                    for (uint32_t ib = 0u; ib < total; ib += 64u) {
                        const uint32_t b = b_n, cj = cj_n;
                        const bool valid = valid_n;
                        const State4 X = X_n;
                        if (ib + 64u < total) {
                            locate(ib + 64u, b_n, cj_n, valid_n);
                            X_n = v5_state4(Pm, D, (size_t) wave_base + cj_n, valid_n && b_n < nb1 ? b_n : 0u);
                        }
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        if (valid) {
                            if (b < nb1) v5_fill_first(Pm, rows, D, cj, X, b, mj, chain_base + cj, inf != 0u);
                            else {
                                const u4 coins = philox4x32_10(Pm.key0, Pm.key1, 0u, mj + 1u, chain_base + cj, TAG_COIN);
                                float *dst = &lds_x[L.coin_off + cj];
                                dst[0] = u32_to_unit(coins.x); dst[64] = u32_to_unit(coins.y); dst[128] = u32_to_unit(coins.z); dst[192] = u32_to_unit(coins.w);
                            }
                        }
                    }
                }
                const unsigned long long f2mask = __ballot(kind == 2);
                if (f2mask) { // second-stage proposals (rejected bold steps), in place over the first-stage rows
                    if (kind == 2) lds_list[prefix(f2mask)] = (int) lane;
                    // blocks per chain: uniforms for a large step (one per dim), the orbital angles (one per pair), Gaussian pairs (one block per two dims)
                    const uint32_t nbs = Pm.type == 2 ? (D / 2u + 3u) / 4u : D / 2u;
                    const uint32_t nb2 = Pm.timid_after_large ? max(nb1, nbs) : nbs;
                    const uint32_t n = (uint32_t) __popcll(f2mask), total = n * nb2;
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t ib = 0u; ib < total; ib += 64u) {
                        const uint32_t i = ib + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        if (valid && b < (inf ? nb1 : nbs)) v5_fill_second(Pm, rows, D, cj, (size_t) wave_base + cj, b, mj, chain_base + cj, inf != 0u);
                    }
                }
                const unsigned long long f3mask = __ballot(kind == 3);
                if (f3mask) { // Green's reverse move y* = z - (y - x), over the rows that held z
                    if (kind == 3) lds_list[prefix(f3mask)] = (int) lane;
                    const uint32_t nb3 = Pm.timid_after_large ? max(nb1, D / 2u) : D / 2u;
                    const uint32_t n = (uint32_t) __popcll(f3mask), total = n * nb3;
                    const float rcp_n = 1.f / (float) n;
                    for (uint32_t ib = 0u; ib < total; ib += 64u) {
                        const uint32_t i = ib + lane;
                        const bool valid = i < total;
                        const uint32_t ii = valid ? i : 0u;
                        const uint32_t b = (uint32_t) (((float) ii + 0.5f) * rcp_n), j = ii - b * n;
                        const uint32_t cj = (uint32_t) lds_list[j];
                        const uint32_t mj = (uint32_t) __shfl((int) maj_mine, (int) cj, 64);
                        const unsigned inf = (unsigned) __shfl((int) info, (int) cj, 64);
                        if (valid && b < (inf ? nb1 : D / 2u)) v5_iid_second_again(Pm, rows, D, cj, (size_t) wave_base + cj, b, mj, chain_base + cj, inf != 0u, true);
                    }
                }
                // (rows in device memory: the flattened stores above land before their chains' lanes read them -- same CU, as for the state)
                if (ROWS_MEM && (f1mask | f2mask | f3mask)) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                // ---- begin the evaluation: film position and camera ray from the first two components; the ray goes into the pool
                if (parked) {
                    if (kind == 0) ps.phase = PH_IDLE;
                    else {
                        path_init(Pm, ps);
                        const float v0 = smp.next(0u), v1 = smp.next(1u);
                        path_begin(Pm, ps, v0, v1);
                    }
                }
                {
                    ShadowRay none;
                    none.o = ps.o; none.d = ps.d; none.tmin = 0.f; none.tmax = 0.f; none.valid = false;
                    push_rays(parked && ps.phase == PH_CLOSEST, false, none); // the camera rays of the evaluations that begin
                }
            }
            t_mh += STAMP5() - t0;
        };
        auto do_trace = [&]() {
            const unsigned long long t0 = STAMP5();
            // ---------------------------------------------------------------- trace: the pool's rays, any lane any ray
            if constexpr (FLAT) {
                // flat scenes: ONE pass of the brute-force loop over up to 64 pending rays; all of them are done when it returns
                if (q_count != 0u) {
                    SECTION_PARAMS(Pt);
                    if (STAMPS) { n_phase++; n_lanes_at_start += (unsigned long long) min(q_count, 64u); }
                    const bool take = lane < q_count;
                    slot = ring[(q_head + lane) & (V5_SLOTS - 1u)];
                    if (take) {
                        const float *r = pool + slot;
                        const Hit h = trace<FEAT>(Pt, mk3(r[0], r[V5_SLOTS], r[2u * V5_SLOTS]), mk3(r[3u * V5_SLOTS], r[4u * V5_SLOTS], r[5u * V5_SLOTS]),
                                                  r[6u * V5_SLOTS], r[7u * V5_SLOTS], slot >= 64u);
                        if (slot < 64u) {
                            float *w = pool + slot;
                            w[0] = __int_as_float(h.prim); w[V5_SLOTS] = h.t; w[2u * V5_SLOTS] = h.u; w[3u * V5_SLOTS] = h.v;
                        } else {
                            pool[slot] = h.prim >= 0 ? 1.f : 0.f;
                        }
                        status[slot] = RS_DONE;
                    }
                    const uint32_t taken = min(q_count, 64u);
                    q_head = (q_head + taken) & (V5_SLOTS - 1u);
                    q_count -= taken;
                }
            } else {
                SECTION_PARAMS(Pt);
                const TravLoop<StackT, DParams, OVF || !STACK16, CAP, FEAT> TL(Pt, my_stack);
                const int yield_lanes = Pt.trace_yield, refill_at = Pt.pool_refill;
                int finished_closest = 0;
                bool first = true;
                if (STAMPS) n_phase++;
                for (;;) {
                    // idle lanes take pending slots off the queue (at the start of a phase, and whenever a few lanes have run dry)
                    const unsigned long long idle = __ballot(!T.active);
                    if (q_count != 0u && idle != 0ull && (first || __popcll(idle) >= refill_at || idle == ~0ull)) {
                        const uint32_t rank = prefix(idle);
                        const bool take = !T.active && rank < q_count;
                        if (take) {
                            slot = ring[(q_head + rank) & (V5_SLOTS - 1u)];
                            const float *r = pool + slot;
                            trav_begin(T, mk3(r[0], r[V5_SLOTS], r[2u * V5_SLOTS]), mk3(r[3u * V5_SLOTS], r[4u * V5_SLOTS], r[5u * V5_SLOTS]),
                                       r[6u * V5_SLOTS], r[7u * V5_SLOTS], slot >= 64u);
                        }
                        const uint32_t taken = min((uint32_t) __popcll(idle), q_count);
                        q_head = (q_head + taken) & (V5_SLOTS - 1u);
                        q_count -= taken;
                        if (STAMPS) n_refill++;
                    }
                    if (STAMPS && first) n_lanes_at_start += (unsigned long long) __popcll(__ballot(T.active));
                    first = false;
                    if (finished_closest >= yield_lanes) break;
                    bool any;
                    const bool done_now = TL.step(T, true, any);
                    if (!any) break; // (the queue is empty too: an idle wave with pending slots refills above)
                    if (done_now) { // result over the ray's record; the owner chain picks it up in the step phase
                        if (slot < 64u) {
                            float *r = pool + slot;
                            r[0] = __int_as_float(T.h.prim); r[V5_SLOTS] = T.h.t; r[2u * V5_SLOTS] = T.h.u; r[3u * V5_SLOTS] = T.h.v;
                        } else {
                            pool[slot] = T.h.prim >= 0 ? 1.f : 0.f;
                        }
                        status[slot] = RS_DONE;
                    }
                    finished_closest += __popcll(__ballot(done_now && slot < 64u));
                }
        
            }
            t_trace += STAMP5() - t0;
        };
        // Flat scenes: every ray of a pass is done when the pass returns, so the chains step first and the bookkeeping branch
        // sees who parked and what is still queued (it then fires for a full batch, or when nothing else is left to do). BVH
        // scenes: a phase leaves traversals running; the branch comes first and its camera rays join the phase that follows.
        if constexpr (FLAT) { do_step(); do_bookkeeping(); do_trace(); }
        else { do_bookkeeping(); do_step(); do_trace(); }
    }
#undef STAMP5
    SECTION_PARAMS(Pe);
    if (STAMPS && lane == 0) {
        atomicAdd(Pe.stats + 16, t_mh); atomicAdd(Pe.stats + 17, t_trace); atomicAdd(Pe.stats + 18, t_step); atomicAdd(Pe.stats + 19, n_outer);
        atomicAdd(Pe.stats + 23, n_mh); atomicAdd(Pe.stats + 24, n_parked); atomicAdd(Pe.stats + 25, n_stepping);
    }
    // "Perform the last splat": the current states with what they have accumulated since they were adopted
    if constexpr (QCAP != 0u) {
        if (qn + 64u > QCAP) v4_flush(Pe, Lq, qn, lane);
        v4_enqueue(Lq, qn, live && cum > 0.f, cs.cur.px, cs.cur.py, cs.cur.r * cum, cs.cur.g * cum, cs.cur.b * cum);
        v4_flush(Pe, Lq, qn, lane);
    } else if (live && cum > 0.f) film_put(Pe, cs.cur.px, cs.cur.py, mk3(cs.cur.r * cum, cs.cur.g * cum, cs.cur.b * cum));
    if (live) { // (the PSS state is at home in device memory already)
        Pe.cur_lum[c] = cs.cur.lum; Pe.cur_px[c] = cs.cur.px; Pe.cur_py[c] = cs.cur.py;
        Pe.cur_r[c] = cs.cur.r; Pe.cur_g[c] = cs.cur.g; Pe.cur_b[c] = cs.cur.b;
        if (Pe.chain_done) Pe.chain_done[c] = base + cs.it;
    }
    if (Pe.chain_done && !reported && lane == 0) atomicSub(Pe.waves_left, 1u); // (a wave none of whose chains had anything to do)
    flush_counters(Pe, ct, lane);
    const unsigned long long decided = wave_sum(live ? cs.it : 0u);
    const unsigned long long nn = FLAT ? 0ull : wave_sum(T.n_nodes), np = FLAT ? 0ull : wave_sum(T.n_prims);
    if (lane == 0) {
        atomicAdd(Pe.stats + 9, decided);
        atomicAdd(Pe.stats + 10, nn); atomicAdd(Pe.stats + 11, np); atomicAdd(Pe.stats + 12, (unsigned long long) T.it_inner); atomicAdd(Pe.stats + 13, (unsigned long long) T.it_leaf);
        if (STAMPS) { atomicAdd(Pe.stats + 20, n_phase); atomicAdd(Pe.stats + 21, n_lanes_at_start); atomicAdd(Pe.stats + 22, n_refill); }
    }
}

// k_mutate_v5 <FEAT, STACK16, OVF, STAMPS, LDS_TABLES, ROWS_MEM>: ray pool, 64 chains per wave
void launch_mutate_v5(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st) {
#define LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(plan.grid), dim3(CHAIN_BLOCK), plan.lds, st, P, n_mut, mut_base); break
    switch (plan.build) {
    case Build::V5_F0_ROWS: LAUNCH(k_mutate_v5<0, true, false, false, true, true>);   case Build::V5_F1_ROWS: LAUNCH(k_mutate_v5<1, true, false, false, true, true>);
    case Build::V5_F3_ROWS: LAUNCH(k_mutate_v5<3, true, false, false, true, true>);   case Build::V5_F7_ROWS: LAUNCH(k_mutate_v5<7, true, false, false, true, true>);
    case Build::V5_F7_GLOBAL: LAUNCH(k_mutate_v5<7, true, false, false, false>);      case Build::V5_F0_STAMPS: LAUNCH(k_mutate_v5<0, true, false, true, true>);
    case Build::V5_F0: LAUNCH(k_mutate_v5<0, true, false, false, true>);             case Build::V5_F1: LAUNCH(k_mutate_v5<1, true, false, false, true>);
    case Build::V5_F3: LAUNCH(k_mutate_v5<3, true, false, false, true>);             case Build::V5_F7: LAUNCH(k_mutate_v5<7, true, false, false, true>);
    case Build::V5_F8_S32_ROWS: LAUNCH(k_mutate_v5<8, false, true, false, false, true>); case Build::V5_F15_S32_ROWS: LAUNCH(k_mutate_v5<15, false, true, false, false, true>);
    case Build::V5_F8_OVF_ROWS: LAUNCH(k_mutate_v5<8, true, true, false, false, true>);  case Build::V5_F15_OVF_ROWS: LAUNCH(k_mutate_v5<15, true, true, false, false, true>);
    case Build::V5_F8_ROWS: LAUNCH(k_mutate_v5<8, true, false, false, false, true>);     case Build::V5_F15_ROWS: LAUNCH(k_mutate_v5<15, true, false, false, false, true>);
    case Build::V5_F8_S32: LAUNCH(k_mutate_v5<8, false, true>); case Build::V5_F15_S32: LAUNCH(k_mutate_v5<15, false, true>);
    case Build::V5_F8_OVF: LAUNCH(k_mutate_v5<8, true, true>);  case Build::V5_F15_OVF: LAUNCH(k_mutate_v5<15, true, true>);
    case Build::V5_F8_STAMPS: LAUNCH(k_mutate_v5<8, true, false, true>); case Build::V5_F8: LAUNCH(k_mutate_v5<8, true, false>); case Build::V5_F15: LAUNCH(k_mutate_v5<15, true, false>);
    default:
        fprintf(stderr, "[drmlt] launch_mutate_v5: build %d is not a k_mutate_v5 build\n", (int) plan.build);
        abort();
    }
#undef LAUNCH
}
