// k_mutate_v3: the chain loop with two lanes per chain in lock-step rounds -- k_mutate_v4's predecessor (kernels_v4.hip), kept as
// the bit-equality cross-check of the later generations. What it shares with them: chain_path.h.
#include <cstdlib>
#include <cstdio>
#include "chain_path.h"

// k_mutate_v3: splat the decided mutation at once and adopt the accepted proposal. The three splats go through ONE
// film_put site (the call expands to ~150 instructions; six inlined copies of it were a sixth of the kernel's code):
// slot 0 current state, 1 first-stage, 2 second-stage proposal.
DEV int mh_decide_splat(const DParams &P, ChainState &cs, LdsSampler &smp, PathState &ps, Counters &ct) {
    const MhDigest o = mh_decide(P, cs, smp, ps, ct);
    if (!o.decided) return 0;
#pragma nounroll
    for (int i = 0; i < 3; ++i) {
        const float w = i == 0 ? o.w.w0 : (i == 1 ? o.w.w1 : o.w.w2);
        const DSplat sp = select_splat(i == 0, cs.cur, select_splat(i == 1, cs.y, cs.z));
        if (w > 0.f) film_put(P, sp.px, sp.py, mk3(sp.r * w, sp.g * w, sp.b * w));
    }
    const int commit = mh_commit_mode(o);
    if (commit) {
        if (o.amap) film_put(P, cs.cur.px, cs.cur.py, mh_amap_colour(o.amap)); // the state that is LEFT (device_mh.h)
        cs.cur = select_splat(o.acc1, cs.y, cs.z);
    }
    return commit;
}

// ------------------------------------------------------------------------------------------
// k_mutate_v3: two lanes per chain. 64 k chains are only 1024 waves = ONE wave per SIMD: every
// LDS / scalar-cache / transcendental latency is exposed and a lone wave can issue a VALU op only
// every 4 cycles (MI355X_MICROARCH.md). Lanes 0..31 of a wave run the chain state machines;
// lane 32+i is the helper of lane i and traces the shadow (NEE) ray of a vertex
// while lane i traces the BSDF-sampled ray of the same vertex. A bounce then costs one loop
// iteration instead of two, a wave carries 32 chains, and the same 64 k chains occupy 2048
// waves = two per SIMD, which hide each other's latencies.
// LDS_TABLES: scene tables staged in LDS (small scenes) or read from HBM/L2 -- a launch-time property, compiled in so
// that the kernel carries ONE copy of the path step (the two-way runtime branch doubled the hot loop's code and pushed
// it past the 64 KB instruction cache).
template <int FEAT, bool LDS_TABLES>
__global__ void __launch_bounds__(CHAIN_BLOCK) k_mutate_v3(DParams P, uint32_t n_mut, uint32_t mut_base) {
    const uint32_t lane = threadIdx.x;
    const uint32_t sub = lane & 31u;
    const bool helper = lane >= 32u;
    const uint32_t c = blockIdx.x * 32u + sub;
    const bool live = !helper && c < P.n_chains;
    const uint32_t cc = c < P.n_chains ? c : P.n_chains - 1;
    const int D = P.eff_dim;
    const uint32_t D4 = ((uint32_t) D + 3u) & ~3u;
    if (!helper)
        for (int k = 0; k < D; ++k) lds_x[(uint32_t) k * 32u + sub] = P.x[(size_t) k * P.n_chains + cc];

    ChainState cs;
    cs.cur.lum = P.cur_lum[cc]; cs.cur.px = P.cur_px[cc]; cs.cur.py = P.cur_py[cc];
    cs.cur.r = P.cur_r[cc]; cs.cur.g = P.cur_g[cc]; cs.cur.b = P.cur_b[cc];
    cs.y = cs.cur; cs.z = cs.cur;
    cs.a1 = 0.f; cs.coin_acc1 = cs.coin_acc2 = cs.coin_mix = 0.f;
    cs.it = 0u; cs.nd1 = cs.nd2 = 0u; cs.stage = -1; cs.large = false;

    LdsSampler smp;
    smp.key0 = P.key0; smp.key1 = P.key1; smp.chain = P.chain_offset + cc; smp.major = 0u;
    smp.mode = SM_STAGE1; smp.type = P.type; smp.large = false; smp.sigma2 = P.sigma2; smp.lane = sub;
    smp.stride = 32u;
    smp.u1_off = (uint32_t) D * 32u;
    smp.s2_off = smp.u1_off + D4 * 32u;
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    PathState ps;
    path_init(P, ps);
    ps.phase = (live && n_mut > 0u) ? PH_DONE : PH_IDLE; // helpers stay PH_IDLE for good
    ps.o = mk3(0.f, 0.f, 0.f); ps.d = mk3(0.f, 0.f, 1.f); ps.tmin = 0.f; ps.tmax = 0.f;
    bool helper_has_ray = false;
    Hit h{-1, 0.f, 0.f, 0.f};
    const int batch = P.mh_batch > 32 ? 32 : P.mh_batch;
    LdsTables LT;
    LT.shade_off = smp.s2_off + D4 * 32u;
    LT.bsdf_off = LT.shade_off + (uint32_t) P.n_shade * 16u;
    LT.emit_off = LT.bsdf_off + (uint32_t) P.n_bsdfs * 12u;
    const GlobalTables GT{P.shade, P.bsdfs, P.emitters};
    if (LDS_TABLES) stage_tables(P, LT, lane);

    // Wave priority by loop section: the two waves of a SIMD are then rarely in the same section with the same claim on the
    // issue port -- the ray loop (dense VALU, its scalar loads pipelined) yields to a partner that is in the latency-bound
    // path step or bookkeeping branch. Measured +5 % on config 2 (any assignment of distinct levels gives most of it;
    // DRMLT_DEBUG bit 1024 switches it off for A/B runs).
    const bool prio = (P.debug & 1024) == 0;
    const bool stamps = (P.debug & 128) != 0;
    unsigned long long t_mh = 0, t_trace = 0, t_step = 0, n_iter = 0, n_mh = 0, n_busy = 0;
    unsigned long long t_decide = 0, t_commit = 0, t_start = 0, t_fill = 0;
    unsigned long long hist[6] = {0, 0, 0, 0, 0, 0}; // iterations by number of chains tracing a closest-hit ray: 0, 1-4, 5-8, 9-16, 17-24, 25-32
#define STAMP() (stamps ? __builtin_amdgcn_s_memtime() : 0ull)
    for (;;) {
        const bool parked = ps.phase == PH_DONE;
        const unsigned long long pmask = __ballot(parked);
        const unsigned long long rmask = __ballot(ps.phase != PH_DONE && ps.phase != PH_IDLE);
        if (!pmask && !rmask) break;
        const unsigned long long s0 = STAMP();
        if (pmask && (__popcll(pmask) >= batch || !rmask)) {
            n_mh++;
            if (prio) __builtin_amdgcn_s_setprio(2);
            // decide (chain lanes) -> commit (both lanes of a pair) -> start (chain lanes) -> draw (both lanes)
            int commit = 0;
            if (parked) commit = mh_decide_splat(P, cs, smp, ps, ct);
            const unsigned long long m1 = STAMP();
            const int commit_pair = (int) from_lower_u((unsigned) commit);
            const uint32_t maj_c = from_lower_u(smp.major);
            const bool large_c = from_lower_u(smp.large ? 1u : 0u) != 0u;
            if (helper) { smp.major = maj_c; smp.large = large_c; }
            if (commit_pair) { // pair-aligned halves: orbital pairs never straddle the split
                const uint32_t split = (((uint32_t) D / 2u) + 1u) & ~1u;
                commit_range(smp, commit_pair, helper ? split : 0u, helper ? (uint32_t) D : split);
            }
            const unsigned long long m2 = STAMP();
            int fill = 0;
            if (parked) fill = mh_start(P, cs, smp, ps, n_mut, mut_base);
            const unsigned long long m3 = STAMP();
            const int fill_pair = (int) from_lower_u((unsigned) fill);
            const uint32_t maj_f = from_lower_u(smp.major);
            const bool large_f = from_lower_u(smp.large ? 1u : 0u) != 0u;
            if (helper) { smp.major = maj_f; smp.large = large_f; }
            if (fill_pair == 1) {
                const uint32_t nb = D4 / 4u, hb = (nb + 1u) / 2u;
                smp.fill_stage1(helper ? hb : 0u, helper ? nb : hb);
            } else if (fill_pair == 2) {
                smp.fill_stage2(D4, helper ? 1u : 0u, 2u);
            }
            const unsigned long long m4 = STAMP();
            t_decide += m1 - s0; t_commit += m2 - m1; t_start += m3 - m2; t_fill += m4 - m3;
        }
        // one ray per lane: chain lanes their camera / bounce ray, helpers the shadow ray they were handed
        const unsigned long long s1 = STAMP();
        const bool tracing = helper ? helper_has_ray : ps.phase == PH_CLOSEST;
        if (stamps) n_busy += __popcll(__ballot(tracing));
        if (stamps) { const int nl = __popcll(__ballot(tracing && !helper)); hist[nl == 0 ? 0 : (nl <= 4 ? 1 : (nl <= 8 ? 2 : (nl <= 16 ? 3 : (nl <= 24 ? 4 : 5))))]++; }
        if (prio) __builtin_amdgcn_s_setprio(0);
        if (tracing) h = trace<FEAT>(P, ps.o, ps.d, ps.tmin, ps.tmax, helper);
        if (prio) __builtin_amdgcn_s_setprio(3);
        const unsigned long long s2 = STAMP();
        const unsigned occluded = from_upper_u((helper_has_ray && h.prim >= 0) ? 1u : 0u);
        helper_has_ray = false;
        ShadowRay sr;
        sr.o = ps.o; sr.d = ps.d; sr.tmin = 0.f; sr.tmax = 0.f; sr.valid = false;
        if (!helper && ps.phase != PH_DONE && ps.phase != PH_IDLE) {
            if (LDS_TABLES) path_step<true, FEAT>(P, LT, ps, smp, h, occluded == 0u, sr);
            else path_step<true, FEAT>(P, GT, ps, smp, h, occluded == 0u, sr);
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
        const unsigned long long s3 = STAMP();
        t_mh += s1 - s0; t_trace += s2 - s1; t_step += s3 - s2; n_iter++;
    }
#undef STAMP
    if (stamps && lane == 0) {
        atomicAdd(P.stats + 16, t_mh); atomicAdd(P.stats + 17, t_trace); atomicAdd(P.stats + 18, t_step);
        atomicAdd(P.stats + 19, n_iter); atomicAdd(P.stats + 20, n_mh); atomicAdd(P.stats + 21, n_busy);
        for (int q = 0; q < 6; ++q) atomicAdd(P.stats + 26 + q, hist[q]);
        atomicAdd(P.stats + 22, t_decide); atomicAdd(P.stats + 23, t_commit); atomicAdd(P.stats + 24, t_start); atomicAdd(P.stats + 25, t_fill);
    }

    if (live) {
        for (int k = 0; k < D; ++k) P.x[(size_t) k * P.n_chains + c] = lds_x[(uint32_t) k * 32u + sub];
        P.cur_lum[c] = cs.cur.lum; P.cur_px[c] = cs.cur.px; P.cur_py[c] = cs.cur.py;
        P.cur_r[c] = cs.cur.r; P.cur_g[c] = cs.cur.g; P.cur_b[c] = cs.cur.b;
    }
    flush_counters(P, ct, lane);
}

// k_mutate_v3 <FEAT, LDS_TABLES>: the bit-equality cross-check
void launch_mutate_v3(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st) {
#define LAUNCH(...) hipLaunchKernelGGL((__VA_ARGS__), dim3(plan.grid), dim3(CHAIN_BLOCK), plan.lds, st, P, n_mut, mut_base); break
    switch (plan.build) {
    case Build::V3_F0: LAUNCH(k_mutate_v3<0, true>); case Build::V3_F3: LAUNCH(k_mutate_v3<3, true>); case Build::V3_F7: LAUNCH(k_mutate_v3<7, true>);
    case Build::V3_F15: LAUNCH(k_mutate_v3<15, true>); case Build::V3_F15_GLOBAL: LAUNCH(k_mutate_v3<15, false>);
    default:
        fprintf(stderr, "[drmlt] launch_mutate_v3: build %d is not a k_mutate_v3 build\n", (int) plan.build);
        abort();
    }
#undef LAUNCH
}
