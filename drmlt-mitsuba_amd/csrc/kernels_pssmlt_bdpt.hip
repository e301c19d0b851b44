// algo=pssmlt over technique=bdpt (gfx950): stock Mitsuba's PSSMLT -- PSSMLTRenderer::process (src/integrators/pssmlt/
// pssmlt_proc.cpp:110-285) over PathSampler::sampleSplats(EBidirectional). One Markov chain per lane, one wave per workgroup.
//
//   k_mutate_pssmlt_bdpt   the chain loop: one proposal per mutation from the three PSSMLT samplers (device_bdpt.h:
//                          PssmltSampler3), one evaluation into a splat LIST (eval_bdpt), regular Metropolis-Hastings
//
// Bootstrap, seed replay, evaluation points and the chains' storage are technique=bdpt's (kernels_bdpt.hip): the same LDS rows
// ([row][lane]: the walks' part of the state [0, S + E), then eval_bdpt's two density row groups and its row of segment heads;
// the staged BSDF / emitter records behind them in the LDS_BSDFS build), the same list slots in HBM (slot 0 = current state,
// slot 1 = the proposal; lists unnormalised next to their luminance), the direct sampler's Dd components in memory.
#include <cstdlib>
#include "bdpt_lists.h"

// FEAT / OCC / LDS_BSDFS: as for k_mutate_bdpt (7: no BVH traversal and no LDS stack, 15: everything; OCC 2: registers capped at
// 256 for two waves per SIMD; LDS_BSDFS: BSDF and emitter records staged in LDS behind the rows).
// The loop is LOCKSTEP: every mutation is exactly one evaluation (there is no second stage), and the whole wave must make every
// eval_bdpt call -- the connections of all its chains are handed out to all its lanes -- so lanes without a chain run along with
// `live` unset. Chains keep their lanes (no execution order: nothing tells their work apart).
template <int FEAT, int OCC, bool LDS_BSDFS = false> __global__ void __launch_bounds__(CHAIN_BLOCK, OCC) k_mutate_pssmlt_bdpt(DParams P, uint32_t n_mut, uint32_t mut_base) {
    const uint32_t lane = threadIdx.x;
    MixedTables MT;
    MT.sh = P.shade;
    MT.L.shade_off = ((uint32_t) P.mmlt_S + (uint32_t) P.mmlt_E) * 64u + (uint32_t) bdpt_eval_lds_floats(P.max_depth); // (the emitters' shape records)
    MT.L.bsdf_off = MT.L.shade_off + (uint32_t) P.n_emitters * 16u;
    MT.L.emit_off = MT.L.bsdf_off + (uint32_t) P.n_bsdfs * 12u;
    if (LDS_BSDFS) stage_bsdfs_emitters(P, MT.L, lane);
    const uint32_t c = blockIdx.x * CHAIN_BLOCK + lane;
    const bool live = c < P.n_chains;
    const uint32_t cc = live ? c : P.n_chains - 1;
    const uint32_t NX = bdpt_nx_lds(P);
    for (uint32_t k = 0; k < NX; ++k) lds_x[k * 64u + lane] = P.x[(size_t) k * P.n_chains + cc];
    float cur_lum = P.cur_lum[cc];
    float *L0 = list_col(P, 0, cc), *L1 = list_col(P, 1, cc); // current state, proposal
    float cum = 0.f; // cumulativeWeight: what the current state has gathered since it was adopted (:175,226)

    PssmltSampler3 smp;
    pssmlt3_setup(smp, P, lane, P.x + (size_t) NX * P.n_chains + cc);
    smp.chain = P.chain_offset + cc;
    const GlobalTables T{P.shade, P.bsdfs, P.emitters};
    Counters ct = {0u, 0u, 0u, 0u, 0u};
    const float b = P.luminance_b, pLarge = P.p_large;
    // Kelemen-style weights "don't work for 2-stage MLT" (:205-206): under an importance map EVERY mutation deposits Veach's
    // expectations, a rejected zero proposal (:218-222) included. (The reference keeps the Kelemen form in that one branch, and so
    // does k_mutate_pssmlt with it; a film that mixes b-scaled and unit weights is biased -- DESIGN.md section 5, deviation 21.)
    const bool kelemen_w = P.kelemen_weights != 0 && !P.importance;

    for (uint32_t it = 0u; it < n_mut; ++it) { // (uniform: n_mut is the launch's)
        const uint32_t m = mut_base + it;
        const u4 coins = philox4x32_10(P.key0, P.key1, 0u, m, smp.chain, TAG_COIN);
        const bool large = u32_to_unit(coins.x) < pLarge; // :183
        smp.major = m;
        smp.large = large;
        BdptResult R;
        if (LDS_BSDFS) eval_bdpt<FEAT>(P, MT, smp, live, cc, NX, L1, R); // the whole wave: the connections of all chains go to all lanes
        else eval_bdpt<FEAT>(P, T, smp, live, cc, NX, L1, R);
        if (!live) continue;
        ct.rays += R.nrays;
        const float y_lum = list_finalize(P, L1, R.lum); // proposed->normalize(importanceMap): two-stage importance
        float a = fminf(1.f, y_lum / cur_lum);
        if (isnan(y_lum) || y_lum < 0.f) a = 0.f; // :194-198
        bool accept = false;
        float wc, wp = 0.f;
        if (a > 0.f) {
            if (kelemen_w) { // :205-210
                wc = (1.f - a) * cur_lum / (cur_lum / b + pLarge);
                wp = (a + (large ? 1.f : 0.f)) * y_lum / (y_lum / b + pLarge);
            } else { // Veach-style use of expectations
                wc = 1.f - a;
                wp = a;
            }
            accept = a == 1.f || u32_to_unit(coins.y) < a;
        } else {
            wc = kelemen_w ? cur_lum / (cur_lum / b + pLarge) : 1.f; // :218-222
        }
        cum += wc;
        mh_count(ct, large, accept, false, false);
        if (accept) {
            list_splat(P, L0, cur_lum, cum); // the state that is replaced, once, with everything it gathered
            cum = wp;
            for (int sg = 0; sg < 3; ++sg) { // PSSMLTSampler::accept of all three samplers: every component, consumed or not
                smp.select(sg);
                const uint32_t nk = sg == 0 ? smp.S : (sg == 1 ? smp.E : (uint32_t) P.bd_Dd);
                for (uint32_t k = 0; k < nk; ++k) smp.put(k, smp.next(k));
            }
            { float *t = L0; L0 = L1; L1 = t; } // the accepted list becomes the current one: swap, do not copy
            cur_lum = y_lum;
        } else {
            list_splat(P, L1, y_lum, wp); // a rejected proposal's list, with its own weight
        }
    }

    if (live) {
        list_splat(P, L0, cur_lum, cum); // "Perform the last splat" -- at every launch end: splatting is linear
        if (L0 != list_col(P, 0, cc)) list_copy(P, list_col(P, 0, cc), L0); // slot 0 is where the next launch (and drmlt_chain_state) look
        for (uint32_t k = 0; k < NX; ++k) P.x[(size_t) k * P.n_chains + c] = lds_x[k * 64u + lane];
        P.cur_lum[c] = cur_lum;
    }
    flush_counters(P, ct, lane);
}

void launch_mutate_pssmlt_bdpt(const ChainPlan &plan, const DParams &P, uint32_t n_mut, uint32_t mut_base, hipStream_t st) {
    const dim3 grid(plan.grid), block(CHAIN_BLOCK);
    switch (plan.build) {
    case Build::PSSMLT_BDPT_F15: hipLaunchKernelGGL((k_mutate_pssmlt_bdpt<15, 1>), grid, block, plan.lds, st, P, n_mut, mut_base); break;
    case Build::PSSMLT_BDPT_F7_OCC2_TABLES: hipLaunchKernelGGL((k_mutate_pssmlt_bdpt<7, 2, true>), grid, block, plan.lds, st, P, n_mut, mut_base); break;
    case Build::PSSMLT_BDPT_F7_OCC2: hipLaunchKernelGGL((k_mutate_pssmlt_bdpt<7, 2>), grid, block, plan.lds, st, P, n_mut, mut_base); break;
    case Build::PSSMLT_BDPT_F7: hipLaunchKernelGGL((k_mutate_pssmlt_bdpt<7, 1>), grid, block, plan.lds, st, P, n_mut, mut_base); break;
    default: fprintf(stderr, "[drmlt] launch_mutate_pssmlt_bdpt: build %d is not an algo=pssmlt, technique=bdpt kernel\n", (int) plan.build); abort();
    }
}
