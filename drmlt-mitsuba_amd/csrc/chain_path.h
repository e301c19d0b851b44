// What more than one technique=path chain-kernel family shares: the chain state and its decide / commit / start pieces (v3, v4, w2,
// v5), the half-wave exchanges (v3, v4, w2), the run-ahead resolution and the LDS splat queue with its flush (v4, w2, v5).
// Included by kernels_v3.hip (k_mutate_v3) and kernels_v4.hip (k_mutate_v4, k_mutate_w2, k_mutate_v5): the machine code of either
// unit's kernels depends only on that unit and on the headers.
#pragma once
#include "kernel_common.h"
#include "launch_plan.h" // V4_* / V5_* LDS constants, the Build each launcher dispatches on

struct ChainState {
    DSplat cur, y, z;
    float a1, coin_acc1, coin_acc2, coin_mix;
    uint32_t it, nd1, nd2;
    int stage;       // -1: no mutation in flight, 0/1/2: evaluating first / second / reverse
    bool large;
};

// The bookkeeping branch in four pieces so that k_mutate_v3 can share the two heavy ones
// (committing D_eff dimensions, drawing the next mutation's uniforms) between a chain lane and
// its helper lane:
//   mh_decide  digest the finished evaluation (device_mh.h: mh_digest); the caller splats a decided mutation --
//              k_mutate_v3 at once, k_mutate_v4 / v5 through their LDS queue -- and commits the adopted proposal
//   commit     x[k] = wrap(proposal[k]) for a range of dimensions           (shareable)
//   mh_start   advance to the next evaluation (next stage or next mutation); returns which
//              uniforms must be drawn (0 none, 1 first stage, 2 second stage)
//   fill       Philox draws into LDS for a range of blocks                    (shareable)

// Tierney & Mira's transition ratio Q1(y|z) / Q1(y|x) over the dimensions either stage used (drmlt_sampler.cpp:400-414)
template <class SamplerT> DEV float mira_ratio(SamplerT &smp, uint32_t nd1, uint32_t nd2) {
    const uint32_t dimStage = max(nd1, nd2) - 1u;
    float num = 0.f, den = 0.f;
    // (not unrolled: the unrolled copies' compare masks were live at once and spilled scalar registers in every chain kernel)
#pragma nounroll
    for (uint32_t i = 0; i < dimStage; ++i) {
        const float yi = smp.y_raw(i);
        num += kelemen_logpdf(smp.z_raw(i) - yi);
        den += kelemen_logpdf(smp.x(i) - yi);
    }
    return __expf(num - den);
}

// commit mode of a decided mutation: 0 none, SM_STAGE1 = adopt y, SM_STAGE2 = adopt z
DEV int mh_commit_mode(const MhDigest &d) { return d.acc1 ? SM_STAGE1 : (d.acc2 ? SM_STAGE2 : 0); }

// What the path kernels add to mh_digest: the evaluation's result comes out of a PathState and is normalised, the dimensions each
// stage consumed are kept for Mira's ratio, and a decided mutation advances the chain's counter (stage -1: between mutations).
// RULE_ORBITAL (k_mutate_v4's orbital body): mh_digest with the rule compiled in; nd1 / nd2, which only Mira's ratio reads, are not kept.
template <int RULE = RULE_GENERIC, class SamplerT> DEV MhDigest mh_decide(const DParams &P, ChainState &cs, SamplerT &smp, PathState &ps, Counters &ct) {
    if (cs.stage < 0) return MhDigest{false, false, false, AMAP_NONE, {0.f, 0.f, 0.f}}; // nothing evaluated yet (first call of a launch)
    DSplat res;
    res.px = ps.px; res.py = ps.py; res.r = ps.Li.x; res.g = ps.Li.y; res.b = ps.Li.z;
    res.lum = luminance3(ps.Li);
    normalize_splat(res, P);
    ct.rays += ps.nrays;
    // (selected VALUES: `if (stage == 0) cs.y = res; else if (stage == 1) cs.z = res;` is merged into one store through a selected
    // ADDRESS, and the chain state then lives in scratch memory -- see select_splat)
    const bool first = cs.stage == 0, second = cs.stage == 1;
    cs.y = select_splat(first, res, cs.y); if constexpr (RULE != RULE_ORBITAL) cs.nd1 = first ? ps.k : cs.nd1;
    cs.z = select_splat(second, res, cs.z); if constexpr (RULE != RULE_ORBITAL) cs.nd2 = second ? ps.k : cs.nd2;
    const MhRules R{P.use_mixture != 0, P.acceptance_map != 0, P.timid_after_large != 0, P.type};
    const MhDigest d = mh_digest<RULE>(R, cs.large, cs.coin_acc1, cs.coin_acc2, cs.coin_mix, res.lum, cs.cur.lum, cs.y.lum, cs.z.lum, cs.a1, cs.stage, ct,
                                 [&]() { return mira_ratio(smp, cs.nd1, cs.nd2); });
    if (d.decided) { cs.it++; cs.stage = -1; }
    return d;
}

// DRMLTSampler::accept for dimensions [k0, k1): uCurrent = wrap(chosen proposal)
DEV void commit_range(LdsSampler &smp, int commit_mode, uint32_t k0, uint32_t k1) {
    smp.mode = commit_mode;
    if (smp.type == 2 && !(k0 & 1u) && !(k1 & 1u)) { // orbital: pair by pair (k0, k1 are pair-aligned)
        const bool second = commit_mode == SM_STAGE2;
        for (uint32_t k = k0; k < k1; k += 2u) {
            float v0, v1;
            smp.orbital_pair(k, second, v0, v1);
            // a large step's proposal is the uniforms themselves (second stage after a large step: the s2 rows): selects,
            // so that lanes committing a large step do not drag the wave through the per-component loop
            const float l0 = second ? smp.s2(k) : smp.u1(k), l1 = second ? smp.s2(k + 1u) : smp.u1(k + 1u);
            lds_x[k * smp.stride + smp.lane] = wrap01(smp.large ? l0 : v0);
            lds_x[(k + 1u) * smp.stride + smp.lane] = wrap01(smp.large ? l1 : v1);
        }
        return;
    }
    for (uint32_t k = k0; k < k1; ++k) lds_x[k * smp.stride + smp.lane] = smp.next(k);
}

DEV int mh_start(const DParams &P, ChainState &cs, LdsSampler &smp, PathState &ps, uint32_t n_mut, uint32_t mut_base) {
    int fill = 0;
    if (cs.stage < 0) { // next mutation
        if (cs.it >= n_mut) { ps.phase = PH_IDLE; return 0; }
        const uint32_t m = mut_base + cs.it;
        const u4 coins = philox4x32_10(P.key0, P.key1, 0u, m, smp.chain, TAG_COIN);
        cs.large = u32_to_unit(coins.x) < P.p_large;
        cs.coin_acc1 = u32_to_unit(coins.y); cs.coin_acc2 = u32_to_unit(coins.z); cs.coin_mix = u32_to_unit(coins.w);
        smp.major = m;
        smp.large = cs.large;
        cs.stage = 0;
        cs.nd1 = cs.nd2 = 0u;
        fill = 1;
    } else if (cs.stage == 1) {
        fill = 2;
    }
    smp.mode = cs.stage == 0 ? SM_STAGE1 : (cs.stage == 1 ? SM_STAGE2 : SM_REVERSE);
    path_init(P, ps);
    return fill;
}

// The half-wave exchanges of the two-lanes-per-chain kernels (k_mutate_v3, v4, w2: chain lane i, helper lane 32 + i)
DEV float from_lower(float v) { // value of lane (l & 31) for every lane l (v_permlane32_swap)
    unsigned u = __float_as_uint(v);
    return __uint_as_float(__builtin_amdgcn_permlane32_swap(u, u, false, false)[0]);
}
DEV unsigned from_lower_u(unsigned u) { return __builtin_amdgcn_permlane32_swap(u, u, false, false)[0]; }
DEV unsigned from_upper_u(unsigned u) { // value of lane 32 + (l & 31) for every lane l
    return __builtin_amdgcn_permlane32_swap(u, u, false, false)[1];
}

// The run-ahead resolution of k_mutate_v4 / v5's bookkeeping branch. (Its decide step -- digesting mh_decide's outcome into the
// cumulative weight and the three queued splats -- is written out in each kernel: as a shared function it cost the headline
// build of k_mutate_v4 its scalar-register budget)
// Between mutations (kind 4): go on while short of the target; beyond it (run-ahead, P.chain_done) while anybody in the grid is
// short, up to `limit`. Called by the whole wave; `live`: the lane owns a chain (never a helper lane of k_mutate_v4). A wave all
// of whose chains are at the target says so once (`reported`) in P.waves_left.
DEV int mh_resolve_kind(const DParams &Pm, int kind, bool live, uint32_t done_now, uint32_t target, uint32_t limit, bool &reported, uint32_t lane) {
    const bool under = __ballot(live && done_now < target) != 0ull;
    bool more = under;
    if (Pm.chain_done) {
        if (!under && !reported) { reported = true; if (lane == 0) atomicSub(Pm.waves_left, 1u); }
        if (!under) more = __builtin_amdgcn_readfirstlane((int) __hip_atomic_load(Pm.waves_left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) != 0;
    }
    if (kind == 4) kind = (done_now < target || (done_now < limit && more)) ? 1 : 0;
    return kind;
}

// k_mutate_v4's splat queue in LDS and its flush (kernels_v4.hip has the layout around it); k_mutate_v5 queues its splats through them too
struct V4Lds {
    uint32_t coin_off, list_off, q_off; // float offsets into lds_x
    uint32_t qcap;                      // queue entries (row length of the five queue rows)
};

// one colour channel of ImageBlock::put (see film_put): lanes 3s, 3s+1, 3s+2 carry the channels of splat s
DEV void film_put_channel(const DParams &P, float px, float py, float v, int ch) {
    if (P.debug & 1) return;
    float posx = px - 0.5f, posy = py - 0.5f;
    int minx = max((int) ceilf(posx - P.filter_radius), 0), miny = max((int) ceilf(posy - P.filter_radius), 0);
    int maxx = min((int) floorf(posx + P.filter_radius), P.width - 1), maxy = min((int) floorf(posy + P.filter_radius), P.height - 1);
    const bool box = P.box_weight > 0.f;
    for (int y = miny; y <= maxy; ++y) {
        const int iy = min((int) fabsf(((float) y - posy) * P.filter_scale), 31);
        float wy = box ? (iy < 31 ? P.box_weight : 0.f) : P.filter_lut[iy];
        for (int x = minx; x <= maxx; ++x) {
            const int ix = min((int) fabsf(((float) x - posx) * P.filter_scale), 31);
            float w = (box ? (ix < 31 ? P.box_weight : 0.f) : P.filter_lut[ix]) * wy;
            atomic_add_global_f32(P.film + ((size_t) y * P.width + x) * 3 + ch, w * v);
        }
    }
}

// queue a splat (all lanes call; `want` selects). ImageBlock::put's validity test (imageblock.h:155-165) is applied here.
DEV void v4_enqueue(const V4Lds &L, uint32_t &qn, bool want, float px, float py, float r, float g, float b) {
    want = want && isfinite(r) && isfinite(g) && isfinite(b) && r >= 0.f && g >= 0.f && b >= 0.f;
    const unsigned long long m = __ballot(want);
    if (want) {
        const uint32_t slot = qn + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
        float *q = &lds_x[L.q_off + slot];
        q[0] = px; q[L.qcap] = py; q[2u * L.qcap] = r; q[3u * L.qcap] = g; q[4u * L.qcap] = b;
    }
    qn += (uint32_t) __popcll(m);
}
DEV void v4_flush(const DParams &P, const V4Lds &L, uint32_t &qn, uint32_t lane) {
    const uint32_t s = lane / 3u, ch = lane - 3u * s;
    for (uint32_t base = 0u; base < qn; base += 21u) {
        const uint32_t e = base + s;
        if (e < qn && s < 21u) {
            const float *q = &lds_x[L.q_off + e];
            film_put_channel(P, q[0], q[L.qcap], q[(2u + ch) * L.qcap], (int) ch);
        }
    }
    qn = 0u;
}
