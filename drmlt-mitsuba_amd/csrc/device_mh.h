// The decision logic of the chain loops, ONE copy for every chain kernel (k_mutate_v3 / v4 / v5, k_mutate_mmlt, k_mutate_bdpt):
// the two-stage state machine (mh_digest: which rule applies at which stage, when Green goes on to the reverse move, when Mira's
// ratio is needed, when a mutation is decided and who is adopted) over the acceptance rules of both stages, the expectation
// weights, the event counters behind the seven ratios and the acceptance-map rule. The kernels differ in how a proposal is
// evaluated and where its splats live (a DSplat in registers, a list in memory); what is decided from the luminances is the same
// code, and the kernels call nothing of this file but mh_digest (k_mutate_pssmlt, another algorithm, counts with mh_count).
//
// Reference (paths relative to the checkout):
//   stage 1 (Eq. 5), doSecond gating          src/integrators/drmlt/drmlt_proc.cpp:544-558
//   Green / Mira / orbital second stage       :588-621 / :625-650 / :655-669
//   expectation weights                       :677-688
//   acceptance map                            :443-450, :693-709
//   statistics                                :711-768 (mixture :336-376)
//   processMixture                            :161-380
#pragma once
#include "device_math.h"
#include "device_types.h"

DEV bool lum_invalid(float x) { return isnan(x) || isinf(x) || x <= 0.f; }        // drmlt_proc.cpp:428
DEV bool lum_invalid_mix(float x) { return isnan(x) || isinf(x) || x < 0.f; }     // drmlt_proc.cpp:181

// Per-lane event counters of one launch, packed 2 x 16 bit (launch length is capped at 32768).
struct Counters {
    uint32_t large_acc1l; // lo: large steps                hi: accepted first stage after large
    uint32_t acc1b_secl;  // lo: accepted first stage, bold  hi: second stages after large
    uint32_t secb_acc2l;  // lo: second stages after bold    hi: accepted second stage after large
    uint32_t acc2b_rev;   // lo: accepted second, bold       hi: Green reverse evaluations
    uint32_t rays;
};

// flipCoin (drmlt_proc.cpp:419-422): x >= 1 accepts without a draw; the coins are addressed (TAG_COIN), so "without a
// draw" only means the value is not looked at
DEV bool mh_flip(float a, float coin) { return a >= 1.f || coin < a; }

// First stage: Metropolis-Hastings on the luminances (Eq. 5) and whether a second stage follows.
//   delayed rejection: after a rejected first stage, not after a large step unless timidAfterLarge (:553-558)
//   mixture:           with probability 1/2 on every non-large step, whatever the first test said (:296-299)
DEV void mh_first(bool mix, bool timid_after_large, bool large, float y_lum, float cur_lum, float coin_acc1, float coin_mix,
                  float &a1, bool &acc1, bool &do_second) {
    a1 = 0.f;
    if (!(mix ? lum_invalid_mix(y_lum) : lum_invalid(y_lum))) a1 = fminf(1.f, y_lum / cur_lum);
    acc1 = a1 > 0.f && mh_flip(a1, coin_acc1);
    if (!mix) do_second = !acc1 && (timid_after_large || !large);
    else do_second = !large && coin_mix < 0.5f;
}

// processMixture's second proposal REPLACES the first one and is tested by plain Metropolis-Hastings (:313-324)
DEV void mh_second_mixture(float z_lum, float cur_lum, float coin_acc2, float &a2, bool &acc2) {
    a2 = 0.f; acc2 = false;
    if (!lum_invalid_mix(z_lum)) {
        a2 = fminf(1.f, z_lum / cur_lum);
        acc2 = mh_flip(a2, coin_acc2);
    }
}

// Tierney & Mira (:625-650). `ratio` = Q1(y|z) / Q1(y|x) over the dimensions used (1 after a large step).
DEV void mh_second_mira(float y_lum, float z_lum, float cur_lum, float a1, float ratio, float coin_acc2, float &a2, bool &acc2) {
    a2 = 0.f; acc2 = false;
    const float aRev = fminf(1.f, y_lum / z_lum);
    if (!(aRev >= 1.f) && !lum_invalid(ratio)) {
        a2 = fminf(1.f, (z_lum / cur_lum) * ratio * (1.f - aRev) / (1.f - a1));
        acc2 = mh_flip(a2, coin_acc2);
    }
}

// pairwise orbital, DRMLT Eq. 11 (:655-669)
DEV void mh_second_orbital(float y_lum, float z_lum, float cur_lum, float coin_acc2, float &a2, bool &acc2) {
    a2 = 0.f; acc2 = false;
    if (z_lum < y_lum) return;
    if (z_lum >= cur_lum) { a2 = 1.f; acc2 = true; return; }
    a2 = (z_lum - y_lum) / (cur_lum - y_lum);
    acc2 = mh_flip(a2, coin_acc2);
}

// Green & Mira, Eq. 13-14 (:599-615): `rev_lum` = luminance of the reverse move y* = z - (y - x)
DEV void mh_second_green(float rev_lum, float z_lum, float cur_lum, float a1, float coin_acc2, float &a2, bool &acc2) {
    a2 = 0.f; acc2 = false;
    const float aRev = lum_invalid(rev_lum) ? 0.f : fminf(1.f, rev_lum / z_lum);
    if (aRev != 1.f) {
        a2 = fminf(1.f, (z_lum / cur_lum) * (1.f - aRev) / (1.f - a1));
        acc2 = mh_flip(a2, coin_acc2);
    }
}

// Expectation weights of the current state, the first-stage and the second-stage proposal (:677-688; mixture :327-333,
// where `a` is the acceptance of whichever proposal was tested). An acceptance-map run of the delayed-rejection loop
// splats no radiance (:432); the mixture loop has no such switch (:183-194).
struct MhWeights { float w0, w1, w2; };
DEV MhWeights mh_weights(bool mix, bool amap, bool do_second, float a1, float a2) {
    MhWeights w;
    if (!mix) {
        w.w1 = a1; w.w2 = (1.f - a1) * a2; w.w0 = 1.f - w.w1 - w.w2;
        if (!do_second) w.w2 = 0.f;
        if (amap) w.w0 = w.w1 = w.w2 = 0.f;
    } else {
        const float a = do_second ? a2 : a1;
        w.w0 = 1.f - a; w.w1 = do_second ? 0.f : a; w.w2 = do_second ? a : 0.f;
    }
    return w;
}

// Event counts of one decided mutation (the seven ratios of :34-49 are assembled from them on the host).
DEV void mh_count(Counters &ct, bool large, bool acc1, bool acc2, bool do_second) {
    // Every counter is updated unconditionally, by a selected VALUE. Written as `if (large) ct.a += .. else ct.b += ..` the two
    // branches were merged into one add through a selected ADDRESS, and the counters then lived in scratch memory (12 bytes per
    // lane in every chain kernel: VERDICT r03 #8).
    const bool bold = !large;
    ct.large_acc1l += (large ? 1u : 0u) + ((large && acc1) ? 1u << 16 : 0u);
    ct.acc1b_secl += ((bold && acc1) ? 1u : 0u) + ((large && do_second) ? 1u << 16 : 0u);
    ct.secb_acc2l += ((bold && do_second) ? 1u : 0u) + ((large && acc2) ? 1u << 16 : 0u);
    ct.acc2b_rev += (bold && acc2) ? 1u : 0u;
}

// Acceptance map (:693-709). The reference swaps the accepted proposal into `current` FIRST and then calls
// splatAcceptanceOnly on `proposed.first` / `proposed.second` -- which, after the swap, own the list that WAS current. The
// mark therefore goes to every splat position of the state being REPLACED: red (1,0,0) when a bold first stage was
// accepted (nothing after a large step), green (0,1,0) when the second stage was. Returns 0 none, 1 red, 2 green; the
// caller puts it at the OLD current state's positions. processMixture draws no map.
enum { AMAP_NONE = 0, AMAP_RED = 1, AMAP_GREEN = 2 };
DEV int mh_amap_mark(bool mix, bool amap, bool large, bool acc1, bool acc2) {
    if (!amap || mix || !(acc1 || acc2)) return AMAP_NONE;
    return acc1 ? (large ? AMAP_NONE : AMAP_RED) : AMAP_GREEN;
}
DEV f3 mh_amap_colour(int mark) { return mark == AMAP_RED ? mk3(1.f, 0.f, 0.f) : mk3(0.f, 1.f, 0.f); }

// ------------------------------------------------------------------------------------------ the two-stage state machine
// Rule switches of a render, wave-uniform: built by the caller from the parameter copy of the loop section it is in.
struct MhRules {
    bool mix, amap, timid_after_large;
    int type; // 0 Green, 1 Mira, 2 orbital
};
// Outcome of one digested evaluation. !decided: `stage` has been advanced (1: second stage, 2: Green's reverse move) and the
// chain evaluates again. decided: the mutation is over -- acc1 / acc2: the first- / second-stage proposal is adopted; w: the
// expectation weights of the current state and the two proposals; amap: the acceptance-map mark (AMAP_*) for the state that is
// being REPLACED (mh_amap_mark).
struct MhDigest {
    bool decided, acc1, acc2;
    int amap;
    MhWeights w;
};

// DRMLTRenderer::process / processMixture from the end of one evaluation to the next (drmlt_proc.cpp:518-770, 161-380).
// `lum` is the luminance of the evaluation just finished: of y at stage 0, of z at stage 1, of the reverse move y* at stage 2;
// y_lum / z_lum are those of the stages before it. `mira_ratio()` yields Q1(y|z) / Q1(y|x) and is called only when the rule
// needs it: after a large step both proposals are uniform (ratio 1), and with min(1, y/z) >= 1 the rule rejects without it.
// Counts the decided mutation (and every reverse evaluation) in `ct`; the mutation counter, the sampler state and the splats
// belong to the caller.
// RULE (device_types.h): under RULE_ORBITAL the rule switches are compile-time constants -- mix, amap and the Green / Mira arms are
// dead code, `stage` never reaches 2 -- and R's mix / amap / type are not read; the default compiles to the generic routine.
template <int RULE = RULE_GENERIC, class MiraRatio>
DEV MhDigest mh_digest(const MhRules R, bool large, float coin_acc1, float coin_acc2, float coin_mix, float lum, float cur_lum,
                       float y_lum, float z_lum, float &a1, int &stage, Counters &ct, MiraRatio mira_ratio) {
    constexpr bool orbital = RULE == RULE_ORBITAL;
    const bool mix = orbital ? false : R.mix, amap = orbital ? false : R.amap;
    const int type = orbital ? 2 : R.type;
    MhDigest d{false, false, false, AMAP_NONE, {0.f, 0.f, 0.f}};
    float a2 = 0.f;
    if (stage == 0) {
        bool do_second = false;
        mh_first(mix, R.timid_after_large, large, lum, cur_lum, coin_acc1, coin_mix, a1, d.acc1, do_second);
        if (do_second) { d.acc1 = false; stage = 1; return d; }
    } else if (orbital || stage == 1) {
        if (mix) {
            a1 = 0.f; // the second proposal replaces the first
            mh_second_mixture(lum, cur_lum, coin_acc2, a2, d.acc2);
        } else if (!lum_invalid(lum)) {
            if (type == 0) { stage = 2; return d; } // Green: evaluate the reverse move first
            if (type == 1) {
                float ratio = 1.f;
                if (!large && !(fminf(1.f, y_lum / lum) >= 1.f)) ratio = mira_ratio();
                mh_second_mira(y_lum, lum, cur_lum, a1, ratio, coin_acc2, a2, d.acc2);
            } else {
                mh_second_orbital(y_lum, lum, cur_lum, coin_acc2, a2, d.acc2);
            }
        }
    } else {
        ct.acc2b_rev += 1u << 16;
        mh_second_green(lum, z_lum, cur_lum, a1, coin_acc2, a2, d.acc2);
    }
    const bool do_second = stage != 0;
    d.decided = true;
    d.w = mh_weights(mix, amap, do_second, a1, a2);
    mh_count(ct, large, d.acc1, d.acc2, do_second);
    d.amap = mh_amap_mark(mix, amap, large, d.acc1, d.acc2);
    return d;
}
