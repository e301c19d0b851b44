// Host-only launch plan of the chain kernels: every DRMLT_* knob the library reads (read_knobs, once per context), the LDS
// formulas the kernels are laid out by, and the one function that picks a chain-kernel build, its grid and its LDS bytes
// (plan_chains). drmlt_create computes the plan once and the launchers only dispatch on it. No HIP headers: the plan
// is pinned down on the CPU (tests/native/plan_harness.cpp), and the device code includes this file for the constants.
#pragma once
#include "../../include/drmlt_abi.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

// ---- LDS layout constants and formulas (kernels_v3.hip, kernels_v4.hip, kernels_mmlt.hip, kernels_bdpt.hip, kernels_pssmlt_bdpt.hip)
constexpr uint32_t V4_STRIDE = 33u;   // row stride of the sampler rows: (row + chain) mod 32 banks serve per-chain AND per-dimension access patterns
constexpr uint32_t V4_QCAP = 160u;    // splat queue entries: flushed when a bookkeeping branch (at most 2 x 32 new entries) might not fit
constexpr uint32_t V4_QCAP_BVH = 100u; // BVH scenes: their kernel also keeps the traversal stack in LDS (6 KB); flushes are a negligible part of it
constexpr uint32_t V5_QCAP = 96u;     // splat queue entries (a round of the bookkeeping branch adds at most 64: flushed in between)
constexpr uint32_t V5_QCAP_STACK32 = 0u; // the builds with 32-bit traversal stacks splat straight from the bookkeeping branch: their LDS goes to the stack column
constexpr uint32_t V5_SLOTS = 128u;

// LDS floats of a bdpt evaluation beside the sampler rows: the two density row groups and the 64 segment heads of a connection round
constexpr int bdpt_eval_lds_floats(int max_depth) { return (2 * (2 * max_depth + 1) + 1) * 64; }

// dynamic LDS bytes per wave (+ the scene tables, when they are staged)
inline size_t v3_lds_bytes(size_t D) { return (D + 2 * ((D + 3) & ~(size_t) 3)) * 32 * sizeof(float); }
// (k_mutate_v4: three row groups of D4 = D rounded up to 4 rows each; the D4 - D rows this formula does not count are taken from
// the queue rows, which are up to 20 entries shorter than `qcap` -- v4_layout, kernels_v4.hip)
inline size_t v4_lds_bytes(size_t D, size_t qcap) { return ((D + 2 * ((D + 3) & ~(size_t) 3) + 4) * V4_STRIDE + 32 + 5 * qcap + 3) / 4 * 4 * sizeof(float); }
inline size_t v5_lds_bytes(uint32_t D, uint32_t qcap, bool coin_rows) { return ((size_t) D * 64u + (coin_rows ? 4u * 64u : 0u) + 64u + 5u * qcap + 8u * V5_SLOTS + 2u * (V5_SLOTS / 4u)) * sizeof(float); }
inline size_t mmlt_lds_bytes(int mmlt_S, int mmlt_E, int max_depth) { return ((size_t) mmlt_S + mmlt_E + 1 + 3 * ((size_t) max_depth + 3)) * 64 * sizeof(float); }
inline size_t bdpt_lds_bytes(int mmlt_S, int mmlt_E, int max_depth) { return (((size_t) mmlt_S + mmlt_E) * 64 + (size_t) bdpt_eval_lds_floats(max_depth)) * sizeof(float); }

// ---- knobs: every DRMLT_* environment variable of the library (drmlt_node.cpp's node-level hooks aside), read once per context
struct Knobs {
    bool verbose = false;                    // DRMLT_VERBOSE
    int debug = 0;                           // DRMLT_DEBUG: bit mask (diagnostics)
    int kernel = 0;                          // DRMLT_KERNEL: 3, 4 or 5 (any other value: 4); 0 = the default choice
    int slice = 1024;                        // DRMLT_SLICE: mutations per chain per launch, 1..32768 (16-bit event counters per lane)
    int bvh_threshold = 48, bvh_max_depth = 64, bvh_leaf = 1; // DRMLT_BVH_THRESHOLD, DRMLT_BVH_MAX_DEPTH (<= 64), DRMLT_BVH_LEAF (bvh_build.h: 1..4)
    bool bvh_stack32 = false;                // DRMLT_BVH_STACK32
    bool no_quad_merge = false, no_box_merge = false, no_flat_loop = false, feat_all = false; // DRMLT_NO_QUAD_MERGE, _NO_BOX_MERGE, _NO_FLAT_LOOP, _FEAT_ALL
    bool tables_lds_off = false;             // DRMLT_TABLES_LDS=0: scene tables in device memory
    int mh_batch = 0, trace_yield = -1, pool_refill = 0, trace_vote = 0; // DRMLT_MH_BATCH, _TRACE_YIELD, _POOL_REFILL, _TRACE_VOTE; 0 / -1: the plan's
    int rows_mem = -1;                       // DRMLT_ROWS_MEM=0|1: k_mutate_v5's proposal rows in LDS / device memory; -1 = by the chain count
    bool no_small_tables = false, mmlt_tables_global = false, bdpt_tables_global = false; // DRMLT_NO_SMALL_TABLES, _MMLT_TABLES_GLOBAL, _BDPT_TABLES_GLOBAL
    int bdpt_occ = 0;                        // DRMLT_BDPT_OCC=1|2: waves per SIMD of k_mutate_bdpt; 0 = by the grid and the LDS
    size_t bdpt_lds_pad = 0;                 // DRMLT_BDPT_LDS_PAD: extra LDS bytes of every bdpt kernel (occupancy experiments)
    bool no_run_ahead = false;               // DRMLT_NO_RUN_AHEAD
    bool rule_generic = false;               // DRMLT_RULE_GENERIC: k_mutate_v4 runs its generic body whatever the rule (device_types.h: rule_is_orbital)
    bool no_w2 = false;                      // DRMLT_NO_W2: the orbital one-light launches of V4_F0 stay on k_mutate_v4's twin (kernels_v4.hip: k_mutate_w2)
    bool no_w2_held = false;                 // DRMLT_NO_W2_HELD: k_mutate_w2 keeps streaming its ray records where k_mutate_w2h would hold them in registers (w2_held_launch below)
    bool one_light_generic = false;          // DRMLT_ONE_LIGHT_GENERIC: k_mutate_v4 reads the light from the staged tables however many the scene has (device_types.h: scene_has_one_light)
    long long ahead_cap = -1;               // DRMLT_AHEAD_CAP: mutations a chain may run beyond the launch's target; -1 = min(8 slices, 8192)
    bool mmlt_no_sort = false, no_regroup = false, regroup_on_host = false, regroup_check = false; // DRMLT_MMLT_NO_SORT, _NO_REGROUP, _REGROUP_ON_HOST, _REGROUP_CHECK
    int regroup_first = 0;                   // DRMLT_REGROUP_FIRST: length of a call's first launch when regrouping, 1..slice; 0 = by the call
};

inline Knobs read_knobs() {
    Knobs K;
    const struct { const char *name; bool *on; } flags[] = {
        {"DRMLT_VERBOSE", &K.verbose}, {"DRMLT_BVH_STACK32", &K.bvh_stack32}, {"DRMLT_NO_QUAD_MERGE", &K.no_quad_merge}, {"DRMLT_NO_BOX_MERGE", &K.no_box_merge},
        {"DRMLT_NO_FLAT_LOOP", &K.no_flat_loop}, {"DRMLT_FEAT_ALL", &K.feat_all}, {"DRMLT_NO_SMALL_TABLES", &K.no_small_tables},
        {"DRMLT_MMLT_TABLES_GLOBAL", &K.mmlt_tables_global}, {"DRMLT_BDPT_TABLES_GLOBAL", &K.bdpt_tables_global}, {"DRMLT_NO_RUN_AHEAD", &K.no_run_ahead},
        {"DRMLT_RULE_GENERIC", &K.rule_generic}, {"DRMLT_ONE_LIGHT_GENERIC", &K.one_light_generic}, {"DRMLT_NO_W2", &K.no_w2}, {"DRMLT_NO_W2_HELD", &K.no_w2_held},
        {"DRMLT_MMLT_NO_SORT", &K.mmlt_no_sort}, {"DRMLT_NO_REGROUP", &K.no_regroup}, {"DRMLT_REGROUP_ON_HOST", &K.regroup_on_host}, {"DRMLT_REGROUP_CHECK", &K.regroup_check}};
    for (const auto &f : flags) *f.on = getenv(f.name) != nullptr;
    int v = 0;
    auto num = [&v](const char *name) { const char *e = getenv(name); if (e) v = atoi(e); return e != nullptr; };
    if (num("DRMLT_DEBUG")) K.debug = v;
    if (num("DRMLT_KERNEL")) K.kernel = v == 3 ? 3 : (v == 5 ? 5 : 4);
    if (num("DRMLT_SLICE")) K.slice = std::max(1, std::min(32768, v));
    if (num("DRMLT_BVH_THRESHOLD")) K.bvh_threshold = v;
    if (num("DRMLT_BVH_MAX_DEPTH")) K.bvh_max_depth = std::min(K.bvh_max_depth, v);
    if (num("DRMLT_BVH_LEAF")) K.bvh_leaf = v;
    if (num("DRMLT_TABLES_LDS")) K.tables_lds_off = v == 0;
    if (num("DRMLT_MH_BATCH")) K.mh_batch = std::max(1, std::min(64, v));
    if (num("DRMLT_TRACE_YIELD")) K.trace_yield = std::max(0, std::min(64, v));
    if (num("DRMLT_POOL_REFILL")) K.pool_refill = std::max(1, std::min(64, v));
    if (num("DRMLT_TRACE_VOTE")) K.trace_vote = std::max(1, std::min(1024, v));
    if (num("DRMLT_ROWS_MEM")) K.rows_mem = v != 0;
    if (num("DRMLT_BDPT_OCC")) K.bdpt_occ = v;
    if (num("DRMLT_BDPT_LDS_PAD")) K.bdpt_lds_pad = (size_t) v;
    if (num("DRMLT_AHEAD_CAP")) K.ahead_cap = std::max(0, v);
    if (num("DRMLT_REGROUP_FIRST")) K.regroup_first = std::max(1, std::min(K.slice, v));
    return K;
}

// ---- what the decisions rest on (drmlt_create fills it from the configuration and the flattened scene)
struct PlanInputs {
    int technique = DRMLT_TECH_PATH, algo = DRMLT_ALGO_DRMLT;
    int work_units = -1, work_units_rule = DRMLT_WORK_UNITS_DEVICE;
    uint64_t budget = 0;                          // width x height x sampleCount
    int features = 0;                             // DParams::features (after DRMLT_FEAT_ALL)
    bool use_bvh = false, bvh_stack16 = false;
    bool bvh_overflow = false;                    // the traversal stacks have an overflow area (ovf_entries > 0)
    uint32_t n_shade = 0, n_bsdfs = 0, n_emitters = 0;
    uint64_t scene_bytes = 0;                     // 4-wide nodes + intersection records (BVH scenes)
    int eff_dim = 0, max_depth = 0, mmlt_S = 0, mmlt_E = 0;
    int cus = 256;                                // compute units of the device
    int n_box = 0, n_flat_rec = 0;                // records of the brute-force ray loop: cuboids, flat records that are no cuboid's face (flat scenes)
    bool has_plain_tri = false;                   // any PRIM_TRIANGLE record among the flat ones
};

// one enumerator per chain-kernel instantiation that is launched (the launchers' switch statements name the template arguments)
enum class Build {
    PSSMLT,
    V5_F0_ROWS, V5_F1_ROWS, V5_F3_ROWS, V5_F7_ROWS,
    V5_F7_GLOBAL, V5_F0_STAMPS, V5_F0, V5_F1, V5_F3, V5_F7,
    V5_F8_S32_ROWS, V5_F15_S32_ROWS, V5_F8_OVF_ROWS, V5_F15_OVF_ROWS, V5_F8_ROWS, V5_F15_ROWS,
    V5_F8_S32, V5_F15_S32, V5_F8_OVF, V5_F15_OVF, V5_F8_STAMPS, V5_F8, V5_F15,
    V4_F0_STAMPS, V4_F0, V4_F3_STAMPS, V4_F3, V4_F7, V4_F15_S32, V4_F15_OVF, V4_F15,
    V4_F7_GLOBAL, V4_F8_S32_GLOBAL, V4_F15_S32_GLOBAL, V4_F15_OVF_GLOBAL, V4_F15_STAMPS_GLOBAL, V4_F8_GLOBAL, V4_F15_GLOBAL,
    V3_F0, V3_F3, V3_F7, V3_F15, V3_F15_GLOBAL,
    MMLT_F7_TABLES, MMLT_F15, MMLT_F7,
    BDPT_F15, BDPT_F7_OCC2_TABLES, BDPT_F7_OCC2, BDPT_F7,
    PSSMLT_BDPT_F15, PSSMLT_BDPT_F7_OCC2_TABLES, PSSMLT_BDPT_F7_OCC2, PSSMLT_BDPT_F7, // algo=pssmlt over technique=bdpt (kernels_pssmlt_bdpt.hip)
};

struct ChainPlan {
    Build build = Build::PSSMLT;
    uint32_t chains_per_wave = 64, grid = 0; // workgroups of one wave each
    size_t lds = 0;                          // dynamic LDS bytes of the chain kernel
    size_t aux_lds = 0;                      // ... of the technique's bootstrap / seed replay / evaluation kernels (mmlt, bdpt)
    int kernel_variant = 5, tables_in_lds = 0, small_tables_lds = 0;
    bool rows_mem = false;                   // k_mutate_v5's proposal rows in device memory (three waves per SIMD)
    int mh_batch = 0, trace_yield = 0, pool_refill = 0, trace_vote = 0;
    bool w2 = false;                         // V4_F0 only: launch_mutate may run k_mutate_w2 in place of the orbital one-light twin (w2_launch below)
    bool w2_held = false;                    // ... and then k_mutate_w2h in place of k_mutate_w2: the scene's ray records fit its registers (w2_held_launch below)
    bool run_ahead = false;                  // drmlt_run: chains run beyond a launch's target towards the call's total
    bool verbose = false;
    std::string note;                        // the DRMLT_VERBOSE line of the path kernels' launches
};

namespace plan_detail {
inline size_t lds_table_bytes(const PlanInputs &in) { return (size_t) in.n_shade * 64 + (size_t) in.n_bsdfs * 48 + (size_t) in.n_emitters * 32; }
inline size_t small_table_bytes(const PlanInputs &in) { return ((size_t) in.n_bsdfs * 12 + (size_t) in.n_emitters * 24) * sizeof(float); }
inline bool path_mh(const PlanInputs &in) { return in.technique == DRMLT_TECH_PATH && in.algo != DRMLT_ALGO_PSSMLT; }

// The family of technique=path's chain kernel at n chains: the rule derive_chains and plan_chains share.
// (The ray-pool kernel v5 keeps ONE proposal row group in LDS; on flat scenes it needs two of its 64-chain waves on a SIMD: from
// 98 304 chains up it is the default -- Cornell: v5 2.15e9 at 131 072 chains, 1.11e9 at 65 536; v4 1.79e9 at 65 536, 1.55e9 at
// 131 072. BASELINE's config 2 fixes 65 536 chains and therefore runs k_mutate_v4. With chains for more than two waves per SIMD
// (from 163 840 per 256 CUs) its proposal rows move to device memory and it is built for three waves per SIMD: kernels_v4.hip, ROWS_MEM.)
// k_mutate_w2 (kernels_v4.hip) is compiled for two waves per SIMD and spends the registers of a third on constants it would otherwise
// re-read. It may replace a launch that can never have a third wave on a SIMD, for one of two reasons: the workgroup's LDS
// exceeds a twelfth of a compute unit's 160 KB (four SIMDs x three waves), or the grid has no more than two waves per SIMD
// of the device. The ONE place the condition is written down.
constexpr size_t CU_LDS_BYTES = 160u * 1024u;
inline bool w2_launch(size_t lds, uint32_t grid, int cus) { return lds * 12u > CU_LDS_BYTES || (uint64_t) grid <= (uint64_t) cus * 4u * 2u; }
// k_mutate_w2h (kernels_v4.hip) is k_mutate_w2 with the scene's ray records held in vector registers: room for three cuboids and one
// flat record, tested without the plain-triangle arm. A scene without cuboids gains nothing from it (cornell_c1: three flat
// records) and keeps streaming. The ONE place the condition is written down.
// k_mutate_w2h's code leans on two things that follow from it (and from w2_launch's one-light condition): there is a cuboid in slot 0
// (n_box >= 1: trace_held tests it without a guard), and the light is a RECTANGLE (no plain triangle among the flat records, and a
// triangle that emits is always one: device_path.h, HeldLightTablesT -- the step is compiled without the triangle light's arm).
// Whoever widens the condition takes both back.
inline bool w2_held_launch(int n_box, int n_flat_rec, bool has_plain_tri) { return n_box >= 1 && n_box <= 3 && n_flat_rec >= 0 && n_flat_rec <= 1 && !has_plain_tri; }

struct Family { int variant; bool tables_in_lds, rows_mem; };
inline Family family(const PlanInputs &in, uint32_t n_chains, const Knobs &K) {
    Family f;
    f.tables_in_lds = lds_table_bytes(in) <= 16384 && !K.tables_lds_off; // small tables ride in LDS (Cornell class); 16 KB keeps 4+ waves per CU
    f.variant = K.kernel ? K.kernel : 5;
    if (f.variant == 5 && !in.use_bvh && K.kernel != 5 && n_chains < 98304u) f.variant = 4;
    const bool can = f.variant == 5 && (in.use_bvh || f.tables_in_lds) && path_mh(in);
    f.rows_mem = can && (K.rows_mem >= 0 ? K.rows_mem == 1 : (uint64_t) n_chains * 2u >= (uint64_t) in.cus * 4u * 64u * 5u);
    return f;
}
} // namespace plan_detail

// workUnits = -1 (the default): the chain count that fills the device. The reference sizes work units for its CPU scheduler --
// 200 000 (path) or 100 000 (mmlt, bdpt) mutations each, drmlt.cpp:434-444 -- a few hundred chains for a whole image;
// work_units_rule = DRMLT_WORK_UNITS_REFERENCE restores that formula. The device's counts, never chains shorter than 64 mutations:
// - path: 196 608 when the pool kernel runs three 64-chain waves per SIMD at that count (traversed scenes, whose node fetches the
//   extra wave covers, + 4 % (2000 triangles) ... + 17 % (50 000, 1 000 000); flat scenes + 20 %: DESIGN section 6), else 131 072
//   (two waves of the pool kernel); 65 536 for a kernel chosen by DRMLT_KERNEL and for pssmlt (over path and over bdpt);
// - bdpt: 131 072 (one chain per lane; its workspace is 2 KB per chain and loses with more than fill the device);
// - mmlt: MANY rounds of waves, run in depth order -- 262 144 chains 2.56e9 mutations/s on BASELINE's config 5, 524 288 2.79e9,
//   1 048 576 2.91e9. The price is paid before the first mutation: 50 x maxDepth bootstrap samples per chain (drmlt.cpp:456-473),
//   2.3 s of seeding for a million chains at maxDepth 6 against 0.6 s for 262 144. A render gets the million chains from 2^35
//   mutations (12 s of kernel time) up.
// An explicit workUnits is taken as given.
inline uint32_t derive_chains(const PlanInputs &in, const Knobs &K) {
    if (in.work_units > 0) return (uint32_t) in.work_units;
    const bool mmlt = in.technique == DRMLT_TECH_MMLT, bdpt = in.technique == DRMLT_TECH_BDPT;
    if (in.work_units_rule == DRMLT_WORK_UNITS_REFERENCE) {
        const uint64_t per_unit = (mmlt || bdpt) ? 100000 : 200000;
        return (uint32_t) std::max<uint64_t>(1, (in.budget + per_unit - 1) / per_unit);
    }
    uint64_t fill = 65536;
    if (in.algo == DRMLT_ALGO_PSSMLT) fill = 65536;
    else if (mmlt) fill = in.budget >= (1ull << 35) ? 1048576 : 262144;
    else if (bdpt) fill = 131072;
    else if (plan_detail::path_mh(in) && !K.kernel) fill = plan_detail::family(in, 196608, K).rows_mem ? 196608 : 131072;
    return (uint32_t) std::min<uint64_t>(fill, std::max<uint64_t>(64, in.budget / 64 / 64 * 64));
}

inline ChainPlan plan_chains(const PlanInputs &in, uint32_t n_chains, const Knobs &K) {
    using namespace plan_detail;
    ChainPlan p;
    const Family f = family(in, n_chains, K);
    const bool mmlt = in.technique == DRMLT_TECH_MMLT, bdpt = in.technique == DRMLT_TECH_BDPT, pssmlt = in.algo == DRMLT_ALGO_PSSMLT;
    const bool bvh = in.use_bvh, s16 = in.bvh_stack16, ovf = in.bvh_overflow, stamps = (K.debug & 128) != 0;
    const int F = in.features;
    p.kernel_variant = f.variant;
    p.tables_in_lds = f.tables_in_lds;
    p.rows_mem = f.rows_mem;
    p.verbose = K.verbose;
    // A scene whose nodes and records exceed the L2 caches (8 x 4 MB) is traversed against memory latency: the ray pool then wants
    // SHORT phases -- chains step and refill it as soon as a few rays are done (1 000 000 triangles, 2-step calls: yield x batch
    // 20 x 16 6.9e7, 12 x 8 7.5e7, 8 x 8 7.7e7, 4 x 8 7.7e7 mutations/s; 50 000 triangles, in the L2s: 2.82e8 / 2.75e8 / 2.61e8)
    const bool beyond_l2 = bvh && in.scene_bytes > ((uint64_t) 32 << 20);
    // parked chains before the bookkeeping branch (v5 on the Cornell scene, 131 072 chains: batch 16 1.98e9, 24 2.08e9, 32 2.13e9, 48 1.84e9;
    // on the soup: 8 5.05e8, 16 5.24e8, 32 5.06e8; round 4, with the cuboid records: v4 on config 2 batch 8 1.99e9, 12 2.02e9, 14 2.05e9,
    // 16 2.04e9, 20 1.94e9; v5 on the same scene at 131 072 chains 24 2.33e9, 32 2.39e9, 40 2.42e9, 48 2.36e9)
    p.mh_batch = K.mh_batch ? K.mh_batch : f.variant == 5 ? (bvh ? (beyond_l2 ? 8 : 16) : 40) : f.variant == 4 ? (bvh ? (s16 ? 6 : 4) : (F == 0 ? 14 : 8)) : 32;
    // k_mutate_v5 on traversed scenes: room for the small tables beside the pool? LDS per wave without them: 20 480 B in the builds with
    // 32-bit stacks and rows in LDS (none), 19.5 KB with 16-bit stacks, 11.5 / 10.8 KB with the rows in device memory (twelve waves per CU: 13 KB)
    const size_t room = f.rows_mem ? (s16 ? 1536 : 1024) : (s16 ? 768 : 0);
    p.small_tables_lds = bvh && f.variant == 5 && small_table_bytes(in) <= room && !K.no_small_tables;
    // rays that end a trace phase (measured, 5-launch calls, on the 2000-triangle soup: 16 3.69e8, 20 3.80e8, 24 3.84e8, 28 3.84e8 mutations/s;
    // on 50 000 triangles (32-bit stacks, longer traversals): 20 1.90e8, 24 1.86e8, 28 1.79e8; k_mutate_v5 (131 072 chains, 3-step calls) on
    // the soup, yield x bookkeeping batch -- 12: 4.84 / 5.13 / 5.12e8 (batch 8 / 16 / 28), 16: 5.08 / 5.37 / 5.20, 20: 5.25 / 5.44 / 5.10, 24: 5.31 / 5.40 / 4.81)
    p.trace_yield = K.trace_yield >= 0 ? K.trace_yield : f.variant == 5 ? (beyond_l2 ? 8 : 20) : (s16 ? 24 : 20);
    p.pool_refill = K.pool_refill ? K.pool_refill : 8; // soup, 131 072 chains: 1 5.38e8, 2 5.41e8, 4 5.43e8, 8 5.45e8, 16 5.37e8 mutations/s
    p.trace_vote = K.trace_vote ? K.trace_vote : 10;   // the 2000-triangle soup: 16 (plain majority) 2.70e8, 10 2.78e8, 5 2.73e8 mutations/s
    p.run_ahead = path_mh(in) && f.variant >= 4 && !K.no_run_ahead;

    const size_t D = (size_t) in.eff_dim, tables = f.tables_in_lds ? lds_table_bytes(in) : 0;
    auto waves = [&](uint32_t per_wave) { p.chains_per_wave = per_wave; p.grid = (n_chains + per_wave - 1) / per_wave; };
    char note[160];
    note[0] = 0;
    if (mmlt) { // tables in LDS where they and the rows still fit eight waves (20 KB)
        waves(64);
        p.aux_lds = p.lds = mmlt_lds_bytes(in.mmlt_S, in.mmlt_E, in.max_depth);
        const size_t tb = ((size_t) in.n_shade * 16 + (size_t) in.n_bsdfs * 12 + (size_t) in.n_emitters * 8) * sizeof(float);
        if (!bvh && f.tables_in_lds && !K.mmlt_tables_global && p.lds + tb <= 20480) p.build = Build::MMLT_F7_TABLES, p.lds += tb;
        else p.build = bvh ? Build::MMLT_F15 : Build::MMLT_F7;
    } else if (bdpt) { // two waves per SIMD on flat scenes with more than 1280 waves, when the rows leave room for them
        waves(64);
        p.aux_lds = p.lds = K.bdpt_lds_pad + bdpt_lds_bytes(in.mmlt_S, in.mmlt_E, in.max_depth);
        const bool two = K.bdpt_occ ? K.bdpt_occ == 2 : (!bvh && p.grid > 1024u + 256u && p.lds <= 20480);
        const size_t tb = ((size_t) in.n_bsdfs * 12 + (size_t) in.n_emitters * (8 + 16)) * sizeof(float); // BSDFs, emitters, the emitters' shape records
        if (bvh) p.build = Build::BDPT_F15;
        else if (two && !K.bdpt_tables_global && p.lds + tb <= 20480) p.build = Build::BDPT_F7_OCC2_TABLES, p.lds += tb;
        else p.build = two ? Build::BDPT_F7_OCC2 : Build::BDPT_F7;
        if (pssmlt) // k_mutate_pssmlt_bdpt: the same rows, the same tables, the same occupancy rule -- its own loop
            p.build = p.build == Build::BDPT_F15 ? Build::PSSMLT_BDPT_F15 : p.build == Build::BDPT_F7_OCC2_TABLES ? Build::PSSMLT_BDPT_F7_OCC2_TABLES
                    : p.build == Build::BDPT_F7_OCC2 ? Build::PSSMLT_BDPT_F7_OCC2 : Build::PSSMLT_BDPT_F7;
    } else if (pssmlt) {
        waves(64);
        p.lds = D * 64 * sizeof(float);
        p.build = Build::PSSMLT;
    } else if (f.variant == 5) { // ray pool, 64 chains per wave
        waves(64);
        const bool flat = (F & 8) == 0, diffuse = F == 8;
        p.lds = v5_lds_bytes(f.rows_mem ? 0u : (uint32_t) D, (flat || s16) ? V5_QCAP : V5_QCAP_STACK32, flat || s16);
        if (flat) p.lds += tables;
        else if (p.small_tables_lds) p.lds += small_table_bytes(in);
        snprintf(note, sizeof note, "[drmlt] k_mutate_v5: %zu B of LDS per wave%s%s", p.lds, flat ? "" : " (+ the traversal stack)",
                 f.rows_mem ? "; proposal rows in device memory, three waves per SIMD" : "");
        if (flat && f.rows_mem) p.build = F == 0 ? Build::V5_F0_ROWS : F == 1 ? Build::V5_F1_ROWS : (F & ~3) == 0 ? Build::V5_F3_ROWS : Build::V5_F7_ROWS;
        else if (flat && !f.tables_in_lds) p.build = Build::V5_F7_GLOBAL;
        else if (flat) p.build = F == 0 ? (stamps ? Build::V5_F0_STAMPS : Build::V5_F0) : F == 1 ? Build::V5_F1 : (F & ~3) == 0 ? Build::V5_F3 : Build::V5_F7;
        else if (f.rows_mem) p.build = !s16 ? (diffuse ? Build::V5_F8_S32_ROWS : Build::V5_F15_S32_ROWS) : ovf ? (diffuse ? Build::V5_F8_OVF_ROWS : Build::V5_F15_OVF_ROWS)
                                                                  : (diffuse ? Build::V5_F8_ROWS : Build::V5_F15_ROWS);
        else p.build = !s16 ? (diffuse ? Build::V5_F8_S32 : Build::V5_F15_S32) : ovf ? (diffuse ? Build::V5_F8_OVF : Build::V5_F15_OVF)
                                                        : diffuse ? (stamps ? Build::V5_F8_STAMPS : Build::V5_F8) : Build::V5_F15;
    } else if (f.variant == 4) { // free-running chains, flattened bookkeeping, queued splats (rows of 33 floats), 32 chains per wave
        waves(32);
        p.lds = v4_lds_bytes(D, (F & 8) ? V4_QCAP_BVH : V4_QCAP) + tables;
        snprintf(note, sizeof note, "[drmlt] k_mutate_v4: %zu B of LDS per wave", p.lds);
        // BVH: 32-bit stacks always run the build with the spill / refill paths (short LDS column), 16-bit stacks only for trees
        // deeper than their column. Flat scenes with tables too large for LDS (many point lights) run V4_F7_GLOBAL: the BVH builds
        // would traverse a tree the scene does not have -- their resumable traversal reads P.bvh whatever P.use_bvh says.
        if (f.tables_in_lds)
            p.build = F == 0 ? (stamps ? Build::V4_F0_STAMPS : Build::V4_F0) : (F & ~3) == 0 ? (stamps ? Build::V4_F3_STAMPS : Build::V4_F3)
                    : (F & 8) == 0 ? Build::V4_F7 : !s16 ? Build::V4_F15_S32 : ovf ? Build::V4_F15_OVF : Build::V4_F15;
        else
            p.build = (F & 8) == 0 ? Build::V4_F7_GLOBAL : !s16 ? (F == 8 ? Build::V4_F8_S32_GLOBAL : Build::V4_F15_S32_GLOBAL) : ovf ? Build::V4_F15_OVF_GLOBAL
                    : stamps ? Build::V4_F15_STAMPS_GLOBAL : F == 8 ? Build::V4_F8_GLOBAL : Build::V4_F15_GLOBAL;
        p.w2 = p.build == Build::V4_F0 && !K.no_w2 && w2_launch(p.lds, p.grid, in.cus);
        p.w2_held = p.w2 && !K.no_w2_held && w2_held_launch(in.n_box, in.n_flat_rec, in.has_plain_tri);
    } else { // k_mutate_v3, the cross-check: 32 chains per wave, rows of 32 floats; 0 = diffuse polygons, 3 = + rough conductor /
             // dielectric, 7 = + spheres, 15 = everything (BVH traversal); large scenes (tables in device memory): one general variant
        waves(32);
        p.lds = v3_lds_bytes(D) + tables;
        snprintf(note, sizeof note, "[drmlt] k_mutate_v3: %zu B of LDS per wave", p.lds);
        p.build = !f.tables_in_lds ? Build::V3_F15_GLOBAL : F == 0 ? Build::V3_F0 : (F & ~3) == 0 ? Build::V3_F3 : (F & 8) == 0 ? Build::V3_F7 : Build::V3_F15;
    }
    p.note = note;
    return p;
}
