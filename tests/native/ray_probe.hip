// Calls the device's ray loops one ray per lane and writes the hits they return (tests/ray_probe.py builds and runs it,
// tests/test_gpu_rays.py checks the numbers). Nothing but the library's own headers; the parameter block and the tables are the
// bytes tests/native/scene_prep_harness.cpp writes for a scene, i.e. what the library would upload. One process: one scene, one
// ray list, any number of ops.
//
//   ray_probe <request> <result>
// request: int32 magic, n, n_ops, n_prims, n_shade, n_bvh, n_flat (records with the two sentinels), n_boxes (records with the
//          sentinel), ovf_entries, trace_vote, sizeof(DParams), 0 x 5; the DParams block (pointers null); the DPrim, DShade,
//          DBvh4Node, DPrimFlat and DPrimBox tables; n rows of 9 float32 (o, d, tmin, tmax, any_hit); n_ops int32.
// result:  per op n rows of (prim as int32, t, u, v as float32).
//   trace15      trace<15> (the dispatcher, following P)        trace0   trace<0> (k_mutate_w2's; flat scenes only)
//   brute        trace_brute<15>                                brute_vec  the same under P.debug | 64 (vector-memory loads)
//   held         trace_held over plain field copies of prims_box[0 .. n_box) and prims_flat[0] (scenes w2_held_launch accepts)
//   bvh32        trace_bvh                                      bvh16    trav_run<short, DParams, true, BVH_STACK, 15>
//   bvh32_cap12  trav_run<int, DParams, true, 12, 15>
// One wave per workgroup (trav_run owns a __shared__ column per lane of one wave and votes with __ballot); no lane returns before
// a loop: a lane beyond n traces a copy of the last ray and only its store is masked.
// main() checks every index the device will follow before it touches HIP, and refuses an op the tables do not support: exit
// status 2. A HIP error is exit status 3.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "device_path.h"
#include "launch_plan.h"

enum { OP_TRACE15, OP_TRACE0, OP_BRUTE, OP_BRUTE_VEC, OP_HELD, OP_BVH32, OP_BVH16, OP_BVH32_CAP12, N_OPS };
#define RAY_PROBE_MAGIC 0x59415250 // "PRAY"
#define CAP12 12

DEV void held_rows(float2v &cx, float2v &cy, float2v &cz, float2v &cw, float &z0, float &z1, float &z2, float &z3, const float *c, const float *rz) {
    cx = float2v{c[0], c[1]}; cy = float2v{c[2], c[3]}; cz = float2v{c[4], c[5]}; cw = float2v{c[6], c[7]};
    z0 = rz[0]; z1 = rz[1]; z2 = rz[2]; z3 = rz[3];
}

__global__ void __launch_bounds__(64) k_probe(DParams P, int op, int n, const float *rays, uint32_t *out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool mine = i < n;
    const float *x = rays + (size_t) (mine ? i : n - 1) * 9;
    const f3 o = ld3(x), d = ld3(x + 3);
    const float tmin = x[6], tmax = x[7];
    const bool any_hit = x[8] != 0.f;
    Hit h{-1, tmax, 0.f, 0.f};
    if (op == OP_TRACE15) h = trace<15>(P, o, d, tmin, tmax, any_hit);
    else if (op == OP_TRACE0) h = trace<0>(P, o, d, tmin, tmax, any_hit);
    else if (op == OP_BRUTE || op == OP_BRUTE_VEC) h = trace_brute<15>(P, o, d, tmin, tmax);
    else if (op == OP_HELD) {
        const float2v z2 = {0.f, 0.f};
        const BoxRec no_box = {z2, z2, z2, z2, 0.f, 0.f, 0.f, 0.f, 0u, 0u, 0u};
        auto box = [&](int b) {
            BoxRec G = no_box;
            if (b < P.n_box) {
                const DPrimBox *q = P.prims_box + b;
                held_rows(G.cx, G.cy, G.cz, G.cw, G.z0, G.z1, G.z2, G.z3, q->c, q->rz);
                G.f0 = q->fw[0]; G.f1 = q->fw[1]; G.f2 = q->fw[2];
            }
            return G;
        };
        FlatRec F = {z2, z2, z2, z2, 0.f, 0.f, 0.f, 0.f, -1};
        if (P.n_flat_rec > 0) {
            const DPrimFlat *q = P.prims_flat;
            held_rows(F.cx, F.cy, F.cz, F.cw, F.z0, F.z1, F.z2, F.z3, q->c, q->rz);
            F.ks = q->kind_shade;
        }
        const HeldScene S = {{box(0), box(1), box(2)}, F};
        h = trace_held(S, (uint32_t) P.n_box, (uint32_t) P.n_flat_rec, o, d, tmin, tmax);
    } else if (op == OP_BVH32) h = trace_bvh(P, o, d, tmin, tmax, any_hit);
    else {
        Trav T;
        trav_reset_counters(T);
        trav_begin(T, o, d, tmin, tmax, any_hit);
        if (op == OP_BVH16) trav_run<short, DParams, true, BVH_STACK, 15>(P, T, true, 0);
        else trav_run<int, DParams, true, CAP12, 15>(P, T, true, 0);
        h = T.h;
    }
    if (mine) {
        uint32_t *r = out + (size_t) i * 4;
        r[0] = (uint32_t) h.prim; r[1] = __float_as_uint(h.t); r[2] = __float_as_uint(h.u); r[3] = __float_as_uint(h.v);
    }
}

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    fprintf(stderr, "ray_probe: %s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)
#define BAD(...) do { fprintf(stderr, "ray_probe: " __VA_ARGS__); fprintf(stderr, "\n"); return 2; } while (0)

// a shading index as an intersection record, a flat record or a face half-word carries it: the record itself and, for a merged pair, the next one
static bool shade_ok(int kind, long long shade, int n_shade) { return shade >= 0 && shade + (kind == PRIM_QUAD2 ? 1 : 0) < n_shade; }

int main(int argc, char **argv) {
    if (argc != 3) BAD("usage: ray_probe <request> <result>");
    FILE *f = fopen(argv[1], "rb");
    int32_t head[16];
    if (!f || fread(head, 4, 16, f) != 16) BAD("cannot read %s", argv[1]);
    const int n = head[1], n_ops = head[2], n_prims = head[3], n_shade = head[4], n_bvh = head[5], n_flat_all = head[6], n_box_all = head[7], ovf_entries = head[8],
              trace_vote = head[9];
    const int lim = 1 << 20;
    if (head[0] != RAY_PROBE_MAGIC || head[10] != (int) sizeof(DParams)) BAD("bad header: magic or the size of DParams");
    if (n < 1 || n > lim || n_ops < 1 || n_ops > 64 || n_prims < 1 || n_prims > lim || n_shade < 1 || n_shade > lim || n_bvh < 0 || n_bvh > lim ||
        n_flat_all < 0 || n_flat_all > lim || n_box_all < 0 || n_box_all > lim || ovf_entries < 0 || ovf_entries > 4096 || trace_vote < 1 || trace_vote > 1024)
        BAD("bad header: a count out of range");
    DParams P;
    std::vector<DPrim> prims(n_prims);
    std::vector<DShade> shade(n_shade);
    std::vector<DBvh4Node> bvh(n_bvh);
    std::vector<DPrimFlat> flat(n_flat_all);
    std::vector<DPrimBox> boxes(n_box_all);
    std::vector<float> rays((size_t) n * 9);
    std::vector<int32_t> ops(n_ops);
    auto rd = [&](void *p, size_t size, size_t count) { return count == 0 || fread(p, size, count, f) == count; };
    if (!rd(&P, sizeof P, 1) || !rd(prims.data(), sizeof(DPrim), n_prims) || !rd(shade.data(), sizeof(DShade), n_shade) || !rd(bvh.data(), sizeof(DBvh4Node), n_bvh) ||
        !rd(flat.data(), sizeof(DPrimFlat), n_flat_all) || !rd(boxes.data(), sizeof(DPrimBox), n_box_all) || !rd(rays.data(), 4, rays.size()) || !rd(ops.data(), 4, n_ops))
        BAD("short request");
    if (fgetc(f) != EOF) BAD("bytes after the request");
    fclose(f);

    // ---- every index the device will follow
    if (P.prims || P.shade || P.bsdfs || P.emitters || P.bvh || P.filter_lut || P.film || P.x || P.stats || P.error_flag || P.bvh_overflow || P.prims_flat || P.prims_box ||
        P.normals || P.rows || P.importance)
        BAD("the parameter block carries a pointer");
    if (P.n_prims != n_prims || P.n_shade != n_shade || P.n_bvh_nodes != n_bvh) BAD("the parameter block's counts are not the tables'");
    if (P.n_flat < 0 || P.n_flat > n_prims) BAD("n_flat %d outside [0, n_prims]", P.n_flat);
    if (P.bvh_leaf_shift != 0 && P.bvh_leaf_shift != 3) BAD("bvh_leaf_shift %d", P.bvh_leaf_shift);
    bool spheres = false, ordered = true; // ordered: flat records first, spheres last (what the sphere loop of trace<15> assumes)
    for (int i = 0; i < n_prims; ++i) {
        const DPrim &g = prims[i];
        if (g.type != PRIM_TRIANGLE && g.type != PRIM_RECTANGLE && g.type != PRIM_SPHERE && g.type != PRIM_QUAD2) BAD("primitive %d: kind %d", i, g.type);
        if (!shade_ok(g.type, g.shade, n_shade)) BAD("primitive %d: shading record %d outside the table", i, g.shade);
        if (g.kind_shade != (g.type | (g.shade << 8))) BAD("primitive %d: kind_shade is not type | shade << 8", i);
        spheres = spheres || g.type == PRIM_SPHERE;
        ordered = ordered && ((g.type == PRIM_SPHERE) == (i >= P.n_flat));
    }
    for (int i = 0; i < n_shade; ++i) {
        const int kind = shade[i].bsdf >> 24;
        if (kind < PRIM_TRIANGLE || kind > PRIM_SMOOTH) BAD("shading record %d: kind %d", i, kind);
        if (shade[i].emitter < -1) BAD("shading record %d: emitter %d", i, shade[i].emitter);
    }
    const bool has_flat = n_flat_all > 0, has_boxes = n_box_all > 0;
    if (has_flat) {
        if (P.n_flat_rec != n_flat_all - 2 || P.n_flat_rec < 0) BAD("flat: n_flat_rec %d needs %d records and two sentinels, the table has %d", P.n_flat_rec, P.n_flat_rec, n_flat_all);
        for (int i = 0; i < P.n_flat_rec; ++i) {
            const int kind = flat[i].kind_shade & 0xff, sh = flat[i].kind_shade >> 8;
            if (flat[i].kind_shade < 0 || (kind != PRIM_TRIANGLE && kind != PRIM_RECTANGLE && kind != PRIM_QUAD2)) BAD("flat record %d: kind_shade %d", i, flat[i].kind_shade);
            if (kind == PRIM_TRIANGLE && !P.has_plain_tri) BAD("flat record %d: a plain triangle, has_plain_tri is 0", i);
            if (!shade_ok(kind, sh, n_shade)) BAD("flat record %d: shading record %d outside the table", i, sh);
        }
        for (int i = P.n_flat_rec; i < n_flat_all; ++i) { // no ray can hit a sentinel: ld.z = 0, lo.z = 1
            const DPrimFlat &s = flat[i];
            bool zero = s.rz[0] == 0.f && s.rz[1] == 0.f && s.rz[2] == 0.f && s.rz[3] == 1.f && s.kind_shade == PRIM_RECTANGLE;
            for (int k = 0; k < 8; ++k) zero = zero && s.c[k] == 0.f;
            if (!zero) BAD("flat: record %d is no sentinel", i);
        }
    } else if (P.n_flat_rec != 0) BAD("n_flat_rec %d without a flat table", P.n_flat_rec);
    if (has_boxes) {
        if (!has_flat) BAD("cuboids without a flat table");
        if (P.n_box != n_box_all - 1 || P.n_box < 1) BAD("boxes: n_box %d needs %d records and a sentinel, the table has %d", P.n_box, P.n_box, n_box_all);
        for (int i = 0; i < P.n_box; ++i)
            for (int a = 0; a < 3; ++a)
                for (int side = 0; side < 2; ++side) {
                    const uint32_t hc = side ? boxes[i].fw[a] >> 16 : boxes[i].fw[a] & 0xffffu;
                    if (!(hc & 1u)) continue;
                    const int kind = (int) ((hc >> 4) & 3u), sh = (int) (hc >> 6);
                    if (kind != PRIM_RECTANGLE && kind != PRIM_QUAD2) BAD("cuboid %d axis %d side %d: kind %d", i, a, side, kind);
                    if (!shade_ok(kind, sh, n_shade)) BAD("cuboid %d axis %d side %d: shading record %d outside the table", i, a, side, sh);
                }
        const DPrimBox zero{};
        if (memcmp(&boxes[P.n_box], &zero, sizeof zero) != 0) BAD("boxes: record %d is no sentinel", P.n_box);
    } else if (P.n_box != 0) BAD("n_box %d without a cuboid table", P.n_box);
    // the tree: children behind their parent (so it is a tree and the walk below ends), leaf references inside the primitives under
    // the block's bvh_leaf_shift, the depth the stacks have to hold
    int depth = 0;
    if (n_bvh > 0) {
        std::vector<int> level(n_bvh, 0);
        level[0] = 1;
        for (int i = 0; i < n_bvh; ++i) {
            if (level[i] == 0) BAD("bvh node %d: no parent", i);
            depth = level[i] > depth ? level[i] : depth;
            for (int c = 0; c < 4; ++c) {
                const int ch = bvh[i].child[c];
                if (ch >= 0) {
                    if (ch <= i || ch >= n_bvh) BAD("bvh node %d child %d: node %d outside (%d, %d)", i, c, ch, i, n_bvh);
                    if (level[ch] != 0) BAD("bvh node %d child %d: node %d has two parents", i, c, ch);
                    level[ch] = level[i] + 1;
                } else {
                    const long long ref = ~(long long) ch, first = ref >> P.bvh_leaf_shift, cnt = P.bvh_leaf_shift ? (ref & 7) : 1;
                    if (first < 0 || first + cnt > n_prims) BAD("bvh node %d child %d: leaf reference [%lld, %lld) outside the %d primitives", i, c, first, first + cnt, n_prims);
                }
            }
        }
    }
    for (size_t k = 0; k < rays.size(); ++k)
        if (std::isnan(rays[k])) BAD("ray %zu: NaN", k / 9);
    // ---- what each op needs
    const int ovf_needed = 3 * depth + 3;
    auto bvh_ok = [&](int cap, bool short_stack) -> const char * {
        if (n_bvh < 1 || !P.use_bvh) return "no BVH";
        if (short_stack && (!P.bvh_stack16 || n_bvh >= 32768 || (((long long) n_prims << P.bvh_leaf_shift) | 7) >= 32768)) return "the stack entries do not fit 16 bits";
        if (ovf_entries == 0 ? 3 * depth > cap : ovf_entries < ovf_needed) return "the tree is deeper than the stack column and the overflow area";
        return nullptr;
    };
    for (int k = 0; k < n_ops; ++k) {
        const char *why = nullptr;
        switch (ops[k]) {
        case OP_TRACE15: why = P.use_bvh ? bvh_ok(BVH_STACK, false) : (has_flat && !ordered ?"spheres are not behind the flat records" : nullptr); break;
        case OP_TRACE0: why = (P.use_bvh || !has_flat || spheres) ? "no flat scene" : nullptr; break;
        case OP_BRUTE: case OP_BRUTE_VEC: break;
        case OP_HELD: why = (P.use_bvh || !has_flat || spheres || !plan_detail::w2_held_launch(P.n_box, P.n_flat_rec, P.has_plain_tri != 0)) ? "w2_held_launch does not accept the scene" : nullptr; break;
        case OP_BVH32: why = bvh_ok(BVH_STACK, false); break;
        case OP_BVH16: why = bvh_ok(BVH_STACK, true); break;
        case OP_BVH32_CAP12: why = bvh_ok(CAP12, false); break;
        default: why = "no such op";
        }
        if (why) BAD("op %d: %s", ops[k], why);
    }

    // ---- upload and run
    const int blocks = (n + 63) / 64;
    DPrim *d_prims = nullptr; DBvh4Node *d_bvh = nullptr; DPrimFlat *d_flat = nullptr; DPrimBox *d_boxes = nullptr;
    int32_t *d_ovf = nullptr; float *d_rays = nullptr; uint32_t *d_out = nullptr;
    HIP_OK(hipMalloc(&d_prims, sizeof(DPrim) * n_prims));
    HIP_OK(hipMemcpy(d_prims, prims.data(), sizeof(DPrim) * n_prims, hipMemcpyHostToDevice));
    if (n_bvh) { HIP_OK(hipMalloc(&d_bvh, sizeof(DBvh4Node) * n_bvh)); HIP_OK(hipMemcpy(d_bvh, bvh.data(), sizeof(DBvh4Node) * n_bvh, hipMemcpyHostToDevice)); }
    if (has_flat) { HIP_OK(hipMalloc(&d_flat, sizeof(DPrimFlat) * n_flat_all)); HIP_OK(hipMemcpy(d_flat, flat.data(), sizeof(DPrimFlat) * n_flat_all, hipMemcpyHostToDevice)); }
    if (has_boxes) { HIP_OK(hipMalloc(&d_boxes, sizeof(DPrimBox) * n_box_all)); HIP_OK(hipMemcpy(d_boxes, boxes.data(), sizeof(DPrimBox) * n_box_all, hipMemcpyHostToDevice)); }
    const size_t ovf_ints = (size_t) ovf_entries * 64 * blocks;
    if (ovf_ints) { HIP_OK(hipMalloc(&d_ovf, ovf_ints * 4)); HIP_OK(hipMemset(d_ovf, 0xff, ovf_ints * 4)); }
    HIP_OK(hipMalloc(&d_rays, rays.size() * 4));
    HIP_OK(hipMemcpy(d_rays, rays.data(), rays.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMalloc(&d_out, (size_t) n * 16));
    P.prims = d_prims; P.bvh = d_bvh; P.prims_flat = d_flat; P.prims_box = d_boxes;
    P.bvh_overflow = d_ovf; P.bvh_ovf_lanes = 64u * (uint32_t) blocks; P.trace_vote = trace_vote;
    const int debug = P.debug & ~64;
    std::vector<uint32_t> out((size_t) n * 4);
    f = fopen(argv[2], "wb");
    if (!f) BAD("cannot write %s", argv[2]);
    for (int k = 0; k < n_ops; ++k) {
        P.debug = ops[k] == OP_BRUTE_VEC ? debug | 64 : debug;
        HIP_OK(hipMemset(d_out, 0xff, (size_t) n * 16));
        k_probe<<<blocks, 64>>>(P, ops[k], n, d_rays, d_out);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data(), d_out, (size_t) n * 16, hipMemcpyDeviceToHost));
        if (fwrite(out.data(), 16, n, f) != (size_t) n) BAD("cannot write %s", argv[2]);
    }
    if (fclose(f) != 0) BAD("cannot write %s", argv[2]);
    HIP_OK(hipFree(d_prims)); HIP_OK(hipFree(d_out)); HIP_OK(hipFree(d_rays));
    if (d_bvh) HIP_OK(hipFree(d_bvh));
    if (d_flat) HIP_OK(hipFree(d_flat));
    if (d_boxes) HIP_OK(hipFree(d_boxes));
    if (d_ovf) HIP_OK(hipFree(d_ovf));
    return 0;
}
