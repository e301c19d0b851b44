// Host-only preparation of a scene for the kernels: every scene check of drmlt_create, the flattening of shapes into intersection
// and shading records (triangle pairs merged), the BVH or the brute-force loop's flat and cuboid records, the feature bits, the
// PSS dimensions and the planner's inputs (prepare_scene). drmlt_create calls it before it opens a device and then only
// allocates and uploads what it returns. No HIP headers: the tables are pinned down on the CPU (tests/native/scene_prep_harness.cpp).
#pragma once
#include "../../include/drmlt_abi.h"
#include "box_merge.h"
#include "bvh_build.h"
#include "device_types.h"
#include "launch_plan.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

// What drmlt_create computes without a device. The tables are in their final order; `P` has every field that does not depend on
// an allocation (all pointers null, the plan's fields and the chain count unset); `plan` lacks the device's CU count.
struct PreparedScene {
    std::vector<DPrim> prims;       // leaf order (BVH) or flat records first, spheres last (brute force); kind_shade set
    std::vector<DShade> shade;      // the primitives' records, then one per point light / for the environment
    std::vector<DBsdf> bsdfs;
    std::vector<DEmitter> emitters;
    std::vector<DBvh4Node> bvh;     // empty: brute force
    std::vector<DPrimFlat> flat;    // n_flat_rec records + two sentinels; empty: no flat loop (BVH, DRMLT_NO_FLAT_LOOP)
    std::vector<DPrimBox> boxes;    // n_box records + one sentinel; empty: no cuboids
    std::vector<DSmooth> normals;   // one entry per smooth triangle, in shape order (its shading record holds the index); empty: none
    std::array<float, 32> lut{};    // reconstruction filter table
    DParams P{};
    int bvh_depth = 0;
    int ovf_entries = 0;            // capacity per lane of the traversal stacks' overflow area (0: every stack fits its LDS column)
    PlanInputs plan;
};

namespace scene_prep_detail {

inline bool invert3x4(const double *m, double *o) {
    double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], i = m[10];
    double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det == 0 || !std::isfinite(det)) return false;
    double id = 1.0 / det;
    o[0] = (e * i - f * h) * id; o[1] = (c * h - b * i) * id; o[2] = (b * f - c * e) * id;
    o[4] = (f * g - d * i) * id; o[5] = (a * i - c * g) * id; o[6] = (c * d - a * f) * id;
    o[8] = (d * h - e * g) * id; o[9] = (b * g - a * h) * id; o[10] = (a * e - b * d) * id;
    for (int r = 0; r < 3; ++r) o[r * 4 + 3] = -(o[r * 4] * m[3] + o[r * 4 + 1] * m[7] + o[r * 4 + 2] * m[11]);
    return true;
}

// ConstantBackgroundEmitter::createShape (constant.cpp:67-92): the bounding sphere of the scene's box, its radius times 1.5 (at least
// Epsilon). The box is the geometry's (the kd-tree's) expanded by the sensor's position: DRMLT calls Scene::initializeBidirectional
// (scene.cpp:396-423), which builds it before any emitter's shape. AABB::getBSphere: the box's centre, the distance to its max
// corner. The kd-tree's box is the geometry's tight one enlarged by MTS_KD_AABB_EPSILON = 1e-3 of its extent plus 1e-3, the upper
// side from the already lowered minimum (gkdtree.h:1213-1220, in Float). Only the length of the light sample's shadow ray
// depends on it.
inline void scene_bsphere(const drmlt_scene &s, const std::vector<PrimBounds> &bounds, float centre[3], float &radius) {
    const double cam[3] = {s.camera.to_world[3], s.camera.to_world[7], s.camera.to_world[11]};
    double lo[3], hi[3], r2 = 0;
    for (int k = 0; k < 3; ++k) {
        lo[k] = hi[k] = cam[k];
        if (!bounds.empty()) {
            float tlo = bounds[0].lo[k], thi = bounds[0].hi[k];
            for (const PrimBounds &b : bounds) { tlo = std::min(tlo, b.lo[k]); thi = std::max(thi, b.hi[k]); }
            const float eps = 1e-3f;
            tlo -= (thi - tlo) * eps + eps;
            thi += (thi - tlo) * eps + eps;
            lo[k] = std::min(lo[k], (double) tlo); hi[k] = std::max(hi[k], (double) thi);
        }
        const double c = 0.5 * (lo[k] + hi[k]);
        centre[k] = (float) c;
        r2 += (hi[k] - c) * (hi[k] - c);
    }
    radius = (float) std::max(1e-4, 1.5 * std::sqrt(r2)); // Epsilon (single precision builds)
}

// BSDF types and the smooth conductor's parameters (SmoothConductor, conductor.cpp). Returns "" or an error.
inline std::string validate_bsdfs(const drmlt_scene &s) {
    for (int i = 0; i < s.n_bsdfs && s.bsdfs; ++i) {
        const drmlt_bsdf &b = s.bsdfs[i];
        if (b.type < DRMLT_BSDF_DIFFUSE || b.type > DRMLT_BSDF_CONDUCTOR)
            return "unsupported BSDF type " + std::to_string(b.type) + " (supported: diffuse, dielectric, roughconductor, conductor)";
        if (b.type != DRMLT_BSDF_CONDUCTOR) continue;
        const std::string which = "conductor " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(b.rgb[k]) || b.rgb[k] < 0.f) return which + "specularReflectance must be finite and non-negative";
            if (!std::isfinite(b.p[1 + k]) || b.p[1 + k] < 0.f) return which + "eta must be finite and non-negative";
            if (!std::isfinite(b.p[4 + k]) || b.p[4 + k] < 0.f) return which + "k must be finite and non-negative";
        }
    }
    return "";
}

// Emitter types, point lights (PointEmitter, point.cpp) and the environment (ConstantBackgroundEmitter, constant.cpp). Returns ""
// or an error.
inline std::string validate_emitters(const drmlt_scene &s, int technique) {
    if (s.n_points < 0 || (s.n_points > 0 && !s.points)) return "point lights: n_points must be >= 0 and points non-null";
    if (s.n_emitters <= 0 || !s.emitters) return "";
    for (int i = 0; i < s.n_shapes && s.shapes; ++i) {
        const int ei = s.shapes[i].emitter;
        if (ei >= 0 && ei < s.n_emitters && s.emitters[ei].type == DRMLT_EMITTER_POINT)
            return "emitter/shape link mismatch: shape " + std::to_string(i) + " carries point light " + std::to_string(ei);
        if (ei >= 0 && ei < s.n_emitters && s.emitters[ei].type == DRMLT_EMITTER_CONSTANT)
            return "emitter/shape link mismatch: shape " + std::to_string(i) + " carries the environment emitter " + std::to_string(ei);
    }
    std::vector<int> owner((size_t) s.n_points, -1);
    int env = -1;
    for (int i = 0; i < s.n_emitters; ++i) {
        const drmlt_emitter &e = s.emitters[i];
        if (e.type != DRMLT_EMITTER_AREA && e.type != DRMLT_EMITTER_POINT && e.type != DRMLT_EMITTER_CONSTANT)
            return "unsupported emitter type " + std::to_string(e.type) + " (supported: area, point, constant)";
        if (e.type == DRMLT_EMITTER_CONSTANT) { // ConstantBackgroundEmitter (constant.cpp)
            const std::string which = "environment emitter " + std::to_string(i) + ": ";
            if (env >= 0) return which + "the scene may only contain one environment emitter (emitter " + std::to_string(env) + " is one)";
            env = i;
            if (technique != DRMLT_TECH_PATH) return which + "environment emitters are supported for technique=path only";
            if (e.shape != -1) return which + "shape must be -1 (it has no shape), got " + std::to_string(e.shape);
            for (int k = 0; k < 3; ++k)
                if (!std::isfinite(e.radiance[k]) || e.radiance[k] < 0.f) return which + "radiance must be finite and non-negative";
            continue;
        }
        if (e.type != DRMLT_EMITTER_POINT) continue;
        const std::string which = "point light " + std::to_string(i) + ": ";
        if (technique != DRMLT_TECH_PATH) return which + "point lights are supported for technique=path only";
        if (e.shape < 0 || e.shape >= s.n_points) return which + "position index " + std::to_string(e.shape) + " out of range (n_points = " + std::to_string(s.n_points) + ")";
        if (owner[(size_t) e.shape] >= 0) return which + "shares position entry " + std::to_string(e.shape) + " with emitter " + std::to_string(owner[(size_t) e.shape]);
        owner[(size_t) e.shape] = i;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(s.points[3 * e.shape + k])) return which + "position is not finite";
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(e.radiance[k]) || e.radiance[k] < 0.f) return which + "intensity must be finite and non-negative";
    }
    return "";
}

// Vertex normals (drmlt_shape.normals, drmlt_scene.normals): triangles only, technique=path only. Returns "" or an error.
inline std::string validate_normals(const drmlt_scene &s, int technique) {
    if (s.n_normals < 0 || (s.n_normals > 0 && !s.normals)) return "vertex normals: n_normals must be >= 0 and normals non-null";
    for (int i = 0; i < s.n_shapes && s.shapes; ++i) {
        const drmlt_shape &in = s.shapes[i];
        if (in.normals == 0) continue;
        const std::string which = "shape " + std::to_string(i) + ": ";
        if (in.type != DRMLT_SHAPE_TRIANGLE) return which + "vertex normals on a " + (in.type == DRMLT_SHAPE_RECTANGLE ? "rectangle" : in.type == DRMLT_SHAPE_SPHERE ? "sphere" : "shape that is no triangle") + " (only triangles carry them)";
        if (in.normals < 0 || in.normals > s.n_normals) return which + "vertex-normal index " + std::to_string(in.normals) + " out of range (n_normals = " + std::to_string(s.n_normals) + "; 0 = face normal, k = entry k - 1)";
        if (technique != DRMLT_TECH_PATH)
            return which + "vertex normals are supported for technique=path only: bdpt and mmlt need the geometric normal beside the shading normal in every vertex record, and the adjoint correction of the light subpath's BSDFs";
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(s.normals[9 * (size_t) (in.normals - 1) + k])) return which + "vertex normal is not finite";
    }
    return "";
}

// Flatten the scene into intersection + shading records (out.prims in the caller's order, out.shade, out.bsdfs, out.emitters).
// BSDF and emitter types: validate_bsdfs / validate_emitters have checked them. Returns "" or an error.
inline std::string build_scene(const drmlt_scene &s, const Knobs &K, PreparedScene &out, std::vector<PrimBounds> &bounds, std::vector<QuadGeo> &geo) {
    if (s.n_shapes <= 0) return "scene has no shapes";
    if (s.n_emitters <= 0) return "scene has no emitters";
    for (int i = 0; i < s.n_bsdfs; ++i) {
        const drmlt_bsdf &in = s.bsdfs[i];
        DBsdf b{};
        b.type = in.type;
        for (int k = 0; k < 3; ++k) b.rgb[k] = in.rgb[k];
        if (in.type == DRMLT_BSDF_DIFFUSE) {
        } else if (in.type == DRMLT_BSDF_DIELECTRIC) {
            if (!(in.p[0] > 0.f) || !(in.p[1] > 0.f)) return "dielectric: IORs must be positive";
            b.p[0] = in.p[0] / in.p[1];
            b.p[1] = 1.f / b.p[0];
        } else if (in.type == DRMLT_BSDF_ROUGHCONDUCTOR) {
            if (!(in.p[0] > 0.f)) return "roughconductor: alpha must be positive";
            for (int k = 0; k < 8; ++k) b.p[k] = in.p[k];
        } else { // DRMLT_BSDF_CONDUCTOR: eta, k in the rough conductor's slots; p[0] and p[7] are not read
            for (int k = 1; k < 7; ++k) b.p[k] = in.p[k];
        }
        out.bsdfs.push_back(b);
    }
    for (int i = 0; i < s.n_shapes; ++i) {
        const drmlt_shape &in = s.shapes[i];
        if (in.bsdf < 0 || in.bsdf >= s.n_bsdfs) return "shape references an invalid bsdf";
        if (in.emitter >= s.n_emitters) return "shape references an invalid emitter";
        DPrim g{};
        DShade sh{};
        PrimBounds pb;
        QuadGeo qg{};
        qg.usable = false;
        sh.bsdf = in.bsdf; // | kind << 24, set below
        sh.emitter = in.emitter < 0 ? -1 : in.emitter;
        double m[12], inv[12];
        if (in.type == DRMLT_SHAPE_TRIANGLE) {
            double p0[3], e1[3], e2[3], n[3];
            for (int k = 0; k < 3; ++k) { p0[k] = in.data[k]; e1[k] = (double) in.data[3 + k] - p0[k]; e2[k] = (double) in.data[6 + k] - p0[k]; }
            n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
            double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            if (!(len > 0)) return "degenerate triangle";
            for (int k = 0; k < 3; ++k) n[k] /= len;
            for (int r = 0; r < 3; ++r) { m[r * 4] = e1[r]; m[r * 4 + 1] = e2[r]; m[r * 4 + 2] = n[r]; m[r * 4 + 3] = p0[r]; }
            if (!invert3x4(m, inv)) return "degenerate triangle";
            g.type = PRIM_TRIANGLE;
            for (int k = 0; k < 3; ++k) { sh.origin[k] = (float) p0[k]; sh.eu[k] = (float) e1[k]; sh.ev[k] = (float) e2[k]; sh.n[k] = (float) n[k]; }
            sh.inv_len_eu = (float) (1.0 / std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]));
            sh.inv_area = (float) (1.0 / (0.5 * len));
            if (in.normals > 0) { // validate_normals has checked the index: the shading record alone knows (kind PRIM_SMOOTH, below)
                const float *vn = s.normals + 9 * (size_t) (in.normals - 1);
                DSmooth e{};
                for (int k = 0; k < 3; ++k) { e.n0[k] = vn[k]; e.d1[k] = vn[3 + k] - vn[k]; e.d2[k] = vn[6 + k] - vn[k]; }
                const uint32_t index = (uint32_t) out.normals.size() + SMOOTH_INDEX_BIAS; // a normal float's bits (smooth_frame.h)
                sh.n[1] = sh.n[2] = 0.f;
                memcpy(&sh.n[0], &index, sizeof index); // where a flat primitive has its normal (device_types.h: PRIM_SMOOTH)
                out.normals.push_back(e);
            }
            for (int k = 0; k < 3; ++k) {
                double a = p0[k], b = p0[k] + e1[k], c = p0[k] + e2[k];
                pb.lo[k] = (float) std::min(a, std::min(b, c)); pb.hi[k] = (float) std::max(a, std::max(b, c));
            }
        } else if (in.type == DRMLT_SHAPE_RECTANGLE) {
            for (int k = 0; k < 12; ++k) m[k] = in.data[k];
            if (!invert3x4(m, inv)) return "rectangle: singular toWorld";
            double eu[3] = {m[0], m[4], m[8]}, ev[3] = {m[1], m[5], m[9]};
            double lu = std::sqrt(eu[0] * eu[0] + eu[1] * eu[1] + eu[2] * eu[2]), lv = std::sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
            double sdot = (eu[0] * ev[0] + eu[1] * ev[1] + eu[2] * ev[2]) / (lu * lv);
            if (std::fabs(sdot) > 1e-4) return "Error: 'toWorld' transformation contains shear!"; // rectangle.cpp:107-108
            // normal: objectToWorld(Normal(0,0,1)) = third row of the inverse, normalised
            double n[3] = {inv[8], inv[9], inv[10]};
            double ln = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
            g.type = PRIM_RECTANGLE;
            // parametrise the rectangle on [0,1]^2 from its (-1,-1) corner: u' = (u + 1) / 2 (same test as a merged
            // triangle pair). Shading record: origin = that corner, eu / ev = the full edge vectors.
            for (int c = 0; c < 4; ++c) { inv[c] = 0.5 * inv[c] + (c == 3 ? 0.5 : 0.0); inv[4 + c] = 0.5 * inv[4 + c] + (c == 3 ? 0.5 : 0.0); }
            for (int k = 0; k < 3; ++k) {
                sh.origin[k] = (float) (m[k * 4 + 3] - eu[k] - ev[k]); sh.eu[k] = (float) (2.0 * eu[k]); sh.ev[k] = (float) (2.0 * ev[k]);
                sh.n[k] = (float) (n[k] / ln);
            }
            sh.inv_len_eu = (float) (1.0 / (2.0 * lu));
            sh.inv_area = (float) (1.0 / (4.0 * lu * lv)); // |dpdu| |dpdv| with dpdu = 2 eu
            for (int k = 0; k < 3; ++k) { qg.a[k] = m[k * 4 + 3] - eu[k] - ev[k]; qg.e1[k] = 2.0 * eu[k]; qg.e2[k] = 2.0 * ev[k]; }
            qg.usable = true; // the record's (u, v) run over [0, 1]^2 from that corner
            for (int k = 0; k < 3; ++k) {
                double c = m[k * 4 + 3], ext = std::fabs(eu[k]) + std::fabs(ev[k]);
                pb.lo[k] = (float) (c - ext); pb.hi[k] = (float) (c + ext);
            }
        } else if (in.type == DRMLT_SHAPE_SPHERE) {
            double r = in.data[3];
            if (!(r > 0)) return "sphere: radius must be positive";
            for (int k = 0; k < 12; ++k) inv[k] = 0;
            for (int k = 0; k < 3; ++k) { inv[k * 4 + k] = 1.0 / r; inv[k * 4 + 3] = -(double) in.data[k] / r; }
            g.type = PRIM_SPHERE;
            for (int k = 0; k < 3; ++k) { sh.origin[k] = in.data[k]; pb.lo[k] = (float) (in.data[k] - r); pb.hi[k] = (float) (in.data[k] + r); }
            sh.eu[0] = (float) r;
            sh.inv_area = (float) (1.0 / (4.0 * M_PI * r * r));
        } else {
            return "unknown shape type " + std::to_string(in.type);
        }
        for (int k = 0; k < 12; ++k) g.m[k] = (float) inv[k];
        sh.bsdf |= (in.type == DRMLT_SHAPE_TRIANGLE && in.normals > 0 ? PRIM_SMOOTH : g.type) << 24;
        g.shade = (int32_t) out.shade.size();
        out.prims.push_back(g);
        out.shade.push_back(sh);
        bounds.push_back(pb);
        geo.push_back(qg);
    }
    // ---- merge triangle pairs (a,b,c),(a,c,d) that form a parallelogram into one intersection record.
    // Exact: the hit is attributed to the sub-triangle it falls in, with that triangle's barycentrics and
    // shading record, so every path is the one two separate triangles would give -- at half the tests.
    if (!K.no_quad_merge) {
        std::vector<DPrim> merged;
        std::vector<PrimBounds> mb;
        std::vector<QuadGeo> mg;
        for (size_t i = 0; i < out.prims.size(); ++i) {
            bool did = false;
            if (i + 1 < out.prims.size() && s.shapes[i].type == DRMLT_SHAPE_TRIANGLE && s.shapes[i + 1].type == DRMLT_SHAPE_TRIANGLE &&
                s.shapes[i].bsdf == s.shapes[i + 1].bsdf && s.shapes[i].emitter < 0 && s.shapes[i + 1].emitter < 0 &&
                s.shapes[i].normals == 0 && s.shapes[i + 1].normals == 0) { // (smooth triangles stay single: no pair, so no cuboid face either)
                const float *A = s.shapes[i].data, *B = s.shapes[i + 1].data; // A: a,b,c   B: a',c',d
                bool shared = true;
                for (int k = 0; k < 3; ++k) shared = shared && A[k] == B[k] && A[6 + k] == B[3 + k];
                double a[3], b[3], c[3], d[3], e1[3], e2[3], n[3], err = 0, scale = 0;
                for (int k = 0; k < 3; ++k) {
                    a[k] = A[k]; b[k] = A[3 + k]; c[k] = A[6 + k]; d[k] = B[6 + k];
                    err = std::max(err, std::fabs(d[k] - (a[k] + c[k] - b[k])));
                    scale = std::max(scale, std::max(std::fabs(c[k] - a[k]), std::fabs(b[k] - a[k])));
                    e1[k] = b[k] - a[k]; e2[k] = d[k] - a[k];
                }
                if (shared && err <= 1e-6 * scale) {
                    n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
                    double len = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
                    double m[12], inv[12];
                    for (int r = 0; r < 3; ++r) { m[r * 4] = e1[r]; m[r * 4 + 1] = e2[r]; m[r * 4 + 2] = n[r] / len; m[r * 4 + 3] = a[r]; }
                    if (len > 0 && invert3x4(m, inv)) {
                        DPrim g{};
                        for (int k = 0; k < 12; ++k) g.m[k] = (float) inv[k];
                        g.type = PRIM_QUAD2;
                        g.shade = (int32_t) i; // records i (a,b,c) and i+1 (a,c,d)
                        PrimBounds pb = bounds[i];
                        for (int k = 0; k < 3; ++k) { pb.lo[k] = std::min(pb.lo[k], bounds[i + 1].lo[k]); pb.hi[k] = std::max(pb.hi[k], bounds[i + 1].hi[k]); }
                        QuadGeo qg{};
                        for (int k = 0; k < 3; ++k) { qg.a[k] = a[k]; qg.e1[k] = e1[k]; qg.e2[k] = e2[k]; }
                        qg.usable = true;
                        merged.push_back(g); mb.push_back(pb); mg.push_back(qg);
                        ++i;
                        did = true;
                    }
                }
            }
            if (!did) { merged.push_back(out.prims[i]); mb.push_back(bounds[i]); mg.push_back(geo[i]); }
        }
        out.prims.swap(merged);
        bounds.swap(mb);
        geo.swap(mg);
    }
    // emitters + DiscreteDistribution over sampling weights (scene.cpp m_emitterPDF, pmf.h:109-121), in the caller's order
    double total = 0;
    for (int i = 0; i < s.n_emitters; ++i) {
        const drmlt_emitter &e = s.emitters[i];
        if (e.type == DRMLT_EMITTER_AREA && (e.shape < 0 || e.shape >= s.n_shapes || s.shapes[e.shape].emitter != i)) return "emitter/shape link mismatch";
        if (!(e.sampling_weight >= 0)) return "negative emitter sampling weight";
        total += e.sampling_weight;
    }
    if (!(total > 0)) return "emitter sampling weights sum to zero";
    float cdf = 0.f, norm = 1.0f / (float) total;
    std::vector<float> raw(s.n_emitters + 1, 0.f);
    for (int i = 0; i < s.n_emitters; ++i) { cdf += s.emitters[i].sampling_weight; raw[i + 1] = cdf; }
    for (int i = 1; i <= s.n_emitters; ++i) raw[i] *= norm;
    raw[s.n_emitters] = 1.f;
    for (int i = 0; i < s.n_emitters; ++i) {
        DEmitter e{};
        for (int k = 0; k < 3; ++k) e.radiance[k] = s.emitters[i].radiance[k];
        e.prim = s.emitters[i].shape;
        if (s.emitters[i].type == DRMLT_EMITTER_POINT) { // a shading record of its own behind the primitives' (device_path.h: path_step)
            DShade sh{};
            for (int k = 0; k < 3; ++k) sh.origin[k] = s.points[3 * s.emitters[i].shape + k];
            sh.bsdf = PRIM_POINT << 24;
            sh.emitter = i;
            e.prim = (int32_t) out.shade.size();
            out.shade.push_back(sh);
        }
        if (s.emitters[i].type == DRMLT_EMITTER_CONSTANT) { // the same for the environment: the scene's bounding sphere
            DShade sh{};
            scene_bsphere(s, bounds, sh.origin, sh.eu[0]);
            sh.bsdf = PRIM_ENV << 24;
            sh.emitter = i;
            e.prim = (int32_t) out.shade.size();
            out.shade.push_back(sh);
        }
        e.cdf_lo = raw[i]; e.cdf_hi = raw[i + 1];
        // Every pick loop of the device (path_step, direct_emitter_sample, device_bidir.h, device_bdpt.h) takes the last emitter whose
        // cdf_lo lies below the sample. Behind leading emitters of
        // weight 0 the first one that can be sampled starts at 0 as they do, and a sample of exactly 0 would stay with entry 0 and
        // its probability 0, where DiscreteDistribution::sample steps over zero-width entries (pmf.h:124-139). The smallest normal
        // number below 0 sends that sample to it; cdf_hi - cdf_lo and the reused sample (sx - cdf_lo) / (cdf_hi - cdf_lo) keep their
        // values but for 1e-38.
        if (i > 0 && raw[i] == 0.f && raw[i + 1] > 0.f) e.cdf_lo = -std::numeric_limits<float>::min();
        out.emitters.push_back(e);
    }
    return "";
}

// ReconstructionFilter::configure (rfilter.cpp:37-55) for box.cpp / gaussian.cpp
inline void build_filter(int type, float param, float lut[32], float &radius, float &scale) {
    const int res = 31;
    bool gauss = type == DRMLT_FILTER_GAUSSIAN;
    float stddev = param;
    radius = gauss ? 4.f * stddev : param + 1e-5f;
    float sum = 0.f;
    for (int i = 0; i < res; ++i) {
        float x = (radius * i) / res, v;
        if (!gauss) v = std::fabs(x) <= radius ? 1.f : 0.f;
        else {
            float alpha = -1.f / (2.f * stddev * stddev);
            v = std::max(0.f, std::exp(alpha * x * x) - std::exp(alpha * radius * radius));
        }
        lut[i] = v;
        sum += v;
    }
    lut[res] = 0.f;
    scale = res / radius;
    sum *= 2.f * radius / res;
    float normalization = 1.f / sum;
    for (int i = 0; i < res; ++i) lut[i] *= normalization;
}

inline int find_max_dim_path(int maxDepth, int rrDepth) { // pssmlt_utils.h:62-68 (no media, no rough dielectric)
    int maxDim = (maxDepth + 2) * (4 + (rrDepth < maxDepth ? 1 : 0));
    if (maxDim % 2 == 1) ++maxDim;
    return maxDim;
}
// dimensions MIPathTracer::Li can actually consume: 2 (film) + 4 per scattering event at depth
// 1..maxDepth-1 + one roulette draw per event at depth >= rrDepth; rounded up to a full pair
inline int effective_dim_path(int maxDepth, int rrDepth) {
    int events = maxDepth - 1;
    int rr = std::max(0, maxDepth - std::max(rrDepth, 1));
    int d = 2 + 4 * events + rr;
    if (d % 2 == 1) ++d;
    return d;
}

} // namespace scene_prep_detail

// Checks the scene (the configuration's own checks come first, in drmlt_create) and fills `out`. Returns "" or the refusal.
inline std::string prepare_scene(const drmlt_config &cfg, const drmlt_scene &scene, const Knobs &K, PreparedScene &out) {
    using namespace scene_prep_detail;
    out = PreparedScene();
    std::string e = validate_bsdfs(scene);
    if (e.empty()) e = validate_emitters(scene, cfg.technique);
    if (e.empty()) e = validate_normals(scene, cfg.technique);
    if (!e.empty()) return e;
    const drmlt_camera &cam = scene.camera;
    if (cam.width <= 0 || cam.height <= 0) return "film size must be positive";
    if (cam.filter != DRMLT_FILTER_BOX && cam.filter != DRMLT_FILTER_GAUSSIAN) return "unsupported reconstruction filter";
    if (cfg.acceptance_map && !(cam.filter == DRMLT_FILTER_BOX && cam.filter_param + 1e-5f - 0.500010f <= 1e-6f))
        return "Box filter required for acceptance map!"; // drmlt_proc.cpp:76-79
    std::vector<PrimBounds> bounds;
    std::vector<QuadGeo> geo; // world-space parallelograms of the flat records (box_merge.h)
    e = build_scene(scene, K, out, bounds, geo);
    if (!e.empty()) return e;
    // one table entry per smooth triangle; the kernels address it by 32-bit byte offsets, the records by a biased index (smooth_frame.h)
    if ((uint64_t) out.normals.size() * sizeof(DSmooth) >= (1ull << 32) || out.normals.size() >= SMOOTH_INDEX_MAX - SMOOTH_INDEX_BIAS)
        return "scene too large: the vertex-normal table (one entry per smooth triangle) must stay below 4 GiB";

    // ---- acceleration structure: brute force over wave-uniform records for tiny scenes, BVH otherwise
    DParams &P = out.P;
    P.use_bvh = (int) out.prims.size() > K.bvh_threshold ? 1 : 0;
    if (P.use_bvh) {
        std::vector<DBvhNode> nodes; // binary SAH tree; out.bvh is what the kernels traverse
        std::vector<int> order;
        // SAH splits wherever they lead (the builder's recursion bound, 64 levels, is far from what a surface-area tree
        // needs): a traversal stack that outgrows its LDS column spills to memory (device_path.h: trav_run)
        // (DRMLT_BVH_MAX_DEPTH, tests: exercise the depth-bounded splits)
        const int median_splits = build_bvh(bounds, nodes, order, K.bvh_max_depth, K.bvh_leaf);
        int leaf_shift = 0;
        const int depth4 = build_bvh4(nodes, out.bvh, &leaf_shift);
        P.bvh_leaf_shift = leaf_shift;
        // the traversal addresses node and primitive records by 32-bit byte offsets into buffer resources of 2 GiB (trav_run)
        if (out.bvh.size() * sizeof(DBvh4Node) >= (1ull << 31) || out.prims.size() * sizeof(DPrim) >= (1ull << 31))
            return "scene too large: the BVH node and primitive arrays must stay below 2 GiB each";
        // 16-bit stack entries when every node index and leaf reference fits (k_mutate_v4: 3 KB of LDS instead of 6)
        P.bvh_stack16 = (out.bvh.size() < 32768 && ((order.size() << leaf_shift) | 7u) < 32768 && !K.bvh_stack32) ? 1 : 0;
        // a 4-wide node pushes at most 3 entries, so a node at level l is entered with at most 3 (l - 1) on the stack and
        // 3 * depth4 bound it: up to BVH_STACK that is the LDS column (the branch-free pushes use its spare rows); deeper
        // trees get an overflow area in memory, sized per launch (drmlt_capi.cpp: ensure_overflow)
        out.bvh_depth = depth4;
        // (k_mutate_v4 keeps only 11 entries of a 32-bit stack in LDS: those scenes always have the area)
        out.ovf_entries = (3 * depth4 > BVH_STACK || !P.bvh_stack16) ? (3 * depth4 + 3 + BVH_SPILL - 1) / BVH_SPILL * BVH_SPILL : 0;
        if (K.verbose) fprintf(stderr, "[drmlt] BVH: %zu primitives, %zu binary / %zu 4-wide nodes, 4-wide depth %d (stack %d in LDS + %d in memory), %d median splits, %d-bit stack entries\n", order.size(), nodes.size(), out.bvh.size(), depth4, BVH_STACK, out.ovf_entries, median_splits, P.bvh_stack16 ? 16 : 32);
        // intersection records go into leaf order; shading records stay where the emitters expect them
        std::vector<DPrim> np(order.size());
        for (size_t i = 0; i < order.size(); ++i) np[i] = out.prims[order[i]];
        out.prims.swap(np);
    } else { // brute-force order: flat records first, spheres last (trace(): flat loop, then the sphere loop)
        std::vector<size_t> perm(out.prims.size());
        for (size_t i = 0; i < perm.size(); ++i) perm[i] = i;
        std::stable_partition(perm.begin(), perm.end(), [&](size_t i) { return out.prims[i].type != PRIM_SPHERE; });
        std::vector<DPrim> np(perm.size());
        std::vector<QuadGeo> ng(perm.size());
        for (size_t i = 0; i < perm.size(); ++i) { np[i] = out.prims[perm[i]]; ng[i] = geo[perm[i]]; }
        out.prims.swap(np);
        geo.swap(ng);
    }
    for (DPrim &g : out.prims) g.kind_shade = g.type | (g.shade << 8);
    // flat-primitive fast path of the brute-force loop: interleaved records + two sentinels no ray can hit
    // (ld.z = 0, lo.z = 1: t = -inf fails t >= tmin)
    for (const DPrim &g : out.prims) if (g.type != PRIM_SPHERE) P.n_flat++;
    if (!P.use_bvh && !K.no_flat_loop) {
        // Faces that bound a parallelepiped -- a `cube`'s six merged triangle pairs, the walls of a room -- become ONE cuboid
        // record (box_merge.h; device_path.h: test_box): config 2's 18 records -> 1 + 3 cuboids. DRMLT_NO_BOX_MERGE: the
        // separate faces (the tests compare the two).
        std::vector<char> in_box((size_t) P.n_flat, 0);
        if (!K.no_box_merge) {
            std::vector<QuadGeo> fg(geo.begin(), geo.begin() + P.n_flat);
            for (size_t i = 0; i < fg.size(); ++i) // a record's shading index must fit the face half-word
                if (out.prims[i].shade >= 1024 || (out.prims[i].type != PRIM_RECTANGLE && out.prims[i].type != PRIM_QUAD2)) fg[i].usable = false;
            for (const BoxGeo &bg : find_boxes(fg)) {
                double m[12], inv[12];
                for (int r = 0; r < 3; ++r) { m[r * 4] = bg.E[0][r]; m[r * 4 + 1] = bg.E[1][r]; m[r * 4 + 2] = bg.E[2][r]; m[r * 4 + 3] = bg.a[r]; }
                if (!invert3x4(m, inv)) continue;
                DPrimBox b{};
                for (int c = 0; c < 4; ++c) { b.c[2 * c] = (float) inv[c]; b.c[2 * c + 1] = (float) inv[4 + c]; b.rz[c] = (float) inv[8 + c]; }
                for (int f = 0; f < 6; ++f) {
                    if (bg.face[f] < 0) continue;
                    const DPrim &g = out.prims[(size_t) bg.face[f]];
                    const uint32_t half = 1u | ((uint32_t) bg.code[f] << 1) | ((uint32_t) g.type << 4) | ((uint32_t) g.shade << 6);
                    b.fw[f >> 1] |= half << ((f & 1) ? 16 : 0);
                    in_box[(size_t) bg.face[f]] = 1;
                }
                out.boxes.push_back(b);
            }
            if (K.verbose) fprintf(stderr, "[drmlt] brute-force loop: %d flat records, %zu of them as the faces of %zu cuboids\n", P.n_flat,
                                                 (size_t) std::count(in_box.begin(), in_box.end(), 1), out.boxes.size());
        }
        for (size_t i = 0; i < (size_t) P.n_flat; ++i) {
            if (in_box[i]) continue;
            const DPrim &g = out.prims[i];
            if (g.type == PRIM_TRIANGLE) P.has_plain_tri = 1;
            DPrimFlat f{};
            for (int c = 0; c < 4; ++c) { f.c[2 * c] = g.m[c]; f.c[2 * c + 1] = g.m[4 + c]; f.rz[c] = g.m[8 + c]; }
            f.kind_shade = g.kind_shade;
            out.flat.push_back(f);
        }
        P.n_flat_rec = (int) out.flat.size();
        for (int k = 0; k < 2; ++k) { DPrimFlat f{}; f.rz[3] = 1.f; f.kind_shade = PRIM_RECTANGLE; out.flat.push_back(f); }
        if (!out.boxes.empty()) {
            P.n_box = (int) out.boxes.size();
            out.boxes.push_back(DPrimBox{}); // sentinel for the read-ahead (never tested)
        }
    } else {
        for (const DPrim &g : out.prims) if (g.type == PRIM_TRIANGLE) P.has_plain_tri = 1;
    }

    float radius, scale;
    build_filter(cam.filter, cam.filter_param, out.lut.data(), radius, scale);
    P.n_prims = (int) out.prims.size(); P.n_shade = (int) out.shade.size(); P.n_emitters = (int) out.emitters.size(); P.n_bvh_nodes = (int) out.bvh.size();
    P.n_bsdfs = (int) out.bsdfs.size();
    P.box_weight = cam.filter == DRMLT_FILTER_BOX ? out.lut[0] : 0.f;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) P.cam[r * 4 + c] = cam.to_world[r * 4 + c];
    P.tan_half_fov = (float) std::tan(0.5 * (double) cam.fov_x_deg * M_PI / 180.0);
    P.inv_aspect = (float) cam.height / (float) cam.width;
    P.near_clip = cam.near_clip; P.far_clip = cam.far_clip;
    P.width = cam.width; P.height = cam.height;
    P.filter_radius = radius; P.filter_scale = scale;
    P.type = cfg.type; P.max_depth = cfg.max_depth; P.rr_depth = cfg.rr_depth;
    P.exclude_direct = cfg.direct_samples >= 0 ? 1 : 0; // separateDirect, drmlt.cpp:242
    P.acceptance_map = cfg.acceptance_map; P.timid_after_large = cfg.timid_after_large; P.use_mixture = cfg.use_mixture;
    P.max_dim = find_max_dim_path(cfg.max_depth, cfg.rr_depth);
    P.eff_dim = std::min(P.max_dim, effective_dim_path(cfg.max_depth, cfg.rr_depth));
    P.p_large = cfg.p_large; P.sigma2 = cfg.scale_second * cfg.sigma;
    P.kelemen_weights = cfg.kelemen_style_weights; P.kelemen_mutation = cfg.kelemen_style_mutation;
    P.pss_sigma = cfg.sigma; P.luminance_b = 1.f;
    P.technique = cfg.technique; P.light_image = cfg.no_light_image ? 0 : 1; P.fix_emitter_path = cfg.fix_emitter_path;
    if (cfg.technique == DRMLT_TECH_MMLT) { // PSS layout of a chain: [sensor S | emitter E | direct] (device_bidir.h)
        P.mmlt_S = 2 * (cfg.max_depth + 1); P.mmlt_E = 2 * cfg.max_depth;
        P.mmlt_dmax = (cfg.max_depth + 2) * 3; P.mmlt_dmax += P.mmlt_dmax & 1; // pssmlt_utils.h:58-63
        P.max_dim = 2 * P.mmlt_dmax + 1;
        P.eff_dim = P.mmlt_S + P.mmlt_E + 1;
    }
    if (cfg.technique == DRMLT_TECH_BDPT) { // [sensor S | emitter E | direct Dd]: what the two walks and the direct strategies can consume (device_bdpt.h)
        const int rr = cfg.max_depth + 1 - (cfg.rr_depth > 0 ? cfg.rr_depth : 0);
        P.mmlt_S = 2 * (cfg.max_depth + 1) + (rr > 0 ? rr : 0); P.mmlt_S += P.mmlt_S & 1;
        P.mmlt_E = 2 * cfg.max_depth + (rr > 1 ? rr - 1 : 0); P.mmlt_E += P.mmlt_E & 1;
        P.mmlt_dmax = (cfg.max_depth + 2) * (2 + (cfg.rr_depth < cfg.max_depth ? 1 : 0)); P.mmlt_dmax += P.mmlt_dmax & 1; // pssmlt_utils.h:69-75
        // directSampling=true (the reference's default): every s = 1 / t = 1 connection draws two components of the direct
        // sampler (pathsampler.cpp:424-452, vertex.cpp:1304-1305), a sample makes up to maxDepth + (maxDepth - 1) of them. The
        // reference sizes that sampler maxDepth (pssmlt_utils.h:75) and reads past it; here it holds what can be consumed.
        P.bd_Dd = cfg.no_direct_sampling ? 0 : 2 * (2 * cfg.max_depth - 1); // bdpt_dims_direct, device_bdpt.h
        P.max_dim = 2 * P.mmlt_dmax + P.bd_Dd;
        P.eff_dim = P.mmlt_S + P.mmlt_E + P.bd_Dd;
    }

    P.debug = K.debug | (K.rule_generic ? DBG_RULE_GENERIC : 0) | (K.one_light_generic ? DBG_ONE_LIGHT_GENERIC : 0);
    // the first light's joined record (device_types.h: scene_has_one_light decides whether a kernel reads it)
    if (!out.emitters.empty()) { P.light = out.emitters[0]; P.light_shade = out.shade[(size_t) out.emitters[0].prim]; }
    for (const DBsdf &b : out.bsdfs) P.features |= b.type == DRMLT_BSDF_ROUGHCONDUCTOR ? 1 : ((b.type == DRMLT_BSDF_DIELECTRIC || b.type == DRMLT_BSDF_CONDUCTOR) ? 2 : 0);
    for (const DPrim &g : out.prims) if (g.type == PRIM_SPHERE) P.features |= 4;
    if (!out.normals.empty()) P.features |= 4; // not a flat polygon
    P.env_emitter = -1;
    for (int i = 0; i < scene.n_emitters; ++i) {
        if (scene.emitters[i].type == DRMLT_EMITTER_POINT) P.features |= 4; // what is not a polygon
        if (scene.emitters[i].type == DRMLT_EMITTER_CONSTANT) P.features |= 4, P.env_emitter = i;
    }
    if (P.use_bvh) P.features |= 8;
    if (K.feat_all) P.features = 15;

    // ---- what the chain count (workUnits = -1: derive_chains) and the chain kernel's build (plan_chains) rest on
    PlanInputs &in = out.plan;
    in.technique = cfg.technique; in.algo = cfg.algo;
    in.work_units = cfg.work_units; in.work_units_rule = cfg.work_units_rule;
    in.budget = (uint64_t) cam.width * cam.height * (uint64_t) cfg.sample_count; // drmlt.cpp:434-476
    in.features = P.features; in.use_bvh = P.use_bvh != 0; in.bvh_stack16 = P.bvh_stack16 != 0; in.bvh_overflow = out.ovf_entries > 0;
    in.n_shade = (uint32_t) P.n_shade; in.n_bsdfs = (uint32_t) P.n_bsdfs; in.n_emitters = (uint32_t) P.n_emitters;
    in.scene_bytes = P.use_bvh ? (uint64_t) P.n_bvh_nodes * sizeof(DBvh4Node) + out.prims.size() * sizeof(DPrim) : 0;
    in.eff_dim = P.eff_dim; in.max_depth = cfg.max_depth; in.mmlt_S = P.mmlt_S; in.mmlt_E = P.mmlt_E;
    in.n_box = P.n_box; in.n_flat_rec = P.n_flat_rec; in.has_plain_tri = P.has_plain_tri != 0;
    return "";
}
