// Device code of the direct-illumination pass: MIDirectIntegrator::Li for one camera ray, and the weighted film reconstruction
// of one pixel's samples. (The kernel around it: kernels_direct.hip; the host side: drmlt_render_direct, drmlt_capi.cpp.)
//
// Reference behaviour restated here (paths relative to the reference checkout):
//   renderDirectComponent    src/libbidir/util.cpp:30-92 (the `direct` integrator, hdrfilm, the scene's own filter)
//   MIDirectIntegrator::Li   src/integrators/direct/direct.cpp:146-314 (strictNormals = false, no subsurface, no media)
//   ImageBlock::put          include/mitsuba/render/imageblock.h:150-216 (weight channel; hdrfilm develops rgb / weight)
//
// The building blocks are device_path.h's: ray queries, tables, camera ray, the per-shape light samples. The light sample and
// the emitter-hit term are written out a second time below rather than carved out of path_step: path_step is inlined into every
// chain kernel, whose code must not move for a pass that runs once per render. The two copies follow the same lines of the
// reference (scene.cpp:879-904, path.cpp:190-218 = direct.cpp:220-244) and tests/test_gpu_direct.py holds one against the other.
//
// Random numbers: Philox block b of the stream addressed by (seed, pixel index of the full frame, pixel-sample index, TAG_DIRECT).
// Block 1 + j: shading sample j = (emitter sample, BSDF sample), independent draws. The position of pixel sample i inside its
// pixel is point i of the (0, 2)-sequence (van der Corput, Sobol' dimension 2; Kollig and Keller 2002), XOR-scrambled by two
// words of block 0 of the pixel's own stream (sample index DIRECT_PIXEL_STREAM): every point is uniform over the pixel, and
// the 2^k points of a pixel are stratified as those of the reference's `ldsampler` are (util.cpp:56-60).
#pragma once
#include "device_path.h"

#define DIRECT_PIXEL_STREAM 0xffffffffu
DEV float direct_vdc(uint32_t i, uint32_t scramble) { return u32_to_unit(__brev(i) ^ scramble); }
DEV float direct_sobol2(uint32_t i, uint32_t scramble) {
    for (uint32_t v = 1u << 31; i != 0u; i >>= 1, v ^= v >> 1)
        if (i & 1u) scramble ^= v;
    return u32_to_unit(scramble);
}

// One emitter sample at the surface point p (frame s, t, n; local incident direction wi; smooth BSDF B): Scene::sampleEmitterDirect
// without its visibility test, times BSDF and MIS weight (direct.cpp:220-244). Returns the contribution that waits for the shadow
// ray (dd, dist), zero if there is none. fracLum = fracBSDF = 1/2 cancel in the power heuristic.
template <int FEAT, class TablesT>
DEV f3 direct_emitter_sample(const DParams &P, const TablesT &T, const DBsdf &B, f3 p, f3 n, f3 s, f3 t, f3 wi, float sx, float sy, f3 &dd, float &dist) {
    const f3 zero = mk3(0.f, 0.f, 0.f);
    int ei = 0; // DiscreteDistribution::sample (lower_bound semantics)
    for (int i = 1; i < P.n_emitters; ++i)
        if (T.emitter_cdf_lo(i) < sx) ei = i;
    const DEmitter E = T.emitter(ei);
    const float emPdf = E.cdf_hi - E.cdf_lo;
    sx = (sx - E.cdf_lo) / emPdf; // sampleReuse
    const DShade L = T.emitter_shade(ei, E);
    const int kind = L.bsdf >> 24;
    f3 lp;
    float lu = 0.f, lv = 0.f; // a triangle's sample: barycentrics of p1 and p2
    if (kind == PRIM_RECTANGLE) lp = fma3(ld3(L.eu), sx, fma3(ld3(L.ev), sy, ld3(L.origin))); // rectangle.cpp:210-216
    else if ((FEAT & 4) && kind == PRIM_POINT) lp = ld3(L.origin);                            // point.cpp:131-151
    else { const float a = sqrtf(fmaxf(0.f, 1.f - sx)); lu = 1.f - a; lv = a * sy; lp = fma3(ld3(L.eu), lu, fma3(ld3(L.ev), lv, ld3(L.origin))); } // squareToUniformTriangle
    f3 ln = ld3(L.n);
    if ((FEAT & 4) && kind == PRIM_SMOOTH) smooth_record_normal(P, lu, lv, ln); // triangle.cpp:34-42: the interpolated normal; zero: pdf = 0 below
    const f3 dv = lp - p;
    const float dist2 = dot3(dv, dv);
    dist = sqrtf(dist2);
    dd = dv * (1.f / dist);
    float dln = dot3(dd, ln);
    float pdf = dln != 0.f ? L.inv_area * dist2 / fabsf(dln) : 0.f; // Shape::sampleDirect
    if ((FEAT & 4) && kind == PRIM_SPHERE) // sphere.cpp:286-355
        sphere_sample_direct(ld3(L.origin), L.eu[0], L.inv_area, p, sx, sy, dd, dist, ln, pdf), dln = dot3(dd, ln);
    if ((FEAT & 4) && kind == PRIM_ENV) // constant.cpp:173-214
        env_sample_direct(ld3(L.origin), L.eu[0], p, n, sx, sy, dd, dist, pdf), dln = -1.f;
    const bool point = (FEAT & 4) && kind == PRIM_POINT; // discrete pdf 1, value I / dist^2, not on a surface: bsdfPdf = 0, weight 1
    if (point) pdf = dist2, dln = -1.f;
    if (!(dot3(dd, n) >= 0.f && dln < 0.f && pdf != 0.f)) return zero; // AreaLight::sampleDirect (refN = n: a smooth BSDF reflects only)
    const f3 wo = mk3(dot3(dd, s), dot3(dd, t), dot3(dd, n));
    if (!(wi.z > 0.f && wo.z > 0.f)) return zero;
    f3 bsdfVal;
    float bsdfPdf;
    if (!(FEAT & 1) || B.type == 0) { // diffuse.cpp:110-127
        bsdfVal = ld3(B.rgb) * (INV_PI_F * wo.z);
        bsdfPdf = INV_PI_F * wo.z;
    } else { // roughconductor.cpp:258-323
        const DRoughConductor rc{DMicrofacet{B.p[7] != 0.f, fmaxf(B.p[0], 1e-4f)}, mk3(B.p[1], B.p[2], B.p[3]), mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
        bsdfVal = rc.eval(wi, wo);
        bsdfPdf = rc.pdf(wi, wo);
    }
    const float lpdf = pdf * emPdf;
    const float a = lpdf * lpdf, b = bsdfPdf * bsdfPdf;
    return ld3(E.radiance) * (1.f / lpdf) * bsdfVal * (point ? 1.f : a / (a + b));
}

// One BSDF sample at the same vertex (direct.cpp:251-306): the sampled ray is traced; it contributes if it meets an emitter's
// front side or leaves the scene into the environment, weighted against the emitter sampling's density (0 after a delta lobe).
template <int FEAT, class TablesT>
DEV f3 direct_bsdf_sample(const DParams &P, const TablesT &T, const DBsdf &B, bool transmissive, f3 p, f3 n, f3 s, f3 t, f3 wi, float bx, float by) {
    const f3 zero = mk3(0.f, 0.f, 0.f);
    f3 wo, bweight;
    float bpdf = 0.f;
    bool bdelta = false;
    if (B.type == 0) { // diffuse.cpp:139-149
        if (!(wi.z > 0.f)) return zero;
        wo = square_to_cosine_hemisphere(bx, by);
        bpdf = INV_PI_F * wo.z;
        bweight = ld3(B.rgb);
    } else if ((FEAT & 2) && B.type == 1) { // dielectric.cpp:270-306 (ERadiance)
        const float eta = B.p[0], invEta = B.p[1];
        float cosThetaT;
        const float F = fresnel_dielectric_ext(wi.z, cosThetaT, eta);
        bdelta = true;
        if (bx <= F) {
            wo = mk3(-wi.x, -wi.y, wi.z);
            bpdf = F;
            bweight = mk3(1.f, 1.f, 1.f);
        } else {
            const float scale = -(cosThetaT < 0.f ? invEta : eta);
            wo = mk3(scale * wi.x, scale * wi.y, cosThetaT);
            bpdf = 1.f - F;
            const float factor = cosThetaT < 0.f ? invEta : eta;
            bweight = mk3(factor * factor, factor * factor, factor * factor);
        }
    } else if ((FEAT & 1) && B.type == 2) { // roughconductor.cpp:371-409
        const DRoughConductor rc{DMicrofacet{B.p[7] != 0.f, fmaxf(B.p[0], 1e-4f)}, mk3(B.p[1], B.p[2], B.p[3]), mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
        bweight = rc.sample(wi, bx, by, wo, bpdf);
    } else if ((FEAT & 2) && B.type == 3) { // conductor.cpp:254-290
        const DConductor mc{mk3(B.p[1], B.p[2], B.p[3]), mk3(B.p[4], B.p[5], B.p[6]), ld3(B.rgb)};
        bweight = mc.sample(wi, wo);
        bpdf = 1.f;
        bdelta = true;
    } else return zero;
    if (is_zero3(bweight)) return zero;
    const f3 d = fma3(s, wo.x, fma3(t, wo.y, n * wo.z));
    const Hit h = trace<FEAT>(P, p, d, ray_eps_closest(p), INFINITY, false);
    f3 value;
    float lumPdf = 0.f; // Scene::pdfEmitterDirect
    if (h.prim < 0) { // the environment, if there is one (:284-294)
        if (!((FEAT & 4) && P.env_emitter >= 0)) return zero;
        const DEmitter E = T.emitter(P.env_emitter);
        value = ld3(E.radiance);
        if (!bdelta) lumPdf = INV_PI_F * fmaxf(0.f, dot3(d, n)) * (E.cdf_hi - E.cdf_lo);
    } else {
        const DShade S = T.shade(h.prim);
        if (S.emitter < 0) return zero;
        f3 en = ld3(S.n);
        const bool sphere = (FEAT & 4) && (S.bsdf >> 24) == PRIM_SPHERE;
        if (sphere) en = normalize3(fma3(d, h.t, p) - ld3(S.origin));
        if ((FEAT & 4) && (S.bsdf >> 24) == PRIM_SMOOTH) smooth_record_normal(P, h.u, h.v, en); // its.shFrame.n; zero: dn = 0, nothing
        const float dn = dot3(d, en);
        if (!(dn < 0.f)) return zero; // AreaLight::eval: dot(n, -d) > 0
        const DEmitter E = T.emitter(S.emitter);
        value = ld3(E.radiance);
        const float dr = transmissive ? 0.f : dot3(d, n); // DirectSamplingRecord(its) zeroes refN for a transmissive BSDF
        if (!bdelta && dr >= 0.f) {
            lumPdf = S.inv_area * h.t * h.t / fabsf(dn);
            if (sphere) lumPdf = sphere_pdf_direct(ld3(S.origin), S.eu[0], S.inv_area, p, h.t, fabsf(dn));
            lumPdf *= E.cdf_hi - E.cdf_lo;
        }
    }
    const float a = bpdf * bpdf, b = lumPdf * lumPdf;
    return value * bweight * (a / (a + b));
}

// MIDirectIntegrator::Li for the camera ray (o, d, [tmin, tmax]) of pixel sample `sample` of pixel `pixel`.
template <int FEAT, class TablesT>
DEV f3 direct_li(const DParams &P, const TablesT &T, const DirectJob &J, f3 o, f3 d, float tmin, float tmax, uint32_t pixel, uint32_t sample) {
    const Hit h = trace<FEAT>(P, o, d, tmin, tmax, false);
    if (h.prim < 0) { // :156-163: the environment's radiance, or nothing
        if ((FEAT & 4) && P.env_emitter >= 0 && !J.hide_emitters) return ld3(T.emitter(P.env_emitter).radiance);
        return mk3(0.f, 0.f, 0.f);
    }
    const DShade S = T.shade(h.prim);
    // surface point + shading frame (skdtree.h:340-429, rectangle.cpp:155-168, sphere.cpp:207-255)
    f3 p, n, s;
    if (!(FEAT & 4) || (S.bsdf >> 24) != PRIM_SPHERE) {
        p = fma3(ld3(S.eu), h.u, fma3(ld3(S.ev), h.v, ld3(S.origin)));
        n = ld3(S.n);
        s = ld3(S.eu) * S.inv_len_eu;
        // vertex normals (skdtree.h:355-396,426); a normal without a direction makes the sample invalid
        if ((FEAT & 4) && (S.bsdf >> 24) == PRIM_SMOOTH && !smooth_record_frame(P, h.u, h.v, n, s)) return mk3(0.f, 0.f, 0.f);
    } else {
        const f3 c = ld3(S.origin);
        const f3 local = normalize3(fma3(d, h.t, o) - c);
        p = fma3(local, S.eu[0], c);
        n = local;
        const float zrad2 = local.x * local.x + local.y * local.y, inv = rsqrtf(zrad2);
        s = zrad2 > 0.f ? mk3(-local.y * inv, local.x * inv, 0.f) : mk3(1.f, 0.f, 0.f);
    }
    f3 Li = mk3(0.f, 0.f, 0.f);
    if (S.emitter >= 0 && !J.hide_emitters && dot3(d, n) < 0.f) Li = ld3(T.emitter(S.emitter).radiance); // :166-167, area.cpp: front side only
    const f3 t = cross3(n, s);
    const f3 md = -d;
    const f3 wi = mk3(dot3(md, s), dot3(md, t), dot3(md, n));
    const DBsdf B = T.bsdf(S.bsdf & 0xffffff);
    // ESmooth: diffuse, rough conductor. The dielectric and the smooth conductor draw no emitter sample (:217)
    const bool smooth = P.n_emitters > 0 && (B.type == 0 || ((FEAT & 1) && B.type == 2));
    const bool transmissive = (FEAT & 2) && B.type == 1;
    f3 sum = mk3(0.f, 0.f, 0.f);
    for (int j = 0; j < J.shading_samples; ++j) {
        const Unit4 u = philox_unit4(J.key0, J.key1, 1u + (uint32_t) j, pixel, sample, TAG_DIRECT);
        if (smooth) {
            f3 dd;
            float dist;
            const f3 c = direct_emitter_sample<FEAT>(P, T, B, p, n, s, t, wi, u.v[0], u.v[1], dd, dist);
            if (!is_zero3(c)) { // the visibility test of sampleEmitterDirect (scene.cpp:891-893)
                const Hit sh = trace<FEAT>(P, p, dd, ray_eps_shadow(p), dist * (1.f - SHADOW_EPSILON_F), true);
                if (sh.prim < 0) sum = sum + c;
            }
        }
        sum = sum + direct_bsdf_sample<FEAT>(P, T, B, transmissive, p, n, s, t, wi, u.v[2], u.v[3]);
    }
    return fma3(sum, 1.f / (float) J.shading_samples, Li); // weightLum = weightBSDF = 1 / N
}

// All samples of the pixels a wave holds, through the scene's filter into `acc` (ImageBlock::put with its weight channel). Lane
// `lane` holds sample (lane mod G) of the wave's pixel (lane / G), G = 2^group_log2; `live`: the lane holds a sample at all;
// `have`: its group holds a pixel. Every target pixel of the (2 margin + 1)^2 window round the group's pixel gets the GROUP's sum,
// formed across its lanes in a fixed order: one add per source pixel instead of one per sample. Under the box filter (margin 0)
// a sample touches its own pixel only, every pixel has exactly one writer and the sum is stored, not added -- no float atomics,
// the image is a function of its arguments bit for bit. Called by all 64 lanes (cross-lane sums).
DEV void direct_film_put(const DParams &P, const DirectJob &J, bool live, bool have, uint32_t lane, int X, int Y, float px, float py, f3 L) {
    // an invalid sample is dropped, weight and all (imageblock.h:170-178)
    const bool ok = live && isfinite(L.x) && isfinite(L.y) && isfinite(L.z) && L.x >= 0.f && L.y >= 0.f && L.z >= 0.f;
    const float posx = px - 0.5f, posy = py - 0.5f;
    const int minx = (int) ceilf(posx - P.filter_radius), maxx = (int) floorf(posx + P.filter_radius);
    const int miny = (int) ceilf(posy - P.filter_radius), maxy = (int) floorf(posy + P.filter_radius);
    const bool box = P.box_weight > 0.f; // box table = one constant in entries 0..30 and 0 in entry 31
    const uint32_t G = 1u << J.group_log2;
    const bool writer = have && (lane & (G - 1u)) == 0u;
    for (int dy = -J.margin; dy <= J.margin; ++dy) {
        const int ty = Y + dy;
        const int iy = min((int) fabsf(((float) ty - posy) * P.filter_scale), 31);
        const float wy = (ok && ty >= miny && ty <= maxy) ? (box ? (iy < 31 ? P.box_weight : 0.f) : P.filter_lut[iy]) : 0.f;
        for (int dx = -J.margin; dx <= J.margin; ++dx) {
            const int tx = X + dx;
            const int ix = min((int) fabsf(((float) tx - posx) * P.filter_scale), 31);
            const float w = (ok && tx >= minx && tx <= maxx) ? (box ? (ix < 31 ? P.box_weight : 0.f) : P.filter_lut[ix]) * wy : 0.f;
            float r = w * L.x, g = w * L.y, b = w * L.z, ws = w;
            if (!ok) r = g = b = 0.f; // (0 * inf)
            for (uint32_t off = 1u; off < G; off <<= 1) {
                r += __shfl_xor(r, (int) off, 64); g += __shfl_xor(g, (int) off, 64);
                b += __shfl_xor(b, (int) off, 64); ws += __shfl_xor(ws, (int) off, 64);
            }
            if (writer && tx >= 0 && tx < P.width && ty >= J.row_lo && ty < J.row_hi) {
                float *dst = J.acc + ((size_t) (ty - J.row_lo) * P.width + tx) * 4;
                if (J.margin == 0) { dst[0] = r; dst[1] = g; dst[2] = b; dst[3] = ws; }
                else if (ws > 0.f) { atomic_add_global_f32(dst + 0, r); atomic_add_global_f32(dst + 1, g); atomic_add_global_f32(dst + 2, b); atomic_add_global_f32(dst + 3, ws); }
            }
        }
    }
}
