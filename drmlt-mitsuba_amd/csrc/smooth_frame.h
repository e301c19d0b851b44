// Shading frame of a triangle with vertex normals (technique=path, the direct pass): what TriMesh's intersection record and
// computeShadingFrame produce in the reference, as one routine shared by the kernels and the host (tests/native/normals_harness.cpp
// runs it on the CPU; it needs no HIP header).
//
// Reference behaviour restated here (paths relative to the reference checkout):
//   include/mitsuba/render/skdtree.h:355-396,426   shFrame.n = normalize(n0 (1 - u - v) + n1 u + n2 v): the vertex normals are
//                                                  interpolated AS STORED, only the sum is normalised
//   src/libcore/util.cpp:610-616                   computeShadingFrame: s = normalize(dpdu - n (n . dpdu)), t = n x s, dpdu = p1 - p0
//   src/libcore/triangle.cpp:34-42                 Triangle::sample hands the same interpolated normal to an area light's sample
// strictNormals is false on this path (integrator.cpp:221), so the geometric normal takes no part.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SMOOTH_FN __host__ __device__ inline
#else
#define SMOOTH_FN inline
#endif

// One entry of the device table (scene_prep.h fills it from drmlt_scene.normals): n0 and the two differences, so that the
// interpolation is two FMAs per component from the hit's own (u, v). 48 B = three 16-byte words, which the kernels fetch one
// after the other (device_path.h: smooth_record_frame).
struct DSmooth {
    float n0[3], pad0;
    float d1[3], pad1; // n1 - n0
    float d2[3], pad2; // n2 - n0
};

struct SmoothFrame {
    float nx, ny, nz; // unit shading normal, or (0, 0, 0): the interpolated normal has no direction (or dpdu none beside it)
    float sx, sy, sz; // unit tangent
};

// (a): the interpolated, unnormalised normal. (e): p1 - p0 times any positive factor (the frame does not depend on its length). A
// normal of zero length, or one that is not finite, gives the zero frame: the callers end the path there (an invalid sample,
// f = 0) where the reference would carry a NaN into the film.
SMOOTH_FN SmoothFrame smooth_finish(float ax, float ay, float az, float ex, float ey, float ez) {
    const float l2 = fmaf(ax, ax, fmaf(ay, ay, az * az));
    const float il = 1.f / sqrtf(l2);
    const float nx = ax * il, ny = ay * il, nz = az * il;
    const float d = fmaf(nx, ex, fmaf(ny, ey, nz * ez));
    const float bx = fmaf(-nx, d, ex), by = fmaf(-ny, d, ey), bz = fmaf(-nz, d, ez);
    const float m2 = fmaf(bx, bx, fmaf(by, by, bz * bz));
    const float im = 1.f / sqrtf(m2);
    const bool ok = l2 > 0.f && l2 < INFINITY && m2 > 0.f && m2 < INFINITY;
    SmoothFrame F;
    F.nx = ok ? nx : 0.f; F.ny = ok ? ny : 0.f; F.nz = ok ? nz : 0.f;
    F.sx = ok ? bx * im : 0.f; F.sy = ok ? by * im : 0.f; F.sz = ok ? bz * im : 0.f;
    return F;
}

// The normal alone (an area light's sample or hit: triangle.cpp:34-42): valid whenever the interpolated normal has a direction --
// no tangent takes part, so none can make it invalid.
SMOOTH_FN SmoothFrame smooth_finish_normal(float ax, float ay, float az) {
    const float l2 = fmaf(ax, ax, fmaf(ay, ay, az * az));
    const float il = 1.f / sqrtf(l2);
    const bool ok = l2 > 0.f && l2 < INFINITY;
    SmoothFrame F;
    F.nx = ok ? ax * il : 0.f; F.ny = ok ? ay * il : 0.f; F.nz = ok ? az * il : 0.f;
    F.sx = F.sy = F.sz = 0.f;
    return F;
}

// The frame at the barycentrics (u, v) of p1 and p2: n0 + u (n1 - n0) + v (n2 - n0) = n0 (1 - u - v) + n1 u + n2 v, then smooth_finish.
SMOOTH_FN SmoothFrame smooth_frame(const DSmooth &N, float ex, float ey, float ez, float u, float v) {
    return smooth_finish(fmaf(N.d2[0], v, fmaf(N.d1[0], u, N.n0[0])), fmaf(N.d2[1], v, fmaf(N.d1[1], u, N.n0[1])),
                         fmaf(N.d2[2], v, fmaf(N.d1[2], u, N.n0[2])), ex, ey, ez);
}
SMOOTH_FN SmoothFrame smooth_normal(const DSmooth &N, float u, float v) {
    return smooth_finish_normal(fmaf(N.d2[0], v, fmaf(N.d1[0], u, N.n0[0])), fmaf(N.d2[1], v, fmaf(N.d1[1], u, N.n0[1])),
                                fmaf(N.d2[2], v, fmaf(N.d1[2], u, N.n0[2])));
}

// The index of a PRIM_SMOOTH record's table entry travels through float registers (DShade::n[0], then the step's `n.x`) in kernels
// built to flush denormals: as plain bits a small index would be a denormal, and the first canonicalising operation on it would
// make it 0. It is therefore stored with bit 23 added -- every value a normal float -- and read back with smooth_index.
#define SMOOTH_INDEX_BIAS 0x00800000u
#define SMOOTH_INDEX_MAX 0x7f000000u // bits below the infinities' exponent
