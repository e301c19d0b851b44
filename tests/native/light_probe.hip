// Calls the device's light-sampling routines one element per thread and writes what they return (tests/light_probe.py builds
// and runs it, tests/test_gpu_lights.py checks the numbers). Nothing but the library's own headers; the shading, BSDF and
// emitter tables are the bytes tests/native/scene_prep_harness.cpp writes for a scene, i.e. what the library would upload.
//
//   light_probe <request> <result>
// request: int32 op, n, n_shade, n_bsdfs, n_emitters, 0, 0, 0; the DShade, DBsdf and DEmitter tables; n rows of NIN[op] float32.
// result:  n rows of NOUT[op] float32.
//   sphere    emitter, ref, sx, sy                 -> d, dist, n, pdf (sphere_sample_direct), sphere_pdf_direct(dist, |d.n|)
//   env       emitter, ref, n, sx, sy              -> d, dist, pdf (env_sample_direct), ray_eps_closest(ref), ray_eps_shadow(ref)
//   light     bsdf, p, n, s, wi, sx, sy            -> contribution, dd, dist (direct_emitter_sample<7, GlobalTables>; t = n x s)
//   pdf_area  emitter, ref, ref n, point, its n    -> emitter_direct_pdf_area<GlobalTables>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <hip/hip_runtime.h>
#include "device_direct.h"
#include "device_bdpt.h"

enum { OP_SPHERE, OP_ENV, OP_LIGHT, OP_PDF_AREA, N_OPS };
static const int NIN[N_OPS] = {6, 9, 15, 13}, NOUT[N_OPS] = {9, 7, 7, 1};
#define CHUNK 65536 // elements per launch

DEV void st3(float *o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

__global__ void k_probe(DParams P, GlobalTables T, int op, int n, int nin, int nout, const float *in, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *x = in + (size_t) i * nin;
    float *o = out + (size_t) i * nout;
    if (op == OP_SPHERE) {
        const DShade L = T.shade(T.emitter((int) x[0]).prim);
        f3 d = mk3(0.f, 0.f, 0.f), nn = d;
        float dist = 0.f, pdf = 0.f;
        sphere_sample_direct(ld3(L.origin), L.eu[0], L.inv_area, ld3(x + 1), x[4], x[5], d, dist, nn, pdf);
        st3(o, d); o[3] = dist; st3(o + 4, nn); o[7] = pdf;
        o[8] = sphere_pdf_direct(ld3(L.origin), L.eu[0], L.inv_area, ld3(x + 1), dist, fabsf(dot3(d, nn)));
    } else if (op == OP_ENV) {
        const DShade L = T.shade(T.emitter((int) x[0]).prim);
        f3 d = mk3(0.f, 0.f, 0.f);
        float dist = 0.f, pdf = 0.f;
        env_sample_direct(ld3(L.origin), L.eu[0], ld3(x + 1), ld3(x + 4), x[7], x[8], d, dist, pdf);
        st3(o, d); o[3] = dist; o[4] = pdf;
        o[5] = ray_eps_closest(ld3(x + 1)); o[6] = ray_eps_shadow(ld3(x + 1));
    } else if (op == OP_LIGHT) {
        const DBsdf B = T.bsdf((int) x[0]);
        const f3 nn = ld3(x + 4), s = ld3(x + 7);
        f3 dd = mk3(0.f, 0.f, 0.f);
        float dist = 0.f;
        const f3 c = direct_emitter_sample<7>(P, T, B, ld3(x + 1), nn, s, cross3(nn, s), ld3(x + 10), x[13], x[14], dd, dist);
        st3(o, c); st3(o + 3, dd); o[6] = dist;
    } else {
        o[0] = emitter_direct_pdf_area(T, ld3(x + 1), ld3(x + 4), false, ld3(x + 7), ld3(x + 10), (int) x[0]);
    }
}

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    fprintf(stderr, "light_probe: %s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)
#define BAD(...) do { fprintf(stderr, "light_probe: " __VA_ARGS__); fprintf(stderr, "\n"); return 2; } while (0)

int main(int argc, char **argv) {
    if (argc != 3) BAD("usage: light_probe <request> <result>");
    FILE *f = fopen(argv[1], "rb");
    int32_t head[8];
    if (!f || fread(head, 4, 8, f) != 8) BAD("cannot read %s", argv[1]);
    const int op = head[0], n = head[1], n_shade = head[2], n_bsdfs = head[3], n_emitters = head[4];
    if (op < 0 || op >= N_OPS || n < 0 || n_shade < 1 || n_shade > 4096 || n_bsdfs < 1 || n_bsdfs > 4096 || n_emitters < 1 || n_emitters > 4096) BAD("bad header");
    const int nin = NIN[op], nout = NOUT[op];
    std::vector<DShade> shade(n_shade);
    std::vector<DBsdf> bsdfs(n_bsdfs);
    std::vector<DEmitter> emitters(n_emitters);
    std::vector<float> in((size_t) n * nin), out((size_t) n * nout);
    if (fread(shade.data(), sizeof(DShade), n_shade, f) != (size_t) n_shade || fread(bsdfs.data(), sizeof(DBsdf), n_bsdfs, f) != (size_t) n_bsdfs ||
        fread(emitters.data(), sizeof(DEmitter), n_emitters, f) != (size_t) n_emitters || fread(in.data(), 4, in.size(), f) != in.size()) BAD("short request");
    fclose(f);
    // every index the device follows is checked here: an emitter's shape record, and per row the emitter or the BSDF
    for (int e = 0; e < n_emitters; ++e) {
        const int prim = emitters[e].prim;
        if (prim < 0 || prim >= n_shade) BAD("emitter %d: shape record %d outside the table", e, prim);
        const int kind = shade[prim].bsdf >> 24;
        if (kind != PRIM_TRIANGLE && kind != PRIM_RECTANGLE && kind != PRIM_SPHERE && kind != PRIM_POINT && kind != PRIM_ENV) BAD("emitter %d: kind %d has no probe", e, kind);
    }
    const int want_kind = op == OP_SPHERE ? PRIM_SPHERE : op == OP_ENV ? PRIM_ENV : -1;
    const int bound = op == OP_LIGHT ? n_bsdfs : n_emitters;
    for (int i = 0; i < n; ++i) {
        const float v = in[(size_t) i * nin];
        if (!(v >= 0.f && v < (float) bound && v == (float) (int) v)) BAD("row %d: bad index", i);
        if (want_kind >= 0 && (shade[emitters[(int) v].prim].bsdf >> 24) != want_kind) BAD("row %d: emitter %d is of another kind", i, (int) v);
    }
    DShade *dsh = nullptr;
    DBsdf *dbs = nullptr;
    DEmitter *dem = nullptr;
    float *di = nullptr, *dout = nullptr;
    const int cap = n < CHUNK ? (n > 0 ? n : 1) : CHUNK;
    HIP_OK(hipMalloc(&dsh, sizeof(DShade) * n_shade));
    HIP_OK(hipMalloc(&dbs, sizeof(DBsdf) * n_bsdfs));
    HIP_OK(hipMalloc(&dem, sizeof(DEmitter) * n_emitters));
    HIP_OK(hipMalloc(&di, sizeof(float) * cap * nin));
    HIP_OK(hipMalloc(&dout, sizeof(float) * cap * nout));
    HIP_OK(hipMemcpy(dsh, shade.data(), sizeof(DShade) * n_shade, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dbs, bsdfs.data(), sizeof(DBsdf) * n_bsdfs, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dem, emitters.data(), sizeof(DEmitter) * n_emitters, hipMemcpyHostToDevice));
    DParams P;
    memset(&P, 0, sizeof P);
    P.n_emitters = n_emitters; P.n_shade = n_shade; P.n_bsdfs = n_bsdfs;
    P.shade = dsh; P.bsdfs = dbs; P.emitters = dem;
    const GlobalTables T{dsh, dbs, dem};
    for (int at = 0; at < n; at += CHUNK) {
        const int m = n - at < CHUNK ? n - at : CHUNK;
        HIP_OK(hipMemcpy(di, in.data() + (size_t) at * nin, sizeof(float) * m * nin, hipMemcpyHostToDevice));
        k_probe<<<(m + 255) / 256, 256>>>(P, T, op, m, nin, nout, di, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data() + (size_t) at * nout, dout, sizeof(float) * m * nout, hipMemcpyDeviceToHost));
    }
    HIP_OK(hipFree(dsh)); HIP_OK(hipFree(dbs)); HIP_OK(hipFree(dem)); HIP_OK(hipFree(di)); HIP_OK(hipFree(dout));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) BAD("cannot write %s", argv[2]);
    return 0;
}
