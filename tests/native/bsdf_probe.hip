// Calls the device's local-frame BSDF, Fresnel and warp routines one element per thread and writes what they return
// (tests/bsdf_probe.py builds and runs it, tests/test_gpu_bsdf.py checks the numbers). Nothing but the library's own headers.
//
//   bsdf_probe <request> <result>
// request: int32 op, n, nmat, 0; nmat material records of 12 float32 (type, rgb[3], p[8]: the fields of DBsdf);
//          n rows of NIN[op] float32, column 0 the row's material index.
// result:  n rows of NOUT[op] float32.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <hip/hip_runtime.h>
#include "device_bidir.h"

enum { OP_RC_SAMPLE, OP_SA_EVAL, OP_DISTR, OP_FR_COND, OP_FR_DIEL, OP_WARP, OP_SCALAR, N_OPS };
static const int NIN[N_OPS] = {6, 7, 9, 8, 8, 3, 2}, NOUT[N_OPS] = {7, 8, 6, 10, 3, 3, 6};
#define CHUNK 65536 // elements per launch

struct Mat { float type, rgb[3], p[8]; };

DEV DBsdf bsdf_of(const Mat *mats, float idx) {
    const Mat &m = mats[(int) idx];
    DBsdf B;
    B.type = (int32_t) m.type;
    for (int c = 0; c < 3; ++c) B.rgb[c] = m.rgb[c];
    for (int c = 0; c < 8; ++c) B.p[c] = m.p[c];
    return B;
}
DEV void st3(float *o, f3 v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

__global__ void k_probe(int op, int n, int nin, int nout, const Mat *mats, const float *in, float *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *x = in + (size_t) i * nin;
    float *o = out + (size_t) i * nout;
    const DBsdf B = bsdf_of(mats, x[0]);
    if (op == OP_RC_SAMPLE) {          // wi, sx, sy -> wo, pdf, weight
        f3 wo = mk3(0.f, 0.f, 0.f);
        float pdf = 0.f;
        const f3 w = make_rc(B).sample(ld3(x + 1), x[4], x[5], wo, pdf);
        st3(o, wo); o[3] = pdf; st3(o + 4, w);
    } else if (op == OP_SA_EVAL) {     // wi, wo -> f cos, pdf, and the same with the two directions exchanged
        const f3 wi = ld3(x + 1), wo = ld3(x + 4);
        st3(o, bsdf_eval_sa(B, wi, wo)); o[3] = bsdf_pdf_sa(B, wi, wo);
        st3(o + 4, bsdf_eval_sa(B, wo, wi)); o[7] = bsdf_pdf_sa(B, wo, wi);
    } else if (op == OP_DISTR) {       // v, m, sx, sy -> D(m), G1(v, m), pdfVisible(v, m), sampleVisible(v, sx, sy)
        const DMicrofacet d = make_rc(B).distr;
        const f3 v = ld3(x + 1), m = ld3(x + 4);
        o[0] = d.eval(m); o[1] = d.smithG1(v, m); o[2] = d.pdfVisible(v, m);
        st3(o + 3, d.sampleVisible(v, x[7], x[8]));
    } else if (op == OP_FR_COND) {     // cos, wi, wo -> F per channel, the mirror's wo and weight, pdf_delta(wi, wo)
        const DConductor c = make_conductor(B);
        for (int ch = 0; ch < 3; ++ch) o[ch] = fresnel_conductor_exact(x[1], B.p[1 + ch], B.p[4 + ch]);
        f3 wo = mk3(0.f, 0.f, 0.f);
        const f3 w = c.sample(ld3(x + 2), wo);
        st3(o + 3, wo); st3(o + 6, w);
        o[9] = DConductor::pdf_delta(ld3(x + 2), ld3(x + 5));
    } else if (op == OP_FR_DIEL) {     // cos, wi, wo -> F, cosT, pdf_delta(wi, wo); eta = p[0], 1 / eta = p[1]
        float cosT = 0.f;
        o[0] = fresnel_dielectric_ext(x[1], cosT, B.p[0]);
        o[1] = cosT;
        o[2] = dielectric_pdf_delta(B, ld3(x + 2), ld3(x + 5));
    } else if (op == OP_WARP) {        // sx, sy -> direction
        st3(o, square_to_cosine_hemisphere(x[1], x[2]));
    } else {                           // x -> rc_exp, rc_log, mts_erf, mts_erfinv, sin_rev, cos_rev
        o[0] = rc_exp(x[1]); o[1] = rc_log(x[1]); o[2] = mts_erf(x[1]); o[3] = mts_erfinv(x[1]);
        o[4] = sin_rev(x[1]); o[5] = cos_rev(x[1]);
    }
}

#define HIP_OK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
    fprintf(stderr, "bsdf_probe: %s: %s\n", #call, hipGetErrorString(e_)); return 3; } } while (0)

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: bsdf_probe <request> <result>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t head[4];
    if (!f || fread(head, 4, 4, f) != 4) { fprintf(stderr, "bsdf_probe: cannot read %s\n", argv[1]); return 2; }
    const int op = head[0], n = head[1], nmat = head[2];
    if (op < 0 || op >= N_OPS || n < 0 || nmat < 1 || nmat > 4096) { fprintf(stderr, "bsdf_probe: bad header\n"); return 2; }
    const int nin = NIN[op], nout = NOUT[op];
    std::vector<Mat> mats(nmat);
    std::vector<float> in((size_t) n * nin), out((size_t) n * nout);
    if (fread(mats.data(), sizeof(Mat), nmat, f) != (size_t) nmat || fread(in.data(), 4, in.size(), f) != in.size()) {
        fprintf(stderr, "bsdf_probe: short request\n"); return 2;
    }
    fclose(f);
    for (int i = 0; i < n; ++i) { // a material index outside the table would be read out of bounds on the device
        const float m = in[(size_t) i * nin];
        if (!(m >= 0.f && m < (float) nmat && m == (float) (int) m)) { fprintf(stderr, "bsdf_probe: row %d: bad material\n", i); return 2; }
    }
    Mat *dm = nullptr;
    float *di = nullptr, *dout = nullptr;
    const int cap = n < CHUNK ? (n > 0 ? n : 1) : CHUNK;
    HIP_OK(hipMalloc(&dm, sizeof(Mat) * nmat));
    HIP_OK(hipMalloc(&di, sizeof(float) * cap * nin));
    HIP_OK(hipMalloc(&dout, sizeof(float) * cap * nout));
    HIP_OK(hipMemcpy(dm, mats.data(), sizeof(Mat) * nmat, hipMemcpyHostToDevice));
    for (int at = 0; at < n; at += CHUNK) {
        const int m = n - at < CHUNK ? n - at : CHUNK;
        HIP_OK(hipMemcpy(di, in.data() + (size_t) at * nin, sizeof(float) * m * nin, hipMemcpyHostToDevice));
        k_probe<<<(m + 255) / 256, 256>>>(op, m, nin, nout, dm, di, dout);
        HIP_OK(hipGetLastError());
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(out.data() + (size_t) at * nout, dout, sizeof(float) * m * nout, hipMemcpyDeviceToHost));
    }
    HIP_OK(hipFree(dm)); HIP_OK(hipFree(di)); HIP_OK(hipFree(dout));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) { fprintf(stderr, "bsdf_probe: cannot write %s\n", argv[2]); return 2; }
    return 0;
}
