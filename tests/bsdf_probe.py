"""Helper of tests/test_bsdf_probe.py and tests/test_gpu_bsdf.py: builds and runs tests/native/bsdf_probe.hip, lays out the
inputs, computes the references (the oracle in float and in double, and independent fp64 closed forms in numpy) and measures
the device against them under one rule:

    |device - oracle64| <= 32 * max |oracle32 - oracle64| + 4 ulp        per quantity and per cell

32 is the next power of two above what the project allowed itself when it moved exp and log to the hardware's base-2 units
(csrc/device_bsdf.h: ~2e-6 against 1e-7 for libm's, a factor 20). tests/test_gpu_bsdf.py writes the measured ratios as JSON where DRMLT_BSDF_PROBE_JSON names a file
(profiles/r10_bsdf_probe.json is one such run).
"""
import json
import os
import re
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "bsdf_probe.hip")
UNITS = ("kernels", "kernels_bdpt")       # the two device flag sets under which the routines are inlined in the library
OPS = dict(rc_sample=0, sa_eval=1, distr=2, fr_cond=3, fr_diel=4, warp=5, scalar=6)
NIN = dict(rc_sample=6, sa_eval=7, distr=9, fr_cond=8, fr_diel=8, warp=3, scalar=2)
NOUT = dict(rc_sample=7, sa_eval=8, distr=6, fr_cond=10, fr_diel=3, warp=3, scalar=6)
FACTOR = 32.0
EPS = 2.0 ** -23                          # one ulp of 1.f
F32 = np.float32


# ------------------------------------------------------------------ build and run
def _make_var(name):
    return subprocess.run(["make", "-s", "-C", CSRC, "--eval", "print-%: ; @echo $($*)", "print-" + name], check=True,
                          capture_output=True, text=True).stdout.split()


def flags(unit):
    """The library's device flags for one translation unit, read from its Makefile."""
    return _make_var("CXXFLAGS") + _make_var("DEVFLAGS") + _make_var("FLAGS_" + unit)


def build(out_dir, unit, src=SRC):
    """-> (executable, the compiler's kernel-resource-usage remarks). src: the probe program (tests/light_probe.py has another)."""
    name = os.path.splitext(os.path.basename(src))[0]
    exe = os.path.join(str(out_dir), name + "_" + unit)
    hipcc = _make_var("HIPCC")[0]
    r = subprocess.run([hipcc, "--offload-arch=" + _make_var("ARCH")[0], *flags(unit), "-I", CSRC,
                        "-Rpass-analysis=kernel-resource-usage", "-o", exe, src], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s does not compile (%s):\n%s" % (name, unit, r.stderr[-4000:]))
    return exe, r.stderr


def resource(remarks, key):
    return [int(v) for v in re.findall(r"remark:\s+%s[^:]*: (\d+)" % re.escape(key), remarks)]


class ProbeDied(RuntimeError):
    pass


class Probe:
    """Runs the program as a fresh child process, one at a time. After a run that failed, was killed or timed out nothing
    more is started: `dead` holds the reason."""
    dead = None                            # shared by every instance: one fault ends all GPU work of the module

    def __init__(self, exe, work_dir):
        self.exe, self.dir, self.runs = exe, str(work_dir), 0

    def run(self, op, mats, rows):
        if Probe.dead:
            raise ProbeDied(Probe.dead)
        rows = np.ascontiguousarray(rows, dtype=F32)
        mats = np.ascontiguousarray(mats, dtype=F32).reshape(-1, 12)
        assert rows.ndim == 2 and rows.shape[1] == NIN[op], rows.shape
        assert np.all((rows[:, 0] >= 0) & (rows[:, 0] < len(mats)))
        req, res = os.path.join(self.dir, op + ".req"), os.path.join(self.dir, op + ".res")
        with open(req, "wb") as f:
            f.write(struct.pack("<4i", OPS[op], len(rows), len(mats), 0))
            f.write(mats.tobytes())
            f.write(rows.tobytes())
        self.runs += 1
        try:
            r = subprocess.run(["timeout", "-k", "10", "60", self.exe, req, res], capture_output=True, text=True, timeout=80)
        except subprocess.TimeoutExpired:
            Probe.dead = "%s %s: no answer within 80 s" % (os.path.basename(self.exe), op)
            raise ProbeDied(Probe.dead)
        if r.returncode != 0:
            Probe.dead = "%s %s: exit status %d: %s" % (os.path.basename(self.exe), op, r.returncode, r.stderr[-500:])
            raise ProbeDied(Probe.dead)
        out = np.fromfile(res, dtype=F32)
        os.remove(req), os.remove(res)
        return out.reshape(len(rows), NOUT[op])


# ------------------------------------------------------------------ inputs
COPPER = ((0.2004, 0.9240, 1.1022), (3.9129, 2.4528, 2.1421))
MATERIALS = dict(copper=COPPER, k_only=((0.0,) * 3, (1e3,) * 3), eta_only=((1.5,) * 3, (0.0,) * 3))
REFL = (0.9, 0.8, 0.7)
ALPHAS = (1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5, 1.0)
WI_Z = (1.0, 0.999995, 0.99998, 0.9, 0.5, 0.1, 0.02, 1e-3)
ONE_M = 1.0 - 2.0 ** -24
CORNERS = (0.0, 2.0 ** -24, 1e-6, 0.5, 0.5 + 2.0 ** -24, ONE_M)


def sample_points():
    """The 64 x 64 stratified midpoints, then the 36 corner pairs: (4132, 2) float32."""
    g = (np.arange(64, dtype=F32) + F32(0.5)) / F32(64)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    c = np.array(CORNERS, dtype=F32)
    return np.concatenate([grid, np.stack(np.meshgrid(c, c, indexing="ij"), axis=-1).reshape(-1, 2)]).astype(F32)


N_GRID = 4096


def _dir(z, azimuth=(0.6, 0.8)):
    s = np.sqrt(max(0.0, 1.0 - z * z))
    return np.array([s * azimuth[0], s * azimuth[1], z]).astype(F32)


def _z_for_stretched(z_stretched, alpha):
    """wi.z whose alpha-stretched, renormalised direction has z = z_stretched (microfacet.h:424-426)."""
    t = np.sqrt(1.0 - z_stretched ** 2) / z_stretched / alpha
    return 1.0 / np.sqrt(1.0 + t * t)


def rc_cells():
    """(model, alpha, material, wi) cells of the rough conductor and its distribution."""
    cells = []
    for ggx in (0, 1):
        for alpha in ALPHAS:
            wis = [("z=%g" % z, _dir(z)) for z in WI_Z]
            wis += [("z=0.5 az=%d" % (90 * i), _dir(0.5, az)) for i, az in enumerate(((1, 0), (0, 1), (-1, 0), (0, -1)))]
            if alpha in (0.1, 1.0):        # either side of the wi.z < 0.99999 test of sampleVisible, clear of fp32 rounding
                wis += [("stretched z=0.99999%+g" % d, _dir(_z_for_stretched(0.99999 + d, alpha))) for d in (-2e-6, 2e-6)]
            wis += [("z=0", _dir(0.0)), ("z=-0.5", _dir(-0.5))]
            cells += [dict(ggx=ggx, alpha=alpha, mat="copper", tag=t, wi=w) for t, w in wis]
            if alpha == 0.1:
                cells += [dict(ggx=ggx, alpha=alpha, mat=m, tag="z=%g" % z, wi=_dir(z)) for m in ("k_only", "eta_only") for z in (0.9, 0.1)]
    for c in cells:
        c["name"] = "%s a=%g %s %s" % ("ggx" if c["ggx"] else "beckmann", c["alpha"], c["mat"], c["tag"])
    return cells


def material_row(bsdf_type, p, rgb=REFL):
    return [float(bsdf_type), *rgb, *p]


def rc_material(c):
    eta, k = MATERIALS[c["mat"]]
    return material_row(2, [c["alpha"], *eta, *k, float(c["ggx"])])


def hemisphere_dirs(n=256, seed=3):
    r = np.random.default_rng(seed)
    z, phi = 1.0 - r.random(n), 2 * np.pi * r.random(n)
    s = np.sqrt(1 - z * z)
    return np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1).astype(F32)


DIEL_ETAS = (1.0, 1.000277, 1.33, 1.5046, 2.4, 1 / 1.5)
DIEL_COS = (0.0, 1e-4, 1e-2, 0.3, 0.7, 1.0)


def dielectric_inputs():
    """(eta, cos) pairs as float32: the listed cosines of both signs and the critical angle -+ {1e-2, 1e-3, 1e-4, 0}."""
    rows = []
    for eta in DIEL_ETAS:
        e = float(F32(eta))
        cs = [s * c for c in DIEL_COS for s in (1, -1)]
        if e != 1.0:                       # total internal reflection from the denser side: sin^2 = 1 / max(eta, 1/eta)^2
            big = max(e, 1 / e)
            crit = np.sqrt(1 - 1 / big ** 2) * (-1 if e > 1 else 1)
            cs += [crit + np.sign(crit) * s * d for d in (1e-2, 1e-3, 1e-4, 0.0) for s in (1, -1)]
        rows += [(e, float(F32(c))) for c in cs]
    return np.array(rows, dtype=np.float64)


def warp_points():
    g = (np.arange(128, dtype=F32) + F32(0.5)) / F32(128)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    t = np.linspace(0, ONE_M, 257).astype(F32)
    e = np.array([0.0, 0.5, ONE_M], dtype=F32)
    edges = [np.stack(np.meshgrid(e, t, indexing="ij"), axis=-1).reshape(-1, 2), np.stack(np.meshgrid(t, e, indexing="ij"), axis=-1).reshape(-1, 2)]
    diag = [np.stack([t, t], axis=1), np.stack([t, (F32(1) - t).astype(F32)], axis=1)]
    return np.concatenate([grid, sample_points()[N_GRID:], *edges, *diag, [[0.5, 0.5]]]).astype(F32)


# ------------------------------------------------------------------ independent fp64 references (numpy)
def fresnel_conductor_complex(cos_i, eta, k):
    """1/2 (|r_s|^2 + |r_p|^2) from the complex index n = eta + i k."""
    c = np.asarray(cos_i, dtype=np.float64)
    n = np.asarray(eta, dtype=np.float64) + 1j * np.asarray(k, dtype=np.float64)
    ct = np.sqrt(n * n - (1 - c * c)) / n          # n cos(theta_t) = sqrt(n^2 - sin^2)
    rs = (c - n * ct) / (c + n * ct)
    rp = (n * c - ct) / (n * c + ct)
    return 0.5 * (np.abs(rs) ** 2 + np.abs(rp) ** 2)


def fresnel_dielectric_signed(cos_i, eta):
    """Fresnel reflectance and the signed cosine of the refracted direction for either side (fp64): from below, the relative
    index is 1 / eta. Built on tests/direct_scenes.py's front-side formula. -> (F, cosT, cosT^2 before the clamp)."""
    import direct_scenes as ds
    c, eta = np.broadcast_arrays(np.asarray(cos_i, dtype=np.float64), np.asarray(eta, dtype=np.float64))
    rel = np.where(c > 0, eta, 1 / eta)
    with np.errstate(invalid="ignore"):            # 0 / 0 at cos = 0 under total reflection, where F is selected to be 1
        F, ct = ds.fresnel_dielectric(np.abs(c), rel)
    ct2 = 1.0 - (1.0 - c * c) / (rel * rel)
    same = eta == 1
    return np.where(same, 0.0, F), np.where(same, -c, np.where(ct2 <= 0, 0.0, np.where(c > 0, -ct, ct))), np.where(same, c * c, ct2)


def cosine_hemisphere(sxy):
    """Shirley's concentric map and the lift onto the hemisphere, fp64."""
    s = np.asarray(sxy, dtype=np.float64)
    a, b = 2 * s[:, 0] - 1, 2 * s[:, 1] - 1
    first = a * a > b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, a, b)
        phi = np.where(first, (np.pi / 4) * (b / a), np.pi / 2 - (np.pi / 4) * (a / b))
    phi = np.where((a == 0) & (b == 0), 0.0, phi)
    x, y = r * np.cos(phi), r * np.sin(phi)
    z = np.sqrt(np.maximum(0.0, 1 - x * x - y * y))
    return np.stack([x, y, np.where(z == 0, 1e-10, z)], axis=1)


# ------------------------------------------------------------------ the rule
def rel_err(a, ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(a - ref) / np.abs(ref)


def worst(err, mask=None):
    err = np.asarray(err, dtype=np.float64)
    if mask is not None:
        err = err[mask]
    return float(np.max(err)) if err.size else 0.0


def judge(dev_err, floor):
    """-> dict(dev, floor, bound, ratio = dev / bound): the device meets the rule where ratio <= 1."""
    bound = FACTOR * floor + 4 * EPS
    return dict(dev=dev_err, floor=floor, bound=bound, ratio=dev_err / bound)


# ------------------------------------------------------------------ the rough conductor's references
def rc_reference(ob, cells, sxy):
    """Per cell the oracle in both precisions: the samples for sxy, and D, G1, pdfVisible at the fp64 oracle's sampled normal
    rounded to float32. Computed once and shared."""
    ref = []
    for c in cells:
        eta, k = MATERIALS[c["mat"]]
        wi = np.repeat(c["wi"][None, :].astype(np.float64), len(sxy), axis=0)
        kw = dict(ggx=c["ggx"], alpha=float(F32(c["alpha"])), eta=np.array(eta, dtype=F32), k=np.array(k, dtype=F32), wi=wi, sxy=sxy,
                  specular_reflectance=np.array(REFL, dtype=F32))
        m = ob.bsdf_probe(64, **kw)["m"].astype(F32)
        ref.append({p: ob.bsdf_probe(p, m=m, **kw) for p in (64, 32)})
        ref[-1]["m_in"] = m
    return ref


GROUPS = (("", slice(0, N_GRID)), ("corners ", slice(N_GRID, None)))   # the stratified grid and the corner pairs are judged apart


def _id_eval(weight, pdf, ev):
    return np.abs(weight * pdf[:, None] - ev).max(axis=1) / np.maximum(ev.max(axis=1), 1e-300)


def rc_floors(ref, c, part=slice(0, N_GRID)):
    """The fp32 oracle against the fp64 oracle in one cell, over the grid (or the corner pairs): the rule's floors, and the
    number of samples that one precision rejects and the other accepts."""
    o64, o32 = ({k: v[part] for k, v in ref[p].items()} for p in (64, 32))
    rej64, rej32 = np.all(o64["weight"] == 0, axis=1), np.all(o32["weight"] == 0, axis=1)
    ok = ~rej64 & ~rej32
    vis = (o64["pdf_visible"] > 0) & (o32["pdf_visible"] > 0)
    fl = dict(wo=worst(np.abs(o32["wo"] - o64["wo"]).max(axis=1), ok), weight=worst(np.abs(o32["weight"] - o64["weight"]).max(axis=1), ok),
              pdf=worst(rel_err(o32["spdf"], o64["spdf"]), ok), m=worst(np.abs(o32["m"] - o64["m"]).max(axis=1)) if c["wi"][2] > 0 else 0.0,
              D=worst(rel_err(o32["D"], o64["D"]), (o64["D"] > 0) & (o32["D"] > 0)), G1=worst(np.abs(o32["G1"] - o64["G1"])),
              pdf_visible=worst(rel_err(o32["pdf_visible"], o64["pdf_visible"]), vis),
              id_pdf=worst(rel_err(o32["pdf_at_wo"], o32["spdf"]), ok & (o32["pdf_at_wo"] > 0)),
              id_eval=worst(_id_eval(o32["weight"], o32["spdf"], o32["eval_at_wo"]), ok & (o32["eval_at_wo"].max(axis=1) > 0)))
    return fl, int(np.sum(rej64 != rej32))


# ------------------------------------------------------------------ the measurement (GPU)
def measure_rc(ob, probe, cells, sxy, ref, uniform):
    """rc_sample, distr and sa_eval of every cell in three runs -> per-cell records."""
    mats = np.array([rc_material(c) for c in cells], dtype=F32)
    n, ns = len(cells), len(sxy)
    idx = np.repeat(np.arange(n, dtype=F32), ns)[:, None]
    wi = np.repeat(np.stack([c["wi"] for c in cells]), ns, axis=0)
    s = np.tile(sxy, (n, 1))
    smp = probe.run("rc_sample", mats, np.concatenate([idx, wi, s], axis=1)).reshape(n, ns, 7)
    m_in = np.concatenate([r["m_in"] for r in ref])
    dis = probe.run("distr", mats, np.concatenate([idx, wi, m_in, s], axis=1)).reshape(n, ns, 6)
    # sa_eval: per cell the fp64 oracle's sampled directions, the device's own, the mirror direction and the uniform ones
    extra = 1 + len(uniform)
    rows = []
    for i, (c, r) in enumerate(zip(cells, ref)):
        wo = np.concatenate([r[64]["wo"].astype(F32), smp[i, :, 0:3], (c["wi"] * F32([-1, -1, 1]))[None, :], uniform])
        rows.append(np.concatenate([np.full((len(wo), 1), i, dtype=F32), np.repeat(c["wi"][None, :], len(wo), axis=0), wo], axis=1))
    # ... and the diffuse BSDF (type 0) from four incident directions, one of them below the surface, towards +-uniform
    dwi = np.stack([_dir(z) for z in (1.0, 0.5, 1e-3, -0.5)])
    dwo = np.concatenate([uniform, uniform * F32([1, 1, -1])])
    drows = np.concatenate([np.concatenate([np.full((len(dwo), 1), n, dtype=F32), np.repeat(w[None, :], len(dwo), axis=0), dwo], axis=1) for w in dwi])
    sa = probe.run("sa_eval", np.concatenate([mats, np.array([material_row(0, [0] * 8)], dtype=F32)]), np.concatenate(rows + [drows]))
    sa, dsa = sa[:n * (2 * ns + extra)].reshape(n, 2 * ns + extra, 8), sa[n * (2 * ns + extra):].astype(np.float64)
    out = [diffuse_record(drows.astype(np.float64), dsa)]
    for i, (c, r) in enumerate(zip(cells, ref)):
        out.append(rc_cell_record(ob, c, r, sxy, smp[i].astype(np.float64), dis[i].astype(np.float64), sa[i].astype(np.float64), uniform))
    return out, dict(rc_sample=smp, distr=dis, sa_eval=sa)


def diffuse_record(rows, d):
    """bsdf_eval_sa / bsdf_pdf_sa of the diffuse BSDF against rgb / pi * wo.z and wo.z / pi; 0 unless both directions are above."""
    wi_z, wo_z = rows[:, 3], rows[:, 6]
    up = (wi_z > 0) & (wo_z > 0)
    rgb = np.array(REFL, dtype=F32).astype(np.float64)
    want = np.where(up[:, None], rgb[None, :] / np.pi * wo_z[:, None], 0.0)
    f32 = (np.array(REFL, dtype=F32)[None, :] * (F32(1 / np.pi) * wo_z.astype(F32))[:, None]).astype(np.float64)   # the same product in float
    rec = dict(name="diffuse", nonfinite=int((~np.isfinite(d)).sum()), corner_rejections=[],
               zero_below=bool(np.all(d[~up] == 0)), checks={})
    rec["checks"]["f_cos"] = judge(worst(np.abs(d[:, 0:3] - want).max(axis=1), up), worst(np.abs(f32 - want).max(axis=1), up))
    rec["checks"]["pdf_sa"] = judge(worst(np.abs(d[:, 3] - want[:, 0] / rgb[0]), up), worst(np.abs(f32[:, 0] / rgb[0] - want[:, 0] / rgb[0]), up))
    rec["checks"]["reciprocity"] = judge(worst(np.abs(d[:, 0] / wo_z - d[:, 4] / wi_z), up), worst(np.abs(f32[:, 0] / wo_z - rgb[0] / np.pi), up))
    return rec


def rc_cell_record(ob, c, r, sxy, smp, dis, sa, uniform):
    o64, o32 = r[64], r[32]
    ns = len(sxy)
    rec = dict(name=c["name"], checks={}, nonfinite=0, corner_rejections=[])
    wo, pdf, wt = smp[:, 0:3], smp[:, 3], smp[:, 4:7]
    rej_d, rej64, rej32 = np.all(wt == 0, axis=1), np.all(o64["weight"] == 0, axis=1), np.all(o32["weight"] == 0, axis=1)
    if not c["wi"][2] > 0:                     # wi.z <= 0: weight, pdf, f cos and the solid-angle pdf exactly zero
        rec["zero_below"] = bool(np.all(wt == 0) and np.all(pdf == 0) and np.all(sa[:, 0:4] == 0))
        return rec
    rec["nonfinite"] = int((~np.isfinite(smp)).sum() + (~np.isfinite(dis)).sum() + (~np.isfinite(sa)).sum())
    rec["rejection_mismatch_grid"] = int(np.sum((rej_d != rej64)[:N_GRID]))
    rec["corner_rejections"] = [dict(sx=float(sxy[j, 0]), sy=float(sxy[j, 1]), device=bool(rej_d[j]), oracle64=bool(rej64[j]), oracle32=bool(rej32[j]))
                                for j in range(N_GRID, ns) if rej_d[j] != rej64[j]]
    rec["D_zero_mismatch"] = int(np.sum((dis[:, 0] > 0) != (o64["D"] > 0)))
    # sa_eval at the fp64 oracle's directions, the mirror direction and the uniform ones: f cos and pdf against the oracle
    eta, k = MATERIALS[c["mat"]]
    sel = np.r_[0:ns, 2 * ns:len(sa)]
    wo_in = np.concatenate([o64["wo"].astype(F32), (c["wi"] * F32([-1, -1, 1]))[None, :], uniform]).astype(np.float64)
    kw = dict(ggx=c["ggx"], alpha=float(F32(c["alpha"])), eta=np.array(eta, dtype=F32), k=np.array(k, dtype=F32),
              wi=np.repeat(c["wi"][None, :].astype(np.float64), len(wo_in), axis=0), wo=wo_in, specular_reflectance=np.array(REFL, dtype=F32))
    e64, e32 = ob.bsdf_probe(64, **kw), ob.bsdf_probe(32, **kw)
    d = sa[sel]
    rec["eval_zero_mismatch"] = int(np.sum((d[:, 3] > 0) != (e64["pdf"] > 0)))
    g = lambda a: a[:, 1]                      # the green channel: every material's is non-zero
    with np.errstate(divide="ignore", invalid="ignore"):
        rcp = lambda e, er: np.abs(g(e) / wo_in[:, 2] - g(er) / c["wi"][2]) / np.abs(g(e) / wo_in[:, 2])
        rcp_d, rcp_32 = rcp(d[:, 0:3], d[:, 4:7]), rcp(e32["eval"], e32["eval_rev"])
    lit = (e64["pdf"] > 0) & (e32["pdf"] > 0) & (d[:, 3] > 0) & np.all(np.isfinite(d), axis=1) & (g(e64["eval"]) > 0)
    both = lit & (g(d[:, 0:3]) > 0) & (g(d[:, 4:7]) > 0) & (g(e32["eval"]) > 0) & (g(e32["eval_rev"]) > 0)
    own = sa[ns:2 * ns]                        # eval / pdf at the device's own sampled direction
    acc = ~rej_d & np.all(np.isfinite(own), axis=1) & np.isfinite(pdf) & (own[:, 3] > 0)
    ok = ~rej_d & ~rej64 & ~rej32 & np.all(np.isfinite(smp), axis=1)
    fin = np.all(np.isfinite(dis), axis=1)
    ch = rec["checks"]
    for tag, part in GROUPS:
        fl, _ = rc_floors(r, c, part)
        P = np.zeros(ns, dtype=bool)
        P[part] = True
        ch[tag + "wo"] = judge(worst(np.abs(wo - o64["wo"]).max(axis=1), ok & P), fl["wo"])
        ch[tag + "weight"] = judge(worst(np.abs(wt - o64["weight"]).max(axis=1), ok & P), fl["weight"])
        ch[tag + "pdf"] = judge(worst(rel_err(pdf, o64["spdf"]), ok & P), fl["pdf"])
        ch[tag + "m"] = judge(worst(np.abs(dis[:, 3:6] - o64["m"]).max(axis=1), fin & P), fl["m"])
        ch[tag + "D"] = judge(worst(rel_err(dis[:, 0], o64["D"]), fin & P & (o64["D"] > 0) & (o32["D"] > 0) & (dis[:, 0] > 0)), fl["D"])
        ch[tag + "G1"] = judge(worst(np.abs(dis[:, 1] - o64["G1"]), fin & P), fl["G1"])
        ch[tag + "pdf_visible"] = judge(worst(rel_err(dis[:, 2], o64["pdf_visible"]), fin & P & (o64["pdf_visible"] > 0) & (o32["pdf_visible"] > 0) & (dis[:, 2] > 0)),
                                        fl["pdf_visible"])
        # the sample's pdf and weight against pdf and eval at the sampled direction, on the device's own output
        ch[tag + "id_pdf"] = judge(worst(rel_err(own[:, 3], pdf), acc & P), fl["id_pdf"])
        ch[tag + "id_eval"] = judge(worst(_id_eval(wt, pdf, own[:, 0:3]), acc & P & (own[:, 0:3].max(axis=1) > 0)), fl["id_eval"])
    for tag, part in GROUPS + (("dirs ", slice(ns, None)),):    # dirs: the mirror direction and the uniform ones
        P = np.zeros(len(d), dtype=bool)
        P[part if tag != "corners " else slice(N_GRID, ns)] = True
        ch[tag + "f_cos"] = judge(worst(rel_err(g(d[:, 0:3]), g(e64["eval"])), lit & P), worst(rel_err(g(e32["eval"]), g(e64["eval"])), lit & P))
        ch[tag + "pdf_sa"] = judge(worst(rel_err(d[:, 3], e64["pdf"]), lit & P), worst(rel_err(e32["pdf"], e64["pdf"]), lit & P))
        ch[tag + "reciprocity"] = judge(worst(rcp_d, both & P), worst(rcp_32, both & P))
    return rec


def rotated(v, one_minus_cos):             # v turned by the angle in its vertical plane, away from the surface: it stays on its side
    up = np.array([[0.0, 0.0, 1.0]]) - v * v[:, 2:3]
    ln = np.linalg.norm(up, axis=1)[:, None]
    up = np.where(ln > 1e-6, up / np.maximum(ln, 1e-300), [[1.0, 0.0, 0.0]]) * np.where(v[:, 2:3] < 0, -1.0, 1.0)
    cth = 1 - one_minus_cos
    return v * cth + up * np.sqrt(1 - cth * cth)


def measure_fresnel(ob, probe):
    out = {}
    # conductor: every material's channels over cos in [0, 1]; eta_only against the dielectric formula as well
    cos = np.concatenate([np.linspace(0, 1, 513), [1e-4, 1e-3, 1 - 1e-6]]).astype(F32)
    names = list(MATERIALS)
    mats = np.array([material_row(3, [0.0, *MATERIALS[m][0], *MATERIALS[m][1], 0.0]) for m in names], dtype=F32)
    wi = np.stack([np.sqrt(np.maximum(0, 1 - cos.astype(np.float64) ** 2)) * 0.6, np.sqrt(np.maximum(0, 1 - cos.astype(np.float64) ** 2)) * 0.8, cos], axis=1).astype(F32)
    mir = wi * F32([-1, -1, 1])
    rows = np.concatenate([np.concatenate([np.full((len(cos), 1), i, dtype=F32), cos[:, None], wi, mir], axis=1) for i in range(len(names))])
    # pdf_delta once more with wo turned away from the mirror direction, to either side of DeltaEpsilon = 1e-3
    turned = [np.concatenate([np.zeros((len(cos), 1), dtype=F32), cos[:, None], wi, rotated(mir.astype(np.float64), e).astype(F32)], axis=1) for e in (0.5e-3, 2e-3)]
    d = probe.run("fr_cond", mats, np.concatenate([rows, *turned])).astype(np.float64)
    near, far = d[len(rows):len(rows) + len(cos), 9], d[len(rows) + len(cos):, 9]
    d = raw_cond = d[:len(rows)].reshape(len(names), len(cos), 10)
    for i, m in enumerate(names):
        eta, k = np.array(MATERIALS[m][0], dtype=F32).astype(np.float64), np.array(MATERIALS[m][1], dtype=F32).astype(np.float64)
        c64 = cos.astype(np.float64)[:, None]
        want = fresnel_conductor_complex(c64, eta[None, :], k[None, :])
        o32 = np.stack([ob.fresnel_conductor(32, cos, eta[j], k[j]) for j in range(3)], axis=1)
        rec = dict(F=judge(worst(np.abs(d[i, :, 0:3] - want)), worst(np.abs(o32 - want))), nonfinite=int((~np.isfinite(d[i])).sum()),
                   in_unit=bool(np.all((d[i, :, 0:3] >= 0) & (d[i, :, 0:3] <= 1))), at_grazing_ulp=float(np.max(np.abs(d[i, 0, 0:3] - 1)) / EPS),
                   mirror_wo=bool(np.array_equal(d[i, :, 3:6], mir.astype(np.float64))),
                   weight=judge(worst(np.abs(d[i, 1:, 6:9] - want[1:] * np.array(REFL, dtype=F32)[None, :])), worst(np.abs(o32 - want))),
                   weight_zero_at_grazing=bool(np.all(d[i, 0, 6:9] == 0)), pdf_delta_is_one=bool(np.all(d[i, 1:, 9] == 1) and d[i, 0, 9] == 0), pdf_delta_far_is_zero=bool(np.all(far == 0)),
                   pdf_delta_near_share=float(np.mean(near[1:] == 1)))
        if m == "eta_only":
            Fd, _, _ = fresnel_dielectric_signed(cos.astype(np.float64), 1.5)
            rec["as_dielectric"] = judge(worst(np.abs(d[i, :, 0] - Fd)), worst(np.abs(o32[:, 0] - Fd)))
        out["conductor " + m] = rec
    # dielectric: F and cosT over the (eta, cos) list; pdf_delta at the exact and the rotated directions
    ec = dielectric_inputs()
    eta, cs = ec[:, 0], ec[:, 1]
    F64, ct64, ct2 = fresnel_dielectric_signed(cs, eta)
    etas = sorted(set(eta))
    dmats = np.array([material_row(1, [e, float(F32(1) / F32(e)), 0, 0, 0, 0, 0, 0], (1, 1, 1)) for e in etas], dtype=F32)
    mi = np.array([etas.index(e) for e in eta], dtype=F32)
    sin = np.sqrt(np.maximum(0, 1 - cs * cs))
    wi = np.stack([sin * 0.6, sin * 0.8, cs], axis=1)
    refl = wi * [-1, -1, 1]
    scale = -np.where(ct64 < 0, 1 / eta, eta)
    refr = np.stack([scale * wi[:, 0], scale * wi[:, 1], ct64], axis=1)

    variants = [("reflect", refl), ("refract", refr)] + [("%s off %g" % (nm, e), rotated(v, e)) for nm, v in (("reflect", refl), ("refract", refr)) for e in (0.5e-3, 2e-3)]
    rows = np.concatenate([np.concatenate([mi[:, None], cs[:, None], wi, v], axis=1) for _, v in variants]).astype(F32)
    d = probe.run("fr_diel", dmats, rows).astype(np.float64).reshape(len(variants), len(cs), 3)
    F32o, ct32o = ob.fresnel_dielectric(32, cs, eta)
    band = np.abs(ct2) < 1e-5
    same = eta == 1
    Fd, ctd = d[0, :, 0], d[0, :, 1]
    rec = dict(nonfinite=int((~np.isfinite(d)).sum()), n=len(cs), in_band=int(band.sum()), cells={},
               band_F_in_unit=bool(np.all((Fd[band] >= 0) & (Fd[band] <= 1))),
               band_cosT_sign=bool(np.all((ctd[band] == 0) | (np.sign(ctd[band]) == -np.sign(cs[band])))),
               eta_one_exact=bool(np.all(Fd[same] == 0) and np.array_equal(ctd[same], -cs[same].astype(F32).astype(np.float64))))
    for e in etas:                             # one cell per eta and side of the critical angle's neighbourhood (cos^2 theta_t below 1e-2)
        for tag, sel in (("", (eta == e) & ~band & (np.abs(ct2) >= 1e-2)), (" near critical", (eta == e) & ~band & (np.abs(ct2) < 1e-2))):
            if sel.any():
                rec["cells"]["eta=%.6g%s" % (e, tag)] = dict(F=judge(worst(np.abs(Fd - F64), sel), worst(np.abs(F32o - F64), sel)),
                                                             cosT=judge(worst(np.abs(ctd - ct64), sel), worst(np.abs(ct32o - ct64), sel)))
    # pdf_delta: F at the reflection, 1 - F at the refraction (where there is one), 0 beyond DeltaEpsilon
    has_t = (F64 < 1) & ~band
    rec["pdf_reflect"] = bool(np.array_equal(d[0, ~band, 2], Fd[~band]))
    rec["pdf_refract"] = bool(np.array_equal(d[1, has_t, 2], (F32(1) - Fd[has_t].astype(F32)).astype(np.float64)))
    rec["pdf_far_is_zero"] = bool(np.all(d[3, :, 2] == 0) and np.all(d[5, has_t, 2] == 0))
    rec["pdf_near_nonzero_share"] = [float(np.mean(d[2, ~band, 2] > 0)), float(np.mean(d[4, has_t, 2] > 0))]
    out["dielectric"] = rec
    return out, dict(fr_cond=raw_cond, fr_diel=d)


def measure_warp(ob, probe):
    s = warp_points()
    d = probe.run("warp", [material_row(0, [0] * 8)], np.concatenate([np.zeros((len(s), 1), dtype=F32), s], axis=1)).astype(np.float64)
    want, o32 = cosine_hemisphere(s), ob.cosine_hemisphere(32, s)
    # z = sqrt(1 - r^2) loses its digits at the disk's rim: the rim is a cell of its own
    r = np.maximum(np.abs(2 * s[:, 0].astype(np.float64) - 1), np.abs(2 * s[:, 1].astype(np.float64) - 1))
    cells = {"r <= 0.9": r <= 0.9, "0.9 < r <= 0.999": (r > 0.9) & (r <= 0.999), "rim": r > 0.999}
    return dict(n=len(s), nonfinite=int((~np.isfinite(d)).sum()), z_positive=bool(np.all(d[:, 2] > 0)),
                unit_length_ulp=float(np.max(np.abs(np.linalg.norm(d, axis=1) - 1)) / EPS),
                cells={k: judge(worst(np.abs(d - want).max(axis=1), m), worst(np.abs(o32 - want).max(axis=1), m)) for k, m in cells.items()},
                oracle64_vs_numpy=worst(np.abs(ob.cosine_hemisphere(64, s) - want).max(axis=1))), d


# What csrc/device_bsdf.h states about rc_exp and rc_log, as measured on the device (the header's earlier "~2e-6" did not hold
# for rc_exp: x * log2(e) is rounded before v_exp_f32 sees it, an error of |x| * 2^-24 in the exponent, 3.8e-6 at x = -87).
SCALAR_CLAIMS = dict(rc_exp_rel=4e-6, rc_exp_rel_above_minus_10=5e-7, rc_log_rel=2e-7, rc_log_abs=2e-7)


def measure_scalar(ob, probe):
    """One run over the concatenated ranges; each routine is read on its own range. rc_exp and rc_log against numpy in fp64
    (the header's claims); erf, erfinv, sin and cos under the rule, the floor being the fp32 oracle's (libm's) own error."""
    xe = np.linspace(-87, 0, 8193).astype(F32)
    xl = np.concatenate([np.geomspace(1e-7, 1, 8192), [ONE_M, 1.0]]).astype(F32)
    xr = np.linspace(-1, 2, 6145).astype(F32)
    xf = np.concatenate([np.linspace(-6, 6, 4097), 1 / np.geomspace(1e-3, 1e3, 512)]).astype(F32)                 # erf: cot(theta) of any size
    xi = np.concatenate([np.linspace(-1, 1, 4097)[1:-1], [ONE_M, -ONE_M, 1 - 2.0 ** -23], 1 - np.geomspace(1e-7, 1e-1, 256)]).astype(F32)
    parts, at, sl = (xe, xl, xr, xf, xi), 0, []
    for p in parts:
        sl.append(slice(at, at + len(p)))
        at += len(p)
    x = np.concatenate(parts)
    d = probe.run("scalar", [material_row(0, [0] * 8)], np.stack([np.zeros_like(x), x], axis=1)).astype(np.float64)
    e, l, r, f, i = (d[s] for s in sl)
    x64 = [p.astype(np.float64) for p in parts]
    logx = np.log(x64[1])
    small = np.abs(logx) < 1
    exp_err = rel_err(e[:, 0], np.exp(x64[0]))
    out = dict(rc_exp_rel=worst(exp_err), rc_exp_rel_above_minus_10=worst(exp_err, x64[0] >= -10),
               rc_log_rel=worst(rel_err(l[:, 1], logx), ~small), rc_log_abs=worst(np.abs(l[:, 1] - logx), small))
    erf64, inv64 = ob.mts_erf(64, x64[3]), ob.mts_erf(64, x64[4], inverse=True)
    two_pi_x = (F32(2 * np.pi) * parts[2]).astype(F32)                        # what the oracle in float computes
    s64, c64 = np.sin(2 * np.pi * x64[2]), np.cos(2 * np.pi * x64[2])
    nz = x64[4] != 0
    out["mts_erf"] = judge(worst(np.abs(f[:, 2] - erf64)), worst(np.abs(ob.mts_erf(32, x64[3]) - erf64)))
    out["mts_erfinv"] = judge(worst(rel_err(i[:, 3], inv64), nz), worst(rel_err(ob.mts_erf(32, x64[4], inverse=True), inv64), nz))
    out["sin_rev"] = judge(worst(np.abs(r[:, 4] - s64)), worst(np.abs(np.sin(two_pi_x).astype(np.float64) - s64)))
    out["cos_rev"] = judge(worst(np.abs(r[:, 5] - c64)), worst(np.abs(np.cos(two_pi_x).astype(np.float64) - c64)))
    out["nonfinite"] = int((~np.isfinite(e[:, 0])).sum() + (~np.isfinite(l[:, 1])).sum() + (~np.isfinite(r[:, 4:6])).sum() + (~np.isfinite(f[:, 2])).sum() + (~np.isfinite(i[:, 3])).sum())
    import math                                                               # for the record only: the approximation against erf itself
    out["record"] = dict(mts_erf_vs_math_erf=worst(np.abs(f[:, 2] - np.array([math.erf(v) for v in x64[3]]))))
    return out, d


def clamp_is_exact(cells, raw):
    """alpha = 1e-5 gives the bits of alpha = 1e-4 (make_rc's floor) in every output of the three rough-conductor ops."""
    lo = [i for i, c in enumerate(cells) if c["alpha"] == 1e-5]
    hi = [next(j for j, b in enumerate(cells) if b["alpha"] == 1e-4 and (b["ggx"], b["mat"], b["tag"]) == (cells[i]["ggx"], cells[i]["mat"], cells[i]["tag"])) for i in lo]
    return bool(lo) and all(np.array_equal(raw[op][lo].view(np.uint32), raw[op][hi].view(np.uint32)) for op in ("rc_sample", "distr", "sa_eval"))


def findings(rep, raw, cells):
    """What the measurement holds against the device, by the test that asserts it: {test: [what, ...]}, empty lists when all is well."""
    over = lambda name, checks, keep: ["%s %s: %.3g > %.3g (floor %.3g, %.1f x the bound)" % (name, k, v["dev"], v["bound"], v["floor"], v["ratio"])
                                       for k, v in checks.items() if keep(k) and not v["ratio"] <= 1]
    ident = lambda k: k.split()[-1] in ("id_pdf", "id_eval", "reciprocity")
    rc, fr, warp, sc = rep["rough_conductor"], rep["fresnel"], rep["warp"], rep["scalar"]
    f = dict(non_finite=[], rejection=[], values=[], identities=[], clamp=[], conductor_fresnel=[], dielectric=[], pdf_delta=[], warp=[], scalar=[])
    for c in rc:
        if c["nonfinite"]:
            f["non_finite"].append("%s: %d non-finite outputs" % (c["name"], c["nonfinite"]))
        if c.get("zero_below") is False:
            f["rejection"].append("%s: non-zero weight, pdf or value from below the surface" % c["name"])
        for key, n in (("rejection_mismatch_grid", N_GRID), ("D_zero_mismatch", N_GRID + len(CORNERS) ** 2), ("eval_zero_mismatch", N_GRID + len(CORNERS) ** 2 + 257)):
            if c.get(key, 0) > 1e-3 * n:
                f["rejection"].append("%s: %s %d of %d" % (c["name"], key, c[key], n))
        f["rejection"] += ["%s: corner (%g, %g) device %s, both oracles %s" % (c["name"], q["sx"], q["sy"], q["device"], q["oracle64"])
                           for q in c["corner_rejections"] if q["device"] != q["oracle32"]]
        f["values"] += over(c["name"], c["checks"], lambda k: not ident(k))
        f["identities"] += over(c["name"], c["checks"], ident)
    if not clamp_is_exact(cells, raw):
        f["clamp"].append("alpha = 1e-5 and alpha = 1e-4 differ")
    for name, r in fr.items():
        if r["nonfinite"]:
            f["non_finite"].append("%s: %d non-finite outputs" % (name, r["nonfinite"]))
        if name == "dielectric":
            for cell, ch in r["cells"].items():
                f["dielectric"] += over(cell, ch, lambda k: True)
            f["dielectric"] += ["dielectric: %s" % k for k in ("band_F_in_unit", "band_cosT_sign", "eta_one_exact") if not r[k]]
            f["pdf_delta"] += ["dielectric: %s" % k for k in ("pdf_reflect", "pdf_refract", "pdf_far_is_zero") if not r[k]]
        else:
            f["conductor_fresnel"] += over(name, {k: v for k, v in r.items() if isinstance(v, dict)}, lambda k: True)
            f["conductor_fresnel"] += ["%s: %s" % (name, k) for k in ("in_unit", "mirror_wo", "weight_zero_at_grazing", "pdf_delta_is_one", "pdf_delta_far_is_zero") if not r[k]]
            if r["at_grazing_ulp"] > 4:
                f["conductor_fresnel"].append("%s: F(cos = 0) is %.1f ulp from 1" % (name, r["at_grazing_ulp"]))
    if warp["nonfinite"]:
        f["non_finite"].append("warp: %d non-finite outputs" % warp["nonfinite"])
    f["warp"] += over("warp", warp["cells"], lambda k: True)
    f["warp"] += ["warp: z <= 0"] * (not warp["z_positive"]) + ["warp: length %.1f ulp from 1" % warp["unit_length_ulp"]] * (warp["unit_length_ulp"] > 4)
    if sc["nonfinite"]:
        f["non_finite"].append("scalar: %d non-finite outputs" % sc["nonfinite"])
    f["scalar"] += ["%s: %.3g > %.3g" % (k, sc[k], v) for k, v in SCALAR_CLAIMS.items() if not sc[k] <= v]
    f["scalar"] += over("scalar", {k: v for k, v in sc.items() if isinstance(v, dict) and "ratio" in v}, lambda k: True)
    return f


def measure(ob, probe, cells=None, ref=None):
    sxy = sample_points()
    cells = rc_cells() if cells is None else cells
    ref = rc_reference(ob, cells, sxy) if ref is None else ref
    rc, raw = measure_rc(ob, probe, cells, sxy, ref, hemisphere_dirs())
    fr, raw_fr = measure_fresnel(ob, probe)
    warp, raw_warp = measure_warp(ob, probe)
    scalar, raw_scalar = measure_scalar(ob, probe)
    raw.update(raw_fr, warp=raw_warp, scalar=raw_scalar)
    return dict(rough_conductor=rc, fresnel=fr, warp=warp, scalar=scalar, runs=probe.runs), raw


def builds_differ(a, b):
    """Per op, how many output elements differ between the two builds and by how much."""
    out = {}
    for k in a:
        x, y = a[k].astype(np.float64).ravel(), b[k].astype(np.float64).ravel()
        ne = (x != y) & ~(np.isnan(x) & np.isnan(y))
        with np.errstate(invalid="ignore"):
            gap = np.abs(x - y)
        out[k] = dict(elements=int(ne.sum()), of=int(x.size), max_abs=float(np.max(gap[ne & np.isfinite(gap)], initial=0.0)))
    return out


def summary(reports, diff):
    """What profiles/r10_bsdf_probe.json holds. Per cell and quantity the larger of the two builds' ratios (device error over the
    rule's bound), as rows of one table; per build the worst ratio of each quantity, the Fresnel, warp and scalar records."""
    units = list(reports)
    cells = [c for c in reports[units[0]]["rough_conductor"] if c["checks"]]
    keys = sorted({k for c in cells for k in c["checks"]})
    by_name = {u: {c["name"]: c for c in reports[u]["rough_conductor"]} for u in units}
    ratio = lambda c, k: max(by_name[u][c["name"]]["checks"][k]["ratio"] for u in units) if k in c["checks"] else None
    floors = {k: [float("%.3g" % f(c["checks"][k]["floor"] for c in cells if k in c["checks"])) for f in (min, max)] for k in keys}
    out = {"rule": "|device - oracle64| <= %g * max|oracle32 - oracle64| + 4 ulp; ratio = device error / that bound, <= 1 passes" % FACTOR,
           "builds_differ": diff, "quantities": keys, "floor_min_max": floors,
           "cells": {c["name"]: [None if ratio(c, k) is None else round(ratio(c, k), 3) for k in keys] for c in cells}}
    for u in units:
        rep = reports[u]
        worst_of = {k: max((c["checks"][k]["ratio"], c["name"]) for c in rep["rough_conductor"] if k in c["checks"]) for k in keys}
        out[u] = dict(worst_ratio={k: [round(v[0], 4), v[1]] for k, v in worst_of.items()},
                      corner_rejections={c["name"]: [[q["sx"], q["sy"]] for q in c["corner_rejections"]] for c in rep["rough_conductor"] if c["corner_rejections"]},
                      nonfinite=sum(c["nonfinite"] for c in rep["rough_conductor"]), rejection_mismatch_grid=sum(c.get("rejection_mismatch_grid", 0) for c in rep["rough_conductor"]),
                      fresnel=rep["fresnel"], warp=rep["warp"], scalar=rep["scalar"], runs=rep["runs"])
    return out


def write_summary(path, s):
    """One line per top-level entry and per cell: the file stays readable in a diff."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in s.items():
            if k == "cells":
                f.write(' "cells": {\n' + ",\n".join("  %s: %s" % (json.dumps(n), line(r)) for n, r in v.items()) + "\n },\n")
            elif k != list(s)[-1]:
                f.write(" %s: %s,\n" % (json.dumps(k), line(v)))
            else:
                f.write(" %s: %s\n}\n" % (json.dumps(k), line(v)))
