"""Helper of tests/test_light_probe.py and tests/test_gpu_lights.py: builds and runs tests/native/light_probe.hip over the tables
csrc/scene_prep.h makes for a scene (written by tests/native/scene_prep_harness.cpp), lays out the inputs, computes the
references -- Scene<F> of the oracle in float and in double (oracle_light_probe) and independent fp64 closed forms in numpy --
and measures the device against them under the rule of tests/bsdf_probe.py, per quantity and per cell:

    |device - oracle64| <= 32 * max |oracle32 - oracle64| + 4 ulp

Identities on the device's own output are held to the residual the fp32 oracle's own output leaves, under the same rule.

The branch band. Cone or area sampling of a sphere is chosen by sinAlpha < 1 - Epsilon, and Epsilon is 1e-4 in Mitsuba's single
precision build and 1e-7 in its double precision build. For 1 - 1e-4 < sinAlpha < 1 - 1e-7 the two oracles sample different
distributions, so the cells of that band (two inside it, and the cells at 1 - (1e-4 -+ 2e-5)) are judged against the fp32
oracle only: its choice of branch is the device's, and the fp64 side of the rule is the closed form, in numpy, of the
distribution the fp32 oracle samples there (sphere_area_sample / cone_density below, which tests/test_light_probe.py holds
against the fp64 oracle to 1e-12 outside the band).
"""
import json
import os
import struct
import subprocess

import numpy as np

import bsdf_probe as bp
from bsdf_probe import EPS, F32, FACTOR, judge, rel_err

ROOT = bp.ROOT
SRC = os.path.join(ROOT, "tests", "native", "light_probe.hip")
HARNESS = os.path.join(ROOT, "tests", "native", "scene_prep_harness.cpp")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
UNITS = bp.UNITS
OPS = dict(sphere=0, env=1, light=2, pdf_area=3)
NIN = dict(sphere=6, env=9, light=15, pdf_area=13)
NOUT = dict(sphere=9, env=7, light=7, pdf_area=1)
RUNS = 4                                       # child runs per build
CAP = 1e-3                                     # share of a cell's grid on which a zero pattern may differ (tests/test_gpu_bsdf.py's)
EPSILON_F = float(F32(1e-4))                   # Mitsuba's single precision Epsilon, as the device has it
SHADE = np.dtype([("origin", "<f4", 3), ("eu", "<f4", 3), ("ev", "<f4", 3), ("n", "<f4", 3), ("inv_len_eu", "<f4"), ("bsdf", "<i4"), ("emitter", "<i4"), ("inv_area", "<f4")])
EMITTER = np.dtype([("radiance", "<f4", 3), ("prim", "<i4"), ("cdf_lo", "<f4"), ("cdf_hi", "<f4"), ("pad", "<f4", 2)])


def build(out_dir, unit):
    return bp.build(out_dir, unit, SRC)


# ------------------------------------------------------------------ the tables the library would upload
def harness(out_dir):
    exe = os.path.join(str(out_dir), "scene_prep_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", bp.CSRC, "-I", HOST, "-o", exe, HARNESS], check=True)
    return exe


def tables(pkg, exe, sd, work_dir):
    """prepare_scene's DShade, DBsdf and DEmitter tables for one scene: their bytes, and a view of the first and the last."""
    scene, blob = os.path.join(str(work_dir), sd.name + ".drmlt"), os.path.join(str(work_dir), sd.name + ".tables")
    sd.save(scene)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1)
    args = ["%s=%s" % (name, ("%.9g" if isinstance(getattr(cfg, name), float) else "%d") % getattr(cfg, name))
            for name, _ in cfg._fields_ if name not in ("struct_size", "reserved")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}
    r = subprocess.run([exe, "scene=" + scene, "tables=" + blob, *args], check=True, capture_output=True, text=True, env=env)
    out = json.loads(r.stdout)
    assert out["refusal"] == "", out["refusal"]
    raw, at, part = open(blob, "rb").read(), 0, {}
    for name, n in out["tables"]:
        part[name] = raw[at:at + n]
        at += n
    t = dict(n_shade=len(part["shade"]) // 64, n_bsdfs=len(part["bsdfs"]) // 48, n_emitters=len(part["emitters"]) // 32,
             bytes=part["shade"] + part["bsdfs"] + part["emitters"], shade=np.frombuffer(part["shade"], dtype=SHADE),
             emitters=np.frombuffer(part["emitters"], dtype=EMITTER))
    assert t["n_shade"] == out["params"]["n_shade"] and t["n_emitters"] == out["params"]["n_emitters"] and SHADE.itemsize == 64 and EMITTER.itemsize == 32
    return t


class Probe(bp.Probe):
    """bsdf_probe.Probe over light_probe's request format; `dead` is the base class's, so one fault ends all probe runs."""

    def run(self, op, t, rows):
        if bp.Probe.dead:
            raise bp.ProbeDied(bp.Probe.dead)
        rows = np.ascontiguousarray(rows, dtype=F32)
        assert rows.ndim == 2 and rows.shape[1] == NIN[op], rows.shape
        assert np.all((rows[:, 0] >= 0) & (rows[:, 0] < (t["n_bsdfs"] if op == "light" else t["n_emitters"])))
        req, res = os.path.join(self.dir, op + ".req"), os.path.join(self.dir, op + ".res")
        with open(req, "wb") as f:
            f.write(struct.pack("<8i", OPS[op], len(rows), t["n_shade"], t["n_bsdfs"], t["n_emitters"], 0, 0, 0))
            f.write(t["bytes"])
            f.write(rows.tobytes())
        self.runs += 1
        try:
            r = subprocess.run(["timeout", "-k", "10", "60", self.exe, req, res], capture_output=True, text=True, timeout=80)
        except subprocess.TimeoutExpired:
            bp.Probe.dead = "%s %s: no answer within 80 s" % (os.path.basename(self.exe), op)
            raise bp.ProbeDied(bp.Probe.dead)
        if r.returncode != 0:
            bp.Probe.dead = "%s %s: exit status %d: %s" % (os.path.basename(self.exe), op, r.returncode, r.stderr[-500:])
            raise bp.ProbeDied(bp.Probe.dead)
        out = np.fromfile(res, dtype=F32)
        os.remove(req), os.remove(res)
        return out.reshape(len(rows), NOUT[op]).astype(np.float64)


# ------------------------------------------------------------------ inputs
def sample_points():
    """bsdf_probe's 64 x 64 grid and 36 corner pairs, and sx = 1.0 exactly with every corner sy: (4138, 2) float32."""
    one = np.array([(1.0, c) for c in bp.CORNERS], dtype=F32)
    return np.concatenate([bp.sample_points(), one]).astype(F32)


N_GRID = bp.N_GRID
GROUPS = bp.GROUPS


def _camera(pkg, sd):
    sd.set_camera(pkg.scenes.lookat((0.0, -3.0, 0.5), (0.0, 0.0, 0.5), (0.0, 0.0, 1.0)), 40.0, 16, 16)
    return sd


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


SPHERES = (((0.3, -0.2, 0.5), 0.25), ((-0.4, 0.7, 0.2), 0.06))     # (centre, radius); 0.06 is caustic_c5's light
DIRS = [("+x", (1, 0, 0)), ("-x", (-1, 0, 0)), ("+y", (0, 1, 0)), ("-y", (0, -1, 0)), ("+z", (0, 0, 1)), ("-z", (0, 0, -1)),
        ("generic", _unit((0.3, -0.5, 0.81))), ("111", _unit((1, 1, 1))), ("1-1.5", (1 / 1.5, -1 / 1.5, 0.5 / 1.5))]
SIN_ALPHA = (1e-3, 1e-2, 0.03, 0.1, 0.5, 0.9, 0.99, 1 - 1e-3)
INSIDE = (0.0, 0.5, 0.999)                                          # D / r
BAND = (1 - 1.2e-4, 1 - 8e-5, 1 - 3e-5, 1 - 3e-6)                   # sinAlpha: 1 - (1e-4 +- 2e-5), and two inside the band


def sphere_scene(pkg):
    sd = pkg.scenes.SceneData("light_probe_spheres")
    grey = sd.diffuse(0.5)
    for c, r in SPHERES:
        sd.sphere(c, r, grey, radiance=(1.0, 1.0, 1.0))
    return _camera(pkg, sd)


def sphere_cells():
    """kind "cone": both oracles sample the cone; "area": both the area; "band": judged against the fp32 oracle (the docstring)."""
    cells = []
    for e, (c, r) in enumerate(SPHERES):
        c = np.array(c, dtype=F32).astype(np.float64)
        add = lambda kind, tag, dn, v, D: cells.append(dict(name="r=%g %s %s" % (r, tag, dn), emitter=e, kind=kind, ref=(c + np.asarray(v, dtype=np.float64) * D).astype(F32)))
        for dn, v in DIRS:
            for s in SIN_ALPHA:
                add("cone", "sin=%.9g" % s, dn, v, float(F32(r)) / s)
            for s in BAND:
                if dn in ("generic", "+x"):
                    add("band" if s > 1 - 1e-4 else "cone", "sin=1-%.3g" % (1 - s), dn, v, float(F32(r)) / s)
            for k in INSIDE:
                if k > 0 or dn == "+x":
                    add("area", "D/r=%g" % k, dn, v, float(F32(r)) * k)
    for cell in cells:     # refN: towards the centre (the direction of every cone sample's hemisphere)
        c = np.array(SPHERES[cell["emitter"]][0], dtype=F32).astype(np.float64)
        v = c - cell["ref"].astype(np.float64)
        cell["ref_n"] = (v / np.linalg.norm(v) if np.any(v != 0) else np.array([0.0, 0.0, 1.0])).astype(F32)
    return cells


ENV_AT = (0.0, 0.5, 0.999, 1.0, 1.001)                              # |ref - centre| / R
NORMALS = DIRS[:7] + [("nx=ny", _unit((1, 1, 1))), ("nx=-ny", _unit((0.6, -0.6, 0.5)))]
RAY_ORIGINS = [(0, 0, 0), (3, 0, 0), (0, -0.25, 0), (0, 0, 1e-6), (1e-5, 1e-5, -1e-5), (0.3, -0.2, 0.5), (-400, 20, 1), (1e-4, 0, 0), (0.999e-4, 0, 0)]

WEIGHTS = (0.0, 1.0, 0.7, 0.0, 2.5, 0.4, 0.0)                        # rectangle, rectangle, sphere, point, point, sky, triangle
CENTRES = ((1.5, 0.0, 1.5), (-1.5, 0.0, 1.5), (0.0, 1.5, 1.5), (0.0, -1.5, 1.5), (1.2, -1.2, 1.5), None, (-1.2, 1.2, 1.5))
SKY = 5
REFL = bp.REFL


def _facing_frame(centre, half):
    """Columns eu, ev, n and the centre of a rectangle at `centre` whose normal points at the origin."""
    n = -_unit(centre)
    eu = _unit(np.cross((0.0, 1.0, 0.0), n) if abs(n[1]) < 0.9 else np.cross((1.0, 0.0, 0.0), n))
    ev = np.cross(n, eu)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = eu * half, ev * half, n, centre
    return m


def light_scene(pkg):
    """Seven emitters in disjoint cones seen from the origin, all above z = 0 and facing it, three of them with weight 0."""
    sd = pkg.scenes.SceneData("light_probe_pick")
    sd.diffuse(*REFL)
    eta, k = bp.COPPER
    sd.roughconductor(0.1, eta, k, ggx=False, reflectance=REFL)
    sd.rectangle(_facing_frame(CENTRES[0], 0.3), 0, radiance=(3.0, 2.0, 1.0))
    sd.rectangle(_facing_frame(CENTRES[1], 0.3), 0, radiance=(1.0, 2.0, 3.0))
    sd.sphere(CENTRES[2], 0.25, 0, radiance=(2.0, 2.5, 1.5))
    sd.point_light(CENTRES[3], intensity=(1.0, 1.0, 1.0), sampling_weight=0.0)
    sd.point_light(CENTRES[4], intensity=(4.0, 3.2, 2.0), sampling_weight=2.5)
    sd.constant_environment((0.9, 1.0, 1.2), sampling_weight=0.4)
    m = _facing_frame(CENTRES[6], 0.3)
    corner = lambda a, b: m[:3, 3] + a * m[:3, 0] + b * m[:3, 1]
    sd.triangle(corner(-1, -1), corner(-1, 1), corner(1, -1), 0, radiance=(1.0, 1.0, 1.0))   # eu x ev = n: it faces the origin
    for e, w in zip(sd.emitters, WEIGHTS):
        e.sampling_weight = w
    return _camera(pkg, sd)


def name_emitter(d, dist, sky_from):
    """The emitter a sample from the origin went to, from its direction and distance alone: -1 where that names none."""
    d, dist = np.asarray(d, dtype=np.float64), np.asarray(dist, dtype=np.float64)
    out = np.full(len(d), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for i, c in enumerate(CENTRES):
            if c is not None:
                out[(d @ _unit(c) > 0.97) & (dist < sky_from)] = i   # the cones' axes are 32 degrees apart or more, cos 14 degrees = 0.97
        out[dist >= sky_from] = SKY
    return out


def light_cells(t):
    """(name, bsdf, receiver normal n, tangent s) and the sx, sy rows shared by the cells. sx: 0, 1 - 2^-24, every entry of the
    uploaded CDF with its two float neighbours, and the midpoints of 1024 strata; sy: the midpoints of 16 strata."""
    em = t["emitters"]
    cdf = np.unique(np.concatenate([em["cdf_lo"], em["cdf_hi"]]))
    edges = np.unique(np.clip(np.concatenate([np.nextafter(cdf, F32(-1)), cdf, np.nextafter(cdf, F32(2))]), 0, 1).astype(F32))
    sx = np.concatenate([edges, [F32(bp.ONE_M)], (np.arange(1024, dtype=F32) + F32(0.5)) / F32(1024)]).astype(F32)
    sy = (np.arange(16, dtype=F32) + F32(0.5)) / F32(16)
    sxy = np.stack(np.meshgrid(sx, sy, indexing="ij"), axis=-1).reshape(-1, 2)
    edge = np.min(np.abs(sxy[:, 0:1].astype(np.float64) - cdf[None, :].astype(np.float64)), axis=1) <= 2.0 ** -24   # within one ulp of a CDF entry
    # the receiver whose horizon cuts rectangle 1 in half: its normal is perpendicular to the rectangle's centre
    nh = _unit(np.cross(CENTRES[1], (0.0, 1.0, 0.0)))
    nh = nh if nh[2] > 0 else -nh
    cells = [("diffuse", 0, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), ("copper", 1, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)), ("diffuse, horizon through rectangle 1", 0, nh, (0.0, 1.0, 0.0))]
    return [dict(name=n, bsdf=b, n=np.array(nn, dtype=F32), s=np.array(s, dtype=F32)) for n, b, nn, s in cells], sxy.astype(F32), edge


# ------------------------------------------------------------------ independent fp64 closed forms (numpy)
def cone_density(c, r, ref):
    """1 / (2 pi (1 - cos alpha)) with 1 - cos alpha = sin^2 alpha / (1 + cos alpha): no cancellation at small solid angles."""
    v = np.asarray(c, dtype=np.float64) - np.asarray(ref, dtype=np.float64)
    sin2 = r * r / np.sum(v * v, axis=-1)
    return (1 + np.sqrt(1 - sin2)) / (2 * np.pi * sin2)


def flat_density(dist, area, cos):
    return dist * dist / (area * np.abs(cos))


def sphere_area_sample(c, r, ref, sxy):
    """Uniform on the sphere's area, seen from ref (sphere.cpp:257-268 and :340-353) -> d, dist, n, pdf in fp64."""
    s = np.asarray(sxy, dtype=np.float64)
    z = 1 - 2 * s[:, 1]
    rad = np.sqrt(np.maximum(0.0, 1 - z * z))
    n = np.stack([rad * np.cos(2 * np.pi * s[:, 0]), rad * np.sin(2 * np.pi * s[:, 0]), z], axis=1)
    dv = np.asarray(c, dtype=np.float64) + n * r - np.asarray(ref, dtype=np.float64)
    dist = np.linalg.norm(dv, axis=1)
    d = dv / dist[:, None]
    return dict(d=d, dist=dist, n=n, pdf=flat_density(dist, 4 * np.pi * r * r, np.sum(d * n, axis=1)))


def ray_eps(o):
    """skdtree.cpp:125-129 and :213-218 in fp64 with the single precision Epsilon -> (closest, shadow)."""
    m = np.max(np.abs(np.asarray(o, dtype=np.float64)), axis=1)
    return EPSILON_F * np.maximum(m, EPSILON_F), EPSILON_F * m


# ------------------------------------------------------------------ references
def _oracle(ob, sd, prec, emitters, **kw):
    """ob.light_probe over rows with a forced emitter each: one call per emitter, scattered back."""
    out = None
    for e in np.unique(emitters):
        sel = emitters == e
        r = ob.light_probe(prec, sd, emitter=int(e), **{k: v[sel] for k, v in kw.items()})
        if out is None:
            out = {k: np.zeros((len(emitters),) + v.shape[1:]) for k, v in r.items() if k in ("d", "dist", "n", "pdf", "pdf_direct", "pdf_area", "p", "value")}
        for k in out:
            out[k][sel] = r[k]
    return out


def _round(a):
    return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def _geometry_term(ref, p, n):
    """dist^2 / |d . n| of the segment ref -> p in fp64, and d . n."""
    dv = p - ref
    d2 = np.sum(dv * dv, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        dn = np.sum(dv * n, axis=1) / np.sqrt(d2)
        return d2 / np.abs(dn), dn


def sphere_reference(ob, sd, cells, sxy):
    """Per row of (cell, sample): both oracles' samples, the fp64 side R of the rule (the fp64 oracle; in the band the closed
    form of what the fp32 oracle samples), and the fp32 oracle's density of its own sample under the area measure."""
    ns = len(sxy)
    em = np.repeat([c["emitter"] for c in cells], ns)
    ref = np.repeat(np.stack([c["ref"] for c in cells]).astype(np.float64), ns, axis=0)
    refn = np.repeat(np.stack([c["ref_n"] for c in cells]).astype(np.float64), ns, axis=0)
    s = np.tile(sxy.astype(np.float64), (len(cells), 1))
    o = {p: _oracle(ob, sd, p, em, ref=ref, ref_n=refn, sxy=s) for p in (64, 32)}
    R = {k: v.copy() for k, v in o[64].items()}
    band = np.repeat([c["kind"] == "band" for c in cells], ns)
    for e, (c, r) in enumerate(SPHERES):
        sel = band & (em == e)
        if sel.any():
            a = sphere_area_sample(_round(c), float(F32(r)), ref[sel], s[sel])
            for k in ("d", "dist", "n", "pdf"):
                R[k][sel] = a[k]
            R["pdf_direct"][sel] = a["pdf"]
    p32, n32 = _round(o[32]["p"]), _round(o[32]["n"])
    own = _oracle(ob, sd, 32, em, ref=ref, ref_n=refn, point=p32, point_n=n32)
    return dict(ns=ns, sxy=sxy, em=em, ref=ref, refn=refn, s=s, o64=o[64], o32=o[32], R=R, band=band, own32_pdf_area=own["pdf_area"], own32_g=_geometry_term(ref, p32, n32)[0], own32_dn=_geometry_term(ref, p32, n32)[1])


def _sphere_identities(x, ref, c, r, cos_alpha):
    """Residuals of one output set (d, dist, n): |d| = 1, ref + d dist on the sphere, n = (p - c) / r, d inside the cone."""
    d, dist, n = x["d"], x["dist"], x["n"]
    p = ref + d * dist[:, None]
    fn = c - ref
    with np.errstate(divide="ignore", invalid="ignore"):
        fn = fn / np.linalg.norm(fn, axis=1)[:, None]
        return dict(id_unit=np.abs(np.linalg.norm(d, axis=1) - 1), id_on_sphere=np.abs(np.linalg.norm(p - c, axis=1) - r) / r,
                    id_normal=np.abs(n - (p - c) / r[:, None]).max(axis=1), id_cone=np.where(cos_alpha > -1.5, np.maximum(0.0, cos_alpha - np.sum(d * fn, axis=1)), 0.0))


def _per_cell(err, mask, ncell, part):
    """Worst err over the rows of `part` of every cell; a NaN under the mask stays a NaN."""
    return np.where(mask, err, 0.0).reshape(ncell, -1)[:, part].max(axis=1)


def sphere_groups(sxy):
    """The grid, the corner pairs short of the cone's rim, and the rim (sx = 1 - 2^-24 and sx = 1), as row indices of a cell."""
    rim = sxy[:, 0] >= F32(bp.ONE_M)
    idx = np.arange(len(sxy))
    return (("", idx[:N_GRID]), ("corners ", idx[N_GRID:][~rim[N_GRID:]]), ("rim ", idx[rim]))


# The explained class (tests/test_gpu_lights.py has the account): (cell, quantity) pairs in which the device exceeds the rule's
# per-cell bound because the quantity is ONE amplified rounding error there, of which the cell's own |oracle32 - oracle64| is a
# single draw -- the cone's density near sinAlpha = 1, where 1 - sqrt(1 - sin^2) amplifies by up to 1 / (1 - sin^2), and on the
# rim everything behind the quadratic, whose discriminant is zero there (a rounding error e moves the intersection by sqrt(e), or
# by nothing when its sign sends the code to the fallback). The rule stays per cell for every pair; these pairs, and no others,
# are asserted instead against the floor of the same cone seen from all directions whose frame is not a tie (|n.x| == |n.y|,
# where the two oracles may take different frames), the two densities under the area measure in units of the cosine |d.n|, which
# is what divides them and goes through zero on the rim.
EXPLAINED = frozenset([
    ('r=0.06 sin=0.1 +x', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 +y', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 +z', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 -x', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 -y', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 -z', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 1-1.5', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 111', 'rim id_pdf_area'),
    ('r=0.06 sin=0.1 generic', 'rim id_pdf_area'),
    ('r=0.06 sin=0.5 +z', 'rim pdf_area'),
    ('r=0.06 sin=0.5 111', 'rim id_pdf_area'),
    ('r=0.06 sin=0.999 generic', 'rim dist'),
    ('r=0.06 sin=0.999 generic', 'rim id_on_sphere'),
    ('r=0.06 sin=0.999 generic', 'rim n'),
    ('r=0.06 sin=1-0.00012 +x', 'corners pdf'),
    ('r=0.06 sin=1-0.00012 +x', 'corners pdf_area'),
    ('r=0.06 sin=1-0.00012 +x', 'corners pdf_direct'),
    ('r=0.06 sin=1-0.00012 +x', 'pdf'),
    ('r=0.06 sin=1-0.00012 +x', 'pdf_direct'),
    ('r=0.06 sin=1-0.00012 +x', 'rim d'),
    ('r=0.06 sin=1-0.00012 +x', 'rim id_cone'),
    ('r=0.06 sin=1-0.00012 +x', 'rim pdf'),
    ('r=0.06 sin=1-0.00012 +x', 'rim pdf_direct'),
    ('r=0.06 sin=1-0.00012 generic', 'rim pdf_area'),
    ('r=0.25 sin=0.1 +x', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 +y', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 +z', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 -x', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 -y', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 -z', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 1-1.5', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 111', 'rim id_pdf_area'),
    ('r=0.25 sin=0.1 generic', 'rim id_pdf_area'),
    ('r=0.25 sin=0.5 111', 'rim id_pdf_area'),
    ('r=0.25 sin=0.9 +x', 'rim id_pdf_area'),
    ('r=0.25 sin=0.99 +x', 'rim id_on_sphere'),
    ('r=0.25 sin=0.99 +z', 'rim id_on_sphere'),
    ('r=0.25 sin=0.99 -y', 'rim id_on_sphere'),
    ('r=0.25 sin=0.99 -z', 'rim id_on_sphere'),
    ('r=0.25 sin=0.99 111', 'rim id_pdf_area'),
    ('r=0.25 sin=0.999 +x', 'rim dist'),
    ('r=0.25 sin=0.999 +x', 'rim id_on_sphere'),
    ('r=0.25 sin=0.999 +x', 'rim n'),
    ('r=0.25 sin=0.999 +z', 'rim dist'),
    ('r=0.25 sin=0.999 +z', 'rim id_on_sphere'),
    ('r=0.25 sin=0.999 +z', 'rim n'),
    ('r=0.25 sin=0.999 -y', 'rim dist'),
    ('r=0.25 sin=0.999 -y', 'rim id_on_sphere'),
    ('r=0.25 sin=0.999 -y', 'rim n'),
])
TIES = ("111", "1-1.5")


def _checks(ncell, quantities, groups=GROUPS, classes=None):
    """quantities: {name: (device error, floor error, mask)} per row -> per cell {tag + name: judge()} for every group.
    classes: None for the rule as it stands; else per cell (class id, whether the cell lends its floor to the class), and the
    floor is the class's (the assertion of the EXPLAINED pairs)."""
    out = [dict() for _ in range(ncell)]
    for tag, part in groups:
        for q, (dev, floor, mask) in quantities.items():
            dv, fl = _per_cell(dev, mask, ncell, part), _per_cell(floor, mask, ncell, part)
            if classes is not None:
                pool = {}
                for (cid, lends), f in zip(classes, fl):
                    if lends:
                        pool[cid] = max(pool.get(cid, 0.0), f)
                fl = np.array([max(f, pool.get(cid, 0.0)) for (cid, _), f in zip(classes, fl)])
            for i in range(ncell):
                out[i][tag + q] = judge(float(dv[i]), float(fl[i]))
    return out


def sphere_classes(cells):
    """(sphere and sinAlpha, lends its floor) per cell; cells that sample the area are classes of their own."""
    return [((c["emitter"], c["name"].split()[1]) if c["kind"] == "cone" else i, c["name"].split()[-1] not in TIES) for i, c in enumerate(cells)]


def sphere_floors(cells, ref):
    """What the two oracles alone say about every cell: {quantity: floor} per cell and group, the rows where either is not finite."""
    R, A = ref["R"], ref["o32"]
    fin = np.all([np.all(np.isfinite(x[k].reshape(len(x[k]), -1)), axis=1) for x in (R, A) for k in ("d", "dist", "n", "pdf", "pdf_direct")], axis=0)
    q = dict(d=(np.abs(A["d"] - R["d"]).max(axis=1),) * 2 + (fin,), dist=(rel_err(A["dist"], R["dist"]),) * 2 + (fin,),
             n=(np.abs(A["n"] - R["n"]).max(axis=1),) * 2 + (fin,), pdf=(rel_err(A["pdf"], R["pdf"]),) * 2 + (fin,))
    return _checks(len(cells), q, sphere_groups(ref["sxy"])), fin


# ------------------------------------------------------------------ the measurement (GPU)
def measure_spheres(ob, probe, t, sd, cells, sxy, ref):
    """The sphere run and the pdf_area run over every sphere cell -> per-cell records, the raw output."""
    ns, ncell, em = ref["ns"], len(cells), ref["em"]
    rows = np.concatenate([em[:, None], ref["ref"], ref["s"]], axis=1)
    dev = probe.run("sphere", t, rows)
    D = dict(d=dev[:, 0:3], dist=dev[:, 3], n=dev[:, 4:7], pdf=dev[:, 7], pdf_direct=dev[:, 8])
    R, A = ref["R"], ref["o32"]
    _, fin = sphere_floors(cells, ref)
    # the density under the area measure of the device's own sample: the point and its normal as float32, the same for all three
    c = np.stack([_round(SPHERES[e][0]) for e in em])
    r = np.array([float(F32(SPHERES[e][1])) for e in em])
    sp, sn = _round(c + D["n"] * r[:, None]), D["n"]                      # the point of the sphere that has the sampled normal
    pa = probe.run("pdf_area", t, np.concatenate([em[:, None], ref["ref"], ref["refn"], sp, sn], axis=1))[:, 0]
    ok_in = np.all(np.isfinite(sp), axis=1) & np.all(np.isfinite(sn), axis=1)
    safe = lambda a: np.where(ok_in[(...,) + (None,) * (a.ndim - 1)], a, 0.5)
    m64, m32 = (_oracle(ob, sd, p, em, ref=ref["ref"], ref_n=ref["refn"], point=safe(sp), point_n=safe(sn))["pdf_area"] for p in (64, 32))
    g, dn = _geometry_term(ref["ref"], sp, sn)
    with np.errstate(invalid="ignore"):
        facing = (np.sum((sp - ref["ref"]) * ref["refn"], axis=1) >= 0) & (dn < 0)
    em_pdf = (t["emitters"]["cdf_hi"].astype(np.float64) - t["emitters"]["cdf_lo"].astype(np.float64))[em]
    area = 4 * np.pi * np.array([float(F32(r)) ** 2 for _, r in SPHERES])[em]
    m64 = np.where(ref["band"], np.where(facing, em_pdf / area, 0.0), m64)
    lit = ok_in & fin & (pa > 0) & (m64 > 0) & (m32 > 0)
    v = c - ref["ref"]
    with np.errstate(divide="ignore", invalid="ignore"):
        sin2 = r * r / np.sum(v * v, axis=1)
    cone = np.repeat([cl["kind"] == "cone" for cl in cells], ns)
    cos_alpha = np.where(cone, np.sqrt(np.maximum(0.0, 1 - np.where(cone, sin2, 0.0))), -2.0)   # no cone outside the cone cells
    with np.errstate(invalid="ignore"):
        cos_scale = np.where(cone & np.isfinite(dn), np.abs(dn), 1.0)      # for the EXPLAINED pairs alone
    idD, idA = _sphere_identities(D, ref["ref"], c, r, cos_alpha), _sphere_identities(A, ref["ref"], c, r, cos_alpha)
    q = dict(d=(np.abs(D["d"] - R["d"]).max(axis=1), np.abs(A["d"] - R["d"]).max(axis=1), fin), dist=(rel_err(D["dist"], R["dist"]), rel_err(A["dist"], R["dist"]), fin),
             n=(np.abs(D["n"] - R["n"]).max(axis=1), np.abs(A["n"] - R["n"]).max(axis=1), fin), pdf=(rel_err(D["pdf"], R["pdf"]), rel_err(A["pdf"], R["pdf"]), fin),
             pdf_direct=(rel_err(D["pdf_direct"], R["pdf_direct"]), rel_err(A["pdf_direct"], R["pdf_direct"]), fin),
             pdf_area=(rel_err(pa, m64), rel_err(m32, m64), lit))
    for k in idD:
        q[k] = (idD[k], idA[k], fin)
    q["id_pdf_direct"] = (rel_err(D["pdf_direct"], D["pdf"]), rel_err(A["pdf_direct"], A["pdf"]), fin)
    own_lit = (ref["own32_pdf_area"] > 0) & fin
    with np.errstate(invalid="ignore"):   # the third copy: pdf_area dist^2 / |d.n| / emPdf = pdf
        own_id = np.where(own_lit, rel_err(ref["own32_pdf_area"] * ref["own32_g"] / em_pdf, A["pdf"]), 0.0)
        q["id_pdf_area"] = (rel_err(pa * g / em_pdf, D["pdf"]), own_id, lit & own_lit)
        alt = dict(q, pdf_area=(q["pdf_area"][0] * cos_scale, q["pdf_area"][1] * cos_scale, lit),
                   id_pdf_area=(q["id_pdf_area"][0] * np.abs(dn), own_id * np.abs(ref["own32_dn"]), lit & own_lit))
    checks = _checks(ncell, q, sphere_groups(sxy))
    pooled = _checks(ncell, alt, sphere_groups(sxy), sphere_classes(cells))
    bad = fin[:, None] & ~np.isfinite(np.concatenate([dev, pa[:, None]], axis=1))
    zero = fin & ok_in & ((pa > 0) != (m64 > 0))
    rim = sxy[:, 0] >= F32(bp.ONE_M)                                       # there d . n is zero but for rounding: its sign is not judged
    recs = []
    for i, cl in enumerate(cells):
        sl = slice(i * ns, (i + 1) * ns)
        recs.append(dict(name=cl["name"], kind=cl["kind"], checks=checks[i], over={k: pooled[i][k] for k, v in checks[i].items() if not v["ratio"] <= 1}, nonfinite=int(bad[sl].sum()), pdf_area_zero_mismatch_grid=int(zero[sl][:N_GRID].sum()),
                         corner_zero_mismatch=[[float(sxy[j, 0]), float(sxy[j, 1])] for j in np.nonzero(zero[sl])[0] if j >= N_GRID and not rim[j] and (pa[sl][j] > 0) != (m32[sl][j] > 0)]))
    return recs, dict(sphere=dev, pdf_area=pa[:, None])


def env_inputs(t):
    """Cells (position in units of R) x (normal), the environment's centre and radius as uploaded, and the ray origins."""
    L = t["shade"][t["emitters"]["prim"][SKY]]
    assert (L["bsdf"] >> 24) == 5
    c, R = L["origin"].astype(np.float64), float(L["eu"][0])
    off = _unit((0.5, -0.3, 0.81))
    cells = [dict(name="|ref-c|=%gR n=%s" % (k, nn), at=k, ref=(c + off * (R * k)).astype(F32), n=np.asarray(n, dtype=np.float64).astype(F32)) for k in ENV_AT for nn, n in NORMALS]
    return cells, c, R


def env_reference(ob, sd, cells, sxy):
    ns = len(sxy)
    ref = np.repeat(np.stack([c["ref"] for c in cells]).astype(np.float64), ns, axis=0)
    n = np.repeat(np.stack([c["n"] for c in cells]).astype(np.float64), ns, axis=0)
    s = np.tile(sxy.astype(np.float64), (len(cells), 1))
    o = {p: ob.light_probe(p, sd, ref, n, sxy=s, emitter=SKY) for p in (64, 32)}
    return dict(ns=ns, ref=ref, n=n, s=s, o64=o[64], o32=o[32])


def _on_bsphere(x, ref, c, R):
    return np.abs(np.linalg.norm(ref + x["d"] * x["dist"][:, None] - c, axis=1) - R) / R


def env_quantities(cells, ref, c_dev, R_dev, D):
    """{quantity: (device error, floor, mask)} per row; D = None: the floors alone (the fp32 oracle in the device's place)."""
    o64, o32, ns = ref["o64"], ref["o32"], ref["ns"]
    at = np.repeat([c["at"] for c in cells], ns)
    X = o32 if D is None else D
    inside = (o64["pdf"] > 0) & (o32["pdf"] > 0) & (X["pdf"] > 0)
    # d and the pdf do not depend on the position: their reference is the cell of the same normal at the centre, wherever the pdf
    # is above 0 -- on the sphere (1.0 R, where the fp64 oracle, whose sphere the rounded point lies outside of, gives none) as well
    centre = lambda a: np.tile(a[:len(NORMALS) * ns], (len(ENV_AT),) + (1,) * (a.ndim - 1))
    d64, d32 = centre(o64["d"]), centre(o32["d"])
    cos64 = np.sum(d64 * ref["n"], axis=1) / np.sum(ref["n"] * ref["n"], axis=1)     # d = s x + t y + n z: d . n = z |n|^2
    have_d = (at <= 1.0) & (X["pdf"] > 0)
    q = dict(d=(np.abs(X["d"] - d64).max(axis=1), np.abs(d32 - d64).max(axis=1), have_d),
             pdf=(np.abs(X["pdf"] - cos64 / np.pi), np.abs(centre(o32["pdf"]) - cos64 / np.pi), have_d),      # absolute: cos / pi <= 1 / pi, and 1e-10 / pi at the rim
             dist=(rel_err(X["dist"], o64["dist"]), rel_err(o32["dist"], o64["dist"]), inside & (at < 1.0)),
             on_sphere=(_on_bsphere(X, ref["ref"], c_dev if D is not None else o32["env_center"], R_dev if D is not None else o32["env_radius"]),
                        _on_bsphere(o32, ref["ref"], o32["env_center"], o32["env_radius"]), inside & (at < 1.0)))
    return q, at


def measure_env(probe, t, cells, sxy, ref, c_dev, R_dev):
    ns, ncell = ref["ns"], len(cells)
    o = np.array(RAY_ORIGINS, dtype=F32)
    rows = np.concatenate([np.full((ncell * ns, 1), SKY), ref["ref"], ref["n"], ref["s"]], axis=1)
    extra = np.concatenate([np.full((len(o), 1), SKY), o, np.tile([[0.0, 0.0, 1.0, 0.5, 0.5]], (len(o), 1))], axis=1)
    dev = probe.run("env", t, np.concatenate([rows, extra]))
    eps_dev, dev = dev[ncell * ns:, 5:7], dev[:ncell * ns]
    D = dict(d=dev[:, 0:3], dist=dev[:, 3], pdf=dev[:, 4])
    q, at = env_quantities(cells, ref, c_dev, R_dev, D)
    checks = _checks(ncell, q)
    o64, o32 = ref["o64"], ref["o32"]
    both = (np.isfinite(o64["dist"]) & np.isfinite(o32["dist"]))[:, None]
    bad = both & ~np.isfinite(dev[:, 0:5])
    outside_nonzero = (at > 1.0) & (D["pdf"] != 0)
    zero = (at < 1.0) & ((D["pdf"] > 0) != (o64["pdf"] > 0))
    on_it = (at == 1.0) & ((D["pdf"] > 0) != (o32["pdf"] > 0))           # on the sphere the precision decides: the fp32 oracle's pattern
    recs = []
    for i, cl in enumerate(cells):
        sl = slice(i * ns, (i + 1) * ns)
        recs.append(dict(name=cl["name"], checks=checks[i], nonfinite=int(bad[sl].sum()), outside_nonzero=int(outside_nonzero[sl].sum()), zero_mismatch=int(zero[sl].sum()),
                         on_sphere_mismatch=int(on_it[sl].sum()), lit_on_sphere=int(((D["pdf"] > 0) & (at == 1.0))[sl].sum())))
    # ray epsilons: the fp64 formula; the floor is the same formula in float32
    want = np.stack(ray_eps(o), axis=1)
    m32 = np.max(np.abs(o), axis=1)
    f32 = np.stack([F32(1e-4) * np.maximum(m32, F32(1e-4)), F32(1e-4) * m32], axis=1).astype(np.float64)
    nz = want > 0
    eps = dict(closest=judge(bp.worst(rel_err(eps_dev[:, 0], want[:, 0])), bp.worst(rel_err(f32[:, 0], want[:, 0]))),
               shadow=judge(bp.worst(rel_err(eps_dev[:, 1], want[:, 1]), nz[:, 1]), bp.worst(rel_err(f32[:, 1], want[:, 1]), nz[:, 1])),
               shadow_zero_at_origin=bool(np.all(eps_dev[~nz[:, 1], 1] == 0)), nonfinite=int((~np.isfinite(eps_dev)).sum()), n=len(o))
    return recs, eps, dict(env=dev, ray_eps=eps_dev)


def _local(d, cell):
    n, s = cell["n"].astype(np.float64), cell["s"].astype(np.float64)
    return np.stack([d @ s, d @ np.cross(n, s), d @ n], axis=1)


def light_contribution(ob, prec, o, cell):
    """radiance / (pdf emPdf) * f cos * a / (a + b) (direct.cpp:220-244) in fp64 from one oracle's sample; the BSDF terms come
    from the oracle's rough conductor in that oracle's precision, the diffuse ones from rgb / pi * cos in fp64."""
    wo = _local(o["d"], cell)
    wi = np.array([[0.0, 0.0, 1.0]])
    if cell["bsdf"] == 0:
        up = wo[:, 2] > 0
        f = np.where(up[:, None], np.array(REFL, dtype=F32).astype(np.float64)[None, :] * wo[:, 2:3] / np.pi, 0.0)
        bpdf = np.where(up, wo[:, 2] / np.pi, 0.0)
    else:
        eta, k = bp.COPPER
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(wo).all(axis=1)
        r = ob.bsdf_probe(prec, 0, float(F32(0.1)), np.array(eta, dtype=F32), np.array(k, dtype=F32), np.repeat(wi, len(wo), axis=0), wo=np.where(ok[:, None], wo, [[0.0, 0.0, -1.0]]),
                          specular_reflectance=np.array(REFL, dtype=F32))
        f, bpdf = r["eval"], r["pdf"]
    discrete = np.all(o["n"] == 0, axis=1) & (o["pdf"] > 0)          # a point light's sample: weight 1
    a, b = o["pdf"] ** 2, bpdf ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(discrete, 1.0, a / (a + b))
        return np.where((o["pdf"] > 0)[:, None], o["value"] * f * w[:, None], 0.0)


def light_reference(ob, sd, cells, sxy):
    ref = []
    for c in cells:
        z = np.zeros((len(sxy), 3))
        o = {p: ob.light_probe(p, sd, z, np.repeat(c["n"][None, :].astype(np.float64), len(sxy), axis=0), sxy=sxy.astype(np.float64)) for p in (64, 32)}
        ref.append(dict(o64=o[64], o32=o[32], c64=light_contribution(ob, 64, o[64], c), c32=light_contribution(ob, 32, o[32], c)))
    return ref


def measure_lights(probe, t, cells, sxy, edge, ref, sky_from):
    rows = np.concatenate([np.concatenate([np.full((len(sxy), 1), c["bsdf"]), np.zeros((len(sxy), 3)), np.repeat(c["n"][None, :], len(sxy), axis=0),
                                           np.repeat(c["s"][None, :], len(sxy), axis=0), np.tile([[0.0, 0.0, 1.0]], (len(sxy), 1)), sxy], axis=1) for c in cells])
    dev = probe.run("light", t, rows).reshape(len(cells), len(sxy), 7)
    recs = []
    for c, r, d in zip(cells, ref, dev):
        o64, o32 = r["o64"], r["o32"]
        picked = name_emitter(d[:, 3:6], d[:, 6], sky_from)
        rej_d, rej64, rej32 = np.all(d[:, 0:3] == 0, axis=1), np.all(r["c64"] == 0, axis=1), np.all(r["c32"] == 0, axis=1)
        ok = ~rej_d & ~rej64 & ~rej32
        scale = np.maximum(np.abs(r["c64"]).max(axis=1), 1e-300)
        err = lambda x: np.abs(x - r["c64"]).max(axis=1) / scale
        with np.errstate(invalid="ignore"):
            same = ok & (picked == o64["emitter"]) & (o32["emitter"] == o64["emitter"])
            dirs = dict(dd=judge(bp.worst(np.abs(d[:, 3:6] - o64["d"]).max(axis=1), same), bp.worst(np.abs(o32["d"] - o64["d"]).max(axis=1), same)),
                        dist=judge(bp.worst(rel_err(d[:, 6], o64["dist"]), same), bp.worst(rel_err(o32["dist"], o64["dist"]), same)),
                        contribution=judge(bp.worst(err(d[:, 0:3]), same), bp.worst(err(r["c32"]), same)))
        recs.append(dict(name=c["name"], checks=dirs, nonfinite=int((~np.isfinite(d)).sum()), rows=len(sxy), edge_rows=int(edge.sum()),
                         pick_mismatch=[[float(sxy[j, 0]), float(sxy[j, 1]), int(picked[j]), int(o64["emitter"][j])] for j in np.nonzero(~edge & (picked != o64["emitter"]))[0]][:20],
                         edge_mismatch=[[float(sxy[j, 0]), float(sxy[j, 1]), int(picked[j]), int(o32["emitter"][j])] for j in np.nonzero(edge & (picked != o32["emitter"]))[0]][:20],
                         zero_weight_picked=int(np.sum(np.isin(picked, [i for i, w in enumerate(WEIGHTS) if w == 0]))),
                         not_zero_where_both_reject=int(np.sum(rej64 & rej32 & ~rej_d)), rejected=int(rej64[~edge].sum()),
                         rejection_mismatch=int(np.sum((rej_d != rej64)[~edge])), grid_rows=int((~edge).sum())))
    return recs, dict(light=dev.reshape(-1, 7))


def measure(ob, probe, world):
    """All four runs of one build. world: what prepare() made once for both builds."""
    sp, sxy = world["spheres"], world["sxy"]
    spheres, raw = measure_spheres(ob, probe, sp["tables"], sp["scene"], sp["cells"], sxy, sp["ref"])
    lt = world["lights"]
    env, eps, raw_env = measure_env(probe, lt["tables"], lt["env_cells"], sxy, lt["env_ref"], lt["env_c"], lt["env_R"])
    lights, raw_l = measure_lights(probe, lt["tables"], lt["cells"], lt["sxy"], lt["edge"], lt["ref"], lt["sky_from"])
    raw.update(raw_env, **raw_l)
    return dict(spheres=spheres, env=env, ray_eps=eps, lights=lights, runs=probe.runs), raw


def prepare(pkg, ob, work_dir):
    """Scenes, uploaded tables, cells and both oracles' references: the part of the measurement that needs no GPU."""
    exe = harness(work_dir)
    sxy = sample_points()
    sd = sphere_scene(pkg)
    cells = sphere_cells()
    spheres = dict(scene=sd, tables=tables(pkg, exe, sd, work_dir), cells=cells, ref=sphere_reference(ob, sd, cells, sxy))
    ld = light_scene(pkg)
    t = tables(pkg, exe, ld, work_dir)
    lcells, lsxy, edge = light_cells(t)
    ecells, c, R = env_inputs(t)
    lights = dict(scene=ld, tables=t, cells=lcells, sxy=lsxy, edge=edge, ref=light_reference(ob, ld, lcells, lsxy), env_cells=ecells, env_c=c, env_R=R,
                  env_ref=env_reference(ob, ld, ecells, sxy), sky_from=0.6 * R)
    far = max(np.linalg.norm(c) for c in CENTRES if c is not None) + 0.1         # every shape's samples are nearer to the origin than the sky's
    assert far < lights["sky_from"] < R - np.linalg.norm(c), (far, R, c)
    return dict(sxy=sxy, spheres=spheres, lights=lights)


IDENTITIES = ("id_unit", "id_on_sphere", "id_normal", "id_cone", "id_pdf_direct", "id_pdf_area")


def findings(rep):
    """What the measurement holds against the device, by the test that asserts it."""
    over = lambda name, checks, keep: ["%s %s: %.3g > %.3g (floor %.3g, %.1f x the bound)" % (name, k, v["dev"], v["bound"], v["floor"], v["ratio"])
                                       for k, v in checks.items() if keep(k) and not v["ratio"] <= 1]
    ident = lambda k: k.split()[-1] in IDENTITIES
    f = dict(non_finite=[], sphere_values=[], sphere_identities=[], branch_band=[], environment=[], ray_eps=[], light_pick=[], contribution=[], rejection=[])
    n_corner = len(sample_points()) - N_GRID
    for c in rep["spheres"]:
        if c["nonfinite"]:
            f["non_finite"].append("%s: %d non-finite outputs" % (c["name"], c["nonfinite"]))
        band = c["kind"] == "band" or "sin=1-" in c["name"]
        held = lambda k: (c["name"], k) in EXPLAINED and c["over"].get(k, dict(ratio=0.0))["ratio"] <= 1      # the class's own assertion
        f["branch_band" if band else "sphere_values"] += over(c["name"], c["checks"], lambda k: not ident(k) and not held(k))
        f["branch_band" if band else "sphere_identities"] += over(c["name"], c["checks"], lambda k: ident(k) and not held(k))
        if c["pdf_area_zero_mismatch_grid"] > CAP * N_GRID:
            f["rejection"].append("%s: emitter_direct_pdf_area is zero where the oracle's is not, or the reverse, on %d of %d" % (c["name"], c["pdf_area_zero_mismatch_grid"], N_GRID))
        f["rejection"] += ["%s: corner (%g, %g): pdf_area zero against both oracles" % (c["name"], *q) for q in c["corner_zero_mismatch"]]
    for c in rep["env"]:
        if c["nonfinite"]:
            f["non_finite"].append("env %s: %d non-finite outputs" % (c["name"], c["nonfinite"]))
        f["environment"] += over("env " + c["name"], c["checks"], lambda k: True)
        if c["outside_nonzero"]:
            f["environment"].append("env %s: pdf != 0 on %d samples from outside the bounding sphere" % (c["name"], c["outside_nonzero"]))
        if c["on_sphere_mismatch"]:
            f["environment"].append("env %s: pdf zero or not against the fp32 oracle on %d samples" % (c["name"], c["on_sphere_mismatch"]))
        if c["zero_mismatch"] > CAP * (N_GRID + n_corner):
            f["environment"].append("env %s: pdf zero or not against the oracle on %d samples" % (c["name"], c["zero_mismatch"]))
    e = rep["ray_eps"]
    f["ray_eps"] += over("ray_eps", {k: v for k, v in e.items() if isinstance(v, dict)}, lambda k: True)
    f["ray_eps"] += ["ray_eps_shadow(0) != 0"] * (not e["shadow_zero_at_origin"])
    if e["nonfinite"]:
        f["non_finite"].append("ray_eps: %d non-finite outputs" % e["nonfinite"])
    for c in rep["lights"]:
        if c["nonfinite"]:
            f["non_finite"].append("light %s: %d non-finite outputs" % (c["name"], c["nonfinite"]))
        f["light_pick"] += ["light %s: sx %.9g sy %g: device %d, oracle64 %d" % (c["name"], *q) for q in c["pick_mismatch"]]
        f["light_pick"] += ["light %s: sx %.9g sy %g on a CDF entry: device %d, oracle32 %d" % (c["name"], *q) for q in c["edge_mismatch"]]
        if c["zero_weight_picked"]:
            f["light_pick"].append("light %s: %d samples went to an emitter of weight 0" % (c["name"], c["zero_weight_picked"]))
        f["contribution"] += over("light " + c["name"], c["checks"], lambda k: True)
        if c["not_zero_where_both_reject"]:
            f["rejection"].append("light %s: %d samples not zero that both oracles reject" % (c["name"], c["not_zero_where_both_reject"]))
        if c["rejection_mismatch"] > CAP * c["grid_rows"]:
            f["rejection"].append("light %s: rejection differs from the fp64 oracle on %d of %d" % (c["name"], c["rejection_mismatch"], c["grid_rows"]))
    return f


def summary(reports, diff):
    """What profiles/r11_light_probe.json holds: per cell and quantity the larger of the two builds' ratios (device error over the
    rule's bound), per build the worst ratio of each quantity and the counts."""
    units = list(reports)
    out = {"rule": "|device - oracle64| <= %g * max|oracle32 - oracle64| + 4 ulp; ratio = device error / that bound, <= 1 passes" % FACTOR, "builds_differ": diff}
    for group in ("spheres", "env", "lights"):
        cells = reports[units[0]][group]
        keys = sorted({k for c in cells for k in c["checks"]})
        by = {u: {c["name"]: c for c in reports[u][group]} for u in units}
        out[group + "_quantities"] = keys
        out[group] = {c["name"]: [round(max(by[u][c["name"]]["checks"][k]["ratio"] for u in units), 3) for k in keys] for c in cells}
        for u in units:
            worst = {k: max((c["checks"][k]["ratio"], c["name"]) for c in reports[u][group]) for k in keys}
            out.setdefault(u, {})[group] = dict(worst_ratio={k: [round(v[0], 4), v[1]] for k, v in worst.items()},
                                                counts={n: cnt for n, cnt in ((c["name"], {k: v for k, v in c.items() if k not in ("name", "kind", "checks", "over") and v not in (0, [])})
                                                                              for c in reports[u][group]) if cnt})
            if group == "spheres":   # every pair above the rule's bound: its ratio under the rule, and under the explained class's assertion
                out[u]["over_the_rule"] = {"%s | %s" % (c["name"], k): [round(c["checks"][k]["ratio"], 3), round(v["ratio"], 3), (c["name"], k) in EXPLAINED]
                                           for c in reports[u][group] for k, v in c["over"].items()}
    for u in units:
        out[u]["ray_eps"], out[u]["runs"] = reports[u]["ray_eps"], reports[u]["runs"]
    return out


def write_summary(path, s):
    """One line per top-level entry and per cell: the file stays readable in a diff."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in s.items():
            end = "\n}\n" if k == list(s)[-1] else ",\n"
            if k in ("spheres", "env", "lights"):
                f.write(' %s: {\n' % json.dumps(k) + ",\n".join("  %s: %s" % (json.dumps(n), line(r)) for n, r in v.items()) + "\n }" + end)
            else:
                f.write(" %s: %s%s" % (json.dumps(k), line(v), end))
