"""Helper of tests/test_ray_probe.py and tests/test_gpu_rays.py: builds and runs tests/native/ray_probe.hip over the parameter
block and the tables csrc/scene_prep.h makes for a scene (written by tests/native/scene_prep_harness.cpp), generates the rays,
computes the references -- a brute force over the scene's shapes in fp64 (numpy) and the oracle's own shape loop in float and in
double (oracle_ray_probe) -- and judges what the device's ray loops return under the rule of tests/bsdf_probe.py:

    |device - fp64| <= 32 * max |oracle32 - fp64| + 4 ulp        per quantity, scene and ray class; the ulp is of the scene's extent

The quantities are t, the hit point rebuilt in fp64 from the device's (prim, u, v) through the uploaded DShade bytes (origin +
u eu + v ev; a sphere: o + t d, held to |p - c| = r), and which shape. The same expression for the point, its maximum over the
classes 1 to 6 of a scene, is the scene's decision margin delta, in world units: measured from the two references alone.

Candidates. For a ray, every crossing of a shape's plane (sphere: both roots) is a candidate with its t, its point and its
margin: the distance from the point to the shape's boundary, positive inside (sphere: radius minus the ray's closest approach).
A plane met at the cosine c turns the rule's 4 ulp across it into 4 ulp / c along the ray, so a candidate's own allowance is
e = delta + 4 ulp / c; a ray that runs in a shape's plane has that shape as a candidate at any t, met at the cosine 0. A
candidate is PLAUSIBLE when margin > -e and tmin - e <= t <= tmax + e, SURE when margin >= e, tmin + e <= t <= tmax - e and
e <= 2 delta. With t* the smallest t + e of a sure candidate, the device may return any plausible candidate with t - e <= t*,
or a miss when no candidate is sure. A ray is DECIDED when that leaves one answer: then the device names that shape (or misses)
on every such ray, with no quantile, and t and the point obey the rule's bound as it stands. On the others the same list is the
candidate rule, and the candidate's t and point are held to the bound with 4 ulp / c in the place of 4 ulp. With any_hit the
loops that traverse may return any plausible candidate; hit or miss is compared where every answer agrees on it.

Why the cosine is in it, in figures of the references alone (tests/test_ray_probe.py asserts the consequences). With e = delta the
float oracle itself fails the decided-ray rule: on a ray that leaves a wall of cornell_c2 at a cosine of 3e-3 it finds that wall
again at t = 9.4e-5, beyond tmin = 6.6e-5, where fp64 has it at 2.2e-5 -- 4.7 delta away; on rays in a face's plane (cosine 1e-8)
it names shapes 0.1 to 1 away from the fp64 answer. And the double oracle and the numpy brute force, both in fp64, differ by
2e-12 relative in t at a cosine of 2e-4, past the 1e-12 asked of them on decided rays: hence e <= 2 delta, i.e. c >= 4 ulp /
delta, about 0.06. The errors under the rule's plain bound, 4 ulp whatever the cosine, are measured and recorded beside the
asserted ones (t_plain, p_plain in judge_op and in the JSON): on decided rays the two bounds are one.
"""
import json
import os
import struct
import subprocess

import numpy as np

import bsdf_probe as bp
from bsdf_probe import EPS, F32, FACTOR

ROOT = bp.ROOT
SRC = os.path.join(ROOT, "tests", "native", "ray_probe.hip")
HARNESS = os.path.join(ROOT, "tests", "native", "scene_prep_harness.cpp")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
UNITS = bp.UNITS
OPS = dict(trace15=0, trace0=1, brute=2, brute_vec=3, held=4, bvh32=5, bvh16=6, bvh32_cap12=7)
BVH_OPS = ("bvh32", "bvh16", "bvh32_cap12")
MAGIC = 0x59415250
TRACE_VOTE = 10                                # launch_plan.h
VOTES = (1, 10, 1024)
EPSILON_F, SHADOW_EPSILON_F = float(F32(1e-4)), float(F32(1e-3))   # device_math.h
CAP = 0.02                                     # share of the rays of a class (1 to 6) that may be undecided
CLASSES = ("random", "axis", "surface", "shadow", "window", "outside", "aimed")
LDS_BYTES = (27 * 4 + 27 * 2 + 15 * 4) * 64    # trav_run's columns: <int, 24>, <short, 24>, <int, 12>, CAP + 3 rows of 64 lanes each
PRIM = np.dtype([("m", "<f4", 12), ("type", "<i4"), ("shade", "<i4"), ("kind_shade", "<i4"), ("pad", "<i4")])
SHADE = np.dtype([("origin", "<f4", 3), ("eu", "<f4", 3), ("ev", "<f4", 3), ("n", "<f4", 3), ("inv_len_eu", "<f4"), ("bsdf", "<i4"), ("emitter", "<i4"), ("inv_area", "<f4")])
NODE = np.dtype([("box", "<f4", 24), ("child", "<i4", 4), ("pad", "<i4", 4)])
TRI, RECT, SPHERE = 0, 1, 2                    # abi.SHAPE_*, asserted in scene_geometry


def build(out_dir, unit):
    return bp.build(out_dir, unit, SRC)


def harness(out_dir):
    exe = os.path.join(str(out_dir), "scene_prep_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", bp.CSRC, "-I", HOST, "-o", exe, HARNESS], check=True)
    return exe


# ------------------------------------------------------------------ scenes
def one_box_room(scenes, res=32):
    """cornell_c2's five diffuse walls and its quad light, nothing inside: one cuboid + one flat record (tests/test_gpu_w2h.py runs it too)"""
    sd = scenes.SceneData("one_box_room")
    white, red, green, black = sd.diffuse(0.725, 0.71, 0.68), sd.diffuse(0.63, 0.065, 0.05), sd.diffuse(0.14, 0.45, 0.091), sd.diffuse(0.0)
    scenes._room(sd, white, red, green)
    sd.rectangle(scenes.translate(0, 0.995, 0) @ scenes.rotate("x", 90) @ scenes.scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(scenes.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, scenes.abi.FILTER_BOX, 0.5)
    return sd


def two_box_room(scenes, res=32):
    """... and an axis-aligned diffuse box on its floor: two cuboids + one flat record"""
    sd = one_box_room(scenes, res)
    sd.name = "two_box_room"
    sd.box(scenes.translate(0.2, -0.7, 0.1) @ scenes.scale(0.3, 0.3, 0.3), 0)
    return sd


def open_glass_box(pkg, res=48):
    """Cornell room + a dielectric box (rays travel INSIDE it: exits through existing faces) + a box whose top is missing (tests/test_gpu_boxes.py runs it too)."""
    sc = pkg.scenes
    sd = sc.cornell_c2(res)
    glass = sd.dielectric(1.5, 1.0)
    sd.box(sc.translate(-0.55, 0.35, 0.35) @ sc.rotate("x", 20) @ sc.rotate("y", 33) @ sc.scale(0.18, 0.22, 0.15), glass)
    n0 = len(sd.shapes)
    sd.box(sc.translate(0.55, 0.3, -0.4) @ sc.rotate("z", 25) @ sc.scale(0.2, 0.15, 0.2), 0)
    del sd.shapes[n0 + 2:n0 + 4]      # a face of the last box taken away: rays enter through the hole and hit the inside
    return sd


def _room_scene(pkg, name):
    return dict(one_box_room=one_box_room, two_box_room=two_box_room)[name](pkg.scenes, 32)


def _open_glass_box(pkg):
    sd = open_glass_box(pkg)
    sd.name = "open_glass_box"
    return sd


def _flat_mix(pkg, extra):
    """Plain triangles, one merged pair and a rectangle (the light), none forming a cuboid: 5 flat records, 6 with `extra`."""
    sc = pkg.scenes
    sd = sc.SceneData("flat_mix_%d" % (5 + extra))
    grey, black = sd.diffuse(0.5), sd.diffuse(0.0)
    sd.rectangle(sc.translate(0.1, 0.9, -0.2) @ sc.rotate("x", 80) @ sc.scale(0.6, 0.4, 1.0), black, radiance=(5.0, 5.0, 5.0))
    a, b, c = np.array((-0.8, -0.7, -0.5)), np.array((0.9, -0.6, -0.4)), np.array((0.7, -0.5, 0.8))
    sd.triangle(a, b, c, grey)                                 # (a, b, c), (a, c, d) with d = a + c - b: a merged pair
    sd.triangle(a, c, a + c - b, grey)
    sd.triangle((-0.9, -0.2, -0.9), (0.8, -0.3, -0.95), (0.1, 0.9, -0.8), grey)
    sd.triangle((-0.95, -0.8, 0.7), (-0.9, 0.6, 0.1), (-0.85, -0.7, -0.8), grey)
    sd.triangle((0.3, 0.1, 0.2), (0.5, 0.15, 0.1), (0.35, 0.4, 0.3), grey)
    if extra:
        sd.triangle((0.9, -0.9, 0.9), (0.95, 0.8, 0.2), (0.85, -0.6, -0.7), grey)
    sd.set_camera(sc.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.0, 16, 16)
    return sd


def _two_spheres(pkg):
    """glass_sphere and a second, larger sphere around part of the room: many ray origins lie inside it."""
    sd = pkg.scenes.glass_sphere(16)
    sd.name = "two_spheres"
    sd.sphere((0.3, 0.2, -0.2), 0.6, 0)
    return sd


def _soup(pkg):
    return pkg.scenes.triangle_soup(300, res=16)


def _deep_chain(pkg):
    return pkg.scenes.deep_chain(16, 90)


# name: (scene, knobs, ops, the prepared counts that show the scene reaches its loop)
CONFIGS = {
    "cornell_c2": (lambda pkg: pkg.scenes.cornell_c2(16), {}, ("trace0", "trace15", "held"), dict(n_box=3, n_flat_rec=1, has_plain_tri=0, use_bvh=0)),
    "cornell_c2 faces": (lambda pkg: pkg.scenes.cornell_c2(16), {"DRMLT_NO_BOX_MERGE": 1}, ("trace0", "trace15"), dict(n_box=0, n_flat_rec=18, has_plain_tri=0, use_bvh=0)),
    "one_box_room": (lambda pkg: _room_scene(pkg, "one_box_room"), {}, ("trace0", "trace15", "held"), dict(n_box=1, n_flat_rec=1, has_plain_tri=0, use_bvh=0)),
    "two_box_room": (lambda pkg: _room_scene(pkg, "two_box_room"), {}, ("trace0", "trace15", "held"), dict(n_box=2, n_flat_rec=1, has_plain_tri=0, use_bvh=0)),
    "open_glass_box": (_open_glass_box, {}, ("trace0", "trace15"), dict(n_box=5, n_flat_rec=1, has_plain_tri=0, use_bvh=0)),
    "flat_mix odd": (lambda pkg: _flat_mix(pkg, 0), {}, ("trace0", "trace15"), dict(n_box=0, n_flat_rec=5, has_plain_tri=1, use_bvh=0)),
    "flat_mix even": (lambda pkg: _flat_mix(pkg, 1), {}, ("trace0", "trace15"), dict(n_box=0, n_flat_rec=6, has_plain_tri=1, use_bvh=0)),
    "two_spheres": (_two_spheres, {}, ("trace15",), dict(n_box=1, n_flat_rec=1, has_plain_tri=0, use_bvh=0, n_flat=6, n_prims=8)),
    "two_spheres brute": (_two_spheres, {"DRMLT_NO_FLAT_LOOP": 1}, ("brute", "brute_vec", "trace15"), dict(n_box=0, n_flat_rec=0, use_bvh=0, n_prims=8)),
    "soup stack16": (_soup, {"DRMLT_BVH_THRESHOLD": 0}, ("bvh16", "bvh32", "trace15"), dict(use_bvh=1, bvh_stack16=1, ovf_entries=0)),
    "soup stack32": (_soup, {"DRMLT_BVH_THRESHOLD": 0, "DRMLT_BVH_STACK32": 1}, ("bvh32", "bvh32_cap12"), dict(use_bvh=1, bvh_stack16=0, ovf_entries=24)),
    "soup brute": (_soup, {"DRMLT_BVH_THRESHOLD": 100000}, ("brute", "brute_vec", "trace15"), dict(use_bvh=0, n_box=1, n_flat_rec=301, has_plain_tri=1)),
    "deep_chain": (_deep_chain, {"DRMLT_BVH_THRESHOLD": 0}, ("bvh16", "bvh32", "bvh32_cap12", "trace15"), dict(use_bvh=1, bvh_stack16=1, ovf_entries=48, bvh_depth=14)),
    "deep_chain brute": (_deep_chain, {"DRMLT_BVH_THRESHOLD": 100000}, ("brute", "brute_vec", "trace15"), dict(use_bvh=0, n_box=3, n_flat_rec=91, has_plain_tri=1)),
    "deep_chain bounded": (_deep_chain, {"DRMLT_BVH_THRESHOLD": 0, "DRMLT_BVH_MAX_DEPTH": 9}, ("bvh16", "bvh32"), dict(use_bvh=1, bvh_stack16=1, ovf_entries=0)),
}
# the scenes (geometry, rays and references are per scene, shared by its configurations)
SCENE_OF = {"cornell_c2": "cornell_c2", "cornell_c2 faces": "cornell_c2", "one_box_room": "one_box_room", "two_box_room": "two_box_room",
            "open_glass_box": "open_glass_box", "flat_mix odd": "flat_mix odd", "flat_mix even": "flat_mix even", "two_spheres": "two_spheres",
            "two_spheres brute": "two_spheres", "soup stack16": "soup", "soup stack32": "soup", "soup brute": "soup", "deep_chain": "deep_chain", "deep_chain bounded": "deep_chain", "deep_chain brute": "deep_chain"}


def prepared(pkg, exe, sd, knobs, work_dir, tag):
    """prepare_scene's parameter block and tables for one scene under `knobs`."""
    base = os.path.join(str(work_dir), tag.replace(" ", "_"))
    sd.save(base + ".drmlt")
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1)
    args = ["%s=%s" % (name, ("%.9g" if isinstance(getattr(cfg, name), float) else "%d") % getattr(cfg, name))
            for name, _ in cfg._fields_ if name not in ("struct_size", "reserved")]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}
    r = subprocess.run([exe, "scene=" + base + ".drmlt", "tables=" + base + ".tables", "params=" + base + ".params", *args, *["%s=%s" % kv for kv in knobs.items()]],
                       check=True, capture_output=True, text=True, env=env)
    out = json.loads(r.stdout)
    assert out["refusal"] == "", out["refusal"]
    raw, at, part = open(base + ".tables", "rb").read(), 0, {}
    for name, n in out["tables"]:
        part[name] = raw[at:at + n]
        at += n
    params = open(base + ".params", "rb").read()
    counts = dict(out["params"], ovf_entries=out["ovf_entries"], bvh_depth=out["bvh_depth"])
    assert len(part["prims"]) == 64 * counts["n_prims"] and len(part["shade"]) == 64 * counts["n_shade"] and len(part["bvh"]) == 128 * counts["n_bvh_nodes"]
    return dict(params=params, part=part, counts=counts, shade=np.frombuffer(part["shade"], dtype=SHADE), prims=np.frombuffer(part["prims"], dtype=PRIM))


def request(t, rays, ops, vote=TRACE_VOTE, part=None, params=None):
    """The bytes of a request. part / params: tables or a block other than the prepared ones (the refusal tests)."""
    part, params, c = part or t["part"], params or t["params"], t["counts"]
    rays = np.ascontiguousarray(rays, dtype=F32)
    assert rays.ndim == 2 and rays.shape[1] == 9
    head = struct.pack("<16i", MAGIC, len(rays), len(ops), len(part["prims"]) // 64, len(part["shade"]) // 64, len(part["bvh"]) // 128, len(part["flat"]) // 64,
                       len(part["boxes"]) // 64, c["ovf_entries"], vote, len(params), 0, 0, 0, 0, 0)
    return head + params + part["prims"] + part["shade"] + part["bvh"] + part["flat"] + part["boxes"] + rays.tobytes() + struct.pack("<%di" % len(ops), *[OPS[o] for o in ops])


def run_raw(exe, work_dir, req, limit=60):
    """One child run under `timeout -k 10 <limit>` -> (exit status, stderr, result bytes or None)."""
    a, b = os.path.join(str(work_dir), "ray.req"), os.path.join(str(work_dir), "ray.res")
    with open(a, "wb") as f:
        f.write(req)
    if os.path.exists(b):
        os.remove(b)
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe, a, b], capture_output=True, text=True, timeout=limit + 20)
    res = open(b, "rb").read() if r.returncode == 0 else None
    os.remove(a)
    return r.returncode, r.stderr, res


class Probe(bp.Probe):
    """bsdf_probe.Probe over ray_probe's request format; `dead` is the base class's, so one fault ends all probe runs."""

    def run(self, t, rays, ops, vote=TRACE_VOTE):
        """-> {op: (n, 4) uint32: prim, and the bits of t, u, v}"""
        if bp.Probe.dead:
            raise bp.ProbeDied(bp.Probe.dead)
        req = request(t, rays, ops, vote)
        self.runs += 1
        try:
            code, err, res = run_raw(self.exe, self.dir, req)
        except subprocess.TimeoutExpired:
            bp.Probe.dead = "%s %s: no answer within 80 s" % (os.path.basename(self.exe), ops)
            raise bp.ProbeDied(bp.Probe.dead)
        if code != 0:
            bp.Probe.dead = "%s %s: exit status %d: %s" % (os.path.basename(self.exe), ops, code, err[-500:])
            raise bp.ProbeDied(bp.Probe.dead)
        out = np.frombuffer(res, dtype=np.uint32).reshape(len(ops), len(rays), 4)
        return {o: out[i] for i, o in enumerate(ops)}


# ------------------------------------------------------------------ the scene's shapes, as the device receives them (float32), in fp64
def scene_geometry(pkg, sd):
    abi = pkg.abi
    assert (abi.SHAPE_TRIANGLE, abi.SHAPE_RECTANGLE, abi.SHAPE_SPHERE) == (TRI, RECT, SPHERE)
    n = len(sd.shapes)
    kind = np.array([s.type for s in sd.shapes])
    data = np.array([[float(F32(v)) for v in s.data[:12]] for s in sd.shapes], dtype=np.float64)
    org, eu, ev, c, r = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    for i in range(n):
        if kind[i] == TRI:
            org[i], eu[i], ev[i] = data[i, 0:3], data[i, 3:6] - data[i, 0:3], data[i, 6:9] - data[i, 0:3]
        elif kind[i] == RECT:
            m = data[i].reshape(3, 4)
            org[i], eu[i], ev[i] = m[:, 3], m[:, 0], m[:, 1]
        else:
            c[i], r[i] = data[i, 0:3], data[i, 3]
    nrm = np.cross(eu, ev)
    ln = np.linalg.norm(nrm, axis=1)
    nrm = nrm / np.where(ln > 0, ln, 1.0)[:, None]
    flat = kind != SPHERE
    pts = np.concatenate([org[flat], (org + eu)[flat], (org + ev)[flat], (org - eu)[flat & (kind == RECT)], (org - ev)[flat & (kind == RECT)],
                          (org + eu + ev)[flat & (kind == RECT)], (org - eu - ev)[flat & (kind == RECT)], (c - r[:, None])[~flat], (c + r[:, None])[~flat]])
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    return dict(n=n, kind=kind, org=org, eu=eu, ev=ev, nrm=nrm, c=c, r=r, lo=lo, hi=hi, extent=float(np.max(hi - lo)))


def point_on(g, i, a, b):
    """A point of flat shape i: a, b in [0, 1]^2 (a triangle: folded into it)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    tri = g["kind"][i] == TRI
    fold = tri & (a + b > 1)
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)
    u, v = np.where(tri, a, 2 * a - 1), np.where(tri, b, 2 * b - 1)
    return g["org"][i] + u[:, None] * g["eu"][i] + v[:, None] * g["ev"][i]


def candidates(g, o, d):
    """Every crossing of every shape, in fp64 -> t, margin (n_rays, n_cand) and the shape of each candidate column. A flat shape
    has one column, a sphere two (its roots). No crossing: t = +inf, margin = -inf. Last: the cosine at which the ray meets the shape's
    plane (a sphere: its surface; 0 at the silhouette and beyond)."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    T, M, S, C = [], [], [], []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(g["n"]):
            if g["kind"][i] != SPHERE:
                nn, eu, ev = g["nrm"][i], g["eu"][i], g["ev"][i]
                den = d @ nn
                t = ((g["org"][i] - o) @ nn) / den
                q = o + t[:, None] * d - g["org"][i]
                # in-plane coordinates by the dual basis, then the distance to each edge line, positive inside
                uu, vv, uv = eu @ eu, ev @ ev, eu @ ev
                det = uu * vv - uv * uv
                a, b = ((q @ eu) * vv - (q @ ev) * uv) / det, ((q @ ev) * uu - (q @ eu) * uv) / det
                hu, hv = np.sqrt(det / vv), np.sqrt(det / uu)        # world distance per unit of a across the line a = const, of b across b = const
                if g["kind"][i] == TRI:
                    hw = np.sqrt(det) / np.linalg.norm(eu - ev)      # height of the origin above the edge a + b = 1
                    m = np.minimum(np.minimum(a * hu, b * hv), (1 - a - b) * hw)
                else:
                    m = np.minimum((1 - np.abs(a)) * hu, (1 - np.abs(b)) * hv)
                ok = np.isfinite(t) & (np.abs(den) > 1e-12)            # a ray in the shape's plane crosses it nowhere (|d| = 1: 1e-12 is far below a float32 direction's rounding)
                # ... unless it runs IN the plane (within 4 ulp of the extent): then the shape is a candidate at any t, met at the cosine 0
                lies = ~ok & (np.abs((g["org"][i] - o) @ nn) <= 4 * EPS * g["extent"])
                T.append(np.where(ok, t, np.where(lies, 0.0, np.inf))), M.append(np.where(ok, m, np.where(lies, 0.0, -np.inf))), S.append(i)
                C.append(np.where(lies, 0.0, np.abs(den) / np.linalg.norm(d, axis=1)))
            else:
                oc = o - g["c"][i]
                A, b = np.sum(d * d, axis=1), np.sum(oc * d, axis=1)
                tc = -b / A                                            # closest approach
                dist = np.linalg.norm(oc + tc[:, None] * d, axis=1)
                m = g["r"][i] - dist
                half = np.sqrt(np.maximum(g["r"][i] ** 2 - dist ** 2, 0.0) / A)
                for s in (-1.0, 1.0):
                    T.append(np.where(np.isfinite(tc), tc + s * half, np.inf)), M.append(np.where(np.isfinite(tc), m, -np.inf)), S.append(i), C.append(np.sqrt(np.maximum(g["r"][i] ** 2 - dist ** 2, 0.0)) / g["r"][i])
    return np.stack(T, axis=1), np.stack(M, axis=1), np.array(S), np.stack(C, axis=1)


def brute_force(g, o, d, tmin, tmax):
    """The nearest hit in [tmin, tmax] in fp64 -> shape (-1: none), t, point."""
    T, M, S, _ = candidates(g, o, d)
    ok = (M >= 0) & (T >= np.asarray(tmin, dtype=np.float64)[:, None]) & (T <= np.asarray(tmax, dtype=np.float64)[:, None])
    tt = np.where(ok, T, np.inf)
    k = np.argmin(tt, axis=1)
    t = tt[np.arange(len(tt)), k]
    hit = np.isfinite(t)
    with np.errstate(invalid="ignore"):
        p = np.asarray(o, dtype=np.float64) + np.where(hit, t, 0.0)[:, None] * np.asarray(d, dtype=np.float64)
    return np.where(hit, S[k], -1), np.where(hit, t, np.inf), p


# ------------------------------------------------------------------ rays
def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(F32)


def _unit_rows(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def eps_closest(o):
    o = _f32(o)
    return (F32(1e-4) * np.maximum(np.max(np.abs(o), axis=1), F32(1e-4))).astype(F32)


def eps_shadow(o):
    o = _f32(o)
    return (F32(1e-4) * np.max(np.abs(o), axis=1)).astype(F32)


def _rows(o, d, tmin, tmax, any_hit=0.0):
    o, d = _f32(o), _f32(d)
    n = len(o)
    r = np.zeros((n, 9), dtype=F32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7], r[:, 8] = np.broadcast_to(_f32(tmin), n), np.broadcast_to(_f32(tmax), n), any_hit
    return r


def make_rays(g, seed, per=5000):
    """(rays (n, 9) float32, class index per ray), the classes interleaved by one fixed permutation: short and long traversals,
    closest-hit and any-hit rays share a wave."""
    rng = np.random.default_rng(seed)
    lo, hi, ext = g["lo"], g["hi"], g["extent"]
    centre = 0.5 * (lo + hi)
    flat = np.nonzero(g["kind"] != SPHERE)[0]
    inside = lambda n: rng.uniform(lo + 1e-3 * ext, hi - 1e-3 * ext, (n, 3))
    sphere_dirs = lambda n: _unit_rows(rng.normal(size=(n, 3)))
    size = np.sqrt(np.linalg.norm(np.cross(g["eu"][flat], g["ev"][flat]), axis=1))     # a primitive is chosen in proportion to its linear size
    on_flat = lambda n: (lambda idx: (idx, np.stack([point_on(g, i, rng.random(1), rng.random(1))[0] for i in idx])))(rng.choice(flat, n, p=size / size.sum()))
    verts = np.concatenate([g["org"][flat], (g["org"] + g["eu"])[flat], (g["org"] + g["ev"])[flat]])
    free = [k for k in range(3) if not np.any(verts[:, k] == 0)] or [0]               # coordinates in whose zero plane no shape has a vertex
    out = []
    # 1 random
    o = inside(per)
    out.append(_rows(o, sphere_dirs(per), eps_closest(o), np.inf))
    # 2 axis-parallel: d = +-e_i, the other components +0 and -0; origins anywhere, with a coordinate exactly 0, exactly on a face's plane
    n = per // 2
    o = inside(n)
    third = np.arange(n) % 3
    o[third == 1, rng.choice(free, n)[third == 1]] = 0.0
    idx, pf = on_flat(n)
    o = np.where((third == 2)[:, None], pf, o)
    axis = np.where(third == 2, np.argmax(np.abs(g["nrm"][idx]), axis=1), rng.integers(0, 3, n))   # off a face along its normal's main axis
    in_plane = (o[third == 2][: n // 8], g["nrm"][idx][third == 2][: n // 8])                          # (the rays IN a face's plane are class 7's)
    d = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0)
    d[np.arange(n), axis] = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    out.append(_rows(o, d, eps_closest(o), np.inf))
    # 3 from a surface: a point of a primitive as float32, the hemisphere on either side down to grazing, tmin as the library sets it
    idx, pf = on_flat(per)
    nn = g["nrm"][idx] * np.where(rng.random(per) < 0.5, 1.0, -1.0)[:, None]
    tang = _unit_rows(np.cross(nn, sphere_dirs(per)))
    cos = np.where(rng.random(per) < 0.5, np.maximum(rng.random(per), 0.05), 10.0 ** rng.uniform(np.log10(0.05), 0, per))
    graze = np.arange(per) < per // 8                              # (the departures between 1e-3 and 0.05 are class 7's: the ray's own surface is borderline)
    cos = np.where(graze, 10.0 ** rng.uniform(-3, np.log10(0.05), per), cos)
    d = nn * cos[:, None] + tang * np.sqrt(1 - cos * cos)[:, None]
    # (the library's tmin is 1e-4 of the origin's largest coordinate: where that is below 0.15 of the extent, tmin comes within delta of the ray's own surface)
    far = np.max(np.abs(pf), axis=1) >= 0.15 * ext
    out.append(_rows(pf[~graze & far], d[~graze & far], eps_closest(pf[~graze & far]), np.inf))
    grazing = _rows(pf[graze | ~far], d[graze | ~far], eps_closest(pf[graze | ~far]), np.inf)   # (moved, not dropped)
    # 4 shadow rays: from a point of one primitive at a point of another, tmax = dist (1 - ShadowEpsilon) in float32, any_hit 0 and 1
    n = per // 2
    ia, pa = on_flat(n)
    ib, pb = on_flat(n)
    pa, pb = _f32(pa), _f32(pb)
    dv = (pb - pa).astype(F32)
    dist = np.sqrt(np.sum(dv * dv, axis=1, dtype=F32)).astype(F32)
    with np.errstate(invalid="ignore", divide="ignore"):   # another primitive, not in the plane of either
        du = dv.astype(np.float64) / dist[:, None]
        apart = dist > F32(1e-3 * ext)                   # (two points in one place give no direction)
        keep = (np.max(np.abs(pa), axis=1) >= 0.15 * ext) & (np.abs(np.sum(du * g["nrm"][ia], axis=1)) > 0.05) & (np.abs(np.sum(du * g["nrm"][ib], axis=1)) > 0.05)
    pa, dv, dist, keep = pa[apart], dv[apart], dist[apart], keep[apart]
    d = (dv / dist[:, None]).astype(F32)
    tmax = (dist * (F32(1) - F32(1e-3))).astype(F32)
    for any_hit in (0.0, 1.0):
        out.append(_rows(pa[keep], d[keep], eps_shadow(pa[keep]), tmax[keep], any_hit))
    grazing = np.concatenate([grazing] + [_rows(pa[~keep], d[~keep], eps_shadow(pa[~keep]), tmax[~keep], a) for a in (0.0, 1.0)])   # the others: class 7's
    shadow_parts = 2
    # 5 windows: tmin beyond the first surface, tmax short of it
    n = per // 2
    o, d = _f32(inside(n)), _f32(sphere_dirs(n))
    T, M, _, _ = candidates(g, o, d)
    tt = np.sort(np.where((M >= 0) & (T > 1e-3 * ext), T, np.inf), axis=1)
    t1, t2 = tt[:, 0], tt[:, 1] if tt.shape[1] > 1 else np.full(n, np.inf)
    ok = np.isfinite(t1)
    beyond = np.where(np.isfinite(t2), 0.5 * (t1 + t2), 2 * t1)
    out.append(_rows(o[ok], d[ok], beyond[ok], np.inf))
    out.append(_rows(o[ok], d[ok], eps_closest(o[ok]), t1[ok] * rng.uniform(0.5, 0.999, ok.sum())))
    window_parts = 2
    # 6 from outside: at points inside the scene's box (through an open side, or against the back of a wall), and pointing away
    n = per // 2
    away = sphere_dirs(n)
    o = centre + away * ext * rng.uniform(1.0, 1.5, n)[:, None]
    aim = _unit_rows(inside(n) - o)
    out.append(_rows(o, aim, eps_closest(o), np.inf))
    out.append(_rows(o, away, eps_closest(o), np.inf))
    outside_parts = 2
    # 7 aimed at vertices, edges and silhouettes chosen in fp64, the direction's components offset by 0, +-1, +-16 ulp: borderline by construction
    n = per // 2
    idx = rng.choice(flat, n)
    kind = rng.integers(0, 3, n)                                   # 0 a vertex, 1 a point of an edge, 2 a point of an edge of the merged diagonal / the centre line
    s = rng.random(n)
    tri = g["kind"][idx] == TRI
    a = np.where(kind == 0, rng.integers(0, 2, n), np.where(kind == 1, s, s))
    b = np.where(kind == 0, rng.integers(0, 2, n), np.where(kind == 1, 0.0, s))
    fold = tri & (a + b > 1)
    b = np.where(fold, 1 - a, b)
    u, v = np.where(tri, a, 2 * a - 1), np.where(tri, b, 2 * b - 1)
    target = g["org"][idx] + u[:, None] * g["eu"][idx] + v[:, None] * g["ev"][idx]
    balls = np.nonzero(g["kind"] == SPHERE)[0]
    o = inside(n)
    if len(balls):                                                 # a third of them at a sphere's silhouette as seen from the origin
        which = rng.choice(balls, n)
        c, r = g["c"][which], g["r"][which]
        oc = c - o
        L = np.linalg.norm(oc, axis=1)
        w = oc / L[:, None]
        side = _unit_rows(np.cross(w, sphere_dirs(n)))
        sin = np.minimum(r / L, 1.0)
        tangent = o + (w * np.sqrt(1 - sin * sin)[:, None] + side * sin[:, None]) * (L * np.sqrt(1 - sin * sin))[:, None]
        use = (np.arange(n) % 3 == 0) & (L > r * 1.01)
        target = np.where(use[:, None], tangent, target)
    d = _f32(_unit_rows(target - _f32(o).astype(np.float64)))
    ulps = rng.choice(np.array([0, 1, -1, 16, -16]), n)
    comp = rng.integers(0, 3, n)
    bits = d.view(np.int32).copy()
    bits[np.arange(n), comp] += ulps * np.where(d[np.arange(n), comp] < 0, -1, 1) * (d[np.arange(n), comp] != 0)
    d = bits.view(F32)
    po, pn = in_plane                                              # ... and rays that run in a face's plane, along an axis where the face is axis-aligned
    pd = np.cross(pn, np.eye(3)[np.argmin(np.abs(pn), axis=1)])
    pd = np.where(np.abs(pd) < 1e-6, 0.0, pd)
    o, d = np.concatenate([o, po]), np.concatenate([d, _f32(_unit_rows(pd))])
    out.append(np.concatenate([_rows(o, d, eps_closest(o), np.inf), grazing]))
    # classes 1 to 6 keep the rays whose nearest surface is met at a cosine above 0.2: a condition on the inputs, from the fp64 side alone,
    # which keeps the float oracle's worst error -- and with it delta -- at a few ulp of the extent, below the library's own tmin. The
    # others are not dropped: they move to class 7, which is judged by the candidate rule and by the decided-ray rule where it decides.
    # Rays that start on, or first meet, two shapes in one place (a box standing on the floor: its bottom face lies in the floor) name
    # either shape: they move to class 7.
    moved = []
    for k in range(len(out) - 1):
        r = out[k]
        shape, t1, _ = brute_force(g, r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7])
        cosi = np.abs(np.sum(r[:, 3:6].astype(np.float64) * g["nrm"][np.maximum(shape, 0)], axis=1))
        T, M, _, _ = candidates(g, r[:, 0:3], r[:, 3:6])
        with np.errstate(invalid="ignore"):
            twice = (np.sum((M > 0) & (np.abs(T - t1[:, None]) < 1e-6 * ext), axis=1) > 1) | (np.sum((M > 0) & (np.abs(T) < 1e-6 * ext), axis=1) > 1)
        stay = ~twice & ((shape < 0) | (g["kind"][np.maximum(shape, 0)] == SPHERE) | (cosi > 0.2))
        moved.append(r[~stay])
        out[k] = r[stay]
    out[-1] = np.concatenate([out[-1]] + moved)
    cls = np.concatenate([np.full(len(r), k) for k, r in zip([0, 1, 2] + [3] * shadow_parts + [4] * window_parts + [5] * outside_parts + [6], out)])
    rays = np.concatenate(out)
    away_mask = np.zeros(len(rays), dtype=bool)
    at = sum(len(r) for r in out[:-2])
    away_mask[at:at + len(out[-2])] = True                        # the rays that point away from the scene: every loop returns -1
    perm = rng.permutation(len(rays))
    return rays[perm], cls[perm], away_mask[perm]


# ------------------------------------------------------------------ references and the rule
def references(ob, sd, g, rays):
    """Per ray: the candidates in fp64, the fp64 brute force, the oracle in double and in float."""
    o, d, tmin, tmax = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64), rays[:, 6].astype(np.float64), rays[:, 7].astype(np.float64)
    T, M, S, C = candidates(g, o, d)
    shape, t, p = brute_force(g, o, d, tmin, tmax)
    return dict(o=o, d=d, tmin=tmin, tmax=tmax, T=T, M=M, S=S, C=C, ball=g["kind"][S] == SPHERE, shape=shape, t=t, p=p, o64=ob.ray_probe(64, sd, o, d, tmin, tmax), o32=ob.ray_probe(32, sd, o, d, tmin, tmax))


def floors(g, ref, cls):
    """max |oracle32 - fp64| of t and of the point, per class, over the rays on which both name the same shape; and delta."""
    same = (ref["o32"]["shape"] == ref["shape"]) & (ref["shape"] >= 0)
    ulp = 4 * EPS * g["extent"]
    et, ep = np.abs(ref["o32"]["t"] - ref["t"]), np.linalg.norm(ref["o32"]["p"] - ref["p"], axis=1)
    fl = {}
    for k, name in enumerate(CLASSES):
        m = same & (cls == k)
        fl[name] = dict(t=bp.worst(et, m), p=bp.worst(ep, m), n=int(m.sum()), bound_t=FACTOR * bp.worst(et, m) + ulp, bound_p=FACTOR * bp.worst(ep, m) + ulp)
    delta = FACTOR * max(fl[name]["p"] for name in CLASSES[:6]) + ulp
    return fl, delta


def allowed(ref, delta, ulp, any_hit=None):
    """Per ray the answers the rule allows: a mask over the candidate columns, and whether a miss is allowed. any_hit: the rows
    traced for any hit (every plausible candidate is allowed there)."""
    T, M = ref["T"], ref["M"]
    tmin, tmax = ref["tmin"][:, None], ref["tmax"][:, None]
    with np.errstate(divide="ignore", invalid="ignore"):   # (inf - inf where the cosine is 0 and tmax infinite: the comparison is then false)
        e = delta + ulp / ref["C"]         # delta, and the rule's 4 ulp along the ray: a plane met at the cosine c turns them into 4 ulp / c
        em = np.where(ref["ball"][None, :], delta, e)      # a sphere's margin is its closest approach's: no cosine amplifies it
        plausible = (M > -em) & (T >= tmin - e) & (T <= tmax + e)
        sure = (M >= em) & (T >= tmin + e) & (T <= tmax - e) & (e <= 2 * delta)    # (met at a cosine below 4 ulp / delta its own allowance exceeds the margin)
        tstar = np.min(np.where(sure, T + e, np.inf), axis=1)
        ok = plausible & ~(T - e > tstar[:, None])
    if any_hit is not None:
        ok = np.where(any_hit[:, None], plausible, ok)
    return ok, ~sure.any(axis=1)


def decided(ref, delta, ulp):
    """-> (decided, the shape the device must name there or -1). Closest-hit semantics for every ray."""
    ok, miss = allowed(ref, delta, ulp)
    n_ans = ok.sum(axis=1) + miss
    k = np.argmax(ok, axis=1)
    return n_ans == 1, np.where(miss, -1, ref["S"][k])


def judge_op(t, g, ref, cls, fl, delta, raw, honours_any_hit, rays):
    """One op's output against the rule -> a record of counts, worst ratios per class and quantity, and the first offenders."""
    prim = raw[:, 0].view(np.int32).astype(np.int64)
    tt, u, v = (raw[:, k].view(F32).astype(np.float64) for k in (1, 2, 3))
    n = len(prim)
    hit = prim >= 0
    rec = dict(n=n, findings={k: [] for k in ("decided_shapes", "bounds", "candidates", "misses", "any_hit", "non_finite", "bad_prim")}, ratios={})
    F = rec["findings"]
    bad = hit & (prim >= len(t["shade"]))
    if bad.any():
        F["bad_prim"].append("%d hits name a record outside the table, the first: ray %d prim %d" % (bad.sum(), np.argmax(bad), prim[np.argmax(bad)]))
        hit = hit & ~bad
    sh = t["shade"]
    pi = np.where(hit, prim, 0)
    kind = sh["bsdf"][pi] >> 24
    ball = hit & (kind == SPHERE)
    with np.errstate(invalid="ignore", over="ignore"):
        on_ray = ref["o"] + ref["d"] * np.where(hit, tt, 0.0)[:, None]
        p = sh["origin"][pi].astype(np.float64) + u[:, None] * sh["eu"][pi].astype(np.float64) + v[:, None] * sh["ev"][pi].astype(np.float64)
    p = np.where(ball[:, None], on_ray, p)
    nf = hit & ~(np.isfinite(tt) & np.isfinite(u) & np.isfinite(v))
    if nf.any():
        F["non_finite"].append("%d hits with a non-finite t, u or v, the first: ray %d (class %s)" % (nf.sum(), np.argmax(nf), CLASSES[cls[np.argmax(nf)]]))
        hit = hit & ~nf
    any_hit = (rays[:, 8] != 0) & honours_any_hit
    ulp = 4 * EPS * g["extent"]
    ok, miss_ok = allowed(ref, delta, ulp, any_hit)
    dec, want = decided(ref, delta, ulp)
    # the candidate the device returned: the allowed column of its shape nearest in t
    col_shape = ref["S"][None, :] == prim[:, None]
    with np.errstate(invalid="ignore"):
        gap = np.where(ok & col_shape, np.abs(ref["T"] - tt[:, None]), np.inf)
    k = np.argmin(gap, axis=1)
    found = hit & np.isfinite(gap[np.arange(n), k])
    tc = ref["T"][np.arange(n), k]
    pc = ref["o"] + ref["d"] * np.where(np.isfinite(tc), tc, 0.0)[:, None]
    bt = np.array([fl[CLASSES[c]]["bound_t"] for c in cls])
    bpnt = np.array([fl[CLASSES[c]]["bound_p"] for c in cls])
    # on an undecided ray the candidate's own allowance takes the place of the rule's 4 ulp: 4 ulp / c along the ray
    with np.errstate(divide="ignore", invalid="ignore"):
        wider = np.where(found & (~dec | any_hit), ulp / ref["C"][np.arange(n), k] - ulp, 0.0)
    plain_t, base = bt, bpnt
    bt, bpnt = bt + wider, bpnt + wider
    with np.errstate(invalid="ignore"):
        et = np.where(found, np.abs(tt - tc), 0.0)
    ep = np.where(found, np.linalg.norm(p - pc, axis=1), 0.0)
    # a sphere's point lies on it; a flat hit's rebuilt point lies on the ray at its t (the check of any-hit answers, made for all)
    with np.errstate(invalid="ignore"):
        c_r = np.where(ball, np.abs(np.linalg.norm(on_ray - g["c"][np.clip(pi, 0, g["n"] - 1)], axis=1) - g["r"][np.clip(pi, 0, g["n"] - 1)]), 0.0)
        own = np.where(hit & ~ball, np.linalg.norm(p - on_ray, axis=1), 0.0)
    closest = ~any_hit
    # -- decided rays: the shape, and a miss where the reference misses
    wrong = dec & closest & (np.where(hit, prim, -1) != want) & ~bad
    for j in np.nonzero(wrong & (want >= 0))[0][:5]:
        F["decided_shapes"].append("ray %d (%s): device %d t %.9g, reference shape %d t %.9g" % (j, CLASSES[cls[j]], prim[j], tt[j], want[j], ref["t"][j]))
    for j in np.nonzero(wrong & (want < 0))[0][:5]:
        F["misses"].append("ray %d (%s): device %d t %.9g where the reference misses" % (j, CLASSES[cls[j]], prim[j], tt[j]))
    rec["decided_wrong_shape"], rec["decided_wrong_miss"] = int((wrong & (want >= 0)).sum()), int((wrong & (want < 0)).sum())
    # -- every ray: what it returned is an allowed answer
    stray = closest & ((hit & ~found) | (~hit & ~miss_ok & ~bad & ~nf))
    for j in np.nonzero(stray & ~dec)[0][:5]:
        F["candidates"].append("ray %d (%s): device %d t %.9g is no allowed candidate (nearest sure hit t %.9g)" % (j, CLASSES[cls[j]], prim[j], tt[j], ref["t"][j]))
    rec["undecided_stray"] = int((stray & ~dec).sum())
    # -- any-hit rows: hit or miss where every allowed answer agrees, and the answer a plausible candidate
    ah_wrong = any_hit & ((hit & ~found) | (~hit & ~miss_ok))
    for j in np.nonzero(ah_wrong)[0][:5]:
        F["any_hit"].append("ray %d (%s): device %d t %.9g, reference %s" % (j, CLASSES[cls[j]], prim[j], tt[j], "misses" if not ok[j].any() else "hits"))
    rec["any_hit_wrong"], rec["any_hit_rows"] = int(ah_wrong.sum()), int(any_hit.sum())
    # -- bounds, per class
    for c, name in enumerate(CLASSES):
        m = cls == c
        # t_plain, p_plain: the same errors over the rule's bound as it stands, 4 ulp whatever the cosine -- recorded, so that what the
        # allowance 4 ulp / c lets pass on undecided rays is on the record (on decided rays the two bounds are one)
        r = dict(t=bp.worst(et / bt, m), p=bp.worst(ep / bpnt, m), on_ray=bp.worst(own / base, m), on_sphere=bp.worst(c_r / base, m),
                 t_plain=bp.worst(et / plain_t, m), p_plain=bp.worst(ep / base, m))
        rec["ratios"][name] = {q: round(x, 4) for q, x in r.items()}
        for q, x in r.items():
            if not x <= 1 and not q.endswith("_plain"):
                F["bounds"].append("%s %s: %.3g x the bound (%.3g)" % (name, q, x, fl[name]["bound_t" if q == "t" else "bound_p"]))
    rec["hits"], rec["undecided"] = int(hit.sum()), int((~dec).sum())
    return rec


def builds_differ(a, b):
    """Per configuration and op, how many of the 4 n output words differ between the two builds."""
    return {"%s %s" % (cfg, op): dict(elements=int((a[cfg][op] != b[cfg][op]).sum()), of=int(a[cfg][op].size)) for cfg in a for op in a[cfg]}


# ------------------------------------------------------------------ the world: everything that needs no GPU, once for both builds
SEEDS = {name: 100 + i for i, name in enumerate(sorted(set(SCENE_OF.values())))}


def prepare(pkg, ob, work_dir, per=5000):
    exe = harness(work_dir)
    scenes, configs = {}, {}
    for cfg, (make, knobs, ops, want) in CONFIGS.items():
        sd = make(pkg)
        name = SCENE_OF[cfg]
        if name not in scenes:
            g = scene_geometry(pkg, sd)
            rays, cls, away = make_rays(g, SEEDS[name], per)
            ref = references(ob, sd, g, rays)
            fl, delta = floors(g, ref, cls)
            dec, want_shape = decided(ref, delta, 4 * EPS * g["extent"])
            scenes[name] = dict(sd=sd, g=g, rays=rays, cls=cls, away=away, ref=ref, floors=fl, delta=delta, decided=dec, want=want_shape,
                                perm=np.random.default_rng(SEEDS[name] + 1000).permutation(len(rays)))
        configs[cfg] = dict(scene=name, ops=ops, want=want, t=prepared(pkg, exe, sd, knobs, work_dir, cfg))
    return dict(scenes=scenes, configs=configs)


def undecided_shares(world):
    """{scene: {class: share of its rays that are undecided}}"""
    out = {}
    for name, s in world["scenes"].items():
        out[name] = {c: float(np.mean(~s["decided"][s["cls"] == k])) for k, c in enumerate(CLASSES)}
    return out


# ------------------------------------------------------------------ the measurement (GPU)
def _traverses(cfg, op):
    return op in BVH_OPS or (op == "trace15" and cfg["t"]["counts"]["use_bvh"] == 1)


def measure(probe, world):
    """All child runs of one build: per configuration the ops at the library's vote; for the ops that traverse also at the votes
    1 and 1024 and over the permuted ray list. -> (report per configuration, raw output per configuration and op)"""
    report, raw = {}, {}
    for name, cfg in world["configs"].items():
        s = world["scenes"][cfg["scene"]]
        t, rays = cfg["t"], s["rays"]
        out = probe.run(t, rays, cfg["ops"])
        raw[name] = out
        rec = dict(ops={}, identities=[])
        for op in cfg["ops"]:
            rec["ops"][op] = judge_op(t, s["g"], s["ref"], s["cls"], s["floors"], s["delta"], out[op], _traverses(cfg, op), rays)
            prim = out[op][:, 0].view(np.int32)
            if np.any(prim[s["away"]] != -1):
                rec["ops"][op]["findings"]["misses"].append("%d rays that point away from the scene return a hit" % int(np.sum(prim[s["away"]] != -1)))
        if "held" in cfg["ops"]:
            ne = np.any(out["held"] != out["trace0"], axis=1)
            rec["held_differs"] = int(ne.sum())
            if ne.any():
                rec["identities"].append(("held", "held differs from trace0 on %d rays, the first: ray %d (%s)" % (ne.sum(), np.argmax(ne), CLASSES[s["cls"][np.argmax(ne)]])))
        trav = tuple(op for op in cfg["ops"] if _traverses(cfg, op))
        if trav:
            for vote in VOTES:
                if vote == TRACE_VOTE:
                    continue
                other = probe.run(t, rays, trav, vote)
                for op in trav:
                    ne = np.any(other[op] != out[op], axis=1)
                    rec.setdefault("vote_differs", {})["%s vote %d" % (op, vote)] = int(ne.sum())
                    if ne.any():
                        rec["identities"].append(("vote", "%s: trace_vote %d differs from %d on %d rays, the first: ray %d" % (op, vote, TRACE_VOTE, ne.sum(), np.argmax(ne))))
            perm = s["perm"]
            other = probe.run(t, rays[perm], trav)
            for op in trav:
                back = np.empty_like(other[op])
                back[perm] = other[op]
                ne = np.any(back != out[op], axis=1)
                rec.setdefault("perm_differs", {})[op] = int(ne.sum())
                if ne.any():
                    rec["identities"].append(("perm", "%s: the permuted ray list differs on %d rays, the first: ray %d" % (op, ne.sum(), np.argmax(ne))))
        report[name] = rec
    return dict(configs=report, runs=probe.runs), raw


def runs_of(world):
    """Child runs of measure() per build: one per configuration, three more where an op traverses."""
    return sum(1 + (3 if any(_traverses(c, op) for op in c["ops"]) else 0) for c in world["configs"].values())
TESTS = ("decided_shapes", "bounds", "candidates", "misses", "any_hit", "non_finite", "held", "vote", "perm")


def findings(rep):
    """What the measurement holds against the device, by the test that asserts it."""
    f = {k: [] for k in TESTS}
    for name, rec in rep["configs"].items():
        for op, r in rec["ops"].items():
            for k, v in r["findings"].items():
                f["non_finite" if k == "bad_prim" else k] += ["%s %s: %s" % (name, op, x) for x in v]
        for k, what in rec["identities"]:
            f[k].append("%s: %s" % (name, what))
    return f


def summary(world, reports, diff, parent=""):
    """What DRMLT_RAY_PROBE_JSON=<file> gets (profiles/r18_ray_probe.json is one such run): delta, the floors and the undecided shares per scene; per configuration, op and
    class the larger of the two builds' ratios (worst device error over the rule's bound) and the counts; the builds' differences."""
    units = list(reports)
    out = {"parent_commit": parent,
           "rule": "|device - fp64| <= %g * max|oracle32 - fp64| + 4 ulp of the extent; ratio = worst device error / that bound, <= 1 passes" % FACTOR,
           "quantities": ["t", "p", "on_ray", "on_sphere", "t_plain", "p_plain"], "classes": list(CLASSES), "builds_differ": diff, "undecided_share": undecided_shares(world),
           "scenes": {n: dict(delta=s["delta"], rays=len(s["rays"]), floors={c: [f["t"], f["p"]] for c, f in s["floors"].items()}) for n, s in world["scenes"].items()},
           "ratios": {}, "counts": {}}
    for cfg in reports[units[0]]["configs"]:
        for op in reports[units[0]]["configs"][cfg]["ops"]:
            recs = [reports[u]["configs"][cfg]["ops"][op] for u in units]
            out["ratios"]["%s | %s" % (cfg, op)] = {c: [max(r["ratios"][c][q] for r in recs) for q in out["quantities"]] for c in CLASSES}
            out["counts"]["%s | %s" % (cfg, op)] = {k: max(r[k] for r in recs) for k in ("n", "hits", "undecided", "decided_wrong_shape", "decided_wrong_miss", "undecided_stray", "any_hit_rows", "any_hit_wrong")}
        rec = reports[units[0]]["configs"][cfg]
        for k in ("held_differs", "vote_differs", "perm_differs"):
            if k in rec:
                out["counts"]["%s | %s" % (cfg, k)] = rec[k]
    out["runs"] = {u: reports[u]["runs"] for u in units}
    return out


def write_summary(path, s):
    """One line per top-level entry, per scene and per (configuration, op): the file stays readable in a diff."""
    line = lambda v: json.dumps(v, separators=(",", ":"))
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in s.items():
            end = "\n}\n" if k == list(s)[-1] else ",\n"
            if isinstance(v, dict) and k in ("undecided_share", "scenes", "ratios", "counts", "builds_differ"):
                f.write(' %s: {\n' % json.dumps(k) + ",\n".join("  %s: %s" % (json.dumps(n), line(r)) for n, r in v.items()) + "\n }" + end)
            else:
                f.write(" %s: %s%s" % (json.dumps(k), line(v), end))


# ------------------------------------------------------------------ a stand-in for the device (CPU tests of the judge)
def emulate_brute(t, rays, w_test=True):
    """intersect_prim over the uploaded DPrim records in numpy float32 (no fused multiply-add, IEEE division), in table order: what
    trace_brute computes, to rounding -> (n, 4) uint32 as the probe writes them. Gives tests/test_ray_probe.py a device-shaped
    answer to run the judge on without a GPU. w_test=False: the hit test as it was before this probe found its hole (min3 alone)."""
    rays = np.ascontiguousarray(rays, dtype=F32)
    o, d, tmin = rays[:, 0:3], rays[:, 3:6], rays[:, 6]
    n = len(rays)
    best, prim, bu, bv = rays[:, 7].copy(), np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    with np.errstate(all="ignore"):
        for g in t["prims"]:
            m = g["m"].reshape(3, 4)
            lo = (o @ m[:, :3].T + m[:, 3]).astype(F32)
            ld = (d @ m[:, :3].T).astype(F32)
            if g["type"] != 2:
                tt = (-lo[:, 2] / ld[:, 2]).astype(F32)
                u, v = (tt * ld[:, 0] + lo[:, 0]).astype(F32), (tt * ld[:, 1] + lo[:, 1]).astype(F32)
                w = F32(1) - (u + v) if g["type"] == 0 else np.fmin(F32(1) - u, F32(1) - v)      # np.fmin skips a NaN, as fminf does
                hit = (np.fmin(np.fmin(u, v), w) >= 0) & (tt >= tmin) & (tt <= best)
                if w_test:
                    hit = hit & (w >= 0)
                idx = np.full(n, g["shade"], dtype=np.int32)
                if g["type"] == 3:
                    second = v > u
                    idx = idx + second
                    u, v = np.where(second, u, u - v).astype(F32), np.where(second, v - u, v).astype(F32)
            else:
                A, b = np.sum(ld * ld, axis=1), np.sum(lo * ld, axis=1)
                l = lo - ld * (b / A)[:, None]
                disc = A * (F32(1) - np.sum(l * l, axis=1))
                sq = np.sqrt(np.maximum(disc, 0))
                q = np.where(b < 0, -(b - sq), -(b + sq))
                t0, t1 = q / A, (np.sum(lo * lo, axis=1) - F32(1)) / q
                near, far = np.minimum(t0, t1), np.maximum(t0, t1)
                tt = np.where(near < tmin, far, near).astype(F32)
                hit = (disc >= 0) & (near <= best) & (far >= tmin) & ((near >= tmin) | (far <= best))
                u = v = np.zeros(n, dtype=F32)
                idx = np.full(n, g["shade"], dtype=np.int32)
            best, prim, bu, bv = np.where(hit, tt, best).astype(F32), np.where(hit, idx, prim).astype(np.int32), np.where(hit, u, bu).astype(F32), np.where(hit, v, bv).astype(F32)
    out = np.zeros((n, 4), dtype=np.uint32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = prim.view(np.uint32), best.view(np.uint32), bu.view(np.uint32), bv.view(np.uint32)
    return out
