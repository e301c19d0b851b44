"""Synthetic scenes (the reference ships none: README.md:155-160 links external downloads).

Every builder returns a SceneData whose .struct() is the flat drmlt_scene the C-ABI takes
(include/drmlt_abi.h). Geometry conventions are Mitsuba's: a `rectangle` is the local square
[-1,1]^2 in the z=0 plane with normal +z under a toWorld transform
(reference src/shapes/rectangle.cpp:80-112); cameras use Transform::lookAt and a horizontal fov.
All constants are deterministic.
"""
import ctypes as C
import math
import os

import numpy as np

from . import abi


# ---- small transform helpers (4x4, column-vector convention) --------------------------------
def translate(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def scale(x, y=None, z=None):
    y = x if y is None else y
    z = x if z is None else z
    return np.diag([x, y, z, 1.0])


def rotate(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    m = np.eye(4)
    if axis == "x":
        m[1, 1], m[1, 2], m[2, 1], m[2, 2] = c, -s, s, c
    elif axis == "y":
        m[0, 0], m[0, 2], m[2, 0], m[2, 2] = c, s, -s, c
    else:
        m[0, 0], m[0, 1], m[1, 0], m[1, 1] = c, -s, s, c
    return m


def lookat(origin, target, up):
    """Mitsuba's Transform::lookAt: columns (left, newUp, dir, origin)."""
    o, t, u = (np.asarray(v, dtype=np.float64) for v in (origin, target, up))
    d = t - o
    d /= np.linalg.norm(d)
    left = np.cross(u, d)
    left /= np.linalg.norm(left)
    new_up = np.cross(d, left)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = left, new_up, d, o
    return m


POINTS_TAG = 0x53544E50  # "PNTS": the point-light block of a scene file (SceneData.save)
NORMALS_TAG = 0x534D524E  # "NRMS": the vertex-normal block


class SceneData:
    def __init__(self, name):
        self.name = name
        self.shapes, self.bsdfs, self.emitters = [], [], []
        self.points = []   # positions of the point lights (drmlt_scene.points)
        self.normals = []  # vertex normals of the smooth triangles, nine floats each (drmlt_scene.normals)
        self.camera = abi.Camera()
        self._keep = None

    # -- materials
    def diffuse(self, r, g=None, b=None):
        g = r if g is None else g
        b = r if b is None else b
        m = abi.Bsdf()
        m.type = abi.BSDF_DIFFUSE
        m.rgb[:] = (r, g, b)
        self.bsdfs.append(m)
        return len(self.bsdfs) - 1

    def dielectric(self, int_ior=1.5046, ext_ior=1.000277):
        m = abi.Bsdf()
        m.type = abi.BSDF_DIELECTRIC
        m.rgb[:] = (1, 1, 1)
        m.p[0], m.p[1] = int_ior, ext_ior
        self.bsdfs.append(m)
        return len(self.bsdfs) - 1

    def roughconductor(self, alpha=0.1, eta=(0.2004, 0.9240, 1.1022), k=(3.9129, 2.4528, 2.1421), ggx=False,
                       reflectance=(1, 1, 1)):
        m = abi.Bsdf()
        m.type = abi.BSDF_ROUGHCONDUCTOR
        m.rgb[:] = reflectance
        m.p[0] = alpha
        m.p[1], m.p[2], m.p[3] = eta
        m.p[4], m.p[5], m.p[6] = k
        m.p[7] = 1.0 if ggx else 0.0
        self.bsdfs.append(m)
        return len(self.bsdfs) - 1

    def conductor(self, eta=(0.2004, 0.9240, 1.1022), k=(3.9129, 2.4528, 2.1421), specular_reflectance=1.0):
        """Mitsuba `conductor` (src/bsdfs/conductor.cpp): the perfect mirror with the exact conductor Fresnel term. eta and k
        are relative to the exterior (already divided by extEta); the defaults are roughconductor's copper."""
        m = abi.Bsdf()
        m.type = abi.BSDF_CONDUCTOR
        m.rgb[:] = specular_reflectance if hasattr(specular_reflectance, "__len__") else (specular_reflectance,) * 3
        m.p[1], m.p[2], m.p[3] = eta
        m.p[4], m.p[5], m.p[6] = k
        self.bsdfs.append(m)
        return len(self.bsdfs) - 1

    # -- shapes
    def _emit(self, radiance):
        e = abi.Emitter()
        e.type = abi.EMITTER_AREA
        e.shape = len(self.shapes)
        e.radiance[:] = radiance if hasattr(radiance, "__len__") else (radiance,) * 3
        e.sampling_weight = 1.0
        self.emitters.append(e)
        return len(self.emitters) - 1

    def rectangle(self, to_world, bsdf, radiance=None):
        s = abi.Shape()
        s.type = abi.SHAPE_RECTANGLE
        s.bsdf = bsdf
        s.emitter = self._emit(radiance) if radiance is not None else -1
        s.data[:] = np.asarray(to_world, dtype=np.float64)[:3, :].reshape(-1)
        self.shapes.append(s)
        return len(self.shapes) - 1

    def triangle(self, p0, p1, p2, bsdf, radiance=None, normals=None):
        """normals: the three vertex normals (at p0, p1, p2) of a smooth-shaded triangle, handed on as they are -- Mitsuba
        interpolates them as stored and normalises only the sum (skdtree.h:355-396). None: the face normal. technique=path only."""
        s = abi.Shape()
        s.type = abi.SHAPE_TRIANGLE
        s.bsdf = bsdf
        s.emitter = self._emit(radiance) if radiance is not None else -1
        s.data[:9] = list(p0) + list(p1) + list(p2)
        if normals is not None:
            vn = np.asarray(normals, dtype=np.float64).reshape(9)
            self.normals.append(tuple(float(v) for v in vn))
            s.normals = len(self.normals)
        self.shapes.append(s)
        return len(self.shapes) - 1

    def sphere(self, center, radius, bsdf, radiance=None):
        s = abi.Shape()
        s.type = abi.SHAPE_SPHERE
        s.bsdf = bsdf
        s.emitter = self._emit(radiance) if radiance is not None else -1
        s.data[:4] = list(center) + [radius]
        self.shapes.append(s)
        return len(self.shapes) - 1

    def point_light(self, position, intensity=1.0, sampling_weight=1.0):
        """Mitsuba `point` emitter (src/emitters/point.cpp): intensity in W/sr, default (1, 1, 1) (Spectrum::getD65() in RGB
        builds). Takes the next emitter index, so the sampling order is the order of the calls. technique=path only."""
        e = abi.Emitter()
        e.type = abi.EMITTER_POINT
        e.shape = len(self.points)
        e.radiance[:] = intensity if hasattr(intensity, "__len__") else (intensity,) * 3
        e.sampling_weight = sampling_weight
        self.points.append(tuple(float(v) for v in position))
        self.emitters.append(e)
        return len(self.emitters) - 1

    def constant_environment(self, radiance=1.0, sampling_weight=1.0):
        """Mitsuba `constant` emitter (src/emitters/constant.cpp): radiance seen by every ray that leaves the scene, default
        (1, 1, 1) (Spectrum::getD65() in RGB builds). It has no shape (`shape` = -1) and takes the next emitter index, so its
        place in the sampling order is the order of the calls. At most one per scene; technique=path only."""
        e = abi.Emitter()
        e.type = abi.EMITTER_CONSTANT
        e.shape = -1
        e.radiance[:] = radiance if hasattr(radiance, "__len__") else (radiance,) * 3
        e.sampling_weight = sampling_weight
        self.emitters.append(e)
        return len(self.emitters) - 1

    def box(self, to_world, bsdf):
        """Mitsuba `cube`: [-1,1]^3 under to_world, 12 outward-facing triangles."""
        m = np.asarray(to_world, dtype=np.float64)
        v = np.array([[x, y, z, 1.0] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]) @ m.T
        v = v[:, :3]
        quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
        for a, b, c, d in quads:
            self.triangle(v[a], v[b], v[c], bsdf)
            self.triangle(v[a], v[c], v[d], bsdf)

    def set_camera(self, to_world, fov_x_deg, width, height, filt=abi.FILTER_BOX, filter_param=0.5,
                   near=1e-2, far=1e4):
        c = self.camera
        c.to_world[:] = np.asarray(to_world, dtype=np.float64).reshape(-1)
        c.fov_x_deg, c.near_clip, c.far_clip = fov_x_deg, near, far
        c.width, c.height, c.filter, c.filter_param = width, height, filt, filter_param

    def save(self, path):
        """Flat binary scene file read by the C++ host (host/drmlt_integrator.hpp: SceneFile::load). Point lights follow the
        camera as a trailing block ("PNTS", count, xyz float32 each), written only when there are any: a scene without them
        gives the same bytes as before the block existed. The vertex normals follow in the same way ("NRMS", count, nine float32
        each), only when there are any."""
        import struct as _st
        with open(path, "wb") as f:
            f.write(_st.pack("<8I", 0x4C4D5244, abi.ABI_VERSION, len(self.shapes), len(self.bsdfs), len(self.emitters),
                             C.sizeof(abi.Shape), C.sizeof(abi.Bsdf), C.sizeof(abi.Emitter)))
            for group in (self.shapes, self.bsdfs, self.emitters):
                for item in group:
                    f.write(bytes(item))
            f.write(bytes(self.camera))
            if self.points:
                f.write(_st.pack("<2I", POINTS_TAG, len(self.points)))
                f.write(np.asarray(self.points, dtype="<f4").tobytes())
            if self.normals:
                f.write(_st.pack("<2I", NORMALS_TAG, len(self.normals)))
                f.write(np.asarray(self.normals, dtype="<f4").tobytes())

    @classmethod
    def load(cls, path, name=None):
        """The scene of a file that save() wrote (or the C++ side, in the same format): SceneFile::load's twin."""
        import struct as _st
        raw = open(path, "rb").read()
        hdr = _st.unpack_from("<8I", raw, 0)
        if hdr[0] != 0x4C4D5244 or hdr[1] != abi.ABI_VERSION or hdr[5:8] != (C.sizeof(abi.Shape), C.sizeof(abi.Bsdf), C.sizeof(abi.Emitter)):
            raise ValueError("malformed scene file %s" % path)
        sd = cls(name or os.path.basename(path))
        off = 32
        for group, T, n in ((sd.shapes, abi.Shape, hdr[2]), (sd.bsdfs, abi.Bsdf, hdr[3]), (sd.emitters, abi.Emitter, hdr[4])):
            if off + n * C.sizeof(T) > len(raw):
                raise ValueError("malformed scene file %s" % path)
            group.extend((T * n).from_buffer_copy(raw, off))
            off += n * C.sizeof(T)
        if off + C.sizeof(abi.Camera) > len(raw):
            raise ValueError("malformed scene file %s" % path)
        sd.camera = abi.Camera.from_buffer_copy(raw, off)
        off += C.sizeof(abi.Camera)
        while off < len(raw):   # optional tagged blocks, points before normals
            if off + 8 > len(raw):
                raise ValueError("malformed scene file %s" % path)
            tag, n = _st.unpack_from("<2I", raw, off)
            off += 8
            per = {POINTS_TAG: 3, NORMALS_TAG: 9}.get(tag)
            dst = sd.points if tag == POINTS_TAG else sd.normals
            if per is None or dst or (tag == POINTS_TAG and sd.normals) or off + 4 * per * n > len(raw):
                raise ValueError("malformed scene file %s" % path)
            vals = np.frombuffer(raw, dtype="<f4", count=per * n, offset=off).reshape(n, per)
            dst.extend(tuple(float(v) for v in row) for row in vals)
            off += 4 * per * n
        return sd

    def struct(self):
        sh = (abi.Shape * len(self.shapes))(*self.shapes)
        bs = (abi.Bsdf * len(self.bsdfs))(*self.bsdfs)
        em = (abi.Emitter * max(1, len(self.emitters)))(*self.emitters)
        s = abi.Scene()
        s.struct_size = C.sizeof(abi.Scene)
        s.n_shapes, s.n_bsdfs, s.n_emitters = len(self.shapes), len(self.bsdfs), len(self.emitters)
        s.shapes = C.cast(sh, C.POINTER(abi.Shape))
        s.bsdfs = C.cast(bs, C.POINTER(abi.Bsdf))
        s.emitters = C.cast(em, C.POINTER(abi.Emitter))
        s.camera = self.camera
        pts = (C.c_float * max(3, 3 * len(self.points)))(*[v for p in self.points for v in p])
        s.n_points = len(self.points)
        s.points = C.cast(pts, C.POINTER(C.c_float))
        nrm = (C.c_float * max(9, 9 * len(self.normals)))(*[v for n in self.normals for v in n])
        s.n_normals = len(self.normals)
        s.normals = C.cast(nrm, C.POINTER(C.c_float))
        self._keep = (sh, bs, em, pts, nrm)
        return s


def _room(sd, white, red, green, walls=("floor", "ceiling", "back", "left", "right")):
    t = {
        "floor": (translate(0, -1, 0) @ rotate("x", -90), white),
        "ceiling": (translate(0, 1, 0) @ rotate("x", 90), white),
        "back": (translate(0, 0, -1), white),
        "left": (translate(-1, 0, 0) @ rotate("y", 90), red),
        "right": (translate(1, 0, 0) @ rotate("y", -90), green),
    }
    for w in walls:
        sd.rectangle(t[w][0], t[w][1])


def cornell_c1(res=256, filt=abi.FILTER_BOX):
    """floor + back wall diffuse quads + one area-light quad, pinhole fov 39 deg."""
    sd = SceneData("cornell_c1")
    grey = sd.diffuse(0.5)
    red = sd.diffuse(0.63, 0.065, 0.05)
    black = sd.diffuse(0.0)
    sd.rectangle(translate(0, -1, 0) @ rotate("x", -90), grey)
    sd.rectangle(translate(0, 0, -1), red)
    sd.rectangle(translate(0, 0.98, 0) @ rotate("x", 90) @ scale(0.25), black, radiance=15.0)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.0, res, res, filt,
                  0.5 if filt == abi.FILTER_BOX else 0.5)
    return sd


def cornell_c2(res=512, filt=abi.FILTER_BOX):
    """5 wall quads + tall and short box (24 triangles) + light quad."""
    sd = SceneData("cornell_c2")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    _room(sd, white, red, green)
    sd.box(translate(-0.33, -0.4, -0.3) @ rotate("y", 17) @ scale(0.3, 0.6, 0.3), white)
    sd.box(translate(0.33, -0.7, 0.3) @ rotate("y", -17) @ scale(0.3, 0.3, 0.3), white)
    sd.rectangle(translate(0, 0.995, 0) @ rotate("x", 90) @ scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, filt, 0.5)
    return sd


def glass_sphere(res=128):
    """Dielectric sphere above a diffuse floor inside the box, quad light (technique=path variant of C5)."""
    sd = SceneData("glass_sphere")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    glass = sd.dielectric(1.5, 1.0)
    _room(sd, white, red, green)
    sd.sphere((0.0, -0.55, 0.1), 0.3, glass)
    sd.rectangle(translate(0, 0.995, 0) @ rotate("x", 90) @ scale(0.15), black, radiance=40.0)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, abi.FILTER_BOX, 0.5)
    return sd


def door_c3(res=256, ggx=False):
    """closed room, partition wall with a 5 % gap hiding a quad light, rough-conductor floor."""
    sd = SceneData("door_c3")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    copper = sd.roughconductor(alpha=0.1, ggx=ggx)
    sd.rectangle(translate(0, -1, 0) @ rotate("x", -90), copper)                      # floor: glossy metal
    _room(sd, white, red, green, walls=("ceiling", "back", "left", "right"))
    sd.rectangle(translate(0, 0, 1) @ rotate("y", 180), white)                        # front wall (room is closed)
    # partition at z = -0.4 leaving a 0.1-wide gap at the right wall (5 % of the room width); two one-sided faces
    sd.rectangle(translate(-0.05, 0, -0.4) @ scale(0.95, 1, 1), white)                # faces the camera room
    sd.rectangle(translate(-0.05, 0, -0.42) @ rotate("y", 180) @ scale(0.95, 1, 1), white)  # faces the light room
    sd.rectangle(translate(-0.3, 0.2, -0.99) @ scale(0.3), black, radiance=40.0)      # light on the back wall
    sd.set_camera(lookat((0, -0.2, 0.95), (0, -0.3, -0.4), (0, 1, 0)), 70.0, res, res, abi.FILTER_BOX, 0.5)
    return sd


def mirror_room(res=256):
    """door_c3's closed room (no partition) with a smooth copper floor (Mitsuba `conductor`) and the quad light on the ceiling:
    the walls are seen a second time in the floor, and the floor throws a reflected caustic of the light onto them."""
    sd = SceneData("mirror_room")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    copper = sd.conductor()
    sd.rectangle(translate(0, -1, 0) @ rotate("x", -90), copper)                      # floor: polished metal
    _room(sd, white, red, green, walls=("ceiling", "back", "left", "right"))
    sd.rectangle(translate(0, 0, 1) @ rotate("y", 180), white)                        # front wall (room is closed)
    sd.rectangle(translate(0, 0.995, -0.2) @ rotate("x", 90) @ scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(lookat((0, -0.2, 0.95), (0, -0.3, -0.4), (0, 1, 0)), 70.0, res, res, abi.FILTER_BOX, 0.5)
    return sd


def triangle_soup(n_tris=2000, res=128, seed=7, smooth=False):
    """Closed room filled with small random diffuse triangles: a scene large enough that the BVH matters. smooth: every triangle
    carries vertex normals, each jittered about the face normal (by less than 44 degrees, unnormalised); the geometry is the same."""
    rng = np.random.default_rng(seed)
    nrng = np.random.default_rng([seed, 1])   # the normals' own stream: the triangles do not depend on the flag
    sd = SceneData("soup_%d" % n_tris)
    white = sd.diffuse(0.7)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    _room(sd, white, red, green)
    mats = [white, red, green]
    for i in range(n_tris):
        c = rng.uniform(-0.85, 0.85, 3)
        c[1] = rng.uniform(-0.95, 0.5)
        e1 = rng.normal(size=3) * 0.06
        e2 = rng.normal(size=3) * 0.06
        vn = None
        if smooth:
            fn = np.cross(e1, e2)
            fn /= np.linalg.norm(fn)
            vn = (fn + nrng.uniform(-0.4, 0.4, (3, 3))) * nrng.uniform(0.5, 2.0, (3, 1))
        sd.triangle(c, c + e1, c + e2, mats[i % 3], normals=vn)
    sd.rectangle(translate(0, 0.995, 0) @ rotate("x", 90) @ scale(0.3), black, radiance=20.0)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, abi.FILTER_BOX, 0.5)
    return sd


def icosphere(level=1):
    """Unit icosphere: (vertices [n, 3], faces [m, 3]) after `level` subdivisions (20 * 4^level faces), outward winding. On the
    unit sphere a vertex is its own radial normal."""
    g = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
         (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(p, dtype=np.float64) / math.sqrt(1.0 + g * g) for p in v]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    return np.asarray(verts), np.asarray(faces, dtype=np.int64)


def smooth_room(res=64, level=1, smooth=True):
    """mirror_room's closed room with a diffuse floor and an icosphere (20 * 4^level triangles, radius 0.35) standing on it,
    shaded with its radial vertex normals. smooth=False: the faceted twin, the same triangles with face normals."""
    sd = SceneData("smooth_room" if smooth else "faceted_room")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    _room(sd, white, red, green)
    sd.rectangle(translate(0, 0, 1) @ rotate("y", 180), white)                        # front wall (room is closed)
    verts, faces = icosphere(level)
    centre, radius = np.array([0.0, -0.65, -0.4]), 0.35
    for a, b, c in faces:
        vn = (verts[a], verts[b], verts[c]) if smooth else None
        sd.triangle(centre + radius * verts[a], centre + radius * verts[b], centre + radius * verts[c], white, normals=vn)
    sd.rectangle(translate(0, 0.995, -0.2) @ rotate("x", 90) @ scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(lookat((0, -0.2, 0.95), (0, -0.3, -0.4), (0, 1, 0)), 70.0, res, res, abi.FILTER_BOX, 0.5)
    return sd


def caustic_c5(res=128):
    """SURVEY 8(d) C5 with the small SPHERE area light (the reference rejects point lights under mmlt, A11):
    dielectric sphere (eta 1.5, r 0.3) above the diffuse floor, emissive sphere r 0.06 under the ceiling, and a
    second, dimmer quad light so that emitter selection is exercised."""
    sd = SceneData("caustic_c5")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    glass = sd.dielectric(1.5, 1.0)
    _room(sd, white, red, green)
    sd.sphere((0.0, -0.55, 0.1), 0.3, glass)
    sd.sphere((0.25, 0.7, 0.0), 0.06, black, radiance=(300.0, 260.0, 200.0))
    sd.rectangle(translate(-0.6, 0.995, -0.4) @ rotate("x", 90) @ scale(0.1), black, radiance=12.0)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, abi.FILTER_BOX, 0.5)
    return sd


def cornell_point(res=512, filt=abi.FILTER_BOX, quad_light=False, point_weight=1.0):
    """C2's box lit by a point light under the ceiling (BASELINE config 5 names a point light; technique=path).
    quad_light: keep C2's ceiling quad light as well, emitter 0 -- the point light (sampling weight `point_weight`) is
    emitter 1."""
    sd = SceneData("cornell_point")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    _room(sd, white, red, green)
    sd.box(translate(-0.33, -0.4, -0.3) @ rotate("y", 17) @ scale(0.3, 0.6, 0.3), white)
    sd.box(translate(0.33, -0.7, 0.3) @ rotate("y", -17) @ scale(0.3, 0.3, 0.3), white)
    if quad_light:
        sd.rectangle(translate(0, 0.995, 0) @ rotate("x", 90) @ scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.point_light((0.0, 0.8, 0.0), intensity=(4.0, 3.2, 2.0), sampling_weight=point_weight)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, filt, 0.5)
    return sd


def cornell_sky(res=512, filt=abi.FILTER_BOX, quad_light=False, env_weight=1.0):
    """C2's room, open at the front, under a constant sky of radiance (0.9, 1.0, 1.2) (technique=path): light reaches the room
    through the opening. quad_light: keep C2's ceiling quad light as well, emitter 0 -- the sky (sampling weight `env_weight`)
    is then emitter 1."""
    sd = SceneData("cornell_sky")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    black = sd.diffuse(0.0)
    _room(sd, white, red, green)
    sd.box(translate(-0.33, -0.4, -0.3) @ rotate("y", 17) @ scale(0.3, 0.6, 0.3), white)
    sd.box(translate(0.33, -0.7, 0.3) @ rotate("y", -17) @ scale(0.3, 0.3, 0.3), white)
    if quad_light:
        sd.rectangle(translate(0, 0.995, 0) @ rotate("x", 90) @ scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.constant_environment((0.9, 1.0, 1.2), sampling_weight=env_weight)
    sd.set_camera(lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, filt, 0.5)
    return sd


def deep_chain(res=64, n=160):
    """C2 plus `n` geometrically shrinking triangles: SAH peels a few of them per level, a chain more than 20 levels deep. A test
    scene (the traversal stacks' overflow area), not one of SCENES."""
    sd = cornell_c2(res)
    white = 0
    for i in range(n):
        s = 0.7 * 0.5 ** (i * 0.3)        # down to 2e-15: areas stay representable in fp32
        x = 0.9 * 0.5 ** (i * 0.3)        # clustered towards the origin, where fp32 keeps resolving them
        sd.triangle((x, 0.0, 0.0), (x + 0.3 * s, 0.0, 0.0), (x, 0.3 * s, 0.1 * s), white)
    return sd


SCENES = {"cornell_c1": cornell_c1, "cornell_c2": cornell_c2, "glass_sphere": glass_sphere, "door_c3": door_c3, "mirror_room": mirror_room,
          "triangle_soup": triangle_soup, "caustic_c5": caustic_c5, "cornell_point": cornell_point, "cornell_sky": cornell_sky,
          "smooth_room": smooth_room}
