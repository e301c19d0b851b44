"""Scenes and closed forms for the vertex-normal tests (tests/test_gpu_smooth_normals.py). Plain builders: no fixtures, nothing
that needs a GPU. The closed-form scenes share direct_scenes' camera: at (0, 0, 3), looking down -z at the origin, 32 x 32."""
import numpy as np

import direct_scenes as ds

RES = ds.RES
FOV = 30.0
RHO = np.array([0.2, 0.5, 0.8])
LIGHT = np.array([0.3, 0.4, 1.2])
INTEN = np.array([2.0, 3.0, 5.0])
TILT = np.radians(20.0)
TILTED = np.array([np.sin(TILT) * np.cos(0.7), np.sin(TILT) * np.sin(0.7), np.cos(TILT)])   # 20 degrees off +z
# one triangle that overfills the view, three different unnormalised vertex normals (each within 35 degrees of +z)
BIG_TRI = np.array([(-3.0, -3.0, 0.0), (3.0, -3.0, 0.0), (0.0, 3.0, 0.0)])
BIG_TRI_NORMALS = np.array([(0.5, 0.1, 1.0), (-0.6, 0.4, 2.0), (0.1, -0.3, 0.5)])
# the small triangle light: edge 1e-5 at a distance of at least 1.2 from the plane, outside the camera's view, facing down. (One
# light sample sees ONE point of the light, not its mean: against the light's centroid a single f(u) is off to first order in
# size / distance, 2e-5 here; only the mean over the light is off to second order.)
LAMP_CENTRE = np.array([0.9, 0.4, 1.2])
LAMP_SIZE = 1e-5
LAMP_RADIANCE = np.array([2.0e10, 3.0e10, 5.0e10])
# a light beside the view whose vertex normals point exactly along -x, the axis a dummy tangent would lie on
SIDE_LAMP_CENTRE = np.array([1.5, 0.4, 1.2])
SIDE_LAMP_NORMAL = np.array([-1.0, 0.0, 0.0])
LAMP_NORMAL = np.array([np.sin(TILT) * np.cos(2.1), np.sin(TILT) * np.sin(2.1), -np.cos(TILT)])   # 20 degrees off -z


def _f32(a):
    """What the device is given: the values rounded to fp32, as fp64."""
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def tilted_pair(pkg, normal=TILTED):
    """A diffuse square in z = 0 that overfills the view, as two triangles whose vertex normals all equal `normal`; one point light."""
    sc = pkg.scenes
    sd = sc.SceneData("tilted_pair")
    rho = sd.diffuse(*RHO)
    a, b, c, d = (-2.0, -2.0, 0.0), (2.0, -2.0, 0.0), (2.0, 2.0, 0.0), (-2.0, 2.0, 0.0)
    vn = None if normal is None else (normal,) * 3
    sd.triangle(a, b, c, rho, normals=vn)
    sd.triangle(a, c, d, rho, normals=vn)
    sd.point_light(tuple(LIGHT), intensity=tuple(INTEN))
    sd.set_camera(sc.lookat(ds.CAM, (0, 0, 0), (0, 1, 0)), FOV, RES, RES)
    return sd


def big_triangle(pkg, normals=BIG_TRI_NORMALS):
    """One diffuse triangle in z = 0 that overfills the view, with three different vertex normals; the same light."""
    sc = pkg.scenes
    sd = sc.SceneData("big_triangle")
    sd.triangle(*BIG_TRI, sd.diffuse(*RHO), normals=normals)
    sd.point_light(tuple(LIGHT), intensity=tuple(INTEN))
    sd.set_camera(sc.lookat(ds.CAM, (0, 0, 0), (0, 1, 0)), FOV, RES, RES)
    return sd


def plane_points(pkg, x, y, fov=FOV):
    """Where the camera rays through the film positions (x, y), in pixels, meet z = 0: (n, 3), fp64 (perspective.cpp:271-286)."""
    cam = pkg.scenes.lookat(ds.CAM, (0, 0, 0), (0, 1, 0))
    th = np.tan(np.radians(fov) / 2)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dl = np.stack([(1 - 2 * x / RES) * th, (1 - 2 * y / RES) * th, np.ones_like(x)], axis=1)
    dl /= np.linalg.norm(dl, axis=1)[:, None]
    d = dl @ cam[:3, :3].T
    o = np.asarray(ds.CAM, dtype=np.float64)
    return o[None, :] + (-o[2] / d[:, 2])[:, None] * d


def interpolated_normals(p, tri, vn):
    """skdtree.h:355-396 in fp64: normalize(n0 b0 + n1 b1 + n2 b2) at the points p of the triangle `tri`, the vertex normals as stored."""
    tri, vn = _f32(tri), _f32(vn)
    e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
    m = np.stack([e1[:2], e2[:2]], axis=1)                       # the triangles here lie in z = 0
    uv = np.linalg.solve(m, (p[:, :2] - tri[0, :2]).T).T
    b = np.stack([1 - uv[:, 0] - uv[:, 1], uv[:, 0], uv[:, 1]], axis=1)
    n = b @ vn
    return n / np.linalg.norm(n, axis=1)[:, None], b


def point_lit_closed_form(p, n):
    """f = rho / pi * I * (n_s . omega) / d^2 at the points p with shading normals n: ((n, 3) rgb, n_s . omega)."""
    lv = _f32(LIGHT)[None, :] - p
    d2 = (lv * lv).sum(axis=1)
    cos = (lv * n).sum(axis=1) / np.sqrt(d2)
    return (_f32(RHO) / np.pi * _f32(INTEN))[None, :] * (cos / d2)[:, None], cos


def view_corners_cos(pkg, tri, vn, fov=FOV):
    """min over the view of n_s . omega. The shading normal of a planar triangle and omega both vary smoothly and slowly over the
    view: a 65 x 65 grid of film positions, corners and edges included, bounds the minimum to well within the margin asked."""
    g = np.linspace(0.0, RES, 65)
    x, y = (a.reshape(-1) for a in np.meshgrid(g, g))
    p = plane_points(pkg, x, y, fov)
    n, b = interpolated_normals(p, tri, vn)
    return point_lit_closed_form(p, n)[1].min(), b.min()


# ---- the smooth emitter
def lamp_triangle(centre=LAMP_CENTRE):
    """Vertices of the small light: an equilateral triangle of edge LAMP_SIZE about LAMP_CENTRE in the plane z = 1.2, wound so that
    its face normal points down."""
    r = LAMP_SIZE / np.sqrt(3.0)
    ang = np.radians([90.0, 330.0, 210.0])                        # clockwise seen from above: (p1 - p0) x (p2 - p0) points to -z
    return np.asarray(centre, dtype=np.float64)[None, :] + r * np.stack([np.cos(ang), np.sin(ang), np.zeros(3)], axis=1)


def lamp_lit_plane(pkg, normal=LAMP_NORMAL, fov=FOV, centre=LAMP_CENTRE):
    """A diffuse square in z = 0 (a rectangle: flat) that overfills the view, lit by the small triangle light whose vertex
    normals all equal `normal` (None: its face normal)."""
    sc = pkg.scenes
    sd = sc.SceneData("lamp_lit_plane")
    sd.rectangle(sc.scale(5.0), sd.diffuse(*RHO))
    tri = lamp_triangle(centre)
    sd.triangle(tri[0], tri[1], tri[2], sd.diffuse(0.0), radiance=tuple(LAMP_RADIANCE), normals=None if normal is None else (normal,) * 3)
    sd.set_camera(sc.lookat(ds.CAM, (0, 0, 0), (0, 1, 0)), fov, RES, RES)
    return sd


def lamp_closed_form(p, normal=LAMP_NORMAL, centre=LAMP_CENTRE):
    """f = rho / pi * L * A * cos theta_l (shading) * cos theta / d^2 at the plane points p, the light taken as a point at its
    centroid: a single light sample is off by up to 2 size / distance = 2e-5 relative, the mean over the light by its square. (n, 3)."""
    tri = _f32(lamp_triangle(centre))
    area = 0.5 * np.linalg.norm(np.cross(tri[1] - tri[0], tri[2] - tri[0]))
    nl = _f32(normal)
    nl = nl / np.linalg.norm(nl)
    lv = tri.mean(axis=0)[None, :] - p
    d2 = (lv * lv).sum(axis=1)
    w = lv / np.sqrt(d2)[:, None]
    cos_l = np.maximum(-(w @ nl), 0.0)
    cos_p = w[:, 2]
    return (_f32(RHO) / np.pi * _f32(LAMP_RADIANCE))[None, :] * (area * cos_l * cos_p / d2)[:, None]


def lamp_pixels_closed_form(pkg, fov, sub=16, normal=LAMP_NORMAL, centre=LAMP_CENTRE):
    """Pixel values of render_direct on lamp_lit_plane: the mean of the closed form over the pixel, (RES, RES, 3)."""
    d = ds.camera_dirs(pkg, fov, sub)
    o = np.asarray(ds.CAM)
    p = (o + d * (-o[2] / d[..., 2])[..., None]).reshape(-1, 3)
    return lamp_closed_form(p, normal, centre).reshape(RES, RES, sub * sub, 3).mean(axis=2)


# ---- the face-normal twin
def face_normal_twin(pkg, sd, split_emitters=True):
    """The same scene with every triangle shaded by vertex normals that all equal its own face normal (fp64, rounded to fp32), so
    that the device takes the smooth branch on every hit and computes what it computed before. Rectangles become the two triangles
    (a, b, c), (a, c, d) -- an emitting rectangle two emitters of equal weight and area, the same density -- so that the scenes
    that have no triangles get them. An oracle that never reads the normals sees the triangulated, faceted scene.
    split_emitters=False keeps an emitting rectangle whole: the light samples then map u to the same points as the original's."""
    sc, abi = pkg.scenes, pkg.abi
    tw = sc.SceneData(sd.name + "_twin")
    tw.bsdfs = [abi.Bsdf.from_buffer_copy(bytes(b)) for b in sd.bsdfs]
    tw.camera = abi.Camera.from_buffer_copy(bytes(sd.camera))
    assert not sd.points and all(e.type == abi.EMITTER_AREA for e in sd.emitters)

    def add(p0, p1, p2, s):
        p = _f32([p0, p1, p2])
        fn = np.cross(p[1] - p[0], p[2] - p[0])
        fn /= np.linalg.norm(fn)
        rad = tuple(sd.emitters[s.emitter].radiance) if s.emitter >= 0 else None
        tw.triangle(p0, p1, p2, s.bsdf, radiance=rad, normals=(fn,) * 3)
        if s.emitter >= 0:
            tw.emitters[-1].sampling_weight = sd.emitters[s.emitter].sampling_weight

    for s in sd.shapes:
        d = np.array(list(s.data), dtype=np.float64)
        if s.type == abi.SHAPE_TRIANGLE:
            add(d[0:3], d[3:6], d[6:9], s)
        elif s.type == abi.SHAPE_RECTANGLE and (split_emitters or s.emitter < 0):
            m = d.reshape(3, 4)
            corner = lambda x, y: m[:, 3] + x * m[:, 0] + y * m[:, 1]
            a, b, c, e = corner(-1, -1), corner(1, -1), corner(1, 1), corner(-1, 1)
            add(a, b, c, s)
            add(a, c, e, s)
        else:
            c = abi.Shape.from_buffer_copy(bytes(s))
            if s.emitter >= 0:
                em = abi.Emitter.from_buffer_copy(bytes(sd.emitters[s.emitter]))
                em.shape = len(tw.shapes)
                c.emitter = len(tw.emitters)
                tw.emitters.append(em)
            tw.shapes.append(c)
    return tw


def faceted(pkg, sd):
    """The same scene without its vertex normals."""
    abi = pkg.abi
    tw = pkg.scenes.SceneData(sd.name + "_faceted")
    tw.bsdfs, tw.emitters, tw.points, tw.camera = sd.bsdfs, sd.emitters, sd.points, sd.camera
    for s in sd.shapes:
        c = abi.Shape.from_buffer_copy(bytes(s))
        c.normals = 0
        tw.shapes.append(c)
    return tw
