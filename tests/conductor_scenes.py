"""Scenes for the smooth conductor tests (plain builders; tests/test_conductor.py, tests/test_gpu_conductor.py)."""
import copy

import numpy as np

COPPER_ETA, COPPER_K = (0.2004, 0.9240, 1.1022), (3.9129, 2.4528, 2.1421)


def fresnel_conductor_exact(cos_i, eta, k):
    """fresnelConductorExact (src/libcore/util.cpp:723-745) in fp64: cos_i of shape (n,), eta and k of shape (3,) -> (n, 3)."""
    c = np.asarray(cos_i, dtype=np.float64)[:, None]
    eta, k = np.asarray(eta, dtype=np.float64)[None, :], np.asarray(k, dtype=np.float64)[None, :]
    c2 = c * c
    s2 = 1.0 - c2
    s4 = s2 * s2
    t1 = eta * eta - k * k - s2
    a2pb2 = np.sqrt(np.maximum(0.0, t1 * t1 + 4.0 * k * k * eta * eta))
    a = np.sqrt(np.maximum(0.0, 0.5 * (a2pb2 + t1)))
    term1, term2 = a2pb2 + c2, 2.0 * a * c
    rs2 = (term1 - term2) / (term1 + term2)
    term3, term4 = a2pb2 * c2 + s4, term2 * s2
    rp2 = rs2 * (term3 - term4) / (term3 + term4)
    return 0.5 * (rp2 + rs2)


# ---- the closed form: camera -> mirror at 45 degrees -> point-lit diffuse plane
MIRROR_PLANE = dict(cam=(0.0, 0.0, 3.0), fov=30.0, W=48, H=2.0, half=1.0, light=(0.3, 1.2, 0.2),
                    rho=(0.2, 0.5, 0.8), inten=(2.0, 3.0, 5.0), refl=(0.9, 0.6, 0.3))


def mirror_plane(pkg):
    """A copper mirror through the origin with normal (0, 1, 1) / sqrt 2 fills the view of a camera on the z axis; what the
    camera sees in it is a diffuse square at y = H that faces down, lit by one point light below it."""
    sc, m = pkg.scenes, MIRROR_PLANE
    sd = sc.SceneData("mirror_plane")
    mirror = sd.conductor(eta=COPPER_ETA, k=COPPER_K, specular_reflectance=m["refl"])
    plane = sd.diffuse(*m["rho"])
    sd.rectangle(sc.rotate("x", -45) @ sc.scale(2.0), mirror)
    sd.rectangle(sc.translate(0, m["H"], 0) @ sc.rotate("x", 90) @ sc.scale(m["half"]), plane)
    sd.point_light(m["light"], intensity=m["inten"])
    sd.set_camera(sc.lookat(m["cam"], (0, 0, 0), (0, 1, 0)), m["fov"], m["W"], m["W"])
    return sd


def mirror_plane_closed_form(pkg, x, y):
    """f at film positions (x, y) in pixels, fp64: (rgb of shape (n, 3), inside, outside), the two masks with a margin of
    1e-3 about the square's edge."""
    sc, m = pkg.scenes, MIRROR_PLANE
    cam = sc.lookat(m["cam"], (0, 0, 0), (0, 1, 0))
    th = np.tan(np.radians(m["fov"]) / 2)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    dl = np.stack([(1 - 2 * x / m["W"]) * th, (1 - 2 * y / m["W"]) * th, np.ones_like(x)], axis=1)   # perspective.cpp:317-343
    dl /= np.linalg.norm(dl, axis=1)[:, None]
    d = dl @ cam[:3, :3].T
    o = np.asarray(m["cam"], dtype=np.float64)
    n = np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)
    t1 = -(o @ n) / (d @ n)
    p1 = o[None, :] + t1[:, None] * d
    cos1 = -(d @ n)
    r = d + 2.0 * cos1[:, None] * n[None, :]
    t2 = (m["H"] - p1[:, 1]) / r[:, 1]
    p2 = p1 + t2[:, None] * r
    lv = np.asarray(m["light"], dtype=np.float64)[None, :] - p2
    d2 = (lv * lv).sum(axis=1)
    cos2 = -lv[:, 1] / np.sqrt(d2)                                     # the square's normal is -y
    F = fresnel_conductor_exact(cos1, COPPER_ETA, COPPER_K) * np.asarray(m["refl"])[None, :]
    f = F * (np.asarray(m["rho"]) / np.pi)[None, :] * np.asarray(m["inten"])[None, :] * (cos2 / d2)[:, None]
    h = m["half"]
    inside = (np.abs(p2[:, 0]) < h - 1e-3) & (np.abs(p2[:, 2]) < h - 1e-3)
    outside = (np.abs(p2[:, 0]) > h + 1e-3) | (np.abs(p2[:, 2]) > h + 1e-3)
    return f, inside, outside


# ---- the oracle's alpha -> 0 limit
def floor_view(pkg, res=32):
    """mirror_room's room seen from a camera that looks down at the smooth copper floor, which fills its view and shows it the
    edge between the back wall and the ceiling. The ceiling light sits to the side, outside what the floor shows the camera:
    no camera ray reaches it over the mirror alone, and the back wall it lights is seen through the mirror."""
    sc = pkg.scenes
    sd = sc.SceneData("floor_view")
    white, red, green, black = sd.diffuse(0.725, 0.71, 0.68), sd.diffuse(0.63, 0.065, 0.05), sd.diffuse(0.14, 0.45, 0.091), sd.diffuse(0.0)
    copper = sd.conductor(eta=COPPER_ETA, k=COPPER_K, specular_reflectance=(0.9, 0.8, 0.7))
    sd.rectangle(sc.translate(0, -1, 0) @ sc.rotate("x", -90), copper)
    sc._room(sd, white, red, green, walls=("ceiling", "back", "left", "right"))
    sd.rectangle(sc.translate(0, 0, 1) @ sc.rotate("y", 180), white)
    sd.rectangle(sc.translate(0.8, 0.995, -0.3) @ sc.rotate("x", 90) @ sc.scale(0.15), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(sc.lookat((0, 0, 0.5), (0, -1, 0), (0, 0, -1)), 20.0, res, res)
    return sd


def rough_twin(pkg, sd, alpha):
    """The same scene with every smooth conductor replaced by a Beckmann rough conductor of roughness alpha (same eta, k and
    reflectance): what the oracle renders."""
    abi = pkg.abi
    tw = copy.copy(sd)
    tw.bsdfs = []
    for b in sd.bsdfs:
        c = abi.Bsdf.from_buffer_copy(bytes(b))
        if c.type == abi.BSDF_CONDUCTOR:
            c.type = abi.BSDF_ROUGHCONDUCTOR
            c.p[0], c.p[7] = alpha, 0.0
        tw.bsdfs.append(c)
    tw._keep = None
    return tw


LIMIT_SCENES = {"floor_view": floor_view, "mirror_room": lambda pkg, res=32: pkg.scenes.mirror_room(res)}
