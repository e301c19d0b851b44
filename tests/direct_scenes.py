"""Scenes and closed forms for the direct-illumination pass (tests/test_gpu_direct.py). Plain builders: no fixtures, nothing that
needs a GPU. The closed-form scenes share one camera: at (0, 0, 3), looking down -z at the origin, RES x RES pixels."""
import numpy as np

import conductor_scenes as cs

RES = 32
CAM = (0.0, 0.0, 3.0)
WALL_RADIANCE = np.array([3.0, 1.7, 0.6])
PLANE = dict(fov=40.0, rho=np.array([0.2, 0.5, 0.8]), light=np.array([0.3, 0.4, 1.2]), inten=np.array([2.0, 3.0, 5.0]))
MIRROR = dict(fov=2.0, refl=np.array([0.9, 0.6, 0.3]), radiance=np.array([5.0, 3.0, 2.0]))
PANE = dict(fov=2.0, eta=1.5, behind=np.array([3.0, 0.0, 0.0]), above=np.array([0.0, 6.0, 0.0]))
N45 = np.array([0.0, 1.0, 1.0]) / np.sqrt(2.0)   # normal of the 45 degree mirror / pane through the origin


def _camera(pkg, sd, fov, filt=None):
    sc = pkg.scenes
    sd.set_camera(sc.lookat(CAM, (0, 0, 0), (0, 1, 0)), fov, RES, RES, pkg.abi.FILTER_BOX if filt is None else filt, 0.5)
    return sd


def emitter_wall(pkg, filt=None):
    """An emitting square in z = 0 that faces the camera and overfills its view."""
    sc = pkg.scenes
    sd = sc.SceneData("emitter_wall")
    sd.rectangle(sc.scale(5.0), sd.diffuse(0.0), radiance=tuple(WALL_RADIANCE))
    return _camera(pkg, sd, 40.0, filt)


def lit_plane(pkg):
    """A diffuse square in z = 0 that overfills the view, under one point light."""
    sc = pkg.scenes
    sd = sc.SceneData("lit_plane")
    sd.rectangle(sc.scale(5.0), sd.diffuse(*PLANE["rho"]))
    sd.point_light(tuple(PLANE["light"]), intensity=tuple(PLANE["inten"]))
    return _camera(pkg, sd, PLANE["fov"])


def camera_dirs(pkg, fov, sub):
    """Unit directions of the camera rays through a sub x sub midpoint grid in every pixel: (RES, RES, sub * sub, 3), fp64
    (perspective.cpp:271-286)."""
    cam = pkg.scenes.lookat(CAM, (0, 0, 0), (0, 1, 0))
    th = np.tan(np.radians(fov) / 2)
    off = (np.arange(sub) + 0.5) / sub
    x = (np.arange(RES)[None, :, None, None] + off[None, None, None, :]) + np.zeros((RES, 1, sub, 1))
    y = (np.arange(RES)[:, None, None, None] + off[None, None, :, None]) + np.zeros((1, RES, 1, sub))
    dl = np.stack([(1 - 2 * x / RES) * th, (1 - 2 * y / RES) * th, np.ones_like(x)], axis=-1).reshape(RES, RES, sub * sub, 3)
    dl /= np.linalg.norm(dl, axis=-1, keepdims=True)
    return dl @ cam[:3, :3].T


def lit_plane_closed_form(pkg, sub=16):
    """Pixel values of lit_plane: the mean over the pixel of rho / pi * I * cos(theta) / d^2, (RES, RES, 3)."""
    d = camera_dirs(pkg, PLANE["fov"], sub)
    o = np.asarray(CAM)
    p = o + d * (-o[2] / d[..., 2])[..., None]
    lv = PLANE["light"] - p
    d2 = (lv * lv).sum(-1)
    g = lv[..., 2] / np.sqrt(d2) / d2
    return (PLANE["rho"] / np.pi * PLANE["inten"]) * g.mean(axis=2)[..., None]


def mirrored_light(pkg):
    """Camera -> copper mirror at 45 degrees -> an area light above it that faces down and overfills the mirrored view."""
    sc = pkg.scenes
    sd = sc.SceneData("mirrored_light")
    mirror = sd.conductor(eta=cs.COPPER_ETA, k=cs.COPPER_K, specular_reflectance=tuple(MIRROR["refl"]))
    sd.rectangle(sc.rotate("x", -45) @ sc.scale(2.0), mirror)
    sd.rectangle(sc.translate(0, 2.0, 0) @ sc.rotate("x", 90) @ sc.scale(3.0), sd.diffuse(0.0), radiance=tuple(MIRROR["radiance"]))
    return _camera(pkg, sd, MIRROR["fov"])


def mirrored_light_closed_form(pkg, sub=4):
    """R o F(cos theta) * Le, the mean over the pixel: (RES, RES, 3)."""
    d = camera_dirs(pkg, MIRROR["fov"], sub)
    cos1 = -(d @ N45)
    F = cs.fresnel_conductor_exact(cos1.reshape(-1), cs.COPPER_ETA, cs.COPPER_K).reshape(RES, RES, sub * sub, 3)
    return F.mean(axis=2) * MIRROR["refl"] * MIRROR["radiance"]


def fresnel_dielectric(cos_i, eta):
    """fresnelDielectricExt (src/libcore/util.cpp:659-689) for cos_i > 0, fp64: (F, cos_t)."""
    c = np.asarray(cos_i, dtype=np.float64)
    ct2 = 1.0 - (1.0 - c * c) / (eta * eta)
    ct = np.sqrt(np.maximum(ct2, 0.0))
    rs = (c - eta * ct) / (c + eta * ct)
    rp = (eta * c - ct) / (eta * c + ct)
    return np.where(ct2 <= 0, 1.0, 0.5 * (rs * rs + rp * rp)), ct


def glass_pane(pkg):
    """Camera -> one dielectric interface at 45 degrees. The reflected ray meets a green light above, the refracted ray a red
    light behind; both overfill what the pane shows."""
    sc = pkg.scenes
    sd = sc.SceneData("glass_pane")
    sd.rectangle(sc.rotate("x", -45) @ sc.scale(2.0), sd.dielectric(PANE["eta"], 1.0))
    black = sd.diffuse(0.0)
    sd.rectangle(sc.translate(0, 2.0, 0) @ sc.rotate("x", 90) @ sc.scale(6.0), black, radiance=tuple(PANE["above"]))
    sd.rectangle(sc.translate(0, 0, -3.0) @ sc.scale(6.0), black, radiance=tuple(PANE["behind"]))
    return _camera(pkg, sd, PANE["fov"])


def glass_pane_closed_form(pkg, sub=4):
    """(pixel values F * above + (1 - F) / eta^2 * behind, F per pixel): the radiance scaling of a refracted ray entering the
    medium is 1 / eta^2 (dielectric.cpp:300-306)."""
    d = camera_dirs(pkg, PANE["fov"], sub)
    F, _ = fresnel_dielectric(-(d @ N45), PANE["eta"])
    F = F.mean(axis=2)
    return F[..., None] * PANE["above"] + ((1 - F) / PANE["eta"] ** 2)[..., None] * PANE["behind"], F


def sphere_mask(pkg, sd, centre, radius, sub=8, grow=1.03):
    """Pixels of `sd`'s camera in which some camera ray meets the (slightly grown) sphere: (RES, RES) bool."""
    cam = np.asarray(sd.camera.to_world, dtype=np.float64).reshape(4, 4)
    th = np.tan(np.radians(sd.camera.fov_x_deg) / 2)
    off = (np.arange(sub + 1)) / sub
    x = (np.arange(RES)[None, :, None, None] + off[None, None, None, :]) + np.zeros((RES, 1, sub + 1, 1))
    y = (np.arange(RES)[:, None, None, None] + off[None, None, :, None]) + np.zeros((1, RES, 1, sub + 1))
    dl = np.stack([(1 - 2 * x / RES) * th, (1 - 2 * y / RES) * th, np.ones_like(x)], axis=-1).reshape(RES, RES, -1, 3)
    dl /= np.linalg.norm(dl, axis=-1, keepdims=True)
    d = dl @ cam[:3, :3].T
    oc = cam[:3, 3] - np.asarray(centre, dtype=np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - (radius * grow) ** 2)
    return (disc >= 0).any(axis=2)
