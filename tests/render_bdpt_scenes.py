"""Scenes, closed forms and the host-side film for the render_bdpt tests (tests/test_gpu_render_bdpt.py). Plain builders: no
fixtures, nothing that needs a GPU."""
import numpy as np

import direct_scenes as ds
import normals_scenes as ns

LUMW = np.array([0.212671, 0.715160, 0.072169])
FACE_DOWN = np.array([0.0, 0.0, -1.0])   # face normal of normals_scenes' small triangle light (wound to face the plane)
LAMP_FOV = 30.0


def lum(img):
    return img @ LUMW


# ---- the lamp-lit plane with face normals (technique=bdpt refuses vertex normals)
def lamp_plane(pkg):
    """normals_scenes.lamp_lit_plane without vertex normals: a view-filling diffuse square in z = 0 under the triangle light of
    edge 1e-5 at (0.9, 0.4, 1.2), which faces straight down and lies outside the camera's view. 32 x 32, box filter."""
    sd = ns.lamp_lit_plane(pkg, normal=None, fov=LAMP_FOV)
    assert all(s.normals == 0 for s in sd.shapes)
    return sd


def lamp_plane_closed_form(pkg, sub=16):
    """Pixel values at maxDepth 2: rho / pi * L * A * cos theta_l * cos theta / d^2, the mean over the pixel on a sub x sub grid."""
    return ns.lamp_pixels_closed_form(pkg, LAMP_FOV, sub=sub, normal=FACE_DOWN)


def lamp_is_out_of_view(pkg):
    """The light's three vertices, seen from the camera, lie outside the film (so neither the s = 0, t = 2 nor the s = 1, t = 1
    strategy ever contributes and the image is the closed form's depth-2 light alone): distance of the nearest vertex to the
    film's edge, in units of the film's half-width -- positive means outside."""
    cam = pkg.scenes.lookat(ds.CAM, (0, 0, 0), (0, 1, 0))
    v = (ns.lamp_triangle() - np.asarray(ds.CAM)[None, :]) @ cam[:3, :3]          # camera space (the columns are its axes)
    assert np.all(v[:, 2] > 0)
    th = np.tan(np.radians(LAMP_FOV) / 2)
    return float((np.maximum(np.abs(v[:, 0] / v[:, 2]), np.abs(v[:, 1] / v[:, 2])) / th).min() - 1.0)


def two_rectangles(pkg, res):
    """The smallest scene a context accepts: a diffuse floor and a light above it, on a res x res film."""
    sc = pkg.scenes
    sd = sc.SceneData("two_rectangles")
    sd.rectangle(sc.translate(0, -1, 0) @ sc.rotate("x", -90), sd.diffuse(0.5))
    sd.rectangle(sc.translate(0, 0.98, 0) @ sc.rotate("x", 90) @ sc.scale(0.25), sd.diffuse(0.0), radiance=15.0)
    sd.set_camera(sc.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.0, res, res, pkg.abi.FILTER_BOX, 0.5)
    return sd


def floor_disc_mask(sd, centre_xz, radius, floor_y=-1.0):
    """Pixels of `sd`'s camera whose centre ray meets the plane y = floor_y within `radius` of (x, z) = centre_xz: (res, res) bool.
    (What stands between the camera and the floor is not looked at: take a sphere's own pixels out with direct_scenes.sphere_mask.)"""
    res = sd.camera.width
    cam = np.asarray(sd.camera.to_world, dtype=np.float64).reshape(4, 4)
    th = np.tan(np.radians(sd.camera.fov_x_deg) / 2)
    x, y = np.meshgrid(np.arange(res) + 0.5, np.arange(res) + 0.5)
    dl = np.stack([(1 - 2 * x / res) * th, (1 - 2 * y / res) * th, np.ones_like(x)], axis=-1)
    d = dl @ cam[:3, :3].T
    o = cam[:3, 3]
    t = (floor_y - o[1]) / np.where(d[..., 1] < 0, d[..., 1], -1e-30)
    p = o + d * t[..., None]
    return (d[..., 1] < 0) & ((p[..., 0] - centre_xz[0]) ** 2 + (p[..., 2] - centre_xz[1]) ** 2 < radius ** 2)


# ---- the oracle's lists, splatted on the host
def list_points(cfg, n, seed):
    """n uniform points for bdpt_eval: (u_sensor, u_emitter, u_direct or None), wide enough for every component a path can read."""
    rr = cfg.max_depth + 1 - max(cfg.rr_depth, 0)
    w = max(2 * (cfg.max_depth + 1) + max(rr, 0) + 1, 2 * (2 * cfg.max_depth - 1))
    w += w & 1
    rng = np.random.default_rng(seed)
    us, ue, ud = (rng.random((n, w), dtype=np.float32) for _ in range(3))
    return us, ue, (None if cfg.no_direct_sampling else ud)


def block_contributions(rows, res, block=4):
    """Per-sample contributions to the block means of the box-filtered luminance image: (n, res / block, res / block), fp64. Row
    layout: [lum, hasMain, px, py, r, g, b, nMore, nDims, nRays, nMore x (px, py, r, g, b)]. Every splat lands in the pixel that
    contains it with weight res^2 / n, so the mean over the samples of sample i's array * res^2 / block^2 is the block image.
    film_put's rule is kept: a splat with a negative or non-finite channel is dropped."""
    rows = np.asarray(rows, dtype=np.float64)
    n, nb = len(rows), res // block
    out = np.zeros((n, nb, nb))

    def put(px, py, rgb, on):
        ok = on & np.isfinite(rgb).all(axis=1) & (rgb >= 0).all(axis=1)
        ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
        ok &= (ix >= 0) & (ix < res) & (iy >= 0) & (iy < res)
        i = np.nonzero(ok)[0]
        np.add.at(out, (i, iy[i] // block, ix[i] // block), rgb[i] @ LUMW)

    put(rows[:, 2], rows[:, 3], rows[:, 4:7], rows[:, 1] > 0)
    more = rows[:, 10:].reshape(n, -1, 5)
    for k in range(more.shape[1]):
        put(more[:, k, 0], more[:, k, 1], more[:, k, 2:5], rows[:, 7] > k)
    return out * (res * res / (block * block))


def blocks_of(img, block=4):
    """Block means of an image's luminance: (res / block, res / block)."""
    res = img.shape[0]
    return lum(np.asarray(img, dtype=np.float64)).reshape(res // block, block, res // block, block).mean(axis=(1, 3))
