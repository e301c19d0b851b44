"""Scenes with point lights and the constant environment, shared by the oracle's own tests (test_oracle_emitters.py) and the
device tests that hold the emitters to it (test_gpu_point_lights.py, test_gpu_environment_emitter.py,
test_gpu_emitter_parity.py). Plain scene builders: no fixtures, nothing that needs a GPU."""
import copy

import numpy as np

# ---------------------------------------------------------------- closed forms on one diffuse plane
W, H_CAM, FOV = 48, 3.0, 45.0
RHO, SKY = np.array([0.2, 0.5, 0.8]), np.array([2.0, 3.0, 5.0])
H_POINT, INTENSITY = 0.7, np.array([2.0, 3.0, 5.0])


def sky_plane(pkg, point_below=None):
    """One diffuse square [-1, 1]^2 in z = 0 (normal +z) under the sky, seen by a pinhole straight above. point_below = p: the
    sky takes sampling weight p, and a point light under the square (which can never light it) takes 1 - p."""
    sc = pkg.scenes
    sd = sc.SceneData("sky_plane")
    sd.rectangle(np.eye(4), sd.diffuse(*RHO))
    if point_below is None:
        sd.constant_environment(tuple(SKY))
    else:
        sd.constant_environment(tuple(SKY), sampling_weight=point_below)
        sd.point_light((0.0, 0.0, -0.5), intensity=(50.0, 50.0, 50.0), sampling_weight=1.0 - point_below)
    sd.set_camera(sc.lookat((0, 0, H_CAM), (0, 0, 0), (0, 1, 0)), FOV, W, W)
    return sd


def point_plane(pkg):
    """The same square under a point light at height H_POINT on the camera axis."""
    sc = pkg.scenes
    sd = sc.SceneData("point_plane")
    sd.rectangle(np.eye(4), sd.diffuse(*RHO))
    sd.point_light((0.0, 0.0, H_POINT), intensity=tuple(INTENSITY))
    sd.set_camera(sc.lookat((0, 0, H_CAM), (0, 0, 0), (0, 1, 0)), FOV, W, W)
    return sd


def plane_coords(g):
    """World (x, y) on the plane of each splat's film position, and the masks of the splats clearly on / off the square."""
    scale = H_CAM * 2.0 * np.tan(np.radians(FOV) / 2) / W
    wx, wy = (g["x"] - W / 2) * scale, (W / 2 - g["y"]) * scale        # film rows run down the world's y
    inside = (np.abs(wx) < 1 - 1e-3) & (np.abs(wy) < 1 - 1e-3)
    outside = (np.abs(wx) > 1 + 1e-3) | (np.abs(wy) > 1 + 1e-3)
    assert inside.sum() > 8192 and outside.sum() > 1000
    return wx, wy, inside, outside


# ---------------------------------------------------------------- the sky as a closed box of area lights
R_BOX = 6.0


def boxed(pkg, sd_sky):
    """The sky replaced by six inward-facing black rectangles of radiance L that enclose the scene and the camera. A ray that
    leaves the scene hits the box; under directTracing = false (camera rays and escapes after delta vertices add nothing, in
    both scenes) the expected f(u) of the two scenes is the same. Their MIS weights differ point by point."""
    sc = pkg.scenes
    sd = sc.SceneData(sd_sky.name + "_boxed")
    sd.shapes = [copy.copy(s) for s in sd_sky.shapes]
    sd.bsdfs = [copy.copy(b) for b in sd_sky.bsdfs]
    env = [i for i, e in enumerate(sd_sky.emitters) if e.type == pkg.abi.EMITTER_CONSTANT]
    assert len(env) == 1 and env[0] == len(sd_sky.emitters) - 1
    sd.emitters = [copy.copy(e) for e in sd_sky.emitters[:-1]]
    L = tuple(sd_sky.emitters[-1].radiance)
    black = sd.diffuse(0.0)
    R = R_BOX
    faces = [sc.translate(0, -R, 0) @ sc.rotate("x", -90), sc.translate(0, R, 0) @ sc.rotate("x", 90),
             sc.translate(0, 0, -R), sc.translate(0, 0, R) @ sc.rotate("y", 180),
             sc.translate(-R, 0, 0) @ sc.rotate("y", 90), sc.translate(R, 0, 0) @ sc.rotate("y", -90)]
    for m in faces:
        m = m @ sc.scale(R)
        n = m[:3, :3] @ np.array([0.0, 0.0, 1.0])
        assert np.dot(n, -m[:3, 3]) > 0        # faces the inside
        sd.rectangle(m, black, radiance=L)
    sd.camera = sd_sky.camera
    assert np.all(np.abs(np.array(sd.camera.to_world)[[3, 7, 11]]) < R)
    return sd


# ---------------------------------------------------------------- a point light as the limit of a vanishing sphere light
def limit_pair(pkg, name):
    """(scene with a point light, scene with a black sphere of radius r in its place whose area emitter has radiance
    I / (pi r^2), the same emitter index and the same sampling weight). The proxy's own error is first order in r (oracle
    against oracle on cornell_point, q99 of the relative luminance error: 6.6e-3 at r = 1e-3, 6.0e-4 at 1e-4), so r = 1e-5
    leaves the tolerance to the device."""
    sc = pkg.scenes
    r = 1e-5

    def build(point):
        if name == "cornell_point":
            sd = sc.cornell_point(32, quad_light=True, point_weight=3.0)
            pos, inten, w = sd.points[0], tuple(sd.emitters[1].radiance), 3.0
            if not point:                                          # rebuild without it, then the proxy as emitter 1
                sd = sc.cornell_c2(32)
        elif name == "door":
            sd = sc.door_c3(32)
            pos, inten, w = (0.4, 0.3, 0.4), (1.5, 1.2, 0.8), 1.0
        else:
            sd = sc.triangle_soup(2000, 32)
            pos, inten, w = (0.1, 0.8, 0.2), (3.0, 2.5, 2.0), 2.0
        if point:
            if name != "cornell_point":
                sd.point_light(pos, intensity=inten, sampling_weight=w)
        else:
            black = sd.diffuse(0.0)
            sd.sphere(pos, r, black, radiance=tuple(v / (np.pi * r * r) for v in inten))
            sd.emitters[-1].sampling_weight = w
        return sd

    return build(True), build(False)


# ---------------------------------------------------------------- scenes lit by the new emitters
def rough_sky(pkg, res=32):
    """C2's room open at the front with a rough-conductor floor under the sky: the light sample's power heuristic matters."""
    sc = pkg.scenes
    sd = sc.SceneData("rough_sky")
    white = sd.diffuse(0.725, 0.71, 0.68)
    red = sd.diffuse(0.63, 0.065, 0.05)
    green = sd.diffuse(0.14, 0.45, 0.091)
    copper = sd.roughconductor(alpha=0.2)
    sd.rectangle(sc.translate(0, -1, 0) @ sc.rotate("x", -90), copper)
    sc._room(sd, white, red, green, walls=("ceiling", "back", "left", "right"))
    sd.box(sc.translate(-0.33, -0.4, -0.3) @ sc.rotate("y", 17) @ sc.scale(0.3, 0.6, 0.3), white)
    sd.constant_environment((1.0, 0.9, 0.8))
    sd.set_camera(sc.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, pkg.abi.FILTER_BOX, 0.5)
    return sd


def glass_sphere_sky(pkg, res=32):
    """Dielectric vertices: refN is zero there, and an escape after a delta sample has lumPdf = 0."""
    sd = pkg.scenes.glass_sphere(res)
    sd.constant_environment((0.8, 0.9, 1.0), sampling_weight=2.0)
    return sd


def mixed(pkg, res=32):
    """cornell_sky with its quad light, two point lights and uneven weights: emitters [quad 1.0, sky 0.7, point 2.5, point 0.4].
    The last point light sits behind the back wall: from the back wall a light sample towards it lands on the wall's back
    side, from everywhere else the wall occludes it."""
    sd = pkg.scenes.cornell_sky(res, quad_light=True, env_weight=0.7)
    sd.point_light((-0.3, 0.7, 0.1), intensity=(2.0, 1.6, 1.2), sampling_weight=2.5)
    sd.point_light((0.2, 0.3, -1.3), intensity=(6.0, 6.0, 6.0), sampling_weight=0.4)
    return sd


def soup(pkg, res=32):
    """triangle_soup(2000) (open at the front, like C2's room) with a point light and the sky: the scene traversed through the BVH."""
    sd = pkg.scenes.triangle_soup(2000, res)
    sd.point_light((0.1, 0.8, 0.2), intensity=(3.0, 2.5, 2.0), sampling_weight=2.0)
    sd.constant_environment((0.6, 0.7, 0.9), sampling_weight=0.5)
    return sd


def door_point(pkg, res=32):
    """Config 3's closed room (rough-conductor floor, hidden quad light) with a point light in the camera's half."""
    sd = pkg.scenes.door_c3(res)
    sd.point_light((0.4, 0.3, 0.4), intensity=(1.5, 1.2, 0.8))
    return sd


EMITTER_SCENES = {
    "cornell_sky": lambda pkg: pkg.scenes.cornell_sky(32),
    "cornell_sky_quad": lambda pkg: pkg.scenes.cornell_sky(32, quad_light=True, env_weight=0.5),
    "glass_sphere_sky": glass_sphere_sky,
    "rough_sky": rough_sky,
    "cornell_point_quad": lambda pkg: pkg.scenes.cornell_point(32, quad_light=True, point_weight=3.0),
    "door_point": door_point,
    "mixed": mixed,
    "soup": soup,
}
