"""k_mutate_w2h's ray pass computes the rows of its records component by component (device_path.h: rows_at_point and its
neighbours, test_box<true, true>, box_candidate<true>, test_flat_held): scalar fmaf / multiply chains in the nesting of the packed
expressions the streaming loops keep, and its `hole` test is one compare of a pinned word (held_hole). A packed fused multiply-add
is two independent fused multiply-adds, so no component rounds differently, and the three contexts of tests/test_gpu_w2h.py --
default (k_mutate_w2h), DRMLT_NO_W2_HELD=1 (k_mutate_w2, streaming, packed rows) and DRMLT_NO_W2=1 (k_mutate_v4's twin) -- must
run the same chains BIT FOR BIT: the chain state rows, cur_* and every counter of stats() (test_gpu_w2.assert_same).

Films: float atomics of three waves land in an order that differs from run to run. The bound is the one two runs of the twin
set on the same case: test_gpu_w2.assert_same's reordering bound (rtol 160 * 2^-24, worked out for 6144 mutations on 32 x 32
pixels; these cases run 5120 on 32 x 32), asked of a second run of the twin against the first as well as of the other two
kernels against the first.

The cases are those tests/test_gpu_w2h_iter.py's five do not reach. Each: 32 x 32 pixels, 80 chains (two full waves and a half
one), 64 mutations per chain in two calls of 32.
  front_and_ceiling_open   one_box_room without its ceiling (its front is missing anyway), the camera outside the front. A ray that
                           enters through the missing front and leaves through the missing ceiling must miss: the exit
                           candidate that `hole` merges in has a half-word of its own, and that decides it.
  exit_face_missing        the same room, the camera inside, looking out through the missing front past the right wall and the
                           floor: `inside` lanes whose exit face is missing.
  block_before_the_room    one_box_room and a closed block that stands outside it, between the camera and the opening: a lane
                           without an entry face in the room's slot finds the room's far wall and loses to the block's slot.
Before anything runs on the device, tests/ray_probe.py's fp64 brute force over the scene's shapes says whether a case's camera
rays (one per pixel centre) hold the classes it is there for; a case that degenerates fails instead of passing empty.

Not here: a camera ray exactly parallel to a slab of the room (ld = 0 in test_box, the (-inf, +inf) case of its comment). The
chain kernels make their camera rays from the chain's own primary-sample components, not from pixel centres, so a scene cannot
place one: d.x = 0 needs a component of exactly 0.5. tests/test_gpu_rays.py hands trace_held such rays one by one (its class of
axis-parallel rays, on cornell_c2, one_box_room and two_box_room) and holds them to the streaming loop's words."""
import numpy as np
import pytest

import ray_probe as rp
import test_gpu_w2 as w2
from ray_probe import one_box_room
from test_gpu_w2 import assert_same
from test_gpu_w2h import held_waves

RES, N_CHAINS, CALLS = 32, 80, [32, 32]
WAVES = 3 * len(CALLS)  # one launch of three waves per call
FOV = 39.3077
WALLS = ("floor", "back", "left", "right")


def open_room(scenes, res, name):
    """one_box_room without its ceiling: four walls (still a cuboid: box_merge.h asks for four faces) and the light, which hangs free"""
    sd = scenes.SceneData(name)
    white, red, green, black = sd.diffuse(0.725, 0.71, 0.68), sd.diffuse(0.63, 0.065, 0.05), sd.diffuse(0.14, 0.45, 0.091), sd.diffuse(0.0)
    scenes._room(sd, white, red, green, walls=WALLS)
    sd.rectangle(scenes.translate(0, 0.995, 0) @ scenes.rotate("x", 90) @ scenes.scale(0.25), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(scenes.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), FOV, res, res, scenes.abi.FILTER_BOX, 0.5)
    return sd


def front_and_ceiling_open(scenes, res=RES):
    return open_room(scenes, res, "front_and_ceiling_open")


def exit_face_missing(scenes, res=RES):
    sd = open_room(scenes, res, "exit_face_missing")
    sd.set_camera(scenes.lookat((-0.5, 0, -0.5), (1, -0.6, 1), (0, 1, 0)), FOV, res, res, scenes.abi.FILTER_BOX, 0.5)
    return sd


def block_before_the_room(scenes, res=RES):
    sd = one_box_room(scenes, res)
    sd.name = "block_before_the_room"
    sd.box(scenes.translate(0.2, -0.3, 1.8) @ scenes.scale(0.3, 0.3, 0.3), 0)
    return sd


SCENES = {"front_and_ceiling_open": front_and_ceiling_open, "exit_face_missing": exit_face_missing, "block_before_the_room": block_before_the_room}
N_WALLS = {"front_and_ceiling_open": 4, "exit_face_missing": 4, "block_before_the_room": 5}  # the walls come first, then the light, then the block


def camera_rays(sd, res):
    """path_begin's camera ray through every pixel centre, in fp64 -> origins, directions"""
    m = np.array(sd.camera.to_world[:], dtype=np.float64).reshape(4, 4)
    tan = np.tan(np.radians(0.5 * sd.camera.fov_x_deg))
    v = (np.arange(res) + 0.5) / res
    v0, v1 = (a.reshape(-1) for a in np.meshgrid(v, v))
    dl = np.stack([(1 - 2 * v0) * tan, (1 - 2 * v1) * tan, np.ones_like(v0)], axis=1)   # (square film: inv_aspect = 1)
    dl /= np.linalg.norm(dl, axis=1)[:, None]
    return np.broadcast_to(m[:3, 3], dl.shape).copy(), dl @ m[:3, :3].T


def ray_classes(pkg, name):
    """What the fp64 brute force says of the case's camera rays."""
    sd = SCENES[name](pkg.scenes)
    g = rp.scene_geometry(pkg, sd)
    o, d = camera_rays(sd, RES)
    n = len(o)
    shape, t, p = rp.brute_force(g, o, d, np.full(n, 1e-2), np.full(n, np.inf))
    with np.errstate(divide="ignore", invalid="ignore"):
        at = lambda axis, value: o + ((value - o[:, axis]) / d[:, axis])[:, None] * d     # the ray's point in the plane axis = value
        within = lambda q, axes: np.all(np.abs(q[:, axes]) < 1.0, axis=1)
        front, top = at(2, 1.0), at(1, 1.0)
        through_front = within(front, [0, 1]) & ((1.0 - o[:, 2]) / d[:, 2] > 0)
        through_top = within(top, [0, 2]) & ((1.0 - o[:, 1]) / d[:, 1] > 0)
    in_room = np.all(np.abs(o) < 1.0, axis=1)
    return dict(shape=shape, walls=(shape >= 0) & (shape < N_WALLS[name]), block=shape > N_WALLS[name], miss=shape < 0,
                through_front=through_front, through_top=through_top, in_room=in_room)


def check_front_and_ceiling_open(c):
    assert not c["in_room"].any()
    assert (c["miss"] & c["through_front"] & c["through_top"]).sum() >= 1, "a camera ray enters through the front and leaves through the ceiling"
    assert (c["walls"] & c["through_front"]).sum() >= 1, "a camera ray enters through the front and hits a wall"


def check_exit_face_missing(c):
    assert c["in_room"].all()
    assert (c["miss"] & c["through_front"]).sum() >= 1, "a camera ray leaves the room through the missing front"
    assert c["walls"].sum() >= 1, "a camera ray hits a wall"


def check_block_before_the_room(c):
    assert not c["in_room"].any()
    assert (c["block"] & c["through_front"]).sum() >= 1, "a camera ray aimed at the opening hits the block in front of it"
    assert (c["walls"] & c["through_front"]).sum() >= 1, "a camera ray passes the block and hits a wall"


CHECKS = {"front_and_ceiling_open": check_front_and_ceiling_open, "exit_face_missing": check_exit_face_missing, "block_before_the_room": check_block_before_the_room}


@pytest.fixture(autouse=True)
def scenes_of_this_file(monkeypatch):
    """test_gpu_w2.run_chains makes its scene by name"""
    monkeypatch.setattr(w2, "make_scene", lambda pkg, scene: SCENES[scene](pkg.scenes))


def check_classes(pkg, scene):
    classes = ray_classes(pkg, scene)
    print(scene, {k: int(v.sum()) for k, v in classes.items() if k != "shape"})
    CHECKS[scene](classes)


@pytest.mark.parametrize("scene", list(SCENES))
def test_scenes_hold_their_ray_classes(pkg, scene):
    """no GPU: the fp64 brute force alone"""
    check_classes(pkg, scene)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", list(SCENES))
def test_same_chains_as_the_streamed_kernel_and_the_twin(pkg, native_lib, capfd, scene):
    check_classes(pkg, scene)

    def run(no_w2, env=None):
        return w2.run_chains(pkg, capfd, scene, CALLS, no_w2, n_chains=N_CHAINS, env=env, type="orbital")
    held, streamed, twin, twin_again = run(False), run(False, {"DRMLT_NO_W2_HELD": "1"}), run(True), run(True)
    assert held["w2_waves"] == WAVES and streamed["w2_waves"] == WAVES
    assert held_waves(held) == WAVES, "every wave of the default context ran k_mutate_w2h"
    assert held_waves(streamed) == 0 and held_waves(twin) == 0
    st = held["stats"]
    assert st.accepted > 0 and st.rays > 0 and 0 < st.first_acc < st.first_base
    mutations = N_CHAINS * sum(CALLS)
    assert_same(twin_again, twin, mutations)  # the bound two runs of the twin set
    assert_same(held, twin, mutations)
    assert_same(streamed, twin, mutations)
