"""k_mutate_w2h's loop iteration without its scaffolding: the ray pass's tail by selects and its slots behind scalar flag tests
(device_path.h: trace_held, HELD_*), a closed cuboid that skips the `hole` test (test_box<true>), the step without the triangle
light's arm (HeldLightTablesT<true>), the hand-off's copies ahead of its swaps (kernels_v4.hip), the wave's ray test from two
compare masks. None of it changes a floating-point expression
or the order of one, so the three contexts of tests/test_gpu_w2h.py -- default (k_mutate_w2h), DRMLT_NO_W2_HELD=1 (k_mutate_w2,
streaming) and DRMLT_NO_W2=1 (k_mutate_v4's twin) -- must still run the same chains BIT FOR BIT: the chain state rows, cur_*, and
every counter of stats() (test_gpu_w2.assert_same; the chains' own mutation counts enter through `mutations`, the sum the epilogue
writes from them, and through the state a chain that ran more or less would have left).

Films: float atomics of three waves land in an order that differs from run to run. The bound is the one two runs of the twin set
on the same case: test_gpu_w2.assert_same's reordering bound (rtol 160 * 2^-24, worked out for 6144 mutations on 32 x 32 pixels;
5120 mutations on 64 x 64 put fewer splats on a pixel), asked here of a second run of the twin against the first as well as of the
other two kernels against the first.

Cases, each 64 x 64 pixels, 80 chains (two full waves and a half one), 64 mutations per chain in two calls of 32, so that run-ahead
and the epilogue are crossed:
  cornell_c2           three cuboids and the light; the room lacks its front face and the camera stands outside it, so every camera
                       ray is a `hole` lane; the two blocks are closed, their faces triangle pairs (HELD_QUAD2)
  one_box_room         slots 1 and 2 unused; the open room alone, no triangle pair among the records (the tail's sub-triangle arm is
                       skipped by the wave)
  two_box_room         slot 2 unused; an open and a closed cuboid
  camera inside        cornell_c2 seen from z = 0.9: no ray enters the room from outside, no lane is a `hole` lane
  max_depth 2, rr 1    every path ends by depth or roulette within two steps

No case with a light that is not a rectangle: launch_plan.h's w2_held_launch admits none (HeldLightTablesT in device_path.h has the
argument: a triangle that emits stays a plain-triangle flat record, and such a scene keeps streaming). That such a scene runs no
wave of k_mutate_w2h is tests/test_w2h_plan.py's business."""
import pytest

import test_gpu_w2 as w2
from ray_probe import one_box_room, two_box_room
from test_gpu_w2 import assert_same
from test_gpu_w2h import held_waves

pytestmark = pytest.mark.gpu
RES, N_CHAINS, CALLS = 64, 80, [32, 32]
WAVES = 3 * len(CALLS)  # one launch of three waves per call


def camera_inside(scenes, res):
    sd = scenes.cornell_c2(res)
    sd.name = "cornell_c2_inside"
    sd.set_camera(scenes.lookat((0, 0, 0.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, scenes.abi.FILTER_BOX, 0.5)
    return sd


SCENES = {
    "cornell_c2": lambda scenes: scenes.cornell_c2(RES),
    "one_box_room": lambda scenes: one_box_room(scenes, RES),
    "two_box_room": lambda scenes: two_box_room(scenes, RES),
    "camera_inside": lambda scenes: camera_inside(scenes, RES),
}
CASES = [("cornell_c2", {}), ("one_box_room", {}), ("two_box_room", {}), ("camera_inside", {}), ("cornell_c2", dict(max_depth=2, rr_depth=1))]


@pytest.fixture(autouse=True)
def scenes_of_this_file(monkeypatch):
    """test_gpu_w2.run_chains makes its scene by name"""
    monkeypatch.setattr(w2, "make_scene", lambda pkg, scene: SCENES[scene](pkg.scenes))


@pytest.mark.parametrize("scene,kw", CASES, ids=["cornell_c2", "one_box_room", "two_box_room", "camera_inside", "short_paths"])
def test_same_chains_as_the_streamed_kernel_and_the_twin(pkg, native_lib, capfd, scene, kw):
    def run(no_w2, env=None):
        return w2.run_chains(pkg, capfd, scene, CALLS, no_w2, n_chains=N_CHAINS, env=env, type="orbital", **kw)
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
