"""k_mutate_w2h (kernels_v4.hip) is k_mutate_w2 with the scene's ray records -- up to three cuboids and one flat record -- read once
and held in vector registers: its ray pass is trace_held (device_path.h), test_box and test_flat in the streaming loops' order
on the same values, with no memory access. launch_mutate runs it where the plan allows (launch_plan.h: w2_held_launch).

Three contexts run the same chains BIT FOR BIT -- states, f(u) of the current states, every counter of stats(): the default one
(k_mutate_w2h), one under DRMLT_NO_W2_HELD=1 (k_mutate_w2, streaming) and one under DRMLT_NO_W2=1 (k_mutate_v4's twin). Films
are held to the reordering bound of tests/test_gpu_w2.py, whose helpers this file imports.

Which kernel ran is read from the device: a wave of k_mutate_w2h counts itself in stats[16] like k_mutate_w2's and in stats[17],
printed by drmlt_stats_get under DRMLT_VERBOSE as "waves with the ray records held in registers".

The two rooms built here give the cuboid counts cornell_c2 does not: one cuboid (the five walls) and two (an axis-aligned box
inside); the slots beyond the count stay empty and are skipped. That they prepare to those counts is checked on the CPU."""
import re

import pytest

import test_gpu_w2 as w2
from test_gpu_w2 import N_CHAINS, N_MUT, assert_eventful, assert_same
from test_scene_prep import prep  # noqa: F401  (the scene-prep harness fixture)

gpu = pytest.mark.gpu
PATH8 = dict(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=N_CHAINS, sample_count=1, type="orbital")


from ray_probe import one_box_room, two_box_room  # noqa: E402  (the two rooms: one copy, shared with the ray probe)


BUILT = {"one_box_room": one_box_room, "two_box_room": two_box_room}
_stock_make_scene = w2.make_scene


@pytest.fixture(autouse=True)
def built_scenes(monkeypatch):
    """test_gpu_w2.run_chains makes its scene by name: the names of the rooms built here as well"""
    monkeypatch.setattr(w2, "make_scene", lambda pkg, scene: BUILT[scene](pkg.scenes, 32) if scene in BUILT else _stock_make_scene(pkg, scene))


@pytest.mark.parametrize("scene,n_box", [("one_box_room", 1), ("two_box_room", 2)])
def test_the_built_rooms_prepare_to_their_counts(pkg, prep, scene, n_box):  # noqa: F811
    out, _, _ = prep(BUILT[scene](pkg.scenes, 32), PATH8)
    assert out["refusal"] == ""
    P = out["params"]
    assert (P["n_box"], P["n_flat_rec"], P["has_plain_tri"], P["features"], P["n_emitters"]) == (n_box, 1, 0, 0, 1), P


def held_waves(run):
    m = re.search(r"waves with the ray records held in registers: (\d+)", run["log"])
    assert m, run["log"]
    return int(m.group(1))


def three(pkg, capfd, scene, calls, env=None, **kw):
    """default (held), DRMLT_NO_W2_HELD=1 (streamed), DRMLT_NO_W2=1 (k_mutate_v4's twin)"""
    kw.setdefault("type", "orbital")
    held = w2.run_chains(pkg, capfd, scene, calls, False, env=env, **kw)
    streamed = w2.run_chains(pkg, capfd, scene, calls, False, env=dict(env or {}, DRMLT_NO_W2_HELD="1"), **kw)
    twin = w2.run_chains(pkg, capfd, scene, calls, True, env=env, **kw)
    return held, streamed, twin


def check(held, streamed, twin, waves, mutations, eventful=True):
    assert held["w2_waves"] == waves and streamed["w2_waves"] == waves
    assert held_waves(held) == waves, "every wave of the default context ran k_mutate_w2h"
    assert held_waves(streamed) == 0 and held_waves(twin) == 0
    if eventful:
        assert_eventful(held["stats"])
    assert_same(held, twin, mutations)
    assert_same(streamed, twin, mutations)


@gpu
@pytest.mark.parametrize("n_chains", [96, 80], ids=["three_full_waves", "last_wave_half_empty"])
def test_three_cuboids_and_the_light(pkg, native_lib, capfd, n_chains):
    """cornell_c2: what bench.py's flagship line runs"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], n_chains=n_chains)
    check(h, s, t, 3, n_chains * N_MUT)


@gpu
def test_sliced_calls_reload_state_and_records(pkg, native_lib, capfd):
    """two calls in launches of 16 mutations: four launches, each prologue reads the state and the records anew"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT // 2, N_MUT // 2], env={"DRMLT_SLICE": "16"})
    check(h, s, t, 12, N_CHAINS * N_MUT)


@gpu
@pytest.mark.parametrize("kw", [dict(max_depth=2), dict(rr_depth=1)], ids=["max_depth_2", "rr_depth_1"])
def test_short_paths(pkg, native_lib, capfd, kw):
    """paths that end early: PH_FLUSH steps read the hit of a lane whose ray pass ran on whatever its registers held"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], **kw)
    check(h, s, t, 3, N_CHAINS * N_MUT, eventful=False)
    assert h["stats"].accepted > 0 and h["stats"].rays > 0


@gpu
@pytest.mark.parametrize("scene", ["one_box_room", "two_box_room"])
def test_empty_cuboid_slots_are_skipped(pkg, native_lib, capfd, scene):
    h, s, t = three(pkg, capfd, scene, [N_MUT])
    check(h, s, t, 3, N_CHAINS * N_MUT)


@gpu
def test_a_scene_without_cuboids_keeps_streaming(pkg, native_lib, capfd):
    """cornell_c1: three flat records, no cuboid -- k_mutate_w2 runs, no wave holds records"""
    h, t = w2.pair(pkg, capfd, "cornell_c1", [N_MUT], type="orbital")
    assert h["w2_waves"] == 3 and held_waves(h) == 0 and held_waves(t) == 0
    assert h["stats"].accepted > 0
    assert_same(h, t, N_CHAINS * N_MUT)
