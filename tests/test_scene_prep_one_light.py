"""The first light's joined record in the parameter block (csrc/scene_prep.h: DParams::light, DParams::light_shade) and the
predicate that lets k_mutate_v4's one-light builds read it (csrc/device_types.h: scene_has_one_light), checked on the CPU.
tests/native/one_light_harness.cpp runs prepare_scene on a scene file written by SceneData.save() and prints the record beside
the table entries it must copy, byte for byte, and the predicate."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
PRIM_TRIANGLE, PRIM_RECTANGLE, PRIM_SPHERE, PRIM_POINT, PRIM_ENV = 0, 1, 2, 4, 5
DBG_ONE_LIGHT_GENERIC = 4096


def two_lights(scenes, res=64):
    """cornell_c2 plus a second quad light on the ceiling (emitter 1): still diffuse polygons only, the V4_F0 class"""
    sd = scenes.cornell_c2(res)
    sd.rectangle(scenes.translate(0.5, 0.99, 0.5) @ scenes.rotate("x", 90) @ scenes.scale(0.1), 3, radiance=(5.0, 5.0, 5.0))
    return sd


def no_lights(scenes):
    sd = scenes.cornell_c2(64)
    sd.emitters = []
    for s in sd.shapes:
        s.emitter = -1
    return sd


def triangle_light(scenes):
    sd = scenes.cornell_c1(64)
    sd.emitters = []
    sd.shapes.pop()
    sd.triangle((-0.25, 0.98, -0.25), (0.25, 0.98, -0.25), (0.0, 0.98, 0.25), 2, radiance=15.0)
    return sd


def sphere_light(scenes):
    sd = scenes.cornell_c1(64)
    sd.emitters = []
    sd.shapes.pop()
    sd.sphere((0.0, 0.7, 0.0), 0.1, 2, radiance=15.0)
    return sd


@pytest.fixture(scope="module")
def light(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("one_light")
    exe = str(d / "one_light_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "one_light_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(sd, knobs=None):
        scene = str(d / "scene.drmlt")
        sd.save(scene)
        r = subprocess.run([exe, "scene=" + scene] + ["%s=%s" % kv for kv in (knobs or {}).items()], check=True, capture_output=True, text=True, env=env)
        out = json.loads(r.stdout)
        assert out["sizeof_params_mod_8"] == 0   # the block is copied in 8-byte words (kernel_common.h: load_params)
        return out
    return run


def assert_joined(out):
    assert out["refusal"] == "" and out["n_emitters"] >= 1
    assert len(out["light"]) == 2 * 32 and len(out["light_shade"]) == 2 * 64
    assert out["light"] == out["emitter0"]
    assert out["light_shade"] == out["shade_of_emitter0"]


def test_cornell_c2_has_one_light(pkg, light):
    out = light(pkg.scenes.cornell_c2(64))
    assert_joined(out)
    assert out["n_emitters"] == 1 and out["kind"] == PRIM_RECTANGLE and out["features"] == 0
    assert out["one_light"] == 1


def test_a_triangle_light_counts(pkg, light):
    out = light(triangle_light(pkg.scenes))
    assert_joined(out)
    assert out["n_emitters"] == 1 and out["kind"] == PRIM_TRIANGLE and out["one_light"] == 1


def test_the_debug_bit_clears_the_predicate(pkg, light):
    out = light(pkg.scenes.cornell_c2(64), {"DRMLT_ONE_LIGHT_GENERIC": "1"})
    assert_joined(out)   # the record is filled whatever the knob says
    assert out["debug"] & DBG_ONE_LIGHT_GENERIC and out["one_light"] == 0
    assert light(pkg.scenes.cornell_c2(64))["debug"] & DBG_ONE_LIGHT_GENERIC == 0


def test_no_emitters(pkg, light):
    out = light(no_lights(pkg.scenes))
    assert out["refusal"] == "scene has no emitters"
    assert out["n_emitters"] == 0 and out["one_light"] == 0
    assert out["light"] == "00" * 32 and out["light_shade"] == "00" * 64


def test_two_quad_lights(pkg, light):
    out = light(two_lights(pkg.scenes))
    assert_joined(out)
    assert out["n_emitters"] == 2 and out["features"] == 0 and out["kind"] == PRIM_RECTANGLE
    assert out["one_light"] == 0


@pytest.mark.parametrize("scene,kind", [("cornell_point", PRIM_POINT), ("cornell_sky", PRIM_ENV)])
def test_lights_the_straight_line_step_does_not_sample(pkg, light, scene, kind):
    out = light(getattr(pkg.scenes, scene)(64))
    assert_joined(out)
    assert out["n_emitters"] == 1 and out["kind"] == kind
    assert out["one_light"] == 0


def test_a_sphere_light_does_not_count(pkg, light):
    out = light(sphere_light(pkg.scenes))
    assert_joined(out)
    assert out["n_emitters"] == 1 and out["kind"] == PRIM_SPHERE and out["one_light"] == 0
