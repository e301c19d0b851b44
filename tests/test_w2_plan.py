"""Which launches may run k_mutate_w2 (csrc/launch_plan.h: w2_launch, ChainPlan::w2), checked on the CPU through
tests/native/w2_plan_harness.cpp. The kernel is compiled for two waves per SIMD, so the plan offers it only where a third wave
cannot be resident: the workgroup's LDS exceeds a twelfth of a compute unit's 160 KB (13 653 bytes), or the grid has at most
two waves per SIMD (8 per compute unit). launch_mutate adds the two conditions it reads from the parameter block (orbital
rule, one light)."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")

B = 512 * 512
C2 = dict(features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=34, max_depth=8, budget=B * 256)  # bench.py's Cornell box
# the same scene at max_depth 3: 10 dimensions, 10 496 B of LDS per wave -- twelve waves fit a compute unit
SHALLOW = dict(C2, eff_dim=10, max_depth=3)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("w2plan") / "w2_plan_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "w2_plan_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(inputs, knobs=None):
        args = ["%s=%d" % kv for kv in inputs.items()] + ["%s=%s" % kv for kv in (knobs or {}).items()]
        return json.loads(subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout)
    return run


def test_headline_is_selected(plan):
    """Cornell at 65 536 chains: 20 000 B of LDS per wave caps a compute unit at eight waves, whatever the grid"""
    p = plan(dict(C2, work_units=65536))
    assert p["v4_f0"] == 1 and p["lds"] == 20000 and p["grid"] == 2048
    assert p["lds"] * 12 > 160 * 1024
    assert p["w2"] == 1


def test_third_wave_possible_is_not_selected(plan):
    """LDS for twelve waves per compute unit AND a grid of more than two waves per SIMD: the twin keeps its third wave"""
    p = plan(dict(SHALLOW, work_units=98272), {"DRMLT_KERNEL": "4"})
    assert p["v4_f0"] == 1 and p["lds"] == 10496 and p["lds"] * 12 <= 160 * 1024 and p["grid"] == 3071 > 256 * 8
    assert p["w2"] == 0 and p["no_third_wave"] == 0


def test_small_grid_is_selected_whatever_the_lds(plan):
    """the same LDS on a grid of exactly two waves per SIMD, and one wave beyond it"""
    p = plan(dict(SHALLOW, work_units=256 * 8 * 32), {"DRMLT_KERNEL": "4"})
    assert p["grid"] == 256 * 8 and p["w2"] == 1
    p = plan(dict(SHALLOW, work_units=256 * 8 * 32 + 1), {"DRMLT_KERNEL": "4"})
    assert p["grid"] == 256 * 8 + 1 and p["w2"] == 0
    p = plan(dict(SHALLOW, work_units=256 * 8 * 32 + 1, cus=304), {"DRMLT_KERNEL": "4"})
    assert p["w2"] == 1  # a larger device: still at most two waves per SIMD


def test_knob_switches_it_off(plan):
    p = plan(dict(C2, work_units=65536), {"DRMLT_NO_W2": "1"})
    assert p["v4_f0"] == 1 and p["no_third_wave"] == 1 and p["w2"] == 0


@pytest.mark.parametrize("inputs,knobs", [
    (dict(C2, work_units=65536), {"DRMLT_DEBUG": "128"}),   # V4_F0_STAMPS: the stamps stay k_mutate_v4's
    (dict(C2, features=1, work_units=65536), {}),            # V4_F3
    (dict(C2, work_units=131072), {}),                       # k_mutate_v5
    (dict(C2, work_units=65536), {"DRMLT_KERNEL": "3"}),     # k_mutate_v3
], ids=["stamps", "V4_F3", "v5", "v3"])
def test_other_builds_are_never_selected(plan, inputs, knobs):
    p = plan(inputs, knobs)
    assert p["v4_f0"] == 0 and p["w2"] == 0
