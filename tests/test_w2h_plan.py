"""Which k_mutate_w2 launches run k_mutate_w2h instead (csrc/launch_plan.h: w2_held_launch, ChainPlan::w2_held), checked on the CPU
through tests/native/w2h_plan_harness.cpp. The kernel holds the scene's ray records in vector registers and has room for three
cuboids and one flat record, tested without the plain-triangle arm: the plan offers it where `w2` holds, the scene has one to
three cuboids, at most one flat record beside them and no plain triangle, and DRMLT_NO_W2_HELD is unset. `lds` and `grid` are
the same with and without it."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")

B = 512 * 512
C2 = dict(features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=34, max_depth=8, budget=B * 256, work_units=65536)  # bench.py's Cornell box


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("w2hplan") / "w2h_plan_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "w2h_plan_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(inputs, knobs=None):
        args = ["%s=%d" % kv for kv in inputs.items()] + ["%s=%s" % kv for kv in (knobs or {}).items()]
        return json.loads(subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout)
    return run


@pytest.mark.parametrize("n_box,n_flat_rec,has_plain_tri,held", [
    (3, 1, 0, 1),   # bench.py's Cornell box: three cuboids and the light
    (1, 1, 0, 1),   # a room and its light
    (3, 0, 0, 1),   # cuboids only
    (0, 3, 0, 0),   # cornell_c1: no cuboid, three flat records -- keeps streaming
    (4, 1, 0, 0),   # a fourth cuboid has no slot
    (3, 2, 0, 0),   # nor a second flat record
    (3, 1, 1, 0),   # a plain triangle needs test_flat<true>
])
def test_selection_by_the_record_counts(plan, n_box, n_flat_rec, has_plain_tri, held):
    p = plan(dict(C2, n_box=n_box, n_flat_rec=n_flat_rec, has_plain_tri=has_plain_tri))
    assert p["v4_f0"] == 1 and p["w2"] == 1
    assert p["w2_held"] == held and p["fits"] == held
    assert p["lds"] == 20000 and p["grid"] == 2048   # what tests/test_w2_plan.py pins for the headline: unchanged


def test_knob_keeps_k_mutate_w2(plan):
    p = plan(dict(C2, n_box=3, n_flat_rec=1), {"DRMLT_NO_W2_HELD": "1"})
    assert p["w2"] == 1 and p["fits"] == 1 and p["w2_held"] == 0
    assert p["lds"] == 20000 and p["grid"] == 2048


@pytest.mark.parametrize("inputs,knobs", [
    (dict(C2), {"DRMLT_NO_W2": "1"}),                                                       # the twin
    (dict(C2, eff_dim=10, max_depth=3, work_units=98272), {"DRMLT_KERNEL": "4"}),           # a third wave per SIMD is possible
    (dict(C2), {"DRMLT_DEBUG": "128"}),                                                     # V4_F0_STAMPS
    (dict(C2, features=1), {}),                                                             # V4_F3
    (dict(C2, work_units=131072), {}),                                                      # k_mutate_v5
], ids=["no_w2", "third_wave", "stamps", "V4_F3", "v5"])
def test_never_without_w2(plan, inputs, knobs):
    p = plan(dict(inputs, n_box=3, n_flat_rec=1), knobs)
    assert p["fits"] == 1 and p["w2"] == 0 and p["w2_held"] == 0
