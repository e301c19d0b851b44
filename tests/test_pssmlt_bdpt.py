"""algo=pssmlt over technique=bdpt, what a machine without a GPU can check: drmlt_create accepts the combination (and still refuses
technique=mmlt), launch_plan.h plans its builds, and the compiler's resource remarks of k_mutate_pssmlt_bdpt keep it at two waves
per SIMD. The chains themselves: tests/test_gpu_pssmlt_bdpt.py."""
import json
import os
import subprocess

import pytest

from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_create_accepts_pssmlt_over_bdpt(pkg, abi, native_lib):
    sd = pkg.scenes.cornell_c2(8)
    for nodirect in (0, 1):
        cfg = abi.make_config(algo=abi.ALGO_PSSMLT, technique="bdpt", max_depth=6, rr_depth=4, work_units=64, no_direct_sampling=nodirect)
        if _has_gpu():
            ctx = pkg.Context(cfg, sd)
            assert ctx.stats().n_chains == 64
            ctx.close()
        else:
            with pytest.raises(pkg.DrmltError) as e:
                pkg.Context(cfg, sd)
            assert "no HIP device" in str(e.value), str(e.value)   # past every refusal of the configuration and the scene


def test_pssmlt_over_mmlt_is_still_refused(pkg, abi, native_lib):
    with pytest.raises(pkg.DrmltError) as e:
        pkg.Context(abi.make_config(algo=abi.ALGO_PSSMLT, technique="mmlt", max_depth=5, work_units=64), pkg.scenes.cornell_c2(8))
    assert "technique=path" in str(e.value) and "technique=bdpt" in str(e.value) and "mmlt" in str(e.value)
    # the limits of technique=bdpt hold for this loop as they do for the delayed-rejection one
    with pytest.raises(pkg.DrmltError, match="maxDepth above 24"):
        pkg.Context(abi.make_config(algo=abi.ALGO_PSSMLT, technique="bdpt", max_depth=25, work_units=64), pkg.scenes.cornell_c2(8))


# PlanInputs of bench.py's bdpt scene (tests/test_launch_plan.py: BD), directSampling on (eff_dim = S + E + Dd) and off
B = 512 * 512
BD = dict(technique=1, features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=72, max_depth=8, mmlt_S=22, mmlt_E=20, budget=B * 256)
BD_NODIRECT = dict(BD, eff_dim=42)
BVH = dict(features=8, use_bvh=1, bvh_stack16=1)
PB, PB_NODIRECT = dict(BD, algo=1), dict(BD_NODIRECT, algo=1)

# (name, PlanInputs, environment, (build, chains, LDS bytes))
CASES = [
    ("derived: 65 536 chains, one wave per SIMD", PB, {}, ("PSSMLT_BDPT_F7", 65536, 19712)),
    ("derived, no direct sampling", PB_NODIRECT, {}, ("PSSMLT_BDPT_F7", 65536, 19712)),
    ("derived, bvh", dict(PB, **BVH), {}, ("PSSMLT_BDPT_F15", 65536, 19712)),
    ("derived, bvh, no direct sampling", dict(PB_NODIRECT, **BVH), {}, ("PSSMLT_BDPT_F15", 65536, 19712)),
    ("budget caps the count", dict(PB, budget=64 * 64 * 100), {}, ("PSSMLT_BDPT_F7", 6400, 19712)),
    ("131 072 chains: two waves per SIMD, tables in LDS", dict(PB, work_units=131072), {}, ("PSSMLT_BDPT_F7_OCC2_TABLES", 131072, 20000)),
    ("131 072 chains, no direct sampling", dict(PB_NODIRECT, work_units=131072), {}, ("PSSMLT_BDPT_F7_OCC2_TABLES", 131072, 20000)),
    ("131 072 chains, bvh", dict(PB, work_units=131072, **BVH), {}, ("PSSMLT_BDPT_F15", 131072, 19712)),
    ("tables global", dict(PB, work_units=131072), {"DRMLT_BDPT_TABLES_GLOBAL": "1"}, ("PSSMLT_BDPT_F7_OCC2", 131072, 19712)),
    ("1280 waves", dict(PB, work_units=81920), {}, ("PSSMLT_BDPT_F7", 81920, 19712)),
    ("1281 waves", dict(PB, work_units=81984), {}, ("PSSMLT_BDPT_F7_OCC2_TABLES", 81984, 20000)),
    ("occ 1", dict(PB, work_units=131072), {"DRMLT_BDPT_OCC": "1"}, ("PSSMLT_BDPT_F7", 131072, 19712)),
    ("maxDepth 9: LDS above 20480", dict(PB, max_depth=9, mmlt_S=24, mmlt_E=22, work_units=131072), {}, ("PSSMLT_BDPT_F7", 131072, 21760)),
    # existing plans, unchanged (rows of tests/test_launch_plan.py)
    ("drmlt bench bdpt", dict(BD, work_units=131072), {}, ("BDPT_F7_OCC2_TABLES", 131072, 20000)),
    ("drmlt derived bdpt", BD, {}, ("BDPT_F7_OCC2_TABLES", 131072, 20000)),
    ("drmlt bdpt bvh", dict(BD, work_units=131072, **BVH), {}, ("BDPT_F15", 131072, 19712)),
    ("drmlt bdpt 1280 waves", dict(BD, work_units=81920), {}, ("BDPT_F7", 81920, 19712)),
    ("pssmlt over path", dict(features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=34, max_depth=8, budget=B * 256, algo=1), {}, ("PSSMLT", 65536, 8704)),
]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "pssmlt_bdpt_plan_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "pssmlt_bdpt_plan_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(inputs, knobs):
        args = ["%s=%d" % kv for kv in inputs.items()] + ["%s=%s" % kv for kv in knobs.items()]
        return json.loads(subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout)
    return run


@pytest.mark.parametrize("name,inputs,knobs,want", CASES, ids=[c[0] for c in CASES])
def test_plan(plan, name, inputs, knobs, want):
    p = plan(inputs, knobs)
    assert (p["build"], p["chains"], p["lds"]) == want, p
    assert p["grid"] == (p["chains"] + 63) // 64, p
    if inputs.get("technique"):   # bootstrap, seed replay and evaluation kernels: the rows without the staged tables (288 B)
        assert p["aux_lds"] == p["lds"] - (288 if p["build"].endswith("_TABLES") else 0), p
    assert p["note"] == "" and not p["run_ahead"] and not p["rows_mem"], p


def test_kernel_resources(native_lib):
    """Every build of k_mutate_pssmlt_bdpt fits 256 registers, the builds compiled for two waves per SIMD get them, and the build with
    its tables in LDS has no static LDS (no traversal stack), like k_mutate_bdpt<7, 2, true>."""
    k = kernels(os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources"))
    mine = {n: r for n, r in k.items() if n.startswith("_Z20k_mutate_pssmlt_bdptILi")}
    assert sorted(mine) == ["_Z20k_mutate_pssmlt_bdptILi15ELi1ELb0EEv7DParamsjj", "_Z20k_mutate_pssmlt_bdptILi7ELi1ELb0EEv7DParamsjj",
                            "_Z20k_mutate_pssmlt_bdptILi7ELi2ELb0EEv7DParamsjj", "_Z20k_mutate_pssmlt_bdptILi7ELi2ELb1EEv7DParamsjj"]
    for n, r in mine.items():
        assert r["VGPRs"] + r["AGPRs"] <= 256, (n, r)
        if "ELi2ELb" in n:
            assert r["Occupancy"] >= 2, (n, r)
    assert mine["_Z20k_mutate_pssmlt_bdptILi7ELi2ELb1EEv7DParamsjj"]["LDS"] == 0
    assert mine["_Z20k_mutate_pssmlt_bdptILi7ELi2ELb0EEv7DParamsjj"]["LDS"] == 0 and mine["_Z20k_mutate_pssmlt_bdptILi15ELi1ELb0EEv7DParamsjj"]["LDS"] > 0


def test_standalone_host_reads_the_integrator(native_lib):
    """drmlt_render: integrator=pssmlt|drmlt (default drmlt) and kelemenStyleMutation reach the configuration, so the combination
    is reachable without Python."""
    host = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)

    def check(**kw):
        args = [os.path.join(host, "drmlt_render"), "--check"] + [a for k, v in kw.items() for a in ("-D", "%s=%s" % (k, v))]
        p = subprocess.run(args, capture_output=True, text=True)
        return p.returncode, dict(t.split("=") for t in p.stdout.split()), p.stderr

    rc, kv, _ = check(integrator="pssmlt", technique="bdpt", maxDepth=6, kelemenStyleMutation="false")   # PSSMLT has no `type`
    assert rc == 0 and (kv["integrator"], kv["technique"], kv["kelemenStyleMutation"], kv["kelemenStyleWeights"]) == ("pssmlt", "1", "0", "1")
    rc, kv, _ = check(technique="bdpt", type="orbital", maxDepth=6)
    assert rc == 0 and (kv["integrator"], kv["kelemenStyleMutation"]) == ("drmlt", "1")
    rc, _, err = check(technique="bdpt", maxDepth=6)
    assert rc == 1 and '"type" has not been specified' in err
    rc, _, err = check(integrator="mlt", technique="bdpt", type="orbital")
    assert rc == 1 and "Unknown integrator" in err
