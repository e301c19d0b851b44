"""The chain-kernel plan (csrc/launch_plan.h), checked on the CPU: which build a configuration gets, with how many chains and how
much LDS. tests/native/plan_harness.cpp runs derive_chains + plan_chains on PlanInputs and an environment of DRMLT_* knobs.
The table was written from the selection as it stood before launch_plan.h (the derivation in drmlt_create, the launchers'
if-ladders); the last rows are the named differences."""
import glob
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")

# PlanInputs of the bench.py scenes (record counts of drmlt-mitsuba_amd/scenes.py; budget = 512 x 512 x sampleCount)
B = 512 * 512
C2 = dict(features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=34, max_depth=8, budget=B * 256)
C3 = dict(features=1, n_shade=9, n_bsdfs=5, n_emitters=1, eff_dim=34, max_depth=8, budget=B * 240)
C5 = dict(technique=2, features=6, n_shade=8, n_bsdfs=5, n_emitters=2, eff_dim=27, max_depth=6, mmlt_S=14, mmlt_E=12, budget=B * 256)
BD = dict(technique=1, features=0, n_shade=30, n_bsdfs=4, n_emitters=1, eff_dim=72, max_depth=8, mmlt_S=22, mmlt_E=20, budget=B * 256)
SOUP = dict(features=8, use_bvh=1, bvh_stack16=1, n_shade=2006, n_bsdfs=4, n_emitters=1, eff_dim=34, max_depth=8, scene_bytes=400000, budget=B * 240)
S50K = dict(SOUP, n_shade=50006, bvh_stack16=0, bvh_overflow=1, scene_bytes=9600000)
S1M = dict(SOUP, n_shade=1000006, bvh_stack16=0, bvh_overflow=1, scene_bytes=188000000, budget=B * 60)
PTS = dict(C2, features=4, n_shade=30 + 400, n_emitters=401)  # 400 point lights: tables beyond 16 KB

# (name, PlanInputs, environment, (build, chains, LDS bytes, mh_batch, trace_yield, rows_mem))
CASES = [
    # every bench.py config (bench fixes the chain count)
    ("bench 2", dict(C2, work_units=65536), {}, ("V4_F0", 65536, 20000, 14, 20, 0)),
    ("bench 2x", dict(C2, work_units=196608), {}, ("V5_F0_ROWS", 196608, 9696, 40, 20, 1)),
    ("bench 3", dict(C3, work_units=196608), {}, ("V5_F1_ROWS", 196608, 8400, 40, 20, 1)),
    ("bench 5", dict(C5, work_units=1048576), {}, ("MMLT_F7_TABLES", 1048576, 14640, 40, 20, 0)),
    ("bench bdpt", dict(BD, work_units=131072), {}, ("BDPT_F7_OCC2_TABLES", 131072, 20000, 40, 20, 0)),
    ("bench soup", dict(SOUP, work_units=196608), {}, ("V5_F8_ROWS", 196608, 7840, 16, 20, 1)),
    ("bench soup50k", dict(S50K, work_units=196608), {}, ("V5_F8_S32_ROWS", 196608, 4896, 16, 20, 1)),
    ("bench soup1m", dict(S1M, work_units=196608), {}, ("V5_F8_S32_ROWS", 196608, 4896, 8, 8, 1)),
    # workUnits = -1
    ("derived flat", C2, {}, ("V5_F0_ROWS", 196608, 9696, 40, 20, 1)),
    ("derived soup", SOUP, {}, ("V5_F8_ROWS", 196608, 7840, 16, 20, 1)),
    ("derived bdpt", BD, {}, ("BDPT_F7_OCC2_TABLES", 131072, 20000, 40, 20, 0)),
    ("budget caps the count", dict(C2, budget=64 * 64 * 100), {}, ("V4_F0", 6400, 20000, 14, 20, 0)),
    ("tiny budget", dict(C2, budget=1000), {}, ("V4_F0", 64, 20000, 14, 20, 0)),
    ("mmlt below 2^35", C5, {}, ("MMLT_F7_TABLES", 262144, 14640, 40, 20, 0)),
    ("mmlt at 2^35", dict(C5, budget=1 << 35), {}, ("MMLT_F7_TABLES", 1048576, 14640, 40, 20, 0)),
    ("reference rule path", dict(C2, work_units_rule=1), {}, ("V4_F0", 336, 20000, 14, 20, 0)),
    ("reference rule mmlt", dict(C5, work_units_rule=1), {}, ("MMLT_F7_TABLES", 672, 14640, 8, 20, 0)),
    # DRMLT_KERNEL, pssmlt
    ("kernel 3", C2, {"DRMLT_KERNEL": "3"}, ("V3_F0", 65536, 15712, 32, 20, 0)),
    ("kernel 4", C2, {"DRMLT_KERNEL": "4"}, ("V4_F0", 65536, 20000, 14, 20, 0)),
    ("kernel 5", C2, {"DRMLT_KERNEL": "5"}, ("V5_F0", 65536, 18400, 40, 20, 0)),
    ("kernel 4 bvh", dict(SOUP, work_units=65536), {"DRMLT_KERNEL": "4"}, ("V4_F8_GLOBAL", 65536, 16656, 6, 24, 0)),
    ("kernel 3 bvh", dict(SOUP, work_units=2048), {"DRMLT_KERNEL": "3"}, ("V3_F15_GLOBAL", 2048, 13568, 32, 24, 0)),
    ("kernel 3 large tables", dict(PTS, work_units=65536), {"DRMLT_KERNEL": "3"}, ("V3_F15_GLOBAL", 65536, 13568, 32, 20, 0)),
    ("pssmlt", dict(C2, algo=1), {}, ("PSSMLT", 65536, 8704, 14, 20, 0)),
    # flat scenes
    ("flat 65536", dict(C3, work_units=65536), {}, ("V4_F3", 65536, 18704, 8, 20, 0)),
    ("flat 131072", dict(C3, work_units=131072), {}, ("V5_F1", 131072, 17104, 40, 20, 0)),
    ("flat 98303", dict(C2, work_units=98303), {}, ("V4_F0", 98303, 20000, 14, 20, 0)),
    ("flat tables too large, v4", dict(PTS, work_units=65536), {}, ("V4_F7_GLOBAL", 65536, 17856, 8, 20, 0)),
    ("flat tables too large, v5", dict(PTS, work_units=131072), {}, ("V5_F7_GLOBAL", 131072, 16256, 40, 20, 0)),
    ("flat tables too large, derived", PTS, {}, ("V5_F7_GLOBAL", 131072, 16256, 40, 20, 0)),
    ("all feature bits on a flat scene", dict(C2, features=15, work_units=131072), {}, ("V5_F15_S32", 131072, 13312, 40, 20, 0)),
    # BVH scenes
    ("bvh stack16", dict(SOUP, features=15, work_units=131072), {}, ("V5_F15", 131072, 16544, 16, 20, 0)),
    ("bvh stack32", dict(S50K, features=15, work_units=131072), {}, ("V5_F15_S32", 131072, 13312, 16, 20, 0)),
    ("bvh stack16 overflow", dict(SOUP, bvh_overflow=1, work_units=131072), {}, ("V5_F8_OVF", 131072, 16544, 16, 20, 0)),
    ("bvh stack16 overflow rows", dict(SOUP, features=12, bvh_overflow=1, work_units=196608), {}, ("V5_F15_OVF_ROWS", 196608, 7840, 16, 20, 1)),
    ("bvh diffuse v4 stack16", dict(SOUP, work_units=65536), {"DRMLT_KERNEL": "4"}, ("V4_F8_GLOBAL", 65536, 16656, 6, 24, 0)),
    ("bvh diffuse v4 stack32", dict(S50K, work_units=65536), {"DRMLT_KERNEL": "4"}, ("V4_F8_S32_GLOBAL", 65536, 16656, 4, 20, 0)),
    ("bvh v4 overflow", dict(SOUP, features=15, bvh_overflow=1, work_units=65536), {"DRMLT_KERNEL": "4"}, ("V4_F15_OVF_GLOBAL", 65536, 16656, 6, 24, 0)),
    ("mmlt bvh", dict(C5, features=14, use_bvh=1, bvh_stack16=1, n_shade=5000, work_units=262144), {}, ("MMLT_F15", 262144, 13824, 16, 20, 0)),
    ("bdpt bvh", dict(BD, features=8, use_bvh=1, bvh_stack16=1, work_units=131072), {}, ("BDPT_F15", 131072, 19712, 16, 20, 0)),
    # DRMLT_DEBUG=128: the stamp builds
    ("stamps v4 flat", dict(C2, work_units=65536), {"DRMLT_DEBUG": "128"}, ("V4_F0_STAMPS", 65536, 20000, 14, 20, 0)),
    ("stamps v4 glossy", dict(C3, work_units=65536), {"DRMLT_DEBUG": "128"}, ("V4_F3_STAMPS", 65536, 18704, 8, 20, 0)),
    ("stamps v4 bvh", dict(SOUP, features=15, work_units=65536), {"DRMLT_KERNEL": "4", "DRMLT_DEBUG": "128"}, ("V4_F15_STAMPS_GLOBAL", 65536, 16656, 6, 24, 0)),
    ("stamps v5 flat", dict(C2, work_units=131072), {"DRMLT_DEBUG": "128"}, ("V5_F0_STAMPS", 131072, 18400, 40, 20, 0)),
    ("stamps v5 bvh", dict(SOUP, work_units=131072), {"DRMLT_DEBUG": "128"}, ("V5_F8_STAMPS", 131072, 16544, 16, 20, 0)),
    # switches
    ("rows mem 1", dict(C2, work_units=131072), {"DRMLT_ROWS_MEM": "1"}, ("V5_F0_ROWS", 131072, 9696, 40, 20, 1)),
    ("rows mem 0", dict(SOUP, work_units=196608), {"DRMLT_ROWS_MEM": "0"}, ("V5_F8", 196608, 16544, 16, 20, 0)),
    ("rows mem 1, v4", dict(C2, work_units=65536), {"DRMLT_ROWS_MEM": "1"}, ("V4_F0", 65536, 20000, 14, 20, 0)),
    ("no small tables", dict(SOUP, work_units=196608), {"DRMLT_NO_SMALL_TABLES": "1"}, ("V5_F8_ROWS", 196608, 7552, 16, 20, 1)),
    ("mmlt tables global", dict(C5, work_units=262144), {"DRMLT_MMLT_TABLES_GLOBAL": "1"}, ("MMLT_F7", 262144, 13824, 40, 20, 0)),
    ("bdpt tables global", dict(BD, work_units=131072), {"DRMLT_BDPT_TABLES_GLOBAL": "1"}, ("BDPT_F7_OCC2", 131072, 19712, 40, 20, 0)),
    ("bdpt 1280 waves", dict(BD, work_units=81920), {}, ("BDPT_F7", 81920, 19712, 14, 20, 0)),
    ("bdpt 1281 waves", dict(BD, work_units=81984), {}, ("BDPT_F7_OCC2_TABLES", 81984, 20000, 14, 20, 0)),
    ("bdpt maxDepth 9: LDS above 20480", dict(BD, max_depth=9, mmlt_S=24, mmlt_E=22, work_units=131072), {}, ("BDPT_F7", 131072, 21760, 40, 20, 0)),
    ("bdpt occ 1", dict(BD, work_units=131072), {"DRMLT_BDPT_OCC": "1"}, ("BDPT_F7", 131072, 19712, 40, 20, 0)),
    ("mh batch, trace yield clamped", dict(SOUP, work_units=196608), {"DRMLT_MH_BATCH": "99", "DRMLT_TRACE_YIELD": "-3"}, ("V5_F8_ROWS", 196608, 7840, 64, 0, 1)),
    # workUnits = -1 asks the plan's own rule: where the derivation predicted a third wave that the selection then refused, it now
    # derives the two-wave count (before this rule: 196 608 chains, run by the build in the last column)
    ("derived flat, DRMLT_TABLES_LDS=0", dict(C2), {"DRMLT_TABLES_LDS": "0"}, ("V5_F7_GLOBAL", 131072, 16256, 40, 20, 0)),  # was V5_F7_GLOBAL at 196608
    ("derived soup, DRMLT_ROWS_MEM=0", dict(SOUP), {"DRMLT_ROWS_MEM": "0"}, ("V5_F8", 131072, 16544, 16, 20, 0)),          # was V5_F8 at 196608
    ("derived flat, 320 CUs", dict(C2, cus=320), {}, ("V5_F0", 131072, 18400, 40, 20, 0)),                                  # was V5_F0 at 196608
]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "native", "plan_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(inputs, knobs):
        args = ["%s=%d" % kv for kv in inputs.items()] + ["%s=%s" % kv for kv in knobs.items()]
        return json.loads(subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout)
    return run


@pytest.mark.parametrize("name,inputs,knobs,want", CASES, ids=[c[0] for c in CASES])
def test_plan(plan, name, inputs, knobs, want):
    p = plan(inputs, knobs)
    assert (p["build"], p["chains"], p["lds"], p["mh_batch"], p["trace_yield"], p["rows_mem"]) == want, p
    per_wave = 32 if p["build"].startswith(("V3_", "V4_")) else 64
    assert p["grid"] == (p["chains"] + per_wave - 1) // per_wave, p
    if p["build"].startswith(("V3_", "V4_", "V5_")):
        assert p["note"] == "[drmlt] k_mutate_%s: %d B of LDS per wave" % (p["build"][:2].lower(), p["lds"]) + (
            (" (+ the traversal stack)" if inputs.get("features", 0) & 8 else "") +
            ("; proposal rows in device memory, three waves per SIMD" if p["rows_mem"] else "") if p["build"].startswith("V5_") else ""), p
    else:
        assert p["note"] == "", p


def test_knob_table_names_every_knob():
    """INTEGRATION.md's knob table names every DRMLT_* variable that launch_plan.h reads."""
    knobs = set(re.findall(r'"(DRMLT_[A-Z0-9_]+)"', open(os.path.join(CSRC, "launch_plan.h")).read()))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = "\n".join(line for line in doc.splitlines() if line.startswith("| `DRMLT_"))
    missing = sorted(k for k in knobs if "`" + k not in table)
    assert len(knobs) > 25 and not missing, missing


def test_every_build_has_its_case_in_one_unit():
    """Every enumerator of launch_plan.h's Build is a `case Build::X` of exactly one launcher, and the chain-kernel families of
    technique=path keep to their units (k_mutate_v4 and k_mutate_v5 share one: DESIGN.md section 3k): a build lost between them would
    only show as an abort on the device. Source text only."""
    enum = re.search(r"enum class Build \{(.*?)\};", open(os.path.join(CSRC, "launch_plan.h")).read(), re.S).group(1)
    builds = re.findall(r"\b[A-Z][A-Z0-9_]*\b", re.sub(r"//.*", "", enum))
    assert len(builds) > 50 and len(set(builds)) == len(builds), builds
    cases = {}  # enumerator -> [unit, ...], one entry per occurrence
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        for b in re.findall(r"\bcase Build::(\w+)\b", open(path).read()):
            cases.setdefault(b, []).append(os.path.basename(path))
    assert sorted(cases) == sorted(builds), set(cases) ^ set(builds)
    assert all(len(units) == 1 for units in cases.values()), {b: u for b, u in cases.items() if len(u) != 1}
    for prefixes, unit in ((("V3_",), "kernels_v3.hip"), (("V4_", "V5_"), "kernels_v4.hip")):
        mine = [b for b in builds if b.startswith(prefixes)]
        assert mine and all(cases[b] == [unit] for b in mine), (unit, {b: cases[b] for b in mine})
        assert [b for b, u in cases.items() if u == [unit] and not b.startswith(prefixes)] == [], unit
