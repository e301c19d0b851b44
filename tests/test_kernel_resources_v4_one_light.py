"""Resources of k_mutate_v4's one-light builds (kernels_v4.hip: V4_ONE_LIGHT_BUILD), from the compiler's resource remarks of the build
(libdrmlt_amd.so.resources): each runs in place of V4_F0 / V4_F0_STAMPS under one of the two rules, on the grid and the LDS planned
for that build, so it must not need more of anything that decides how many waves share a SIMD. The twins move the light's records
from vector to scalar registers, so the vector registers are held to the replaced build's as well.

As measured on the commit that adds this file (replaced build -> twin: VGPRs, spilled SGPRs, occupancy):
    V4_F0                 157 -> 139,  4 ->  0, 3 -> 3
    V4_F0 orbital         165 -> 134,  0 ->  0, 3 -> 3   (bench.py's flagship build)
    V4_F0_STAMPS          173 -> 143, 32 -> 26, 2 -> 3
    V4_F0_STAMPS orbital  169 -> 138, 22 -> 22, 2 -> 3
The stamps twins count their events (iterations, branches, tracing lanes, the histogram) in 32 bits per wave where the builds they
replace use 64 (kernels_v4.hip: StampCount): with 64-bit counts the orbital stamps twin spilled 24 scalars against 22, whatever was
done to the light's records or to the build counters."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "_Z11k_mutate_v4ILi%dELb1ELb%dELb0ELb0EEv7DParamsjj"  # <BUILD, LDS_TABLES = true, STAMPS, false, false>
ORBITAL, ONE_LIGHT = 16, 32
KEYS = ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


def remarks(name):
    path = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(path), "the Makefile writes it next to the library"
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z /\[\]]*): (\d+)", line)
        if m and cur == name:
            out[m.group(1).strip()] = int(m.group(2))
    assert all(k in out for k in KEYS), (name, out)
    return out


@pytest.mark.parametrize("rule,stamps", [(0, 0), (ORBITAL, 0), (0, 1), (ORBITAL, 1)],
                         ids=["V4_F0", "V4_F0 orbital", "V4_F0_STAMPS", "V4_F0_STAMPS orbital"])
def test_one_light_build_needs_no_more_than_the_build_it_replaces(native_lib, rule, stamps):
    gen, one = remarks(SYMBOL % (rule, stamps)), remarks(SYMBOL % (rule | ONE_LIGHT, stamps))
    print({k: (gen[k], one[k]) for k in KEYS})
    assert one["VGPRs"] <= gen["VGPRs"]
    assert one["SGPRs Spill"] <= gen["SGPRs Spill"]
    assert one["VGPRs Spill"] == 0 and one["ScratchSize [bytes/lane]"] <= gen["ScratchSize [bytes/lane]"]
    assert one["Occupancy [waves/SIMD]"] >= gen["Occupancy [waves/SIMD]"]


def test_headline_one_light_build_within_the_headline_limits(native_lib):
    """bench.py's flagship line runs this one: the limits tests/test_kernel_resources_v4_spills.py sets for V4_F0."""
    r = remarks(SYMBOL % (ORBITAL | ONE_LIGHT, 0))
    assert r["SGPRs Spill"] <= 8 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs"] <= 168 and r["Occupancy [waves/SIMD]"] == 3, r
