"""Resources of k_mutate_v4's orbital builds (kernels_v4.hip: V4_ORBITAL_BUILD), from the compiler's resource remarks of the build
(libdrmlt_amd.so.resources): each runs in place of a generic build on the grid and the LDS planned for that one, so it must not
need more of anything that decides how many waves share a SIMD."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "_Z11k_mutate_v4ILi%dELb1ELb%dELb0ELb0EEv7DParamsjj"  # <BUILD, LDS_TABLES = true, STAMPS, false, false>
ORBITAL = 16
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


@pytest.mark.parametrize("feat,stamps", [(0, 0), (0, 1), (3, 0), (7, 0)], ids=["V4_F0", "V4_F0_STAMPS", "V4_F3", "V4_F7"])
def test_orbital_build_needs_no_more_than_its_generic_twin(native_lib, feat, stamps):
    gen, orb = remarks(SYMBOL % (feat, stamps)), remarks(SYMBOL % (feat | ORBITAL, stamps))
    print({k: (gen[k], orb[k]) for k in KEYS})
    assert orb["Occupancy [waves/SIMD]"] >= gen["Occupancy [waves/SIMD]"]
    assert orb["ScratchSize [bytes/lane]"] == 0 and orb["VGPRs Spill"] == 0
    assert orb["SGPRs Spill"] <= gen["SGPRs Spill"]


def test_headline_orbital_build_within_the_headline_limits(native_lib):
    """bench.py's flagship line runs this one: the limits tests/test_kernel_resources_v4_spills.py sets for the generic build."""
    r = remarks(SYMBOL % (ORBITAL, 0))
    assert r["SGPRs Spill"] <= 8 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs"] <= 168 and r["Occupancy [waves/SIMD]"] == 3, r
