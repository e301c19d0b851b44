"""Scalar-register spills of config 2's chain kernel, read from the compiler's resource remarks of the build
(libdrmlt_amd.so.resources). A spilled SGPR lives in a lane of a VGPR: every use inside the chain loop is a v_readlane /
v_writelane, an instruction that issues like an FMA and does no arithmetic."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = "_Z11k_mutate_v4ILi0ELb1ELb0ELb0ELb0EEv7DParamsjj"


def remarks(path, name):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"remark:\s+(SGPRs Spill|VGPRs Spill|VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and cur == name:
            out[m.group(1)] = int(m.group(2))
    return out


def test_headline_v4_spills_at_most_eight_sgprs(native_lib):
    res = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(res), "the Makefile writes it next to the library"
    r = remarks(res, HEADLINE)
    assert "SGPRs Spill" in r, r
    assert r["SGPRs Spill"] <= 8, r
    assert r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, r
    assert r["VGPRs"] <= 168, r
