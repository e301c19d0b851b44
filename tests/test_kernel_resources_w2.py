"""Resources of k_mutate_w2 (kernels_v4.hip), from the compiler's resource remarks of the build (libdrmlt_amd.so.resources). The kernel
is declared for two waves per SIMD and runs only launches that cannot have a third (launch_plan.h: w2_launch): it may use the
whole register file of two waves -- 256 registers per lane, vector and accumulator registers together -- but nothing may spill
and nothing may sit in scratch memory. As measured on the commit that adds this file: 199 VGPRs, no AGPRs, no spilled scalar."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "_Z11k_mutate_w2ILb0EEv7DParamsjj"  # k_mutate_w2<false>, the streaming instantiation of the template
KEYS = ("VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]")


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


def test_two_waves_per_simd_without_spills(native_lib):
    r = remarks(SYMBOL)
    print(r)
    assert r["Occupancy [waves/SIMD]"] >= 2
    assert r["VGPRs"] + r["AGPRs"] <= 256
    assert r["VGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0
