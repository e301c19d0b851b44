"""The seed-selection kernels' (kernels_seed.hip) scratch and spills, read from the compiler's resource remarks of the build
(libdrmlt_amd.so.resources): five small kernels that keep everything in registers -- a lane's sixteen counts in
k_seed_scan_counts and the four-sample reads of the block sums are arrays in the source and must not become scratch."""
import os
import re

from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("k_seed_block_sums", "k_seed_scan_sums", "k_seed_pick", "k_seed_scan_counts", "k_seed_expand")


def spills(path):
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(SGPRs|VGPRs) Spill: (\d+)", line)
        if m and name:
            out[name][m.group(1)] = int(m.group(2))
    return out


def test_seed_kernels_use_no_scratch_and_spill_nothing(native_lib):
    res = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(res), "the Makefile writes it next to the library"
    k, s = kernels(res), spills(res)
    seed = sorted(n for n in k if "k_seed_" in n)
    assert len(seed) == len(NAMES) and all(any(want in n for n in seed) for want in NAMES), seed
    for n in seed:
        print("%s: %d VGPRs, scratch %d B/lane, spilled %d SGPRs + %d VGPRs, occupancy %d, static LDS %d B"
              % (n, k[n]["VGPRs"], k[n]["ScratchSize"], s[n]["SGPRs"], s[n]["VGPRs"], k[n]["Occupancy"], k[n]["LDS"]))
        assert k[n]["ScratchSize"] == 0, (n, k[n])
        assert s[n] == {"SGPRs": 0, "VGPRs": 0}, (n, s[n])
