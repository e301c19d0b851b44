"""k_mutate_w2h with its select-only decide (kernels_v4.hip: w2h_decide), from the compiler's resource remarks of the build. The decide
is one long block with a dozen lane masks alive in scalar registers, and the kernel stands at the edge of its vector registers:
what tests/test_kernel_resources_w2h.py asks, and no spilled SCALAR register either (a prototype of the decide spilled six, and
a spilled scalar pair is a v_writelane / v_readlane pair in the loop or across it). As measured on the commit that adds this
file: 255 VGPRs, no AGPRs, nothing spilled."""
from test_kernel_resources_w2 import remarks
from test_kernel_resources_w2h import SYMBOL


def test_nothing_spills(native_lib):
    r = remarks(SYMBOL)
    print(r)
    assert r["SGPRs Spill"] == 0
    assert r["VGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["VGPRs"] + r["AGPRs"] <= 256
    assert r["Occupancy [waves/SIMD]"] >= 2
