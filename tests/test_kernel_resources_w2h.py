"""Resources of k_mutate_w2h (kernels_v4.hip), from the compiler's resource remarks of the build (libdrmlt_amd.so.resources). The kernel
is k_mutate_w2 plus the scene's ray records in vector registers, 58 dwords and a count word: it is declared for two waves per SIMD
and may use their whole register file -- 256 registers per lane, vector and accumulator registers together -- but nothing may
spill and nothing may sit in scratch memory (a spilled record would be re-read from memory in the pass that holds it in order
not to read memory). As measured on the commit that adds this file: 252 VGPRs, no AGPRs, no spilled scalar.
k_mutate_w2h is k_mutate_w2<true>, k_mutate_w2 the streaming instantiation k_mutate_w2<false> of the same template: the latter
keeps the resources it had as a kernel of its own."""
from test_kernel_resources_w2 import SYMBOL as W2_SYMBOL, remarks

SYMBOL = "_Z11k_mutate_w2ILb1EEv7DParamsjj"


def test_two_waves_per_simd_without_spills(native_lib):
    r = remarks(SYMBOL)
    print(r)
    assert r["Occupancy [waves/SIMD]"] >= 2
    assert r["VGPRs"] + r["AGPRs"] <= 256
    assert r["VGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0


def test_k_mutate_w2_keeps_its_resources(native_lib):
    r = remarks(W2_SYMBOL)
    print(r)
    assert r["VGPRs"] == 193 and r["AGPRs"] == 0
    assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0
    assert r["ScratchSize [bytes/lane]"] == 0
    assert r["Occupancy [waves/SIMD]"] == 2
