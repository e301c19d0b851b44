"""eval_mmlt's sink (device_bidir.h: MmltNoSink) costs the kernels that do not use it nothing, and k_render_mmlt / k_layers_mmlt fit
where the bootstrap fits. Read from the compiler's resource remarks of the build (libdrmlt_amd.so.resources).
  - Every kernel built from eval_mmlt before the sink -- all k_mutate_mmlt builds, k_bootstrap_mmlt, k_init_chains_mmlt and
    k_eval_paths_mmlt -- keeps the numbers of the commit before it (its libdrmlt_amd.so.resources, pinned in PARENT below) exactly:
    VGPRs + AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, occupancy in waves per SIMD. The set of those kernels is the
    parent's plus the two new ones. (Compared file against file when the sink went in: the remarks of all 95 kernels of the parent's
    library are unchanged.)
  - k_render_mmlt, k_layers_mmlt: at least k_bootstrap_mmlt's occupancy and no more static LDS. Registers and scratch are printed,
    not bounded: 199 and 202 VGPRs, 0 AGPRs, 106 SGPRs, no scratch, occupancy 2, 6912 B LDS (k_bootstrap_mmlt: 191)."""
import os
import re

from test_kernel_resources_layers import ROOT, _row, kernels

MMLT = re.compile(r"_Z\d+k_(mutate_mmlt|bootstrap_mmlt|init_chains_mmlt|eval_paths_mmlt|render_mmlt|layers_mmlt)(?![a-z_])")

# name: (VGPRs + AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, occupancy) of the parent commit
PARENT = {
    "_Z13k_mutate_mmltILi15ELb0EEv7DParamsjj": (256, 104, 28, 6912, 2),
    "_Z13k_mutate_mmltILi7ELb0EEv7DParamsjj": (245, 104, 0, 0, 2),
    "_Z13k_mutate_mmltILi7ELb1EEv7DParamsjj": (243, 104, 0, 0, 2),
    "_Z16k_bootstrap_mmlt7DParamsjPf": (191, 106, 0, 6912, 2),
    "_Z17k_eval_paths_mmlt7DParamsPKfjjPf": (190, 106, 0, 6912, 2),
    "_Z18k_init_chains_mmlt7DParamsPKjPKf": (198, 106, 0, 6912, 2),
}
NEW = ["_Z13k_layers_mmlt7DParamsjfPdi", "_Z13k_render_mmlt7DParamsjfPd"]


def _mmlt(native_lib):
    res = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(res), "the Makefile writes it next to the library"
    return {n: r for n, r in kernels(res).items() if MMLT.match(n)}


def test_the_sink_costs_the_existing_mmlt_kernels_nothing(native_lib):
    now = _mmlt(native_lib)
    for n, want in sorted(PARENT.items()):
        assert n in now and _row(now[n]) == want, (n, now.get(n), want)


def test_the_kernels_built_from_eval_mmlt_are_the_parents_and_the_two_new_ones(native_lib):
    assert sorted(_mmlt(native_lib)) == sorted(list(PARENT) + NEW)


def test_the_render_kernels_fit_where_the_bootstrap_fits(native_lib):
    now = _mmlt(native_lib)
    boot = now["_Z16k_bootstrap_mmlt7DParamsjPf"]
    for name in NEW + ["_Z16k_bootstrap_mmlt7DParamsjPf"]:
        r = now[name]
        print("%s: %d VGPRs + %d AGPRs, %d SGPRs, scratch %d B/lane, occupancy %d, static LDS %d B"
              % (name, r["VGPRs"], r["AGPRs"], r["SGPRs"], r["ScratchSize"], r["Occupancy"], r["LDS"]))
    for name in NEW:
        assert now[name]["Occupancy"] >= boot["Occupancy"] >= 1, (name, now[name], boot)
        assert now[name]["LDS"] <= boot["LDS"], (name, now[name], boot)
        # the existing resource tests count kernels by these prefixes: the new symbols must not fall under them
        assert not re.match(r"_Z\d+(k_render_bdpt|k_render_pt|k_layers_bdpt|k_bootstrap_mmlt|k_mutate_)", name)
