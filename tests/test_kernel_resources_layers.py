"""eval_bdpt's per-cell sink (device_bdpt.h) costs the kernels that do not use it nothing, and k_layers_bdpt, which does, fits where
the bootstrap fits. Read from the compiler's resource remarks of the build (libdrmlt_amd.so.resources).
  - Every kernel that is built from device_bdpt.h -- all k_mutate_bdpt and k_mutate_pssmlt_bdpt builds, k_bootstrap_bdpt,
    k_init_chains_bdpt, k_render_bdpt and the list evaluation k_eval_lists_bdpt -- keeps the numbers of the commit before the sink
    (its libdrmlt_amd.so.resources, pinned in PARENT below) exactly: VGPRs + AGPRs, SGPRs, scratch bytes per lane, static LDS bytes,
    occupancy in waves per SIMD. The set of those kernels is the parent's plus k_layers_bdpt. (Compared file against file when the
    sink went in: the remarks of all 87 kernels of the library are the parent's, and the device assembly of kernels_bdpt.hip,
    kernels_pssmlt_bdpt.hip and kernels_render_bdpt.hip is the parent's instruction for instruction with the sink passed by value;
    passed by reference, a dozen register initialisations changed places in two of them.)
  - k_layers_bdpt: at least k_bootstrap_bdpt's occupancy and no more static LDS, tests/test_kernel_resources_render_bdpt.py's
    bounds. Its registers and scratch are printed, not bounded: 247 VGPRs, 0 AGPRs, 106 SGPRs, no scratch, occupancy 2, 6912 B LDS
    (k_render_bdpt: 244; k_bootstrap_bdpt: 246)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "ScratchSize",
          "Occupancy [waves/SIMD]": "Occupancy", "LDS Size [bytes/block]": "LDS"}
BIDIR = re.compile(r"_Z\d+k_(mutate_bdpt|mutate_pssmlt_bdpt|bootstrap_bdpt|init_chains_bdpt|render_bdpt|eval_lists_bdpt|layers_bdpt)(?![a-z_])")

# name: (VGPRs + AGPRs, SGPRs, scratch bytes per lane, static LDS bytes, occupancy) of the parent commit
PARENT = {
    "_Z13k_mutate_bdptILi15ELi1ELb0EEv7DParamsjj": (282, 106, 0, 6912, 1),
    "_Z13k_mutate_bdptILi7ELi1ELb0EEv7DParamsjj": (259, 106, 0, 0, 1),
    "_Z13k_mutate_bdptILi7ELi2ELb0EEv7DParamsjj": (256, 106, 16, 0, 2),
    "_Z13k_mutate_bdptILi7ELi2ELb1EEv7DParamsjj": (256, 106, 16, 0, 2),
    "_Z13k_render_bdpt7DParamsjf": (244, 106, 0, 6912, 2),
    "_Z16k_bootstrap_bdpt7DParamsjPf": (246, 106, 0, 6912, 2),
    "_Z17k_eval_lists_bdpt7DParamsPKfjjPfj": (258, 106, 0, 6912, 1),
    "_Z18k_init_chains_bdpt7DParamsPKjPKf": (197, 106, 0, 6912, 2),
    "_Z20k_mutate_pssmlt_bdptILi15ELi1ELb0EEv7DParamsjj": (256, 104, 0, 6912, 2),
    "_Z20k_mutate_pssmlt_bdptILi7ELi1ELb0EEv7DParamsjj": (227, 106, 0, 0, 2),
    "_Z20k_mutate_pssmlt_bdptILi7ELi2ELb0EEv7DParamsjj": (226, 106, 0, 0, 2),
    "_Z20k_mutate_pssmlt_bdptILi7ELi2ELb1EEv7DParamsjj": (225, 106, 0, 0, 2),
}
LAYERS = "_Z13k_layers_bdpt7DParamsjfPfi"


def kernels(path):
    """tests/test_kernel_resources.py's kernels(), with the scalar registers beside what it reads."""
    out, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(%s): (\d+)" % "|".join(re.escape(f) for f in FIELDS), line)
        if m and name:
            out[name][FIELDS[m.group(1)]] = int(m.group(2))
    return out


def _row(r):
    return (r["VGPRs"] + r["AGPRs"], r["SGPRs"], r["ScratchSize"], r["LDS"], r["Occupancy"])


def _bidir(native_lib):
    res = os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources")
    assert os.path.exists(res), "the Makefile writes it next to the library"
    return {n: r for n, r in kernels(res).items() if BIDIR.match(n)}


def test_the_sink_costs_the_existing_bidirectional_kernels_nothing(native_lib):
    now = _bidir(native_lib)
    assert sorted(now) == sorted(list(PARENT) + [LAYERS])         # the parent's kernels and the one new kernel
    for n, want in sorted(PARENT.items()):
        assert _row(now[n]) == want, (n, _row(now[n]), want)


def test_layers_bdpt_fits_where_the_bootstrap_fits(native_lib):
    now = _bidir(native_lib)
    layers, boot, render = now[LAYERS], now["_Z16k_bootstrap_bdpt7DParamsjPf"], now["_Z13k_render_bdpt7DParamsjf"]
    for name, r in (("k_layers_bdpt", layers), ("k_render_bdpt", render), ("k_bootstrap_bdpt", boot)):
        print("%s: %d VGPRs + %d AGPRs, %d SGPRs, scratch %d B/lane, occupancy %d, static LDS %d B"
              % (name, r["VGPRs"], r["AGPRs"], r["SGPRs"], r["ScratchSize"], r["Occupancy"], r["LDS"]))
    assert layers["Occupancy"] >= boot["Occupancy"], (layers, boot)
    assert layers["LDS"] <= boot["LDS"], (layers, boot)
    # the existing resource tests count kernels by these prefixes: the new symbol must not fall under them
    assert not re.match(r"_Z\d+(k_render_bdpt|k_bootstrap_bdpt|k_mutate_v)", LAYERS)
