"""drmlt_render_mmlt and drmlt_render_mmlt_layers at the boundary (no GPU): what the header declares, the library exports and the
binding exposes and refuses by itself."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drmlt_abi.h")


def _declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _args(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, _declarations())
    assert m, "include/drmlt_abi.h does not declare %s" % name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_both_entry_points_are_declared_exported_and_bound(pkg, native_lib):
    assert _args("drmlt_render_mmlt") == ["drmlt_ctx *ctx", "uint32_t spp", "uint64_t seed", "float *out_rgb"]
    assert _args("drmlt_render_mmlt_layers") == ["drmlt_ctx *ctx", "uint32_t spp", "uint64_t seed", "int32_t mode", "float *out_layers"]
    for name in ("drmlt_render_mmlt", "drmlt_render_mmlt_layers"):
        assert name in pkg.binding.ABI_SYMBOLS and hasattr(native_lib, name)
    assert native_lib.drmlt_render_mmlt.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    assert native_lib.drmlt_render_mmlt_layers.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p]
    sig = inspect.signature(pkg.Context.render_mmlt)
    assert list(sig.parameters) == ["self", "spp", "seed"] and sig.parameters["seed"].default == 1
    sig = inspect.signature(pkg.Context.render_mmlt_layers)
    assert list(sig.parameters) == ["self", "spp", "seed", "weighted"]
    assert sig.parameters["seed"].default == 1 and sig.parameters["weighted"].default is True
    out = np.zeros(3, dtype=np.float32)
    assert native_lib.drmlt_render_mmlt(None, 1, 1, out.ctypes.data) == pkg.abi.E_INVALID               # a NULL context
    assert native_lib.drmlt_render_mmlt_layers(None, 1, 1, 0, out.ctypes.data) == pkg.abi.E_INVALID
    assert np.all(out == 0)


def test_the_header_states_the_sample_rule_and_the_scale():
    """The per-depth sample rule, the 1 / spp scale with its derivation, and the reference lines they restate."""
    text = re.sub(r"\s*\n \*\s*", " ", open(HEADER).read())
    at = text.index("technique=mmlt's own equal-expectation reference")
    doc = text[at:text.index("int drmlt_render_mmlt_layers(")]
    for want in ("(i % max_depth) + 1", "pathsampler.cpp:889", "PER DEPTH", "Scale 1/spp", "pathsampler.cpp:933", "drmlt_develop",
                 "drmlt_bootstrap_luminances", "pathsampler.cpp:84-320", "pathsampler.cpp:131", "pathsampler.cpp:279",
                 "drmlt_bdpt_layer_index(d, s)", "bit for bit"):
        assert want in doc, want
    assert "#define DRMLT_ABI_VERSION 4" in text      # entry points were added before without a new version


@pytest.mark.parametrize("technique,other", [("path", "render_pt"), ("bdpt", "render_bdpt")])
def test_the_binding_refuses_another_technique_before_any_device_work(pkg, technique, other):
    """Context.render_mmlt and render_mmlt_layers look at the configuration first: on a context that was never created on a device
    (no library, no handle -- any call into the library would fail on the missing attribute) the refusal is the binding's own, names
    the technique the context has and points to that technique's reference."""
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.L, ctx.h, ctx.width, ctx.height = None, None, 16, 16
    ctx.cfg = pkg.abi.make_config(technique=technique, max_depth=4)
    for call, ref in ((lambda: ctx.render_mmlt(4), other), (lambda: ctx.render_mmlt_layers(4), other + "_layers")):
        with pytest.raises(pkg.binding.DrmltError, match=r"technique=mmlt.*technique=%s \(%s is" % (technique, ref)) as e:
            call()
        assert e.value.code == pkg.abi.E_INVALID
