"""drmlt_render_pt_layers at the boundary (no GPU): the layer arithmetic of the header, the library and abi.py, what the binding
exposes and refuses by itself, and the resources of k_render_pt_layers beside k_render_pt's."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_kernel_resources import kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drmlt_abi.h")


def _declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_layer_indices_in_the_header_the_library_and_abi_py(pkg, native_lib):
    """count(D) = 2 D and index(d, strategy) = 2 (d - 1) + strategy: index maps {(d, strategy): 1 <= d <= D, strategy in {HIT, DIRECT}}
    one to one onto range(count(D)), depth after depth, and both are -1 outside the ranges."""
    abi = pkg.abi
    src = _declarations()
    assert re.search(r"int\s+drmlt_pt_layer_count\s*\(\s*int32_t max_depth\s*\)\s*;", src)
    assert re.search(r"int\s+drmlt_pt_layer_index\s*\(\s*int32_t depth\s*,\s*int32_t strategy\s*\)\s*;", src)
    m = re.search(r"enum\s*\{\s*DRMLT_PT_HIT\s*=\s*(\d+)\s*,\s*DRMLT_PT_DIRECT\s*=\s*(\d+)\s*\}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (abi.PT_HIT, abi.PT_DIRECT) == (0, 1)
    count, index = native_lib.drmlt_pt_layer_count, native_lib.drmlt_pt_layer_index
    for D in list(range(1, 33)) + [1000, 40000]:
        assert count(D) == abi.pt_layer_count(D) == 2 * D
    for D in range(1, 25):
        got = [index(d, s) for d in range(1, D + 1) for s in (abi.PT_HIT, abi.PT_DIRECT)]
        assert got == list(range(count(D)))
        assert got == [abi.pt_layer_index(d, s) for d in range(1, D + 1) for s in (0, 1)]
    for d in (1, 2, 7, 24, 40000):
        assert index(d, abi.PT_HIT) == 2 * (d - 1) and index(d, abi.PT_DIRECT) == 2 * (d - 1) + 1
    for d, s in ((0, 0), (-1, 0), (1, -1), (1, 2), (5, 7), (0, 1), (2 ** 31 - 1, 0), (2 ** 30, 1), (-2 ** 31, -2 ** 31)):
        assert index(d, s) == abi.pt_layer_index(d, s) == -1, (d, s)
    for D in (0, -1, -24, 2 ** 30, 2 ** 31 - 1, -2 ** 31):
        assert count(D) == abi.pt_layer_count(D) == -1, D
    # the helpers need no device and no context: the largest depth whose products fit answers
    assert count(2 ** 30 - 1) == 2 ** 31 - 2 and index(2 ** 30 - 1, 1) == 2 ** 31 - 3


def test_the_binding_exposes_render_pt_layers(pkg, native_lib):
    m = re.search(r"int\s+drmlt_render_pt_layers\s*\(([^)]*)\)\s*;", _declarations())
    assert m, "include/drmlt_abi.h does not declare drmlt_render_pt_layers"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == \
        ["drmlt_ctx *ctx", "uint32_t spp", "uint64_t seed", "int32_t mode", "float *out_layers"]
    for name in ("drmlt_render_pt_layers", "drmlt_pt_layer_count", "drmlt_pt_layer_index"):
        assert name in pkg.binding.ABI_SYMBOLS and hasattr(native_lib, name)
    assert native_lib.drmlt_render_pt_layers.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p]
    sig = inspect.signature(pkg.Context.render_pt_layers)
    assert list(sig.parameters) == ["self", "spp", "seed", "weighted"]
    assert sig.parameters["seed"].default == 1 and sig.parameters["weighted"].default is True
    out = np.zeros(3, dtype=np.float32)
    assert native_lib.drmlt_render_pt_layers(None, 1, 1, 0, out.ctypes.data) == pkg.abi.E_INVALID      # a NULL context
    assert np.all(out == 0)
    # the header cites what the layers restate and states how the path machine's depth counter maps to d
    text = open(HEADER).read()
    assert "path.cpp:187-238" in text and "path.cpp:253-285" in text and "depth + 1" in text


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
def test_the_binding_refuses_another_technique_before_any_device_work(pkg, technique):
    """Context.render_pt_layers looks at its configuration first: on a context that was never created on a device (no library, no
    handle -- any call into the library would fail on the missing attribute) the refusal is the binding's own and names the
    technique."""
    ctx = pkg.Context.__new__(pkg.Context)
    ctx.L, ctx.h, ctx.width, ctx.height = None, None, 16, 16
    ctx.cfg = pkg.abi.make_config(technique=technique, max_depth=4)
    with pytest.raises(pkg.binding.DrmltError, match="technique=path.*technique=%s" % technique) as e:
        ctx.render_pt_layers(4)
    assert e.value.code == pkg.abi.E_INVALID


def test_the_layer_kernel_keeps_render_pts_occupancy_and_scratch(native_lib):
    """k_render_pt_layers is k_render_pt's loop with the sink's LDS stores: at least its occupancy and no more scratch per lane,
    both read from this build's remarks. (Built for gfx950: 140 against 136 vector registers, three waves per SIMD and no scratch
    for both; the static LDS, the traversal stack, is the same 6 912 bytes.)"""
    k = kernels(os.path.join(ROOT, "drmlt-mitsuba_amd", "libdrmlt_amd.so.resources"))
    mine = [r for n, r in k.items() if n.startswith("_Z18k_render_pt_layers")]
    base = [r for n, r in k.items() if n.startswith("_Z11k_render_pt7DParams")]
    assert len(mine) == 1 and len(base) == 1, (mine, base)
    mine, base = mine[0], base[0]
    print("k_render_pt_layers %s\nk_render_pt        %s" % (mine, base))
    assert mine["Occupancy"] >= base["Occupancy"] >= 1
    assert mine["ScratchSize"] <= base["ScratchSize"]
    assert mine["LDS"] == base["LDS"]          # the rows of the layers are dynamic LDS, sized by the launch
