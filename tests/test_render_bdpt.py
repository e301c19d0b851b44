"""drmlt_render_bdpt at the boundary (no GPU): the header declares it, the binding mirrors its argument types, and a NULL
context is refused like drmlt_render_pt's. And what tests/test_gpu_render_bdpt.py takes for granted about its own scenes and its
CPU-side reference, checked without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import render_bdpt_scenes as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drmlt_abi.h")


def test_the_header_declares_render_bdpt_beside_render_pt():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+drmlt_render_bdpt\s*\(([^)]*)\)\s*;", src)
    assert m, "include/drmlt_abi.h does not declare drmlt_render_bdpt"
    args = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert args == ["drmlt_ctx *ctx", "uint32_t spp", "uint64_t seed", "float *out_rgb"]
    pt = re.search(r"int\s+drmlt_render_pt\s*\(([^)]*)\)\s*;", src)
    assert [re.sub(r"\s+", " ", a.strip()) for a in pt.group(1).split(",")] == args   # the same signature as its unidirectional twin


def test_the_binding_exposes_render_bdpt_with_matching_types(pkg, native_lib):
    assert "drmlt_render_bdpt" in pkg.binding.ABI_SYMBOLS
    assert hasattr(native_lib, "drmlt_render_bdpt")
    assert native_lib.drmlt_render_bdpt.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    assert native_lib.drmlt_render_bdpt.argtypes == native_lib.drmlt_render_pt.argtypes
    assert callable(getattr(pkg.Context, "render_bdpt", None))
    import inspect
    sig = inspect.signature(pkg.Context.render_bdpt)
    assert list(sig.parameters) == ["self", "spp", "seed"] and sig.parameters["seed"].default == 1
    # a node handle is no context: the reference is rendered through Node.context(rank), which inherits the method
    assert "render_bdpt" not in vars(pkg.Node) and issubclass(pkg.binding.BorrowedContext, pkg.Context)


def test_a_null_context_is_refused(pkg, native_lib):
    out = np.zeros(3, dtype=np.float32)
    assert native_lib.drmlt_render_bdpt(None, 1, 1, out.ctypes.data) == pkg.abi.E_INVALID
    assert native_lib.drmlt_render_pt(None, 1, 1, out.ctypes.data) == pkg.abi.E_INVALID   # (as its twin refuses it)
    assert np.all(out == 0)


def test_the_lamp_is_out_of_view_and_lights_every_pixel(pkg):
    """The closed form alone. Were the light inside the view, the camera would see it (s = 0, t = 2 and s = 1, t = 1) and the image
    would not be the depth-2 closed form."""
    assert rs.lamp_is_out_of_view(pkg) > 0.5            # at least half a film half-width beyond the film's edge
    assert rs.lamp_plane_closed_form(pkg).min() > 0


@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
@pytest.mark.parametrize("name", ["glass_sphere", "caustic_c5"])
def test_the_oracles_lists_light_every_block(pkg, ob, name, direct):
    """The oracle alone, as test_image_matches_the_oracles_lists uses it: at n = 16 384 points at most 10 % of the 4 x 4 blocks of
    the 16 x 16 film may be without variance (measured: none), and the host-side film keeps every list's luminance."""
    sd = pkg.scenes.SCENES[name](16)
    cfg = pkg.abi.make_config(technique="bdpt", type="orbital", max_depth=6, rr_depth=4, direct_samples=-1, work_units=64,
                              luminance_samples=1000, no_direct_sampling=1 - direct)
    orc = ob.Oracle(pkg.abi, cfg, sd, 64)
    us, ue, ud = rs.list_points(cfg, 16384, 21)
    rows = orc.bdpt_eval(us, ue, ud) if ud is not None else orc.bdpt_eval(us, ue)
    orc.close()
    c = rs.block_contributions(rows, 16)
    assert (c.var(axis=0, ddof=1) == 0).mean() <= 0.1
    assert c.mean(axis=(1, 2)).mean() == pytest.approx(rows[:, 0].astype(np.float64).mean(), rel=1e-5)
