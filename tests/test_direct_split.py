"""The direct-illumination pass without a device: the sample split of renderDirectComponent (src/libbidir/util.cpp:40-54)
as the library computes it, the three entry points, and their refusals that need no context."""
import ctypes as C

import pytest


@pytest.mark.parametrize("n,pixel,shading", [(1, 1, 1), (8, 8, 1), (9, 4, 2), (16, 8, 2), (17, 8, 2), (64, 8, 8), (100, 6, 16), (1024, 8, 128)])
def test_direct_split_matches_the_reference(pkg, native_lib, n, pixel, shading):
    assert pkg.binding.direct_split(n) == (pixel, shading)


@pytest.mark.parametrize("n", [0, -1])
def test_no_split_without_direct_samples(pkg, native_lib, n):
    with pytest.raises(pkg.binding.DrmltError) as e:
        pkg.binding.direct_split(n)
    assert e.value.code == pkg.abi.E_INVALID
    ps, ss = C.c_int32(7), C.c_int32(7)
    assert native_lib.drmlt_direct_split(n, C.byref(ps), C.byref(ss)) == pkg.abi.E_INVALID
    assert (ps.value, ss.value) == (7, 7)


def test_render_direct_refuses_a_null_context(pkg, native_lib):
    out = (C.c_float * 3)()
    assert native_lib.drmlt_render_direct(None, 16, 0, 1, 0, 1, out) == pkg.abi.E_INVALID
    assert native_lib.drmlt_node_render_direct(None, 16, 0, 1, out) == pkg.abi.E_INVALID


def test_the_library_exports_the_direct_pass(pkg, native_lib):
    for name in ("drmlt_render_direct", "drmlt_direct_split", "drmlt_node_render_direct"):
        assert hasattr(native_lib, name), name
        assert name in pkg.binding.ABI_SYMBOLS


def test_the_abi_version_is_unchanged(native_lib):
    assert native_lib.drmlt_abi_version() == 4
