"""drmlt_render_bdpt_layers at the boundary (no GPU): the layer arithmetic of the header, the library and abi.py, what the
binding exposes, and the oracle's side of tests/test_gpu_bdpt_layers.py's strategy-by-strategy comparison with the oracle alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import bdpt_layers_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drmlt_abi.h")

# what qualifying() gives at n = 16 384 (pinned: a change of the oracle's walks or weights that moves it is looked at)
QUALIFYING = [(2, 1), (2, 2), (3, 1), (3, 2), (3, 3)]


def test_layer_indices_are_a_bijection_in_the_header_the_library_and_abi_py(pkg, native_lib):
    """count(D) = D (D + 5) / 2 and index(d, s) = (d - 1)(d + 4) / 2 + s for D = 1 .. 24 (BDPT_MAX_DEPTH): index maps
    {(d, s): 1 <= d <= D, 0 <= s <= d + 1} one to one onto range(count(D)), depth after depth, and is -1 outside."""
    abi = pkg.abi
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+drmlt_bdpt_layer_count\s*\(\s*int32_t max_depth\s*\)\s*;", src)
    assert re.search(r"int\s+drmlt_bdpt_layer_index\s*\(\s*int32_t depth\s*,\s*int32_t s\s*\)\s*;", src)
    m = re.search(r"enum\s*\{\s*DRMLT_LAYERS_WEIGHTED\s*=\s*(\d+)\s*,\s*DRMLT_LAYERS_UNWEIGHTED\s*=\s*(\d+)\s*\}", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (abi.LAYERS_WEIGHTED, abi.LAYERS_UNWEIGHTED) == (0, 1)
    count, index = native_lib.drmlt_bdpt_layer_count, native_lib.drmlt_bdpt_layer_index
    for D in range(1, 25):
        assert count(D) == abi.bdpt_layer_count(D) == D * (D + 5) // 2
        got = [index(d, s) for d in range(1, D + 1) for s in range(d + 2)]
        assert got == list(range(count(D)))
        assert got == [abi.bdpt_layer_index(d, s) for d in range(1, D + 1) for s in range(d + 2)]
    for d, s in ((0, 0), (-1, 0), (1, -1), (1, 3), (5, 7), (24, 26), (2 ** 31 - 1, 0), (40000, 1), (-2 ** 31, -2 ** 31)):
        assert index(d, s) == abi.bdpt_layer_index(d, s) == -1, (d, s)
    for D in (0, -1, 40000, 2 ** 31 - 1):
        assert count(D) == abi.bdpt_layer_count(D) == -1, D


def test_the_binding_exposes_render_bdpt_layers(pkg, native_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"int\s+drmlt_render_bdpt_layers\s*\(([^)]*)\)\s*;", src)
    assert m, "include/drmlt_abi.h does not declare drmlt_render_bdpt_layers"
    assert [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == \
        ["drmlt_ctx *ctx", "uint32_t spp", "uint64_t seed", "int32_t mode", "float *out_layers"]
    for name in ("drmlt_render_bdpt_layers", "drmlt_bdpt_layer_count", "drmlt_bdpt_layer_index"):
        assert name in pkg.binding.ABI_SYMBOLS and hasattr(native_lib, name)
    assert native_lib.drmlt_render_bdpt_layers.argtypes == [C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_void_p]
    sig = inspect.signature(pkg.Context.render_bdpt_layers)
    assert list(sig.parameters) == ["self", "spp", "seed", "weighted"]
    assert sig.parameters["seed"].default == 1 and sig.parameters["weighted"].default is True
    out = np.zeros(3, dtype=np.float32)
    assert native_lib.drmlt_render_bdpt_layers(None, 1, 1, 0, out.ctypes.data) == pkg.abi.E_INVALID     # a NULL context, as render_bdpt
    assert np.all(out == 0)
    # the header cites what the layers restate
    text = open(HEADER).read()
    assert "pathsampler.cpp:369-521" in text and "path.cpp:763-1028" in text


def test_the_oracles_strategies_that_can_be_compared(pkg, ob):
    """cornell_c2(16), maxDepth 4, no direct sampling, light image on: mmlt_eval(d, ...) on n = 16 384 uniform points for d = 2 and 3,
    split by the (s, t) it returns and splatted with weight W * H / n into 4 x 4 blocks. A strategy qualifies for the device
    comparison if at most 10 % of its blocks are without variance on this side.
    Measured (share of blocks without variance; mean of the block image): (2, 0) 0.19, 5.4e-06; (2, 1) 0, 0.0258; (2, 2) 0, 0.0223;
    (2, 3) 1, 0 (t = 0); (3, 0) 0.25, 2.6e-06; (3, 1) 0, 0.00587; (3, 2) 0, 0.00545; (3, 3) 0, 0.0103; (3, 4) 1, 0 (t = 0).
    Each depth has s = 1. A strategy with s >= 2 and t >= 2 exists from d = 3 on only -- s + t = d + 1, so at d = 2 the
    connection strategies are (s, t) = (1, 2) and the light image's (2, 1), both of which qualify; no n changes that."""
    contrib = lr.strategy_contributions(pkg, ob)
    assert sorted(contrib) == [(d, s) for d in lr.DEPTHS_COMPARED for s in range(d + 2)]
    for k, c in sorted(contrib.items()):
        print("strategy (d, s) = %s: %.3f of the blocks without variance, block-image mean %.4g"
              % (k, (c.var(axis=0, ddof=1) == 0).mean(), c.mean()))
        assert c.shape == (lr.N_POINTS, 4, 4) and np.isfinite(c).all() and (c >= 0).all()
    q = lr.qualifying(contrib)
    print("qualifying:", q)
    assert q == QUALIFYING
    for d in lr.DEPTHS_COMPARED:
        assert (d, 1) in q
        if d >= 3:
            assert any(s >= 2 and d + 1 - s >= 2 for dd, s in q if dd == d)
        else:
            assert (d, 2) in q                     # d = 2: s >= 2 means t = 1, the light image
    # a t = 0 strategy is never drawn (t >= 1, pathsampler.cpp:107-113)
    assert not contrib[(2, 3)].any() and not contrib[(3, 4)].any()
