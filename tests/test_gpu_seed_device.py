"""Seed selection on the device (csrc/kernels_seed.hip) against its serial host restatement, bit for bit, and drmlt_seed_device /
drmlt_seed_pool_device / drmlt_node_seed_device against the host calls they stand beside: the same picks, the same chains.

The blocked fp64 sums of the device rule and the serial CDF of the host path may disagree on a pick whose uniform lies within
n 2^-51 of a table entry (tests/test_seed_device.py); every comparison between the two asserts first, on the context's own
bootstrap luminances, that no uniform does. Chain states are compared, not films: the film's fp32 atomics have no fixed order."""
import numpy as np
import pytest

from test_seed_device import SEEDS, cases, margin_of

pytestmark = pytest.mark.gpu


def bits(x):
    return np.float64(x).view(np.uint64)


@pytest.fixture(scope="module")
def any_ctx(pkg, native_lib):
    ctx = pkg.Context(pkg.abi.make_config(max_depth=4, direct_samples=-1, work_units=64, luminance_samples=1000), pkg.scenes.cornell_c2(32))
    yield ctx
    ctx.close()


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "weighted"])
def test_device_selection_equals_the_blocked_rule_bit_for_bit(pkg, ob, any_ctx, name):
    lum, w, n_select = cases()[name]
    for seed, stream in SEEDS:
        got, mean, total = any_ctx.select_seeds_device(lum, seed, stream, n_select, weights=w)
        want, mean_h, total_h = pkg.binding.select_seeds_blocked(lum, seed, stream, n_select, weights=w)
        assert np.array_equal(got, want)
        assert bits(mean) == bits(mean_h) and bits(total) == bits(total_h), (mean, mean_h, total, total_h)
        if w is None:   # (the oracle's selectSeeds has no weights; test_seed_device.py asserts the margin of these cases)
            assert np.array_equal(got, ob.select_seeds(lum, seed, stream, n_select))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 65537])
def test_block_edges(pkg, any_ctx, n):
    rng = np.random.default_rng(n)
    lum = np.exp(3 * rng.standard_normal(n)).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    if n > 1:
        lum[rng.integers(0, n, n // 8)] = 0
        w[rng.integers(0, n, n // 8)] = 0
        lum[n // 2] = np.nan
    for weights in (None, w):
        got, mean, total = any_ctx.select_seeds_device(lum, 0x5EED, 1, 300, weights=weights)
        want, mean_h, total_h = pkg.binding.select_seeds_blocked(lum, 0x5EED, 1, 300, weights=weights)
        assert np.array_equal(got, want) and bits(mean) == bits(mean_h) and bits(total) == bits(total_h)
        assert np.all(np.diff(got.astype(np.int64)) >= 0) and got.max() < n


def test_zero_luminance_is_an_error_on_the_device_too(pkg, any_ctx):
    z = np.zeros(300, dtype=np.float32)
    one = z.copy()
    one[17] = 3.0
    for lum, w in ((z, None), (np.full(300, np.nan, dtype=np.float32), None), (one, z)):
        with pytest.raises(pkg.DrmltError) as e:
            any_ctx.select_seeds_device(lum, 0x5EED, 0, 8, weights=w)
        assert e.value.code == pkg.abi.E_ZERO_LUM


def n_boot(cfg, n_select):
    mmlt = cfg.technique == 2   # abi.TECH_MMLT: x 50 per chain, and as many again per depth (drmlt.cpp:456-473)
    return max(cfg.luminance_samples, n_select * (50 if mmlt else 10)) * (cfg.max_depth if mmlt else 1)


def safe_seed(ctx, cfg, n_select, stream=0, first=0x5EED):
    """The first seed from `first` on whose uniforms all keep the margin from the serial table of the context's own bootstrap
    luminances (0x5EED itself wherever this file uses it, as the printed line shows)."""
    for seed in range(first, first + 8):
        lum = ctx.bootstrap_luminances(seed, stream, n_boot(cfg, n_select))
        gap, margin = margin_of(lum, None, seed, stream, n_select)
        print("seed %#x: %d bootstrap samples, min |cdf - xi| = %.3g, margin %.3g" % (seed, lum.size, gap, margin))
        if gap > margin:
            return seed, lum.size
    raise AssertionError("no seed keeps the margin")


def state_bytes(ctx, dim):
    cur, u = ctx.chain_state(dim)
    return cur.tobytes(), u.tobytes()


CONFIGS = {
    "path": (lambda s: s.cornell_c2(64), dict(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=4096), 34),
    "bdpt": (lambda s: s.cornell_c2(32), dict(technique="bdpt", type="orbital", max_depth=6, direct_samples=-1, luminance_samples=20000, work_units=1024), None),
    "mmlt": (lambda s: s.caustic_c5(32), dict(technique="mmlt", type="orbital", max_depth=6, direct_samples=-1, luminance_samples=1000, work_units=2048), 27),
    "pssmlt": (lambda s: s.cornell_c2(64), dict(algo=1, type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=2048), 34),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_seed_device_equals_seed(pkg, native_lib, name):
    scene, kw, dim = CONFIGS[name]
    assert pkg.abi.ALGO_PSSMLT == 1 and pkg.abi.TECH_MMLT == 2
    cfg = pkg.abi.make_config(sample_count=1, **kw)
    with pkg.Context(cfg, scene(pkg.scenes)) as ctx:
        n = cfg.work_units
        dim = dim or ctx.stats().max_dim
        seed, samples = safe_seed(ctx, cfg, n)
        res = []
        for call in (ctx.seed, ctx.seed_device):
            b = call(seed)
            idx, s0 = ctx.seed_indices(), state_bytes(ctx, dim)
            ctx.run(64 * n)
            res.append((b, idx, s0, state_bytes(ctx, dim)))
        (bh, ih, h0, h1), (bd, idv, d0, d1) = res
        assert np.array_equal(ih, idv) and np.all(np.diff(idv.astype(np.int64)) >= 0)
        if name == "mmlt":
            assert len(set(idv % cfg.max_depth)) > 2            # several depths: the depth ordering has something to order
        assert d0 == h0, "chain states differ after seeding"
        assert abs(bd - bh) <= samples * 2.0 ** -51 * bh, (bd, bh)
        assert d1 == h1 and d1 != d0, "chain states differ after 64 mutations per chain"


@pytest.mark.parametrize("units,samples", [(100, 20011), (3, 100)])
def test_odd_sizes(pkg, native_lib, units, samples):
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=samples, work_units=units, sample_count=1)
    with pkg.Context(cfg, pkg.scenes.cornell_c2(32)) as ctx:
        seed, n = safe_seed(ctx, cfg, units)
        assert n == samples
        bh = ctx.seed(seed)
        ih, h0 = ctx.seed_indices(), state_bytes(ctx, 34)
        bd = ctx.seed_device(seed)
        assert np.array_equal(ctx.seed_indices(), ih) and state_bytes(ctx, 34) == h0 and abs(bd - bh) <= n * 2.0 ** -51 * bh


@pytest.mark.parametrize("rule", ["target", "reference"])
def test_two_stage_picks_equal_the_hosts(pkg, native_lib, rule):
    """An importance map with a horizontal ramp of contrast 100. Under seed_rule = TARGET the table is built from the luminances under
    the map (second half of the bootstrap buffer, which no call hands out: the margin is asserted for the plain luminances, under
    REFERENCE the very table that is searched)."""
    imp = np.tile(np.linspace(0.01, 1.0, 32, dtype=np.float32), (32, 1))
    cfg = pkg.abi.make_config(type="orbital", max_depth=6, direct_samples=-1, luminance_samples=20000, work_units=2048, sample_count=1, seed_rule=rule)
    res = []
    with pkg.Context(cfg, pkg.scenes.cornell_c2(32)) as ctx:
        seed, n = safe_seed(ctx, cfg, 2048)
        ctx.set_importance_map(imp)
        for call in (ctx.seed, ctx.seed_device):
            b = call(seed)
            res.append((b, ctx.seed_indices(), state_bytes(ctx, 34)))
    (bh, ih, sh), (bd, idv, sd_) = res
    assert np.array_equal(ih, idv) and sh == sd_ and abs(bd - bh) <= n * 2.0 ** -51 * bh
    plain = pkg.abi.make_config(type="orbital", max_depth=6, direct_samples=-1, luminance_samples=20000, work_units=2048, sample_count=1)
    with pkg.Context(plain, pkg.scenes.cornell_c2(32)) as ctx:   # the ramp moves the seeds under TARGET, and only there
        ctx.seed_device(seed)
        assert np.array_equal(ctx.seed_indices(), idv) == (rule == "reference")


def test_a_map_that_is_zero_where_the_scene_contributes(pkg, native_lib):
    sd = pkg.scenes.cornell_c2(32)
    cfg = pkg.abi.make_config(technique="path", type="orbital", max_depth=6, direct_samples=-1, work_units=256, luminance_samples=5000)
    msgs = []
    for device in (False, True):
        with pkg.Context(cfg, sd) as ctx:
            ctx.set_importance_map(np.zeros((32, 32), dtype=np.float32))
            with pytest.raises(pkg.DrmltError, match="under the importance map") as e:
                (ctx.seed_device if device else ctx.seed)(1)
            assert e.value.code == pkg.abi.E_ZERO_LUM
            msgs.append(str(e.value))
    assert msgs[0] == msgs[1]     # (the average luminance in the message is printed with %g: six digits)


def test_pool_slices(pkg, native_lib):
    sd = pkg.scenes.cornell_c2(32)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=1000, work_units=1024, sample_count=1)
    with pkg.Context(cfg, sd) as c0, pkg.Context(cfg, sd) as c1:
        seed, n = safe_seed(c0, cfg, 2048)
        host = []
        for c, first in ((c0, 0), (c1, 1024)):
            b = c.seed_pool(seed, first, 2048)
            host.append((b, c.seed_indices(), state_bytes(c, 34)))
        for (bh, ih, sh), (c, first) in zip(host, ((c0, 0), (c1, 1024))):
            bd = c.seed_pool_device(seed, first, 2048)
            assert np.array_equal(c.seed_indices(), ih) and state_bytes(c, 34) == sh and abs(bd - bh) <= n * 2.0 ** -51 * bh
        assert host[0][1][-1] <= host[1][1][0]      # one sorted list, cut in two
        with pytest.raises(pkg.DrmltError, match="does not cover"):
            c1.seed_pool_device(seed, 1025, 2048)


def test_node_seed_device(pkg, native_lib, monkeypatch):
    sd = pkg.scenes.cornell_c2(32)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=1000, work_units=1024, sample_count=1)
    monkeypatch.setenv("DRMLT_TEST_HOOKS", "1")
    monkeypatch.setenv("DRMLT_NODE_DEVICES", "0,0")
    node = pkg.Node(cfg, sd, device_mask=1)
    monkeypatch.delenv("DRMLT_NODE_DEVICES")
    assert node.device_count == 2
    seed, n = safe_seed(node.context(0), cfg, 2048)
    bh = node.seed(seed)
    host = [(node.context(r).seed_indices(), state_bytes(node.context(r), 34)) for r in range(2)]
    bd = node.seed_device(seed)
    for r in range(2):
        assert np.array_equal(node.context(r).seed_indices(), host[r][0]) and state_bytes(node.context(r), 34) == host[r][1]
    assert abs(bd - bh) <= n * 2.0 ** -51 * bh
    node.close()


def test_state_after_mixed_calls(pkg, native_lib):
    """seed_device twice gives the same chains; either call after the other leaves what it alone would; seed_ms grows with every
    call. (The replay check runs inside every seed_device call of this file: a seed luminance gathered from the wrong sample makes
    it return DRMLT_E_REPLAY, as on the host path.)"""
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=1024, sample_count=1)
    with pkg.Context(cfg, pkg.scenes.cornell_c2(32)) as ctx:
        seed, n = safe_seed(ctx, cfg, 1024)
        other, _ = safe_seed(ctx, cfg, 1024, first=seed + 1)
        ms = [ctx.stats().seed_ms]
        seen = {}
        for call, s in ((ctx.seed_device, seed), (ctx.seed_device, seed), (ctx.seed, other), (ctx.seed_device, seed), (ctx.seed_device, other), (ctx.seed, seed)):
            b = call(s)
            ctx.run(16 * 1024)      # the next seeding starts from a context that has run
            b2 = call(s)
            assert b2 == b
            ms.append(ctx.stats().seed_ms)
            now = (ctx.seed_indices().tobytes(), state_bytes(ctx, 34))
            assert seen.setdefault(s, now) == now, "the context's state depends on what was called before"
            st = ctx.stats()
            assert st.mutations >= 0 and ms[-1] > ms[-2]
        assert seen[seed] != seen[other]
        ctx.run(1024 * 8)
        assert np.isfinite(ctx.develop()).all()
