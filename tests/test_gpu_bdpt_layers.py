"""drmlt_render_bdpt_layers on the device (k_layers_bdpt): render_bdpt's samples split by path length and strategy, layer
(d, s) holding the connections of s emitter-side and t = d + 1 - s sensor-side vertices. What it refuses; that the weighted layers
are render_bdpt's image and which layers must be empty; single strategies against a closed form, unweighted, and their weights
summing to one; every strategy the oracle can resolve against the oracle's own per-strategy estimate; that a context is left as it
was; a traversed scene."""
import numpy as np
import pytest

import bdpt_layers_ref as lr
import render_bdpt_scenes as rs

pytestmark = pytest.mark.gpu
lum = rs.lum
DEPTHS = dict(max_depth=6, rr_depth=4, direct_samples=-1)


def _cfg(pkg, **kw):
    base = dict(technique="bdpt", type="orbital", work_units=16384, luminance_samples=20000, **DEPTHS)
    base.update(kw)
    return pkg.abi.make_config(**base)


def _layers_are_the_image(pkg, ctx, tag, spp=64, seed=11):
    """Test 2's identity on `ctx`: the weighted layers, summed over the layer axis in fp64 on the host, against render_bdpt of the
    same seed, rtol 1e-4 per pixel and channel. Both sides add the same non-negative fp32 terms in different orders (the image sums
    a sample's t >= 2 cells before the filter, the layers put each through it): a pixel that receives n adds is off by at most
    n * 2^-24 relative, so 1e-4 allows about 1 600 adds where a pixel here has 64 * 7 on average. Returns (layers, image), fp64."""
    layers = ctx.render_bdpt_layers(spp, seed=seed).astype(np.float64)
    img = ctx.render_bdpt(spp, seed=seed).astype(np.float64)
    assert layers.shape == (pkg.abi.bdpt_layer_count(ctx.cfg.max_depth),) + img.shape
    total = layers.sum(axis=0)
    assert np.isfinite(layers).all() and (layers >= 0).all() and img.mean() > 0
    rel = np.abs(total - img) / np.maximum(img, 1e-300)
    print("%s: sum of the %d weighted layers against render_bdpt(%d): largest difference %.3g relative (pixels lit: %d of %d)"
          % (tag, len(layers), spp, rel[img > 0].max(), (img > 0).all(axis=2).sum(), img.shape[0] * img.shape[1]))
    assert not total[img == 0].any()
    np.testing.assert_allclose(total, img, rtol=1e-4, atol=0)
    return layers, img


def _layer(pkg, stack, d, s):
    return stack[..., pkg.abi.bdpt_layer_index(d, s), :, :, :]


# ---------------------------------------------------------------- 1. refusals
def test_refusals_say_what_is_wrong(pkg, native_lib):
    E = pkg.abi.E_INVALID
    sd = pkg.scenes.cornell_c2(16)
    for kw in (dict(technique="path", work_units=64), dict(technique="mmlt", work_units=64)):
        with pkg.Context(_cfg(pkg, **kw), sd) as ctx:
            with pytest.raises(pkg.binding.DrmltError, match="technique=bdpt") as e:
                ctx.render_bdpt_layers(4)
            assert e.value.code == E
    with pkg.Context(_cfg(pkg, work_units=64), sd) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="spp is 0") as e:
            ctx.render_bdpt_layers(0)
        assert e.value.code == E
        for mode in (2, -1):
            with pytest.raises(pkg.binding.DrmltError, match="unknown mode %d" % mode) as e:
                ctx.render_bdpt_layers(1, weighted=mode)
            assert e.value.code == E
        for weighted in (True, False, pkg.abi.LAYERS_UNWEIGHTED):
            assert ctx.render_bdpt_layers(1, weighted=weighted).shape == (pkg.abi.bdpt_layer_count(6), 16, 16, 3) == (33, 16, 16, 3)
    # 64 spp on 8192 x 8192 pixels are exactly 2^32 samples: refused before the layered film (26 GB here) is asked for
    with pkg.Context(_cfg(pkg, work_units=64), rs.two_rectangles(pkg, 8192)) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="different seeds") as e:
            ctx.render_bdpt_layers(64)
        assert e.value.code == E and "32 bits" in str(e.value)


# ---------------------------------------------------------------- 2. the layers are the image
@pytest.mark.parametrize("light_image", [1, 0], ids=["lightimage", "nolightimage"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
def test_the_weighted_layers_sum_to_render_bdpts_image(pkg, native_lib, direct, light_image):
    """cornell_c2(16), maxDepth 6, 64 spp: _layers_are_the_image's identity and bound. Every t = 0 layer is exactly zero (a pinhole
    cannot be hit); without the light image every t = 1 layer is; with it some t = 1 layer is not. The same seed again agrees within
    rtol 1e-5 (only the order of the fp32 atomics differs), another seed does not.
    Measured on the MI355X (largest difference of the sum from the image; of the same seed again; direct sampling on / off): 1.95e-06,
    3.6e-07 / 1.52e-06, 4.7e-07 with the light image; 4.2e-07, 2.3e-07 / 4.4e-07, 2.5e-07 without. Depth 1 carries 0.54 of the image
    (0.57 without the light image), depth 2 0.25, depth 3 0.11, depth 6 0.013."""
    abi = pkg.abi
    sd = pkg.scenes.cornell_c2(16)
    with pkg.Context(_cfg(pkg, no_direct_sampling=1 - direct, no_light_image=1 - light_image), sd) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "cornell_c2(16) direct %d light image %d" % (direct, light_image))
        again = ctx.render_bdpt_layers(64, seed=11).astype(np.float64)
        other = ctx.render_bdpt_layers(64, seed=12).astype(np.float64)
    for d in range(1, 7):
        assert not _layer(pkg, layers, d, d + 1).any(), d                    # t = 0
        t1 = _layer(pkg, layers, d, d)
        assert t1.any() if light_image else not t1.any(), d                  # t = 1 (d = 1: the lamp's own light-image splat)
        assert _layer(pkg, layers, d, 1).any() if d >= 2 else True           # s = 1 carries light at every depth from 2 on
    print("    the same seed again: largest difference %.3g relative" % (np.abs(again - layers)[layers > 0] / layers[layers > 0]).max())
    np.testing.assert_allclose(again, layers, rtol=1e-5, atol=0)
    assert not np.array_equal(other, layers) and abs(other.sum() - layers.sum()) > 0
    share = layers.sum(axis=(1, 2, 3)) / layers.sum()
    print("    share of the image by depth: " + ", ".join("d=%d %.4f" % (d, share[abi.bdpt_layer_index(d, 0):abi.bdpt_layer_index(d, d + 1) + 1].sum())
                                                         for d in range(1, 7)))


def test_separate_direct_light_empties_the_layers_up_to_depth_two(pkg, native_lib):
    """direct_samples = 16: the chains, render_bdpt and the layers exclude depth <= 2 (render_direct carries it). Every d <= 2
    layer is exactly zero, the deeper ones are render_bdpt's image of that context.
    Measured on the MI355X: largest difference 5.7e-07 relative."""
    sd = pkg.scenes.cornell_c2(16)
    with pkg.Context(_cfg(pkg, direct_samples=16), sd) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "cornell_c2(16) direct_samples 16")
    first = pkg.abi.bdpt_layer_index(3, 0)
    assert first == 7 and not layers[:first].any() and layers[first:].any()


# ---------------------------------------------------------------- 3. one strategy against the closed form
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
def test_single_strategies_match_the_closed_form_on_the_lamp_lit_plane(pkg, native_lib, direct):
    """render_bdpt_scenes.lamp_plane (a view-filling diffuse plane under a triangle light of edge 1e-5 outside the view), maxDepth 2,
    K = 16 seeds of 256 spp. The depth-2 light of a pixel is the closed form's; UNWEIGHTED, strategy (d, s) = (2, 1) -- connect the
    camera's hit to a light sample -- and strategy (2, 2) -- connect the light path's hit to the camera -- each estimate it alone:
    every pixel within 6 of its standard error measured over the K images, the image mean within 4 of its own. WEIGHTED, layers
    (2, 0) + (2, 1) + (2, 2) together meet it under test_lamp_lit_plane_matches_the_closed_form's bounds (z < 6, mean within 1e-3):
    the three weights sum to one. Every d = 1 layer is exactly zero, the lamp is out of view. Unweighted (2, 0) -- the camera path
    hits the lamp by itself -- is printed only: hits on a lamp of edge 1e-5 are too rare to test.
    Measured on the MI355X (direct sampling on; off gives the same figures to three digits, the s = 1 vertex of a light this small is
    the same point either way): unweighted (2, 1) max z 4.86, mean off by 7.2e-04 = 1.84 standard errors; unweighted (2, 2) 3.65,
    8.2e-04 = 0.96; weighted sum 4.94, 5.9e-04 (2.02 standard errors). Weighted shares of (2, 0), (2, 1), (2, 2): 0, 0.908, 0.091;
    unweighted (2, 0): no pixel hit in 16 renders."""
    K, spp = 16, 256
    sd = rs.lamp_plane(pkg)
    cfg = _cfg(pkg, max_depth=2, no_direct_sampling=1 - direct)
    with pkg.Context(cfg, sd) as ctx:
        wt = np.array([ctx.render_bdpt_layers(spp, seed=100 + k) for k in range(K)], dtype=np.float64)
        un = np.array([ctx.render_bdpt_layers(spp, seed=100 + k, weighted=False) for k in range(K)], dtype=np.float64)
    want = rs.lamp_plane_closed_form(pkg)
    assert wt.shape == un.shape == (K, 7, 32, 32, 3)

    def held(tag, imgs):
        mean, se = imgs.mean(axis=0), imgs.std(axis=0, ddof=1) / np.sqrt(K)
        z = np.abs(mean - want) / se
        per = imgs.mean(axis=(1, 2, 3))
        mse = per.std(ddof=1) / np.sqrt(K)
        zm, rel = abs(per.mean() - want.mean()) / mse, abs(per.mean() - want.mean()) / want.mean()
        print("lamp plane direct %d, %s: max z %.2f, image mean off by %.3g relative = %.2f of its standard errors, median rel se %.3g"
              % (direct, tag, z.max(), rel, zm, np.median(se / want)))
        assert np.all(se > 0) and z.max() < 6, z.max()
        return zm, rel

    for s in (1, 2):
        zm, _ = held("unweighted (2, %d)" % s, _layer(pkg, un, 2, s))
        assert zm < 4, zm
    _, rel = held("weighted (2, 0) + (2, 1) + (2, 2)", _layer(pkg, wt, 2, 0) + _layer(pkg, wt, 2, 1) + _layer(pkg, wt, 2, 2))
    assert rel < 1e-3, rel
    hits = _layer(pkg, un, 2, 0)
    print("    unweighted (2, 0): mean %.4g against the closed form's %.4g, pixels hit in %d renders: %d; weighted shares of (2, 0), (2, 1), (2, 2): %s"
          % (hits.mean(), want.mean(), K, (hits.sum(axis=(0, 3)) > 0).sum(),
             ", ".join("%.4g" % (_layer(pkg, wt, 2, s).mean() / want.mean()) for s in (0, 1, 2))))
    for s in range(3):
        assert not _layer(pkg, wt, 1, s).any() and not _layer(pkg, un, 1, s).any()
    assert not _layer(pkg, wt, 2, 3).any() and not _layer(pkg, un, 2, 3).any()       # t = 0


# ---------------------------------------------------------------- 4. strategy by strategy against the oracle
def test_weighted_layers_match_the_oracle_strategy_by_strategy(pkg, ob, native_lib):
    """cornell_c2(16), maxDepth 4, no direct sampling, light image on (bdpt_layers_ref.config). For every strategy (d, s) that
    qualifies on the oracle's side (tests/test_bdpt_layers.py: (2, 1), (2, 2), (3, 1), (3, 2), (3, 3)), K = 16 seeds of the weighted
    layer at 64 spp in 4 x 4 blocks against the fp64 oracle's mmlt_eval points of that strategy: every kept block within 6 combined
    standard errors (oracle: from its per-point contributions; device: from the K images), the layer's mean within 3. A block
    without variance on the oracle's side is left out, at most 10 % of a strategy's. MMLT picks one of a depth's strategies
    uniformly and multiplies by their number, which cancel; its weights are miWeight's without the sampleDirect ratios, hence no
    direct sampling here.
    Measured on the MI355X (max block z, z of the layer means; no block left out anywhere): (2, 1) 2.55, 1.23; (2, 2) 5.37, 0.69;
    (3, 1) 2.81, 0.60; (3, 2) 1.83, 1.28; (3, 3) 1.59, 0.21. The 5.37 of the light-image strategy (2, 2) is close to the bound: its
    oracle side is heavy-tailed (a block's relative standard error is still 0.13 at n = 262 144 points). Measured apart from this test
    with sixteen times the samples on both sides (n = 262 144, K = 64 seeds of 256 spp): (2, 2) max z 2.18, no strategy above 2.35 --
    noise of the variance estimate at this n, not a bias. The bound stays."""
    K, n = 16, lr.N_POINTS
    contrib = lr.strategy_contributions(pkg, ob)
    q = lr.qualifying(contrib)
    assert len(q) >= 4
    with pkg.Context(lr.config(pkg), pkg.scenes.cornell_c2(lr.RES)) as ctx:
        stacks = np.array([ctx.render_bdpt_layers(64, seed=500 + k) for k in range(K)], dtype=np.float64)
    worst = []
    for d, s in q:
        c = contrib[(d, s)]
        mo, vo = c.mean(axis=0), c.var(axis=0, ddof=1)
        bg = np.array([rs.blocks_of(img) for img in _layer(pkg, stacks, d, s)])
        mg, vg = bg.mean(axis=0), bg.var(axis=0, ddof=1)
        keep = vo > 0
        z = np.abs(mg - mo)[keep] / np.sqrt(vo[keep] / n + vg[keep] / K)
        to, tg = c.mean(axis=(1, 2)), bg.mean(axis=(1, 2))
        zm = abs(tg.mean() - to.mean()) / np.sqrt(to.var(ddof=1) / n + tg.var(ddof=1) / K)
        print("layer (d, s) = (%d, %d) vs the oracle's strategy: %d of %d blocks left out, max z %.2f, layer means %.6g / %.6g, z %.2f"
              % (d, s, (~keep).sum(), keep.size, z.max(), tg.mean(), to.mean(), zm))
        worst.append(((d, s), (~keep).mean(), z.max(), zm))
    for k, out, z, zm in worst:
        assert out <= 0.1, (k, out)
        assert z < 6, (k, z)
        assert zm < 3, (k, zm)


# ---------------------------------------------------------------- 5. the context is left as it was
@pytest.mark.parametrize("algo", [0, 1], ids=["drmlt", "pssmlt"])
def test_layers_between_two_runs_change_nothing(pkg, native_lib, algo):
    """seed, run, render_bdpt_layers, run against seed, run, run with 1 024 chains on cornell_c2(16): the chain states bit for bit
    (u, luminance, positions), the counters equal, the films within rtol 2e-4, atol 1e-6 (atomics in another order) --
    test_a_render_between_two_runs_changes_nothing's bounds. The layers' scratch is render_bdpt's: the workspace columns and list
    slot 1, which every mutation writes before it reads."""
    sd = pkg.scenes.cornell_c2(16)
    out = []
    for render in (True, False):
        with pkg.Context(_cfg(pkg, algo=algo, work_units=1024), sd) as ctx:
            b = ctx.seed(0xABCD)
            ctx.run(1024 * 32)
            if render:
                layers = ctx.render_bdpt_layers(16, seed=3)
                assert lum(layers.sum(axis=0, dtype=np.float64)).mean() == pytest.approx(b, rel=0.2)
            ctx.run(1024 * 32)
            st = ctx.stats()
            cur, u = ctx.chain_state(st.max_dim)
            counters = {k: v for k, v in st.as_dict().items() if k not in ("kernel_ms", "seed_ms")}
            out.append((b, cur, u, counters, ctx.film()))
    (ba, ca, ua, sa, fa), (bb, cb, ub, sb, fb) = out
    assert ba == bb and sa == sb, (sa, sb)
    assert sa["mutations"] == 2 * 1024 * 32
    assert ua.tobytes() == ub.tobytes() and ca.tobytes() == cb.tobytes()
    np.testing.assert_allclose(fa, fb, rtol=2e-4, atol=1e-6)


# ---------------------------------------------------------------- 6. a traversed scene
def test_the_weighted_layers_sum_to_the_image_on_a_traversed_scene(pkg, native_lib):
    """The 2000-triangle soup (eval_bdpt traverses a BVH; the stacks and their overflow area are sized by the grid, as
    render_bdpt's): _layers_are_the_image's identity and bound.
    Measured on the MI355X: largest difference 8.7e-07 relative."""
    sd = pkg.scenes.triangle_soup(2000, res=16)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        _layers_are_the_image(pkg, ctx, "soup(2000, 16)")
