"""drmlt_render_mmlt and drmlt_render_mmlt_layers on the device (k_render_mmlt, k_layers_mmlt): technique=mmlt's own reference,
sample i the bootstrap's sample i, depth (i % maxDepth) + 1, layer (d, s) holding the depth-d samples that drew strategy s. What
they refuse; that the weighted layers are render_mmlt's image; that a sample is the bootstrap's sample and the scale 1 / spp; what
stays empty; every strategy the oracle can resolve against the oracle's own per-strategy estimate; every layer against the
bidirectional layers; that a context is left as it was; that the chain seeds follow the layers' depth shares; a traversed scene."""
import ctypes as C

import numpy as np
import pytest

import bdpt_layers_ref as lr
import render_bdpt_scenes as rs

pytestmark = pytest.mark.gpu
lum = rs.lum


def _cfg(pkg, **kw):
    """bdpt_layers_ref.config with technique=mmlt: maxDepth 4, rrDepth 4, no separate direct light, light image on."""
    base = dict(technique="mmlt", work_units=64)
    base.update(kw)
    return lr.config(pkg, **base)


def _layer(pkg, stack, d, s):
    return stack[..., pkg.abi.bdpt_layer_index(d, s), :, :, :]


def _layers_are_the_image(pkg, ctx, tag, spp=64, seed=11):
    """The weighted layers, summed over the layer axis in fp64 on the host, against render_mmlt of the same seed, per pixel and
    channel within (layers + 1) * 2^-24 of the sum: both sides add the same fp32 products in fp64 on the device and round once per
    film, the layers' roundings and the image's are all that differs. Returns (layers, image), fp64."""
    layers = ctx.render_mmlt_layers(spp, seed=seed).astype(np.float64)
    img = ctx.render_mmlt(spp, seed=seed).astype(np.float64)
    assert layers.shape == (pkg.abi.bdpt_layer_count(ctx.cfg.max_depth),) + img.shape
    total = layers.sum(axis=0)
    assert np.isfinite(layers).all() and (layers >= 0).all() and img.mean() > 0
    err = np.abs(total - img)
    print("%s: sum of the %d weighted layers against render_mmlt(%d): largest difference %.3g of the bound, %.3g relative (pixels lit: %d of %d)"
          % (tag, len(layers), spp, (err / np.maximum((len(layers) + 1) * 2.0 ** -24 * total, 1e-300))[total > 0].max(),
             (err / np.maximum(total, 1e-300))[total > 0].max(), (img > 0).all(axis=2).sum(), img.shape[0] * img.shape[1]))
    assert not total[img == 0].any() and not img[total == 0].any()
    assert np.all(err <= (len(layers) + 1) * 2.0 ** -24 * total)
    return layers, img


# ---------------------------------------------------------------- 1. refusals
def test_refusals_say_what_is_wrong(pkg, native_lib):
    abi = pkg.abi
    E = abi.E_INVALID
    sd = pkg.scenes.cornell_c2(16)
    out = np.zeros(abi.bdpt_layer_count(4) * 16 * 16 * 3, dtype=np.float32)

    def raw(ctx, layered, spp, mode=0, ptr=out.ctypes.data):
        L = ctx.L
        rc = L.drmlt_render_mmlt_layers(ctx.h, spp, 1, mode, ptr) if layered else L.drmlt_render_mmlt(ctx.h, spp, 1, ptr)
        return rc, L.drmlt_last_error(ctx.h).decode()

    for tech, other in (("path", "render_pt"), ("bdpt", "render_bdpt")):
        with pkg.Context(_cfg(pkg, technique=tech), sd) as ctx:
            for layered in (False, True):
                ref = other + ("_layers" if layered else "")
                with pytest.raises(pkg.binding.DrmltError, match=r"technique=mmlt.*technique=%s \(%s is" % (tech, ref)) as e:
                    ctx.render_mmlt_layers(4) if layered else ctx.render_mmlt(4)
                assert e.value.code == E
                rc, msg = raw(ctx, layered, 4)
                assert rc == E and "technique=mmlt" in msg and "technique=%s" % tech in msg and "drmlt_" + ref in msg, msg
    with pkg.Context(_cfg(pkg), sd) as ctx:
        for layered, call in ((False, lambda: ctx.render_mmlt(0)), (True, lambda: ctx.render_mmlt_layers(0))):
            with pytest.raises(pkg.binding.DrmltError, match="spp is 0") as e:
                call()
            assert e.value.code == E
            rc, msg = raw(ctx, layered, 0)
            assert rc == E and "spp is 0" in msg
            assert raw(ctx, layered, 1, ptr=None)[0] == E                                    # NULL output
        for mode in (2, -1):
            with pytest.raises(pkg.binding.DrmltError, match="unknown mode %d" % mode) as e:
                ctx.render_mmlt_layers(1, weighted=mode)
            assert e.value.code == E
            rc, msg = raw(ctx, True, 1, mode=mode)
            assert rc == E and "unknown mode %d" % mode in msg
        assert not out.any()                                                                  # no refusal wrote anything
        for weighted in (True, False, abi.LAYERS_UNWEIGHTED):
            assert ctx.render_mmlt_layers(1, weighted=weighted).shape == (abi.bdpt_layer_count(4), 16, 16, 3) == (18, 16, 16, 3)
        assert ctx.render_mmlt(1).shape == (16, 16, 3)
    # 16 spp on 8192 x 8192 pixels and 4 depths are exactly 2^32 samples: refused before any film is asked for
    with pkg.Context(_cfg(pkg), rs.two_rectangles(pkg, 8192)) as ctx:
        for layered, call in ((False, lambda: ctx.render_mmlt(16)), (True, lambda: ctx.render_mmlt_layers(16))):
            with pytest.raises(pkg.binding.DrmltError, match="different seeds") as e:
                call()
            assert e.value.code == E and "32 bits" in str(e.value)
            rc, msg = raw(ctx, layered, 16, ptr=C.c_void_p(8))                               # (refused before the pointer is used)
            assert rc == E and "average several calls with different seeds" in msg


# ---------------------------------------------------------------- 2. the layers are the image
@pytest.mark.parametrize("filt", ["box", "gaussian"])
@pytest.mark.parametrize("no_light_image", [0, 1], ids=["lightimage", "nolightimage"])
def test_the_weighted_layers_sum_to_render_mmlts_image(pkg, native_lib, no_light_image, filt):
    """cornell_c2(16), maxDepth 4, 64 spp: _layers_are_the_image's identity and bound. Every d = 1 and every t = 0 layer is exactly
    zero; without the light image every t = 1 layer is, with it every t = 1 layer from d = 2 on carries light, as every other layer does.
    Measured on the MI355X (largest difference as a share of the bound; relative): box 0.084, 9.5e-08 with the light image and 0.081,
    9.2e-08 without; Gaussian 0.072, 8.1e-08 and 0.076, 8.6e-08."""
    abi = pkg.abi
    sd = pkg.scenes.cornell_c2(16, filt=abi.FILTER_BOX if filt == "box" else abi.FILTER_GAUSSIAN)
    with pkg.Context(_cfg(pkg, no_light_image=no_light_image), sd) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "cornell_c2(16) %s no_light_image %d" % (filt, no_light_image))
    for d in range(1, 5):
        assert not _layer(pkg, layers, d, d + 1).any(), d                        # t = 0
        t1 = _layer(pkg, layers, d, d)
        assert t1.any() if (not no_light_image and d >= 2) else not t1.any(), d  # t = 1
        for s in range(d):
            assert _layer(pkg, layers, d, s).any() if d >= 2 else not _layer(pkg, layers, d, s).any(), (d, s)


# ---------------------------------------------------------------- 3. a sample is the bootstrap's sample; the scale
def test_samples_are_the_bootstraps_and_the_scale_is_one_over_spp(pkg, native_lib):
    """cornell_c2(8), box filter, maxDepth 3, spp 4: n = 4 * 64 * 3 = 768 samples. For each depth d, spp times the luminance of the
    depth-d layers summed over pixels and strategies is the sum of bootstrap_luminances(seed, 0, n)[i] over i % 3 == d - 1 with a
    finite positive luminance, times the box filter's weight of a splat, rel 1e-5 (a handful of fp32 roundings on non-negative
    terms). That weight is not 1: the reference's box filter has radius 0.5 + 1e-5 (box.cpp) and its table is normalised to
    integrate to one (rfilter.cpp:37-55, scene_prep.h: build_filter), so each axis weighs 1 / (1 + 2e-5) and a splat
    (1 + 2e-5)^-2 = 1 - 4e-5 -- measured on the MI355X before the factor was in the test: 11.3691388 against 11.3695941 at depth 2,
    4.0e-5 relative. The factor is the filter's, computed here from its definition; the bound stays. With it: 5.0e-08 relative at
    depth 2 (94 samples carry light) and 5.8e-08 at depth 3 (79). No splat fell outside the film in these samples (the light-image
    position is tested against the film before it is returned, cam_sample_position; the sensor position lies on it by
    construction); one within 1e-5 of a pixel's edge, where that radius puts it into both pixels, would show as a whole sample's
    luminance. The d = 1 and t = 0 layers are exactly zero; the same call twice gives the same bits."""
    abi = pkg.abi
    spp, D, seed = 4, 3, 77
    sd = pkg.scenes.cornell_c2(8)
    with pkg.Context(_cfg(pkg, max_depth=D, rr_depth=D), sd) as ctx:
        n = spp * 8 * 8 * D
        layers = ctx.render_mmlt_layers(spp, seed=seed)
        again = ctx.render_mmlt_layers(spp, seed=seed)
        img, img2 = ctx.render_mmlt(spp, seed=seed), ctx.render_mmlt(spp, seed=seed)
        boot = ctx.bootstrap_luminances(seed, 0, n).astype(np.float64)
    assert layers.tobytes() == again.tobytes() and img.tobytes() == img2.tobytes()
    assert layers.shape == (abi.bdpt_layer_count(D), 8, 8, 3)
    layers = layers.astype(np.float64)
    ok = np.isfinite(boot) & (boot > 0)
    w = (1.0 / (2.0 * (0.5 + 1e-5))) ** 2             # a splat's weight under the box filter: both axes' table value
    for d in range(1, D + 1):
        got = spp * sum(lum(_layer(pkg, layers, d, s)).sum() for s in range(d + 2))
        want = w * boot[(np.arange(n) % D == d - 1) & ok].sum()
        print("depth %d: spp * layers' luminance %.9g, the bootstrap's %.9g (%d samples carry light), relative difference %.3g"
              % (d, got, want, ((np.arange(n) % D == d - 1) & ok).sum(), abs(got - want) / max(want, 1e-300)))
        assert got == pytest.approx(want, rel=1e-5)
        assert not _layer(pkg, layers, d, d + 1).any()
    assert not layers[:abi.bdpt_layer_index(2, 0)].any() and boot[np.arange(n) % D == 0].sum() == 0
    assert spp * lum(img.astype(np.float64)).sum() == pytest.approx(w * boot[ok].sum(), rel=1e-5)


# ---------------------------------------------------------------- 4. separate direct light
def test_separate_direct_light_empties_the_layers_up_to_depth_two(pkg, native_lib):
    """direct_samples = 16: depth <= 2 is excluded (pathsampler.cpp:279). Every d <= 2 layer is exactly zero, the others (t >= 1) are not."""
    abi = pkg.abi
    with pkg.Context(_cfg(pkg, direct_samples=16), pkg.scenes.cornell_c2(16)) as ctx:
        layers, _ = _layers_are_the_image(pkg, ctx, "cornell_c2(16) direct_samples 16")
    first = abi.bdpt_layer_index(3, 0)
    assert first == 7 and not layers[:first].any()
    for d in (3, 4):
        for s in range(d + 1):
            assert _layer(pkg, layers, d, s).any(), (d, s)


# ---------------------------------------------------------------- 5. strategy by strategy against the oracle
def test_weighted_layers_match_the_oracle_strategy_by_strategy(pkg, ob, native_lib):
    """tests/test_gpu_bdpt_layers.py::test_weighted_layers_match_the_oracle_strategy_by_strategy's protocol and bounds with the
    device side K = 16 seeds of render_mmlt_layers(64): for every strategy (d, s) that qualifies on the oracle's side ((2, 1),
    (2, 2), (3, 1), (3, 2), (3, 3): tests/test_bdpt_layers.py) the weighted layer in 4 x 4 blocks against the fp64 oracle's mmlt_eval
    points of that strategy, every kept block within 6 combined standard errors, the layer's mean within 3; a block without variance
    on the oracle's side is left out, at most 10 % of a strategy's. Here both sides are the same estimator: a sample that drew another
    strategy is a zero of this one on both, and the number of strategies is in the splat on both.
    Measured on the MI355X (max block z, z of the layer means; no block left out anywhere): (2, 1) 2.78, 1.25; (2, 2) 5.18, 1.02;
    (3, 1) 2.38, 0.72; (3, 2) 1.54, 1.57; (3, 3) 1.72, 0.17. (2, 2), the light-image strategy, is close to the bound as it is for the bidirectional
    layers (5.37 there): its oracle side is heavy-tailed, see that test's docstring. The bound stays."""
    K, n = 16, lr.N_POINTS
    contrib = lr.strategy_contributions(pkg, ob)
    q = lr.qualifying(contrib)
    assert len(q) >= 4
    with pkg.Context(_cfg(pkg), pkg.scenes.cornell_c2(lr.RES)) as ctx:
        stacks = np.array([ctx.render_mmlt_layers(64, seed=500 + k) for k in range(K)], dtype=np.float64)
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


# ---------------------------------------------------------------- 6. against the bidirectional layers
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
def test_layers_match_the_bidirectional_layers(pkg, native_lib, weighted):
    """cornell_c2(16), maxDepth 4, no direct sampling, light image on: K = 16 seeds of render_bdpt_layers(64) on a bdpt context against
    K = 16 seeds of render_mmlt_layers(64) on an mmlt context, every layer (d, s) with 2 <= d <= 4 and t >= 1 in 4 x 4 blocks, both
    variances from the K images: every kept block within 6 combined standard errors, the layer's mean within 3. A block without
    variance on both sides is left out, at most 10 % of a layer's; a layer on which the bidirectional side alone has more such
    blocks is named and not compared (bdpt_layers_ref.qualifying's rule).
    Measured on the MI355X: no block left out and no layer dropped, all twelve layers compared. Weighted: largest block z 3.28 and
    largest z of the means 2.08, both on (4, 3); the others at most 2.65 and 1.28. Unweighted: largest block z 4.24 on (3, 0), 3.00 on
    (3, 2), the others at most 2.92; largest z of the means 1.88 on (3, 1)."""
    K = 16
    sd = pkg.scenes.cornell_c2(lr.RES)
    with pkg.Context(lr.config(pkg), sd) as ctx:
        bd = np.array([ctx.render_bdpt_layers(64, seed=700 + k, weighted=weighted) for k in range(K)], dtype=np.float64)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        mm = np.array([ctx.render_mmlt_layers(64, seed=900 + k, weighted=weighted) for k in range(K)], dtype=np.float64)
    assert bd.shape == mm.shape
    worst, dropped = [], []
    for d in range(2, lr.MAX_DEPTH + 1):
        for s in range(d + 1):
            bb = np.array([rs.blocks_of(img) for img in _layer(pkg, bd, d, s)])
            bm = np.array([rs.blocks_of(img) for img in _layer(pkg, mm, d, s)])
            vb, vm = bb.var(axis=0, ddof=1), bm.var(axis=0, ddof=1)
            if (vb == 0).mean() > 0.1:
                dropped.append((d, s))
                print("layer (d, s) = (%d, %d): %d of %d blocks without variance on the bidirectional side, not compared" % (d, s, (vb == 0).sum(), vb.size))
                continue
            keep = (vb > 0) | (vm > 0)
            z = np.abs(bm.mean(axis=0) - bb.mean(axis=0))[keep] / np.sqrt((vb[keep] + vm[keep]) / K)
            tb, tm = bb.mean(axis=(1, 2)), bm.mean(axis=(1, 2))
            zm = abs(tm.mean() - tb.mean()) / np.sqrt((tb.var(ddof=1) + tm.var(ddof=1)) / K)
            print("layer (d, s) = (%d, %d) %s: %d of %d blocks left out, max z %.2f, layer means mmlt %.6g / bdpt %.6g, z %.2f"
                  % (d, s, "weighted" if weighted else "unweighted", (~keep).sum(), keep.size, z.max(), tm.mean(), tb.mean(), zm))
            worst.append(((d, s), (~keep).mean(), z.max(), zm))
    assert len(worst) >= 9, dropped
    for k, out, z, zm in worst:
        assert out <= 0.1, (k, out)
        assert z < 6, (k, z)
        assert zm < 3, (k, zm)


# ---------------------------------------------------------------- 7. the context is left as it was
@pytest.mark.parametrize("fix_emitter_path", [0, 1])
def test_renders_between_two_runs_change_nothing(pkg, native_lib, fix_emitter_path):
    """seed, run, render_mmlt, render_mmlt_layers, run against seed, run, run with 1 024 chains of algo=drmlt on cornell_c2(16): the
    chain states bit for bit (u, luminance, positions), the counters equal, the films within rel 1e-5 (fp32 atomics in another order).
    Measured on the MI355X: films differ by at most 5.1e-07 (fix_emitter_path 0) and 3.5e-07 (1) relative."""
    sd = pkg.scenes.cornell_c2(16)
    out = []
    for render in (True, False):
        with pkg.Context(_cfg(pkg, algo=pkg.abi.ALGO_DRMLT, fix_emitter_path=fix_emitter_path, work_units=1024), sd) as ctx:
            b = ctx.seed(0xABCD)
            ctx.run(1024 * 32)
            if render:
                img = ctx.render_mmlt(16, seed=3)
                layers = ctx.render_mmlt_layers(16, seed=3)
                assert lum(img.astype(np.float64)).mean() == pytest.approx(b, rel=0.2)
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
    print("films: largest relative difference %.3g" % (np.abs(fa - fb)[fb > 0] / fb[fb > 0]).max())
    np.testing.assert_allclose(fa, fb, rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 8. the seeds follow b_d
def test_the_chain_seeds_follow_the_depth_shares_of_the_layers(pkg, native_lib):
    """cornell_c2(16), maxDepth 4: after ctx.seed with 16 384 chains the share of seed_indices() % maxDepth == d - 1 against the
    share of b_d, the mean luminance of the depth-d layers at 256 spp, mean of K = 8 seeds: within 5 binomial standard deviations
    (16 384 draws) plus 5 standard errors of the reference share (from the K seeds). The seeds are drawn from a pool of 2^20
    bootstrap samples, so that the pool's own error (about 2e-3 of a share) stays below the binomial one that the bound allows for.
    Measured on the MI355X: shares of the seeds 0.60364 / 0.27020 / 0.12616 at d = 2 / 3 / 4 (none at d = 1) against b_d's 0.60177 /
    0.27002 / 0.12822 (standard errors 0.00098 / 0.00074 / 0.00041): differences 0.00187 / 0.00019 / 0.00206 under bounds of 0.02401 /
    0.02103 / 0.01511."""
    abi = pkg.abi
    K, D, chains = 8, lr.MAX_DEPTH, 16384
    with pkg.Context(_cfg(pkg, work_units=chains, luminance_samples=1 << 20), pkg.scenes.cornell_c2(16)) as ctx:
        stacks = np.array([ctx.render_mmlt_layers(256, seed=300 + k) for k in range(K)], dtype=np.float64)
        ctx.seed(0x5EED)
        depth = ctx.seed_indices() % D
    assert depth.size == chains
    bd = np.array([[lum(st[abi.bdpt_layer_index(d, 0):abi.bdpt_layer_index(d, d + 1) + 1]).sum() for d in range(1, D + 1)] for st in stacks])
    shares = bd / bd.sum(axis=1, keepdims=True)
    p, se = shares.mean(axis=0), shares.std(axis=0, ddof=1) / np.sqrt(K)
    got = np.bincount(depth, minlength=D) / chains
    for d in range(D):
        bound = 5 * np.sqrt(p[d] * (1 - p[d]) / chains) + 5 * se[d]
        print("depth %d: share of the seeds %.5f, of b_d %.5f +- %.5f, difference %.5f of a bound of %.5f" % (d + 1, got[d], p[d], se[d], abs(got[d] - p[d]), bound))
    for d in range(D):
        assert abs(got[d] - p[d]) <= 5 * np.sqrt(p[d] * (1 - p[d]) / chains) + 5 * se[d], d + 1
    assert got[0] == 0 and p[0] == 0


# ---------------------------------------------------------------- 9. a traversed scene
@pytest.mark.parametrize("no_light_image", [0, 1], ids=["lightimage", "nolightimage"])
def test_the_weighted_layers_sum_to_the_image_on_a_traversed_scene(pkg, native_lib, monkeypatch, no_light_image):
    """glass_sphere(16) as a BVH (DRMLT_BVH_THRESHOLD=0: eval_mmlt traverses, the stacks' overflow area is sized by the grid):
    _layers_are_the_image's identity and bound. Measured on the MI355X: 0.078 of the bound with the light image, 0.077 without."""
    monkeypatch.setenv("DRMLT_BVH_THRESHOLD", "0")
    with pkg.Context(_cfg(pkg, no_light_image=no_light_image), pkg.scenes.glass_sphere(16)) as ctx:
        _layers_are_the_image(pkg, ctx, "glass_sphere(16) as a BVH, no_light_image %d" % no_light_image)
