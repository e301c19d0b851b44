"""drmlt_render_pt_layers on the device (k_render_pt_layers): render_pt's samples split by path length and strategy, layer
(d, strategy) holding the light of paths of d edges found by the BSDF-sampled ray (PT_HIT) or by the light sample (PT_DIRECT). What
it refuses; that the weighted layers are render_pt's image and which layers must be empty; closed forms; every depth against the
bidirectional layers and against the fp64 oracle; voided samples; that a context is left as it was."""
import numpy as np
import pytest

import emitter_scenes as es
import render_bdpt_scenes as rs

pytestmark = pytest.mark.gpu
lum = rs.lum
DEPTHS = dict(max_depth=6, rr_depth=4, direct_samples=-1)


def _cfg(pkg, **kw):
    base = dict(technique="path", type="orbital", work_units=64, luminance_samples=20000, **DEPTHS)
    base.update(kw)
    return pkg.abi.make_config(**base)


def _layer(pkg, stack, d, strategy):
    return stack[..., pkg.abi.pt_layer_index(d, strategy), :, :, :]


def _depth(pkg, stack, d):
    return _layer(pkg, stack, d, pkg.abi.PT_HIT) + _layer(pkg, stack, d, pkg.abi.PT_DIRECT)


def _layers_are_the_image(pkg, ctx, tag, spp=64, seed=11):
    """Test 2's identity on `ctx`: the weighted layers, summed over the layer axis in fp64 on the host, against render_pt of the same
    seed, rtol 1e-4 per pixel and channel. Both sides add the same non-negative fp32 terms in different orders (the image sums a
    sample's terms before the filter, the layers put each through it): a pixel that receives n adds is off by at most n * 2^-24
    relative, so 1e-4 allows about 1 600 adds where a pixel here has 64 * 2 * maxDepth at most. Both d = 1 layers are exactly zero.
    Returns (layers, image), fp64."""
    layers = ctx.render_pt_layers(spp, seed=seed).astype(np.float64)
    img = ctx.render_pt(spp, seed=seed).astype(np.float64)
    assert layers.shape == (pkg.abi.pt_layer_count(ctx.cfg.max_depth),) + img.shape
    total = layers.sum(axis=0)
    assert np.isfinite(layers).all() and (layers >= 0).all() and img.mean() > 0
    rel = np.abs(total - img) / np.maximum(img, 1e-300)
    print("%s: sum of the %d weighted layers against render_pt(%d): largest difference %.3g relative (pixels lit: %d of %d)"
          % (tag, len(layers), spp, rel[img > 0].max(), (img > 0).all(axis=2).sum(), img.shape[0] * img.shape[1]))
    assert not total[img == 0].any()
    np.testing.assert_allclose(total, img, rtol=1e-4, atol=0)
    assert not layers[:2].any()
    return layers, img


# ---------------------------------------------------------------- 1. refusals
def test_refusals_say_what_is_wrong(pkg, native_lib):
    E = pkg.abi.E_INVALID
    sd = pkg.scenes.cornell_c2(16)
    out = np.zeros((12, 16, 16, 3), dtype=np.float32)
    for technique in ("bdpt", "mmlt"):
        with pkg.Context(_cfg(pkg, technique=technique), sd) as ctx:
            with pytest.raises(pkg.binding.DrmltError, match="technique=%s" % technique) as e:      # the binding's own refusal
                ctx.render_pt_layers(4)
            assert e.value.code == E
            assert native_lib.drmlt_render_pt_layers(ctx.h, 4, 1, 0, out.ctypes.data) == E          # and the library's
            msg = native_lib.drmlt_last_error(ctx.h).decode()
            assert "technique=path" in msg and "technique=%s" % technique in msg, msg
            assert not out.any()
    with pkg.Context(_cfg(pkg), sd) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="spp is 0") as e:
            ctx.render_pt_layers(0)
        assert e.value.code == E
        for mode in (2, -1):
            with pytest.raises(pkg.binding.DrmltError, match="unknown mode %d" % mode) as e:
                ctx.render_pt_layers(1, weighted=mode)
            assert e.value.code == E
        assert native_lib.drmlt_render_pt_layers(ctx.h, 4, 1, 0, None) == E                          # NULL output
        for weighted in (True, False, pkg.abi.LAYERS_UNWEIGHTED):
            assert ctx.render_pt_layers(1, weighted=weighted).shape == (pkg.abi.pt_layer_count(6), 16, 16, 3) == (12, 16, 16, 3)
    # above bdpt's bound of 24 a sample's terms no longer fit the wave's LDS rows
    with pkg.Context(_cfg(pkg, max_depth=25), sd) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="maxDepth 25") as e:
            ctx.render_pt_layers(1)
        assert e.value.code == E and "24" in str(e.value)
    with pkg.Context(_cfg(pkg, max_depth=24), sd) as ctx:
        assert ctx.render_pt_layers(1).shape == (48, 16, 16, 3)
    # 64 spp on 8192 x 8192 pixels are exactly 2^32 samples: refused before the layered film (9.7 GB here) is asked for
    with pkg.Context(_cfg(pkg), rs.two_rectangles(pkg, 8192)) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="different seeds") as e:
            ctx.render_pt_layers(64)
        assert e.value.code == E and "32 bits" in str(e.value)


# ---------------------------------------------------------------- 2. the layers are the image
def test_the_weighted_layers_sum_to_render_pts_image(pkg, native_lib):
    """cornell_c2(16), maxDepth 6, 64 spp: _layers_are_the_image's identity and bound, both d = 1 layers exactly zero. The same
    seed again agrees within rtol 1e-5 (only the order of the atomics differs), another seed does not. Every depth from 2 on
    carries light by both strategies.
    Measured on the MI355X: largest difference of the sum from the image 4.45e-07 relative (3.55e-07 in another run; 4.36e-07 with
    an fp32 layered film); the same seed again 0 (fp32 layered film: 3.5e-07). Share of the image by depth, hit / direct: d = 2
    0.0002 / 0.5508, d = 3 0.0004 / 0.2438, d = 4 0.0003 / 0.1212, d = 5 0.0001 / 0.0555, d = 6 0.0001 / 0.0276."""
    abi = pkg.abi
    with pkg.Context(_cfg(pkg), pkg.scenes.cornell_c2(16)) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "cornell_c2(16)")
        again = ctx.render_pt_layers(64, seed=11).astype(np.float64)
        other = ctx.render_pt_layers(64, seed=12).astype(np.float64)
    for d in range(2, 7):
        assert _layer(pkg, layers, d, abi.PT_HIT).any() and _layer(pkg, layers, d, abi.PT_DIRECT).any(), d
    print("    the same seed again: largest difference %.3g relative" % (np.abs(again - layers)[layers > 0] / layers[layers > 0]).max())
    np.testing.assert_allclose(again, layers, rtol=1e-5, atol=0)
    assert not np.array_equal(other, layers) and abs(other.sum() - layers.sum()) > 0
    share = layers.sum(axis=(1, 2, 3)) / layers.sum()
    print("    share of the image by (d, hit), (d, direct): " + ", ".join("d=%d %.4f %.4f" % (d, share[2 * d - 2], share[2 * d - 1]) for d in range(1, 7)))


@pytest.mark.parametrize("scene", ["cornell_point", "cornell_sky", "mirror_room", "smooth_room", "triangle_soup"])
def test_the_identity_holds_on_every_kind_of_scene(pkg, native_lib, scene):
    """The same identity with a point light, the constant sky, a smooth conductor, vertex normals and a traversed scene (2000
    triangles, BVH). A point light cannot be hit: every PT_HIT layer of cornell_point is exactly zero.
    Measured on the MI355X (largest difference of the sum from the image, relative): cornell_point 4.08e-07, cornell_sky 6.44e-07,
    mirror_room 4.48e-07, smooth_room 3.81e-07, triangle_soup 4.02e-07."""
    sc = pkg.scenes
    sd = sc.triangle_soup(2000, res=16) if scene == "triangle_soup" else getattr(sc, scene)(16)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "%s(16)" % scene)
    if scene == "cornell_point":
        assert not layers[pkg.abi.PT_HIT::2].any() and layers[pkg.abi.PT_DIRECT::2].any()
    if scene == "cornell_sky":
        assert layers[pkg.abi.PT_HIT::2].any() and layers[pkg.abi.PT_DIRECT::2].any()


def test_separate_direct_light_empties_the_layers_up_to_depth_two(pkg, native_lib):
    """direct_samples = 16: the chains, render_pt and the layers exclude depth <= 2 (render_direct carries it). Every d <= 2 layer
    is exactly zero, the deeper ones are render_pt's image of that context.
    Measured on the MI355X: largest difference 2.78e-07 relative."""
    with pkg.Context(_cfg(pkg, direct_samples=16), pkg.scenes.cornell_c2(16)) as ctx:
        layers, img = _layers_are_the_image(pkg, ctx, "cornell_c2(16) direct_samples 16")
    first = pkg.abi.pt_layer_index(3, 0)
    assert first == 4 and not layers[:first].any() and layers[first:].any()


# ---------------------------------------------------------------- 3. closed forms, deterministic
def _inside_pixels():
    """Pixels of emitter_scenes' 48 x 48 film that lie wholly on the square [-1, 1]^2 (box filter: a sample lands in its own pixel)."""
    scale = es.H_CAM * 2.0 * np.tan(np.radians(es.FOV) / 2) / es.W
    edge = np.maximum(np.abs(np.arange(es.W) - es.W / 2), np.abs(np.arange(es.W) + 1 - es.W / 2)) * scale
    ok = edge < 1 - 1e-3
    return ok[:, None] & ok[None, :]


def test_both_strategies_are_half_the_image_under_the_sky(pkg, native_lib):
    """emitter_scenes.sky_plane, maxDepth 2, 64 spp. The BSDF sample and the sky's light sample have the same density cos / pi, so
    both power-heuristic weights are 1/2 and both estimators have zero variance: on the pixels wholly inside the square, weighted
    (2, hit) and (2, direct) each equal half of render_pt's image of the same seed, and unweighted each equals the whole image,
    rtol 1e-5.
    Measured on the MI355X: all four ratios within 1.17e-06 of 1 (the image's own fp32 atomics; the weights are 1/2 to 1e-7)."""
    abi = pkg.abi
    with pkg.Context(_cfg(pkg, max_depth=2, rr_depth=100), es.sky_plane(pkg)) as ctx:
        img = ctx.render_pt(64, seed=5).astype(np.float64)
        wt = ctx.render_pt_layers(64, seed=5).astype(np.float64)
        un = ctx.render_pt_layers(64, seed=5, weighted=False).astype(np.float64)
    m = _inside_pixels()
    assert wt.shape == un.shape == (4, es.W, es.W, 3) and m.sum() >= 30 * 30 and (img[m] > 0).all()
    assert not wt[:2].any() and not un[:2].any()
    for s in (abi.PT_HIT, abi.PT_DIRECT):
        half, whole = _layer(pkg, wt, 2, s)[m], _layer(pkg, un, 2, s)[m]
        print("sky plane, strategy %d: weighted / (image / 2) - 1 within %.3g, unweighted / image - 1 within %.3g"
              % (s, np.abs(half / (0.5 * img[m]) - 1).max(), np.abs(whole / img[m] - 1).max()))
        np.testing.assert_allclose(half, 0.5 * img[m], rtol=1e-5, atol=0)
        np.testing.assert_allclose(whole, img[m], rtol=1e-5, atol=0)


def test_a_point_lights_sample_is_the_image_in_both_modes(pkg, native_lib):
    """emitter_scenes.point_plane, maxDepth 2: a point light is found by its sample alone, whose weight is 1 by construction, so
    (2, direct) equals the image (rtol 1e-5), weighted and unweighted hold the same bits, and every other layer is zero. The two
    modes are two launches whose atomics arrive in different orders: with an fp32 layered film two launches of even the same mode
    differed in 54 floats at 1 spp and 519 at 4 spp (eight repeats each, none bit-equal), which is why the layered film is fp64 on
    the device and rounded once (kernels_layers_pt.hip). A pixel channel can still differ if its sum lies within some 1e-15 relative
    of an fp32 rounding boundary, about 1e-8 per channel at 4 spp.
    Measured on the MI355X: (2, direct) within 1.72e-07 of the image on 4 572 lit pixel channels; weighted and unweighted bit-equal,
    and so were eight repeats each at 1, 4 and 64 spp."""
    abi = pkg.abi
    with pkg.Context(_cfg(pkg, max_depth=2, rr_depth=100), es.point_plane(pkg)) as ctx:
        img = ctx.render_pt(4, seed=5).astype(np.float64)
        wt = ctx.render_pt_layers(4, seed=5)
        un = ctx.render_pt_layers(4, seed=5, weighted=False)
    direct = _layer(pkg, wt, 2, abi.PT_DIRECT).astype(np.float64)
    lit = img > 0
    print("point plane: (2, direct) / image - 1 within %.3g on %d lit pixel channels; weighted == unweighted: %s"
          % (np.abs(direct[lit] / img[lit] - 1).max(), lit.sum(), np.array_equal(wt, un)))
    assert lit.sum() > 3 * 800
    np.testing.assert_allclose(direct, img, rtol=1e-5, atol=0)
    assert np.array_equal(wt, un)
    for i in range(4):
        if i != abi.pt_layer_index(2, abi.PT_DIRECT):
            assert not wt[i].any() and not un[i].any(), i


# ---------------------------------------------------------------- 4. and 5. depth by depth
K, SPP = 16, 1024
ORACLE_SPP = {2: 512, 3: 1536, 4: 1536}
_DEVICE = {}


def _device_depths(pkg):
    """K seeds of the weighted layers of one maxDepth-4 path context on cornell_c2(16), rr_depth 100, as 4 x 4 block means of
    (d, hit) + (d, direct): {d: (K, 4, 4)}. Computed once, shared by the two comparisons."""
    if not _DEVICE:
        with pkg.Context(_cfg(pkg, max_depth=4, rr_depth=100), pkg.scenes.cornell_c2(16)) as ctx:
            stacks = np.array([ctx.render_pt_layers(SPP, seed=700 + k) for k in range(K)], dtype=np.float64)
        for d in (2, 3, 4):
            _DEVICE[d] = np.array([rs.blocks_of(img) for img in _depth(pkg, stacks, d)])
    return _DEVICE


def _compare(tag, mine, theirs, var_theirs=None):
    """Block means of K images a side: every block within 6 combined standard errors, the mean within 3; the largest relative
    standard error of a block on either side below 5 %."""
    mg, vg = mine.mean(axis=0), mine.var(axis=0, ddof=1) / K
    mo = theirs.mean(axis=0)
    vo = theirs.var(axis=0, ddof=1) / K if var_theirs is None else var_theirs
    z = np.abs(mg - mo) / np.sqrt(vg + vo)
    tg, to = mine.mean(axis=(1, 2)), theirs.mean(axis=(1, 2))
    vto = to.var(ddof=1) / K if var_theirs is None else var_theirs.sum() / var_theirs.size ** 2
    zm = abs(tg.mean() - to.mean()) / np.sqrt(tg.var(ddof=1) / K + vto)
    rse = max((np.sqrt(vg) / mg).max(), (np.sqrt(vo) / mo).max())
    print("%s: max block z %.2f, means %.6g / %.6g, z %.2f, largest relative standard error of a block %.3g" % (tag, z.max(), tg.mean(), to.mean(), zm, rse))
    return z.max(), zm, rse


def test_every_depth_matches_the_bidirectional_layers(pkg, native_lib):
    """cornell_c2(16), maxDepth 4, no importance map, K = 16 seeds of 1 024 spp a side: (d, hit) + (d, direct), weighted, from a
    path context against the sum over s of the weighted render_bdpt_layers (d, s) from a bdpt context, for d = 2, 3, 4, in 4 x 4
    blocks. Two evaluation routines that share no estimator code. Every block within 6 combined standard errors measured over the
    K images, each depth's mean within 3 (test_weighted_layers_match_the_oracle_strategy_by_strategy's bounds); 1 024 spp keep
    the largest relative standard error of a block below 5 %, which is asserted.
    Measured on the MI355X (max block z; z of the means; largest relative standard error of a block): d = 2 1.49, 1.99, 0.92 %;
    d = 3 2.70, 0.49, 0.62 %; d = 4 2.48, 0.66, 0.80 %. Means path / bdpt: 0.047995 / 0.047920, 0.021399 / 0.021387,
    0.010230 / 0.010238."""
    abi = pkg.abi
    mine = _device_depths(pkg)
    cfg = abi.make_config(technique="bdpt", type="orbital", max_depth=4, rr_depth=100, direct_samples=-1, work_units=16384, luminance_samples=20000)
    with pkg.Context(cfg, pkg.scenes.cornell_c2(16)) as ctx:
        stacks = np.array([ctx.render_bdpt_layers(SPP, seed=900 + k) for k in range(K)], dtype=np.float64)
    worst = []
    for d in (2, 3, 4):
        both = stacks[:, abi.bdpt_layer_index(d, 0):abi.bdpt_layer_index(d, d + 1) + 1].sum(axis=1)
        worst.append((d,) + _compare("depth %d, path against bdpt" % d, mine[d], np.array([rs.blocks_of(img) for img in both])))
    for d, z, zm, rse in worst:
        assert rse < 0.05, (d, rse)
        assert z < 6, (d, z)
        assert zm < 3, (d, zm)


def test_every_depth_matches_the_oracle(pkg, ob, native_lib):
    """The same device layers against the fp64 oracle's render_pt at maxDepth 2, 3 and 4 (rr_depth 100: roulette never fires, so
    the depth-d light does not depend on maxDepth), K = 16 images each with independent seeds; depth d is the difference of
    consecutive maxDepths, its variance the sum of the two variances. Blocks and bounds as above. The oracle's spp are chosen on
    the oracle alone: a difference carries the noise of two whole images, and at 512 spp throughout the depth-4 light of the
    darkest block has a relative standard error of 6.2 % (depth 3: 3.1 %, depth 2: 1.2 %), so maxDepth 3 and 4 take 1 536.
    Measured on the MI355X (max block z; z of the means; largest relative standard error of a block): d = 2 1.51, 0.01, 1.2 %;
    d = 3 2.30, 0.30, 3.1 %; d = 4 2.28, 0.30, 3.3 %. Means device / oracle: 0.047995 / 0.047995, 0.021399 / 0.021379,
    0.010230 / 0.010249."""
    abi = pkg.abi
    mine = _device_depths(pkg)
    sd = pkg.scenes.cornell_c2(16)
    imgs = {}
    for md in (2, 3, 4):
        orc = ob.Oracle(abi, _cfg(pkg, max_depth=md, rr_depth=100), sd, precision=64)
        imgs[md] = np.array([rs.blocks_of(orc.render_pt(ORACLE_SPP[md], seed=1000 * md + k, nthreads=16)) for k in range(K)])
        orc.close()
    worst = []
    for d in (2, 3, 4):
        if d == 2:
            theirs, var = imgs[2], imgs[2].var(axis=0, ddof=1) / K
        else:       # the K differences have the right mean; the variance of a difference of independent renders is the sum
            theirs, var = imgs[d] - imgs[d - 1], imgs[d].var(axis=0, ddof=1) / K + imgs[d - 1].var(axis=0, ddof=1) / K
        worst.append((d,) + _compare("depth %d, device against the oracle" % d, mine[d], theirs, var))
    for d, z, zm, rse in worst:
        assert rse < 0.05, (d, rse)
        assert z < 6, (d, z)
        assert zm < 3, (d, zm)


# ---------------------------------------------------------------- 6. voided samples
def _room_with_a_normal_less_triangle(pkg, normals):
    """cornell_c2(16) with a diffuse triangle hung in the middle of the room whose vertex normals are all zero: a path that reaches
    it is voided, whatever light it has gathered before. normals=None: the twin with the face normal."""
    sd = pkg.scenes.cornell_c2(16)
    sd.triangle((-0.7, 0.1, 0.5), (0.7, 0.1, 0.5), (0.0, 0.1, -0.7), sd.diffuse(0.5), normals=normals)
    return sd


def test_a_voided_sample_is_in_no_layer(pkg, native_lib):
    """path_step voids a sample that reaches a vertex normal without direction: Li = 0, whatever was added before. On C2's room with
    such a triangle in it, eval_paths finds the samples in question -- f exactly 0 where the twin scene (the same triangle with its
    face normal, the same points) has light, after at least one surface vertex (three rays or more) -- and the sum of the layers
    still equals render_pt's image at rtol 1e-4: had their earlier terms gone to the layers, the sum would exceed the image.
    Measured on the MI355X: 1 293 of 16 384 points voided after their first vertex; largest difference of the sum 4.57e-07 relative."""
    u = np.random.default_rng(3).random((16384, 32), dtype=np.float32)
    g = {}
    for key, normals in (("void", np.zeros((3, 3))), ("twin", None)):
        with pkg.Context(_cfg(pkg), _room_with_a_normal_less_triangle(pkg, normals)) as ctx:
            g[key] = ctx.eval_paths(u)
            if key == "void":
                layers, img = _layers_are_the_image(pkg, ctx, "room with a normal-less triangle")
    voided_late = (g["void"]["luminance"] == 0) & (g["twin"]["luminance"] > 0) & (g["void"]["n_rays"] >= 3)
    print("    eval_paths: %d of %d points are voided after their first vertex (f = 0, the twin's f > 0)" % (voided_late.sum(), len(u)))
    assert voided_late.sum() >= 100
    assert np.isfinite(g["void"]["rgb"]).all()


# ---------------------------------------------------------------- 7. the context is left as it was
def test_layers_between_two_runs_change_nothing(pkg, native_lib):
    """seed, run, render_pt_layers, run against seed, run, run with 1 024 chains on cornell_c2(16): the chain states bit for bit
    (u, luminance, positions), the counters equal, the films within rtol 2e-4, atol 1e-6 (atomics in another order) --
    test_layers_between_two_runs_change_nothing's bounds for the bidirectional layers. Like render_pt the call renders into a film
    of its own and writes nothing of the context."""
    sd = pkg.scenes.cornell_c2(16)
    out = []
    for render in (True, False):
        with pkg.Context(_cfg(pkg, work_units=1024), sd) as ctx:
            b = ctx.seed(0xABCD)
            ctx.run(1024 * 32)
            if render:
                layers = ctx.render_pt_layers(16, seed=3)
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
