"""drmlt_render_bdpt on the device (k_render_bdpt): independent samples of sampleSplats(EBidirectional) into a film. What it refuses,
that the film holds exactly the bootstrap's samples, a closed form per pixel, the device's path tracer and the fp64 oracle's lists by
blocks, the direct-light split, the chain loops against it as their reference, and that it leaves a context as it found it.

technique=path adds no emitted light on camera rays (path.cpp:115,162-165) and drops an emitter reached over delta vertices alone;
the bidirectional integrand has both (s = 0, t = 2 and the specular chains). Wherever render_pt is the other side, the pixels that
show an emitter (and, on the caustic scene, the glass sphere) are left out of the block means on BOTH sides, as
test_direct_image_matches_the_oracles_depth_two_path_tracer leaves the sphere out: under the box filter a sample reaches only
the pixel that contains it, so the remaining pixels are compared in full."""
import numpy as np
import pytest

import direct_scenes as ds
import render_bdpt_scenes as rs
import test_gpu_direct as gd

pytestmark = pytest.mark.gpu
lum = rs.lum
DEPTHS = dict(max_depth=6, rr_depth=4, direct_samples=-1)


def _cfg(pkg, **kw):
    base = dict(technique="bdpt", type="orbital", work_units=16384, luminance_samples=20000, **DEPTHS)
    base.update(kw)
    return pkg.abi.make_config(**base)


def _path_cfg(pkg, **kw):
    base = dict(technique="path", type="orbital", work_units=64, luminance_samples=1000, **DEPTHS)
    base.update(kw)
    return pkg.abi.make_config(**base)


# ---------------------------------------------------------------- 1. refusals
def test_refusals_say_what_is_wrong(pkg, native_lib):
    E = pkg.abi.E_INVALID
    sd = pkg.scenes.cornell_c2(16)
    for kw in (dict(technique="path", work_units=64), dict(technique="mmlt", work_units=64)):
        with pkg.Context(_cfg(pkg, **kw), sd) as ctx:
            with pytest.raises(pkg.binding.DrmltError, match="technique=bdpt") as e:
                ctx.render_bdpt(4)
            assert e.value.code == E
    with pkg.Context(_cfg(pkg, work_units=64), sd) as ctx:
        with pytest.raises(pkg.binding.DrmltError) as e:
            ctx.render_bdpt(0)
        assert e.value.code == E
        assert ctx.render_bdpt(1).shape == (16, 16, 3)
    # 64 spp on 8192 x 8192 pixels are exactly 2^32 samples: one more than a 32-bit address reaches
    with pkg.Context(_cfg(pkg, work_units=64), rs.two_rectangles(pkg, 8192)) as ctx:
        with pytest.raises(pkg.binding.DrmltError, match="different seeds") as e:
            ctx.render_bdpt(64)
        assert e.value.code == E and "32 bits" in str(e.value)


# ---------------------------------------------------------------- 2. the film holds the bootstrap's samples
@pytest.mark.parametrize("light_image", [1, 0], ids=["lightimage", "nolightimage"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
def test_the_film_holds_the_bootstraps_samples(pkg, native_lib, direct, light_image):
    """Under the box filter the image's mean luminance is the mean list luminance of bootstrap samples 0 .. spp * W * H - 1 of stream
    0: 1e-4 relative, test_config5_caustic_acceptance_map's bound for film sums under the discretised box filter (fp32 rounding of
    a few hundred adds per pixel is below it). Sums in fp64 on the host.
    Measured on the MI355X: off by 3.5e-05 (light image) and 4.0e-05 (none) relative; the same seed again within 1.1e-06."""
    sd = pkg.scenes.cornell_c2(16)
    spp, n = 64, 64 * 256
    with pkg.Context(_cfg(pkg, no_direct_sampling=1 - direct, no_light_image=1 - light_image), sd) as ctx:
        img = ctx.render_bdpt(spp, seed=11).astype(np.float64)
        again = ctx.render_bdpt(spp, seed=11).astype(np.float64)
        other = ctx.render_bdpt(spp, seed=12).astype(np.float64)
        boot = ctx.bootstrap_luminances(11, 0, n).astype(np.float64)
        boot_other = ctx.bootstrap_luminances(12, 0, n).astype(np.float64)
    rel = abs(lum(img).mean() / boot.mean() - 1)
    print("cornell_c2(16) direct %d light image %d: image mean %.8g, bootstrap mean %.8g, off by %.3g relative; same seed max rel diff %.3g"
          % (direct, light_image, lum(img).mean(), boot.mean(), rel, (np.abs(img - again) / np.maximum(img, 1e-30)).max()))
    assert np.isfinite(boot).all() and boot.mean() > 0
    assert rel < 1e-4, rel
    assert abs(lum(other).mean() / boot_other.mean() - 1) < 1e-4
    assert not np.array_equal(img, other) and abs(lum(other).mean() - lum(img).mean()) > 0
    np.testing.assert_allclose(again, img, rtol=1e-5, atol=0)   # the same samples: only the order of the fp32 atomics differs


def test_the_film_holds_the_bootstraps_samples_on_a_traversed_scene(pkg, native_lib):
    """The same identity where eval_bdpt traverses a BVH (the 2000-triangle soup, test_gpu_direct's FEAT-15 scene): the
    traversal stacks and their overflow area are the bootstrap's, sized by the grid. Measured on the MI355X: off by 2.2e-05."""
    sd = pkg.scenes.triangle_soup(2000, res=16)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        img = ctx.render_bdpt(64, seed=11).astype(np.float64)
        boot = ctx.bootstrap_luminances(11, 0, 64 * 256).astype(np.float64)
    rel = abs(lum(img).mean() / boot.mean() - 1)
    print("soup(2000, 16): image mean %.8g, bootstrap mean %.8g, off by %.3g relative" % (lum(img).mean(), boot.mean(), rel))
    assert np.isfinite(boot).all() and boot.mean() > 0
    assert rel < 1e-4, rel


# ---------------------------------------------------------------- 3. closed form, per pixel
@pytest.mark.parametrize("light_image", [1, 0], ids=["lightimage", "nolightimage"])
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
def test_lamp_lit_plane_matches_the_closed_form(pkg, native_lib, direct, light_image):
    """A view-filling diffuse plane under a triangle light of edge 1e-5 outside the view, maxDepth 2: per pixel E = rho / pi * L * A *
    cos theta_l * cos theta / d^2 over the pixel (16 x 16 sub-pixel grid). The MIS weights of the strategies that reach a path sum
    to one, so the expectation does not depend on which of them run. K = 16 seeds at 256 spp: every pixel within 6 of its measured
    standard error, the image mean within 1e-3 -- test_direct_pass_of_the_smooth_emitter_matches_the_closed_form's protocol and bounds.
    Without the light image no list carries a light-image splat (at maxDepth 2 the only t = 1 strategy is s = 2, t = 1, which the
    flag removes): the film's light-image share is exactly 0, and it is not with the flag clear. (That the light is out of view and
    every pixel's expectation positive: tests/test_render_bdpt.py, on the CPU.)
    Measured on the MI355X: max z 4.94, mean off by 5.9e-04 with the light image (its share of f: 0.098); 4.86, 7.2e-04 without. With
    a light this small direct sampling moves no figure in the third digit: the s = 1 vertex is the same point either way. The film of
    seed 100 against its own lists' luminance (bootstrap_luminances): off by 1.4e-05 / 1.6e-05 relative."""
    K, spp = 16, 256
    sd = rs.lamp_plane(pkg)
    cfg = _cfg(pkg, max_depth=2, no_direct_sampling=1 - direct, no_light_image=1 - light_image)
    with pkg.Context(cfg, sd) as ctx:
        imgs = np.array([ctx.render_bdpt(spp, seed=100 + k) for k in range(K)], dtype=np.float64)
        boot = ctx.bootstrap_luminances(100, 0, spp * 32 * 32).astype(np.float64)
        us, ue, ud = rs.list_points(cfg, 4096, 5)
        rows = ctx.eval_lists_bdpt(us, ue, ud)
    want = rs.lamp_plane_closed_form(pkg)
    mean, se = imgs.mean(axis=0), imgs.std(axis=0, ddof=1) / np.sqrt(K)
    z = np.abs(mean - want) / se
    rel = abs(mean.mean() - want.mean()) / want.mean()
    more = rows[:, 10:].reshape(len(rows), -1, 5)[:, :, 2:]
    share = float(lum(more).sum() / rows[:, 0].sum())
    print("lamp plane direct %d light image %d: max z %.2f, image mean off by %.3g relative, median rel se %.3g, light-image share of f %.3g"
          % (direct, light_image, z.max(), rel, np.median(se / want), share))
    assert np.all(se > 0) and z.max() < 6, z.max()
    assert rel < 1e-3, rel
    # the film of seed 100 holds the luminance of that seed's lists and nothing besides (test 2's identity and bound): with lists that
    # carry no light-image splat, what k_render_bdpt put into the film is the main splats alone
    film_rel = abs(lum(imgs[0]).mean() / boot.mean() - 1)
    print("    film of seed 100 against its lists' luminance: off by %.3g relative" % film_rel)
    assert film_rel < 1e-4, film_rel
    if light_image:
        assert share > 0 and (rows[:, 7] > 0).any()
    else:
        assert share == 0 and not rows[:, 7].any() and not more.any()


# ---------------------------------------------------------------- 4. against the device's path tracer, by blocks
_EMIT, _PT = {}, {}
# door_c3 is lit through a gap: K = 16 images of render_pt(1024) leave a block at a relative standard error of 0.037 (render_bdpt(512):
# 0.011), measured, which misses _hold_blocks' own precision bound of 0.02 whatever the bidirectional side does. There a path-traced
# image is the mean of 16 renders of 1024 spp (0.0365 / 4) and the bidirectional side renders 2048 spp; the bounds are unchanged.
PT_RENDERS = {"door_c3": 16}
BDPT_SPP = {"door_c3": 2048}


def _emitter_pixels(pkg, name):
    """(SCENES[name](32), binding.visible_emitter_mask of it): computed once a session."""
    if name not in _EMIT:
        sd = pkg.scenes.SCENES[name](32)
        mask = pkg.binding.visible_emitter_mask(sd)
        mask.setflags(write=False)
        _EMIT[name] = (sd, mask)
    return _EMIT[name]


def _left_out(pkg, name):
    """(SCENES[name](32), the pixels left out of a comparison with render_pt): the emitters' and, on caustic_c5, the glass sphere's."""
    sd, mask = _emitter_pixels(pkg, name)
    return sd, (mask | ds.sphere_mask(pkg, sd, (0.0, -0.55, 0.1), 0.3) if name == "caustic_c5" else mask)


def _pt_blocks(pkg, name, K=16):
    """K block images of render_pt(1024) on SCENES[name](32) (door_c3: each the mean of 16 such renders) without the pixels left out:
    computed once a session."""
    if name not in _PT:
        sd, mask = _left_out(pkg, name)
        r = PT_RENDERS.get(name, 1)
        with pkg.Context(_path_cfg(pkg), sd) as ctx:
            b = np.array([gd._blocks(np.mean([ctx.render_pt(1024, seed=300 + k * r + i) for i in range(r)], axis=0, dtype=np.float64), mask)
                          for k in range(K)])
        b.setflags(write=False)
        _PT[name] = b
    return _PT[name]


@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
@pytest.mark.parametrize("name", ["cornell_c2", "door_c3", "mirror_room"])
def test_image_matches_the_devices_path_tracer(pkg, native_lib, name, direct):
    """K = 16 images of render_bdpt(512) against K = 16 of render_pt(1024) at the same depths (door_c3: more samples on both sides,
    see PT_RENDERS), test_gpu_direct's _blocks / _hold_blocks with their own bounds (max z < 6, max rel se < 0.02 on the lit blocks).
    Measured on the MI355X (max z, max rel se; direct sampling on / off): cornell_c2 2.11, 0.0031 / 2.10, 0.0032;
    mirror_room 1.99, 0.0061 / 1.94, 0.0061; door_c3 1.66, 0.0107 / 1.81, 0.0105 (at the issue's 512 against 1024 spp: 2.30, 0.0372 /
    2.33, 0.0372 -- the path tracer's noise)."""
    (sd, mask), bp = _left_out(pkg, name), _pt_blocks(pkg, name)
    assert mask.mean() < 0.1                                             # (cornell_c2: the ceiling light's sliver; the others: none)
    spp = BDPT_SPP.get(name, 512)
    with pkg.Context(_cfg(pkg, no_direct_sampling=1 - direct), sd) as ctx:
        bg = np.array([gd._blocks(ctx.render_bdpt(spp, seed=100 + k), mask) for k in range(16)])
    gd._hold_blocks("render_bdpt(%d) %s direct %d vs render_pt (%d emitter pixels left out)" % (spp, name, direct, mask.sum()), bg, bp)


# ---------------------------------------------------------------- 5. against an independent implementation
@pytest.mark.parametrize("direct", [1, 0], ids=["direct", "nodirect"])
@pytest.mark.parametrize("name", ["glass_sphere", "caustic_c5"])
def test_image_matches_the_oracles_lists(pkg, ob, native_lib, name, direct):
    """The fp64 oracle's bdpt_eval on n = 16 384 uniform points of its own, its lists splatted in numpy with weight W * H / n (box
    filter: a splat lands in the pixel that contains it), against K = 16 seeds of render_bdpt(64): every 4 x 4 block within 6
    combined standard errors (oracle: from the per-sample contributions; device: from the K images), the image means within 3.
    A block whose oracle-side variance is 0 is left out; at most 10 % may be (on the CPU, with the oracle alone: none is, in
    either scene, with or without direct sampling, at this n: tests/test_render_bdpt.py).
    Measured on the MI355X (max block z, image-mean z; direct sampling on / off): glass_sphere 2.58, 0.32 / 2.55, 0.36;
    caustic_c5 2.38, 0.01 / 1.16, 0.10."""
    n, K = 16384, 16
    sd = pkg.scenes.SCENES[name](16)
    cfg = _cfg(pkg, no_direct_sampling=1 - direct)
    orc = ob.Oracle(pkg.abi, cfg, sd, 64)
    us, ue, ud = rs.list_points(cfg, n, 21)
    rows = orc.bdpt_eval(us, ue, ud) if ud is not None else orc.bdpt_eval(us, ue)
    orc.close()
    c = rs.block_contributions(rows, 16)
    mo, vo = c.mean(axis=0), c.var(axis=0, ddof=1)
    with pkg.Context(cfg, sd) as ctx:
        bg = np.array([rs.blocks_of(ctx.render_bdpt(64, seed=500 + k)) for k in range(K)])
    mg, vg = bg.mean(axis=0), bg.var(axis=0, ddof=1)
    keep = vo > 0
    z = np.abs(mg - mo)[keep] / np.sqrt(vo[keep] / n + vg[keep] / K)
    to, tg = c.mean(axis=(1, 2)), bg.mean(axis=(1, 2))
    zm = abs(tg.mean() - to.mean()) / np.sqrt(to.var(ddof=1) / n + tg.var(ddof=1) / K)
    print("render_bdpt %s direct %d vs oracle lists: %d of %d blocks left out, max z %.2f, image means %.6g / %.6g, z %.2f"
          % (name, direct, (~keep).sum(), keep.size, z.max(), tg.mean(), to.mean(), zm))
    assert (~keep).mean() <= 0.1
    assert z.max() < 6, z
    assert zm < 3, zm


# ---------------------------------------------------------------- 6. direct light excluded
def test_render_bdpt_plus_render_direct_is_the_full_image(pkg, native_lib):
    """direct_samples = 16: the chains, and this render with them, exclude depth <= 2; render_direct carries it. Their sum against
    render_bdpt of a context whose lists carry everything, K = 16 each, _hold_blocks' bounds.
    Measured on the MI355X: max z 2.18, max rel se 0.0076; the indirect share of the image mean is 0.203."""
    sd = pkg.scenes.cornell_c2(32)
    K = 16
    with pkg.Context(_cfg(pkg, direct_samples=16), sd) as ctx:
        split = np.array([gd._blocks(ctx.render_bdpt(512, seed=100 + k).astype(np.float64) + ctx.render_direct(16, seed=700 + k)) for k in range(K)])
        indirect = lum(ctx.render_bdpt(64, seed=9)).mean()
    with pkg.Context(_cfg(pkg), sd) as ctx:
        full = np.array([gd._blocks(ctx.render_bdpt(512, seed=300 + k)) for k in range(K)])
    print("indirect share of the image mean: %.3f" % (indirect / full.mean()))
    assert 0.05 < indirect / full.mean() < 0.95                           # the split does split
    gd._hold_blocks("render_bdpt + render_direct vs render_bdpt", split, full)


# ---------------------------------------------------------------- 7. the chains against their own reference
def _blk(a, keep):
    """8 x 8 block means over the pixels of `keep` ((32, 32) of 0 / 1; all ones: a.reshape(8, 4, 8, 4, 3).mean((1, 3)))."""
    s = (a * keep[..., None]).reshape(8, 4, 8, 4, 3).sum((1, 3))
    return s / np.maximum(keep.reshape(8, 4, 8, 4).sum((1, 3)), 1)[..., None]


@pytest.fixture(scope="module")
def caustic_reference(pkg, native_lib):
    """caustic_c5(32): K = 8 images of render_bdpt(2048), unchanged by the tests that share them."""
    sd = pkg.scenes.caustic_c5(32)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        imgs = np.array([ctx.render_bdpt(2048, seed=900 + k) for k in range(8)], dtype=np.float64)
    imgs.setflags(write=False)
    return sd, imgs


CHAIN_RENDERS = {
    "drmlt-bdpt": dict(technique="bdpt"),
    "pssmlt-bdpt": dict(technique="bdpt", algo=1),
    "drmlt-mmlt": dict(technique="mmlt", fix_emitter_path=1, luminance_samples=1000),
}


@pytest.mark.parametrize("which", list(CHAIN_RENDERS))
def test_chain_renders_match_render_bdpt(pkg, native_lib, caustic_reference, which):
    """technique=bdpt under algo=drmlt and algo=pssmlt, and technique=mmlt with fixEmitterPath, at 2048 mutations per pixel with
    16 384 chains, against the mean of K = 8 render_bdpt(2048) images: b within 3 % of the reference's mean luminance, mean absolute
    error of the 4 x 4 block means below 4 % of the reference mean -- the bounds of test_mmlt_image_matches_path_tracing. The
    reference's own block error, half the difference of its two halves of four images, is printed beside them: a miss with that
    above a quarter of the bound would mean a noisy reference, to be met with more reference samples.
    technique=mmlt drops the emitters the camera sees (pathsampler.cpp:84-320, DESIGN.md section 5: "a BDPT image is not its
    expectation" -- here b 0.465 against 0.869, measured), so for it the pixels that show an emitter are left out on both sides:
    under the box filter that light lies in those pixels alone. Its b is then held through the developed image, whose mean
    luminance is b by construction: the mean over the remaining pixels against the reference's.
    Measured on the MI355X (mean luminance off by, block error; the reference's own block error): drmlt-bdpt 0.0028, 0.0061; 0.0010.
    pssmlt-bdpt 0.0028, 0.0057; 0.0010. drmlt-mmlt (993 pixels) 0.0023, 0.0232; 0.0019."""
    sd, imgs = caustic_reference
    ref = imgs.mean(axis=0)
    keep = np.ones((32, 32))
    if CHAIN_RENDERS[which]["technique"] == "mmlt":
        keep = (~_emitter_pixels(pkg, "caustic_c5")[1]).astype(np.float64)
        assert keep.mean() > 0.9
    spp = 2048
    with pkg.Context(_cfg(pkg, sample_count=spp, **CHAIN_RENDERS[which]), sd) as ctx:
        b = ctx.seed(0x5EED)
        ctx.run(32 * 32 * spp)
        img = ctx.develop().astype(np.float64)
    assert lum(img).mean() == pytest.approx(b, rel=1e-3)                  # develop's normalisation: what ties b to the pixels below
    kept = lambda a: (lum(a) * keep).sum() / keep.sum()
    ref_mean = (ref * keep[..., None]).sum() / (3 * keep.sum())
    own = 0.5 * np.abs(_blk(imgs[:4].mean(axis=0), keep) - _blk(imgs[4:].mean(axis=0), keep)).mean() / ref_mean
    err = np.abs(_blk(img, keep) - _blk(ref, keep)).mean() / ref_mean
    print("caustic_c5 %s: b %.6g, mean luminance over the %d pixels compared %.6g, the reference's %.6g (off by %.4f), block error %.4f; "
          "the reference's own block error %.4f" % (which, b, keep.sum(), kept(img), kept(ref), abs(kept(img) / kept(ref) - 1), err, own))
    assert own < 0.01                                                     # a quarter of the bound
    assert kept(img) == pytest.approx(kept(ref), rel=0.03)
    if keep.all():
        assert b == pytest.approx(lum(ref).mean(), rel=0.03)
    assert err < 0.04, err


# ---------------------------------------------------------------- 8. the context is left as it was
@pytest.mark.parametrize("algo", [0, 1], ids=["drmlt", "pssmlt"])
def test_a_render_between_two_runs_changes_nothing(pkg, native_lib, algo):
    """seed, run, render_bdpt, run against seed, run, run: the chain states bit for bit (u, luminance, positions), the counters
    equal, the films within test_single_device_node_is_the_plain_context's tolerance (atomics in another order). The render's
    scratch -- the workspace columns and list slot 1 -- is what every mutation writes before it reads."""
    sd = pkg.scenes.cornell_c2(16)
    out = []
    for render in (True, False):
        with pkg.Context(_cfg(pkg, algo=algo, work_units=1024), sd) as ctx:
            b = ctx.seed(0xABCD)
            ctx.run(1024 * 32)
            if render:
                img = ctx.render_bdpt(16, seed=3)
                assert lum(img).mean() == pytest.approx(b, rel=0.2)
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


# ---------------------------------------------------------------- 9. variance on the caustic
def test_caustic_variance_against_the_path_tracer(pkg, native_lib):
    """caustic_c5(32), K = 16 images of render_bdpt(256) and of render_pt(256): the means agree by blocks (_hold_blocks' bounds; the
    pixels that show an emitter or the glass sphere left out, see the module's head). Recorded, not asserted: the ratio of the
    summed per-pixel variances, path tracer over bdpt, inside and outside the floor region under the sphere (the floor within 0.5
    of the sphere's foot).
    Measured on the MI355X: 103 inside (28 pixels), 6.84 outside (905 pixels); the means: max z 2.41, max rel se 0.0161."""
    K = 16
    sd, mask = _left_out(pkg, "caustic_c5")
    with pkg.Context(_path_cfg(pkg), sd) as ctx:
        pt3 = np.array([ctx.render_pt(256, seed=300 + k) for k in range(K)], dtype=np.float64)
    pt = lum(pt3)
    with pkg.Context(_cfg(pkg), sd) as ctx:
        bd3 = np.array([ctx.render_bdpt(256, seed=100 + k) for k in range(K)], dtype=np.float64)
    bd = lum(bd3)
    inside = rs.floor_disc_mask(sd, (0.0, 0.1), 0.5) & ~mask
    outside = ~inside & ~mask
    vp, vb = pt.var(axis=0, ddof=1), bd.var(axis=0, ddof=1)
    print("caustic_c5 at 256 spp, summed per-pixel variance, render_pt / render_bdpt: %.3g inside the floor region under the sphere (%d pixels), "
          "%.3g outside (%d pixels)" % (vp[inside].sum() / vb[inside].sum(), inside.sum(), vp[outside].sum() / vb[outside].sum(), outside.sum()))
    assert inside.sum() >= 16
    gd._hold_blocks("render_bdpt vs render_pt on caustic_c5", np.array([gd._blocks(i, mask) for i in bd3]), np.array([gd._blocks(i, mask) for i in pt3]))
