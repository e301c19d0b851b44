"""The fp64 oracle's point lights (src/emitters/point.cpp) and constant environment (src/emitters/constant.cpp), technique=path,
on the CPU: closed forms of a sky-lit and a point-lit plane, the sky's pick probability in both MIS weights, a point light as
the limit of a vanishing sphere light and the sky as a closed box of area lights (oracle against oracle), and the refusals of
the bidirectional techniques. These hold before the oracle judges the device (test_gpu_emitter_parity.py)."""
import numpy as np
import pytest

import emitter_scenes as es


def _oracle(pkg, ob, sd, **kw):
    base = dict(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64)
    base.update(kw)
    return ob.Oracle(pkg.abi, pkg.abi.make_config(**base), sd, precision=64)


def test_sky_lit_plane_matches_the_closed_form(pkg, ob):
    """Light sample and BSDF sample both have the density cos / pi, so each gets MIS weight 1/2: f = rho * L on the square.
    Camera rays that miss give exactly 0 (directTracing = false), and with directSamples >= 0 the sky is not seen at all."""
    sd = es.sky_plane(pkg)
    u = np.random.default_rng(11).random((32768, 32), dtype=np.float32)
    for depth in (2, 5):
        orc = _oracle(pkg, ob, sd, max_depth=depth)
        g = orc.eval_paths(u)
        orc.close()
        _, _, inside, outside = es.plane_coords(g)
        want = es.RHO * es.SKY
        rel = np.abs(g["rgb"][inside] - want) / want
        assert rel.max() < 1e-6, rel.max()
        assert np.all(g["rgb"][outside] == 0) and np.all(g["luminance"][outside] == 0)
        # the vertex draws its light sample (2), its BSDF sample (2), and the path ends at the escape: no roulette draw
        assert np.all(g["n_dims"][inside] == 6) and np.all(g["n_rays"][inside] == 3)
    orc = _oracle(pkg, ob, sd, max_depth=5, direct_samples=16)
    g = orc.eval_paths(u)
    orc.close()
    assert np.all(g["rgb"] == 0)


def test_sky_pick_probability_enters_the_mis_weights(pkg, ob):
    """Sky picked with probability p: f = rho L (1 + p) / (1 + p^2) (light sample + BSDF escape); the point light below the square
    picked instead: f = rho L / (1 + p^2) (the escape alone). Their frequencies are p and 1 - p."""
    p = 0.3
    sd = es.sky_plane(pkg, point_below=p)
    orc = _oracle(pkg, ob, sd, max_depth=4)
    u = np.random.default_rng(12).random((65536, 32), dtype=np.float32)
    g = orc.eval_paths(u)
    orc.close()
    _, _, inside, _ = es.plane_coords(g)
    f = g["rgb"][inside]
    v_sky, v_pt = es.RHO * es.SKY * (1 + p) / (1 + p * p), es.RHO * es.SKY / (1 + p * p)
    is_sky = np.all(np.abs(f - v_sky) / v_sky < 1e-6, axis=1)
    is_pt = np.all(np.abs(f - v_pt) / v_pt < 1e-6, axis=1)
    assert np.all(is_sky | is_pt), f[~(is_sky | is_pt)][:4]
    n = inside.sum()
    assert abs(is_sky.sum() - p * n) < 5 * np.sqrt(n * p * (1 - p)), (is_sky.sum(), p * n)
    # the pick is the light sample's first component (u[2]: the vertex's first draw after the film position)
    u2 = u[inside, 2]
    clear = np.abs(u2 - p) > 1e-6
    assert np.array_equal(is_sky[clear], u2[clear] < p)


def test_point_lit_plane_matches_the_closed_form(pkg, ob):
    """f = rho / pi * I * h / (h^2 + r^2)^(3/2) at floor radius r (MIS weight 1: a point light has no BSDF-sampling density);
    camera rays that miss the square give 0."""
    sd = es.point_plane(pkg)
    orc = _oracle(pkg, ob, sd, max_depth=4)
    g = orc.eval_paths(np.random.default_rng(11).random((32768, 32), dtype=np.float32))
    orc.close()
    wx, wy, inside, outside = es.plane_coords(g)
    h = es.H_POINT
    r2 = wx.astype(np.float64) ** 2 + wy.astype(np.float64) ** 2
    want = (es.RHO / np.pi)[None, :] * es.INTENSITY[None, :] * (h / (h * h + r2) ** 1.5)[:, None]
    # the oracle's film position is the fp32 splat's: compare at the precision x / y carry
    rel = np.abs(g["rgb"][inside] - want[inside]) / want[inside]
    assert rel.max() < 1e-5, rel.max()
    assert np.all(g["rgb"][outside] == 0)


@pytest.mark.parametrize("name", ["cornell_point", "door", "soup"])
def test_point_light_is_the_limit_of_a_vanishing_sphere_light(pkg, ob, name):
    """Oracle against oracle: the point light against a black sphere light of radius 1e-5. The bound is the proxy's error
    measured at ten times that radius (q99 6.0e-4 at r = 1e-4, emitter_scenes.limit_pair)."""
    pt_sd, sph_sd = es.limit_pair(pkg, name)
    assert [e.type for e in pt_sd.emitters][-1] == pkg.abi.EMITTER_POINT
    assert [e.sampling_weight for e in pt_sd.emitters] == [e.sampling_weight for e in sph_sd.emitters]
    a, b = _oracle(pkg, ob, pt_sd), _oracle(pkg, ob, sph_sd)
    u = np.random.default_rng(5).random((8192, 64), dtype=np.float32)
    g, o = a.eval_paths(u), b.eval_paths(u)
    a.close(), b.close()
    same = g["n_dims"] == o["n_dims"]
    assert same.mean() >= 0.995, same.mean()
    rel = np.abs(g["luminance"][same] - o["luminance"][same]) / np.maximum(o["luminance"][same], 1e-3)
    assert np.quantile(rel, 0.99) < 6e-4, np.quantile(rel, 0.99)
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert (g["luminance"] > 0).mean() > 0.3


@pytest.mark.parametrize("name", ["cornell_sky", "cornell_sky_quad", "glass_sphere_sky", "rough_sky"])
def test_sky_matches_the_boxed_twin_in_expectation(pkg, ob, name):
    """Oracle against oracle: the sky against six area-light walls of the same radiance. Only the means can agree (the MIS
    weights differ point by point), within 4 standard errors."""
    sd = es.EMITTER_SCENES[name](pkg)
    n = 1 << 16
    a, b = _oracle(pkg, ob, sd), _oracle(pkg, ob, es.boxed(pkg, sd))
    g = a.eval_paths(np.random.default_rng(21).random((n, 64), dtype=np.float32))["luminance"].astype(np.float64)
    o = b.eval_paths(np.random.default_rng(22).random((n, 64), dtype=np.float32))["luminance"].astype(np.float64)
    a.close(), b.close()
    assert np.all(np.isfinite(g)) and g.min() >= 0
    assert (g > 0).mean() > 0.2
    se = np.sqrt(g.var() / n + o.var() / n)
    assert abs(g.mean() - o.mean()) < 4 * se, (g.mean(), o.mean(), se)


def _cosine_warp(sx, sy):
    """warp.cpp:81-102 (concentric disk) lifted to the hemisphere, in float64."""
    r1, r2 = 2 * sx - 1, 2 * sy - 1
    first = r1 * r1 > r2 * r2
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, r1, r2)
        phi = np.where(first, np.pi / 4 * (r2 / r1), np.pi / 2 - (r1 / r2) * np.pi / 4)
    phi = np.where((r1 == 0) & (r2 == 0), 0.0, phi)
    x, y = r * np.cos(phi), r * np.sin(phi)
    return np.stack([x, y, np.sqrt(np.maximum(0.0, 1 - x * x - y * y))], axis=-1)


def test_sky_light_sample_direction_is_read_from_the_pss_point(pkg, ob):
    """A black roof over the sky-lit plane makes each sample's direction visible in f. On the square (normal +z, dpdu along +x)
    both the light sample, in Frame(n) (coordinateSystem: s = +x, t = +y), and the BSDF sample, in the shading frame
    (s = +x, t = +y), map their two components through the cosine warp to (x, y, z) in world space. Each contributes rho L / 2
    when its ray passes the roof and 0 when the roof blocks it: f follows from u[2:4] and u[4:6] alone."""
    sc = pkg.scenes
    sd = es.sky_plane(pkg)
    sd.rectangle(sc.translate(0.2, -0.1, 0.5) @ sc.rotate("x", 180) @ sc.scale(0.3, 0.2, 1.0), sd.diffuse(0.0))
    orc = _oracle(pkg, ob, sd, max_depth=2)
    u = np.random.default_rng(31).random((32768, 32), dtype=np.float32)
    g = orc.eval_paths(u)
    orc.close()
    wx, wy, inside, _ = es.plane_coords(g)
    # camera rays through the roof (its footprint seen from the pinhole at height 3, dilated) are left out
    s_roof = es.H_CAM / (es.H_CAM - 0.5)
    under = (np.abs(wx / s_roof - 0.2) < 0.31) & (np.abs(wy / s_roof + 0.1) < 0.21)
    on = inside & ~under
    uu = u[on].astype(np.float64)
    p = np.stack([wx[on], wy[on]], axis=-1).astype(np.float64)
    k = np.zeros(on.sum())
    sharp = np.ones(on.sum(), bool)
    for a in (2, 4):
        d = _cosine_warp(uu[:, a], uu[:, a + 1])
        q = p + d[:, :2] * (0.5 / d[:, 2:3])             # where the ray crosses the roof's plane
        ex, ey = np.abs(q[:, 0] - 0.2) - 0.3, np.abs(q[:, 1] + 0.1) - 0.2
        k += ~((ex <= 0) & (ey <= 0))
        sharp &= (np.abs(ex) > 1e-3) | (ey > 1e-3)
        sharp &= (np.abs(ey) > 1e-3) | (ex > 1e-3)
    half = es.RHO * es.SKY / 2
    f = g["rgb"][on]
    assert sharp.mean() > 0.99 and np.all(np.isin(k, (0, 1, 2)))
    assert (k[sharp] == 0).any() and (k[sharp] == 1).any()
    assert np.allclose(f[sharp], k[sharp, None] * half[None, :], rtol=1e-6, atol=1e-9), \
        np.flatnonzero(~np.isclose(f[sharp, 0], k[sharp] * half[0]))[:8]


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
@pytest.mark.parametrize("emitter", ["point", "sky"])
def test_oracle_refuses_point_lights_and_the_sky_for_the_bidirectional_techniques(pkg, ob, technique, emitter):
    sd = pkg.scenes.cornell_point(8, quad_light=True) if emitter == "point" else pkg.scenes.cornell_sky(8, quad_light=True)
    cfg = pkg.abi.make_config(type="orbital", technique=technique, max_depth=6, work_units=64)
    with pytest.raises(ob.OracleError) as e:
        ob.Oracle(pkg.abi, cfg, sd, precision=64)
    assert "technique=path only" in str(e.value)
    # the same scene is taken under technique=path
    ob.Oracle(pkg.abi, pkg.abi.make_config(type="orbital", max_depth=6, work_units=64), sd, precision=64).close()


def test_oracle_loads_what_the_device_accepts(pkg, ob):
    """Point positions come from the trailing `points` array; a struct of the layout that ends at `camera` has none."""
    sd = es.mixed(pkg, 8)
    kinds = [e.type for e in sd.emitters]
    assert kinds == [pkg.abi.EMITTER_AREA, pkg.abi.EMITTER_CONSTANT, pkg.abi.EMITTER_POINT, pkg.abi.EMITTER_POINT]
    ob.Oracle(pkg.abi, pkg.abi.make_config(type="orbital", max_depth=6, work_units=64), sd, precision=32).close()
    sd.emitters[2].shape = 5
    with pytest.raises(ob.OracleError) as e:
        ob.Oracle(pkg.abi, pkg.abi.make_config(type="orbital", max_depth=6, work_units=64), sd, precision=64)
    assert "out of range" in str(e.value)
