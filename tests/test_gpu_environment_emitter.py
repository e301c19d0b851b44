"""The constant environment emitter (src/emitters/constant.cpp) on the device, technique=path: f(u) against the closed form of a
sky-lit plane, against the fp64 oracle on a twin whose sky is a closed box of area lights, the same chains across the kernel
generations that carry the branch, the pool kernel with its rows in memory, and unbiased MLT images."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LUMW = np.array([0.212671, 0.715160, 0.072169])


def lum(img):
    return img @ LUMW


def rel_mse(img, ref):
    li, lr = lum(img), lum(ref)
    return float(np.mean((li - lr) ** 2 / (lr ** 2 + 1e-2 * lr.mean() ** 2)))


def _ctx_with_env(pkg, cfg, sd, **env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return pkg.Context(cfg, sd)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- closed form
W, H_CAM, FOV = 48, 3.0, 45.0
RHO, SKY = np.array([0.2, 0.5, 0.8]), np.array([2.0, 3.0, 5.0])


def _sky_plane(pkg, point_below=None):
    """One diffuse square [-1, 1]^2 in z = 0 (normal +z) under the sky, seen by a pinhole straight above. point_below = p: the
    sky takes sampling weight p, and a point light under the square (which can never light it) takes 1 - p."""
    sc = pkg.scenes
    sd = sc.SceneData("sky_plane")
    sd.rectangle(np.eye(4), sd.diffuse(*RHO))
    if point_below is None:
        sd.constant_environment(tuple(SKY))
    else:
        sd.constant_environment(tuple(SKY), sampling_weight=point_below)
        sd.point_light((0.0, 0.0, -0.5), intensity=(50.0, 50.0, 50.0), sampling_weight=1.0 - point_below)
    sd.set_camera(sc.lookat((0, 0, H_CAM), (0, 0, 0), (0, 1, 0)), FOV, W, W)
    return sd


def _inside_outside(g):
    scale = H_CAM * 2.0 * np.tan(np.radians(FOV) / 2) / W
    wx, wy = (g["x"] - W / 2) * scale, (g["y"] - W / 2) * scale
    inside = (np.abs(wx) < 1 - 1e-3) & (np.abs(wy) < 1 - 1e-3)
    outside = (np.abs(wx) > 1 + 1e-3) | (np.abs(wy) > 1 + 1e-3)
    assert inside.sum() > 8192 and outside.sum() > 1000
    return inside, outside


def test_sky_lit_plane_matches_the_closed_form(pkg, native_lib):
    """Light sample and BSDF sample both have the density cos / pi, so each gets MIS weight 1/2: f = rho * L on the square.
    Camera rays that miss give exactly 0 (directTracing = false), and with directSamples >= 0 the sky is not seen at all."""
    sd = _sky_plane(pkg)
    u = np.random.default_rng(11).random((32768, 32), dtype=np.float32)
    for depth in (2, 5):
        ctx = pkg.Context(pkg.abi.make_config(type="orbital", max_depth=depth, direct_samples=-1, work_units=64), sd)
        g = ctx.eval_paths(u)
        inside, outside = _inside_outside(g)
        want = RHO * SKY
        rel = np.abs(g["rgb"][inside] - want) / want
        assert rel.max() < 1e-4, rel.max()
        assert np.all(g["rgb"][outside] == 0) and np.all(g["luminance"][outside] == 0)
        ctx.close()
    ctx = pkg.Context(pkg.abi.make_config(type="orbital", max_depth=5, direct_samples=16, work_units=64), sd)
    g = ctx.eval_paths(u)
    assert np.all(g["rgb"] == 0)
    ctx.close()


def test_sky_pick_probability_enters_the_mis_weights(pkg, native_lib):
    """Sky picked with probability p: f = rho L (1 + p) / (1 + p^2) (light sample + BSDF escape); the point light below the square
    picked instead: f = rho L / (1 + p^2) (the escape alone). Their frequencies are p and 1 - p."""
    p = 0.3
    sd = _sky_plane(pkg, point_below=p)
    ctx = pkg.Context(pkg.abi.make_config(type="orbital", max_depth=4, direct_samples=-1, work_units=64), sd)
    u = np.random.default_rng(12).random((65536, 32), dtype=np.float32)
    g = ctx.eval_paths(u)
    inside, _ = _inside_outside(g)
    f = g["rgb"][inside]
    v_sky, v_pt = RHO * SKY * (1 + p) / (1 + p * p), RHO * SKY / (1 + p * p)
    is_sky = np.all(np.abs(f - v_sky) / v_sky < 1e-4, axis=1)
    is_pt = np.all(np.abs(f - v_pt) / v_pt < 1e-4, axis=1)
    assert np.all(is_sky | is_pt), f[~(is_sky | is_pt)][:4]
    n = inside.sum()
    assert abs(is_sky.sum() - p * n) < 5 * np.sqrt(n * p * (1 - p)), (is_sky.sum(), p * n)
    # the pick is the light sample's first component (u[2]: the vertex's first draw after the film position)
    u2 = u[inside, 2]
    clear = np.abs(u2 - p) > 1e-5
    assert np.array_equal(is_sky[clear], u2[clear] < p)
    ctx.close()


# ---------------------------------------------------------------- against the oracle: the sky as a closed box of area lights
# (an independent check beside test_gpu_emitter_parity.py, where the oracle renders the sky itself: a twin whose sky is six
# area-light walls, compared in expectation)
from emitter_scenes import boxed as _boxed, rough_sky as _rough_sky  # noqa: E402


def _sky_scene(pkg, name):
    sc = pkg.scenes
    if name == "cornell_sky":
        return sc.cornell_sky(32)
    if name == "cornell_sky_quad":
        return sc.cornell_sky(32, quad_light=True, env_weight=0.5)
    if name == "glass_sphere_sky":
        sd = sc.glass_sphere(32)
        sd.constant_environment((0.8, 0.9, 1.0), sampling_weight=2.0)
        return sd
    return _rough_sky(pkg)


@pytest.mark.parametrize("name", ["cornell_sky", "cornell_sky_quad", "glass_sphere_sky", "rough_sky"])
def test_sky_matches_the_oracle_on_the_boxed_twin_in_expectation(pkg, ob, native_lib, name):
    sd = _sky_scene(pkg, name)
    twin = _boxed(pkg, sd)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64)
    n = 1 << 18
    ctx = pkg.Context(cfg, sd)
    g = ctx.eval_paths(np.random.default_rng(21).random((n, 64), dtype=np.float32))["luminance"].astype(np.float64)
    ctx.close()
    orc = ob.Oracle(pkg.abi, cfg, twin, precision=64)
    o = orc.eval_paths(np.random.default_rng(22).random((n, 64), dtype=np.float32))["luminance"].astype(np.float64)
    orc.close()
    assert np.all(np.isfinite(g)) and g.min() >= 0
    assert (g > 0).mean() > 0.2   # the sky lights the scene
    se = np.sqrt(g.var() / n + o.var() / n)
    assert abs(g.mean() - o.mean()) < 4 * se, (g.mean(), o.mean(), se)


def test_sky_render_matches_the_boxed_twin_on_the_device(pkg, native_lib):
    sd = pkg.scenes.cornell_sky(32, quad_light=True)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64)
    a = pkg.Context(cfg, sd)
    img = a.render_pt(16384, seed=3)
    a.close()
    b = pkg.Context(cfg, _boxed(pkg, sd))
    ref = b.render_pt(16384, seed=4)
    b.close()
    la, lb = lum(img).reshape(4, 8, 4, 8).mean(axis=(1, 3)), lum(ref).reshape(4, 8, 4, 8).mean(axis=(1, 3))
    assert lb.min() > 0
    err = np.abs(la - lb) / lb
    assert err.max() < 0.04, err


# ---------------------------------------------------------------- chains
@pytest.mark.parametrize("kw", [dict(type="orbital"), dict(type="green"), dict(type="mira")],
                         ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
def test_sky_lit_chains_are_the_same_across_kernel_generations(pkg, native_lib, kw):
    sd = pkg.scenes.cornell_sky(32, quad_light=True)
    n_chains, n_mut = 1024, 40
    cfg = pkg.abi.make_config(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1, **kw)
    results = []
    for env in (dict(DRMLT_KERNEL=3, DRMLT_MH_BATCH=12), dict(DRMLT_KERNEL=4, DRMLT_MH_BATCH=1), dict(DRMLT_KERNEL=4, DRMLT_MH_BATCH=12)):
        ctx = _ctx_with_env(pkg, cfg, sd, **env)
        ctx.seed(0x77)
        ctx.run(n_chains * n_mut)
        results.append((ctx.chain_state(34), ctx.stats(), ctx.film()))
        ctx.close()
    (c0, u0), s0, f0 = results[0]
    assert s0.mutations == n_chains * n_mut and s0.accepted > 0
    for (c, u), s, f in results[1:]:
        assert np.array_equal(u, u0) and np.array_equal(c["luminance"], c0["luminance"])
        for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
            assert getattr(s, k + "_base") == getattr(s0, k + "_base") and getattr(s, k + "_acc") == getattr(s0, k + "_acc")
        assert s.rays == s0.rays and s.path_evals == s0.path_evals and s.accepted == s0.accepted
        assert lum(f).sum() == pytest.approx(lum(f0).sum(), rel=1e-5)
        assert np.abs(lum(f) - lum(f0)).sum() / lum(f0).sum() < 1e-4


def test_sky_lit_pool_kernel_with_rows_in_memory(pkg, native_lib, capfd):
    """k_mutate_v5 at 163 840 chains: its proposal rows move to device memory (three waves per SIMD)."""
    sd = pkg.scenes.cornell_sky(128)
    n_chains = 163840
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=n_chains,
                              luminance_samples=655360, sample_count=256)
    os.environ["DRMLT_VERBOSE"] = "1"
    try:
        ctx = pkg.Context(cfg, sd)
        b = ctx.seed(0x5EED)
        total = n_chains * 64
        ctx.run(total)
        log = capfd.readouterr().err
    finally:
        del os.environ["DRMLT_VERBOSE"]
    assert re.search(r"k_mutate_v5: \d+ B of LDS per wave; proposal rows in device memory", log), log
    st = ctx.stats()
    M = st.mutations
    assert M == total and st.n_chains == n_chains
    assert st.first_base == M and st.large_base + st.bold_base == M
    assert st.overall_base == M + st.second_base and st.overall_acc == st.first_acc + st.second_acc == st.accepted
    assert st.path_evals == M + st.second_base
    film = ctx.film()
    assert np.all(np.isfinite(film)) and film.min() >= 0
    assert lum(film).sum() == pytest.approx(M * 0.99998 ** 2, rel=2e-3)
    cur, u = ctx.chain_state(34)
    assert np.all((u >= 0) & (u <= 1)) and np.all(cur["luminance"] > 0)
    assert lum(ctx.develop()).mean() == pytest.approx(b, rel=1e-3)
    ctx.close()


@pytest.mark.parametrize("algo", ["drmlt", "pssmlt"])
def test_sky_lit_mlt_image_is_unbiased(pkg, native_lib, algo):
    abi = pkg.abi
    sd = pkg.scenes.cornell_sky(32)
    spp = 2048
    base = dict(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=200000)
    ref = pkg.Context(abi.make_config(work_units=64, **base), sd).render_pt(8192, seed=5)
    extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
    ctx = pkg.Context(abi.make_config(work_units=4096, sample_count=spp, **base, **extra), sd)
    b = ctx.seed(9)
    assert b == pytest.approx(lum(ref).mean(), rel=0.02)
    ctx.run(32 * 32 * spp)
    img = ctx.develop()
    assert lum(img).mean() == pytest.approx(b, rel=1e-3)
    assert rel_mse(img, ref) < 1e-2, rel_mse(img, ref)
    ctx.close()


def test_standalone_host_renders_a_sky_scene_file(pkg, native_lib, tmp_path):
    """The scene file carries the sky in its emitter array (shape = -1): the stand-alone host renders what the binding does."""
    import subprocess
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "drmlt-mitsuba_amd", "host")
    subprocess.check_call(["make", "-C", host], stdout=subprocess.DEVNULL)
    sd = pkg.scenes.cornell_sky(32, quad_light=True)
    scene, out = str(tmp_path / "sky.bin"), str(tmp_path / "o.pfm")
    sd.save(scene)
    args = dict(technique="path", type="orbital", maxDepth=8, directSamples=-1, workUnits=1024, luminanceSamples=20000, sampleCount=64)
    cmd = [os.path.join(host, "drmlt_render"), scene, "-o", out]
    for k, v in args.items():
        cmd += ["-D", "%s=%s" % (k, v)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()
    with open(out, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"32 32\n" and f.readline() == b"-1.0\n"
        img = np.frombuffer(f.read(), dtype="<f4").reshape(32, 32, 3)[::-1]
    ctx = pkg.Context(pkg.abi.make_config(type="orbital", max_depth=8, direct_samples=-1, work_units=1024, luminance_samples=20000,
                                          sample_count=64), sd)
    b = ctx.seed(0x5EED)
    ctx.run(32 * 32 * 64)
    ref = ctx.develop()
    ctx.close()
    assert ("b=%.9g" % b) in p.stdout.decode()
    assert np.allclose(img, ref, rtol=1e-3, atol=1e-5)
