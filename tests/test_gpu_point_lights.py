"""Point emitters (src/emitters/point.cpp) on the device, technique=path: f(u) against the closed form of a point-lit plane,
against the fp64 oracle's limit of a vanishing sphere light, the same chains across the kernel generations that carry the
branch, and an unbiased MLT image."""
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


def test_point_lit_plane_matches_the_closed_form(pkg, native_lib):
    """One diffuse square (rho per channel) under a point light at height h on the camera axis, the camera straight above:
    f = rho / pi * I * h / (h^2 + r^2)^(3/2) at floor radius r; camera rays that miss the square give 0."""
    sc = pkg.scenes
    W = 48
    h_cam, h, fov = 3.0, 0.7, 45.0
    rho, inten = np.array([0.2, 0.5, 0.8]), np.array([2.0, 3.0, 5.0])
    sd = sc.SceneData("point_plane")
    floor = sd.diffuse(*rho)
    sd.rectangle(np.eye(4), floor)                                   # [-1, 1]^2 in z = 0, normal +z
    sd.point_light((0.0, 0.0, h), intensity=tuple(inten))
    sd.set_camera(sc.lookat((0, 0, h_cam), (0, 0, 0), (0, 1, 0)), fov, W, W)
    cfg = pkg.abi.make_config(type="orbital", max_depth=4, direct_samples=-1, work_units=64)
    ctx = pkg.Context(cfg, sd)
    u = np.random.default_rng(11).random((32768, 32), dtype=np.float32)
    g = ctx.eval_paths(u)
    scale = h_cam * 2.0 * np.tan(np.radians(fov) / 2) / W              # floor distance per film pixel
    wx, wy = (g["x"] - W / 2) * scale, (g["y"] - W / 2) * scale
    r2 = wx.astype(np.float64) ** 2 + wy.astype(np.float64) ** 2
    want = (rho / np.pi)[None, :] * inten[None, :] * (h / (h * h + r2) ** 1.5)[:, None]
    inside = (np.abs(wx) < 1 - 1e-3) & (np.abs(wy) < 1 - 1e-3)
    outside = (np.abs(wx) > 1 + 1e-3) | (np.abs(wy) > 1 + 1e-3)
    assert inside.sum() > 8192 and outside.sum() > 1000
    rel = np.abs(g["rgb"][inside] - want[inside]) / want[inside]
    assert rel.max() < 1e-4, rel.max()
    assert np.all(g["rgb"][outside] == 0)


# (an independent check beside test_gpu_emitter_parity.py, where the oracle renders the point light itself)
from emitter_scenes import limit_pair as _limit_pair  # noqa: E402


@pytest.mark.parametrize("name", ["cornell_point", "door", "soup"])
def test_point_light_is_the_limit_of_a_vanishing_sphere_light(pkg, ob, native_lib, name):
    dev_sd, orc_sd = _limit_pair(pkg, name)
    assert [e.type for e in dev_sd.emitters][-1] == pkg.abi.EMITTER_POINT
    assert len(dev_sd.emitters) == len(orc_sd.emitters)
    assert [e.sampling_weight for e in dev_sd.emitters] == [e.sampling_weight for e in orc_sd.emitters]
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64)
    ctx = pkg.Context(cfg, dev_sd)
    orc = ob.Oracle(pkg.abi, cfg, orc_sd, precision=64)
    u = np.random.default_rng(5).random((8192, 64), dtype=np.float32)
    g, o = ctx.eval_paths(u), orc.eval_paths(u)
    same = g["n_dims"] == o["n_dims"]
    assert same.mean() >= 0.995, same.mean()
    rel = np.abs(g["luminance"][same] - o["luminance"][same]) / np.maximum(o["luminance"][same], 1e-3)
    assert np.quantile(rel, 0.99) < 2e-3, np.quantile(rel, 0.99)
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert (g["luminance"] > 0).mean() > 0.3   # the scene is lit
    orc.close()
    ctx.close()


@pytest.mark.parametrize("kw", [dict(type="orbital"), dict(type="green"), dict(type="mira")],
                         ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
def test_point_lit_chains_are_the_same_across_kernel_generations(pkg, native_lib, kw):
    sd = pkg.scenes.cornell_point(32)
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


def test_point_lit_pool_kernel_with_rows_in_memory(pkg, native_lib, capfd):
    """k_mutate_v5 at 163 840 chains: its proposal rows move to device memory (three waves per SIMD)."""
    sd = pkg.scenes.cornell_point(128)
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
def test_point_lit_mlt_image_is_unbiased(pkg, native_lib, algo):
    abi = pkg.abi
    sd = pkg.scenes.cornell_point(32)
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
