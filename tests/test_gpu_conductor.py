"""Smooth conductor (src/bsdfs/conductor.cpp) on the device: f(u) against a closed form, against the fp64 oracle's
alpha -> 0 limit of the rough conductor under all three techniques, the same chains across the kernel builds that carry
the branch, and images of every technique and both chain loops."""
import os

import numpy as np
import pytest

import conductor_scenes as cs

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


# ---------------------------------------------------------------- 1. closed form, technique=path
def test_mirrored_point_lit_plane_matches_the_closed_form(pkg, native_lib):
    """Camera -> copper mirror at 45 degrees -> diffuse square lit by one point light:
    f = R o F_exact(cos theta_1) * rho / pi * I * cos theta_2 / d^2, within 1e-4 (the bound of
    test_point_lit_plane_matches_the_closed_form); a mirrored ray that misses the square gives 0."""
    sd = cs.mirror_plane(pkg)
    cfg = pkg.abi.make_config(type="orbital", max_depth=3, rr_depth=100, direct_samples=-1, work_units=64)
    ctx = pkg.Context(cfg, sd)
    u = np.random.default_rng(11).random((32768, 32), dtype=np.float32)
    g = ctx.eval_paths(u)
    ctx.close()
    want, inside, outside = cs.mirror_plane_closed_form(pkg, g["x"], g["y"])
    assert inside.sum() > 8192 and outside.sum() > 1000, (inside.sum(), outside.sum())
    rel = np.abs(g["rgb"][inside] - want[inside]) / want[inside]
    print("closed form: max rel err %.3g over %d points, %d outside" % (rel.max(), inside.sum(), outside.sum()))
    assert rel.max() < 1e-4, rel.max()
    assert np.all(g["rgb"][outside] == 0)
    assert np.all(g["n_dims"][inside] == 8)        # film 2, mirror 2 (no light sample), plane 2 + 2


# ---------------------------------------------------------------- 2. the oracle's alpha -> 0 limit
def _profile(tag, lum_a, lum_b, same):
    """Topology share and the relative luminance error quantiles of run a against run b (b the reference)."""
    share = float(same.mean())
    same = same & ((lum_a > 0) | (lum_b > 0))     # quantiles over the points that carry light on either side: zeros agree trivially
    rel = np.abs(lum_a - lum_b)[same] / np.maximum(lum_b[same], 1e-3)
    q = [float(np.quantile(rel, p)) for p in (0.5, 0.9, 0.99)]
    print("%s: topology %.4f %%, rel err over %d lit points q50 %.3g q90 %.3g q99 %.3g" % (tag, 100 * share, same.sum(), *q))
    return share, q


def _hold_to_the_oracle_pair(tag, lg, lo1, lo2, same_g, same_o):
    """Device (mirror) against oracle(alpha = 1e-4), held to the oracle's own alpha = 1e-4 against 2e-4: to first order in alpha
    the mirror is as far from 1e-4 as 1e-4 is from 2e-4; the factor 2 covers the linearisation and fp32, the floor of 1e-5
    the scenes on which the pair's median is 0."""
    share_o, q_o = _profile(tag + " oracle 1e-4 vs 2e-4", lo2, lo1, same_o)
    share_g, q_g = _profile(tag + " device vs oracle 1e-4", lg, lo1, same_g)
    nz = lo1 > 0
    print("%s: %.4f %% of the %d non-zero points enter the comparison" % (tag, 100 * same_g[nz].mean(), nz.sum()))
    d = lg.astype(np.float64) - lo1.astype(np.float64)
    se = d.std(ddof=1) / np.sqrt(len(d))           # the two means share their points: Var(mean_g - mean_o) = Var(g - o) / n
    print("%s: mean f device %.6g oracle %.6g, difference %.3g = %.2f standard errors" % (tag, lg.mean(), lo1.mean(), d.mean(), abs(d.mean()) / se))
    assert share_g >= share_o - 1e-3, (share_g, share_o)
    for p, a, b in zip((50, 90, 99), q_g, q_o):
        assert a <= 2 * b + 1e-5, (tag, p, a, b)
    assert same_g[nz].mean() >= 0.99, same_g[nz].mean()
    assert abs(d.mean()) <= 3 * se, (d.mean(), se)


def test_path_is_the_limit_of_the_oracles_rough_conductor(pkg, ob, native_lib):
    """technique=path on the view-filling floor, maxDepth 3: the floor can only be vertex 1, where the rough twin draws two
    light-sample components that the mirror does not -- the oracle gets the device's u with two fresh components at 2 and 3.
    The twin's light sample there is always valid (every floor point lies below the ceiling light, which faces it), so the
    oracle, like the reference, traces its shadow ray before it evaluates the BSDF: the same topology is two components and
    one ray more on the oracle's side."""
    sd = cs.floor_view(pkg)
    cfg = pkg.abi.make_config(type="orbital", max_depth=3, rr_depth=100, direct_samples=-1, work_units=64)
    ctx = pkg.Context(cfg, sd)
    o1 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 1e-4), precision=64)
    o2 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 2e-4), precision=64)
    rng = np.random.default_rng(5)
    n = 16384
    u = rng.random((n, 32), dtype=np.float32)
    uo = np.concatenate([u[:, :2], rng.random((n, 2), dtype=np.float32), u[:, 2:]], axis=1)
    g, a, b = ctx.eval_paths(u), o1.eval_paths(uo), o2.eval_paths(uo)
    ctx.close(), o1.close(), o2.close()
    assert (g["luminance"] > 0).mean() > 0.3
    same_g = (g["n_dims"] + 2 == a["n_dims"]) & (g["n_rays"] + 1 == a["n_rays"])
    same_o = (b["n_dims"] == a["n_dims"]) & (b["n_rays"] == a["n_rays"])
    _hold_to_the_oracle_pair("path floor_view", g["luminance"], a["luminance"], b["luminance"], same_g, same_o)


@pytest.mark.parametrize("name", ["floor_view", "mirror_room"])
def test_bdpt_is_the_limit_of_the_oracles_rough_conductor(pkg, ob, native_lib, name):
    """technique=bdpt without direct sampling, the same u on both sides: every walk vertex draws two components either way.
    (With direct sampling the same u does not hold: the direct sampler's components are drawn in sequence, one pair per cell
    whose vertex can be connected -- bdpt.cpp skips a degenerate vertex before it samples --, so the rough twin draws pairs
    the mirror does not and every later pair shifts. That difference is what the next test holds the device to.)"""
    direct = 0
    sd = cs.LIMIT_SCENES[name](pkg)
    cfg = pkg.abi.make_config(technique="bdpt", type="orbital", max_depth=6, rr_depth=100, direct_samples=-1,
                              no_direct_sampling=0 if direct else 1, luminance_samples=20000, work_units=1024)
    ctx = pkg.Context(cfg, sd)
    o1 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 1e-4), 64)
    o2 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 2e-4), 64)
    rng = np.random.default_rng(11)
    n = 16384
    us, ue, ud = (rng.random((n, 24), dtype=np.float32) for _ in range(3))
    args = (us, ue, ud) if direct else (us, ue)
    g, a, b = ctx.eval_lists_bdpt(*args), o1.bdpt_eval(*args), o2.bdpt_eval(*args)
    ctx.close(), o1.close(), o2.close()
    topo = lambda p, q: (p[:, 1] == q[:, 1]) & (p[:, 7] == q[:, 7]) & (p[:, 8] == q[:, 8]) & (p[:, 9] == q[:, 9])
    _hold_to_the_oracle_pair("bdpt %s %s" % (name, "direct" if direct else "nodirect"), g[:, 0], a[:, 0], b[:, 0], topo(g, a), topo(b, a))


def test_bdpt_direct_sampling_draws_nothing_at_the_mirror(pkg, ob, native_lib):
    """directSampling = true on the view-filling floor: the camera's first surface vertex is always the floor, and the cell
    s = 1, t = 2 connects a directly sampled emitter point to it. The oracle's rough twin can be connected there and draws
    that cell's pair of direct components; the mirror is degenerate and must draw none (bdpt.cpp: `isDegenerate` is tested
    before `sampleDirect`). So wherever both sides made the same walks (the same component count without direct sampling),
    the oracle consumes at least one pair more than the device, and both consume whole pairs."""
    sd = cs.floor_view(pkg)
    rng = np.random.default_rng(13)
    n = 8192
    us, ue, ud = (rng.random((n, 24), dtype=np.float32) for _ in range(3))
    dims = {}
    for direct in (0, 1):
        cfg = pkg.abi.make_config(technique="bdpt", type="orbital", max_depth=6, rr_depth=100, direct_samples=-1,
                                  no_direct_sampling=1 - direct, luminance_samples=20000, work_units=1024)
        ctx, orc = pkg.Context(cfg, sd), ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 1e-4), 64)
        args = (us, ue, ud) if direct else (us, ue)
        dims[direct] = (ctx.eval_lists_bdpt(*args)[:, 8].astype(int), orc.bdpt_eval(*args)[:, 8].astype(int))
        ctx.close(), orc.close()
    walks = dims[0][0] == dims[0][1]
    nd_g, nd_o = dims[1][0] - dims[0][0], dims[1][1] - dims[0][1]
    print("bdpt direct floor_view: same walks %.4f %%, direct components device mean %.2f oracle twin mean %.2f, oracle >= device + 2 on %.4f %%"
          % (100 * walks.mean(), nd_g[walks].mean(), nd_o[walks].mean(), 100 * (nd_o - nd_g >= 2)[walks].mean()))
    assert walks.mean() > 0.99
    assert np.all(nd_g % 2 == 0) and np.all(nd_g >= 0) and nd_g.max() > 0
    assert (nd_o - nd_g >= 2)[walks].mean() > 0.99


@pytest.mark.parametrize("name", ["floor_view", "mirror_room"])
def test_mmlt_is_the_limit_of_the_oracles_rough_conductor(pkg, ob, native_lib, name):
    """technique=mmlt, every depth of a maxDepth-6 path space, the same u on both sides."""
    sd = cs.LIMIT_SCENES[name](pkg)
    cfg = pkg.abi.make_config(technique="mmlt", type="orbital", max_depth=6, direct_samples=-1, luminance_samples=20000, work_units=64)
    ctx = pkg.Context(cfg, sd)
    o1 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 1e-4), 64)
    o2 = ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 2e-4), 64)
    rng = np.random.default_rng(7)
    n = 4096
    us, ue = rng.random((n, 14), dtype=np.float32), rng.random((n, 14), dtype=np.float32)
    ud = rng.random(n, dtype=np.float32)
    lg, la, lb, sg, so = [], [], [], [], []
    for depth in range(2, 7):
        g, stg = ctx.eval_paths_mmlt(depth, us, ue, ud)
        a, sta = o1.mmlt_eval(depth, us, ue, ud)
        b, stb = o2.mmlt_eval(depth, us, ue, ud)
        topo = lambda p, sp: (p["n_dims"] == a["n_dims"]) & (p["n_rays"] == a["n_rays"]) & (sp == sta).all(axis=1)
        lg.append(g["luminance"]), la.append(a["luminance"]), lb.append(b["luminance"]), sg.append(topo(g, stg)), so.append(topo(b, stb))
    ctx.close(), o1.close(), o2.close()
    lg, la, lb, sg, so = (np.concatenate(v) for v in (lg, la, lb, sg, so))
    _hold_to_the_oracle_pair("mmlt " + name, lg, la, lb, sg, so)


# ---------------------------------------------------------------- 3. chains and kernels
BUILDS = [dict(DRMLT_KERNEL=3), dict(DRMLT_KERNEL=4), dict(DRMLT_KERNEL=5), dict(DRMLT_KERNEL=5, DRMLT_ROWS_MEM=1),
          dict(DRMLT_KERNEL=4, DRMLT_TABLES_LDS=0), dict(DRMLT_KERNEL=5, DRMLT_TABLES_LDS=0)]


@pytest.mark.parametrize("kw", [dict(type="orbital"), dict(type="green"), dict(type="mira")], ids=lambda k: k["type"])
def test_mirror_room_chains_are_the_same_across_kernel_builds(pkg, native_lib, kw):
    sd = pkg.scenes.mirror_room(32)
    n_chains, n_mut = 1000, 60
    cfg = pkg.abi.make_config(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1, **kw)
    results = []
    for env in BUILDS:
        ctx = _ctx_with_env(pkg, cfg, sd, **env)
        ctx.seed(0x5005)
        ctx.run(n_chains * n_mut)
        results.append((ctx.chain_state(34), ctx.stats(), ctx.film()))
        ctx.close()
    (c0, u0), s0, f0 = results[0]
    assert s0.mutations == n_chains * n_mut and s0.accepted > 0
    for env, ((c, u), s, f) in zip(BUILDS[1:], results[1:]):
        assert np.array_equal(u, u0) and np.array_equal(c["luminance"], c0["luminance"]), env
        for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
            assert getattr(s, k + "_base") == getattr(s0, k + "_base") and getattr(s, k + "_acc") == getattr(s0, k + "_acc"), (env, k)
        assert s.rays == s0.rays and s.path_evals == s0.path_evals and s.accepted == s0.accepted, env
        assert lum(f).sum() == pytest.approx(lum(f0).sum(), rel=1e-5)
        assert np.abs(lum(f) - lum(f0)).sum() / lum(f0).sum() < 1e-4


# ---------------------------------------------------------------- 4. images
BASE = dict(type="orbital", max_depth=6, rr_depth=100, direct_samples=-1)


@pytest.fixture(scope="module")
def mirror_room_pt(pkg, native_lib):
    sd = pkg.scenes.mirror_room(32)
    ctx = pkg.Context(pkg.abi.make_config(work_units=64, **BASE), sd)
    ref = ctx.render_pt(8192, seed=5)
    ctx.close()
    return ref


@pytest.mark.parametrize("algo", ["drmlt", "pssmlt"])
def test_mirror_room_path_image_matches_path_tracing(pkg, native_lib, mirror_room_pt, algo):
    """The bounds of test_point_lit_mlt_image_is_unbiased."""
    abi, ref = pkg.abi, mirror_room_pt
    spp = 2048
    extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
    ctx = pkg.Context(abi.make_config(work_units=4096, sample_count=spp, luminance_samples=200000, **BASE, **extra), pkg.scenes.mirror_room(32))
    b = ctx.seed(9)
    ctx.run(32 * 32 * spp)
    img = ctx.develop()
    ctx.close()
    print("mirror_room %s path: b %.6g, render_pt mean %.6g, rel MSE %.3g" % (algo, b, lum(ref).mean(), rel_mse(img, ref)))
    assert b == pytest.approx(lum(ref).mean(), rel=0.02)
    assert lum(img).mean() == pytest.approx(b, rel=1e-3)
    assert rel_mse(img, ref) < 1e-2, rel_mse(img, ref)


@pytest.mark.parametrize("technique", ["bdpt", "bdpt-direct", "mmlt"])
def test_mirror_room_bidirectional_image_matches_path_tracing(pkg, native_lib, mirror_room_pt, technique):
    """The bounds of test_bdpt_image_and_acceptance_map and test_mmlt_image_matches_path_tracing."""
    abi, ref = pkg.abi, mirror_room_pt
    if technique.startswith("bdpt"):   # bdpt-direct: directSampling = true, the reference's default
        kw, spp, tol_b = dict(technique="bdpt", no_direct_sampling=0 if technique == "bdpt-direct" else 1, work_units=8192, luminance_samples=200000), 512, 0.02
    else:
        kw, spp, tol_b = dict(technique="mmlt", fix_emitter_path=1, work_units=16384, luminance_samples=100000), 2048, 0.03
    ctx = pkg.Context(abi.make_config(sample_count=spp, **dict(BASE, **kw)), pkg.scenes.mirror_room(32))
    b = ctx.seed(0x5EED)
    ctx.run(32 * 32 * spp)
    img = ctx.develop()
    ctx.close()
    blk = lambda a: a.reshape(8, 4, 8, 4, 3).mean((1, 3))
    err = np.abs(blk(img) - blk(ref)).mean() / ref.mean()
    print("mirror_room %s: b %.6g, render_pt mean %.6g, block error %.3g" % (technique, b, lum(ref).mean(), err))
    assert b == pytest.approx(lum(ref).mean(), rel=tol_b)
    assert err < 0.04, err


def test_mirror_room_path_traced_image_matches_the_oracles_limit(pkg, ob, native_lib):
    """Device render_pt of the mirror against the oracle's render_pt of the alpha = 1e-4 twin, the protocol of
    test_path_traced_image_matches_the_oracle: 4 x 4 blocks of 8 x 8 pixels, K independent images a side, the bound 6 of the
    combined measured standard error."""
    sd = pkg.scenes.mirror_room(32)
    cfg = pkg.abi.make_config(work_units=64, **BASE)
    ctx, orc = pkg.Context(cfg, sd), ob.Oracle(pkg.abi, cfg, cs.rough_twin(pkg, sd, 1e-4), precision=64)
    K = 16
    blocks = lambda img: lum(img).reshape(4, 8, 4, 8).mean(axis=(1, 3))
    bg = np.array([blocks(ctx.render_pt(1024, seed=100 + k)) for k in range(K)])
    bo = np.array([blocks(orc.render_pt(128, seed=200 + k, nthreads=8)) for k in range(K)])
    ctx.close(), orc.close()
    mg, mo = bg.mean(axis=0), bo.mean(axis=0)
    se = np.sqrt(bg.var(axis=0, ddof=1) / K + bo.var(axis=0, ddof=1) / K)
    z = np.abs(mg - mo) / se
    print("render_pt mirror_room: max z %.2f, max rel se %.3g, max rel diff %.3g" % (z.max(), (se / mo).max(), (np.abs(mg - mo) / mo).max()))
    assert mo.min() > 0 and (se / mo).max() < 0.02
    assert z.max() < 6, z
