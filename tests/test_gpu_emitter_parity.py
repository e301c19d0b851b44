"""Point lights and the constant environment on the device, held to the fp64 oracle point by point and chain by chain
(test_gpu_parity.py's protocols on the scenes of emitter_scenes.py):
  a. f(u) per PSS point: eval_paths (path_step<false, 15> with global tables) against the oracle;
  b. bootstrap luminances and the seed picks;
  c. chains against the oracle's chains;
  d. every chain kernel build that carries feature bit 4 (path_step<true, FEAT>: shadow rays on the partner lane, LDS /
     hybrid / global tables, BVH or brute-force loop), replayed: the oracle evaluates the device's own chain states; and the
     BVH builds of v3 / v4 / v5 run the same chains bit for bit;
  e. path-traced images against the oracle's, block by block, within a bound taken from the measured spread."""
import os
import re

import numpy as np
import pytest

import emitter_scenes as es

pytestmark = pytest.mark.gpu
LUMW = np.array([0.212671, 0.715160, 0.072169])


def lum(img):
    return img @ LUMW


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def make(pkg, ob, sd, **kw):
    base = dict(max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000)
    base.update(kw)
    cfg = pkg.abi.make_config(**base)
    return cfg, pkg.Context(cfg, sd), ob.Oracle(pkg.abi, cfg, sd, 64)


# ---------------------------------------------------------------- a. f(u) per point
EVAL_CASES = [(name, -1) for name in es.EMITTER_SCENES] + [("cornell_sky", 16)]


@pytest.mark.parametrize("name,direct_samples", EVAL_CASES, ids=["%s-ds%d" % c for c in EVAL_CASES])
def test_eval_paths_match_the_oracle(pkg, ob, native_lib, name, direct_samples):
    sd = es.EMITTER_SCENES[name](pkg)
    cfg, ctx, orc = make(pkg, ob, sd, type="orbital", work_units=64, direct_samples=direct_samples)
    u = np.random.default_rng(1).random((8192, 64), dtype=np.float32)
    g, o = ctx.eval_paths(u), orc.eval_paths(u)
    ctx.close(), orc.close()
    same = g["n_dims"] == o["n_dims"]
    rel = np.abs(g["luminance"] - o["luminance"])[same] / np.maximum(o["luminance"][same], 1e-3)
    q99 = float(np.quantile(rel, 0.99))
    print("eval_paths %s ds=%d: same topology %.5f, q99 rel %.3g, lit %.3f" % (name, direct_samples, same.mean(), q99, (o["luminance"] > 0).mean()))
    assert same.mean() >= 0.995, same.mean()
    assert np.all(g["n_rays"][same] <= o["n_rays"][same])
    assert np.allclose(g["x"], o["x"], atol=1e-3) and np.allclose(g["y"], o["y"], atol=1e-3)
    assert q99 < 1e-3, q99
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert np.allclose(g["rgb"][same], o["rgb"][same], rtol=5e-2, atol=1e-3)
    assert (o["luminance"] > 0).mean() > (0.02 if direct_samples >= 0 else 0.2)   # the emitters light the scene


# ---------------------------------------------------------------- b. bootstrap and seeding
SEED_SCENES = ["cornell_sky_quad", "cornell_point_quad"]


@pytest.mark.parametrize("name", SEED_SCENES)
def test_bootstrap_and_seed_picks_match_the_oracle(pkg, ob, native_lib, name):
    sd = es.EMITTER_SCENES[name](pkg)
    cfg, ctx, orc = make(pkg, ob, sd, type="orbital", work_units=4096, sample_count=1)
    bg, bo = ctx.seed(0x5EED), orc.seed(0x5EED)
    assert bg == pytest.approx(bo, rel=2e-4)
    # (1) the oracle's resampler on the device's own bootstrap luminances picks exactly the device's seeds
    n_boot = 10 * 4096
    lum_dev = ctx.bootstrap_luminances(0x5EED, 0, n_boot)
    picks = ob.select_seeds(lum_dev, 0x5EED, 0, 4096)
    assert np.array_equal(picks, ctx.seed_indices())
    assert np.all(lum_dev[picks] > 0)
    # (2) device and oracle luminances agree but for the few samples on a discontinuity of f
    lum_orc = orc.bootstrap_lum(0x5EED, 0, n_boot)
    rel = np.abs(lum_dev - lum_orc) / np.maximum(np.maximum(lum_orc, lum_dev), 1e-6)
    jumps = rel > 1e-3
    q99 = float(np.quantile(rel, 0.99))
    print("bootstrap %s: q99 rel %.3g, %d jumps of %d" % (name, q99, int(jumps.sum()), n_boot))
    assert q99 < 1e-4 and jumps.sum() < 3e-3 * n_boot, (q99, int(jumps.sum()))
    picks_fixed = ob.select_seeds(np.where(jumps, lum_dev, lum_orc), 0x5EED, 0, 4096)
    assert np.intersect1d(picks, picks_fixed).size / np.unique(picks_fixed).size >= 0.95
    ctx.close(), orc.close()


# ---------------------------------------------------------------- c. chains against the oracle's
CHAIN_VARIANTS = [dict(type="orbital"), dict(type="green"), dict(type="mira"), dict(type="orbital", use_mixture=1),
                  dict(type="mira", timid_after_large=1)]


@pytest.mark.parametrize("kw", CHAIN_VARIANTS, ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
@pytest.mark.parametrize("name", SEED_SCENES)
def test_chains_track_the_oracle(pkg, ob, native_lib, name, kw):
    sd = es.EMITTER_SCENES[name](pkg)
    n_chains, n_mut = 2048, 48
    cfg, ctx, orc = make(pkg, ob, sd, work_units=n_chains, sample_count=1, **kw)
    ctx.seed(0xABCD), orc.seed(0xABCD)
    (c0g, u0g), (c0o, u0o) = ctx.chain_state(34), orc.chain_state(34)
    same0 = np.all(u0g == u0o, axis=1)
    ctx.run(n_chains * n_mut)
    orc.run(n_chains * n_mut, 8)
    (cg, ug), (co, uo) = ctx.chain_state(34), orc.chain_state(34)
    tracked = np.all(np.abs(ug - uo) < 2e-3, axis=1) & same0
    frac = tracked.sum() / same0.sum()
    print("chains %s %s: tracked %.4f of %d" % (name, kw, frac, int(same0.sum())))
    assert frac > 0.97, frac
    sg, so = ctx.stats(), orc.stats()
    assert sg.mutations == so.mutations == n_chains * n_mut
    for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
        bg, bo = getattr(sg, k + "_base"), getattr(so, k + "_base")
        assert abs(bg - bo) <= 0.01 * max(bo, 1) + 20, (k, bg, bo)
        if bo > 200:
            pg, po = getattr(sg, k + "_acc") / bg, getattr(so, k + "_acc") / bo
            assert abs(pg - po) < 4 * np.sqrt(po * (1 - po) / bo) + 0.01, (k, pg, po)
    assert abs(sg.path_evals - so.path_evals) <= 0.01 * so.path_evals
    # The device skips the shadow ray of a light sample whose BSDF value is zero; the reference traces it first
    # (scene.cpp:890-895). A point light has no facing test, so on its scenes that is a few percent of the rays: measured here
    # on the states the chains hold, as the gap between the oracle's and the device's ray counts of the same paths.
    pad = np.pad(ug, ((0, 0), (0, 30)))
    rg, ro = ctx.eval_paths(pad)["n_rays"].astype(np.int64), orc.eval_paths(pad)["n_rays"].astype(np.int64)
    assert np.all(rg <= ro)
    skip = (ro - rg).sum() / ro.sum()
    print("chains %s %s: rays device %d oracle %d, shadow rays skipped on the states %.4f" % (name, kw, sg.rays, so.rays, skip))
    assert abs(sg.rays - so.rays * (1 - skip)) <= 0.02 * so.rays
    fg, fo = ctx.film(), orc.film()
    assert lum(fg).sum() == pytest.approx(lum(fo).sum(), rel=2e-3)
    bgk, bok = (lum(f).reshape(8, 4, 8, 4).sum(axis=(1, 3)) for f in (fg, fo))
    assert np.abs(bgk - bok).sum() / bok.sum() < 0.06
    assert lum(ctx.develop()).mean() == pytest.approx(lum(orc.develop()).mean(), rel=2e-3)
    ctx.close(), orc.close()


# ---------------------------------------------------------------- d. every build that carries bit 4, replayed
# (id, environment, algo, kernel named by DRMLT_VERBOSE or None, BVH forced on the flat scene)
BUILDS = [
    ("v3", dict(DRMLT_KERNEL=3), "drmlt", "k_mutate_v3", False),
    ("v4", dict(DRMLT_KERNEL=4), "drmlt", "k_mutate_v4", False),
    ("v5", dict(DRMLT_KERNEL=5), "drmlt", "k_mutate_v5", False),
    ("v5-rows-mem", dict(DRMLT_KERNEL=5, DRMLT_ROWS_MEM=1), "drmlt", "k_mutate_v5", False),
    ("v3-bvh", dict(DRMLT_KERNEL=3, DRMLT_BVH_THRESHOLD=0), "drmlt", "k_mutate_v3", True),
    ("v4-bvh", dict(DRMLT_KERNEL=4, DRMLT_BVH_THRESHOLD=0), "drmlt", "k_mutate_v4", True),
    ("v5-bvh", dict(DRMLT_KERNEL=5, DRMLT_BVH_THRESHOLD=0), "drmlt", "k_mutate_v5", True),
    ("v4-stack32", dict(DRMLT_KERNEL=4, DRMLT_BVH_THRESHOLD=0, DRMLT_BVH_STACK32=1), "drmlt", "k_mutate_v4", True),
    ("v5-stack32", dict(DRMLT_KERNEL=5, DRMLT_BVH_THRESHOLD=0, DRMLT_BVH_STACK32=1), "drmlt", "k_mutate_v5", True),
    ("v4-global-tables", dict(DRMLT_KERNEL=4, DRMLT_TABLES_LDS=0), "drmlt", "k_mutate_v4", False),
    ("v5-global-tables", dict(DRMLT_KERNEL=5, DRMLT_TABLES_LDS=0), "drmlt", "k_mutate_v5", False),
    ("pssmlt", dict(), "pssmlt", None, False),
]
REPLAY_CHAINS, REPLAY_MUT = 2048, 64


def _run_build(pkg, sd, env, algo, capfd, kw=None):
    """Seed and run REPLAY_MUT mutations per chain under `env` (read at creation and by drmlt_run); returns chain state,
    statistics, film and the DRMLT_VERBOSE log."""
    abi = pkg.abi
    extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
    cfg = abi.make_config(max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=REPLAY_CHAINS,
                          sample_count=1, **(kw or dict(type="orbital")), **extra)
    capfd.readouterr()

    def go():
        ctx = pkg.Context(cfg, sd)
        ctx.seed(0x77)
        ctx.run(REPLAY_CHAINS * REPLAY_MUT)
        out = (ctx.chain_state(34), ctx.stats(), ctx.film())
        ctx.close()
        return out

    out = _with_env(dict(env, DRMLT_VERBOSE=1), go)
    return out + (capfd.readouterr().err,)


@pytest.mark.parametrize("scene", ["mixed", "soup"])
@pytest.mark.parametrize("build", BUILDS, ids=[b[0] for b in BUILDS])
def test_chain_kernel_builds_replay_against_the_oracle(pkg, ob, native_lib, capfd, scene, build):
    bid, env, algo, kernel, forced_bvh = build
    sd = es.EMITTER_SCENES[scene](pkg)
    (cur, u), st, film, log = _run_build(pkg, sd, env, algo, capfd)
    # the build that ran
    bvh = scene == "soup" or forced_bvh
    assert ("BVH:" in log) == bvh, log
    if kernel:
        assert ("[drmlt] %s:" % kernel) in log, log
    if "DRMLT_ROWS_MEM" in env:
        assert re.search(r"k_mutate_v5: \d+ B of LDS per wave.*; proposal rows in device memory", log), log
    if "DRMLT_BVH_STACK32" in env:
        assert "32-bit stack entries" in log, log
    if kernel in ("k_mutate_v4", "k_mutate_v5"):
        assert (st.bvh_node_visits > 0) == bvh, st.bvh_node_visits
    assert st.mutations == REPLAY_CHAINS * REPLAY_MUT and st.accepted > 0
    # the oracle on the device's own states
    orc = ob.Oracle(pkg.abi, pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64), sd, 64)
    chk = orc.eval_paths(np.pad(u, ((0, 0), (0, 30))))
    orc.close()
    ok = np.abs(chk["luminance"] - cur["luminance"]) <= 1e-3 * cur["luminance"]
    print("replay %s %s: %.4f of %d chains agree" % (scene, bid, ok.mean(), len(ok)))
    assert np.all(cur["luminance"] > 0)
    assert ok.mean() >= 0.995, ok.mean()
    assert np.allclose(chk["x"][ok], cur["x"][ok], atol=1e-3) and np.allclose(chk["y"][ok], cur["y"][ok], atol=1e-3)
    film_sum = lum(film).sum()
    assert np.isfinite(film_sum) and film_sum > 0


@pytest.mark.parametrize("kw", [dict(type="orbital"), dict(type="green"), dict(type="mira")],
                         ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
@pytest.mark.parametrize("scene", ["mixed", "soup"])
def test_bvh_builds_run_the_same_chains_across_kernel_generations(pkg, native_lib, capfd, scene, kw):
    sd = es.EMITTER_SCENES[scene](pkg)
    res = []
    for k in (3, 4, 5):
        env = dict(DRMLT_KERNEL=k, DRMLT_BVH_THRESHOLD=0)
        (c, u), s, f, log = _run_build(pkg, sd, env, "drmlt", capfd, kw)
        assert "BVH:" in log and ("[drmlt] k_mutate_v%d:" % k) in log, log
        res.append(((c, u), s, f))
    (c0, u0), s0, f0 = res[0]
    for (c, u), s, f in res[1:]:
        assert np.array_equal(u, u0) and np.array_equal(c["luminance"], c0["luminance"])
        for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
            assert getattr(s, k + "_base") == getattr(s0, k + "_base") and getattr(s, k + "_acc") == getattr(s0, k + "_acc")
        assert s.rays == s0.rays and s.path_evals == s0.path_evals and s.accepted == s0.accepted
        assert lum(f).sum() == pytest.approx(lum(f0).sum(), rel=1e-5)
        assert np.abs(lum(f) - lum(f0)).sum() / lum(f0).sum() < 1e-4
    assert res[1][1].bvh_node_visits > 0 and res[2][1].bvh_node_visits > 0


def test_flat_scene_whose_tables_do_not_fit_in_lds(pkg, ob, native_lib, capfd):
    """160 more point lights: the brute-force scene's shading, BSDF and emitter tables (> 16 KB) stay in device memory. The
    default chain kernel at this chain count, k_mutate_v4, then runs its global-table build of the brute-force loop (it once
    took a BVH build, whose traversal reads a tree the scene does not have). Its chains replay against the oracle and equal
    k_mutate_v3's bit for bit."""
    sd = es.mixed(pkg)
    rng = np.random.default_rng(9)
    for p in rng.uniform((-0.9, -0.9, -0.9), (0.9, 0.9, 0.9), (160, 3)):
        sd.point_light(tuple(p), intensity=tuple(rng.uniform(0.01, 0.05, 3)), sampling_weight=float(rng.uniform(0.02, 0.1)))
    assert len(sd.emitters) == 164
    res = []
    for env in (dict(), dict(DRMLT_KERNEL=3)):
        (c, u), st, film, log = _run_build(pkg, sd, env, "drmlt", capfd)
        m = re.search(r"\[drmlt\] (k_mutate_v\d): (\d+) B of LDS per wave", log)
        assert m and m.group(1) == ("k_mutate_v3" if env else "k_mutate_v4") and "BVH:" not in log, log
        assert int(m.group(2)) < 24576 and st.bvh_node_visits == 0, log   # rows and queue only: the tables would add > 16 KB
        res.append(((c, u), st, film))
    ((c4, u4), s4, f4), ((c3, u3), s3, f3) = res
    assert np.array_equal(u4, u3) and np.array_equal(c4["luminance"], c3["luminance"])
    assert s4.accepted == s3.accepted and s4.rays == s3.rays and s4.path_evals == s3.path_evals
    assert lum(f4).sum() == pytest.approx(lum(f3).sum(), rel=1e-5)
    orc = ob.Oracle(pkg.abi, pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=64), sd, 64)
    chk = orc.eval_paths(np.pad(u4, ((0, 0), (0, 30))))
    orc.close()
    ok = np.abs(chk["luminance"] - c4["luminance"]) <= 1e-3 * c4["luminance"]
    print("replay mixed + 160 point lights, v4 global tables: %.4f of %d chains agree" % (ok.mean(), len(ok)))
    assert ok.mean() >= 0.995, ok.mean()


# ---------------------------------------------------------------- e. images
@pytest.mark.parametrize("name", ["rough_sky", "mixed"])
def test_path_traced_image_matches_the_oracle(pkg, ob, native_lib, name):
    """Device render_pt against oracle render_pt, 4 x 4 blocks of 8 x 8 pixels, independent seeds. Each side renders K images;
    the spread of their block means gives each side's standard error, and the bound is 6 of the combined error."""
    sd = es.EMITTER_SCENES[name](pkg)
    cfg, ctx, orc = make(pkg, ob, sd, type="orbital", work_units=64)
    K = 16

    def blocks(img):
        return lum(img).reshape(4, 8, 4, 8).mean(axis=(1, 3))

    bg = np.array([blocks(ctx.render_pt(1024, seed=100 + k)) for k in range(K)])
    bo = np.array([blocks(orc.render_pt(128, seed=200 + k, nthreads=8)) for k in range(K)])
    ctx.close(), orc.close()
    mg, mo = bg.mean(axis=0), bo.mean(axis=0)
    se = np.sqrt(bg.var(axis=0, ddof=1) / K + bo.var(axis=0, ddof=1) / K)
    z = np.abs(mg - mo) / se
    print("render_pt %s: max z %.2f, max rel se %.3g, max rel diff %.3g" % (name, z.max(), (se / mo).max(), (np.abs(mg - mo) / mo).max()))
    assert mo.min() > 0 and (se / mo).max() < 0.02            # the bound is tight enough to mean something
    assert z.max() < 6, z
