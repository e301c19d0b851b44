"""algo=pssmlt over technique=bdpt on the device (k_mutate_pssmlt_bdpt, PssmltSampler3): stock Mitsuba's PSSMLT,
PSSMLTRenderer::process (src/integrators/pssmlt/pssmlt_proc.cpp:110-285) over sampleSplats(EBidirectional).

No oracle restates this combination. What pins it down: a chain always holds the f of its u (the evaluation routine is
technique=bdpt's, which IS held to the oracle), the geometry of its proposals, its bookkeeping, its independence of launch
boundaries and of the build, its weights against algo=pssmlt over technique=path, and its image against the fp64 bdpt estimator."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LUMW = np.array([0.212671, 0.715160, 0.072169])
S1, S2 = 1.0 / 1024.0, 1.0 / 64.0   # Kelemen's mutation sizes (pssmlt_sampler.h:120-121)
N_CHAINS = 1024


def lum(img):
    return img @ LUMW


def config(pkg, **kw):
    base = dict(algo=pkg.abi.ALGO_PSSMLT, technique="bdpt", type="orbital", max_depth=6, rr_depth=4, direct_samples=-1,
                work_units=N_CHAINS, sample_count=1, luminance_samples=20000)
    base.update(kw)
    return pkg.abi.make_config(**base)


def make(pkg, sd=None, **kw):
    cfg = config(pkg, **kw)
    return cfg, pkg.Context(cfg, sd if sd is not None else pkg.scenes.cornell_c2(32))


def dims(cfg):
    """(S, E, Dd): components of the sensor, emitter and direct segments of a chain's state (csrc/device_bdpt.h)."""
    rr = cfg.max_depth + 1 - max(cfg.rr_depth, 0)
    S = 2 * (cfg.max_depth + 1) + max(rr, 0); S += S & 1
    E = 2 * cfg.max_depth + max(rr - 1, 0); E += E & 1
    return S, E, 0 if cfg.no_direct_sampling else 2 * (2 * cfg.max_depth - 1)


def state(ctx):
    """(current splats, u [chains, S + E + Dd]) of a context's chains"""
    S, E, Dd = dims(ctx.cfg)
    cur, u = ctx.chain_state(ctx.stats().max_dim)
    assert not u[:, S + E + Dd:].any()
    return cur, u[:, :S + E + Dd]


def f_of(ctx, u):
    S, E, Dd = dims(ctx.cfg)
    return ctx.eval_lists_bdpt(u[:, :S], u[:, S:S + E], u[:, S + E:] if Dd else None)[:, 0]


def counters(st):
    return {k: v for k, v in st.as_dict().items() if k.endswith(("_acc", "_base")) or k in ("mutations", "path_evals", "rays", "accepted")}


def toroidal(a, b):
    d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return np.minimum(d, 1.0 - d)


@pytest.mark.parametrize("kelemen", [1, 0], ids=["kelemen", "gaussian"])
@pytest.mark.parametrize("nodirect", [0, 1], ids=["direct", "nodirect"])
def test_a_chain_holds_the_f_of_its_u(pkg, native_lib, nodirect, kelemen):
    """After seeding and after every run, evaluating a chain's state gives the chain's luminance, bit for bit: the same routine
    on the same inputs. A proposal that was evaluated from one vector and committed as another cannot pass."""
    cfg, ctx = make(pkg, no_direct_sampling=nodirect, kelemen_style_mutation=kelemen)
    ctx.seed(0xABCD)
    for n_mut in (0, 40, 40):
        if n_mut:
            ctx.run(N_CHAINS * n_mut)
        cur, u = state(ctx)
        f = f_of(ctx, u)
        same = f.view(np.uint32) == cur["luminance"].view(np.uint32)
        print("after %d more mutations: %d of %d chains hold f(u); max rel diff %.3g" % (
            n_mut, same.sum(), same.size, np.max(np.abs(f - cur["luminance"]) / cur["luminance"])))
        assert same.all()
        assert (u >= 0).all() and (u <= 1).all()
    assert ctx.stats().accepted > 0
    ctx.close()


@pytest.mark.parametrize("p_large", [0.3, 1.0, 0.0])
def test_proposal_geometry(pkg, native_lib, p_large):
    """One Kelemen mutation from a dumped state: a chain is unchanged (rejected), moved in EVERY component of all three segments by
    a toroidal distance in [1/1024, 1/64] (small step accepted), or redrawn (large step accepted).

    A redrawn component lands within that distance of the old one with probability q = 2 (1/64 - 1/1024) = 2.9 %: over all
    redrawn chains together fewer than 5 % of the components do. One chain has 54 components, and 3 or more of them (5 %) do so
    in one redrawn chain in five (binomial: 21 %), so a single chain is held to the count that not one of 1024 correctly
    redrawn chains exceeds with probability 1e-6 (13 of 54), and the 5 % to the redrawn chains as a whole."""
    cfg, ctx = make(pkg, p_large=p_large)
    S, E, Dd = dims(cfg)
    ctx.seed(0xABCD)
    ctx.run(N_CHAINS * 8)
    _, u0 = state(ctx)
    ctx.run(N_CHAINS * 1)
    _, u1 = state(ctx)
    assert ctx.stats().mutations == N_CHAINS * 9
    ctx.close()
    slack = 1e-6   # the fp32 add and wrap
    d = toroidal(u0, u1)
    inside = (d >= S1 - slack) & (d <= S2 + slack)
    rejected = (u0.view(np.uint32) == u1.view(np.uint32)).all(axis=1)
    small = ~rejected & inside.all(axis=1)
    q, nc = 2 * (S2 - S1), u0.shape[1]
    tail = lambda k: sum(math.comb(nc, j) * q ** j * (1 - q) ** (nc - j) for j in range(k + 1, nc + 1))   # P(more than k of nc inside)
    k_max = next(k for k in range(nc) if N_CHAINS * tail(k) < 1e-6)
    large = ~rejected & (inside.sum(axis=1) <= k_max) & (u1 >= 0).all(axis=1) & (u1 < 1).all(axis=1)
    print("p_large %.1f: %d rejected, %d small steps accepted, %d large steps accepted, %d none of these" % (
        p_large, rejected.sum(), small.sum(), large.sum(), (~(rejected | small | large)).sum()))
    assert (rejected | small | large).all()
    assert (rejected.astype(int) + small + large == 1).all() and k_max < nc // 2
    if large.any():
        print("components of the redrawn chains within the small-step distance: %.4f (q = %.4f); per chain at most %d, bound %d of %d" % (
            inside[large].mean(), q, inside[large].sum(axis=1).max(), k_max, nc))
        assert inside[large].mean() < 0.05
    if p_large == 1.0:
        assert not small.any() and large.sum() > 100
        # overlapping draw bases would give two segments the same uniforms
        ul = u1[large]
        ke, kd = min(S, E), min(S, Dd)
        assert not (ul[:, :ke] == ul[:, S:S + ke]).any() and not (ul[:, :kd] == ul[:, S + E:S + E + kd]).any()
        assert not (ul[:, S:S + min(E, Dd)] == ul[:, S + E:S + E + min(E, Dd)]).any()
    elif p_large == 0.0:
        assert not large.any() and small.sum() > 100
    else:
        assert small.sum() > 100 and large.sum() > 20
    if p_large < 1.0:
        # a reflecting wrap (wrap01) fails the distance test on chains that start within 1/64 of 0 or 1
        edge = ((u0 < S2) | (u0 > 1 - S2)).any(axis=1)
        wrapped = (np.abs(u1.astype(np.float64) - u0) > 0.5).any(axis=1)
        print("accepted small steps that start within 1/64 of an end: %d; that wrapped around: %d" % ((small & edge).sum(), (small & wrapped).sum()))
        assert (small & edge).sum() >= 20


def test_bookkeeping(pkg, native_lib):
    cfg, ctx = make(pkg)
    n = N_CHAINS * 40
    ctx.seed(0xABCD)
    ctx.run(n)
    st = ctx.stats()
    ctx.close()
    assert st.mutations == st.path_evals == st.overall_base == st.large_base + st.bold_base == n
    assert st.n_chains == N_CHAINS
    for k in ("first", "second", "second_large", "second_bold"):
        assert getattr(st, k + "_base") == 0 and getattr(st, k + "_acc") == 0, k
    p = cfg.p_large
    assert abs(st.large_base / n - p) <= 5 * np.sqrt(p * (1 - p) / n), st.large_base / n
    assert 0 < st.accepted < n and st.accepted == st.overall_acc == st.large_acc + st.bold_acc
    assert st.rays > n


def test_launch_splitting(pkg, native_lib):
    """The cumulative weight is flushed at every launch end and the chain goes on: one run and two runs are the same chains."""
    n = N_CHAINS * 40
    res = []
    for parts in ((n,), (n // 4, 3 * n // 4)):
        cfg, ctx = make(pkg)
        ctx.seed(0xABCD)
        for part in parts:
            ctx.run(part)
        res.append((state(ctx), counters(ctx.stats()), ctx.film()))
        ctx.close()
    ((c1, u1), s1, f1), ((c2, u2), s2, f2) = res
    assert np.array_equal(u1.view(np.uint32), u2.view(np.uint32))
    assert np.array_equal(c1["luminance"].view(np.uint32), c2["luminance"].view(np.uint32))
    assert s1 == s2
    assert lum(f2).sum() == pytest.approx(lum(f1).sum(), rel=1e-5)


def test_flat_and_bvh_builds_run_the_same_chains(pkg, native_lib, monkeypatch, capfd):
    """tests/test_gpu_bdpt.py::test_bvh_builds_of_the_bidirectional_kernels_run_the_same_chains for this loop: its scene, its
    environment settings."""
    sd = pkg.scenes.glass_sphere(32)
    n_chains, n_mut = 1000, 40
    cfg = config(pkg, no_direct_sampling=0, work_units=n_chains)
    res = []
    monkeypatch.setenv("DRMLT_NO_BOX_MERGE", "1")
    for thr in (None, "0"):
        if thr is None:
            monkeypatch.delenv("DRMLT_BVH_THRESHOLD", raising=False)
        else:
            monkeypatch.setenv("DRMLT_BVH_THRESHOLD", thr)
        monkeypatch.setenv("DRMLT_VERBOSE", "1")
        capfd.readouterr()
        ctx = pkg.Context(cfg, sd)
        built_bvh = "[drmlt] BVH:" in capfd.readouterr().err
        monkeypatch.delenv("DRMLT_VERBOSE")
        ctx.seed(0xB7)
        ctx.run(n_chains * n_mut)
        res.append((state(ctx), counters(ctx.stats()), ctx.film(), built_bvh))
        ctx.close()
    ((cf, uf), sf, ff, bvh_f), ((cb, ub), sb, fb, bvh_b) = res
    assert not bvh_f and bvh_b
    assert np.array_equal(ub, uf) and np.array_equal(cb["luminance"], cf["luminance"])
    assert sb == sf and sf["accepted"] > 0
    assert lum(fb).sum() == pytest.approx(lum(ff).sum(), rel=1e-5)


def test_veach_weights_deposit_one_per_mutation(pkg, native_lib):
    """kelemen_style_weights=0: (1 - a) on the current list and a on the proposal, each list of unit luminance -- as much per
    mutation as algo=pssmlt over technique=path deposits on the same film (box filter)."""
    sd = pkg.scenes.cornell_c2(32)
    n = N_CHAINS * 40
    per = []
    for tech in ("bdpt", "path"):
        _, ctx = make(pkg, sd, technique=tech, kelemen_style_weights=0)
        ctx.seed(0xABCD)
        ctx.run(n)
        per.append(lum(ctx.film().astype(np.float64)).sum() / n)
        ctx.close()
    print("film luminance per mutation: bdpt %.6f, path %.6f" % tuple(per))
    assert per[0] == pytest.approx(per[1], rel=1e-3)


def test_an_importance_map_switches_to_veach_weights(pkg, native_lib):
    """pssmlt_proc.cpp:205: under an importance map the Kelemen weights are not used. A map of ones changes no list, so the
    chains are those of the run without it and the film is the one Veach's weights give."""
    n = N_CHAINS * 40
    res = []
    for with_map in (True, False):
        _, ctx = make(pkg, kelemen_style_weights=1 if with_map else 0)
        if with_map:
            ctx.set_importance_map(np.ones((32, 32), dtype=np.float32))
        ctx.seed(0xABCD)
        ctx.run(n)
        res.append((state(ctx), counters(ctx.stats()), ctx.film()))
        ctx.close()
    ((cm, um), sm, fm), ((c0, u0), s0, f0) = res
    assert np.array_equal(um.view(np.uint32), u0.view(np.uint32))
    assert sm == s0
    assert lum(fm.astype(np.float64)).sum() == pytest.approx(lum(f0.astype(np.float64)).sum(), rel=1e-5)


def blocks(a):
    return a.reshape(8, 4, 8, 4, 3).mean((1, 3))


def render(pkg, sd, **kw):
    """(b, developed image) of 32 x 32 x 512 mutations over 8192 chains"""
    cfg = config(pkg, work_units=8192, sample_count=512, luminance_samples=200000, **kw)
    ctx = pkg.Context(cfg, sd)
    b = ctx.seed(0x5EED)
    ctx.run(32 * 32 * 512)
    img = ctx.develop()
    ctx.close()
    return b, img


@pytest.fixture(scope="module")
def cornell_reference(pkg, ob, native_lib):
    """tests/test_gpu_bdpt.py::test_direct_sampling_image_matches_the_plain_estimator: independent bdpt samples of the fp64
    oracle, drawn without direct sampling (the oracle is built from an algo=drmlt configuration: it is not asked to run
    pssmlt over bdpt). Beside it the statistic of algo=drmlt over technique=bdpt under the same protocol."""
    sd = pkg.scenes.cornell_c2(32)
    plain = ob.Oracle(pkg.abi, config(pkg, algo=pkg.abi.ALGO_DRMLT, work_units=4, no_direct_sampling=1), sd, 64)
    ref = plain.bdpt_render(32 * 32 * 3000, seed=9, nthreads=8)
    plain.close()
    b, img = render(pkg, sd, algo=pkg.abi.ALGO_DRMLT, no_direct_sampling=0)
    drmlt = (abs(b / lum(ref).mean() - 1), np.abs(blocks(img) - blocks(ref)).mean() / ref.mean())
    return sd, ref, drmlt


@pytest.mark.parametrize("kw", [dict(), dict(kelemen_style_weights=0), dict(kelemen_style_mutation=0), dict(no_direct_sampling=1)],
                         ids=["kelemen-weights", "veach-weights", "gaussian-mutation", "no-direct-sampling"])
def test_image_matches_the_bdpt_estimator(pkg, native_lib, cornell_reference, kw):
    sd, ref, drmlt = cornell_reference
    b, img = render(pkg, sd, **kw)
    err = np.abs(blocks(img) - blocks(ref)).mean() / ref.mean()
    print("pssmlt/bdpt %s: b off by %.4f, block error %.4f, mean(develop) / b - 1 = %.2g | drmlt/bdpt (direct sampling): b off by %.4f, block error %.4f" % (
        kw, abs(b / lum(ref).mean() - 1), err, lum(img).mean() / b - 1, drmlt[0], drmlt[1]))
    assert b == pytest.approx(lum(ref).mean(), rel=0.02)
    assert err < 0.04
    assert lum(img).mean() == pytest.approx(b, rel=1e-3)


def test_image_with_light_image_splats_and_specular_chains(pkg, ob, native_lib):
    """tests/test_gpu_bdpt.py::test_bdpt_image_and_acceptance_map's scene, protocol and bounds."""
    sd = pkg.scenes.glass_sphere(32)
    orc = ob.Oracle(pkg.abi, config(pkg, algo=pkg.abi.ALGO_DRMLT, work_units=4, no_direct_sampling=1), sd, 64)
    ref = orc.bdpt_render(32 * 32 * 3000, seed=9, nthreads=8)
    orc.close()
    b, img = render(pkg, sd, no_direct_sampling=1)
    err = np.abs(blocks(img) - blocks(ref)).mean() / ref.mean()
    print("glass sphere: b off by %.4f, block error %.4f" % (abs(b / lum(ref).mean() - 1), err))
    assert b == pytest.approx(lum(ref).mean(), rel=0.02)
    assert err < 0.04


def test_single_device_node_is_the_plain_context(pkg, native_lib):
    """tests/test_gpu_node.py's test of the same name, for this combination."""
    sd = pkg.scenes.cornell_c2(32)
    kw = dict(rr_depth=5, sample_count=4, luminance_samples=1000)
    node, ctx = pkg.Node(config(pkg, **kw), sd, device_mask=1), pkg.Context(config(pkg, **kw), sd)
    assert node.seed(3) == ctx.seed_pool(3, 0, N_CHAINS)
    node.run(32 * 32 * 4); ctx.run(32 * 32 * 4)
    np.testing.assert_allclose(node.develop(), ctx.develop(), rtol=2e-4, atol=1e-6)
    assert node.stats().mutations == ctx.stats().mutations == 32 * 32 * 4
    node.close(); ctx.close()
