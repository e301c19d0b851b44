"""k_mutate_v4 adopts a proposal by exchanging the roles of two of the chain's LDS row groups (RowSampler, device_sampler.h): no
commit pass, the current state is kept unwrapped and wrapped where it is read. The chains must stay those of k_mutate_v3, which
commits with an explicit wrapped copy -- bit for bit: states, f(u) of the current state, mutation and acceptance counts."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DIM = 34  # consumable PSS dimensions at max_depth 8: D4 - D = 2 padding rows per group
COUNTS = ("first", "large", "bold", "second", "second_large", "second_bold", "overall")


def ctx_with_env(pkg, cfg, sd, **env):
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


def config(pkg, n_chains, **kw):
    base = dict(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1)
    base.update(kw)
    return pkg.abi.make_config(**base)


def run_chains(pkg, cfg, sd, n_chains, calls, **env):
    ctx = ctx_with_env(pkg, cfg, sd, **env)
    ctx.seed(0x40E5)
    for n_mut in calls:
        ctx.run(n_chains * n_mut)
    out = ctx.chain_state(DIM), ctx.stats()
    ctx.close()
    return out


def assert_same_chains(a, b, mutations):
    ((ca, ua), sa), ((cb, ub), sb) = a, b
    assert sa.mutations == sb.mutations == mutations
    assert np.array_equal(ua, ub)                                   # P.x
    for f in ("luminance", "x", "y", "rgb"):                        # cur_*
        assert np.array_equal(ca[f], cb[f]), f
    for k in COUNTS:
        assert getattr(sa, k + "_base") == getattr(sb, k + "_base") and getattr(sa, k + "_acc") == getattr(sb, k + "_acc"), k
    assert sa.accepted == sb.accepted and sa.rays == sb.rays


@pytest.mark.parametrize("n_chains", [33, 64, 96], ids=["partial-wave", "two-waves", "three-waves"])
@pytest.mark.parametrize("typ", ["orbital", "green", "mira"])  # green: the reverse move reads x; mira: its ratio reads x, y and z
def test_v4_runs_the_chains_of_v3(pkg, native_lib, typ, n_chains):
    sd = pkg.scenes.SCENES["cornell_c2"](res=32)
    cfg = config(pkg, n_chains, type=typ)
    v3 = run_chains(pkg, cfg, sd, n_chains, [200], DRMLT_KERNEL=3)
    v4 = run_chains(pkg, cfg, sd, n_chains, [200], DRMLT_KERNEL=4)
    assert_same_chains(v4, v3, n_chains * 200)


def test_roles_start_afresh_with_every_launch(pkg, native_lib):
    """One call of 2N mutations against two calls of N, in launches of 16: whichever group holds x when a launch ends, the state
    that leaves the kernel is the wrapped one, and the next launch finds it in the first group."""
    sd = pkg.scenes.SCENES["cornell_c2"](res=32)
    n_chains, n = 96, 64
    cfg = config(pkg, n_chains, type="orbital")
    one = run_chains(pkg, cfg, sd, n_chains, [2 * n], DRMLT_KERNEL=4, DRMLT_SLICE=16)
    two = run_chains(pkg, cfg, sd, n_chains, [n, n], DRMLT_KERNEL=4, DRMLT_SLICE=16)
    assert_same_chains(two, one, n_chains * 2 * n)
    u = two[0][1]
    assert (u >= 0).all() and (u < 1).all()


def test_adopting_the_second_stage_proposal(pkg, native_lib):
    """The x <-> z exchange, on the glossy door scene (the V4_F3 build)."""
    sd = pkg.scenes.SCENES["door_c3"](res=32)
    n_chains, n_mut = 64, 200
    cfg = config(pkg, n_chains, type="orbital")
    v3 = run_chains(pkg, cfg, sd, n_chains, [n_mut], DRMLT_KERNEL=3)
    v4 = run_chains(pkg, cfg, sd, n_chains, [n_mut], DRMLT_KERNEL=4)
    assert v4[1].second_acc >= 1, "no second-stage proposal was accepted: nothing exchanged x and z"
    assert_same_chains(v4, v3, n_chains * n_mut)
