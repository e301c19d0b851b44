"""k_mutate_w2 (kernels_v4.hip) is k_mutate_v4's orbital one-light twin compiled for two waves per SIMD: launch_mutate runs it in
place of the twin on V4_F0 launches that cannot have a third wave on a SIMD (launch_plan.h: w2_launch; the 96- and 80-chain
grids here are such launches on any device). Its constants wait in vector registers and a fill item draws one Philox block,
but every floating-point expression is a header routine it shares with the
twin, applied to the same values: a default context and one created under DRMLT_NO_W2=1 must run the same chains, bit for bit --
states, f(u) of the current states, every counter of stats().

Films: the reordering bound of tests/test_gpu_v4_one_light.py for these shapes (32 x 32 pixels, 6144 mutations, at most two
splats each: rtol = 160 * 2^-24 = 1e-5, atol for flushed denormals).

Which kernel ran is read from the device: every wave of k_mutate_w2 counts itself in stats[16], printed by drmlt_stats_get
under DRMLT_VERBOSE."""
import os
import re

import numpy as np
import pytest

from test_scene_prep_one_light import two_lights

pytestmark = pytest.mark.gpu
DIM = 34  # consumable PSS dimensions at max_depth 8 (shorter states are padded with zeros)
N_CHAINS, N_MUT = 96, 64  # three waves of 32 chains
COUNTERS = ("first_acc", "first_base", "large_acc", "large_base", "bold_acc", "bold_base", "second_acc", "second_base",
            "second_large_acc", "second_large_base", "second_bold_acc", "second_bold_base", "overall_acc", "overall_base",
            "mutations", "path_evals", "rays", "accepted")


def make_scene(pkg, scene):
    return two_lights(pkg.scenes, 32) if scene == "two_lights" else getattr(pkg.scenes, scene)(32)


def run_chains(pkg, capfd, scene, calls, no_w2, n_chains=N_CHAINS, env=None, **cfg_kw):
    env = dict(env or {}, DRMLT_KERNEL="4", DRMLT_VERBOSE="1")
    if no_w2:
        env["DRMLT_NO_W2"] = "1"
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        base = dict(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1)
        base.update(cfg_kw)
        cfg = pkg.abi.make_config(**base)
        ctx = pkg.Context(cfg, make_scene(pkg, scene))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    ctx.seed(0x40E5)
    for n_mut in calls:
        ctx.run(n_chains * n_mut)
    capfd.readouterr()
    st = ctx.stats()
    log = capfd.readouterr().err
    m = re.search(r"waves through k_mutate_w2: (\d+)", log)
    assert m, log
    out = dict(state=ctx.chain_state(DIM), stats=st, image=ctx.develop(), w2_waves=int(m.group(1)), log=log)
    ctx.close()
    return out


def assert_same(default, forced, mutations):
    (ca, ua), (cb, ub) = default["state"], forced["state"]
    sa, sb = default["stats"], forced["stats"]
    for k in COUNTERS:
        print(k, getattr(sa, k), getattr(sb, k))
    assert sa.mutations == sb.mutations == mutations
    assert np.array_equal(ua, ub)                                   # P.x
    for f in ("luminance", "x", "y", "rgb"):                        # cur_*
        assert np.array_equal(ca[f], cb[f]), f
    for k in COUNTERS:
        assert getattr(sa, k) == getattr(sb, k), k
    err = np.abs(default["image"] - forced["image"])
    print("image: max abs difference", err.max(), "max", forced["image"].max())
    np.testing.assert_allclose(default["image"], forced["image"], rtol=1e-5, atol=1e-7)
    assert forced["w2_waves"] == 0, "DRMLT_NO_W2=1 must keep the context on k_mutate_v4"


def pair(pkg, capfd, scene, calls, **kw):
    return run_chains(pkg, capfd, scene, calls, False, **kw), run_chains(pkg, capfd, scene, calls, True, **kw)


def assert_eventful(st):
    """second stages, large steps, accepted and rejected mutations all occurred: otherwise the comparison shows nothing"""
    assert st.second_base > 0 and st.large_base > 0 and st.bold_base > 0
    assert 0 < st.first_acc < st.first_base and st.accepted > 0


def test_three_full_waves(pkg, native_lib, capfd):
    """cornell_c2 under the orbital rule: what bench.py's flagship line runs"""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], type="orbital")
    assert d["w2_waves"] == 3, "one launch of three waves"
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


def test_last_wave_half_empty(pkg, native_lib, capfd):
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], n_chains=80, type="orbital")
    assert d["w2_waves"] == 3
    assert_eventful(d["stats"])
    assert_same(d, g, 80 * N_MUT)


def test_run_ahead_and_state_reload(pkg, native_lib, capfd):
    """Two calls in launches of 16: run-ahead between the launches and prologues that reload the state."""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT // 2, N_MUT // 2], env={"DRMLT_SLICE": "16"}, type="orbital")
    # two calls of 32 mutations per chain in slices of 16: four launches of three waves (drmlt_run issues one launch per slice
    # whatever the chains ran ahead) -- six would mean the slicing, and with it run-ahead and the state reload, did not happen
    assert d["w2_waves"] == 12
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


def test_second_stage_large_steps(pkg, native_lib, capfd):
    """timid_after_large: a rejected large step gets a second stage, filled by the uniform arm of fill_second"""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], type="orbital", timid_after_large=1)
    assert d["w2_waves"] == 3
    assert_eventful(d["stats"])
    assert d["stats"].second_large_base > 0
    assert_same(d, g, N_CHAINS * N_MUT)


@pytest.mark.parametrize("batch", [1, 32])
def test_fill_passes(pkg, native_lib, capfd, batch):
    """DRMLT_MH_BATCH=1: one chain per fill, a single pass holds its proposal items and its coin item together; 32: every chain of
    the wave fills at once and every pass but the last is full"""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], env={"DRMLT_MH_BATCH": str(batch)}, type="orbital")
    assert d["w2_waves"] == 3
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


def test_padding_rows(pkg, native_lib, capfd):
    """max_depth 3: 10 dimensions, not a multiple of 4 -- the last Philox block of a proposal fills two padding rows"""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], type="orbital", max_depth=3)
    assert d["w2_waves"] == 3
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


@pytest.mark.parametrize("scene,rule", [("cornell_c2", "green"), ("two_lights", "orbital"), ("door_c3", "orbital")])
def test_other_launches_run_no_wave_of_it(pkg, native_lib, capfd, scene, rule):
    """Green's rule, two lights (V4_F0's generic step), a rough conductor (V4_F3): not what k_mutate_w2 implements"""
    d, g = pair(pkg, capfd, scene, [N_MUT], type=rule)
    assert d["w2_waves"] == 0
    assert d["stats"].accepted > 0
    assert_same(d, g, N_CHAINS * N_MUT)
