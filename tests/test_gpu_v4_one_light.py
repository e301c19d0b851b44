"""k_mutate_v4's one-light builds (kernels_v4.hip: V4_ONE_LIGHT_BUILD) read the scene's one emitter and its shape's shading record
from the parameter block instead of the staged tables: launch_mutate runs them in place of V4_F0 / V4_F0_STAMPS when
scene_has_one_light(P) holds (device_types.h). The records are byte copies and every expression of the step is the same source
expression, so a context forced onto the generic build (DRMLT_ONE_LIGHT_GENERIC=1) and a default one must run the same chains, bit
for bit: states, f(u) of the current states, every counter of stats().

Films are sums of non-negative float32 terms added by atomics in an order that differs from run to run; reordering n such terms
moves a sum by at most (n - 1) * 2^-24 of its value. A pixel of the 32 x 32 films here receives far fewer than 160 filter taps
(6144 mutations, at most two splats each, over 1024 pixels), hence rtol = 160 * 2^-24 = 1e-5; atol covers flushed denormals
(tests/test_gpu_v4_rule_builds.py: the same shapes, the same bound).

Which build ran is read from the device: every wave of a one-light build counts itself in stats[15], printed by drmlt_stats_get
under DRMLT_VERBOSE."""
import os
import re

import numpy as np
import pytest

from test_scene_prep_one_light import two_lights

pytestmark = pytest.mark.gpu
DIM = 34  # consumable PSS dimensions at max_depth 8
N_CHAINS, N_MUT = 96, 64  # three waves of 32 chains
COUNTERS = ("first_acc", "first_base", "large_acc", "large_base", "bold_acc", "bold_base", "second_acc", "second_base",
            "second_large_acc", "second_large_base", "second_bold_acc", "second_bold_base", "overall_acc", "overall_base",
            "mutations", "path_evals", "rays", "accepted")


def make_scene(pkg, scene):
    return two_lights(pkg.scenes, 32) if scene == "two_lights" else getattr(pkg.scenes, scene)(32)


def run_chains(pkg, capfd, scene, calls, generic, n_chains=N_CHAINS, **cfg_kw):
    env = {"DRMLT_KERNEL": "4", "DRMLT_VERBOSE": "1"}
    if generic:
        env["DRMLT_ONE_LIGHT_GENERIC"] = "1"
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        base = dict(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1)
        base.update(cfg_kw)
        ctx = pkg.Context(pkg.abi.make_config(**base), make_scene(pkg, scene))
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
    m = re.search(r"waves through a one-light build: (\d+)", log)
    assert m, log
    out = dict(state=ctx.chain_state(DIM), stats=st, image=ctx.develop(), one_light_waves=int(m.group(1)), log=log)
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
    assert forced["one_light_waves"] == 0, "DRMLT_ONE_LIGHT_GENERIC=1 must keep the context on the generic build"


def pair(pkg, capfd, scene, calls, **kw):
    return run_chains(pkg, capfd, scene, calls, False, **kw), run_chains(pkg, capfd, scene, calls, True, **kw)


def assert_eventful(st):
    """second stages, large steps, accepted and rejected mutations all occurred: otherwise the comparison shows nothing"""
    assert st.second_base > 0 and st.large_base > 0 and st.bold_base > 0
    assert 0 < st.first_acc < st.first_base and st.accepted > 0


def test_orbital_headline_twin(pkg, native_lib, capfd):
    """cornell_c2 under the orbital rule: the build bench.py's flagship line runs."""
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], type="orbital")
    assert d["one_light_waves"] == 3, "one launch of three waves on the one-light build"
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


def test_generic_rule_twin(pkg, native_lib, capfd):
    d, g = pair(pkg, capfd, "cornell_c2", [N_MUT], type="green")
    assert d["one_light_waves"] == 3
    assert d["stats"].second_base > 0 and d["stats"].accepted > 0
    assert_same(d, g, N_CHAINS * N_MUT)


def test_run_ahead_with_timid_after_large(pkg, native_lib, capfd):
    """Two calls in launches of 16: run-ahead between the launches and prologues that reload the state."""
    os.environ["DRMLT_SLICE"] = "16"
    try:
        d, g = pair(pkg, capfd, "cornell_c2", [N_MUT // 2, N_MUT // 2], type="orbital", timid_after_large=1)
    finally:
        del os.environ["DRMLT_SLICE"]
    assert d["one_light_waves"] >= 3 and d["one_light_waves"] % 3 == 0  # whole launches of three waves
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * N_MUT)


@pytest.mark.parametrize("scene", ["two_lights", "cornell_point", "door_c3"])
def test_other_scenes_run_the_generic_build(pkg, native_lib, capfd, scene):
    """two lights (V4_F0, a light pick that picks), a point light (V4_F7), a rough conductor (V4_F3): not one-light scenes"""
    d, g = pair(pkg, capfd, scene, [N_MUT], type="orbital")
    assert d["one_light_waves"] == 0, "scene_has_one_light accepted a scene the one-light build does not implement"
    assert d["stats"].accepted > 0
    assert_same(d, g, N_CHAINS * N_MUT)
