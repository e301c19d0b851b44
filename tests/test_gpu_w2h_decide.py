"""k_mutate_w2h's bookkeeping branch decides by selects (kernels_v4.hip: w2h_decide) and its step runs the emitter-hit block only in
an iteration in which a bounce ray of the wave hit the light (device_path.h: path_step_diffuse<.., RARE_EMITTER_HIT = true>).
k_mutate_w2 and k_mutate_v4's twin keep the state machine with its arms (mh_decide) and the unconditional block, so the three
contexts of tests/test_gpu_w2h.py -- default (held), DRMLT_NO_W2_HELD=1, DRMLT_NO_W2=1 -- compare the two forms: the same chains
BIT FOR BIT (states, cur_*, every counter of stats()), films under test_gpu_w2.assert_same's reordering bound.

The cases steer the decide -- second stages after large steps, one chain or every chain of a wave per call, a half-empty wave,
launches that open with nothing evaluated and run ahead, an importance map (the one arm that stays behind a wave-uniform
branch) -- and the step: a light that most bounce rays hit, paths without a bounce ray, roulette from the first vertex."""
import os
import re

import numpy as np
import pytest

import test_gpu_w2 as w2
from test_gpu_w2 import DIM, N_CHAINS, N_MUT, assert_eventful, assert_same
from test_gpu_w2h import check, held_waves, three

gpu = pytest.mark.gpu


def wide_light_room(scenes, res=32):
    """test_gpu_w2h.one_box_room with the light scaled to 0.9: most of the ceiling, most bounce rays that go up hit it"""
    sd = scenes.SceneData("wide_light_room")
    white, red, green, black = sd.diffuse(0.725, 0.71, 0.68), sd.diffuse(0.63, 0.065, 0.05), sd.diffuse(0.14, 0.45, 0.091), sd.diffuse(0.0)
    scenes._room(sd, white, red, green)
    sd.rectangle(scenes.translate(0, 0.995, 0) @ scenes.rotate("x", 90) @ scenes.scale(0.9), black, radiance=(17.0, 12.0, 4.0))
    sd.set_camera(scenes.lookat((0, 0, 3.9), (0, 0, 0), (0, 1, 0)), 39.3077, res, res, scenes.abi.FILTER_BOX, 0.5)
    return sd


_stock_make_scene = w2.make_scene


@pytest.fixture(autouse=True)
def built_scenes(monkeypatch):
    """test_gpu_w2.run_chains makes its scene by name"""
    monkeypatch.setattr(w2, "make_scene", lambda pkg, scene: wide_light_room(pkg.scenes, 32) if scene == "wide_light_room" else _stock_make_scene(pkg, scene))


def assert_stages(st):
    """the short runs: at least second stages and large steps occurred"""
    assert st.second_base > 0 and st.large_base > 0 and st.accepted > 0


@gpu
def test_second_stages_after_large_steps(pkg, native_lib, capfd):
    """timid_after_large: do_second = !acc1 && (timid || !large) takes its first operand on large steps too"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], timid_after_large=1)
    check(h, s, t, 3, N_CHAINS * N_MUT)
    assert h["stats"].second_large_base > 0


@gpu
@pytest.mark.parametrize("batch", [1, 32])
def test_one_chain_and_every_chain_per_call(pkg, native_lib, capfd, batch):
    """DRMLT_MH_BATCH=1: one parked lane decides, 63 lanes compute and keep what they had; 32: every chain lane is parked"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], env={"DRMLT_MH_BATCH": str(batch)})
    check(h, s, t, 3, N_CHAINS * N_MUT)


@gpu
def test_last_wave_half_empty(pkg, native_lib, capfd):
    """80 chains: sixteen chain lanes of the last wave own no chain and never park"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], n_chains=80)
    check(h, s, t, 3, 80 * N_MUT)


@gpu
def test_launches_open_with_nothing_evaluated(pkg, native_lib, capfd):
    """two calls under DRMLT_SLICE=16: four launches, each opens with cs.stage < 0 on every chain (no counter, weight or cs.it
    may move there), and chains run ahead between them"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT // 2, N_MUT // 2], env={"DRMLT_SLICE": "16"})
    check(h, s, t, 12, N_CHAINS * N_MUT)


def run_chains_with_map(pkg, capfd, scene, calls, env, n_chains=N_CHAINS, **cfg_kw):
    """test_gpu_w2.run_chains with an importance map set before the seeds are drawn"""
    env = dict(env, DRMLT_KERNEL="4", DRMLT_VERBOSE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        base = dict(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1, type="orbital")
        base.update(cfg_kw)
        ctx = pkg.Context(pkg.abi.make_config(**base), w2.make_scene(pkg, scene))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    yy, xx = np.mgrid[0:32, 0:32]
    ctx.set_importance_map((0.25 + ((3 * xx + 5 * yy) % 17) / 8.0).astype(np.float32))  # fixed, positive, not flat
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


@gpu
def test_importance_map(pkg, native_lib, capfd):
    """two-stage MLT: the splat is divided by the map at its pixel before it is normalised -- the arm of the decide that stays
    behind a (wave-uniform) branch, where only lanes with an evaluation read the map"""
    h = run_chains_with_map(pkg, capfd, "cornell_c2", [N_MUT], {})
    s = run_chains_with_map(pkg, capfd, "cornell_c2", [N_MUT], {"DRMLT_NO_W2_HELD": "1"})
    t = run_chains_with_map(pkg, capfd, "cornell_c2", [N_MUT], {"DRMLT_NO_W2": "1"})
    check(h, s, t, 3, N_CHAINS * N_MUT)


@gpu
def test_a_light_that_most_bounce_rays_hit(pkg, native_lib, capfd):
    """the light is most of the ceiling: the emitter-hit block runs in nearly every iteration"""
    h, s, t = three(pkg, capfd, "wide_light_room", [N_MUT])
    check(h, s, t, 3, N_CHAINS * N_MUT)


@gpu
@pytest.mark.parametrize("kw", [dict(max_depth=2), dict(rr_depth=1)], ids=["max_depth_2", "rr_depth_1"])
def test_short_paths(pkg, native_lib, capfd, kw):
    """max_depth 2: no bounce ray exists, the emitter-hit block never runs; rr_depth 1: roulette from the first vertex on"""
    h, s, t = three(pkg, capfd, "cornell_c2", [N_MUT], **kw)
    check(h, s, t, 3, N_CHAINS * N_MUT, eventful=False)
    assert_stages(h["stats"])
    assert h["stats"].rays > 0
