"""What the Mitsuba plugin adaptor hands over for scenes with point lights and a constant environment, run on the device: the
scene it marshals renders exactly as the scenes.py scene it was built from, and directPass=device renders the direct image on
the GPU. The scenes are captured by tests/native/adaptor_emitters_harness.cpp -DMOCK_ABI (no GPU needed for that step) and
loaded with SceneData.load; the end-to-end run links the harness with libdrmlt_amd.so."""
import os
import subprocess

import numpy as np
import pytest

from test_adaptor_emitters import BASE, D, SCENES, run, scene_a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
RES, CHAINS = 32, 64
DIRECT_SEED_XOR = 0xD12EC7          # mitsuba_adaptor.cpp: the direct pass's seed is the render's seed ^ this


def lum(img):
    return img @ np.array([0.212671, 0.715160, 0.072169], dtype=np.float32)


@pytest.fixture(scope="module")
def captured(pkg, tmp_path_factory):
    """{name: (the scenes.py scene, the scene loaded from what the adaptor handed to drmlt_node_create)} for (a), (b), (c)"""
    subprocess.run(["make", "-C", HOST, "adaptor_emitters_harness_mock"], check=True, capture_output=True)
    d = tmp_path_factory.mktemp("captured")
    out = {}
    for name, make in SCENES.items():
        sd = make(pkg.scenes, RES)
        path, prefix = str(d / (name + ".bin")), str(d / name)
        sd.save(path)
        rc, log = run(os.path.join(HOST, "adaptor_emitters_harness_mock"), path, prefix, *D(**dict(BASE, workUnits=CHAINS)))
        assert rc == 0, log
        out[name] = (sd, pkg.scenes.SceneData.load(prefix + ".scene"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_marshalled_scene_evaluates_paths_bit_for_bit(pkg, native_lib, captured, name):
    """f(u) on 4096 primary-sample points: the same library on the scene the adaptor marshalled and on the scenes.py scene. Any
    difference is a marshalling error."""
    sd, got = captured[name]
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, work_units=CHAINS, luminance_samples=20000)
    u = np.random.default_rng(11).random((4096, 64), dtype=np.float32)
    with pkg.Context(cfg, sd) as want_ctx:
        want = want_ctx.eval_paths(u)
    with pkg.Context(cfg, got) as got_ctx:
        have = got_ctx.eval_paths(u)
    assert (want["luminance"] > 0).mean() > 0.1            # the points do reach the lights
    for field in want.dtype.names:
        assert np.array_equal(have[field], want[field]), field


@pytest.mark.gpu
def test_marshalled_scene_runs_the_same_chains(pkg, native_lib, captured):
    """(a): 1024 chains x 40 mutations from one seed -- the same chain states, proposals' counters and film."""
    sd, got = captured["a_quad_and_point"]
    n_chains, n_mut = 1024, 40
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1)
    results = []
    for scene in (sd, got):
        with pkg.Context(cfg, scene) as ctx:
            b = ctx.seed(0x77)
            ctx.run(n_chains * n_mut)
            results.append((b, ctx.chain_state(34), ctx.stats(), ctx.film()))
    (b0, (c0, u0), s0, f0), (b1, (c1, u1), s1, f1) = results
    assert s0.mutations == n_chains * n_mut and s0.accepted > 0
    assert b1 == b0 and np.array_equal(u1, u0)
    for field in c0.dtype.names:
        assert np.array_equal(c1[field], c0[field]), field
    for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
        assert getattr(s1, k + "_base") == getattr(s0, k + "_base") and getattr(s1, k + "_acc") == getattr(s0, k + "_acc"), k
    assert (s1.rays, s1.path_evals, s1.accepted, s1.mutations) == (s0.rays, s0.path_evals, s0.accepted, s0.mutations)
    assert lum(f1).sum() == pytest.approx(lum(f0).sum(), rel=1e-5)         # atomics: the order of the adds is not fixed


@pytest.mark.gpu
def test_direct_pass_on_the_device_end_to_end(pkg, native_lib, tmp_path):
    """Scene (a) through the plugin surface on the real library, directSamples=4, 16 mutations per pixel, 64 chains. With
    directPass=device the image is finite and its mean luminance is within 2 % (the bound test_point_lit_mlt_image_is_unbiased
    puts on b) of the directPass-less render -- whose direct image is the fake host pass's constant 0.25, taken off again --
    plus Context.render_direct(4) added in Python.

    Measured on an MI355X: mean luminance 0.524334 for both (the direct part is 0.342958 of it), relative difference 0, largest
    difference of any pixel value 4.8e-7. The chains repeat under one seed and the direct image is a function of its arguments
    alone, so what the bound has to absorb is rounding only."""
    subprocess.run(["make", "-C", HOST, "adaptor_emitters_harness"], check=True, capture_output=True)
    exe = os.path.join(HOST, "adaptor_emitters_harness")
    sd = scene_a(pkg.scenes, RES)
    path = str(tmp_path / "a.bin")
    sd.save(path)
    seed = 4242
    props = dict(technique="path", type="orbital", maxDepth=8, directSamples=4, sampleCount=16, workUnits=CHAINS, luminanceSamples=20000,
                 seed=seed, device=0)
    rc, log = run(exe, path, str(tmp_path / "dev"), *D(directPass="device", **props))
    assert rc == 0 and any("render returned true, 1 refresh signal(s), 0 direct pass sample(s)" in t for _, t in log), log
    dev = np.fromfile(str(tmp_path / "dev.img"), dtype=np.float32).reshape(RES, RES, 3)
    rc, log = run(exe, path, str(tmp_path / "host"), *D(**props))
    assert rc == 0 and any("render returned true, 1 refresh signal(s), 4 direct pass sample(s)" in t for _, t in log), log
    host = np.fromfile(str(tmp_path / "host.img"), dtype=np.float32).reshape(RES, RES, 3)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, direct_samples=4, work_units=CHAINS, luminance_samples=20000, sample_count=16)
    with pkg.Context(cfg, sd) as ctx:
        direct = ctx.render_direct(4, seed=seed ^ DIRECT_SEED_XOR)
    composed = host - np.float32(0.25) + direct
    diff = abs(lum(dev).mean() - lum(composed).mean()) / lum(composed).mean()
    print("directPass=device: mean luminance %.6f, composed %.6f (direct part %.6f), relative difference %.3g, max |pixel difference| %.3g"
          % (lum(dev).mean(), lum(composed).mean(), lum(direct).mean(), diff, np.abs(dev - composed).max()))
    assert np.all(np.isfinite(dev)) and dev.min() >= 0
    assert lum(direct).mean() > 0.05 * lum(composed).mean()                # the direct image is a real part of the picture
    assert diff < 0.02
