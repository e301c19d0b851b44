"""k_mutate_w2's film flush under a TABULATED filter (kernels_v4.hip: w2_flush stages P.filter_lut in the wave's list area and the
footprint loops read it from LDS; the box cases are those of tests/test_gpu_w2.py and tests/test_gpu_w2_step.py). A default
context against one created under DRMLT_NO_W2=1 (k_mutate_v4, whose flush reads the table from device memory), on the shapes of
tests/test_gpu_w2.py: a 32 x 32 film, 96 chains, cornell_c2 with a Gaussian filter of radius 2 -- up to 4 x 4 adds per channel
and splat, footprints clipped at all four film borders.

States, current splats and every counter: bit-equal, as in test_gpu_w2.assert_same. Films: the two kernels add the same terms in
another order (another occupancy, another interleaving of the waves), so they agree within rtol = N * 2^-24 with N the run's
WHOLE tap count -- 2 splats x 16 taps per mutation, the worst case of one pixel receiving all of them; re-ordered float adds of
positive terms stay inside that by construction. A wrong table entry, a stale staging area or a dropped pass moves pixels by
percent. atol = 1e-7 covers flushed denormals."""
import numpy as np
import pytest

import test_gpu_w2 as w2

pytestmark = pytest.mark.gpu
SPLATS, TAPS = 2, 16


@pytest.fixture(autouse=True)
def gaussian_scene(monkeypatch):
    def make_scene(pkg, scene):
        assert scene == "cornell_c2_gaussian"
        return pkg.scenes.cornell_c2(32, filt=pkg.abi.FILTER_GAUSSIAN)
    monkeypatch.setattr(w2, "make_scene", make_scene)


def assert_same_gaussian(default, forced, n_chains, n_mut):
    (ca, ua), (cb, ub) = default["state"], forced["state"]
    sa, sb = default["stats"], forced["stats"]
    for k in w2.COUNTERS:
        print(k, getattr(sa, k), getattr(sb, k))
    assert sa.mutations == sb.mutations == n_chains * n_mut
    assert np.array_equal(ua, ub)
    for f in ("luminance", "x", "y", "rgb"):
        assert np.array_equal(ca[f], cb[f]), f
    for k in w2.COUNTERS:
        assert getattr(sa, k) == getattr(sb, k), k
    rtol = SPLATS * TAPS * n_chains * n_mut * 2.0 ** -24
    a, b = default["image"], forced["image"]
    err = np.abs(a - b)
    print("image: max abs difference", err.max(), "max rel", (err / np.maximum(np.abs(b), 1e-30)).max(), "max", b.max(), "rtol", rtol)
    assert b.max() > 0, "an empty film compares nothing"
    np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-7)
    assert forced["w2_waves"] == 0, "DRMLT_NO_W2=1 must keep the context on k_mutate_v4"


def test_many_passes(pkg, native_lib, capfd):
    """every chain of a wave digests at once: about 560 queue entries per wave, several in-loop flushes of five and more passes"""
    n_mut = 16
    d, g = w2.pair(pkg, capfd, "cornell_c2_gaussian", [n_mut], env={"DRMLT_MH_BATCH": "32"}, type="orbital")
    assert d["w2_waves"] == 3
    w2.assert_eventful(d["stats"])
    assert_same_gaussian(d, g, w2.N_CHAINS, n_mut)


def test_batch_of_one(pkg, native_lib, capfd):
    """one chain per bookkeeping call: a flush fires with 97 or 98 entries, its last pass nearly empty"""
    n_mut = 16
    d, g = w2.pair(pkg, capfd, "cornell_c2_gaussian", [n_mut], env={"DRMLT_MH_BATCH": "1"}, type="orbital")
    assert d["w2_waves"] == 3
    w2.assert_eventful(d["stats"])
    assert_same_gaussian(d, g, w2.N_CHAINS, n_mut)


def test_half_empty_last_wave_in_two_launches(pkg, native_lib, capfd):
    """80 chains, two launches of 16 mutations per chain: the epilogue's two flushes stage the table in waves whose fills have
    overwritten it, one of them half empty"""
    n_mut = 32
    d, g = w2.pair(pkg, capfd, "cornell_c2_gaussian", [n_mut], n_chains=80, env={"DRMLT_SLICE": "16"}, type="orbital")
    assert d["w2_waves"] == 6, "two launches of three waves"
    w2.assert_eventful(d["stats"])
    assert_same_gaussian(d, g, 80, n_mut)
