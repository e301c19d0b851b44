"""k_mutate_w2's step writes the vertex, the bounce, ps.nee and the shadow ray on every lane that steps and selects only what
a path that has ended is still read for (path_step_diffuse<.., MASKED = false>, device_path.h), and its shadow ray reaches the
helper lanes in one v_permlane32_swap per value (lower_keeps, kernels_v4.hip). When any lane has a ray the whole wave runs the ray
pass, so a lane without one overwrites its hit with what a garbage ray finds. None of this changes a floating-point expression, so
a default context and one created under DRMLT_NO_W2=1 (k_mutate_v4's twin, masked copy-backs and copied hand-off) must
still run the same chains bit for bit: states, f(u) of the current states, every counter of stats() -- tests/test_gpu_w2.py's
pair() and assert_same(), on the cases where an unconditionally written field could be read by mistake:

  max_depth 1, 2   every path ends AT the depth bound: at 2 the first vertex hands over a shadow ray and bounces, the second
                   ends with that ray pending (PH_FLUSH reads ps.nee after a step that wrote garbage over the vertex); at 1
                   the first vertex already ends and no path carries light (see test_depth_bound_one)
  rr_depth 1       roulette from the first bounce: paths end with thr already divided by the survival probability
  cornell_c1       three quads (an odd count of flat records, no boxes); most camera rays miss and end in their first step
  48 chains        the second wave's upper 16 chain lanes are idle: they never step and keep what the prologue wrote
  MH batch 1, 32   the bookkeeping branch runs for one parked chain at a time / for the whole wave at once
  DRMLT_SLICE=16   two launches: the state written by the epilogue is what the next prologue reloads

At most 48 chains and 64 mutations each."""
import pytest

from test_gpu_w2 import N_MUT, assert_eventful, assert_same, pair

pytestmark = pytest.mark.gpu
N_CHAINS = 48  # one full wave of 32 chains and one half-empty wave


def check(pkg, capfd, scene, calls, waves, **kw):
    d, g = pair(pkg, capfd, scene, calls, n_chains=N_CHAINS, type="orbital", **kw)
    assert d["w2_waves"] == waves, "the default context must run k_mutate_w2"
    assert_eventful(d["stats"])
    assert_same(d, g, N_CHAINS * sum(calls))
    return d


def test_depth_bound_two(pkg, native_lib, capfd):
    d = check(pkg, capfd, "cornell_c2", [N_MUT], 2, max_depth=2)
    # two rays at the most: the camera ray and the first vertex's shadow ray or bounce ray or both
    assert d["stats"].rays <= 3 * d["stats"].path_evals


def test_depth_bound_one(pkg, native_lib, monkeypatch):
    """max_depth 1 ends every path at its first vertex, before any light is sampled or hit by a bounce: f(u) = 0 everywhere.
    Seeding refuses such a scene (no chain can start from zero luminance), identically for both kernels -- the chain loop
    does not run at all, which is the most this depth bound can show."""
    cfg = pkg.abi.make_config(type="orbital", max_depth=1, direct_samples=-1, luminance_samples=2000, work_units=N_CHAINS, sample_count=1)
    for no_w2 in (False, True):
        monkeypatch.setenv("DRMLT_KERNEL", "4")
        if no_w2:
            monkeypatch.setenv("DRMLT_NO_W2", "1")
        ctx = pkg.Context(cfg, pkg.scenes.cornell_c2(32))
        with pytest.raises(pkg.DrmltError, match="luminance appears to be zero"):
            ctx.seed(0x40E5)
        ctx.close()


def test_roulette_from_the_first_bounce(pkg, native_lib, capfd):
    check(pkg, capfd, "cornell_c2", [N_MUT], 2, rr_depth=1)


def test_flat_records_only_odd_count(pkg, native_lib, capfd):
    check(pkg, capfd, "cornell_c1", [N_MUT], 2)


def test_second_wave_half_empty(pkg, native_lib, capfd):
    check(pkg, capfd, "cornell_c2", [N_MUT], 2)


@pytest.mark.parametrize("batch", [1, 32])
def test_bookkeeping_batches(pkg, native_lib, capfd, batch):
    check(pkg, capfd, "cornell_c2", [N_MUT], 2, env={"DRMLT_MH_BATCH": str(batch)})


def test_two_sliced_launches(pkg, native_lib, capfd):
    check(pkg, capfd, "cornell_c2", [N_MUT // 2], 4, env={"DRMLT_SLICE": "16"})
