"""The device's local-frame BSDF, Fresnel and warp routines, call by call (tests/native/bsdf_probe.hip, built under both
device flag sets of the library and run as a child process, seven runs a build) against the oracle in double and against
closed forms in fp64 -- tests/bsdf_probe.py has the inputs, the references and the rule:

    |device - oracle64| <= 32 * max |oracle32 - oracle64| + 4 ulp        per quantity and per cell.

Measured on an MI355X (profiles/r10_bsdf_probe.json). The two builds round differently -- 17 % of rc_sample's and 18 % of
sa_eval's output elements differ in the last bits, fr_cond by at most 2.4e-7; distr, warp and the scalars are bit-equal --
and share the figures below to the digits shown:

  rough conductor, 212 cells (Beckmann / GGX, alpha 1e-5 .. 1, 16 incident directions, three materials), 4096 stratified
  samples and 36 corner pairs each: nothing non-finite for wi.z > 0; on the grid the device rejects exactly the samples
  the fp64 oracle rejects, in every cell. Worst device error as a share of the rule's bound, over all cells of the grid:
  wo 0.09, weight 0.20, pdf 0.06, sampled normal 0.12, D 0.07, G1 0.11, pdfVisible 0.06, f cos and pdf(wi, wo) 0.06 at the
  sampled directions and 0.27 at the mirror and the 256 uniform ones; identities: pdf 0.05, weight * pdf = eval 0.05,
  reciprocity 0.09. The corner pairs, judged against their own floors: at most 0.70 (pdf identity). No cell needs more
  than the rule gives, so no cell has a bound of its own.
  The diffuse BSDF (type 0) through the same two entry points: 0.03, exactly 0 from or towards below.
  Conductor Fresnel 0.03 of the bound; the mirror's pdf_delta is 1 at and 0.5e-3 off the mirror direction and 0 at 2e-3 off.
  F(cos = 0) = 1 - 2^-24 in one channel of copper: the quotient term1 / term1 goes through v_rcp_f32 (the library is built
  without correctly rounded division), so "equals 1" is held to the rule's 4 ulp.
  Dielectric F and cos theta_t at most 0.09 of the bound, eta == 1 exact, pdf_delta exact. Warp 0.04, length within 0.6 ulp.
  Scalars: rc_exp 3.8e-6 relative over [-87, 0] (4.7e-7 over [-10, 0]) -- the "~2e-6" of device_bsdf.h did not hold and the
  comment now states the measured figures, which SCALAR_CLAIMS pins --, rc_log 1.5e-7 relative / 1.0e-7 absolute, sin_rev and
  cos_rev 1.1e-7, mts_erf 3.3e-7 and mts_erfinv 1.2e-7 relative against Mitsuba's polynomials in fp64 (the fp32 oracle: 3.0e-7, 1.6e-7).

Corner pairs on which the device and the fp64 oracle disagree about rejection, 52 in all, one class: GGX with sx == 0 at
alpha <= 1e-3 and grazing wi. There A = -1 and sampleVisible11 moves it by Epsilon, which is 1e-4 in Mitsuba's single
precision build and 1e-7 in its double precision build (core/constants.h): the two precisions sample different slopes, the
double one a normal at grazing angle whose reflection goes below the surface. The device uses the single precision constant
and decides as the fp32 oracle does on every one of them; a corner on which it differs from both oracles fails the test.
The two suppositions that prompted this module: no output is non-finite for wi.z > 0, so mts_erfinv never handed back an
infinite slope on these inputs (the Newton start value stays 2.4e-7 below c = erf(cot theta) even at sx = 1 - 2^-24); and
rc_exp does miss the header's figure (above). For wi.z <= 0 sampleVisible returns NaN (tan theta is infinite or negative
there), which sample() never uses: it returns before (wi.z < 0) or rejects on pdfVisible == 0 (wi.z == 0).

Which test turns red when the device code is broken on purpose (each tried on the GPU in a scratch copy of the headers):
  no fmaxf(sx, 1e-6f) floor      -> nothing_is_non_finite (44 cells), rejection, values
  s1 and s2 exchanged (GGX)      -> rejection, values (wo 1000 x the bound)
  eta for 1 / eta (dielectric)   -> dielectric_fresnel_and_snell, dielectric_pdf_delta
  no alpha clamp in make_rc      -> alpha_clamp, rejection, values, identities
"""
import os

import numpy as np
import pytest

import bsdf_probe as bp
import bsdf_scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference(ob):
    """The oracle's side of the rough conductor, computed once for both builds."""
    cells, sxy = bp.rc_cells(), bp.sample_points()
    return cells, bp.rc_reference(ob, cells, sxy)


@pytest.fixture(scope="module")
def measured(ob, reference, tmp_path_factory):
    """{build: (report, findings, raw output)}: all 14 child runs of the module. A run that fails ends them."""
    cells, ref = reference
    tmp = tmp_path_factory.mktemp("bsdf_probe")
    out = {}
    for unit in bp.UNITS:
        exe, _ = bp.build(tmp, unit)
        try:
            rep, raw = bp.measure(ob, bp.Probe(exe, tmp), cells, ref)
        except bp.ProbeDied as e:
            out[unit] = e
            break
        out[unit] = (rep, bp.findings(rep, raw, cells), raw)
    return out


@pytest.fixture(params=bp.UNITS)
def found(request, measured):
    """The findings of one build; after a failed run the tests of that build fail and the later build's skip."""
    m = measured.get(request.param)
    if m is None:
        pytest.skip("not run: " + str(bp.Probe.dead))
    if isinstance(m, Exception):
        pytest.fail(str(m))
    rep, f, raw = m
    assert rep["runs"] == 7
    return f


def _none(found, key):
    assert not found[key], "%d findings, the first: %s" % (len(found[key]), found[key][:5])


def test_nothing_is_non_finite(found):
    _none(found, "non_finite")


def test_rejection_agrees_with_the_fp64_oracle(found):
    """>= 99.9 % of each cell's grid; every corner pair that differs from the fp64 oracle agrees with the fp32 oracle (the
    class explained above); weight, pdf and value are exactly 0 for wi.z <= 0."""
    _none(found, "rejection")


def test_values_meet_the_rule_in_every_cell(found):
    _none(found, "values")


def test_identities_hold_on_the_devices_own_output(found):
    _none(found, "identities")


def test_alpha_clamp(found):
    """alpha = 1e-5 gives the bits of alpha = 1e-4."""
    _none(found, "clamp")


def test_conductor_fresnel(found):
    _none(found, "conductor_fresnel")


def test_dielectric_fresnel_and_snell(found):
    _none(found, "dielectric")


def test_dielectric_pdf_delta(found):
    _none(found, "pdf_delta")


def test_warp(found):
    _none(found, "warp")


def test_scalar_routines_meet_what_the_header_states(found):
    _none(found, "scalar")


def test_the_two_builds_are_recorded_side_by_side(measured):
    """Their difference is recorded, not asserted; DRMLT_BSDF_PROBE_JSON=<file> keeps the whole report."""
    if any(isinstance(m, Exception) for m in measured.values()) or len(measured) < 2:
        pytest.skip("not run: " + str(bp.Probe.dead))
    a, b = (measured[u][2] for u in bp.UNITS)
    diff = bp.builds_differ(a, b)
    print("elements that differ between the builds:", diff)
    assert sum(measured[u][0]["runs"] for u in bp.UNITS) <= 16
    path = os.environ.get("DRMLT_BSDF_PROBE_JSON")
    if path:
        bp.write_summary(path, bp.summary({u: measured[u][0] for u in bp.UNITS}, diff))


@pytest.mark.parametrize("alpha,ggx", [(0.01, 0), (0.5, 0), (0.01, 1), (0.5, 1)])
def test_parameters_reach_the_routines(pkg, ob, native_lib, alpha, ggx):
    """eval_paths on a room with a rough-conductor floor against the oracle, the criteria of test_eval_paths_matches_oracle:
    roughness, the p[7] flag and the reflectance arrive at the routines probed above."""
    sd = bsdf_scenes.rough_floor_room(pkg, alpha, ggx)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=64)
    ctx, orc = pkg.Context(cfg, sd), ob.Oracle(pkg.abi, cfg, sd, 64)
    u = np.random.default_rng(1).random((4096, 50), dtype=np.float32)
    g, o = ctx.eval_paths(u), orc.eval_paths(u)
    ctx.close(), orc.close()
    same = g["n_dims"] == o["n_dims"]
    rel = np.abs(g["luminance"] - o["luminance"])[same] / np.maximum(o["luminance"][same], 1e-3)
    print("alpha %g ggx %d: topology %.4f, q99 %.3g, mean %.6g vs %.6g" % (alpha, ggx, same.mean(), np.quantile(rel, 0.99), g["luminance"].mean(), o["luminance"].mean()))
    assert same.mean() >= 0.995, same.mean()
    assert np.all(g["n_rays"][same] <= o["n_rays"][same])
    assert np.allclose(g["x"], o["x"], atol=1e-3) and np.allclose(g["y"], o["y"], atol=1e-3)
    assert np.quantile(rel, 0.99) < 1e-3, np.quantile(rel, 0.99)
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert np.allclose(g["rgb"][same], o["rgb"][same], rtol=5e-2, atol=1e-3)
    assert (g["luminance"] > 0).mean() > 0.5
