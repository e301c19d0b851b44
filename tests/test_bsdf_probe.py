"""What tests/test_gpu_bsdf.py relies on, checked without a GPU: the probe compiles for gfx950 under both of the library's
device flag sets and keeps everything in registers, the oracle's new entry agrees with the old one, the numpy references
agree with the oracle's Fresnel code, and the float and double oracles give the rule a finite floor in every cell and reject
the same samples of the stratified grid."""
import numpy as np
import pytest

import bsdf_probe as bp


@pytest.mark.parametrize("unit", bp.UNITS)
def test_probe_cross_compiles_without_scratch(tmp_path, unit):
    fl = bp.flags(unit)
    assert "-fno-slp-vectorize" in fl and ("-ffp-contract=on" in fl) == (unit == "kernels"), fl
    exe, remarks = bp.build(tmp_path, unit)
    assert "k_probe" in remarks
    assert bp.resource(remarks, "ScratchSize") == [0], remarks
    assert bp.resource(remarks, "VGPRs Spill") == [0] and bp.resource(remarks, "SGPRs Spill") == [0], remarks


@pytest.mark.parametrize("ggx", [0, 1])
def test_new_oracle_entry_reproduces_the_old_one(ob, ggx):
    eta, k = bp.COPPER
    sxy = bp.sample_points()[::7].astype(np.float64)
    wi = np.array(bp._dir(0.5), dtype=np.float64)
    old = ob.roughconductor(ggx, 0.1, eta, k, wi, sxy=sxy)
    new = ob.bsdf_probe(64, ggx, 0.1, eta, k, np.repeat(wi[None, :], len(sxy), axis=0), wo=old["wo"], sxy=sxy)
    acc = ~np.all(old["weight"] == 0, axis=1)
    assert acc.sum() > 500
    assert np.array_equal(new["weight"], old["weight"]) and np.array_equal(new["spdf"], old["spdf"])
    assert np.array_equal(new["wo"][acc], old["wo"][acc])
    at = ob.roughconductor(ggx, 0.1, eta, k, wi, wo=old["wo"])
    assert np.array_equal(new["eval"], at["eval"]) and np.array_equal(new["pdf"], at["pdf"])
    assert np.array_equal(new["eval_at_wo"][acc], at["eval"][acc]) and np.array_equal(new["pdf_at_wo"][acc], at["pdf"][acc])
    # the reflectance scales the weight and nothing else
    half = ob.bsdf_probe(64, ggx, 0.1, eta, k, np.repeat(wi[None, :], len(sxy), axis=0), sxy=sxy, specular_reflectance=(0.5, 0.25, 1.0))
    assert np.allclose(half["weight"], old["weight"] * [0.5, 0.25, 1.0], rtol=1e-15, atol=0) and np.array_equal(half["spdf"], old["spdf"])
    with pytest.raises(ob.OracleError):
        ob.bsdf_probe(16, ggx, 0.1, eta, k, wi[None, :], sxy=sxy[:1])


def test_numpy_fresnel_references_agree_with_the_oracle(ob):
    cos = np.concatenate([np.linspace(0, 1, 257), [1e-4, 1e-3]])
    for m, (eta, k) in bp.MATERIALS.items():
        for j in range(3):
            want = bp.fresnel_conductor_complex(cos, eta[j], k[j])
            assert np.max(np.abs(ob.fresnel_conductor(64, cos, eta[j], k[j]) - want)) < 1e-12, m
    ec = bp.dielectric_inputs()
    F, ct, ct2 = bp.fresnel_dielectric_signed(ec[:, 1], ec[:, 0])
    Fo, cto = ob.fresnel_dielectric(64, ec[:, 1], ec[:, 0])
    off = np.abs(ct2) >= 1e-5                       # at the critical angle itself cos theta_t is the root of a rounding error
    assert off.sum() >= 90 and (~off).sum() >= 10
    assert np.max(np.abs(Fo - F)[off]) < 1e-12 and np.max(np.abs(cto - ct)[off]) < 1e-12
    assert np.all((Fo >= 0) & (Fo <= 1)) and np.all(np.abs(cto[~off]) < 4e-3)
    # eta == 1: no reflection, the direction goes straight on
    one = ec[:, 0] == 1
    assert one.sum() == 12 and np.all(Fo[one] == 0) and np.array_equal(cto[one], -ec[one, 1])
    # and the conductor with k = 0 is the dielectric seen from outside
    c = np.linspace(0.01, 1, 100)
    assert np.max(np.abs(bp.fresnel_conductor_complex(c, 1.5, 0.0) - bp.fresnel_dielectric_signed(c, 1.5)[0])) < 1e-12
    assert np.max(np.abs(ob.cosine_hemisphere(64, bp.warp_points()) - bp.cosine_hemisphere(bp.warp_points()))) < 1e-12


def test_float_and_double_oracles_give_every_cell_a_finite_floor(ob):
    """The precondition of the GPU test: on the stratified grid the two oracles reject the same samples in every cell (so
    holding the device to 99.9 % costs the reference nothing), nothing they return is non-finite for wi.z > 0, corner pairs
    included, and the floors of the rule are finite. The floors differ by orders of magnitude between cells -- the reason
    the rule is applied per cell."""
    cells, sxy = bp.rc_cells(), bp.sample_points()
    assert len(sxy) == bp.N_GRID + 36 and len(cells) == 212
    ref = bp.rc_reference(ob, cells, sxy)
    wo_floors, pdf_floors = [], []
    for c, r in zip(cells, ref):
        if not c["wi"][2] > 0:
            assert np.all(r[64]["weight"] == 0) and np.all(r[32]["weight"] == 0) and np.all(r[64]["spdf"] == 0), c["name"]
            continue
        for p in (64, 32):
            for key in ("wo", "weight", "spdf", "m", "D", "G1", "pdf_visible", "pdf_at_wo", "eval_at_wo"):
                assert np.all(np.isfinite(r[p][key])), (c["name"], p, key)
        for tag, part in bp.GROUPS:
            fl, mismatch = bp.rc_floors(r, c, part)
            assert all(np.isfinite(v) for v in fl.values()), (c["name"], tag, fl)
            if tag == "":
                assert mismatch == 0, (c["name"], mismatch)
                wo_floors.append(fl["wo"]), pdf_floors.append(fl["pdf"])
    print("grid floors: wo %.2g .. %.2g, pdf %.2g .. %.2g relative" % (min(wo_floors), max(wo_floors), min(pdf_floors), max(pdf_floors)))
    assert max(wo_floors) < 1e-3 and max(pdf_floors) < 1e-2
    assert max(wo_floors) > 100 * min(wo_floors)
