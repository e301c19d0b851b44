"""What tests/test_gpu_lights.py relies on, checked without a GPU: the probe compiles for gfx950 under both of the library's
device flag sets and keeps everything in registers, the numpy closed forms agree with the fp64 oracle, and in every cell the
float and double oracles are finite, give the rule a finite floor, reject the same samples of the grid and pick the same
emitter off the CDF's entries."""
import numpy as np
import pytest

import bsdf_probe as bp
import light_probe as lp


@pytest.fixture(scope="module")
def world(pkg, ob, tmp_path_factory):
    return lp.prepare(pkg, ob, tmp_path_factory.mktemp("light_probe"))


@pytest.mark.parametrize("unit", lp.UNITS)
def test_probe_cross_compiles_without_scratch(tmp_path, unit):
    exe, remarks = lp.build(tmp_path, unit)
    assert "k_probe" in remarks and exe.endswith("light_probe_" + unit)
    assert bp.resource(remarks, "ScratchSize") == [0], remarks
    assert bp.resource(remarks, "VGPRs Spill") == [0] and bp.resource(remarks, "SGPRs Spill") == [0], remarks
    assert bp.resource(remarks, "LDS Size") == [0], remarks


def test_the_tables_are_the_scene(world):
    """The uploaded records say what the scenes were built from: kinds, radii, the CDF over the weights with its zero-width entries."""
    t = world["lights"]["tables"]
    kinds = t["shade"]["bsdf"][t["emitters"]["prim"]] >> 24
    assert list(kinds) == [1, 1, 2, 4, 4, 5, 0] and t["n_emitters"] == 7 and t["n_bsdfs"] == 2
    cdf = np.cumsum(np.array(lp.WEIGHTS)) / sum(lp.WEIGHTS)
    assert np.allclose(t["emitters"]["cdf_hi"], cdf, atol=1e-7) and np.allclose(t["emitters"]["cdf_lo"][1:], cdf[:-1], atol=1e-7)
    assert t["emitters"]["cdf_hi"][-1] == 1 and np.all(t["emitters"]["cdf_hi"][[0, 3, 6]] == t["emitters"]["cdf_lo"][[0, 3, 6]])
    s = world["spheres"]["tables"]
    assert [float(v) for v in s["shade"]["eu"][:, 0]] == [float(np.float32(r)) for _, r in lp.SPHERES]
    # the environment's sphere is the fp32 oracle's to rounding
    o32 = world["lights"]["env_ref"]["o32"]
    assert np.allclose(world["lights"]["env_c"], o32["env_center"], atol=1e-6) and world["lights"]["env_R"] == pytest.approx(o32["env_radius"], rel=1e-6)


def test_numpy_closed_forms_agree_with_the_fp64_oracle(world):
    """Away from the branch band, to 1e-12: the area sample and its dist^2 / (A |cos|), cos / pi for the sky, and the cone's
    density. The oracle forms 1 - cos alpha by subtraction, which costs it one rounding of 1, 2^-52 / (1 - cos alpha) relative -- 4e-10
    at sin alpha = 1e-3, 2e-12 at 1e-2 --: that error of the reference's is added to the 1e-12."""
    sp = world["spheres"]
    ref, ns, seen = sp["ref"], sp["ref"]["ns"], set()
    for i, cl in enumerate(sp["cells"]):
        sl = slice(i * ns, (i + 1) * ns)
        c, r = lp._round(lp.SPHERES[cl["emitter"]][0]), float(np.float32(lp.SPHERES[cl["emitter"]][1]))
        o = {k: v[sl] for k, v in ref["o64"].items()}
        if cl["kind"] == "cone":
            want = lp.cone_density(c, r, cl["ref"].astype(np.float64))
            assert np.all(np.abs(o["pdf"] / want - 1) < 1e-12 + 2.0 ** -52 * 2 * np.pi * want), cl["name"]
            assert np.max(np.abs(o["pdf_direct"] / o["pdf"] - 1)) < 1e-12 + 2.0 ** -52 * 2 * np.pi * want, cl["name"]     # the oracle's second copy
        elif cl["kind"] == "area":
            a = lp.sphere_area_sample(c, r, cl["ref"].astype(np.float64), ref["s"][sl])
            for k in ("d", "dist", "n"):
                assert np.max(np.abs(a[k] - o[k])) < 1e-12, (cl["name"], k)
            assert np.max(np.abs(a["pdf"] / o["pdf"] - 1)) < 1e-12, cl["name"]
        seen.add(cl["kind"])
    assert seen == {"cone", "area", "band"}
    lt = world["lights"]
    o = lt["env_ref"]["o64"]
    inside = o["pdf"] > 0
    assert inside.sum() >= 3 * len(lp.NORMALS) * ns
    nn = np.sum(lt["env_ref"]["n"] ** 2, axis=1)        # the float32 normals are unit to 6e-8 only: d = s x + t y + n z has d . n = z |n|^2
    assert np.max(np.abs(o["pdf"] - np.sum(o["d"] * lt["env_ref"]["n"], axis=1) / nn / np.pi)[inside]) < 1e-12
    # a flat light's density: the rectangle's samples of the light-pick scene
    r = lt["ref"][0]["o64"]
    rect = r["emitter"] == 1
    m = np.array(list(lt["scene"].shapes[1].data[:12]), dtype=np.float64).reshape(3, 4)     # toWorld as stored, in float32
    area = 4 * np.linalg.norm(m[:, 0]) * np.linalg.norm(m[:, 1])
    want = lp.flat_density(r["dist"], area, np.sum(r["d"] * r["n"], axis=1)) * (r["cdf"][2] - r["cdf"][1])
    assert rect.sum() > 1000 and np.max(np.abs(r["pdf"] / want - 1)[rect]) < 1e-12


def test_the_branch_band_is_where_the_two_oracles_part(world):
    """In the band the fp32 oracle samples the area and the fp64 oracle the cone; at 1 - 1.2e-4 both sample the cone."""
    sp = world["spheres"]
    ref, ns, n_band = sp["ref"], sp["ref"]["ns"], 0
    for i, cl in enumerate(sp["cells"]):
        if "sin=1-" not in cl["name"]:
            continue
        sl = slice(i * ns, (i + 1) * ns)
        c, r = lp._round(lp.SPHERES[cl["emitter"]][0]), float(np.float32(lp.SPHERES[cl["emitter"]][1]))
        cone = lp.cone_density(c, r, cl["ref"].astype(np.float64))
        is_cone = lambda o: np.all(np.abs(o["pdf"][sl] / cone - 1) < 1e-2)
        assert is_cone(ref["o64"]), cl["name"]
        assert is_cone(ref["o32"]) == (cl["kind"] == "cone"), cl["name"]
        n_band += cl["kind"] == "band"
    assert n_band == 3 * 2 * len(lp.SPHERES)


def test_float_and_double_oracles_give_every_cell_a_finite_floor(world):
    """The precondition of the GPU test. Spheres: nothing non-finite, finite floors. Environment: the same, and the same
    samples inside. Light pick: the same emitter off the CDF's entries, the same rejections on the grid (mismatch 0)."""
    sp = world["spheres"]
    checks, fin = lp.sphere_floors(sp["cells"], sp["ref"])
    assert fin.all(), int((~fin).sum())
    assert len(sp["cells"]) == 2 * (9 * 8 + 2 * 4 + 1 + 9 * 2)
    for cl, ch in zip(sp["cells"], checks):
        assert all(np.isfinite(v["floor"]) for v in ch.values()), (cl["name"], ch)
    pdf = [ch["pdf"]["floor"] for cl, ch in zip(sp["cells"], checks)]
    print("sphere grid floors: pdf %.2g .. %.2g relative" % (min(pdf), max(pdf)))
    lt = world["lights"]
    q, at = lp.env_quantities(lt["env_cells"], lt["env_ref"], None, None, None)
    o64, o32 = lt["env_ref"]["o64"], lt["env_ref"]["o32"]
    for k in ("d", "dist", "pdf"):
        assert np.all(np.isfinite(o64[k])) and np.all(np.isfinite(o32[k])), k
    for k, (_, floor, mask) in q.items():
        assert np.all(np.isfinite(floor[mask])) and mask.sum() > 1000, k
    assert np.all((o64["pdf"] > 0)[at < 1.0]) and np.all((o32["pdf"] > 0)[at < 1.0])
    assert np.all(o64["pdf"][at > 1.0] == 0) and np.all(o32["pdf"][at > 1.0] == 0)
    # on the sphere (1.0 R as float32) the precisions part: the point lies outside the fp64 oracle's sphere and inside the fp32 oracle's,
    # so there the device is held to the fp32 oracle's zero pattern, and d and cos / pi to the cells at the centre (env_quantities)
    assert np.all(o64["pdf"][at == 1.0] == 0) and np.all(o32["pdf"][at == 1.0] > 0) and q["d"][2][at == 1.0].all() and q["pdf"][2][at == 1.0].all()
    edge = lt["edge"]
    assert 100 < edge.sum() < len(edge) // 10
    for c, r in zip(lt["cells"], lt["ref"]):
        assert np.all(np.isfinite(r["c64"])) and np.all(np.isfinite(r["c32"])), c["name"]
        assert np.array_equal(r["o32"]["emitter"][~edge], r["o64"]["emitter"][~edge]), c["name"]
        assert not np.any(np.isin(r["o64"]["emitter"], [0, 3, 6])) and not np.any(np.isin(r["o32"]["emitter"], [0, 3, 6])), c["name"]
        assert set(r["o64"]["emitter"]) == {1, 2, 4, 5}
        rej64, rej32 = np.all(r["c64"] == 0, axis=1), np.all(r["c32"] == 0, axis=1)
        assert np.sum((rej64 != rej32)[~edge]) == 0, c["name"]
        named = lp.name_emitter(r["o64"]["d"], r["o64"]["dist"], lt["sky_from"])
        assert np.array_equal(named, r["o64"]["emitter"]), c["name"]          # direction and distance do name the emitter
    half = lt["ref"][2]
    rect = (half["o64"]["emitter"] == 1) & ~edge
    share = np.all(half["c64"] == 0, axis=1)[rect].mean()
    assert 0.45 < share < 0.55, share                                       # half of rectangle 1 lies below that receiver's horizon
    # with its zero-weight first emitter, the scene's sx == 0 goes to emitter 1 in both oracles
    zero = lt["sxy"][:, 0] == 0
    assert zero.sum() == 16 and np.all(lt["ref"][0]["o64"]["emitter"][zero] == 1) and np.all(lt["ref"][0]["o32"]["emitter"][zero] == 1)
