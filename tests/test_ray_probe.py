"""What tests/test_gpu_rays.py relies on, checked without a GPU: the probe compiles for gfx950 under both of the library's device
flag sets, keeps everything in registers and takes the LDS of the three stack instantiations; every scene prepares to the counts
that show it reaches its loop; a shading record's index is its shape's; the numpy brute force agrees with the double oracle and
the float oracle passes the decided-ray rule against it (so delta is large enough); at most 2 % of the rays of a class 1 to 6 are
undecided (the class that comes closest: deep_chain's axis-parallel rays, 0.8 %; class 7 is exempt, 46 - 77 % of it are
undecided); the judge accepts a float32 stand-in for trace_brute; and the probe refuses a malformed request with exit status 2
before it touches HIP."""
import struct

import numpy as np
import pytest

import bsdf_probe as bp
import ray_probe as rp


@pytest.fixture(scope="module")
def world(pkg, ob, tmp_path_factory):
    return rp.prepare(pkg, ob, tmp_path_factory.mktemp("ray_probe"))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("ray_probe_exe")
    return {unit: rp.build(d, unit) for unit in rp.UNITS}, d


@pytest.mark.parametrize("unit", rp.UNITS)
def test_probe_cross_compiles_without_scratch(built, unit):
    exe, remarks = built[0][unit]
    assert "k_probe" in remarks and exe.endswith("ray_probe_" + unit)
    assert bp.resource(remarks, "ScratchSize") == [0], remarks
    assert bp.resource(remarks, "VGPRs Spill") == [0] and bp.resource(remarks, "SGPRs Spill") == [0], remarks
    assert bp.resource(remarks, "LDS Size") == [rp.LDS_BYTES], remarks


@pytest.mark.parametrize("name", list(rp.CONFIGS))
def test_every_scene_prepares_to_the_counts_of_its_loop(world, name):
    cfg = world["configs"][name]
    got = {k: cfg["t"]["counts"][k] for k in cfg["want"]}
    assert got == cfg["want"], (name, got)
    c = cfg["t"]["counts"]
    assert len(cfg["t"]["part"]["flat"]) == (64 * (c["n_flat_rec"] + 2) if not c["use_bvh"] and "DRMLT_NO_FLAT_LOOP" not in rp.CONFIGS[name][1] else 0)
    assert len(cfg["t"]["part"]["boxes"]) == (64 * (c["n_box"] + 1) if c["n_box"] else 0)


def test_the_spill_paths_are_reached(world):
    """deep_chain's tree is deeper than the 24 entries of the column (and its overflow area holds it); under the 32-bit-stack knob
    the soup has the area k_mutate_v4's 12-entry column needs, and a tree deeper than that column."""
    deep, soup = world["configs"]["deep_chain"]["t"]["counts"], world["configs"]["soup stack32"]["t"]["counts"]
    assert 3 * deep["bvh_depth"] > 24 and deep["ovf_entries"] >= 3 * deep["bvh_depth"] + 3
    assert 3 * soup["bvh_depth"] > 12 and soup["ovf_entries"] >= 3 * soup["bvh_depth"] + 3
    assert 3 * world["configs"]["deep_chain bounded"]["t"]["counts"]["bvh_depth"] <= 24


@pytest.mark.parametrize("name", list(rp.CONFIGS))
def test_a_shading_record_index_is_its_shapes(world, name):
    """scene_prep.h pushes one record per shape, in order (point and environment records after them): what the device returns
    as `prim` names the scene's shape. Kind and first vertex / centre of every record against the scene."""
    cfg = world["configs"][name]
    g, sh = world["scenes"][cfg["scene"]]["g"], cfg["t"]["shade"]
    assert len(sh) >= g["n"]
    kind = sh["bsdf"][:g["n"]] >> 24
    assert np.array_equal(kind, g["kind"])
    # a triangle: p0 and its two edges; a rectangle: its (-1, -1) corner and the full edges (device_types.h says "centre" of the rectangle's
    # origin; scene_prep.h parametrises it on [0, 1]^2 from that corner, and the records say so); a sphere: centre and radius
    tri, rect, ball = (g["kind"] == k for k in (rp.TRI, rp.RECT, rp.SPHERE))
    o, eu, ev = (sh[k][:g["n"]].astype(np.float64) for k in ("origin", "eu", "ev"))
    tol = 4 * rp.EPS * g["extent"]
    assert np.allclose(o[tri], g["org"][tri], atol=tol, rtol=0) and np.allclose(eu[tri], g["eu"][tri], atol=tol, rtol=0) and np.allclose(ev[tri], g["ev"][tri], atol=tol, rtol=0)
    assert np.allclose(o[rect], (g["org"] - g["eu"] - g["ev"])[rect], atol=tol, rtol=0) and np.allclose(eu[rect], 2 * g["eu"][rect], atol=tol, rtol=0) and np.allclose(ev[rect], 2 * g["ev"][rect], atol=tol, rtol=0)
    assert np.allclose(o[ball], g["c"][ball], atol=tol, rtol=0) and np.allclose(eu[ball, 0], g["r"][ball], atol=tol, rtol=0)
    # every record an intersection record names is one of them, a merged pair's two
    pr = cfg["t"]["prims"]
    assert np.all((pr["shade"] >= 0) & (pr["shade"] + (pr["type"] == 3) < g["n"]))


@pytest.mark.parametrize("scene", sorted(set(rp.SCENE_OF.values())))
def test_numpy_brute_force_agrees_with_the_double_oracle(world, scene):
    """The same shape on every decided ray, t to 1e-12 relative."""
    s = world["scenes"][scene]
    ref, dec = s["ref"], s["decided"]
    assert np.array_equal(ref["o64"]["shape"][dec], s["want"][dec])
    assert np.array_equal(ref["shape"][dec], s["want"][dec])
    hit = dec & (s["want"] >= 0)
    assert hit.sum() > 3000 and (dec & (s["want"] < 0)).sum() > 1000
    assert np.max(np.abs(ref["o64"]["t"][hit] / ref["t"][hit] - 1)) < 1e-12
    assert np.max(np.linalg.norm(ref["o64"]["p"][hit] - ref["p"][hit], axis=1)) < 1e-12 * s["g"]["extent"] * 10


@pytest.mark.parametrize("scene", sorted(set(rp.SCENE_OF.values())))
def test_the_float_oracle_passes_the_decided_ray_rule(world, scene):
    """It names the reference's shape on every decided ray and misses on every decided miss: delta is large enough. Every class
    has rays on which both references name one shape, so every bound has a floor."""
    s = world["scenes"][scene]
    dec = s["decided"]
    assert np.array_equal(s["ref"]["o32"]["shape"][dec], s["want"][dec])
    for c in rp.CLASSES:
        f = s["floors"][c]
        assert f["n"] >= 20 and np.isfinite(f["t"]) and np.isfinite(f["p"]), (c, f)
    # some tens of ulp of the extent, and below the smallest tmin the library gives a ray of class 3 or 4 (make_rays keeps their origins' largest coordinate above 0.15 of the extent)
    assert 4 * rp.EPS * s["g"]["extent"] < s["delta"] < rp.EPSILON_F * 0.15 * s["g"]["extent"], s["delta"]


def test_the_undecided_share_of_every_class_is_within_its_cap(world):
    shares = rp.undecided_shares(world)
    worst = max((v, n, c) for n, sc in shares.items() for c, v in sc.items() if c != "aimed")
    print("undecided: the worst class of 1 to 6 is %s %s, %.4f; class 7: %s" % (worst[1], worst[2], worst[0], {n: round(sc["aimed"], 3) for n, sc in shares.items()}))
    for n, sc in shares.items():
        for c, v in sc.items():
            if c != "aimed":
                assert v <= rp.CAP, (n, c, v)
        assert sc["aimed"] > 0.2, (n, sc["aimed"])                      # borderline by construction
    for s in world["scenes"].values():                                  # every class is there, a few tens of thousands of rays in all
        assert np.all(np.bincount(s["cls"], minlength=7) > 500) and 20000 < len(s["rays"]) < 40000
        assert s["away"].sum() > 1000 and np.all(s["want"][s["away"]] == -1) and np.all(s["decided"][s["away"]])


def test_the_ray_classes_hold_their_special_cases(world):
    """Components of exactly +0 and -0, origins with a coordinate exactly 0, shadow rays traced for any hit and for the closest."""
    s = world["scenes"]["cornell_c2"]
    r = s["rays"][s["cls"] == 1]
    d = r[:, 3:6]
    assert np.all(np.sum(d != 0, axis=1) == 1) and np.any(np.signbit(d) & (d == 0)) and np.any(~np.signbit(d) & (d == 0))
    assert np.sum(np.any(r[:, 0:3] == 0, axis=1)) > 300
    sh = s["rays"][s["cls"] == 3]
    assert 0.4 < np.mean(sh[:, 8] != 0) < 0.6 and np.all(np.isfinite(sh[:, 7]))
    w = s["rays"][s["cls"] == 4]
    assert np.any(np.isfinite(w[:, 7])) and np.any(w[:, 6] > 0.1)


@pytest.mark.parametrize("name", ["cornell_c2 faces", "open_glass_box", "flat_mix even", "two_spheres brute", "soup brute", "deep_chain brute"])
def test_the_judge_accepts_a_float32_stand_in_for_trace_brute(world, name):
    cfg = world["configs"][name]
    s = world["scenes"][cfg["scene"]]
    raw = rp.emulate_brute(cfg["t"], s["rays"])
    rec = rp.judge_op(cfg["t"], s["g"], s["ref"], s["cls"], s["floors"], s["delta"], raw, False, s["rays"])
    assert all(not v for v in rec["findings"].values()), rec["findings"]
    assert rec["hits"] > 5000
    # ... and turns red on a subtly wrong answer: the two sub-triangles of every merged pair exchanged
    prim = raw[:, 0].view(np.int32)
    second = np.isin(prim, cfg["t"]["prims"]["shade"][cfg["t"]["prims"]["type"] == 3] + 1)
    if second.sum() > 100:
        wrong = raw.copy()
        wrong[second, 0] -= 1
        rec = rp.judge_op(cfg["t"], s["g"], s["ref"], s["cls"], s["floors"], s["delta"], wrong, False, s["rays"])
        assert rec["findings"]["decided_shapes"], rec


def test_a_triangle_parallel_to_the_ray_is_no_hit_at_infinity(world):
    """What the probe found in intersect_prim, intersect_leaf and test_flat<true> (tests/test_gpu_rays.py has the account): under the
    hit test as it was, min3(u, v, w) >= 0 alone, the stand-in returns the device's seven hits at t = +inf with NaN barycentrics on
    deep_chain's axis-parallel rays; with w >= 0 beside it, none. This shows the cause and that the judge sees it. It runs numpy, not
    device_path.h: what guards the header's w >= 0 is tests/test_gpu_rays.py::test_nothing_is_non_finite, on the GPU."""
    cfg = world["configs"]["deep_chain brute"]
    s = world["scenes"]["deep_chain"]
    judge = lambda raw: rp.judge_op(cfg["t"], s["g"], s["ref"], s["cls"], s["floors"], s["delta"], raw, False, s["rays"])["findings"]
    was = rp.emulate_brute(cfg["t"], s["rays"], w_test=False)
    bad = (was[:, 0].view(np.int32) >= 0) & ~np.isfinite(was[:, 1].view(np.float32))
    assert bad.sum() == 7 and np.all(s["cls"][bad] == 1) and np.all(s["want"][bad] == -1) and np.all(s["decided"][bad])
    assert judge(was)["non_finite"] and not any(judge(rp.emulate_brute(cfg["t"], s["rays"])).values())


def _words(raw, dtype, field):
    a = np.frombuffer(raw, dtype=dtype).copy()
    return a, a[field]


def test_the_probe_refuses_malformed_requests_before_it_touches_hip(world, built):
    """Exit status 2 for one out-of-range child index, leaf reference or shading index, a missing sentinel, and an op the scene's
    tables do not support. main() checks all of it before the first HIP call, so this runs without a GPU."""
    exe, d = built[0][rp.UNITS[0]][0], built[1]
    soup, c2 = world["configs"]["soup stack16"]["t"], world["configs"]["cornell_c2"]["t"]
    rays = world["scenes"]["soup"]["rays"][:64]

    def refused(t, ops, what, **kw):
        code, err, _ = rp.run_raw(exe, d, rp.request(t, rays, ops, **kw), limit=20)
        assert code == 2 and what in err, (code, err)

    def with_part(t, name, raw):
        part = dict(t["part"])
        part[name] = raw
        return dict(part=part)

    n_nodes, n_prims, n_shade = soup["counts"]["n_bvh_nodes"], soup["counts"]["n_prims"], soup["counts"]["n_shade"]
    a, child = _words(soup["part"]["bvh"], rp.NODE, "child")
    inner = np.argwhere(child >= 0)[-1]
    child[tuple(inner)] = n_nodes
    refused(soup, ("bvh32",), "outside", **with_part(soup, "bvh", a.tobytes()))
    a, child = _words(soup["part"]["bvh"], rp.NODE, "child")
    child[tuple(inner)] = inner[0]                                      # its own parent: a cycle
    refused(soup, ("bvh32",), "outside", **with_part(soup, "bvh", a.tobytes()))
    a, child = _words(soup["part"]["bvh"], rp.NODE, "child")
    leaf = np.argwhere(child < -1)[0]
    child[tuple(leaf)] = ~n_prims
    refused(soup, ("bvh16",), "leaf reference", **with_part(soup, "bvh", a.tobytes()))
    a, shade = _words(soup["part"]["prims"], rp.PRIM, "shade")
    shade[5] = n_shade
    a["kind_shade"][5] = a["type"][5] | (n_shade << 8)
    refused(soup, ("bvh32",), "shading record", **with_part(soup, "prims", a.tobytes()))
    # the flat table's kind_shade, a face word's shade field, the sentinels
    flat = np.frombuffer(c2["part"]["flat"], dtype=np.int32).copy().reshape(-1, 16)
    flat[0, 12] = 1 | (c2["counts"]["n_shade"] << 8)
    refused(c2, ("trace0",), "flat record 0", **with_part(c2, "flat", flat.tobytes()))
    boxes = np.frombuffer(c2["part"]["boxes"], dtype=np.uint32).copy().reshape(-1, 16)
    boxes[1, 13] = (boxes[1, 13] & 0xffff003f) | (1023 << 6)
    refused(c2, ("trace0",), "cuboid 1", **with_part(c2, "boxes", boxes.tobytes()))
    refused(c2, ("trace0",), "sentinel", **with_part(c2, "flat", c2["part"]["flat"][:-64]))
    refused(c2, ("trace0",), "sentinel", **with_part(c2, "boxes", c2["part"]["boxes"][:-64]))
    # ops the tables do not support
    refused(soup, ("held",), "w2_held_launch")
    refused(soup, ("trace0",), "no flat scene")
    refused(c2, ("bvh32",), "no BVH")
    refused(world["configs"]["soup stack32"]["t"], ("bvh16",), "16 bits")
    no_area = dict(world["configs"]["deep_chain"]["t"])
    no_area["counts"] = dict(no_area["counts"], ovf_entries=0)
    refused(no_area, ("bvh32",), "deeper than the stack column")
    # a parameter block that carries a pointer, and a short request
    p = bytearray(c2["params"])
    p[0:8] = struct.pack("<Q", 0x1000)
    refused(c2, ("trace0",), "pointer", params=bytes(p))
    code, err, _ = rp.run_raw(exe, d, rp.request(c2, rays, ("trace0",))[:-8], limit=20)
    assert code == 2 and "short request" in err, (code, err)
