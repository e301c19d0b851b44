"""Vertex normals of triangle meshes on the device (technique=path and the direct pass): f(u) against closed forms (a constant
tilted normal, an interpolated one, a light with vertex normals), the face-normal twins of the parity scenes against the fp64
oracle point by point, chain by chain and build by build, genuinely smooth scenes across the kernel builds, and images.
The protocols are those of test_gpu_parity.py, test_gpu_emitter_parity.py, test_gpu_conductor.py and test_gpu_direct.py."""
import numpy as np
import pytest

import conductor_scenes  # noqa: F401  (test_gpu_conductor imports it)
import emitter_scenes as es
import normals_scenes as ns
import direct_scenes as ds
import test_gpu_conductor as gc
import test_gpu_direct as gd
import test_gpu_emitter_parity as ep

pytestmark = pytest.mark.gpu
lum, rel_mse = gc.lum, gc.rel_mse
FLAT, BVH = dict(DRMLT_BVH_THRESHOLD=1000000), dict(DRMLT_BVH_THRESHOLD=0)


def _eval(pkg, sd, env, n=16384, max_depth=2, seed=11):
    cfg = pkg.abi.make_config(type="orbital", max_depth=max_depth, rr_depth=100, direct_samples=-1, work_units=64)
    ctx = gc._ctx_with_env(pkg, cfg, sd, **env)
    g = ctx.eval_paths(np.random.default_rng(seed).random((n, 32), dtype=np.float32))
    ctx.close()
    return g


# ---------------------------------------------------------------- 1. closed form, constant tilted normal
@pytest.mark.parametrize("env", [FLAT, BVH], ids=["flat", "bvh"])
def test_constant_tilted_normal_matches_the_closed_form(pkg, native_lib, env):
    """A view-filling diffuse triangle pair whose vertex normals all point 20 degrees off the face normal, one point light, maxDepth 2:
    f = rho / pi * I * (n_s . omega) / d^2 at the hit the splat position implies, within 1e-4 (the bound of
    test_mirrored_point_lit_plane_matches_the_closed_form): n_s . omega >= 0.2 over the whole view, and the fp32 error of a unit
    vector and of d^2 is a few 1e-7. With face normals the cosine is that of the face normal: off by up to 30 %.
    Measured on the MI355X: max rel err 5.9e-07 (flat loop), 5.9e-07 (BVH); against the face normal's value 0.40."""
    sd = ns.tilted_pair(pkg)
    cos_min, _ = ns.view_corners_cos(pkg, [(-2, -2, 0), (2, -2, 0), (2, 2, 0)], [ns.TILTED] * 3)
    assert cos_min >= 0.2, cos_min
    g = _eval(pkg, sd, env)
    p = ns.plane_points(pkg, g["x"], g["y"])
    want, cos = ns.point_lit_closed_form(p, np.tile(ns._f32(ns.TILTED) / np.linalg.norm(ns._f32(ns.TILTED)), (len(p), 1)))
    rel = np.abs(g["rgb"] - want) / want
    flat_want, _ = ns.point_lit_closed_form(p, np.tile([0.0, 0.0, 1.0], (len(p), 1)))
    print("tilted pair %s: max rel err %.3g over %d points (against the face normal's value: %.3g)"
          % (env, rel.max(), len(p), (np.abs(g["rgb"] - flat_want) / flat_want).max()))
    assert rel.max() < 1e-4, rel.max()
    assert np.all(g["n_dims"] == 6)                    # film 2, light sample 2, bounce 2


# ---------------------------------------------------------------- 2. closed form, interpolated normal
@pytest.mark.parametrize("env", [FLAT, BVH], ids=["flat", "bvh"])
def test_interpolated_normal_matches_the_closed_form(pkg, native_lib, env):
    """One triangle with three different, unnormalised vertex normals: the shading normal is normalize(sum b_i n_i) of the normals
    as stored. Same light, same bound. Measured on the MI355X: max rel err 5.9e-07 (flat loop), 5.9e-07 (BVH); against normalised vertex normals 0.24."""
    sd = ns.big_triangle(pkg)
    cos_min, b_min = ns.view_corners_cos(pkg, ns.BIG_TRI, ns.BIG_TRI_NORMALS)
    assert cos_min >= 0.2 and b_min > 0, (cos_min, b_min)    # lit everywhere, and the triangle overfills the view
    g = _eval(pkg, sd, env)
    p = ns.plane_points(pkg, g["x"], g["y"])
    n, _ = ns.interpolated_normals(p, ns.BIG_TRI, ns.BIG_TRI_NORMALS)
    want, _ = ns.point_lit_closed_form(p, n)
    rel = np.abs(g["rgb"] - want) / want
    # normalising the vertex normals first is a different interpolation: the test can tell the two apart
    unit = ns.BIG_TRI_NORMALS / np.linalg.norm(ns.BIG_TRI_NORMALS, axis=1)[:, None]
    other, _ = ns.point_lit_closed_form(p, ns.interpolated_normals(p, ns.BIG_TRI, unit)[0])
    print("big triangle %s: max rel err %.3g over %d points (against normalised vertex normals: %.3g)"
          % (env, rel.max(), len(p), (np.abs(g["rgb"] - other) / other).max()))
    assert rel.max() < 1e-4, rel.max()
    assert np.all(g["luminance"] > 0) and np.all(g["n_dims"] == 6)


@pytest.mark.parametrize("bsdf", ["diffuse", "roughconductor", "dielectric", "conductor"])
@pytest.mark.parametrize("env", [FLAT, BVH], ids=["flat", "bvh"])
def test_a_normal_without_a_direction_is_an_invalid_sample(pkg, native_lib, env, bsdf):
    """Vertex normals that cancel everywhere (a zero table entry) on the view-filling triangle, under every BSDF and at a depth at
    which the path could go on: every f is exactly 0, never a NaN."""
    sd = ns.big_triangle(pkg, normals=np.zeros((3, 3)))
    m = pkg.scenes.SceneData("m")
    getattr(m, bsdf)(*((0.5,) if bsdf == "diffuse" else ()))
    sd.bsdfs[0] = m.bsdfs[0]
    g = _eval(pkg, sd, env, n=4096, max_depth=6)
    assert np.isfinite(g["rgb"]).all() and np.all(g["rgb"] == 0) and np.all(g["luminance"] == 0)


# ---------------------------------------------------------------- 3. closed form, smooth emitter
@pytest.mark.parametrize("env", [FLAT, BVH], ids=["flat", "bvh"])
def test_smooth_emitter_matches_the_closed_form(pkg, native_lib, env):
    """A diffuse plane under a triangle light of edge 1e-5 at a distance above 1.2 whose vertex normals point 20 degrees off its face
    normal: f = rho / pi * L * A * cos theta_l (shading) * cos theta / d^2 within 1e-4. A light sample is one point of the light:
    against the centroid's value it is off by up to 2 size / distance = 2e-5 (a light of 1e-3 measured 1.1e-3); the MIS weight
    differs from 1 by less than 1e-13. With the vertex normals flipped the light faces away: every f is 0.
    Measured on the MI355X: max rel err 1.1e-05 (flat loop), 1.1e-05 (BVH); against the face normal's value 0.34."""
    g = _eval(pkg, ns.lamp_lit_plane(pkg), env)
    want = ns.lamp_closed_form(ns.plane_points(pkg, g["x"], g["y"]))
    assert want.min() > 0
    rel = np.abs(g["rgb"] - want) / want
    face = ns.lamp_closed_form(ns.plane_points(pkg, g["x"], g["y"]), normal=(0.0, 0.0, -1.0))
    print("lamp %s: max rel err %.3g over %d points (against the face normal's value: %.3g)" % (env, rel.max(), len(want), (np.abs(g["rgb"] - face) / face).max()))
    assert rel.max() < 1e-4, rel.max()
    assert np.all(g["n_dims"] == 6)
    flipped = _eval(pkg, ns.lamp_lit_plane(pkg, normal=-ns.LAMP_NORMAL), env)
    assert np.all(flipped["rgb"] == 0)


@pytest.mark.parametrize("sign", [-1.0, 1.0], ids=["minus-x", "plus-x"])
def test_smooth_emitter_with_an_axis_aligned_normal(pkg, native_lib, sign):
    """A light beside the view whose vertex normals are exactly (-1, 0, 0): a normal on a coordinate axis is as good as any other
    (the light's normal is built without a tangent). Same closed form and bound, for eval_paths and -- under
    test_point_lit_plane_matches_the_closed_form's protocol -- for render_direct; with (+1, 0, 0) the light faces away: all 0."""
    nl, c = sign * ns.SIDE_LAMP_NORMAL * -1.0 if sign > 0 else ns.SIDE_LAMP_NORMAL, ns.SIDE_LAMP_CENTRE
    sd = ns.lamp_lit_plane(pkg, normal=nl, centre=c)
    g = _eval(pkg, sd, FLAT)
    K = 32
    with pkg.Context(gd._cfg(pkg), sd) as ctx:
        imgs = np.array([ctx.render_direct(4, seed=100 + k) for k in range(K)], dtype=np.float64)
    if sign > 0:
        assert np.all(g["rgb"] == 0) and np.all(imgs == 0)
        return
    want = ns.lamp_closed_form(ns.plane_points(pkg, g["x"], g["y"]), nl, c)
    assert want.min() > 0
    rel = np.abs(g["rgb"] - want) / want
    pix = ns.lamp_pixels_closed_form(pkg, ns.FOV, normal=nl, centre=c)
    mean, se = imgs.mean(axis=0), imgs.std(axis=0, ddof=1) / np.sqrt(K)
    z = np.abs(mean - pix) / se
    off = abs(mean.mean() - pix.mean()) / pix.mean()
    print("side lamp: eval_paths max rel err %.3g; direct pass max z %.2f, image mean off by %.3g relative" % (rel.max(), z.max(), off))
    assert rel.max() < 1e-4, rel.max()
    assert np.all(se > 0) and z.max() < 6 and off < 1e-3, (z.max(), off)


def test_direct_pass_of_the_smooth_emitter_matches_the_closed_form(pkg, native_lib):
    """render_direct of the same scene under test_point_lit_plane_matches_the_closed_form's protocol: K = 32 seeds against the
    closed form on a 16 x 16 sub-pixel grid, every pixel within 6 of its measured standard error, the image mean within 1e-3.
    Measured on the MI355X: max z 4.66, image mean off by 1.9e-07 relative."""
    K, fov = 32, 40.0
    with pkg.Context(gd._cfg(pkg), ns.lamp_lit_plane(pkg, fov=fov)) as ctx:
        imgs = np.array([ctx.render_direct(4, seed=100 + k) for k in range(K)], dtype=np.float64)
        with pkg.Context(gd._cfg(pkg), ns.lamp_lit_plane(pkg, normal=-ns.LAMP_NORMAL, fov=fov)) as dark:
            assert np.all(dark.render_direct(4, seed=100) == 0)
    want = ns.lamp_pixels_closed_form(pkg, fov)
    mean, se = imgs.mean(axis=0), imgs.std(axis=0, ddof=1) / np.sqrt(K)
    z = np.abs(mean - want) / se
    rel = abs(mean.mean() - want.mean()) / want.mean()
    print("lamp, direct pass: max z %.2f, image mean off by %.3g relative, median rel se %.3g" % (z.max(), rel, np.median(se / want)))
    assert np.all(se > 0) and z.max() < 6, z.max()
    assert rel < 1e-3, rel


# ---------------------------------------------------------------- 4. face-normal twins against the oracle
TWINS = {
    "triangle_soup": lambda pkg, res=64: ns.face_normal_twin(pkg, pkg.scenes.triangle_soup(600, res)),
    "door_c3": lambda pkg, res=64: ns.face_normal_twin(pkg, pkg.scenes.door_c3(res)),
    "glass_sphere": lambda pkg, res=64: ns.face_normal_twin(pkg, pkg.scenes.glass_sphere(res)),
}


@pytest.mark.parametrize("name", list(TWINS))
def test_face_normal_twin_eval_paths_match_the_oracle(pkg, ob, native_lib, name):
    """Every triangle carries vertex normals equal to its face normal (the rectangles as triangle pairs, so every hit but a sphere's
    takes the smooth branch, the light samples too); the oracle never reads normals. test_eval_paths_matches_oracle's bounds."""
    sd = TWINS[name](pkg)
    assert len(sd.normals) == sum(s.type == pkg.abi.SHAPE_TRIANGLE for s in sd.shapes) >= 12
    cfg, ctx, orc = ep.make(pkg, ob, sd, type="orbital", work_units=64)
    u = np.random.default_rng(1).random((8192, 50), dtype=np.float32)
    g, o = ctx.eval_paths(u), orc.eval_paths(u)
    ctx.close(), orc.close()
    same = g["n_dims"] == o["n_dims"]
    rel = np.abs(g["luminance"] - o["luminance"])[same] / np.maximum(o["luminance"][same], 1e-3)
    print("twin %s: same topology %.5f, q99 rel %.3g, mean device %.6g oracle %.6g, lit %.3f"
          % (name, same.mean(), np.quantile(rel, 0.99), g["luminance"].mean(), o["luminance"].mean(), (o["luminance"] > 0).mean()))
    assert same.mean() >= 0.995, same.mean()
    assert np.all(g["n_rays"][same] <= o["n_rays"][same])
    assert np.allclose(g["x"], o["x"], atol=1e-3) and np.allclose(g["y"], o["y"], atol=1e-3)
    assert np.quantile(rel, 0.99) < 1e-3, np.quantile(rel, 0.99)
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert np.allclose(g["rgb"][same], o["rgb"][same], rtol=5e-2, atol=1e-3)
    assert (o["luminance"] > 0).mean() > 0.02                  # (door_c3's light is behind the partition: 5 % of the points carry light)


def test_mirror_room_twin_matches_its_faceted_self_on_the_device(pkg, native_lib):
    """mirror_room's floor is a smooth conductor, which the oracle does not have (it refuses the BSDF; test_gpu_conductor.py holds
    the device to its rough conductor's limit instead). Its twin is therefore held to the device's own f(u) on the same triangles
    without their vertex normals -- flat records, code that predates the normals -- under the same bounds. (Not to the room of
    rectangles: the triangle (a, c, d) has its tangent along the diagonal, so the same u is another path there.)"""
    tw = ns.face_normal_twin(pkg, pkg.scenes.mirror_room(64))
    sd = ns.faceted(pkg, tw)
    assert len(tw.normals) == 14 and len(tw.emitters) == 2 and not sd.normals and all(s.normals == 0 for s in sd.shapes)
    cfg = pkg.abi.make_config(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1, luminance_samples=20000, work_units=64)
    u = np.random.default_rng(1).random((8192, 50), dtype=np.float32)
    with pkg.Context(cfg, tw) as a, pkg.Context(cfg, sd) as b:
        g, o = a.eval_paths(u), b.eval_paths(u)
    same = g["n_dims"] == o["n_dims"]
    rel = np.abs(g["luminance"] - o["luminance"])[same] / np.maximum(o["luminance"][same], 1e-3)
    print("twin mirror_room against its faceted self: same topology %.5f, q99 rel %.3g, mean twin %.6g faceted %.6g, lit %.3f"
          % (same.mean(), np.quantile(rel, 0.99), g["luminance"].mean(), o["luminance"].mean(), (o["luminance"] > 0).mean()))
    assert same.mean() >= 0.995, same.mean()
    assert np.all(g["n_rays"][same] == o["n_rays"][same])
    assert np.allclose(g["x"], o["x"], atol=1e-3) and np.allclose(g["y"], o["y"], atol=1e-3)
    assert np.quantile(rel, 0.99) < 1e-3, np.quantile(rel, 0.99)
    assert g["luminance"].mean() == pytest.approx(o["luminance"].mean(), rel=5e-3)
    assert np.allclose(g["rgb"][same], o["rgb"][same], rtol=5e-2, atol=1e-3)
    assert (o["luminance"] > 0).mean() > 0.2


@pytest.fixture
def twins_as_emitter_scenes(monkeypatch):
    """The protocols of test_gpu_emitter_parity.py take their scenes by name from emitter_scenes.EMITTER_SCENES, and the replay
    protocol expects a BVH under the name "soup" and the flat loop under "mixed": for the duration of a test those names stand for
    the soup's twin (605 records, traversed) and door_c3's (18 triangles and no other shape, brute force; rough-conductor floor)."""
    monkeypatch.setitem(es.EMITTER_SCENES, "soup", lambda pkg: TWINS["triangle_soup"](pkg, 32))
    monkeypatch.setitem(es.EMITTER_SCENES, "mixed", lambda pkg: TWINS["door_c3"](pkg, 32))


@pytest.mark.parametrize("kw", ep.CHAIN_VARIANTS, ids=lambda k: "-".join("%s=%s" % i for i in k.items()))
@pytest.mark.parametrize("scene", ["mixed", "soup"], ids=["door_c3", "triangle_soup"])
def test_face_normal_twin_chains_track_the_oracle(pkg, ob, native_lib, twins_as_emitter_scenes, scene, kw):
    ep.test_chains_track_the_oracle(pkg, ob, native_lib, scene, kw)


@pytest.mark.parametrize("scene", ["mixed", "soup"], ids=["door_c3", "triangle_soup"])
@pytest.mark.parametrize("build", ep.BUILDS, ids=[b[0] for b in ep.BUILDS])
def test_face_normal_twin_chain_kernel_builds_replay_against_the_oracle(pkg, ob, native_lib, capfd, twins_as_emitter_scenes, scene, build):
    ep.test_chain_kernel_builds_replay_against_the_oracle(pkg, ob, native_lib, capfd, scene, build)


# ---------------------------------------------------------------- 5. genuinely smooth chains, across builds
SMOOTH = {"smooth_room": lambda pkg: pkg.scenes.smooth_room(32, 1), "smooth_soup": lambda pkg: pkg.scenes.triangle_soup(600, 32, smooth=True)}
# test_gpu_conductor.BUILDS as the scene's own plan runs them (both scenes are traversed), the same with the BVH forced (what the
# issue asks for), and -- smooth_room's 87 records -- in the brute-force loop: the builds without bit 8
BUILD_GROUPS = [("own", {}), ("bvh", BVH), ("flat", FLAT)]


# (the soup's 605 records in the brute-force loop are not a build the plan ever picks)
BUILD_CASES = [(n, g) for n in SMOOTH for g in BUILD_GROUPS if not (n == "smooth_soup" and g[0] == "flat")]


@pytest.mark.parametrize("kw", [dict(type="orbital"), dict(type="green"), dict(type="mira")], ids=lambda k: k["type"])
@pytest.mark.parametrize("name,group", BUILD_CASES, ids=["%s-%s" % (n, g[0]) for n, g in BUILD_CASES])
def test_smooth_chains_are_the_same_across_kernel_builds(pkg, native_lib, name, group, kw):
    """test_mirror_room_chains_are_the_same_across_kernel_builds' comparisons: chains, counters and film of every build equal v3's."""
    gid, extra = group
    sd = SMOOTH[name](pkg)
    n_chains, n_mut = 1000, 60
    cfg = pkg.abi.make_config(max_depth=8, direct_samples=-1, luminance_samples=20000, work_units=n_chains, sample_count=1, **kw)
    results = []
    for env in gc.BUILDS:
        ctx = gc._ctx_with_env(pkg, cfg, sd, **dict(env, **extra))
        ctx.seed(0x5005)
        ctx.run(n_chains * n_mut)
        results.append((ctx.chain_state(34), ctx.stats(), ctx.film()))
        ctx.close()
    (c0, u0), s0, f0 = results[0]
    assert s0.mutations == n_chains * n_mut and s0.accepted > 0
    assert (s0.bvh_node_visits > 0 or results[1][1].bvh_node_visits > 0) == (gid != "flat")
    for env, ((c, u), s, f) in zip(gc.BUILDS[1:], results[1:]):
        assert np.array_equal(u, u0) and np.array_equal(c["luminance"], c0["luminance"]), env
        for k in ("first", "large", "bold", "second", "second_large", "second_bold", "overall"):
            assert getattr(s, k + "_base") == getattr(s0, k + "_base") and getattr(s, k + "_acc") == getattr(s0, k + "_acc"), (env, k)
        assert s.rays == s0.rays and s.path_evals == s0.path_evals and s.accepted == s0.accepted, env
        assert lum(f).sum() == pytest.approx(lum(f0).sum(), rel=1e-5)
        assert np.abs(lum(f) - lum(f0)).sum() / lum(f0).sum() < 1e-4


# ---------------------------------------------------------------- 6. images
BASE = gc.BASE
SPHERE = ((0.0, -0.65, -0.4), 0.35)     # scenes.smooth_room


@pytest.fixture(scope="module")
def room_refs(pkg, native_lib):
    """render_pt of smooth_room(32, 1) and of its faceted twin: K = 8 independent images of 8 192 spp a side."""
    out = {}
    for smooth in (True, False):
        with pkg.Context(pkg.abi.make_config(work_units=64, **BASE), pkg.scenes.smooth_room(32, 1, smooth=smooth)) as ctx:
            out[smooth] = np.array([ctx.render_pt(8192, seed=5 + k) for k in range(8)], dtype=np.float64)
    return out


def test_smooth_and_faceted_room_images_match_path_tracing(pkg, native_lib, room_refs):
    """drmlt and pssmlt images of smooth_room(32, 1) and of its faceted twin against render_pt at 8 192 spp, the bounds of
    test_mirror_room_path_image_matches_path_tracing. The faceted twin runs code that predates the vertex normals: it has to meet
    the bounds with a factor 2 to spare (b and the rel MSE), else the scene is too hard for them, not the feature wrong. And the two
    path-traced images differ by more than 10 standard errors on blocks the sphere covers: ignored normals cannot pass. The blocks
    are 2 x 2 pixels (a facet of the 80 is some 3 pixels wide, and over larger blocks brighter and darker facets cancel: 4 x 4
    blocks at 8 x 1024 spp measured 5.6 standard errors), the error that of K = 8 images of 8 192 spp a side.
    Measured on the MI355X: rel MSE faceted 0.0023 (drmlt) / 0.0020 (pssmlt), smooth 0.0022 / 0.0021; b off by 3.6e-4 / 2.4e-4; 24 blocks inside
    the sphere, z there median 9.3, max 46.5 (elsewhere: median 0.3)."""
    abi, spp = pkg.abi, 2048
    refs = {k: v[0] for k, v in room_refs.items()}           # 8 192 spp
    for smooth in (False, True):
        ref = refs[smooth]
        for algo in ("drmlt", "pssmlt"):
            extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
            ctx = pkg.Context(abi.make_config(work_units=4096, sample_count=spp, luminance_samples=200000, **BASE, **extra), pkg.scenes.smooth_room(32, 1, smooth=smooth))
            b = ctx.seed(9)
            ctx.run(32 * 32 * spp)
            img = ctx.develop()
            ctx.close()
            err = rel_mse(img, ref)
            print("%s room %s: b %.6g, render_pt mean %.6g (off by %.3g), rel MSE %.3g" % ("smooth" if smooth else "faceted", algo, b, lum(ref).mean(), abs(b / lum(ref).mean() - 1), err))
            spare = 1.0 if smooth else 0.5
            assert b == pytest.approx(lum(ref).mean(), rel=0.02 * spare)
            assert lum(img).mean() == pytest.approx(b, rel=1e-3)
            assert err < 1e-2 * spare, err
    # the two references on the sphere's blocks
    blocks = lambda a: lum(a).reshape(-1, 16, 2, 16, 2).mean(axis=(2, 4))
    bs, bf = blocks(room_refs[True]), blocks(room_refs[False])
    se = np.sqrt(bs.var(axis=0, ddof=1) / len(bs) + bf.var(axis=0, ddof=1) / len(bf))
    z = np.abs(bs.mean(axis=0) - bf.mean(axis=0)) / se
    mask = ds.sphere_mask(pkg, pkg.scenes.smooth_room(32, 1), *SPHERE, grow=0.9).reshape(16, 2, 16, 2).all(axis=(1, 3))
    print("smooth vs faceted render_pt: %d blocks inside the sphere, z there min %.1f median %.1f max %.1f; elsewhere median %.1f"
          % (mask.sum(), z[mask].min(), np.median(z[mask]), z[mask].max(), np.median(z[~mask])))
    assert mask.sum() >= 16 and z[mask].max() > 10 and np.median(z[mask]) > 5, z[mask]   # not one lucky block: the typical one differs too


def test_smooth_room_direct_image_matches_the_devices_path_tracer(pkg, native_lib):
    """render_direct against the device's own render_pt at maxDepth 2, test_gpu_direct._hold_blocks' protocol and bounds (the smooth
    branches of device_direct.h against those of path_step). Measured on the MI355X: max z 2.06, max rel se 0.0022."""
    sd = pkg.scenes.smooth_room(32, 1)
    K = 16
    with pkg.Context(gd._cfg(pkg, max_depth=2, rr_depth=100, direct_samples=-1), sd) as ctx:
        bg = np.array([gd._blocks(gd._direct_image(ctx, 100 + k)) for k in range(K)])
        bp = np.array([gd._blocks(ctx.render_pt(1024, seed=300 + k)) for k in range(K)])
    gd._hold_blocks("render_direct smooth_room vs render_pt", bg, bp)


def test_a_node_develops_the_contexts_smooth_image(pkg, native_lib):
    """Node(mask = 1) runs the chains of a Context with the same seed: the same image (test_single_device_node_is_the_plain_context)."""
    sd = pkg.scenes.smooth_room(32, 1)
    cfg = pkg.abi.make_config(work_units=1024, sample_count=64, luminance_samples=20000, **BASE)
    with pkg.Context(cfg, sd) as ctx:
        ba = ctx.seed_pool(0x5EED, 0, 1024)          # a node draws its ranks' seeds from one pool
        ctx.run(32 * 32 * 64)
        a = ctx.develop()
    node = pkg.Node(cfg, sd, device_mask=1)
    bb = node.seed(0x5EED)
    node.run(32 * 32 * 64)
    b = node.develop()
    node.close()
    assert ba == bb and lum(a).mean() > 0
    np.testing.assert_allclose(b, a, rtol=2e-4, atol=1e-6)   # test_single_device_node_is_the_plain_context's
