"""Vertex normals of triangle meshes (technique=path) at the C-ABI and on the host, without a GPU: the header and its ctypes
mirror agree, drmlt_create takes the three scene layouts and refuses what it cannot render before it looks for a device, the
scene file carries the normals, prepare_scene keeps a smooth triangle out of every merged record, the kernels' own frame routine
(csrc/smooth_frame.h, run on the CPU) reproduces the reference's formulas, and the Mitsuba adaptor hands the normals through."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
PRIM_TRIANGLE, PRIM_RECTANGLE, PRIM_QUAD2, PRIM_SMOOTH = 0, 1, 3, 6   # csrc/device_types.h


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _run_c(src, lang="c"):
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "t." + ("c" if lang == "c" else "cpp"))
        open(path, "w").write(src)
        exe = os.path.join(d, "t")
        cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
        subprocess.check_call(cc + ["-I", INCLUDE, path, "-o", exe])
        return subprocess.check_output([exe]).decode().split()


def test_header_and_mirror_agree_on_vertex_normals(abi):
    out = _run_c(r'''
#include <stdio.h>
#include <stddef.h>
#include "drmlt_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", offsetof(drmlt_shape, normals), sizeof(drmlt_shape), offsetof(drmlt_scene, n_normals),
         offsetof(drmlt_scene, normals), sizeof(drmlt_scene), (size_t) DRMLT_SCENE_SIZE_NO_NORMALS, (size_t) DRMLT_SCENE_SIZE_NO_POINTS,
         offsetof(drmlt_scene, points), (int) DRMLT_ABI_VERSION);
  return 0; }
''')
    assert [int(v) for v in out] == [abi.Shape.normals.offset, C.sizeof(abi.Shape), abi.Scene.n_normals.offset, abi.Scene.normals.offset,
                                     C.sizeof(abi.Scene), abi.SCENE_SIZE_NO_NORMALS, abi.SCENE_SIZE_NO_POINTS, abi.Scene.points.offset,
                                     abi.ABI_VERSION]
    # the field takes the place of `reserved`; the new fields trail `points`; the version and the older sizes stay what they were
    assert abi.Shape.normals.offset == 12 and C.sizeof(abi.Shape) == 64 and abi.ABI_VERSION == 4
    assert abi.SCENE_SIZE_NO_POINTS < abi.SCENE_SIZE_NO_NORMALS < C.sizeof(abi.Scene)
    assert abi.SCENE_SIZE_NO_NORMALS == abi.Scene.points.offset + C.sizeof(C.c_void_p) == abi.Scene.n_normals.offset


def _tilted_floor(pkg, normals=((0.1, 0.0, 1.0), (0.0, 0.2, 2.0), (-0.1, 0.0, 0.5))):
    """cornell_c1 plus one smooth triangle."""
    sd = pkg.scenes.cornell_c1(8)
    sd.triangle((-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0), 0, normals=normals)
    return sd


def _refusal(pkg, cfg, sd):
    with pytest.raises(pkg.DrmltError) as e:
        pkg.Context(cfg, sd)
    return str(e.value)


def _create_raw(pkg, abi, sd, struct_size, **cfg_kw):
    L = pkg.binding.load_library()
    s = sd.struct()
    s.struct_size = struct_size
    cfg = abi.make_config(type="orbital", max_depth=8, **cfg_kw)
    err = C.create_string_buffer(512)
    h = L.drmlt_create(C.byref(cfg), C.byref(s), 0, err, 512)
    if h:
        L.drmlt_destroy(h)
    return bool(h), err.value.decode()


def test_the_three_scene_layouts_are_accepted_and_their_neighbours_are_not(pkg, abi, native_lib):
    sd = pkg.scenes.cornell_c1(8)
    sizes = (abi.SCENE_SIZE_NO_POINTS, abi.SCENE_SIZE_NO_NORMALS, C.sizeof(abi.Scene))
    for size in sizes:
        ok, msg = _create_raw(pkg, abi, sd, size)
        assert "struct_size" not in msg, (size, msg)
        if not _has_gpu():
            assert not ok and "no HIP device" in msg, (size, msg)
    for size in sizes:
        for bad in (size - 8, size + 4, size + 8):
            if bad in sizes:
                continue
            ok, msg = _create_raw(pkg, abi, sd, bad)
            assert not ok and "struct_size mismatch" in msg, (bad, msg)
    # with either older size the per-shape field is not read: to those callers it is `reserved`, whatever it holds
    sd = pkg.scenes.cornell_c1(8)
    sd.shapes[0].normals = 12345
    for size in sizes[:2]:
        ok, msg = _create_raw(pkg, abi, sd, size)
        assert "vertex" not in msg and "struct_size" not in msg, (size, msg)
        assert ok == _has_gpu(), (size, msg)
    ok, msg = _create_raw(pkg, abi, sd, sizes[2])
    assert not ok and "vertex normals on a rectangle" in msg, msg
    # ... and the table is not read either: a smooth scene handed over in the older layout is the faceted one
    ok, msg = _create_raw(pkg, abi, _tilted_floor(pkg), abi.SCENE_SIZE_NO_NORMALS)
    assert "vertex" not in msg and ok == _has_gpu(), msg


def test_create_refuses_what_vertex_normals_cannot_be(pkg, abi, native_lib):
    cfg = abi.make_config(type="orbital", max_depth=8)
    sd = _tilted_floor(pkg)
    sd.shapes[-1].normals = 2                          # only one entry
    assert "out of range (n_normals = 1" in _refusal(pkg, cfg, sd)
    sd = _tilted_floor(pkg)
    sd.shapes[-1].normals = -1
    assert "out of range" in _refusal(pkg, cfg, sd)
    sd = _tilted_floor(pkg)
    sd.shapes[0].normals = 1                           # a rectangle
    assert "vertex normals on a rectangle" in _refusal(pkg, cfg, sd)
    sd = pkg.scenes.glass_sphere(8)
    sd.triangle((-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.0, 0.5, 0.0), 0, normals=np.eye(3))
    sphere = [i for i, s in enumerate(sd.shapes) if s.type == abi.SHAPE_SPHERE][0]
    sd.shapes[sphere].normals = 1
    assert "vertex normals on a sphere" in _refusal(pkg, cfg, sd)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for slot in (0, 4, 8):
            vn = np.array([[0.1, 0.0, 1.0], [0.0, 0.2, 2.0], [-0.1, 0.0, 0.5]])
            vn.reshape(-1)[slot] = bad
            assert "vertex normal is not finite" in _refusal(pkg, cfg, _tilted_floor(pkg, vn))
    # what passes: the refusals above come from the scene, not from the feature
    if _has_gpu():
        pkg.Context(cfg, _tilted_floor(pkg)).close()
    else:
        assert "no HIP device" in _refusal(pkg, cfg, _tilted_floor(pkg))
        assert "no HIP device" in _refusal(pkg, abi.make_config(algo=abi.ALGO_PSSMLT, type="orbital", max_depth=8), _tilted_floor(pkg))


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
def test_vertex_normals_are_for_technique_path_only(pkg, abi, native_lib, technique):
    cfg = abi.make_config(type="orbital", technique=technique, max_depth=6)
    msg = _refusal(pkg, cfg, _tilted_floor(pkg))
    assert "technique=path only" in msg and "geometric normal" in msg and "adjoint" in msg, msg
    # the same scene without the normals is not refused for them
    sd = _tilted_floor(pkg)
    sd.shapes[-1].normals = 0
    if not _has_gpu():
        assert "no HIP device" in _refusal(pkg, cfg, sd)


def test_scene_file_without_normals_keeps_its_bytes(pkg, abi, tmp_path):
    for sd in (pkg.scenes.cornell_c2(16), pkg.scenes.cornell_point(16, quad_light=True)):
        path = str(tmp_path / "plain.drmlt")
        sd.save(path)
        want = 32 + len(sd.shapes) * C.sizeof(abi.Shape) + len(sd.bsdfs) * C.sizeof(abi.Bsdf) + \
            len(sd.emitters) * C.sizeof(abi.Emitter) + C.sizeof(abi.Camera) + ((8 + 12 * len(sd.points)) if sd.points else 0)
        data = open(path, "rb").read()
        assert len(data) == want and b"NRMS" not in data
    # the faceted twin of a smooth scene is byte for byte the smooth one without the block and the per-shape indices
    a, b = pkg.scenes.smooth_room(8, 0, smooth=False), pkg.scenes.smooth_room(8, 0)
    pa, pb = str(tmp_path / "a.drmlt"), str(tmp_path / "b.drmlt")
    a.save(pa)
    b.save(pb)
    da, db = open(pa, "rb").read(), open(pb, "rb").read()
    assert len(db) == len(da) + 8 + 36 * len(b.normals) and len(b.normals) == 20
    assert db[len(da):len(da) + 4] == b"NRMS"


def test_scene_file_round_trips_normals(pkg, abi, tmp_path):
    hpp = os.path.join(HOST, "drmlt_integrator.hpp")
    prog = r'''
#include "%s"
#include <cstdio>
int main() {
  drmlt_host::SceneFile sf = drmlt_host::SceneFile::load("%s");
  drmlt_scene s = sf.view();
  printf("%%d %%d %%d %%d\n", s.n_shapes, s.n_points, s.n_normals, (int) s.struct_size);
  for (int i = 0; i < s.n_shapes; ++i) printf("%%d\n", s.shapes[i].normals);
  for (int i = 0; i < 3 * s.n_points; ++i) printf("%%.9g\n", s.points[i]);
  for (int i = 0; i < 9 * s.n_normals; ++i) printf("%%.9g\n", s.normals[i]);
  return 0; }
'''
    for with_points in (False, True):
        sd = pkg.scenes.triangle_soup(7, 8, smooth=True)
        sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0)   # one faceted triangle among them
        if with_points:
            sd.point_light((0.25, -0.125, 0.5), intensity=(1.0, 2.0, 3.0))
        path = str(tmp_path / ("soup%d.drmlt" % with_points))
        sd.save(path)
        out = _run_c(prog % (hpp, path), lang="c++")
        assert [int(v) for v in out[:4]] == [len(sd.shapes), len(sd.points), 7, C.sizeof(abi.Scene)]
        idx = [int(v) for v in out[4:4 + len(sd.shapes)]]
        assert idx == [s.normals for s in sd.shapes] and sorted(i for i in idx if i) == list(range(1, 8)) and idx[-2] == 0
        rest = np.array([float(v) for v in out[4 + len(sd.shapes):]], dtype=np.float32)
        assert np.array_equal(rest[:3 * len(sd.points)], np.asarray(sd.points, dtype=np.float32).reshape(-1))
        assert np.array_equal(rest[3 * len(sd.points):], np.asarray(sd.normals, dtype=np.float32).reshape(-1))
    # a block the loader does not know, or a second block of normals, is a malformed file
    data = open(path, "rb").read()
    for tail in (b"XXXX\x00\x00\x00\x00", b"NRMS\x00\x00\x00\x00"):
        bad = str(tmp_path / "bad.drmlt")
        open(bad, "wb").write(data + tail)
        with pytest.raises(subprocess.CalledProcessError):
            _run_c(prog % (hpp, bad), lang="c++")


def test_triangle_soup_keeps_its_geometry_under_the_smooth_flag(pkg):
    a, b = pkg.scenes.triangle_soup(50, 8), pkg.scenes.triangle_soup(50, 8, smooth=True)
    assert [bytes(s.data) for s in a.shapes] == [bytes(s.data) for s in b.shapes]
    assert not a.normals and len(b.normals) == 50
    vn = np.asarray(b.normals).reshape(50, 3, 3)
    tri = np.array([list(s.data)[:9] for s in b.shapes if s.normals], dtype=np.float64).reshape(50, 3, 3)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    cos = np.einsum("tvk,tk->tv", vn, fn) / np.linalg.norm(vn, axis=2)
    assert cos.min() > 0.71 and cos.max() < 1.0                      # jittered about the face normal: |jitter| <= 0.4 sqrt(3) < 0.7 = sin 44 deg ...
    assert np.abs(np.linalg.norm(vn, axis=2) - 1.0).max() > 0.3      # ... and not normalised


def test_icosphere_is_closed_outward_and_radial(pkg):
    for level, faces in ((0, 20), (1, 80), (2, 320)):
        v, f = pkg.scenes.icosphere(level)
        assert len(f) == faces and len(v) == faces // 2 + 2          # Euler: V - 3F/2 + F = 2
        assert np.abs(np.linalg.norm(v, axis=1) - 1.0).max() < 1e-12
        fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        assert (np.einsum("fk,fk->f", fn, v[f].mean(axis=1)) > 0).all()
        edges = {}
        for a, b, c in f:
            for e in ((a, b), (b, c), (c, a)):
                edges[e] = edges.get(e, 0) + 1
        assert all(n == 1 for n in edges.values()) and all((b, a) in edges for a, b in edges)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    subprocess.run(["make", "-C", HOST, "normals_harness"], check=True, capture_output=True)
    exe = os.path.join(HOST, "normals_harness")
    d = tmp_path_factory.mktemp("normals")
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}

    def run(sd, uv=None, **kw):
        path = str(d / "scene.drmlt")
        sd.save(path)
        args = [exe, "scene=" + path] + ["%s=%s" % kv for kv in kw.items()]
        out = None
        if uv is not None:
            np.asarray(uv, dtype="<f4").tofile(str(d / "uv.bin"))
            args += ["uv=" + str(d / "uv.bin"), "out=" + str(d / "out.bin")]
        r = subprocess.run(args, check=True, capture_output=True, text=True, env=env)
        if uv is not None:
            out = np.fromfile(str(d / "out.bin"), dtype="<f4").reshape(-1, 9)
        return json.loads(r.stdout), out
    return run


def test_prepare_scene_sets_the_feature_bit_and_refuses_on_the_cpu(pkg, abi, harness):
    plain, _ = harness(pkg.scenes.cornell_c1(8))
    assert plain["refusal"] == "" and plain["features"] & 4 == 0 and plain["n_normals"] == 0
    res, _ = harness(_tilted_floor(pkg))
    assert res["refusal"] == "" and res["features"] & 4 == 4 and res["n_normals"] == 1
    assert res["shade_kinds"][-1] == PRIM_SMOOTH and res["prim_kinds"].count(PRIM_TRIANGLE) == 1
    assert res["lds_table_bytes"] == plain["lds_table_bytes"] + 64     # one more shading record, nothing for the table
    for technique in (abi.TECH_BDPT, abi.TECH_MMLT):
        res, _ = harness(_tilted_floor(pkg), technique=technique)
        assert "technique=path only" in res["refusal"] and "geometric normal" in res["refusal"]
    sd = _tilted_floor(pkg)
    sd.shapes[-1].normals = 5
    assert "out of range" in harness(sd)[0]["refusal"]
    # a scene whose one light is a smooth triangle is not a one-light scene for the scalar-register builds
    sd = pkg.scenes.SceneData("lamp")
    grey = sd.diffuse(0.5)
    sd.rectangle(np.eye(4), grey)
    sd.set_camera(pkg.scenes.lookat((0, 0, 3), (0, 0, 0), (0, 1, 0)), 40.0, 8, 8)
    sd.triangle((-0.5, -0.5, 2), (0, 0.5, 2), (0.5, -0.5, 2), grey, radiance=1.0)
    assert harness(sd)[0]["one_light"] == 1
    sd.shapes[-1].normals = 1
    sd.normals.append((0, 0, -1) * 3)
    res, _ = harness(sd)
    assert res["refusal"] == "" and res["one_light"] == 0 and res["features"] & 4


def test_a_coplanar_smooth_pair_is_neither_a_quad_nor_a_cuboid_face(pkg, harness):
    """cornell_c2's two boxes are twelve triangle pairs: six merged pairs each, both cuboids. With vertex normals on the pairs of
    one box they stay twelve single triangles, and only the other box and the room remain cuboids."""
    def scene(smooth_box):
        sd = pkg.scenes.cornell_c2(8)
        tris = [i for i, s in enumerate(sd.shapes) if s.type == pkg.abi.SHAPE_TRIANGLE]
        assert len(tris) == 24
        for i in tris[:12] if smooth_box else []:
            d = np.array(list(sd.shapes[i].data)[:9]).reshape(3, 3)
            fn = np.cross(d[1] - d[0], d[2] - d[0])
            sd.normals.append(tuple(np.tile(fn / np.linalg.norm(fn), 3)))
            sd.shapes[i].normals = len(sd.normals)
        return sd
    base, _ = harness(scene(False))
    assert base["refusal"] == "" and base["prim_kinds"].count(PRIM_QUAD2) == 12 and base["prim_kinds"].count(PRIM_TRIANGLE) == 0
    res, _ = harness(scene(True))
    assert res["refusal"] == "" and res["features"] & 4
    assert res["prim_kinds"].count(PRIM_QUAD2) == 6 and res["prim_kinds"].count(PRIM_TRIANGLE) == 12
    assert res["shade_kinds"].count(PRIM_SMOOTH) == 12
    assert res["n_box"] == base["n_box"] - 1 and res["n_flat_rec"] == base["n_flat_rec"] + 12
    # ... and under the BVH (no flat loop, no cuboids) the pairs stay apart as well
    res, _ = harness(scene(True), DRMLT_BVH_THRESHOLD=0)
    assert res["use_bvh"] == 1 and res["prim_kinds"].count(PRIM_QUAD2) == 6 and res["prim_kinds"].count(PRIM_TRIANGLE) == 12


def test_the_frame_routine_matches_the_reference_formulas(pkg, harness):
    """1000 random triangles, each with three unnormalised vertex normals, each at one random (u, v): the frame the kernels'
    routine builds from the PREPARED tables against skdtree.h:355-396 / util.cpp:610-616 in fp64, to 1e-6, and orthonormal to 1e-6.
    The cases: edges of length 0.05 .. 2, positions within +-10; vertex normals within 45 degrees of the face normal (a mesh's
    normals follow its surface), lengths 0.25 .. 4. dpdu lies in the face, so the angle between n and dpdu stays above 45 degrees and
    the Gram-Schmidt step loses at most a factor sqrt(2): what is left is fp32 rounding of ten-odd operations, 1e-7 each."""
    rng = np.random.default_rng(11)
    n = 1000
    sd = pkg.scenes.cornell_c1(8)
    first = len(sd.shapes)
    p0 = rng.uniform(-10, 10, (n, 3))
    e1 = rng.normal(size=(n, 3))
    e1 *= (rng.uniform(0.05, 2.0, n) / np.linalg.norm(e1, axis=1))[:, None]
    e2 = rng.normal(size=(n, 3))
    e2 -= e1 * (np.einsum("nk,nk->n", e1, e2) / np.einsum("nk,nk->n", e1, e1))[:, None] * rng.uniform(0.0, 0.9, n)[:, None]
    e2 *= (rng.uniform(0.05, 2.0, n) / np.linalg.norm(e2, axis=1))[:, None]
    fn = np.cross(e1, e2)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    vn = np.empty((n, 3, 3))
    for k in range(3):
        d = rng.normal(size=(n, 3))
        d -= fn * np.einsum("nk,nk->n", d, fn)[:, None]
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        ang = rng.uniform(0.0, np.pi / 4, n)
        vn[:, k] = (fn * np.cos(ang)[:, None] + d * np.sin(ang)[:, None]) * rng.uniform(0.25, 4.0, n)[:, None]
    for i in range(n):
        sd.triangle(p0[i], p0[i] + e1[i], p0[i] + e2[i], 0, normals=vn[i])
    u = rng.uniform(0, 1, n)
    v = rng.uniform(0, 1, n) * (1 - u)
    uv = np.zeros((len(sd.shapes), 2), dtype=np.float32)
    uv[first:, 0], uv[first:, 1] = u, v
    res, out = harness(sd, uv=uv)
    assert res["refusal"] == "" and res["n_normals"] == n and res["shade_kinds"][first:first + n] == [PRIM_SMOOTH] * n
    got = out[first:first + n].astype(np.float64)
    # the reference, in fp64, from what the device is given: float32 positions, normals and (u, v)
    tri = np.array([list(s.data)[:9] for s in sd.shapes[first:]], dtype=np.float64).reshape(n, 3, 3)
    vn32 = np.asarray(sd.normals, dtype=np.float32).astype(np.float64).reshape(n, 3, 3)
    u64, v64 = uv[first:, 0].astype(np.float64), uv[first:, 1].astype(np.float64)
    nn = vn32[:, 0] * (1 - u64 - v64)[:, None] + vn32[:, 1] * u64[:, None] + vn32[:, 2] * v64[:, None]
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    dpdu = tri[:, 1] - tri[:, 0]
    ss = dpdu - nn * np.einsum("nk,nk->n", nn, dpdu)[:, None]
    ss /= np.linalg.norm(ss, axis=1, keepdims=True)
    tt = np.cross(nn, ss)
    err = max(np.abs(got[:, 0:3] - nn).max(), np.abs(got[:, 3:6] - ss).max(), np.abs(got[:, 6:9] - tt).max())
    gn, gs, gt = got[:, 0:3], got[:, 3:6], got[:, 6:9]
    dots = lambda a, b: np.einsum("nk,nk->n", a, b)
    ortho = max(np.abs(dots(gn, gn) - 1).max(), np.abs(dots(gs, gs) - 1).max(), np.abs(dots(gt, gt) - 1).max(),
                np.abs(dots(gn, gs)).max(), np.abs(dots(gn, gt)).max(), np.abs(dots(gs, gt)).max())
    print("frame: max |error| %.3g, orthonormality %.3g" % (err, ortho))
    assert err < 1e-6 and ortho < 1e-6, (err, ortho)


def test_a_normal_without_a_direction_gives_the_zero_frame(pkg, harness):
    """Opposite vertex normals cancel on the line between them; a zero table entry cancels everywhere: the routine returns the zero
    frame (the kernels end the path there), never a NaN."""
    sd = pkg.scenes.cornell_c1(8)
    first = len(sd.shapes)
    sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, normals=((0, 0, 1), (0, 0, -1), (0, 0, 1)))
    sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, normals=np.zeros((3, 3)))
    sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0, normals=((1, 0, 0),) * 3)       # parallel to dpdu: no tangent beside it
    uv = np.zeros((len(sd.shapes), 2), dtype=np.float32)
    uv[first] = (0.5, 0.25)
    uv[first + 1] = (0.3, 0.3)
    uv[first + 2] = (0.3, 0.3)
    res, out = harness(sd, uv=uv)
    assert res["refusal"] == "" and np.isfinite(out).all() and (out[first:first + 3] == 0).all()
    uv[first] = (0.25, 0.25)
    _, out = harness(sd, uv=uv)
    assert np.allclose(out[first, :3], (0, 0, 1)) and np.allclose(out[first, 3:6], (1, 0, 0))


@pytest.fixture(scope="module")
def adaptor():
    subprocess.run(["make", "-C", HOST, "normals_adaptor_harness"], check=True, capture_output=True)
    exe = os.path.join(HOST, "normals_adaptor_harness")

    def run(technique, face_normals):
        r = subprocess.run([exe, technique, "1" if face_normals else "0"], check=True, capture_output=True, text=True)
        lines = r.stdout.splitlines()
        shapes = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("shape ")]
        normals = np.array([[float(v) for v in l.split()[1:]] for l in lines if l.startswith("normals ")])
        size = [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith("size ")]
        warnings = [l for l in lines if l.startswith("log ") and "smooth vertex normals are ignored" in l]
        return shapes, normals, size, warnings
    return run


def test_adaptor_hands_vertex_normals_through_under_technique_path(adaptor, abi):
    shapes, normals, size, warnings = adaptor("path", False)
    # (type, emitter, normals) per triangle: the quad's two, then the emitting mesh's one -- mesh emitters included
    assert shapes == [(abi.SHAPE_TRIANGLE, -1, 1), (abi.SHAPE_TRIANGLE, -1, 2), (abi.SHAPE_TRIANGLE, 0, 3)]
    assert size == [(C.sizeof(abi.Scene), 3)] and not warnings
    vq = np.array([(0.125, 0, 1), (0, 0.25, 2), (-0.5, 0, 0.75), (0, -0.375, 1.5)])   # as stored: not normalised
    vl = np.array([(0, 0.0625, -1), (0.03125, 0, -1), (0, 0, -3)])
    want = np.array([vq[[0, 1, 2]].reshape(-1), vq[[2, 3, 0]].reshape(-1), vl[[0, 2, 1]].reshape(-1)])
    assert np.array_equal(normals, want)


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
def test_adaptor_keeps_face_normals_and_the_warning_under_the_bidirectional_techniques(adaptor, abi, technique):
    shapes, normals, size, warnings = adaptor(technique, False)
    assert [s[2] for s in shapes] == [0, 0, 0] and normals.size == 0 and size == [(C.sizeof(abi.Scene), 0)]
    assert len(warnings) == 2 and '"quad"' in warnings[0] and '"lamp"' in warnings[1]


@pytest.mark.parametrize("technique", ["path", "bdpt"])
def test_adaptor_honours_face_normals_true(adaptor, abi, technique):
    shapes, normals, size, warnings = adaptor(technique, True)
    assert [s[2] for s in shapes] == [0, 0, 0] and normals.size == 0 and size == [(C.sizeof(abi.Scene), 0)] and not warnings
