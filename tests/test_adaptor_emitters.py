"""The Mitsuba plugin adaptor on emitters that no shape carries (Mitsuba's `point` and `constant` plugins; every other plugin is
refused) and its directPass property. tests/native/adaptor_emitters_harness.cpp rebuilds a scenes.py scene as Mitsuba objects
-- Scene::getEmitters() included -- and drives the plugin against a recording stand-in for the C-ABI, whose drmlt_node_create
answers with the library's own scene checks (csrc/scene_prep.h). No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden")

BASE = dict(technique="path", type="orbital", maxDepth=8, directSamples=-1, sampleCount=16, workUnits=1024, seed=1234)


def D(**kw):
    out = []
    for k, v in kw.items():
        out += ["-D", "%s=%s" % (k, str(v).lower() if isinstance(v, bool) else v)]
    return out


def run(exe, scene, prefix, *args):
    p = subprocess.run([exe, scene, prefix, *args], capture_output=True, text=True, timeout=120)
    log = [l.rstrip("\n").split("\t", 1) for l in open(prefix + ".log")] if os.path.exists(prefix + ".log") else []
    return p.returncode, [(int(a), b) for a, b in log]


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", HOST, "adaptor_emitters_harness_mock"], check=True, capture_output=True)
    return os.path.join(HOST, "adaptor_emitters_harness_mock")


def scene_a(scenes, res=16):
    return scenes.cornell_point(res, quad_light=True, point_weight=3.0)


def scene_c(scenes, res=16):
    return scenes.cornell_point(res)          # lit by the point light alone


SCENES = {"a_quad_and_point": scene_a, "b_sky": lambda scenes, res=16: scenes.cornell_sky(res), "c_point_only": scene_c}


def f32(values):
    return np.asarray(values, dtype=np.float32).tobytes()


def assert_same_scene(abi, got, want):
    """`got` (a SceneData loaded from what the adaptor handed over) against `want` (the Python scene), through struct(): field by
    field, floats by their bits."""
    g, w = got.struct(), want.struct()
    assert (g.n_shapes, g.n_emitters, g.n_points, g.n_normals) == (w.n_shapes, w.n_emitters, w.n_points, w.n_normals)
    for i in range(w.n_shapes):
        a, b = g.shapes[i], w.shapes[i]
        assert (a.type, a.emitter, a.normals, bytes(a.data)) == (b.type, b.emitter, b.normals, bytes(b.data)), i
        ba, bb = g.bsdfs[a.bsdf], w.bsdfs[b.bsdf]             # the plugin does not share BSDF records between shapes
        assert (ba.type, bytes(ba.rgb), bytes(ba.p)) == (bb.type, bytes(bb.rgb), bytes(bb.p)), i
    for i in range(w.n_shapes - 1):                           # ... but the triangles of one mesh share theirs, which is what lets
        if w.shapes[i].type == w.shapes[i + 1].type == abi.SHAPE_TRIANGLE:   # prepare_scene pair them into parallelograms
            assert (g.shapes[i].bsdf == g.shapes[i + 1].bsdf) == (w.shapes[i].bsdf == w.shapes[i + 1].bsdf), i
    for i in range(w.n_emitters):
        a, b = g.emitters[i], w.emitters[i]
        assert (a.type, a.shape, bytes(a.radiance), f32([a.sampling_weight])) == (b.type, b.shape, bytes(b.radiance), f32([b.sampling_weight])), i
    assert f32(g.points[0:3 * w.n_points]) == f32(w.points[0:3 * w.n_points])
    assert bytes(g.camera) == bytes(w.camera)


def capture(pkg, harness, tmp_path, sd, *args, **props):
    scene = str(tmp_path / "s.bin")
    sd.save(scene)
    prefix = str(tmp_path / ("o%d" % len(os.listdir(tmp_path))))
    rc, log = run(harness, scene, prefix, *args, *D(**dict(BASE, **props)))
    return rc, log, prefix


@pytest.mark.parametrize("name", sorted(SCENES))
def test_captured_scene_equals_the_python_scene(pkg, harness, tmp_path, name):
    """(a) a quad light and a point light of sampling weight 3, (b) the constant sky, (c) a point light alone: emitter types,
    `shape` indices, radiance / intensity bits, sampling weights, n_points, the points and struct_size."""
    abi = pkg.abi
    sd = SCENES[name](pkg.scenes)
    rc, log, prefix = capture(pkg, harness, tmp_path, sd)
    assert rc == 0, log
    struct_size, sizeof_scene, n_points, n_normals = (int(v) for v in open(prefix + ".scene.meta").read().split())
    assert struct_size == sizeof_scene == C.sizeof(abi.Scene)
    assert (n_points, n_normals) == (len(sd.points), 0)
    got = pkg.scenes.SceneData.load(prefix + ".scene")
    assert_same_scene(abi, got, sd)
    kinds = [e.type for e in got.emitters]
    assert kinds == {"a_quad_and_point": [abi.EMITTER_AREA, abi.EMITTER_POINT], "b_sky": [abi.EMITTER_CONSTANT],
                     "c_point_only": [abi.EMITTER_POINT]}[name]
    if name == "a_quad_and_point":
        assert got.emitters[1].sampling_weight == 3.0 and got.emitters[1].shape == 0 and got.points == [(0.0, pytest.approx(0.8), 0.0)]
        assert list(got.emitters[1].radiance) == pytest.approx([4.0, 3.2, 2.0])
    if name == "b_sky":
        assert got.emitters[0].shape == -1


def test_free_emitters_are_placed_where_mitsuba_has_them(pkg, harness, tmp_path):
    """INTEGRATION.md, "Emitter order": a free emitter stands behind as many emitting shapes' lights as Scene::getEmitters()
    holds shape-carried emitters in front of it, and the area lights keep shape order. Scene::m_emitters as the harness fills it
    by default has the quad lights first (area lights in front of the point light); --free-first is where Mitsuba's XML loader
    leaves a free emitter, in front of every area light -- wherever the file declares it."""
    abi = pkg.abi
    S = pkg.scenes
    sd = S.cornell_c2(16)                             # two area lights: C2's ceiling quad (emitter 0) and a second, smaller one (emitter 1)
    sd.rectangle(S.translate(-0.6, 0.995, -0.4) @ S.rotate("x", 90) @ S.scale(0.1), 3, radiance=5.0)
    sd.point_light((0.0, 0.5, 0.0), intensity=2.0, sampling_weight=0.5)
    second = [i for i, s in enumerate(sd.shapes) if s.emitter == 1][0]
    first = [i for i, s in enumerate(sd.shapes) if s.emitter == 0][0]
    assert first < second

    rc, log, prefix = capture(pkg, harness, tmp_path, sd)
    assert rc == 0, log
    got = pkg.scenes.SceneData.load(prefix + ".scene")
    assert [e.type for e in got.emitters] == [abi.EMITTER_AREA, abi.EMITTER_AREA, abi.EMITTER_POINT]
    assert_same_scene(abi, got, sd)

    rc, log, prefix = capture(pkg, harness, tmp_path, sd, "--free-first")
    assert rc == 0, log
    got = pkg.scenes.SceneData.load(prefix + ".scene")
    assert [e.type for e in got.emitters] == [abi.EMITTER_POINT, abi.EMITTER_AREA, abi.EMITTER_AREA]
    assert [got.emitters[1].shape, got.emitters[2].shape] == [first, second]       # area lights: shape order among themselves
    assert (got.shapes[first].emitter, got.shapes[second].emitter) == (1, 2)       # the shapes' links follow their emitters
    assert got.emitters[0].shape == 0 and got.emitters[0].sampling_weight == 0.5 and got.points == [(0.0, 0.5, 0.0)]

    # a point light between the two area lights: Scene::m_emitters = [first quad light, point light, second quad light]
    mid = pkg.scenes.SceneData("mid")
    mid.shapes, mid.bsdfs, mid.camera = list(sd.shapes), list(sd.bsdfs), sd.camera
    mid.emitters = [sd.emitters[0], sd.emitters[2], sd.emitters[1]]
    mid.points = list(sd.points)
    mid.shapes[second].emitter = 2
    rc, log, prefix = capture(pkg, harness, tmp_path, mid)
    assert rc == 0, log
    got = pkg.scenes.SceneData.load(prefix + ".scene")
    assert [e.type for e in got.emitters] == [abi.EMITTER_AREA, abi.EMITTER_POINT, abi.EMITTER_AREA]
    assert_same_scene(abi, got, mid)


def test_two_point_lights_index_their_own_positions(pkg, harness, tmp_path):
    sd = scene_c(pkg.scenes)
    sd.point_light((0.25, 0.5, -0.5), intensity=(1.0, 2.0, 3.0), sampling_weight=0.25)
    rc, log, prefix = capture(pkg, harness, tmp_path, sd)
    assert rc == 0, log
    got = pkg.scenes.SceneData.load(prefix + ".scene")
    assert [e.shape for e in got.emitters] == [0, 1] and len(got.points) == 2
    assert_same_scene(pkg.abi, got, sd)


def test_other_emitter_plugins_are_refused_by_name(pkg, harness, tmp_path):
    rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), "--spot")
    errors = [t for lvl, t in log if lvl >= 400]
    assert rc == 1 and len(errors) == 1, log
    assert "SpotEmitter" in errors[0] and "refusing rather than approximating" in errors[0]
    assert not os.path.exists(prefix + ".scene")          # refused before anything reaches the library


@pytest.mark.parametrize("name,message", [("a_quad_and_point", "point lights are supported for technique=path only"),
                                          ("b_sky", "environment emitters are supported for technique=path only")])
def test_bdpt_refusal_is_the_librarys_own(pkg, harness, tmp_path, name, message):
    """The adaptor does not filter by technique: the scene goes through, prepare_scene refuses it, and its message comes back
    through Log(EError)."""
    rc, log, prefix = capture(pkg, harness, tmp_path, SCENES[name](pkg.scenes), technique="bdpt")
    assert rc == 1 and any(lvl >= 400 and message in t for lvl, t in log), log
    got = pkg.scenes.SceneData.load(prefix + ".scene")    # handed over in full all the same
    assert len(got.emitters) == len(SCENES[name](pkg.scenes).emitters)


@pytest.mark.parametrize("fixture,scene,args", [("adaptor_parent_caustic_c5_16.scene", "caustic_c5", ()),
                                                ("adaptor_parent_cornell_c2_16_meshlight.scene", "cornell_c2", ("--meshlight",))])
def test_area_light_only_scenes_give_the_bytes_of_before(pkg, tmp_path, fixture, scene, args):
    """tests/golden/adaptor_parent_*.scene: what adaptor_harness -DMOCK_ABI recorded for its own scene (two area lights; a quad
    light as a two-triangle mesh) with the adaptor as it was before it looked at Scene::getEmitters()."""
    subprocess.run(["make", "-C", HOST, "adaptor_harness_mock"], check=True, capture_output=True)
    path = str(tmp_path / "s.bin")
    pkg.scenes.SCENES[scene](res=16).save(path)
    prefix = str(tmp_path / "o")
    rc, log = run(os.path.join(HOST, "adaptor_harness_mock"), path, prefix, *args, *D(**BASE))
    assert rc == 0, log
    assert open(prefix + ".scene", "rb").read() == open(os.path.join(GOLDEN, fixture), "rb").read()


def test_area_lights_listed_by_the_scene_change_nothing(pkg, harness, tmp_path):
    """Scene::getEmitters() that lists the shapes' own area lights and nothing else (every scene of Mitsuba's that has area lights
    only): the same records, in the same order, as from the shapes alone."""
    sd = pkg.scenes.caustic_c5(16)
    for flag in ((), ("--free-first",)):
        rc, log, prefix = capture(pkg, harness, tmp_path, sd, *flag)
        assert rc == 0, log
        got = pkg.scenes.SceneData.load(prefix + ".scene")
        assert [bytes(e) for e in got.emitters] == [bytes(e) for e in sd.emitters] and len(got.emitters) == 2
        assert [s.emitter for s in got.shapes] == [s.emitter for s in sd.shapes] and got.points == []


def direct_calls(prefix):
    return [l.split() for l in open(prefix + ".direct")] if os.path.exists(prefix + ".direct") else []


def test_direct_pass_stays_on_the_host_by_default(pkg, harness, tmp_path):
    rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), directSamples=4)
    assert rc == 0, log
    assert direct_calls(prefix) == []
    assert any("render returned true, 1 refresh signal(s), 4 direct pass sample(s)" in t for _, t in log)
    img = np.fromfile(prefix + ".img", dtype=np.float32)
    assert img.size == 16 * 16 * 3 and np.all(img == 1.25)               # develop(direct): the host pass's 0.25
    assert "directPass = host" in open(prefix + ".tostring").read()


def test_direct_pass_on_the_device(pkg, harness, tmp_path):
    rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), directSamples=4, directPass="device")
    assert rc == 0, log
    calls = direct_calls(prefix)
    assert len(calls) == 1 and calls[0][:2] == ["4", "0"]                # once: directSamples, hide_emitters = 0
    assert int(calls[0][2]) != BASE["seed"]                              # not the chains' seed
    assert any("render returned true, 1 refresh signal(s), 0 direct pass sample(s)" in t for _, t in log)   # renderDirectComponent never ran
    img = np.fromfile(prefix + ".img", dtype=np.float32)
    assert img.size == 16 * 16 * 3 and np.all(img == 1.375)              # the full frame went straight into develop
    assert "directPass = device" in open(prefix + ".tostring").read()
    # directSamples <= 0: the chains carry the direct light, nobody renders a direct image
    rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), directSamples=-1, directPass="device")
    assert rc == 0 and direct_calls(prefix) == [] and np.all(np.fromfile(prefix + ".img", dtype=np.float32) == 1.0), log


def test_unknown_direct_pass_is_refused(pkg, harness, tmp_path):
    rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), directSamples=4, directPass="banana")
    assert rc == 1 and any(lvl >= 400 and "Unknown directPass (host | device)" in t for lvl, t in log), log


def test_direct_pass_survives_serialization_in_the_same_payload(pkg, harness, tmp_path):
    abi = pkg.abi
    payload = C.sizeof(abi.Config) + 4 + 1 + 1 + 4 + 1 + 4                # test_adaptor.py's figure: mask, twoStage, firstStage, reduction, hasSeed, seed
    sizes = {}
    for value, lum in (("device", 1.375), ("host", 1.25), (None, 1.25)):
        props = dict(directSamples=4) if value is None else dict(directSamples=4, directPass=value)
        rc, log, prefix = capture(pkg, harness, tmp_path, scene_a(pkg.scenes), "--unserialize", **props)
        assert rc == 0, log
        sizes[value] = os.path.getsize(prefix + ".ser")
        assert "directPass = %s" % (value or "host") in open(prefix + ".tostring").read()       # the unserialized instance's
        assert len(direct_calls(prefix)) == (1 if value == "device" else 0)
        assert np.all(np.fromfile(prefix + ".img", dtype=np.float32) == lum)
        cfg = abi.Config.from_buffer_copy(open(prefix + ".cfg", "rb").read())
        assert list(cfg.reserved) == [0, 0, 0] and cfg.direct_samples == 4   # what the library sees has its reserved words zero
    assert sizes == {"device": payload, "host": payload, None: payload}


def test_first_stage_scene_carries_the_point_lights(pkg, harness, tmp_path):
    sd = scene_a(pkg.scenes, res=32)
    rc, log, prefix = capture(pkg, harness, tmp_path, sd, twoStage=True, firstStageSizeReduction=4)
    assert rc == 0 and any("Executing first MLT stage" in t for _, t in log), log
    first, full = pkg.scenes.SceneData.load(prefix + ".first.scene"), pkg.scenes.SceneData.load(prefix + ".scene")
    assert open(prefix + ".first.scene.meta").read().split()[2] == open(prefix + ".scene.meta").read().split()[2] == "1"
    assert first.points == full.points == [(0.0, pytest.approx(0.8), 0.0)]
    assert [bytes(e) for e in first.emitters] == [bytes(e) for e in full.emitters] and len(first.emitters) == 2
    assert (first.camera.width, first.camera.height) == (8, 8) and (full.camera.width, full.camera.height) == (32, 32)


def test_scene_file_load_is_the_inverse_of_save(pkg, tmp_path):
    for sd in (scene_a(pkg.scenes), pkg.scenes.cornell_sky(16), pkg.scenes.smooth_room(16, level=0)):
        path = str(tmp_path / "s.bin")
        sd.save(path)
        back = pkg.scenes.SceneData.load(path)
        assert_same_scene(pkg.abi, back, sd)
        assert f32([v for n in back.normals for v in n]) == f32([v for n in sd.normals for v in n])
        back.save(path + "2")
        assert open(path, "rb").read() == open(path + "2", "rb").read()
    open(str(tmp_path / "bad.bin"), "wb").write(open(path, "rb").read()[:-3])
    with pytest.raises(ValueError):
        pkg.scenes.SceneData.load(str(tmp_path / "bad.bin"))
