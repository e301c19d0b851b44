"""Point emitters (src/emitters/point.cpp) at the C-ABI, without a GPU: the header and its ctypes mirror agree, drmlt_create
refuses what it cannot render before it looks for a device, a drmlt_scene of the layout that ends at `camera` is still
taken, and the scene file and the Mitsuba XML export carry the point lights."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


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


def test_header_and_mirror_agree_on_point_lights(abi):
    out = _run_c(r'''
#include <stdio.h>
#include <stddef.h>
#include "drmlt_abi.h"
int main(void) {
  printf("%d %zu %zu %zu %zu\n", (int) DRMLT_EMITTER_POINT, offsetof(drmlt_scene, n_points), offsetof(drmlt_scene, points),
         sizeof(drmlt_scene), (size_t) DRMLT_SCENE_SIZE_NO_POINTS);
  return 0; }
''')
    assert [int(v) for v in out] == [abi.EMITTER_POINT, abi.Scene.n_points.offset, abi.Scene.points.offset,
                                     C.sizeof(abi.Scene), abi.SCENE_SIZE_NO_POINTS]
    assert abi.EMITTER_POINT == 1 and abi.EMITTER_AREA == 0
    # the fields trail `camera`, whose offset and the ABI version stay what they were
    assert abi.Scene.n_points.offset >= abi.Scene.camera.offset + C.sizeof(abi.Camera)
    assert abi.SCENE_SIZE_NO_POINTS < C.sizeof(abi.Scene) and abi.ABI_VERSION == 4


def _lit_floor(pkg, **light):
    sd = pkg.scenes.cornell_c1(8)
    sd.point_light((0.0, 0.5, 0.0), **light)
    return sd


def _refusal(pkg, cfg, sd):
    with pytest.raises(pkg.DrmltError) as e:
        pkg.Context(cfg, sd)
    return str(e.value)


def test_create_refuses_what_a_point_light_cannot_be(pkg, abi, native_lib):
    cfg = abi.make_config(type="orbital", max_depth=8)
    sd = _lit_floor(pkg)
    sd.emitters[-1].shape = 1                          # only one position entry
    assert "out of range" in _refusal(pkg, cfg, sd)
    sd = _lit_floor(pkg)
    sd.emitters[-1].shape = -1
    assert "out of range" in _refusal(pkg, cfg, sd)
    sd = _lit_floor(pkg)
    sd.point_light((0.2, 0.5, 0.0))
    sd.emitters[-1].shape = 0                          # two emitters, one position
    assert "shares position entry 0" in _refusal(pkg, cfg, sd)
    for bad in (float("nan"), float("inf")):
        sd = pkg.scenes.cornell_c1(8)
        sd.point_light((0.0, bad, 0.0))
        assert "position is not finite" in _refusal(pkg, cfg, sd)
    for bad in ((1.0, -0.5, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        assert "intensity must be finite and non-negative" in _refusal(pkg, cfg, _lit_floor(pkg, intensity=bad))
    sd = _lit_floor(pkg)
    sd.shapes[0].emitter = len(sd.emitters) - 1        # a shape cannot carry a point light
    assert "emitter/shape link mismatch" in _refusal(pkg, cfg, sd)
    sd = _lit_floor(pkg)
    sd.emitters[-1].type = 7
    assert "unsupported emitter type" in _refusal(pkg, cfg, sd)


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
def test_point_lights_are_for_technique_path_only(pkg, abi, native_lib, technique):
    cfg = abi.make_config(type="orbital", technique=technique, max_depth=6)
    msg = _refusal(pkg, cfg, _lit_floor(pkg))
    assert "technique=path only" in msg, msg
    assert "technique=path only" in _refusal(pkg, cfg, pkg.scenes.cornell_point(8))


def _create_raw(pkg, abi, sd, struct_size):
    L = pkg.binding.load_library()
    s = sd.struct()
    s.struct_size = struct_size
    cfg = abi.make_config(type="orbital", max_depth=8)
    err = C.create_string_buffer(512)
    h = L.drmlt_create(C.byref(cfg), C.byref(s), 0, err, 512)
    if h:
        L.drmlt_destroy(h)
    return bool(h), err.value.decode()


def test_scene_struct_of_the_layout_without_point_lights_is_accepted(pkg, abi, native_lib):
    sd = pkg.scenes.cornell_c1(8)
    ok, msg = _create_raw(pkg, abi, sd, abi.SCENE_SIZE_NO_POINTS)
    assert "struct_size" not in msg
    if not _has_gpu():
        assert not ok and "no HIP device" in msg, msg
    for bad in (abi.SCENE_SIZE_NO_POINTS - 8, abi.SCENE_SIZE_NO_POINTS + 4, C.sizeof(abi.Scene) + 8):
        ok, msg = _create_raw(pkg, abi, sd, bad)
        assert not ok and "struct_size mismatch" in msg, (bad, msg)
    # the short layout means "no point lights": what follows `camera` is not read, so a point emitter has no position
    ok, msg = _create_raw(pkg, abi, _lit_floor(pkg), abi.SCENE_SIZE_NO_POINTS)
    assert not ok and "out of range (n_points = 0)" in msg, msg
    ok, msg = _create_raw(pkg, abi, _lit_floor(pkg), C.sizeof(abi.Scene))
    assert "point light" not in msg and "struct_size" not in msg


def test_point_only_scene_passes_validation(pkg, abi, native_lib):
    """A scene lit by point lights alone is valid for technique=path (as in the reference): without a GPU, creation gets
    as far as the device check."""
    sd = pkg.scenes.cornell_point(8)
    assert [e.type for e in sd.emitters] == [abi.EMITTER_POINT]
    if _has_gpu():
        pkg.Context(abi.make_config(type="orbital", max_depth=8), sd).close()
    else:
        assert "no HIP device" in _refusal(pkg, abi.make_config(type="orbital", max_depth=8), sd)
    # and under algo=pssmlt, which runs over technique=path
    if not _has_gpu():
        msg = _refusal(pkg, abi.make_config(algo=abi.ALGO_PSSMLT, type="orbital", max_depth=8), sd)
        assert "no HIP device" in msg, msg


def test_scene_file_without_point_lights_keeps_its_size(pkg, abi, tmp_path):
    sd = pkg.scenes.cornell_c2(16)
    path = str(tmp_path / "c2.drmlt")
    sd.save(path)
    want = 32 + len(sd.shapes) * C.sizeof(abi.Shape) + len(sd.bsdfs) * C.sizeof(abi.Bsdf) + \
        len(sd.emitters) * C.sizeof(abi.Emitter) + C.sizeof(abi.Camera)
    data = open(path, "rb").read()
    assert len(data) == want
    assert data[-C.sizeof(abi.Camera):] == bytes(sd.camera)


def test_scene_file_round_trips_point_lights(pkg, abi, tmp_path):
    sd = pkg.scenes.cornell_point(16, quad_light=True, point_weight=3.0)
    sd.point_light((0.25, -0.125, 0.5), intensity=(1.0, 2.0, 3.0))
    path = str(tmp_path / "cp.drmlt")
    sd.save(path)
    hpp = os.path.join(ROOT, "drmlt-mitsuba_amd", "host", "drmlt_integrator.hpp")
    out = _run_c(r'''
#include "%s"
#include <cstdio>
int main() {
  drmlt_host::SceneFile sf = drmlt_host::SceneFile::load("%s");
  drmlt_scene s = sf.view();
  printf("%%d %%d %%d %%d\n", s.n_shapes, s.n_emitters, s.n_points, (int) s.struct_size);
  for (int i = 0; i < s.n_emitters; ++i) printf("%%d %%d %%.9g\n", s.emitters[i].type, s.emitters[i].shape, s.emitters[i].sampling_weight);
  for (int i = 0; i < 3 * s.n_points; ++i) printf("%%.9g\n", s.points[i]);
  return 0; }
''' % (hpp, path), lang="c++")
    head = [int(v) for v in out[:4]]
    assert head == [len(sd.shapes), len(sd.emitters), len(sd.points), C.sizeof(abi.Scene)]
    rows = out[4:4 + 3 * len(sd.emitters)]
    for i, e in enumerate(sd.emitters):
        assert (int(rows[3 * i]), int(rows[3 * i + 1]), float(rows[3 * i + 2])) == (e.type, e.shape, pytest.approx(e.sampling_weight))
    pts = np.array([float(v) for v in out[4 + 3 * len(sd.emitters):]], dtype=np.float32)
    assert np.array_equal(pts, np.asarray(sd.points, dtype=np.float32).reshape(-1))
    # the same file without its trailing block loads as a scene without point lights
    data = open(path, "rb").read()
    short = str(tmp_path / "short.drmlt")
    open(short, "wb").write(data[:len(data) - 8 - 12 * len(sd.points)])
    out = _run_c(r'''
#include "%s"
#include <cstdio>
int main() { drmlt_host::SceneFile sf = drmlt_host::SceneFile::load("%s"); printf("%%d %%zu\n", sf.view().n_points, sf.emitters.size()); return 0; }
''' % (hpp, short), lang="c++")
    assert out == ["0", str(len(sd.emitters))]


def test_mitsuba_xml_export_carries_the_point_light(pkg, abi, tmp_path):
    spec = importlib.util.spec_from_file_location("cpu_baseline", os.path.join(ROOT, "tools", "cpu_baseline.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    sd = pkg.scenes.cornell_point(16, quad_light=True, point_weight=3.0)
    path = cb.scene_to_xml(pkg, sd, dict(cfg=dict(max_depth=8), spp=4), str(tmp_path), "cp")
    xml = open(path).read()
    import xml.etree.ElementTree as ET
    root = ET.fromstring(xml.replace("$integrator", "drmlt").replace("$technique", "path").replace("$type", "orbital")
                         .replace("$fixEmitterPath", "false").replace("$acceptanceMap", "false"))
    points = [e for e in root.findall("emitter") if e.get("type") == "point"]
    assert len(points) == 1
    p = points[0].find("point")
    assert [float(p.get(k)) for k in "xyz"] == pytest.approx(list(sd.points[0]))
    assert points[0].find("spectrum").get("name") == "intensity"
    assert [float(v) for v in points[0].find("spectrum").get("value").split(",")] == pytest.approx(list(sd.emitters[1].radiance))
    assert float(points[0].find("float").get("value")) == pytest.approx(3.0)
    # document order = emitter order (m_emitters, the sampling PMF): the quad light's shape comes first, then the point light
    kinds = [("area" if c.tag == "shape" else "point") for c in root
             if (c.tag == "shape" and c.find("emitter") is not None) or (c.tag == "emitter")]
    assert kinds == ["area", "point"]
