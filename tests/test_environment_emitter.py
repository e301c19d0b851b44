"""The constant environment emitter (src/emitters/constant.cpp) at the C-ABI, without a GPU: the header and its ctypes mirror
agree, drmlt_create refuses what it cannot render before it looks for a device, and the scene file and the Mitsuba XML
export carry the sky."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

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


def test_header_and_mirror_agree_on_the_constant_emitter(abi):
    out = _run_c(r'''
#include <stdio.h>
#include "drmlt_abi.h"
int main(void) {
  printf("%d %d %d %d\n", (int) DRMLT_EMITTER_AREA, (int) DRMLT_EMITTER_POINT, (int) DRMLT_EMITTER_CONSTANT, (int) DRMLT_ABI_VERSION);
  return 0; }
''')
    assert [int(v) for v in out] == [abi.EMITTER_AREA, abi.EMITTER_POINT, abi.EMITTER_CONSTANT, abi.ABI_VERSION]
    assert (abi.EMITTER_AREA, abi.EMITTER_POINT, abi.EMITTER_CONSTANT, abi.ABI_VERSION) == (0, 1, 2, 4)


def _sky_floor(pkg, **env):
    sd = pkg.scenes.cornell_c1(8)
    sd.constant_environment(**env)
    return sd


def _refusal(pkg, cfg, sd):
    with pytest.raises(pkg.DrmltError) as e:
        pkg.Context(cfg, sd)
    return str(e.value)


def test_constant_environment_record(pkg, abi):
    sd = pkg.scenes.SceneData("t")
    i = sd.constant_environment((0.5, 1.0, 2.0), sampling_weight=3.0)
    e = sd.emitters[i]
    assert (e.type, e.shape, list(e.radiance), e.sampling_weight) == (abi.EMITTER_CONSTANT, -1, [0.5, 1.0, 2.0], 3.0)
    e = sd.emitters[sd.constant_environment()]
    assert list(e.radiance) == [1.0, 1.0, 1.0] and e.sampling_weight == 1.0   # constant.cpp: D65 = (1, 1, 1), weight 1
    assert not sd.points


def test_create_refuses_what_an_environment_emitter_cannot_be(pkg, abi, native_lib):
    cfg = abi.make_config(type="orbital", max_depth=8)
    sd = _sky_floor(pkg)
    sd.constant_environment()
    assert "only contain one environment emitter" in _refusal(pkg, cfg, sd)
    for shape in (0, 1, -2):
        sd = _sky_floor(pkg)
        sd.emitters[-1].shape = shape
        assert "shape must be -1" in _refusal(pkg, cfg, sd)
    sd = _sky_floor(pkg)
    sd.shapes[0].emitter = len(sd.emitters) - 1        # a shape cannot carry the environment
    assert "emitter/shape link mismatch" in _refusal(pkg, cfg, sd)
    for bad in ((1.0, -0.5, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0)):
        assert "radiance must be finite and non-negative" in _refusal(pkg, cfg, _sky_floor(pkg, radiance=bad))
    sd = _sky_floor(pkg)
    sd.emitters[-1].type = 7
    assert "unsupported emitter type" in _refusal(pkg, cfg, sd)


@pytest.mark.parametrize("technique", ["bdpt", "mmlt"])
def test_environment_emitters_are_for_technique_path_only(pkg, abi, native_lib, technique):
    cfg = abi.make_config(type="orbital", technique=technique, max_depth=6)
    msg = _refusal(pkg, cfg, _sky_floor(pkg))
    assert "technique=path only" in msg, msg
    assert "technique=path only" in _refusal(pkg, cfg, pkg.scenes.cornell_sky(8, quad_light=True))


@pytest.mark.parametrize("algo", ["drmlt", "pssmlt"])
@pytest.mark.parametrize("quad_light", [False, True])
def test_sky_scene_passes_validation(pkg, abi, native_lib, algo, quad_light):
    """A scene lit by the sky alone, or by the sky and a quad light, is valid for technique=path and for algo=pssmlt (which
    runs over it): without a GPU, creation gets as far as the device check."""
    sd = pkg.scenes.cornell_sky(8, quad_light=quad_light, env_weight=2.0)
    kinds = [e.type for e in sd.emitters]
    assert kinds == ([abi.EMITTER_AREA] if quad_light else []) + [abi.EMITTER_CONSTANT]
    assert sd.emitters[-1].sampling_weight == 2.0
    extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
    cfg = abi.make_config(type="orbital", max_depth=8, **extra)
    if _has_gpu():
        pkg.Context(cfg, sd).close()
    else:
        msg = _refusal(pkg, cfg, sd)
        assert "no HIP device" in msg, msg


def test_cornell_sky_is_registered(pkg):
    assert pkg.scenes.SCENES["cornell_sky"] is pkg.scenes.cornell_sky
    sd = pkg.scenes.SCENES["cornell_sky"](res=16)
    assert (sd.camera.width, sd.camera.height) == (16, 16)
    # C2's room without a front wall: every rectangle but the (optional) light is one of C2's five walls
    assert len(sd.shapes) == len(pkg.scenes.cornell_c2(16).shapes) - 1


def test_scene_file_without_a_sky_keeps_its_size(pkg, abi, tmp_path):
    for sd in (pkg.scenes.cornell_c2(16), pkg.scenes.cornell_point(16)):
        path = str(tmp_path / "s.drmlt")
        sd.save(path)
        want = 32 + len(sd.shapes) * C.sizeof(abi.Shape) + len(sd.bsdfs) * C.sizeof(abi.Bsdf) + \
            len(sd.emitters) * C.sizeof(abi.Emitter) + C.sizeof(abi.Camera) + (8 + 12 * len(sd.points) if sd.points else 0)
        assert len(open(path, "rb").read()) == want


def test_scene_file_round_trips_the_sky(pkg, abi, tmp_path):
    sd = pkg.scenes.cornell_sky(16, quad_light=True, env_weight=3.0)
    sd.point_light((0.25, -0.125, 0.5), intensity=(1.0, 2.0, 3.0))
    path = str(tmp_path / "sky.drmlt")
    sd.save(path)
    hpp = os.path.join(ROOT, "drmlt-mitsuba_amd", "host", "drmlt_integrator.hpp")
    out = _run_c(r'''
#include "%s"
#include <cstdio>
int main() {
  drmlt_host::SceneFile sf = drmlt_host::SceneFile::load("%s");
  drmlt_scene s = sf.view();
  printf("%%d %%d %%d\n", s.n_shapes, s.n_emitters, s.n_points);
  for (int i = 0; i < s.n_emitters; ++i)
    printf("%%d %%d %%.9g %%.9g %%.9g %%.9g\n", s.emitters[i].type, s.emitters[i].shape, s.emitters[i].radiance[0], s.emitters[i].radiance[1],
           s.emitters[i].radiance[2], s.emitters[i].sampling_weight);
  return 0; }
''' % (hpp, path), lang="c++")
    assert [int(v) for v in out[:3]] == [len(sd.shapes), len(sd.emitters), len(sd.points)]
    rows = out[3:]
    assert len(rows) == 6 * len(sd.emitters)
    for i, e in enumerate(sd.emitters):
        r = rows[6 * i:6 * i + 6]
        assert (int(r[0]), int(r[1])) == (e.type, e.shape)
        assert [float(v) for v in r[2:]] == pytest.approx(list(e.radiance) + [e.sampling_weight])
    assert [int(rows[6 * i]) for i in range(len(sd.emitters))] == [abi.EMITTER_AREA, abi.EMITTER_CONSTANT, abi.EMITTER_POINT]


def test_mitsuba_xml_export_carries_the_sky(pkg, abi, tmp_path):
    spec = importlib.util.spec_from_file_location("cpu_baseline", os.path.join(ROOT, "tools", "cpu_baseline.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    sd = pkg.scenes.cornell_sky(16, quad_light=True, env_weight=3.0)
    sd.point_light((0.0, 0.8, 0.0), intensity=(4.0, 3.2, 2.0))
    path = cb.scene_to_xml(pkg, sd, dict(cfg=dict(max_depth=8), spp=4), str(tmp_path), "sky")
    xml = open(path).read()
    import xml.etree.ElementTree as ET
    root = ET.fromstring(xml.replace("$integrator", "drmlt").replace("$technique", "path").replace("$type", "orbital")
                         .replace("$fixEmitterPath", "false").replace("$acceptanceMap", "false"))
    skies = [e for e in root.findall("emitter") if e.get("type") == "constant"]
    assert len(skies) == 1
    spec_el = skies[0].find("spectrum")
    assert spec_el.get("name") == "radiance"
    assert [float(v) for v in spec_el.get("value").split(",")] == pytest.approx(list(sd.emitters[1].radiance))
    w = skies[0].find("float")
    assert w.get("name") == "samplingWeight" and float(w.get("value")) == pytest.approx(3.0)
    # document order = emitter order (m_emitters, the sampling PMF): the quad light's shape, the sky, the point light
    kinds = [("area" if c.tag == "shape" else c.get("type")) for c in root
             if (c.tag == "shape" and c.find("emitter") is not None) or (c.tag == "emitter")]
    assert kinds == ["area", "constant", "point"]
