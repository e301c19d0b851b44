"""Smooth conductor (src/bsdfs/conductor.cpp) at the C-ABI and in the tools, without a GPU: the header and its ctypes mirror
agree on the type, drmlt_create takes it as far as the device lookup and refuses bad parameters before that, SceneData,
the scene file and the Mitsuba XML export carry it, and the Mitsuba adaptor maps SmoothConductor to it."""
import ctypes as C
import importlib.util
import os
import subprocess
import tempfile

import numpy as np
import pytest

import conductor_scenes as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _run_cpp(src):
    with tempfile.TemporaryDirectory() as d:
        path, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(path, "w").write(src)
        subprocess.check_call(["g++", "-std=c++17", "-I", INCLUDE, path, "-o", exe])
        return subprocess.check_output([exe]).decode().split()


def _refusal(pkg, cfg, sd):
    with pytest.raises(pkg.DrmltError) as e:
        pkg.Context(cfg, sd)
    return str(e.value)


def test_header_and_mirror_agree_on_the_conductor(abi):
    out = _run_cpp('#include <cstdio>\n#include "drmlt_abi.h"\n'
                   'int main() { printf("%d %d %zu\\n", (int) DRMLT_BSDF_CONDUCTOR, (int) DRMLT_ABI_VERSION, sizeof(drmlt_bsdf)); return 0; }')
    assert [int(v) for v in out] == [abi.BSDF_CONDUCTOR, abi.ABI_VERSION, C.sizeof(abi.Bsdf)]
    assert abi.BSDF_CONDUCTOR == 3 and abi.ABI_VERSION == 4


def test_scene_data_fills_the_struct(pkg, abi):
    sd = pkg.scenes.SceneData("t")
    i = sd.conductor()
    b = sd.bsdfs[i]
    assert b.type == abi.BSDF_CONDUCTOR and list(b.rgb) == [1.0, 1.0, 1.0]
    assert list(b.p)[1:7] == pytest.approx([0.2004, 0.9240, 1.1022, 3.9129, 2.4528, 2.1421]) and b.p[0] == 0 and b.p[7] == 0
    rc = sd.bsdfs[sd.roughconductor()]
    assert list(rc.p)[1:7] == list(b.p)[1:7]                      # the rough conductor's copper, in its slots
    j = sd.conductor(eta=(1, 2, 3), k=(4, 5, 6), specular_reflectance=(0.9, 0.6, 0.3))
    assert list(sd.bsdfs[j].p)[1:7] == [1, 2, 3, 4, 5, 6] and list(sd.bsdfs[j].rgb) == pytest.approx([0.9, 0.6, 0.3])
    room = pkg.scenes.SCENES["mirror_room"](16)
    assert [b.type for b in room.bsdfs].count(abi.BSDF_CONDUCTOR) == 1 and room.bsdfs[room.shapes[0].bsdf].type == abi.BSDF_CONDUCTOR


@pytest.mark.parametrize("technique,algo", [("path", "drmlt"), ("bdpt", "drmlt"), ("mmlt", "drmlt"), ("path", "pssmlt")])
def test_create_takes_a_conductor_scene_as_far_as_the_device(pkg, abi, native_lib, technique, algo):
    extra = dict(algo=abi.ALGO_PSSMLT) if algo == "pssmlt" else {}
    cfg = abi.make_config(type="orbital", technique=technique, max_depth=6, **extra)
    sd = pkg.scenes.mirror_room(8)
    if _has_gpu():
        pkg.Context(cfg, sd).close()
    else:
        msg = _refusal(pkg, cfg, sd)
        assert "unsupported BSDF" not in msg and "no HIP device" in msg, msg


def test_create_refuses_bad_conductor_parameters_before_the_device_lookup(pkg, abi, native_lib):
    cfg = abi.make_config(type="orbital", max_depth=6)
    for slot, what in ((1, "eta"), (3, "eta"), (4, "k"), (6, "k")):
        for bad in (float("nan"), float("inf"), -0.5):
            sd = pkg.scenes.mirror_room(8)
            [b for b in sd.bsdfs if b.type == abi.BSDF_CONDUCTOR][0].p[slot] = bad
            msg = _refusal(pkg, cfg, sd)
            assert "conductor" in msg and what + " must be finite and non-negative" in msg, msg
    for bad in (float("nan"), float("inf"), -0.5):
        sd = pkg.scenes.mirror_room(8)
        [b for b in sd.bsdfs if b.type == abi.BSDF_CONDUCTOR][0].rgb[1] = bad
        assert "specularReflectance must be finite and non-negative" in _refusal(pkg, cfg, sd)
    # p[0] and p[7] are ignored
    sd = pkg.scenes.mirror_room(8)
    m = [b for b in sd.bsdfs if b.type == abi.BSDF_CONDUCTOR][0]
    m.p[0], m.p[7] = float("nan"), -1.0
    if _has_gpu():
        pkg.Context(cfg, sd).close()
    else:
        assert "no HIP device" in _refusal(pkg, cfg, sd)
    # what is still refused says what is supported, before any device is looked for
    sd = pkg.scenes.mirror_room(8)
    sd.bsdfs[0].type = 4
    msg = _refusal(pkg, cfg, sd)
    assert "unsupported BSDF type 4" in msg and "conductor)" in msg, msg


def test_scene_file_round_trips_the_conductor(pkg, abi, tmp_path):
    sd = pkg.scenes.mirror_room(16)
    sd.conductor(eta=(1, 2, 3), k=(4, 5, 6), specular_reflectance=(0.9, 0.6, 0.3))
    path = str(tmp_path / "mr.drmlt")
    sd.save(path)
    hpp = os.path.join(HOST, "drmlt_integrator.hpp")
    out = _run_cpp(r'''
#include "%s"
#include <cstdio>
int main() {
  drmlt_host::SceneFile sf = drmlt_host::SceneFile::load("%s");
  drmlt_scene s = sf.view();
  printf("%%d\n", s.n_bsdfs);
  for (int i = 0; i < s.n_bsdfs; ++i) {
    printf("%%d", s.bsdfs[i].type);
    for (int k = 0; k < 3; ++k) printf(" %%.9g", s.bsdfs[i].rgb[k]);
    for (int k = 0; k < 8; ++k) printf(" %%.9g", s.bsdfs[i].p[k]);
    printf("\n");
  }
  return 0; }
''' % (hpp, path))
    assert int(out[0]) == len(sd.bsdfs)
    rows = np.array([float(v) for v in out[1:]]).reshape(len(sd.bsdfs), 12)
    for row, b in zip(rows, sd.bsdfs):
        assert int(row[0]) == b.type
        assert np.array_equal(row[1:].astype(np.float32), np.array(list(b.rgb) + list(b.p), dtype=np.float32))
    assert [int(r[0]) for r in rows].count(abi.BSDF_CONDUCTOR) == 2


def test_mitsuba_xml_export_carries_the_conductor(pkg, abi, tmp_path):
    spec = importlib.util.spec_from_file_location("cpu_baseline", os.path.join(ROOT, "tools", "cpu_baseline.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    sd = pkg.scenes.mirror_room(16)
    sd.bsdfs[sd.shapes[0].bsdf].rgb[:] = (0.9, 0.6, 0.3)
    path = cb.scene_to_xml(pkg, sd, dict(cfg=dict(max_depth=8), spp=4), str(tmp_path), "mr")
    import xml.etree.ElementTree as ET
    root = ET.fromstring(open(path).read().replace("$integrator", "drmlt").replace("$technique", "path").replace("$type", "orbital")
                         .replace("$fixEmitterPath", "false").replace("$acceptanceMap", "false"))
    mirrors = [e for e in root.findall("bsdf") if e.get("type") == "conductor"]
    assert len(mirrors) == 1 and not [e for e in root.findall("bsdf") if e.get("type") == "roughconductor"]
    spectra = {e.get("name"): [float(v) for v in e.get("value").split(",")] for e in mirrors[0].findall("spectrum")}
    assert spectra["eta"] == pytest.approx(list(cs.COPPER_ETA)) and spectra["k"] == pytest.approx(list(cs.COPPER_K))
    assert spectra["specularReflectance"] == pytest.approx([0.9, 0.6, 0.3])
    assert float(mirrors[0].find("float").get("value")) == 1.0 and mirrors[0].find("float").get("name") == "extEta"
    assert mirrors[0].get("id") == "b%d" % sd.shapes[0].bsdf


@pytest.fixture(scope="module")
def conductor_harness():
    subprocess.check_call(["make", "-C", HOST, "conductor_harness"], stdout=subprocess.DEVNULL)
    return os.path.join(HOST, "conductor_harness")


def _mirror_row(harness, abi, *args):
    rows = [l.split() for l in subprocess.check_output([harness, *args]).decode().splitlines() if l.startswith("bsdf ")]
    rows = [[float(v) for v in r[1:]] for r in rows]
    mirrors = [r for r in rows if int(r[0]) == abi.BSDF_CONDUCTOR]
    assert len(rows) == 2 and len(mirrors) == 1, rows
    return mirrors[0][1:4], mirrors[0][4:]


def test_adaptor_maps_the_smooth_conductor(conductor_harness, abi):
    rgb, p = _mirror_row(conductor_harness, abi, "none")               # material = none: eta 0, k 1 over extEta = air
    assert rgb == [1.0, 1.0, 1.0]
    assert p[1:4] == [0.0, 0.0, 0.0] and p[4:7] == pytest.approx([1 / 1.000277] * 3, rel=1e-6) and p[0] == 0 and p[7] == 0
    rgb, p = _mirror_row(conductor_harness, abi, "explicit")           # eta, k given, extEta = 2
    assert rgb == pytest.approx([0.9, 0.6, 0.3])
    assert p[1:4] == pytest.approx([0.1, 0.45, 0.55]) and p[4:7] == pytest.approx([1.95, 1.2, 1.05])
    rgb, p = _mirror_row(conductor_harness, abi, "material", "Au", "fake:0.2_0.9_1.1/")   # through the FileResolver
    assert rgb == [1.0, 1.0, 1.0] and p[1:4] == pytest.approx([0.2, 0.9, 1.1]) and p[4:7] == pytest.approx([0.2, 0.9, 1.1])
