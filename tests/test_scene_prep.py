"""The host-side scene preparation (csrc/scene_prep.h), checked on the CPU. tests/native/scene_prep_harness.cpp runs prepare_scene on
a scene file written by SceneData.save() and a configuration, prints the scalar results as JSON and writes the raw tables.

PINS was recorded from drmlt_create as it stood BEFORE scene_prep.h existed (the commit that adds this file names the recording
patch): the tables drmlt_create uploaded and the DParams / PlanInputs it derived, byte for byte. The refusals are asserted on the
harness and through drmlt_create in the library, which answers them with or without a GPU. One thing has changed on purpose since:
the environment's bounding sphere is now that of the kd-tree's enlarged box, as in the reference (scene_bsphere;
tests/test_light_probe.py::test_the_tables_are_the_scene holds it against the fp32 oracle's for the light-pick scene), so the shading
tables of the two cornell_sky cases, which hold that sphere, were recorded anew."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")

PATH8 = dict(type="orbital", max_depth=8, rr_depth=5, direct_samples=-1)
BENCH = {  # bench.py's configurations (res 512), by the name of test_launch_plan.py's dictionary
    "C2": ("cornell_c2", {}, dict(PATH8, sample_count=256)),
    "C3": ("door_c3", {}, dict(PATH8, type="green", sample_count=240)),
    "C5": ("caustic_c5", {}, dict(technique="mmlt", type="orbital", max_depth=6, fix_emitter_path=1, acceptance_map=1, direct_samples=-1, sample_count=256)),
    "BD": ("cornell_c2", {}, dict(PATH8, technique="bdpt", sample_count=256)),
    "SOUP": ("triangle_soup", dict(n_tris=2000), dict(PATH8, sample_count=240)),
}


def _points400(scenes):
    sd = scenes.cornell_c2(64)
    for i in range(400):
        sd.point_light((-0.9 + 1.8 * (i % 20) / 19.0, 0.9, -0.9 + 1.8 * (i // 20) / 19.0), intensity=(0.02, 0.016, 0.01))
    return sd


# (name, scene, configuration, DRMLT_* environment)
CASES = [
    ("cornell_c1", lambda s: s.cornell_c1(64), PATH8, {}),
    ("cornell_c2", lambda s: s.cornell_c2(64), PATH8, {}),
    ("glass_sphere", lambda s: s.glass_sphere(64), PATH8, {}),
    ("door_c3 beckmann", lambda s: s.door_c3(64), PATH8, {}),
    ("door_c3 ggx", lambda s: s.door_c3(64, ggx=True), PATH8, {}),
    ("mirror_room", lambda s: s.mirror_room(64), PATH8, {}),
    ("soup 2000", lambda s: s.triangle_soup(2000, 64), PATH8, {}),
    ("caustic_c5", lambda s: s.caustic_c5(64), PATH8, {}),
    ("cornell_point", lambda s: s.cornell_point(64), PATH8, {}),
    ("cornell_point + quad", lambda s: s.cornell_point(64, quad_light=True, point_weight=0.5), PATH8, {}),
    ("cornell_sky", lambda s: s.cornell_sky(64), PATH8, {}),
    ("cornell_sky + quad", lambda s: s.cornell_sky(64, quad_light=True, env_weight=2.0), PATH8, {}),
    ("cornell_c2 gaussian pssmlt", lambda s: s.cornell_c2(48, filt=1), dict(PATH8, algo=1, direct_samples=16, work_units=4096), {}),
    ("cornell_c2 bdpt", lambda s: s.cornell_c2(64), dict(PATH8, technique="bdpt"), {}),
    ("cornell_c2 bdpt no direct sampling", lambda s: s.cornell_c2(64), dict(PATH8, technique="bdpt", no_direct_sampling=1), {}),
    ("caustic_c5 mmlt", lambda s: s.caustic_c5(64), dict(technique="mmlt", type="orbital", max_depth=6, fix_emitter_path=1, direct_samples=-1), {}),
    ("cornell_c2 no box merge", lambda s: s.cornell_c2(64), PATH8, {"DRMLT_NO_BOX_MERGE": "1"}),
    ("cornell_c2 no quad merge", lambda s: s.cornell_c2(64), PATH8, {"DRMLT_NO_QUAD_MERGE": "1"}),
    ("cornell_c2 no flat loop", lambda s: s.cornell_c2(64), PATH8, {"DRMLT_NO_FLAT_LOOP": "1"}),
    ("cornell_c2 feat all, debug", lambda s: s.cornell_c2(64), PATH8, {"DRMLT_FEAT_ALL": "1", "DRMLT_DEBUG": "128"}),
    ("cornell_c2 as a BVH", lambda s: s.cornell_c2(64), PATH8, {"DRMLT_BVH_THRESHOLD": "0"}),
    ("soup stack32", lambda s: s.triangle_soup(2000, 64), PATH8, {"DRMLT_BVH_STACK32": "1"}),
    ("soup median splits", lambda s: s.triangle_soup(2000, 64), PATH8, {"DRMLT_BVH_MAX_DEPTH": "6"}),
    ("soup leaves of 4", lambda s: s.triangle_soup(2000, 64), PATH8, {"DRMLT_BVH_LEAF": "4"}),
    ("deep chain", lambda s: s.deep_chain(64), PATH8, {"DRMLT_BVH_THRESHOLD": "0"}),
    ("400 point lights", _points400, PATH8, {}),
    ("49 records", lambda s: s.triangle_soup(43, 64), PATH8, {}),
    ("48 records", lambda s: s.triangle_soup(42, 64), PATH8, {}),
] + [("bench " + k, (lambda s, n=n, kw=kw: s.SCENES[n](res=512, **kw)), cfg, {}) for k, (n, kw, cfg) in BENCH.items()]

# Per case: the sha256 (first 16 hex digits) of the harness's whole JSON line in canonical form, the fields a reader wants to see, and
# the sha256 of every table.
PINS = {
    'cornell_c1': dict(n_prims=3, n_shade=3, n_bvh_nodes=0, n_flat=3, n_flat_rec=3, n_box=0, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='8efe67312b93cfca',
        tables={'prims': 'a6845641985dbb97', 'shade': '99af36c16e97c089', 'bsdfs': 'd9282b78af3cd2e7', 'emitters': '77d648d3cb7049df', 'lut': '4f3edc52216d8d9d', 'flat': '764078d190758bd2'}),
    'cornell_c2': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='4db2f18efeb4e956',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'glass_sphere': dict(n_prims=7, n_shade=7, n_bvh_nodes=0, n_flat=6, n_flat_rec=1, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=6, bvh_depth=0, ovf_entries=0, json='215e0ee01ddb049e',
        tables={'prims': '5ca986d9985e8b65', 'shade': 'dd35cc45a1966c20', 'bsdfs': '3c6eb3cc0e74b9af', 'emitters': '1f84b3aad52c6212', 'lut': '4f3edc52216d8d9d', 'flat': 'cf7a28cb301931fb', 'boxes': '6e79619957cc703d'}),
    'door_c3 beckmann': dict(n_prims=9, n_shade=9, n_bvh_nodes=0, n_flat=9, n_flat_rec=3, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=1, bvh_depth=0, ovf_entries=0, json='ddcdd7afc8eb3406',
        tables={'prims': '03ddff1155cfa376', 'shade': '4aaa7b85ba2ad8fb', 'bsdfs': 'e114180a48d9785e', 'emitters': '08243aad541404e4', 'lut': '4f3edc52216d8d9d', 'flat': '7fc751c3884737b7', 'boxes': '2243b1161a506fad'}),
    'door_c3 ggx': dict(n_prims=9, n_shade=9, n_bvh_nodes=0, n_flat=9, n_flat_rec=3, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=1, bvh_depth=0, ovf_entries=0, json='ddcdd7afc8eb3406',
        tables={'prims': '03ddff1155cfa376', 'shade': '4aaa7b85ba2ad8fb', 'bsdfs': '446712eab32a83f3', 'emitters': '08243aad541404e4', 'lut': '4f3edc52216d8d9d', 'flat': '7fc751c3884737b7', 'boxes': '2243b1161a506fad'}),
    'mirror_room': dict(n_prims=7, n_shade=7, n_bvh_nodes=0, n_flat=7, n_flat_rec=1, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=2, bvh_depth=0, ovf_entries=0, json='704b6db89757c4c2',
        tables={'prims': 'c1b6a2cdd99a250c', 'shade': 'ea36184d537b41d9', 'bsdfs': 'c489c4963fd872f8', 'emitters': '4e057d431ef0e3ad', 'lut': '4f3edc52216d8d9d', 'flat': '2b00ba32fc704f1d', 'boxes': '2243b1161a506fad'}),
    'soup 2000': dict(n_prims=2006, n_shade=2006, n_bvh_nodes=959, n_flat=2006, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=8, ovf_entries=0, json='47c33c97374c2d06',
        tables={'prims': 'efeddb54e21d325a', 'shade': '0dc8d88b3d93a888', 'bsdfs': '329f341dca0717bd', 'emitters': 'ed0152bcb79f1f80', 'lut': '4f3edc52216d8d9d', 'bvh': '4e631a55bbadf372'}),
    'caustic_c5': dict(n_prims=8, n_shade=8, n_bvh_nodes=0, n_flat=6, n_flat_rec=1, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=6, bvh_depth=0, ovf_entries=0, json='02f6c98d02ea0697',
        tables={'prims': 'f2b902f09b075d87', 'shade': 'ab21a6686c141a00', 'bsdfs': '3c6eb3cc0e74b9af', 'emitters': '1bbf3d8960a4c682', 'lut': '4f3edc52216d8d9d', 'flat': '33013f4c45743f57', 'boxes': '6e79619957cc703d'}),
    'cornell_point': dict(n_prims=17, n_shade=30, n_bvh_nodes=0, n_flat=17, n_flat_rec=0, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=4, bvh_depth=0, ovf_entries=0, json='f33058240d0a20fe',
        tables={'prims': '2c16b3705478b4d4', 'shade': 'c08a7465c2996fb6', 'bsdfs': '1537300c70f75b70', 'emitters': '2521e2d1fcecb7a1', 'lut': '4f3edc52216d8d9d', 'flat': '849bb4339794fa26', 'boxes': '69db5e6572cc00f5'}),
    'cornell_point + quad': dict(n_prims=18, n_shade=31, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=4, bvh_depth=0, ovf_entries=0, json='ce3df7754b5a146d',
        tables={'prims': '0bda5970666e4a1f', 'shade': '471ffb484f3f2624', 'bsdfs': '1537300c70f75b70', 'emitters': 'b6c2c2e7c8c9cc65', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'cornell_sky': dict(n_prims=17, n_shade=30, n_bvh_nodes=0, n_flat=17, n_flat_rec=0, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=4, bvh_depth=0, ovf_entries=0, json='9bf6f8aa0984bc4e',
        tables={'prims': '2c16b3705478b4d4', 'shade': '5e23016d4c92a3cd', 'bsdfs': '1537300c70f75b70', 'emitters': '3b2e924d6a4c8d5c', 'lut': '4f3edc52216d8d9d', 'flat': '849bb4339794fa26', 'boxes': '69db5e6572cc00f5'}),
    'cornell_sky + quad': dict(n_prims=18, n_shade=31, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=4, bvh_depth=0, ovf_entries=0, json='24a100df961884f7',
        tables={'prims': '0bda5970666e4a1f', 'shade': '3e5a18d5df905463', 'bsdfs': '1537300c70f75b70', 'emitters': '7a64bd4107f36084', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'cornell_c2 gaussian pssmlt': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='7bc1757c1fa460c7',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': 'a0bff93d8b0ad07f', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'cornell_c2 bdpt': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=90, eff_dim=72, features=0, bvh_depth=0, ovf_entries=0, json='b9765bc2aa05ba51',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'cornell_c2 bdpt no direct sampling': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=60, eff_dim=42, features=0, bvh_depth=0, ovf_entries=0, json='f35bd1a2a0aeb085',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'caustic_c5 mmlt': dict(n_prims=8, n_shade=8, n_bvh_nodes=0, n_flat=6, n_flat_rec=1, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=49, eff_dim=27, features=6, bvh_depth=0, ovf_entries=0, json='dc3d436d3447e37f',
        tables={'prims': 'f2b902f09b075d87', 'shade': 'ab21a6686c141a00', 'bsdfs': '3c6eb3cc0e74b9af', 'emitters': '1bbf3d8960a4c682', 'lut': '4f3edc52216d8d9d', 'flat': '33013f4c45743f57', 'boxes': '6e79619957cc703d'}),
    'cornell_c2 no box merge': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=18, n_box=0, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='cb914c00395fbc77',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': 'd628f1a60cc20efb'}),
    'cornell_c2 no quad merge': dict(n_prims=30, n_shade=30, n_bvh_nodes=0, n_flat=30, n_flat_rec=25, n_box=1, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='7cb4b0614b5d8523',
        tables={'prims': 'a6538615378b2d02', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': 'ffeee5b01ea8974f', 'boxes': '6e79619957cc703d'}),
    'cornell_c2 no flat loop': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=0, n_box=0, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='86e77cc2ee7611e3',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d'}),
    'cornell_c2 feat all, debug': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=15, bvh_depth=0, ovf_entries=0, json='b5eef9e7135f7da2',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'cornell_c2 as a BVH': dict(n_prims=18, n_shade=30, n_bvh_nodes=7, n_flat=18, n_flat_rec=0, n_box=0, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=3, ovf_entries=0, json='9ab8f5070f7ee847',
        tables={'prims': 'ac64e66caf3efe8e', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'bvh': '7c8435f8f2a577f5'}),
    'soup stack32': dict(n_prims=2006, n_shade=2006, n_bvh_nodes=959, n_flat=2006, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=8, bvh_depth=8, ovf_entries=36, json='d07f464efb5e0eba',
        tables={'prims': 'efeddb54e21d325a', 'shade': '0dc8d88b3d93a888', 'bsdfs': '329f341dca0717bd', 'emitters': 'ed0152bcb79f1f80', 'lut': '4f3edc52216d8d9d', 'bvh': '4e631a55bbadf372'}),
    'soup median splits': dict(n_prims=2006, n_shade=2006, n_bvh_nodes=1001, n_flat=2006, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=7, ovf_entries=0, json='0220a1380305f8e2',
        tables={'prims': 'a986df22df42e7a6', 'shade': '0dc8d88b3d93a888', 'bsdfs': '329f341dca0717bd', 'emitters': 'ed0152bcb79f1f80', 'lut': '4f3edc52216d8d9d', 'bvh': '1dcccc47e3ff601c'}),
    'soup leaves of 4': dict(n_prims=2006, n_shade=2006, n_bvh_nodes=308, n_flat=2006, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=3, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=7, ovf_entries=0, json='4405d342c46a963b',
        tables={'prims': '12d3f1f6af1f65aa', 'shade': '0dc8d88b3d93a888', 'bsdfs': '329f341dca0717bd', 'emitters': 'ed0152bcb79f1f80', 'lut': '4f3edc52216d8d9d', 'bvh': '06e39fc65be9070b'}),
    'deep chain': dict(n_prims=178, n_shade=190, n_bvh_nodes=81, n_flat=178, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=22, ovf_entries=72, json='e9cab0833b409b6e',
        tables={'prims': '798cdb9851727781', 'shade': 'ad31324a94668216', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'bvh': '1189ed513a662c28'}),
    '400 point lights': dict(n_prims=18, n_shade=430, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=4, bvh_depth=0, ovf_entries=0, json='31545ff86f407079',
        tables={'prims': '0bda5970666e4a1f', 'shade': 'c7fa1022d7465c95', 'bsdfs': '1537300c70f75b70', 'emitters': 'fc636bb14fac93e7', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    '49 records': dict(n_prims=49, n_shade=49, n_bvh_nodes=26, n_flat=49, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=4, ovf_entries=0, json='ba16d1d7cae43fab',
        tables={'prims': '315b5c7c43fcce04', 'shade': 'edf371f0252c022e', 'bsdfs': '329f341dca0717bd', 'emitters': 'f0ac9d4a0402ebad', 'lut': '4f3edc52216d8d9d', 'bvh': 'efb3af0e5007a553'}),
    '48 records': dict(n_prims=48, n_shade=48, n_bvh_nodes=0, n_flat=48, n_flat_rec=43, n_box=1, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='a863e7f985828b1a',
        tables={'prims': '1d3bba569ebb68fd', 'shade': 'a5d827d6ac8b54ea', 'bsdfs': '329f341dca0717bd', 'emitters': '1d9a17af252be297', 'lut': '4f3edc52216d8d9d', 'flat': '4da824283d21b556', 'boxes': '6e79619957cc703d'}),
    'bench C2': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=0, bvh_depth=0, ovf_entries=0, json='cad53666db7af7a1',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'bench C3': dict(n_prims=9, n_shade=9, n_bvh_nodes=0, n_flat=9, n_flat_rec=3, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=50, eff_dim=34, features=1, bvh_depth=0, ovf_entries=0, json='cca62c55042115b5',
        tables={'prims': '03ddff1155cfa376', 'shade': '4aaa7b85ba2ad8fb', 'bsdfs': 'e114180a48d9785e', 'emitters': '08243aad541404e4', 'lut': '4f3edc52216d8d9d', 'flat': '7fc751c3884737b7', 'boxes': '2243b1161a506fad'}),
    'bench C5': dict(n_prims=8, n_shade=8, n_bvh_nodes=0, n_flat=6, n_flat_rec=1, n_box=1, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=49, eff_dim=27, features=6, bvh_depth=0, ovf_entries=0, json='61b0f94cf07d53c8',
        tables={'prims': 'f2b902f09b075d87', 'shade': 'ab21a6686c141a00', 'bsdfs': '3c6eb3cc0e74b9af', 'emitters': '1bbf3d8960a4c682', 'lut': '4f3edc52216d8d9d', 'flat': '33013f4c45743f57', 'boxes': '6e79619957cc703d'}),
    'bench BD': dict(n_prims=18, n_shade=30, n_bvh_nodes=0, n_flat=18, n_flat_rec=1, n_box=3, has_plain_tri=0, bvh_leaf_shift=0, bvh_stack16=0, max_dim=90, eff_dim=72, features=0, bvh_depth=0, ovf_entries=0, json='54ef05433bd455a8',
        tables={'prims': '0bda5970666e4a1f', 'shade': '5173acc8a6a4dad0', 'bsdfs': '1537300c70f75b70', 'emitters': '08f219b8477ce116', 'lut': '4f3edc52216d8d9d', 'flat': '763a23a2e3615e43', 'boxes': '69db5e6572cc00f5'}),
    'bench SOUP': dict(n_prims=2006, n_shade=2006, n_bvh_nodes=959, n_flat=2006, n_flat_rec=0, n_box=0, has_plain_tri=1, bvh_leaf_shift=0, bvh_stack16=1, max_dim=50, eff_dim=34, features=8, bvh_depth=8, ovf_entries=0, json='25754d7ff1879ad6',
        tables={'prims': 'efeddb54e21d325a', 'shade': '0dc8d88b3d93a888', 'bsdfs': '329f341dca0717bd', 'emitters': 'ed0152bcb79f1f80', 'lut': '4f3edc52216d8d9d', 'bvh': '4e631a55bbadf372'}),
}


def canonical(out):
    return hashlib.sha256(json.dumps(out, sort_keys=True).encode()).hexdigest()[:16]


SHOWN = ("n_prims", "n_shade", "n_bvh_nodes", "n_flat", "n_flat_rec", "n_box", "has_plain_tri", "bvh_leaf_shift", "bvh_stack16", "max_dim", "eff_dim", "features")


def pin_of(out, blob):
    """What PINS holds for one run of the harness (or of the recording build, which writes the same two files)."""
    tables, at = {}, 0
    for name, n in out["tables"]:
        if n:
            tables[name] = hashlib.sha256(blob[at:at + n]).hexdigest()[:16]
        at += n
    assert at == len(blob)
    pin = {k: out["params"][k] for k in SHOWN}
    pin.update(bvh_depth=out["bvh_depth"], ovf_entries=out["ovf_entries"], json=canonical(out), tables=tables)
    return pin


def config_args(abi, kw):
    cfg = abi.make_config(**kw)
    return ["%s=%s" % (name, ("%.9g" if isinstance(getattr(cfg, name), float) else "%d") % getattr(cfg, name))
            for name, _ in cfg._fields_ if name not in ("struct_size", "reserved")]


@pytest.fixture(scope="module")
def prep(pkg, tmp_path_factory):
    d = tmp_path_factory.mktemp("scene_prep")
    exe = str(d / "scene_prep_harness")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, "-I", HOST, "-o", exe, os.path.join(ROOT, "tests", "native", "scene_prep_harness.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("DRMLT_")}
    memo = {}

    def run(sd, cfg_kw, knobs=None, key=None):
        if key is not None and key in memo:
            return memo[key]
        scene, tables = str(d / "scene.drmlt"), str(d / "tables.bin")
        sd.save(scene)
        args = ["scene=" + scene, "tables=" + tables] + config_args(pkg.abi, cfg_kw) + ["%s=%s" % kv for kv in (knobs or {}).items()]
        r = subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env)
        res = (json.loads(r.stdout), open(tables, "rb").read(), r.stderr)
        if key is not None:
            memo[key] = res
        return res
    return run


@pytest.mark.parametrize("name,scene,cfg,knobs", CASES, ids=[c[0] for c in CASES])
def test_tables_and_parameters_are_what_drmlt_create_made(pkg, prep, name, scene, cfg, knobs):
    out, blob, _ = prep(scene(pkg.scenes), cfg, knobs, key=name)
    assert out["refusal"] == ""
    got, want = pin_of(out, blob), PINS[name]
    assert got["tables"] == want["tables"], (name, out["tables"])
    assert got == want, (name, out)


def test_the_cases_take_every_path():
    """The pinned cases between them: BVH and brute force, one above and at the threshold, 32-bit stacks, an overflow area, median
    splits (fewer levels than SAH's), multi-primitive leaves, cuboids, no flat loop, plain triangles, every feature bit."""
    p = PINS
    assert p["49 records"]["n_bvh_nodes"] > 0 and p["49 records"]["n_prims"] == 49 and p["48 records"]["n_bvh_nodes"] == 0 and p["48 records"]["n_prims"] == 48
    assert p["soup 2000"]["bvh_stack16"] == 1 and p["soup stack32"]["bvh_stack16"] == 0 and p["soup stack32"]["ovf_entries"] > 0
    assert p["soup 2000"]["ovf_entries"] == 0 and p["deep chain"]["ovf_entries"] > 0 and 3 * p["deep chain"]["bvh_depth"] > 24
    assert p["soup median splits"]["tables"]["bvh"] != p["soup 2000"]["tables"]["bvh"]
    assert p["soup leaves of 4"]["bvh_leaf_shift"] == 3 and p["soup 2000"]["bvh_leaf_shift"] == 0
    assert p["cornell_c2"]["n_box"] == 3 and p["cornell_c2 no box merge"]["n_box"] == 0 and p["cornell_c2 no box merge"]["n_flat_rec"] == 18
    assert p["cornell_c2 no quad merge"]["n_prims"] == 30 and p["cornell_c2 no quad merge"]["has_plain_tri"] == 1
    assert "flat" not in p["cornell_c2 no flat loop"]["tables"] and "flat" in p["cornell_c2"]["tables"]
    assert {p[k]["features"] for k in ("cornell_c2", "door_c3 ggx", "mirror_room", "caustic_c5", "cornell_sky", "soup 2000", "cornell_c2 feat all, debug")} == {0, 1, 2, 6, 4, 8, 15}
    assert p["400 point lights"]["n_shade"] == 30 + 400 and p["400 point lights"]["features"] == 4


def test_deep_chain_reports_its_overflow_area(pkg, prep):
    """DRMLT_VERBOSE's line, as tests/test_gpu_parity.py reads it on the device."""
    _, _, log = prep(pkg.scenes.deep_chain(64), PATH8, {"DRMLT_BVH_THRESHOLD": "0", "DRMLT_VERBOSE": "1"})
    want = PINS["deep chain"]
    assert "4-wide depth %d (stack 24 in LDS + %d in memory), 0 median splits, 16-bit stack entries" % (want["bvh_depth"], want["ovf_entries"]) in log, log
    _, _, log = prep(pkg.scenes.triangle_soup(2000, 64), PATH8, {"DRMLT_BVH_MAX_DEPTH": "6", "DRMLT_VERBOSE": "1"})
    assert int(re.search(r", (\d+) median splits", log).group(1)) > 0, log   # the bound does force them
    _, _, log = prep(pkg.scenes.cornell_c2(64), PATH8, {"DRMLT_VERBOSE": "1"})
    assert "[drmlt] brute-force loop: 18 flat records, 17 of them as the faces of 3 cuboids\n" in log, log


# ---- the mirrors other tests carry by hand
def test_launch_plan_inputs_of_the_bench_scenes(pkg, prep):
    """tests/test_launch_plan.py types the bench scenes' PlanInputs by hand: they are what prepare_scene derives."""
    import test_launch_plan as lp
    for k, (n, kw, cfg) in BENCH.items():
        out, _, _ = prep(pkg.scenes.SCENES[n](res=512, **kw), cfg, key="bench " + k)
        want = getattr(lp, k)
        for f in ("n_shade", "n_bsdfs", "n_emitters", "eff_dim", "mmlt_S", "mmlt_E", "features"):
            assert out["params"][f] == want.get(f, 0), (k, f, out["params"])
        for f, v in want.items():
            if f != "scene_bytes":
                assert out["plan"][f] == v, (k, f, out["plan"])
        if "scene_bytes" in want:   # typed as a round figure (400 000 for 251 136): what the plan asks is the side of 32 MiB it lies on
            assert out["plan"]["scene_bytes"] == out["params"]["n_bvh_nodes"] * 128 + out["params"]["n_prims"] * 64
            assert max(out["plan"]["scene_bytes"], want["scene_bytes"]) <= 32 << 20, out["plan"]


def test_cornell_box_cuboids_match_the_python_rederivation(pkg, prep):
    """tests/test_box_merge.py re-derives the parallelograms in Python and expects 3 cuboids over 17 faces, the light left flat."""
    out, blob, _ = prep(pkg.scenes.cornell_c2(64), PATH8, {}, key="cornell_c2")
    P = out["params"]
    assert (P["n_flat"], P["n_box"], P["n_flat_rec"]) == (18, 3, 1)
    sizes = dict(out["tables"])
    at = sum(n for name, n in out["tables"][:[t[0] for t in out["tables"]].index("boxes")])
    assert sizes["boxes"] == (3 + 1) * 64 and sizes["flat"] == (1 + 2) * 64
    fw = np.frombuffer(blob[at:at + sizes["boxes"]], dtype="<u4").reshape(4, 16)[:, 12:15]
    halves = np.concatenate([fw & 0xFFFF, fw >> 16], axis=None)
    faces = halves[(halves & 1) == 1]
    assert len(faces) == 17 and sorted(np.bincount((fw[:3] & 1).sum(1) + ((fw[:3] >> 16) & 1).sum(1))[5:].tolist()) == [1, 2]   # 5 + 6 + 6
    shade = sorted(int(h >> 6) for h in faces)
    assert len(set(shade)) == 17 and 29 not in shade                       # the light's shading record (the last shape) stays flat
    assert not fw[3].any()                                                 # the sentinel


# ---- refusals: every message of the flattening, by a smallest scene that triggers it
def _quad(pkg):
    """One emitting rectangle in front of the camera."""
    sd = pkg.scenes.SceneData("quad")
    sd.rectangle(np.eye(4), sd.diffuse(0.5), radiance=1.0)
    sd.set_camera(pkg.scenes.lookat((0, 0, 3), (0, 0, 0), (0, 1, 0)), 40.0, 8, 8)
    return sd


def _no_shapes(pkg, sd):
    del sd.shapes[:]


def _no_emitters(pkg, sd):
    del sd.emitters[:]
    sd.shapes[0].emitter = -1


def _bad_ior(pkg, sd):
    sd.dielectric(0.0, 1.0)


def _bad_alpha(pkg, sd):
    sd.roughconductor(alpha=0.0)


def _bad_bsdf_index(pkg, sd):
    sd.shapes[0].bsdf = 1


def _bad_emitter_index(pkg, sd):
    sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0)
    sd.shapes[-1].emitter = 1


def _flat_triangle(pkg, sd):
    sd.triangle((0, 0, 0), (1, 1, 1), (2, 2, 2), 0)


def _singular_rectangle(pkg, sd):
    sd.rectangle(pkg.scenes.scale(1, 0, 1), 0)


def _sheared_rectangle(pkg, sd):
    m = np.eye(4)
    m[0, 1] = 0.5
    sd.rectangle(m, 0)


def _flat_sphere(pkg, sd):
    sd.sphere((0, 0, 0), 0.0, 0)


def _unknown_shape(pkg, sd):
    sd.sphere((0, 0, 0), 1.0, 0)
    sd.shapes[-1].type = 9


def _unlinked_emitter(pkg, sd):
    sd.triangle((0, 0, 0), (1, 0, 0), (0, 1, 0), 0)
    sd.emitters[0].shape = 1


def _negative_weight(pkg, sd):
    sd.emitters[0].sampling_weight = -1.0


def _zero_weights(pkg, sd):
    sd.emitters[0].sampling_weight = 0.0


REFUSALS = [
    (_no_shapes, "scene has no shapes"),
    (_no_emitters, "scene has no emitters"),
    (_bad_ior, "dielectric: IORs must be positive"),
    (_bad_alpha, "roughconductor: alpha must be positive"),
    (_bad_bsdf_index, "shape references an invalid bsdf"),
    (_bad_emitter_index, "shape references an invalid emitter"),
    (_flat_triangle, "degenerate triangle"),
    (_singular_rectangle, "rectangle: singular toWorld"),
    (_sheared_rectangle, "Error: 'toWorld' transformation contains shear!"),
    (_flat_sphere, "sphere: radius must be positive"),
    (_unknown_shape, "unknown shape type 9"),
    (_unlinked_emitter, "emitter/shape link mismatch"),
    (_negative_weight, "negative emitter sampling weight"),
    (_zero_weights, "emitter sampling weights sum to zero"),
]


@pytest.mark.parametrize("spoil,message", REFUSALS, ids=[r[0].__name__[1:] for r in REFUSALS])
def test_refusal(pkg, prep, native_lib, spoil, message):
    """The harness and drmlt_create in the library give the same message, before any device is looked for: with or without a GPU,
    and whatever the device index."""
    sd = _quad(pkg)
    assert prep(sd, PATH8)[0]["refusal"] == ""
    spoil(pkg, sd)
    out, blob, _ = prep(sd, PATH8)
    assert out["refusal"] == message and not any(blob)                      # nothing but the (zeroed) filter table
    cfg = pkg.abi.make_config(**PATH8)
    for device in (0, 99):
        with pytest.raises(pkg.DrmltError) as e:
            pkg.Context(cfg, sd, device=device)
        assert str(e.value).endswith(message), str(e.value)


def test_scene_checks_keep_their_order(pkg, prep):
    """BSDF validation, emitter validation, camera and filter, then the flattening's checks: a scene that is wrong in all four
    ways is refused for the first, and so on down."""
    sd = _quad(pkg)
    _flat_triangle(pkg, sd)
    sd.camera.width = 0
    sd.point_light((0, 0, 1), intensity=-1.0)
    sd.bsdfs[0].type = 17
    want = ["unsupported BSDF type 17 (supported: diffuse, dielectric, roughconductor, conductor)",
            "point light 1: intensity must be finite and non-negative", "film size must be positive", "degenerate triangle"]
    fixes = [lambda: setattr(sd.bsdfs[0], "type", 0), lambda: sd.emitters[1].radiance.__setitem__(slice(0, 3), (1.0, 1.0, 1.0)),
             lambda: setattr(sd.camera, "width", 8), lambda: None]
    for message, fix in zip(want, fixes):
        assert prep(sd, PATH8)[0]["refusal"] == message
        fix()
