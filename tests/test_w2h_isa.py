"""k_mutate_w2h's ray pass reads no memory, and its film flush is k_mutate_w2's: a test of the BUILD, not of the GPU. kernels_v4.hip
is compiled to assembly once, by tests/test_w2_flush_isa.py's `build` fixture (the unit's flags plus -S --cuda-device-only
-gline-tables-only, about a minute of CPU), which this module hands on to the four that import it from here.

The ray pass is the kernel's source lines between its s_setprio(0) and s_setprio(3). tools/isa_sections.py counts the
instructions those lines produced, with everything they inline (trace_held, test_box, test_flat): none of them is a scalar
load or a vector-memory load. The same is asked of the assembly text between the two s_setprio instructions, where
s_buffer_load*, buffer_load* and scratch_load* are looked for as well. Both sections must hold the pass's arithmetic (the
reciprocals of three cuboid tests and one flat test), or the test would pass on an empty section.

The flush: what tests/test_w2_flush_isa.py asserts for k_mutate_w2, by tools/isa_waits.py, on this kernel's three flush sites."""
import ast
import os
import re
import subprocess
import sys

from test_w2_flush_isa import build, routine_lines  # noqa: F401  (the fixture: kernels_v4.hip compiled to assembly, once per run)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import isa_waits  # noqa: E402

SYMBOL = "_Z11k_mutate_w2ILb1EEv7DParamsjj"  # k_mutate_w2<true>
FLUSH_SITES = 3  # the bookkeeping branch's and the epilogue's two
LOADS = ("s_load", "s_buffer_load", "flat_load", "global_load", "buffer_load", "scratch_load")
RCPS = 3 * 3 + 1  # test_box: one per slab; test_flat: one


def test_ray_pass_by_source_lines(build):
    src, (first, last) = build["src"], build["kernel"]
    lo = next(i for i in range(first, last) if "s_setprio(0)" in src[i]) + 1   # 1-based line of the marker
    hi = next(i for i in range(lo, last) if "s_setprio(3)" in src[i]) + 1
    assert any("trace_held(" in l for l in src[lo:hi - 1])
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "isa_sections.py"), build["asm"], SYMBOL, build["file"], "rays=%d-%d" % (lo + 1, hi - 1)],
                       check=True, capture_output=True, text=True)
    print(r.stdout)
    m = re.search(r"^rays\s+(\d+)\s+(\{.*\})$", r.stdout, re.M)
    assert m, r.stdout
    n, kinds = int(m.group(1)), ast.literal_eval(m.group(2))
    assert n > 200 and kinds.get("valu", 0) > 200
    assert kinds.get("s_load", 0) == 0 and kinds.get("vmem_load", 0) == 0 and kinds.get("vmem", 0) == 0, kinds


def test_ray_pass_by_the_assembly_text(build):
    body = [l.split(";", 1)[0].strip() for l in isa_waits.kernel_body(build["text"].split("\n"), SYMBOL)]
    ins = [t for t in body if t and not t.startswith((".", "//")) and not t.endswith(":")]
    lo = [i for i, t in enumerate(ins) if re.match(r"s_setprio\s+0\b", t)]
    hi = [i for i, t in enumerate(ins) if re.match(r"s_setprio\s+3\b", t)]
    assert len(lo) == 1 and len(hi) == 1 and lo[0] < hi[0], (lo, hi)
    seg = ins[lo[0]:hi[0]]
    loads = [t for t in seg if t.split()[0].startswith(LOADS)]
    print(len(seg), "instructions,", sum(t.startswith("v_rcp") for t in seg), "reciprocals")
    assert sum(t.startswith("v_rcp_f32") for t in seg) == RCPS
    assert not loads, loads
    assert not [t for t in seg if t.startswith("s_waitcnt") and "vmcnt" in t]


def test_flush_as_k_mutate_w2s(build):
    src, (first, last) = build["src"], build["kernel"]
    put = routine_lines(src, "template <bool BOX> DEV void w2_film_put_channel(")
    passes = routine_lines(src, "template <bool BOX> DEV void w2_flush_passes(")
    flush = routine_lines(src, "DEV void w2_flush(")
    sites = [i + 1 for i in range(first - 1, last) if re.search(r"\bw2_flush\(", src[i])]
    assert len(sites) == FLUSH_SITES, sites
    res = isa_waits.scan(build["text"], SYMBOL, build["file"], {"passes": (put[0], passes[1]), "staging": flush})
    c = res["passes"]
    print(dict((k, v) for k, v in c.items() if k != "where"), c["where"])
    assert c["vmem_atomic"] == 2 * FLUSH_SITES
    assert c["lds"] > 0
    assert c["wait_vmcnt"] == 0 and c["vmem_load"] == 0, c["where"]
    c = res["staging"]
    print(dict((k, v) for k, v in c.items() if k != "where"), c["where"])
    assert c["vmem_atomic"] == 0
    for site in sites:
        mine = [t for _, s, t in c["where"] if s == site]
        loads = [t for t in mine if t.startswith(("flat_load", "global_load"))]
        waits = [t for t in mine if t.startswith("s_waitcnt")]
        assert len(loads) == 1 and len(waits) == 1, (site, mine)
        assert mine.index(loads[0]) < mine.index(waits[0]), (site, mine)
    assert c["vmem_load"] == FLUSH_SITES and c["wait_vmcnt"] == FLUSH_SITES, c["where"]
