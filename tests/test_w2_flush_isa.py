"""k_mutate_w2's film flush (kernels_v4.hip: w2_film_put_channel, w2_flush_passes, w2_flush) issues its no-return atomics and never
waits for them: a test of the BUILD, not of the GPU. kernels_v4.hip is compiled to assembly once for the whole run (the `build`
fixture below, which tests/test_w2h_isa.py and the modules beside it import), with the unit's flags from the Makefile plus -S
--cuda-device-only -gline-tables-only (about a minute of CPU), and the instructions of k_mutate_w2 that the
flush's source lines produced -- theirs, and those of everything they inline -- are read with tools/isa_waits.py:

  inside the pass loops (w2_film_put_channel, w2_flush_passes): no s_waitcnt names vmcnt, no vector-memory load;
  outside them (w2_flush): per flush site exactly one vector-memory load, the staging of the filter table, with one wait.

The atomics are counted too: the test would pass vacuously on a section without any. The line ranges are read from the source."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import bsdf_probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_waits  # noqa: E402

FLUSH_SITES = 3  # the bookkeeping branch's and the epilogue's two
SYMBOL = "_Z11k_mutate_w2ILb0EEv7DParamsjj"  # k_mutate_w2<false>: the source name alone matches both instantiations
KERNEL_HEAD = " k_mutate_w2(DParams P,"     # the template's __global__ line in kernels_v4.hip
UNIT = "kernels_v4"                          # the translation unit of k_mutate_v4 and k_mutate_w2


def routine_lines(src, head):
    """first and last line (1-based) of the routine whose definition starts with `head` at the beginning of a line"""
    first = next(i for i, l in enumerate(src) if l.startswith(head))
    last = next(i for i in range(first, len(src)) if src[i] == "}")
    return first + 1, last + 1


_BUILT = {}  # the one compilation of a run: a module-scoped fixture that other modules import is set up once per module


@pytest.fixture(scope="module")
def build(tmp_path_factory):
    """kernels_v4.hip compiled to assembly with line tables: the file, its text, the source lines and k_mutate_w2's (first, last)"""
    if not _BUILT:
        hipcc = bsdf_probe._make_var("HIPCC")[0]
        if not (os.path.exists(hipcc) or shutil.which(hipcc)):
            pytest.skip("no hipcc")
        out = str(tmp_path_factory.mktemp("w2_isa") / (UNIT + ".s"))
        r = subprocess.run([hipcc, "--offload-arch=" + bsdf_probe._make_var("ARCH")[0], *bsdf_probe.flags(UNIT), "-S", "--cuda-device-only",
                            "-gline-tables-only", "-o", out, UNIT + ".hip"], cwd=CSRC, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        src = open(os.path.join(CSRC, UNIT + ".hip")).read().split("\n")
        first = next(i for i, l in enumerate(src) if "__global__" in l and KERNEL_HEAD in l)
        last = next(i for i in range(first, len(src)) if src[i] == "}")
        _BUILT.update(asm=out, text=open(out).read(), src=src, kernel=(first + 1, last + 1), file=UNIT + ".hip")
    return _BUILT


@pytest.fixture(scope="module")
def flush_asm(build):
    src = build["src"]
    put = routine_lines(src, "template <bool BOX> DEV void w2_film_put_channel(")
    passes = routine_lines(src, "template <bool BOX> DEV void w2_flush_passes(")
    flush = routine_lines(src, "DEV void w2_flush(")
    assert put[1] < passes[0] and passes[1] < flush[0], "the pass loops' routines stand together, in front of w2_flush"
    first, last = build["kernel"][0] - 1, build["kernel"][1] - 1
    sites = [i + 1 for i in range(first, last) if re.search(r"\bw2_flush\(", src[i])]  # the kernel's own calls
    assert len(sites) == FLUSH_SITES, sites
    ranges = {"passes": (put[0], passes[1]), "staging": flush}
    print("source lines:", ranges, "flush sites:", sites)
    return isa_waits.scan(build["text"], SYMBOL, build["file"], ranges), sites


def test_no_wait_for_the_atomics_inside_the_pass_loops(flush_asm):
    res, _ = flush_asm
    c = res["passes"]
    print(dict((k, v) for k, v in c.items() if k != "where"), c["where"])
    # the box nest and the tabulated nest of every site, one atomic each (the three channels are three lanes)
    assert c["vmem_atomic"] == 2 * FLUSH_SITES
    assert c["lds"] > 0, "the queue rows and the staged table are read from LDS"
    assert c["wait_vmcnt"] == 0, c["where"]
    assert c["vmem_load"] == 0, c["where"]


def test_one_staging_load_and_its_wait_outside_them(flush_asm):
    res, sites = flush_asm
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
