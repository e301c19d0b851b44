"""k_mutate_w2h fills the proposal rows in one flattened pass with one Philox site: a test of the BUILD, not of the GPU. kernels_v4.hip
is compiled to assembly once, as tests/test_w2h_isa.py does it (the unit's flags plus -S --cuda-device-only -gline-tables-only,
about two minutes of CPU), and an instruction belongs to the kernel's own source line at which the chain of inlined calls that
produced it starts (tools/isa_sections.py's rule).

The section is the kernel's lines from `// ---- proposals` to `// ---- begin`. With the two loops (k_mutate_w2<false> keeps them)
it held 633 instructions on the commit before this file, 40 of them the generator multiplies of two Philox copies
(v_mad_u64_u32 with a zero addend; three more with a register addend are address arithmetic). With the one pass the build
produces 359; the bound is that plus 20 for compiler drift. The second-stage tail is the line that calls
row_fill_second_pair_drawn: its reads, ONE wait, then the rotation, then the stores."""
import re

from test_w2h_isa import SYMBOL
from test_w2h_isa import build  # noqa: F401  (the fixture: kernels_v4.hip compiled to assembly, once per run)
from test_w2h_decide_isa import marker

SYMBOL_STREAMED = "_Z11k_mutate_w2ILb0EEv7DParamsjj"  # k_mutate_w2<false>
SECTION_IS = 359   # what the build produces (633 with the two loops)
SECTION_MAX = SECTION_IS + 20
PHILOX_MULTIPLIES = 20  # one philox4x32_10: ten rounds of two 32 x 32 -> 64 multiplies


def by_line(build, symbol, lo, hi):  # noqa: F811
    """[(source line of kernels_v4.hip, instruction)] of `symbol` for the lines lo .. hi"""
    lines = build["text"].split("\n")
    st = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    en = next(i for i in range(st, len(lines)) if "s_endpgm" in lines[i])
    out, cur = [], None
    for l in lines[st:en]:
        if re.match(r"\s*\.loc\s", l):
            sites = re.findall(r"([\w.+-]+):(\d+):\d+", l.split(";", 1)[1] if ";" in l else "")
            if sites and int(sites[-1][1]) > 0:
                cur = int(sites[-1][1]) if sites[-1][0] == build["file"] else None
            continue
        t = l.split(";", 1)[0].strip()
        if not t or t.startswith((".", "//")) or t.endswith(":") or re.match(r"\.?\w+:", t):
            continue
        if cur is not None and lo <= cur <= hi:
            out.append((cur, t))
    return out


def section(build, symbol):  # noqa: F811
    src, (first, last) = build["src"], build["kernel"]
    lo = marker(src, first, last, "// ---- proposals")
    hi = marker(src, lo, last, "// ---- begin") - 1
    return lo, hi, by_line(build, symbol, lo, hi)


def generator_multiplies(ins):
    return [t for _, t in ins if t.startswith("v_mad_u64_u32") and re.search(r",\s*0$", t)]


def test_one_philox_site_and_the_size(build):  # noqa: F811
    lo, hi, ins = section(build, SYMBOL)
    assert any("row_fill_second_pair_drawn(" in l for l in build["src"][lo:hi]), "the section holds the pass"
    print(len(ins), "instructions,", len(generator_multiplies(ins)), "generator multiplies")
    assert len(generator_multiplies(ins)) == PHILOX_MULTIPLIES
    assert 200 < len(ins) <= SECTION_MAX, len(ins)


def test_second_tail_waits_once(build):  # noqa: F811
    lo, hi, ins = section(build, SYMBOL)
    call = marker(build["src"], lo, hi, "row_fill_second_pair_drawn(")
    tail = [t for line, t in ins if line == call]
    reads = [i for i, t in enumerate(tail) if t.startswith("ds_read")]
    writes = [i for i, t in enumerate(tail) if t.startswith("ds_write")]
    rotation = [i for i, t in enumerate(tail) if t.startswith(("v_cos_f32", "v_sqrt_f32"))]
    assert reads and writes and len(rotation) == 2, "the tail holds its reads, one rotation (a cosine, a root) and its stores"
    assert reads[-1] < rotation[0] and rotation[-1] < writes[0], tail
    waits = [i for i in range(reads[0], writes[0]) if tail[i].startswith("s_waitcnt")]
    print(len(tail), "instructions; waits at", waits, "reads", reads, "rotation", rotation, "stores", writes)
    assert len(waits) == 1 and reads[-1] < waits[0] < rotation[0], [tail[i] for i in waits]


def test_the_streamed_kernel_keeps_its_two_loops(build):  # noqa: F811
    _, _, ins = section(build, SYMBOL_STREAMED)
    assert len(generator_multiplies(ins)) == 2 * PHILOX_MULTIPLIES
