"""k_mutate_w2h's ray pass holds no packed f32 instruction, and the loop's common iteration falls through: a test of the BUILD, not
of the GPU. kernels_v4.hip is compiled to assembly once, by tests/test_w2h_isa.py's fixture (the unit's flags plus -S
--cuda-device-only -gline-tables-only, about two minutes of CPU), and an instruction belongs to the kernel's own source line at
which the chain of inlined calls that produced it starts (tools/isa_sections.py's rule).

The sections are tests/test_w2h_iter_isa.py's (lines_of), and what they held on the parent commit (063dd59) and hold now:

  ray pass   from `const bool tracing` to s_setprio(3)      382 -> 401   v_pk_* 32 -> 0, saved exec masks 0 both
  step       behind s_setprio(3) up to the hand-off         362 -> 363

Each bound is what this build produces plus 20 for compiler drift. The pass's rows -- lo, ld, bxy and uv of test_box<true, true>,
box_candidate<true> and test_flat_held (device_path.h: rows_at_point and its neighbours) -- are scalar fmaf / multiply chains: a
v_pk_fma_f32 occupies the SIMD for two passes, and the plain instructions that replace the pass's 32 packed ones cost this loop
less. The streaming loops keep the packed rows, so the assertion is asked of this section only.

The layout: k_mutate_w2<true> expects its bookkeeping branch to be skipped, and the compiler lays the ray pass directly behind the
loop head and the branch behind the hand-off. In the assembly text the one s_setprio 2 (the branch opens with it) then stands
behind s_setprio 0 and s_setprio 3 (the ray pass between them); on the parent it stood ahead of both.

That the unit's other kernels keep their machine code is tools/isa_same.py's business, parent against tree; it needs
the parent's tree and is run by hand."""
import re
import sys

from test_w2h_isa import SYMBOL, TOOLS
from test_w2h_isa import build  # noqa: F401  (the fixture: kernels_v4.hip compiled to assembly, once per run)
from test_w2h_decide_isa import sections
from test_w2h_fill_isa import by_line
from test_w2h_iter_isa import lines_of

sys.path.insert(0, TOOLS)
import isa_waits  # noqa: E402

DRIFT = 20
RAY_PASS_IS, STEP_IS = 401, 363  # parent: 382, 362


def test_sections_hold_no_more_than_they_do(build):  # noqa: F811
    lines = lines_of(build)
    s = sections(build, rays=lines["rays"], step=lines["step"])
    for name, now in (("rays", RAY_PASS_IS), ("step", STEP_IS)):
        print(name, s[name][0], "bound", now + DRIFT)
        assert 0 < s[name][0] <= now + DRIFT, (name, s[name])
    n, kinds = s["rays"]
    assert n > 200 and kinds.get("valu", 0) > 200, "the section holds the pass"
    assert kinds.get("saveexec", 0) == 0, kinds


def test_ray_pass_holds_no_packed_instruction(build):  # noqa: F811
    lo, hi = lines_of(build)["rays"]
    ins = [t for _, t in by_line(build, SYMBOL, lo, hi)]
    assert sum(t.startswith("v_fma") for t in ins) > 50, "the section holds the rows"
    packed = [t for t in ins if t.startswith("v_pk_")]
    print(len(ins), "instructions,", len(packed), "packed")
    assert not packed, packed


def test_common_iteration_falls_through(build):  # noqa: F811
    body = [l.split(";", 1)[0].strip() for l in isa_waits.kernel_body(build["text"].split("\n"), SYMBOL)]
    ins = [t for t in body if t and not t.startswith((".", "//")) and not t.endswith(":")]
    at = {k: [i for i, t in enumerate(ins) if re.match(r"s_setprio\s+%d\b" % k, t)] for k in (0, 2, 3)}
    print(at)
    assert all(len(v) == 1 for v in at.values()), at
    assert at[0][0] < at[3][0] < at[2][0], at
