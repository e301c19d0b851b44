"""k_mutate_w2h's loop iteration carries less around its arithmetic: a test of the BUILD, not of the GPU. kernels_v4.hip is compiled to
assembly once, by tests/test_w2h_isa.py's fixture (the unit's flags plus -S --cuda-device-only -gline-tables-only, about two
minutes of CPU), and an instruction belongs to the kernel's own source line at which the chain of inlined calls that produced it
starts (tools/isa_sections.py's rule).

The sections, by the kernel's own lines, and what they held on the parent commit (9855a45) and hold now:

  ray pass   from `const bool tracing` to s_setprio(3)      388 -> 382   saved exec masks 4 -> 0, branches 14 -> 11
  step       behind s_setprio(3) up to the hand-off         374 -> 362   v_sqrt_f32 3 -> 2
  hand-off   `// hand the shadow ray` to the loop's end       20 -> 16    s_nop 4 -> 0, v_mov_b32 4 -> 3, nine swaps both
  loop head  `for (;;)` to the bookkeeping branch's test      20 -> 20

Each bound is what this build produces plus 20 for compiler drift. The ray pass's tail is selects on the winner's half-word
(trace_held, device_path.h), so nothing of the pass stands behind a saved exec mask. The hand-off's three copies of the ray's
origin -- a swap writes both operands and the shadow ray starts where the bounce ray does -- stand ahead of the block of swaps:
no s_nop between a copy and the swap that reads it. The step has
no triangle-light arm (HeldLightTablesT<true>): its two roots are the distance to the light point and the cosine-hemisphere's.

That the unit's other kernels keep their machine code is tools/isa_same.py's business, parent against tree; it needs
the parent's tree and is run by hand."""
import re

from test_w2h_isa import SYMBOL
from test_w2h_isa import build  # noqa: F401  (the fixture: kernels_v4.hip compiled to assembly, once per run)
from test_w2h_decide_isa import marker, sections
from test_w2h_fill_isa import by_line

DRIFT = 20
RAY_PASS_IS, STEP_IS, HAND_OFF_IS, LOOP_HEAD_IS = 382, 362, 16, 20  # parent: 388, 374, 20, 20
RAY_PASS_MASKS_WERE = 4
SWAPS = 9


def lines_of(build):  # noqa: F811
    src, (first, last) = build["src"], build["kernel"]
    loop = marker(src, first, last, "for (;;) {")
    book = marker(src, loop, last, "if (pmask && (__popcll(pmask)")
    tracing = marker(src, book, last, "const bool tracing")
    prio3 = marker(src, tracing, last, "s_setprio(3)")
    hand = marker(src, prio3, last, "// hand the shadow ray")
    end = marker(src, hand, last, "// the epilogue of k_mutate_v4")
    assert any("trace_held(" in l for l in src[tracing:prio3]) and any("path_step_diffuse<" in l for l in src[prio3:hand])
    return dict(head=(loop, book), rays=(tracing, prio3), step=(prio3 + 1, hand - 1), handoff=(hand, end - 1))


def test_sections_hold_no_more_than_they_did(build):  # noqa: F811
    s = sections(build, **lines_of(build))
    for name, now in (("rays", RAY_PASS_IS), ("step", STEP_IS), ("handoff", HAND_OFF_IS), ("head", LOOP_HEAD_IS)):
        print(name, s[name][0], "bound", now + DRIFT)
        assert 0 < s[name][0] <= now + DRIFT, (name, s[name])
    n, kinds = s["rays"]
    assert n > 200 and kinds.get("valu", 0) > 200, "the section holds the pass"
    assert kinds.get("saveexec", 0) < RAY_PASS_MASKS_WERE, kinds


def test_hand_off_copies_stand_ahead_of_the_swaps(build):  # noqa: F811
    lo, hi = lines_of(build)["handoff"]
    ins = [t for _, t in by_line(build, SYMBOL, lo, hi)]
    swaps = [i for i, t in enumerate(ins) if t.startswith("v_permlane32_swap")]
    assert len(swaps) == SWAPS, ins
    for i, t in enumerate(ins):
        m = re.match(r"v_mov_b32\w*\s+(v\d+),", t)
        if not m:
            continue
        reader = next((j for j in swaps if j > i and re.search(r"\b%s\b" % m.group(1), ins[j])), None)
        if reader is not None:
            assert not [u for u in ins[i + 1:reader] if u.startswith("s_nop")], ins[i:reader + 1]


def test_step_has_no_triangle_light_arm(build):  # noqa: F811
    lo, hi = lines_of(build)["step"]
    roots = [t for _, t in by_line(build, SYMBOL, lo, hi) if t.startswith("v_sqrt_f32")]
    print(roots)
    assert len(roots) == 2, roots  # the distance to the light point, the cosine-weighted hemisphere; the parent's third was sqrt(1 - sx)
