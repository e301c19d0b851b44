"""k_mutate_w2h decides by selects and tests once per wave whether its step needs the emitter-hit block: a test of the BUILD, not
of the GPU. kernels_v4.hip is compiled to assembly once, as tests/test_w2h_isa.py does it (the unit's flags plus -S
--cuda-device-only -gline-tables-only, about two minutes of CPU), and tools/isa_sections.py counts the instructions that the
kernel's own source lines produced, with everything they inline.

The decide is the lines from the kernel's `---- decide` marker to its call of mh_resolve_kind (w2h_decide inlined). With the
state machine's arms (mh_decide and the digest written out, as in k_mutate_w2) those lines made 324 instructions behind 14 saved
exec masks on the commit before this file; the select-only routine made 214 in a prototype that did not fit the registers. The
section may hold 244: the 30 between are what fitting it may cost. What is left behind a saved exec mask is the importance-map
arm and mh_resolve_kind's run-ahead arm, both wave-uniform.

The step is the lines between s_setprio(3) and the hand-off of the shadow ray. It had three branches; the wave's test in front
of the emitter-hit block is the fourth, and the block itself stays straight-line code (a fifth or sixth branch means the compiler
split it by lane again)."""
import ast
import os
import re
import subprocess
import sys

import pytest

from test_w2h_isa import SYMBOL, TOOLS
from test_w2h_isa import build  # noqa: F401  (the fixture: kernels_v4.hip compiled to assembly, once per run)

DECIDE_MAX = 244        # 324 with the arms, 214 in the prototype
DECIDE_MASKS_WERE = 14  # saved exec masks of the section with the arms
STEP_BRANCHES = 3 + 1   # the step's three, and the wave's test of the emitter-hit block


def sections(build, **ranges):  # noqa: F811
    r = subprocess.run([sys.executable, os.path.join(TOOLS, "isa_sections.py"), build["asm"], SYMBOL, build["file"],
                        *["%s=%d-%d" % (k, lo, hi) for k, (lo, hi) in ranges.items()]], check=True, capture_output=True, text=True)
    print(r.stdout)
    out = {}
    for name in ranges:
        m = re.search(r"^%s\s+(\d+)\s+(\{.*\})$" % name, r.stdout, re.M)
        assert m, r.stdout
        out[name] = (int(m.group(1)), ast.literal_eval(m.group(2)))
    return out


def marker(src, first, last, text):
    """1-based number of the first line of the kernel from `first` on that holds `text`"""
    return next(i for i in range(first - 1, last) if text in src[i]) + 1


def test_decide_by_selects(build):  # noqa: F811
    src, (first, last) = build["src"], build["kernel"]
    lo = marker(src, first, last, "// ---- decide")
    hi = marker(src, lo, last, "mh_resolve_kind(")
    assert any("w2h_decide(" in l for l in src[lo:hi]), "the section holds the call"
    n, kinds = sections(build, decide=(lo, hi))["decide"]
    assert n > 100 and kinds.get("v_cndmask", 0) >= 20, "the section holds the decide"
    assert n <= DECIDE_MAX, n
    assert kinds.get("saveexec", 0) < DECIDE_MASKS_WERE, kinds


def test_step_has_one_more_branch(build):  # noqa: F811
    src, (first, last) = build["src"], build["kernel"]
    lo = marker(src, first, last, "s_setprio(3)") + 1
    hi = marker(src, lo, last, "// hand the shadow ray") - 1
    assert any("path_step_diffuse<" in l for l in src[lo - 1:hi])
    n, kinds = sections(build, step=(lo, hi))["step"]
    assert n > 300 and kinds.get("valu", 0) > 250, "the section holds the step"
    assert kinds.get("s_cbranch", 0) == STEP_BRANCHES, kinds
