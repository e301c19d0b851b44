"""The chain-kernel generations of technique=path run the same chains because the transition arithmetic exists once
(csrc/device_sampler.h). Pinned in the source text: the two constants only the orbital stages use occur in one routine each, and
the kernels call no transition kernel themselves. (device_bidir.h: MSampler, out of scope on purpose -- see its comment.)"""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")


def _uses(name):
    """file name -> occurrences of `name` outside its #define, over csrc/"""
    found = {}
    for path in glob.glob(os.path.join(CSRC, "*")):
        if not os.path.isfile(path):
            continue
        text = "".join(l for l in open(path, errors="replace") if not l.startswith("#define " + name))
        n = len(re.findall(r"\b%s\b" % name, text))
        if n:
            found[os.path.basename(path)] = n
    return found


@pytest.mark.parametrize("name", ["WC_DISPERSION", "ORBITAL_SCALE"])
def test_constant_is_used_by_one_routine(name):
    uses = _uses(name)
    uses.pop("device_bidir.h", None)
    assert uses == {"device_sampler.h": 1}


def test_kernels_call_no_transition_kernel():
    for name in ("kernels.hip", "kernels_v3.hip", "kernels_v4.hip", "chain_path.h"):  # technique=path's units and what they share
        text = open(os.path.join(CSRC, name)).read()
        assert re.findall(r"\b(kelemen_sample|gaussian_sample|cos_rev)\s*\(", text) == [], name
