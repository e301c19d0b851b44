"""Generates tests/golden/mitsuba_emitters_signatures.json from a checkout of the reference fork:

  python tests/golden/make_mitsuba_emitters_signatures.py <reference checkout>

tests/native/fake_mitsuba_emitters/mitsuba/fake_mitsuba.h is tests/native/fake_mitsuba/mitsuba/fake_mitsuba.h plus declarations. For
every method a class of the first declares and the class of the same name in the second does not, the declarations that the
reference's class of that name -- with its bases -- holds, read by the scanner of tests/test_fake_mitsuba_signatures.py and the
header walk of make_mitsuba_signatures.py. Run again whenever that header gains a class or a method. The JSON is data, in the
format of mitsuba_signatures.json's "classes".
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mitsuba_emitters_signatures.json")
sys.path.insert(0, os.path.dirname(HERE))

import test_fake_mitsuba_emitters_signatures as E  # noqa: E402

spec = importlib.util.spec_from_file_location("make_mitsuba_signatures", os.path.join(HERE, "make_mitsuba_signatures.py"))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)


def main(ref):
    srcs = G.headers(ref)
    classes = {}
    for cls, names in sorted(E.added_methods().items()):
        ms, hdr = G.class_methods(srcs, cls, set())
        if ms is None:
            continue
        classes[cls] = {"header": hdr, "methods": {m: sorted([s[0], s[1], s[2], s[3], s[4], list(s[5])] for s in ms[m]) for m in sorted(names) if m in ms}}
    with open(OUT, "w") as f:
        json.dump({"classes": classes}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d classes" % (OUT, len(classes)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
