"""Generates tests/golden/mitsuba_signatures.json from a checkout of the reference fork:

  python tests/golden/make_mitsuba_signatures.py <reference checkout>

For every class of the fake Mitsuba headers (tests/native/fake_mitsuba/), the declarations that the reference's class of the same
name -- with its bases -- holds for the method names the fake class declares, read by the scanner of
tests/test_fake_mitsuba_signatures.py from include/mitsuba/{core,render,bidir}/*.h; and the integrator properties the reference's
DRMLT constructor reads (src/integrators/drmlt/drmlt.cpp). Run again whenever the fake headers gain a class or a method. The JSON it
writes is data: (parameter count, defaulted parameters, const, static, return type, parameter types) per declaration.
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mitsuba_signatures.json")

spec = importlib.util.spec_from_file_location("sigtest", os.path.join(os.path.dirname(HERE), "test_fake_mitsuba_signatures.py"))
T = importlib.util.module_from_spec(spec)
spec.loader.exec_module(T)


def headers(ref):
    srcs = {}
    for sub in ("core", "render", "bidir"):
        d = os.path.join(ref, "include", "mitsuba", sub)
        for fn in sorted(os.listdir(d)):
            if fn.endswith(".h"):
                srcs[sub + "/" + fn] = T.strip_comments(open(os.path.join(d, fn), errors="replace").read())
    return srcs


def class_methods(srcs, name, seen):
    """methods of reference class `name` including its bases: (methods, header) or (None, None); the first header that declares it"""
    if name in seen:
        return {}, None
    seen.add(name)
    for hdr, src in srcs.items():
        found = T.find_class(src, name)
        if not found:
            continue
        bases, body = found
        ms = T.methods(body, with_types=True)
        for b in bases:
            bm, _ = class_methods(srcs, b, seen)
            for k, v in (bm or {}).items():
                ms.setdefault(k, set()).update(v)
        return ms, hdr
    return None, None


def main(ref):
    srcs = headers(ref)
    classes = {}
    for cls, (_, fake_ms) in sorted(T.fake_classes().items()):
        ms, hdr = class_methods(srcs, cls, set())
        if ms is None:
            continue
        classes[cls] = {"header": hdr,
                        "methods": {m: sorted([s[0], s[1], s[2], s[3], s[4], list(s[5])] for s in ms[m]) for m in sorted(fake_ms) if m in ms}}
    props = T.props_read(open(os.path.join(ref, "src", "integrators", "drmlt", "drmlt.cpp")).read())
    with open(OUT, "w") as f:
        json.dump({"classes": classes, "drmlt_properties": dict(sorted(props.items()))}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d classes, %d properties" % (OUT, len(classes), len(props)))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
