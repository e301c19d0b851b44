"""Mechanical check of the hand-written Mitsuba stand-ins (tests/native/fake_mitsuba/) against the reference's real headers
(VERDICT r02 item 7). The reference side is data: tests/golden/mitsuba_signatures.json, written from the reference's headers by
tests/golden/make_mitsuba_signatures.py with the scanner below.

For every method the adaptor (drmlt-mitsuba_amd/host/mitsuba_adaptor.cpp) calls or overrides, the declaration in the fake
header must exist in the reference class of the same name -- or one of its bases -- with the same name, the same number of
parameters, the same number of defaulted parameters, the same const-ness and the same static-ness
(the reference's include/mitsuba/{core,render,bidir}/*.h, e.g. sensor.h:403-499, scene.h:1011-1115, trimesh.h:122-139,
cobject.h:77-107). The parser is a small brace / parenthesis scanner, not a C++ front end: it reads declarations at class
scope, which is all this comparison needs.

Second half: the integrator properties tools/cpu_baseline.py exports as Mitsuba XML are names (and types) that the adaptor
reads, and that the reference's DRMLT constructor reads (drmlt.cpp:193-349)."""
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mitsuba_signatures.json")
FAKE = os.path.join(ROOT, "tests", "native", "fake_mitsuba", "mitsuba", "fake_mitsuba.h")
ADAPTOR = os.path.join(ROOT, "drmlt-mitsuba_amd", "host", "mitsuba_adaptor.cpp")


def strip_comments(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"(?m)^[ \t]*#(?:[^\n]*\\\n)*[^\n]*$", " ", src)   # preprocessor lines (both arms of an #if stay: a superset)
    return re.sub(r'"(\\.|[^"\\])*"', '""', src)


def match_close(s, i, open_ch, close_ch):
    depth = 0
    for j in range(i, len(s)):
        if s[j] == open_ch:
            depth += 1
        elif s[j] == close_ch:
            depth -= 1
            if depth == 0:
                return j
    raise ValueError("unbalanced %s" % open_ch)


CLASS_RE = r"\b(?:class|struct)\s+(?:MTS_EXPORT_\w+\s+)?%s\b\s*(?:final\s*)?(:[^{;]*)?\{"


def find_class(src, name):
    """(bases, body) of `class name` in comment-free source, or None."""
    m = re.search(CLASS_RE % re.escape(name), src)
    if not m:
        return None
    start = m.end() - 1
    end = match_close(src, start, "{", "}")
    bases = []
    if m.group(1):
        for b in m.group(1)[1:].split(","):
            b = re.sub(r"\b(public|protected|private|virtual)\b", "", b)
            b = re.sub(r"<.*>", "", b).strip()
            if b:
                bases.append(b.split("::")[-1])
    return bases, src[start + 1:end]


def flatten(body):
    """class-scope text with every nested { ... } collapsed to '{}' (inline bodies, nested types)."""
    out, i = [], 0
    while i < len(body):
        if body[i] == "{":
            j = match_close(body, i, "{", "}")
            out.append("{};")
            i = j + 1
        else:
            out.append(body[i])
            i += 1
    return "".join(out)


def split_args(args):
    parts, depth, cur = [], 0, ""
    for ch in args:
        if ch in "(<[":
            depth += 1
        elif ch in ")>]":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur)
            cur = ""
        else:
            cur += ch
    if cur.strip():
        parts.append(cur)
    return [p.strip() for p in parts if p.strip() and p.strip() != "void"]


BUILTIN = {"int", "char", "long", "short", "float", "double", "bool", "unsigned", "signed", "void", "Float", "size_t", "uint32_t", "int32_t",
           "uint64_t", "int64_t", "uint8_t", "uint16_t"}


def norm_type(t, is_param):
    """Canonical token string of a parameter or return type: no parameter name, no default value, no storage / linkage words,
    no namespace qualifiers, `T const` -> `const T`, single spaces. The SAME function reads both sides, so only equality matters."""
    t = re.sub(r"[^=!<>]=[^=].*$", lambda m: m.group(0)[0], t) if is_param else t          # default value
    t = re.sub(r"\b(virtual|inline|static|explicit|MTS_EXPORT_\w+|FINLINE)\b", " ", t)
    t = re.sub(r"\b(?:mitsuba|std)::", "", t)
    t = re.sub(r"\s+", " ", t).strip()
    if is_param:
        m = re.match(r"^(.*[\s\*&])([A-Za-z_]\w*)$", t)
        if m and m.group(2) not in BUILTIN and m.group(1).strip() not in ("const", "unsigned", "signed", "struct", "class"):
            t = m.group(1)
    t = re.sub(r"\s*([\*&<>,])\s*", r"\1", t).strip()
    t = re.sub(r"^(\w+) const\b", r"const \1", t)
    return t


def methods(body, with_types=False):
    """{name: set of (n_params, n_defaults, is_const, is_static)} of the declarations at class scope
    (with_types: (n_params, n_defaults, is_const, is_static, return type, (parameter types ...)))."""
    out = {}
    flat = flatten(body)
    flat = re.sub(r"\b(public|protected|private)\s*:", ";", flat)
    for stmt in flat.split(";"):
        stmt = " ".join(stmt.split())
        if "(" not in stmt or stmt.startswith(("typedef", "using", "friend", "#")):
            continue
        m = re.search(r"([~A-Za-z_]\w*)\s*\(", stmt)
        if not m or m.group(1) in ("operator", "if", "for", "while", "return", "sizeof", "MTS_DECLARE_CLASS", "static_assert", "BOOST_STATIC_ASSERT"):
            continue
        if re.search(r"\boperator\b", stmt[:m.start() + 1]):
            continue
        close = match_close(stmt, m.end() - 1, "(", ")")
        args = split_args(stmt[m.end():close])
        tail = stmt[close + 1:]
        is_const = bool(re.match(r"\s*const\b", tail))
        is_static = bool(re.search(r"\bstatic\b", stmt[:m.start()]))
        n_def = sum(1 for a in args if re.search(r"[^=!<>]=[^=]", a))
        sig = (len(args), n_def, is_const, is_static)
        if with_types:
            sig += (norm_type(stmt[:m.start()], False), tuple(norm_type(a, True) for a in args))
        out.setdefault(m.group(1), set()).add(sig)
    return out


_golden = {}


def golden():
    """the reference side, as tests/golden/make_mitsuba_signatures.py recorded it"""
    if not _golden:
        _golden.update(json.load(open(GOLDEN)))
    return _golden


def ref_class_methods(name, with_types=False):
    """methods of reference class `name` including its bases (the names the fake class declares); (methods, header) or (None, None)."""
    rec = golden()["classes"].get(name)
    if rec is None:
        return None, None
    ms = {m: {(s[0], s[1], s[2], s[3], s[4], tuple(s[5]))[:6 if with_types else 4] for s in sigs} for m, sigs in rec["methods"].items()}
    return ms, rec["header"]


def adaptor_calls():
    src = strip_comments(open(ADAPTOR).read())
    called = set(re.findall(r"(?:->|\.|::)\s*([A-Za-z_]\w*)\s*\(", src))
    overridden = set(re.findall(r"\b(?:bool|void)\s+(preprocess|render|cancel|serialize|postprocess|configureSampler)\s*\(", src))
    return called | overridden


# fake class -> reference class (same name unless listed); classes that exist only for the tests are skipped
TEST_ONLY = {"FakeLog", "InterpolatedSpectrum"}       # InterpolatedSpectrum: only its constructor is used
STD_LIKE = {"size", "data", "c_str", "push_back", "begin", "end", "empty", "resize", "assign", "get", "count", "at", "find", "insert"}


def fake_classes(with_types=False):
    src = strip_comments(open(FAKE).read())
    names = re.findall(r"\b(?:class|struct)\s+(\w+)\s*(?::[^{;]*)?\{", src)
    out = {}
    for n in names:
        if n in TEST_ONLY:
            continue
        bases, body = find_class(src, n)
        out[n] = (bases, methods(body, with_types))
    return out


def test_parameter_and_return_types_match_the_reference_header():
    """beyond name / arity / const / static, the TYPES -- return type and every parameter type, compared as
    normalised token strings (parameter names, default values, `virtual` / `inline` / export macros and namespace qualifiers
    removed) -- of every method the adaptor calls or overrides."""
    calls = adaptor_calls() - STD_LIKE
    problems, checked = [], 0
    for cls, (bases, ms) in sorted(fake_classes(with_types=True).items()):
        wanted = {m: sigs for m, sigs in ms.items() if m in calls and m != cls}
        if not wanted:
            continue
        ref_ms, hdr = ref_class_methods(cls, with_types=True)
        if ref_ms is None:
            continue            # reported by the test above
        for m, sigs in sorted(wanted.items()):
            for sig in sorted(sigs):
                same_shape = [r for r in ref_ms.get(m, ()) if r[:4] == sig[:4]]
                if not same_shape:
                    continue    # reported by the test above
                if any(r[4:] == sig[4:] for r in same_shape):
                    checked += 1
                else:
                    problems.append("%s::%s: fake %s %s, reference (%s) %s" % (cls, m, sig[4], list(sig[5]), hdr, [(r[4], list(r[5])) for r in same_shape]))
    assert not problems, "\n".join(problems)
    assert checked >= 45, checked


def test_every_called_method_matches_the_reference_header():
    calls = adaptor_calls() - STD_LIKE
    fakes = fake_classes()
    checked, problems = [], []
    for cls, (bases, ms) in sorted(fakes.items()):
        wanted = {m: sigs for m, sigs in ms.items() if m in calls and m != cls}
        if not wanted:
            continue
        ref_ms, hdr = ref_class_methods(cls)
        if ref_ms is None:
            problems.append("%s: no such class in the reference headers" % cls)
            continue
        for m, sigs in sorted(wanted.items()):
            if m not in ref_ms:
                problems.append("%s::%s is not declared in %s (or its bases)" % (cls, m, hdr))
                continue
            for sig in sorted(sigs):
                if sig in ref_ms[m]:
                    checked.append("%s::%s%s" % (cls, m, sig))
                else:
                    problems.append("%s::%s: fake (params, defaults, const, static) = %s, reference %s has %s" % (cls, m, sig, hdr, sorted(ref_ms[m])))
    assert not problems, "\n".join(problems)
    # the check must have had teeth: the accessors SURVEY 8(b) lists are among what was compared
    names = {c.split("(")[0] for c in checked}
    for must in ("Scene::getShapes", "Scene::getSensor", "Sensor::getFilm", "PerspectiveCamera::getXFov", "PerspectiveCamera::getNearClip",
                 "PerspectiveCamera::getWorldTransform", "TriMesh::getTriangles", "TriMesh::getVertexPositions", "TriMesh::getTriangleCount",
                 "ConfigurableObject::getProperties", "Film::setBitmap", "Film::getCropSize", "Integrator::render", "Integrator::preprocess",
                 "Integrator::cancel", "Shape::getBSDF", "Shape::getEmitter", "Shape::isEmitter", "RenderQueue::signalRefresh",
                 "Properties::getString", "Properties::getInteger", "Properties::getFloat", "Properties::getBoolean", "Bitmap::convert",
                 "Sampler::getSampleCount", "Emitter::getSamplingWeight", "BSDF::getDiffuseReflectance", "Spectrum::toLinearRGB"):
        assert must in names, "%s was not compared (parser lost it?)" % must
    assert len(checked) >= 45, len(checked)


def test_every_adaptor_call_is_declared_by_some_fake_class():
    """Nothing the adaptor calls slips past the comparison above by living outside the fake classes."""
    declared = set()
    for _, (bases, ms) in fake_classes().items():
        declared |= set(ms)
    free_functions = {"drmlt_", "memset", "memcpy", "snprintf", "strlen", "time", "clock", "min", "max", "tolower", "isfinite", "sqrt", "tan", "fabs", "floor", "ceil"}
    missing = [c for c in sorted(adaptor_calls() - STD_LIKE)
               if c not in declared and not any(c.startswith(f) for f in free_functions) and not c[0].isupper()]
    # what is left must be members of the adaptor's own class (helpers defined in the adaptor itself)
    own = set(re.findall(r"\b([A-Za-z_]\w*)\s*\([^;{]*\)\s*(?:const\s*)?\{", strip_comments(open(ADAPTOR).read())))
    assert not [m for m in missing if m not in own], [m for m in missing if m not in own]


# ---------------------------------------------------------------------------------------------------------------------
XML_TYPE_TO_GETTER = {"integer": "getInteger", "string": "getString", "boolean": "getBoolean", "float": "getFloat"}


def props_read(src):
    """{name: getter} of props.getX("name" ...) calls"""
    return {m.group(2): m.group(1) for m in re.finditer(r"props\.(get(?:Integer|String|Boolean|Float|Size))\(\s*\"(\w+)\"", strip_comments_keep_strings(src))}


def strip_comments_keep_strings(src):
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def test_exported_xml_property_names_round_trip(pkg, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("cpu_baseline", os.path.join(ROOT, "tools", "cpu_baseline.py"))
    cb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cb)
    adaptor = props_read(open(ADAPTOR).read())
    reference = golden()["drmlt_properties"]
    assert len(adaptor) >= 20 and len(reference) >= 20
    # the adaptor reads every property the reference's constructor reads, with the same getter (`devices` / `device` / `seed` are its backend additions)
    for name, getter in reference.items():
        assert adaptor.get(name) == getter or (getter == "getSize" and adaptor.get(name) == "getInteger"), (name, getter, adaptor.get(name))
    assert set(adaptor) - set(reference) <= {"devices", "device", "seed", "firstStageSeeding", "workUnitsRule"}, set(adaptor) - set(reference)   # backend parameters
    for cname, conf in cb.CONFIGS.items():
        if conf["mitsuba"]["integrator"] != "drmlt":
            continue
        sd = pkg.scenes.SCENES[conf["scene"]](res=16)
        cb.scene_to_xml(pkg, sd, conf, str(tmp_path), cname)
        xml = open(os.path.join(str(tmp_path), cname + ".xml")).read()
        block = re.search(r"<integrator[^>]*>(.*?)</integrator>", xml, flags=re.S).group(1)
        props = re.findall(r"<(integer|string|boolean|float)\s+name=\"(\w+)\"", block)
        assert len(props) >= 5
        for typ, name in props:
            assert name in adaptor, "%s exports integrator property %r that the adaptor never reads" % (cname, name)
            assert adaptor[name] == XML_TYPE_TO_GETTER[typ], (cname, name, typ, adaptor[name])
        # the -D substitutions the export leaves open are property values, and every one of them is given for this config
        for var in re.findall(r"\$(\w+)", block):
            assert var in ("integrator",) or var in conf["mitsuba"] or var in ("fixEmitterPath", "acceptanceMap", "type", "technique")
