"""tests/native/fake_mitsuba_emitters/mitsuba/fake_mitsuba.h -- the fake Mitsuba header the plugin is compiled against since
drmlt-mitsuba_amd/host/mitsuba_emitters.hpp calls Scene::getEmitters() and the emitters' accessors -- checked the way
tests/test_fake_mitsuba_signatures.py checks tests/native/fake_mitsuba/mitsuba/fake_mitsuba.h, with that module's scanner:

  * it is the other header plus added lines, so what that test establishes for the other header holds for this one;
  * every method it adds and mitsuba_emitters.hpp calls exists in the reference class of the same name, or one of its bases, with
    the same arity, defaulted parameters, const-ness, static-ness, return type and parameter types (the reference side is data:
    tests/golden/mitsuba_emitters_signatures.json, written by tests/golden/make_mitsuba_emitters_signatures.py);
  * nothing mitsuba_emitters.hpp calls lives outside the fake classes."""
import json
import os
import re

import test_fake_mitsuba_signatures as T

ROOT = T.ROOT
BASE_FAKE = T.FAKE
FAKE = os.path.join(ROOT, "tests", "native", "fake_mitsuba_emitters", "mitsuba", "fake_mitsuba.h")
SOURCE = os.path.join(ROOT, "drmlt-mitsuba_amd", "host", "mitsuba_emitters.hpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "mitsuba_emitters_signatures.json")
PLUGIN_FAKES = {"PointEmitter", "ConstantBackgroundEmitter", "SpotEmitter"}   # src/emitters/*.cpp: no header declares them


def classes_of(path, with_types=False):
    src = T.strip_comments(open(path).read())
    out = {}
    for n in re.findall(r"\b(?:class|struct)\s+(\w+)\s*(?::[^{;]*)?\{", src):
        if n not in T.TEST_ONLY:
            out[n] = T.methods(T.find_class(src, n)[1], with_types)
    return out


def added_methods():
    """{class: names of the methods this header declares and the other header's class of that name does not}"""
    base, out = classes_of(BASE_FAKE), {}
    for cls, ms in classes_of(FAKE).items():
        new = {m for m in ms if m != cls and m not in base.get(cls, {})}
        if new:
            out[cls] = new
    return out


def source_calls():
    src = T.strip_comments(open(SOURCE).read())
    return set(re.findall(r"(?:->|\.|::)\s*([A-Za-z_]\w*)\s*\(", src)) - T.STD_LIKE


def test_the_header_is_the_other_header_plus_added_lines():
    base = open(BASE_FAKE).read().splitlines()
    mine = iter(open(FAKE).read().splitlines())
    for n, line in enumerate(base, 1):
        assert any(line == m for m in mine), "line %d of the other header is changed or missing: %r" % (n, line)


def test_added_methods_match_the_reference_headers():
    ref = json.load(open(GOLDEN))["classes"]
    calls, added = source_calls(), added_methods()
    typed = classes_of(FAKE, with_types=True)
    assert not (set(added) & PLUGIN_FAKES), "the plugin fakes declare constructors only: %s" % {c: added[c] for c in set(added) & PLUGIN_FAKES}
    checked, problems = set(), []
    for cls, names in sorted(added.items()):
        if cls not in ref:
            problems.append("%s: no such class in the reference headers" % cls)
            continue
        for m in sorted(names):
            sigs = {(s[0], s[1], s[2], s[3], s[4], tuple(s[5])) for s in ref[cls]["methods"].get(m, ())}
            if not sigs:
                problems.append("%s::%s is not declared in %s (or its bases)" % (cls, m, ref[cls]["header"]))
            for sig in sorted(typed[cls][m]):
                if sig in sigs:
                    checked.add("%s::%s" % (cls, m))
                elif sigs:
                    problems.append("%s::%s: fake %s, reference (%s) %s" % (cls, m, sig, ref[cls]["header"], sorted(sigs)))
    assert not problems, "\n".join(problems)
    for must in ("Scene::getEmitters", "Emitter::getShape", "Emitter::getWorldTransform", "AnimatedTransform::eval",
                 "Transform::transformAffine", "Spectrum::getD65"):
        assert must in checked and must.split("::")[1] in calls, must
    # every added declaration is one that the plugin or its harness needs: nothing rides along unchecked
    assert {c.split("::")[1] for c in checked} <= calls | {"toString"}, checked


def test_the_existing_checks_hold_for_the_whole_plugin_against_this_header(monkeypatch, tmp_path):
    """tests/test_fake_mitsuba_signatures.py reads mitsuba_adaptor.cpp and the other header. Here its three comparisons run as
    they are over the plugin's whole source -- mitsuba_adaptor.cpp and mitsuba_emitters.hpp, which it includes -- against the
    header the plugin is compiled with, the reference side being both recorded files together."""
    plugin = str(tmp_path / "plugin.cpp")
    with open(plugin, "w") as f:
        f.write(open(T.ADAPTOR).read() + "\n" + open(SOURCE).read())
    merged = json.load(open(T.GOLDEN))
    for cls, rec in json.load(open(GOLDEN))["classes"].items():
        dst = merged["classes"].setdefault(cls, {"header": rec["header"], "methods": {}})
        for m, sigs in rec["methods"].items():
            dst["methods"][m] = sorted(dst["methods"].get(m, []) + [s for s in sigs if s not in dst["methods"].get(m, [])])
    monkeypatch.setattr(T, "ADAPTOR", plugin)
    monkeypatch.setattr(T, "FAKE", FAKE)
    monkeypatch.setattr(T, "_golden", merged)
    calls = T.adaptor_calls()
    assert {"getEmitters", "getShape", "getWorldTransform", "eval", "transformAffine", "getD65"} <= calls   # the scan sees the new calls
    T.test_every_called_method_matches_the_reference_header()
    T.test_parameter_and_return_types_match_the_reference_header()
    T.test_every_adaptor_call_is_declared_by_some_fake_class()


def test_every_call_is_declared_by_some_fake_class():
    declared = set()
    for ms in classes_of(FAKE).values():
        declared |= set(ms)
    missing = [c for c in sorted(source_calls()) if c not in declared and not c[0].isupper()]
    assert not missing, missing
