"""The device's ray loops, ray by ray (tests/native/ray_probe.hip, built under both device flag sets of the library and run as a
child process, 27 runs a build, over the parameter block and the tables csrc/scene_prep.h makes) against a brute force over the
scene's shapes in fp64 and the oracle's own shape loop in double and in float -- tests/ray_probe.py has the scenes, the rays, the
references and the rule:

    |device - fp64| <= 32 * max |oracle32 - fp64| + 4 ulp        per quantity, scene and ray class.

Measured on an MI355X (profiles/r18_ray_probe.json: every ratio per preparation, op, class and quantity), the two builds side by
side, the figures the larger of the two. The builds' outputs are bit-equal but for 995 of 118 448 words of trace0 and of trace15
on open_glass_box (last bits of t, u, v on the rotated boxes).

  Nine scenes in fifteen preparations, 26894 to 29612 rays a scene, delta 1.16e-5 (two_spheres) .. 1.98e-5 (flat_mix even).
  Undecided: at most 0.76 % of a class 1 to 6 (deep_chain, axis-parallel); 46 - 77 % of class 7.
  Decided rays: every op names the reference's shape and misses on every decided miss, on every ray; 0 undecided rays return
  anything but an allowed candidate; the 27 500 any-hit rows agree with the reference; nothing non-finite.
  Worst device error as a share of the bound, classes 1 to 6, by op: trace0 and held 0.06, trace15, brute and brute_vec 0.12
  (two_spheres, shadow rays: the sphere), bvh16, bvh32 and bvh32_cap12 0.04. By quantity: t 0.12, point 0.09, rebuilt point on
  the ray 0.06, on the sphere 0.05. Class 7: t 0.24, point 0.18 (two_box_room, trace0), on the ray 0.03, on the sphere 0.01.
  Under the rule's plain bound -- 4 ulp whatever the cosine, recorded as t_plain and p_plain -- classes 1 to 6 are at 0.47 at
  most; class 7's undecided rays reach 858 x (soup, bvh16, rays aimed at the triangles' edges and vertices), which is why a candidate of an
  undecided ray is held to 4 ulp / c in the place of 4 ulp (tests/ray_probe.py has the references' own figures).
  held = trace0 on all rays of cornell_c2, one_box_room and two_box_room; every op that traverses gives the same bits under
  trace_vote 1, 10 and 1024 and over the permuted ray list, on the soup under both stack widths and on both chain trees.

Found by this module and fixed in csrc/device_path.h: a ray parallel to a plain triangle's plane has t = +inf, which passes
t <= h.t when the ray has no far end (tmax = INFINITY, every closest-hit ray of the library); where one of the triangle's rows u, v
is orthogonal to the ray too, that coordinate and w = 1 - (u + v) are inf * 0 = NaN, fminf skips a NaN, and min3(u, v, w) >= 0 held:
a hit at t = +inf with NaN barycentrics (test_nothing_is_non_finite: 7 axis-parallel rays of deep_chain, whose triangles have an
edge along x, in bvh16, bvh32, bvh32_cap12 and trace15 of both its trees). intersect_prim, intersect_leaf and test_flat<true> now
ask w >= 0 as well; test_flat<false> is as it was. With the fix: no finding in either build. This module is the header's guard:
tests/test_ray_probe.py shows the cause with a numpy stand-in and would stay green if the terms were taken out again.

Which test turns red when the device code is broken on purpose (each tried once on the GPU in a scratch copy of the headers,
build `kernels`; only arithmetic that cannot alter an address or a loop's exit):
  no `hc & 4` flip in trace_flat's tail          -> t_and_the_rebuilt_point (120 findings: point and on-ray 1.9e5 x the bound),
                                                    held_equals_streamed (1952 - 2451 rays of the three held scenes)
  (lda < 0) == leave in box_candidate            -> decided_rays_name_the_references_shape, misses_and_windows,
                                                    undecided_rays_return_an_allowed_candidate (70 each), t_and_the_rebuilt_point (124)
  a < f for a <= f in the node test              -> decided_rays_name_the_references_shape, undecided_rays_return_an_allowed_candidate,
                                                    any_hit_rays (55 each: misses behind flat, axis-aligned boxes)
  v >= u for v > u in every PRIM_QUAD2 split     -> nothing: it changes the answer only where v == u exactly, on the shared
                                                    diagonal, where both sub-triangles are allowed candidates and rebuild one point
  !(tnear > tmin) for !(tnear >= tmin)           -> nothing: it changes the answer only where a cuboid's entry distance equals tmin
                                                    to the bit, which no ray of the lists does, and where the rule allows both faces
"""
import os

import pytest

import bsdf_probe as bp
import ray_probe as rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg, ob, tmp_path_factory):
    """Scenes, tables, rays and the references, computed once for both builds."""
    return rp.prepare(pkg, ob, tmp_path_factory.mktemp("ray_probe_ref"))


@pytest.fixture(scope="module")
def measured(world, tmp_path_factory):
    """{build: (report, findings, raw output)}: all child runs of the module. A run that fails ends them."""
    tmp = tmp_path_factory.mktemp("ray_probe")
    out = {}
    for unit in rp.UNITS:
        exe, _ = rp.build(tmp, unit)
        try:
            rep, raw = rp.measure(rp.Probe(exe, tmp), world)
        except bp.ProbeDied as e:
            out[unit] = e
            break
        out[unit] = (rep, rp.findings(rep), raw)
    return out


@pytest.fixture(params=rp.UNITS)
def found(request, world, measured):
    """The findings of one build; after a failed run the tests of that build fail and the later build's skip."""
    m = measured.get(request.param)
    if m is None:
        pytest.skip("not run: " + str(bp.Probe.dead))
    if isinstance(m, Exception):
        pytest.fail(str(m))
    rep, f, raw = m
    assert rep["runs"] == rp.runs_of(world)
    return f


def _none(found, key):
    assert not found[key], "%d findings, the first: %s" % (len(found[key]), found[key][:5])


def test_decided_rays_name_the_references_shape(found):
    """Every loop, on every decided ray of every scene: no quantile."""
    _none(found, "decided_shapes")


def test_t_and_the_rebuilt_point_meet_the_rule(found):
    """t, origin + u eu + v ev through the uploaded DShade bytes against the candidate's point, the rebuilt point on the ray at the
    returned t, a sphere's point on the sphere: per scene, class and op."""
    _none(found, "bounds")


def test_undecided_rays_return_an_allowed_candidate(found):
    _none(found, "candidates")


def test_misses_and_windows(found):
    """A miss on every decided miss: tmax short of the first surface, rays that point away from the scene, rays from outside
    against nothing; behind tmin the second surface (test_decided_rays_name_the_references_shape)."""
    _none(found, "misses")


def test_any_hit_rays(found):
    """The loops that traverse: hit or miss as the reference says, and what they return is a plausible candidate on the ray."""
    _none(found, "any_hit")


def test_held_equals_streamed(found):
    """trace_held's bits are trace<0>'s on every ray, the undecided ones included."""
    _none(found, "held")


def test_the_vote_does_not_change_a_lanes_traversal(found):
    """trace_vote 1, 10 and 1024: the same bits from every op that traverses."""
    _none(found, "vote")


def test_a_permuted_ray_list_gives_the_same_bits(found):
    """Across lanes and blocks, the classes interleaved, on the deep tree too: the spare rows, spill, refill and overflow columns."""
    _none(found, "perm")


def test_nothing_is_non_finite(found):
    """No hit with a non-finite t, u or v, and none that names a record outside the table."""
    _none(found, "non_finite")


def test_the_two_builds_are_recorded_side_by_side(world, measured):
    """Their difference is recorded, not asserted; DRMLT_RAY_PROBE_JSON=<file> keeps the whole report."""
    if any(isinstance(m, Exception) for m in measured.values()) or len(measured) < 2:
        pytest.skip("not run: " + str(bp.Probe.dead))
    a, b = (measured[u][2] for u in rp.UNITS)
    diff = rp.builds_differ(a, b)
    print("words that differ between the builds:", {k: v for k, v in diff.items() if v["elements"]})
    assert sum(measured[u][0]["runs"] for u in rp.UNITS) == 2 * rp.runs_of(world)
    path = os.environ.get("DRMLT_RAY_PROBE_JSON")
    if path:
        rp.write_summary(path, rp.summary(world, {u: measured[u][0] for u in rp.UNITS}, diff, os.environ.get("DRMLT_PARENT_COMMIT", "")))
