"""Seed selection on the device, the parts that need no device: the new symbols, the selection rule of csrc/seed_select.h run
serially on the host (drmlt_select_seeds_blocked) against the oracle's selectSeeds, and the header under the host compiler's
address and undefined-behaviour sanitizers (a stand-alone program, tests/native/seed_select_probe.cpp).

The blocked rule sums the table in another order than the serial fp64 CDF of drmlt_seed / the oracle, so the two may differ
where a pick's uniform lies within rounding of a boundary of the table. Any two summation orders of n non-negative fp64 terms
differ by at most 2 (n - 1) 2^-53 relative, the normalisation and the product add a few ulp: the margin is n 2^-51. Every
comparison with the serial rule ASSERTS first that no uniform of the case lies that close to a boundary (margin_of)."""
import ctypes as C
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "drmlt_abi.h")
CSRC = os.path.join(ROOT, "drmlt-mitsuba_amd", "csrc")
HOST = os.path.join(ROOT, "drmlt-mitsuba_amd", "host")
NEW = ("drmlt_seed_device", "drmlt_seed_pool_device", "drmlt_node_seed_device", "drmlt_select_seeds_device", "drmlt_select_seeds_blocked")
SEEDS = ((0x5EED, 0), (0x5EED, 3), (12345678901234, 0))
TAG_SEEDSEL = 1


def cases():
    """name -> (luminances, weights or None, n_select): the four arrays of the issue, drawn in its order, and the weighted case."""
    rng = np.random.default_rng(7)
    a = np.exp(4 * rng.standard_normal(20011)).astype(np.float32)
    a[::7] = 0
    a[[5, 1000, 20010]] = np.nan
    b = np.zeros(100, dtype=np.float32)
    b[37] = 2.5
    c = np.full(1000, 1e-12, dtype=np.float32)
    c[500] = 1e8
    d = np.exp(4 * rng.standard_normal(65537)).astype(np.float32)
    d[:300] = 0
    d[-300:] = 0
    w = rng.random(a.size).astype(np.float32)
    w[::5] = 0
    w[11] = np.inf      # (a[11], a[12] are admissible luminances: neither a multiple of 7 nor one of the NaNs)
    w[12] = np.nan
    return {"a": (a, None, 4096), "b": (b, None, 64), "c": (c, None, 256), "d": (d, None, 1000), "weighted": (a, w, 4096)}


def philox_xi(seed, stream, n_select):
    """xi_j of chain slot j: word 0 of philox(key, (0, j, stream, TAG_SEEDSEL)), 24 bits, as float32."""
    k0, k1 = np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)
    c = [np.zeros(n_select, dtype=np.uint64), np.arange(n_select, dtype=np.uint64), np.full(n_select, stream, dtype=np.uint64), np.full(n_select, TAG_SEEDSEL, dtype=np.uint64)]
    m32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m32, (k1 + np.uint64(0xBB67AE85)) & m32
    return ((c[0] >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def serial_table(lum, weights=None):
    """seed_impl's inclusion and its normalised serial fp64 CDF (leading zero included), with the sample index of every entry."""
    lum = np.asarray(lum, dtype=np.float32)
    lw = lum if weights is None else np.asarray(weights, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(lum) & (lum != 0) & (lw > 0) & np.isfinite(lw)
    idx = np.flatnonzero(ok)
    cdf = np.concatenate([[0.0], np.cumsum(lw[idx].astype(np.float64))])   # (cumsum is sequential)
    cdf[1:] *= 1.0 / cdf[-1]
    cdf[-1] = 1.0
    return idx, cdf


def serial_picks(lum, weights, seed, stream, n_select):
    """DiscreteDistribution::sample with the host's zero-width skip on serial_table, sorted."""
    idx, cdf = serial_table(lum, weights)
    out = []
    for xi in philox_xi(seed, stream, n_select).astype(np.float64):
        i = min(max(int(np.searchsorted(cdf, xi, side="left")) - 1, 0), cdf.size - 2)
        while cdf[i + 1] - cdf[i] == 0 and i < cdf.size - 1:
            i += 1
        out.append(idx[i])
    return np.sort(np.array(out, dtype=np.uint32))


def margin_of(lum, weights, seed, stream, n_select):
    """(smallest distance of a uniform to an entry of the serial table, the margin n 2^-51 it has to exceed)."""
    _, cdf = serial_table(lum, weights)
    xi = philox_xi(seed, stream, n_select).astype(np.float64)
    at = np.searchsorted(cdf, xi)
    gap = np.minimum(np.abs(cdf[np.clip(at, 0, cdf.size - 1)] - xi), np.abs(cdf[np.clip(at - 1, 0, cdf.size - 1)] - xi))
    return gap.min(), np.asarray(lum).size * 2.0 ** -51


def test_header_library_and_binding_agree_on_the_new_symbols(pkg, native_lib):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"int\s+%s\s*\(" % name, src), "include/drmlt_abi.h does not declare " + name
        assert name in pkg.binding.ABI_SYMBOLS and hasattr(native_lib, name), name
    assert "pathsampler.cpp:936-957" in open(HEADER).read()
    assert native_lib.drmlt_abi_version() == 4
    assert native_lib.drmlt_seed_device.argtypes == native_lib.drmlt_seed.argtypes
    assert native_lib.drmlt_seed_pool_device.argtypes == native_lib.drmlt_seed_pool.argtypes
    assert native_lib.drmlt_node_seed_device.argtypes == native_lib.drmlt_node_seed.argtypes
    for cls, names in ((pkg.Context, ("seed_device", "seed_pool_device", "select_seeds_device")), (pkg.Node, ("seed_device",))):
        for n in names:
            assert callable(getattr(cls, n, None)), (cls, n)
    assert list(inspect.signature(pkg.Context.seed_device).parameters) == list(inspect.signature(pkg.Context.seed).parameters)
    assert list(inspect.signature(pkg.Context.seed_pool_device).parameters) == list(inspect.signature(pkg.Context.seed_pool).parameters)
    assert callable(pkg.binding.select_seeds_blocked)


def test_null_arguments_are_refused(pkg, native_lib):
    b = C.c_double()
    lum, out = np.ones(4, dtype=np.float32), np.zeros(2, dtype=np.uint32)
    assert native_lib.drmlt_seed_device(None, 1, 0, C.byref(b)) == pkg.abi.E_INVALID
    assert native_lib.drmlt_seed_pool_device(None, 1, 0, 8, C.byref(b)) == pkg.abi.E_INVALID
    assert native_lib.drmlt_node_seed_device(None, 1, C.byref(b)) == pkg.abi.E_INVALID
    assert native_lib.drmlt_select_seeds_device(None, lum.ctypes.data, None, 4, 1, 0, 2, out.ctypes.data, None, None) == pkg.abi.E_INVALID
    assert native_lib.drmlt_select_seeds_blocked(None, None, 4, 1, 0, 2, out.ctypes.data, None, None) == pkg.abi.E_INVALID
    assert native_lib.drmlt_select_seeds_blocked(lum.ctypes.data, None, 4, 1, 0, 2, None, None, None) == pkg.abi.E_INVALID
    assert native_lib.drmlt_select_seeds_blocked(lum.ctypes.data, None, 0, 1, 0, 2, out.ctypes.data, None, None) == pkg.abi.E_INVALID
    assert np.all(out == 0)
    assert native_lib.drmlt_select_seeds_blocked(lum.ctypes.data, None, 4, 1, 0, 2, out.ctypes.data, None, None) == 0   # mean and total are optional


def test_the_cli_knows_seed_pass(native_lib):
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    cli = os.path.join(HOST, "drmlt_render")

    def run(*args):
        p = subprocess.run([cli, *args], capture_output=True, text=True)
        return p.returncode, p.stdout, p.stderr

    base = ["-D", "technique=path", "-D", "type=orbital"]
    for extra in (["--check"], []):   # refused by the parameter surface itself: no scene is read, no device is looked for
        rc, _, err = run(*extra, *base, "-D", "seedPass=bogus")
        assert rc == 1 and "Unknown seedPass (host | device)" in err, err
    for given, want in (([], "host"), (["-D", "seedPass=host"], "host"), (["-D", "seedPass=device"], "device")):
        rc, out, _ = run("--check", *base, *given)
        assert rc == 0 and dict(t.split("=") for t in out.split())["seedPass"] == want


@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_blocked_selection_equals_the_oracle(pkg, native_lib, ob, name):
    lum, _, n_select = cases()[name]
    for seed, stream in SEEDS:
        gap, margin = margin_of(lum, None, seed, stream, n_select)
        print("%s seed %#x stream %d: min |cdf - xi| = %.3g, margin %.3g" % (name, seed, stream, gap, margin))
        assert gap > margin, "a uniform of this case lies within rounding of a table entry: the comparison would prove nothing"
        picks, mean, total = pkg.binding.select_seeds_blocked(lum, seed, stream, n_select)
        want = ob.select_seeds(lum, seed, stream, n_select)
        assert picks.dtype == np.uint32 and np.array_equal(picks, want)
        assert np.array_equal(picks, serial_picks(lum, None, seed, stream, n_select))   # (the numpy restatement used for the weighted case)
        ref = np.nansum(lum.astype(np.float64)) / np.count_nonzero(~np.isnan(lum))
        assert abs(mean - ref) <= lum.size * 2.0 ** -51 * ref
        with np.errstate(invalid="ignore"):
            ref_total = lum[~np.isnan(lum) & (lum > 0)].astype(np.float64).sum()
        assert abs(total - ref_total) <= lum.size * 2.0 ** -51 * ref_total


def test_philox_of_this_file_is_the_oracles(ob):
    for seed, stream in SEEDS:
        xi = philox_xi(seed, stream, 9)
        for j in (0, 8):
            assert xi[j] == ob.uniforms(seed, stream, TAG_SEEDSEL, j, 0, 1)[0]


def test_weighted_selection_equals_the_serial_rule(pkg, native_lib):
    lum, w, n_select = cases()["weighted"]
    assert np.isinf(w[11]) and np.isnan(w[12]) and lum[11] > 0 and lum[12] > 0 and np.count_nonzero(w == 0) > 1000
    for seed, stream in SEEDS:
        gap, margin = margin_of(lum, w, seed, stream, n_select)
        print("weighted seed %#x stream %d: min |cdf - xi| = %.3g, margin %.3g" % (seed, stream, gap, margin))
        assert gap > margin
        picks, mean, total = pkg.binding.select_seeds_blocked(lum, seed, stream, n_select, weights=w)
        assert np.array_equal(picks, serial_picks(lum, w, seed, stream, n_select))
        assert not np.isin(picks, [11, 12]).any() and np.all(w[picks] > 0) and np.all(lum[picks] > 0)
        ref = np.nansum(lum.astype(np.float64)) / np.count_nonzero(~np.isnan(lum))    # b is the mean of f, not of f under the map
        assert abs(mean - ref) <= lum.size * 2.0 ** -51 * ref


def test_zero_luminance_is_an_error(pkg, native_lib):
    z, nan = np.zeros(300, dtype=np.float32), np.full(300, np.nan, dtype=np.float32)
    one = z.copy()
    one[17] = 3.0
    for lum, w in ((z, None), (nan, None), (one, z), (one, nan)):   # the last two: a positive mean, no admissible weight
        with pytest.raises(pkg.DrmltError) as e:
            pkg.binding.select_seeds_blocked(lum, 0x5EED, 0, 8, weights=w)
        assert e.value.code == pkg.abi.E_ZERO_LUM


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seed_probe") / "seed_select_probe")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I", CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "native", "seed_select_probe.cpp")], check=True)
    return exe


def test_the_header_under_the_sanitizers(pkg, native_lib, probe, tmp_path):
    p = subprocess.run([probe, "sizes"], capture_output=True, text=True)   # n = 1, 255, 256, 257
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr
    for name, (lum, w, n_select) in cases().items():
        lum.tofile(tmp_path / "lum.f32")
        if w is not None:
            w.tofile(tmp_path / "w.f32")
        for seed, stream in SEEDS:
            p = subprocess.run([probe, "file", str(tmp_path / "lum.f32"), str(tmp_path / "w.f32") if w is not None else "-", str(seed), str(stream), str(n_select)],
                               capture_output=True, text=True)
            assert p.returncode == 0, p.stderr
            r = json.loads(p.stdout)
            picks, mean, total = pkg.binding.select_seeds_blocked(lum, seed, stream, n_select, weights=w)
            # another compiler, the same header: the same bits
            assert r["rc"] == 0 and np.array_equal(np.array(r["picks"], dtype=np.uint32), picks)
            assert float.fromhex(r["mean"]) == mean and float.fromhex(r["total"]) == total
