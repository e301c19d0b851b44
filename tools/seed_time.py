"""Diagnostic: time of seeding (bootstrap + seed selection + replay) for a bench configuration and chain count.

    python tools/seed_time.py CONFIG CHAINS            the host pass (drmlt_seed_pool), wall time
    python tools/seed_time.py CONFIG CHAINS --device   the device pass (drmlt_seed_pool_device)
    python tools/seed_time.py CONFIG CHAINS --both [--reps N]
        both on ONE context, interleaved (device, host, device, host, ...), and one JSON line: seed_ms of every call and
        their medians, whether the two passes picked the same seed_indices (and how many differ), b of each, the device pass's workspace (the
        library's own DRMLT_VERBOSE line) and how far each pass raised the process's peak resident set.
"""
import argparse, json, os, re, resource, statistics, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("config")
ap.add_argument("chains", type=int)
ap.add_argument("--device", action="store_true")
ap.add_argument("--both", action="store_true")
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()
both, device, reps = a.both, a.device, a.reps
if both:
    os.environ["DRMLT_VERBOSE"] = "1"   # read once, when the context is created
import __graft_entry__ as g
import bench
pkg = g.load_package()
name, chains = a.config, a.chains
conf = bench.CONFIGS[name]
sd = bench.build_scene(pkg, conf, conf["res"])
cfg = pkg.abi.make_config(work_units=chains, luminance_samples=100000, direct_samples=-1, sample_count=conf["spp"], **conf["cfg"])
ctx = pkg.Context(cfg, sd)
if not both:
    t = time.perf_counter()
    b = (ctx.seed_pool_device if device else ctx.seed_pool)(0x5EED, 0, chains)
    print("config %s, %d chains: seed %.2f s on the %s (b = %.4g)" % (name, chains, time.perf_counter() - t, "device" if device else "host", b))
    sys.exit(0)


def stderr_of(call):
    """(result, what the library wrote to stderr meanwhile)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            r = call()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return r, f.read().decode(errors="replace")


peak = lambda: resource.getrusage(resource.RUSAGE_SELF).ru_maxrss   # KiB; it only ever grows: the device pass goes first
out = {"config": name, "chains": chains, "reps": reps, "host": {"seed_ms": [], "wall_ms": []}, "device": {"seed_ms": [], "wall_ms": []}}
rss0 = peak()
for rep in range(reps):
    for which, call in (("device", ctx.seed_pool_device), ("host", ctx.seed_pool)):
        before, t = ctx.stats().seed_ms, time.perf_counter()
        b, log = stderr_of(lambda: call(0x5EED, 0, chains))
        o = out[which]
        o["wall_ms"].append(round(1e3 * (time.perf_counter() - t), 3))
        o["seed_ms"].append(round(ctx.stats().seed_ms - before, 3))
        o["b"] = b
        idx = ctx.seed_indices()
        if rep == 0:
            o["indices"] = idx
            o["peak_rss_raised_kib"] = peak() - (rss0 if which == "device" else rss_dev)
            rss_dev = peak()
        else:
            assert (idx == o["indices"]).all()
        m = re.search(r"(\d+) bytes of workspace beside (\d+) bytes of luminances \((\d+) samples", log)
        if m:
            o["workspace_bytes"], o["luminance_bytes"], out["samples"] = int(m.group(1)), int(m.group(2)), int(m.group(3))
        m = re.search(r"depth ordering of \d+ chains on the host, ([0-9.]+) ms", log)
        if m:
            o["host_depth_ordering_ms"] = float(m.group(1))
ih, idv = out["host"].pop("indices"), out["device"].pop("indices")
out["seed_indices_equal"] = bool((ih == idv).all())
# (the two passes sum the table in different orders: a pick whose uniform lies within samples x 2^-51 of a table entry may go to the neighbouring sample)
out["seed_indices_differing"], out["margin"] = int((ih != idv).sum()), out.get("samples", 0) * 2.0 ** -51
for which in ("host", "device"):
    out[which]["median_seed_ms"] = statistics.median(out[which]["seed_ms"])
out["host_over_device"] = round(out["host"]["median_seed_ms"] / out["device"]["median_seed_ms"], 3)
print(json.dumps(out))
