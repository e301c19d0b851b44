"""Throughput of the chain kernel on bench.py's config 2 with a TABULATED reconstruction filter: the Cornell box 512 x 512,
technique=path type=orbital, maxDepth 8, rrDepth 5, 65 536 chains, sampleCount 256 -- and a Gaussian filter of radius 2 in
place of the box, so that a splat makes up to 4 x 4 atomic adds per channel through the filter table (k_mutate_w2: w2_flush,
kernels_v4.hip). bench.py has no such line. One warm-up call of one step, then --steps timed steps in one call, as bench.py runs
them; one JSON line: mutations/s by the wall clock of the call, and Context.kernel_time() per launch (HIP events around the
chain kernel's launches). A measurement, not a test:
    python tools/w2_flush_rate.py [--steps 5] [--filter gaussian|box] [--tag NAME]
DRMLT_LIBRARY / DRMLT_NO_W2 select another build or the twin kernel, as everywhere."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES, CHAINS, SPP = 512, 65536, 256
CFG = dict(technique="path", type="orbital", max_depth=8, rr_depth=5, direct_samples=-1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--filter", default="gaussian", choices=("gaussian", "box"))
    ap.add_argument("--tag", default="", help="copied into the line (which build this was)")
    a = ap.parse_args()
    import __graft_entry__ as entry
    pkg = entry.load_package()
    filt = pkg.abi.FILTER_GAUSSIAN if a.filter == "gaussian" else pkg.abi.FILTER_BOX
    sd = pkg.scenes.cornell_c2(RES, filt=filt)
    step = RES * RES * SPP
    cfg = pkg.abi.make_config(work_units=CHAINS, luminance_samples=100000, sample_count=SPP, **CFG)
    with pkg.Context(cfg, sd) as ctx:
        b = ctx.seed(0x5EED)
        ctx.run(step)                       # warm-up: code object load, first touch of the workspace
        ctx.film_clear()
        ctx.kernel_time(reset=True)
        m0 = ctx.stats().mutations
        t0 = time.perf_counter()
        ctx.run(a.steps * step)             # (returns when the device is done: the statistics come back with it)
        muts = ctx.stats().mutations - m0
        elapsed = time.perf_counter() - t0
        ms, launches = ctx.kernel_time()
        img = ctx.develop()
    assert muts == a.steps * step, (muts, a.steps * step)
    print(json.dumps({"tag": a.tag, "config": "cornell_c2 %d x %d, %s filter, %s, %d chains, sampleCount %d" % (RES, RES, a.filter, CFG, CHAINS, SPP),
                      "steps": a.steps, "mutations": int(muts), "value": muts / elapsed, "unit": "mutations/s", "elapsed_s": elapsed,
                      "kernel_ms_per_launch": ms, "launches": int(launches),
                      "kernel_mutations_per_s": muts / (ms * launches * 1e-3) if ms > 0 else None,
                      "b": b, "image_mean": float(img.mean())}))


if __name__ == "__main__":
    main()
