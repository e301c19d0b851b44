"""Throughput of k_render_bdpt beside k_bootstrap_bdpt: the same N samples of the bench's `bdpt` configuration (Cornell box
512 x 512, technique=bdpt type=orbital, maxDepth 8, rrDepth 5, 131 072 chains), once into a film and once into a luminance array.

Two modes:
    python tools/render_bdpt_rate.py --run [--spp 16] [--layers] the workload: one warm-up and --reps timed calls of each kernel
                                                                 (--layers: of k_layers_bdpt too, drmlt_render_bdpt_layers)
    python tools/render_bdpt_rate.py --stats <kernel_stats.csv>  read the kernels' own durations out of a rocprofv3
                                                                 --kernel-trace --stats run of the workload; one JSON line

The kernels' durations come from the profiler's kernel trace (start to end of the kernel alone: no allocation, memset or copy
of the call around it):
    rocprofv3 --kernel-trace --stats -d <dir> -o rate -- python tools/render_bdpt_rate.py --run
"""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES, CHAINS = 512, 131072
CFG = dict(technique="bdpt", type="orbital", max_depth=8, rr_depth=5, direct_samples=-1)


def run(spp, reps, layers=False):
    import __graft_entry__ as entry
    pkg = entry.load_package()
    sd = pkg.scenes.cornell_c2(RES)
    n = spp * RES * RES
    with pkg.Context(pkg.abi.make_config(work_units=CHAINS, luminance_samples=20000, **CFG), sd) as ctx:
        for k in range(reps + 1):   # (the first of each is the warm-up: code object load, first touch of the workspace)
            img = ctx.render_bdpt(spp, seed=7 + k)
            lums = ctx.bootstrap_luminances(7 + k, 0, n)
            if layers:
                stack = ctx.render_bdpt_layers(spp, seed=7 + k)
        print("samples %d, image mean luminance %.6g, bootstrap mean %.6g" % (n, (img @ [0.212671, 0.715160, 0.072169]).mean(), lums.mean()))
        if layers:
            print("%d layers, mean luminance of their sum %.6g" % (len(stack), (stack.sum(axis=0, dtype="f8") @ [0.212671, 0.715160, 0.072169]).mean()))


def stats(path, spp, reps):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            rows[r["Name"].split("(")[0]] = r
    n = spp * RES * RES
    out = {"config": "bdpt: cornell_c2 %d x %d, %s, %d chains" % (RES, RES, CFG, CHAINS), "samples_per_call": n, "calls": reps + 1,
           "timing": "kernel durations of a rocprofv3 --kernel-trace --stats run (the kernels alone); the minimum over the calls"}
    for k in ("k_render_bdpt", "k_bootstrap_bdpt") + (("k_layers_bdpt",) if "k_layers_bdpt" in rows else ()):
        r = rows[k]
        assert int(r["Calls"]) == reps + 1, r
        out[k] = {"min_ms": int(r["MinNs"]) / 1e6, "avg_ms": float(r["AverageNs"]) / 1e6, "max_ms": int(r["MaxNs"]) / 1e6,
                  "samples_per_second": n / (int(r["MinNs"]) / 1e9)}
    out["render_over_bootstrap_time"] = out["k_render_bdpt"]["min_ms"] / out["k_bootstrap_bdpt"]["min_ms"]
    if "k_layers_bdpt" in out:
        out["layers_over_render_time"] = out["k_layers_bdpt"]["min_ms"] / out["k_render_bdpt"]["min_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--stats")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.run:
        run(a.spp, a.reps, a.layers)
    elif a.stats:
        stats(a.stats, a.spp, a.reps)
    else:
        ap.error("--run or --stats")
