"""The multiplexed estimate by path length and strategy (drmlt_render_mmlt_layers): a table, b_d per depth, the stack and a
montage; and the kernels' rates beside k_bootstrap_mmlt's.

For a named scene one table row per layer (d, s) -- depth d, the samples that drew s emitter-side and t = d + 1 - s sensor-side
vertices -- with the layer's mean luminance and its share of the image; per depth b_d, the mean luminance of the depth's layers
(the share of the chain seeds that have that depth, pathsampler.cpp:889), and its share of b; the stack as .npy (layers, H, W, 3)
and a montage .png: one row per depth, one column per s, every layer of a depth under that depth's exposure (its layers' sum at
mean luminance 0.18, gamma 2.2). --unweighted: every strategy used alone, without its MIS weight (the shares are then of the sum
of the layers, which is no image). spp is per pixel AND depth.

    python tools/mmlt_layers.py --scene caustic_c5 --res 64 --spp 64 [--unweighted] [--out layers]

The rates, on bench configuration 5's scene and depth (glass caustic 512 x 512, maxDepth 6): the kernels' own durations from a
profiler's kernel trace (start to end of the kernel alone: no allocation, memset or copy of the call around it), k_render_mmlt and
k_layers_mmlt beside k_bootstrap_mmlt on the same samples:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o rate -- python tools/mmlt_layers.py --rate-run [--spp 3]
    python tools/mmlt_layers.py --rate-stats <dir>/.../rate_kernel_stats.csv [--spp 3]      one JSON line
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

from bdpt_layers import LUMW, montage  # noqa: E402  (the same (d, s) grid)

RATE = dict(scene="caustic_c5", res=512, cfg=dict(technique="mmlt", type="orbital", max_depth=6, fix_emitter_path=1, direct_samples=-1))


def table(a):
    pkg = entry.load_package()
    abi = pkg.abi
    sd = pkg.scenes.SCENES[a.scene](a.res)
    cfg = abi.make_config(technique="mmlt", type="orbital", work_units=64, max_depth=a.max_depth, rr_depth=a.rr_depth,
                          direct_samples=a.direct_samples, no_light_image=a.no_light_image)
    with pkg.Context(cfg, sd) as ctx:
        stack = ctx.render_mmlt_layers(a.spp, seed=a.seed, weighted=not a.unweighted).astype(np.float64)
    means = (stack @ LUMW).mean(axis=(1, 2))
    total = means.sum()
    print("%s %d x %d, maxDepth %d, %d spp per depth, %s layers; mean luminance of their sum %.6g"
          % (a.scene, a.res, a.res, a.max_depth, a.spp, "unweighted" if a.unweighted else "weighted", total))
    print("%3s %3s %3s  %14s  %8s" % ("d", "s", "t", "mean luminance", "share"))
    for d in range(1, a.max_depth + 1):
        for s in range(d + 2):
            m = means[abi.bdpt_layer_index(d, s)]
            print("%3d %3d %3d  %14.6g  %8.5f" % (d, s, d + 1 - s, m, m / total if total > 0 else 0.0))
        lo, hi = abi.bdpt_layer_index(d, 0), abi.bdpt_layer_index(d, d + 1) + 1
        print("%3d %7s  %14.6g  %8.5f   b_%d and its share of b" % (d, "all", means[lo:hi].sum(), means[lo:hi].sum() / total if total > 0 else 0.0, d))
    np.save(a.out + ".npy", stack.astype(np.float32))
    pkg.heatmap.write_png(a.out + ".png", montage(abi, stack, a.max_depth))
    print("wrote %s.npy %s and %s.png" % (a.out, stack.shape, a.out))


def rate_run(spp, reps):
    pkg = entry.load_package()
    sd = pkg.scenes.SCENES[RATE["scene"]](RATE["res"])
    n = spp * RATE["res"] ** 2 * RATE["cfg"]["max_depth"]
    with pkg.Context(pkg.abi.make_config(work_units=64, **RATE["cfg"]), sd) as ctx:
        for k in range(reps + 1):   # (the first of each is the warm-up: code object load)
            img = ctx.render_mmlt(spp, seed=7 + k)
            stack = ctx.render_mmlt_layers(spp, seed=7 + k)
            boot = ctx.bootstrap_luminances(7 + k, 0, n)
    print("samples %d, image mean luminance %.6g, of the %d layers' sum %.6g, maxDepth x the bootstrap's mean %.6g"
          % (n, (img @ LUMW).mean(), len(stack), (stack.sum(axis=0, dtype="f8") @ LUMW).mean(),
             RATE["cfg"]["max_depth"] * boot[np.isfinite(boot)].mean(dtype="f8")))


def rate_stats(path, spp, reps):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            rows[r["Name"].split("(")[0]] = r
    n = spp * RATE["res"] ** 2 * RATE["cfg"]["max_depth"]
    out = {"config": "bench configuration 5's scene: %s %d x %d, %s" % (RATE["scene"], RATE["res"], RATE["res"], RATE["cfg"]), "samples_per_call": n,
           "calls": reps + 1, "timing": "kernel durations of a rocprofv3 --kernel-trace --stats run (the kernels alone); samples_per_second from the "
                                        "minimum over the calls, samples_per_second_range from the maximum and the minimum"}
    for k in ("k_bootstrap_mmlt", "k_render_mmlt", "k_layers_mmlt"):
        r = rows[k]
        assert int(r["Calls"]) == reps + 1, r
        out[k] = {"min_ms": int(r["MinNs"]) / 1e6, "avg_ms": float(r["AverageNs"]) / 1e6, "max_ms": int(r["MaxNs"]) / 1e6,
                  "samples_per_second": n / (int(r["MinNs"]) / 1e9),
                  "samples_per_second_range": [n / (int(r["MaxNs"]) / 1e9), n / (int(r["MinNs"]) / 1e9)]}
    for k in ("k_render_mmlt", "k_layers_mmlt"):
        out[k + "_over_bootstrap_time"] = out[k]["min_ms"] / out["k_bootstrap_mmlt"]["min_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="caustic_c5")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--spp", type=int, default=None, help="per pixel and depth: default 64 for the table, 3 for the rate")
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--rr-depth", type=int, default=5)
    ap.add_argument("--direct-samples", type=int, default=-1)
    ap.add_argument("--no-light-image", type=int, default=0)
    ap.add_argument("--unweighted", action="store_true")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=1)
    ap.add_argument("--out", default="mmlt_layers", help="writes <out>.npy and <out>.png")
    ap.add_argument("--rate-run", action="store_true")
    ap.add_argument("--rate-stats")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.rate_run:
        rate_run(a.spp or 3, a.reps)
    elif a.rate_stats:
        rate_stats(a.rate_stats, a.spp or 3, a.reps)
    else:
        a.spp = a.spp or 64
        table(a)


if __name__ == "__main__":
    main()
