"""The path-traced estimate by path length and strategy (drmlt_render_pt_layers): a table, the stack and a montage; and the
kernel's rate beside k_render_pt's.

For a named scene one table row per layer (d, strategy) -- d edges from the camera to the emitter, found by the BSDF-sampled ray
(hit) or by the light sample (direct) -- with the layer's mean luminance weighted and unweighted and its share of the image, the
weighted stack as .npy (layers, H, W, 3) and a montage .png: one row per depth, columns hit and direct, weighted then unweighted,
every cell of a depth under that depth's exposure (its weighted layers' sum at mean luminance 0.18, gamma 2.2).

    python tools/pt_layers.py --scene cornell_c2 --res 64 --spp 64 [--out layers]

The rate, on bench configuration 2's scene and depths (Cornell box 512 x 512, maxDepth 8, rrDepth 5): the kernels' own durations
from a profiler's kernel trace (start to end of the kernel alone: no allocation, memset or copy of the call around it):

    rocprofv3 --kernel-trace --stats -d <dir> -o rate -- python tools/pt_layers.py --rate-run [--spp 16]
    python tools/pt_layers.py --rate-stats <dir>/.../rate_kernel_stats.csv [--spp 16]      one JSON line
"""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LUMW = np.array([0.212671, 0.715160, 0.072169])
RATE = dict(res=512, cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5, direct_samples=-1))


def montage(abi, weighted, unweighted, max_depth, gap=2):
    """uint8 (rows, cols, 3): row d - 1 holds (d, hit), (d, direct) weighted, then the same two unweighted."""
    _, h, w, _ = weighted.shape
    out = np.full((max_depth * (h + gap) - gap, 4 * (w + gap) - gap, 3), 0.05)
    for d in range(1, max_depth + 1):
        lo = abi.pt_layer_index(d, abi.PT_HIT)
        mean = (weighted[lo:lo + 2].sum(axis=0) @ LUMW).mean()
        for col, layer in enumerate(list(weighted[lo:lo + 2]) + list(unweighted[lo:lo + 2])):
            y, x = (d - 1) * (h + gap), col * (w + gap)
            out[y:y + h, x:x + w] = np.clip(layer * (0.18 / mean if mean > 0 else 0.0), 0.0, 1.0) ** (1 / 2.2)
    return (out * 255.0 + 0.5).astype(np.uint8)


def table(a):
    pkg = entry.load_package()
    abi = pkg.abi
    sd = pkg.scenes.SCENES[a.scene](a.res)
    cfg = abi.make_config(technique="path", type="orbital", work_units=64, max_depth=a.max_depth, rr_depth=a.rr_depth, direct_samples=a.direct_samples)
    with pkg.Context(cfg, sd) as ctx:
        wt = ctx.render_pt_layers(a.spp, seed=a.seed).astype(np.float64)
        un = ctx.render_pt_layers(a.spp, seed=a.seed, weighted=False).astype(np.float64)
    mw, mu = (wt @ LUMW).mean(axis=(1, 2)), (un @ LUMW).mean(axis=(1, 2))
    total = mw.sum()
    print("%s %d x %d, maxDepth %d, %d spp; mean luminance of the weighted layers' sum (render_pt's image) %.6g" % (a.scene, a.res, a.res, a.max_depth, a.spp, total))
    print("%3s %8s  %14s  %8s  %14s" % ("d", "strategy", "weighted", "share", "unweighted"))
    for d in range(1, a.max_depth + 1):
        for s, name in ((abi.PT_HIT, "hit"), (abi.PT_DIRECT, "direct")):
            i = abi.pt_layer_index(d, s)
            print("%3d %8s  %14.6g  %8.5f  %14.6g" % (d, name, mw[i], mw[i] / total if total > 0 else 0.0, mu[i]))
        lo = abi.pt_layer_index(d, 0)
        print("%3d %8s  %14.6g  %8.5f" % (d, "both", mw[lo:lo + 2].sum(), mw[lo:lo + 2].sum() / total if total > 0 else 0.0))
    np.save(a.out + ".npy", wt.astype(np.float32))
    pkg.heatmap.write_png(a.out + ".png", montage(abi, wt, un, a.max_depth))
    print("wrote %s.npy %s and %s.png" % (a.out, wt.shape, a.out))


def rate_run(spp, reps):
    pkg = entry.load_package()
    sd = pkg.scenes.cornell_c2(RATE["res"])
    with pkg.Context(pkg.abi.make_config(work_units=64, **RATE["cfg"]), sd) as ctx:
        for k in range(reps + 1):   # (the first of each is the warm-up: code object load)
            img = ctx.render_pt(spp, seed=7 + k)
            stack = ctx.render_pt_layers(spp, seed=7 + k)
    print("samples %d, image mean luminance %.6g, of the %d layers' sum %.6g"
          % (spp * RATE["res"] ** 2, (img @ LUMW).mean(), len(stack), (stack.sum(axis=0, dtype="f8") @ LUMW).mean()))


def rate_stats(path, spp, reps):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            rows[r["Name"].split("(")[0]] = r
    n = spp * RATE["res"] ** 2
    out = {"config": "bench configuration 2's scene: cornell_c2 %d x %d, %s" % (RATE["res"], RATE["res"], RATE["cfg"]), "samples_per_call": n,
           "calls": reps + 1, "timing": "kernel durations of a rocprofv3 --kernel-trace --stats run (the kernels alone); the minimum over the calls"}
    for k in ("k_render_pt", "k_render_pt_layers"):
        r = rows[k]
        assert int(r["Calls"]) == reps + 1, r
        out[k] = {"min_ms": int(r["MinNs"]) / 1e6, "avg_ms": float(r["AverageNs"]) / 1e6, "max_ms": int(r["MaxNs"]) / 1e6,
                  "samples_per_second": n / (int(r["MinNs"]) / 1e9)}
    out["layers_over_render_time"] = out["k_render_pt_layers"]["min_ms"] / out["k_render_pt"]["min_ms"]
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell_c2")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--spp", type=int, default=None, help="default 64 for the table, 16 for the rate")
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--rr-depth", type=int, default=4)
    ap.add_argument("--direct-samples", type=int, default=-1)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=1)
    ap.add_argument("--out", default="pt_layers", help="writes <out>.npy and <out>.png")
    ap.add_argument("--rate-run", action="store_true")
    ap.add_argument("--rate-stats")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.rate_run:
        rate_run(a.spp or 16, a.reps)
    elif a.rate_stats:
        rate_stats(a.rate_stats, a.spp or 16, a.reps)
    else:
        a.spp = a.spp or 64
        table(a)


if __name__ == "__main__":
    main()
