"""The bidirectional estimate by path length and strategy (drmlt_render_bdpt_layers): a table, the stack and a montage.

For a named scene (or --config bdpt, the bench's `bdpt` configuration: Cornell box 512 x 512, maxDepth 8, rrDepth 5, 131 072
chains) one table row per layer (d, s) -- d edges, s emitter-side and t = d + 1 - s sensor-side vertices -- with the layer's mean
luminance and its share of the image, the stack as .npy (layers, H, W, 3) and a montage .png: one row per depth, one column per
s, every layer of a depth under that depth's exposure (its layers' sum at mean luminance 0.18, gamma 2.2), so that a row
shows which strategy carries which part of that depth's light. --unweighted: every strategy used alone, without its MIS weight
(the shares are then of the sum of the layers, which is no image).

    python tools/bdpt_layers.py --scene cornell_c2 --res 64 --spp 64 [--unweighted] [--out layers]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LUMW = np.array([0.212671, 0.715160, 0.072169])
BENCH = {"bdpt": dict(scene="cornell_c2", res=512, chains=131072, max_depth=8, rr_depth=5)}


def montage(abi, stack, max_depth, gap=2):
    """uint8 (rows, cols, 3): row d - 1 holds layers (d, 0) .. (d, d + 1) side by side, the unused cells dark grey."""
    _, h, w, _ = stack.shape
    out = np.full((max_depth * (h + gap) - gap, (max_depth + 2) * (w + gap) - gap, 3), 0.05)
    for d in range(1, max_depth + 1):
        row = stack[abi.bdpt_layer_index(d, 0):abi.bdpt_layer_index(d, d + 1) + 1]
        mean = (row.sum(axis=0) @ LUMW).mean()
        for s in range(d + 2):
            y, x = (d - 1) * (h + gap), s * (w + gap)
            out[y:y + h, x:x + w] = np.clip(row[s] * (0.18 / mean if mean > 0 else 0.0), 0.0, 1.0) ** (1 / 2.2)
    return (out * 255.0 + 0.5).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell_c2")
    ap.add_argument("--config", choices=sorted(BENCH), help="a bench configuration instead of --scene / --res / --chains / depths")
    ap.add_argument("--res", type=int, default=64)
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max-depth", type=int, default=6)
    ap.add_argument("--rr-depth", type=int, default=4)
    ap.add_argument("--no-direct-sampling", type=int, default=0)
    ap.add_argument("--no-light-image", type=int, default=0)
    ap.add_argument("--unweighted", action="store_true")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=1)
    ap.add_argument("--out", default="bdpt_layers", help="writes <out>.npy and <out>.png")
    a = ap.parse_args()
    if a.config:
        for k, v in BENCH[a.config].items():
            setattr(a, k, v)

    pkg = entry.load_package()
    abi = pkg.abi
    sd = pkg.scenes.SCENES[a.scene](a.res)
    cfg = abi.make_config(technique="bdpt", type="orbital", work_units=a.chains, max_depth=a.max_depth, rr_depth=a.rr_depth,
                          direct_samples=-1, no_direct_sampling=a.no_direct_sampling, no_light_image=a.no_light_image)
    with pkg.Context(cfg, sd) as ctx:
        stack = ctx.render_bdpt_layers(a.spp, seed=a.seed, weighted=not a.unweighted).astype(np.float64)
    means = (stack @ LUMW).mean(axis=(1, 2))
    total = means.sum()
    print("%s %d x %d, maxDepth %d, %d spp, %s layers; mean luminance of their sum %.6g"
          % (a.scene, a.res, a.res, a.max_depth, a.spp, "unweighted" if a.unweighted else "weighted", total))
    print("%3s %3s %3s  %14s  %8s" % ("d", "s", "t", "mean luminance", "share"))
    for d in range(1, a.max_depth + 1):
        for s in range(d + 2):
            m = means[abi.bdpt_layer_index(d, s)]
            print("%3d %3d %3d  %14.6g  %8.5f" % (d, s, d + 1 - s, m, m / total if total > 0 else 0.0))
        lo, hi = abi.bdpt_layer_index(d, 0), abi.bdpt_layer_index(d, d + 1) + 1
        print("%3d %7s  %14.6g  %8.5f" % (d, "all", means[lo:hi].sum(), means[lo:hi].sum() / total if total > 0 else 0.0))
    np.save(a.out + ".npy", stack.astype(np.float32))
    pkg.heatmap.write_png(a.out + ".png", montage(abi, stack, a.max_depth))
    print("wrote %s.npy %s and %s.png" % (a.out, stack.shape, a.out))


if __name__ == "__main__":
    main()
