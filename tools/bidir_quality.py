"""Image quality of a bidirectional chain render against the device's own bidirectional reference (drmlt_render_bdpt), or, for
technique=mmlt with --reference mmlt, against that technique's own reference (drmlt_render_mmlt), with no pixel left out.

For a named scene, a technique (bdpt, mmlt) and a chain loop (drmlt, pssmlt): the relative MSE of the developed image at a given
mutation count per pixel against 2 x S spp of render_bdpt at the same depths. The reference is rendered as two halves with
different seeds; their difference prices the reference's own error (rel. MSE of the mean of two halves = that of their
difference / 4), as bench.py --full prices its path-traced reference. One JSON line.

    python tools/bidir_quality.py --scene cornell_c2 --technique bdpt --res 128 --chains 131072 --mpp 256 --ref-spp 4096
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

LUMW = np.array([0.212671, 0.715160, 0.072169])


def lum(img):
    return np.asarray(img, dtype=np.float64) @ LUMW


def reference(pkg, sd, depths, spp, no_direct_sampling=0, chains=131072):
    """(the two render_bdpt halves of `spp` each, seconds). A half above 2^32 / (W * H) samples a pixel is averaged from several
    calls, as drmlt_render_bdpt asks."""
    cfg = pkg.abi.make_config(technique="bdpt", type="orbital", work_units=chains, no_direct_sampling=no_direct_sampling, **depths)
    per_call = max(1, min(spp, ((1 << 32) - 1) // (sd.camera.width * sd.camera.height)))
    t0 = time.perf_counter()
    halves = []
    with pkg.Context(cfg, sd) as ctx:
        for h, seed0 in enumerate((4242, 977)):
            acc, done, k = np.zeros((sd.camera.height, sd.camera.width, 3)), 0, 0
            while done < spp:
                n = min(per_call, spp - done)
                acc += n * ctx.render_bdpt(n, seed=seed0 + 1000 * k).astype(np.float64)
                done, k = done + n, k + 1
            halves.append(acc / spp)
    return halves[0], halves[1], time.perf_counter() - t0


def reference_mmlt(pkg, sd, kw, spp):
    """The same two halves from render_mmlt on a technique=mmlt context with the chain render's own options `kw`; `spp` is per
    pixel and depth. A half of 2^32 samples or more is averaged from several calls, as drmlt_render_mmlt asks."""
    per_call = max(1, min(spp, ((1 << 32) - 1) // (sd.camera.width * sd.camera.height * kw["max_depth"])))
    t0 = time.perf_counter()
    halves = []
    with pkg.Context(pkg.abi.make_config(**kw), sd) as ctx:
        for seed0 in (4242, 977):
            acc, done, k = np.zeros((sd.camera.height, sd.camera.width, 3)), 0, 0
            while done < spp:
                n = min(per_call, spp - done)
                acc += n * ctx.render_mmlt(n, seed=seed0 + 1000 * k).astype(np.float64)
                done, k = done + n, k + 1
            halves.append(acc / spp)
    return halves[0], halves[1], time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="cornell_c2")
    ap.add_argument("--technique", default="bdpt", choices=["bdpt", "mmlt"])
    ap.add_argument("--algo", default="drmlt", choices=["drmlt", "pssmlt"])
    ap.add_argument("--type", default="orbital")
    ap.add_argument("--res", type=int, default=128)
    ap.add_argument("--chains", type=int, default=131072)
    ap.add_argument("--mpp", type=int, default=256, help="mutations per pixel of the chain render")
    ap.add_argument("--ref-spp", type=int, default=4096, help="S: the reference is 2 x S spp of render_bdpt")
    ap.add_argument("--max-depth", type=int, default=8)
    ap.add_argument("--rr-depth", type=int, default=5)
    ap.add_argument("--fix-emitter-path", type=int, default=0)
    ap.add_argument("--no-direct-sampling", type=int, default=0)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x5EED)
    ap.add_argument("--reference", default="bdpt", choices=["bdpt", "mmlt"],
                    help="mmlt (with --technique mmlt): 2 x S spp per depth of render_mmlt with the render's own options, no pixel left out")
    a = ap.parse_args()
    if a.reference == "mmlt" and a.technique != "mmlt":
        ap.error("--reference mmlt is technique=mmlt's reference: it needs --technique mmlt")

    pkg = entry.load_package()
    sd = pkg.scenes.SCENES[a.scene](a.res)
    depths = dict(max_depth=a.max_depth, rr_depth=a.rr_depth, direct_samples=-1)
    kw = dict(technique=a.technique, type=a.type, algo=pkg.abi.ALGO_PSSMLT if a.algo == "pssmlt" else pkg.abi.ALGO_DRMLT,
              work_units=a.chains, sample_count=a.mpp, **depths)
    if a.technique == "mmlt":
        kw["fix_emitter_path"] = a.fix_emitter_path
    else:
        kw["no_direct_sampling"] = a.no_direct_sampling
    npix = sd.camera.width * sd.camera.height
    t0 = time.perf_counter()
    with pkg.Context(pkg.abi.make_config(**kw), sd) as ctx:
        b = ctx.seed(a.seed)
        t1 = time.perf_counter()
        ctx.run(npix * a.mpp)
        img = ctx.develop()
        t2 = time.perf_counter()
        n_chains = ctx.stats().n_chains
    own = a.reference == "mmlt"
    if own:
        ra, rb, ref_s = reference_mmlt(pkg, sd, kw, a.ref_spp)
    else:
        ra, rb, ref_s = reference(pkg, sd, depths, a.ref_spp, a.no_direct_sampling if a.technique == "bdpt" else 0)
    li, lr = lum(img), lum(0.5 * (ra + rb))
    eps = 1e-2 * lr.mean() ** 2
    # technique=mmlt drops the emitters the camera sees, the reference has them: under the box filter that
    # light lies in the pixels that show an emitter, which are left out of every figure below. (technique=mmlt's own reference
    # drops what the chains drop, under any filter: nothing is left out.)
    keep = ~pkg.binding.visible_emitter_mask(sd) if a.technique == "mmlt" and not own else np.ones(li.shape, dtype=bool)
    kf = keep.astype(np.float64)
    blk = lambda x: (x * kf).reshape(8, a.res // 8, 8, a.res // 8).sum((1, 3)) / np.maximum(kf.reshape(8, a.res // 8, 8, a.res // 8).sum((1, 3)), 1)
    print(json.dumps({
        "scene": a.scene, "res": a.res, "technique": a.technique, "algo": a.algo, "type": a.type, "chains": int(n_chains),
        "max_depth": a.max_depth, "rr_depth": a.rr_depth, "fix_emitter_path": a.fix_emitter_path, "no_direct_sampling": a.no_direct_sampling,
        "mutations_per_pixel": a.mpp, "rel_mse": float(np.mean(((li - lr) ** 2 / (lr ** 2 + eps))[keep])),
        "block_error": float(np.abs(blk(li) - blk(lr)).mean() / lr[keep].mean()),
        "pixels_left_out": int((~keep).sum()),
        "b": b, "mean_luminance": float(li[keep].mean()), "reference_mean_luminance": float(lr[keep].mean()),
        "reference": ("independent samples of the multiplexed estimator ON THE DEVICE (drmlt_render_mmlt), 2 x %d spp per depth, no pixel left out" % a.ref_spp) if own
                     else "independent bidirectional samples ON THE DEVICE (drmlt_render_bdpt), 2 x %d spp" % a.ref_spp,
        "reference_self_rel_mse": float(np.mean(((lum(ra) - lum(rb)) ** 2 / (lr ** 2 + eps))[keep])) / 4.0, "reference_seconds": ref_s, "seed_seconds": t1 - t0, "render_seconds": t2 - t1,
        "note": "per-pixel relative MSE mean((I-R)^2 / (R^2 + 0.01 mean(R)^2)), as bench.py --full; block_error: mean absolute error of "
                "the 8 x 8 block means over the reference mean",
    }))


if __name__ == "__main__":
    main()
