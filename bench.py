#!/usr/bin/env python3
"""Benchmark of the DRMLT hot path on MI355X.

Default workload = BASELINE.json configs[1]: Cornell box 512x512, `integrator=drmlt technique=path type=orbital`,
65 536 chains per GPU, sampleCount 256 => one step = one full mutation phase of that render
(512*512*256 = 67 108 864 chain-loop iterations, 1 024 per chain), scene and chain state resident in HBM
before the timed region. Metric = mutations/s (accepted + rejected; one mutation = one first-stage proposal,
reference drmlt_proc.cpp:541).

  python bench.py --gpus 1 --steps 10 --warmup 2      # the defaults: set up, warm up, time the steps, print the line
  python bench.py --full                              # + image quality against a device path-traced reference, CPU baseline
  python bench.py --dump-outputs DIR                  # + what the timed render computed, as DIR/<name>.npy
  python bench.py --config 3|5|bdpt|soup|soup50k  # the other kernels, same JSON line (roofline of THAT kernel)
  python bench.py --gpus N --steps K --warmup W       # N > 1, no launcher: ONE process drives the N devices (drmlt_node_*)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
      bench.py --gpus N --steps K --warmup W          # N > 1 under a launcher: one process per GPU (drmlt_comm_*)

N > 1 without a launcher (WORLD_SIZE unset): the process creates one drmlt_node over devices 0 .. N-1 -- what the Mitsuba
plugin does (`devices` property) --, one host thread per device inside the library, an in-process RCCL communicator
(ncclCommInitAll). It exits non-zero only when fewer than N devices are visible. On a one-GPU box the same code runs with
`DRMLT_TEST_HOOKS=1 DRMLT_NODE_DEVICES=0,0 python bench.py --gpus 2` (ranks share the device, loopback transport).
N > 1: chains partitioned by chain id out of ONE seed pool (no data-path collective). The K timed steps
are ONE render (one drmlt_run call, as the Mitsuba adaptor issues it) that ends with ONE film exchange, issued from C++
inside libdrmlt_amd.so (drmlt_exchange_tiled) and enqueued behind the chain kernels: ncclReduceScatter(sum) of the
W*H*3 fp32 film -- rank r keeps rows [r ceil(H/N), ...) -- plus one two-element ncclAllReduce, then every rank develops its
tile (reference: DRMLTProcess::processResult / develop, drmlt_proc.cpp:813-867). The JSON line says so ("exchanges": 1) and
reports a blocking exchange timed on its own ("exchange_ms", outside the timed region), the communicator's own rank count
("rccl_nranks", from ncclCommCount -- the run FAILS if it differs from --gpus) and every rank's chain range.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md

# name -> (scene builder args, config kwargs, chains, sampleCount per step, kernel, description)
CONFIGS = {
    "2": dict(scene=("cornell_c2", {}), res=512, cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5),
              spp=256, kernel="k_mutate_v4", pmc="r02_c2_pmc.json",   # (BASELINE fixes 65 536 chains: k_mutate_v4's ground)
              what="Cornell box %(res)dx%(res)d, integrator=drmlt technique=path type=orbital, %(chains)d chains/GPU, "
                   "sampleCount %(spp)d (BASELINE.json configs[1])"),
    # the same render with the chain count left to the library (workUnits = -1 -> 196 608 chains, k_mutate_v5 with its proposal rows in
    # device memory and three waves per SIMD; sampleCount 240: a whole number of mutations per chain): NOT the headline
    "2x": dict(scene=("cornell_c2", {}), res=512, chains=196608, cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5),
               spp=240, kernel="k_mutate_v5", pmc="r03_2x_pmc.json",
               what="Cornell box %(res)dx%(res)d, integrator=drmlt technique=path type=orbital, %(chains)d chains/GPU (the library's own "
                    "choice for workUnits = -1; BASELINE.json configs[1] fixes 65 536: see config 2), sampleCount %(spp)d"),
    # BASELINE's config 3 does not fix the chain count: 196 608 chains (what workUnits = -1 derives) run k_mutate_v5 -- 64 chains per
    # wave, three waves per SIMD, proposal rows in device memory; sampleCount 240: a whole number of mutations per chain
    "3": dict(scene=("door_c3", {}), res=512, chains=196608, cfg=dict(technique="path", type="green", max_depth=8, rr_depth=5),
              spp=240, kernel="k_mutate_v5", pmc="r02_c3_pmc.json",
              what="door scene (occluded area light, rough-conductor floor) %(res)dx%(res)d, drmlt technique=path type=green, "
                   "%(chains)d chains/GPU, sampleCount %(spp)d (BASELINE.json configs[2])"),
    # 262 144 chains: k_mutate_mmlt runs one chain per lane at 256 VGPRs, so 65 536 chains are 1024 waves = one per SIMD
    # (7.3e8 mutations/s); 131 072 put two on a SIMD (1.3e9); 262 144 are two ROUNDS of such waves, and with the chains run in
    # order of their depth the shallow waves' slots are re-used while the deep ones still run (2.1e9; 2.5e9 since its chains run free). BASELINE's config 5
    # does not fix the chain count.
    # (round 4: 1 048 576 chains -- what workUnits = -1 derives for long renders, 2^35 mutations and more -- queue eight rounds of waves: the
    # more rounds, the less of a launch is its tail; the bootstrap set of a million chains costs 2.3 s of seeding, outside the timed region,
    # against 0.6 s at 262 144 chains = 2.56e9: DESIGN section 6)
    "5": dict(scene=("caustic_c5", {}), res=512, chains=1048576,
              cfg=dict(technique="mmlt", type="orbital", max_depth=6, fix_emitter_path=1, acceptance_map=1), spp=256,
              kernel="k_mutate_mmlt", pmc="r02_c5_pmc.json",
              what="glass caustic (dielectric sphere, small sphere light) %(res)dx%(res)d, drmlt technique=mmlt type=orbital "
                   "fixEmitterPath acceptanceMap, %(chains)d chains/GPU, sampleCount %(spp)d (BASELINE.json configs[4])"),
    # 131 072 chains, as config 5: above 65 536 the launcher picks the two-waves-per-SIMD build of k_mutate_bdpt
    "bdpt": dict(scene=("cornell_c2", {}), res=512, chains=131072, cfg=dict(technique="bdpt", type="orbital", max_depth=8, rr_depth=5),
                 spp=256, kernel="k_mutate_bdpt", pmc="r02_bdpt_pmc.json",
                 what="Cornell box %(res)dx%(res)d, drmlt technique=bdpt type=orbital, %(chains)d chains/GPU, sampleCount %(spp)d"),
    # BVH scenes run k_mutate_v5 (ray pool, 64 chains per wave): 196 608 chains put three waves on every SIMD (proposal rows in device
    # memory; sampleCount 240: a whole number of mutations per chain)
    "soup": dict(scene=("triangle_soup", dict(n_tris=2000)), res=512, chains=196608,
                 cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5), spp=240, kernel="k_mutate_v5",
                 pmc="r02_soup_pmc.json", ref_spp=2048,
                 what="closed room with 2000 random triangles (BVH in HBM) %(res)dx%(res)d, drmlt technique=path type=orbital, "
                      "%(chains)d chains/GPU, sampleCount %(spp)d"),
    # 50 000 / 1 000 000 triangles: the waves are parked on node fetches more than half of their time, and what covers a fetch is
    # another wave. From 163 840 chains up k_mutate_v5 keeps its proposal rows in device memory and is built for THREE waves per
    # SIMD (kernels.hip: ROWS_MEM): 196 608 chains fill them (sampleCount 240 / 60: a whole number of mutations per chain).
    "soup50k": dict(scene=("triangle_soup", dict(n_tris=50000)), res=512, chains=196608,
                    cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5), spp=240, kernel="k_mutate_v5",
                    pmc="r02_soup50k_pmc.json", ref_spp=512,
                    what="closed room with 50000 random triangles (BVH, primitive and shading records: 9.6 MB in HBM / L2; "
                         "32-bit traversal stacks) %(res)dx%(res)d, drmlt technique=path type=orbital, %(chains)d chains/GPU, "
                         "sampleCount %(spp)d"),
    # a scene whose node / primitive / shading records (188 MB) exceed the L2 caches: the regime SURVEY 8(d) names as the one
    # where memory, not instruction issue, would bound the path. 60 mutations/pixel per step (the scene is slow to traverse).
    "soup1m": dict(scene=("triangle_soup", dict(n_tris=1000000)), res=512, chains=196608,
                   cfg=dict(technique="path", type="orbital", max_depth=8, rr_depth=5), spp=60, kernel="k_mutate_v5",
                   pmc="r02_soup1m_pmc.json", no_cpu_baseline="the CPU restatement has no acceleration structure: brute force over "
                   "1e6 triangles per ray is not a baseline (soup50k already runs 3e3 mutations/s on 16 threads)", no_quality=True,
                   what="closed room with 1000000 random triangles (BVH, primitive and shading records: 188 MB, beyond L2, inside "
                        "the MALL) %(res)dx%(res)d, drmlt technique=path type=orbital, %(chains)d chains/GPU, sampleCount %(spp)d"),
}


def host_threads():
    """Threads for the CPU baseline: the cgroup CPU quota / affinity of this box, not the host's core count."""
    if os.environ.get("BENCH_CPU_THREADS"):
        return max(1, int(os.environ["BENCH_CPU_THREADS"]))
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except Exception:
            pass
    return min(n, 64)


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def _clean(o):
    """Strict JSON: NaN / inf become null."""
    if isinstance(o, float):
        return o if np.isfinite(o) else None
    if isinstance(o, dict):
        return {k: _clean(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_clean(v) for v in o]
    return o


def dump_outputs(out_dir, arrays, budget=64 << 20):
    """DIR/<name>.npy, float32 or float64. An array larger than half the budget is stored as a fixed, seeded sample of its rows (pixels
    of an image): <name>.npy holds the sampled rows, <name>_index.npy their flat indices."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        if a.nbytes > budget // 2:
            rows = a.reshape(-1, a.shape[-1] if a.ndim > 1 else 1)
            n = (budget // 2) // (rows.shape[1] * a.itemsize + 8)
            idx = np.sort(np.random.default_rng(0x5EED).choice(rows.shape[0], size=n, replace=False))
            np.save(os.path.join(out_dir, name + "_index.npy"), idx.astype(np.float64))
            a = rows[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def lum(img):
    return img @ np.array([0.212671, 0.715160, 0.072169])


def build_scene(pkg, conf, res):
    name, kw = conf["scene"]
    return pkg.scenes.SCENES[name](res=res, **kw)


def cpu_baseline(pkg, conf, res, cfg_kw, target_seconds):
    """Time the CPU restatement (oracle/, -O3 -march=native, fp64 like the reference's CMake build) on all host cores on a
    bounded sample of the same workload: same scene/config, fewer chains x fewer mutations."""
    ob = entry.load_oracle()
    ob.build(native=True)
    abi = pkg.abi
    cores = host_threads()
    sd = build_scene(pkg, conf, res)
    chains = 64 * cores
    cfg = abi.make_config(work_units=chains, luminance_samples=20000, **cfg_kw)
    orc = ob.Oracle(abi, cfg, sd, precision=64, native=True)
    orc.seed(0x5EED)
    probe, rate = chains * 4, 0.0
    while True:  # a probe long enough to time (the oracle has no acceleration structure: big scenes are slow)
        t = time.time()
        orc.run(probe, cores)
        dt = time.time() - t
        rate = probe / max(dt, 1e-6)
        if dt > 0.5 or probe >= chains * 256:
            break
        probe *= 4
    per_chain = max(8, int(rate * target_seconds / chains))
    total = chains * per_chain
    t = time.time()
    orc.run(total, cores)
    dt = time.time() - t
    orc.close()
    return {"value": total / dt, "unit": "mutations/s", "cores": cores, "kind": "port", "cpu": cpu_model(),
            "sample": "oracle (fp64 CPU restatement, one chain per work unit on a thread pool) on %d threads: same scene and "
                      "config, %d chains x %d mutations = %d mutations in %.1f s" % (cores, chains, per_chain, total, dt),
            "per_core": total / dt / cores}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--config", default="2", choices=sorted(CONFIGS))
    ap.add_argument("--res", type=int, default=0, help="film size (default: the configuration's)")
    ap.add_argument("--chains", type=int, default=None, help="chains per GPU (default: the configuration's own, 65536 unless noted)")
    ap.add_argument("--spp", type=int, default=0, help="mutations per pixel per step (sampleCount)")
    ap.add_argument("--type", default="")
    ap.add_argument("--full", action="store_true", help="also measure what the headline figure does not need: image quality against a "
                    "device path-traced reference (technique=path) and the CPU baseline (world size 1); off by default")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="after the timed steps, write what they computed as DIR/<name>.npy: "
                    "the developed image, the luminance normalisation b and the timed steps' mutation counts")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--no-quality", action="store_true", help="with --full: leave out the image quality")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--with-progress", action="store_true", help="run with a progress callback, as the Mitsuba plugin does: the library then cuts "
                    "the call into launches of 256 mutations per chain and synchronises after each (ADVICE r03: the plugin path's own line)")
    args = ap.parse_args()
    conf = CONFIGS[args.config]
    res = args.res or conf["res"]
    spp = args.spp or conf["spp"]
    if args.chains is None:
        args.chains = conf.get("chains", 65536)

    # Libraries loaded below write to the process's stdout on their own (RCCL prints a version banner when its first
    # communicator comes up): keep file descriptor 1 pointed at stderr until the one JSON line is ready.
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist

    env_world = os.environ.get("WORLD_SIZE")
    # No launcher and --gpus N > 1: ONE process drives the N devices through drmlt_node_* 
    node_mode = env_world is None and args.gpus > 1
    world = args.gpus if node_mode else int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the DRMLT path has no CPU fallback")
    hook = os.environ.get("DRMLT_NODE_DEVICES") if os.environ.get("DRMLT_TEST_HOOKS") == "1" else None
    if node_mode:
        node_devices = [int(d) for d in hook.split(",")] if hook else list(range(args.gpus))
        if len(node_devices) != args.gpus:
            raise SystemExit("bench.py: --gpus %d but DRMLT_NODE_DEVICES names %d ranks" % (args.gpus, len(node_devices)))
        if max(node_devices) >= torch.cuda.device_count():
            raise SystemExit("bench.py: --gpus %d but only %d device(s) visible" % (args.gpus, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    # BENCH_FORCE_DIST=1 rehearses the one-process-per-GPU path (process group, RCCL communicator, tiled exchange) on one GPU
    use_dist = not node_mode and (world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1")
    multi = use_dist or node_mode
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29512")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))

    pkg = entry.load_package()
    abi = pkg.abi
    cfg_kw = dict(direct_samples=-1, sample_count=spp, **conf["cfg"])
    if args.type:
        cfg_kw["type"] = args.type
    sd = build_scene(pkg, conf, res)
    # luminanceSamples: the reference's floor max(100000, 10 workUnits) (50 x for mmlt), applied inside drmlt_seed
    cfg = abi.make_config(work_units=args.chains, luminance_samples=100000, **cfg_kw)
    npix = res * res
    step_mutations = npix * spp                                # per GPU
    node = None
    if node_mode:
        # cfg.work_units is PER DEVICE; seeds from one pool, one host thread per device, film exchange over the node's communicator
        node = pkg.Node(cfg, sd, device_mask=sum(1 << d for d in set(node_devices)))
        if node.device_count != args.gpus:
            raise SystemExit("bench.py: --gpus %d but the node drives %d device(s)" % (args.gpus, node.device_count))
        ctxs = [node.context(r) for r in range(world)]
        ctx = ctxs[0]
        b = node.seed(0x5EED)
        ranks_info = []
        for r in range(world):
            nr, rr = ctxs[r].comm_info()   # ncclCommCount / ncclCommUserRank of rank r's communicator (loopback: the node's own count)
            ranks_info.append({"rank": r, "rccl_rank": rr, "rccl_nranks": nr, "device": node_devices[r],
                               "chains": [r * args.chains, (r + 1) * args.chains], "film_rows": list(pkg.binding.film_tile(res, r, world)[:2])})
        rccl_nranks = ranks_info[0]["rccl_nranks"]
    else:
        ctx = pkg.Context(cfg, sd, device=local_rank)
        ctxs = [ctx]
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        # bootstrap + seed replay: outside the timed region. One seed pool for the job: every rank finds the same b
        b = ctx.seed_pool(0x5EED, rank * args.chains, world * args.chains)
        if use_dist:  # the library's own RCCL communicator: rank 0 creates the id, the process group only carries its 128 bytes
            uid = torch.zeros(128, dtype=torch.uint8, device="cuda")
            if rank == 0:
                uid.copy_(torch.frombuffer(bytearray(pkg.comm_unique_id()), dtype=torch.uint8))
            dist.broadcast(uid, 0)
            ctx.comm_init(bytes(uid.cpu().numpy().tobytes()), rank, world)
        # what the library's communicator says about itself, and which chains of the pool every rank runs
        rccl_nranks, rccl_rank = ctx.comm_info() if use_dist else (1, 0)
        mine = {"rank": rank, "rccl_rank": rccl_rank, "rccl_nranks": rccl_nranks, "device": local_rank,
                "chains": [rank * args.chains, (rank + 1) * args.chains], "film_rows": list(pkg.binding.film_tile(res, rank, world)[:2])}
        ranks_info = [mine]
        if use_dist:
            ranks_info = [None] * world
            dist.all_gather_object(ranks_info, mine)
    bad = [r for r in ranks_info if r["rccl_nranks"] != args.gpus or r["rccl_rank"] != r["rank"]]
    if bad or world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the RCCL communicator reports %s (WORLD_SIZE=%s)" % (args.gpus, bad or ranks_info, env_world))

    def barrier():
        if use_dist:
            dist.barrier()
        if node_mode:
            for d in sorted(set(node_devices)):
                torch.cuda.synchronize(d)
        else:
            torch.cuda.synchronize()

    last = {}
    progress = (lambda done, total: None) if args.with_progress else None

    def steps(k):
        """k steps of the render = ONE call into the library, which cuts it into launches of 1024 mutations per chain (one per
        step at 65 536 chains) -- as a renderer calls it (the adaptor hands drmlt_run its whole budget). Between those launches
        chains that have reached a launch's target run ahead towards the call's total instead of idling until the slowest chain
        is there; the call returns with every chain at exactly its count. Followed, for N > 1, by the render's film exchange:
        reduce-scatter + scalar all-reduce + tile develop, all in C++ -- enqueued behind the chain kernels (one process per GPU),
        or drmlt_node_develop, which also brings the stitched image to the host (one process, N devices)."""
        if node_mode:
            node.run(k * step_mutations * world, progress=progress)   # the node's total: an N-th of it per device
            if not os.environ.get("BENCH_SKIP_EXCHANGE"):
                last["image"] = node.develop()
            return
        if os.environ.get("BENCH_CALL_PER_STEP"):
            for _ in range(k):
                ctx.run(step_mutations, progress=progress)
        else:
            ctx.run(k * step_mutations, progress=progress)
        if use_dist and not os.environ.get("BENCH_SKIP_EXCHANGE"):
            ctx.exchange_tiled(b, want_tile=False, wait=False)

    def job_stats():
        return node.stats() if node_mode else ctx.stats()

    if args.warmup:
        steps(args.warmup)
        for c in ctxs:
            c.film_clear()
    for c in ctxs:
        c.kernel_time(reset=True)
    st0 = job_stats()
    rank_m0 = [c.stats().mutations for c in ctxs]
    barrier()
    t0 = time.perf_counter()
    steps(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if use_dist:
        et = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(et, op=dist.ReduceOp.MAX)
        elapsed = float(et.item())

    st1 = job_stats()
    # the dominant kernel's launches by HIP events on the launch stream: one process, N devices -> the slowest device's average
    kt = [c.kernel_time() for c in ctxs]
    launch_ms, launches = max(kt)
    exchange_ms = None
    if use_dist:  # one BLOCKING exchange on its own clock (the timed region's exchange is enqueued behind the chain kernels)
        barrier()
        te = time.perf_counter()
        ctx.exchange_tiled(b, want_tile=False, wait=True)
        barrier()
        xt = torch.tensor([time.perf_counter() - te], dtype=torch.float64, device="cuda")
        dist.all_reduce(xt, op=dist.ReduceOp.MAX)
        exchange_ms = 1e3 * float(xt.item())
    selfcheck = None
    if node_mode:  # drmlt_node_develop on its own clock: reduce-scatter + all-reduce + develop of every tile + the image to the host
        te = time.perf_counter()
        img_node = node.develop()
        exchange_ms = 1e3 * (time.perf_counter() - te)
        # self-check inside the line: every device ran its share, and the stitched image is normalised to b
        rank_muts = [c.stats().mutations - m0 for c, m0 in zip(ctxs, rank_m0)]
        want_mut = args.steps * step_mutations
        mean_lum = float(lum(img_node.astype(np.float64)).mean())
        amap = bool(cfg_kw.get("acceptance_map"))
        selfcheck = {"rank_mutations": rank_muts, "sum_rank_mutations": int(sum(rank_muts)), "expected_total": int(want_mut * world),
                     "mutations_ok": all(m == want_mut for m in rank_muts),
                     "image_mean_luminance": mean_lum, "b": b,
                     "luminance_ok": True if amap else bool(abs(mean_lum - b) <= 1e-3 * b),
                     "timed_image_equals_this_one": bool(np.array_equal(last.get("image"), img_node)) if "image" in last else None,
                     "rank_film_mass": [float(c.film().astype(np.float64).sum()) for c in ctxs]}
        if not (selfcheck["mutations_ok"] and selfcheck["luminance_ok"]):
            raise SystemExit("bench.py: self-check failed: %s" % json.dumps(selfcheck))
    # (one process, N devices: the node's statistics are already sums over its devices)
    per_dev = 1.0 / world if node_mode else 1.0   # job statistics -> one device's share
    agg = 1 if node_mode else world                # this process's statistics -> the job's
    muts = st1.mutations - st0.mutations
    accepted = st1.accepted - st0.accepted
    evals = st1.path_evals - st0.path_evals
    rays = st1.rays - st0.rays
    value = world * args.steps * step_mutations / elapsed

    if args.dump_outputs:
        # what the timed render computed, as its caller receives it (outside the timed region): the developed image -- the node's
        # stitched one; one process per GPU: every rank's tile, gathered on rank 0 --, b and the timed steps' mutation counts (mutations,
        # accepted: this process's, the node's sums in node mode)
        if node_mode:
            img_out = img_node
        elif use_dist:
            tile, rows, _ = ctx.exchange_tiled(b)
            parts = [None] * world
            dist.all_gather_object(parts, (rows, tile))
            img_out = np.zeros((res, res, 3), dtype=np.float32)
            for (lo, hi), t in parts:
                img_out[lo:hi] = t
        else:
            img_out = ctx.develop()
        if rank == 0:
            dump_outputs(args.dump_outputs, {"image": img_out, "b": np.array([b], dtype=np.float64),
                                             "mutations": np.array([muts, accepted], dtype=np.float64)})

    out = None
    if rank == 0:
        # ---- roofline of the dominant kernel: algorithmic bytes per SURVEY 8(d) / DESIGN.md section 3
        D = st1.max_dim
        p_acc = accepted / muts
        n_splats = 2.0 + (st1.second_base - st0.second_base) / muts
        bytes_per_mut = (4 * D + 32) * (1.0 + p_acc) + 24.0 * n_splats
        # BVH scenes: the scene part of the algorithmic bytes (SURVEY 8d B_scene) is what the traversals fetched, counted by the
        # kernel itself: 128 B per 4-wide node visited, 64 B per primitive record tested
        bvh_nodes = (st1.bvh_node_visits - st0.bvh_node_visits) / muts
        bvh_prims = (st1.bvh_prim_tests - st0.bvh_prim_tests) / muts
        scene_bytes = 128.0 * bvh_nodes + 64.0 * bvh_prims
        bytes_per_mut += scene_bytes
        muts_per_launch = muts * per_dev / max(launches, 1)   # per device, like launch_ms
        achieved = bytes_per_mut * muts_per_launch / (launch_ms * 1e-3) / 1e9 if launch_ms > 0 else 0.0
        traffic = valu_frac = lane_util = atomics_per_mut = None
        traffic_source = None
        # the newest committed counter summary of this configuration (profiles/rNN_<name>_pmc.json)
        stem = conf["pmc"].split("_", 1)[1]
        pmc_name = next((n for n in ("r%02d_%s" % (r, stem) for r in range(9, 1, -1)) if os.path.exists(os.path.join(ROOT, "profiles", n))), conf["pmc"])
        pmc = os.path.join(ROOT, "profiles", pmc_name)
        if os.path.exists(pmc):
            try:
                # NOT measured in this run: counters cannot be read from inside the process. The committed summary holds
                # rocprofv3 --pmc passes (one per counter group, gfx950 corrections applied) of this same command with a
                # shorter launch; HBM traffic and instruction counts are proportional to the mutation count.
                pj = json.load(open(pmc))
                traffic = pj.get("hbm_bytes_per_mutation") * muts_per_launch
                traffic_source = "scaled per mutation from profiles/%s (rocprofv3 --pmc, separate passes), not read in this run" % pmc_name
                # wave-level VALU instructions per mutation (SQ_INSTS_VALU) against 1024 SIMDs x one wave64 VALU op per 2 cycles
                valu_frac = pj["instructions_per_mutation"]["valu"] * muts_per_launch / (launch_ms * 1e-3) / (1024 * 2.4e9 / 2)
                lane_util = pj.get("valu_lane_utilisation")
                atomics_per_mut = pj.get("atomic_requests_per_mutation")
            except Exception:
                traffic = None
        bvh_scene = args.config.startswith("soup")
        hbm_measured_gbs = (traffic / (launch_ms * 1e-3) / 1e9) if traffic and launch_ms > 0 else None
        roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source,
                "kernel": conf["kernel"], "avg_launch_ms": launch_ms, "launches": launches,
                "algorithmic_bytes_per_mutation": bytes_per_mut,
                "scene_bytes_per_mutation": scene_bytes, "bvh_node_visits_per_mutation": bvh_nodes,
                "bvh_prim_tests_per_mutation": bvh_prims,
                "mutations_per_launch": muts_per_launch,
                "hbm_measured_gbs": hbm_measured_gbs,
                "hbm_measured_frac": hbm_measured_gbs / HBM_PEAK_GBS if hbm_measured_gbs else None,
                "note": "north_star's '>= 30 % of the HBM-read roofline' is not met and cannot be on this scene class: "
                        "scene (scalar cache / LDS) and chain state (LDS) are on chip, compulsory HBM traffic is the film "
                        "atomics (SURVEY 8d); the kernel is bound by VALU issue x lane utilisation: see roofline_valu"}
        if args.config == "bdpt":
            roof["note"] = ("bdpt keeps every stored vertex in device memory (80 B records, written by the walks, gathered two per connection "
                            "cell: ~17 cells per evaluation) next to its splat lists: `traffic` is what of that misses the L2s; "
                            "`algorithmic_bytes_per_mutation` is SURVEY 8(d)'s state + lists + film formula and leaves the vertex workspace out. "
                            "Bound by VALU issue x lane utilisation: see roofline_valu")
        if bvh_scene:
            # requested bytes that L2 serves must never stand in for HBM bytes. On BVH scenes the node / primitive
            # fetches the kernel counts are (mostly) L2 hits, so `achieved` / `frac` are the MEASURED HBM figure here (PMC
            # summary scaled per mutation) and the requested-bytes rate is reported under its own name.
            roof.update({"achieved": hbm_measured_gbs, "frac": hbm_measured_gbs / HBM_PEAK_GBS if hbm_measured_gbs else None,
                         "achieved_source": "measured HBM bytes (" + (traffic_source or "no PMC summary committed") + ")",
                         "requested_gbs_incl_l2_hits": achieved, "requested_frac_of_hbm_peak_NOT_A_ROOFLINE_FIGURE": achieved / HBM_PEAK_GBS,
                         "note": "BVH and primitive records live in HBM / L2: frac = measured HBM bytes / peak; the requested-bytes rate "
                                 "(128 B per node visited + 64 B per primitive tested, counted by the kernel) is mostly L2 hits and is "
                                 "listed separately. The traversal is latency-bound (dependent node fetches), not bandwidth-bound"})
        # The bound that actually binds: wave64 VALU instructions issued per SIMD-cycle (peak: one per 2 cycles
        # per SIMD, 1024 SIMDs at 2.4 GHz) x the fraction of lanes active in them = useful lane-operations against the VALU peak.
        roof_valu = None
        lane_util_source = "SQ_THREAD_CYCLES_VALU / (64 SQ_ACTIVE_INST_VALU)"
        it_node, it_leaf = st1.bvh_node_iterations - st0.bvh_node_iterations, st1.bvh_leaf_iterations - st0.bvh_leaf_iterations
        if bvh_scene and lane_util is not None and it_node + it_leaf > 0:
            # BVH lines: the exec mask of the straight-line traversal blocks counts lanes that compute on zeros and
            # keep nothing. The kernel's own counters say how many lanes ADVANCE per traversal iteration; weighted by what an
            # iteration of either kind costs (a leaf iteration ~ 0.4 node iterations, drmlt_capi.cpp: trace_vote).
            adv = ((st1.bvh_node_visits - st0.bvh_node_visits) + 0.4 * (st1.bvh_prim_tests - st0.bvh_prim_tests)) / (64.0 * (it_node + 0.4 * it_leaf))
            lane_util_pmc, lane_util = lane_util, min(lane_util, adv)
            lane_util_source = ("lanes that ADVANCE per traversal iteration, counted by the kernel in this run (%.1f of 64 per node iteration, %.1f per leaf "
                                "iteration); the counters' exec-mask figure (%.2f) includes lanes that compute on zeros" %
                                ((st1.bvh_node_visits - st0.bvh_node_visits) / max(it_node, 1), (st1.bvh_prim_tests - st0.bvh_prim_tests) / max(it_leaf, 1), lane_util_pmc))
        if valu_frac is not None and lane_util is not None:
            roof_valu = {"bound": "valu", "achieved": valu_frac * lane_util * 1024 * 2.4e9 / 2 * 64 / 1e12, "peak": 1024 * 2.4e9 / 2 * 64 / 1e12,
                         "unit": "T lane-ops/s", "frac": valu_frac * lane_util, "valu_issue_frac_of_peak": valu_frac,
                         "valu_lane_utilisation": lane_util, "valu_lane_utilisation_source": lane_util_source, "source": traffic_source,
                         "note": "frac = (SQ_INSTS_VALU per mutation x mutations/s / (1024 SIMDs x 1.2e9 wave-instructions/s)) x "
                                 "(SQ_ACTIVE_INST lanes / 64): instruction counts from the committed PMC summary, rate from this run"}
        # The nearest MEMORY-side ceiling: the film splats are no-return float atomics executed at the memory side
        # (MI355X_MICROARCH.md, Global float atomics). A flush instruction carries 21 splats = 21 x 3 adjacent dwords in (mostly)
        # 21 different film rows -- the guide's scattered shape: 64 lanes in 64 rows run at ~0.08 TB/s of ADDED bytes, 256
        # contiguous bytes at ~1.3 TB/s. Requests per mutation from the committed counter summary (TCC_EA0_ATOMIC), rate from this run.
        roof_atomic = None
        if atomics_per_mut is not None and launch_ms > 0:
            # The guide's scattered figure is 64 lanes adding one dword each to 64 different rows: 0.08 TB/s of added bytes = 2.0e10
            # row REQUESTS per second (each leaves L2 as its own memory-side atomic). A splat is one such request carrying three dwords,
            # so the ceiling is priced in requests, not in bytes.
            req_s = atomics_per_mut * muts_per_launch / (launch_ms * 1e-3)
            peak_req = 0.08e12 / 4.0
            roof_atomic = {"bound": "memory-side float atomics, scattered (one request per splat: 3 adjacent dwords of one film row)",
                           "achieved": req_s / 1e9, "peak": peak_req / 1e9, "unit": "G atomic requests/s", "frac": req_s / peak_req,
                           "atomic_requests_per_mutation": atomics_per_mut, "added_gbs": req_s * 12.0 / 1e9, "source": traffic_source,
                           "note": "peak = MI355X_MICROARCH.md (Global float atomics): 64 lanes in 64 different rows run at ~0.08 TB/s of added bytes = 2.0e10 "
                                   "requests/s (256 contiguous bytes per instruction: 1.3 TB/s); scales with every mutations/s gain"}
        out = {
            "metric": "mutations/sec (accepted+rejected)", "value": value, "unit": "mutations/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": conf["what"] % dict(res=res, chains=args.chains, spp=spp), "name": args.config,
                       "max_depth": cfg_kw["max_depth"], "rr_depth": cfg_kw.get("rr_depth", 5), "p_large": 0.3, "filter": "box",
                       "mutations_per_step_per_gpu": step_mutations, "progress_callback": bool(args.with_progress),
                       "parallelism": ("chains partitioned x%d, one seed pool; film reduce-scatter + scalar all-reduce (RCCL from C++); " % world +
                                       ("one process drives the %d devices (drmlt_node_*, ncclCommInitAll)" % world if node_mode else "one process per GPU (drmlt_comm_*)"))
                       if multi else "1 GPU"},
            "roofline": roof, "roofline_valu": roof_valu, "roofline_atomic": roof_atomic,
            "rccl_nranks": rccl_nranks if multi else None, "ranks": ranks_info,
            "launch_mode": "node" if node_mode else ("process-per-gpu" if use_dist else "single"),
            "transport": None if not multi else ("loopback (test hook: ranks share a device, films summed by a device kernel)"
                                                 if node_mode and len(set(node_devices)) < len(node_devices) else "rccl"),
            "exchanges": (0 if os.environ.get("BENCH_SKIP_EXCHANGE") else 1) if multi else 0, "exchange_ms": exchange_ms,
            "selfcheck": selfcheck,
            "accepted_mutations_per_s": agg * accepted / elapsed,
            "path_evals_per_s": agg * evals / elapsed, "rays_per_s": agg * rays / elapsed,
            "acceptance": {k: (round(v, 5) if v is not None else None) for k, v in st1.ratios().items()},
        }
        # the committed device-vs-oracle statistics of THIS configuration (tools/parity_protocol.py; the BVH scenes: the 300-triangle sweep run)
        pname = {"2": "parity_protocol_c2", "2x": "parity_protocol_c2", "3": "parity_protocol_c3", "5": "parity_protocol_c5", "bdpt": "parity_protocol_bdpt"}.get(args.config, "protocol_sweep_soup300_path")
        proto = next((q for q in (os.path.join(ROOT, "profiles", n) for n in ["r%02d_%s.json" % (r, pname) for r in range(9, 2, -1)] + ["r02_parity_protocol.json"]) if os.path.exists(q)), "")
        if os.path.exists(proto):
            try:
                out["parity_protocol"] = json.load(open(proto)).get("summary")
            except Exception:
                pass

    # ---- --full: image quality at the accumulated budget (outside the timed region)
    # (technique=path only: the device path tracer used as reference shares the path integrator's treatment of maxDepth;
    # the bidirectional techniques are held to the oracle's bdpt / mmlt renders in tests/test_gpu_bdpt.py, test_gpu_mmlt.py)
    if args.full and not args.no_quality and not conf.get("no_quality") and not cfg_kw.get("acceptance_map") and cfg_kw.get("technique", "path") == "path":
        if use_dist:  # every rank develops its tile of the summed film; rank 0 collects them
            tile, rows, b_mean = ctx.exchange_tiled(b)
            parts = [None] * world
            dist.all_gather_object(parts, (rows, tile))
            img = np.zeros((res, res, 3), dtype=np.float32)
            for (lo, hi), t in parts:
                img[lo:hi] = t
        elif node_mode:
            img, b_mean = img_node, b
        else:
            img, b_mean = ctx.develop(), b
        if rank == 0:
            li = lum(img)
            # Reference: independent path tracing of the same integrand on the device, two halves with different seeds: their
            # difference prices the reference's own error (rel. MSE of the mean of two halves = that of their difference / 4).
            ref_spp = int(os.environ.get("BENCH_REF_SPP", str(conf.get("ref_spp", 16384))))
            tq = time.perf_counter()
            ra, rb = ctx.render_pt(ref_spp, seed=4242), ctx.render_pt(ref_spp, seed=977)
            ref = 0.5 * (ra.astype(np.float64) + rb.astype(np.float64))
            lr = lum(ref)
            eps = 1e-2 * lr.mean() ** 2
            ref_self = float(np.mean((lum(ra) - lum(rb)) ** 2 / (lr ** 2 + eps))) / 4.0
            rmse = float(np.mean((li - lr) ** 2 / (lr ** 2 + eps)))
            out["quality"] = {"rel_mse": rmse, "mutations_per_pixel": spp * args.steps * world,
                              "reference": "independent path tracing of the same integrand ON THE DEVICE, 2 x %d spp" % ref_spp,
                              "reference_self_rel_mse": ref_self, "reference_seconds": time.perf_counter() - tq,
                              "b": b_mean, "mean_luminance": float(li.mean()),
                              "note": "per-pixel relative MSE mean((I-R)^2 / (R^2 + 0.01 mean(R)^2)) (SURVEY 8d); device vs CPU-oracle "
                                      "protocol at equal budgets: parity_protocol"}
        # north_star's bar (rel. MSE < 1e-3 at equal sample budget) at a NAMED budget: keep mutating, outside the timed region
        goal_mpp = int(os.environ.get("BENCH_QUALITY_MPP", "8192"))
        done_mpp = spp * args.steps * world
        if goal_mpp > done_mpp and not multi:
            ctx.run((goal_mpp - done_mpp) * npix)
            img2 = ctx.develop()
            if rank == 0:
                out["quality"]["at_budget"] = {"mutations_per_pixel": goal_mpp,
                                               "rel_mse": float(np.mean((lum(img2) - lr) ** 2 / (lr ** 2 + eps))),
                                               "meets_1e-3": bool(np.mean((lum(img2) - lr) ** 2 / (lr ** 2 + eps)) < 1e-3)}
    # ---- --full: the CPU baseline
    if args.full:
        if rank == 0 and world == 1 and conf.get("no_cpu_baseline"):
            out["cpu_baseline"] = {"value": None, "unit": "mutations/s", "cores": 0, "kind": "port", "sample": "not measured: " + conf["no_cpu_baseline"]}
        elif rank == 0 and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(pkg, conf, res, cfg_kw, args.cpu_seconds)
        elif rank == 0:
            out["cpu_baseline"] = None
    if rank == 0:
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(_clean(out)), flush=True)
        os.dup2(2, 1)  # whatever is printed during teardown goes to stderr as well
    for c in ctxs:
        c.close()
    if node is not None:
        node.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
