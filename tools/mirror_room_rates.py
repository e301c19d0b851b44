"""mutations/s of scenes.mirror_room at 512^2 (orbital, maxDepth 8): technique=path at 65 536 and 196 608 chains, mmlt at
262 144, bdpt at 131 072. One warm-up run, then the median, minimum and maximum of three timed runs.   python tools/mirror_room_rates.py"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
abi = pkg.abi
sd = pkg.scenes.mirror_room(512)
for name, kw in (("path 65536", dict(work_units=65536)), ("path 196608", dict(work_units=196608)),
                 ("mmlt 262144", dict(technique="mmlt", fix_emitter_path=1, work_units=262144)),
                 ("bdpt 131072", dict(technique="bdpt", work_units=131072))):
    n = kw["work_units"]
    cfg = abi.make_config(type="orbital", max_depth=8, direct_samples=-1, luminance_samples=4 * n, sample_count=64, **kw)
    ctx = pkg.Context(cfg, sd)
    ctx.seed(0x5EED)
    total = 512 * 512 * (16 if kw.get("technique") == "bdpt" else 64)
    ctx.run(total)
    rates = []
    for _ in range(3):
        t = time.perf_counter(); ctx.run(total); rates.append(total / (time.perf_counter() - t))
    print("mirror_room %s: %.4e mutations/s (min %.4e max %.4e)" % (name, sorted(rates)[1], min(rates), max(rates)), flush=True)
    ctx.close()
