"""Throughput of the technique=bdpt chain kernels (Cornell config-2 scene); DIRECT=0/1 selects directSampling.
--algo drmlt (default: k_mutate_bdpt, orbital) | pssmlt (k_mutate_pssmlt_bdpt), anywhere among the positional arguments
[res] [chains] [mutations per chain] [scene]."""
import sys, time
import os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
abi = pkg.abi
algo = 'drmlt'
if '--algo' in sys.argv:
    i = sys.argv.index('--algo')
    algo = sys.argv[i + 1]
    del sys.argv[i:i + 2]
if algo not in ('drmlt', 'pssmlt'):
    sys.exit('--algo drmlt | pssmlt')
res = int(sys.argv[1]) if len(sys.argv) > 1 else 256
chains = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
per_chain = int(sys.argv[3]) if len(sys.argv) > 3 else 64
scene = sys.argv[4] if len(sys.argv) > 4 else 'cornell_c2'
sd = pkg.scenes.SCENES[scene](res)
cfg = abi.make_config(algo=abi.ALGO_PSSMLT if algo == 'pssmlt' else abi.ALGO_DRMLT, technique='bdpt', type='orbital', max_depth=8, rr_depth=5, direct_samples=-1, no_direct_sampling=0 if os.environ.get('DIRECT', '1') == '1' else 1,
                      work_units=chains, sample_count=1, luminance_samples=100000)
ctx = pkg.Context(cfg, sd)
t0 = time.time(); b = ctx.seed(0x5EED); t_seed = time.time() - t0
ctx.run(chains * 8)
ctx.kernel_time(reset=True)
t0 = time.time(); ctx.run(chains * per_chain); dt = time.time() - t0
ms, n = ctx.kernel_time()
st = ctx.stats()
print('bdpt %s %s res=%d chains=%d: b=%.4f seed %.2fs; %.3e mutations/s wall, %.3e by kernel time, kernel %.2f ms x %d; rays/mut %.2f evals/mut %.3f %s' % (
    algo, scene, res, chains, b, t_seed, chains * per_chain / dt, chains * per_chain / (ms * n * 1e-3) if ms * n > 0 else 0.0, ms, n, st.rays / st.mutations,
    st.path_evals / st.mutations,
    'acc %.3f' % (st.overall_acc / st.overall_base) if algo == 'pssmlt' else 'acc1 %.3f acc2 %.3f' % (st.first_acc / st.first_base, st.second_acc / max(st.second_base, 1))))
