"""The oracle's side of the strategy-by-strategy comparison of drmlt_render_bdpt_layers (tests/test_bdpt_layers.py on the CPU,
tests/test_gpu_bdpt_layers.py on the device): Oracle.mmlt_eval evaluates ONE strategy (s, t) of a given depth per point, so its
points, split by the strategy they drew, are per-strategy estimates that share no code with the device's cell loop. Plain
functions: no fixtures, nothing that needs a GPU."""
import numpy as np

import render_bdpt_scenes as rs

RES, MAX_DEPTH, DEPTHS_COMPARED, N_POINTS = 16, 4, (2, 3), 16384
_CACHE = {}


def config(pkg, **kw):
    """cornell_c2(16)'s configuration: maxDepth 4, no direct sampling (MMLT's weights are miWeight without the sampleDirect
    ratios), light image on."""
    base = dict(technique="bdpt", type="orbital", max_depth=MAX_DEPTH, rr_depth=4, direct_samples=-1, no_direct_sampling=1,
                work_units=16384, luminance_samples=20000)
    base.update(kw)
    return pkg.abi.make_config(**base)


def strategy_contributions(pkg, ob, n=N_POINTS):
    """{(d, s): (n, 4, 4) fp64}: per-point contributions to the 4 x 4 block means of the luminance of weighted layer (d, s), from
    n uniform points per depth d of DEPTHS_COMPARED. sampleSplats(EMMLT) picks one of the depth's strategies uniformly and
    multiplies by their number (pathsampler.cpp:107-113, :296), so a point that drew another strategy contributes 0 to this one and
    the mean over ALL n points is the strategy's weighted share: the two factors cancel. Computed once a session, read-only."""
    if n not in _CACHE:
        sd = pkg.scenes.cornell_c2(RES)
        orc = ob.Oracle(pkg.abi, config(pkg), sd, 64)
        out = {}
        for d in DEPTHS_COMPARED:
            rng = np.random.default_rng(40 + d)
            us, ue = rng.random((n, 24), dtype=np.float32), rng.random((n, 24), dtype=np.float32)
            sp, st = orc.mmlt_eval(d, us, ue, rng.random(n, dtype=np.float32))
            assert (st.sum(axis=1) == d + 1).all()
            for s in range(d + 2):
                on = st[:, 0] == s
                rows = np.zeros((n, 10))                       # block_contributions' list rows, with a main splat only
                rows[:, 0], rows[:, 1] = sp["luminance"], on
                rows[:, 2], rows[:, 3], rows[:, 4:7] = sp["x"], sp["y"], sp["rgb"]
                c = rs.block_contributions(rows, RES)
                c.setflags(write=False)
                out[(d, s)] = c
        orc.close()
        _CACHE[n] = out
    return _CACHE[n]


def qualifying(contrib):
    """The strategies whose oracle side can be compared: at most 10 % of the blocks without variance."""
    return sorted(k for k, c in contrib.items() if (c.var(axis=0, ddof=1) == 0).mean() <= 0.1)
