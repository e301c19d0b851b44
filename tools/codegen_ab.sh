#!/bin/bash
# A/B of library builds that differ in code-generation flags (on the GPU box): build them first, e.g.
#   cd drmlt-mitsuba_amd/csrc && make -B OUT=../variants/libD.so DEVFLAGS="<the Makefile's DEVFLAGS> -mllvm -amdgpu-sched-strategy=max-ilp"
# (drmlt-mitsuba_amd/variants/ is git-ignored; DRMLT_LIBRARY makes the binding load another build of the same ABI).
# k_mutate_w2's ingredient switches (kernels.hip) are source switches, built the same way through CXXFLAGS, e.g.
#   make -B OUT=../variants/libH.so CXXFLAGS="<the Makefile's CXXFLAGS> -DW2_NO_HELD_CONSTANTS"   (likewise -DW2_SCALARS_LOADED, -DW2_TWO_PHILOX,
#   -DW2_MASKED_STEP, -DW2_COPIED_HANDOFF, -DW2_MASKED_TRACE, -DW2_SHARED_FLUSH: the film flush through v4_flush, as the twin)
# and run with VARIANTS="A H ..." here or in codegen_ab_bench.sh (config 2). Nothing else builds them: after an edit to k_mutate_w2,
# build all seven once (no spill in any) and run tests/test_gpu_w2.py, tests/test_gpu_w2_step.py and
# tests/test_gpu_w2_flush.py under DRMLT_LIBRARY.
# k_mutate_w2h (the ray records held in registers) against k_mutate_w2 needs no second build: DRMLT_NO_W2_HELD=1 is a run-time
# knob of the same library (launch_plan.h). The -DW2_* switches above are k_mutate_w2's alone; k_mutate_w2h has two of its own,
# built the same way: -DW2H_BRANCHED_DECIDE (the decide through mh_decide and its arms, as k_mutate_w2) and -DW2H_EMITTER_HIT_ALWAYS
# (the step's emitter-hit block in every iteration). The second spills four scalar registers: a build to be measured, not shipped.
# Round 2: -amdgpu-early-ifcvt, -amdgpu-sched-strategy=max-ilp and raised SimplifyCFG phi-folding thresholds all stay within
# +-1 % of the default build on config 2, config 3 and the soup.
for v in ${VARIANTS:-A B D E}; do
  if [ $v = A ]; then unset DRMLT_LIBRARY; else export DRMLT_LIBRARY=$GRAFT_REPO_ROOT/drmlt-mitsuba_amd/variants/lib$v.so; fi
  for sc in "cornell_c2 orbital" "door_c3 green" "triangle_soup orbital"; do set -- $sc
    r=$(SCENE=$1 TYPE=$2 SPP=1280 REPS=3 python tools/perf_ab.py 0 2>/dev/null | grep variant | cut -c1-60)
    echo "$v $1 $r"
  done
done
