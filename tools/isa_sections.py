"""Static instruction count of one kernel by SECTIONS of its own source file, inlined callees included (asm from -S
-gline-tables-only): an instruction belongs to the line of the kernel's file at which the chain of inlined calls that produced it
starts -- the last `file:line` of the .loc comment -- so a routine of a header counts where the kernel calls it. isa_region.py and
isa_profile.py count by the innermost line instead: what a header routine costs, whoever calls it.
  python tools/isa_sections.py /tmp/k.s <mangled kernel> kernels_v4.hip bookkeeping=1049-1190 rays=1191-1198 step=1199-1240
Instructions of the kernel outside every section (and those without a line) are reported as `other`.
Per section it also reports `wait_vmcnt`, the s_waitcnt instructions that name vmcnt (loads, and on gfx9 no-return atomics and
stores, count there: such a wait parks the wave until they have completed), and `vmem_load`, the vector-memory loads
(flat_load*, global_load*)."""
import collections
import re
import sys

path, sym, fname = sys.argv[1], sys.argv[2], sys.argv[3]
sections = []
for a in sys.argv[4:]:
    name, rng = a.split('=')
    lo, hi = rng.split('-')
    sections.append((name, int(lo), int(hi)))
lines = open(path).read().split('\n')
st = next(i for i, l in enumerate(lines) if l.startswith(sym + ':'))
en = next(i for i in range(st, len(lines)) if 's_endpgm' in lines[i])
WATCH = ('v_mov_b32', 's_nop', 'v_permlane32_swap', 'saveexec', 'v_cndmask', 's_waitcnt', 'ds_', 's_load', 's_cbranch')
count, kinds = collections.Counter(), collections.defaultdict(collections.Counter)
cur = None
for l in lines[st:en]:
    if re.match(r'\s*\.loc\s', l):
        sites = re.findall(r'([\w.+-]+):(\d+):\d+', l.split(';', 1)[1] if ';' in l else '')
        if sites and int(sites[-1][1]) > 0:  # (line 0: compiler-made code, counted with what precedes it)
            cur = int(sites[-1][1]) if sites[-1][0] == fname else None
        continue
    t = l.strip()
    if not t or t.startswith(('.', ';', '//')) or t.endswith(':') or re.match(r'\.?\w+:', t):
        continue
    sec = next((n for n, lo, hi in sections if cur is not None and lo <= cur <= hi), 'other')
    count[sec] += 1
    op = t.split()[0]
    kinds[sec]['valu' if op.startswith('v_') else 'salu+smem' if op.startswith('s_') else 'lds' if op.startswith('ds_') else 'vmem'] += 1
    for w in WATCH:
        if w in op:
            kinds[sec][w] += 1
    if op == 's_waitcnt' and 'vmcnt' in t:
        kinds[sec]['wait_vmcnt'] += 1
    if op.startswith(('flat_load', 'global_load')):
        kinds[sec]['vmem_load'] += 1
print('total', sum(count.values()))
for name in [n for n, _, _ in sections] + ['other']:
    print('%-12s %5d  %s' % (name, count[name], dict(kinds[name])))
