"""Waits on the vector-memory counter and vector-memory loads of one kernel, by source-line ranges of one file (asm from -S
-gline-tables-only). An instruction belongs to the first range that holds ANY line of the chain of inlined calls that produced it
(the .loc directive's own line and the `@[ file:line:col ]` sites of its comment), so a range names a routine's own lines and
collects what the routine inlines as well, whichever kernel calls it; isa_sections.py reports the same two figures by the
kernel's call sites alone. Per range: instructions, `wait_vmcnt` (s_waitcnt that name vmcnt: loads, and on gfx9 no-return
atomics and stores, count there), `vmem_load` (flat_load*, global_load*), `vmem_atomic`, `lds` (ds_*).
  python tools/isa_waits.py /tmp/k.s k_mutate_w2 kernels_v4.hip passes=991-1015 staging=1016-1026
The kernel is named by its source name or its mangled symbol. tests/test_w2_flush_isa.py imports scan()."""
import collections
import re
import sys


def kernel_body(lines, kernel):
    """the lines of the kernel's symbol, up to its s_endpgm"""
    pat = re.compile(r'^(_Z\d+%s\w*|%s):' % (re.escape(kernel), re.escape(kernel)))
    st = next(i for i, l in enumerate(lines) if pat.match(l))
    en = next(i for i in range(st, len(lines)) if 's_endpgm' in lines[i])
    return lines[st:en]


def scan(asm_text, kernel, fname, ranges):
    """ranges: {name: (first line, last line)} of `fname`, in order of precedence. Returns {name: Counter}; every Counter also
    lists under 'where' the (innermost line, call-site line in the kernel, instruction) of its waits and loads."""
    lines = asm_text.split('\n')
    files = {}
    for l in lines:
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
        if m:
            files[m.group(1)] = (m.group(3) or m.group(2)).split('/')[-1]
    out = {name: collections.Counter() for name in ranges}
    where = {name: [] for name in ranges}
    chain = []
    for l in kernel_body(lines, kernel):
        m = re.match(r'\s*\.loc\s+(\d+)\s+(\d+)', l)
        if m:
            if int(m.group(2)) > 0:  # (line 0: compiler-made code, counted with what precedes it)
                chain = [(files.get(m.group(1)), int(m.group(2)))]
                if '@[' in l:
                    chain += [(f.split('/')[-1], int(n)) for f, n in re.findall(r'([^\s\[\]]+):(\d+):\d+', l.split('@[', 1)[1])]
            continue
        t = l.split(';', 1)[0].strip()
        if not t or t.startswith(('.', '//')) or t.endswith(':'):
            continue
        mine = [n for f, n in chain if f == fname]
        name = next((name for name, (lo, hi) in ranges.items() if any(lo <= n <= hi for n in mine)), None)
        if name is None:
            continue
        op = t.split()[0]
        c = out[name]
        c['instructions'] += 1
        if op == 's_waitcnt' and 'vmcnt' in t:
            c['wait_vmcnt'] += 1
            where[name].append((chain[0][1], mine[-1], t))
        elif op.startswith(('flat_load', 'global_load')):
            c['vmem_load'] += 1
            where[name].append((chain[0][1], mine[-1], t))
        elif op.startswith(('flat_atomic', 'global_atomic')):
            c['vmem_atomic'] += 1
        elif op.startswith('ds_'):
            c['lds'] += 1
    for name in ranges:
        out[name]['where'] = where[name]
    return out


if __name__ == '__main__':
    path, kernel, fname = sys.argv[1], sys.argv[2], sys.argv[3]
    ranges = {}
    for a in sys.argv[4:]:
        name, rng = a.split('=')
        lo, hi = rng.split('-')
        ranges[name] = (int(lo), int(hi))
    res = scan(open(path).read(), kernel, fname, ranges)
    for name in ranges:
        c = res[name]
        print('%-12s %5d  wait_vmcnt %d  vmem_load %d  vmem_atomic %d  lds %d' % (name, c['instructions'], c['wait_vmcnt'], c['vmem_load'],
                                                                                 c['vmem_atomic'], c['lds']))
        for line, site, t in c['where']:
            print('    line %d (called from line %d): %s' % (line, site, t))
