"""Are the kernels of two assembly files (hipcc -S --cuda-device-only, same flags, without -g) the same machine code? For every
kernel symbol of the first file: the instruction sequence from its label to s_endpgm, compared with the same symbol's of the second
file. Comments, directives and .loc lines are dropped, and local labels (.LBB<n>_<m>) are renumbered by order of appearance, so that
a kernel that moved within its file, or whose neighbours changed, still compares equal. A renamed kernel is given as old=new
(mangled symbols); kernels that moved to other translation units are looked up in all the new files given. Per kernel: `identical`;
`operands` -- equal once the two source operands of every commutative scalar instruction (s_and_b64 s[0:1], vcc, s[2:3]) are put in
one order, the same machine operation; or `DIFFERS` with the first differing instruction and the two instruction counts.
  python tools/isa_same.py parent.s new.s _Z11k_mutate_w27DParamsjj=_Z11k_mutate_w2ILb0EEv7DParamsjj
  python tools/isa_same.py parent/kernels.s kernels.s kernels_v3.s kernels_v4.s
Exit status 1 if some kernel DIFFERS or is missing; `operands` is the same machine code and leaves it 0."""
import re
import sys


def kernels(path):
    """{symbol: [instruction or label, ...]} of the file's kernels (.amdhsa_kernel names them)"""
    lines = open(path).read().split('\n')
    names = [m.group(1) for m in (re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l) for l in lines) if m]
    out = {}
    for sym in names:
        st = next(i for i, l in enumerate(lines) if l.startswith(sym + ':'))
        labels, body = {}, []
        for l in lines[st + 1:]:
            t = l.split(';', 1)[0].split('//', 1)[0].strip()
            if not t or (t.startswith('.') and not t.endswith(':')):
                continue  # comments, directives, .loc
            body.append(re.sub(r'\.LBB\d+_\d+', lambda m: labels.setdefault(m.group(0), '.L%d' % len(labels)), t))
            if t.startswith('s_endpgm'):
                break
        out[sym] = body
    return out


COMMUTATIVE = re.compile(r'(s_(?:and|or|xor|nand|nor|xnor)_b(?:32|64)|s_(?:add|min|max)_[iu]32|s_mul_i32)\s+([^,]+), ([^,]+), ([^,]+)$')


def ordered(body):
    """the body with the source operands of its commutative scalar instructions sorted"""
    return [COMMUTATIVE.sub(lambda m: '%s %s, %s, %s' % ((m.group(1), m.group(2)) + tuple(sorted(m.group(3, 4)))), t) for t in body]


if __name__ == '__main__':
    files = [a for a in sys.argv[1:] if '=' not in a]
    old, new = kernels(files[0]), {}
    for f in files[1:]:
        new.update(kernels(f))
    renamed = dict(a.split('=') for a in sys.argv[1:] if '=' in a)
    differ = 0
    for sym, a in old.items():
        b = new.get(renamed.get(sym, sym))
        name = sym if sym not in renamed else '%s -> %s' % (sym, renamed[sym])
        if b is None:
            differ += 1
            print('MISSING    %s' % name)
        elif a == b:
            print('identical  %s (%d)' % (name, len(a)))
        elif ordered(a) == ordered(b):
            print('operands   %s (%d): %d commutative scalar instructions with their sources exchanged' % (name, len(a), sum(x != y for x, y in zip(a, b))))
        else:
            differ += 1
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print('DIFFERS    %s: %d against %d instructions; first difference at %d: %r against %r'
                  % (name, len(a), len(b), i, a[i] if i < len(a) else None, b[i] if i < len(b) else None))
    for sym in sorted(set(new) - set(renamed.get(s, s) for s in old)):
        print('NEW        %s' % sym)
    sys.exit(1 if differ else 0)
