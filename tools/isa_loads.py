#!/usr/bin/env python3
"""Global loads by width and vmcnt waits of ONE kernel, per region between two workgroup barriers.

    python tools/isa_loads.py <file.s> <kernel>

<file.s> is the gfx950 assembly hipcc keeps with -save-temps (tools/isa.sh); <kernel> is a substring of the kernel's mangled name,
e.g. rs_step_kernel_v64ILi896.  Region 0 runs from the kernel's entry to its first s_barrier, region k from barrier k to barrier
k + 1, in the order of the text.  The step kernel's tick loop is the three regions that end in the barriers of its loop body; the
regions are numbered, not named: read the loop's labels in the .s to tell them apart.  Columns: the region, its instructions,
global_load_{ubyte,sbyte,ushort,sshort,dword,dwordx2,dwordx3,dwordx4} and the s_waitcnt instructions that name vmcnt.
"""
import re
import sys

WIDTHS = ('ubyte', 'sbyte', 'ushort', 'sshort', 'dword', 'dwordx2', 'dwordx3', 'dwordx4')


def kernel_text(path, name):
    body, inside = [], False
    for line in open(path):
        if not inside:
            inside = re.match(r'^_Z\w*' + re.escape(name) + r'\w*:', line) is not None
            continue
        if line.startswith('.Lfunc_end'):
            return body
        code = line.split(';')[0].strip()
        if code and not code.endswith(':') and not code.startswith('.'):
            body.append(code)
    if not inside:
        raise SystemExit('no kernel matching %r in %s' % (name, path))
    return body


def regions(body):
    out = [dict(n=0, vmcnt=0, **{w: 0 for w in WIDTHS})]
    for code in body:
        op = code.split()[0]
        r = out[-1]
        r['n'] += 1
        if op == 's_barrier':
            out.append(dict(n=0, vmcnt=0, **{w: 0 for w in WIDTHS}))
        elif op.startswith('global_load_'):
            w = op[len('global_load_'):].split('_')[0]
            if w in r:
                r[w] += 1
        elif op == 's_waitcnt' and 'vmcnt' in code:
            r['vmcnt'] += 1
    return out


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    regs = regions(kernel_text(argv[1], argv[2]))
    cols = ('n',) + WIDTHS + ('vmcnt',)
    print('%-7s' % 'region' + ''.join('%9s' % c for c in ('insts',) + WIDTHS + ('vmcnt',)))
    for i, r in enumerate(regs):
        print('%-7d' % i + ''.join('%9d' % r[c] for c in cols))
    print('%-7s' % 'all' + ''.join('%9d' % sum(r[c] for r in regs) for c in cols))


if __name__ == '__main__':
    main(sys.argv)
