#!/usr/bin/env python3
"""Scalar loads from the constant argument block (StepArgs) of ONE step kernel, per region between two workgroup barriers, named.

    python tools/isa_sloads.py <file.s> <kernel> [--check]

<file.s> is the gfx950 assembly hipcc keeps with -save-temps (tools/isa_map.sh, tools/isa.sh); <kernel> is a substring of the kernel's
mangled name, e.g. rs_step_kernel_v64ILi896 or rs_step_kernel_fix_v64I20ScnFix_ingolstadt21.  Regions as in tools/isa_loads.py; the
tick loop (P, C, M) is taken to be the largest region and the two that follow it, and is marked with `*`.

Every s_load whose base is the kernel's first argument (the pointer to StepArgs; register copies are followed) is named by the
member(s) of StepArgs its offset and width cover -- the layout comes from the host-only library of the build (rs_step_args_layout) --
and falls into one of three classes:
  const    a value fixed for the handle: a scalar of KTab or any member of the Lds table (offsets, gstride, lcap, cell_inv)
  pointer  a table pointer of KTab / KCold, a pointer of State / Out
  state    State.nc and the dimensions of Out (they follow from the number of environments)
An s_load from another base (a table read with a uniform index, a re-loaded copy of the argument pointer the tool could not follow) is
counted as `other`.  Columns per region: instructions, SALU instructions (s_* that are neither loads, waits, barriers, branches nor
nops), s_waitcnt with lgkmcnt(0), s_load in all, const / pointer / state / other, and the const loads by member.
--check: exit with status 1 if a `const` load is left in the tick loop (what a per-map kernel must not have).
"""
import collections
import ctypes
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.isa_loads import kernel_text  # noqa: E402

WIDTH = {'s_load_dword': 4, 's_load_dwordx2': 8, 's_load_dwordx3': 12, 's_load_dwordx4': 16, 's_load_dwordx8': 32, 's_load_dwordx16': 64}
NOT_SALU = ('s_load', 's_waitcnt', 's_barrier', 's_nop', 's_branch', 's_cbranch', 's_endpgm', 's_sleep', 's_setprio', 's_buffer_load')


def layout():
    """[(name, class, offset, bytes)] of StepArgs"""
    from resco_amd.build import build_scn_consts_library
    L = ctypes.CDLL(build_scn_consts_library())
    L.rs_step_args_layout.restype = ctypes.c_char_p
    out = []
    for item in L.rs_step_args_layout().decode().strip(',').split(','):
        name, cls, off, size = item.split(':')
        out.append((name, cls, int(off), int(size)))
    return out


def pair(reg):
    m = re.fullmatch(r's\[(\d+):(\d+)\]', reg)
    return (int(m.group(1)), int(m.group(2))) if m else None


def analyse(body, lay):
    regions = [collections.Counter()]
    members = [collections.Counter()]
    base = set()
    for code in body:
        ops = [o.strip() for o in code.replace(',', ' ').split()]
        op, r, mem = ops[0], regions[-1], members[-1]
        r['insts'] += 1
        if op == 's_barrier':
            regions.append(collections.Counter())
            members.append(collections.Counter())
            continue
        if op == 's_mov_b64' and pair(ops[2]) in base:
            base.add(pair(ops[1]))
        elif op == 's_mov_b64' and pair(ops[1]) in base:
            base.discard(pair(ops[1]))
        if op in WIDTH:
            r['s_load'] += 1
            dst, src = ops[1], pair(ops[2])
            off = int(ops[3], 0) if len(ops) > 3 and re.fullmatch(r'(0x[0-9a-fA-F]+|\d+)', ops[3]) else None
            if not base and off == 0 and op == 's_load_dwordx2':      # the first argument of the kernel: the pointer to StepArgs
                base.add(pair(dst))
                continue
            if src in base and off is not None:
                hit = [(n, c) for n, c, o, s in lay if o < off + WIDTH[op] and off < o + s]
                classes = {c for _, c in hit}
                cls = 'const' if 'const' in classes else ('pointer' if 'pointer' in classes else ('state' if hit else 'other'))
                r[cls] += 1
                if cls == 'const':
                    for n, c in hit:
                        if c == 'const':
                            mem[n] += 1
            else:
                r['other'] += 1
            d = pair(dst)
            if d in base:
                base.discard(d)
        elif op == 's_waitcnt' and 'lgkmcnt(0)' in code:
            r['lgkm0'] += 1
        elif op.startswith('s_') and not op.startswith(NOT_SALU):
            r['salu'] += 1
    return regions, members


def main(argv):
    check = '--check' in argv
    argv = [a for a in argv if a != '--check']
    if len(argv) != 3:
        raise SystemExit(__doc__)
    regions, members = analyse(kernel_text(argv[1], argv[2]), layout())
    big = max(range(len(regions)), key=lambda i: regions[i]['insts'])
    tick = [i for i in (big, big + 1, big + 2) if i < len(regions)]
    cols = ('insts', 'salu', 'lgkm0', 's_load', 'const', 'pointer', 'state', 'other')
    print('%-8s' % 'region' + ''.join('%9s' % c for c in cols) + '  const loads by member')
    for i, r in enumerate(regions):
        print('%-8s' % ('%d%s' % (i, '*' if i in tick else '')) + ''.join('%9d' % r[c] for c in cols) + '  ' +
              ' '.join('%s:%d' % kv for kv in sorted(members[i].items(), key=lambda kv: -kv[1])))
    tot = collections.Counter()
    mem = collections.Counter()
    for i in tick:
        tot.update(regions[i])
        mem.update(members[i])
    print('%-8s' % 'tick' + ''.join('%9d' % tot[c] for c in cols) + '  ' + ' '.join('%s:%d' % kv for kv in sorted(mem.items(), key=lambda kv: -kv[1])))
    if check and tot['const']:
        raise SystemExit('%d loads of handle constants left in the tick loop' % tot['const'])


if __name__ == '__main__':
    main(sys.argv)
