#!/usr/bin/env python3
"""Compare the gfx950 assembly of two builds of the library kernel by kernel (no GPU needed).

    hipcc <the flags of resco_amd/build.py> resco_amd/csrc/resco_sim.hip -o lib.so -save-temps     (once per build, in its own directory)
    tools/isa_compare.py A/resco_sim-hip-amdgcn-amd-amdhsa-gfx950.s B/resco_sim-hip-amdgcn-amd-amdhsa-gfx950.s

Both files are normalised (comment lines and trailing `; ...` comments, .ident / .file lines and the __hip_cuid_* symbol dropped, the
function number taken out of the local labels); then per kernel: the resource metadata, the number of instructions per opcode, and
the unified diff of the instruction streams.  Exit status 1 when a kernel's metadata or opcode counts differ."""
import collections
import difflib
import re
import subprocess
import sys

META = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size', '.sgpr_spill_count',
        '.vgpr_spill_count', '.max_flat_workgroup_size', '.kernarg_segment_size')


def normalise(path):
    out = []
    for line in open(path):
        line = line.split(';', 1)[0].rstrip()
        if not line.strip() or re.match(r'\s*\.(ident|file)\b', line) or '__hip_cuid_' in line:
            continue
        out.append(re.sub(r'\.L(BB|func_end|func_begin|tmp)\d+', r'.L\1', line))
    return out


def kernels(lines):
    """name -> (metadata dict, instruction lines)"""
    meta, body = {}, {}
    cur = None
    for ln in lines:
        m = re.match(r'(\w+):$', ln)
        if m and cur is None:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            if ln.startswith('.Lfunc_end'):
                cur = None
            elif ln.startswith('\t') and not ln.lstrip().startswith('.'):
                body[cur].append(ln.strip())
            elif re.match(r'\.L\w+:$', ln):
                body[cur].append(ln)
    blocks = '\n'.join(lines).split('\n  - ')
    for b in blocks[1:]:
        name = re.search(r'^\s*\.name:\s+(\S+)', b, re.M)
        if name:
            meta[name.group(1)] = {k: v for k, v in re.findall(r'^\s*(\.\w+):\s+(\S+)$', b, re.M) if k in META}
    missing = [k for k in meta if not body.get(k)]
    if missing:
        raise SystemExit('no instructions found for %s: the label style of the assembly is not the one this script parses' % ', '.join(missing))
    return {k: (meta[k], body[k]) for k in meta}


def main(a_path, b_path):
    A, B = kernels(normalise(a_path)), kernels(normalise(b_path))
    names = sorted(set(A) | set(B))
    demangled = dict(zip(names, subprocess.run(['c++filt'] + names, capture_output=True, text=True).stdout.split('\n')))
    bad = 0
    for k in names:
        if k not in A or k not in B:
            print('%s: only in %s' % (demangled[k], 'A' if k in A else 'B'))
            bad += 1
            continue
        (ma, ia), (mb, ib) = A[k], B[k]
        ops_a, ops_b = (collections.Counter(i.split()[0] for i in x if not i.endswith(':')) for x in (ia, ib))
        diff = list(difflib.unified_diff(ia, ib, 'A', 'B', lineterm='', n=2))
        verdict = 'IDENTICAL' if not diff else ('same metadata, same opcode counts, %d diff lines' % len(diff) if ma == mb and ops_a == ops_b else 'DIFFERENT')
        print('%s: %d / %d instructions, vgpr %s sgpr %s scratch %s spills s%s v%s: %s' % (
            demangled[k], sum(ops_a.values()), sum(ops_b.values()), mb.get('.vgpr_count'), mb.get('.sgpr_count'), mb.get('.private_segment_fixed_size'),
            mb.get('.sgpr_spill_count'), mb.get('.vgpr_spill_count'), verdict))
        if ma != mb:
            bad += 1
            print('    metadata A %s\n    metadata B %s' % (ma, mb))
        if ops_a != ops_b:
            bad += 1
            print('    opcode counts that differ (A, B): %s' % {o: (ops_a[o], ops_b[o]) for o in sorted(set(ops_a) | set(ops_b)) if ops_a[o] != ops_b[o]})
        for d in diff:
            print('    ' + d)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
