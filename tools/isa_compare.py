#!/usr/bin/env python3
"""Compare the gfx950 device assembly of one unit before and after a host-side refactor, kernel by kernel.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 --offload-device-only -S unit.hip -o unit.s     (once per tree)
  tools/isa_compare.py old/unit.s new/unit.s

A whole-file diff is too strict for this purpose: the order in which the compiler emits template instantiations (rocPRIM's
kernels) follows the order of their first use in the source, and the number of a function is part of its local labels
(.LBB<function>_<block>) and of the comments that name them.  So the text is cut into functions and kernel descriptors by
symbol name, comments and the function number in local labels are taken out, and the two sets are compared by name: instructions, register counts, LDS and scratch sizes
(.amdhsa_* directives and the metadata entry of every kernel).  Lines that carry only the source file name, the compiler
ident or the compilation-unit id (a hash of the source text) are dropped.  Exit status 0 = identical.
"""
import re
import sys


def parse(path):
    funcs, descs, meta = {}, {}, {}
    cur = None
    lines = open(path, errors='replace').read().split('\n')
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r'^([A-Za-z_$][\w$.]*):\s*(;.*)?$', ln)
        if cur is None and m and not m.group(1).startswith('.L') and not m.group(1).startswith('__hip_cuid'):
            cur = m.group(1)
            funcs[cur] = []
        elif cur is not None and (re.match(r'^\.Lfunc_end\d+:', ln) or re.match(r'^\s*\.size\s+' + re.escape(cur) + ',', ln)):
            cur = None
        elif cur is not None:
            s = re.sub(r'\.LBB\d+_', '.LBB_', ln.split(';')[0].rstrip())      # (comments repeat the function number)
            s = re.sub(r'\.L(func_begin|func_end|tmp)\d+', r'.L\1', s)
            if s.strip() and not re.match(r'^\s*(\.file|\.loc|\.ident|\.cfi)', s):
                funcs[cur].append(' '.join(s.split()))
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m:
            name, body = m.group(1), []
            i += 1
            while not lines[i].strip().startswith('.end_amdhsa_kernel'):
                body.append(lines[i].strip())
                i += 1
            descs[name] = body
        m = re.match(r'^\s*-\s+\.agpr_count:', ln) or re.match(r'^\s*-\s+\.args:', ln)
        if m:      # one kernel's metadata entry: up to the next entry or the end of the list
            body = [ln.strip().lstrip('- ')]
            i += 1
            while i < len(lines) and not re.match(r'^\s*-\s+\.(agpr_count|args):', lines[i]) and not lines[i].startswith('amdhsa.target'):
                body.append(lines[i].strip())
                i += 1
            name = next((b.split(':', 1)[1].strip() for b in body if b.startswith('.name:')), None)
            meta[name] = body
            continue
        i += 1
    return funcs, descs, meta


def main():
    old, new = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    for what, a, b in zip(('function', 'kernel descriptor', 'metadata'), old, new):
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                print(f'{what} only in {"new" if name in b else "old"}: {name}')
                bad += 1
            elif a[name] != b[name]:
                print(f'{what} differs: {name}')
                bad += 1
    print(f'{len(old[0])} functions, {len(old[1])} kernels compared: ' + ('identical' if bad == 0 else f'{bad} differences'))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
