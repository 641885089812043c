#!/usr/bin/env python
"""Compares the gfx950 device code of two versions of lcgp_hip.hip kernel by kernel (no GPU needed).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC --cuda-device-only -S -o old.s <old lcgp_hip.hip>
    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC --cuda-device-only -S -o new.s lcgp_amd/csrc/lcgp_hip.hip
    python tools/codeobj_diff.py old.s new.s

A host-only change may reorder the template instantiations, so the files are not compared as text: every function's
instruction stream and every kernel descriptor is compared under its symbol, with the function ordinal in local labels
(.LBB<ordinal>_<block>) removed.  Prints the kernel count and the symbols that were added, removed or changed; exit
status 1 if there are any."""
import re
import sys


def functions(path):
    """{symbol: normalised body} of the functions and {symbol: descriptor} of the kernels of an assembly file"""
    body, desc, cur, kern = {}, {}, None, None
    for line in open(path):
        m = re.match(r'\t\.type\t(\S+),@function', line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None and line.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None and not re.match(r'\s*(;|\.p2align|\.loc|\.file|\.cfi_)', line) and not line.startswith(cur + ':'):
            body[cur].append(re.sub(r'\.(LBB|Ltmp|LJTI|Lfunc_begin)\d+', r'.\1', line.split(';')[0].rstrip()))
        m = re.match(r'\s*\.amdhsa_kernel (\S+)', line)
        if m:
            kern = m.group(1)
            desc[kern] = []
        elif kern is not None and '.end_amdhsa_kernel' in line:
            kern = None
        elif kern is not None:
            desc[kern].append(line.strip())
    return body, desc


def main():
    (b0, d0), (b1, d1) = functions(sys.argv[1]), functions(sys.argv[2])
    print('kernels: %d -> %d, functions: %d -> %d' % (len(d0), len(d1), len(b0), len(b1)))
    gone, new = sorted(set(b0) - set(b1)), sorted(set(b1) - set(b0))
    changed = sorted(s for s in set(b0) & set(b1) if b0[s] != b1[s] or d0.get(s) != d1.get(s))
    for what, syms in (('removed', gone), ('added', new), ('changed', changed)):
        print('%s: %d' % (what, len(syms)))
        for s in syms:
            print('  ' + s)
    print('instructions compared: %d' % sum(len(b0[s]) for s in set(b0) & set(b1)))
    sys.exit(1 if gone or new or changed else 0)


if __name__ == '__main__':
    main()
