#!/usr/bin/env python3
"""What the compiler makes of the list build's kernels (csrc/cluster.hip: k_cbuild), and how much of a wavefront's text runs before
its first batch of row molecules.

    python scripts/build_tables_isa.py [--label TEXT] [--asm FILE | --src atomsmm_amd/csrc/cluster.hip]

compiles cluster.hip to gfx950 assembly (as scripts/trip_loop_isa.py does, whose parsing this script reuses) -- or reads an assembly
file made that way -- and prints, for every k_cbuild<COUNT_ONLY, RINT, SLICE> instantiation, VGPRs, SGPRs, scratch and LDS bytes from
the kernel's metadata and

    setup    instructions between the kernel's entry (SLICE: the head of the loop over the slice's units) and the head of the batch
             loop: the early return, the unit's bounds and whatever prepares the stencil tables of the cell
    LDS ops  ds_* instructions among them
    waits    s_waitcnt among them
    whole    instructions of the whole kernel

The batch loop is found by the compiler's own loop annotations (setup_span).  The script counts lines with a mnemonic; it knows no
instruction.

The table of the parent commit and of this one is kept in profiles/build_tables_isa.txt."""
import argparse
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location('trip_loop_isa', os.path.join(ROOT, 'scripts', 'trip_loop_isa.py'))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)


def kernels(lines):
    """-> {symbol: (first line, last line)} of the k_cbuild kernels' bodies (not k_cbuild_split: 14 characters)."""
    out = {}
    sym = None
    for i, line in enumerate(lines):
        m = re.match(r'(_Z8k_cbuildI\w+):', line)
        if m:
            sym, start = m.group(1), i
        elif sym and line.startswith('.Lfunc_end'):
            out[sym] = (start, i)
            sym = None
    return out


def template_args(sym):
    return tuple(bool(int(v)) for v in re.findall(r'Lb(\d)E', re.match(r'_Z8k_cbuildI((?:Lb\dE)+)E', sym).group(1)))


def lds_bytes(lines):
    """-> {symbol: group_segment_fixed_size}."""
    out = {}
    size = None
    for line in lines:
        m = re.match(r'\s+\.group_segment_fixed_size:\s+(\d+)', line)
        if m:
            size = int(m.group(1))
        m = re.match(r'\s+\.symbol:\s+(\S+)\.kd', line)
        if m and size is not None:
            out[m.group(1)] = size
            size = None
    return out


def tally(lines, a, b):
    n = lds = waits = 0
    for i in range(a, b):
        mn = T.mnemonic(lines[i])
        if mn:
            n += 1
            lds += mn.startswith('ds_')
            waits += mn == 's_waitcnt'
    return n, lds, waits


def setup_span(lines, lo, hi, slice_):
    """The compiler marks every loop head with its depth and, if it has any, its child loops.  The batch loop is the first loop with
    children at depth 1 (SLICE: at depth 2, inside the loop over units, where the count starts)."""
    heads = []
    for i in range(lo, hi):
        m = re.search(r'; =>\s*This Loop Header: Depth=(\d+)', lines[i])          # (a nested head: its label stands some comment lines above)
        if m and 'Child Loop' in lines[i + 1]:
            heads.append((int(m.group(1)), i))
    if not slice_:
        return lo, next(i for d, i in heads if d == 1)
    return next(i for d, i in heads if d == 1), next(i for d, i in heads if d == 2)


def report(lines, label):
    ks = kernels(lines)
    md = T.metadata(lines)
    lds = lds_bytes(lines)
    print('== %s: %d k_cbuild instantiations' % (label, len(ks)))
    print('%-36s %5s %5s %8s %6s   %6s %8s %6s %7s' % ('k_cbuild<COUNT_ONLY, RINT, SLICE>', 'VGPR', 'SGPR', 'scratch', 'LDS', 'setup', 'LDS ops', 'waits', 'whole'))
    for sym in sorted(ks, key=template_args):
        args = template_args(sym)
        lo, hi = ks[sym]
        a, b = setup_span(lines, lo, hi, args[2])
        n, nlds, nwait = tally(lines, a, b)
        m = md[sym]
        print('%-36s %5d %5d %8d %6d   %6d %8d %6d %7d' % ('<%s>' % ', '.join(str(v).lower() for v in args), m['vgpr'], m['sgpr'], m['scratch'],
                                                         lds[sym], n, nlds, nwait, tally(lines, lo, hi)[0]))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm', default=None, help='an assembly file made by hipcc -S --cuda-device-only (default: compile --src)')
    ap.add_argument('--src', default=os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'cluster.hip'))
    ap.add_argument('--label', default=None)
    a = ap.parse_args()
    path = a.asm or T.compile_asm(a.src)
    with open(path) as fh:
        text = fh.read().split('\n')
    report(text, a.label or os.path.basename(path))
    sys.exit(0)
