#!/usr/bin/env python3
"""What the compiler makes of the trip loops of the molecule-row pair kernels (csrc/cluster.hip: k_cpair / cwalk_rows).

    python scripts/trip_loop_isa.py [--label TEXT] [--asm FILE | --src atomsmm_amd/csrc/cluster.hip] [--all]

compiles cluster.hip to gfx950 assembly (hipcc -S, device side only, the flags of atomsmm_amd/build.py) -- or reads an assembly
file made that way -- and prints, for the k_cpair instantiations the bench and its legs launch (--all: every instantiation, one
line each), the kernel's VGPRs, SGPRs and private_seg_size from its metadata and, per image variant of the trip loop,

    VALU     instructions of one trip whose mnemonic begins with v_
    lane     v_readlane_b32 + v_writelane_b32 among them (scalar values parked in lanes of a VGPR: reloads and stores)

How a trip loop is found: a loop is a label and a later line that jumps back to it; the trip loops are the first three loops of a
kernel's text that hold at least MIN_VALU vector instructions and no other such loop (the walks come first; the loops of the
epilogue follow).  Inside a trip loop, a stretch that a forward jump skips and that holds COLD_VALU vector instructions or more is
the analytic redo of pairs below the tables (one per partner atom, behind a wave-uniform branch: never taken in a liquid; the
guest's block, which a back trip skips the same way, holds fewer: 86); such stretches are counted apart ("cold").  A kernel walks
its rows in three variants -- no periodic image (interior), one image per molecule pair, minimum image per atom pair -- which
differ by the rounding instructions of the image: the variants are told apart by their VALU count (fewest = interior, most = per
atom pair).  The script counts mnemonics by prefix and reads the metadata; it knows no other instruction.

The table of the parent commit and of this one is kept in profiles/trip_loop_isa.txt."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_VALU = 250
COLD_VALU = 100
VARIANTS = ('interior', 'image/molecule', 'image/pair')
# <FAM, CMODE, GFAM, BS, SMASK, EPI, GUNIT> of the launches of bench.py (C3 headline, its PME variant, the C5 leg): FAM 2 = near force
# with force switch, 3 = damped, 4 = NonbondedForce (CMODE 1: Ewald direct space); GFAM 2: the near force rides along; -1: one force;
# GUNIT: the guest's factor relative to the host is exactly 1.0 and the product by it is left out (what RESPASystem builds)
BENCH = [
    ((3, 1, 2, 512, 1, True, True), 'fused pass, damped host + near guest, epilogue (C3 step boundary)'),
    ((2, 0, -1, 512, 1, True, False), 'near pass, epilogue (C3 middle evaluation)'),
    ((3, 1, 2, 512, 1, False, True), 'fused pass without epilogue (C5 molecule rows)'),
    ((2, 0, -1, 512, 1, False, False), 'near pass without epilogue (C5 molecule rows)'),
    ((4, 1, 2, 512, 1, False, False), 'fused pass, Ewald direct host + near guest (PME variant)'),
    ((3, 1, 2, 512, 1, True, False), 'fused pass with epilogue for a guest factor other than 1.0 (not launched by the bench)'),
    ((3, 1, 2, 512, 1, False, False), 'fused pass without epilogue for a guest factor other than 1.0 (not launched by the bench)'),
]


def demangle_args(sym):
    """_Z7k_cpairILi3ELi1ELi2ELi512ELi1ELb1ELb0EE... -> (3, 1, 2, 512, 1, True, False), or None (an assembly file of a build from
    before the GUNIT flag has six arguments: the seventh is taken as False)."""
    m = re.match(r'_Z7k_cpairI((?:L[ib]n?\d+E)+)E', sym)
    if not m:
        return None
    out = []
    for kind, neg, val in re.findall(r'L([ib])(n?)(\d+)E', m.group(1)):
        v = -int(val) if neg else int(val)
        out.append(bool(v) if kind == 'b' else v)
    if len(out) == 6:
        out.append(False)
    return tuple(out)


def compile_asm(src):
    out = os.path.join(tempfile.mkdtemp(prefix='trip_loop_isa_'), 'cluster.s')
    cmd = [os.environ.get('HIPCC', 'hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only', src, '-o', out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return out


def kernels(lines):
    """-> {symbol: (first line, last line)} of the k_cpair kernels' bodies."""
    out = {}
    sym = None
    for i, line in enumerate(lines):
        m = re.match(r'(_Z7k_cpairI\w+):', line)
        if m:
            sym, start = m.group(1), i
        elif sym and line.startswith('.Lfunc_end'):
            out[sym] = (start, i)
            sym = None
    return out


def metadata(lines):
    """-> {symbol: dict(vgpr, sgpr, scratch, kernarg)} from the amdhsa metadata at the end of the file."""
    out = {}
    cur = {}
    for line in lines:
        m = re.match(r'\s+\.(kernarg_segment_size|private_segment_fixed_size|sgpr_count|vgpr_count|name):\s+(\S+)', line)
        if m:
            cur[m.group(1)] = m.group(2)
        m = re.match(r'\s+\.symbol:\s+(\S+)\.kd', line)
        if m:
            cur['symbol'] = m.group(1)
        if 'symbol' in cur and all(k in cur for k in ('kernarg_segment_size', 'private_segment_fixed_size', 'sgpr_count', 'vgpr_count')) \
                and re.match(r'\s+\.(wavefront_size|workgroup_processor_mode|uses_dynamic_stack):', line):
            out[cur['symbol']] = dict(vgpr=int(cur['vgpr_count']), sgpr=int(cur['sgpr_count']), scratch=int(cur['private_segment_fixed_size']),
                                      kernarg=int(cur['kernarg_segment_size']))
            cur = {}
    return out


def mnemonic(line):
    s = line.split(';')[0].strip()
    if not s or s.startswith('.') or s.endswith(':'):
        return None
    return s.split()[0]


def loops_of(lines, lo, hi):
    """Loops of lines[lo:hi] as (label line, jump line): a jump to a label defined above it."""
    label_at = {}
    out = []
    for i in range(lo, hi):
        m = re.match(r'(\.LBB\d+_\d+):', lines[i])
        if m:
            label_at[m.group(1)] = i
            continue
        m = re.search(r'\s(\.LBB\d+_\d+)\s*(;.*)?$', lines[i])
        if m and m.group(1) in label_at and mnemonic(lines[i]):
            out.append((label_at[m.group(1)], i))
    # one loop per label: its farthest jump back
    best = {}
    for a, b in out:
        best[a] = max(best.get(a, b), b)
    return sorted(best.items())


def count(lines, spans):
    valu = lane = 0
    for a, b in spans:
        for i in range(a, b + 1):
            mn = mnemonic(lines[i])
            if mn and mn.startswith('v_'):
                valu += 1
                if mn in ('v_readlane_b32', 'v_writelane_b32'):
                    lane += 1
    return valu, lane


def subtract(span, holes):
    """span minus the (disjoint, sorted) holes inside it -> list of spans."""
    out = []
    at = span[0]
    for a, b in holes:
        if a > at:
            out.append((at, a - 1))
        at = b + 1
    if at <= span[1]:
        out.append((at, span[1]))
    return out


def cold_regions(lines, span):
    """Stretches of a loop that a forward jump skips and that hold at least COLD_VALU vector instructions (the outermost such)."""
    label_at = {}
    for i in range(span[0], span[1] + 1):
        m = re.match(r'(\.LBB\d+_\d+):', lines[i])
        if m:
            label_at[m.group(1)] = i
    found = []
    for i in range(span[0], span[1] + 1):
        m = re.search(r'\s(\.LBB\d+_\d+)\s*(;.*)?$', lines[i])
        if m and mnemonic(lines[i]) and label_at.get(m.group(1), -1) > i:
            r = (i + 1, label_at[m.group(1)] - 1)
            if count(lines, [r])[0] >= COLD_VALU:
                found.append(r)
    out = []
    for r in sorted(found):
        if not out or r[0] > out[-1][1]:
            out.append(r)
    return out


def trip_loops(lines, lo, hi):
    """-> [(VALU, lane, cold VALU, cold lane)] of the kernel's trip loops, sorted by VALU."""
    loops = loops_of(lines, lo, hi)
    big = [l for l in loops if count(lines, [l])[0] >= MIN_VALU]
    leaves = [l for l in big if not any(o != l and l[0] <= o[0] and o[1] <= l[1] for o in big)]
    out = []
    for l in sorted(leaves)[:3]:          # (the walks come first in the kernel's text; behind them: the loops of the epilogue)
        cold = cold_regions(lines, l)
        hot = count(lines, subtract(l, cold))
        out.append(hot + count(lines, cold))
    return sorted(out)


def report(lines, label, want_all):
    ks = kernels(lines)
    md = metadata(lines)
    by_args = {demangle_args(s): s for s in ks}
    print('== %s: %d k_cpair instantiations' % (label, len(ks)))
    rows = BENCH if not want_all else [(a, '') for a in sorted(by_args, key=str)]
    print('%-36s %5s %5s %8s %8s   %s' % ('k_cpair<FAM,CMODE,GFAM,BS,SMASK,EPI,GUNIT>', 'VGPR', 'SGPR', 'scratch', 'kernarg',
                                           'per trip: VALU / lane moves (+ cold: analytic redo)'))
    for args, what in rows:
        sym = by_args.get(args)
        if sym is None:
            print('%-36s not in this build' % (args,))
            continue
        m = md.get(sym, dict(vgpr=-1, sgpr=-1, scratch=-1, kernarg=-1))
        trips = trip_loops(lines, *ks[sym])
        name = '<%s>' % ', '.join(str(a).lower() if isinstance(a, bool) else str(a) for a in args)
        cells = []
        for k, (valu, lane, cvalu, clane) in enumerate(trips):
            tag = VARIANTS[k] if len(trips) == 3 else 'loop %d' % k
            cells.append('%s %d / %d (+ %d / %d)' % (tag, valu, lane, cvalu, clane))
        print('%-36s %5d %5d %8d %8d   %s' % (name, m['vgpr'], m['sgpr'], m['scratch'], m['kernarg'], ' | '.join(cells)))
        if what:
            print('%-36s %s' % ('', what))
    worst = max((md[s]['vgpr'] for s in ks if s in md), default=-1)
    print('largest VGPR count of all instantiations: %d; with scratch: %d of %d; total scratch bytes %d' % (
        worst, sum(1 for s in ks if md.get(s, {}).get('scratch', 0) > 0), len(ks), sum(md.get(s, {}).get('scratch', 0) for s in ks)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm', default=None, help='an assembly file made by hipcc -S --cuda-device-only (default: compile --src)')
    ap.add_argument('--src', default=os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'cluster.hip'))
    ap.add_argument('--label', default=None)
    ap.add_argument('--all', action='store_true', help='one line per instantiation')
    a = ap.parse_args()
    path = a.asm or compile_asm(a.src)
    with open(path) as fh:
        text = fh.read().split('\n')
    report(text, a.label or os.path.basename(path), a.all)
    sys.exit(0)
