#!/usr/bin/env python3
"""What the compiler makes of the loops of the list build (csrc/cluster.hip: k_cbuild): the vector instructions a wavefront spends its
life in, and how many of them only keep books.

    python scripts/build_loops_isa.py [--label TEXT] [--asm FILE | --src atomsmm_amd/csrc/cluster.hip [--whole]]

compiles cluster.hip to gfx950 assembly (as scripts/trip_loop_isa.py does, whose compile and parsing this script reuses, like
scripts/build_tables_isa.py) -- or reads an assembly file made that way -- and prints, for every k_cbuild<COUNT_ONLY, RINT, SLICE>
instantiation, VGPRs, SGPRs, scratch and LDS bytes, SGPR and VGPR spills, the instructions and the text bytes of the whole kernel, and
the vector instructions (mnemonics that begin with v_) of these spans:

    test        the sphere test of a row molecule against one chunk pair of 128 candidates, filing of the hits included: of all the
                copies the kernel holds (1 row = a loop over the batch's rows, 5 = unrolled over the batch) and per row
    chunk       what a chunk pair costs whatever the batch: head of the chunk loop, the fetch of the next 128 candidates (one trip of
                each piece walk counted), the tail
    drain 128   the packed drain of a full ring inside the chunk loop (two survivors per lane), with what parks its results
    final 2/1   the drains of a row's leftover after the stream: packed (more than 64 survivors) and one survivor per lane

each split into  lane (v_readlane / v_writelane) + mov (v_mov) + sel (v_cndmask, v_cmp) + arithmetic (the rest).

How the spans are found: the compiler marks every block with the loop it belongs to ("in Loop: Header=... Depth=d") and every loop head
with its depth.  The chunk loop is the first loop with child loops inside the batch loop (the batch loop: first loop with children at
depth 1; SLICE: at depth 2, inside the loop over units); its first two children are the fetch's piece walks.  If its third child
files hits (ds_write_b32) it is the loop over the batch's rows: the test runs from its head to the wave barrier that precedes the
drain, the rest of it is the drain.  Otherwise the third child is the loop over the pending rows = the drain, and the tests are the
chunk loop's own blocks from the first packed instruction to the wave barrier.  The loop that follows the chunk loop in the batch loop
holds the final drains; the packed form is told from the other by its v_pk_ instructions.  The script counts mnemonics by prefix and
reads the metadata; it knows no other instruction.

The table of the parent commit and of this one is kept in profiles/build_loops_isa.txt; tests/test_build_loops_isa.py holds the
committed kernel to it."""
import argparse
import importlib.util
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load('trip_loop_isa')
B = _load('build_tables_isa')
KINDS = ('lane', 'mov', 'sel', 'arith')


def kind(mn):
    if mn in ('v_readlane_b32', 'v_writelane_b32'):
        return 'lane'
    if mn.startswith('v_mov_'):
        return 'mov'
    if mn.startswith('v_cndmask') or mn.startswith('v_cmp'):
        return 'sel'
    return 'arith'


def spills(lines):
    """-> {symbol: (sgpr_spill_count, vgpr_spill_count)} from the metadata."""
    out = {}
    cur = {}
    for line in lines:
        m = re.match(r'    \.(sgpr_spill_count|vgpr_spill_count|symbol):\s+(\S+)', line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1) == 'vgpr_spill_count':          # (the last of the three in a kernel's record)
            out[cur['symbol'][:-3]] = (int(cur['sgpr_spill_count']), int(cur['vgpr_spill_count']))
            cur = {}
    return out


def text_bytes(lines, hi):
    for i in range(hi, min(hi + 40, len(lines))):
        m = re.match(r'; codeLenInByte = (\d+)', lines[i])
        if m:
            return int(m.group(1))
    return -1


def blocks(lines, lo, hi):
    """-> [(first line, last line, innermost loop head label or None)] of a kernel's basic blocks, in text order, and
    {head label: (depth, line)}."""
    out = []
    heads = {}
    start, tag = lo, None
    for i in range(lo, hi):
        m = re.match(r'(?:(\.LBB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$', lines[i])
        if not m:
            continue
        if i > start:
            out.append((start, i - 1, tag))
        start = i
        label, note, tag = m.group(1), m.group(2) or '', None
        for j in range(i, min(i + 12, hi)):           # the loop notes of a head run over the comment lines that follow its label
            text = lines[j] if j > i else note
            if j > i and not lines[j].startswith(' ' * 30):
                break
            mm = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', text)
            if mm:
                tag = '.L' + mm.group(1)
            mm = re.search(r'=>\s*This (?:Inner )?Loop Header: Depth=(\d+)', text)
            if mm and label:
                tag = label
                heads[label] = (int(mm.group(1)), i)
    out.append((start, hi - 1, tag))
    return out, heads


def tally(lines, spans):
    c = dict.fromkeys(KINDS, 0)
    for a, b in spans:
        for i in range(a, b + 1):
            mn = T.mnemonic(lines[i])
            if mn and mn.startswith('v_'):
                c[kind(mn)] += 1
    return c


def first_line(lines, spans, needle):
    for a, b in spans:
        for i in range(a, b + 1):
            if needle in lines[i]:
                return i
    return None


def cut(spans, at, before):
    """The part of the (text-ordered) spans before / from line `at`."""
    out = []
    for a, b in spans:
        if before and a < at:
            out.append((a, min(b, at - 1)))
        if not before and b >= at:
            out.append((max(a, at), b))
    return out


def loop_spans(lines, lo, hi, slice_):
    """-> dict(rows, test, chunk, drain, final2, final1): lists of (first line, last line)."""
    blks, heads = blocks(lines, lo, hi)
    own = lambda h: [(a, b) for a, b, t in blks if t == h]
    by_line = sorted((line, h, d) for h, (d, line) in heads.items())
    children = lambda h: [hh for line, hh, d in by_line if d == heads[h][0] + 1 and parent_of(hh) == h]

    def parent_of(h):          # the nearest head above it in the text with a smaller depth
        d, line = heads[h]
        best = None
        for l2, h2, d2 in by_line:
            if l2 < line and d2 == d - 1:
                best = h2
        return best
    depth0 = 2 if slice_ else 1
    batch = next(h for line, h, d in by_line if d == depth0 and children(h))
    chunk = next(h for h in children(batch) if children(h))
    kids = children(chunk)
    assert len(kids) == 3, 'two piece walks and the loop over rows (or over pending rows) expected in the chunk loop'
    after = [h for h in children(batch) if heads[h][1] > heads[chunk][1] and not children(h)]
    final = after[0]
    third = own(kids[2])
    third_text = sorted(third)
    out = {}
    if first_line(lines, third_text, 'ds_write_b32') is not None:          # a loop over the rows of the batch: test, then drain
        head_line = heads[kids[2]][1]
        body = cut(third_text, head_line, before=False)
        barrier = first_line(lines, body, '; wave barrier')
        out['rows'] = 1
        out['test'] = cut(body, barrier, before=True)
        out['drain'] = cut(body, barrier, before=False) + cut(third_text, head_line, before=True)
        out['chunk'] = own(chunk) + own(kids[0]) + own(kids[1])
    else:                                                                  # unrolled tests in the chunk loop's own blocks; a loop of drains
        mine = sorted(own(chunk))
        first_pk = first_line(lines, mine, 'v_pk_')
        barrier = first_line(lines, cut(mine, first_pk, before=False), '; wave barrier')
        tests = cut(cut(mine, first_pk, before=False), barrier, before=True)
        out['rows'] = 0          # (counted by unrolled_rows)
        out['test'] = tests
        out['drain'] = third_text
        out['chunk'] = cut(mine, first_pk, before=True) + cut(mine, barrier, before=False) + own(kids[0]) + own(kids[1])
    fin = sorted(own(final))
    pk = [i for a, b in fin for i in range(a, b + 1) if (T.mnemonic(lines[i]) or '').startswith('v_pk_')]
    # the two forms are runs of blocks one behind the other; the packed one is the run around the v_pk_ instructions: it starts with
    # the block that reads the ring ahead of them (the last ds_read before the first v_pk_) and ends before the other form's ring read
    reads = [i for a, b in fin for i in range(a, b + 1) if (T.mnemonic(lines[i]) or '').startswith('ds_read')]
    start2 = max(i for i in reads if i < pk[0])
    start2 = max(a for a, b in fin if a <= start2)
    later = [i for i in reads if i > pk[-1]]
    if later:          # [packed][one per lane]
        end2 = max(a for a, b in fin if a <= later[0]) - 1
        out['final2'] = cut(cut(fin, start2, before=False), end2 + 1, before=True)
        out['final1'] = cut(fin, end2 + 1, before=False)
    else:              # [one per lane][packed]
        out['final2'] = cut(fin, start2, before=False)
        out['final1'] = cut(fin, start2, before=True)
    return out


def unrolled_rows(lines, spans):
    """Copies of the test in the spans: every copy files the hits of its two halves (one ds_write_b32 each)."""
    n = sum(1 for a, b in spans for i in range(a, b + 1) if T.mnemonic(lines[i]) == 'ds_write_b32')
    return max(1, n // 2)


def analyse(lines):
    """-> {(COUNT_ONLY, RINT, SLICE): dict(vgpr, sgpr, scratch, lds, sgpr_spills, vgpr_spills, whole, bytes, rows,
    test / chunk / drain / final2 / final1: {lane, mov, sel, arith, valu})}; test: of the `rows` copies together."""
    ks = B.kernels(lines)
    md, lds, sp = T.metadata(lines), B.lds_bytes(lines), spills(lines)
    out = {}
    for sym in ks:
        args = B.template_args(sym)
        lo, hi = ks[sym]
        spans = loop_spans(lines, lo, hi, args[2])
        rows = unrolled_rows(lines, spans['test']) if spans['rows'] != 1 else 1
        rec = dict(vgpr=md[sym]['vgpr'], sgpr=md[sym]['sgpr'], scratch=md[sym]['scratch'], lds=lds[sym], sgpr_spills=sp[sym][0],
                   vgpr_spills=sp[sym][1], whole=B.tally(lines, lo, hi)[0], bytes=text_bytes(lines, hi), rows=rows)
        for name in ('test', 'chunk', 'drain', 'final2', 'final1'):
            c = tally(lines, spans[name])
            c['valu'] = sum(c[k] for k in KINDS)
            rec[name] = c
        out[args] = rec
    return out


SPANS = (('test', 'test'), ('chunk', 'chunk pair'), ('drain', 'drain 128'), ('final2', 'final drain, packed'), ('final1', 'final drain, one per lane'))


def parse_table(text, label):
    """The table that report() printed under `== <label>:` in a file such as profiles/build_loops_isa.txt
    -> {(COUNT_ONLY, RINT, SLICE): dict(vgpr, sgpr, scratch, whole, bytes, rows, test / chunk / drain / final2 / final1: vector
    instructions)}."""
    out = {}
    cur = None
    on = False
    for line in text.split('\n'):
        if line.startswith('== '):
            on = line.startswith('== %s:' % label)
            continue
        if not on:
            continue
        m = re.match(r'<(\w+), (\w+), (\w+)>\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)/(\d+)\s+(\d+)\s+(\d+)', line)
        if m:
            cur = out.setdefault(tuple(v == 'true' for v in m.group(1, 2, 3)), {})
            cur.update(vgpr=int(m.group(4)), sgpr=int(m.group(5)), scratch=int(m.group(6)), whole=int(m.group(10)), bytes=int(m.group(11)))
            continue
        m = re.match(r'    (.+?)\s+(\d+) =\s+\d+ \+', line)
        if m and cur is not None:
            for key, starts in SPANS:
                if m.group(1).startswith(starts):
                    cur[key] = int(m.group(2))
            mm = re.match(r'test: (\d+) row', m.group(1))
            if mm:
                cur['rows'] = int(mm.group(1))
    return out


def compile_asm(src, whole=False):
    """cluster.hip -> assembly.  Unless `whole`, the pair kernels are cut down to the two of a tuning build (-DAMM_CLUSTER_TUNE), which
    compiles in a sixth of the time; k_cbuild does not see the macro: its eight kernels come out the same, to the instruction."""
    if whole:
        return T.compile_asm(src)
    import subprocess
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix='build_loops_isa_'), 'cluster.s')
    cmd = [os.environ.get('HIPCC', 'hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-S', '--cuda-device-only', '-DAMM_CLUSTER_TUNE', src, '-o', out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
    return out


def report(lines, label):
    res = analyse(lines)
    print('== %s: %d k_cbuild instantiations' % (label, len(res)))
    print('%-28s %4s %4s %7s %6s %6s %6s %6s   %s' % ('<COUNT_ONLY, RINT, SLICE>', 'VGPR', 'SGPR', 'scratch', 'LDS', 'spills', 'whole', 'bytes',
                                                      'vector instructions: all = lane + mov + sel + arithmetic'))
    for args in sorted(res):
        r = res[args]
        print('%-28s %4d %4d %7d %6d %3d/%-2d %6d %6d' % ('<%s>' % ', '.join(str(v).lower() for v in args), r['vgpr'], r['sgpr'], r['scratch'],
                                                        r['lds'], r['sgpr_spills'], r['vgpr_spills'], r['whole'], r['bytes']))
        for name, what in (('test', 'test: %d row%s, %.1f per row' % (r['rows'], '' if r['rows'] == 1 else 's', r['test']['valu'] / r['rows'])),
                           ('chunk', 'chunk pair: head + fetch + tail'),
                           ('drain', 'drain 128 (packed, in the chunk loop)'), ('final2', 'final drain, packed'), ('final1', 'final drain, one per lane')):
            c = r[name]
            print('    %-40s %4d = %3d + %3d + %3d + %3d' % (what, c['valu'], c['lane'], c['mov'], c['sel'], c['arith']))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm', default=None, help='an assembly file made by hipcc -S --cuda-device-only (default: compile --src)')
    ap.add_argument('--src', default=os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'cluster.hip'))
    ap.add_argument('--label', default=None)
    ap.add_argument('--whole', action='store_true', help='compile every pair kernel too (the build of the library: slower, the same k_cbuild)')
    a = ap.parse_args()
    path = a.asm or compile_asm(a.src, a.whole)
    with open(path) as fh:
        text = fh.read().split('\n')
    report(text, a.label or os.path.basename(path))
    sys.exit(0)
