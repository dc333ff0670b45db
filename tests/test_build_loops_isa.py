"""CPU test (no GPU; skipped without hipcc): what the compiler makes of the loops of the list build (scripts/build_loops_isa.py on
csrc/cluster.hip of this tree: all eight k_cbuild<COUNT_ONLY, RINT, SLICE> instantiations).  The sphere test is unrolled over the batch
with a row's constants and ring state in scalar registers; the drains take their lane masks from the scalar side and store through a
32-bit offset.  The committed kernel's vector instructions per span -- the tests of a chunk pair, the chunk pair's head + fetch +
tail, the packed drain of a full ring, the two final drains -- are not above what profiles/build_loops_isa.txt records for this build
(and the test and the drains are below the parent's, recorded there too), and the register guards hold:

    whole-box instantiations <= 96 VGPRs (5 wavefronts per SIMD), slices no more VGPRs than at the parent (114 to 120),
    no scratch, no SGPR spill (a spilled scalar comes back as the v_writelane / v_readlane that the change removes), no VGPR spill,
    no lane moves at all in a whole-box kernel's tests."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which(os.environ.get('HIPCC', 'hipcc')) is None, reason='needs hipcc')

_spec = importlib.util.spec_from_file_location('build_loops_isa', os.path.join(ROOT, 'scripts', 'build_loops_isa.py'))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)
ALL = [(co, ri, sl) for co in (False, True) for ri in (False, True) for sl in (False, True)]
SPANS = ('test', 'chunk', 'drain', 'final2', 'final1')


@pytest.fixture(scope='module')
def build():
    path = S.compile_asm(os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'cluster.hip'))
    try:
        with open(path) as fh:
            lines = fh.read().split('\n')
    finally:
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    return S.analyse(lines)


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(ROOT, 'profiles', 'build_loops_isa.txt')) as fh:
        text = fh.read()
    return S.parse_table(text, 'parent'), S.parse_table(text, 'this build')


def test_every_instantiation_is_there(build, recorded):
    parent, new = recorded
    assert sorted(build) == sorted(ALL) and sorted(parent) == sorted(ALL) and sorted(new) == sorted(ALL)


@pytest.mark.parametrize('args', ALL)
def test_vector_instructions_per_span(build, recorded, args):
    parent, new = recorded
    r = build[args]
    print(args, {k: r[k] for k in SPANS}, 'recorded', {k: new[args][k] for k in SPANS}, 'parent', {k: parent[args][k] for k in SPANS})
    assert r['rows'] == new[args]['rows'] == 5 and parent[args]['rows'] == 1          # unrolled over the batch
    for span in SPANS:
        assert r[span]['valu'] <= new[args][span], span
    # per row the test is shorter than the parent's, and so is every drain; what a chunk pair costs besides is no longer
    assert r['test']['valu'] < 5 * parent[args]['test']
    for span in ('drain', 'final2', 'final1'):
        assert r[span]['valu'] < parent[args][span], span
    assert r['chunk']['valu'] <= parent[args]['chunk'] + (3 if args[2] else 0)          # (a slice's kernel reads row 0's constants ahead of the branch)
    if not args[2]:
        assert r['test']['lane'] == 0 and r['test']['mov'] == 0


@pytest.mark.parametrize('args', ALL)
def test_register_guards(build, recorded, args):
    parent, new = recorded
    r = build[args]
    print(args, {k: r[k] for k in ('vgpr', 'sgpr', 'scratch', 'sgpr_spills', 'vgpr_spills', 'whole', 'bytes')})
    assert r['scratch'] == 0 and r['sgpr_spills'] == 0 and r['vgpr_spills'] == 0
    if args[2]:
        assert r['vgpr'] <= parent[args]['vgpr'] and 114 <= parent[args]['vgpr'] <= 120
    else:
        assert r['vgpr'] <= 96
    assert r['lds'] == 31928          # the rings and the cell's tables, as before
