"""CPU test (no GPU; skipped without hipcc): what the compiler makes of the trip loops of the molecule-row pair kernels the bench
launches (scripts/trip_loop_isa.py on csrc/cluster.hip of this tree).  With the zone's base folded into the look-up's address
(csrc/pair_tab.h: amm_tab_fetch_pass) a look-up is one vector instruction shorter, and the fused pass whose guest factor is exactly
1.0 drops nine more per front trip:

    near pass   k_cpair<2, 0, -1, 512, 1, EPI>        interior <= 290, image per molecule <= 311     (before: 299 / 320)
    fused pass  k_cpair<3, 1, 2, 512, 1, EPI, true>   interior <= 492, image per molecule <= 513     (before: 510 / 532; measured 483 / 505)

no lane moves (scalars parked in lanes of a vector register) in the interior loops, no scratch in these kernels, no instantiation
above 256 VGPRs, and no more scratch in all than before the change (10 instantiations, 572 bytes).  The fused pass for any other
guest factor keeps the product: its interior loop obeys the same bound (its image-per-molecule loop with the epilogue holds one lane
reload, 514; profiles/lookup_offset_isa.txt)."""
import importlib.util
import os
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.skipif(shutil.which(os.environ.get('HIPCC', 'hipcc')) is None, reason='needs hipcc')

_spec = importlib.util.spec_from_file_location('trip_loop_isa', os.path.join(ROOT, 'scripts', 'trip_loop_isa.py'))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


@pytest.fixture(scope='module')
def build():
    """-> {template arguments: (metadata, [(VALU, lane moves, cold VALU, cold lane moves)] per trip loop, fewest first)}."""
    path = S.compile_asm(os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'cluster.hip'))
    try:
        with open(path) as fh:
            lines = fh.read().split('\n')
    finally:
        shutil.rmtree(os.path.dirname(path), ignore_errors=True)
    ks, md = S.kernels(lines), S.metadata(lines)
    return {S.demangle_args(sym): (md[sym], S.trip_loops(lines, *span)) for sym, span in ks.items()}


@pytest.mark.parametrize('epi', [True, False])
def test_near_pass_trip_loop(build, epi):
    md, trips = build[(2, 0, -1, 512, 1, epi, False)]
    print(md, trips)
    assert len(trips) == 3
    (interior, lane0, _, _), (image, _, _, _) = trips[0], trips[1]
    assert interior <= 290 and image <= 311 and lane0 == 0
    assert md['scratch'] == 0 and md['vgpr'] <= 256


@pytest.mark.parametrize('epi', [True, False])
def test_fused_pass_trip_loop(build, epi):
    # what the bench launches: the guest's factor is exactly 1.0
    md, trips = build[(3, 1, 2, 512, 1, epi, True)]
    print(md, trips)
    assert len(trips) == 3
    (interior, lane0, _, _), (image, _, _, _) = trips[0], trips[1]
    assert interior <= 492 and image <= 513 and lane0 == 0
    assert md['scratch'] == 0 and md['vgpr'] <= 256
    # any other factor: the same look-ups, the product kept
    md_f, trips_f = build[(3, 1, 2, 512, 1, epi, False)]
    print(md_f, trips_f)
    assert trips_f[0][0] <= 492 and trips_f[0][1] == 0 and interior < trips_f[0][0]          # (nine v_mul_f64 fewer, as compiled today)
    assert md_f['scratch'] == 0 and md_f['vgpr'] <= 256


def test_registers_and_scratch_of_all_instantiations(build):
    assert len(build) == 71          # 65 + the six fused zero-slot kernels for a unit guest factor
    assert max(md['vgpr'] for md, _ in build.values()) <= 256
    with_scratch = {k: md['scratch'] for k, (md, _) in build.items() if md['scratch'] > 0}
    print(with_scratch)
    assert len(with_scratch) <= 10 and sum(with_scratch.values()) <= 572
    # the flag exists for the fused zero-slot kernels only
    assert sorted(k[:3] for k in build if k[6]) == sorted([(3, 1, 2), (4, 0, 2), (4, 2, 2)] * 2)
