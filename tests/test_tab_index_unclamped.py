"""CPU test (no GPU): the molecule-row pair kernels read a radial table WITHOUT clamping the interval index for a pair that counts
(csrc/pair_tab.h: amm_tab_fetch_pass).  That is sound only if r2min <= r2 < rc2 -- for a site pair also ss_r2min <= r2 -- puts the
index inside the table.  amm_pair_table_check builds a descriptor's tables on the host as amm_pair_create does and forms the index
as the kernels do (r2 * scale in fp64, exponent and leading mantissa bits minus the zone's base) at r2 = r2min, the next double,
every interval boundary and the two doubles on either side of it, and the last double below rc2, likewise from ss_r2min for the
site-site table; no point may fall outside [0, nint) -- site pairs: [ss_first, nint).

Tables: every family and parameter set the tests and the bench build -- the near force with force switch (0.7 / 0.5 and 0.6 / 0.45
nm), with shift and plain; the damped force 2.9 / 1.0 / 0.9 and its general-degree variants; Ewald direct space; reaction field;
plain cutoff; the guarded discount of the near force (looked up to its guard radius only) -- each with the site-site table of the
TIP3P oxygens and without."""
import pytest

from atomsmm_amd import backend as B

O_SITE = dict(site_sigma=0.315075, site_eps=0.635968, site_q=-0.834)
EPS_RF = 78.3

TABLES = {
    'near_fswitch_0.7_0.5': dict(family=B.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5),
    'near_fswitch_0.6_0.45': dict(family=B.NEAR_FSWITCH, rc=0.6, rc0=0.6, rs0=0.45),
    'near_shift_0.7_0.5': dict(family=B.NEAR_SHIFT, rc=0.7, rc0=0.7, rs0=0.5),
    'near_none_0.7_0.5': dict(family=B.NEAR_NONE, rc=0.7, rc0=0.7, rs0=0.5),
    'near_discount_guarded': dict(family=B.NEAR_FSWITCH, rc=1.0, rc0=0.7, rs0=0.5, flags=B.GUARD_RC0, sign=-1.0),
    'damped_2.9_1.0_0.9': dict(family=B.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=1),
    'damped_degree2': dict(family=B.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=2),
    'damped_degree3': dict(family=B.DAMPED, rc=1.0, rswitch=0.9, alpha=2.9, degree=3),
    'ewald_direct': dict(family=B.NONBONDED, rc=1.0, rswitch=0.9, alpha=2.628260884878466, flags=B.COULOMB_EWALD | B.SWITCH),
    'ewald_direct_no_switch': dict(family=B.NONBONDED, rc=0.9, alpha=3.1, flags=B.COULOMB_EWALD),
    'reaction_field': dict(family=B.NONBONDED, rc=1.0, rswitch=0.9, flags=B.COULOMB_RF | B.SWITCH, krf=(EPS_RF - 1) / (2 * EPS_RF + 1),
                           crf=3 * EPS_RF / (2 * EPS_RF + 1)),
    'plain_cutoff': dict(family=B.NONBONDED, rc=1.2),
}


@pytest.mark.parametrize('sites', [False, True])
@pytest.mark.parametrize('name', sorted(TABLES))
def test_unclamped_index_stays_inside_the_table(name, sites):
    kw = dict(TABLES[name])
    desc = B.pair_desc(kw.pop('family'), kw.pop('rc'), **kw)
    res = B.pair_table_check(desc, **(O_SITE if sites else {}))
    print(name, 'sites' if sites else 'no sites', res)
    assert res['nint'] > 0
    # every interval's lower boundary was met on both sides, for the Coulomb table and (with sites) the site-site table
    assert res['points'] >= 3 * (res['nint'] - 2)
    if sites:
        assert 0 <= res['ss_first'] < res['n_below_kink']
        assert res['points'] >= 3 * (res['nint'] - 2) + 3 * (res['nint'] - res['ss_first'] - 2)
    else:
        assert res['ss_first'] == -1
    assert res['bad'] == 0
    # the ends: the first interval is reached, and the last one a counting pair reads lies below the spare interval beyond the cutoff
    assert res['idx_min'] == 0 and 0 < res['idx_max'] <= res['nint'] - 2
