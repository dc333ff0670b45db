"""CPU checks of the bond-list test infrastructure (tests/bonded_ref.py, tests/bonded_cases.py): the mpmath reference's forces against
an independent differentiation, the fp64 restatement against the reference (the measured deviations that set the GPU tolerances),
the zoo's declared layouts against the restated finalize rules, and the geometry filter's yield."""
import numpy as np
import pytest
from mpmath import mp, mpf

import bonded_cases as Z
import bonded_ref as R


def _sample_terms():
    """one term of every kind out of Z9 (all kinds, periodic flags per kind, images across the faces) and a torsion of Z6-9"""
    z9 = Z.zoo()['Z9']
    seen, out = set(), []
    for kind, at, p in z9.terms:
        if kind not in seen:
            seen.add(kind)
            out.append((z9, kind, at, p))
    z6 = Z.zoo()['Z6-9']
    out.append((z6,) + [t for t in z6.terms if t[0] == Z.TORSION][3])
    assert seen == set(range(8))
    return out


def test_reference_forces_against_richardson_differences():
    """The h = 1e-25 central differences against a Richardson-extrapolated pair of far larger steps at 80 digits (h = 1e-12 and
    5e-13: error O(h^4)): they agree to 1e-28 of the term's largest force (or of 1 kJ/mol/nm where the term's force vanishes), so the
    step is neither too small for 60 digits nor too large for the curvature."""
    for case, kind, at, p in _sample_terms():
        _, f = R.term_forces_mp(kind, case.x[list(at)], p, case.periodic[kind], case.box)
        mp.dps = 80
        x = [[mpf(float(v)) for v in row] for row in case.x[list(at)]]

        def diff(a, k, h):
            keep = x[a][k]
            x[a][k] = keep + h
            ep = R.term_energy_mp(kind, x, p, case.periodic[kind], case.box)
            x[a][k] = keep - h
            em = R.term_energy_mp(kind, x, p, case.periodic[kind], case.box)
            x[a][k] = keep
            return -(ep - em) / (2 * h)

        scale = max([abs(v) for row in f for v in row] + [mpf(1)])
        for a in range(len(at)):
            for k in range(3):
                d1, d2 = diff(a, k, mpf('1e-12')), diff(a, k, mpf('5e-13'))
                rich = (4 * d2 - d1) / 3
                assert abs(rich - f[a][k]) <= mpf('1e-28') * scale, (kind, a, k)
        mp.dps = 50


def test_reference_forces_sum_to_zero_and_carry_no_torque():
    """translation and rotation invariance of every energy: what a wrong sign or a wrong image in the reference would break (the
    torque about the term's first atom, with the other atoms at their nearest image where the kind is periodic)"""
    for case, kind, at, p in _sample_terms():
        _, f = R.term_forces_mp(kind, case.x[list(at)], p, case.periodic[kind], case.box)
        f = np.array([[float(v) for v in row] for row in f])
        assert np.abs(f.sum(0)).max() <= 1e-13 * np.abs(f).max()
        rel = case.x[list(at)] - case.x[at[0]]
        if case.periodic[kind] or kind == Z.EWALD:
            rel = rel - case.box * np.rint(rel / case.box)
        torque = np.cross(rel, f).sum(0)
        assert np.abs(torque).max() <= 1e-13 * np.abs(f).max() * max(np.abs(rel).max(), 1e-3), (kind, torque)


def test_dihedral_convention_is_iupac():
    """cis = 0, trans = pi, and d turned clockwise from a, looking along b -> c (here: from below, up the z axis, where x -> y is clockwise), is positive"""
    a, b, c = [1.0, 0, 0], [0.0, 0, 0], [0.0, 0, 1.0]
    box = np.ones(3)
    for d, want in (([1.0, 0, 1], 0.0), ([-1.0, 0, 1], np.pi), ([0.0, 1.0, 1], np.pi / 2), ([0.0, -1.0, 1], -np.pi / 2)):
        got = float(R.dihedral_mp([[mpf(v) for v in q] for q in (a, b, c, d)], box, False))
        assert abs(got - want) < 1e-15
        assert abs(Z.dihedral_of(*map(np.array, (a, b, c, d))) - want) < 1e-15


def measured_deviation():
    """Worst deviation of the fp64 restatement from the reference over the atoms of the plain zoo, in the unit S_i (forces) and, per
    case, sum |E_t| (energies): all kinds together [8], and the part of each kind [0..7]."""
    wf, we = np.zeros(9), np.zeros(9)
    for name in Z.NAMES:
        case, ref = Z.zoo()[name], Z.reference(name)
        df, de = np.zeros((9, case.n, 3)), np.zeros(9)
        for t, (kind, at, p) in enumerate(case.terms):
            e, f = R.term_np(kind, case.x[list(at)], p, case.periodic[kind], case.box)
            for r, a in enumerate(at):
                df[kind, a] += f[r] - ref.f_terms[t, r]
            de[kind] += e - ref.e_terms[t]
        df[8], de[8] = df[:8].sum(0), de[:8].sum()
        S = ref.units(case)
        live = S > 0
        if live.any():
            wf = np.maximum(wf, (np.linalg.norm(df, axis=2)[:, live] / S[live]).max(1))
            we = np.maximum(we, np.abs(de) / ref.e_unit)
    return wf, we


def test_restatement_deviation_is_what_the_tolerance_says():
    """The recorded W_FORCE_CPU / W_ENERGY_CPU (the GPU tests allow 16 x their last entry) are ceilings of what a CPU run measures,
    and tight ones: the measurement reaches at least a quarter of each (another libm moves the last digit, not the exponent)."""
    wf, we = measured_deviation()
    print('force ', ' '.join('%.2e' % v for v in wf))
    print('energy', ' '.join('%.2e' % v for v in we))
    rec_f, rec_e = np.array(Z.W_FORCE_CPU), np.array(Z.W_ENERGY_CPU)
    assert (wf <= rec_f).all() and (wf >= 0.25 * rec_f).all(), (wf, rec_f)
    assert (we <= rec_e).all() and (we >= 0.25 * rec_e).all(), (we, rec_e)


@pytest.mark.parametrize('name', Z.ALL_NAMES)
def test_declared_layout_follows_from_the_finalize_rules(name):
    case = Z.zoo()[name]
    assert case.n % 64 != 0 and case.n <= 1500 and len(case.terms) <= 600
    assert Z.layout(case.n, case.terms) == case.expect
    assert Z.layout(case.n, case.terms, terms_from=1) == case.expect_tf1
    if case.expect['max_comp'] <= 8:
        assert (case.expect['ncomp'] * case.expect['G']) % 256 != 0
    for kind, at, _ in case.terms:
        assert len(set(at)) == len(at) == Z.ARITY[kind]


def test_zoo_covers_both_sides_of_every_guard():
    z = {n: Z.zoo()[n] for n in Z.NAMES}
    e, e1 = {n: c.expect for n, c in z.items()}, {n: c.expect_tf1 for n, c in z.items()}
    assert {e[n]['G'] for n in z if e[n]['max_comp'] in (4, 5)} == {4, 8}
    assert e['Z7-8']['terms_ok'] == 1 and e['Z7-9']['terms_ok'] == 0 and e['Z7-8']['max_comp'] == 8 and e['Z7-9']['max_comp'] == 9
    assert (e['Z2']['terms_ok'], e['Z3']['terms_ok'], e['Z6-8']['terms_ok'], e['Z6-9']['terms_ok']) == (1, 0, 1, 0)
    assert [n for n in z if e[n]['mol3_ok']] == ['Z1', 'Z2']
    assert not any(c.expect['mol3_ok'] for n, c in Z.zoo().items() if n.endswith('~'))
    assert (e1['Z8-above']['mixed_ok'], e1['Z8-equal']['mixed_ok'], e1['Z8-below']['mixed_ok']) == (1, 1, 0)
    for n, tag in (('Z8-above', 1), ('Z8-equal', 0), ('Z8-below', -1)):
        lay = Z.layout(z[n].n, z[n].terms, 1)
        nsmall_atoms = z[n].n - 19
        assert np.sign(2 * nsmall_atoms - z[n].n) == tag and lay['max_comp'] == 19
    assert e1['Z5']['mixed_ok'] == 0 and e1['Z5']['n_gterms'] > 0 and e1['Z5']['terms_ok'] == 0
    assert all(v['mixed_ok'] == 0 and v['n_gterms'] == 0 for v in e.values())
    z9 = z['Z9']
    assert {k for k, _, _ in z9.terms} == set(range(8)) and len(set(z9.periodic)) == 2
    d = z9.x[z9.n - 1, 0] - z9.x[z9.n - 2, 0]
    assert d == np.nextafter(1.5, 0.0) and z9.box[0] == 3.0
    ew = [np.linalg.norm((lambda v: v - 3.0 * np.rint(v / 3.0))(z9.x[at[0]] - z9.x[at[1]])) for k, at, _ in z9.terms if k == Z.EWALD]
    assert abs(min(ew) - 0.05) < 1e-12 and abs(max(ew) - 0.3) < 1e-12
    straddle = sum(1 for k, at, _ in z9.terms if z9.periodic[k] and np.abs(z9.x[at[0]] - z9.x[at[1]]).max() > 1.5)
    assert straddle >= 20


def test_filter_keeps_nine_in_ten():
    Z.zoo()
    assert Z.DRAWN['drawn'] > 1000
    assert Z.DRAWN['kept'] >= 0.9 * Z.DRAWN['drawn'], Z.DRAWN
    for name in Z.NAMES:
        case = Z.zoo()[name]
        if name != 'Z9':
            assert Z.usable(case.x, case.terms), name
