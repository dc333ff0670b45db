"""CPU tests of the checker the PME GPU tests rely on (tests/pme_cases.py): before it judges a kernel it must itself reproduce the
two reciprocal-space numbers that OpenMM wrote (G8, G14), agree with 80-bit arithmetic, have forces that are the gradient of its
energy, converge to the explicit Ewald sum with the order of its splines -- and notice six planted errors of the kinds a kernel can
have, each by more than the tolerance the GPU test of that case grants.  A last test reads the constants that the case table
mirrors out of the kernel sources and asserts that the table still reaches every spread path."""
import os
import re

import numpy as np
import pytest

import pme_cases as PC
from helpers import solvation_respa_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SMALL = [name for name in PC.CASES if np.prod(PC.MESHES[name]) <= 32 ** 3 and name != 'many_blocks']


def reference(c, **kw):
    return PC.pme_reference(c['pos'], c['box'], c['q'], c['alpha'], c['K'], c['Kc'], **kw)


def test_cases_are_what_the_gpu_tests_assume():
    """At least 64 charged atoms, about one atom in nine without charge, a rectangular box with three different edges, and the
    seven edge atoms where they are said to be."""
    assert SMALL == ['aligned', 'atomic', 'one_tile_halo', 'ragged']
    for name in PC.CASES:
        c = PC.case(name)
        charged = np.flatnonzero(c['q'])
        assert len(charged) >= 64 and len(set(c['box'])) == 3
        if name != 'many_blocks':
            assert 0.08 < np.mean(c['q'] == 0) < 0.15
        else:
            assert len(c['q']) == 262400 and len(charged) == 256
        L, K = c['box'], np.array(c['K'])
        e = c['pos'][charged[:7]]
        assert np.array_equal(e[0], [0, 0, 0]) and np.array_equal(e[1], L) and e[2, 0] == -1e-18
        assert np.array_equal(e[3], np.array([2, -1, 3]) * L)       # whole boxes, to the rounding of the product
        assert (np.abs(e[4] / L) > 3).all() and (np.abs(e[4] / L) < 5).all()
        assert (np.abs(e[5] / L * K - np.rint(e[5] / L * K)) <= 2 * EPS * K).all()       # on a node, to the rounding of L k / K
        below = e[6] / L * K - np.rint(e[5] / L * K)
        assert (below < 0).all() and (below > -1e-11).all()
        assert PC.case(name) is c                                   # one set of arrays, shared


@pytest.mark.parametrize('which', ['spcfw', 'heaq'])
def test_reference_reproduces_openmm_literals(spcfw, heaq, goldens, which):
    """On OpenMM's default mesh, ceil(2 alpha L / (3 tol^(1/5))), the reference gives the reciprocal-space energy (self term
    included) that OpenMM gave: G8 and G14 to rel 1e-10, the bound of the GPU test of the same literals (measured 1.3e-13, both)."""
    if which == 'spcfw':
        c, q, gold = spcfw, spcfw['charge'], goldens['G8']['value']
    else:
        c, q, gold = heaq, solvation_respa_inputs(heaq, 0.5)[0], goldens['G14']['value']
    alpha = np.sqrt(-np.log(2 * 5e-4)) / 1.0
    K = [int(np.ceil(2 * alpha * L / (3 * 5e-4 ** 0.2))) for L in c['box']]
    er, es, _ = PC.run_reference(PC.PmeReference(), c['positions'], c['box'], q, alpha, K, want_forces=False)
    print(which, K, 'reference vs literal: rel', abs(er + es - gold) / abs(gold))
    assert er + es == pytest.approx(gold, rel=1e-10)


@pytest.mark.parametrize('name', SMALL)
def test_float64_reference_agrees_with_80_bit(name):
    """Bound 256 eps (of max|F|, and of E_rec + |E_self|): what the GPU tests grant double-precision transforms.  Measured 1e-15."""
    if np.finfo(np.longdouble).eps >= EPS:
        pytest.fail('np.longdouble is no wider than float64 on this platform: the reference has nothing to be compared with')
    c = PC.case(name)
    t = PC.case_tolerances(name)
    er, es, F = reference(c, dtype=np.longdouble)
    assert F.dtype == np.longdouble
    dF, dE = float(np.abs(t['F'] - F).max()), float(abs((er + es) - (np.longdouble(t['E_rec']) + np.longdouble(t['E_self']))))
    print(name, 'float64 vs longdouble: dF/max|F| %.2e  dE/(E_rec+|E_self|) %.2e' % (dF / t['fmax'], dE / (t['E_rec'] + abs(t['E_self']))))
    assert dF <= 256 * EPS * t['fmax']
    assert dE <= 256 * EPS * (t['E_rec'] + abs(t['E_self']))


@pytest.mark.parametrize('name', ['atomic', 'one_tile_halo', 'ragged'])
def test_forces_are_the_gradient_of_the_energy(name):
    """Central differences of the 80-bit energy, h = 1e-5 nm, for a handful of atoms and axes (edge atoms among them): 1e-9 of
    max|F| (measured 3.6e-11 to 7.8e-11: the truncation term h^2 E''' / 6)."""
    c = PC.case(name)
    t = PC.case_tolerances(name)
    charged = np.flatnonzero(c['q'])
    model, h = PC.PmeReference(np.longdouble), 1e-5
    worst = 0.0
    for atom, axis in ((charged[PC.EDGE_ATOMS['origin']], 0), (charged[PC.EDGE_ATOMS['minus 1e-18']], 0),
                       (charged[PC.EDGE_ATOMS['on a node']], 2), (charged[20], 1), (charged[-1], 2)):
        e = []
        for sign in (+1, -1):
            x = c['pos'].copy()
            x[atom, axis] += sign * h
            e.append(PC.run_reference(model, x, c['box'], c['q'], c['alpha'], c['K'], want_forces=False)[0])
        worst = max(worst, abs(float(-(e[0] - e[1]) / (2 * h)) - t['F'][atom, axis]))
    print(name, 'central differences vs forces: %.2e of max|F|' % (worst / t['fmax']))
    assert worst <= 1e-9 * t['fmax']


def test_reference_converges_to_the_explicit_ewald_sum():
    """Meshes in ratio 1 : 2 : 4 at fixed alpha: the errors of energy and forces against the k-sum fall by at least 8 per doubling
    (order-5 splines: 16 to 32 in theory; measured 16 to 20 for the forces, 33 to 67 for the energy)."""
    c = PC.case('ragged')
    e0, f0 = PC.ewald_k_sum(c['pos'], c['box'], c['q'], c['alpha'], 12)
    err_e, err_f = [], []
    for scale in (1, 2, 4):
        er, _, F = PC.pme_reference(c['pos'], c['box'], c['q'], c['alpha'], [scale * k for k in (24, 28, 23)], c['Kc'])
        err_e.append(abs(er - e0) / abs(e0))
        err_f.append(np.abs(F - f0).max() / np.abs(f0).max())
    print('energy', err_e, 'forces', err_f)
    assert err_f[0] < 1e-4 and err_e[0] < 1e-4
    for err in (err_e, err_f):
        assert err[0] >= 8 * err[1] and err[1] >= 8 * err[2]


# ---- sensitivity: the kernels cannot be mutated from a test, so each kind of error is planted in a copy of the reference ----------
class NyquistTwice(PC.PmeReference):
    def plane_weights(self, Kz):
        w = PC.PmeReference.plane_weights(self, Kz)
        assert Kz % 2 == 0
        w[-1] = 2
        return w


class FoldBelowHalf(PC.PmeReference):
    def frequencies(self, axis, K):
        if axis != 0:
            return PC.PmeReference.frequencies(self, axis, K)
        assert K % 2 == 1
        k = np.arange(K)
        return np.where(k < K // 2, k, k - K)          # (K + 1) / 2 is the right bound on an odd mesh


class OneWeightOff(PC.PmeReference):
    def axis_terms(self, axis, x, L, K):
        pts, w, dw = PC.PmeReference.axis_terms(self, axis, x, L, K)
        if axis == 1:
            w, dw = w.copy(), dw.copy()
            w[:, 3] *= 1 + 1e-9
            dw[:, 3] *= 1 + 1e-9
        return pts, w, dw


class NoWrap(PC.PmeReference):
    def axis_terms(self, axis, x, L, K):
        pts, w, dw = PC.PmeReference.axis_terms(self, axis, x, L, K)
        idx = pts[:, :1]
        inside = idx + np.arange(PC.ORDER)[None, :] < K
        return pts, w * inside, dw * inside


class ForceOnUncharged(PC.PmeReference):
    def force_charge(self, q):
        return np.where(q == 0, self.T(1e-9), q)


class ModuliOfAnotherAxis(PC.PmeReference):
    K_other = None

    def moduli(self, axis, K):
        if axis != 1:
            return PC.PmeReference.moduli(self, axis, K)
        return PC.PmeReference.moduli(self, 0, self.K_other)[np.arange(K) % self.K_other]


MUTATIONS = {
    # (on 'aligned', Kz = 32, the plane's terms are below 1e-40 of the energy: the error shows where the plane carries weight)
    'Nyquist plane counted twice on an even Kz': (NyquistTwice, 'one_tile_halo'),
    'mx folded below Kx / 2 on an odd Kx': (FoldBelowHalf, 'ragged'),
    'one spline weight scaled by 1 + 1e-9': (OneWeightOff, 'ragged'),
    'no wrap through the upper face': (NoWrap, 'one_tile_halo'),
    'a force on atoms without charge': (ForceOnUncharged, 'atomic'),
    'moduli of x used for y': (ModuliOfAnotherAxis, 'ragged'),
}


@pytest.mark.parametrize('what', sorted(MUTATIONS))
def test_reference_notices_a_planted_error(what):
    """Each planted error moves the energy or a force by more than the tolerance that tests/test_gpu_pme.py grants the case it is
    planted in -- here by more than twice that, so that a kernel with the error cannot hide in the tolerance's far side."""
    mutant, name = MUTATIONS[what]
    c = PC.case(name)
    t = PC.case_tolerances(name)
    model = mutant()
    model.K_other = c['K'][0]
    assert c['K'][0] != c['K'][1] or mutant is not ModuliOfAnotherAxis
    er, es, F = PC.run_reference(model, c['pos'], c['box'], c['q'], c['alpha'], c['K'], c['Kc'])
    moved_F, moved_E = np.abs(F - t['F']).max(), abs(er + es - t['E'])
    print('%s on %s: forces moved by %.2e (tolerance %.2e), energy by %.2e (tolerance %.2e)'
          % (what, name, moved_F, t['tol_F'], moved_E, t['tol_E']))
    assert moved_F > 2 * t['tol_F'] or moved_E > 2 * t['tol_E']
    if mutant is ForceOnUncharged:
        assert np.abs(F[c['q'] == 0]).max() > 2 * t['tol_F']       # (and the GPU test wants exact zeros there)


def test_quantisation_term_is_alive_in_every_small_case():
    """dF, the part of the tolerance that models the 2^-42 mesh, is neither zero nor large: about 1e-12 of max|F|."""
    for name in SMALL:
        t = PC.case_tolerances(name)
        print(name, 'dF/max|F| %.2e  dE/|E| %.2e  tol_F/max|F| %.2e' % (t['dF'] / t['fmax'], t['dE'] / abs(t['E']), t['tol_F'] / t['fmax']))
        assert 1e-14 * t['fmax'] <= t['dF'] <= 1e-10 * t['fmax']


# ---- the constants the case table mirrors ----------------------------------------------------------------------------------------
def _constant(text, pattern):
    found = re.findall(pattern, text)
    assert len(found) >= 1 and len(set(found)) == 1, (pattern, found)
    return int(found[0])


def test_case_table_straddles_the_kernels_constants():
    """PME_TILE, PME_ORDER and PME_LDS_BINS of csrc/pme.hip, KEEP and the two-level ticket threshold of device_utils.h, read out of
    the source text: the meshes still lie below, at and above them, so a later change of a constant cannot un-cover a path."""
    with open(os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'pme.hip')) as fh:
        pme = fh.read()
    with open(os.path.join(ROOT, 'atomsmm_amd', 'csrc', 'device_utils.h')) as fh:
        utils = fh.read()
    tile = _constant(pme, r'#define PME_TILE (\d+)')
    order = _constant(pme, r'#define PME_ORDER (\d+)')
    lds_bins = _constant(pme, r'#define PME_LDS_BINS (\d+)')
    scan = utils[utils.index('int amm_block_scan_counts('):]
    keep = _constant(scan, r'constexpr int KEEP = (\d+);')
    two_level = _constant(utils[utils.index('bool amm_last_block('):utils.index('bool amm_last_of(')], r'if \(nb < (\d+)\)')
    block = _constant(pme, r'k_pme_bin_count_lds, dim3\(nb\), dim3\((\d+)\)')
    assert order == PC.ORDER
    edge = tile + order - 1

    def tiles(name):
        return int(np.prod([-(-k // tile) for k in PC.MESHES[name]]))

    def blocks(name):
        return -(-len(PC.case(name)['q']) // block)

    K = PC.MESHES
    assert min(K['atomic']) < edge and max(K['atomic']) < edge + tile           # device atomics
    assert set(K['one_tile_halo']) == {edge}                                    # the smallest tiled mesh
    for name in PC.CASES:
        if name != 'atomic':
            assert min(K[name]) >= edge
    assert all(k % tile for k in K['ragged']) and K['ragged'][0] % 2 == 1 and K['ragged'][2] % 2 == 1
    assert not any(k % tile for k in K['aligned']) and K['aligned'][2] % 2 == 0
    assert K['atomic'][2] % 2 == 1
    assert max(tiles(n) for n in ('one_tile_halo', 'ragged', 'aligned', 'many_blocks')) <= lds_bins
    assert lds_bins < tiles('global_bins') <= keep * 256 < tiles('long_scan')
    assert max(blocks(n) for n in PC.CASES if n != 'many_blocks') < two_level <= blocks('many_blocks')
    assert blocks('many_blocks') % 32 != 0                                      # ticket classes of unequal size
    assert len(PC.case('many_blocks')['q']) // tiles('many_blocks') > 1000      # thousands of atoms per tile
