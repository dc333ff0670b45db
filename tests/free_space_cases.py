"""Inputs of the free-space tests (NoCutoff / CutoffNonPeriodic), cut from the committed fixtures, and the oracle calls that
check them.  The checker is the periodic oracle in a box of 1000 nm: d - L rint(d / L) = d exactly for every distance met here,
so no minimum image is ever taken."""
import numpy as np

from oracle import oracle as O

FREE_BOX = np.full(3, 1000.0)        # the oracle's box: free space
BIG_BOX = np.full(3, 8.0)            # a periodic box that exceeds the droplet's extent plus every cutoff used here
EPS_RF = 78.3


def first_atoms(case, n):
    """The first n atoms of a fixture with every term whose atoms all lie among them, and no 'box'."""
    out = {}
    for key in ('positions', 'charge', 'sigma', 'epsilon', 'mass', 'residue', 'resname', 'atomname'):
        out[key] = case[key][:n].copy()
    for idx, rest in (('bonds', ('bond_r0', 'bond_k')), ('angles', ('angle_theta0', 'angle_k')),
                      ('torsions', ('torsion_n', 'torsion_phase', 'torsion_k')),
                      ('exc_pairs', ('exc_chargeprod', 'exc_sigma', 'exc_epsilon'))):
        keep = (case[idx] < n).all(axis=1)
        out[idx] = case[idx][keep].copy()
        for key in rest:
            out[key] = case[key][keep].copy()
    return out


def s33(heaq):
    """The 33 solute atoms of hydroxyethylaminoanthraquinone-in-water (they come first), with their bonds, angles, 6 torsions and
    exceptions: 170 of the 528 pairs are excluded."""
    n = int((heaq['resname'] != 'HOH').sum())
    assert n == 33 and (heaq['resname'][:n] != 'HOH').all()
    return first_atoms(heaq, n)


def d1527(spcfw):
    """The first 509 waters of q-SPC-FW: a droplet of 1527 atoms (whole molecules), not a multiple of 64 or 256."""
    return first_atoms(spcfw, 1527)


def tiny(n):
    """n = 1: nothing to evaluate; n = 2: one pair at 0.31 nm."""
    pos = np.array([[0.1, 0.2, 0.3], [0.35, 0.05, 0.42]])[:n]
    return dict(positions=pos, charge=np.array([-0.8, 0.4])[:n], sigma=np.array([0.3, 0.25])[:n],
                epsilon=np.array([0.6, 0.2])[:n], mass=np.array([16.0, 1.0])[:n], exc_pairs=np.zeros((0, 2), np.int32))


def rf_constants(rc, eps_rf=EPS_RF):
    return (eps_rf - 1) / ((2 * eps_rf + 1) * rc ** 3), 3 * eps_rf / ((2 * eps_rf + 1) * rc)


# name -> (descriptor arguments for the library, descriptor arguments for the oracle): every instantiation of csrc/free.hip.
# NoCutoff is rc = 0 for the library and, for the oracle, a cutoff no pair reaches with the reaction-field constants at zero.
def descriptors():
    krf, crf = rf_constants(1.0)
    NB, NN, NS, NF, DP = O.NONBONDED, O.NEAR_NONE, O.NEAR_SHIFT, O.NEAR_FSWITCH, O.DAMPED
    nocut = dict(family=NB, rc=400.0, flags=O.COULOMB_RF)
    table = {
        'nocutoff': (dict(family=NB, rc=0.0), nocut),
        # (what the engine hands over for NoCutoff never carries these; the library must ignore them without a cutoff)
        'nocutoff-rf-switch-ignored': (dict(family=NB, rc=0.0, rswitch=0.9, flags=O.COULOMB_RF | O.SWITCH, krf=krf, crf=crf), nocut),
        'plain': (dict(family=NB, rc=1.0),) * 2,
        'plain-switch': (dict(family=NB, rc=1.0, rswitch=0.9, flags=O.SWITCH),) * 2,
        'rf': (dict(family=NB, rc=1.0, flags=O.COULOMB_RF, krf=krf, crf=crf),) * 2,
        'rf-switch': (dict(family=NB, rc=1.0, rswitch=0.9, flags=O.COULOMB_RF | O.SWITCH, krf=krf, crf=crf),) * 2,
        'damped-1': (dict(family=DP, rc=1.0, rswitch=0.9, alpha=2.9, degree=1),) * 2,
        'damped-2': (dict(family=DP, rc=1.0, rswitch=0.9, alpha=2.9, degree=2),) * 2,
        'fswitch-noshift': (dict(family=NF, rc=0.7, rc0=0.7, rs0=0.5, flags=O.NO_SHIFT),) * 2,
    }
    for name, family in (('none', NN), ('shift', NS), ('fswitch', NF)):
        table['near-' + name] = (dict(family=family, rc=0.7, rc0=0.7, rs0=0.5),) * 2
        # the discount of FarNonbondedForce / group 31 of RESPASystem: guarded by step(rc0 - r) below a longer cutoff, sign -1
        table['near-' + name + '-guard'] = (dict(family=family, rc=1.0, rc0=0.7, rs0=0.5, flags=O.GUARD_RC0, sign=-1.0),) * 2
    return table


def oracle_pair(kw, case, box=FREE_BOX, charge=None):
    kw = dict(kw)
    d = O.desc(kw.pop('family'), **kw)
    q = case['charge'] if charge is None else charge
    return O.pair_eval(d, case['positions'], box, q, case['sigma'], case['epsilon'], case['exc_pairs'])


def oracle_bonded(case, pos=None, want_forces=True):
    """(energy, forces) of the exceptions, bonds, angles and torsions of a case in free space (periodic=False), as a dict."""
    pos = case['positions'] if pos is None else pos
    out = {}
    if len(case.get('exc_pairs', ())) and 'exc_chargeprod' in case:
        out['exceptions'] = O.ljc_bonds(case['exc_pairs'], case['exc_chargeprod'], case['exc_sigma'], case['exc_epsilon'], pos, FREE_BOX,
                                        periodic=False, want_forces=want_forces)
    if len(case.get('bonds', ())):
        out['bonds'] = O.harmonic_bonds(case['bonds'], case['bond_r0'], case['bond_k'], pos, FREE_BOX, periodic=False, want_forces=want_forces)
    if len(case.get('angles', ())):
        out['angles'] = O.harmonic_angles(case['angles'], case['angle_theta0'], case['angle_k'], pos, FREE_BOX, periodic=False,
                                          want_forces=want_forces)
    if len(case.get('torsions', ())):
        out['torsions'] = O.periodic_torsions(case['torsions'], case['torsion_n'], case['torsion_phase'], case['torsion_k'], pos, FREE_BOX,
                                              periodic=False, want_forces=want_forces)
    return out
