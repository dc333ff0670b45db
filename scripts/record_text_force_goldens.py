#!/usr/bin/env python3
"""Cases and goldens of tests/test_gpu_text_force_bits.py: what the force families that evaluate a user-written energy text compute
must not depend on where their shared pieces are written down (csrc/expr_force.h: the program holder, the variable table, the CSR
builders, the staging of program and table into LDS, the search of an exclusion row; csrc/device_utils.h: the block reduction of the
energy and the write of a force row).  These kernels use no atomics and keep fp contraction off, so the same inputs give the same bits.

    python scripts/record_text_force_goldens.py [--out DIR] [case ...]     # on a GPU, with the library that sets the standard

writes tests/golden/text_force_<case>.npz (or DIR/...): `positions` [n][3], and of three evaluations of the case's force through
HipContext.force_eval -- with the energy, without it, and with the energy accumulating onto a buffer that holds numbers -- `energy`
[3] (0 where none was asked for) and `forces` [3][n][3], all float64.  The files in the repository were recorded by the build of the
commit BEFORE csrc/expr_force.h; the test asks for the same bits.  Nothing here calls more than the public methods of
backend.HipContext and the OpenMM-shaped classes over them, so the file runs unchanged against that build (AMM_LIB names it).

The cases are the smallest shapes at which each shared piece can go wrong; texts and layouts come from the case modules of the tests
(tests/*_cases.py).  CASES maps a name to a function that returns (HipContext, force id, positions, keep-alive)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EDGE = 2.0
BOX = np.full(3, EDGE)


def golden_path(name, where=GOLDEN):
    return os.path.join(where, 'text_force_%s.npz' % name.replace(' ', '_'))


# ------------------------------------------------------------------------------------------------ helpers
def _mods():
    import compound_cases as C
    import hbond_cases as H
    import manyparticle_cases as M
    import term_expr_cases as TE
    import cmap_cases as CM
    from atomsmm_amd import backend as B
    from atomsmm_amd import expr as X
    from atomsmm_amd import openmm, unit
    from atomsmm_amd import tables as T
    return dict(C=C, H=H, M=M, TE=TE, CM=CM, B=B, X=X, openmm=openmm, unit=unit, T=T)


def scattered(n, seed, edge=EDGE, closest=0.12):
    """n points in the cube of `edge`, no two closer than `closest` under the minimum image."""
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3))
    for t in range(n):
        while True:
            x = rng.uniform(0.0, edge, 3)
            d = pos[:t] - x
            d -= edge * np.rint(d / edge)
            if not t or np.sqrt((d ** 2).sum(axis=1)).min() >= closest:
                break
        pos[t] = x
    return pos


def through_a_context(force, positions, box=None, options=None, parameters=None):
    """The force alone in a System; -> (HipContext, its backend id, positions, the Context that owns them)."""
    m = _mods()
    openmm, unit = m['openmm'], m['unit']
    system = openmm.System()
    for _ in range(len(positions)):
        system.addParticle(12.0)
    if box is not None:
        system.setDefaultPeriodicBoxVectors((float(box[0]), 0, 0), (0, float(box[1]), 0), (0, 0, float(box[2])))
    system.addForce(force)
    props = {'Option.' + k: str(v) for k, v in (options or {}).items()}
    context = openmm.Context(system, openmm.VerletIntegrator(0.001), openmm.Platform.getPlatformByName('HIP'), props)
    context.setPositions(np.asarray(positions) * unit.nanometers)
    for name, value in (parameters or {}).items():          # (set_globals, then the evaluation)
        context.setParameter(name, value)
    engine = context._engine
    return engine.ctx, engine.entries[0].term_ids[-1], np.asarray(positions, dtype=np.float64), context


def evaluations(ctx, fid, positions):
    """-> (energy [3], forces [3][n][3]): with the energy, without it, with the energy and accumulating."""
    import torch

    def dev(a):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')
    n = len(positions)
    start = np.random.default_rng(5).normal(size=(n, 3)) * 100.0
    energy, forces = np.zeros(3), np.zeros((3, n, 3))
    pos = dev(positions)
    for k, (with_energy, accumulate) in enumerate(((True, False), (False, False), (True, True))):
        f = dev(start if accumulate else np.full((n, 3), 7.0))       # (a buffer that holds numbers: every row must be written)
        e = torch.zeros(1, dtype=torch.float64, device='cuda') if with_energy else None
        ctx.force_eval(fid, pos, f, accumulate=accumulate, energy=e)
        ctx.synchronize()
        energy[k] = e.item() if with_energy else 0.0
        forces[k] = f.cpu().numpy()
    ctx.check()
    return energy, forces


# ------------------------------------------------------------------------------------------------ term expressions
N_TERM_ATOMS = 300
TERM_TEXT = dict(bond='morse', angle='cosine-angle', torsion='rb-torsion', external='wall')


def term_case(which, n_terms=257):
    """257 terms: two blocks, the second holds one term.  Atom 0 is in the first five terms: the gather's four records in flight and a
    remainder.  n_terms = 0: the force still writes its rows."""
    def make():
        m = _mods()
        TE, B, X = m['TE'], m['B'], m['X']
        case = TE.TEXTS[TERM_TEXT[which]]
        arity = TE.ARITY[case['kind']]
        rng = np.random.default_rng(100 + arity)
        k = np.arange(N_TERM_ATOMS)
        pos = np.stack([0.2 + 0.13 * (k % 12), 0.3 + 0.11 * (k // 12 % 5), 0.2 + 0.07 * (k // 60)], axis=1) + rng.uniform(-0.03, 0.03, (N_TERM_ATOMS, 3))
        rows = np.full((n_terms, 4), -1, dtype=np.int32)
        for t in range(n_terms):
            rows[t, :arity] = ([0, 1 + t, 7 + t, 13 + t] if t < 5 else [(t + 6 * j) % N_TERM_ATOMS for j in range(4)])[:arity]
        ranges = dict(D=(1.0, 20.0), a=(8.0, 20.0), r0=(0.1, 0.3), theta0=(1.5, 2.2), k=(10.0, 100.0), m=(1.0, 16.0))
        par = np.array([[rng.uniform(*ranges.get(p, (0.5, 2.0))) for _ in range(n_terms)] for p in case['names']]).reshape(len(case['names']), n_terms)
        g = dict(case['globals'])
        prog = X.compile_term(case['text'], TE.VARIABLES[case['kind']], case['names'], g)
        ctx = B.HipContext(N_TERM_ATOMS, BOX)
        fid = ctx.term_expr_create(case['kind'], prog.code, prog.consts, [g[q] for q in prog.globals_], rows, par, periodic=which == 'torsion')
        return ctx, fid, pos, None
    return make


# ------------------------------------------------------------------------------------------------ compound and centroid bonds
COMPOUND_RANGES = dict(r0=(0.3, 0.9), r1=(0.3, 0.9), r2=(0.3, 0.9), t0=(1.2, 2.2), phi=(-3.0, 3.0), dx=(-0.2, 0.2), d0=(0.3, 0.9))


def compound_force(name, rows, params, periodic, text=None, names=None):
    m = _mods()
    case = m['C'].TEXTS[name]
    force = m['openmm'].CustomCompoundBondForce(case['n'], text or case['text'])
    for p in (case['names'] if names is None else names):
        force.addPerBondParameter(p)
    for g, value in (case['globals'] if text is None else {}).items():
        force.addGlobalParameter(g, value)
    for members, row in zip(rows, params):
        force.addBond([int(a) for a in members], [float(v) for v in row])
    force.setUsesPeriodicBoundaryConditions(periodic)
    return force


def compound_rows(name, n_bonds, seed, names=None):
    """(positions of 40 scattered atoms, bonds over distinct atoms drawn from them -- many reach across a face --, parameter rows)."""
    case = _mods()['C'].TEXTS[name]
    rng = np.random.default_rng(seed)
    pos = scattered(40, seed)
    rows = [rng.choice(40, size=case['n'], replace=False) for _ in range(n_bonds)]
    names = case['names'] if names is None else names
    params = [[rng.uniform(*COMPOUND_RANGES.get(p, (5.0, 50.0))) for p in names] for _ in range(n_bonds)]
    return pos, rows, params


def compound_case(name, periodic, n_bonds=17, text=None, names=None, parameters=None):
    """17 bonds: two blocks at V = 16 (16 bonds per block), a padding lane per bond at V = 3."""
    def make():
        pos, rows, params = compound_rows(name, n_bonds, 7 + len(name), names)
        return through_a_context(compound_force(name, rows, params, periodic, text, names), pos, BOX, parameters=parameters)
    return make


def centroid_case():
    """Group 0 has 65 members (a second lane-strided turn of its wavefront); atom 3 belongs to groups 0 and 1."""
    m = _mods()
    case = m['C'].TEXTS['centre-angle']
    pos = scattered(80, 77, closest=0.1)
    rng = np.random.default_rng(78)
    groups = [(list(range(65)), rng.uniform(1.0, 16.0, 65)), ([3, 66, 67, 68], rng.uniform(1.0, 16.0, 4)), ([70, 71, 72, 73, 74], None),
              ([75, 76], rng.uniform(1.0, 16.0, 2))]
    force = m['openmm'].CustomCentroidBondForce(case['n'], case['text'])
    for p in case['names']:
        force.addPerBondParameter(p)
    for g, value in case['globals'].items():
        force.addGlobalParameter(g, value)
    for atoms, weights in groups:
        force.addGroup([int(a) for a in atoms], [] if weights is None else [float(w) for w in weights])
    force.addBond([0, 1, 2], [30.0, 1.9])
    force.addBond([1, 3, 0], [20.0, 1.4])
    force.setUsesPeriodicBoundaryConditions(False)
    return through_a_context(force, pos, BOX)


# ------------------------------------------------------------------------------------------------ collective variables
N_CV_ATOMS = 342        # 3 n = 1026 doubles: a block of k_cv_apply combines 256 x 4, the second block holds the last two


def cv_case(inner_kind, two):
    """K = 1, P = 0 (the text cv1 alone) or K = 2, P = 1 over inner forces of one kind; with two, a global is set before the evaluation."""
    def make():
        m = _mods()
        openmm = m['openmm']
        n = N_CV_ATOMS
        k = np.arange(n)
        rng = np.random.default_rng(11)
        pos = np.stack([0.1 + 0.005 * k, 1.0 + 0.05 * np.sin(0.9 * k), 1.0 + 0.05 * np.cos(1.3 * k)], axis=1) + rng.uniform(-0.001, 0.001, (n, 3))

        def inner(j):
            step = 1 + j
            if inner_kind == 'bonded':
                force = openmm.HarmonicBondForce()
                for i in range(n - step):
                    force.addBond(i, i + step, 0.05 + 0.004 * j, 800.0 + 37.0 * j)
            elif inner_kind == 'term':
                force = openmm.CustomBondForce('D*(1-exp(-a*(r-r0)))^2')
                for p in ('D', 'a', 'r0'):
                    force.addPerBondParameter(p)
                for i in range(n - step):
                    force.addBond(i, i + step, [4.0 + j, 9.0, 0.05 + 0.004 * j])
            else:
                force = openmm.CustomCompoundBondForce(3, '0.5*k*(angle(p1,p2,p3)-t0)^2 + 0.5*kub*(distance(p1,p3)-d0)^2')
                for p in ('t0', 'k', 'd0', 'kub'):
                    force.addPerBondParameter(p)
                for i in range(0, n - 2 * step, 3):
                    force.addBond([i, i + step, i + 2 * step], [2.0, 40.0 + j, 0.01 * step, 300.0])
            return force
        if two:
            outer = openmm.CustomCVForce('0.5*K*(a-a0)^2 + lam*b + 0.01*a*b')
            outer.addCollectiveVariable('a', inner(0))
            outer.addCollectiveVariable('b', inner(1))
            outer.addGlobalParameter('K', 0.002)
            outer.addGlobalParameter('a0', 3.0)
            outer.addGlobalParameter('lam', 0.3)
            outer.addEnergyParameterDerivative('lam')
            return through_a_context(outer, pos, BOX, parameters=dict(K=0.003))
        outer = openmm.CustomCVForce('a')
        outer.addCollectiveVariable('a', inner(0))
        return through_a_context(outer, pos, BOX)
    return make


# ------------------------------------------------------------------------------------------------ hydrogen bonds
METHODS = dict(NoCutoff=0, CutoffNonPeriodic=1, CutoffPeriodic=2)


def hbond_case(name, D, A, method='NoCutoff', cutoff=0.9, options=None, exclusions=None, no_third=False, seed=21, edge=EDGE):
    def make():
        m = _mods()
        H, openmm, unit = m['H'], m['openmm'], m['unit']
        case = H.TEXTS[name]
        pos, donors, acceptors = H.layout(D, A, edge, seed)
        if no_third:
            donors[:, 2] = -1
        if not len(pos):
            pos = scattered(4, seed)
        force = openmm.CustomHbondForce(case['text'])
        for p in case['dnames']:
            force.addPerDonorParameter(p)
        for p in case['anames']:
            force.addPerAcceptorParameter(p)
        for g, value in case['globals'].items():
            force.addGlobalParameter(g, value)
        for members, row in zip(donors, H.parameters(name, D, 'd', seed)):
            force.addDonor(int(members[0]), int(members[1]), int(members[2]), [float(v) for v in row])
        for members, row in zip(acceptors, H.parameters(name, A, 'a', seed)):
            force.addAcceptor(int(members[0]), int(members[1]), int(members[2]), [float(v) for v in row])
        for d, a in (exclusions or ()):
            force.addExclusion(int(d), int(a))
        force.setNonbondedMethod(METHODS[method])
        force.setCutoffDistance(cutoff * unit.nanometers)
        return through_a_context(force, pos, np.full(3, edge), options)
    return make


# donor 0 keeps all its acceptors, donor 1 loses the first and the last 69 of them (the search reaches both ends of its list), donor 2 one
HB_EXCLUSIONS = [(1, 0)] + [(1, a) for a in range(60, 129)] + [(2, 64)]


# ------------------------------------------------------------------------------------------------ many-particle sets
MODES = dict(single=0, central=1)


def many_case(name, n, mode='single', method='NoCutoff', cutoff=0.7, types=None, filters=None, exclusions=(), periodic_layout=False):
    def make():
        m = _mods()
        M, openmm, unit = m['M'], m['openmm'], m['unit']
        case = M.TEXTS[name]
        if periodic_layout:
            pos = M.small_layout(n, True)
        else:
            pos = M.positions(n, EDGE, 3 + n, 0.2, lambda rng, t: M.ball(rng, np.full(3, 0.5 * EDGE), 0.3))
        par = M.parameters(name, n, 9)
        force = openmm.CustomManyParticleForce(3, case['text'])
        for p in case['names']:
            force.addPerParticleParameter(p)
        for g, value in case['globals'].items():
            force.addGlobalParameter(g, value)
        for k in range(n):
            force.addParticle([float(v) for v in par[k]], 0 if types is None else int(types[k]))
        for a, b in exclusions:
            force.addExclusion(int(a), int(b))
        for r, allowed in enumerate(filters or ()):
            force.setTypeFilter(r, allowed)
        force.setNonbondedMethod(METHODS[method])
        force.setPermutationMode(MODES[mode])
        force.setCutoffDistance(cutoff * unit.nanometers)
        return through_a_context(force, pos, BOX)
    return make


def many_empty():
    """A force without particles in a context of four atoms: without accumulate the zeroing kernel writes the rows."""
    m = _mods()
    B, X, M = m['B'], m['X'], m['M']
    case = M.TEXTS['three']
    prog, variables = X.compile_many_particle(case['text'], 3, [], list(case['globals']))
    kinds = [dict(x=B.CVAR_X, y=B.CVAR_Y, z=B.CVAR_Z, distance=B.CVAR_DISTANCE, angle=B.CVAR_ANGLE, dihedral=B.CVAR_DIHEDRAL)[k] for k, _ in variables]
    ctx = B.HipContext(4, None)
    fid = ctx.many_create(prog.code, prog.consts, [case['globals'][g] for g in prog.globals_], kinds, [list(s) for _, s in variables],
                          np.zeros((0, 0)), [], 1, [0])
    return ctx, fid, scattered(4, 1), None


# ------------------------------------------------------------------------------------------------ pair expression, CMAP
def pair_expr_case(tables):
    """65 atoms on a line (tests/test_gpu_pair_expr.py), a Yukawa text -- or a text over two tabulated functions."""
    def make():
        m = _mods()
        B, X, T = m['B'], m['X'], m['T']
        n = 65
        rng = np.random.default_rng(3)
        pos = np.stack([0.1 + 0.02 * np.arange(n) + rng.uniform(-0.002, 0.002, n), np.full(n, 1.0), np.full(n, 2.0)], axis=1)
        ctx = B.HipContext(n, np.full(3, 4.0))
        desc = B.pair_desc(B.PAIR_EXPR, 0.9)
        if tables:
            prog = X.compile_pair('g(t1,t2)*U(r)', ['t'], [], {'U': ('Continuous1D', 1), 'g': ('Discrete2D', 2)})
            fid = ctx.pair_expr_create(desc, prog.code, prog.consts, [], (np.arange(n) % 2).astype(np.float64), None, None)
            u = (T.CONTINUOUS1D, 3, 1, 0.0, 1.0, T.spline_coefficients([4.0, 2.0, 1.0], 0.0, 1.0).reshape(-1))
            g2 = (T.DISCRETE2D, 2, 2, 0.0, 0.0, np.array([1.0, 2.0, 2.0, 3.0]))
            ctx.pair_expr_set_tables(fid, [u, g2])
        else:
            prog = X.compile_pair('q1*q2*exp(-b*r)/r', ['q'], ['b'])
            fid = ctx.pair_expr_create(desc, prog.code, prog.consts, [2.5], rng.uniform(0.5, 1.5, n), None, None)
        return ctx, fid, pos, None
    return make


def cmap_case():
    """257 terms along a chain of 261 atoms (tests/cmap_cases.py: backbone), maps of sizes 5 and 24: two blocks, the second holds one
    term; an inner atom is in eight records."""
    m = _mods()
    CM, openmm = m['CM'], m['openmm']
    pos, terms = CM.backbone(261, seed=5)
    force = openmm.CMAPTorsionForce()
    for size, seed in ((5, 21), (24, 22)):
        force.addMap(*CM.random_map(size, seed))
    for row in terms:
        force.addTorsion(*[int(v) for v in row])
    force.setUsesPeriodicBoundaryConditions(False)
    return through_a_context(force, pos, np.full(3, 6.0))


CASES = {
    'term bond': term_case('bond'), 'term angle': term_case('angle'), 'term torsion': term_case('torsion'), 'term external': term_case('external'),
    'term none': term_case('bond', 0),
    'compound v0': compound_case('harmonic-bond', False, text='2.5*k + r0', names=['r0', 'k']),
    'compound v1': compound_case('harmonic-bond', False), 'compound v1 periodic': compound_case('harmonic-bond', True),
    'compound v3': compound_case('stretch-bend', False), 'compound v3 periodic': compound_case('stretch-bend', True),
    'compound v3 globals': compound_case('stretch-bend', True, parameters=dict(scale=1.75)),
    'compound v16': compound_case('sixteen', False), 'compound v16 periodic': compound_case('sixteen', True),
    'centroid': centroid_case,
    'cv one bonded': cv_case('bonded', False), 'cv one term': cv_case('term', False), 'cv one compound': cv_case('compound', False),
    'cv two bonded': cv_case('bonded', True), 'cv two term': cv_case('term', True), 'cv two compound': cv_case('compound', True),
    'hbond 1x1': hbond_case('three', 1, 1), 'hbond 2x65': hbond_case('three', 2, 65), 'hbond 2x65 v16': hbond_case('sixteen', 2, 65),
    'hbond 3x129 chunks1': hbond_case('three', 3, 129, options=dict(hbond_chunks=1)),
    'hbond 3x129 chunks2': hbond_case('three', 3, 129, options=dict(hbond_chunks=2)),
    'hbond exclusions': hbond_case('three', 3, 129, exclusions=HB_EXCLUSIONS),
    'hbond no third': hbond_case('distance-angle', 3, 129, no_third=True),
    'hbond cutoff': hbond_case('three', 3, 129, 'CutoffNonPeriodic', 0.9), 'hbond periodic': hbond_case('three', 3, 129, 'CutoffPeriodic', 0.9),
    'hbond cutoff batches': hbond_case('three', 3, 129, 'CutoffNonPeriodic', 0.9, options=dict(hbond_compact=0)),
    'hbond periodic batches': hbond_case('parameters', 3, 129, 'CutoffPeriodic', 0.9, options=dict(hbond_compact=0)),
    'hbond no donors': hbond_case('three', 0, 5),
    'many 3': many_case('three', 3), 'many 5': many_case('three', 5), 'many 13': many_case('three', 13), 'many 13 v16': many_case('sixteen', 13),
    'many 5 central': many_case('three', 5, 'central'), 'many 13 central': many_case('parameters', 13, 'central'),
    'many types': many_case('three', 13, types=[k % 2 for k in range(13)], filters=[{0}, set(), set()]),
    'many exclusion': many_case('three', 13, exclusions=[(2, 7)]),
    'many periodic': many_case('three', 6, method='CutoffPeriodic', periodic_layout=True),
    'many periodic central': many_case('three', 6, 'central', 'CutoffPeriodic', periodic_layout=True),
    'many none': many_empty,
    'pair expr': pair_expr_case(False), 'pair expr tables': pair_expr_case(True),
    'cmap 257': cmap_case,
}


def run_case(name):
    """-> (positions, energy [3], forces [3][n][3]) of case `name` on the library that is loaded."""
    ctx, fid, positions, keep = CASES[name]()
    try:
        energy, forces = evaluations(ctx, fid, positions)
    finally:
        if keep is None:
            ctx.close()
    return positions, energy, forces


if __name__ == '__main__':
    import torch
    assert torch.cuda.is_available(), 'needs a GPU'          # (before the library is loaded: torch brings its own HIP runtime)
    from atomsmm_amd import backend
    print('kernel revision', backend.kernel_revision(), 'library', backend.LIB_PATH)
    args = sys.argv[1:]
    where = GOLDEN
    if args and args[0] == '--out':
        where = args[1]
        args = args[2:]
    os.makedirs(where, exist_ok=True)
    for name in (args or list(CASES)):
        positions, energy, forces = run_case(name)
        path = golden_path(name, where)
        np.savez_compressed(path, positions=positions, energy=energy, forces=forces)
        print('%-24s %5.1f KB  n = %4d  E = %s  max|F| = %.6g' % (name, os.path.getsize(path) / 1024.0, len(positions), energy, np.abs(forces[0]).max()), flush=True)
        assert np.all(np.isfinite(energy)) and np.all(np.isfinite(forces)), name
        if not np.array_equal(forces[0], forces[1]):
            print('    (the forces with and without the energy differ in their last bits)', flush=True)
