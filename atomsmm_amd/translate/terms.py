"""Forces whose terms are lists of atoms -- bonds, angles, torsions, external terms, compound and centroid bonds, CMAP, RMSD:
bond-list terms of the hand-written kinds, or one backend force of their own carried in entry.term_ids."""
import math

import numpy as np

from .. import backend as B
from .. import expr as X
from .. import openmm as mm
from .. import tables as T
from ..utils import InputError
from .common import COMPOUND_KINDS, descriptor_of, effective, family_of, globals_update, pair_desc_from, replace_bonded

RB_TEXT = 'c0 + cp*(c1 + cp*(c2 + cp*(c3 + cp*(c4 + cp*c5)))); cp = -cos(theta)'

# (class, kind, variables, per-term names: count / name getters, rows attribute, atoms per term, what OpenMM calls a term)
_TERM_CLASSES = (('CustomBondForce', B.TERM_BOND, ('r',), 'PerBond', '_bonds', 2, 'bonds'),
                 ('CustomAngleForce', B.TERM_ANGLE, ('theta',), 'PerAngle', '_angles', 3, 'angles'),
                 ('CustomTorsionForce', B.TERM_TORSION, ('theta',), 'PerTorsion', '_torsions', 4, 'torsions'),
                 ('CustomExternalForce', B.TERM_EXTERNAL, ('x', 'y', 'z'), 'PerParticle', '_particles', 1, 'particles'))


def translate_harmonic_bond(engine, force, entry):
    b = np.array([[r[0], r[1]] for r in force._bonds], dtype=np.int32).reshape(-1, 2)
    p = np.array([[r[2], r[3]] for r in force._bonds], dtype=np.float64).reshape(-1, 2)
    entry.terms.append((B.BOND_HARMONIC, b, p, force.usesPeriodicBoundaryConditions(), None))


def translate_harmonic_angle(engine, force, entry):
    a = np.array([r[:3] for r in force._angles], dtype=np.int32).reshape(-1, 3)
    p = np.array([r[3:] for r in force._angles], dtype=np.float64).reshape(-1, 2)
    entry.terms.append((B.ANGLE_HARMONIC, a, p, force.usesPeriodicBoundaryConditions(), None))


def translate_periodic_torsion(engine, force, entry):
    t = np.array([r[:4] for r in force._torsions], dtype=np.int32).reshape(-1, 4)
    p = np.array([[r[4], r[5], r[6]] for r in force._torsions], dtype=np.float64).reshape(-1, 3)
    entry.terms.append((B.TORSION_PERIODIC, t, p, force.usesPeriodicBoundaryConditions(), None))


def translate_custom_angle(engine, force, entry):
    if force.getEnergyFunction().replace(' ', '') != '0.5*(K0*(theta-t0)^2-Kn*(theta-tn)^2)':
        return translate_term_expression(engine, force, entry)
    # difference of two harmonic angles (RESPASystem.redefine_angle, systems.py:226)
    a = np.array([r[:3] for r in force._angles], dtype=np.int32).reshape(-1, 3)
    p = np.array([r[3] for r in force._angles], dtype=np.float64).reshape(-1, 4)
    periodic = force.usesPeriodicBoundaryConditions()
    entry.terms.append((B.ANGLE_HARMONIC, a, p[:, [0, 1]], periodic, None))
    entry.terms.append((B.ANGLE_HARMONIC, a, np.stack([p[:, 2], -p[:, 3]], axis=1), periodic, None))


def translate_custom_bond(engine, force, entry):
    idx = np.array([[b[0], b[1]] for b in force._bonds], dtype=np.int32).reshape(-1, 2)
    if force.getEnergyFunction().replace(' ', '') == '0.5*(K0*(r-r0)^2-Kn*(r-rn)^2)':
        # difference of two harmonic bonds (RESPASystem.redefine_bond, systems.py:162): +K0 at r0, -Kn at rn
        par = np.array([b[2] for b in force._bonds], dtype=np.float64).reshape(-1, 4)
        periodic = force.usesPeriodicBoundaryConditions()
        entry.terms.append((B.BOND_HARMONIC, idx, par[:, [0, 1]], periodic, None))
        entry.terms.append((B.BOND_HARMONIC, idx, np.stack([par[:, 2], -par[:, 3]], axis=1), periodic, None))
        return
    if force.getEnergyFunction().replace(' ', '') == '-K*r*(r-r0)':
        # bond-stretching virial of ComputingSystem (systems.py:914): per-bond (r0, K)
        par = np.array([b[2] for b in force._bonds], dtype=np.float64).reshape(-1, 2)
        entry.terms.append((B.BOND_VIRIAL_HARMONIC, idx, par, force.usesPeriodicBoundaryConditions(), None))
        return
    if family_of(force) is None:
        return translate_term_expression(engine, force, entry)
    d = dict(descriptor_of(force))
    nb_ = force.getNumBonds()
    allp = np.array([b[2] for b in force._bonds], dtype=np.float64).reshape(nb_, -1)
    names = list(getattr(force, '_offset_parameters', []))
    base = allp[:, :3]
    scales = np.stack([allp[:, 3 * (k + 1):3 * (k + 2)] for k in range(len(names))]) if names else np.zeros((0, nb_, 3))
    periodic = force.usesPeriodicBoundaryConditions()
    if d['family'] == 'ljc':
        kind, desc = B.BOND_LJC, B.pair_desc(B.NONBONDED, 1.0, Kc=d.get('Kc', B.KC))
    elif d['family'] == 'lj-virial':
        kind, desc = B.BOND_VIRIAL_LJ, None
    else:
        for key in ('rc0', 'rs0', 'Kc'):
            if d.get(key) is None and key in engine.parameters:
                d[key] = engine.parameters[key]
        kind, desc = B.BOND_NEAR, pair_desc_from(d, d['rc0'])

    scale_name = d.get('scale_name')
    if scale_name and kind != B.BOND_NEAR:
        raise NotImplementedError('global scale factor on a bond force of this kind')

    def terms(parameters):
        dsc = desc
        if scale_name:      # respa_switch (systems.py:643, 674): the whole energy times a global parameter
            dsc = pair_desc_from(dict(d, sign=d.get('sign', 1.0) * parameters[scale_name]), d['rc0'])
        return [(kind, idx, effective(base, scales, names, parameters), periodic, dsc)]

    entry.terms = terms(engine.parameters)
    if names or scale_name:
        lam = set(names) | ({scale_name} if scale_name else set())

        def update(parameters, changed):
            if not (lam & changed):
                return False
            entry.terms = terms(parameters)
            replace_bonded(engine, entry, entry.terms)
            return True
        entry.update = update
        entry.depends = set(lam)
        # offsets on the charge product only: the energy is linear in them (energies_at_states, as for the pair forces)
        entry.charge_offsets_in = {nm for k, nm in enumerate(names) if not np.any(scales[k][:, 1:])}


def translate_term_expression(engine, force, entry):
    """A CustomBondForce / CustomAngleForce / CustomTorsionForce / CustomExternalForce whose energy text is none of the hand-written
    kinds: compiled here (expr.compile_term) and interpreted per term, with its derivative in the term's variable, by the
    term-expression kernels (csrc/term_expr.hip).  A force object of its own: no bond-list terms to merge into the group's set."""
    cls, kind, variables, per, attr, arity, what = [c for c in _TERM_CLASSES if isinstance(force, getattr(mm, c[0]))][0]
    text = force.getEnergyFunction()
    generic = '%s: energy expression not recognised as one of the hand-written kinds (%s); the generic term-expression kernel ' % (
        cls, text.split(';')[0])
    if getattr(force, '_derivs', None):
        raise NotImplementedError(generic + 'differentiates in %s only: no addEnergyParameterDerivative' % ', '.join(variables))
    if engine.world > 1:
        raise NotImplementedError(generic + 'runs on a single rank')
    periodic = bool(kind != B.TERM_EXTERNAL and force.usesPeriodicBoundaryConditions())
    if periodic and engine.free_space:
        raise InputError('%s uses periodic boundary conditions in a System in free space' % cls)
    names = [getattr(force, 'get%sParameterName' % per)(k) for k in range(getattr(force, 'getNum%sParameters' % per)())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    try:
        prog = X.compile_term(text, variables, names, gnames)
    except X.ExpressionError as exc:
        raise InputError('%s: energy expression not recognised by the HIP path as one of the hand-written kinds, and not a term '
                         'expression the generic kernel can run: %s' % (cls, exc))

    def tables():
        rows = getattr(force, attr)
        idx = np.full((len(rows), 4), -1, dtype=np.int32)
        par = np.zeros((len(names), len(rows)), dtype=np.float64)
        for t, row in enumerate(rows):
            if len(row[arity]) != len(names):
                raise mm.OpenMMException('%s: every one of the %s needs %d parameters' % (cls, what, len(names)))
            idx[t, :arity] = row[:arity]
            par[:, t] = row[arity]
        if len(rows) and (idx[:, :arity].min() < 0 or idx[:, :arity].max() >= engine.n):
            raise mm.OpenMMException('%s: a particle index is out of range' % cls)
        return idx, par

    idx, par = tables()
    tid = engine.ctx.term_expr_create(kind, prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_], idx, par,
                                      periodic=periodic)
    entry.term_ids.append(tid)
    entry.term_expr = True
    entry.program = prog

    def reload():          # updateParametersInContext: the per-term parameters are read again
        fresh_idx, fresh = tables()
        if len(fresh_idx) != len(idx):
            raise mm.OpenMMException('updateParametersInContext: the number of %s has changed' % what)
        if not np.array_equal(fresh_idx, idx):
            raise mm.OpenMMException('updateParametersInContext: the particles of the %s have changed' % what)
        engine.ctx.term_expr_set_params(tid, fresh, len(idx))
        return 'values'
    entry.reload = reload
    globals_update(entry, prog.globals_, lambda values: engine.ctx.term_expr_set_globals(tid, values))


def translate_rb(engine, force, entry):
    """An RBTorsionForce: sum_n c_n cos(psi)^n with cos(psi) = -cos(phi), lowered to the torsion text RB_TEXT with the six
    per-torsion parameters c0 .. c5 on the term-expression kernel (translate_term_expression): no kernel of its own."""
    if engine.world > 1:
        raise NotImplementedError('RBTorsionForce runs on a single rank')
    if force.usesPeriodicBoundaryConditions() and engine.free_space:
        raise InputError('RBTorsionForce uses periodic boundary conditions in a System in free space')
    text = mm.CustomTorsionForce(RB_TEXT)
    for k in range(6):
        text.addPerTorsionParameter('c%d' % k)

    def restate():
        rows = [[r[0], r[1], r[2], r[3], list(r[4:])] for r in force._torsions]
        if any(not 0 <= a < engine.n for r in rows for a in r[:4]):
            raise mm.OpenMMException('RBTorsionForce: a particle index is out of range')
        text._torsions = rows
        text.setUsesPeriodicBoundaryConditions(force.usesPeriodicBoundaryConditions())
    restate()
    translate_term_expression(engine, text, entry)
    upload = entry.reload

    def reload():          # updateParametersInContext: the coefficients are read again
        restate()
        return upload()
    entry.reload = reload


def translate_cmap(engine, force, entry):
    """A CMAPTorsionForce: every map as the 16 coefficients per cell of tables.cmap_coefficients, every torsion as a map index and
    eight atoms, evaluated with one lane per torsion by the CMAP kernels (csrc/cmap.hip).  One backend force carried in
    entry.term_ids, so every loop over an entry's forces reaches it and the scheduler's fusion rules decline its group, as they
    do for a term-expression force."""
    cls = 'CMAPTorsionForce'
    if engine.world > 1:
        raise NotImplementedError('%s runs on a single rank' % cls)
    periodic = bool(force.usesPeriodicBoundaryConditions())
    if periodic and engine.free_space:
        raise InputError('%s uses periodic boundary conditions in a System in free space' % cls)

    def tables():
        sizes = np.array([size for size, _ in force._maps], dtype=np.int32)
        coeffs = [T.cmap_coefficients(size, energy).reshape(-1) for size, energy in force._maps]
        coeffs = np.concatenate(coeffs) if coeffs else np.zeros(0)
        rows = np.array(force._torsions, dtype=np.int32).reshape(-1, 9)
        if len(rows) and (rows[:, 0].min() < 0 or rows[:, 0].max() >= len(sizes)):
            raise mm.OpenMMException('%s: a map index is out of range' % cls)
        if len(rows) and (rows[:, 1:].min() < 0 or rows[:, 1:].max() >= engine.n):
            raise mm.OpenMMException('%s: a particle index is out of range' % cls)
        return sizes, coeffs, np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1:])

    sizes, coeffs, maps, idx = tables()
    fid = engine.ctx.cmap_create(sizes, coeffs, maps, idx, periodic=periodic)
    entry.term_ids.append(fid)
    entry.cmap = fid

    def reload():          # updateParametersInContext: the maps' values and the torsions' map indices are read again
        fresh_sizes, fresh_coeffs, fresh_maps, fresh_idx = tables()
        if len(fresh_sizes) != len(sizes):
            raise mm.OpenMMException('updateParametersInContext: the number of maps has changed')
        if not np.array_equal(fresh_sizes, sizes):
            raise mm.OpenMMException('updateParametersInContext: the size of a map has changed')
        if len(fresh_idx) != len(idx):
            raise mm.OpenMMException('updateParametersInContext: the number of torsions has changed')
        if not np.array_equal(fresh_idx, idx):
            raise mm.OpenMMException('updateParametersInContext: the particles of a torsion have changed')
        engine.ctx.cmap_set_params(fid, fresh_coeffs, fresh_maps, len(sizes))
        return 'values'
    entry.reload = reload


def translate_compound(engine, force, entry):
    """A CustomCompoundBondForce or CustomCentroidBondForce: the text compiled with its variable table (expr.compile_compound) and
    evaluated with one lane per (bond, variable) by the compound-bond kernels (csrc/compound.hip).  One backend force per
    OpenMM force, carried in entry.term_ids as a term-expression force is, so every loop over an entry's forces reaches it."""
    cls = force.__class__.__name__
    centroid = isinstance(force, mm.CustomCentroidBondForce)
    n_slots = force.getNumGroupsPerBond() if centroid else force.getNumParticlesPerBond()
    if getattr(force, '_functions', None):
        raise NotImplementedError('%s: tabulated functions in the energy expression are not supported' % cls)
    if getattr(force, '_derivs', None):
        raise NotImplementedError('%s: addEnergyParameterDerivative is not supported (the compound-bond kernel differentiates in '
                                  'the geometric variables only)' % cls)
    if engine.world > 1:
        raise NotImplementedError('%s runs on a single rank' % cls)
    periodic = bool(force.usesPeriodicBoundaryConditions())
    if periodic and engine.free_space:
        raise InputError('%s uses periodic boundary conditions in a System in free space' % cls)
    names = [force.getPerBondParameterName(k) for k in range(force.getNumPerBondParameters())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    try:
        prog, variables = X.compile_compound(force.getEnergyFunction(), n_slots, 'g' if centroid else 'p', names, gnames)
    except X.ExpressionError as exc:
        raise InputError('%s: not an energy expression the compound-bond kernel can run: %s' % (cls, exc))
    kinds = [COMPOUND_KINDS[kind] for kind, _ in variables]
    slots = [list(s) for _, s in variables]

    def groups():
        masses = engine.system._masses
        ptr, atoms, weights = [0], [], []
        for g, (particles, w) in enumerate(force._groups):
            if not particles:
                raise mm.OpenMMException('%s: group %d is empty' % (cls, g))
            if min(particles) < 0 or max(particles) >= engine.n:
                raise mm.OpenMMException('%s: a particle index of group %d is out of range' % (cls, g))
            w = list(w) if len(w) else [float(masses[i]) for i in particles]
            if not (math.fsum(w) != 0.0 and math.isfinite(math.fsum(w))):
                raise mm.OpenMMException('%s: the weights of group %d sum to zero' % (cls, g))
            atoms += list(particles)
            weights += w
            ptr.append(len(atoms))
        return np.array(ptr, dtype=np.int32), np.array(atoms, dtype=np.int32), np.array(weights, dtype=np.float64)

    def tables(limit):
        rows = force._bonds
        idx = np.zeros((len(rows), n_slots), dtype=np.int32)
        par = np.zeros((len(names), len(rows)), dtype=np.float64)
        for t, (members, p) in enumerate(rows):
            if len(p) != len(names):
                raise mm.OpenMMException('%s: every bond needs %d parameters' % (cls, len(names)))
            idx[t] = members
            par[:, t] = p
        if len(rows) and (idx.min() < 0 or idx.max() >= limit):
            raise mm.OpenMMException('%s: a %s index is out of range' % (cls, 'group' if centroid else 'particle'))
        return idx, par

    grp = groups() if centroid else None
    idx, par = tables(len(grp[0]) - 1 if centroid else engine.n)
    if centroid and len(grp[0]) == 1:
        grp = None if not len(idx) else grp          # (no groups and no bonds: a force without terms)
    fid = engine.ctx.compound_create(n_slots, prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_], kinds, slots, idx, par,
                                     periodic=periodic, groups=grp)
    entry.term_ids.append(fid)
    entry.term_expr = True
    entry.program = prog
    entry.compound = dict(id=fid, variables=variables, centroid=centroid)

    def reload():          # updateParametersInContext: per-bond parameters and (centroid bonds) group weights are read again
        fresh_grp = groups() if centroid else None
        if centroid and grp is not None:
            if len(fresh_grp[0]) != len(grp[0]):
                raise mm.OpenMMException('updateParametersInContext: the number of groups has changed')
            if not (np.array_equal(fresh_grp[0], grp[0]) and np.array_equal(fresh_grp[1], grp[1])):
                raise mm.OpenMMException('updateParametersInContext: the particles of a group have changed')
        fresh_idx, fresh = tables(len(fresh_grp[0]) - 1 if centroid else engine.n)
        if len(fresh_idx) != len(idx):
            raise mm.OpenMMException('updateParametersInContext: the number of bonds has changed')
        if not np.array_equal(fresh_idx, idx):
            raise mm.OpenMMException('updateParametersInContext: the %s of a bond have changed' % ('groups' if centroid else 'particles'))
        engine.ctx.compound_set_params(fid, fresh, len(idx))
        if centroid and grp is not None:
            engine.ctx.compound_set_weights(fid, fresh_grp[2])
        return 'values'
    entry.reload = reload
    globals_update(entry, prog.globals_, lambda values: engine.ctx.compound_set_globals(fid, values))


def translate_rmsd(engine, force, entry):
    """An RMSDForce: the selected particles and the reference rows of those particles go to the RMSD kernels (csrc/rmsd.hip), which
    centre the reference, fit and differentiate.  One backend force carried in entry.term_ids, so every loop over an entry's forces
    reaches it and the scheduler's fusion rules decline its group, as they do for a term-expression force.  (Also an inner force
    of a CustomCVForce.)  It reads no parameter: deriv(energy, p) sees no dependence through it."""
    cls = 'RMSDForce'
    if engine.world > 1:
        raise NotImplementedError('%s runs on a single rank' % cls)
    n = engine.n

    def tables():
        reference = np.array(force._reference, dtype=np.float64).reshape(-1, 3)
        if len(reference) != n:
            raise mm.OpenMMException('%s: %d reference positions, the System has %d particles' % (cls, len(reference), n))
        particles = force.getParticles() or list(range(n))
        if min(particles) < 0 or max(particles) >= n:
            raise mm.OpenMMException('%s: a particle index is out of range' % cls)
        if len(set(particles)) != len(particles):
            raise mm.OpenMMException('%s: a particle is listed twice' % cls)
        if not np.isfinite(reference).all():
            raise mm.OpenMMException('%s: a reference position is not finite' % cls)
        particles = np.array(particles, dtype=np.int32)
        return particles, np.ascontiguousarray(reference[particles])

    fid = engine.ctx.rmsd_create(*tables())
    entry.term_ids.append(fid)
    entry.rmsd = fid

    def reload():          # updateParametersInContext: the reference and the particle list are read again
        engine.ctx.rmsd_set_reference(fid, *tables())
        return 'values'
    entry.reload = reload
