"""The one table of force classes, and everything that is a loop over it: the dispatch of a System force (translate), of the inner
force of a collective variable (translate_cv_general), the refusals made when a Context is created (check_system), those of
deriv(energy, p) (refuse_derivative) and the decision between free space and a periodic box (free_space_mode)."""
from collections import namedtuple

from .. import expr as X
from .. import openmm as mm
from ..utils import InputError
from . import allpairs as A
from . import pair as P
from . import terms as M
from .common import _Entry, finish_entry, make_bonded, register_globals

# One row per OpenMM class, or per tuple of classes that share a translator, in the order in which a force is matched and in which
# the refusals of check_system fire:
#   classes      the OpenMM classes;
#   translate    translate(engine, force, entry);
#   attr         the _Entry attribute that carries the backend id or dict of such a force (None: pair_ids / terms only);
#   cv_inner     a bond-list class: may be a collective variable of a general CustomCVForce;
#   pair         counts as a pair force when free space or a periodic box is decided;  free_only: ... and runs in free space only;
#   single_rank  (exception type, sentence) refused with more than one rank when the Context is created -- the classes whose only
#                single-rank refusal is their translator's have None here: theirs fires later, at the force's turn;
#   deriv        the end of the sentence that refuses deriv(energy, p) through such a force, or None;
#   max_atoms    (limit, sentence with the limit and the System's count): the force has the System's particles, at most that many;
#   check        check(force) of every such force, ahead of the refusals above;
#   before / after    before(engine, forces) -- even without such a force -- and after(engine, system, integrator, forces): what is
#                genuinely particular to the class.
Row = namedtuple('Row', 'classes translate attr cv_inner pair free_only single_rank deriv max_atoms check before after',
                 defaults=(None, False, False, False, None, None, None, None, None, None))


def translate_cv(engine, force, entry):
    """A CustomCVForce: the pattern of AlchemicalRespaSystem -- ONE collective variable, the energy of a CustomNonbondedForce -- is
    that pair force with an overall factor; any other takes the general path."""
    if force.getNumCollectiveVariables() != 1 or not isinstance(force.getCollectiveVariable(0), mm.CustomNonbondedForce) or \
            getattr(force, '_functions', None):
        return translate_cv_general(engine, force, entry)
    P.translate_scaled_pair_cv(engine, force, entry)


FORCE_TABLE = (
    Row((mm.NonbondedForce,), P.translate_nonbonded, pair=True),
    Row((mm.CustomNonbondedForce,), P.translate_custom_nonbonded, pair=True),
    Row((mm.CustomCVForce,), translate_cv, 'cv'),
    Row((mm.GBSAOBCForce,), A.translate_gb, 'gb', pair=True, free_only=True,
        single_rank=(InputError, 'a GBSAOBCForce runs on a single rank: its passes walk all pairs and are not sliced'),
        deriv='is not supported: the generalized-Born kernels have no parameter-derivative evaluation',
        max_atoms=(A.GB_MAX_ATOMS, 'a GBSAOBCForce walks all n^2 pairs three times per evaluation and takes at most %d atoms (the System '
                                   'has %d)')),
    Row((mm.CustomGBForce,), A.translate_custom_gb, 'custom_gb', pair=True, free_only=True,
        single_rank=(InputError, 'a CustomGBForce runs on a single rank: its passes walk all pairs and are not sliced'),
        deriv='is not supported: the custom generalized-Born kernels have no parameter-derivative evaluation',
        max_atoms=(A.GB_MAX_ATOMS, 'a CustomGBForce walks all n^2 pairs up to three times per evaluation and takes at most %d atoms (the '
                                   'System has %d)'),
        check=A.check_custom_gb_force),
    Row((mm.CustomHbondForce,), A.translate_hbond, 'hbond',
        single_rank=(InputError, 'a CustomHbondForce runs on a single rank: its passes walk all donor-acceptor pairs and are not sliced'),
        deriv='is not supported: the hydrogen-bond kernel differentiates in the geometric variables only'),
    Row((mm.CustomManyParticleForce,), A.translate_many_particle, 'many',
        single_rank=(InputError, 'a CustomManyParticleForce runs on a single rank: its wavefronts walk the neighbours of every particle '
                                 'and are not sliced'),
        deriv='is not supported: the many-particle kernel differentiates in the geometric variables only'),
    Row((mm.GayBerneForce,), A.translate_gayberne, 'gayberne',
        single_rank=(InputError, 'a GayBerneForce runs on a single rank: its wavefronts walk all pairs of ellipsoids and are not sliced')),
    Row((mm.DrudeForce,), A.translate_drude, 'drude',
        single_rank=(InputError, 'a DrudeForce runs on a single rank: its springs and screened pairs are not sliced'),
        before=A.check_drude_integrator, after=A.check_drude_system),
    Row((mm.CMAPTorsionForce,), M.translate_cmap, 'cmap'),
    Row((mm.RBTorsionForce,), M.translate_rb),
    # the bond-list classes, in the order in which a CustomCVForce names them
    Row((mm.HarmonicBondForce,), M.translate_harmonic_bond, cv_inner=True),
    Row((mm.HarmonicAngleForce,), M.translate_harmonic_angle, cv_inner=True),
    Row((mm.PeriodicTorsionForce,), M.translate_periodic_torsion, cv_inner=True),
    Row((mm.CustomBondForce,), M.translate_custom_bond, cv_inner=True),
    Row((mm.CustomAngleForce,), M.translate_custom_angle, cv_inner=True),
    Row((mm.CustomTorsionForce, mm.CustomExternalForce), M.translate_term_expression, cv_inner=True),
    Row((mm.CustomCompoundBondForce, mm.CustomCentroidBondForce), M.translate_compound, 'compound', cv_inner=True),
    Row((mm.RMSDForce,), M.translate_rmsd, 'rmsd', cv_inner=True),
)
CV_INNER_CLASSES = tuple(cls.__name__ for row in FORCE_TABLE if row.cv_inner for cls in row.classes)


def row_of(force):
    return next((row for row in FORCE_TABLE if isinstance(force, row.classes)), None)


def translate(engine, force):
    """One force of the System becomes an entry of engine.entries (a CMMotionRemover: nothing; a MonteCarloBarostat: engine.barostat)."""
    register_globals(engine, force)
    if isinstance(force, mm.CMMotionRemover):
        return
    if isinstance(force, mm.MonteCarloBarostat):
        if engine.free_space:
            raise InputError('a MonteCarloBarostat needs a periodic box: a System in free space (NoCutoff / CutoffNonPeriodic) has '
                             'no volume to change')
        if engine.barostat is not None:
            raise InputError('a System holds one MonteCarloBarostat at most')
        engine.barostat = force       # no energy of its own: it drives Engine.step (_barostat_attempt)
        engine.parameters[force.Pressure()] = force.getDefaultPressure()._value
        engine.parameters[force.Temperature()] = force.getDefaultTemperature()._value
        return
    row = row_of(force)
    if row is None:
        raise InputError('force type {} is not supported by the HIP path'.format(force.__class__.__name__))
    entry = _Entry(force, force.getForceGroup())
    row.translate(engine, force, entry)
    finish_entry(engine, entry)
    engine.entries.append(entry)


def translate_cv_general(engine, force, entry):
    """CustomCVForce with any energy text over several collective variables, each the energy of a bond / angle / torsion / external
    force: one backend object (csrc/cv.hip, AMM_FORCE_CV) that owns the compiled outer text (expr.compile_cv) and the ids of the
    inner forces -- bond-list sets for the hand-written kinds, term-expression forces for any other text, members of no group.
    Its id goes into entry.term_ids, so every loop over an entry's forces reaches it; entry.cv names it, its collective
    variables and the parameters it differentiates in."""
    cls = 'CustomCVForce'
    n_cv = force.getNumCollectiveVariables()
    if engine.world > 1:
        raise NotImplementedError('%s with a general energy expression (%d collective variables) runs on a single rank' % (cls, n_cv))
    if getattr(force, '_functions', None):
        raise NotImplementedError('%s: tabulated functions in the energy expression of collective variables are not supported' % cls)
    if n_cv < 1:
        raise InputError('%s without a collective variable' % cls)
    text = force.getEnergyFunction()
    names = [force.getCollectiveVariableName(k) for k in range(n_cv)]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    derivs = list(dict.fromkeys(getattr(force, '_derivs', ())))
    for p in derivs:
        if p not in gnames:
            raise InputError('%s: addEnergyParameterDerivative(%r) names no global parameter of the force' % (cls, p))
    inners = [force.getCollectiveVariable(k) for k in range(n_cv)]
    for name, inner in zip(names, inners):
        row = row_of(inner)
        if row is None or not row.cv_inner:
            raise NotImplementedError('%s over a %s (collective variable %s): outside the pattern of AlchemicalRespaSystem, a collective '
                                      'variable is the energy of one of %s' % (cls, inner.__class__.__name__, name, ', '.join(CV_INNER_CLASSES)))
        if hasattr(inner, 'getEnergyFunction'):
            inner_globals = {inner.getGlobalParameterName(k) for k in range(inner.getNumGlobalParameters())}
            shared = sorted(set(derivs) & inner_globals & X.symbols(inner.getEnergyFunction()))
            if shared:
                raise NotImplementedError('%s: the derivative parameter %s is also read by the energy expression of collective variable %s; '
                                          'parameter derivatives through inner forces are not supported' % (cls, shared[0], name))
    try:
        prog = X.compile_cv(text, names, derivs, gnames)
    except X.ExpressionError as exc:
        raise InputError('%s: not an energy expression the collective-variable kernel can run: %s' % (cls, exc))
    subs, inner_ids = [], []
    for name, inner in zip(names, inners):
        register_globals(engine, inner)
        sub = _Entry(inner, entry.group)
        row_of(inner).translate(engine, inner, sub)
        finish_entry(engine, sub)
        ids = ([sub.bonded_id] if sub.bonded_id is not None else []) + sub.term_ids
        if not ids:          # (a force without terms: an empty bond-list set, energy 0)
            sub.bonded_id = make_bonded(engine, [], sliced=False)
            ids = [sub.bonded_id]
        if sub.update is not None and not sub.term_expr:
            raise NotImplementedError('%s: collective variable %s is a %s whose bond-list terms are rebuilt when a global parameter '
                                      'changes' % (cls, name, inner.__class__.__name__))
        subs.append(sub)
        inner_ids.append(ids[0])
    cid = engine.ctx.cv_create(inner_ids, len(derivs), prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_])
    if derivs:
        engine.ctx.cv_set_variables(cid, [engine.parameters[p] for p in derivs])
    entry.term_ids.append(cid)
    entry.program = prog
    entry.cv = dict(id=cid, names=names, derivs=derivs, inner=subs, inner_ids=inner_ids)
    outer, seeded = set(prog.globals_), set(derivs)

    def update(parameters, changed):
        hit = False
        if outer & changed:
            engine.ctx.cv_set_globals(cid, [parameters[g] for g in prog.globals_])
            hit = True
        if seeded & changed:
            engine.ctx.cv_set_variables(cid, [parameters[p] for p in derivs])
            hit = True
        for sub in subs:
            if sub.update is not None and sub.update(parameters, changed):
                hit = True
        return 'values' if hit else False
    entry.update = update
    entry.depends = outer | seeded | set().union(*[sub.depends for sub in subs])
    reloads = [sub.reload for sub in subs if getattr(sub, 'reload', None) is not None]
    if reloads:
        def reload():          # updateParametersInContext: the inner forces that can read their per-term parameters again
            for one in reloads:
                one()
            return 'values'
        entry.reload = reload


def derivative_refusal(row, what, step=None):
    cls = row.classes[0].__name__
    return NotImplementedError('deriv(energy, %s) through a %s %s' % (what, cls, row.deriv)
                               + (' (step: %s)' % step if step is not None else ''))


def refuse_derivative(engine, name):
    """deriv(energy, name) in a Context that holds a force whose kernels have no parameter-derivative evaluation."""
    for row in FORCE_TABLE:
        if row.deriv and any(getattr(entry, row.attr, None) is not None for entry in engine.entries):
            raise derivative_refusal(row, name)


def check_system(engine, system, integrator):
    """What the classes of the table cannot run with, refused by name when the Context is created and in the table's order
    (CutoffPeriodic and box-periodic companions of a generalized-Born force: free_space_mode; texts and other limits: the
    translators)."""
    n = system.getNumParticles()
    for row in FORCE_TABLE:
        forces = [f for f in system.getForces() if isinstance(f, row.classes)]
        if row.before:
            row.before(engine, forces)
        if not forces:
            continue
        cls = row.classes[0].__name__
        for force in forces:
            if row.max_atoms and force.getNumParticles() != n:
                raise mm.OpenMMException('%s must have exactly as many particles as the System it belongs to (%d, the System has %d)'
                                         % (cls, force.getNumParticles(), n))
            if row.check:
                row.check(force)
        if engine.world > 1 and row.single_rank:
            raise row.single_rank[0](row.single_rank[1])
        if row.max_atoms and n > row.max_atoms[0]:
            raise InputError(row.max_atoms[1] % (row.max_atoms[0], n))
        if row.deriv:
            for _kind, _target, expr in getattr(integrator, '_steps', []):
                if expr and 'deriv(' in expr:
                    raise derivative_refusal(row, '...', expr)
        if row.after:
            row.after(engine, system, integrator, forces)


def free_space_mode(system, has_box):
    """True: a free-space Context -- every NonbondedForce / CustomNonbondedForce is NoCutoff or CutoffNonPeriodic, no bonded
    force uses periodic boundary conditions and the System holds a force (box vectors may be absent; present ones are ignored).
    False: all nonbonded forces periodic, as ever.  A mixture is an InputError."""
    pair_classes = tuple(cls for row in FORCE_TABLE if row.pair for cls in row.classes)

    def pair_forces(force):
        if isinstance(force, pair_classes):
            return [force]
        if isinstance(force, mm.CustomCVForce):
            return [f for k in range(force.getNumCollectiveVariables()) for f in pair_forces(force.getCollectiveVariable(k))]
        return []
    forces = list(system.getForces())
    pairs = [f for force in forces for f in pair_forces(force)]
    # a generalized-Born force runs in free space only (csrc/gb.hip): refused by name, not as a mixture
    for cls in (cls for row in FORCE_TABLE if row.free_only for cls in row.classes):
        if not any(isinstance(f, cls) for f in pairs):
            continue
        for f in pairs:
            if isinstance(f, cls) and f.usesPeriodicBoundaryConditions():
                raise InputError('%s: CutoffPeriodic is not supported: generalized-Born solvent runs in free space only '
                                 '(NoCutoff / CutoffNonPeriodic)' % cls.__name__)
            if f.usesPeriodicBoundaryConditions():
                raise InputError('a %s in a System with a box-periodic %s: generalized-Born solvent runs in free space '
                                 'only (every nonbonded method NoCutoff or CutoffNonPeriodic)' % (cls.__name__, f.__class__.__name__))
    free = [f for f in pairs if not f.usesPeriodicBoundaryConditions()]
    if free and len(free) != len(pairs):
        raise InputError('the System mixes periodic and non-periodic nonbonded methods: every NonbondedForce / CustomNonbondedForce '
                         'must be NoCutoff or CutoffNonPeriodic (free space), or every one periodic')
    if (pairs and not free) or (not pairs and (has_box or not forces)):
        return False              # periodic, or nothing to decide by (no box and no forces: the error of old)
    periodic = [f for f in forces if not pair_forces(f) and not isinstance(f, mm.MonteCarloBarostat) and f.usesPeriodicBoundaryConditions()]
    if periodic:
        raise InputError('the System mixes non-periodic nonbonded methods (or no box) with a %s that uses periodic boundary '
                         'conditions' % periodic[0].__class__.__name__)
    return True
