"""Forces with kernels that walk all pairs (or all sets) of their own rows: GBSAOBCForce, CustomGBForce, CustomHbondForce,
CustomManyParticleForce, GayBerneForce, DrudeForce.  One backend force each, carried in entry.term_ids, so every loop over an
entry's forces reaches it and the scheduler's fusion rules decline its group.  What they cannot run with on the whole -- several
ranks, deriv(energy, ...) steps, too many atoms -- is in their rows of the force table (table.py)."""
import numpy as np

from .. import expr as X
from .. import openmm as mm
from .. import tables as T
from ..utils import InputError
from .common import COMPOUND_KINDS, backend_refusals, globals_update

GB_MAX_ATOMS = 32768      # csrc/amm_ctx.h: AMM_FREE_MAX_ATOMS
HBOND_MAX = 32768         # csrc/hbond.hip: AMM_HB_MAX_ROWS donors, and as many acceptors
MANY_MAX = 32768          # csrc/manyparticle.hip: AMM_MP_MAX_PARTICLES
MANY_MAX_NOCUTOFF = 2048  # ... AMM_MP_MAX_NOCUTOFF: the neighbour table is n x (n - 1) without a cutoff
MANY_MAX_TYPES = 16       # ... AMM_MP_MAX_TYPES
GAYBERNE_MAX = 32768      # csrc/gayberne.hip: AMM_GY_MAX_ROWS interacting particles
MANY_PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # of a tuple's positions, in lexicographic order


def translate_gb(engine, force, entry):
    """A GBSAOBCForce (csrc/gb.hip)."""
    def arrays():
        if force.getNumParticles() != engine.n:
            raise mm.OpenMMException('GBSAOBCForce must have exactly as many particles as the System it belongs to')
        par = np.array(force._particles, dtype=np.float64).reshape(-1, 3)
        if force.usesPeriodicBoundaryConditions():
            raise InputError('GBSAOBCForce: CutoffPeriodic is not supported: generalized-Born solvent runs in free space only')
        rc = force._cutoff if force.getNonbondedMethod() == force.CutoffNonPeriodic else 0.0
        return (par[:, 0], par[:, 1], par[:, 2]), dict(eps_in=force.getSoluteDielectric(), eps_out=force.getSolventDielectric(),
                                                        sa_energy=force._sa_energy, rc=rc)
    with backend_refusals('GBSAOBCForce'):
        per_atom, scalars = arrays()
        gid = engine.ctx.gb_create(*per_atom, **scalars)
    entry.term_ids.append(gid)
    entry.gb = gid

    def reload():          # updateParametersInContext: everything is read again
        per_atom, scalars = arrays()
        with backend_refusals('GBSAOBCForce'):
            engine.ctx.gb_set_params(gid, *per_atom, **scalars)
        return 'values'
    entry.reload = reload


def check_custom_gb_force(force):
    """The force table's check of one CustomGBForce at creation: the kernels differentiate in positions only."""
    if force.getNumEnergyParameterDerivatives():
        raise NotImplementedError('CustomGBForce.addEnergyParameterDerivative(%r) is not supported: the custom generalized-Born '
                                  'kernels differentiate in positions only' % force.getEnergyParameterDerivativeName(0))


def check_custom_gb_symmetry(text, per_particle_names, value_names, global_values, rows, functions=None, samples=6, seed=20240607):
    """A pair energy term is evaluated from both rows and counted half (csrc/custom_gb.hip), so it must not change when the
    particles swap -- parameters AND computed values: check_pair_symmetry with the values among the swapped names.  The sample
    parameters are rows the force has (`rows`: [n][parameters]; a type index is no uniform draw), the values seeded draws."""
    rng = np.random.default_rng(seed)
    rows = np.unique(np.asarray(rows, dtype=np.float64).reshape(-1, len(per_particle_names)), axis=0) if per_particle_names else np.zeros((1, 0))
    for _ in range(samples):
        a, b = rows[rng.integers(0, len(rows))], rows[rng.integers(0, len(rows))]
        one = dict(zip(per_particle_names, map(float, a)), **{nm: float(rng.uniform(0.2, 1.5)) for nm in value_names})
        two = dict(zip(per_particle_names, map(float, b)), **{nm: float(rng.uniform(0.2, 1.5)) for nm in value_names})
        env = dict(global_values, r=float(rng.uniform(0.3, 1.2)))
        fwd = dict(env, **{nm + '1': v for nm, v in one.items()}, **{nm + '2': v for nm, v in two.items()})
        swp = dict(env, **{nm + '1': v for nm, v in two.items()}, **{nm + '2': v for nm, v in one.items()})
        try:
            x, y = X.eval_global(text, fwd, functions=functions), X.eval_global(text, swp, functions=functions)
        except (ArithmeticError, ValueError) as exc:
            if isinstance(exc, X.ExpressionError):
                raise
            continue               # (outside the text's domain at this draw: says nothing about symmetry)
        if x != x and y != y:
            continue
        if not abs(x - y) <= 1e-12 * max(abs(x), abs(y), 1e-300):
            raise InputError('CustomGBForce: the pair energy term %r is not symmetric in particles 1 and 2' % text.split(';')[0])


def translate_custom_gb(engine, force, entry):
    """A CustomGBForce: its texts compiled here (expr.compile_custom_gb) for the kernels of csrc/custom_gb.hip."""
    cls = 'CustomGBForce'
    names = [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    values = [tuple(force.getComputedValueParameters(k)) for k in range(force.getNumComputedValues())]
    terms = [tuple(force.getEnergyTermParameters(k)) for k in range(force.getNumEnergyTerms())]
    functions = list(force._functions)
    try:
        progs = X.compile_custom_gb(names, gnames, values, terms, T.declared(functions) if functions else None)
    except X.ExpressionError as exc:
        raise InputError('%s: not a model the custom generalized-Born kernels can run: %s' % (cls, exc))
    uses_tables = any(X.table_words(p.code) for p in progs.programs)
    n = engine.n

    def params():
        if force.getNumParticles() != n:
            raise mm.OpenMMException('%s must have exactly as many particles as the System it belongs to' % cls)
        allp = np.array(force._particles, dtype=np.float64).reshape(n, -1) if names else np.zeros((n, 0))
        if allp.shape[1] != len(names):
            raise mm.OpenMMException('%s: every particle needs %d parameters' % (cls, len(names)))
        return allp

    def checked():
        """The particles' rows after the checks the host can make: every pair energy term is symmetric over them."""
        rows = params()
        callables = {name: T.host_callable(fn) for name, fn in functions} or None
        for text, kind in terms:
            if kind != force.SingleParticle:
                check_custom_gb_symmetry(text, names, [v[0] for v in values], {g: engine.parameters[g] for g in gnames}, rows,
                                         functions=callables)
        return rows

    rows = checked()
    rc = force._cutoff if force.getNonbondedMethod() == force.CutoffNonPeriodic else 0.0
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    frozen = (len(values), len(terms), [list(v) for v in values], [list(t) for t in terms], excl.copy(), len(functions))
    with backend_refusals(cls):
        gid = engine.ctx.custom_gb_create(len(values), progs.types, [(p.code, p.consts) for p in progs.programs],
                                          [engine.parameters[g] for g in gnames], np.ascontiguousarray(rows.T), excl, rc)
        if uses_tables or functions:
            engine.ctx.custom_gb_set_tables(gid, [T.device_table(fn) for _, fn in functions])
    entry.term_ids.append(gid)
    entry.custom_gb = dict(id=gid, n_values=len(values))
    entry.program = progs

    def reload():          # updateParametersInContext: the per-particle parameters and the tables' values are read again
        now = (force.getNumComputedValues(), force.getNumEnergyTerms(), [list(v) for v in force._values], [list(t) for t in force._terms],
               np.array(force._exclusions, dtype=np.int32).reshape(-1, 2), len(force._functions))
        if now[:4] != frozen[:4] or now[5] != frozen[5] or not np.array_equal(now[4], frozen[4]):
            raise mm.OpenMMException('%s.updateParametersInContext: the computed values, energy terms, exclusions and the number of '
                                     'tabulated functions cannot change in a live Context' % cls)
        fresh = checked()
        with backend_refusals(cls):
            if functions:
                engine.ctx.custom_gb_set_tables(gid, [T.device_table(fn) for _, fn in functions])
            engine.ctx.custom_gb_set_params(gid, np.ascontiguousarray(fresh.T))
        return 'values'
    entry.reload = reload
    globals_update(entry, gnames, lambda values: engine.ctx.custom_gb_set_globals(gid, values))


def translate_hbond(engine, force, entry):
    """A CustomHbondForce: the text compiled with its variable table (expr.compile_hbond) and evaluated over all donor-acceptor
    pairs by the hydrogen-bond kernels (csrc/hbond.hip)."""
    cls = 'CustomHbondForce'
    if getattr(force, '_functions', None):
        raise NotImplementedError('%s: tabulated functions in the energy expression are not supported' % cls)
    method = force.getNonbondedMethod()
    periodic = method == force.CutoffPeriodic
    if periodic and engine.free_space:
        raise InputError('%s uses CutoffPeriodic in a System in free space' % cls)
    dnames = [force.getPerDonorParameterName(k) for k in range(force.getNumPerDonorParameters())]
    anames = [force.getPerAcceptorParameterName(k) for k in range(force.getNumPerAcceptorParameters())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    try:
        prog, variables = X.compile_hbond(force.getEnergyFunction(), dnames, anames, gnames)
    except X.ExpressionError as exc:
        raise InputError('%s: not an energy expression the hydrogen-bond kernel can run: %s' % (cls, exc))
    kinds = [COMPOUND_KINDS[kind] for kind, _ in variables]
    slots = [list(s) for _, s in variables]
    named = sorted({s for _, ss in variables for s in ss})
    slot_names = ('d1', 'd2', 'd3', 'a1', 'a2', 'a3')
    n = engine.n

    def tables():
        out = []
        for side, rows, names, limit in (('donor', force._donors, dnames, 0), ('acceptor', force._acceptors, anames, 3)):
            if len(rows) > HBOND_MAX:
                raise InputError('%s: %d %ss (limit %d)' % (cls, len(rows), side, HBOND_MAX))
            idx = np.zeros((len(rows), 3), dtype=np.int32)
            par = np.zeros((len(names), len(rows)), dtype=np.float64)
            for t, (members, p) in enumerate(rows):
                if len(p) != len(names):
                    raise mm.OpenMMException('%s: every %s needs %d parameters' % (cls, side, len(names)))
                if not 0 <= members[0] < n or any(not -1 <= m < n for m in members[1:]):
                    raise mm.OpenMMException('%s: a particle index of %s %d is out of range' % (cls, side, t))
                for r in range(3):
                    if members[r] == -1 and limit + r in named:
                        raise InputError('%s: the energy expression names %s, which %s %d leaves at -1' % (cls, slot_names[limit + r], side, t))
                idx[t] = members
                par[:, t] = p
            out += [idx, par]
        return out

    def exclusions():
        ex = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
        if len(ex) and (ex.min() < 0 or ex[:, 0].max() >= force.getNumDonors() or ex[:, 1].max() >= force.getNumAcceptors()):
            raise mm.OpenMMException('%s: an exclusion names a donor or an acceptor that does not exist (the indices are those of '
                                     'donors and acceptors, not of atoms)' % cls)
        return ex

    didx, dpar, aidx, apar = tables()
    excl = exclusions()
    rc = 0.0 if method == force.NoCutoff else float(force._cutoff)
    if method != force.NoCutoff and not rc > 0.0:
        raise InputError('%s: the cutoff distance must be above zero' % cls)
    with backend_refusals(cls):
        fid = engine.ctx.hbond_create(prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_], kinds, slots, didx, aidx, dpar, apar,
                                      excl, rc=rc, periodic=periodic)
    entry.term_ids.append(fid)
    entry.term_expr = True
    entry.program = prog
    entry.hbond = dict(id=fid, variables=variables)

    def reload():          # updateParametersInContext: the per-donor and per-acceptor parameters are read again
        f_didx, f_dpar, f_aidx, f_apar = tables()
        if len(f_didx) != len(didx) or len(f_aidx) != len(aidx):
            raise mm.OpenMMException('updateParametersInContext: the number of donors or acceptors has changed')
        if not (np.array_equal(f_didx, didx) and np.array_equal(f_aidx, aidx)):
            raise mm.OpenMMException('updateParametersInContext: the particles of a donor or an acceptor have changed')
        if not np.array_equal(exclusions(), excl):
            raise mm.OpenMMException('updateParametersInContext: the exclusions have changed')
        engine.ctx.hbond_set_params(fid, f_dpar, len(didx), f_apar, len(aidx))
        return 'values'
    entry.reload = reload
    globals_update(entry, prog.globals_, lambda values: engine.ctx.hbond_set_globals(fid, values))


def many_particle_table(filters, types, central):
    """The permutation table of a CustomManyParticleForce over sets of three (csrc/manyparticle.hip).  filters[r]: the
    set of types role r takes (empty: any); types: the sorted distinct types of the particles, whose positions are the dense type
    indices.  Entry [a][b][c] speaks for a set whose tuple -- its particles in ascending order or, in central mode, the centre first
    and the satellites ascending -- has the dense types (a, b, c): the code k of the first permutation MANY_PERMUTATIONS[k] = perm,
    in lexicographic order, for which every role r takes the type of the tuple's element perm[r], or -1 when there is none (the set
    is skipped).  Central mode keeps the centre at p1: codes 0 and 1 only.  Returns an int32 array [T][T][T]."""
    T = len(types)
    table = np.full((T, T, T), -1, dtype=np.int32)
    candidates = MANY_PERMUTATIONS[:2] if central else MANY_PERMUTATIONS
    for a in range(T):
        for b in range(T):
            for c in range(T):
                tuple_types = (types[a], types[b], types[c])
                for code, perm in enumerate(candidates):
                    if all(not filters[r] or tuple_types[perm[r]] in filters[r] for r in range(3)):
                        table[a, b, c] = code
                        break
    return table


def translate_many_particle(engine, force, entry):
    """A CustomManyParticleForce over sets of three: the text compiled with its variable table (expr.compile_many_particle), the
    type filters turned into the permutation table (many_particle_table) and the sets enumerated on the device by the
    many-particle kernels (csrc/manyparticle.hip)."""
    cls = 'CustomManyParticleForce'
    per_set = force.getNumParticlesPerSet()
    if per_set != 3:
        raise NotImplementedError('%s: sets of %d particles are not supported (the many-particle kernel enumerates sets of three)' % (cls, per_set))
    if getattr(force, '_functions', None):
        raise NotImplementedError('%s: tabulated functions in the energy expression are not supported' % cls)
    method = force.getNonbondedMethod()
    periodic = method == force.CutoffPeriodic
    if periodic and engine.free_space:
        raise InputError('%s uses CutoffPeriodic in a System in free space' % cls)
    central = force.getPermutationMode() == force.UniqueCentralParticle
    pnames = [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    try:
        prog, variables = X.compile_many_particle(force.getEnergyFunction(), 3, pnames, gnames)
    except X.ExpressionError as exc:
        raise InputError('%s: not an energy expression the many-particle kernel can run: %s' % (cls, exc))
    kinds = [COMPOUND_KINDS[kind] for kind, _ in variables]
    slots = [list(s) for _, s in variables]
    n = engine.n
    if force.getNumParticles() != n:
        raise mm.OpenMMException('%s: the force has %d particles, the System %d' % (cls, force.getNumParticles(), n))
    if n > MANY_MAX:
        raise InputError('%s: %d particles (limit %d)' % (cls, n, MANY_MAX))
    if method == force.NoCutoff and n > MANY_MAX_NOCUTOFF:
        raise InputError('%s: %d particles under NoCutoff (limit %d: the neighbour table is n x (n - 1); use a cutoff)' % (cls, n, MANY_MAX_NOCUTOFF))

    def tables():
        par = np.zeros((len(pnames), n), dtype=np.float64)
        raw = np.zeros(n, dtype=np.int64)
        for t, (p, kind) in enumerate(force._particles):
            if len(p) != len(pnames):
                raise mm.OpenMMException('%s: every particle needs %d parameters' % (cls, len(pnames)))
            par[:, t] = p
            raw[t] = kind
        known = sorted(set(raw.tolist()))
        if len(known) > MANY_MAX_TYPES:
            raise InputError('%s: %d distinct particle types (limit %d)' % (cls, len(known), MANY_MAX_TYPES))
        known = known or [0]
        dense = np.array([known.index(t) for t in raw.tolist()], dtype=np.int32)
        filters = [force.getTypeFilter(r) for r in range(3)]
        return par, dense, len(known), many_particle_table(filters, known, central)

    def exclusions():
        ex = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
        if len(ex) and (ex.min() < 0 or ex.max() >= n):
            raise mm.OpenMMException('%s: an exclusion names a particle that does not exist' % cls)
        return ex

    par, dense, n_types, table = tables()
    excl = exclusions()
    rc = 0.0 if method == force.NoCutoff else float(force._cutoff)
    if method != force.NoCutoff and not rc > 0.0:
        raise InputError('%s: the cutoff distance must be above zero' % cls)
    with backend_refusals(cls):
        fid = engine.ctx.many_create(prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_], kinds, slots, par, dense, n_types, table,
                                     excl, rc=rc, periodic=periodic, central=central)
    entry.term_ids.append(fid)
    entry.term_expr = True
    entry.program = prog
    entry.many = dict(id=fid, variables=variables, types=n_types)

    def reload():          # updateParametersInContext: the per-particle parameters, the types and the filters are read again
        if force.getNumParticles() != n:
            raise mm.OpenMMException('updateParametersInContext: the number of particles has changed')
        if not np.array_equal(exclusions(), excl):
            raise mm.OpenMMException('updateParametersInContext: the exclusions have changed')
        f_par, f_dense, f_types, f_table = tables()
        engine.ctx.many_set_params(fid, f_par, f_dense, f_types, f_table)
        entry.many['types'] = f_types
        return 'values'
    entry.reload = reload
    globals_update(entry, prog.globals_, lambda values: engine.ctx.many_set_globals(fid, values))


def gayberne_tables(force, n):
    """What a GayBerneForce hands to the Gay-Berne kernels (csrc/gayberne.hip), checked against a System of n particles:
    active   int32 [A]: the interacting particles, ascending -- epsilon > 0, or a member of an exception with epsilon > 0;
    axes     int32 [A][2]: x- and y-particle of the row, -1: none;
    par      float64 [A][8]: sigma, epsilon, sx, sy, sz, ex, ey, ez;
    ex_ptr / ex_col / ex_par   the exceptions between active particles as a CSR over rows: columns are ACTIVE indices, ascending,
             (sigma, epsilon) per entry, every pair on both rows (an exception with an inactive member can only have epsilon 0 and a
             partner that the scan never meets: it is dropped);
    rev_ptr / rev_src   int32 [n + 1] / [.]: per particle the entries 2 * row + (0: x-particle, 1: y-particle) that name it, ascending.
    Raises OpenMMException by name for what the definition forbids."""
    cls = 'GayBerneForce'
    if force.getNumParticles() != n:
        raise mm.OpenMMException('%s: the force has %d particles, the System %d' % (cls, force.getNumParticles(), n))
    rows = force._particles
    for i, (sigma, eps, xp, yp, sx, sy, sz, ex, ey, ez) in enumerate(rows):
        if not (-1 <= xp < n and -1 <= yp < n):
            raise mm.OpenMMException('%s: an axis particle of particle %d is out of range' % (cls, i))
        if xp == i or yp == i:
            raise mm.OpenMMException('%s: particle %d is its own axis particle' % (cls, i))
        if sigma < 0.0 or eps < 0.0 or min(sx, sy, sz) <= 0.0 or min(ex, ey, ez) <= 0.0:
            raise mm.OpenMMException('%s: particle %d needs sigma, epsilon >= 0 and diameters and well-depth scales above zero' % (cls, i))
        if xp == -1 and not (sx == sy == sz and ex == ey == ez):
            raise mm.OpenMMException('%s: particle %d has no x-particle, which only a sphere (sx = sy = sz, ex = ey = ez) may omit' % (cls, i))
        if xp == -1 and yp != -1:
            raise mm.OpenMMException('%s: particle %d has a y-particle and no x-particle' % (cls, i))
        if yp == -1 and not (sy == sz and ey == ez):
            raise mm.OpenMMException('%s: particle %d has no y-particle, which only a uniaxial shape (sy = sz, ey = ez) may omit' % (cls, i))
    pairs = {}
    for k, (i, j, sigma, eps) in enumerate(force._exceptions):
        if not (0 <= i < n and 0 <= j < n) or i == j:
            raise mm.OpenMMException('%s: exception %d names a particle that does not exist, or one particle twice' % (cls, k))
        if sigma < 0.0 or eps < 0.0:
            raise mm.OpenMMException('%s: exception %d needs sigma, epsilon >= 0' % (cls, k))
        key = (min(i, j), max(i, j))
        if key in pairs:
            raise mm.OpenMMException('%s: two exceptions for particles %d and %d' % ((cls,) + key))
        pairs[key] = (sigma, eps)
    interacting = {i for i, row in enumerate(rows) if row[1] > 0.0}
    interacting |= {m for key, (_, eps) in pairs.items() if eps > 0.0 for m in key}
    active = np.array(sorted(interacting), dtype=np.int32)
    act_of = {int(p): k for k, p in enumerate(active)}
    axes = np.array([[rows[p][2], rows[p][3]] for p in active], dtype=np.int32).reshape(-1, 2)
    par = np.array([rows[p][:2] + rows[p][4:] for p in active], dtype=np.float64).reshape(-1, 8)
    entries = sorted((act_of[a], act_of[b], v) for (i, j), v in pairs.items() if i in act_of and j in act_of
                     for a, b in ((i, j), (j, i)))
    ex_ptr = np.zeros(len(active) + 1, dtype=np.int32)
    for r, _, _ in entries:
        ex_ptr[r + 1] += 1
    ex_ptr = np.cumsum(ex_ptr, dtype=np.int32)
    ex_col = np.array([c for _, c, _ in entries], dtype=np.int32)
    ex_par = np.array([v for _, _, v in entries], dtype=np.float64).reshape(-1, 2)
    named = sorted((int(axes[k, r]), 2 * k + r) for k in range(len(active)) for r in range(2) if axes[k, r] >= 0)
    rev_ptr = np.zeros(n + 1, dtype=np.int32)
    for p, _ in named:
        rev_ptr[p + 1] += 1
    rev_ptr = np.cumsum(rev_ptr, dtype=np.int32)
    rev_src = np.array([src for _, src in named], dtype=np.int32)
    return dict(active=active, axes=axes, par=par, ex_ptr=ex_ptr, ex_col=ex_col, ex_par=ex_par, rev_ptr=rev_ptr, rev_src=rev_src)


def translate_gayberne(engine, force, entry):
    """A GayBerneForce: the interacting particles compacted, their exceptions as a CSR and the reverse table of the axis particles
    (gayberne_tables) go to the Gay-Berne kernels (csrc/gayberne.hip).  It reads no Context parameter: deriv(energy, p) sees no
    dependence through it."""
    cls = 'GayBerneForce'
    method = force.getNonbondedMethod()
    periodic = method == force.CutoffPeriodic
    if periodic and engine.free_space:
        raise InputError('%s uses CutoffPeriodic in a System in free space' % cls)
    n = engine.n
    rc = 0.0 if method == force.NoCutoff else float(force._cutoff)
    if method != force.NoCutoff and not rc > 0.0:
        raise InputError('%s: the cutoff distance must be above zero' % cls)
    rs = -1.0
    if method != force.NoCutoff and force.getUseSwitchingFunction():
        rs = float(force._switch)
        if not 0.0 <= rs < rc:
            raise InputError('%s: the switching distance %g lies outside [0, cutoff = %g)' % (cls, rs, rc))
    if periodic and rc > 0.5 * float(engine.box.min()):
        raise InputError('%s: the cutoff %g exceeds half the shortest box edge (%g)' % (cls, rc, float(engine.box.min())))
    tab = gayberne_tables(force, n)
    if len(tab['active']) > GAYBERNE_MAX:
        raise InputError('%s: %d particles with epsilon > 0 (limit %d)' % (cls, len(tab['active']), GAYBERNE_MAX))
    with backend_refusals(cls):
        fid = engine.ctx.gayberne_create(tab['active'], tab['axes'], tab['par'], tab['ex_ptr'], tab['ex_col'], tab['ex_par'], tab['rev_ptr'],
                                         tab['rev_src'], rc=rc, rs=rs, periodic=periodic)
    entry.term_ids.append(fid)
    entry.gayberne = fid

    def reload():          # updateParametersInContext: the particle and exception parameters are read again
        new = gayberne_tables(force, n)
        for key, what in (('active', 'the set of interacting particles (epsilon > 0, or in an exception with epsilon > 0)'),
                          ('axes', 'the x- or y-particle of an ellipsoid'), ('ex_ptr', 'the pairs that have an exception'),
                          ('ex_col', 'the pairs that have an exception')):
            if not np.array_equal(new[key], tab[key]):
                raise mm.OpenMMException('updateParametersInContext: %s has changed' % what)
        engine.ctx.gayberne_set_params(fid, new['par'], new['ex_par'])
        return 'values'
    entry.reload = reload


def drude_tables(force, n, constrained=()):
    """What a DrudeForce hands to the Drude kernels (csrc/drude.hip), checked against a System of n particles whose
    constrained particles are `constrained`:
    idx      int32 [D][5]: particle, particle1 .. particle4 (-1: none);
    par      float64 [D][4]: charge, polarizability, aniso12, aniso34;
    pairs    int32 [P][2]: the two Drude entries of a screened pair;  thole  float64 [P].
    Raises OpenMMException by name for what the definition forbids."""
    cls = 'DrudeForce'
    rows = force._particles
    held = set(int(c) for c in constrained)
    seen = {}
    for k, (p, p1, p2, p3, p4, q, alpha, a12, a34) in enumerate(rows):
        if not (0 <= p < n and 0 <= p1 < n):
            raise mm.OpenMMException('%s: Drude particle %d names a particle or a parent that is out of range' % (cls, k))
        if not all(-1 <= a < n for a in (p2, p3, p4)):
            raise mm.OpenMMException('%s: Drude particle %d names an anisotropy particle that is out of range' % (cls, k))
        for a in (p, p1):
            if a in seen or p == p1:
                raise mm.OpenMMException('%s: particle %d is listed twice as a Drude particle or a parent (Drude particles %d and %d)'
                                         % (cls, a, seen.get(a, k), k))
        seen[p] = seen[p1] = k
        if p in held:
            raise mm.OpenMMException('%s: Drude particle %d (particle %d) is constrained' % (cls, k, p))
        if p2 == p1 or (p3 != -1 and p3 == p4):
            raise mm.OpenMMException('%s: an anisotropy direction of Drude particle %d joins a particle to itself' % (cls, k))
        a1 = a12 if p2 != -1 else 1.0
        a2 = a34 if (p3 != -1 and p4 != -1) else 1.0
        if not alpha > 0.0:
            raise mm.OpenMMException('%s: Drude particle %d needs a polarizability above zero' % (cls, k))
        if not (a1 > 0.0 and a2 > 0.0 and 3.0 - a1 - a2 > 0.0):
            raise mm.OpenMMException('%s: Drude particle %d needs aniso12, aniso34 and 3 - aniso12 - aniso34 above zero' % (cls, k))
    for k, (d1, d2, thole) in enumerate(force._pairs):
        if not (0 <= d1 < len(rows) and 0 <= d2 < len(rows)) or d1 == d2:
            raise mm.OpenMMException('%s: screened pair %d names a Drude particle that does not exist, or one twice' % (cls, k))
    idx = np.array([r[:5] for r in rows], dtype=np.int32).reshape(-1, 5)
    par = np.array([r[5:] for r in rows], dtype=np.float64).reshape(-1, 4)
    pairs = np.array([r[:2] for r in force._pairs], dtype=np.int32).reshape(-1, 2)
    thole = np.array([r[2] for r in force._pairs], dtype=np.float64)
    return dict(idx=idx, par=par, pairs=pairs, thole=thole)


def drude_step_of(engine):
    """True: the Context steps with a DrudeLangevinIntegrator."""
    return engine._stock is not None and getattr(engine._stock, '_drude', False)


def check_drude_integrator(engine, forces):
    """The force table's check ahead of the DrudeForce row, whether or not the System holds one."""
    if drude_step_of(engine) and len(forces) != 1:
        raise InputError('a DrudeLangevinIntegrator needs a System with exactly one DrudeForce (this one has %d)' % len(forces))


def check_drude_system(engine, system, integrator, forces):
    """The force table's check behind the DrudeForce row: the step texts a DrudeForce does not run with, and a dry run of its tables."""
    texts = [e.replace(' ', '') for _, _, e in getattr(integrator, '_steps', []) if isinstance(e, str)]
    if any('deriv(energy' in t for t in texts):
        raise NotImplementedError('deriv(energy, ...) in a System with a DrudeForce is not supported: the Drude kernels have no '
                                  'derivative mode')
    if any('cosh(z)' in t and 'LkT' in t for t in texts):
        raise NotImplementedError('a DrudeForce does not run with the SIN(R) / isokinetic path')
    if any('tanh(' in t for t in texts):
        raise NotImplementedError('a DrudeForce does not run with the regulated path')
    constrained = {int(c[k]) for c in system._constraints for k in (0, 1)}
    for force in forces:
        drude_tables(force, system.getNumParticles(), constrained)


def translate_drude(engine, force, entry):
    """A DrudeForce: its rows (drude_tables) go to the Drude kernels (csrc/drude.hip), which derive the spring constants and the
    pair parameters.  It reads no Context parameter."""
    cls = 'DrudeForce'
    periodic = force.usesPeriodicBoundaryConditions()
    if periodic and engine.free_space:
        raise InputError('%s uses periodic boundary conditions in a System in free space' % cls)
    n = engine.n
    constrained = {int(c[k]) for c in engine.system._constraints for k in (0, 1)}
    tab = drude_tables(force, n, constrained)
    with backend_refusals(cls):
        fid = engine.ctx.drude_create(tab['idx'], tab['par'], tab['pairs'], tab['thole'], periodic=periodic)
    entry.term_ids.append(fid)
    entry.drude = fid

    def reload():          # updateParametersInContext: charges, polarizabilities, anisotropies and Thole factors are read again
        new = drude_tables(force, n, constrained)
        for key, what in (('idx', 'a particle of a Drude particle'), ('pairs', 'a Drude particle of a screened pair')):
            if not np.array_equal(new[key], tab[key]):
                raise mm.OpenMMException('updateParametersInContext: %s has changed' % what)
        engine.ctx.drude_set_params(fid, new['idx'], new['par'], new['pairs'], new['thole'])
        return 'values'
    entry.reload = reload
