"""Pair forces over neighbour lists (or, in free space, over all pairs): NonbondedForce and the CustomNonbondedForce families --
near / damped-smoothed, softcore, lj-virial, the alchemical pair forces -- and any other text on the pair-expression kernel."""
import math

import numpy as np

from .. import backend as B
from .. import expr as X
from .. import openmm as mm
from .. import tables as T
from ..utils import InputError
from .common import (custom_long_range_correction, descriptor_of, dispersion_correction, effective, family_of, globals_update,
                     lrc_class_pairs, pair_create, pair_desc_from, register_globals, replace_bonded, softcore_long_range_correction)


def translate_nonbonded(engine, nb, entry):
    method = nb.getNonbondedMethod()
    if method not in (nb.NoCutoff, nb.CutoffNonPeriodic, nb.CutoffPeriodic, nb.Ewald, nb.PME):
        raise InputError('the HIP path evaluates NonbondedForces with NoCutoff, CutoffNonPeriodic, CutoffPeriodic, Ewald or PME')
    periodic = not engine.free_space
    # NoCutoff: all non-excepted pairs, 4 eps ((sigma/r)^12 - (sigma/r)^6) + Kc qq / r -- no switch, no reaction field (rc = 0)
    no_cutoff = method == nb.NoCutoff
    rc = 0.0 if no_cutoff else nb._cutoff
    n = engine.n
    def offsets(records, rows):
        """(parameter names in order of first use, [name][row] -> (charge, sigma, epsilon) scales) of addParticle/ExceptionParameterOffset."""
        names = list(dict.fromkeys(rec[0] for rec in records))
        scales = np.zeros((len(names), rows, 3))
        for name, idx, qs, ss, es in records:
            scales[names.index(name), idx] = [qs, ss, es]
        return names, scales
    base = np.array(nb._particles, dtype=np.float64).reshape(n, 3)
    names, scales = offsets(nb._particle_offsets, n)
    exc = np.array([[r[0], r[1]] for r in nb._exceptions], dtype=np.int32).reshape(-1, 2)
    exc_base = np.array([r[2:] for r in nb._exceptions], dtype=np.float64).reshape(-1, 3)
    enames, escales = offsets(nb._exception_offsets, len(exc))
    use_switch = nb._use_switch and not no_cutoff
    flags = B.SWITCH if use_switch else 0
    alpha = krf = crf = 0.0
    ewald = method in (nb.Ewald, nb.PME)
    if no_cutoff:
        pass
    elif ewald:
        alpha = nb._pme[0] if nb._pme[0] > 0 else math.sqrt(-math.log(2 * nb._ewald_tol)) / rc
        flags |= B.COULOMB_EWALD
    else:
        eps_rf = nb._rf_dielectric
        krf = (eps_rf - 1) / ((2 * eps_rf + 1) * rc ** 3)
        crf = 3 * eps_rf / ((2 * eps_rf + 1) * rc)
        flags |= B.COULOMB_RF
    desc = B.pair_desc(B.NONBONDED, rc, rswitch=nb._switch if use_switch else 0.0, alpha=alpha, flags=flags,
                       krf=krf, crf=crf)
    eff = effective(base, scales, names, engine.parameters)
    pid = pair_create(engine, desc, eff[:, 0], eff[:, 1], eff[:, 2], exc)
    entry.pair_ids.append(pid)
    entry.alpha = alpha
    entry.ewald = ewald
    if ewald:
        entry.recip_group = nb._recip_group if nb._recip_group >= 0 else nb.getForceGroup()
        # PME mesh: explicit setPMEParameters, else OpenMM's rule ceil(2 alpha L / (3 tol^(1/5))) [recalled];
        # nonbondedMethod Ewald is evaluated on the same mesh (smooth PME stands in for the explicit k-sum)
        if nb._pme[0] > 0 and min(nb._pme[1:]) > 0:
            grid = [int(k) for k in nb._pme[1:]]
        else:
            grid = [max(6, int(math.ceil(2 * alpha * L / (3 * nb._ewald_tol ** 0.2)))) for L in engine.box]
        entry.recip = engine.ctx.pme_create(alpha, grid, eff[:, 0])
        entry.recip_grid = grid

    def bonded_terms(parameters):
        q = effective(base, scales, names, parameters)[:, 0]
        terms = []
        ep = effective(exc_base, escales, enames, parameters) if len(exc) else exc_base
        keep = (ep[:, 0] != 0.0) | (ep[:, 2] != 0.0) if len(exc) else np.zeros(0, bool)
        if keep.any():
            terms.append((B.BOND_LJC, exc[keep], ep[keep], periodic, B.pair_desc(B.NONBONDED, rc)))
        if ewald and len(exc):
            terms.append((B.BOND_EWALD_EXCL, exc, (q[exc[:, 0]] * q[exc[:, 1]]).reshape(-1, 1), periodic,
                          B.pair_desc(B.NONBONDED, rc, alpha=alpha)))
        return terms

    defaults = {nb.getGlobalParameterName(i): nb.getGlobalParameterDefaultValue(i)
                for i in range(nb.getNumGlobalParameters())}

    def constant(parameters):
        # OpenMM evaluates the dispersion coefficient with the global parameters at their DEFAULT values and keeps
        # it when Context.setParameter changes them -- pinned by tests/test_systems.py:54 and :121 (sigma/epsilon
        # offsets at lambda_vdw = 0.5: the literals are met to 2e-7 kJ/mol only this way)
        if not nb._dispersion or engine.free_space:       # (no volume: no dispersion correction in free space)
            return 0.0
        p = effective(base, scales, names, defaults)
        return engine._vscale * dispersion_correction(p[:, 1], p[:, 2], engine._box_ref, rc, nb._switch if nb._use_switch else None)

    entry.terms = bonded_terms(engine.parameters)
    entry.constant = constant(engine.parameters)
    entry.rescale = lambda: setattr(entry, 'constant', constant(engine.parameters))
    lam = set(names) | set(enames)

    def update(parameters, changed, force=False):
        if not (lam & changed) and not force:
            return False
        p = effective(base, scales, names, parameters)
        engine.ctx.pair_set_params(pid, p[:, 0], p[:, 1], p[:, 2])
        if entry.recip is not None:
            engine.ctx.pme_set_charges(entry.recip, p[:, 0])
        entry.terms = bonded_terms(parameters)
        replace_bonded(engine, entry, entry.terms)
        entry.constant = constant(parameters)
        return True

    def reload():
        # NonbondedForce.updateParametersInContext: particle and exception parameters are read again (their number
        # and the exception pairs must not have changed, as in OpenMM)
        fresh = np.array(nb._particles, dtype=np.float64).reshape(n, 3)
        fresh_exc = np.array([r[2:] for r in nb._exceptions], dtype=np.float64).reshape(-1, 3)
        if fresh_exc.shape != exc_base.shape:
            raise mm.OpenMMException('updateParametersInContext: the number of exceptions has changed')
        base[:] = fresh
        exc_base[:] = fresh_exc
        return update(engine.parameters, set(), force=True)

    entry.reload = reload
    if lam:
        entry.update = update
        entry.depends = set(lam)
        # parameters whose offsets touch the charges only: the energy is a quadratic form of them
        entry.quadratic_in = {nm for nm in lam
                              if not (nm in names and np.any(scales[names.index(nm)][:, 1:]))
                              and not (nm in enames and np.any(escales[enames.index(nm)][:, 1:]))}


def check_pair_symmetry(text, per_particle_names, global_values, samples=6, seed=20240607, tabulated=None):
    """A pair is evaluated from both atoms' rows and counted once (csrc/pair_expr.hip), so the text must not change when the
    particles swap: evaluate it on the host at a handful of seeded random (r, parameters of 1, parameters of 2) and at the
    swapped parameters.  OpenMM leaves an asymmetric text undefined (which atom is 1 depends on its neighbour list).
    tabulated: (name -> callable, the force's particle rows [n][parameters]) of a force with tabulated functions -- the sample
    parameters are then rows the force HAS (a uniform draw is no type index): every pair of distinct rows when they are few
    (an asymmetric A(type1, type2) shows at the one pair of types it concerns), seeded draws of pairs otherwise."""
    rng = np.random.default_rng(seed)
    if tabulated is None:
        functions, draws = None, [None] * samples
    else:
        functions, rows = tabulated
        if not per_particle_names:
            return                 # (nothing to swap)
        rows = np.unique(np.asarray(rows, dtype=np.float64).reshape(-1, len(per_particle_names)), axis=0)
        if len(rows) <= 24:
            draws = [(rows[i], rows[j]) for i in range(len(rows)) for j in range(i + 1, len(rows))]
        else:
            draws = [(rows[i], rows[j]) for i, j in rng.integers(0, len(rows), size=(16 * samples, 2)) if i != j]
    for draw in draws:
        r = float(rng.uniform(0.3, 1.2))
        if draw is None:
            one = {nm: float(rng.uniform(0.2, 1.5)) for nm in per_particle_names}
            two = {nm: float(rng.uniform(0.2, 1.5)) for nm in per_particle_names}
        else:
            one, two = (dict(zip(per_particle_names, map(float, row))) for row in draw)
        env = dict(global_values, r=r)
        fwd = dict(env, **{nm + '1': one[nm] for nm in per_particle_names}, **{nm + '2': two[nm] for nm in per_particle_names})
        swp = dict(env, **{nm + '1': two[nm] for nm in per_particle_names}, **{nm + '2': one[nm] for nm in per_particle_names})
        try:
            if functions is None:
                a, b = X.eval_global(text, fwd), X.eval_global(text, swp)
            else:
                a, b = X.eval_global(text, fwd, functions=functions), X.eval_global(text, swp, functions=functions)
                if a != a and b != b:
                    continue       # (an index outside its table both ways: NaN on the device too, nothing about symmetry)
        except (ArithmeticError, ValueError) as exc:
            if isinstance(exc, X.ExpressionError):
                raise
            continue               # (outside the text's domain at this draw: says nothing about symmetry)
        if not abs(a - b) <= 1e-12 * max(abs(a), abs(b), 1e-300):      # (a few roundings of operations taken in another order)
            raise InputError('energy expression is not symmetric in particles 1 and 2')


def translate_pair_expression(engine, force, entry):
    """A CustomNonbondedForce whose energy text is none of the AtomsMM families: compiled here (expr.compile_pair) and interpreted
    per pair, with its derivative in r, by the pair-expression kernel (csrc/pair_expr.hip) on per-atom neighbour rows."""
    text = force.getEnergyFunction()
    # (what the generic kernel leaves out is said together with why the force came here)
    generic = 'energy expression not recognised as one of the AtomsMM families (%s); the generic pair-expression kernel ' % text.split(';')[0]
    if getattr(force, '_derivs', None):
        raise NotImplementedError(generic + 'differentiates in r only: no addEnergyParameterDerivative')
    if engine.free_space or force.getNonbondedMethod() != force.CutoffPeriodic:
        raise NotImplementedError(generic + 'evaluates with CutoffPeriodic only (not NoCutoff / CutoffNonPeriodic)')
    if engine.world > 1:
        raise NotImplementedError(generic + 'runs on a single rank')
    if force.getNumInteractionGroups() > 0:
        raise NotImplementedError(generic + 'takes no interaction groups')
    if force.getUseLongRangeCorrection():
        raise NotImplementedError(generic + 'computes no long-range correction')
    names = [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())]
    if len(names) > X.PAIR_MAX_PARAMS:
        raise InputError(generic + 'takes at most %d per-particle parameters (%d given): a neighbour row carries three doubles '
                         'per atom' % (X.PAIR_MAX_PARAMS, len(names)))
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    # addTabulatedFunction: (name, function) in the force's order -- the order of the table indices in the program
    functions = list(getattr(force, '_functions', []))
    try:
        prog = X.compile_pair(text, names, gnames, T.declared(functions)) if functions else X.compile_pair(text, names, gnames)
    except X.ExpressionError as exc:
        raise InputError('energy expression not recognised by the HIP path as one of the AtomsMM families, and not a pair '
                         'expression the generic kernel can run: %s' % exc)
    uses_tables = bool(X.table_words(prog.code))
    if not uses_tables:
        check_pair_symmetry(text, names, {g: engine.parameters[g] for g in prog.globals_})
    n = engine.n
    if force.getNumParticles() != n:
        raise mm.OpenMMException('CustomNonbondedForce must have exactly as many particles as the System')
    direct = T.direct_index_uses(text, functions) if uses_tables else []

    def slots():
        allp = np.array(force._particles, dtype=np.float64).reshape(n, -1)
        if allp.shape[1] != len(names):
            raise mm.OpenMMException('CustomNonbondedForce: every particle needs %d parameters' % len(names))
        # a per-particle value passed straight into a discrete function is an index: a whole number inside the table
        for symbol, fname, size in direct:
            if symbol[:-1] in names and symbol[-1] in '12':
                column = allp[:, names.index(symbol[:-1])]
                bad = np.nonzero(~((column == np.rint(column)) & (column >= 0) & (column < size)))[0]
                if len(bad):
                    raise mm.OpenMMException('CustomNonbondedForce: particle %d has %s = %r, passed to the tabulated function %s as an '
                                             'index: it must be a whole number in 0 .. %d' %
                                             (bad[0], symbol[:-1], float(column[bad[0]]), fname, size - 1))
        return [np.ascontiguousarray(allp[:, k]) if k < len(names) else np.zeros(n) for k in range(3)]

    def tables_checked():
        """What amm_pair_expr_set_tables takes, after the checks the host can make: the particles' indices lie in their tables,
        and the text is symmetric over the rows the force has."""
        rows = np.stack(slots()[:len(names)], axis=1) if names else np.zeros((n, 0))
        check_pair_symmetry(text, names, {g: engine.parameters[g] for g in prog.globals_},
                            tabulated=({name: T.host_callable(fn) for name, fn in functions}, rows))
        return [T.device_table(fn) for _, fn in functions]

    tables = tables_checked() if uses_tables else None
    rc = force._cutoff
    use_switch = force.getUseSwitchingFunction()
    if use_switch and not (0.0 <= force._switch < rc):
        raise mm.OpenMMException('CustomNonbondedForce: the switching distance must lie between 0 and the cutoff')
    desc = B.pair_desc(B.PAIR_EXPR, rc, rswitch=force._switch if use_switch else 0.0, flags=B.SWITCH if use_switch else 0)
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    pid = engine.ctx.pair_expr_create(desc, prog.code, prog.consts, [engine.parameters[g] for g in prog.globals_], *slots(), excl,
                                      skin=engine.skin)
    engine._pair_info[pid] = (float(rc), ('expr', pid))       # (a list of its own: never host or guest of a shared one)
    entry.pair_ids.append(pid)
    entry.pair_expr = True
    entry.program = prog
    if uses_tables:
        engine.ctx.pair_expr_set_tables(pid, tables)

    def reload():          # updateParametersInContext: the per-particle parameters (and the tabulated functions) are read again
        fresh = slots()
        if uses_tables:
            engine.ctx.pair_expr_set_tables(pid, tables_checked())
        engine.ctx.pair_set_params(pid, *fresh)
        return 'values'
    entry.reload = reload
    globals_update(entry, prog.globals_, lambda values: engine.ctx.pair_expr_set_globals(pid, values))


def translate_custom_nonbonded(engine, force, entry):
    d = family_of(force)
    if d is None:
        return translate_pair_expression(engine, force, entry)
    d = dict(d)
    if d['family'] == 'ljc':
        raise InputError('the LJC exception expression belongs in a CustomBondForce')
    if engine.free_space:
        if force.getNonbondedMethod() == force.NoCutoff:
            raise InputError('only a NonbondedForce runs without a cutoff (NoCutoff): the near and damped-smoothed energy texts of '
                             'a CustomNonbondedForce are not defined beyond their cutoff -- use CutoffNonPeriodic')
        if d['family'] in ('softcore', 'lj-virial') or force.getNumInteractionGroups() > 0 or d['family'] == 'lj' \
                or d.get('noshift') or d.get('scale_name') or d.get('scale_text'):
            raise NotImplementedError('softcore forces, interaction groups, lj-virial and the alchemical pair forces are not '
                                      'evaluated under a non-periodic nonbonded method (free space)')
    elif force.getNonbondedMethod() != force.CutoffPeriodic:
        raise InputError('the HIP path evaluates CutoffPeriodic CustomNonbondedForces only')
    if d['family'] == 'softcore':
        return translate_softcore(engine, force, entry, d)
    if d['family'] == 'lj-virial':
        return translate_lj_virial(engine, force, entry)
    if d['family'] == 'lj' or d.get('noshift') or d.get('scale_name') or d.get('scale_text') or force.getNumInteractionGroups() > 0:
        return translate_alchemical_pair(engine, force, entry, d)
    if force.getNumInteractionGroups() > 0:
        raise NotImplementedError('interaction groups are supported for the softcore solute-solvent force only')
    if force.getUseLongRangeCorrection():
        raise NotImplementedError('long-range correction is supported for the softcore solute-solvent force only')
    rc = force._cutoff
    for key in ('rc0', 'rs0', 'alpha', 'rswitch', 'Kc'):
        if d.get(key) is None and key in engine.parameters:
            d[key] = engine.parameters[key]
    builtin = force._switch if force.getUseSwitchingFunction() else None
    if builtin is not None and d['family'] != 'damped':
        raise NotImplementedError('built-in switching function on a near force')
    desc = pair_desc_from(d, rc, builtin)
    n = engine.n
    if force.getNumParticles() != n:
        raise mm.OpenMMException('CustomNonbondedForce must have exactly as many particles as the System')
    allp = np.array(force._particles, dtype=np.float64).reshape(n, -1)
    names = list(getattr(force, '_offset_parameters', []))
    base = allp[:, :3]
    scales = np.stack([allp[:, 3 * (k + 1):3 * (k + 2)] for k in range(len(names))]) if names else np.zeros((0, n, 3))
    eff = effective(base, scales, names, engine.parameters)
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    pid = pair_create(engine, desc, eff[:, 0], eff[:, 1], eff[:, 2], excl)
    entry.pair_ids.append(pid)
    if names:
        lam = set(names)

        def update(parameters, changed):
            if not (lam & changed):
                return False
            p = effective(base, scales, names, parameters)
            engine.ctx.pair_set_params(pid, p[:, 0], p[:, 1], p[:, 2])
            return True
        entry.update = update
        entry.depends = set(lam)
        # offsets that touch the charges only: the energy is a quadratic in them (energies_at_states interpolates; energy_derivative
        # keeps its small central step for this force)
        entry.charge_offsets_in = {nm for k, nm in enumerate(names) if not np.any(scales[k][:, 1:])}


def translate_alchemical_pair(engine, force, entry, d, outer=None, outer_depends=()):
    """Pair forces of AlchemicalRespaSystem (systems.py:628-772): force-switched potentials without the constant
    shift, plain Lennard-Jones, optionally restricted to the (solute, solvent) interaction group, optionally
    multiplied by a global parameter (`respa_switch`) and -- as the collective variable of a CustomCVForce -- by
    `outer(parameters)`, the coupling function."""
    n = engine.n
    if getattr(force, '_offset_parameters', []):
        raise NotImplementedError('alchemical pair force with parameter offsets')
    if engine.free_space:
        raise NotImplementedError('alchemical pair forces (interaction groups, coupling factors) are not evaluated under a '
                                  'non-periodic nonbonded method (free space)')
    if force.getNonbondedMethod() != force.CutoffPeriodic:
        raise InputError('the HIP path evaluates CutoffPeriodic CustomNonbondedForces only')
    p = np.array(force._particles, dtype=np.float64).reshape(n, -1)
    if p.shape[1] == 2:                            # per-particle (sigma, epsilon) only: AlchemicalSystem (systems.py:378-379)
        p = np.concatenate([np.zeros((n, 1)), p], axis=1)
    p = p[:, :3]
    q = p[:, 0].copy()
    ngroups = force.getNumInteractionGroups()
    flags, Kc = 0, d.get('Kc', B.KC)
    codes = None
    if ngroups > 1:
        raise NotImplementedError('more than one interaction group')
    sigma, eps = p[:, 1], p[:, 2]
    if ngroups == 1:
        if not (d['family'] == 'lj' or d.get('lj_only') or d.get('coulomb_only')):
            raise NotImplementedError('interaction groups on a force with both electrostatics and Lennard-Jones')
        set1, set2 = force._groups[0]
        if set1 & set2:
            raise NotImplementedError('overlapping interaction-group sets')
        codes = np.zeros(n)
        codes[sorted(set1)] = 1.0
        codes[sorted(set2)] = 2.0
        if d.get('coulomb_only'):      # the expression has no sigma / epsilon: the sigma slot selects the pairs
            sigma, eps = 2.0 * codes, np.zeros(n)
            flags |= B.GROUP_Q
        else:
            q, Kc = codes, 1.0
            flags |= B.GROUP_LJ
    elif d['family'] == 'lj' or d.get('lj_only'):
        q = np.zeros(n)
    rc = force._cutoff
    rswitch = force._switch if force.getUseSwitchingFunction() else None
    scale_name = d.get('scale_name')
    scale_text = d.get('scale_text')
    scale_symbols = X.symbols(scale_text) if scale_text else set()
    for name in scale_symbols:
        if name not in engine.parameters:          # e.g. the reference's `linear` coupling leaves two_pi undefined
            raise mm.OpenMMException('Unknown variable in expression: ' + name)

    def scale(parameters):
        value = d.get('sign', 1.0)
        if scale_name:
            value *= parameters[scale_name]
        if scale_text:
            value *= X.eval_global(scale_text, {k: parameters[k] for k in scale_symbols})
        if outer is not None:
            value *= outer(parameters)
        return value

    if d['family'] == 'lj':
        if rswitch is not None:
            flags |= B.SWITCH
        desc = B.pair_desc(B.NONBONDED, rc, rswitch=rswitch or 0.0, flags=flags, sign=scale(engine.parameters), Kc=Kc)
    elif d['family'] == 'near-force-switch':
        if rswitch is not None:
            raise NotImplementedError('built-in switching function on a force-switched potential')
        if d.get('noshift'):
            flags |= B.NO_SHIFT
        if d.get('guard'):
            flags |= B.GUARD_RC0
        desc = B.pair_desc(B.NEAR_FSWITCH, rc, rc0=d.get('rc0') or rc, rs0=d['rs0'], flags=flags,
                           sign=scale(engine.parameters), Kc=Kc)
    else:
        raise NotImplementedError('alchemical pair family ' + d['family'])
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    pid = pair_create(engine, desc, q, sigma, eps, excl)
    entry.pair_ids.append(pid)
    if d.get('coulomb_only'):
        def reload():          # updateParametersInContext: the charges may have changed (reset_coulomb_scaling_factor)
            fresh = np.array(force._particles, dtype=np.float64).reshape(n, -1)[:, 0]
            engine.ctx.pair_set_params(pid, fresh, sigma, eps)
            return 'values'
        entry.reload = reload
    lrc = 0.0
    if force.getUseLongRangeCorrection():
        if d['family'] != 'lj':
            raise NotImplementedError('long-range correction of this CustomNonbondedForce')
        lrc = custom_long_range_correction(lambda r, s_, e_: 4.0 * e_ * ((s_ / r) ** 12 - (s_ / r) ** 6), p[:, 1], p[:, 2],
                                           engine._box_ref, rc, rswitch, codes)
    entry.constant = lrc * scale(engine.parameters)
    if lrc:
        entry.rescale = lambda: setattr(entry, 'constant', engine._vscale * lrc * scale(engine.parameters))
    depends = set(outer_depends) | ({scale_name} if scale_name else set()) | scale_symbols
    if depends:
        def update(parameters, changed):
            if not (depends & changed):
                return False
            engine.ctx.pair_set_scale(pid, scale(parameters))
            entry.constant = engine._vscale * lrc * scale(parameters)
            return 'values'
        entry.update = update
        entry.depends = set(depends)


def translate_scaled_pair_cv(engine, force, entry):
    """CustomCVForce of AlchemicalRespaSystem (systems.py:738-772): ((gt0-gt1)*S(lambda) + gt1) times ONE collective
    variable, the energy of a CustomNonbondedForce -- i.e. that pair force with a lambda-dependent overall factor."""
    name, inner = force.getCollectiveVariableName(0), force.getCollectiveVariable(0)
    text = force.getEnergyFunction()
    used = X.symbols(text) - {name}
    register_globals(engine, inner)

    def outer(parameters):
        env = {k: parameters[k] for k in used}
        e1 = X.eval_global(text, dict(env, **{name: 1.0}))
        e0 = X.eval_global(text, dict(env, **{name: 0.0}))
        e2 = X.eval_global(text, dict(env, **{name: 2.0}))
        if e0 != 0.0 or abs(e2 - 2.0 * e1) > 1e-12 * max(1.0, abs(e1)):
            raise NotImplementedError('CustomCVForce energy is not proportional to its collective variable')
        return e1
    d = dict(descriptor_of(inner))
    translate_alchemical_pair(engine, inner, entry, d, outer=outer, outer_depends=used)


def translate_lj_virial(engine, force, entry):
    """ComputingSystem's dispersion virial (systems.py:893-897): a CustomNonbondedForce with the cutoff, switch and
    long-range-correction settings imported from the NonbondedForce."""
    n = engine.n
    if force.getNumInteractionGroups() > 0 or getattr(force, '_offset_parameters', []):
        raise NotImplementedError('virial force with interaction groups or parameter offsets')
    p = np.array(force._particles, dtype=np.float64).reshape(n, -1)[:, :3]
    rc = force._cutoff
    rswitch = force._switch if force.getUseSwitchingFunction() else None
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    desc = B.pair_desc(B.LJ_VIRIAL, rc, rswitch=rswitch or 0.0, flags=B.SWITCH if rswitch is not None else 0)
    entry.pair_ids.append(pair_create(engine, desc, p[:, 0], p[:, 1], p[:, 2], excl))
    if force.getUseLongRangeCorrection():
        virial = custom_long_range_correction(
            lambda r, s, e: 24.0 * e * (2.0 * (s / r) ** 12 - (s / r) ** 6), p[:, 1], p[:, 2], engine._box_ref, rc, rswitch)
        entry.constant = virial
        entry.rescale = lambda: setattr(entry, 'constant', engine._vscale * virial)


def translate_softcore(engine, force, entry, d):
    """SolvationSystem's softcore CustomNonbondedForce (systems.py:266-272): one interaction group solute x
    solvent, cutoff / built-in switch / long-range correction imported from the NonbondedForce
    (forces.py:284-291), lambda_vdw a global parameter."""
    n = engine.n
    if force.getNumInteractionGroups() != 1:
        raise NotImplementedError('softcore force: exactly one interaction group is supported')
    set1, set2 = force._groups[0]
    if set1 & set2:
        raise NotImplementedError('softcore force: overlapping interaction-group sets')
    names = list(getattr(force, '_offset_parameters', []))
    allp = np.array(force._particles, dtype=np.float64).reshape(n, -1)
    if allp.shape[1] == 2:                         # per-particle (sigma, epsilon) only: AlchemicalSoftcoreCVForce
        allp = np.concatenate([np.zeros((n, 1)), allp], axis=1)
    base = allp[:, :3]
    scales = np.stack([allp[:, 3 * (k + 1):3 * (k + 2)] for k in range(len(names))]) if names else np.zeros((0, n, 3))
    codes = np.zeros(n)
    codes[sorted(set1)] = 1.0
    codes[sorted(set2)] = 2.0
    lam_name = d['lambda_name']
    if 'lambda_value' in d:                        # a constant written into the expression, not a Context parameter
        lam_name = '__softcore_lambda_%d' % len(engine.entries)
        engine.parameters[lam_name] = float(d['lambda_value'])
    rc = force._cutoff
    rswitch = force._switch if force.getUseSwitchingFunction() else None
    excl = np.array(force._exclusions, dtype=np.int32).reshape(-1, 2)
    eff = effective(base, scales, names, engine.parameters)
    scale_name = d.get('scale_name')
    desc = B.pair_desc(B.SOFTCORE, rc, rswitch=rswitch or 0.0, alpha=engine.parameters[lam_name],
                       flags=B.SWITCH if rswitch is not None else 0, Kc=1.0,
                       sign=engine.parameters[scale_name] if scale_name else 1.0)
    pid = pair_create(engine, desc, codes, eff[:, 1], eff[:, 2], excl)
    entry.pair_ids.append(pid)
    use_lrc = force.getUseLongRangeCorrection()

    class_pairs = {}        # the (sigma, eps) classes depend on the offset parameters only, not on lambda

    def classes_of(parameters):
        key = tuple(parameters[name] for name in names)
        if key not in class_pairs:
            p = effective(base, scales, names, parameters)
            class_pairs.clear()
            class_pairs[key] = [lrc_class_pairs(p[:, 1], p[:, 2], codes), p[:, 1], p[:, 2], None]
        return class_pairs[key]

    def quadrature(parameters, lam_value):
        record = classes_of(parameters)
        return record, softcore_long_range_correction(record[1], record[2], codes, engine._box_ref, rc, rswitch, lam_value, record[0])

    def on_unit_interval(parameters):
        """The correction as a function of lambda on [0, 1] (it is analytic there): a Chebyshev interpolant through 24 of
        the quadrature's values, made once per set of offset parameters -- an AFED step asks for the correction and
        its lambda-derivative some twenty times, at 0.4 ms of host quadrature each otherwise."""
        record = classes_of(parameters)
        if record[3] is None:
            series = np.polynomial.Chebyshev.interpolate(
                lambda nodes: np.array([quadrature(parameters, float(x))[1] for x in nodes]), 23, domain=[0.0, 1.0])
            record[3] = (series, series.deriv())
        return record[3]

    def constant(parameters):
        if not use_lrc:
            return 0.0
        lam_value = parameters[lam_name]
        if 0.0 <= lam_value <= 1.0:
            value = float(on_unit_interval(parameters)[0](lam_value))
        else:
            value = quadrature(parameters, lam_value)[1]
        return engine._vscale * value * (parameters[scale_name] if scale_name else 1.0)

    def constant_derivative(parameters):
        """d(correction)/d(lambda)"""
        if not use_lrc:
            return 0.0
        lam_value = parameters[lam_name]
        if 0.0 <= lam_value <= 1.0:
            value = float(on_unit_interval(parameters)[1](lam_value))
        else:
            h = 1e-6
            value = (quadrature(parameters, lam_value + h)[1] - quadrature(parameters, lam_value - h)[1]) / (2 * h)
        return engine._vscale * value * (parameters[scale_name] if scale_name else 1.0)

    def derivative_polynomial(parameters):
        """d(correction)/d(lambda) on [0, 1] as monomial coefficients in u = 2 lambda - 1 (lowest first), for the evaluation on
        the device while lambda lives there (amm_expr_eval_scalar: Horner) -- the interpolant's derivative, as constant_derivative."""
        if not use_lrc:
            return []
        record = classes_of(parameters)
        if len(record) < 5:          # (made once per set of offset parameters, like the interpolant)
            cheb = np.array(on_unit_interval(parameters)[1].coef, dtype=np.float64)
            # (the trailing Chebyshev terms of an analytic function are below rounding: |T_k| <= 1 bounds what is dropped)
            keep = len(cheb)
            while keep > 1 and np.abs(cheb[keep - 1:]).sum() < 1e-15 * np.abs(cheb).max():
                keep -= 1
            record.append([float(c) for c in np.polynomial.chebyshev.cheb2poly(cheb[:keep])])
        scale = engine._vscale * (parameters[scale_name] if scale_name else 1.0)
        return record[4] if scale == 1.0 else [c * scale for c in record[4]]

    entry.constant = constant(engine.parameters)
    entry.rescale = lambda: setattr(entry, 'constant', constant(engine.parameters))
    lam = set(names) | {lam_name} | ({scale_name} if scale_name else set())
    entry.softcore = dict(pid=pid, lambda_name=lam_name, constant=constant, constant_derivative=constant_derivative, depends=lam,
                          use_lrc=bool(use_lrc), derivative_polynomial=derivative_polynomial)

    def update(parameters, changed):
        if not (lam & changed):
            return False
        if set(names) & changed:
            p = effective(base, scales, names, parameters)
            engine.ctx.pair_set_params(pid, codes, p[:, 1], p[:, 2])
        engine.ctx.pair_set_lambda(pid, parameters[lam_name])
        if scale_name:
            engine.ctx.pair_set_scale(pid, parameters[scale_name])
        entry.constant = constant(parameters)
        return 'values'            # no bond-list terms changed: group definitions stay
    entry.update = update
    entry.depends = set(lam)
