"""What every translator shares: the entry a force becomes, the helpers that create pair forces and bond-list sets, the two
closures that were once copied from translator to translator, and the long-range corrections (host quadratures)."""
import contextlib
import math

import numpy as np

from .. import backend as B
from .. import openmm as mm
from ..forces import describe_energy
from ..utils import InputError

_FAMILY = {'near-none': B.NEAR_NONE, 'near-shift': B.NEAR_SHIFT, 'near-force-switch': B.NEAR_FSWITCH,
           'damped': B.DAMPED}
COMPOUND_KINDS = dict(x=B.CVAR_X, y=B.CVAR_Y, z=B.CVAR_Z, distance=B.CVAR_DISTANCE, angle=B.CVAR_ANGLE, dihedral=B.CVAR_DIHEDRAL)


class _Entry:
    """One System force translated to backend objects."""

    def __init__(self, force, group):
        self.force = force
        self.group = group
        self.pair_ids = []          # backend pair forces (sliced across ranks)
        self.bonded_id = None       # backend bonded set holding this force's bond-list terms
        self.terms = []             # (kind, idx, params, periodic, desc) for group-level merging
        self.constant = 0.0         # energy-only constant (dispersion correction)
        self.recip_group = None
        self.recip = None
        self.update = None          # callable(parameters) refreshing lambda-dependent parameters
        self.softcore = None        # softcore pair force: dict(pid, lambda_name, constant, depends)
        self.depends = set()        # global parameters this entry's backend data depend on
        self.pair_expr = False      # a CustomNonbondedForce on the pair-expression kernel (generic energy text) ...
        self.program = None         # ... and its compiled program (expr.compile_pair)
        self.term_ids = []          # backend term-expression forces (csrc/term_expr.hip): a bond / angle / torsion / external force with
        self.term_expr = False      # a generic energy text; `program` is then that of expr.compile_term
        self.cv = None              # a CustomCVForce on the collective-variable kernel (csrc/cv.hip): dict(id, names, derivs, inner, inner_ids);
                                    # the id is also in term_ids, `program` is that of expr.compile_cv
        self.compound = None        # a CustomCompoundBondForce / CustomCentroidBondForce (csrc/compound.hip): dict(id, variables, centroid);
                                    # the id is also in term_ids, term_expr is set, `program` is that of expr.compile_compound
        self.gb = None              # a GBSAOBCForce (csrc/gb.hip): its backend id, which is also in term_ids
        self.cmap = None            # a CMAPTorsionForce (csrc/cmap.hip): its backend id, which is also in term_ids
        self.custom_gb = None       # a CustomGBForce (csrc/custom_gb.hip): dict(id, n_values); the id is also in term_ids, `program`
                                    # is what expr.compile_custom_gb returned
        self.hbond = None           # a CustomHbondForce (csrc/hbond.hip): dict(id, variables); the id is also in term_ids, term_expr is
                                    # set, `program` is that of expr.compile_hbond
        self.rmsd = None            # an RMSDForce (csrc/rmsd.hip): its backend id, which is also in term_ids
        self.gayberne = None        # a GayBerneForce (csrc/gayberne.hip): its backend id, which is also in term_ids
        self.drude = None           # a DrudeForce (csrc/drude.hip): its backend id, which is also in term_ids
        self.many = None            # a CustomManyParticleForce (csrc/manyparticle.hip): dict(id, variables, types); carried as hbond is,
                                    # `program` is that of expr.compile_many_particle


def globals_update(entry, names, upload):
    """A force whose only dependence on Context parameters is the list of globals its program reads: `upload(values)` hands the
    backend their values, in the order of `names`, whenever one of them changed.  No names: nothing to follow."""
    if not names:
        return
    depends = set(names)

    def update(parameters, changed):
        if not (depends & changed):
            return False
        upload([parameters[g] for g in names])
        return 'values'
    entry.update = update
    entry.depends = depends


def entry_of(engine, force, attr, what):
    """The entry of `force` in this Context -- the one that carries `attr` (None: any) -- or `what`'s refusal."""
    for entry in engine.entries:
        if entry.force is force and (attr is None or getattr(entry, attr, None) is not None):
            return entry
    raise mm.OpenMMException('%s: the force does not belong to this Context' % what)


@contextlib.contextmanager
def backend_refusals(cls):
    """What the library refuses while a force is made or read again, said as an InputError that names the class."""
    try:
        yield
    except B.HipError as exc:
        raise InputError('%s: %s' % (cls, exc))


def register_globals(engine, force):
    if hasattr(force, 'getNumGlobalParameters'):
        for i in range(force.getNumGlobalParameters()):
            engine.parameters.setdefault(force.getGlobalParameterName(i), force.getGlobalParameterDefaultValue(i))


def pair_create(engine, desc, q, sigma, eps, excl):
    if engine.free_space:
        # all pairs at the distance the positions give (csrc/free.hip): no list to build, to share or to count
        desc.flags |= B.FREE_SPACE
        return engine.ctx.pair_create(desc, q, sigma, eps, excl, skin=engine.skin)
    pid = engine.ctx.pair_create(desc, q, sigma, eps, excl, skin=engine.skin)
    key = np.sort(np.sort(np.asarray(excl, dtype=np.int64).reshape(-1, 2), axis=1), axis=0).tobytes()
    # interaction-group forces keep a list of their own: it holds the (set 1, set 2) pairs only
    if desc.family == B.SOFTCORE or desc.flags & (B.GROUP_LJ | B.GROUP_Q):
        key = ('group', pid)
    # a force guarded by step(rc0 - r) reaches rc0 only (the discount of FarNonbondedForce): it can then walk the front part
    # of the total force's rows, and be evaluated on the total's pass
    reach = min(float(desc.rc), float(desc.rc0)) if (desc.flags & B.GUARD_RC0 and desc.rc0 > 0) else float(desc.rc)
    engine._pair_info[pid] = (reach, key)
    return pid


def share_lists(engine):
    """RESPASystem leaves a short-ranged copy (group 1, and its negative in group 31) and the full force over the
    same particles and exclusions: the shorter-ranged ones traverse the front part of the longest-ranged force's
    neighbour rows instead of building lists of their own (amm_pair_share_list)."""
    by_key = {}
    for pid, (rc, key) in engine._pair_info.items():
        by_key.setdefault(key, []).append((rc, pid))
    engine.shared = {}
    for members in by_key.values():
        members.sort(reverse=True)
        host_rc, host = members[0]
        for rc, pid in members[1:]:
            if rc < host_rc:
                try:
                    engine.ctx.pair_share_list(pid, host)
                    engine.shared[pid] = host
                except B.HipError:
                    pass          # incompatible radius with an earlier guest: keeps its own list


def make_bonded(engine, terms, sliced):
    bid = engine.ctx.bonded_create()
    for kind, idx, par, periodic, desc in terms:
        if len(idx):
            engine.ctx.bonded_add_terms(bid, kind, idx, par, periodic=periodic, desc=desc)
    engine.ctx.bonded_finalize(bid, sliced=sliced)
    return bid


def finish_entry(engine, entry):
    if entry.terms:
        entry.bonded_id = make_bonded(engine, entry.terms, sliced=False)


def replace_bonded(engine, entry, terms):
    """New bond-list set of a force whose terms changed; the set it replaces is freed (amm_bonded_release).  The entry's update then
    returns True, not 'values': the engine drops the group definitions that merged the old set (Engine.set_parameter)."""
    old = entry.bonded_id
    entry.bonded_id = make_bonded(engine, terms, sliced=False) if terms else None
    if old is not None:
        engine.ctx.bonded_release(old)


def effective(base, scales, names, parameters):
    """base (n,3) + sum_p lambda_p * scales[p] (n,3): parameter offsets (forces.py:247-258)."""
    out = base.copy()
    for k, name in enumerate(names):
        out += parameters[name] * scales[k]
    return out


def family_of(force):
    """The AtomsMM family of a force's energy text (forces.describe_energy), or None: a text for one of the generic kernels."""
    if getattr(force, '_amm', None) is not None:
        return force._amm
    globs = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i)
             for i in range(force.getNumGlobalParameters())}
    return describe_energy(force.getEnergyFunction(), globs)


def descriptor_of(force):
    desc = family_of(force)
    if desc is None:
        raise InputError('energy expression not recognised by the HIP path (supported: the AtomsMM near / '
                         'damped-smoothed / exception families): ' + force.getEnergyFunction().split(';')[0])
    return desc


def pair_desc_from(d, rc, builtin_switch=None):
    family = d['family']
    flags = B.GUARD_RC0 if d.get('guard') else 0
    if family == 'damped':
        degree = int(d.get('degree', 1))
        rswitch = builtin_switch if (degree == 1 and builtin_switch is not None) else d['rswitch']
        return B.pair_desc(B.DAMPED, rc, rswitch=rswitch, alpha=d['alpha'], degree=degree, sign=d.get('sign', 1.0),
                           Kc=d.get('Kc', B.KC))
    rc0, rs0 = d.get('rc0'), d.get('rs0')
    if rc0 is None or rs0 is None:
        raise InputError('near force without rc0/rs0')
    if d.get('noshift'):
        flags |= B.NO_SHIFT
    return B.pair_desc(_FAMILY[family], rc, rc0=rc0, rs0=rs0, flags=flags, sign=d.get('sign', 1.0), Kc=d.get('Kc', B.KC))


def custom_long_range_correction(u, sigma, eps, box, rc, rswitch, codes=None, pairs=None):
    """Long-range correction of a CustomNonbondedForce as OpenMM defines it [recalled; pinned by tests/test_systems.py:39
    (interaction group, met to 2e-8) and tests/test_computers.py:31 (no groups)]: with I(s, e) = int_rc^inf u r^2 dr +
    int_rs^rc (1 - S) u r^2 dr for a pair of mixed parameters (s, e),
        E = 2 pi N^2 / V * [sum over class pairs of count * I] / (N (N + 1)/2),
    classes = atoms of equal (sigma, epsilon); count = n_i n_j for two classes, n_i (n_i + 1)/2 within a class; with an
    interaction group (`codes` 1 / 2) the count is the number of (set 1, set 2) pairs.  N = number of particles."""
    n = len(sigma)

    def refine(f):
        """OpenMM's quadrature (CustomNonbondedForceImpl::integrateInteraction [recalled]): midpoint rule on (0, 1),
        the number of points tripled (the old midpoints stay) until two sums agree to 1e-5 -- reproduced as is, because
        the reference literals carry ITS truncation error (tests/test_systems.py:39 is met to 1e-9 this way, to 2e-8
        with an exact quadrature; tests/test_computers.py:33 needs the former)."""
        total, points = 0.0, 1
        for iteration in range(9):
            idx = np.arange(points)
            xs = (idx[idx % 3 != 1] + 0.5) / points
            old = total
            total = float(np.sum(f(xs))) / points + old / 3.0
            if iteration > 2 and (total == 0.0 or abs((total - old) / total) < 1e-5):
                return total
            points *= 3
        raise RuntimeError('long-range correction did not converge')

    def integral(s, e):
        def tail(x):                                   # int_rc^inf u r^2 dr = (1/rc) int_0^1 u(rc/x) r^4 dx, r = rc/x
            r = rc / x
            return u(r, s, e) * r ** 4
        out = refine(tail) / rc
        if rswitch is not None:
            def shell(x):                              # int_rs^rc (1 - S) u r^2 dr
                r = rswitch + x * (rc - rswitch)
                return x ** 3 * (10.0 + x * (-15.0 + x * 6.0)) * u(r, s, e) * r * r
            out += refine(shell) * (rc - rswitch)
        return out

    if pairs is None:
        pairs = lrc_class_pairs(sigma, eps, codes)
    total = sum(weight * integral(s, e) for s, e, weight in pairs)
    return 2.0 * math.pi * n * n / float(np.prod(box)) * total / (n * (n + 1) / 2.0)


def lrc_class_pairs(sigma, eps, codes=None):
    """[(sigma_ij, eps_ij, number of pairs)] over the classes of equal (sigma, epsilon) -- the part of a long-range
    correction that depends on the per-particle parameters only (a 250 000-atom system has a handful of classes): the
    softcore force's correction is re-evaluated at every change of lambda, and twice per deriv(energy, lambda)."""
    table = np.stack([np.asarray(sigma, dtype=np.float64), np.asarray(eps, dtype=np.float64)], axis=1)

    def classes(members):
        values, counts = np.unique(table[members], axis=0, return_counts=True)
        return [(float(s_), float(e_), int(c_)) for (s_, e_), c_ in zip(values, counts)]
    out = []
    if codes is not None:
        for s1, e1, n1 in classes(np.where(np.asarray(codes) == 1.0)[0]):
            for s2, e2, n2 in classes(np.where(np.asarray(codes) == 2.0)[0]):
                s, e = 0.5 * (s1 + s2), math.sqrt(e1 * e2)
                if e != 0.0 and s > 0.0:
                    out.append((s, e, n1 * n2))
    else:
        every = classes(np.arange(len(table)))
        for a, (s1, e1, n1) in enumerate(every):
            for s2, e2, n2 in every[a:]:
                s, e = 0.5 * (s1 + s2), math.sqrt(e1 * e2)
                if e != 0.0 and s > 0.0:
                    out.append((s, e, n1 * (n1 + 1) / 2 if (s1, e1) == (s2, e2) else n1 * n2))
    return out


def softcore_long_range_correction(sigma, eps, codes, box, rc, rswitch, lam, pairs=None):
    """SolvationSystem's softcore force (systems.py:266-272): u = 4 lambda eps (1-x)/x^2, x = (r/sigma)^6 + (1-lambda)/2."""
    def u(r, s, e):
        x = (r / s) ** 6 + 0.5 * (1.0 - lam)
        return 4.0 * lam * e * (1.0 - x) / (x * x)
    return custom_long_range_correction(u, sigma, eps, box, rc, rswitch, codes, pairs)


def dispersion_correction(sigma, eps, box, rc, rswitch=None):
    """Long-range LJ correction of OpenMM's NonbondedForce, with the switching-function term
    (SURVEY.md Appendix B.6): (2 pi N^2/V) <int_rc^inf V r^2 dr + int_rs^rc (1-S) V r^2 dr> over type pairs."""
    classes = {}
    for s, e in zip(sigma, eps):
        classes[(s, e)] = classes.get((s, e), 0) + 1
    keys = list(classes)
    n = float(len(sigma))
    total = 0.0
    for a in range(len(keys)):
        for b in range(a, len(keys)):
            e = math.sqrt(keys[a][1] * keys[b][1])
            if e == 0.0:
                continue
            s = 0.5 * (keys[a][0] + keys[b][0])
            s6 = s ** 6
            s12 = s6 * s6
            w = 0.5 * classes[keys[a]] * (classes[keys[a]] + 1) if a == b else float(classes[keys[a]]) * classes[keys[b]]
            term = 4 * e * (s12 / (9 * rc ** 9) - s6 / (3 * rc ** 3))
            if rswitch is not None:
                r = np.linspace(rswitch, rc, 2001)
                t = (r - rswitch) / (rc - rswitch)
                S = 1 + t ** 3 * (15 * t - 6 * t * t - 10)
                g = (1 - S) * 4 * e * (s12 / r ** 12 - s6 / r ** 6) * r * r
                h = r[1] - r[0]
                term += h / 3 * (g[0] + g[-1] + 4 * g[1:-1:2].sum() + 2 * g[2:-1:2].sum())
            total += w * term
    total /= 0.5 * n * (n + 1)
    return 2 * math.pi * n * n * total / (box[0] * box[1] * box[2])
