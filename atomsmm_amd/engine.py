"""Host engine behind `openmm.Context`: turns a System + integrator *description* into calls of the
HIP library (include/atomsmm_hip.h) and takes over what OpenMM's C++ does for the reference
(SURVEY.md section 3.3): per-group force/energy evaluation (`getState(groups=...)`) and execution of
the CustomIntegrator step program (`integrator.step(n)`).

Design (MI355X-first, not OpenMM's):
  * every Force object becomes backend objects once, at Context creation (atomsmm_amd/translate) -- a pair force (cell list ->
    Verlet list -> lanes-per-atom traversal) or bond-list terms (owner-computes CSR);
  * the step program is *unrolled on the host* into a flat op list (EVAL group / KICK / MOVE / COPY)
    with one force cache per group: a group is re-evaluated only if positions changed since its last
    evaluation.  For RespaPropagator([4,2,1]) that is 1/2/8 evaluations of groups 2/1/0 per outer step
    instead of the 2/4/10 OpenMM's single-buffer VM performs, with identical arithmetic;
  * the op list of a steady-state step is cached and replayed by `amm_run_ops` with no Python in the loop;
  * atom decomposition: with torch.distributed initialised (one process per GPU) every rank integrates all
    atoms redundantly, computes pair forces for its slice of the cell-sorted order and all-reduces the
    per-group force buffer over RCCL.

There is no CPU path: creating a Context without the built HIP library or without a GPU raises.
"""
import os
import threading
import math
import re

import numpy as np

from . import backend as B
from . import expr as X
from . import openmm as mm
from . import translate as TR
from . import unit
# (named here by backend.py, scripts/ and the tests of the forces they belong to)
from .translate import MANY_PERMUTATIONS, _Entry, dispersion_correction, gayberne_tables, many_particle_table  # noqa: F401
from .utils import InputError

_SAFE_FUNCS = {name: getattr(math, name) for name in ('sqrt', 'exp', 'log', 'sin', 'cos', 'tan', 'erf', 'erfc', 'floor', 'ceil')}
_SAFE_FUNCS.update(step=lambda x: 1.0 if x >= 0 else 0.0, delta=lambda x: 1.0 if x == 0 else 0.0,
                   select=lambda c, a, b: a if c != 0 else b, min=min, max=max, abs=abs)
ALLREDUCE = 'allreduce'
_AUX_FORCE = re.compile(r'_f[0-9]*_')      # auxiliary buffers of multi-force expressions (integrators.py:134-145)
_NO_ALIAS = os.environ.get('AMM_NO_ALIAS') is not None      # tuning knob (A/B)
# host-walked step programs evaluate the same few dozen texts every step: compiled code, split conditions, symbol lists
_CODE_CACHE, _CONDITION_CACHE, _PER_DOF_SYMBOLS = {}, {}, {}
_SCALARS = 2048        # device scalars of a host-walked program: deriv(energy, p) sums in flight and the globals computed from them
_COMPARE = {'<': lambda a, b: a < b, '>': lambda a, b: a > b, '<=': lambda a, b: a <= b, '>=': lambda a, b: a >= b,
            '=': lambda a, b: a == b, '!=': lambda a, b: a != b}
_context_factory = B.HipContext   # the only backend; tests of the host logic substitute a call recorder


class LocalWorld:
    """W ranks inside ONE process, one thread each, all on the same GPU and the same stream: the multi-rank code path -- slices, exchange
    chunks, amm_exchange_finish, the launches that integrate a rank's own molecules -- with the collectives made by device-to-device
    copies between the ranks' buffers.  For tests at world sizes a one-GPU box cannot host as processes (8 ranks) and for the per-rank
    budgets of DESIGN.md section 5 (scripts/per_rank_step.py): a rank's kernels are the real ones, the exchange costs nothing.

        world = LocalWorld(8)
        results = world.run(lambda rank: job(rank))        # job builds its own Context; Engine finds the world it runs in
    """
    _tls = threading.local()

    def __init__(self, world):
        self.world = int(world)
        self._barrier = threading.Barrier(self.world)
        self._slots = [None] * self.world

    @classmethod
    def current(cls):
        return getattr(cls._tls, 'membership', None)

    def run(self, job):
        results, errors = [None] * self.world, [None] * self.world

        def body(rank):
            LocalWorld._tls.membership = (self, rank)
            try:
                results[rank] = job(rank)
            except BaseException as exc:      # noqa: BLE001 -- reported below; the others must not wait for this rank for ever
                errors[rank] = exc
                self._barrier.abort()
            finally:
                LocalWorld._tls.membership = None
        threads = [threading.Thread(target=body, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        first = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)] or [e for e in errors if e is not None]
        if first:
            raise first[0]
        return results

    def all_gather(self, rank, buf, count):
        """chunk r of every rank's `buf` (count elements each) <- rank r's chunk r."""
        self._slots[rank] = buf
        self._barrier.wait()
        for r in range(self.world):
            if r != rank:
                buf[r * count:(r + 1) * count].copy_(self._slots[r][r * count:(r + 1) * count])
        self._barrier.wait()

    def all_reduce(self, rank, tensor, op='sum'):
        self._slots[rank] = tensor.clone()
        self._barrier.wait()
        total = self._slots[0].clone()
        for r in range(1, self.world):
            total = total + self._slots[r] if op == 'sum' else total.maximum(self._slots[r])
        self._barrier.wait()
        tensor.copy_(total)

    def broadcast(self, rank, value):
        if rank == 0:
            self._slots[0] = value
        self._barrier.wait()
        out = self._slots[0]
        self._barrier.wait()
        return out


def slice_bounds(n_items, rank, world):
    """[begin, end) of rank's contiguous slice of n_items cell-sorted slots: ceil(n / world) each, the same formula as the
    HIP library (csrc/pair.hip first_build).  Atom decomposition: every rank holds all positions and
    integrates all atoms redundantly; the pair work is split by these slices of the cell-sorted order with full neighbour
    rows, so every force row has one producer and the exchange (all-gather of slices, or all-reduce of zero-filled
    buffers) is exact and identical on all ranks."""
    per = (n_items + world - 1) // world      # (bond-list sets: blocks of atom indices; the pair rows use backend.slice_per)
    begin = min(n_items, rank * per)
    return begin, min(n_items, begin + per)


class VectorExpressionError(NotImplementedError):
    """A per-DOF expression with the vector functions dot() / _x() (the atomic regulated baths) that no native op took."""


def _refuse_vector_functions(expr):
    if re.search(r'(?<![A-Za-z_0-9])(dot|_x|_y|_z|cross|vector)\(', expr):
        raise VectorExpressionError('per-DOF expressions with vector functions (dot, _x, ...) run only as the native bath op of the '
                                    'atomic regulated propagators (a global kT and Q, the reference\'s step text); not: ' + expr)


class Engine:
    native_regulated = True       # regulated moves and baths as native ops (False: per-DOF expressions -- a measurement knob)

    stock_native = True           # a stock integrator's post-force update as ONE native op (False: op by op -- set_stock_native)

    def __init__(self, system, integrator, properties):
        import torch
        self.torch = torch
        self.system = system
        # OpenMM's stock integrators (Verlet, Langevin, LangevinMiddle, Brownian): `self.integrator` is their step written as a
        # CustomIntegrator program, made again whenever one of their setters invalidates it (invalidate_program)
        self._stock = integrator if getattr(integrator, '_stock_kind', None) is not None else None
        if self._stock is not None:
            integrator = self._stock._program()
        self.integrator = integrator
        n = system.getNumParticles()
        if n == 0:
            raise mm.OpenMMException('System has no particles')
        mm.check_virtual_sites(system)
        try:
            vecs = system._box
        except AttributeError:
            vecs = None
        # the forces decide the mode: free space (NoCutoff / CutoffNonPeriodic everywhere, no periodic bonded force) or a periodic box
        self.free_space = self._free_space_mode(system, vecs is not None)
        if self.free_space:
            # box vectors, if the System has any, are ignored by the forces: nothing below reads a placeholder
            self.box = self._box_ref = None
        else:
            if vecs is None:
                raise InputError('the HIP path needs a periodic orthorhombic box: call System.setDefaultPeriodicBoxVectors (CutoffPeriodic, '
                                 'Ewald and PME sums need one; only NoCutoff and CutoffNonPeriodic run in free space)')
            for i in range(3):
                for j in range(3):
                    if i != j and abs(vecs[i][j]) > 1e-12:
                        raise InputError('only orthorhombic periodic boxes are supported by the HIP path')
            self.box = np.array([vecs[0][0], vecs[1][1], vecs[2][2]], dtype=np.float64)
            # every long-range-correction constant is proportional to 1 / V: the quadratures are made for the box of creation and their
            # results multiplied by V(creation) / V(now) where they are handed out (set_box)
            self._box_ref = self.box.copy()
        self._vscale = 1.0
        self.barostat = None
        self.rank, self.world = 0, 1
        dist = torch.distributed
        # (ranks as threads of this process: LocalWorld above)
        self._local = None
        member = LocalWorld.current()
        if member is not None and member[0].world > 1:
            self._local, self.rank = member
            self.world = self._local.world
        elif dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            self.rank, self.world = dist.get_rank(), dist.get_world_size()
        # AMM_FORCE_COLLECTIVES=1: a 1-rank job takes the multi-rank code path (collectives over a 1-rank group), to
        # measure its host-side cost on a single GPU
        self._coll = self.world > 1 or (os.environ.get('AMM_FORCE_COLLECTIVES') == '1' and dist.is_available()
                                        and dist.is_initialized())
        TR.check_system(self, system, integrator)
        # the DrudeForce a DrudeLangevinIntegrator steps (check_system: there is exactly one)
        self._drude_force = [f for f in system.getForces() if isinstance(f, mm.DrudeForce)][0] if TR.drude_step_of(self) else None
        self._check_massless(system, integrator)
        if self.free_space and self.world > 1:
            raise InputError('a System in free space (NoCutoff / CutoffNonPeriodic) runs on a single rank: its pair forces walk all pairs '
                             'and are not sliced')
        # (a VerletIntegrator has always been accepted on any number of ranks, where it serves static energies and minimisations:
        # it is refused at its first step instead)
        if self._stock is not None and self.world > 1 and self._stock._stock_kind != 0:
            raise NotImplementedError('stock integrators run on one rank')
        if self.world > 1 and any(k == mm.CustomIntegrator.ComputePerDof and t == 'x' and 'tanh(' in e
                                  for k, t, e in getattr(integrator, '_steps', [])):
            # (the ranks' fused paths -- state exchange, sliced epilogues -- carry plain moves only)
            raise NotImplementedError('regulated dynamics (RegulatedTranslationPropagator) runs on one rank only')
        device = int(properties.get('DeviceIndex', torch.cuda.current_device() if torch.cuda.is_available() else 0))
        self.ctx = _context_factory(n, self.box, device=device, rank=self.rank, world=self.world)
        self.n = n
        self._native_comm = False
        self._native_ops = {}
        if self._coll and self._local is None and hasattr(self.ctx, 'comm_init') and dist.get_backend() == 'nccl' \
                and os.environ.get('AMM_NATIVE_COMM', '1') != '0':
            self._init_native_comm(dist)
        dev = self.ctx.torch_device
        f64 = torch.float64
        # exchange of the owner-computed force slices: all-gather of the slices in cell-sorted order (1/world of the bytes
        # of the all-reduce of zero-filled buffers; AMM_EXCHANGE=reduce keeps the latter) for groups of ONE pair force
        self._gather = self._coll and hasattr(self.ctx, 'bind_exchange') and os.environ.get('AMM_EXCHANGE', 'gather') == 'gather'
        self._gather_groups = set()
        if self._gather:
            self._per = B.slice_per(n, self.world)
            self._xchg = torch.zeros(self.world * 2 * self._per * 3, dtype=f64, device=dev)
            self.ctx.bind_exchange(self._xchg)
        self.x = torch.zeros((n, 3), dtype=f64, device=dev)
        self.v = torch.zeros((n, 3), dtype=f64, device=dev)
        self.mass = torch.as_tensor(np.array(system._masses, dtype=np.float64), device=dev)
        self.time = 0.0
        self.parameters = {}
        self.entries = []
        self.skin = float(properties.get('Skin', -1.0))
        # The engine is the only writer of the bound position buffer outside the library (set_positions): amm_run_ops may trust
        # the displacement checks its own launches made at the end of the previous call
        if hasattr(self.ctx, 'positions_changed'):
            self.ctx.set_option('positions_private', 1)
        # 'Option.<name>': tuning / test options of the library context (include/atomsmm_hip.h: amm_set_option)
        for key, value in properties.items():
            if key.startswith('Option.') and hasattr(self.ctx, 'set_option'):
                self.ctx.set_option(key[len('Option.'):], float(value))
        if float(properties.get('OuterSkin', -1.0)) > 0:       # dual Verlet list: cell-built outer list pruned to the inner one
            self.ctx.set_outer_skin(float(properties['OuterSkin']))
        self._pair_info = {}
        for force in system.getForces():
            TR.translate(self, force)
        TR.share_lists(self)
        self._slots = {}
        self._buffers = {}
        self._arena_free = []
        self._arena_contiguous = True
        self._group_defs = {}
        self._group_bonded = []     # merged bond-list sets made by _define_group
        self._deriv_cache = {}      # deriv(energy, name) at the current positions and parameters (host-walked programs)
        self._emit_memo = {}        # what the per-DOF steps of a host-walked program emit (_emit_per_dof_memo)
        self._segment_memo, self._segment_ends, self._segment_symbols, self._segment_open = {}, {}, {}, None      # ... and whole runs of them
        self._pending = None        # device scalars that deferred globals wait for: (buffer, number in use)
        self._device_params = {}    # Context parameters whose number is a device scalar for now (name -> [pair force ids]): AFED's lambda
        self._scalar_code, self._scalar_consts = [], []      # assignments to device scalars not yet launched (one launch per batch)
        self._lrc_on_device = {}    # (pair force, lambda's scalar) -> the correction's lambda-derivative there
        self.n_scalar_evals = self.n_scalar_launches = self.n_settles = 0     # (tests / bench: global expressions evaluated on the device, blocking reads of the scalars)
        self.n_state_fallbacks = 0  # energies_at_states calls that took the reference loop for some force
        self.state_paths = dict(once=0, states=0, quadratic=0, loop=0)      # ... and the forces each of its paths served
        self.device_globals = True  # nonlinear uses of deferred globals are evaluated on the device (amm_expr_eval_scalar) instead of waited for
        self._valid = {}
        self._interpreted = None    # None: undecided; True: general (host-walked) step programs
        self._static_exprs = False
        self._expr_ids = {}
        self._seed_set = None
        self._host_rng = None
        self._expr_counter = 0
        self._mirror = {}           # per-DOF buffer -> force symbol it currently mirrors (`_f2_ <- f2`)
        self._programs = {}
        self._energy = torch.zeros(1, dtype=f64, device=dev)
        self._fwork = torch.zeros((n, 3), dtype=f64, device=dev)
        self._fwork2 = torch.zeros((n, 3), dtype=f64, device=dev)
        self.ctx.bind_state(self.x, self.v, self.mass)
        self._define_vsites(system)
        self._has_constraints = system.getNumConstraints() > 0
        if self._has_constraints:
            cons = system._constraints
            self.ctx.constraints_create(np.array([[c[0], c[1]] for c in cons], dtype=np.int32), np.array([c[2] for c in cons]),
                                        integrator.getConstraintTolerance() if hasattr(integrator, 'getConstraintTolerance') else 1e-5)
        if isinstance(integrator, mm.CustomIntegrator):
            integrator._n_hint = n
        if self.barostat is not None:
            self._init_barostat()

    def _check_massless(self, system, integrator):
        """Massless particles (virtual sites among them) never move: the stock integrators, plain kicks and moves, the
        Ornstein-Uhlenbeck bath and per-DOF expressions skip them as OpenMM does.  What has not learnt the rule is refused by name."""
        self._massless = bool(getattr(system, '_vsites', None)) or any(m == 0.0 for m in system._masses)
        if not self._massless:
            return
        texts = [e.replace(' ', '') for _, _, e in getattr(integrator, '_steps', []) if isinstance(e, str)]
        what = None
        if any(c.__name__ == 'AdiabaticDynamicsIntegrator' for c in type(integrator).__mro__):
            what = 'AdiabaticDynamicsIntegrator'
        elif any(c.__name__ == 'ComputingSystem' for c in type(system).__mro__):
            what = 'ComputingSystem / PressureComputer'
        elif self.world > 1:
            what = 'a run on several ranks'
        elif any('deriv(energy' in t for t in texts):
            what = 'a step program with deriv(energy, ...) steps'
        elif any('cosh(z)' in t and 'LkT' in t for t in texts):
            what = 'the SIN(R) / isokinetic path'
        elif any('tanh(' in t for t in texts):
            what = 'the regulated path'
        elif any(self._NHL_UPDATE.fullmatch(t) for t in texts):
            what = 'the native Nose-Hoover-Langevin bath'
        if what is not None:
            raise InputError('a System with massless particles or virtual sites does not run with %s' % what)

    def drude_pairs(self):
        """int32 [P][2]: (Drude particle, parent) of the DrudeForce a DrudeLangevinIntegrator steps."""
        return np.array([r[:2] for r in self._drude_force._particles], dtype=np.int32).reshape(-1, 2)

    def drude_temperatures(self):
        """(system temperature, Drude temperature) in K of a DrudeLangevinIntegrator's System: one read of the stored velocities, summed
        on the host.  System: sum of m v^2 over ordinary massive atoms plus M v_cm^2 over pairs, over dof k_B with dof = 3 per ordinary
        massive atom + 3 per pair - constraints - 3 with a CMMotionRemover.  Drude: sum of m_red v_rel^2 over pairs, over 3 n_pairs k_B."""
        if self._drude_force is None:
            raise mm.OpenMMException('computeSystemTemperature / computeDrudeTemperature need a DrudeLangevinIntegrator')
        v = self.v.cpu().numpy().astype(np.float64)
        m = np.array(self.system._masses, dtype=np.float64)
        pairs = self.drude_pairs()
        both = np.array([m[p] > 0.0 and m[p1] > 0.0 for p, p1 in pairs], dtype=bool).reshape(-1)
        pairs = pairs[both]
        p, p1 = pairs[:, 0], pairs[:, 1]
        ordinary = m > 0.0
        ordinary[p] = False
        ordinary[p1] = False
        M = m[p] + m[p1]
        mu = m[p] * m[p1] / M
        vcm = (m[p, None] * v[p] + m[p1, None] * v[p1]) / M[:, None]
        vrel = v[p] - v[p1]
        ke2 = float((m[ordinary, None] * v[ordinary] ** 2).sum() + (M[:, None] * vcm ** 2).sum())
        dof = 3 * int(ordinary.sum()) + 3 * len(pairs) - self.system.getNumConstraints()
        if any(isinstance(f, mm.CMMotionRemover) for f in self.system.getForces()):
            dof -= 3
        kB = unit.BOLTZMANN_CONSTANT_kB._value
        t_sys = ke2 / (dof * kB) if dof > 0 else 0.0
        t_drude = float((mu[:, None] * vrel ** 2).sum()) / (3 * len(pairs) * kB) if len(pairs) else 0.0
        return t_sys, t_drude

    def _define_vsites(self, system):
        sites = sorted(getattr(system, '_vsites', {}).items())
        if sites:
            parents = np.full((len(sites), 3), -1, dtype=np.int32)
            weights = np.zeros((len(sites), 3))
            for row, (_, site) in enumerate(sites):
                parents[row, :site.getNumParticles()] = site._particles
                weights[row, :len(site._weights)] = site._weights
            self.ctx.vsite_define([index for index, _ in sites], [site._kind for _, site in sites], parents, weights)
        elif self._massless and hasattr(self.ctx, 'set_fuse_inner'):
            # (the fused launches of amm_run_ops divide by every mass; with sites defined the library keeps them out itself)
            self.ctx.set_fuse_inner(False)
        self._has_vsites = bool(sites)

    def compute_virtual_sites(self):
        if self._has_vsites:
            self.ctx.vsite_place(self.x)
            self._invalidate_forces()

    # what translation owns and callers name on the class (atomsmm_amd/translate)
    _free_space_mode = staticmethod(TR.free_space_mode)
    _translate_cv = TR.translate_cv
    check_pair_symmetry = staticmethod(TR.check_pair_symmetry)
    check_custom_gb_symmetry = staticmethod(TR.check_custom_gb_symmetry)
    GAYBERNE_MAX, RB_TEXT, _CV_INNER_CLASSES = TR.GAYBERNE_MAX, TR.RB_TEXT, TR.CV_INNER_CLASSES

    def custom_gb_values(self, force):
        """CustomGBForce.getComputedValues(context): the computed values at the current positions, [value][particle]."""
        cg = TR.entry_of(self, force, 'custom_gb', 'getComputedValues').custom_gb
        out = self.ctx.custom_gb_values(cg['id'], self.x, cg['n_values'])
        self._check()
        return out

    def hbond_stats(self, force):
        """dict(scanned, survivors, launches, chunks) of a CustomHbondForce of this Context (backend.HipContext.hbond_stats)."""
        return self.ctx.hbond_stats(TR.entry_of(self, force, 'hbond', 'hbond_stats').hbond['id'])

    def many_stats(self, force):
        """dict(particles, sets, launches, fullest, capacity) of a CustomManyParticleForce of this Context (backend.HipContext.many_stats)."""
        return self.ctx.many_stats(TR.entry_of(self, force, 'many', 'many_stats').many['id'])

    def gayberne_stats(self, force):
        """dict(active, scanned, survivors, launches, chunks) of a GayBerneForce of this Context (backend.HipContext.gayberne_stats)."""
        return self.ctx.gayberne_stats(TR.entry_of(self, force, 'gayberne', 'gayberne_stats').gayberne)

    # ------------------------------------------------------------------------------- constant pressure
    def _init_barostat(self):
        """A MonteCarloBarostat in the System: what it cannot run with is refused here, when the Context is created."""
        integ = self.integrator
        if self.world > 1:
            raise InputError('a MonteCarloBarostat runs on a single rank')
        steps = getattr(integ, '_steps', [])
        if any(k == mm.CustomIntegrator.ComputePerDof and t == 'x' and 'tanh(' in e for k, t, e in steps):
            raise NotImplementedError('a MonteCarloBarostat with regulated dynamics (RegulatedTranslationPropagator) is not supported')
        # OpenMM makes the attempt at the program's UpdateContextState step (at its start when it has none); here it is made before
        # the step: the same thing unless a step ahead of UpdateContextState moves x or reads a force or an energy
        ahead = []
        for kind, target, expr in steps:
            if kind == mm.CustomIntegrator.UpdateContextState:
                break
            ahead.append((kind, target, expr))
        else:
            ahead = []
        for kind, target, expr in ahead:
            moves = kind == mm.CustomIntegrator.ConstrainPositions or (kind == mm.CustomIntegrator.ComputePerDof and target == 'x')
            reads = bool(re.search(r'(?<![A-Za-z_0-9])(f|energy)[0-9]*(?![A-Za-z_0-9])', expr or ''))
            if moves or reads:
                raise NotImplementedError('MonteCarloBarostat: the step program moves x or reads a force or an energy ahead of its '
                                          'UpdateContextState step; only programs whose attempt can be made before the step are supported')
        molecules = mm.molecules_of(self.system)
        self.ctx.mol_define(molecules)
        self._n_molecules = len(molecules)
        # (device-resident extended variables would carry 1 / V in the coefficients of their correction polynomials across an
        # attempt: with a barostat such globals are waited for instead)
        self.device_globals = False
        seed = self.barostat.getRandomNumberSeed()
        self._baro_rng = np.random.default_rng(seed if seed != 0 else None)
        self._baro_due = None           # steps that run before the next attempt (None: frequency - 1, decided at the first step)
        self._baro_scale = None         # volumeScale (nm^3; 1 % of the volume at the first attempt)
        self._baro_window = [0, 0]      # attempts / acceptances since the step size last changed
        self.barostat_stats = dict(attempts=0, accepted=0)
        self.barostat_log = []          # per attempt: (accepted, w, u2 or None, box edges afterwards) -- the last 1024
        self._x_saved = self.torch.zeros_like(self.x)

    def _refuse_in_free_space(self, what):
        if self.free_space:
            raise NotImplementedError(what + ' is not available for a System in free space (NoCutoff / CutoffNonPeriodic): its pair '
                                      'forces have no parameter-derivative or multi-state evaluation')

    def set_box(self, edges):
        """New box edges (nm) for the live context: Context.setPeriodicBoxVectors.  Positions are not touched.  Every 1 / V constant
        follows and forces and derivative caches become stale.  Compiled step programs stay: they hold no such constant (a program
        that reads an energy is walked by the host, which asks the entries for their constants as it goes).  The PME mesh and alpha
        stay as chosen at creation, as in OpenMM."""
        if self.free_space:
            raise InputError('a Context in free space (NoCutoff / CutoffNonPeriodic) has no periodic box to change')
        if self.world > 1:
            raise InputError('changing the box of a live Context runs on a single rank')
        edges = np.array(edges, dtype=np.float64).reshape(3)
        if not np.all(edges > 0):
            raise InputError('box edges must be positive')
        if np.array_equal(edges, self.box):
            return
        if self._pending is not None and self._pending[1]:
            # (nothing is pending between two steps today; should that change, the integrator's globals hold such scalars too)
            self._settle([getattr(self.integrator, '_gvalues', []), self.parameters])
        self.ctx.set_box(edges)         # (raises, and keeps the old box, when a cutoff exceeds half an edge)
        self.box = edges
        self._vscale = float(np.prod(self._box_ref) / np.prod(edges))
        for entry in self.entries:
            rescale = getattr(entry, 'rescale', None)
            if rescale is not None:
                rescale()
        self._lrc_on_device = {}
        self._invalidate_forces()

    def _potential_energy(self):
        """The potential energy of all force groups with ONE wait for the device: every term adds to one scalar there.  Behind that
        wait amm_check reads the flag block of every built list (64 bytes each, the stream is idle by then) and the scalar is
        read: one pipeline drain, 1 + (lists built) small copies."""
        e = self._energy.zero_()
        fp = self._fwork.zero_()
        const = 0.0
        for entry in self.entries:
            for pid in entry.pair_ids:
                self.ctx.force_eval(pid, self.x, fp, accumulate=True, energy=e)
            if entry.bonded_id is not None:
                self.ctx.force_eval(entry.bonded_id, self.x, fp, accumulate=True, energy=e)
            for tid in entry.term_ids:
                self.ctx.force_eval(tid, self.x, fp, accumulate=True, energy=e)
            if entry.recip is not None:
                self.ctx.force_eval(entry.recip, self.x, fp, accumulate=True, energy=e)
            const += entry.constant
        self._check()
        return e.item() + const

    def _barostat_attempt(self):
        """One Monte Carlo volume move [OpenMM: MonteCarloBarostatImpl::updateContextState]: two energy evaluations, each read with
        one wait for the device (_potential_energy): two pipeline drains per attempt."""
        baro = self.barostat
        pressure = self.parameters[baro.Pressure()] * unit.bar.scale         # bar -> kJ/mol/nm^3 (N_A 1e-25)
        kT = unit.MOLAR_GAS_CONSTANT_R._value * self.parameters[baro.Temperature()]
        e0 = self._potential_energy()
        box0 = self.box.copy()
        volume = float(np.prod(box0))
        if self._baro_scale is None:
            self._baro_scale = 0.01 * volume
        delta = self._baro_scale * 2.0 * (self._baro_rng.random() - 0.5)
        new_volume = volume + delta
        s = (new_volume / volume) ** (1.0 / 3.0)
        valid = dict(self._valid)
        self.set_box(box0 * s)
        self.ctx.mol_scale(self.x, [s, s, s], self._x_saved)
        if self._has_vsites:
            self.ctx.vsite_place(self.x)
        e1 = self._potential_energy()
        w = e1 - e0 + pressure * delta - self._n_molecules * kT * math.log(new_volume / volume)
        u2 = None
        accepted = True
        if w > 0:
            u2 = self._baro_rng.random()
            accepted = not u2 > math.exp(-w / kT)
        if not accepted:
            # the saved bits and the old box: the force buffers that were valid before the attempt are valid again
            self.ctx.copy(self.x, self._x_saved)
            self.ctx.positions_changed()
            self.set_box(box0)
            self._valid.update(valid)
        self.barostat_stats['attempts'] += 1
        self.barostat_stats['accepted'] += int(accepted)
        self.barostat_log.append((accepted, w, u2, self.box.copy()))
        del self.barostat_log[:-1024]
        self._baro_window[0] += 1
        self._baro_window[1] += int(accepted)
        if self._baro_window[0] >= 10:
            attempts, hits = self._baro_window
            if hits < 0.25 * attempts:
                self._baro_scale /= 1.1
                self._baro_window = [0, 0]
            elif hits > 0.75 * attempts:
                self._baro_scale = min(self._baro_scale * 1.1, 0.3 * float(np.prod(self.box)))
                self._baro_window = [0, 0]

    def collective_variable_values(self, force):
        """CustomCVForce.getCollectiveVariableValues(context): the energies of the inner forces at the current positions."""
        cv = TR.entry_of(self, force, None, 'getCollectiveVariableValues').cv
        if cv is None:
            raise NotImplementedError('getCollectiveVariableValues of a CustomCVForce over a CustomNonbondedForce (the pattern of '
                                      'AlchemicalRespaSystem runs as a scaled pair force: its collective variable is never formed)')
        values = self.ctx.cv_values(cv['id'], self.x, len(cv['names']))
        self._check()
        return tuple(float(v) for v in values)

    # ------------------------------------------------------------------------------- state
    def _invalidate_forces(self):
        for g in self._valid:
            self._valid[g] = False
        self._deriv_cache.clear()

    def set_positions(self, arr):
        self.x.copy_(self.torch.as_tensor(arr, device=self.x.device))
        if hasattr(self.ctx, 'positions_changed'):
            self.ctx.positions_changed()
        self._invalidate_forces()

    def set_velocities(self, arr):
        self.v.copy_(self.torch.as_tensor(arr, device=self.v.device))

    def _forget_groups(self):
        """Group definitions are stale (an entry's update or reload rebuilt its bond-list terms): drop them and free the merged sets
        they owned."""
        for bid in self._group_bonded:
            self.ctx.bonded_release(bid)
        del self._group_bonded[:]
        self._group_defs.clear()

    def set_parameter(self, name, value):
        if name not in self.parameters:
            raise mm.OpenMMException('Called setParameter() with invalid parameter name: ' + name)
        if self.parameters[name] == value:
            return
        self.parameters[name] = value
        changed = {name}
        groups, rebuilt = set(), False
        for entry in self.entries:
            if entry.update is not None:
                result = entry.update(self.parameters, changed)
                if result:
                    groups.add(entry.group)
                    if getattr(entry, 'recip', None) is not None:
                        groups.add(entry.recip_group)
                    if result != 'values':
                        rebuilt = True
                        self._forget_groups()       # bond-list terms were rebuilt
        if rebuilt:
            self._programs.clear()
            self._emit_memo.clear()
            self._segment_memo.clear()
            self._invalidate_forces()
        elif groups:
            # only VALUES changed (an extended variable moved: AFED sets lambda_vdw twice per step): the forces of the groups that
            # hold a force that depends on it are stale -- the other groups' buffers, the compiled programs and what the step
            # programs emit are not (invalidating everything cost config C5 a fifth outer + near evaluation per AFED step)
            for g in self._valid:
                if g in groups or g == 'all':
                    self._valid[g] = False
            self._deriv_cache.clear()
            self._programs.clear()          # (compiled programs may hold coefficients that name the parameter; the memos of the
                                            # host-walked path are keyed by the values of the globals they name)

    def get_parameter(self, name):
        return self.parameters[name]

    def update_force_parameters(self, force):
        """`force.updateParametersInContext(context)`: per-particle (and exception) parameters of an existing force are
        uploaded again -- what AlchemicalRespaSystem.reset_coulomb_scaling_factor relies on (systems.py:806-815)."""
        reload = getattr(TR.entry_of(self, force, None, 'updateParametersInContext'), 'reload', None)
        if reload is None:
            raise NotImplementedError('updateParametersInContext for ' + type(force).__name__ + ' with this energy expression')
        result = reload()
        if result:
            if result != 'values':
                self._forget_groups()
            self._programs.clear()
            self._emit_memo.clear()
            self._segment_memo.clear()
            self._invalidate_forces()

    def invalidate_program(self):
        self._programs.clear()
        self._emit_memo.clear()
        self._segment_memo.clear()
        self._interpreted = None
        if self._stock is not None:
            self.integrator = self._stock._program()

    def set_stock_native(self, on=True):
        """Stock integrators: True (the default) runs the post-force update of a step as one AMM_OP_STOCK launch, False emits the
        same step from the existing ops (KICK, CONSTRAIN_V, MOVE, BATH / EXPR, COPY, CONSTRAIN_X, EXPR) -- the fallback for a
        backend without the op, and what the fused step is compared against."""
        self.stock_native = bool(on)
        self.invalidate_program()

    def set_constraint_tolerance(self, tol):
        """setConstraintTolerance of a bound stock integrator: the solver's tolerance lives in the library's constraint set."""
        if self._has_constraints:
            if hasattr(self.ctx, 'constraints_set_tolerance'):
                self.ctx.constraints_set_tolerance(float(tol))
            else:
                cons = self.system._constraints
                self.ctx.constraints_create(np.array([[c[0], c[1]] for c in cons], dtype=np.int32), np.array([c[2] for c in cons]), float(tol))
        self.invalidate_program()

    def reinitialize(self, preserveState=False):
        raise NotImplementedError('Context.reinitialize: create a new Context instead')

    # per-DOF variables live in named device buffers
    def _buffer(self, name, together=()):
        """Per-DOF buffer `name`.  Buffers are carved from arenas; `together` names buffers to create in the same breath as
        neighbours in memory: the force buffers of the sliced groups, whose all-reduces then travel as one message when
        they follow one another (AMM_OP_ALLREDUCE)."""
        if name not in self._buffers:
            names = [name] + [other for other in together if other != name and other not in self._buffers]
            if len(self._arena_free) < len(names) or (len(names) > 1 and not self._arena_contiguous):
                count = max(8, len(names))
                arena = self.torch.zeros((count, self.n, 3), dtype=self.torch.float64, device=self.x.device)
                leftovers = self._arena_free
                self._arena_free = [arena[k] for k in range(count)]
                self._arena_contiguous = True
            else:
                leftovers = []
            integ = self.integrator
            for nm in sorted(names):
                t = self._arena_free.pop(0)
                if isinstance(integ, mm.CustomIntegrator) and nm in integ._pnames:
                    t.fill_(integ._pvalues[integ._pnames.index(nm)])
                self._buffers[nm] = t
            if leftovers:
                self._arena_free += leftovers
                self._arena_contiguous = False
        return self._buffers[name]

    def fill_per_dof(self, name, value):
        self._buffer(name).fill_(value)
        self._mirror.pop(name, None)

    def get_per_dof(self, name):
        src = self._mirror.get(name)
        if src is not None and _AUX_FORCE.fullmatch(name) and src in self._buffers and not _NO_ALIAS:
            self._buffer(name).copy_(self._buffers[src])        # its copy op may have been dropped (_drop_dead_copies)
        return [mm.Vec3(*row) for row in self._buffer(name).cpu().numpy().tolist()]

    def set_per_dof(self, name, values):
        arr = np.array([list(v) for v in values], dtype=np.float64).reshape(self.n, 3)
        self._buffer(name).copy_(self.torch.as_tensor(arr, device=self.x.device))
        self._mirror.pop(name, None)

    # ------------------------------------------------------------------------------- getState
    def _check(self):
        """amm_check on every rank TOGETHER: a neighbour-row overflow or a constraint failure is detected by the rank
        that owns the row, and a rank that raised alone would leave its peers inside the next collective."""
        if not self._coll:
            if self._drude_force is None:
                return self.ctx.check()
            try:
                return self.ctx.check()
            except B.HipError as exc:      # (the hard wall of a DrudeLangevinIntegrator speaks as OpenMM does)
                if 'Drude particle moved too far beyond hard wall constraint' in str(exc):
                    raise mm.OpenMMException('Drude particle moved too far beyond hard wall constraint')
                raise
        err = None
        try:
            self.ctx.check()
        except Exception as exc:       # noqa: BLE001 -- re-raised below, on every rank
            err = exc
        if self._local is not None:
            flag = self.torch.tensor([1 if err is not None else 0], dtype=self.torch.int32)
            self._local.all_reduce(self.rank, flag, op='max')
            if err is not None:
                raise err
            if int(flag.item()):
                raise B.HipError('another rank reported a failed check (neighbour-row overflow or constraint failure)')
            return
        dist = self.torch.distributed
        flag = self.torch.tensor([1 if err is not None else 0], dtype=self.torch.int32,
                                 device=self.x.device if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        if err is not None:
            raise err
        if int(flag.item()):
            raise B.HipError('another rank reported a failed check (neighbour-row overflow or constraint failure)')

    def broadcast_from_rank0(self, array):
        """A host array every rank must hold bit for bit (e.g. randomly drawn velocities): rank 0's copy wins."""
        if not self._coll:
            return array
        if self._local is not None:
            return np.array(self._local.broadcast(self.rank, np.ascontiguousarray(array, dtype=np.float64)))
        dist = self.torch.distributed
        t = self.torch.as_tensor(np.ascontiguousarray(array, dtype=np.float64),
                                 device=self.x.device if dist.get_backend() == 'nccl' else 'cpu')
        dist.broadcast(t, src=0)
        return t.cpu().numpy()

    def _allreduce(self, tensor):
        if self._coll:
            if self._local is not None:
                self._local.all_reduce(self.rank, tensor)
            elif self._native_comm:
                self.ctx.comm_allreduce(tensor)
            else:
                self.torch.distributed.all_reduce(tensor)

    def get_state(self, want_pos, want_vel, want_forces, want_energy, mask):
        torch = self.torch
        energy = forces = None
        if want_forces or want_energy:
            e_pair = self._energy.zero_() if want_energy else None
            fp = self._fwork.zero_()
            fb = self._fwork2.zero_()
            e_bond = torch.zeros(1, dtype=torch.float64, device=self.x.device) if want_energy else None
            const = 0.0
            for entry in self.entries:
                if mask & (1 << entry.group):
                    for pid in entry.pair_ids:
                        self.ctx.force_eval(pid, self.x, fp, accumulate=True, energy=e_pair)
                    if entry.bonded_id is not None:
                        self.ctx.force_eval(entry.bonded_id, self.x, fb, accumulate=True, energy=e_bond)
                    for tid in entry.term_ids:
                        self.ctx.force_eval(tid, self.x, fb, accumulate=True, energy=e_bond)
                    const += entry.constant
                if entry.recip is not None and mask & (1 << entry.recip_group):
                    # reciprocal space: every rank evaluates all of it (spread + FFTs are not sharded)
                    self.ctx.pme_set_sliced(entry.recip, False)
                    self.ctx.force_eval(entry.recip, self.x, fb, accumulate=True, energy=e_bond)
                    self.ctx.pme_set_sliced(entry.recip, getattr(entry, 'recip_sliced', False))
            self._check()
            if self._coll:
                self._allreduce(fp)
                if want_energy:
                    self._allreduce(e_pair)
            if want_forces:
                total = fp + fb
                if self._has_vsites:          # what the sites collected goes to their parents
                    self.ctx.vsite_spread(self.x, total)
                forces = total.cpu().numpy()
            if want_energy:
                energy = e_pair.item() + e_bond.item() + const
        kinetic = None
        if want_energy:
            out = torch.zeros(1, dtype=torch.float64, device=self.x.device)
            expression = getattr(self.integrator, '_kinetic', None)
            if expression is None:
                self.ctx.mvv(self.v, self.mass, out)
                kinetic = 0.5 * out.item()
            else:
                kinetic = self._kinetic_energy(expression, out)
        pos = self.x.cpu().numpy() if want_pos else None
        vel = self.v.cpu().numpy() if want_vel else None
        box = None if self.box is None else [(self.box[0], 0, 0), (0, self.box[1], 0), (0, 0, self.box[2])]
        return mm.State(energy, kinetic, forces, pos, vel, box, self.time)

    def _kinetic_energy(self, expression, out):
        """The integrator's kinetic-energy expression (setKineticEnergyExpression: the regulated propagators' sum of
        m (c tanh(alpha v/c))^2 / 2) summed over the degrees of freedom on the device."""
        integ = self.integrator
        env = dict(self.parameters)
        env.update(zip(integ._gnames, integ._gvalues))

        def resolve(name):
            if name == 'm':
                return ('mass',)
            if name == 'v':
                return ('buf', B.SLOT_V)
            if name == 'x':
                return ('buf', B.SLOT_X)
            if name in integ._pnames:
                return ('buf', self._slot(name))
            if name in env:
                return ('global',)
            return None
        prog = X.compile_per_dof(expression, resolve)
        # (counter 0: the expression draws no random numbers, and the program's random stream is left where it is)
        self.ctx.expr_eval(prog.code, prog.consts, [float(env[name]) for name in prog.globals_], 0, 0, total=out)
        return out.item()

    # ------------------------------------------------------------------------------- step programs
    def _slot(self, name):
        """Slot index of a named per-DOF buffer ('f3' = force of group 3, other names = per-DOF variables)."""
        if name == 'x':
            return B.SLOT_X
        if name == 'v':
            return B.SLOT_V
        if name not in self._slots:
            slot = len(self._slots)
            if slot >= B.SLOT_X:
                raise NotImplementedError('too many per-DOF buffers')
            self._slots[name] = slot
            self.ctx.bind_buffer(slot, self._buffer(name))
        return self._slots[name]

    def _define_group(self, g):
        """Backend group g = pair forces + one merged bonded set of all bond-list terms in the group."""
        if g in self._group_defs:
            return self._group_defs[g]
        members = [e for e in self.entries if (e.group == g if g != 'all' else True)]
        pair_ids = [pid for e in members for pid in e.pair_ids]
        terms = [t for e in members for t in e.terms]
        # multi-rank: a group is evaluated slice-wise and all-reduced as soon as it holds a pair force OR a reciprocal-space
        # force -- the "sliced" switch lives on the PME object, so it must mean the same in every group that evaluates it
        has_recip = any(e.recip is not None and (g == 'all' or e.recip_group == g) for e in self.entries)
        reduced = self._coll and (bool(pair_ids) or has_recip)
        gather = reduced and self._gather and g != 'all' and len(pair_ids) == 1 and not terms and not any(
            e.recip is not None and e.recip_group == g for e in self.entries)
        # a hybrid list (molecule rows + per-atom rows for the atoms outside the three-site molecules) has two sorted orders:
        # its forces are exchanged by all-reduce
        if gather and self.ctx.pair_stats(pair_ids[0]).get('n_rest_atoms', 0) > 0:
            gather = False
        ids = list(pair_ids)
        if terms:
            merged = TR.make_bonded(self, terms, sliced=reduced)
            self._group_bonded.append(merged)
            # the first member of a group writes the buffer, the others add to it: an interaction-group force touches a few rows
            # only (it would have to clear the rest first), so the bond lists go first in its group
            if any(e.softcore is not None for e in members):
                ids.insert(0, merged)
            else:
                ids.append(merged)
        for e in self.entries:
            if e.recip is not None and (g == 'all' or e.recip_group == g):
                e.recip_sliced = reduced
                self.ctx.pme_set_sliced(e.recip, reduced)
                ids.append(e.recip)
        # term-expression forces last: each is a member of its own (the scheduler's fusion rules decline a group that holds one and
        # evaluate it member by member), and the first member still writes the buffer
        ids += [tid for e in members for tid in e.term_ids]
        index = B.GROUP_ALL if g == 'all' else int(g)
        if reduced and g != 'all':
            self._buffer('f{}'.format(g), together=['f{}'.format(e.group) for e in self.entries if e.pair_ids])
        slot = self._slot('f' if g == 'all' else 'f{}'.format(g))
        self.ctx.group_define(index, slot, ids)
        if gather:       # the EVAL op exchanges the slices itself: no all-reduce of the buffer afterwards
            self.ctx.group_set_exchange(index, B.EXCHANGE_GATHER)
            self._gather_groups.add(index)
            reduced = False
        self._group_defs[g] = (index, slot, reduced)
        return self._group_defs[g]

    def _emit_constraint(self, kind, ops, valid):
        """addConstrainPositions / addConstrainVelocities (propagators.py:250, 272): identity without constraints."""
        if not self._has_constraints:
            return
        if kind == mm.CustomIntegrator.ConstrainPositions:
            ops.append(B.Op(B.OP_CONSTRAIN_X, 0, 0, 0, 0.0))
            for g in valid:
                valid[g] = False
            self._deriv_cache.clear()
        else:
            ops.append(B.Op(B.OP_CONSTRAIN_V, 0, 0, 0, 0.0))

    def apply_constraints(self):
        if self._has_constraints:
            self.ctx.run_ops([B.Op(B.OP_SAVE_REF, 0, 0, 0, 0.0), B.Op(B.OP_CONSTRAIN_X, 0, 0, 0, 0.0)], 1)
            self._invalidate_forces()
            self._check()

    def apply_velocity_constraints(self):
        if self._has_constraints:
            self.ctx.run_ops([B.Op(B.OP_CONSTRAIN_V, 0, 0, 0, 0.0)], 1)
            self._check()

    # ------------------------------------------------------------------------------- energy minimisation
    def _constraint_errors(self, pairs, dist):
        """Largest relative error |r - d| / d over the constrained pairs at the current positions (minimum image in a periodic box,
        plain distances in free space; on the device)."""
        torch = self.torch
        d = self.x[pairs[:, 0]] - self.x[pairs[:, 1]]
        if self.box is not None:
            box = torch.as_tensor(self.box, device=self.x.device)
            d = d - box * torch.round(d / box)
        return float((torch.abs(torch.linalg.norm(d, dim=1) - dist) / dist).max().item())

    def minimize(self, tolerance=10.0, max_iterations=0, reporter=None, memory=8, max_step=0.1):
        """LocalEnergyMinimizer.minimize: L-BFGS on the sum of all force groups until the RMS of the free force components is
        <= tolerance (kJ/mol/nm) or max_iterations (0: no limit) iterations are done.  Positions only: velocities, time, per-DOF
        variables, parameters and the random stream stay as they are.  With constraints (as OpenMM): start on the constraint surface,
        minimise with harmonic restraints k (r - d)^2 / 2 over the constrained pairs, stiffen k tenfold while the largest relative
        constraint error exceeds the integrator's tolerance, finish with applyConstraints().  reporter(iteration, x, grad, args) ->
        stop?, x and grad fetched only when one is given.  Returns dict(iterations, evaluations, energy, reason, ...)."""
        if self.world > 1:
            raise InputError('minimisation runs on a single rank')
        tolerance, max_iterations = float(tolerance), int(max_iterations)
        if not tolerance > 0:
            raise ValueError('minimize: the tolerance must be positive')
        torch = self.torch
        dev = self.x.device
        self.compute_virtual_sites()          # (the first energy and gradient are taken with the sites on their parents)
        result = dict(iterations=0, evaluations=0, passes=0, restraint_strength=0.0)
        if self._has_constraints:
            cons = self.system._constraints
            pairs = np.array([[c[0], c[1]] for c in cons], dtype=np.int32)
            dist = np.array([c[2] for c in cons], dtype=np.float64)
            d_pairs, d_dist = torch.as_tensor(pairs.astype(np.int64), device=dev), torch.as_tensor(dist, device=dev)
            ctol = self.integrator.getConstraintTolerance() if hasattr(self.integrator, 'getConstraintTolerance') else 1e-5
            self.apply_constraints()
            k = 100.0 / max(1e-4, ctol)          # (OpenMM's first strength)
            for _ in range(9):                   # k grows by 10^8 at most: beyond that the restraints swamp fp64 sums of the energy
                rid = TR.make_bonded(self, [(B.BOND_HARMONIC, pairs, np.stack([dist, np.full(len(dist), k)], axis=1), True, None)], sliced=False)
                try:
                    done = self._minimize_pass(tolerance, max_iterations, reporter, memory, max_step, rid, k,
                                               lambda: self._constraint_errors(d_pairs, d_dist), result)
                finally:
                    self.ctx.bonded_release(rid)
                error = self._constraint_errors(d_pairs, d_dist)
                result.update(restraint_strength=k, max_constraint_error=error)
                if error <= ctol or done == 'reporter':
                    break
                k *= 10.0
            self.apply_constraints()
        else:
            self._minimize_pass(tolerance, max_iterations, reporter, memory, max_step, None, 0.0, lambda: 0.0, result)
        self._invalidate_forces()
        return result

    def _minimize_pass(self, tolerance, max_iterations, reporter, memory, max_step, restraint, strength, constraint_error, result):
        """One L-BFGS minimisation from the current positions (csrc/minimize.hip holds the vectors; this is the line search).  The host
        reads one block of eight scalars per energy evaluation -- the energy the line search needs, with g.d, g.g and the step factor
        riding along -- and nothing else."""
        torch, ctx = self.torch, self.ctx
        dev, f64 = self.x.device, torch.float64
        scal = torch.zeros(8, dtype=f64, device=dev)
        force = torch.zeros((self.n, 3), dtype=f64, device=dev)
        nfree = 3 * int(np.count_nonzero(np.asarray(self.system._masses, dtype=np.float64) > 0))
        if nfree == 0:
            result.update(reason='converged', energy=float('nan'))
            return 'converged'
        const = sum(entry.constant for entry in self.entries)

        def evaluate(read=True):
            # (every group, as get_state does; the energies add up in scal[0], which amm_min_trial / the zeroing above cleared)
            force.zero_()
            for entry in self.entries:
                for pid in entry.pair_ids:
                    ctx.force_eval(pid, self.x, force, accumulate=True, energy=scal)
                if entry.bonded_id is not None:
                    ctx.force_eval(entry.bonded_id, self.x, force, accumulate=True, energy=scal)
                for tid in entry.term_ids:
                    ctx.force_eval(tid, self.x, force, accumulate=True, energy=scal)
                if entry.recip is not None:
                    ctx.force_eval(entry.recip, self.x, force, accumulate=True, energy=scal)
            if restraint is not None:
                ctx.force_eval(restraint, self.x, force, accumulate=True, energy=scal)
            if self._has_vsites:              # the gradient with respect to the parents; the sites' own rows become 0
                ctx.vsite_spread(self.x, force)
            result['evaluations'] += 1
            if not read:
                return None
            s = ctx.min_scalars(mid)          # the evaluation's one wait
            self._check()                     # a neighbour-row overflow raises instead of corrupting the search
            return s

        def report(iteration, energy):
            e_restraint = 0.0
            if restraint is not None:
                tmp, sink = torch.zeros(1, dtype=f64, device=dev), torch.zeros_like(force)
                ctx.force_eval(restraint, self.x, sink, accumulate=False, energy=tmp)
                e_restraint = tmp.item()
            args = {'system energy': energy - e_restraint, 'restraint energy': e_restraint, 'restraint strength': strength,
                    'max constraint error': constraint_error()}
            return bool(reporter.report(iteration, self.x.cpu().numpy().ravel().tolist(), (-force).cpu().numpy().ravel().tolist(), args))

        def moved():
            # the Verlet lists' displacement checks must see the move (amm_min_trial says so itself; this is the engine's own rule
            # for every write of self.x)
            if self._has_vsites:              # (a trial leaves the massless sites where they were: they follow their parents here)
                ctx.vsite_place(self.x)
            ctx.positions_changed()
            self._invalidate_forces()

        mid = ctx.min_create(scal, mass=self.mass, memory=memory, max_step=max_step, force_input=True)
        try:
            result['passes'] += 1
            evaluate(read=False)
            ctx.min_begin(mid, self.x, force)
            s = ctx.min_scalars(mid)
            self._check()
            energy = s[0] + const
            iteration, reason = 0, None
            if math.sqrt(s[2] / nfree) <= tolerance:
                reason = 'converged'
            alpha = min(1.0, 1.0 / math.sqrt(s[2])) if s[2] > 0 else 1.0
            steepest, pending = True, False
            while reason is None:
                accepted = False
                for _ in range(21):           # alpha, then at most 20 halvings
                    ctx.min_trial(mid, alpha, self.x)
                    moved()
                    s = evaluate()
                    if pending:               # the first read after an advance: g.g of the point the line search starts from
                        pending = False
                        steepest = s[5] == 0
                        if math.sqrt(s[2] / nfree) <= tolerance:
                            reason = 'converged'
                            break
                    trial_energy = s[0] + const
                    if math.isfinite(trial_energy) and trial_energy <= energy + 1e-4 * s[6] * s[1]:
                        accepted = True
                        break
                    alpha = 0.5 * s[6]
                if reason is not None or not accepted:
                    if reason is None and not steepest:
                        ctx.min_begin(mid)    # clear the history, steepest descent from the same point
                        steepest, alpha = True, 1.0
                        continue
                    reason = reason or 'no progress'
                    ctx.min_trial(mid, 0.0, self.x)       # back to the point the line search started from
                    moved()
                    break
                energy = trial_energy
                stop = report(iteration, energy) if reporter is not None else False
                iteration += 1
                if stop:
                    reason = 'reporter'
                elif max_iterations and iteration >= max_iterations:
                    reason = 'max iterations'
                else:
                    ctx.min_advance(mid, self.x, force)
                    pending, alpha = True, 1.0
            stats = ctx.min_stats(mid)
        finally:
            ctx.min_release(mid)
        result['iterations'] += iteration
        result.update(reason=reason, energy=energy, dropped_pairs=stats['dropped'], restarts=stats['restarts'])
        return reason

    def _eval(self, expr, env):
        code = _CODE_CACHE.get(expr)
        if code is None:
            code = _CODE_CACHE[expr] = compile(expr.replace('^', '**').strip(), '<step program>', 'eval')
        return float(eval(code, {'__builtins__': {}}, env))

    def _compile(self):
        """Unroll one outer step of the CustomIntegrator program into backend ops (host-side control flow)."""
        if self._stock is not None and getattr(self._stock, '_drude', False):
            return self._compile_drude()
        if self._stock is not None and self.stock_native and hasattr(self.ctx, 'stock_define'):
            return self._compile_stock()
        integ = self.integrator
        steps = integ._steps
        C = mm.CustomIntegrator
        # block structure
        match, stack = {}, []
        for pc, (kind, _, _) in enumerate(steps):
            if kind in (C.IfBlock, C.WhileBlock):
                stack.append(pc)
            elif kind == C.EndBlock:
                begin = stack.pop()
                match[begin], match[pc] = pc, begin
        env = dict(_SAFE_FUNCS)
        env.update(self.parameters)
        env.update(zip(integ._gnames, integ._gvalues))
        env['dt'] = integ._dt
        valid = dict(self._valid)
        self._mirror_work = dict(self._mirror)
        self._static_exprs = True
        self._iso_found, self._plain_kick = None, False      # isokinetic (SIN(R)) kicks recognised / ordinary kicks emitted
        self._reg_found, self._plain_move = None, False      # regulated moves recognised (alpha, an kT) / ordinary moves emitted
        ops = [B.Op(B.OP_SAVE_REF, 0, 0, 0, 0.0)] if self._has_constraints else []
        pc = 0
        guard = 0
        while pc < len(steps):
            guard += 1
            if guard > 2_000_000:
                raise RuntimeError('step program does not terminate')
            kind, target, expr = steps[pc]
            if kind == C.ComputeGlobal:
                value = self._eval(expr, env)
                if target in self.parameters and target not in integ._gnames:
                    if value != self.parameters[target]:
                        raise NotImplementedError('step programs that change Context parameters (%s) are not supported' % target)
                env[target] = value
            elif kind == C.ComputePerDof:
                skip = self._emit_native_bath_block(steps, pc, env, ops) or self._emit_native_iso_block(steps, pc, env, ops, valid) or \
                    self._emit_regulated_bath_block(steps, pc, env, ops)
                if skip:
                    pc += skip
                    continue
                _refuse_vector_functions(expr)
                self._emit_per_dof(target, expr, env, ops, valid)
            elif kind == C.ComputeSum:
                raise NotImplementedError('ComputeSum steps (thermostat propagators) are outside this round\'s scope')
            elif kind in (C.ConstrainPositions, C.ConstrainVelocities):
                self._emit_constraint(kind, ops, valid)
            elif kind == C.UpdateContextState:
                pass
            elif kind in (C.IfBlock, C.WhileBlock):
                if not self._condition(expr, env):
                    pc = match[pc]
            elif kind == C.EndBlock:
                if steps[match[pc]][0] == C.WhileBlock:
                    pc = match[pc] - 1
            pc += 1
        self._static_exprs = False
        if self._iso_found and self._plain_kick:
            # isokinetic AND ordinary kicks in one program: the context-wide isokinetic mode cannot serve both -- run the
            # isokinetic ones as general expressions
            self._no_native_iso = True
            return self._compile()
        if self._reg_found and (self._plain_move or self._iso_found):
            # regulated AND ordinary moves (or the isokinetic mode as well): the context-wide regulated mode cannot serve both --
            # run the regulated moves as general expressions
            self._no_native_reg = True
            return self._compile()
        if hasattr(self.ctx, 'regulated_define'):
            if self._reg_found:
                self.ctx.regulated_define(True, *self._reg_found)
            else:
                self.ctx.regulated_define(False)
        if hasattr(self.ctx, 'iso_define'):
            if self._iso_found:
                LkT, Q1, v1 = self._iso_found
                self.ctx.iso_define(True, LkT, Q1, self._slot(v1))
            else:
                self.ctx.iso_define(False)
        finals = {name: env[name] for name in integ._gnames}
        return self._drop_dead_copies(self._pair_up_evals(ops)), valid, finals, dict(self._mirror_work)

    def _compile_stock(self):
        """The step of a stock integrator as ONE op behind the evaluation of all forces (no SAVE_REF: the launch takes the bond
        vectors from the positions it loads).  Nothing of the op-by-op program is compiled or registered with the library."""
        stock, integ = self._stock, self.integrator
        valid = dict(self._valid)
        self._mirror_work = dict(self._mirror)
        ops = []
        slot = self._force_ref('f', ops, valid)
        key = ('stock', stock._stock_kind, stock._dt, stock._friction, stock._kT())
        if key not in self._expr_ids:
            self._expr_ids[key] = self.ctx.stock_define(stock._stock_kind, stock._dt, stock._friction, stock._kT())
        ops.append(B.Op(B.OP_STOCK, self._expr_ids[key], slot, 0, 0.0))
        for g in valid:
            valid[g] = False
        self._deriv_cache.clear()
        if hasattr(self.ctx, 'regulated_define'):
            self.ctx.regulated_define(False)
        if hasattr(self.ctx, 'iso_define'):
            self.ctx.iso_define(False)
        return ops, valid, dict(zip(integ._gnames, integ._gvalues)), dict(self._mirror_work)

    def _compile_drude(self):
        """The step of a DrudeLangevinIntegrator as ONE op behind the evaluation of all forces, as _compile_stock: the launch
        thermalises pairs and atoms, moves, constrains and applies the hard wall (csrc/drude.hip).  There is no op-by-op form."""
        stock, integ = self._stock, self.integrator
        valid = dict(self._valid)
        self._mirror_work = dict(self._mirror)
        ops = []
        slot = self._force_ref('f', ops, valid)
        key = ('drude', stock._dt, stock._friction, stock._kT(), stock._drude_friction, stock._drude_kT(), stock._max_drude_distance)
        if key not in self._expr_ids:
            self._expr_ids[key] = self.ctx.drude_step_define(self.drude_pairs(), stock._dt, stock._friction, stock._kT(), stock._drude_friction,
                                                             stock._drude_kT(), stock._max_drude_distance)
        ops.append(B.Op(B.OP_DRUDE_STEP, self._expr_ids[key], slot, 0, 0.0))
        for g in valid:
            valid[g] = False
        self._deriv_cache.clear()
        if hasattr(self.ctx, 'regulated_define'):
            self.ctx.regulated_define(False)
        if hasattr(self.ctx, 'iso_define'):
            self.ctx.iso_define(False)
        return ops, valid, dict(zip(integ._gnames, integ._gvalues)), dict(self._mirror_work)

    _NHL_SCALE = re.compile(r'v\*exp\(-\((.+)\*dt\)\*(\w+)\)')
    _NHL_UPDATE = re.compile(r'z\*(\w+)\+sqrt\(kT\*\(1-z\*z\)/mass\)\*gaussian\+force\*\(1-z\)/\(mass\*friction\);force=m\*v\^2-kT;'
                             r'mass=(\w+);z=exp\(-\((.+)\*dt\)\*friction\)')

    def _emit_native_bath_block(self, steps, pc, env, ops):
        """The three per-DOF steps of a Nose-Hoover-Langevin bath (NHL_R_Integrator, integrators.py:272-330:
        `v <- v*exp(-(h*dt)*v2)` ; `v2 <- z*v2 + sqrt(kT*(1 - z*z)/mass)*gaussian + force*(1 - z)/(mass*friction); ...` ;
        `v <- v*exp(-(h*dt)*v2)`) become ONE native bath op, which the inner-loop kernel carries between its two half moves
        like the Ornstein-Uhlenbeck step of Langevin_R.  Returns the number of program steps consumed (0: not such a block)."""
        C = mm.CustomIntegrator
        if pc + 2 >= len(steps) or any(steps[pc + k][0] != C.ComputePerDof for k in range(3)):
            return 0
        (_, t0, e0), (_, t1, e1), (_, t2, e2) = steps[pc:pc + 3]
        a, b, c = self._NHL_SCALE.fullmatch(e0.replace(' ', '')), self._NHL_UPDATE.fullmatch(e1.replace(' ', '')), \
            self._NHL_SCALE.fullmatch(e2.replace(' ', ''))
        if not (a and b and c and t0 == 'v' and t2 == 'v' and e0 == e2):
            return 0
        w = a.group(2)
        if not (t1 == w and b.group(1) == w and w in self.integrator._pnames and b.group(2) in env and 'kT' in env and 'friction' in env):
            return 0
        h = self._eval(a.group(1), env) * env['dt']
        z = math.exp(-(self._eval(b.group(3), env) * env['dt']) * env['friction'])
        key = ('nhl', h, z, float(env['kT']), float(env[b.group(2)]), float(env['friction']), w)
        if key not in self._expr_ids:
            self._expr_ids[key] = self.ctx.bath_define_nhl(h, z, float(env['kT']), float(env[b.group(2)]), float(env['friction']),
                                                           self._slot(w))
        ops.append(B.Op(B.OP_BATH, self._expr_ids[key], B.SLOT_V, 0, 0.0))
        self._mirror_work.pop(w, None)
        return 3

    _NUM = r'([0-9.eE+-]+)'
    _REG_SCALE = re.compile(r'v\*exp\(-v_eta\*(.+)\*dt\)')
    _REG_SCALE2 = re.compile(_NUM + r'\*c\*asinhz;asinhz=\(2\*step\(z\)-1\)\*log\(select\(step\(za-1E8\),2\*za,za\+sqrt\(1\+z\*z\)\)\);za=abs\(z\);'
                             r'z=sinh\(' + _NUM + r'\*v/c\)\*exp\(-v_eta\*(.+)\*dt\);c=sqrt\(' + _NUM + r'\*kT/m\)')
    # the drive G of each kind: (kfac,) alpha, an
    _REG_DRIVE = {3: r'\(m\*v\*c\*tanh\(' + _NUM + r'\*v/c\)-kT\)/Q;c=sqrt\(' + _NUM + r'\*kT/m\)',
                  4: r'\(' + _NUM + r'\*m\*\(c\*tanh\(' + _NUM + r'\*v/c\)\)\^2-kT\)/Q;c=sqrt\(' + _NUM + r'\*kT/m\)',
                  5: r'\(dot\(m\*v,c\*tanh\(' + _NUM + r'\*v/c\)\)-3\*kT\)/Q;c=sqrt\(' + _NUM + r'\*kT/m\)',
                  6: r'\(' + _NUM + r'\*dot\(m\*c\*y,c\*y\)-3\*kT\)/Q;y=tanh\(' + _NUM + r'\*v/c\);c=sqrt\(' + _NUM + r'\*kT/m\)'}

    def _emit_regulated_bath_block(self, steps, pc, env, ops):
        """The bath block of a regulated Nose-Hoover-Langevin propagator (propagators.py:1598-2007) -- [boost of v_eta ;] scaling of
        v ; Ornstein-Uhlenbeck step of v_eta ; scaling of v [; boost] -- becomes ONE native bath op (amm_bath_define_regulated,
        kinds 3..6), which the inner-loop kernel carries between its two half moves.  Needs the reference's text with global kT,
        Q, omega and friction (not `adiabatic`).  Returns the number of program steps consumed (0: not such a block)."""
        C = mm.CustomIntegrator
        if not (self.native_regulated and hasattr(self.ctx, 'bath_define_regulated')) or steps[pc][1] not in ('v', 'v_eta'):
            return 0
        split = steps[pc][1] == 'v_eta'
        count = 5 if split else 3
        if pc + count > len(steps) or any(steps[pc + k][0] != C.ComputePerDof for k in range(count)):
            return 0
        block = [(t, e.replace(' ', '')) for _, t, e in steps[pc:pc + count]]
        integ = self.integrator
        if [t for t, _ in block] != (['v_eta', 'v', 'v_eta', 'v', 'v_eta'] if split else ['v', 'v_eta', 'v']) or \
                'v_eta' not in integ._pnames or any(g not in env or g in integ._pnames for g in ('kT', 'Q', 'omega', 'friction')):
            return 0
        scale, ou = block[1 if split else 0][1], block[2 if split else 1][1]
        if block[3 if split else 2][1] != scale or (split and block[4][1] != block[0][1]):
            return 0
        s1, s2 = self._REG_SCALE.fullmatch(scale), self._REG_SCALE2.fullmatch(scale)
        twice = s2 is not None
        if not (s1 or s2):
            return 0
        atomic = '_x(gaussian)' in ou
        kind = (5 if atomic else 3) + (1 if twice else 0)
        noise = '_x\\(gaussian\\)' if atomic else 'gaussian'
        drive = self._REG_DRIVE[kind]
        tail = r';z=exp\(-friction\*(.+)\*dt\)'
        if split:
            o = re.fullmatch(r'v_eta\*z\+omega\*sqrt\(1-z\^2\)\*' + noise + tail, ou)
            b = re.fullmatch(r'v_eta\+G\*(.+)\*dt;G=' + drive, block[0][1])
            if not (o and b):
                return 0
            d = b.groups()[1:]
            if self._eval(b.group(1), env) != self._eval((s2 or s1).group(3 if twice else 1), env):
                return 0
        else:
            o = re.fullmatch(r'v_eta\*z\+G\*\(1-z\)/friction\+omega\*sqrt\(1-z\^2\)\*' + noise + ';G=' + drive + tail, ou)
            if not o:
                return 0
            d = o.groups()[:-1]
        numbers = [float(t) for t in d]
        kfac = numbers.pop(0) if twice else None
        alpha, an = numbers
        n = an / alpha
        if twice:
            if float(s2.group(1)) != 1 / alpha or float(s2.group(2)) != alpha or float(s2.group(4)) != an or \
                    abs(kfac - (n + 1) / (alpha * n)) > 1e-12 * kfac:
                return 0
        h = self._eval((s2 or s1).group(3 if twice else 1), env) * env['dt']
        z = math.exp((-env['friction'] * self._eval(o.groups()[-1], env)) * env['dt'])
        args = (kind, split, h, z, float(env['kT']), float(env['Q']), float(env['omega']), float(env['friction']), alpha, an)
        key = ('regulated',) + args
        if key not in self._expr_ids:
            self._expr_ids[key] = self.ctx.bath_define_regulated(*args, self._slot('v_eta'))
        ops.append(B.Op(B.OP_BATH, self._expr_ids[key], B.SLOT_V, 0, 0.0))
        self._mirror_work.pop('v_eta', None)
        return count

    _ISO_KICK = re.compile(r'v\*cosh\(z\)\+sqrt\(LkT/m\)\*sinh\(z\);z=(.+)/sqrt\(m\*LkT\)')
    _ISO_H = re.compile(r'sqrt\(LkT/\(m\*v\^2\+0\.5\*Q1\*\((\w+)\^2\)\)\)')
    _SIN_SCALE = re.compile(r'(\w+)\*exp\(-\((.+)\*dt\)\*(\w+)\)')
    _SIN_UPDATE = re.compile(r'z\*(\w+)\+sqrt\(kT\*\(1-z\*z\)/mass\)\*gaussian\+force\*\(1-z\)/\(mass\*friction\);force=Q1\*(\w+)\^2-kT;'
                             r'mass=(\w+);z=exp\(-\((.+)\*dt\)\*friction\)')

    def _iso_rescale_at(self, steps, pc, env):
        """`H <- sqrt(LkT/(m*v^2 + 0.5*Q1*(v1^2)))` ; `v <- H*v` ; `v1 <- H*v1` at steps[pc:pc+3] (SIN(R) with L = 1,
        propagators.py:300-320): the name of v1, or None."""
        C = mm.CustomIntegrator
        if pc + 2 >= len(steps) or any(steps[pc + k][0] != C.ComputePerDof for k in range(3)):
            return None
        (_, t0, e0), (_, t1, e1), (_, t2, e2) = steps[pc:pc + 3]
        m = self._ISO_H.fullmatch(e0.replace(' ', ''))
        if not (m and t0 == 'H' and t1 == 'v' and e1.replace(' ', '') == 'H*v' and t2 == m.group(1) and
                e2.replace(' ', '') == 'H*' + m.group(1) and m.group(1) in self.integrator._pnames and 'LkT' in env and 'Q1' in env):
            return None
        found = (float(env['LkT']), float(env['Q1']), m.group(1))
        if self._iso_found not in (None, found):
            return None
        return m.group(1)

    def _emit_native_iso_block(self, steps, pc, env, ops, valid):
        """SIN(R) with one thermostat per DOF (SIN_R_Integrator, integrators.py:358-416).  (a) The isokinetic kick --
        `v <- v*cosh(z) + sqrt(LkT/m)*sinh(z); z = (c*dt)*(F)/sqrt(m*LkT)` followed by the rescale triple -- becomes an ordinary
        KICK op of a context in isokinetic mode (amm_iso_define); (b) the bath block between the two half moves -- `v1 <-
        v1*exp(-(h*dt)*v2)`, rescale, the Ornstein-Uhlenbeck-like update of v2 driven by Q1*v1^2 - kT, the scaling and the rescale
        again -- becomes ONE native bath op.  Returns the number of program steps consumed (0: neither)."""
        if getattr(self, '_no_native_iso', False) or not hasattr(self.ctx, 'iso_define'):
            return 0
        C = mm.CustomIntegrator
        kind, target, expr = steps[pc]
        text = expr.replace(' ', '')
        kick = self._ISO_KICK.fullmatch(text) if target == 'v' else None
        if kick:
            v1 = self._iso_rescale_at(steps, pc + 1, env)
            parts = self._split_leading_group(kick.group(1))
            terms = self._signed_terms(parts[1]) if parts else None
            if not (v1 and terms and len(terms) <= 2 and terms[0][0] == 1):
                return 0
            coef = self._eval(parts[0], env)
            a = self._force_ref(terms[0][1], ops, valid)
            b, plus = -1, 0
            if len(terms) == 2:
                b = self._force_ref(terms[1][1], ops, valid)
                plus = 1 if terms[1][0] == 1 else 0
            ops.append(B.Op(B.OP_KICK, a, b, plus, coef))
            self._iso_found = (float(env['LkT']), float(env['Q1']), v1)
            return 4
        scale = self._SIN_SCALE.fullmatch(text)
        if scale and scale.group(1) == target and pc + 8 < len(steps):
            v1, v2 = target, scale.group(3)
            if self._iso_rescale_at(steps, pc + 1, env) != v1 or self._iso_rescale_at(steps, pc + 6, env) != v1:
                return 0
            (k4, t4, e4), (k5, t5, e5) = steps[pc + 4], steps[pc + 5]
            upd = self._SIN_UPDATE.fullmatch(e4.replace(' ', '')) if k4 == C.ComputePerDof else None
            if not (upd and t4 == v2 and upd.group(1) == v2 and upd.group(2) == v1 and k5 == C.ComputePerDof and t5 == v1 and e5 == expr and
                    v2 in self.integrator._pnames and upd.group(3) in env and 'kT' in env and 'friction' in env):
                return 0
            h = self._eval(scale.group(2), env) * env['dt']
            z = math.exp(-(self._eval(upd.group(4), env) * env['dt']) * env['friction'])
            key = ('sin', h, z, float(env['kT']), float(env[upd.group(3)]), float(env['friction']), v2)
            if key not in self._expr_ids:
                self._expr_ids[key] = self.ctx.bath_define_sin(h, z, float(env['kT']), float(env[upd.group(3)]), float(env['friction']),
                                                               self._slot(v2))
            ops.append(B.Op(B.OP_BATH, self._expr_ids[key], B.SLOT_V, 0, 0.0))
            self._iso_found = (float(env['LkT']), float(env['Q1']), v1)
            self._slot(v1)
            return 9
        return 0

    def _pair_up_evals(self, ops):
        """RESPA evaluates the near force (group 1) and, one kick later, the outer force (group 2) at the same positions
        (propagators.py:940-973); the two traverse one neighbour list (_share_lists).  Move the second EVAL (and its
        all-reduce marker) right behind the first, so that the backend evaluates both in one pass: legal when nothing in
        between moves the atoms or touches the second group's buffer."""
        fusable = set()
        for gid, host in self.shared.items():
            ga = [e.group for e in self.entries if gid in e.pair_ids]
            gb = [e.group for e in self.entries if host in e.pair_ids]
            if ga and gb:
                fusable.add(frozenset((ga[0], gb[0])))

        def is_eval(op):
            return not isinstance(op, tuple) and op.op == B.OP_EVAL

        def touches(op, slot):
            if isinstance(op, tuple):
                return op[1] == slot
            if op.op == B.OP_KICK:
                return slot in (op.a, op.b)
            if op.op == B.OP_COPY:
                return slot in (op.a, op.b)
            if op.op == B.OP_COMBINE:
                return slot in (op.a, op.b, op.c)
            return False

        slot_of = {index: slot for (index, slot, _) in self._group_defs.values()}
        out = list(ops)
        k = 0
        while k < len(out):
            if is_eval(out[k]):
                first = k
                end = first + 1
                while end < len(out) and isinstance(out[end], tuple):      # the first EVAL's all-reduce marker
                    end += 1
                j = end
                while j < len(out):
                    op = out[j]
                    if is_eval(op):
                        if frozenset((out[first].a, op.a)) in fusable:
                            slot2 = slot_of.get(op.a)
                            if not any(touches(mid, slot2) for mid in out[end:j]):
                                block = [op]
                                nxt = j + 1
                                while nxt < len(out) and isinstance(out[nxt], tuple):
                                    block.append(out[nxt])
                                    nxt += 1
                                del out[j:nxt]
                                evals = [out[first], block[0]]
                                markers = out[first + 1:end] + block[1:]
                                out[first:end] = evals + markers
                        break
                    if isinstance(op, tuple) or op.op in (B.OP_KICK,) or (op.op in (B.OP_COPY, B.OP_COMBINE) and op.a != B.SLOT_X):
                        j += 1
                        continue
                    break                       # MOVE / writes to x: positions change
            k += 1
        return out

    def _condition(self, expr, env):
        parts = _CONDITION_CACHE.get(expr)
        if parts is None:
            m = re.match(r'^(.*?)(<=|>=|!=|=|<|>)(.*)$', expr)
            if not m:
                raise NotImplementedError('unsupported block condition: ' + expr)
            parts = _CONDITION_CACHE[expr] = (m.group(1), _COMPARE[m.group(2)], m.group(3))
        return parts[1](self._eval(parts[0], env), self._eval(parts[2], env))

    @staticmethod
    def _split_leading_group(text):
        """'(A)*rest' -> ('A', 'rest') with balanced parentheses."""
        if not text.startswith('('):
            return None
        depth = 0
        for k, ch in enumerate(text):
            depth += ch == '('
            depth -= ch == ')'
            if depth == 0:
                if text[k + 1:k + 2] != '*':
                    return None
                return text[1:k], text[k + 2:]
        return None

    def _force_ref(self, name, ops, valid):
        """Slot of a force symbol / per-DOF buffer; emits the EVAL (and all-reduce marker) when stale."""
        m = re.fullmatch(r'f([0-9]*)', name)
        if m:
            g = 'all' if m.group(1) == '' else int(m.group(1))
            index, slot, reduced = self._define_group(g)
            if not valid.get(g, False):
                ops.append(B.Op(B.OP_EVAL, index, 0, 0, 0.0))
                if reduced:
                    ops.append((ALLREDUCE, slot))
                valid[g] = True
                for dst in [d for d, src in self._mirror_work.items() if src == name]:
                    del self._mirror_work[dst]          # copies of the old contents are no longer copies
            return slot
        integ = self.integrator
        if name not in integ._pnames and name not in ('x', 'v'):
            raise NotImplementedError('unknown per-DOF symbol in step program: ' + name)
        # `_f2_` while it mirrors f2 (`_f2_ <- f2`, integrators.py:139-144, and no evaluation of group 2 since): read the
        # group's buffer itself, so that the copy has no reader left and can be dropped (_drop_dead_copies)
        src = self._mirror_work.get(name)
        if src is not None and _AUX_FORCE.fullmatch(name) and not _NO_ALIAS:
            return self._define_group('all' if src == 'f' else int(src[1:]))[1]
        return self._slot(name)

    def _drop_dead_copies(self, ops):
        """Remove COPY ops into the integrator's auxiliary force buffers (`_f2_ <- f2`) that no later op reads before the
        buffer is written again -- the program is cyclic, so the search wraps around.  get_per_dof materialises such a
        buffer from the force it mirrors when the user asks for it."""
        if _NO_ALIAS:
            return ops
        aux = {slot for name, slot in self._slots.items() if _AUX_FORCE.fullmatch(name)}
        if not aux:
            return ops

        def reads(op, slot):
            if isinstance(op, tuple):
                return op[1] == slot
            if op.op == B.OP_KICK:
                return slot in (op.a, op.b)
            if op.op == B.OP_COPY:
                return op.b == slot
            if op.op == B.OP_COMBINE:
                return slot in (op.b, op.c)
            return op.op in (B.OP_EXPR,)            # expression programs may read any buffer

        def writes(op, slot):
            return not isinstance(op, tuple) and op.op in (B.OP_COPY, B.OP_COMBINE) and op.a == slot

        keep = [True] * len(ops)
        for k, op in enumerate(ops):
            if isinstance(op, tuple) or op.op != B.OP_COPY or op.a not in aux:
                continue
            dead = True
            for j in list(range(k + 1, len(ops))) + list(range(0, k)):
                if reads(ops[j], op.a):
                    dead = False
                    break
                if writes(ops[j], op.a):
                    break
            keep[k] = not dead
        return [op for op, kept in zip(ops, keep) if kept]

    def _run_end(self, steps, pc):
        """First step at or after pc that is not a ComputePerDof (cached per program position)."""
        ends = self._segment_ends
        if pc not in ends:
            C = mm.CustomIntegrator
            q = pc
            while q < len(steps) and steps[q][0] == C.ComputePerDof:
                q += 1
            for k in range(pc, q):
                ends[k] = q
        return ends[pc]

    def _segment_key(self, pc, pc_end, steps, env, valid):
        names = self._segment_symbols.get((pc, pc_end))
        if names is None:
            found = set()
            for k in range(pc, pc_end):
                found |= set(X.symbols(steps[k][2]))
            names = self._segment_symbols[(pc, pc_end)] = tuple(sorted(found))
        return (pc, pc_end, tuple(env.get(name) for name in names), tuple(sorted(valid.items(), key=str)),
                tuple(sorted(self._mirror_work.items())), getattr(self, '_static_exprs', False))

    def _replay_segment(self, pc, pc_end, steps, env, ops, valid):
        """Emit the remembered ops of the run of per-DOF steps [pc, pc_end); False when this combination has not been seen (the
        walker then goes through it step by step and _record_segment remembers it) or cannot be keyed (a deferred global)."""
        self._segment_open = None
        try:
            key = self._segment_key(pc, pc_end, steps, env, valid)
            hit = self._segment_memo.get(key)
        except TypeError:
            return False
        if hit is None:
            if len(self._segment_memo) < 512:
                self._segment_open = [key, pc_end, len(ops), True]      # key, end, ops emitted so far, every step emitted natively
            return False
        new_ops, valid_after, mirror_after, moved, kicked = hit
        ops.extend(new_ops)
        valid.clear()
        valid.update(valid_after)
        self._mirror_work.clear()
        self._mirror_work.update(mirror_after)
        if moved:
            self._deriv_cache.clear()
        if kicked:
            self._plain_kick = True
        return True

    def _record_segment(self, pc, emitted, ops, valid):
        rec = getattr(self, '_segment_open', None)
        if rec is None:
            return
        if not emitted or len(ops) < rec[2]:        # a general expression (run outside the op list) or a flush in between: not a unit
            self._segment_open = None
            return
        if pc + 1 == rec[1]:
            key, _, before, _ = rec
            new_ops = tuple(ops[before:])
            moved = any(op.op == B.OP_MOVE or (op.op in (B.OP_COPY, B.OP_COMBINE) and op.a == B.SLOT_X) or
                        (op.op == B.OP_EXPR and op.b == B.SLOT_X) for op in new_ops if not isinstance(op, tuple))
            self._segment_memo[key] = (new_ops, dict(valid), dict(self._mirror_work), moved, self._plain_kick)
            self._segment_open = None

    def _emit_per_dof_memo(self, pc, target, expr, env, ops, valid):
        """_emit_per_dof for the host-walked path, remembered: what a per-DOF step of the program emits is a function of the
        values of the globals its text names, of which force groups are valid and of which auxiliary buffers mirror a force --
        a RESPA block inside an AFED step meets the same few dozen combinations every step, and re-deriving them (regular
        expressions, eval) was what made the host slower than the GPU at config C5."""
        names = _PER_DOF_SYMBOLS.get(expr)
        if names is None:
            names = _PER_DOF_SYMBOLS[expr] = tuple(sorted(X.symbols(expr)))
        try:
            key = (pc, tuple(env.get(name) for name in names), tuple(sorted(valid.items(), key=str)),
                   tuple(sorted(self._mirror_work.items())), getattr(self, '_static_exprs', False))
            hit = self._emit_memo.get(key)
        except TypeError:                # a deferred global (unhashable) among the values: no memo for this one
            return self._emit_per_dof(target, expr, env, ops, valid)
        if hit is None:
            before = len(ops)
            self._emit_per_dof(target, expr, env, ops, valid)
            if len(self._emit_memo) < 4096:
                self._emit_memo[key] = (tuple(ops[before:]), dict(valid), dict(self._mirror_work), target == 'x', self._plain_kick)
            return
        new_ops, valid_after, mirror_after, moved, kicked = hit
        ops.extend(new_ops)
        valid.clear()
        valid.update(valid_after)
        self._mirror_work.clear()
        self._mirror_work.update(mirror_after)
        if moved:
            self._deriv_cache.clear()
        if kicked:
            self._plain_kick = True

    _REG_MOVE = re.compile(r'x\+c\*tanh\(([0-9.eE+-]+)\*v/c\)\*(.+)\*dt;c=sqrt\(([0-9.eE+-]+)\*kT/m\)')

    def _emit_regulated_move(self, target, expr, env, ops, valid):
        """`x <- x + c*tanh(alpha*v/c)*h*dt; c=sqrt(an*kT/m)` with a global kT (RegulatedTranslationPropagator,
        propagators.py:1537-1575): a MOVE op of a context in regulated mode (amm_regulated_define).  Only in unrolled programs, whose
        compilation ends by setting the mode; False: not such a move."""
        m = self._REG_MOVE.fullmatch(expr.replace(' ', '')) if target == 'x' else None
        if not (m and self.native_regulated and getattr(self, '_static_exprs', False) and not getattr(self, '_no_native_reg', False) and
                hasattr(self.ctx, 'regulated_define') and 'kT' in env and 'kT' not in self.integrator._pnames):
            return False
        found = (float(m.group(1)), float(m.group(3)) * float(env['kT']))
        if self._reg_found not in (None, found):
            self._plain_move = True              # two different regulated moves: one mode cannot serve both
            return False
        self._reg_found = found
        ops.append(B.Op(B.OP_MOVE, 0, 0, 0, self._eval('(%s)*dt' % m.group(2), env)))
        for g in valid:
            valid[g] = False
        self._deriv_cache.clear()
        return True

    def _emit_per_dof(self, target, expr, env, ops, valid):
        if self._emit_regulated_move(target, expr, env, ops, valid):
            return
        text = expr.replace(' ', '')
        if ';' in text:
            text = ''         # auxiliary definitions: never a plain kick / move / copy -> general expression below
        # the kick written force first, `v + (f0)*0.0625*dt/m` (RegulatedBoostPropagator, propagators.py:1578-1595): OpenMM's
        # parser computes ((F*a)*b)/m, AMM_OP_KICK (a*b*F)/m -- the same to rounding
        if target == 'v' and text.startswith('v+') and text.endswith('/m'):
            factors = self._split_product(text[2:-2])
            if factors and len(factors) >= 2 and self._is_global_product(factors[1:], env):
                terms = self._signed_terms(factors[0])
                if terms and len(terms) <= 2 and terms[0][0] == 1 and all(self._is_force_symbol(t[1]) for t in terms):
                    coef = self._eval('*'.join(factors[1:]), env)
                    a = self._force_ref(terms[0][1], ops, valid)
                    b, plus = -1, 0
                    if len(terms) == 2:
                        b = self._force_ref(terms[1][1], ops, valid)
                        plus = 1 if terms[1][0] == 1 else 0
                    ops.append(B.Op(B.OP_KICK, a, b, plus, coef))
                    self._plain_kick = True
                    return
        # kick: v <- v + (coef)*FORCE/m
        if target == 'v' and text.startswith('v+') and text.endswith('/m'):
            parts = self._split_leading_group(text[2:-2])
            if parts:
                coef = self._eval(parts[0], env)
                terms = self._signed_terms(parts[1])
                if terms and len(terms) <= 2 and terms[0][0] == 1:
                    a = self._force_ref(terms[0][1], ops, valid)
                    b, plus = -1, 0
                    if len(terms) == 2:
                        b = self._force_ref(terms[1][1], ops, valid)
                        plus = 1 if terms[1][0] == 1 else 0
                    ops.append(B.Op(B.OP_KICK, a, b, plus, coef))
                    self._plain_kick = True
                    return
        # the same kick written as a bare product, `v + 0.5*1.0*dt*f/m` (UnconstrainedVelocityVerletPropagator, propagators.py:1136-1153):
        # OpenMM's parser associates a*b*c*f/m as (((a*b)*c)*f)/m, i.e. (coef * f) / m with coef = the product of the factors in
        # front of the force symbol -- what AMM_OP_KICK computes -- provided the force is the LAST factor
        if target == 'v' and text.startswith('v+') and text.endswith('/m'):
            factors = self._split_product(text[2:-2])
            if factors and len(factors) >= 2 and self._is_global_product(factors[:-1], env):
                terms = self._signed_terms(factors[-1])
                if terms and len(terms) <= 2 and terms[0][0] == 1 and all(self._is_force_symbol(t[1]) for t in terms):
                    coef = self._eval('*'.join(factors[:-1]), env)
                    a = self._force_ref(terms[0][1], ops, valid)
                    b, plus = -1, 0
                    if len(terms) == 2:
                        b = self._force_ref(terms[1][1], ops, valid)
                        plus = 1 if terms[1][0] == 1 else 0
                    ops.append(B.Op(B.OP_KICK, a, b, plus, coef))
                    self._plain_kick = True
                    return
        # move: x <- x + (coef)*v
        if target == 'x' and text.startswith('x+') and text.endswith('*v'):
            parts = self._split_leading_group(text[2:])
            factors = None if parts else self._split_product(text[2:])
            coef_text = parts[0] if parts and parts[1] == 'v' else None
            if coef_text is None and factors and len(factors) >= 2 and factors[-1] == 'v' and self._is_global_product(factors[:-1], env):
                coef_text = '*'.join(factors[:-1])          # `x + 1.0*dt*v`: ((1.0*dt)*v), the move's arithmetic
            if coef_text is not None:
                ops.append(B.Op(B.OP_MOVE, 0, 0, 0, self._eval(coef_text, env)))
                self._plain_move = True
                for g in valid:
                    valid[g] = False
                self._deriv_cache.clear()
                return
        # copies / differences of buffers: `_f2_ <- f2`, `fm1 <- f1`, `fm2 <- f2-f1`, `x0 <- x`
        if target not in ('x', 'v'):
            terms = self._signed_terms(text)
            if terms and terms[0][0] == 1 and len(terms) <= 2:
                src = self._force_ref(terms[0][1], ops, valid)
                dst = self._slot(target)
                for d in [d for d, sname in self._mirror_work.items() if sname == target]:
                    del self._mirror_work[d]
                if len(terms) == 1:
                    # `_f2_ <- f2` opens AND closes the RESPA program (propagators.py:940-973): the copy at the top
                    # of the next step finds _f2_ still equal to the unchanged f2 and is dropped
                    if self._mirror_work.get(target) == terms[0][1]:
                        return
                    ops.append(B.Op(B.OP_COPY, dst, src, 0, 0.0))
                    if re.fullmatch(r'f[0-9]*', terms[0][1]):
                        self._mirror_work[target] = terms[0][1]
                    else:
                        self._mirror_work.pop(target, None)
                else:
                    second = self._force_ref(terms[1][1], ops, valid)
                    ops.append(B.Op(B.OP_COMBINE, dst, src, second, float(terms[1][0])))
                    self._mirror_work.pop(target, None)
                return
        # any other per-DOF expression whose globals are known now (a bath step inside a RESPA loop, ...): registered
        # once with the backend and replayed by amm_run_ops as an EXPR op
        if getattr(self, '_static_exprs', False):
            integ = self.integrator

            def resolve(name):
                if name == 'm':
                    return ('mass',)
                if name in ('x', 'v') or re.fullmatch(r'f[0-9]*', name) or name in integ._pnames:
                    return ('buf', self._force_ref(name, ops, valid))
                if name in env and not callable(env[name]):
                    return ('global',)
                return None
            if target not in ('x', 'v') and target not in integ._pnames:
                raise mm.OpenMMException('unknown per-DOF variable: ' + target)
            # the Ornstein-Uhlenbeck bath on (v, m) without force, as OrnsteinUhlenbeckPropagator writes it
            # (propagators.py:727-733): a native op, which the inner-loop kernel can carry (Langevin_R)
            ou = re.fullmatch(r'z\*v\+sqrt\(kT\*\(1-z\*z\)/mass\)\*gaussian;mass=m;z=exp\(-\((.+)\*dt\)\*friction\)',
                              expr.replace(' ', ''))
            if ou and target == 'v' and 'kT' in env and 'friction' in env:
                z = math.exp(-(self._eval(ou.group(1), env) * env['dt']) * env['friction'])
                key = ('ou', z, float(env['kT']))
                if key not in self._expr_ids:
                    self._expr_ids[key] = self.ctx.bath_define(z, float(env['kT']))
                ops.append(B.Op(B.OP_BATH, self._expr_ids[key], B.SLOT_V, 0, 0.0))
                return
            prog = X.compile_per_dof(expr, resolve)
            gvals = tuple(float(env[name]) for name in prog.globals_)
            key = (expr, gvals)
            if key not in self._expr_ids:
                self._expr_ids[key] = self.ctx.expr_define(prog.code, prog.consts, list(gvals))
            ops.append(B.Op(B.OP_EXPR, self._expr_ids[key], self._slot(target), 0, 0.0))
            self._mirror_work.pop(target, None)
            for d in [d for d, sname in self._mirror_work.items() if sname == target]:
                del self._mirror_work[d]
            if target == 'x':
                for g in valid:
                    valid[g] = False
                self._deriv_cache.clear()
            return
        raise NotImplementedError('per-DOF computation outside the RESPA hot path: {} <- {}'.format(target, expr))

    @staticmethod
    def _split_product(text):
        """'0.5*1.0*dt*(f1-f2)' -> ['0.5', '1.0', 'dt', '(f1-f2)']; None when the text is not a plain product at its top level."""
        parts, depth, start = [], 0, 0
        for k, ch in enumerate(text):
            if ch == '(':
                depth += 1
            elif ch == ')':
                depth -= 1
                if depth < 0:
                    return None
            elif depth == 0:
                if ch == '*':
                    parts.append(text[start:k])
                    start = k + 1
                elif ch in '+-/^;' and k > 0 and text[k - 1] not in 'eE':      # (a sign inside 1e-3 is part of the number)
                    return None
        parts.append(text[start:])
        return parts if depth == 0 and all(parts) else None

    def _is_force_symbol(self, name):
        return bool(re.fullmatch(r'f[0-9]*', name)) or name in self.integrator._pnames

    def _is_global_product(self, factors, env):
        """Every factor a number or a global / Context parameter known now (no per-DOF symbol, no function call)."""
        per_dof = set(self.integrator._pnames) | {'x', 'v', 'm', 'f'}
        for f in factors:
            if re.fullmatch(r'[0-9.]+([eE][+-]?[0-9]+)?', f):
                continue
            if re.fullmatch(r'[A-Za-z_][A-Za-z_0-9]*', f) and f not in per_dof and not re.fullmatch(r'f[0-9]+', f) \
                    and f in env and not callable(env[f]):
                continue
            return False
        return True

    @staticmethod
    def _signed_terms(text):
        """'(f0+fm1)' -> [(1,'f0'), (1,'fm1')]; None if not a signed sum of identifiers."""
        while text.startswith('(') and text.endswith(')'):
            text = text[1:-1]
        if not re.fullmatch(r'[A-Za-z_][A-Za-z_0-9]*([+-][A-Za-z_][A-Za-z_0-9]*)*', text):
            return None
        return [(-1 if s == '-' else 1, name) for s, name in re.findall(r'([+-]?)([A-Za-z_][A-Za-z_0-9]*)', text)]

    def _init_native_comm(self, dist):
        """Give the library its own RCCL communicator (csrc/comm.hip): the all-reduce after the EVAL of a sliced group
        becomes an op of the step program and whole runs of steps stay inside ONE amm_run_ops call, instead of ~10 host
        round trips per outer step (measured 480 us/step of host time).  torch.distributed only carries the 128-byte id."""
        box = [None]
        if self.rank == 0:
            try:
                box[0] = self.ctx.comm_unique_id()
            except Exception as exc:        # e.g. librccl cannot be bound: every rank then keeps torch.distributed
                box[0] = 'failed: %s' % exc
        dist.broadcast_object_list(box, src=0)
        ok = isinstance(box[0], (bytes, bytearray))
        if ok:
            try:
                self.ctx.comm_init(box[0])
            except Exception as exc:
                ok = False
                box[0] = 'failed: %s' % exc
        # all ranks or none: a rank without the communicator would leave the others waiting in the first collective
        flag = self.torch.tensor([1 if ok else 0], device=self.ctx.torch_device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 1:
            self._native_comm = True
        else:
            import warnings
            warnings.warn('library-owned RCCL communicator not available (%s): collectives stay in torch.distributed'
                          % (box[0] if not ok else 'another rank failed'))
            if ok:
                self.ctx.comm_destroy()

    def _run(self, ops, repeat, cache=True):
        """cache=False: `ops` is a throw-away list (the interpreted path flushes a fresh one several times per step); its
        plan is not kept -- the cache is keyed by the list's identity and would otherwise grow without bound."""
        if not self._coll:
            self.ctx.run_ops([op for op in ops if not isinstance(op, tuple)], repeat)
            return
        if self._native_comm:
            native = self._native_ops.get(id(ops)) if cache else None
            if native is None or native[0] is not ops:
                native = (ops, [B.Op(B.OP_ALLREDUCE, op[1], 0, 0, 0.0) if isinstance(op, tuple) else op for op in ops])
                if cache:
                    self._native_ops[id(ops)] = native
            self.ctx.run_ops(native[1], repeat)
            return
        # collectives driven from here (torch.distributed): the op list is cut after every all-reduce marker and after
        # every EVAL of an all-gather group (the library leaves the rank's chunk in the exchange buffer and waits)
        plan = self._native_ops.get(id(ops)) if cache else None
        if plan is None or plan[0] is not ops:
            segments, current = [], []
            for op in ops:
                if isinstance(op, tuple):
                    segments.append((current, ('reduce', op[1])))
                    current = []
                else:
                    current.append(op)
            plan = (ops, segments, current)
            if cache:
                self._native_ops[id(ops)] = plan
        _, segments, tail = plan
        inv = {slot: name for name, slot in self._slots.items()}
        # the all-gather exchanges INSIDE a run of ops are the library's to ask for: it runs up to an exchanged evaluation, hands back,
        # the chunks are gathered here, and it goes on where it stopped (amm_run_ops_from) -- so that the launches which integrate
        # their rows' molecules and exchange positions and velocities (state exchange) see the ops that follow their EVAL
        if not segments:            # no all-reduce markers (groups of one pair force each: the bench): whole repetitions in one go
            if tail:
                self.ctx.run_ops_host_exchanges(tail, repeat, self._host_gather)
            return
        for _ in range(repeat):
            for seg, (kind, slot) in segments:
                if seg:
                    self.ctx.run_ops_host_exchanges(seg, 1, self._host_gather)
                self._allreduce(self._buffers[inv[slot]])
            if tail:
                self.ctx.run_ops_host_exchanges(tail, 1, self._host_gather)

    def _host_gather(self, nf):
        """All-gather of the exchange chunks by torch.distributed (no library-owned communicator), then the unsort."""
        dist = self.torch.distributed
        count = nf * self._per * 3
        if self._local is not None:
            self._local.all_gather(self.rank, self._xchg, count)
            self.ctx.exchange_finish()
            return
        chunks = [self._xchg[r * count:(r + 1) * count] for r in range(self.world)]
        if dist.get_backend() == 'nccl':
            dist.all_gather_into_tensor(self._xchg[:self.world * count], chunks[self.rank].clone())
        else:                     # gloo (CPU tests / several ranks sharing one card): staged through the host
            mine = chunks[self.rank].cpu()
            parts = [self.torch.empty_like(mine) for _ in range(self.world)]
            dist.all_gather(parts, mine)
            for r in range(self.world):
                if r != self.rank:
                    chunks[r].copy_(parts[r])
        self.ctx.exchange_finish()

    @staticmethod
    def _program_key(valid, mirror):
        return (tuple(sorted((str(g), ok) for g, ok in valid.items())), tuple(sorted(mirror.items())))

    def _deriv(self, what, name):
        if what != 'energy':
            raise NotImplementedError('deriv(%s, ...): only deriv(energy, parameter) is supported' % what)
        return self.energy_derivative(name)

    def _energy_of(self, entries):
        """Potential energy of a subset of the translated forces (pair + bond-list + reciprocal-space terms + constants)."""
        torch = self.torch
        e_pair = torch.zeros(1, dtype=torch.float64, device=self.x.device)
        e_bond = torch.zeros(1, dtype=torch.float64, device=self.x.device)
        fp, fb = self._fwork.zero_(), self._fwork2.zero_()
        const = 0.0
        for entry in entries:
            for pid in entry.pair_ids:
                self.ctx.force_eval(pid, self.x, fp, accumulate=True, energy=e_pair)
            if entry.bonded_id is not None:
                self.ctx.force_eval(entry.bonded_id, self.x, fb, accumulate=True, energy=e_bond)
            for tid in entry.term_ids:
                self.ctx.force_eval(tid, self.x, fb, accumulate=True, energy=e_bond)
            if entry.recip is not None:
                self.ctx.pme_set_sliced(entry.recip, False)
                self.ctx.force_eval(entry.recip, self.x, fb, accumulate=True, energy=e_bond)
                self.ctx.pme_set_sliced(entry.recip, getattr(entry, 'recip_sliced', False))
            const += entry.constant
        self._check()
        if self._coll:
            self._allreduce(e_pair)
        return e_pair.item() + e_bond.item() + const

    def energy_derivative(self, name):
        """deriv(energy, name): d(total potential energy)/d(global parameter) at the current positions
        (ExtendedSystemVariable.update_velocity, integrators.py:735-737).

        * lambda of a softcore pair force: the pair kernel in derivative mode + the long-range correction's derivative;
        * an overall coupling factor (AlchemicalSystem's `linear` / `spline` / `art` / custom couplings, systems.py:349-365):
          the factor's derivative times the energy at unit coupling;
        * parameter offsets of a NonbondedForce (SolvationSystem's `lambda_coul`, systems.py:289-308): the energy is a
          quadratic form of the charges, so the central difference over a whole unit of lambda is exact; offsets that act
          on sigma / epsilon (`use_softcore=False`, systems.py:309-312) take a small central step instead (O(h^2))."""
        TR.refuse_derivative(self, name)
        self._refuse_in_free_space('deriv(energy, %s)' % name)
        if name not in self.parameters:
            raise mm.OpenMMException('deriv(energy, %s): no such Context parameter' % name)
        torch = self.torch
        total = 0.0
        by_difference = []
        for entry in self.entries:
            sc = entry.softcore
            if sc is not None and sc['lambda_name'] == name:
                out = torch.zeros(1, dtype=torch.float64, device=self.x.device)
                self.ctx.pair_energy_derivative(sc['pid'], self.x, out)
                if self._coll:
                    self._allreduce(out)
                total += out.item() + sc['constant_derivative'](self.parameters)
            elif entry.cv is not None and name in entry.cv['derivs']:
                # the outer text's explicit dependence: the kernel's forward-mode pass seeded in this parameter (csrc/cv.hip)
                out = torch.zeros(len(entry.cv['derivs']), dtype=torch.float64, device=self.x.device)
                self.ctx.cv_energy_derivative(entry.cv['id'], self.x, out)
                total += out[entry.cv['derivs'].index(name)].item()
            elif name in getattr(entry, 'depends', ()):
                if entry.cv is not None:
                    raise NotImplementedError('deriv(energy, %s) of a CustomCVForce that did not name the parameter with '
                                              'addEnergyParameterDerivative' % name)
                if getattr(entry, 'pair_expr', False):
                    raise NotImplementedError('deriv(energy, %s) of a CustomNonbondedForce with a generic energy expression (the '
                                              'pair-expression kernel differentiates in r only)' % name)
                if getattr(entry, 'term_expr', False):
                    raise NotImplementedError('deriv(energy, %s) of a %s with a generic energy expression (the term-expression '
                                              'kernel differentiates in the term\'s variable only)' % (name, type(entry.force).__name__))
                if entry.update is None:
                    raise NotImplementedError('deriv(energy, %s): the force that depends on it cannot be re-parameterised' % name)
                by_difference.append(entry)
        if by_difference:
            exact = all(getattr(e, 'quadratic_in', None) and name in e.quadratic_in for e in by_difference)
            here = self.parameters[name]
            h = 1.0 if exact else 1e-4
            lo = here - h
            if not exact and lo < 0.0 <= here:
                lo = here                      # sqrt(epsilon) offsets are not analytic below zero: one-sided step
            values, rebuilt = [], False
            for point in (here + h, lo, here):
                trial = dict(self.parameters)
                trial[name] = point
                for entry in by_difference:
                    result = entry.update(trial, {name})
                    rebuilt = rebuilt or (result and result != 'values')
                if point != here:
                    values.append(self._energy_of(by_difference))
            if rebuilt:
                self._forget_groups()
                self._programs.clear()
                self._emit_memo.clear()
                self._segment_memo.clear()
            self._invalidate_forces()
            total += (values[0] - values[1]) / (here + h - lo)
        return total

    def energies_at_states(self, names, rows):
        """Potential energy at K states of global parameters for the current positions: rows[k][i] is the value of names[i] in state k
        (ExtendedStateDataReporter's globalParameterStates, ExpandedEnsembleReporter).  The same numbers as setting each state in
        turn, getState(getEnergy=True) and restoring -- without the set / evaluate / restore round trips where the forces allow:

        * a force that depends on none of the varied parameters is evaluated once;
        * a softcore pair force whose only varied parameter is its lambda: ONE launch at all K lambdas (amm_pair_energy_states), plus
          its long-range correction at each of them;
        * forces that depend on one varied parameter in which their energy is a quadratic (charge offsets: `lambda_coul`) are
          evaluated at three of its values and interpolated -- exact up to rounding;
        * anything else takes the reference loop (counted in `n_state_fallbacks`).

        Leaves no trace for the first two kinds: parameters, lambda bindings, valid force buffers and compiled programs stay as they
        are.  The other two change parameters and restore them as energy_derivative does."""
        self._refuse_in_free_space('energies_at_states')
        names = list(names)
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(names))
        K = len(rows)
        for name in names:
            if name not in self.parameters:
                raise mm.OpenMMException('energies_at_states: no such Context parameter: ' + name)
        if any(isinstance(self.parameters[name], X.Deferred) for name in names):
            integ = self.integrator
            self._settle([integ._gvalues] if isinstance(integ, mm.CustomIntegrator) else [])     # (a lambda still on the device)
        here = {name: self.parameters[name] for name in names}
        varied = {name for i, name in enumerate(names) if np.any(rows[:, i] != here[name])}
        column = {name: rows[:, i] for i, name in enumerate(names)}

        def state(k, base=None):
            trial = dict(self.parameters if base is None else base)
            trial.update({name: float(column[name][k]) for name in varied})
            return trial

        fixed, soft, quadratic, loop = [], [], {}, []
        for entry in self.entries:
            hit = getattr(entry, 'depends', set()) & varied
            sc = entry.softcore
            if not hit:
                fixed.append(entry)
            elif sc is not None and hit == {sc['lambda_name']} and hasattr(self.ctx, 'pair_energy_states'):
                soft.append(entry)
            elif len(hit) == 1 and next(iter(hit)) in (getattr(entry, 'quadratic_in', None) or set()) | getattr(entry, 'charge_offsets_in', set()):
                quadratic.setdefault(next(iter(hit)), []).append(entry)
            else:
                loop.append(entry)
        for path, entries in (('once', fixed), ('states', soft), ('quadratic', [e for g in quadratic.values() for e in g]), ('loop', loop)):
            self.state_paths[path] += len(entries)
        for entry in [e for group in quadratic.values() for e in group] + loop:
            if entry.update is None:
                raise NotImplementedError('energies_at_states: a force that depends on a varied parameter cannot be re-parameterised')
        out = np.zeros(K)
        if soft:                        # (first: the evaluations below may leave the candidate list of the force behind them)
            torch = self.torch
            dev = self.x.device
            pair = torch.zeros(K, dtype=torch.float64, device=dev)
            for entry in soft:
                sc = entry.softcore
                lam = column[sc['lambda_name']]
                for k0 in range(0, K, B.MAX_STATES):
                    k1 = min(K, k0 + B.MAX_STATES)
                    self.ctx.pair_energy_states(sc['pid'], self.x, torch.as_tensor(lam[k0:k1], dtype=torch.float64, device=dev),
                                                pair[k0:k1])
                out += np.array([sc['constant'](state(k)) for k in range(K)])
            self._check()
            if self._coll:
                self._allreduce(pair)
            out += pair.cpu().numpy()
        if fixed:
            out += self._energy_of(fixed)
        if quadratic or loop:
            rebuilt = []

            def apply(trial, entries, names_):
                for entry in entries:
                    result = entry.update(trial, names_)
                    rebuilt.append(bool(result) and result != 'values')
            for name, entries in quadratic.items():
                values = column[name]
                distinct = np.unique(values)
                if len(distinct) <= 3:
                    points = [float(p) for p in distinct]
                else:                           # (the ends and the middle of the range: a well-conditioned interpolation)
                    points = [float(distinct[0]), 0.5 * float(distinct[0] + distinct[-1]), float(distinct[-1])]
                energies = []
                for p in points:
                    apply(dict(self.parameters, **{name: p}), entries, {name})
                    energies.append(self._energy_of(entries))
                for k, v in enumerate(values):
                    basis = [np.prod([(v - q) / (p - q) for q in points if q != p]) for p in points]
                    out[k] += sum(b * e for b, e in zip(basis, energies))
                apply(self.parameters, entries, {name})
            if loop:
                self.n_state_fallbacks += 1
                names_ = varied & set().union(*(e.depends for e in loop))
                for k in range(K):
                    apply(state(k), loop, names_)
                    out[k] += self._energy_of(loop)
                apply(self.parameters, loop, names_)
            if any(rebuilt):
                self._forget_groups()
                self._programs.clear()
                self._emit_memo.clear()
                self._segment_memo.clear()
            self._invalidate_forces()
        return out

    def _deriv_deferred(self, what, name, settle):
        """deriv(energy, name) of a host-walked program without waiting for the GPU: the softcore pair kernel in derivative
        mode leaves its sum in the next free slot of the pending buffer and the value is handed on as a deferred global
        (expr.Deferred); the same positions and parameters give the same object again (a RESPA block ends and the next one
        begins with the same derivative).  Forces that need difference quotients take the waiting path."""
        if what != 'energy':
            raise NotImplementedError('deriv(%s, ...): only deriv(energy, parameter) is supported' % what)
        if name in self._deriv_cache:
            return self._deriv_cache[name]
        if name not in self.parameters:
            raise mm.OpenMMException('deriv(energy, %s): no such Context parameter' % name)
        if any(e.softcore is None and name in getattr(e, 'depends', ()) for e in self.entries):
            settle()
            value = self.energy_derivative(name)
        else:
            if self._pending is None:
                self._pending = [self.torch.zeros(_SCALARS, dtype=self.torch.float64, device=self.x.device), 0]
            value = 0.0
            for entry in self.entries:
                sc = entry.softcore
                if sc is not None and sc['lambda_name'] == name:
                    if self._pending[1] >= _SCALARS:
                        settle()
                    slot = self._pending[1]
                    self._pending[1] += 1
                    lam = self.parameters[sc['lambda_name']]
                    # (lambda is a device scalar: so is the correction's derivative at it -- queued first: one launch with the block that moved lambda)
                    correction = self._lrc_derivative_on_device(sc, lam, settle) if isinstance(lam, X.Deferred) else None
                    self._flush_scalars()                 # (lambda itself may be an assignment still queued)
                    self.ctx.pair_energy_derivative(sc['pid'], self.x, self._pending[0][slot:slot + 1])
                    if isinstance(lam, X.Deferred):
                        if correction is not None:
                            value = value + correction
                        value = value + X.Deferred(0.0, {slot: 1.0})
                    else:
                        value = value + X.Deferred(sc['constant_derivative'](self.parameters), {slot: 1.0})
        self._deriv_cache[name] = value
        return value

    def _device_scalars_ok(self):
        """Deferred globals may be worked on where they are: single rank (the ranks' partial sums are added up at a settle), a
        backend with the scalar kernel."""
        return self.device_globals and not self._coll and hasattr(self.ctx, 'expr_eval_scalar')

    def _scalar_slot(self, settle):
        if self._pending is None:
            self._pending = [self.torch.zeros(_SCALARS, dtype=self.torch.float64, device=self.x.device), 0]
        if self._pending[1] >= _SCALARS:
            settle()
        slot = self._pending[1]
        self._pending[1] += 1
        return slot

    def _eval_global_on_device(self, expr, env, rng, settle, predicate=None, keep=None):
        """A global expression whose operands wait on device results, evaluated by one thread on the stream (amm_expr_eval_scalar):
        its value is a new device scalar, the host goes on without it (AFED: integrators.py:701-737, the extended variable's move,
        walls and thermostat).  Returns the Deferred that names the scalar."""
        return self._queue_scalar(X.compile_scalar(expr, env, rng, predicate, keep), settle)

    def _queue_scalar(self, prog, settle):
        self.n_scalar_evals += 1
        slot = self._scalar_slot(settle)
        # queued: consecutive assignments go out as ONE launch (_flush_scalars: before anything that reads a scalar is enqueued)
        if len(self._scalar_code) + len(prog.code) + 1 > 640 or len(self._scalar_consts) + len(prog.consts) > 96:
            self._flush_scalars()
        base = len(self._scalar_consts)
        const_ops = (X.OPCODES['CONST'], X.OPCODES['HORNER'])      # (words whose argument is a constant's index)
        self._scalar_code += [w + (base << 8) if (w & 0xff) in const_ops else w for w in prog.code]
        self._scalar_code.append(X.OPCODES['OUT'] | (slot << 8))
        self._scalar_consts += prog.consts
        return X.Deferred(0.0, {slot: 1.0})

    def _flush_scalars(self):
        if self._scalar_code:
            self.ctx.expr_eval_scalar(self._scalar_code, self._scalar_consts, self._pending[0])
            self.n_scalar_launches += 1
            self._scalar_code, self._scalar_consts = [], []

    def _lrc_derivative_on_device(self, sc, lam, settle):
        """d(long-range correction)/d(lambda) of a softcore force at a lambda that is a device scalar: the interpolant's monomial form
        in u = 2 lambda - 1, Horner, as one more assignment (queued with the block that moved lambda: no launch of its own)."""
        coef = sc['derivative_polynomial'](self.parameters)
        if not coef:
            return None
        key = (sc['pid'], tuple(sorted(lam.terms.items())), lam.const)
        if key not in self._lrc_on_device:
            self._lrc_on_device[key] = self._queue_scalar(X.compile_polynomial(coef, 2.0, -1.0, lam), settle)
        return self._lrc_on_device[key]

    def _parameter_to_device(self, name, value, settle):
        """context.setParameter(name, <a device scalar>): possible when every force that depends on the parameter is a softcore
        pair force with this lambda and the list-free kernel (its long-range correction's derivative follows as a polynomial) -- the
        solute-solvent force of SolvationSystem under AFED.  Returns False when the number is needed after all."""
        pids = []
        for entry in self.entries:
            sc = entry.softcore
            if sc is not None and name in sc['depends']:
                if sc['lambda_name'] != name:
                    return False
                pids.append(sc['pid'])
            elif name in getattr(entry, 'depends', ()):
                return False
        if not pids:
            return False
        if len(value.terms) != 1 or value.const != 0.0 or list(value.terms.values()) != [1.0]:
            value = self._eval_global_on_device('__v', {'__v': value}, None, settle)         # (a linear form: one scalar of its own)
        slot = next(iter(value.terms))
        try:
            for pid in pids:
                self.ctx.pair_set_lambda_dev(pid, self._pending[0], slot)
        except B.HipError:
            for pid in pids:
                self.ctx.pair_set_lambda_dev(pid, None, 0)
            return False
        self.parameters[name] = value
        self._device_params[name] = pids
        groups = {e.group for e in self.entries if e.softcore is not None and e.softcore['pid'] in pids}
        for g in self._valid:
            if g in groups or g == 'all':
                self._valid[g] = False
        self._deriv_cache.clear()
        self._programs.clear()
        return True

    def _settle(self, containers):
        """Read the pending device scalars (one synchronising copy; summed over the ranks first) and turn every deferred
        global in `containers` (dicts / lists) into its number."""
        if self._pending is None or self._pending[1] == 0:
            return
        self._flush_scalars()
        self._lrc_on_device = {}
        buf, used = self._pending
        if self._coll:
            self._allreduce(buf)
        values = buf[:used].cpu().numpy()
        self.n_settles += 1
        for box in containers + [self._deriv_cache]:
            keys = range(len(box)) if isinstance(box, list) else list(box)
            for k in keys:
                if isinstance(box[k], X.Deferred):
                    box[k] = box[k].resolve(values)
        # Context parameters that lived on the device (an extended variable between two reads): the host has their numbers again, and
        # the library its launch argument -- the same value its kernels read from the scalar until now: no force becomes stale
        for name, pids in self._device_params.items():
            value = self.parameters[name].resolve(values)
            self.parameters[name] = value
            for pid in pids:
                self.ctx.pair_set_lambda(pid, value)
            for entry in self.entries:
                if entry.softcore is not None and entry.softcore['pid'] in pids:
                    entry.constant = entry.softcore['constant'](self.parameters)
        self._device_params = {}
        buf.zero_()
        self._pending[1] = 0

    # ------------------------------------------------------------------------------- general step programs
    def _step_interpreted(self, n):
        """Programs with data-dependent globals (ComputeSum results, random numbers) or per-DOF expressions beyond kick /
        move / copy -- the thermostat propagators (propagators.py:276-827, 1108-2172): the host walks the program step by
        step; runs of kick / move / copy / EVAL ops still go to amm_run_ops, every other per-DOF or sum expression is
        compiled (atomsmm_amd/expr.py) and interpreted on the GPU (amm_expr_eval); global expressions are evaluated on
        the host.  A ComputeSum costs one device -> host read."""
        torch = self.torch
        integ = self.integrator
        steps = integ._steps
        C = mm.CustomIntegrator
        match, stack = {}, []
        for pc, (kind, _, _) in enumerate(steps):
            if kind in (C.IfBlock, C.WhileBlock):
                stack.append(pc)
            elif kind == C.EndBlock:
                begin = stack.pop()
                match[begin], match[pc] = pc, begin
        if self._host_rng is None:
            self._host_rng = np.random.default_rng(integ.getRandomNumberSeed())
        seed = int(integ.getRandomNumberSeed()) & (2 ** 64 - 1)
        total = torch.zeros(1, dtype=torch.float64, device=self.x.device)
        try:
            self._walk_program(int(n), steps, match, seed, total)
        finally:
            self._settle([integ._gvalues])         # no deferred global outlives the call
        self._check()

    def _walk_program(self, n, steps, match, seed, total):
        torch = self.torch
        integ = self.integrator
        C = mm.CustomIntegrator
        for _ in range(n):
            env = dict(_SAFE_FUNCS)
            env.update(self.parameters)
            env.update(zip(integ._gnames, integ._gvalues))
            env['dt'] = integ._dt

            # After a blocking read the GPU has nothing queued: the next ops go out in small batches (at the first moves, i.e. at
            # the end of a kick ... move pattern that amm_run_ops fuses) instead of waiting for the host to walk the whole block
            # -- at config C5 the GPU sat idle for 0.26 ms per AFED step behind the read of deriv(energy, lambda)
            eager = [0]

            preds = []          # if-blocks whose condition waits on the device: [end pc, predicate] (their steps are evaluated there, predicated)

            def settle():
                if self._pending is not None and self._pending[1] > 0 and not self._has_constraints:
                    eager[0] = 3          # (constraint ops stay in one batch with the move they follow)
                if self._device_params:
                    flush()               # (launches recorded so far read the parameter where it is now)
                held = [p[1] for p in preds]
                self._settle([env, integ._gvalues, held])
                for p, value in zip(preds, held):
                    p[1] = value

            def deferred_in(text):
                """Does the expression name a global whose number is still on the device?"""
                if self._pending is None or self._pending[1] == 0:
                    return False
                m = re.match(r'^(.*?)(<=|>=|!=|=|<|>)(.*)$', text) if re.search(r'[<>=]', text) else None      # (a block's condition)
                names = X.symbols(m.group(1)) | X.symbols(m.group(3)) if m else X.symbols(text)
                return any(isinstance(env.get(name), X.Deferred) for name in names)

            env['__deriv__'] = lambda what, name: self._deriv_deferred(what, name, settle)
            valid = self._valid
            self._mirror_work = self._mirror
            ops = [B.Op(B.OP_SAVE_REF, 0, 0, 0, 0.0)] if self._has_constraints else []

            def flush():
                # (a run of per-DOF steps that is being recorded as one unit is no unit any more: the ops before the flush are gone)
                self._segment_open = None
                if ops:
                    self._flush_scalars()     # (assignments to device scalars queued so far: the launches below may read them)
                    # a RESPA block between two host-evaluated steps is a static run of ops: pair the near and the outer
                    # evaluation of one list into a single traversal, as the compiled path does
                    self._run(self._pair_up_evals(list(ops)), 1, cache=False)
                    del ops[:]

            def resolve(name):
                if name == 'm':
                    return ('mass',)
                if name in ('x', 'v') or re.fullmatch(r'f[0-9]*', name) or name in integ._pnames:
                    return ('buf', self._force_ref(name, ops, valid))
                if name in env and not callable(env[name]):
                    return ('global',)
                return None

            pc = 0
            guard = 0
            while pc < len(steps):
                guard += 1
                if guard > 2_000_000:
                    raise RuntimeError('step program does not terminate')
                kind, target, expr = steps[pc]
                if self._pending is not None and self._pending[1] > _SCALARS - 64:
                    settle()            # (room for the scalars a step may ask for; what was deferred is a number from here on)
                if kind == C.ComputePerDof:
                    # a straight run of per-DOF steps (a RESPA block of the atoms inside an AFED step: ~60 kicks, moves and
                    # copies) emits the same ops whenever the globals it names, the valid force groups and the mirrored buffers
                    # are the same: remembered as ONE unit (the host was slower than the GPU at config C5 walking it step by step)
                    pc_end = self._run_end(steps, pc)
                    # (while THIS run is being recorded its later steps must not ask again: _replay_segment would drop the record
                    # and open one for the remainder -- only the last four steps of a run were ever remembered as a unit)
                    rec = self._segment_open
                    recording = rec is not None and rec[1] == pc_end and not eager[0]
                    if not recording and pc_end - pc >= 4 and not eager[0] and self._replay_segment(pc, pc_end, steps, env, ops, valid):
                        pc = pc_end
                        continue
                if kind == C.ComputeGlobal:
                    if 'deriv(' in expr:
                        flush()                                   # the derivative is taken at the current positions
                    rng_state = self._host_rng.bit_generator.state
                    pred = preds[-1][1] if preds else None
                    if isinstance(pred, X.Deferred):
                        # inside an if-block whose condition is still on the device: target <- select(condition, expression, target)
                        value = self._eval_global_on_device(expr, env, self._host_rng, settle, pred, env[target])
                    elif pred is not None and not pred:
                        pc += 1                                   # (the condition was read after all, and is false)
                        continue
                    else:
                        try:
                            value = X.eval_global(expr, env, self._host_rng)
                        except X.NeedsValue:                      # more than sums and multiples of a deferred global
                            self._host_rng.bit_generator.state = rng_state
                            value = None
                            if self._device_scalars_ok():
                                try:
                                    value = self._eval_global_on_device(expr, env, self._host_rng, settle)
                                except (X.NeedsValue, X.ExpressionError):
                                    self._host_rng.bit_generator.state = rng_state
                                    value = None
                            if value is None:
                                settle()
                                value = X.eval_global(expr, env, self._host_rng)
                    if target in self.parameters and target not in integ._gnames:
                        done = False
                        if isinstance(value, X.Deferred):         # a Context parameter: on the device if its forces can read it there
                            if self._device_scalars_ok():
                                flush()
                                done = self._parameter_to_device(target, value, settle)
                                if done:
                                    value = self.parameters[target]
                                    valid = self._valid
                            if not done:
                                env[target] = value
                                settle()
                                value = env[target]
                        if not done and (isinstance(self.parameters[target], X.Deferred) or value != self.parameters[target]):
                            flush()
                            if isinstance(self.parameters[target], X.Deferred):
                                settle()
                            self.set_parameter(target, value)     # an extended-system variable (AFED): forces change
                            valid = self._valid
                    env[target] = value
                elif kind in (C.ComputePerDof, C.ComputeSum):
                    if deferred_in(expr):
                        settle()
                    done = False
                    if kind == C.ComputePerDof:
                        try:
                            self._emit_per_dof_memo(pc, target, expr, env, ops, valid)
                            done = True
                        except (NotImplementedError, NameError, SyntaxError, TypeError):
                            done = False
                        self._record_segment(pc, done, ops, valid)
                        if done and eager[0] and target == 'x':
                            eager[0] -= 1
                            flush()
                    if not done:
                        _refuse_vector_functions(expr)
                        prog = X.compile_per_dof(expr, resolve)
                        flush()                                   # EVALs emitted by resolve() run first
                        gvals = [float(env[name]) for name in prog.globals_]
                        self._expr_counter += 1
                        if kind == C.ComputePerDof:
                            if target not in ('x', 'v') and target not in integ._pnames:
                                raise mm.OpenMMException('unknown per-DOF variable: ' + target)
                            dst = self.x if target == 'x' else (self.v if target == 'v' else self._buffer(target))
                            self._slot(target)
                            self.ctx.expr_eval(prog.code, prog.consts, gvals, seed, self._expr_counter, dst=dst)
                            self._mirror_work.pop(target, None)
                            for d in [d for d, sname in self._mirror_work.items() if sname == target]:
                                del self._mirror_work[d]
                            if target == 'x':
                                for g in valid:
                                    valid[g] = False
                                self._deriv_cache.clear()
                        else:
                            self.ctx.expr_eval(prog.code, prog.consts, gvals, seed, self._expr_counter, total=total)
                            env[target] = total.item()          # device -> host (synchronises)
                elif kind in (C.ConstrainPositions, C.ConstrainVelocities):
                    self._emit_constraint(kind, ops, valid)
                elif kind == C.UpdateContextState:
                    pass
                elif kind in (C.IfBlock, C.WhileBlock):
                    if deferred_in(expr):
                        body = steps[pc + 1:match[pc]]
                        if (kind == C.IfBlock and self._device_scalars_ok() and body and all(b[0] == C.ComputeGlobal for b in body)
                                and not any('deriv(' in b[2] for b in body)):
                            # the condition stays on the device (1 or 0) and the block's steps are evaluated there, predicated --
                            # the reflecting walls of an extended variable (integrators.py:701-714)
                            lhs, op, rhs = re.match(r'^(.*?)(<=|>=|!=|=|<|>)(.*)$', expr).groups()
                            diff = '((%s)-(%s))' % (lhs, rhs)
                            text = {'=': 'delta(%s)', '!=': '1-delta(%s)', '>=': 'step(%s)', '<': '1-step(%s)',
                                    '<=': 'step(-%s)', '>': '1-step(-%s)'}[op] % diff
                            preds.append([match[pc], self._eval_global_on_device(text, env, None, settle)])
                            pc += 1
                            continue
                        settle()
                    if not self._condition(expr, env):
                        pc = match[pc]
                elif kind == C.EndBlock:
                    if preds and preds[-1][0] == pc:
                        preds.pop()
                    if steps[match[pc]][0] == C.WhileBlock:
                        pc = match[pc] - 1
                pc += 1
            flush()
            for k, name in enumerate(integ._gnames):
                integ._gvalues[k] = env[name]
            self.time += integ._dt

    def step(self, n):
        """n steps of the integrator's program.  With a MonteCarloBarostat the attempt of every `frequency`-th step is made right
        before that step, and the steps between two attempts run as one chunk (the compiled `repeat` path)."""
        remaining = int(n)
        if self.barostat is None or remaining <= 0:
            return self._step_program(n)
        while remaining > 0:
            frequency = self.barostat.getFrequency()
            if frequency <= 0:
                return self._step_program(remaining)
            if self._baro_due is None:
                self._baro_due = frequency - 1
            if self._baro_due <= 0:
                self._barostat_attempt()
                self._baro_due = frequency
            count = min(remaining, self._baro_due)
            self._step_program(count)
            self._baro_due -= count
            remaining -= count

    def _step_program(self, n):
        integ = self.integrator
        if not isinstance(integ, mm.CustomIntegrator):
            raise NotImplementedError('the HIP path runs CustomIntegrator step programs and the stock Verlet, Langevin, LangevinMiddle '
                                      'and Brownian integrators; %s is neither' % type(integ).__name__)
        if self._stock is not None and self.world > 1:
            raise NotImplementedError('stock integrators run on one rank')
        if self._seed_set != integ.getRandomNumberSeed():
            self._seed_set = integ.getRandomNumberSeed()
            self.ctx.expr_seed(self._seed_set)
        if self._interpreted is None:
            # static programs (RESPA, also with bath steps inside the loops) are unrolled once and replayed; programs
            # with data-dependent globals (ComputeSum results, random globals) go through the general path
            try:
                self._compile()
                self._interpreted = False
            except VectorExpressionError:
                self._static_exprs = False
                raise
            except (NotImplementedError, NameError, SyntaxError, TypeError, KeyError, X.ExpressionError):
                self._static_exprs = False
                self._interpreted = True
                if hasattr(self.ctx, 'regulated_define'):
                    self.ctx.regulated_define(False)       # (the general path writes regulated moves as expressions)
        if self._interpreted:
            return self._step_interpreted(n)
        remaining = int(n)
        while remaining > 0:
            key = self._program_key(self._valid, self._mirror)
            if key not in self._programs:
                self._programs[key] = self._compile()
            ops, valid_after, finals, mirror_after = self._programs[key]
            after_key = self._program_key(valid_after, mirror_after)
            count = remaining if after_key == key else 1
            self._run(ops, count)
            self._valid = dict(valid_after)
            self._mirror = dict(mirror_after)
            for name, value in finals.items():
                integ._gvalues[integ._gnames.index(name)] = value
            remaining -= count
            self.time += count * integ._dt
        self._check()

    # measurement helpers (bench / tests)
    def pair_force_ids(self, group):
        return [pid for e in self.entries if e.group == group for pid in e.pair_ids]

    def recip_force_ids(self, group):
        """Library ids of the PME reciprocal-space forces of a force group (amm_pme_create)."""
        return [e.recip for e in self.entries if getattr(e, 'recip', None) is not None and e.recip_group == group]
