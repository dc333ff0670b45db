"""GPU tests (run with -m gpu on an MI355X) of virtual sites and massless particles: csrc/vsite.hip through the ABI against the
numpy restatement (tests/vsite_ref.py), the integrating ops over states with massless particles against tests/stock_ref.py on the
massive atoms, and TIP4P-Ew water (tests/golden/data/tip4pew.xml) end to end -- forces, steps, list safety and the drop-in script.

Bounds: positions 1e-12 nm and velocities 1e-12/dt (the device-against-restatement bounds of test_gpu_stock.py), forces 1e-12 of
the largest component, net forces 1e-12 of the sum of the components' magnitudes.

Worst deviations measured on an MI355X (every test prints its own): place and spread give the restatement's bits; the stock steps on
the synthetic state 1.2e-14 nm and 2.7e-12 nm/ps; the forces with sites equal the spread raw forces bit for bit (PME and
CutoffPeriodic); three steps against the manual loop 3.6e-15 nm and 1.1e-12 nm/ps; after 200 steps (38 list builds) the aged lists'
forces differ from a fresh Context's by 1.8e-12 kJ/mol/nm against a bound of 2.8e-9."""
import copy
import functools
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import expr as X  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.openmm import app  # noqa: E402
from atomsmm_amd.utils import InputError  # noqa: E402
import stock_ref as SR  # noqa: E402
import vsite_ref as VR  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'data', 'tip4pew.xml')
KB = unit.BOLTZMANN_CONSTANT_kB._value
DT, TEMPERATURE, SEED, STEPS = 0.002, 300.0, 20261, 3
KT = KB * TEMPERATURE
FRICTION = {SR.VERLET: 0.0, SR.LANGEVIN_MIDDLE: 5.0, SR.LANGEVIN: 5.0, SR.BROWNIAN: 100.0}     # 1/ps
BOUND_X, BOUND_V = 1e-12, 1e-12 / DT
R_OH, THETA, D_OM = 0.09572, math.radians(104.52), 0.0125
W_H = D_OM / (2.0 * R_OH * math.cos(0.5 * THETA))
W_O = 1.0 - 2.0 * W_H
R_HH = 2.0 * R_OH * math.sin(0.5 * THETA)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def same_bits(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64)))


# ------------------------------------------------------------------------------------ the synthetic state of tests 1 .. 4
@functools.lru_cache(maxsize=None)
def synthetic():
    """300 four-site waters (rigid triangle + an average3 site), 20 TIP5P-like molecules (rigid triangle whose O carries two
    out-of-plane sites), 10 constrained pairs with a two-parent average site, one trio of free atoms whose first atom is a parent of
    four sites (in role 0, 1, 2 and 0 again) and 37 free atoms, five of them massless non-sites; the molecules in random order and
    the site table shuffled.  354 sites: more than one 256-thread block, no multiple of 64.  Positions on the constraint surface with
    the sites placed, Gaussian velocities (0 for massless rows), a fixed random force buffer (sigma 300)."""
    rng = np.random.default_rng(4242)
    kinds = ['w4'] * 300 + ['w5'] * 20 + ['pair'] * 10 + ['four'] + ['free'] * 32 + ['ghost'] * 5
    rng.shuffle(kinds)
    xs, ms, pairs, dist, sites = [], [], [], [], []

    def unit_vector():
        a = rng.normal(size=3)
        return a / np.linalg.norm(a)

    def triangle(origin):
        a = unit_vector()
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        half = 0.5 * THETA
        return [origin, origin + R_OH * (np.cos(half) * a + np.sin(half) * b), origin + R_OH * (np.cos(half) * a - np.sin(half) * b)]
    for kind in kinds:
        base, origin = len(xs), rng.uniform(0, 6, 3)
        if kind in ('w4', 'w5'):
            xs += triangle(origin)
            ms += [15.99943, 1.007947, 1.007947]
            pairs += [(base, base + 1), (base, base + 2), (base + 1, base + 2)]
            dist += [R_OH, R_OH, R_HH]
            if kind == 'w4':
                xs.append(origin)
                ms.append(0.0)
                sites.append((base + 3, VR.AVERAGE3, (base, base + 1, base + 2), (W_O, W_H, W_H)))
            else:
                xs += [origin, origin]
                ms += [0.0, 0.0]
                sites.append((base + 3, VR.OUT_OF_PLANE, (base, base + 1, base + 2), (-0.344908, -0.344908, -6.4437903)))
                sites.append((base + 4, VR.OUT_OF_PLANE, (base, base + 1, base + 2), (-0.344908, -0.344908, 6.4437903)))
        elif kind == 'pair':
            xs += [origin, origin + 0.109 * unit_vector(), origin]
            ms += [12.011, 1.008, 0.0]
            pairs.append((base, base + 1))
            dist.append(0.109)
            sites.append((base + 2, VR.AVERAGE2, (base + 1, base), (1.3, -0.3)))
        elif kind == 'four':
            xs += [origin, origin + 0.15 * unit_vector(), origin + 0.15 * unit_vector()] + [origin] * 4
            ms += [12.011, 14.0067, 15.9994, 0.0, 0.0, 0.0, 0.0]
            sites.append((base + 3, VR.AVERAGE2, (base, base + 1), (0.4, 0.6)))
            sites.append((base + 4, VR.AVERAGE2, (base + 1, base), (0.7, 0.3)))
            sites.append((base + 5, VR.AVERAGE3, (base + 1, base + 2, base), (0.2, 0.3, 0.5)))
            sites.append((base + 6, VR.OUT_OF_PLANE, (base, base + 1, base + 2), (0.3, 0.2, 2.5)))
        else:
            xs.append(origin)
            ms.append(0.0 if kind == 'ghost' else float(rng.choice([1.008, 12.011, 15.9994, 35.453])))
    order = rng.permutation(len(sites))
    table = VR.table([sites[k] for k in order])
    mass = np.array(ms)
    n = len(mass)
    x = VR.place(np.array(xs), *table)
    v = rng.normal(size=(n, 3)) * np.sqrt(KT / np.where(mass > 0, mass, 1.0))[:, None]
    v[mass == 0] = 0.0
    f = rng.normal(0.0, 300.0, (n, 3))
    assert len(sites) == 354 and int((mass == 0).sum()) == 359
    owners = np.bincount(table[2][table[2] >= 0].ravel(), minlength=n)
    assert owners.max() == 4 and int((owners == 2).sum()) >= 20           # the parent of four sites; a TIP5P-like O owns two
    return dict(x=x, v=v, f=f, mass=mass, pairs=np.array(pairs, dtype=np.int32), dist=np.array(dist), table=table, n=n)


def abi_context(s, with_sites=True):
    ctx = B.HipContext(s['n'], np.array([6.0, 6.0, 6.0]))
    if with_sites:
        ctx.vsite_define(*s['table'])
    return ctx


# ------------------------------------------------------------------------------------ 1, 2: the kernels through the ABI
def test_place_through_the_abi():
    s = synthetic()
    site = s['table'][0]
    start = s['x'].copy()
    start[site] = np.random.default_rng(1).uniform(-50, 50, (len(site), 3))           # wherever the sites were
    ctx = abi_context(s)
    x = dev(start)
    ctx.vsite_place(x)
    ctx.check()
    got, want = x.cpu().numpy(), VR.place(start, *s['table'])
    err = np.abs(got - want).max()
    print('place: max|dx| = %.2e nm (bound %.0e); same bits as the restatement: %s' % (err, BOUND_X, same_bits(got, want)))
    assert err <= BOUND_X
    rest = np.ones(s['n'], dtype=bool)
    rest[site] = False
    assert same_bits(got[rest], start[rest])
    assert ctx.vsite_stats() == dict(places=1, spreads=0, launches=1, sites=354)
    ctx.close()


def test_spread_through_the_abi():
    s = synthetic()
    site = s['table'][0]
    ctx = abi_context(s)
    x = dev(s['x'])
    want = VR.spread(s['x'], s['f'], *s['table'])
    results = []
    for _ in range(2):
        f = dev(s['f'])
        ctx.vsite_spread(x, f)
        ctx.check()
        results.append(f.cpu().numpy())
    got = results[0]
    fmax = np.abs(s['f']).max()
    err = np.abs(got - want).max()
    net = np.abs(got.sum(axis=0) - s['f'].sum(axis=0)).max()
    print('spread: max|df| = %.2e (bound %.2e), net force off by %.2e (bound %.2e)' % (err, 1e-12 * fmax, net, 1e-12 * np.abs(s['f']).sum()))
    assert err <= 1e-12 * fmax
    assert np.all(got[site] == 0.0)
    assert net <= 1e-12 * np.abs(s['f']).sum()
    assert same_bits(results[0], results[1])
    untouched = np.ones(s['n'], dtype=bool)
    untouched[site] = False
    untouched[s['table'][2][s['table'][2] >= 0]] = False
    assert same_bits(got[untouched], s['f'][untouched])
    assert ctx.vsite_stats() == dict(places=0, spreads=2, launches=4, sites=354)
    ctx.close()


def test_define_refuses_bad_tables():
    s = synthetic()
    site, kind, parents, weights = [a.copy() for a in s['table']]
    ctx = abi_context(s, with_sites=False)
    cases = []
    bad = parents.copy()
    bad[5, 0] = s['n']
    cases.append(((site, kind, bad, weights), 'out of range'))
    bad = parents.copy()
    bad[5, 0] = site[9]
    cases.append(((site, kind, bad, weights), 'is a site itself'))
    bad = site.copy()
    bad[3] = bad[4]
    cases.append(((bad, kind, parents, weights), 'a site already'))
    bad = kind.copy()
    bad[0] = 3
    cases.append(((site, bad, parents, weights), 'unknown kind'))
    for args, text in cases:
        with pytest.raises(B.HipError, match=text):
            ctx.vsite_define(*args)
    assert ctx.vsite_stats()['sites'] == 0
    x = dev(s['x'])
    ctx.vsite_place(x)                         # (no sites: nothing runs)
    assert same_bits(x.cpu().numpy(), s['x'])
    ctx.vsite_define(*s['table'])
    ctx.vsite_define([], [], [], [])
    assert ctx.vsite_stats()['sites'] == 0
    ctx.close()


# ------------------------------------------------------------------------------------ 3: the stock integrators with massless particles
def synthetic_system():
    """The synthetic state as a System whose only force is a constant external one: the fixed force buffer."""
    s = synthetic()
    system = openmm.System()
    for m in s['mass']:
        system.addParticle(float(m))
    for (i, j), d in zip(s['pairs'].tolist(), s['dist']):
        system.addConstraint(i, j, float(d))
    classes = {VR.AVERAGE2: openmm.TwoParticleAverageSite, VR.AVERAGE3: openmm.ThreeParticleAverageSite, VR.OUT_OF_PLANE: openmm.OutOfPlaneSite}
    site, kind, parents, weights = s['table']
    for row in range(len(site)):
        count = 2 if kind[row] == VR.AVERAGE2 else 3
        members, w = [int(p) for p in parents[row, :count]], [float(c) for c in weights[row, :count]]
        system.setVirtualSite(int(site[row]), classes[int(kind[row])](*members, *w))
    force = openmm.CustomExternalForce('-(fx*x+fy*y+fz*z)')
    for name in ('fx', 'fy', 'fz'):
        force.addPerParticleParameter(name)
    for i, row in enumerate(s['f']):
        force.addParticle(i, [float(c) for c in row])
    system.addForce(force)
    return system


def sorted_table(s):
    """The site table in the order the engine defines it: by site index."""
    order = np.argsort(s['table'][0])
    return tuple(a[order] for a in s['table'])


@functools.lru_cache(maxsize=None)
def massive_reference(kind):
    """STEPS steps of the restatement on the massive atoms: the sites' forces spread, stock_ref.step with the massless rows given a
    mass of 1 (the random numbers are indexed by the degree of freedom of the whole system, and a massless atom is in no cluster, so
    its row touches no other) and put back afterwards, the sites placed again."""
    s = synthetic()
    T = sorted_table(s)
    massless = s['mass'] == 0
    safe = np.where(massless, 1.0, s['mass'])
    clusters = SR.Clusters(s['n'], s['pairs'], s['dist'])
    x, v = s['x'], s['v']
    for k in range(1, STEPS + 1):
        f = VR.spread(x, s['f'], *T)
        xn, vn, _ = SR.step(kind, x, v, f, safe, clusters, DT, FRICTION[kind], KT, 1e-5, SEED, k)
        xn[massless], vn[massless] = x[massless], v[massless]
        x, v = VR.place(xn, *T), vn
    return x, v


def stock_integrator(kind):
    fs, ps, K = unit.femtoseconds, unit.picoseconds, unit.kelvin
    if kind == SR.VERLET:
        integrator = openmm.VerletIntegrator(2 * fs)
    elif kind == SR.LANGEVIN_MIDDLE:
        integrator = openmm.LangevinMiddleIntegrator(TEMPERATURE * K, FRICTION[kind] / ps, 2 * fs)
    elif kind == SR.LANGEVIN:
        integrator = openmm.LangevinIntegrator(TEMPERATURE * K, FRICTION[kind] / ps, 2 * fs)
    else:
        integrator = openmm.BrownianIntegrator(TEMPERATURE * K, FRICTION[kind] / ps, 2 * fs)
    integrator.setRandomNumberSeed(SEED)
    return integrator


@pytest.mark.parametrize('native', [True, False], ids=['stock_op', 'op_by_op'])
@pytest.mark.parametrize('kind', [SR.VERLET, SR.LANGEVIN_MIDDLE, SR.LANGEVIN, SR.BROWNIAN])
def test_stock_steps_leave_massless_particles_alone(kind, native):
    s = synthetic()
    massless = s['mass'] == 0
    site = s['table'][0]
    ghosts = massless.copy()
    ghosts[site] = False
    assert int(ghosts.sum()) == 5
    context = openmm.Context(synthetic_system(), stock_integrator(kind))
    context._engine.set_stock_native(native)
    context.setPositions(s['x'] * unit.nanometers)
    context.setVelocities(s['v'])
    context.getIntegrator().step(STEPS)
    state = context.getState(getPositions=True, getVelocities=True)
    x, v = state.getPositions(asNumpy=True)._value, state.getVelocities(asNumpy=True)._value
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(v))
    assert same_bits(x[ghosts], s['x'][ghosts]) and same_bits(v[massless], s['v'][massless])
    want_x, want_v = massive_reference(kind)
    dx, dv = np.abs(x - want_x)[~massless].max(), np.abs(v - want_v)[~massless].max()
    ds = np.abs(x - VR.place(x, *sorted_table(s)))[site].max()
    print('kind %d %s: massive atoms max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e (bound %.0e); sites off their parents by %.2e nm'
          % (kind, 'AMM_OP_STOCK' if native else 'op by op', dx, BOUND_X, dv, BOUND_V, ds))
    assert dx < BOUND_X and dv < BOUND_V
    assert ds <= BOUND_X
    assert np.abs(x - s['x'])[~massless].max() > 1e-4                   # something moved
    rules = context._engine.ctx.run_rule_stats()
    assert sum(v for k, v in rules.items() if k != 'plain') == 0, rules


# ------------------------------------------------------------------------------------ 4: kick, bath and per-DOF expression
def run_primitives(mass):
    """A kick, an Ornstein-Uhlenbeck bath and the per-DOF expression v <- v + 0.5*x/m over the synthetic state with `mass`."""
    s = synthetic()
    ctx = abi_context(s, with_sites=False)
    x, v, f, m = dev(s['x']), dev(s['v']), dev(s['f']), dev(mass)
    ctx.bind_state(x, v, m)
    ctx.bind_buffer(0, f)
    ctx.expr_seed(SEED)
    out = {}
    ctx.kick(v, f, m, 0.001)
    out['kick'] = v.cpu().numpy()
    ctx.run_ops([B.Op(B.OP_KICK, 0, -1, 0, 0.001), B.Op(B.OP_KICK, 0, -1, 0, 0.0005), B.Op(B.OP_MOVE, 0, 0, 0, 0.002)], 1)
    out['kicks_move_v'], out['kicks_move_x'] = v.cpu().numpy(), x.cpu().numpy()
    bid = ctx.bath_define(0.9, KT)
    ctx.run_ops([B.Op(B.OP_BATH, bid, B.SLOT_V, 0, 0.0)], 1)
    out['bath'] = v.cpu().numpy()

    def resolve(name):
        return {'x': ('buf', B.SLOT_X), 'v': ('buf', B.SLOT_V), 'm': ('mass',)}.get(name)
    prog = X.compile_per_dof('v + 0.5*x/m', resolve)
    ctx.expr_eval(prog.code, prog.consts, [], SEED, 7, dst=v)
    out['expr'] = v.cpu().numpy()
    eid = ctx.expr_define(prog.code, prog.consts, [])
    ctx.run_ops([B.Op(B.OP_EXPR, eid, B.SLOT_V, 0, 0.0)], 1)
    out['expr_op'] = v.cpu().numpy()
    # ... and a ComputeSum: massless degrees of freedom add nothing (v = 0 there: with m = 0 the term would be 0/0)
    total = torch.zeros(1, dtype=torch.float64, device='cuda')
    prog = X.compile_per_dof('v*v/m', resolve)
    ctx.expr_eval(prog.code, prog.consts, [], SEED, 8, total=total)
    out['sum'] = total.cpu().numpy()
    ctx.check()
    ctx.close()
    return out


def test_kick_bath_and_expression_skip_massless_rows():
    s = synthetic()
    massless = s['mass'] == 0
    got = run_primitives(s['mass'])
    plain = run_primitives(np.where(massless, 1.0, s['mass']))            # no zero in the mass array: the behaviour before
    # the sum over the massive degrees of freedom only; 4 122 positive terms in another order: within 4 122 x 2^-53 < 1e-12 relative
    total = got.pop('sum')[0]
    plain.pop('sum')
    vm = got['expr_op'][~massless]
    want = float(np.sum(vm * vm / s['mass'][~massless][:, None]))
    assert np.isfinite(total) and abs(total - want) <= 1e-12 * want
    for name, values in got.items():
        assert np.all(np.isfinite(values)), name
        start = s['x'] if name.endswith('_x') else s['v']
        assert same_bits(values[massless], start[massless]), name          # (v = 0 there: the move leaves x as it is)
        assert same_bits(values[~massless], plain[name][~massless]), name
    assert not same_bits(plain['expr'][massless], s['v'][massless])       # (with a mass those rows do move)


# ------------------------------------------------------------------------------------ 5 .. 8: TIP4P-Ew water end to end
@functools.lru_cache(maxsize=None)
def tip4pew_box():
    """512 TIP4P-Ew waters in the 2.5 nm box: the oxygens and the O-H directions of the q-SPC-FW fixture, the bonds cut to r_OH,
    the M site placed by the restatement."""
    d = np.load(os.path.join(HERE, 'golden', 'q-SPC-FW.npz'))
    p = d['positions'].reshape(512, 3, 3)                  # (H1, O, H2)
    x = np.zeros((512, 4, 3))
    x[:, 0] = p[:, 1]
    for k, h in ((1, 0), (2, 2)):
        u = p[:, h] - p[:, 1]
        x[:, k] = p[:, 1] + R_OH * u / np.linalg.norm(u, axis=1)[:, None]
    x = x.reshape(2048, 3)
    table = VR.table([(4 * w + 3, VR.AVERAGE3, (4 * w, 4 * w + 1, 4 * w + 2), (W_O, W_H, W_H)) for w in range(512)])
    top = app.Topology.from_arrays(['O', 'H1', 'H2', 'M'] * 512, ['HOH'] * 2048, residue_index=np.repeat(np.arange(512), 4))
    top.setUnitCellDimensions(tuple(float(b) for b in d['box']))
    return dict(x=VR.place(x, *table), table=table, topology=top, box=d['box'].copy())


def tip4pew_system(method, rigid=True):
    c = tip4pew_box()
    system = app.ForceField(FIXTURE).createSystem(c['topology'], nonbondedMethod=method, nonbondedCutoff=0.9 * unit.nanometers,
                                                  rigidWater=rigid, removeCMMotion=False)
    assert system.getNumParticles() == 2048 and sum(system.isVirtualSite(i) for i in range(2048)) == 512
    assert system.getNumConstraints() == (1536 if rigid else 0)
    return system


def without_sites(system):
    """The same particles and forces, the M particles plain massless ones: the path that was there before virtual sites."""
    plain = copy.deepcopy(system)
    plain._vsites = {}
    return plain


def forces_and_energy(context):
    state = context.getState(getForces=True, getEnergy=True)
    return state.getForces(asNumpy=True)._value, state.getPotentialEnergy()._value


@pytest.mark.parametrize('method', ['PME', 'CutoffPeriodic'])
def test_forces_with_sites_are_the_spread_raw_forces(method):
    c = tip4pew_box()
    system = tip4pew_system(getattr(app, method))
    site = c['table'][0]
    moved = c['x'].copy()
    moved[site] += 0.3                                       # the sites start anywhere: computeVirtualSites brings them home
    with_sites = openmm.Context(system, openmm.VerletIntegrator(0.002))
    with_sites.setPositions(moved * unit.nanometers)
    with_sites.computeVirtualSites()
    x = with_sites.getState(getPositions=True).getPositions(asNumpy=True)._value
    assert np.abs(x - c['x']).max() <= BOUND_X
    plain = openmm.Context(without_sites(system), openmm.VerletIntegrator(0.002))
    plain.setPositions(x * unit.nanometers)
    f, e = forces_and_energy(with_sites)
    raw, e_raw = forces_and_energy(plain)
    want = VR.spread(x, raw, *c['table'])
    fmax = np.abs(raw).max()
    err, net = np.abs(f - want).max(), np.abs(f.sum(axis=0) - raw.sum(axis=0)).max()
    print('%s: E = %.6f, |dE|/|E| = %.2e; max|df| = %.2e (bound %.2e); net force off by %.2e (bound %.2e)' %
          (method, e, abs(e - e_raw) / abs(e_raw), err, 1e-12 * fmax, net, 1e-12 * np.abs(raw).sum()))
    assert np.isfinite(e) and abs(e - e_raw) <= 1e-12 * abs(e_raw)
    assert np.abs(raw[site]).max() > 1.0                    # the sites do collect force
    assert err <= 1e-12 * fmax
    assert np.all(f[site] == 0.0)
    assert net <= 1e-12 * np.abs(raw).sum()


def rule_decisions(context):
    """Decisions of the six fusion rules, epilogue plans offered to an evaluation and epilogues carried: all 0 with sites."""
    ctx = context._engine.ctx
    rules = ctx.run_rule_stats()
    return sum(v for k, v in rules.items() if k != 'plain') + ctx.run_stats()['epilogues']


@pytest.mark.parametrize('name', ['verlet', 'middle'])
def test_steps_against_the_manual_loop(name):
    """Three steps of rigid TIP4P-Ew water, 2 fs, against: raw forces of the Context without sites at the current positions ->
    vsite_ref.spread -> stock_ref.step on the massive atoms -> vsite_ref.place."""
    c = tip4pew_box()
    T = c['table']
    system = tip4pew_system(app.PME)
    kind = SR.VERLET if name == 'verlet' else SR.LANGEVIN_MIDDLE
    friction = 0.0 if name == 'verlet' else 1.0

    def integrator():
        if name == 'verlet':
            return openmm.VerletIntegrator(2 * unit.femtoseconds)
        result = openmm.LangevinMiddleIntegrator(TEMPERATURE * unit.kelvin, friction / unit.picosecond, 2 * unit.femtoseconds)
        result.setRandomNumberSeed(SEED)
        return result
    context = openmm.Context(system, integrator())
    context.setPositions(c['x'] * unit.nanometers)
    context.applyConstraints()
    context.setVelocitiesToTemperature(TEMPERATURE * unit.kelvin, 4)
    state = context.getState(getPositions=True, getVelocities=True)
    x, v = state.getPositions(asNumpy=True)._value, state.getVelocities(asNumpy=True)._value
    site = T[0]
    assert np.abs(x - VR.place(x, *T)).max() <= BOUND_X and np.all(v[site] == 0.0)
    plain = openmm.Context(without_sites(system), openmm.VerletIntegrator(0.002))
    masses = np.array(system._masses)
    massless = masses == 0
    safe = np.where(massless, 1.0, masses)
    clusters = SR.Clusters(2048, np.array([(i, j) for i, j, _ in system._constraints]), np.array([d for _, _, d in system._constraints]))
    stats0 = context._engine.ctx.vsite_stats()
    context.getIntegrator().step(STEPS)
    stats1 = context._engine.ctx.vsite_stats()
    for k in range(1, STEPS + 1):
        plain.setPositions(x * unit.nanometers)
        raw = plain.getState(getForces=True).getForces(asNumpy=True)._value
        f = VR.spread(x, raw, *T)
        xn, vn, _ = SR.step(kind, x, v, f, safe, clusters, DT, friction, KT, 1e-5, SEED, k)
        xn[massless], vn[massless] = x[massless], v[massless]
        x, v = VR.place(xn, *T), vn
    state = context.getState(getPositions=True, getVelocities=True)
    got_x, got_v = state.getPositions(asNumpy=True)._value, state.getVelocities(asNumpy=True)._value
    dx, dv = np.abs(got_x - x).max(), np.abs(got_v - v).max()
    # (the engine keeps one program per set of valid force buffers; each is the evaluation of all forces and the step behind it)
    per_program = {sum(1 for op in ops if not isinstance(op, tuple) and op.op == B.OP_EVAL) for ops, _, _, _ in context._engine._programs.values()}
    assert len(per_program) == 1
    evals = per_program.pop()
    print('%s: max|dx| = %.2e nm (bound %.0e), max|dv| = %.2e (bound %.0e); places %d, spreads %d in %d steps, %d EVAL ops per step'
          % (name, dx, BOUND_X, dv, BOUND_V, stats1['places'] - stats0['places'], stats1['spreads'] - stats0['spreads'], STEPS, evals))
    assert dx < BOUND_X and dv < BOUND_V
    assert np.all(got_v[site] == 0.0)
    assert np.abs(got_x - c['x'])[~massless].max() > 1e-4
    assert rule_decisions(context) == 0
    assert evals >= 1
    assert stats1['places'] - stats0['places'] == STEPS                  # one placement per step
    assert stats1['spreads'] - stats0['spreads'] == STEPS * evals        # one spread per evaluation


def test_lists_stay_safe_over_200_steps():
    """200 Langevin-middle steps at 300 K with the default Verlet buffer: the forces the aged lists give equal those of a fresh
    Context at the final positions.  A site whose displacement went unchecked would be missing partners here."""
    c = tip4pew_box()
    system = tip4pew_system(app.PME)
    integrator = openmm.LangevinMiddleIntegrator(TEMPERATURE * unit.kelvin, 1 / unit.picosecond, 2 * unit.femtoseconds)
    integrator.setRandomNumberSeed(SEED)
    context = openmm.Context(system, integrator)
    context.setPositions(c['x'] * unit.nanometers)
    context.applyConstraints()
    context.setVelocitiesToTemperature(TEMPERATURE * unit.kelvin, 4)
    integrator.step(200)
    x = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    f, e = forces_and_energy(context)
    fresh = openmm.Context(system, openmm.VerletIntegrator(0.002))
    fresh.setPositions(x * unit.nanometers)
    f_fresh, e_fresh = forces_and_energy(fresh)
    fmax = np.abs(f_fresh).max()
    moved = np.abs(x - c['x']).max()
    pid = context._engine.pair_force_ids(0)[0]
    print('after 200 steps: atoms moved up to %.3f nm, %d list builds; max|df| = %.2e (bound %.2e), |dE|/|E| = %.2e' %
          (moved, context._engine.ctx.pair_stats(pid)['n_builds'], np.abs(f - f_fresh).max(), 1e-12 * fmax, abs(e - e_fresh) / abs(e_fresh)))
    assert np.isfinite(e) and moved > 0.05
    assert np.abs(x - VR.place(x, *c['table'])).max() <= BOUND_X
    assert np.abs(f - f_fresh).max() <= 1e-12 * fmax
    assert abs(e - e_fresh) <= 1e-12 * abs(e_fresh)


def sites_on_parents(context, table):
    state = context.getState(getPositions=True, getEnergy=True)
    x = state.getPositions(asNumpy=True)._value
    assert np.abs(x - VR.place(x, *table)).max() <= BOUND_X
    energy = state.getPotentialEnergy()._value
    assert np.isfinite(energy)
    return energy


def test_minimiser_starts_from_placed_sites():
    """Flexible water (no constraint pass in front of the search): a minimisation whose sites start off their parents gives the bits
    of one that starts with them placed -- the first energy and gradient are taken at placed sites."""
    c = tip4pew_box()
    system = tip4pew_system(app.CutoffPeriodic, rigid=False)
    site = c['table'][0]
    results = []
    for shift in (0.0, 0.05):
        start = c['x'].copy()
        start[site] += shift
        context = openmm.Context(system, openmm.VerletIntegrator(0.001))
        context.setPositions(start * unit.nanometers)
        info = context._engine.minimize(10.0, 5)
        results.append((context.getState(getPositions=True).getPositions(asNumpy=True)._value, info['energy'], info['evaluations']))
    (xa, ea, na), (xb, eb, nb) = results
    assert np.isfinite(ea) and same_bits(xa, xb) and ea == eb and na == nb
    assert np.abs(xa - VR.place(xa, *c['table'])).max() <= BOUND_X and np.abs(xa - c['x']).max() > 1e-5


def test_drop_in_script_with_four_site_water():
    c = tip4pew_box()
    system = app.ForceField(FIXTURE).createSystem(c['topology'], nonbondedMethod=app.PME, nonbondedCutoff=0.9 * unit.nanometers, rigidWater=True)
    barostat = openmm.MonteCarloBarostat(1 * unit.bar, TEMPERATURE * unit.kelvin, 5)
    barostat.setRandomNumberSeed(1)
    system.addForce(barostat)
    integrator = openmm.LangevinMiddleIntegrator(TEMPERATURE * unit.kelvin, 1 / unit.picosecond, 2 * unit.femtoseconds)
    integrator.setRandomNumberSeed(SEED)
    simulation = app.Simulation(c['topology'], system, integrator)
    simulation.context.setPositions(c['x'] * unit.nanometers)
    e0 = sites_on_parents(simulation.context, c['table'])
    simulation.minimizeEnergy(maxIterations=50)
    e1 = sites_on_parents(simulation.context, c['table'])
    print('minimizeEnergy: %.3f -> %.3f kJ/mol' % (e0, e1))
    assert e1 < e0
    simulation.context.setVelocitiesToTemperature(TEMPERATURE * unit.kelvin, 3)
    for _ in range(4):
        simulation.step(5)
        sites_on_parents(simulation.context, c['table'])
    eng = simulation.context._engine
    assert eng.barostat_stats['attempts'] == 4
    print('barostat: %d of %d attempts accepted' % (eng.barostat_stats['accepted'], eng.barostat_stats['attempts']))
    assert simulation.context.getState().getTime()._value == pytest.approx(0.04, rel=1e-12)


def test_respa_with_flexible_four_site_water():
    c = tip4pew_box()
    system = tip4pew_system(app.PME, rigid=False)
    for force in system.getForces():
        force.setForceGroup(1 if isinstance(force, openmm.NonbondedForce) else 0)
    integrator = atomsmm.MultipleTimeScaleIntegrator(1 * unit.femtoseconds, [4, 1])
    context = openmm.Context(system, integrator)
    context.setPositions(c['x'] * unit.nanometers)
    context.setVelocitiesToTemperature(TEMPERATURE * unit.kelvin, 3)
    e0 = sites_on_parents(context, c['table'])
    for _ in range(5):
        integrator.step(1)
        e1 = sites_on_parents(context, c['table'])
    v = context.getState(getVelocities=True).getVelocities(asNumpy=True)._value
    assert np.all(v[c['table'][0]] == 0.0) and np.all(np.isfinite(v))
    assert e1 != e0
    assert rule_decisions(context) == 0


def test_massless_systems_are_refused_by_name():
    system = tip4pew_system(app.CutoffPeriodic, rigid=False)
    fs, K, ps = unit.femtoseconds, unit.kelvin, unit.picoseconds
    cases = [(atomsmm.NHL_R_Integrator(1 * fs, [1], 300 * K, 10 * fs, 1 / ps), 'Nose-Hoover-Langevin'),
             (atomsmm.SIN_R_Integrator(1 * fs, [1], 300 * K, 10 * fs, 1 / ps), 'isokinetic')]
    regulated = openmm.CustomIntegrator(0.001)
    regulated.addGlobalVariable('kT', KT)
    regulated.addComputePerDof('x', 'x + c*tanh(1.0*v/c)*0.5*dt; c=sqrt(3.0*kT/m)')
    cases.append((regulated, 'regulated'))
    derivative = openmm.CustomIntegrator(0.001)
    derivative.addGlobalVariable('g', 0.0)
    derivative.addComputeGlobal('g', 'deriv(energy, lambda)')
    cases.append((derivative, r'deriv\(energy'))
    inner = atomsmm.MultipleTimeScaleIntegrator(1 * fs, [1])
    cases.append((atomsmm.AdiabaticDynamicsIntegrator(inner, 1, []), 'AdiabaticDynamicsIntegrator'))
    for integrator, text in cases:
        with pytest.raises(InputError, match='massless particles or virtual sites.*' + text):
            openmm.Context(system, integrator)
    with pytest.raises(InputError, match='massless particles or virtual sites.*ComputingSystem'):
        openmm.Context(atomsmm.ComputingSystem(system), openmm.CustomIntegrator(0))
