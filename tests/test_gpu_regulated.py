"""GPU tests of regulated dynamics (propagators.py:1537-2117 of the reference): the regulated move of a context in regulated mode
(amm_regulated_define) and the regulated Nose-Hoover-Langevin bath ops (amm_bath_define_regulated, kinds 3..6) against numpy
restatements of the reference's expressions on the same Philox stream; the one-launch inner loop against the op-by-op execution;
the epilogue guard; the kinetic-energy expression; and the physics of a run at a long outer step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import atomsmm_amd as atomsmm  # noqa: E402
from atomsmm_amd import backend as B  # noqa: E402
from atomsmm_amd import openmm, unit  # noqa: E402
from atomsmm_amd.testing import lj_fluid, system_from_arrays, tip3p_box  # noqa: E402
from oracle import expr_oracle as XO  # noqa: E402  (checker only)

KB = unit.BOLTZMANN_CONSTANT_kB._value
T, TAU, GAMMA = 300 * unit.kelvin, 10 * unit.femtoseconds, 10 / unit.picoseconds
BATHS = {3: atomsmm.RegulatedMassiveNoseHooverLangevinPropagator, 4: atomsmm.TwiceRegulatedMassiveNoseHooverLangevinPropagator,
         5: atomsmm.RegulatedAtomicNoseHooverLangevinPropagator, 6: atomsmm.TwiceRegulatedAtomicNoseHooverLangevinPropagator}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def gaussians(n, seed, counter):
    u1, u2 = XO.uniforms(3 * n, 0, seed, (1 << 63) | counter)
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586476925 * u2)).reshape(n, 3)


def test_regulated_move_vs_numpy():
    """MOVE in regulated mode: x + c tanh(alpha v/c) coef, c = sqrt(alpha n kT/m), against numpy of the reference's expression to
    1e-13 relative; |dx| <= c |coef| everywhere, saturated velocities (|alpha v/c| >> 1) included, and finite.  The kick + move
    launch (k_kicks_move_atoms) is bit-identical to the op-by-op execution."""
    rng = np.random.default_rng(3)
    n = 3000
    alpha, an_kT, coef = 1.5, 1.5 * 4 * 2.494, 0.000125
    mass = rng.choice([1.008, 15.9994, 39.948], n)
    v0 = rng.normal(0, 1.0, (n, 3)) * np.sqrt(2.494 / mass)[:, None]
    v0[:50] *= 1e4                                       # saturated
    x0, f0 = rng.uniform(0, 3, (n, 3)), rng.normal(0, 300, (n, 3))
    out = []
    for fuse in (True, False):
        ctx = B.HipContext(n, np.array([3.0, 3.0, 3.0]))
        ctx.set_fuse_inner(fuse)
        x, v, f = dev(x0), dev(v0), dev(f0)
        ctx.bind_state(x, v, dev(mass))
        ctx.bind_buffer(0, f)
        ctx.regulated_define(True, alpha, an_kT)
        ctx.run_ops([B.Op(B.OP_MOVE, 0, 0, 0, coef)], 1)
        ctx.check()
        xg = x.cpu().numpy()
        dx = xg - x0
        c = np.sqrt(an_kT / mass)[:, None]
        ref = c * np.tanh(alpha * v0 / c) * coef
        rounding = 2.0 * np.finfo(np.float64).eps * np.abs(x0)          # (of x itself: dx is read back as a difference)
        assert np.isfinite(xg).all()
        assert (np.abs(xg - (x0 + ref)) <= 1e-13 * np.abs(ref) + rounding).all()
        sat = np.abs(alpha * v0 / c) > 40.0                                # tanh = +-1 in double precision
        assert sat.sum() > 100 and (np.abs(np.abs(dx) - c * coef)[sat] <= rounding[sat]).all()
        assert (np.abs(dx) <= c * coef + rounding).all()
        ctx.run_ops([B.Op(B.OP_KICK, 0, -1, 0, 0.5 * coef), B.Op(B.OP_MOVE, 0, 0, 0, coef)], 1)
        ctx.check()
        out.append((x.cpu().numpy(), v.cpu().numpy()))
        ctx.regulated_define(False)
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def reference_bath(kind, split, v, w, m, g, h, z, kT, Q, omega, friction, alpha, an):
    """One regulated bath block in numpy, written from the reference's expressions (propagators.py:1598-2007)."""
    v, w = v.copy(), w.copy()
    c = np.sqrt(an * kT / m)[:, None]
    n = an / alpha
    kfac = (n + 1) / (alpha * n)

    def drive(v):
        if kind == 3:
            return (m[:, None] * v * c * np.tanh(alpha * v / c) - kT) / Q
        if kind == 4:
            return (kfac * m[:, None] * (c * np.tanh(alpha * v / c)) ** 2 - kT) / Q
        y = np.tanh(alpha * v / c)
        d = np.sum(m[:, None] * v * c * y, axis=1) if kind == 5 else kfac * np.sum(m[:, None] * c * y * c * y, axis=1)
        return np.repeat(((d - 3 * kT) / Q)[:, None], 3, axis=1)

    def scale(v):
        if kind in (3, 5):
            return v * np.exp(-w * h)
        zz = np.sinh(alpha * v / c) * np.exp(-w * h)
        za = np.abs(zz)
        return (1 / alpha) * c * np.sign(zz) * np.log(np.where(za >= 1e8, 2 * za, za + np.sqrt(1 + zz * zz)))
    noise = np.repeat(g[:, :1], 3, axis=1) if kind >= 5 else g
    if split:
        w = w + drive(v) * h
    v = scale(v)
    w = w * z + omega * np.sqrt(1 - z ** 2) * noise + (0.0 if split else drive(v) * (1 - z) / friction)
    v = scale(v)
    if split:
        w = w + drive(v) * h
    return v, w


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('kind', [3, 4, 5, 6])
def test_regulated_bath_op_vs_numpy(kind, split):
    """Each regulated bath kind, with and without `split`, two ops in a row, against numpy on the same Philox stream: 1e-12 relative;
    in the atomic kinds the three components of v_eta stay equal."""
    rng = np.random.default_rng(kind + 10 * split)
    n = 2000
    ctx = B.HipContext(n, np.array([3.0, 3.0, 3.0]))
    mass = rng.choice([1.008, 15.9994], n)
    kT, alpha, an = 2.494, 2.0, 6.0
    v0 = rng.normal(0, 1.0, (n, 3)) * np.sqrt(kT / mass)[:, None]
    w0 = rng.normal(0, 50.0, (n, 3))
    if kind >= 5:
        w0[:, 1] = w0[:, 2] = w0[:, 0]
    x, v, w = dev(rng.uniform(0, 3, (n, 3))), dev(v0), dev(w0)
    ctx.bind_state(x, v, dev(mass))
    ctx.bind_buffer(5, w)
    h, friction = 0.00025, 10.0
    Q = (3 if kind >= 5 else 1) * kT * 0.01 ** 2
    omega = np.sqrt(kT / Q) if kind >= 5 else 100.0
    z = float(np.exp(-friction * 2 * h))
    bid = ctx.bath_define_regulated(kind, split, h, z, kT, Q, omega, friction, alpha, an, 5)
    ctx.expr_seed(4242)
    ctx.run_ops([B.Op(B.OP_BATH, bid, B.SLOT_V, 0, 0.0)] * 2, 1)
    ctx.check()
    rv, rw = v0, w0
    for k in (1, 2):
        rv, rw = reference_bath(kind, split, rv, rw, mass, gaussians(n, 4242, k), h, z, kT, Q, omega, friction, alpha, an)
    gv, gw = v.cpu().numpy(), w.cpu().numpy()
    assert np.abs(gv - rv).max() <= 1e-12 * np.abs(rv).max()
    assert np.abs(gw - rw).max() <= 1e-12 * np.abs(rw).max()
    if kind >= 5:
        assert np.array_equal(gw[:, 0], gw[:, 1]) and np.array_equal(gw[:, 0], gw[:, 2])
    ctx.close()


def _water_system(c):
    system = system_from_arrays(c, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 7 * unit.angstroms, 5 * unit.angstroms)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    outer = atomsmm.DampedSmoothedForce(0.29 / unit.angstroms, 10 * unit.angstroms, 9 * unit.angstroms).importFrom(nb)
    outer.setForceGroup(2)
    outer.addTo(respa)
    return respa


def _regulated_integrator(bath, dt_fs, loops=(4, 2, 1), n=2, move=None, scheme='middle'):
    move = move or atomsmm.RegulatedTranslationPropagator(T, n)
    integrator = atomsmm.MultipleTimeScaleIntegrator(dt_fs * unit.femtoseconds, list(loops), move=move,
                                                     boost=atomsmm.RegulatedBoostPropagator(), bath=bath, scheme=scheme)
    integrator.setRandomNumberSeed(99)
    return integrator


def _run(system, c, integrator, steps, fuse=True):
    context = openmm.Context(system, integrator)
    context._engine.ctx.set_fuse_inner(fuse)
    context.setPositions(c['positions'] * unit.nanometers)
    context.setVelocitiesToTemperature(300 * unit.kelvin, 3)
    integrator.step(steps)
    st = context.getState(getPositions=True, getVelocities=True)
    return context, st.getPositions(asNumpy=True)._value.copy(), st.getVelocities(asNumpy=True)._value.copy()


@pytest.mark.parametrize('split', [False, True])
@pytest.mark.parametrize('kind', [3, 4, 5, 6])
def test_regulated_inner_loop_kernel_is_bit_identical(spcfw, kind, split):
    """spcfw under RESPASystem, RESPA [4,2,1] with each regulated bath in the innermost loop: the one-launch inner loop (regulated
    moves + bath between them) and the op-by-op execution give bit-identical positions, velocities and v_eta after 12 steps; the
    program is compiled (no general path) and holds no EXPR op."""
    out = []
    for fuse in (True, False):
        integrator = _regulated_integrator(BATHS[kind](T, 2, TAU, GAMMA, split=split), 2.0)
        context, x, v = _run(_water_system(spcfw), spcfw, integrator, 12, fuse)
        eng = context._engine
        assert eng._interpreted is False
        assert all(B.OP_EXPR not in {o.op for o in prog[0]} for prog in eng._programs.values())
        w = np.array([list(row) for row in integrator.getPerDofVariableByName('v_eta')])
        out.append((x, v, w))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][2]).max() > 0
    if kind >= 5:
        assert np.array_equal(out[0][2][:, 0], out[0][2][:, 1]) and np.array_equal(out[0][2][:, 0], out[0][2][:, 2])


def test_epilogue_guard_water_xo_respa():
    """scheme='xo-respa' leaves the innermost loop bathless, which the fused epilogue of the pair-force launch (cepi_rows) would
    carry with plain moves: in regulated mode it is not planned, and the trajectory equals the fuse-off one bit for bit; the same
    program with TranslationPropagator still runs epilogues."""
    c = tip3p_box(8)
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA)
    runs = [_run(_water_system(c), c, _regulated_integrator(bath, 2.0, scheme='xo-respa'), 6, fuse) for fuse in (True, False)]
    assert runs[0][0]._engine.ctx.run_stats()['epilogues'] == 0
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    plain = _regulated_integrator(bath, 2.0, scheme='xo-respa', move=atomsmm.TranslationPropagator(constrained=False))
    context, _, _ = _run(_water_system(c), c, plain, 6)
    assert context._engine.ctx.run_stats()['epilogues'] > 0


def test_epilogue_guard_lj_fluid_per_atom_rows():
    """The per-atom-row epilogue of a chargeless pair force (velocity-Verlet shape, one force group): not planned in regulated mode,
    bit-identical to the fuse-off trajectory; planned for the same program with plain moves."""
    c = lj_fluid(12)
    rc, rs = 2.5 * 0.34, 0.9 * 2.5 * 0.34

    def system():
        s = system_from_arrays(c, nonbondedMethod='CutoffPeriodic', cutoff=rc)
        nb = atomsmm.hijackForce(s, atomsmm.findNonbondedForce(s))
        atomsmm.NearNonbondedForce(rc * unit.nanometers, rs * unit.nanometers, 'force-switch').importFrom(nb).addTo(s)
        return s
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA)
    runs = [_run(system(), c, _regulated_integrator(bath, 4.0, loops=(1,), scheme='xo-respa'), 6, fuse) for fuse in (True, False)]
    assert runs[0][0]._engine.ctx.run_stats()['epilogues'] == 0
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    plain = _regulated_integrator(bath, 4.0, loops=(1,), scheme='xo-respa', move=atomsmm.TranslationPropagator(constrained=False))
    context, _, _ = _run(system(), c, plain, 6)
    assert context._engine.ctx.run_stats()['epilogues'] > 0


def test_kinetic_energy_expression(spcfw):
    n, alpha = 3, 1.5
    bath = atomsmm.TwiceRegulatedMassiveNoseHooverLangevinPropagator(T, n, TAU, GAMMA, alpha_n=alpha)
    integrator = _regulated_integrator(bath, 2.0, move=atomsmm.RegulatedTranslationPropagator(T, n, alpha_n=alpha))
    context, _, v = _run(_water_system(spcfw), spcfw, integrator, 3)
    ke = context.getState(getEnergy=True).getKineticEnergy()._value
    kT = KB * 300.0
    m = spcfw['mass'][:, None]
    c = np.sqrt(alpha * n * kT / m)
    ref = np.sum(0.5 * m * (c * np.tanh(alpha * v / c)) ** 2)
    assert abs(ke - ref) <= 1e-12 * ref
    assert abs(ke - np.sum(0.5 * m * v * v)) > 1e-6 * ref           # (not the plain m v^2 / 2)


def test_regulated_physics_at_a_long_outer_step(spcfw):
    """Regulated massive NHL, RESPA [4,2,1] at a 6 fs outer step (three times the RESPA tests of test_gpu_thermostats.py): 300 steps
    stay finite; no degree of freedom moves farther per step than its speed limit c_i dt (minimum image); after equilibration the
    mean of m v c tanh(alpha v/c) over all DOFs -- the regulated equipartition <p dH/dp> = kT -- is near kT (measured: 0.956 kT; the
    tolerance of 7 % allows for the time-step bias at this step and the sampling noise of 150 samples)."""
    n, dt = 2, 0.006
    bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, n, TAU, 20 / unit.picoseconds)
    integrator = _regulated_integrator(bath, 1000 * dt)
    context, x, v = _run(_water_system(spcfw), spcfw, integrator, 100)
    assert context._engine._interpreted is False
    kT = KB * 300.0
    m = spcfw['mass'][:, None]
    c = np.sqrt(n * kT / m)
    box = spcfw['box']
    samples = []
    for _ in range(200):
        integrator.step(1)
        st = context.getState(getPositions=True, getVelocities=True)
        x1, v = st.getPositions(asNumpy=True)._value, st.getVelocities(asNumpy=True)._value
        d = x1 - x
        d -= box * np.round(d / box)
        assert np.isfinite(x1).all() and (np.abs(d) <= c * dt * (1 + 1e-9)).all()
        x = x1
        samples.append(np.mean(m * v * c * np.tanh(v / c)))
    ratio = np.mean(samples[50:]) / kT
    print('regulated equipartition <m v c tanh(v/c)> / kT = %.4f' % ratio)
    assert abs(ratio - 1) < 0.07, ratio


@pytest.mark.parametrize('variant', ['adiabatic', 'global'])
def test_general_path_variants_run(spcfw, variant):
    if variant == 'adiabatic':
        bath = atomsmm.RegulatedMassiveNoseHooverLangevinPropagator(T, 2, TAU, GAMMA, adiabatic=True)
    else:
        bath = atomsmm.TwiceRegulatedGlobalNoseHooverLangevinPropagator(3 * len(spcfw['mass']), T, 2, TAU, GAMMA)
    integrator = _regulated_integrator(bath, 2.0)
    context = openmm.Context(_water_system(spcfw), integrator)
    if variant == 'adiabatic':
        context._engine.fill_per_dof('kT', KB * 300.0)
    context.setPositions(spcfw['positions'] * unit.nanometers)
    context.setVelocitiesToTemperature(300 * unit.kelvin, 3)
    integrator.step(10)
    st = context.getState(getPositions=True, getVelocities=True)
    x, v = st.getPositions(asNumpy=True)._value, st.getVelocities(asNumpy=True)._value
    assert np.isfinite(x).all() and np.isfinite(v).all() and np.abs(x - spcfw['positions']).max() > 1e-4
    if variant == 'global':
        assert context._engine._interpreted is True and np.isfinite(integrator.getGlobalVariableByName('v_eta'))
