"""GPU tests (run with -m gpu on an MI355X) of a box that changes under a live context: amm_set_box, amm_mol_define / amm_mol_scale
and amm_box_stats through the C-ABI, and Context.setPeriodicBoxVectors through the OpenMM-style surface, against the CPU oracle
evaluated at each box.

Tolerances are the project's: energies rel 1e-10 and forces 1e-9 max|F| against the oracle.  The PME
reciprocal part has no oracle of that accuracy (the explicit k-sum differs from any mesh by the interpolation error), so it is
compared with a fresh context created at the same box with the same mesh: the same arithmetic, only the order of the fixed-point
spread may differ -- rel 1e-12 on the energy, 1e-10 max|F| on the forces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from oracle import oracle as O  # noqa: E402  (checker only)


def _backend():
    from atomsmm_amd import backend as B
    return B


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device='cuda')


def hip_pair(B, ctx, d, c, skin=-1.0):
    desc = B.pair_desc(d.family, d.rc, rc0=d.rc0, rs0=d.rs0, rswitch=d.rswitch, alpha=d.alpha, degree=d.degree,
                       flags=d.flags, sign=d.sign, Kc=d.Kc, krf=d.krf, crf=d.crf)
    return ctx.pair_create(desc, c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'], skin=skin)


def eval_force(ctx, fid, pos_t, n, energy=True):
    f = torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')
    en = torch.zeros(1, dtype=torch.float64, device='cuda') if energy else None
    ctx.force_eval(fid, pos_t, f, accumulate=False, energy=en)
    ctx.check()
    return (en.item() if energy else None), f.cpu().numpy()


def waters(n):
    return [[3 * m, 3 * m + 1, 3 * m + 2] for m in range(n // 3)]


NEAR = O.desc(O.NEAR_FSWITCH, rc=0.7, rc0=0.7, rs0=0.5)
DAMPED = O.desc(O.DAMPED, rc=1.0, rswitch=0.95, alpha=2.9, degree=1)
ALPHA = np.sqrt(-np.log(2 * 5e-4)) / 1.0
EWALD = O.desc(O.NONBONDED, rc=1.0, rswitch=0.9, alpha=ALPHA, flags=O.COULOMB_EWALD | O.SWITCH)
MESH = [24, 25, 27]


# ---------------------------------------------------------------------------------------------------------------- amm_mol_scale
def mixed_molecules():
    """100 single atoms, 341 waters, a 70-atom and a 200-atom molecule whose atoms alternate over the first 140 slots they share."""
    mols = [[i] for i in range(100)] + [[100 + 3 * m + a for a in range(3)] for m in range(341)]
    first = 100 + 3 * 341
    shared = list(range(first, first + 270))
    a = shared[0:140:2]
    b = shared[1:140:2] + shared[140:]
    assert len(a) == 70 and len(b) == 200
    return mols + [a, b], first + 270


def scale_restated(x, mols, scale):
    out = x.copy()
    for m in mols:
        c = x[m].sum(axis=0) / len(m)
        out[m] = x[m] + (np.asarray(scale) - 1.0) * c
    return out


def test_mol_scale_through_the_abi():
    B = _backend()
    mols, n = mixed_molecules()
    rng = np.random.default_rng(11)
    x0 = rng.uniform(-1.0, 4.0, (n, 3))
    scale = (1.01, 0.98, 1.0)
    ref = scale_restated(x0, mols, scale)
    ctx = B.HipContext(n, [3.0, 3.0, 3.0])
    ctx.mol_define(mols)
    runs = []
    for _ in range(2):
        x = dev(x0)
        saved = torch.full((n, 3), float('nan'), dtype=torch.float64, device='cuda')
        ctx.mol_scale(x, scale, saved)
        ctx.synchronize()
        runs.append(x.cpu().numpy())
        assert np.array_equal(saved.cpu().numpy(), x0)                  # the old bits
    assert np.array_equal(runs[0], runs[1])                             # fixed order of summation: the same bits
    spacing = np.spacing(np.abs(x0).max())
    err = np.abs(runs[0] - ref).max()
    print('amm_mol_scale against numpy: %.3g spacings of max|x|' % (err / spacing))
    assert err <= 4 * spacing
    assert np.array_equal(runs[0][:, 2], x0[:, 2])                      # scale 1 on z: nothing moves
    # without a buffer for the old positions
    x = dev(x0)
    ctx.mol_scale(x, scale)
    assert np.array_equal(x.cpu().numpy(), runs[0])
    # a restore: the saved bits copied back
    ctx.copy(x, saved)
    ctx.positions_changed()
    assert np.array_equal(x.cpu().numpy(), x0)
    # every atom exactly once
    with pytest.raises(RuntimeError, match='exactly once'):
        ctx.mol_define(mols[:-1])                                       # 200 atoms in no molecule
    with pytest.raises(RuntimeError, match='appears twice'):
        ctx.mol_define(mols[:-1] + [mols[-1][:-1] + [0]])               # atom 0 twice, the last atom missing
    # the definition that failed replaced nothing
    x = dev(x0)
    ctx.mol_scale(x, scale)
    assert np.array_equal(x.cpu().numpy(), runs[0])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------- box sequence
def oracle_pair(d, pos, box, c):
    e, f, _ = O.pair_eval(d, pos, box, c['charge'], c['sigma'], c['epsilon'], c['exc_pairs'])
    return e, f


def bonded_oracle(c, pos, box):
    eb, fb = O.harmonic_bonds(c['bonds'], c['bond_r0'], c['bond_k'], pos, box)
    ea, fa = O.harmonic_angles(c['angles'], c['angle_theta0'], c['angle_k'], pos, box)
    return eb + ea, fb + fa


def close_to(e, f, e_ref, f_ref, rel=1e-10, frel=1e-9):
    assert e == pytest.approx(e_ref, rel=rel)
    assert np.abs(f - f_ref).max() <= frel * np.abs(f_ref).max()


def test_box_sequence_every_force_matches_the_oracle_at_each_box(spcfw):
    B = _backend()
    c = spcfw
    n = len(c['positions'])
    box0 = np.asarray(c['box'], dtype=np.float64)
    ctx = B.HipContext(n, box0)
    ctx.mol_define(waters(n))
    pairs = {'near': (hip_pair(B, ctx, NEAR, c), NEAR), 'damped': (hip_pair(B, ctx, DAMPED, c), DAMPED),
             'ewald': (hip_pair(B, ctx, EWALD, c), EWALD)}
    pme = ctx.pme_create(ALPHA, MESH, c['charge'])
    excl = ctx.bonded_create()
    qq = c['charge'][c['exc_pairs'][:, 0]] * c['charge'][c['exc_pairs'][:, 1]]
    ctx.bonded_add_terms(excl, B.BOND_EWALD_EXCL, c['exc_pairs'], qq, periodic=True, desc=B.pair_desc(B.NONBONDED, 1.0, alpha=ALPHA))
    ctx.bonded_finalize(excl)
    bonded = ctx.bonded_create()
    ctx.bonded_add_terms(bonded, B.BOND_HARMONIC, c['bonds'], np.stack([c['bond_r0'], c['bond_k']], 1))
    ctx.bonded_add_terms(bonded, B.ANGLE_HARMONIC, c['angles'], np.stack([c['angle_theta0'], c['angle_k']], 1))
    ctx.bonded_finalize(bonded)
    x = dev(c['positions'])

    def everything(x, box, pos):
        """Energy and forces of every force at the context's box, each checked against its reference at that box; returns what the
        context gave and what the references gave."""
        got, refs = {}, {}
        for name, (fid, d) in pairs.items():
            e_ref, f_ref = oracle_pair(d, pos, box, c)
            f_only = eval_force(ctx, fid, x, n, energy=False)[1]        # molecule rows
            assert ctx.pair_stats(fid)['list_kind'] == 1
            e, f = eval_force(ctx, fid, x, n)                           # per-atom rows
            assert ctx.pair_stats(fid)['list_kind'] == 0
            close_to(e, f, e_ref, f_ref)
            assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
            got[name], refs[name] = (e, f), (e_ref, f_ref)
            got[name + ' (molecule rows)'], refs[name + ' (molecule rows)'] = (e, f_only), (e_ref, f_ref)
        refs['excl'] = O.ewald_exclusion(c['exc_pairs'], pos, box, c['charge'], ALPHA)
        got['excl'] = eval_force(ctx, excl, x, n)
        close_to(*got['excl'], *refs['excl'])
        refs['bonded'] = bonded_oracle(c, pos, box)
        got['bonded'] = eval_force(ctx, bonded, x, n)
        close_to(*got['bonded'], *refs['bonded'])
        # reciprocal space: a fresh context at this box with the same mesh
        fresh = B.HipContext(n, box)
        refs['pme'] = eval_force(fresh, fresh.pme_create(ALPHA, MESH, c['charge']), x, n)
        fresh.close()
        got['pme'] = eval_force(ctx, pme, x, n)
        close_to(*got['pme'], *refs['pme'], rel=1e-12, frel=1e-10)
        return got, refs

    visits, cells, first, factor = [1.0, 1.12, 0.97, 1.0], [], None, 1.0
    for s in visits:
        box = box0 * s
        if s != factor:
            ctx.set_box(box)
            ctx.mol_scale(x, [s / factor] * 3)
            factor = s
        got, refs = everything(x, box, x.cpu().numpy())
        cells.append(ctx.pair_stats(pairs['damped'][0])['n_cells'])
        if first is None:
            first, first_refs = got, refs
    # Back at the first box through three scalings: the last visit reproduces the first to 1e-12 (energy: relative; forces: of
    # max|F|).  The positions are not the first visit's bits -- every scaling rounds them to the spacing of a coordinate, up to
    # 4.4e-16 nm -- so where the REFERENCE itself (the oracle; for reciprocal space the fresh context, whose fixed-point spread
    # rounds every charge share to its grid) moves by more than a tenth of 1e-12 between the two position sets, the bound is ten
    # times that reference-against-reference difference instead.  Measured in the context: every force within 1e-13 except the
    # reciprocal-space forces, 2.4e-12 max|F|; the figures of both sides are printed below.
    for name in first:
        scale_e, scale_f = abs(first[name][0]), np.abs(first[name][1]).max()
        ref_de = abs(refs[name][0] - first_refs[name][0]) / scale_e
        ref_df = np.abs(refs[name][1] - first_refs[name][1]).max() / scale_f
        bound_e = 1e-12 if ref_de <= 1e-13 else 10.0 * ref_de
        bound_f = 1e-12 if ref_df <= 1e-13 else 10.0 * ref_df
        de = abs(got[name][0] - first[name][0]) / scale_e
        df = np.abs(got[name][1] - first[name][1]).max() / scale_f
        print('%-24s back at the first box: dE/E %.2e (references %.2e, bound %.1e), dF/max|F| %.2e (references %.2e, bound %.1e)' % (
            name, de, ref_de, bound_e, df, ref_df, bound_f))
        assert de <= bound_e and df <= bound_f, name
    # ... and at the first visit's position bits nothing but the order of summation can differ
    x.copy_(dev(c['positions']))
    again, _ = everything(x, box0, c['positions'])
    for name in first:
        close_to(*again[name], *first[name], rel=1e-12, frel=1e-12)
    # 4 cells per axis (every cell in one pass) at 2.5 nm, 5 at 2.8 nm; some change alters the count and some change keeps it
    assert cells[0] == 64 and cells[1] == 125
    changes = [a != b for a, b in zip(cells, cells[1:])]
    assert any(changes) and not all(changes)
    st = ctx.box_stats()
    assert st['changes'] == 3 and 1 <= st['regrids'] <= 3
    ctx.close()


def test_clamped_buffer_follows_the_box_and_a_box_too_small_is_refused(spcfw):
    B = _backend()
    c = spcfw
    n = len(c['positions'])
    box0 = np.asarray(c['box'], dtype=np.float64)
    d = O.desc(O.DAMPED, rc=1.2, rswitch=1.15, alpha=2.9, degree=1)      # buffer clamped to 0.999 (L/2 - rc) = 0.05 nm from the start
    ctx = B.HipContext(n, box0)
    ctx.mol_define(waters(n))
    fid = hip_pair(B, ctx, d, c)
    x = dev(c['positions'])
    close_to(*eval_force(ctx, fid, x, n), *oracle_pair(d, c['positions'], box0, c))
    assert ctx.pair_stats(fid)['rlist'] == pytest.approx(1.2 + 0.999 * 0.05, abs=1e-12)
    box = 0.99 * box0
    ctx.set_box(box)
    ctx.mol_scale(x, [0.99] * 3)
    pos = x.cpu().numpy()
    e_ref, f_ref = oracle_pair(d, pos, box, c)
    close_to(*eval_force(ctx, fid, x, n), e_ref, f_ref)
    assert ctx.pair_stats(fid)['rlist'] == pytest.approx(1.2 + 0.999 * (0.5 * box[0] - 1.2), abs=1e-12)
    f_only = eval_force(ctx, fid, x, n, energy=False)[1]
    assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
    with pytest.raises(RuntimeError, match='pair cutoff exceeds half the box edge'):
        ctx.set_box([2.39, box[1], box[2]])
    assert ctx.box_stats()['changes'] == 1
    close_to(*eval_force(ctx, fid, x, n), e_ref, f_ref)                 # the old box is still in force
    f_only = eval_force(ctx, fid, x, n, energy=False)[1]
    assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
    ctx.close()


def test_dual_list_across_box_changes_that_take_its_outer_buffer_away_and_give_it_back(spcfw):
    """A force made with an outer Verlet buffer of 0.2 nm (a cell-built outer list pruned to the traversed one).  At 2.5 and 2.3 nm
    the clamp 0.999 (L/2 - rc) leaves an outer buffer above the inner 0.1 nm; at 2.18 nm it leaves 0.09 nm for both, the list
    becomes a single one, and back at 2.5 nm a dual one again: every visit against the oracle at that box."""
    B = _backend()
    c = spcfw
    n = len(c['positions'])
    box0 = np.asarray(c['box'], dtype=np.float64)
    ctx = B.HipContext(n, box0)
    ctx.set_outer_skin(0.2)
    ctx.mol_define(waters(n))
    fid = hip_pair(B, ctx, DAMPED, c)
    x = dev(c['positions'])
    factor, kinds = 1.0, []
    for s in (1.0, 0.92, 0.872, 1.0):
        box = box0 * s
        if s != factor:
            ctx.set_box(box)
            ctx.mol_scale(x, [s / factor] * 3)
            factor = s
        e_ref, f_ref = oracle_pair(DAMPED, x.cpu().numpy(), box, c)
        close_to(*eval_force(ctx, fid, x, n), e_ref, f_ref)
        f_only = eval_force(ctx, fid, x, n, energy=False)[1]
        assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
        st = ctx.pair_stats(fid)
        clamp = 0.999 * (0.5 * box[0] - 1.0)
        assert st['rlist'] == pytest.approx(1.0 + min(0.1, clamp), abs=1e-12)
        assert st['rlist_outer'] == pytest.approx(1.0 + max(min(0.1, clamp), min(0.2, clamp)), abs=1e-12)
        kinds.append(st['rlist_outer'] > st['rlist'] + 1e-9)
    assert kinds == [True, True, False, True]
    assert ctx.box_stats()['regrids'] >= 2                 # at least the two changes of kind
    ctx.close()


def test_compression_in_small_steps_never_overflows(spcfw):
    B = _backend()
    c = spcfw
    n = len(c['positions'])
    box = np.asarray(c['box'], dtype=np.float64).copy()
    ctx = B.HipContext(n, box)
    ctx.mol_define(waters(n))
    fids = [(hip_pair(B, ctx, NEAR, c), NEAR), (hip_pair(B, ctx, DAMPED, c), DAMPED)]
    x = dev(c['positions'])
    for fid, d in fids:
        eval_force(ctx, fid, x, n)
        eval_force(ctx, fid, x, n, energy=False)
    s = 0.99 ** (1.0 / 3.0)
    regrid_box, stats = box.copy(), ctx.box_stats()
    for step in range(12):
        box = box * s
        ctx.set_box(box)
        ctx.mol_scale(x, [s] * 3)
        now = ctx.box_stats()
        if now['regrids'] > stats['regrids']:
            regrid_box = box.copy()
        elif np.all(np.abs(box - regrid_box) <= 0.02 * regrid_box):
            assert now['waits'] == stats['waits'], 'step %d: a change within 2 %% of the last regrid waited or allocated' % step
        stats = now
        pos = x.cpu().numpy()
        for fid, d in fids:
            e_ref, f_ref = oracle_pair(d, pos, box, c)
            close_to(*eval_force(ctx, fid, x, n), e_ref, f_ref)         # (eval_force calls amm_check: no overflow)
            f_only = eval_force(ctx, fid, x, n, energy=False)[1]
            assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
    print('twelve 1 % compressions:', stats)
    assert stats['changes'] == 12
    ctx.close()


# ---------------------------------------------------------------------------------------------- through the Context
def scale_molecules(x, molecules, s):
    """Every molecule moved rigidly so that its centre (the unweighted mean of its atoms) is scaled by s."""
    out = x.copy()
    for m in molecules:
        out[m] = x[m] + (s - 1.0) * x[m].mean(axis=0)
    return out


def respa_water_context(c, loops):
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.testing import system_from_arrays
    system = system_from_arrays(c, nonbondedMethod='CutoffPeriodic')
    respa = atomsmm.RESPASystem(system, 0.7 * unit.nanometers, 0.5 * unit.nanometers)
    nb = atomsmm.hijackForce(respa, atomsmm.findNonbondedForce(respa))
    outer = atomsmm.DampedSmoothedForce(2.9 / unit.nanometers, 1.0 * unit.nanometers, 0.9 * unit.nanometers).importFrom(nb)
    outer.setForceGroup(2)
    outer.addTo(respa)
    integrator = atomsmm.RespaPropagator(loops).integrator(1 * unit.femtoseconds)
    context = openmm.Context(respa, integrator, openmm.Platform.getPlatformByName('HIP'))
    context.setPositions(c['positions'] * unit.nanometers)
    context.setVelocities(c['velocities'])
    return context, integrator


def test_molecule_rows_and_fused_epilogue_across_a_box_change():
    """1000 flexible waters under RESPA [4, 2, 1]: two steps, the box shrunk by 12 % in edge with the molecules scaled along (through
    setPeriodicBoxVectors and setPositions), two more steps -- against the oracle's RESPA driven the same way, at the bounds of
    tests/test_gpu_minimize.py::test_hand_over_to_dynamics.  The factor takes the list from one periodic image per molecule pair
    (rc + skin + 2 rext < L / 2, cluster_setup_grid) to one per atom pair; the launches that carry the inner loop as their epilogue
    -- and write the next evaluation's sorted copies and cells ahead of time -- must go on after the change, on fresh lists."""
    from atomsmm_amd.testing import tip3p_box
    from oracle.respa_cpu import RespaCPU
    c = tip3p_box(10)
    s = 0.88
    ext = np.linalg.norm(c['positions'].reshape(-1, 3, 3)[:, 1:] - c['positions'].reshape(-1, 3, 3)[:, :1], axis=2).max()
    rext = max(1.5 * ext, ext + 0.05)                       # (cluster_first_build)
    assert 1.0 + 0.1 + 2.0 * rext < 0.5 * c['box'][0] and not 1.0 + 0.1 + 2.0 * (rext - 0.01) < 0.5 * s * c['box'][0]
    context, integrator = respa_water_context(c, [4, 2, 1])
    eng = context._engine
    cpu = RespaCPU(dict(c), dt=0.001)
    integrator.step(2)
    cpu.step(2)
    epilogues = eng.ctx.run_stats()['epilogues']
    assert epilogues > 0
    state = context.getState(getPositions=True)
    molecules = context.getMolecules()
    assert len(molecules) == 1000
    x = scale_molecules(state.getPositions(asNumpy=True)._value, molecules, s)
    box = s * c['box']
    context.setPeriodicBoxVectors((box[0], 0, 0), (0, box[1], 0), (0, 0, box[2]))
    context.setPositions(x)
    cpu.c['box'] = box
    cpu.x[...] = scale_molecules(cpu.x, molecules, s)
    cpu.F.clear()
    integrator.step(2)
    cpu.step(2)
    state = context.getState(getPositions=True, getVelocities=True)
    dx = np.abs(state.getPositions(asNumpy=True)._value - cpu.x).max()
    dv = np.abs(state.getVelocities(asNumpy=True)._value - cpu.v).max()
    print('RESPA across a box change: max|dx| %.2e nm, max|dv| %.2e nm/ps' % (dx, dv))
    assert dx < 1e-10 and dv < 1e-9
    assert [tuple(v._value) for v in state.getPeriodicBoxVectors()] == [(box[0], 0, 0), (0, box[1], 0), (0, 0, box[2])]
    for g in (1, 2):
        for pid in eng.pair_force_ids(g):
            assert eng.ctx.pair_stats(pid)['list_kind'] == 1
    assert eng.ctx.run_stats()['epilogues'] > epilogues
    assert eng.ctx.box_stats()['changes'] == 1


def test_hybrid_list_and_list_free_group_force_across_a_box_change():
    """The smallest solvated chain (waters + a 300-atom chain + a 30-atom solute coupled through a softcore interaction group):
    hybrid lists for the near and the outer force, no list at all for the solute's force.  Two RESPA steps (the fused inner loop
    keeps the group force's candidate set), a box 3 % larger with every molecule scaled along, then every group's energy and forces
    against the oracle at that box -- group 0's energy holds the softcore long-range correction, which goes with 1 / V -- and two
    more steps against the oracle's."""
    import atomsmm_amd as atomsmm
    from atomsmm_amd import openmm, unit
    from atomsmm_amd.testing import build_c5_system, solvated_chain
    from oracle.afed_cpu import AfedCPU
    case = solvated_chain(nside=12, n_chain=300, n_solute=30)
    respa = build_c5_system(case)
    integrator = atomsmm.RespaPropagator([2, 2, 1]).integrator(1 * unit.femtoseconds)
    context = openmm.Context(respa, integrator)
    eng = context._engine
    eng.ctx.set_option('group_candidates', 1)
    context.setPositions(case['positions'] * unit.nanometers)
    context.setVelocities(case['velocities'])
    context.setParameter('lambda_vdw', 0.8)
    integrator.step(2)
    state = context.getState(getPositions=True, getVelocities=True)
    s = 1.03
    molecules = context.getMolecules()
    assert len(molecules) == case['n_waters'] + 2
    x = scale_molecules(state.getPositions(asNumpy=True)._value, molecules, s)
    box = s * case['box']
    context.setPeriodicBoxVectors((box[0], 0, 0), (0, box[1], 0), (0, 0, box[2]))
    context.setPositions(x)
    moved = dict(case, box=box, positions=x, velocities=state.getVelocities(asNumpy=True)._value)
    ref = AfedCPU(moved, loops=(2, 2, 1), dt=0.001, lam=0.8)
    lrc = O.softcore_lrc(case['sigma'], case['epsilon'], ref.codes, box, 1.0, 0.9, 0.8)
    n_rest = len(case['chain']) + len(case['solute'])
    # group 0 is a sum of five forces, some of them large and of either sign: the project's bound of rel 1e-10 per force is taken
    # on the sum of their magnitudes, not on what is left of them.  Its constant, the softcore long-range correction, is a
    # quadrature on either side (the engine's and the oracle's agree to 3.3e-7 at any box; tests/test_gpu_c5.py allows 2e-6 for
    # such numbers): it is checked on its own -- against the oracle at that bound, and against 1 / V exactly.
    entry = [e for e in eng.entries if e.softcore is not None][0]
    assert entry.constant == pytest.approx(lrc, rel=2e-6)
    at_creation = O.softcore_lrc(case['sigma'], case['epsilon'], ref.codes, case['box'], 1.0, 0.9, 0.8)
    assert entry.constant / at_creation == pytest.approx(lrc / at_creation, rel=2e-6) and lrc / at_creation == pytest.approx(s ** -3, rel=1e-12)
    parts = [O.harmonic_bonds(case['bonds'], case['bond_r0'], case['bond_k'], x, box, want_forces=False)[0],
             O.harmonic_angles(case['angles'], case['angle_theta0'], case['angle_k'], x, box, want_forces=False)[0],
             O.periodic_torsions(case['torsions'], case['torsion_n'], case['torsion_phase'], case['torsion_k'], x, box, want_forces=False)[0],
             O.ljc_bonds(ref.ex_pairs, ref.ex_qq, ref.ex_sig, ref.ex_eps, x, box, want_forces=False)[0],
             ref.softcore(0.8, want_forces=False)[0]]
    for g in (0, 1, 2):
        st = context.getState(getForces=True, getEnergy=True, groups={g})
        e_ref, f_ref = ref.group_energy_forces(g)
        if g == 0:
            assert sum(parts) == pytest.approx(e_ref, rel=1e-12)
            scale = sum(abs(p) for p in parts)
            got = st.getPotentialEnergy()._value - entry.constant
            print('group 0 without its constant: E = %.9f, oracle %.9f, sum of |terms| %.3f' % (got, e_ref, scale))
            assert abs(got - e_ref) <= 1e-10 * scale
        else:
            assert st.getPotentialEnergy()._value == pytest.approx(e_ref, rel=1e-10)
        assert np.abs(st.getForces(asNumpy=True)._value - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
        f_only = context.getState(getForces=True, groups={g}).getForces(asNumpy=True)._value        # the kernels the step program runs
        assert np.abs(f_only - f_ref).max() <= 1e-9 * np.abs(f_ref).max()
        for pid in eng.pair_force_ids(g) if g else []:
            stats = eng.ctx.pair_stats(pid)
            assert stats['list_kind'] == 2 and stats['n_rest_atoms'] == n_rest, stats
    softcore = [e for e in eng.entries if e.softcore is not None][0].softcore['pid']
    assert eng.ctx.pair_stats(softcore)['list_kind'] == 3
    # deriv(energy, lambda_vdw) holds the correction's lambda-derivative, another 1 / V number (the bound of tests/test_gpu_c5.py)
    assert eng.energy_derivative('lambda_vdw') == pytest.approx(ref.dE_dlambda(), rel=2e-6)
    integrator.step(2)
    ref.respa(0.001)
    ref.respa(0.001)
    xs = context.getState(getPositions=True).getPositions(asNumpy=True)._value
    print('hybrid list across a box change: max|dx| %.2e nm' % np.abs(xs - ref.x).max())
    assert np.abs(xs - ref.x).max() < 1e-9                   # (the bound of tests/test_gpu_c5.py for this system)
