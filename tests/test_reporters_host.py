"""CPU tests of atomsmm_amd.reporters on a call recorder: exports, headers, column order and text layouts of the five reporters,
and which library calls Engine.energies_at_states makes for a softcore lambda table."""
import io
import subprocess
import sys

import numpy as np
import pytest

import atomsmm_amd
import atomsmm_amd as atomsmm
from atomsmm_amd import engine as E
from atomsmm_amd import openmm, unit
from atomsmm_amd.openmm import app
from atomsmm_amd.testing import system_from_arrays
from fake_backend import RecordingContext



def pandas_or_skip():
    return pytest.importorskip('pandas')


class StatesContext(RecordingContext):
    """The recorder with the multi-state energy entry point: E(lambda_k) = 1000 lambda_k per call."""

    def pair_energy_states(self, fid, pos, lambdas, out):
        self.calls.append(('pair_energy_states', fid, lambdas.tolist()))
        out += 1000.0 * lambdas


@pytest.fixture()
def recorder(monkeypatch):
    made = []

    def factory(*a, **k):
        made.append(StatesContext(*a, **k))
        return made[-1]
    monkeypatch.setattr(E, '_context_factory', factory)
    return made


def test_exports():
    import atomsmm as reference_name
    from atomsmm import ExtendedStateDataReporter  # noqa: F401
    from atomsmm.reporters import ExpandedEnsembleReporter  # noqa: F401
    for name in ('ExtendedStateDataReporter', 'XYZReporter', 'CenterOfMassReporter', 'CustomIntegratorReporter'):
        assert name in atomsmm_amd.__all__ and name in reference_name.__all__
    assert reference_name.reporters is atomsmm_amd.reporters
    # importing the package does not need pandas
    code = 'import sys, atomsmm_amd; assert "pandas" not in sys.modules'
    subprocess.check_call([sys.executable, '-c', code], cwd=str(__import__('pathlib').Path(__file__).resolve().parents[1]))


def heaq_simulation(heaq, integrator=None):
    system = system_from_arrays(heaq, nonbondedMethod='PME', cutoff=1.0, switch=0.9)
    solute = set(int(i) for i in np.where(heaq['resname'] == 'aaa')[0])
    solvation = atomsmm.SolvationSystem(system, solute)
    topology = app.Topology.from_arrays(heaq['atomname'], heaq['resname'])
    integrator = integrator or atomsmm.VelocityVerletPropagator().integrator(1 * unit.femtoseconds)
    simulation = app.Simulation(topology, solvation, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(heaq['positions'] * unit.nanometers)
    simulation.context.setParameter('lambda_vdw', 0.4)
    return simulation


def test_extended_state_data_reporter_columns(heaq, recorder):
    pd = pandas_or_skip()
    simulation = heaq_simulation(heaq)
    table = pd.DataFrame({'lambda_vdw': [0.0, 0.5, 1.0]})
    text = io.StringIO()
    reporter = atomsmm.ExtendedStateDataReporter(text, 2, step=True, potentialEnergy=True, speed=True, globalParameterStates=table,
                                                 globalParameters=['lambda_vdw', 'lambda_coul'])
    simulation.reporters.append(reporter)
    start = len(recorder[0].calls)
    simulation.step(4)
    lines = text.getvalue().splitlines()
    assert lines[0] == ('#"Step","Potential Energy (kJ/mole)","Energy[0] (kJ/mole)","Energy[1] (kJ/mole)","Energy[2] (kJ/mole)",'
                        '"lambda_vdw","lambda_coul","Speed (ns/day)"')
    assert len(lines) == 3
    rows = [line.split(',') for line in lines[1:]]
    assert [int(r[0]) for r in rows] == [2, 4]
    assert all(len(r) == 8 for r in rows)
    eng = simulation.context._engine
    energies = [float(v) for v in rows[-1][2:5]]
    assert energies == pytest.approx(list(eng.energies_at_states(['lambda_vdw'], [[0.0], [0.5], [1.0]])), rel=1e-14)
    # 1000 lambda from the recorder + the long-range correction at lambda: one states launch per report, no reference loop
    assert energies[2] - energies[0] == pytest.approx(1000.0 + (eng.entries[-1].softcore['constant'](dict(eng.parameters, lambda_vdw=1.0))
                                                                - eng.entries[-1].softcore['constant'](dict(eng.parameters, lambda_vdw=0.0))))
    states = [c for c in recorder[0].calls if c[0] == 'pair_energy_states']
    assert len(states) >= 2 and states[0][2] == [0.0, 0.5, 1.0]
    assert not any(c[0] in ('pair_set_lambda', 'pair_set_params') for c in recorder[0].calls[start:])
    assert eng.n_state_fallbacks == 0 and eng.state_paths['states'] >= 2
    assert [float(r[5]) for r in rows] == [0.4, 0.4] and [float(r[6]) for r in rows] == [1.0, 1.0]
    assert simulation.context.getParameter('lambda_vdw') == 0.4


def test_extended_state_data_reporter_extra_file_and_checks(heaq, recorder, tmp_path):
    simulation = heaq_simulation(heaq)
    first, extra = io.StringIO(), tmp_path / 'extra.csv'
    simulation.reporters.append(atomsmm.ExtendedStateDataReporter(first, 1, step=True, extraFile=str(extra), separator=';'))
    simulation.step(2)
    simulation.reporters[0]._out.flush()
    assert first.getvalue() == '#"Step"\n1\n2\n'
    assert extra.read_text() == first.getvalue()
    with pytest.raises(atomsmm.InputError, match='PressureComputer'):
        atomsmm.ExtendedStateDataReporter(io.StringIO(), 1, atomicVirial=True)
    with pytest.raises(NotImplementedError, match='getCollectiveVariableValues'):
        atomsmm.ExtendedStateDataReporter(io.StringIO(), 1, collectiveVariables=[object()])


def test_xyz_and_center_of_mass_layout(spcfw, recorder):
    pandas_or_skip()
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    topology = app.Topology()
    chain = topology.addChain()
    for _ in range(len(spcfw['positions']) // 3):
        residue = topology.addResidue('HOH', chain)
        for name in ('O', 'H1', 'H2'):
            topology.addAtom(name, app._element(name[0]), residue)
    integrator = atomsmm.VelocityVerletPropagator().integrator(1 * unit.femtoseconds)
    simulation = app.Simulation(topology, system, integrator, openmm.Platform.getPlatformByName('HIP'))
    pos = np.array(spcfw['positions'])
    simulation.context.setPositions(pos * unit.nanometers)
    text, cm = io.StringIO(), io.StringIO()
    simulation.reporters += [atomsmm.XYZReporter(text, 1), atomsmm.CenterOfMassReporter(cm, 1, output='positions')]
    simulation.step(1)
    x = simulation.context.getState(getPositions=True).getPositions(asNumpy=True)._value * 10.0
    lines = text.getvalue().splitlines()
    assert lines[0] == str(len(pos))
    assert lines[1] == '\tpositions in angstrom at time step 1\t\t'
    assert lines[2] == 'O\t{}\t{}\t{}'.format(*x[0]) and lines[3].startswith('H\t')
    assert len(lines) == 2 + len(pos)
    mols = cm.getvalue().splitlines()
    assert mols[0] == str(len(pos) // 3) and mols[1] == '\tpositions in angstrom at time step 1\t\t'
    m = np.array([simulation.system.getParticleMass(i)._value for i in range(3)])
    com = (m[:, None] * x[:3]).sum(axis=0) / m.sum()
    assert mols[2].split('\t')[0] == 'HOH'
    assert [float(v) for v in mols[2].split('\t')[1:]] == pytest.approx(list(com), rel=1e-12)
    with pytest.raises(atomsmm.InputError):
        atomsmm.XYZReporter(io.StringIO(), 1, output='accelerations')


def test_custom_integrator_reporter(spcfw, recorder):
    pandas_or_skip()
    system = system_from_arrays(spcfw, nonbondedMethod='CutoffPeriodic')
    integrator = openmm.CustomIntegrator(0.001)
    integrator.addGlobalVariable('kT', 2.5)
    integrator.addPerDofVariable('w', 0.0)
    integrator.addComputePerDof('w', '2*v')
    integrator.addComputePerDof('x', 'x+dt*v')
    simulation = app.Simulation(app.Topology(), system, integrator, openmm.Platform.getPlatformByName('HIP'))
    simulation.context.setPositions(spcfw['positions'] * unit.nanometers)
    text, full = io.StringIO(), io.StringIO()
    simulation.reporters += [atomsmm.CustomIntegratorReporter(text, 1, kT=True, w=True),
                             atomsmm.CustomIntegratorReporter(full, 1, w=True, describeOnly=False)]
    simulation.step(1)
    lines = text.getvalue().splitlines()
    assert lines[:2] == ['kT', '2.5']
    assert lines[2].split() == ['w.x', 'w.y', 'w.z'] and lines[3].split()[0] == 'count'
    table = full.getvalue().splitlines()
    assert table[0] == '\tw.x\tw.y\tw.z' and len(table) == 1 + len(spcfw['positions'])
    with pytest.raises(atomsmm.InputError):
        atomsmm.CustomIntegratorReporter(io.StringIO(), 1)
    simulation.reporters = [atomsmm.CustomIntegratorReporter(io.StringIO(), 1, nope=True)]
    with pytest.raises(atomsmm.InputError, match='Unknown'):
        simulation.step(1)


def test_expanded_ensemble_single_finite_weight(heaq, recorder):
    pd = pandas_or_skip()
    from atomsmm_amd.reporters import ExpandedEnsembleReporter
    simulation = heaq_simulation(heaq)
    states = pd.DataFrame({'lambda_vdw': [0.0, 0.5, 1.0], 'weight': [-np.inf, 0.0, -np.inf]})
    text = io.StringIO()
    reporter = ExpandedEnsembleReporter(text, 1, states, 300 * unit.kelvin)
    simulation.reporters.append(reporter)
    np.random.seed(3)
    simulation.step(5)
    lines = text.getvalue().splitlines()
    assert lines[0] == 'step,state,Energy[0] (kJ/mole),Energy[1] (kJ/mole),Energy[2] (kJ/mole)'
    rows = [line.split(',') for line in lines[1:]]
    assert [int(r[0]) for r in rows] == [1, 2, 3, 4, 5] and {int(r[1]) for r in rows} == {1}
    assert simulation.context.getParameter('lambda_vdw') == 0.5
    assert reporter._walk.visits[0] == reporter._walk.visits[2] == 0
    assert simulation.context._engine.n_state_fallbacks == 0
    walks = reporter.walking_time_analysis(to_file=False)
    assert list(walks.columns) == ['downhill', 'uphill']
    # read_csv accumulates a previous run's reports
    again = ExpandedEnsembleReporter(io.StringIO(), 1, states, 300 * unit.kelvin)
    again.read_csv(io.StringIO(text.getvalue()))
    assert again._reports == 5


def test_expanded_ensemble_prints_the_state_index_between_exchanges(heaq, recorder):
    """reportsPerExchange = 2: the reports without an exchange print the current state's index (-1 before the first exchange when
    the Context's parameters are none of the table's states), and the file reads back."""
    pd = pandas_or_skip()
    from atomsmm_amd.reporters import ExpandedEnsembleReporter
    simulation = heaq_simulation(heaq)                               # lambda_vdw = 0.4: not a state of the table
    states = pd.DataFrame({'lambda_vdw': [0.0, 0.5, 1.0], 'weight': [-np.inf, 0.0, -np.inf]})
    text = io.StringIO()
    simulation.reporters.append(ExpandedEnsembleReporter(text, 1, states, 300 * unit.kelvin, reportsPerExchange=2))
    simulation.step(4)
    rows = [line.split(',') for line in text.getvalue().splitlines()[1:]]
    assert [int(r[1]) for r in rows] == [-1, 1, 1, 1]
    again = ExpandedEnsembleReporter(io.StringIO(), 1, states, 300 * unit.kelvin, reportsPerExchange=2)
    again.read_csv(io.StringIO(text.getvalue()))
    assert again._reports == 4 and list(again._walk.turns) == [2, 4]      # (first = last: every visit turns the walk)


def test_expanded_ensemble_analysis_numbers():
    """read_csv + the analyses on a made-up walk 0 -> 2 -> 0 -> 2 over three states with constant energies, against numbers worked
    out by hand: visits from the report after the first arrival at state 2 on, downhill fractions (0, 1/2, 1), slopes of the
    downhill fraction with n = 2 (ends: 0.3 df1 + 0.2 df2 = 0.35, middle: (1 (f2 - f0) + 2 (f2 - f0)) / 10 = 0.3), and the staging
    of lambda that makes sqrt(df/dlambda) uniform."""
    pd = pandas_or_skip()
    from atomsmm_amd.reporters import ExpandedEnsembleReporter
    lam = [0.0, 0.2, 1.0]
    states = pd.DataFrame({'lambda_vdw': lam})
    E = np.array([-1.0, -2.0, -1.5])
    walk = [0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2]
    lines = ['step,state,Energy[0] (kJ/mole),Energy[1] (kJ/mole),Energy[2] (kJ/mole)']
    lines += ['{},{},{},{},{}'.format(10 * (k + 1), s, *E) for k, s in enumerate(walk)]
    out = io.StringIO()
    reporter = ExpandedEnsembleReporter(out, 10, states, 300 * unit.kelvin)
    reporter.read_csv(io.StringIO('\n'.join(lines) + '\n'))
    assert reporter._reports == len(walk) and reporter._walk.turns == [3, 5, 7, 9, 11]
    assert list(reporter._walk.visits) == [2, 4, 2] and list(reporter._walk.down_visits) == [0, 2, 2]
    beta = 1.0 / (unit.MOLAR_GAS_CONSTANT_R * 300 * unit.kelvin).value_in_unit(unit.kilojoules_per_mole)
    p = np.exp(-beta * E) / np.exp(-beta * E).sum()
    delta = np.array([0.35, 0.3, 0.35])
    frame = reporter.state_sampling_analysis(staging_variable='lambda_vdw')
    assert list(frame.columns) == ['lambda_vdw', 'weight', 'histogram', 'downhill_fraction', 'free_energy', 'isochronal_histogram',
                                   'isochronal_weight', 'staging_lambda_vdw', 'staging_weight']
    assert list(frame['histogram']) == [0.25, 0.5, 0.25] and list(frame['downhill_fraction']) == [0.0, 0.5, 1.0]
    assert np.allclose(frame['free_energy'], beta * (E - E[0]), rtol=1e-12, atol=1e-14)
    assert np.allclose(frame['isochronal_histogram'], np.sqrt(delta * p), rtol=1e-12)
    assert np.allclose(frame['isochronal_weight'], 0.5 * np.log(delta / delta[0]) + 0.5 * beta * (E - E[0]), rtol=1e-12, atol=1e-14)
    # sqrt(df dx) per interval: sqrt(0.5 * 0.2) : sqrt(0.5 * 0.8) = 1 : 2 -> cumulative 0, 1/3, 1; the middle node at 1/2 lands a
    # quarter of the way into the second interval: 0.2 + 0.25 * 0.8 = 0.4, where the free energy is -beta + 0.25 * (beta / 2)
    assert np.allclose(frame['staging_lambda_vdw'], [0.0, 0.4, 1.0], rtol=1e-12, atol=1e-15)
    assert np.allclose(frame['staging_weight'], [0.0, -0.875 * beta, -0.5 * beta], rtol=1e-12, atol=1e-14)
    walks = reporter.walking_time_analysis(history=True)
    assert list(walks['downhill']) == [2, 20.0] and list(walks['uphill']) == [2, 20.0]
    text = out.getvalue()
    assert '# ---------------------------------------- State Sampling Analysis ----------------------------------------' in text
    assert '# ---------- Walking Time History ----------' in text and '# ---------- Walking Time Analysis ----------' in text
