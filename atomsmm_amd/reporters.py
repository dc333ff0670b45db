"""Reporters with the interface of `atomsmm.reporters`, served by app.Simulation's reporter protocol (describeNextReport / report):

* ExtendedStateDataReporter -- app.StateDataReporter plus virials and pressures (PressureComputer), energies at many states of
  global parameters (Engine.energies_at_states: one launch for all the lambdas of a softcore force), parameter values and
  energy derivatives;
* XYZReporter, CenterOfMassReporter -- frames of per-atom / per-molecule positions, velocities, momenta or forces;
* CustomIntegratorReporter -- global and per-DOF variables of a CustomIntegrator;
* ExpandedEnsembleReporter -- expanded-ensemble moves between parameter states and the analysis of the walk.

Column titles and text layouts are those of the reference's reporters (scripts read them back); the code is this package's own.
pandas is imported by the parts that need it only (state tables, text frames), not by `import atomsmm_amd`.
"""
import numpy as np

from . import openmm, unit
from .computers import PressureComputer, _MoleculeTotalizer
from .openmm import app
from .utils import InputError


def _pandas():
    import pandas
    return pandas


def _open(target):
    """(file object, whether this module opened it)"""
    return (open(target, 'w'), True) if isinstance(target, str) else (target, False)


class _Tee:
    """A write-only stream that copies everything to several outputs (a file name is opened here and closed with the tee)."""

    def __init__(self, *targets):
        self._streams = [_open(target) for target in targets]

    def write(self, text):
        for stream, _ in self._streams:
            stream.write(text)

    def flush(self):
        for stream, _ in self._streams:
            stream.flush()

    def __del__(self):
        for stream, owned in self._streams:
            if owned:
                stream.close()


def _output(file, extra):
    return _open(file)[0] if extra is None else _Tee(file, extra)


class _IntervalReporter:
    """Reports every `reportInterval` steps; `_needs` names what the State must carry ('positions', 'velocities', 'forces',
    'energy'); `_setup` runs before the first report, `_write_report` makes every report."""

    def __init__(self, file, reportInterval, extraFile=None, separator=',', **options):
        self._interval = int(reportInterval)
        self._needs = set()
        self._out = _output(file, extraFile)
        self._separator = separator
        self._ready = False

    def describeNextReport(self, simulation):
        wanted = tuple(kind in self._needs for kind in ('positions', 'velocities', 'forces', 'energy'))
        return (self._interval - simulation.currentStep % self._interval,) + wanted

    def report(self, simulation, state):
        if not self._ready:
            self._setup(simulation, state)
            self._ready = True
        self._write_report(simulation, state)

    def _setup(self, simulation, state):
        pass

    def _write_report(self, simulation, state):
        raise NotImplementedError


def _state_energies(simulation, table):
    """Potential energies (kJ/mol) at the states of a DataFrame of global parameters (columns) -- the engine evaluates them at the
    current positions without changing the Context."""
    return simulation.context._engine.energies_at_states([str(name) for name in table.columns], table.to_numpy(dtype=np.float64))


def _kJ(quantity):
    return quantity.value_in_unit(unit.kilojoules_per_mole)


def _atm(quantity):
    return quantity.value_in_unit(unit.atmospheres)


# keyword, column title, what the State must carry besides positions, value (computer, forces)
_VIRIAL_COLUMNS = (
    ('coulombEnergy', 'Coulomb Energy (kJ/mole)', (), lambda pc, f: _kJ(pc.get_coulomb_virial())),      # (-r dE/dr = E for 1/r)
    ('atomicVirial', 'Atomic Virial (kJ/mole)', (), lambda pc, f: _kJ(pc.get_atomic_virial())),
    ('nonbondedVirial', 'Nonbonded Virial (kJ/mole)', (), lambda pc, f: _kJ(pc.get_dispersion_virial() + pc.get_coulomb_virial())),
    ('atomicPressure', 'Atomic Pressure (atm)', ('velocities',), lambda pc, f: _atm(pc.get_atomic_pressure())),
    ('molecularVirial', 'Molecular Virial (kJ/mole)', ('forces',), lambda pc, f: _kJ(pc.get_molecular_virial(f))),
    ('molecularPressure', 'Molecular Pressure (atm)', ('forces', 'velocities'), lambda pc, f: _atm(pc.get_molecular_pressure(f))),
    ('molecularKineticEnergy', 'Molecular Kinetic Energy (kJ/mole)', ('velocities',), lambda pc, f: _kJ(pc.get_molecular_kinetic_energy())),
)


class ExtendedStateDataReporter(app.StateDataReporter):
    """app.StateDataReporter with more columns, placed before the trailing speed column:

    coulombEnergy, atomicVirial, nonbondedVirial, atomicPressure, molecularVirial, molecularPressure, molecularKineticEnergy
        through `pressureComputer` (a PressureComputer; mandatory for these);
    globalParameterStates
        a pandas DataFrame of global parameter values (columns) -- one potential energy per row ('Energy[index] (kJ/mole)');
    globalParameters
        names of global parameters whose values are reported;
    energyDerivatives
        names of global parameters: d(potential energy)/d(parameter), 'diff(E,name)';
    collectiveVariables
        CustomCVForce objects -- not available on this platform (NotImplementedError);
    extraFile
        a second output (file name or file object)."""

    def __init__(self, file, reportInterval, **kwargs):
        self._virials = [column for column in _VIRIAL_COLUMNS if kwargs.pop(column[0], False)]
        self._computer = kwargs.pop('pressureComputer', None)
        self._states = kwargs.pop('globalParameterStates', None)
        self._parameters = list(kwargs.pop('globalParameters', None) or [])
        self._derivatives = list(kwargs.pop('energyDerivatives', None) or [])
        if kwargs.pop('collectiveVariables', None) is not None:
            raise NotImplementedError('ExtendedStateDataReporter(collectiveVariables=...): CustomCVForce.getCollectiveVariableValues is '
                                      'not available on the HIP platform')
        super().__init__(_output(file, kwargs.pop('extraFile', None)), reportInterval, **kwargs)
        if self._virials:
            if not isinstance(self._computer, PressureComputer):
                raise InputError('keyword "pressureComputer" requires a PressureComputer instance')
            carried = {kind for column in self._virials for kind in column[2]}
            self._needsPositions = True
            self._needsVelocities = self._needsVelocities or 'velocities' in carried
            self._needsForces = self._needsForces or 'forces' in carried
        self._trailing = int(self._speed) + int(self._elapsedTime) + int(self._remainingTime)

    def _splice(self, base, extra):
        cut = len(base) - self._trailing
        return base[:cut] + extra + base[cut:]

    def _constructHeaders(self):
        extra = [column[1] for column in self._virials]
        if self._states is not None:
            extra += ['Energy[{}] (kJ/mole)'.format(index) for index in self._states.index]
        extra += self._parameters + ['diff(E,{})'.format(name) for name in self._derivatives]
        return self._splice(super()._constructHeaders(), extra)

    def _constructReportValues(self, simulation, state):
        extra = []
        if self._virials:
            self._computer.import_configuration(state)
            forces = state.getForces(asNumpy=True) if self._needsForces else None
            extra += [column[3](self._computer, forces) for column in self._virials]
        if self._states is not None:
            extra += [float(e) for e in _state_energies(simulation, self._states)]
        extra += [simulation.context.getParameter(name) for name in self._parameters]
        if self._derivatives:
            slopes = simulation.context.getState(getParameterDerivatives=True).getEnergyParameterDerivatives()
            extra += [slopes[name] for name in self._derivatives]
        return self._splice(super()._constructReportValues(simulation, state), extra)


# what a frame holds: unit of the numbers, OpenMM's name of that unit, per-atom quantity of the State (nm, ps, dalton, kJ/mol units)
_FRAME_KINDS = {'positions': (10.0, 'angstrom'),
                'velocities': (10.0, 'angstrom/picosecond'),
                'momenta': (10.0, 'angstrom*dalton/picosecond'),
                'forces': (10.0, 'angstrom*dalton/(picosecond**2)')}      # kJ/mol/nm = dalton nm/ps^2


class XYZReporter(_IntervalReporter):
    """Frames of per-atom positions (angstrom), velocities (angstrom/ps), momenta (dalton angstrom/ps) or forces
    (dalton angstrom/ps^2) in XYZ layout: the atom count, then a tab-separated table headed by what, in which unit, at which step.

    Keyword Args: output ('positions', 'velocities', 'momenta' or 'forces'), groups (force groups of the forces; None: all)."""

    def __init__(self, file, reportInterval, output='positions', groups=None, **kwargs):
        if output not in _FRAME_KINDS:
            raise InputError('Unrecognizable keyword value')
        super().__init__(file, reportInterval, **kwargs)
        self._kind, self._groups = output, groups
        self._needs = {'positions': {'positions'}, 'velocities': {'velocities'}, 'momenta': {'velocities'}, 'forces': {'forces'}}[output]

    def _setup(self, simulation, state):
        self._names = [atom.element.symbol for atom in simulation.topology.atoms()]
        system = simulation.system
        self._masses = np.array([system.getParticleMass(i).value_in_unit(unit.dalton) for i in range(system.getNumParticles())])

    def _per_atom(self, simulation, state):
        """[n][3] in the unit of the frame"""
        if self._kind == 'positions':
            raw = state.getPositions(asNumpy=True)._value
        elif self._kind == 'forces':
            source = state if self._groups is None else simulation.context.getState(getForces=True, groups=self._groups)
            raw = source.getForces(asNumpy=True)._value
        else:
            raw = state.getVelocities(asNumpy=True)._value
            if self._kind == 'momenta':
                raw = self._masses[:, None] * raw
        return _FRAME_KINDS[self._kind][0] * np.asarray(raw, dtype=np.float64)

    def _frame(self, step, names, rows):
        title = '{} in {} at time step {}'.format(self._kind, _FRAME_KINDS[self._kind][1], step)
        print(len(names), file=self._out)
        _pandas().DataFrame(rows, index=names).to_csv(self._out, sep='\t', header=[title, '', ''])

    def _write_report(self, simulation, state):
        self._frame(simulation.currentStep, self._names, self._per_atom(simulation, state))


class CenterOfMassReporter(XYZReporter):
    """XYZReporter per molecule: centre-of-mass positions and velocities, total momenta and resultant forces, each row named by
    the residue of the molecule's first atom."""

    def _setup(self, simulation, state):
        super()._setup(simulation, state)
        self._molecules = _MoleculeTotalizer(simulation.context, simulation.topology)
        residue_of = {atom.index: atom.residue.name for atom in simulation.topology.atoms()}
        self._names = [residue_of[atoms[0]] for atoms in simulation.context.getMolecules()]

    def _write_report(self, simulation, state):
        per_atom = self._per_atom(simulation, state)
        mass_weighted = self._kind in ('positions', 'velocities')
        rows = self._molecules.centre_of_mass(per_atom) if mass_weighted else self._molecules.sum_by_molecule(per_atom)
        self._frame(simulation.currentStep, self._names, rows)


class CustomIntegratorReporter(_IntervalReporter):
    """Global and per-DOF variables of the simulation's CustomIntegrator, named by keyword (`name=True`).  A global variable is
    written as its name and value on two lines; a per-DOF variable as the summary statistics of its x, y, z columns
    (describeOnly=True, the default) or as the whole tab-separated table."""

    def __init__(self, file, reportInterval, describeOnly=True, **kwargs):
        self._wanted = [name for name, flag in kwargs.items() if flag is True]
        super().__init__(file, reportInterval, **kwargs)
        self._summary = describeOnly
        if not self._wanted:
            raise InputError('No global or perDof variables have been passed')

    def _setup(self, simulation, state):
        integrator = simulation.integrator
        if not isinstance(integrator, openmm.CustomIntegrator):
            raise Exception('simulation.integrator is not a CustomIntegrator')
        scalars = [integrator.getGlobalVariableName(k) for k in range(integrator.getNumGlobalVariables())]
        vectors = [integrator.getPerDofVariableName(k) for k in range(integrator.getNumPerDofVariables())]
        unknown = [name for name in self._wanted if name not in scalars and name not in vectors]
        if unknown:
            raise InputError('Unknown variables have been passed: ' + ', '.join(unknown))
        self._integrator = integrator
        self._scalars = [(name, k) for k, name in enumerate(scalars) if name in self._wanted]
        self._vectors = [(name, k) for k, name in enumerate(vectors) if name in self._wanted]

    def _write_report(self, simulation, state):
        for name, k in self._scalars:
            print(name, file=self._out)
            print(self._integrator.getGlobalVariable(k), file=self._out)
        for name, k in self._vectors:
            rows = np.array([list(v) for v in self._integrator.getPerDofVariable(k)], dtype=np.float64).reshape(-1, 3)
            table = _pandas().DataFrame(rows, columns=[name + '.' + axis for axis in 'xyz'])
            if self._summary:
                print(table.describe(), file=self._out)
            else:
                table.to_csv(self._out, sep='\t')


class _Walk:
    """Book-keeping of an expanded-ensemble walk between the `first` and the `last` visitable state.  The walk goes DOWN from an
    arrival at `last` until the next arrival at `first`, and up otherwise; `turns` lists the report numbers of the arrivals that
    changed the direction.  Visits are counted from the report after the first arrival at `last` on."""

    def __init__(self, nstates, first, last):
        self.first, self.last = first, last
        self.down = False
        self.counting = False
        self.turns = []
        self.visits = np.zeros(nstates, dtype=int)
        self.down_visits = np.zeros(nstates, dtype=int)

    def visit(self, state, report):
        if state == (self.first if self.down else self.last):
            self.down = not self.down
            self.turns.append(report)
        if not self.counting:
            self.counting = self.down
            return
        self.visits[state] += 1
        self.down_visits[state] += int(self.down)


def _slope_estimates(f, n):
    """Least-squares slopes of the sorted values of f over windows of +-n neighbours (sum_m m (f[i+m] - f[i-m]) / (2 sum_m m^2), indices
    clamped to the ends); at the two ends a one-sided form: sum_k A_k (f[k] - f[0]) with A_k = sum_{m >= k} m / (2 sum_m m^2) (the
    A_k add up to 1/2).  Returned in the original order of f."""
    N = len(f)
    order = np.argsort(f)
    g = np.asarray(f, dtype=np.float64)[order]
    m = np.arange(1, n + 1)
    norm = 2.0 * np.sum(m * m)
    ahead = np.minimum(np.arange(N)[:, None] + m, N - 1)
    behind = np.maximum(np.arange(N)[:, None] - m, 0)
    slope = ((g[ahead] - g[behind]) * m).sum(axis=1) / norm
    tail = np.cumsum(m[::-1])[::-1] / norm                  # A_k
    k = np.minimum(m, N - 1)
    slope[0] = np.sum(tail * (g[k] - g[0]))
    slope[N - 1] = np.sum(tail * (g[N - 1] - g[N - 1 - k]))
    out = np.empty(N)
    out[order] = slope
    return out


class ExpandedEnsembleReporter(_IntervalReporter):
    """Expanded-ensemble simulation over the parameter states of `states` (a pandas DataFrame: global parameters as columns; an
    optional `weight` column holds each state's log importance weight, -inf for states that are only reported, never visited).

    Every report writes the step, the current state and the potential energy at every state (Engine.energies_at_states); every
    `reportsPerExchange` reports the Context moves to a state drawn with probability proportional to exp(weight - E / RT)
    (np.random.choice).  state_sampling_analysis(), walking_time_analysis() and read_csv() (the output of an earlier run) work on
    the walk (see _Walk)."""

    def __init__(self, file, reportInterval, states, temperature, reportsPerExchange=1, **kwargs):
        super().__init__(file, reportInterval, **kwargs)
        table = states.copy()
        self._log_weights = np.asarray(table.pop('weight'), dtype=np.float64) if 'weight' in table else np.zeros(len(table))
        self._table = table
        self._per_exchange = int(reportsPerExchange)
        RT = (unit.MOLAR_GAS_CONSTANT_R * temperature).value_in_unit(unit.kilojoules_per_mole)
        self._beta = 1.0 / RT
        visitable = np.flatnonzero(np.isfinite(self._log_weights))
        self._walk = _Walk(len(table), int(visitable[0]), int(visitable[-1]))
        self._reports = 0
        self._summed_probabilities = np.zeros(len(table))
        self._current = -1

    def _probabilities(self, energies):
        """exp(w_k - beta E_k), normalised (log-sum-exp)."""
        z = self._log_weights - self._beta * np.asarray(energies, dtype=np.float64)
        return np.exp(z - np.logaddexp.reduce(z))

    def _count(self, energies):
        """one report's share of the statistics; returns its probabilities and whether it is an exchange"""
        self._reports += 1
        p = self._probabilities(energies)
        self._summed_probabilities += p
        return p, self._reports % self._per_exchange == 0

    def _setup(self, simulation, state):
        here = np.array([simulation.context.getParameter(name) for name in self._table.columns])
        match = np.flatnonzero(np.all(self._table.to_numpy(dtype=np.float64) == here, axis=1))
        self._current = int(match[0]) if len(match) else -1
        titles = ['step', 'state'] + ['Energy[{}] (kJ/mole)'.format(index) for index in self._table.index]
        print(self._separator.join(titles), file=self._out)

    def _write_report(self, simulation, state):
        energies = np.asarray(_state_energies(simulation, self._table), dtype=np.float64)
        p, exchange = self._count(energies)
        if exchange:
            self._current = int(np.random.choice(len(p), p=p))
            for name, value in zip(self._table.columns, self._table.iloc[self._current]):
                if simulation.context.getParameter(name) != value:
                    simulation.context.setParameter(name, value)
            self._walk.visit(self._current, self._reports)
        print(self._separator.join(str(v) for v in [simulation.currentStep, self._current] + list(energies)), file=self._out)

    def read_csv(self, file, **kwargs):
        """Take in the reports of an earlier run (its output) as if they had been made here."""
        kwargs.setdefault('comment', '#')
        kwargs.setdefault('sep', self._separator)
        frame = _pandas().read_csv(file, **kwargs)
        columns = ['Energy[{}] (kJ/mole)'.format(index) for index in self._table.index]
        for state, energies in zip(frame['state'].astype(int), frame[columns].to_numpy(dtype=np.float64)):
            if self._count(energies)[1]:
                self._walk.visit(int(state), self._reports)

    def state_sampling_analysis(self, staging_variable=None, to_file=True, isochronal_n=2):
        """Per visited state: the parameters, the weight, the visit histogram and the fraction of visits made on downhill walks; once
        counting has started also the free energy from the mean probabilities (-ln p + weight, zero at the first row), the
        isochronal histogram sqrt(delta p) and weight (weight + ln(delta / p) / 2, zero at the first row), delta being the slope of
        the downhill fraction (_slope_estimates, +-isochronal_n states); with `staging_variable` also the values of that parameter
        that make the downhill fraction's optimal density sqrt(df/dx) uniform, and the free energy interpolated there.  A pandas
        DataFrame."""
        pd = _pandas()
        seen = self._walk.visits > 0
        visits = self._walk.visits[seen]
        weight = self._log_weights[seen]
        downhill = self._walk.down_visits[seen] / visits
        columns = {'weight': weight, 'histogram': visits / visits.sum(), 'downhill_fraction': downhill}
        if self._walk.counting:
            p = self._summed_probabilities[seen] / self._reports
            free = weight - np.log(p)
            delta = _slope_estimates(downhill, isochronal_n)
            iso = weight + 0.5 * np.log(delta / p)
            columns.update(free_energy=free - free[0], isochronal_histogram=np.sqrt(delta * p), isochronal_weight=iso - iso[0])
            if staging_variable is not None:
                x = self._table[staging_variable].to_numpy(dtype=np.float64)[seen]
                mass = np.sqrt(np.diff(downhill) * np.diff(x))                   # integral of sqrt(df/dx) over each interval
                cdf = np.concatenate([[0.0], np.cumsum(mass) / mass.sum()])
                staged = np.interp(np.linspace(0.0, 1.0, len(x)), cdf, x)
                columns['staging_' + staging_variable] = staged
                columns['staging_weight'] = np.interp(staged, x, columns['free_energy'])
        frame = self._table[seen].copy()
        for name, values in columns.items():
            frame[name] = values
        if to_file:
            rule = '-' * 40
            print('# {} State Sampling Analysis {}'.format(rule, rule), file=self._out)
            with pd.option_context('display.max_rows', None, 'display.max_columns', None):
                print('# ' + frame.to_string(index=False).replace('\n', '\n# '), file=self._out)
        return frame

    def walking_time_analysis(self, history=False, to_file=True):
        """Durations in steps of the downhill walks (an arrival at the last visitable state to the next at the first) and of the
        uphill ones; their count and mean, and with `history` every duration."""
        pd = _pandas()
        legs = self._interval * np.diff(np.asarray(self._walk.turns, dtype=int))
        down, up = legs[0::2], legs[1::2]
        rule = '-' * 10
        if history:
            print('# {} Walking Time History {}'.format(rule, rule), file=self._out)
            walks = pd.DataFrame({'downhill': pd.Series(down), 'uphill': pd.Series(up)})
            print('# ' + walks.to_string().replace('\n', '\n# '), file=self._out)
        summary = pd.DataFrame([[down.size, up.size], [down.mean(), up.mean()]], index=['count', 'mean time'],
                               columns=['downhill', 'uphill'], dtype='object')
        if to_file:
            print('# {} Walking Time Analysis {}'.format(rule, rule), file=self._out)
            print('# ' + summary.to_string().replace('\n', '\n# '), file=self._out)
        return summary
