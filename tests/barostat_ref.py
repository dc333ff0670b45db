"""CPU restatement of a constant-pressure RESPA run, for tests: the loop of Engine.step with a MonteCarloBarostat -- when an attempt
is made, the move, the acceptance test, the step-size adaptation, the numpy random stream -- over oracle.respa_cpu.RespaCPU and
the oracle's energies.  The system is flexible water in the composition of BASELINE config C1: harmonic bonds and angles (group 0),
the near force-switched force (group 1) and DampedSmoothedForce as the total (group 2); the near force and its negative in group
31 cancel in the potential energy, which is bonds + angles + the damped total.

TEST INFRASTRUCTURE ONLY: nothing here is imported by the package."""
import math

import numpy as np

from oracle import oracle as O
from oracle.respa_cpu import RespaCPU

R = 1.3806504e-23 * 6.02214179e23 * 1e-3          # kJ/mol/K, the constants of atomsmm_amd.unit
BAR = 1e5 * 1e-27 * 6.02214179e23 * 1e-3          # 1 bar in kJ/mol/nm^3


def scale_molecules(x, molecules, s):
    out = x.copy()
    for m in molecules:
        out[m] = x[m] + (s - 1.0) * (x[m].sum(axis=0) / len(m))
    return out


class PlainRespaCPU(RespaCPU):
    """RespaCPU with every pair force summed by the oracle's plain double loop instead of its 27-cell walk: the oracle's other order
    of summation that a box of 2.5 nm admits (its Verlet lists need three cells of cutoff + buffer per axis: 3.3 nm for the outer
    force)."""

    def f(self, g):
        c = self.c
        if g != 0 and g not in self.F:
            self.evals[g] += 1
            d = self.dn if g == 1 else self.dd
            self.F[g] = O.pair_eval(d, self.x, c['box'], c['charge'], c['sigma'], c['epsilon'], use_cells=False, csr=self.csr)[1]
        return RespaCPU.f(self, g)


class BarostatCPU:
    def __init__(self, case, pressure, temperature, frequency, seed, dt=0.001, loops=(4, 2, 1), plain=False):
        self.case = dict(case)
        self.case['box'] = np.array(case['box'], dtype=np.float64)
        self.plain = plain
        self.cpu = (PlainRespaCPU if plain else RespaCPU)(self.case, dt=dt, loops=loops)
        n = len(case['positions'])
        self.molecules = [[3 * m, 3 * m + 1, 3 * m + 2] for m in range(n // 3)]
        self.pressure, self.kT, self.frequency = pressure * BAR, R * temperature, frequency
        self.rng = np.random.default_rng(seed)
        self.due = frequency - 1
        self.scale = None
        self.window = [0, 0]
        self.stats = dict(attempts=0, accepted=0)
        self.log = []                   # (accepted, w, u2 or None, box afterwards, margin of the decision)

    def energy(self):
        c, x = self.cpu.c, self.cpu.x
        e = O.harmonic_bonds(c['bonds'], c['bond_r0'], c['bond_k'], x, c['box'], want_forces=False)[0]
        e += O.harmonic_angles(c['angles'], c['angle_theta0'], c['angle_k'], x, c['box'], want_forces=False)[0]
        cells = not self.plain and min(c['box']) / self.cpu.dd.rc >= 3.0     # (as RespaCPU.f: the walk needs three cells per axis)
        e += O.pair_eval(self.cpu.dd, x, c['box'], c['charge'], c['sigma'], c['epsilon'], want_forces=False, use_cells=cells,
                         csr=self.cpu.csr)[0]
        return e

    def set_box(self, box):
        self.cpu.c['box'] = np.array(box, dtype=np.float64)

    def attempt(self):
        cpu = self.cpu
        e0 = self.energy()
        box0, x0, forces = cpu.c['box'].copy(), cpu.x.copy(), dict(cpu.F)
        volume = float(np.prod(box0))
        if self.scale is None:
            self.scale = 0.01 * volume
        delta = self.scale * 2.0 * (self.rng.random() - 0.5)
        new_volume = volume + delta
        s = (new_volume / volume) ** (1.0 / 3.0)
        self.set_box(box0 * s)
        cpu.x[...] = scale_molecules(x0, self.molecules, s)
        cpu.F.clear()
        e1 = self.energy()
        w = e1 - e0 + self.pressure * delta - len(self.molecules) * self.kT * math.log(new_volume / volume)
        u2, accepted, margin = None, True, -w
        if w > 0:
            u2 = self.rng.random()
            accepted = not u2 > math.exp(-w / self.kT)
            margin = abs(u2 - math.exp(-w / self.kT))
        if not accepted:
            cpu.x[...] = x0
            self.set_box(box0)
            cpu.F.update(forces)        # (positions and box are the old bits: the forces held before the attempt hold again)
        self.stats['attempts'] += 1
        self.stats['accepted'] += int(accepted)
        self.log.append((accepted, w, u2, cpu.c['box'].copy(), margin))
        self.window[0] += 1
        self.window[1] += int(accepted)
        if self.window[0] >= 10:
            if self.window[1] < 0.25 * self.window[0]:
                self.scale /= 1.1
                self.window = [0, 0]
            elif self.window[1] > 0.75 * self.window[0]:
                self.scale = min(self.scale * 1.1, 0.3 * float(np.prod(cpu.c['box'])))
                self.window = [0, 0]

    def step(self, n):
        remaining = n
        while remaining > 0:
            if self.due <= 0:
                self.attempt()
                self.due = self.frequency
            count = min(remaining, self.due)
            self.cpu.step(count)
            self.due -= count
            remaining -= count
