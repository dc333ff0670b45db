"""Minimal OpenMM-shaped object model for the AtomsMM hot path (host side, pure Python).

AtomsMM's classes subclass OpenMM's SWIG classes (forces.py:134,193,326; systems.py:34;
integrators.py:26).  OpenMM is absent here, and north_star forbids building an OpenMM platform, so
this module supplies just the container/accessor API that AtomsMM and its tests call
(`addParticle`, `getExceptionParameters`, `addComputePerDof`, `getState(groups=...)`, ...), with
the same method names and argument meaning.  It holds *descriptions only*; all arithmetic happens in
the HIP library through `atomsmm_amd.engine` when a `Context` is created.

Usage in a script written for the reference:

    from atomsmm_amd import openmm, unit          # instead of: from simtk import openmm, unit
    from atomsmm_amd.openmm import app
    import atomsmm_amd as atomsmm
"""
import copy
import math

import numpy as np

from .. import unit as _unit
from ..unit import Quantity, md_value
from ..utils import InputError

nm = _unit.nanometer
kjmol = _unit.kilojoule_per_mole


class OpenMMException(Exception):
    pass


class Vec3(tuple):
    def __new__(cls, x, y, z):
        return tuple.__new__(cls, (x, y, z))

    x = property(lambda s: s[0])
    y = property(lambda s: s[1])
    z = property(lambda s: s[2])

    def __add__(self, o):
        return Vec3(self[0] + o[0], self[1] + o[1], self[2] + o[2])

    def __sub__(self, o):
        return Vec3(self[0] - o[0], self[1] - o[1], self[2] - o[2])

    def __mul__(self, s):
        if isinstance(s, (_unit.Unit, Quantity)):
            return Quantity(self, s) if isinstance(s, _unit.Unit) else NotImplemented
        return Vec3(self[0] * s, self[1] * s, self[2] * s)

    __rmul__ = __mul__


# ------------------------------------------------------------------------------------------------ forces
class Force:
    def __init__(self):
        self._group = 0
        self._name = self.__class__.__name__

    def getForceGroup(self):
        return self._group

    def setForceGroup(self, group):
        if not 0 <= int(group) <= 31:
            raise OpenMMException('Force group must be between 0 and 31')
        self._group = int(group)

    def usesPeriodicBoundaryConditions(self):
        return False

    def getName(self):
        return self._name

    def setName(self, name):
        self._name = name


class _GlobalParams:
    """Mixin: global parameters with default values."""

    def _init_globals(self):
        self._gnames = []
        self._gvalues = []

    def addGlobalParameter(self, name, defaultValue):
        self._gnames.append(name)
        self._gvalues.append(float(md_value(defaultValue)))
        return len(self._gnames) - 1

    def getNumGlobalParameters(self):
        return len(self._gnames)

    def getGlobalParameterName(self, index):
        return self._gnames[index]

    def getGlobalParameterDefaultValue(self, index):
        return self._gvalues[index]

    def setGlobalParameterDefaultValue(self, index, value):
        self._gvalues[index] = float(md_value(value))


class NonbondedForce(Force, _GlobalParams):
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic, Ewald, PME, LJPME = range(6)

    def __init__(self):
        Force.__init__(self)
        self._init_globals()
        self._particles = []       # [q, sigma, eps]
        self._exceptions = []      # [i, j, qq, sigma, eps]
        self._exc_index = {}
        self._method = self.NoCutoff
        self._cutoff = 1.0
        self._use_switch = False
        self._switch = -1.0
        self._ewald_tol = 5e-4
        self._pme = (0.0, 0, 0, 0)
        self._dispersion = True
        self._recip_group = -1
        self._rf_dielectric = 78.3
        self._particle_offsets = []    # [param, particle, qs, ss, es]
        self._exception_offsets = []   # [param, exception, qqs, ss, es]

    def usesPeriodicBoundaryConditions(self):
        return self._method in (self.CutoffPeriodic, self.Ewald, self.PME, self.LJPME)

    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, charge, sigma, epsilon):
        self._particles.append([float(md_value(charge)), float(md_value(sigma)), float(md_value(epsilon))])
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        q, s, e = self._particles[index]
        return [Quantity(q, _unit.elementary_charge), Quantity(s, nm), Quantity(e, kjmol)]

    def setParticleParameters(self, index, charge, sigma, epsilon):
        self._particles[index] = [float(md_value(charge)), float(md_value(sigma)), float(md_value(epsilon))]

    def updateParametersInContext(self, context):
        """Upload the particle and exception parameters again (systems.py:811-812)."""
        context._engine.update_force_parameters(self)

    def getNumExceptions(self):
        return len(self._exceptions)

    def addException(self, particle1, particle2, chargeProd, sigma, epsilon, replace=False):
        key = (min(particle1, particle2), max(particle1, particle2))
        rec = [int(particle1), int(particle2), float(md_value(chargeProd)), float(md_value(sigma)), float(md_value(epsilon))]
        if key in self._exc_index:
            if not replace:
                raise OpenMMException('NonbondedForce: There is already an exception for particles %d and %d' % key)
            self._exceptions[self._exc_index[key]] = rec
            return self._exc_index[key]
        self._exceptions.append(rec)
        self._exc_index[key] = len(self._exceptions) - 1
        return len(self._exceptions) - 1

    def getExceptionParameters(self, index):
        i, j, qq, s, e = self._exceptions[index]
        return [i, j, Quantity(qq, _unit.elementary_charge ** 2), Quantity(s, nm), Quantity(e, kjmol)]

    def setExceptionParameters(self, index, particle1, particle2, chargeProd, sigma, epsilon):
        self._exceptions[index] = [int(particle1), int(particle2), float(md_value(chargeProd)), float(md_value(sigma)),
                                   float(md_value(epsilon))]

    def createExceptionsFromBonds(self, bonds, coulomb14Scale, lj14Scale):
        n = self.getNumParticles()
        nbrs = [set() for _ in range(n)]
        for i, j in bonds:
            nbrs[i].add(j); nbrs[j].add(i)
        excl, p14 = set(), set()
        for i, j in bonds:
            excl.add((min(i, j), max(i, j)))
        for j in range(n):
            nb = sorted(nbrs[j])
            for a in range(len(nb)):
                for b in range(a + 1, len(nb)):
                    excl.add((nb[a], nb[b]))
        for j, k in bonds:
            for i in nbrs[j]:
                for l in nbrs[k]:
                    if i != k and l != j and i != l:
                        key = (min(i, l), max(i, l))
                        if key not in excl:
                            p14.add(key)
        for i, j in sorted(excl):
            self.addException(i, j, 0.0, 0.5 * (self._particles[i][1] + self._particles[j][1]), 0.0, True)
        for i, j in sorted(p14):
            qi, si, ei = self._particles[i]
            qj, sj, ej = self._particles[j]
            self.addException(i, j, coulomb14Scale * qi * qj, 0.5 * (si + sj), lj14Scale * math.sqrt(ei * ej), True)

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def getUseSwitchingFunction(self):
        return self._use_switch

    def setUseSwitchingFunction(self, use):
        self._use_switch = bool(use)

    def getSwitchingDistance(self):
        return Quantity(self._switch, nm)

    def setSwitchingDistance(self, distance):
        self._switch = float(md_value(distance))

    def getEwaldErrorTolerance(self):
        return self._ewald_tol

    def setEwaldErrorTolerance(self, tol):
        self._ewald_tol = float(tol)

    def getPMEParameters(self):
        a, nx, ny, nz = self._pme
        return [Quantity(a, nm ** -1), nx, ny, nz]

    def setPMEParameters(self, alpha, nx, ny, nz):
        self._pme = (float(md_value(alpha)), int(nx), int(ny), int(nz))

    def getUseDispersionCorrection(self):
        return self._dispersion

    def setUseDispersionCorrection(self, use):
        self._dispersion = bool(use)

    def getReciprocalSpaceForceGroup(self):
        return self._recip_group

    def setReciprocalSpaceForceGroup(self, group):
        self._recip_group = int(group)

    def getReactionFieldDielectric(self):
        return self._rf_dielectric

    def setReactionFieldDielectric(self, d):
        self._rf_dielectric = float(d)

    def addParticleParameterOffset(self, parameter, particleIndex, chargeScale, sigmaScale, epsilonScale):
        self._particle_offsets.append([parameter, int(particleIndex), float(md_value(chargeScale)),
                                       float(md_value(sigmaScale)), float(md_value(epsilonScale))])
        return len(self._particle_offsets) - 1

    def getNumParticleParameterOffsets(self):
        return len(self._particle_offsets)

    def getParticleParameterOffset(self, index):
        return list(self._particle_offsets[index])

    def addExceptionParameterOffset(self, parameter, exceptionIndex, chargeProdScale, sigmaScale, epsilonScale):
        self._exception_offsets.append([parameter, int(exceptionIndex), float(md_value(chargeProdScale)),
                                        float(md_value(sigmaScale)), float(md_value(epsilonScale))])
        return len(self._exception_offsets) - 1

    def getNumExceptionParameterOffsets(self):
        return len(self._exception_offsets)

    def getExceptionParameterOffset(self, index):
        return list(self._exception_offsets[index])


class GBSAOBCForce(Force):
    """Generalized-Born implicit solvent (OBC2) with a surface-area term, for free-space systems: NoCutoff and CutoffNonPeriodic
    (csrc/gb.hip).  Every particle of the System takes part; exclusions and exceptions of other forces play no role."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)

    def __init__(self):
        Force.__init__(self)
        self._particles = []       # [q, radius, scale]
        self._method = self.NoCutoff
        self._cutoff = 1.0
        self._solvent_dielectric = 78.3
        self._solute_dielectric = 1.0
        self._sa_energy = 2.25936  # kJ/mol/nm^2

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, charge, radius, scalingFactor):
        self._particles.append([float(md_value(charge)), float(md_value(radius)), float(scalingFactor)])
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        q, r, s = self._particles[index]
        return [Quantity(q, _unit.elementary_charge), Quantity(r, nm), s]

    def setParticleParameters(self, index, charge, radius, scalingFactor):
        self._particles[index] = [float(md_value(charge)), float(md_value(radius)), float(scalingFactor)]

    def updateParametersInContext(self, context):
        """Upload the particle parameters, the dielectrics and the surface-area energy again."""
        context._engine.update_force_parameters(self)

    def getSolventDielectric(self):
        return self._solvent_dielectric

    def setSolventDielectric(self, dielectric):
        self._solvent_dielectric = float(dielectric)

    def getSoluteDielectric(self):
        return self._solute_dielectric

    def setSoluteDielectric(self, dielectric):
        self._solute_dielectric = float(dielectric)

    def getSurfaceAreaEnergy(self):
        return Quantity(self._sa_energy, kjmol / nm ** 2)

    def setSurfaceAreaEnergy(self, energy):
        self._sa_energy = float(md_value(energy))

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))


class TabulatedFunction:
    """A function given by numbers, for CustomNonbondedForce.addTabulatedFunction.  Evaluated on the GPU by the pair-expression
    kernel (atomsmm_amd/tables.py): Continuous1DFunction, Discrete1DFunction and Discrete2DFunction."""
    _amm_table_kind = None


def _table_values(values):
    return [float(md_value(v)) for v in values]


class Continuous1DFunction(TabulatedFunction):
    """The natural cubic spline through `values` at equally spaced knots min .. max; 0 outside [min, max]."""
    _amm_table_kind = 0

    def __init__(self, values, min, max, periodic=False):
        if periodic:
            raise NotImplementedError('Continuous1DFunction(periodic=True): periodic splines are not evaluated by the HIP path')
        self.setFunctionParameters(values, min, max)

    def getFunctionParameters(self):
        return list(self._values), self._min, self._max

    def setFunctionParameters(self, values, min, max):
        values, lo, hi = _table_values(values), float(md_value(min)), float(md_value(max))
        if len(values) < 2:
            raise OpenMMException('Continuous1DFunction: must have at least two points')
        if not lo < hi:
            raise OpenMMException('Continuous1DFunction: max <= min for a tabulated function.')
        self._values, self._min, self._max = values, lo, hi

    def getPeriodic(self):
        return False


class Discrete1DFunction(TabulatedFunction):
    """values[i], i the argument rounded to the nearest integer."""
    _amm_table_kind = 1

    def __init__(self, values):
        self.setFunctionParameters(values)

    def getFunctionParameters(self):
        return list(self._values)

    def setFunctionParameters(self, values):
        values = _table_values(values)
        if not values:
            raise OpenMMException('Discrete1DFunction: must have at least one value')
        self._values = values


class Discrete2DFunction(TabulatedFunction):
    """values[i + xsize*j], i and j the arguments rounded to the nearest integers."""
    _amm_table_kind = 2

    def __init__(self, xsize, ysize, values):
        self.setFunctionParameters(xsize, ysize, values)

    def getFunctionParameters(self):
        return self._xsize, self._ysize, list(self._values)

    def setFunctionParameters(self, xsize, ysize, values):
        xsize, ysize, values = int(xsize), int(ysize), _table_values(values)
        if xsize < 1 or ysize < 1 or xsize * ysize != len(values):
            raise OpenMMException('Discrete2DFunction: incorrect number of values (xsize*ysize = %d, %d given)' % (xsize * ysize, len(values)))
        self._xsize, self._ysize, self._values = xsize, ysize, values


def _refused_table(name, what):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError('%s: %s are not evaluated by the HIP path (Continuous1DFunction, Discrete1DFunction and '
                                  'Discrete2DFunction are)' % (name, what))
    return type(name, (TabulatedFunction,), dict(__init__=__init__, __doc__='Not supported: the constructor says so.'))


Continuous2DFunction = _refused_table('Continuous2DFunction', 'two-dimensional splines')
Continuous3DFunction = _refused_table('Continuous3DFunction', 'three-dimensional splines')
Discrete3DFunction = _refused_table('Discrete3DFunction', 'three-dimensional tables')


class CustomNonbondedForce(Force, _GlobalParams):
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)

    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._pnames = []
        self._particles = []
        self._exclusions = []
        self._method = self.NoCutoff
        self._cutoff = 1.0
        self._use_switch = False
        self._switch = -1.0
        self._lrc = False
        self._groups = []
        self._derivs = []
        self._functions = []

    def addTabulatedFunction(self, name, function):
        """The text may call `name(...)`.  The force keeps the object itself, as OpenMM does: setFunctionParameters on it followed by
        updateParametersInContext reaches the Context."""
        if not isinstance(function, TabulatedFunction):
            raise OpenMMException('addTabulatedFunction: not a TabulatedFunction')
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    def getTabulatedFunction(self, index):
        return self._functions[index][1]

    def getTabulatedFunctionName(self, index):
        return self._functions[index][0]

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = energy

    def addPerParticleParameter(self, name):
        self._pnames.append(name)
        return len(self._pnames) - 1

    def getNumPerParticleParameters(self):
        return len(self._pnames)

    def getPerParticleParameterName(self, index):
        return self._pnames[index]

    def addParticle(self, parameters=()):
        self._particles.append([float(md_value(p)) for p in parameters])
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        return tuple(self._particles[index])

    def setParticleParameters(self, index, parameters):
        self._particles[index] = [float(md_value(p)) for p in parameters]

    def updateParametersInContext(self, context):
        """Upload the per-particle parameters again (systems.py:813-814)."""
        context._engine.update_force_parameters(self)

    def addExclusion(self, particle1, particle2):
        self._exclusions.append((int(particle1), int(particle2)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return list(self._exclusions[index])

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def getUseSwitchingFunction(self):
        return self._use_switch

    def setUseSwitchingFunction(self, use):
        self._use_switch = bool(use)

    def getSwitchingDistance(self):
        return Quantity(self._switch, nm)

    def setSwitchingDistance(self, distance):
        self._switch = float(md_value(distance))

    def getUseLongRangeCorrection(self):
        return self._lrc

    def setUseLongRangeCorrection(self, use):
        self._lrc = bool(use)

    def addInteractionGroup(self, set1, set2):
        self._groups.append((set(set1), set(set2)))
        return len(self._groups) - 1

    def getNumInteractionGroups(self):
        return len(self._groups)

    def getInteractionGroupParameters(self, index):
        return [set(self._groups[index][0]), set(self._groups[index][1])]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)


class CustomGBForce(Force, _GlobalParams):
    """A generalized-Born model written as text: computed per-particle values and energy terms, for free-space systems (NoCutoff and
    CutoffNonPeriodic; csrc/custom_gb.hip).  Only the first computed value may be a sum over pairs."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)
    SingleParticle, ParticlePair, ParticlePairNoExclusions = range(3)

    def __init__(self):
        Force.__init__(self)
        self._init_globals()
        self._pnames = []
        self._particles = []
        self._exclusions = []
        self._values = []          # [name, text, type]
        self._terms = []           # [text, type]
        self._functions = []
        self._derivs = []
        self._method = self.NoCutoff
        self._cutoff = 1.0

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def addPerParticleParameter(self, name):
        self._pnames.append(str(name))
        return len(self._pnames) - 1

    def getNumPerParticleParameters(self):
        return len(self._pnames)

    def getPerParticleParameterName(self, index):
        return self._pnames[index]

    def setPerParticleParameterName(self, index, name):
        self._pnames[index] = str(name)

    def addParticle(self, parameters=()):
        self._particles.append([float(md_value(p)) for p in parameters])
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        return tuple(self._particles[index])

    def setParticleParameters(self, index, parameters):
        self._particles[index] = [float(md_value(p)) for p in parameters]

    def addComputedValue(self, name, expression, type):
        self._values.append([str(name), str(expression), int(type)])
        return len(self._values) - 1

    def getNumComputedValues(self):
        return len(self._values)

    def getComputedValueParameters(self, index):
        return list(self._values[index])

    def setComputedValueParameters(self, index, name, expression, type):
        self._values[index] = [str(name), str(expression), int(type)]

    def addEnergyTerm(self, expression, type):
        self._terms.append([str(expression), int(type)])
        return len(self._terms) - 1

    def getNumEnergyTerms(self):
        return len(self._terms)

    def getEnergyTermParameters(self, index):
        return list(self._terms[index])

    def setEnergyTermParameters(self, index, expression, type):
        self._terms[index] = [str(expression), int(type)]

    def addExclusion(self, particle1, particle2):
        self._exclusions.append((int(particle1), int(particle2)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return list(self._exclusions[index])

    def setExclusionParticles(self, index, particle1, particle2):
        self._exclusions[index] = (int(particle1), int(particle2))

    def addTabulatedFunction(self, name, function):
        """The texts may call `name(...)`.  The force keeps the object itself: setFunctionParameters on it followed by
        updateParametersInContext reaches the Context."""
        if not isinstance(function, TabulatedFunction):
            raise OpenMMException('addTabulatedFunction: not a TabulatedFunction')
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    addFunction = addTabulatedFunction

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    getNumFunctions = getNumTabulatedFunctions

    def getTabulatedFunction(self, index):
        return self._functions[index][1]

    def getTabulatedFunctionName(self, index):
        return self._functions[index][0]

    def addEnergyParameterDerivative(self, name):
        """Recorded; a Context refuses the force by name (the kernels differentiate in positions only)."""
        self._derivs.append(str(name))

    def getNumEnergyParameterDerivatives(self):
        return len(self._derivs)

    def getEnergyParameterDerivativeName(self, index):
        return self._derivs[index]

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def updateParametersInContext(self, context):
        """Upload the per-particle parameters and the tabulated functions' values again.  Counts, texts and exclusions must not have
        changed."""
        context._engine.update_force_parameters(self)

    def getComputedValues(self, context):
        """The computed values at the Context's positions, [value][particle] (a diagnostic OpenMM does not have)."""
        return context._engine.custom_gb_values(self)


class CustomHbondForce(Force, _GlobalParams):
    """Donors (d1, d2, d3) against acceptors (a1, a2, a3): every pair that is not excluded and whose distance(d1, a1) lies inside the
    cutoff contributes the energy text -- distance, angle and dihedral over the six particles, per-donor, per-acceptor and global
    parameters (csrc/hbond.hip).  d2, d3, a2, a3 may be -1 when the text does not name them."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)

    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = str(energy)
        self._dnames = []
        self._anames = []
        self._donors = []          # [[d1, d2, d3], [parameters]]
        self._acceptors = []       # [[a1, a2, a3], [parameters]]
        self._exclusions = []      # (donor, acceptor): indices of donors and acceptors, not of atoms
        self._functions = []
        self._method = self.NoCutoff
        self._cutoff = 1.0

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = str(energy)

    def addPerDonorParameter(self, name):
        self._dnames.append(str(name))
        return len(self._dnames) - 1

    def getNumPerDonorParameters(self):
        return len(self._dnames)

    def getPerDonorParameterName(self, index):
        return self._dnames[index]

    def setPerDonorParameterName(self, index, name):
        self._dnames[index] = str(name)

    def addPerAcceptorParameter(self, name):
        self._anames.append(str(name))
        return len(self._anames) - 1

    def getNumPerAcceptorParameters(self):
        return len(self._anames)

    def getPerAcceptorParameterName(self, index):
        return self._anames[index]

    def setPerAcceptorParameterName(self, index, name):
        self._anames[index] = str(name)

    def setGlobalParameterName(self, index, name):
        self._gnames[index] = str(name)

    @staticmethod
    def _row(p1, p2, p3, parameters):
        return [[int(p1), int(p2), int(p3)], [float(md_value(p)) for p in parameters]]

    def addDonor(self, d1, d2, d3, parameters=()):
        self._donors.append(self._row(d1, d2, d3, parameters))
        return len(self._donors) - 1

    def getNumDonors(self):
        return len(self._donors)

    def getDonorParameters(self, index):
        (d1, d2, d3), p = self._donors[index]
        return [d1, d2, d3, tuple(p)]

    def setDonorParameters(self, index, d1, d2, d3, parameters=()):
        self._donors[index] = self._row(d1, d2, d3, parameters)

    def addAcceptor(self, a1, a2, a3, parameters=()):
        self._acceptors.append(self._row(a1, a2, a3, parameters))
        return len(self._acceptors) - 1

    def getNumAcceptors(self):
        return len(self._acceptors)

    def getAcceptorParameters(self, index):
        (a1, a2, a3), p = self._acceptors[index]
        return [a1, a2, a3, tuple(p)]

    def setAcceptorParameters(self, index, a1, a2, a3, parameters=()):
        self._acceptors[index] = self._row(a1, a2, a3, parameters)

    def addExclusion(self, donor, acceptor):
        self._exclusions.append((int(donor), int(acceptor)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return list(self._exclusions[index])

    def setExclusionParticles(self, index, donor, acceptor):
        self._exclusions[index] = (int(donor), int(acceptor))

    def addTabulatedFunction(self, name, function):
        """Recorded; a Context refuses the force by name (the hydrogen-bond kernel runs no tabulated functions)."""
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    addFunction = addTabulatedFunction

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    getNumFunctions = getNumTabulatedFunctions

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        if int(method) not in (self.NoCutoff, self.CutoffNonPeriodic, self.CutoffPeriodic):
            raise OpenMMException('CustomHbondForce: Illegal value for nonbonded method')
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def updateParametersInContext(self, context):
        """Upload the per-donor and per-acceptor parameters again.  The particles, the counts, the text and the exclusions must not
        have changed."""
        context._engine.update_force_parameters(self)


class CustomManyParticleForce(Force, _GlobalParams):
    """Sets of `particlesPerSet` particles: every set of distinct particles no pair of which is excluded and which lies inside the
    cutoff contributes the energy text -- distance, angle and dihedral over p1 p2 ..., the raw coordinates x1 ..., per-particle
    parameters suffixed with the role (sigma1, sigma2, ...) and global parameters.  A Context runs sets of three
    (csrc/manyparticle.hip); the class stores any value."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)
    SinglePermutation, UniqueCentralParticle = range(2)

    def __init__(self, particlesPerSet, energy):
        Force.__init__(self)
        self._init_globals()
        self._per_set = int(particlesPerSet)
        self._energy = str(energy)
        self._pnames = []
        self._particles = []       # [[parameters], type]
        self._exclusions = []
        self._filters = {}         # role index -> set of types; a role without an entry takes every type
        self._functions = []
        self._method = self.NoCutoff
        self._mode = self.SinglePermutation
        self._cutoff = 1.0

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def getNumParticlesPerSet(self):
        return self._per_set

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = str(energy)

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        if int(method) not in (self.NoCutoff, self.CutoffNonPeriodic, self.CutoffPeriodic):
            raise OpenMMException('CustomManyParticleForce: Illegal value for nonbonded method')
        self._method = int(method)

    def getPermutationMode(self):
        return self._mode

    def setPermutationMode(self, mode):
        if int(mode) not in (self.SinglePermutation, self.UniqueCentralParticle):
            raise OpenMMException('CustomManyParticleForce: Illegal value for permutation mode')
        self._mode = int(mode)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def addPerParticleParameter(self, name):
        self._pnames.append(str(name))
        return len(self._pnames) - 1

    def getNumPerParticleParameters(self):
        return len(self._pnames)

    def getPerParticleParameterName(self, index):
        return self._pnames[index]

    def setPerParticleParameterName(self, index, name):
        self._pnames[index] = str(name)

    def setGlobalParameterName(self, index, name):
        self._gnames[index] = str(name)

    def addParticle(self, parameters=(), type=0):
        self._particles.append([[float(md_value(p)) for p in parameters], int(type)])
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        p, t = self._particles[index]
        return [tuple(p), t]

    def setParticleParameters(self, index, parameters, type=0):
        self._particles[index] = [[float(md_value(p)) for p in parameters], int(type)]

    def addExclusion(self, particle1, particle2):
        self._exclusions.append((int(particle1), int(particle2)))
        return len(self._exclusions) - 1

    def getNumExclusions(self):
        return len(self._exclusions)

    def getExclusionParticles(self, index):
        return list(self._exclusions[index])

    def setExclusionParticles(self, index, particle1, particle2):
        self._exclusions[index] = (int(particle1), int(particle2))

    def createExclusionsFromBonds(self, bonds, bondCutoff):
        """Exclude every pair of particles that at most `bondCutoff` bonds separate."""
        if int(bondCutoff) < 1:
            return
        n = len(self._particles)
        partners = [set() for _ in range(n)]
        for a, b in bonds:
            a, b = int(a), int(b)
            if not (0 <= a < n and 0 <= b < n):
                raise OpenMMException('createExclusionsFromBonds: Illegal particle index in list of bonds')
            partners[a].add(b)
            partners[b].add(a)
        have = {(min(a, b), max(a, b)) for a, b in self._exclusions}
        for start in range(n):
            reached, frontier = {start}, {start}
            for _ in range(int(bondCutoff)):
                frontier = {b for a in frontier for b in partners[a]} - reached
                reached |= frontier
            for other in sorted(reached):
                if other > start and (start, other) not in have:
                    have.add((start, other))
                    self.addExclusion(start, other)

    def getTypeFilter(self, index):
        """The types the particle in role `index` may have; an empty set: any."""
        if not 0 <= int(index) < self._per_set:
            raise OpenMMException('CustomManyParticleForce: Index out of range')
        return set(self._filters.get(int(index), ()))

    def setTypeFilter(self, index, types):
        if not 0 <= int(index) < self._per_set:
            raise OpenMMException('CustomManyParticleForce: Index out of range')
        self._filters[int(index)] = {int(t) for t in types}

    def addTabulatedFunction(self, name, function):
        """Recorded; a Context refuses the force by name (the many-particle kernel runs no tabulated functions)."""
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    addFunction = addTabulatedFunction

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    getNumFunctions = getNumTabulatedFunctions

    def getTabulatedFunction(self, index):
        return self._functions[index][1]

    def getTabulatedFunctionName(self, index):
        return self._functions[index][0]

    def updateParametersInContext(self, context):
        """Upload the per-particle parameters, the types and the type filters again.  The number of particles, the text and the
        exclusions must not have changed."""
        context._engine.update_force_parameters(self)


class RMSDForce(Force):
    """Energy = the root-mean-square deviation, in nm, of `particles` from `referencePositions` after the optimal rigid superposition
    (translation and proper rotation; csrc/rmsd.hip).  Reference positions are given for EVERY particle of the System,
    with units or in plain nm; an empty particle list means all particles.  Positions are read raw: no periodic image is taken."""

    def __init__(self, referencePositions, particles=()):
        Force.__init__(self)
        self.setReferencePositions(referencePositions)
        self.setParticles(particles)

    def getReferencePositions(self):
        return Quantity([Vec3(*row) for row in self._reference], nm)

    def setReferencePositions(self, positions):
        v = md_value(positions)
        if isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], Quantity):
            v = [md_value(r) for r in v]
        arr = np.array(v, dtype=np.float64)
        if arr.size == 0:
            arr = arr.reshape(0, 3)
        if arr.ndim != 2 or arr.shape[1] != 3:
            raise OpenMMException('RMSDForce: reference positions are one (x, y, z) per particle')
        self._reference = [tuple(float(c) for c in row) for row in arr]

    def getParticles(self):
        return list(self._rmsd_particles)

    def setParticles(self, particles):
        self._rmsd_particles = [int(p) for p in particles]

    def usesPeriodicBoundaryConditions(self):
        return False

    def updateParametersInContext(self, context):
        """Upload the reference positions and the particle list again; their number may have changed."""
        context._engine.update_force_parameters(self)


class GayBerneForce(Force):
    """Ellipsoids with the Gay-Berne pair energy (csrc/gayberne.hip).  A particle's frame: x along r_i - r_xparticle,
    y the part of r_i - r_yparticle perpendicular to it, z = x cross y; the diameters sx, sy, sz and the well-depth scales ex, ey, ez
    belong to those axes.  xparticle = -1 needs a sphere (sx = sy = sz, ex = ey = ez), yparticle = -1 a uniaxial shape (sy = sz,
    ey = ez).  sigma = (sigma1 + sigma2) / 2, epsilon = sqrt(epsilon1 epsilon2) unless an exception gives both; shapes always come
    from the particles.  The torque on an ellipsoid comes back as forces on its x- and y-particle."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic = range(3)

    def __init__(self):
        Force.__init__(self)
        self._particles = []       # [sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez]
        self._exceptions = []      # [i, j, sigma, epsilon]
        self._exc_index = {}
        self._method = self.NoCutoff
        self._cutoff = 1.0
        self._use_switch = False
        self._switch = -1.0

    def usesPeriodicBoundaryConditions(self):
        return self._method == self.CutoffPeriodic

    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        if int(method) not in (self.NoCutoff, self.CutoffNonPeriodic, self.CutoffPeriodic):
            raise OpenMMException('GayBerneForce: Illegal value for nonbonded method')
        self._method = int(method)

    def getCutoffDistance(self):
        return Quantity(self._cutoff, nm)

    def setCutoffDistance(self, distance):
        self._cutoff = float(md_value(distance))

    def getUseSwitchingFunction(self):
        return self._use_switch

    def setUseSwitchingFunction(self, use):
        self._use_switch = bool(use)

    def getSwitchingDistance(self):
        return Quantity(self._switch, nm)

    def setSwitchingDistance(self, distance):
        self._switch = float(md_value(distance))

    @staticmethod
    def _particle_record(sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez):
        return [float(md_value(sigma)), float(md_value(epsilon)), int(xparticle), int(yparticle), float(md_value(sx)), float(md_value(sy)),
                float(md_value(sz)), float(ex), float(ey), float(ez)]

    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez):
        self._particles.append(self._particle_record(sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez))
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        sigma, epsilon, xp, yp, sx, sy, sz, ex, ey, ez = self._particles[index]
        return [Quantity(sigma, nm), Quantity(epsilon, kjmol), xp, yp, Quantity(sx, nm), Quantity(sy, nm), Quantity(sz, nm), ex, ey, ez]

    def setParticleParameters(self, index, sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez):
        self._particles[index] = self._particle_record(sigma, epsilon, xparticle, yparticle, sx, sy, sz, ex, ey, ez)

    def getNumExceptions(self):
        return len(self._exceptions)

    def addException(self, particle1, particle2, sigma, epsilon, replace=False):
        key = (min(particle1, particle2), max(particle1, particle2))
        rec = [int(particle1), int(particle2), float(md_value(sigma)), float(md_value(epsilon))]
        if key in self._exc_index:
            if not replace:
                raise OpenMMException('GayBerneForce: There is already an exception for particles %d and %d' % key)
            self._exceptions[self._exc_index[key]] = rec
            return self._exc_index[key]
        self._exceptions.append(rec)
        self._exc_index[key] = len(self._exceptions) - 1
        return len(self._exceptions) - 1

    def getExceptionParameters(self, index):
        i, j, sigma, epsilon = self._exceptions[index]
        return [i, j, Quantity(sigma, nm), Quantity(epsilon, kjmol)]

    def setExceptionParameters(self, index, particle1, particle2, sigma, epsilon):
        self._exceptions[index] = [int(particle1), int(particle2), float(md_value(sigma)), float(md_value(epsilon))]

    def updateParametersInContext(self, context):
        """Upload the particle and exception parameters again.  The interacting particles, their axis particles and the pairs that
        have an exception must not have changed."""
        context._engine.update_force_parameters(self)


class DrudeForce(Force):
    """Drude oscillators (csrc/drude.hip): a Drude particle hangs on its parent (particle1) by a harmonic spring whose
    stiffness K q^2 / alpha may differ along the directions particle1 - particle2 and particle3 - particle4 (aniso12, aniso34; -1: no
    such particle, the direction is isotropic), and the dipoles of two Drude particles (the particle with its charge, the parent with
    the opposite one) interact with the Thole-screened energy K q_i q_j (1 - (1 + u/2) exp(-u)) / r, u = thole r / (alpha_1 alpha_2)^(1/6)."""

    def __init__(self):
        Force.__init__(self)
        self._particles = []       # [particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12, aniso34]
        self._pairs = []           # [drude1, drude2, thole]
        self._periodic = False

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    @staticmethod
    def _particle_record(particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12, aniso34):
        return [int(particle), int(particle1), int(particle2), int(particle3), int(particle4), float(md_value(charge)),
                float(md_value(polarizability)), float(aniso12), float(aniso34)]

    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12, aniso34):
        self._particles.append(self._particle_record(particle, particle1, particle2, particle3, particle4, charge, polarizability,
                                                     aniso12, aniso34))
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        p, p1, p2, p3, p4, charge, alpha, aniso12, aniso34 = self._particles[index]
        return [p, p1, p2, p3, p4, Quantity(charge, _unit.elementary_charge), Quantity(alpha, nm ** 3), aniso12, aniso34]

    def setParticleParameters(self, index, particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12, aniso34):
        self._particles[index] = self._particle_record(particle, particle1, particle2, particle3, particle4, charge, polarizability,
                                                       aniso12, aniso34)

    def getNumScreenedPairs(self):
        return len(self._pairs)

    def addScreenedPair(self, drude1, drude2, thole):
        self._pairs.append([int(drude1), int(drude2), float(thole)])
        return len(self._pairs) - 1

    def getScreenedPairParameters(self, index):
        return list(self._pairs[index])

    def setScreenedPairParameters(self, index, drude1, drude2, thole):
        self._pairs[index] = [int(drude1), int(drude2), float(thole)]

    def updateParametersInContext(self, context):
        """Upload charges, polarizabilities, anisotropies and Thole factors again.  No particle index may have changed."""
        context._engine.update_force_parameters(self)


class CustomCVForce(Force, _GlobalParams):
    """Energy = function of collective variables, each the energy of an inner Force object."""

    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._cvs = []
        self._derivs = []
        self._functions = []

    def getEnergyFunction(self):
        return self._energy

    def addTabulatedFunction(self, name, function):
        """Stored as OpenMM stores it; the HIP path refuses a CustomCVForce that has one when the Context is created."""
        self._functions.append((name, function))
        return len(self._functions) - 1

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    def getNumEnergyParameterDerivatives(self):
        return len(self._derivs)

    def getEnergyParameterDerivativeName(self, index):
        return self._derivs[index]

    def usesPeriodicBoundaryConditions(self):
        return any(force.usesPeriodicBoundaryConditions() for _, force in self._cvs)

    def getCollectiveVariableValues(self, context):
        """The current values of the collective variables, in the order they were added."""
        return context._engine.collective_variable_values(self)

    def updateParametersInContext(self, context):
        """Reload the inner forces that have a reload of their own (per-term parameters of a generic text)."""
        context._engine.update_force_parameters(self)

    def addCollectiveVariable(self, name, force):
        self._cvs.append((name, copy.deepcopy(force)))
        return len(self._cvs) - 1

    def getNumCollectiveVariables(self):
        return len(self._cvs)

    def getCollectiveVariableName(self, index):
        return self._cvs[index][0]

    def getCollectiveVariable(self, index):
        return self._cvs[index][1]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)


class CustomBondForce(Force, _GlobalParams):
    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._bnames = []
        self._bonds = []
        self._derivs = []
        self._periodic = False

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = energy

    def addPerBondParameter(self, name):
        self._bnames.append(name)
        return len(self._bnames) - 1

    def getNumPerBondParameters(self):
        return len(self._bnames)

    def getPerBondParameterName(self, index):
        return self._bnames[index]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)

    def addBond(self, particle1, particle2, parameters=()):
        self._bonds.append([int(particle1), int(particle2), [float(md_value(p)) for p in parameters]])
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        i, j, p = self._bonds[index]
        return [i, j, tuple(p)]

    def setBondParameters(self, index, particle1, particle2, parameters=()):
        self._bonds[index] = [int(particle1), int(particle2), [float(md_value(p)) for p in parameters]]

    def updateParametersInContext(self, context):
        """Upload the per-bond parameters again (the atoms and the number of bonds must not have changed)."""
        context._engine.update_force_parameters(self)

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic


class HarmonicBondForce(Force):
    def __init__(self):
        Force.__init__(self)
        self._bonds = []
        self._periodic = False

    def addBond(self, particle1, particle2, length, k):
        self._bonds.append([int(particle1), int(particle2), float(md_value(length)), float(md_value(k))])
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        i, j, r0, k = self._bonds[index]
        return [i, j, Quantity(r0, nm), Quantity(k, kjmol / nm ** 2)]

    def setBondParameters(self, index, particle1, particle2, length, k):
        self._bonds[index] = [int(particle1), int(particle2), float(md_value(length)), float(md_value(k))]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic


class CustomAngleForce(Force, _GlobalParams):
    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._anames = []
        self._angles = []
        self._derivs = []
        self._periodic = False

    def getEnergyFunction(self):
        return self._energy

    def addPerAngleParameter(self, name):
        self._anames.append(name)
        return len(self._anames) - 1

    def getNumPerAngleParameters(self):
        return len(self._anames)

    def getPerAngleParameterName(self, index):
        return self._anames[index]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)

    def addAngle(self, particle1, particle2, particle3, parameters=()):
        self._angles.append([int(particle1), int(particle2), int(particle3), [float(md_value(p)) for p in parameters]])
        return len(self._angles) - 1

    def getNumAngles(self):
        return len(self._angles)

    def getAngleParameters(self, index):
        i, j, k, p = self._angles[index]
        return [i, j, k, tuple(p)]

    def setAngleParameters(self, index, particle1, particle2, particle3, parameters=()):
        self._angles[index] = [int(particle1), int(particle2), int(particle3), [float(md_value(p)) for p in parameters]]

    def setEnergyFunction(self, energy):
        self._energy = energy

    def updateParametersInContext(self, context):
        """Upload the per-angle parameters again (the atoms and the number of angles must not have changed)."""
        context._engine.update_force_parameters(self)

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic


class HarmonicAngleForce(Force):
    def __init__(self):
        Force.__init__(self)
        self._angles = []
        self._periodic = False

    def addAngle(self, particle1, particle2, particle3, angle, k):
        self._angles.append([int(particle1), int(particle2), int(particle3), float(md_value(angle)), float(md_value(k))])
        return len(self._angles) - 1

    def getNumAngles(self):
        return len(self._angles)

    def getAngleParameters(self, index):
        i, j, k_, t0, k = self._angles[index]
        return [i, j, k_, Quantity(t0, _unit.radian), Quantity(k, kjmol / _unit.radian ** 2)]

    def setAngleParameters(self, index, particle1, particle2, particle3, angle, k):
        self._angles[index] = [int(particle1), int(particle2), int(particle3), float(md_value(angle)), float(md_value(k))]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic


class PeriodicTorsionForce(Force):
    def __init__(self):
        Force.__init__(self)
        self._torsions = []
        self._periodic = False

    def addTorsion(self, p1, p2, p3, p4, periodicity, phase, k):
        self._torsions.append([int(p1), int(p2), int(p3), int(p4), int(periodicity), float(md_value(phase)),
                               float(md_value(k))])
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        a, b, c, d, n, ph, k = self._torsions[index]
        return [a, b, c, d, n, Quantity(ph, _unit.radian), Quantity(k, kjmol)]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic


class RBTorsionForce(Force):
    """Ryckaert-Bellemans torsions: E = sum_n c_n cos(psi)^n, n = 0 .. 5, with psi = phi - pi and phi the dihedral of
    PeriodicTorsionForce (so cos(psi) = -cos(phi)).  Lowered to the term-expression kernel (translate/terms.py: translate_rb)."""

    def __init__(self):
        Force.__init__(self)
        self._torsions = []
        self._periodic = False

    @staticmethod
    def _row(p1, p2, p3, p4, c):
        if len(c) != 6:
            raise OpenMMException('RBTorsionForce: a torsion takes the six coefficients c0 .. c5 (%d given)' % len(c))
        return [int(p1), int(p2), int(p3), int(p4)] + [float(md_value(v)) for v in c]

    def addTorsion(self, particle1, particle2, particle3, particle4, c0, c1, c2, c3, c4, c5):
        self._torsions.append(self._row(particle1, particle2, particle3, particle4, (c0, c1, c2, c3, c4, c5)))
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        row = self._torsions[index]
        return row[:4] + [Quantity(v, kjmol) for v in row[4:]]

    def setTorsionParameters(self, index, particle1, particle2, particle3, particle4, c0, c1, c2, c3, c4, c5):
        self._torsions[index] = self._row(particle1, particle2, particle3, particle4, (c0, c1, c2, c3, c4, c5))

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def updateParametersInContext(self, context):
        """Upload the coefficients again (the atoms and the number of torsions must not have changed)."""
        context._engine.update_force_parameters(self)


class CMAPTorsionForce(Force):
    """Pairs of dihedrals (phi, psi) whose energy is read from a map over [0, 2 pi)^2 by bicubic interpolation: the tensor-product
    periodic cubic spline through the map's values (tables.cmap_coefficients; csrc/cmap.hip).  A map of size n holds n * n values in
    kJ/mol, energy[i + n * j] at phi = 2 pi i / n and psi = 2 pi j / n: the first angle runs fastest."""

    def __init__(self):
        Force.__init__(self)
        self._maps = []             # [size, [size * size values]]
        self._torsions = []         # [map, a1, a2, a3, a4, b1, b2, b3, b4]
        self._periodic = False

    @staticmethod
    def _map(size, energy):
        size = int(size)
        if isinstance(energy, Quantity):
            energy = Quantity(np.asarray(energy._value, dtype=np.float64), energy.unit)
        energy = [float(v) for v in np.asarray(md_value(energy), dtype=np.float64).reshape(-1)]
        if size < 2:
            raise OpenMMException('CMAPTorsionForce: the size of a map must be at least 2')
        if len(energy) != size * size:
            raise OpenMMException('CMAPTorsionForce: a map of size %d takes %d energies (%d given)' % (size, size * size, len(energy)))
        return [size, energy]

    def addMap(self, size, energy):
        self._maps.append(self._map(size, energy))
        return len(self._maps) - 1

    def getNumMaps(self):
        return len(self._maps)

    def getMapParameters(self, index):
        size, energy = self._maps[index]
        return [size, Quantity(list(energy), kjmol)]

    def setMapParameters(self, index, size, energy):
        self._maps[index] = self._map(size, energy)

    def addTorsion(self, map, a1, a2, a3, a4, b1, b2, b3, b4):
        self._torsions.append([int(v) for v in (map, a1, a2, a3, a4, b1, b2, b3, b4)])
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        return list(self._torsions[index])

    def setTorsionParameters(self, index, map, a1, a2, a3, a4, b1, b2, b3, b4):
        self._torsions[index] = [int(v) for v in (map, a1, a2, a3, a4, b1, b2, b3, b4)]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def updateParametersInContext(self, context):
        """Upload the maps' values and the torsions' map indices again.  The number of maps, a map's size, the number of torsions and
        a torsion's atoms must not have changed."""
        context._engine.update_force_parameters(self)


class CustomTorsionForce(Force, _GlobalParams):
    """Torsions with any energy text in `theta`, the dihedral angle in (-pi, pi] (PeriodicTorsionForce's convention)."""

    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._tnames = []
        self._derivs = []
        self._torsions = []
        self._periodic = False

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = energy

    def addPerTorsionParameter(self, name):
        self._tnames.append(name)
        return len(self._tnames) - 1

    def getNumPerTorsionParameters(self):
        return len(self._tnames)

    def getPerTorsionParameterName(self, index):
        return self._tnames[index]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)

    def addTorsion(self, particle1, particle2, particle3, particle4, parameters=()):
        self._torsions.append([int(particle1), int(particle2), int(particle3), int(particle4), [float(md_value(p)) for p in parameters]])
        return len(self._torsions) - 1

    def getNumTorsions(self):
        return len(self._torsions)

    def getTorsionParameters(self, index):
        a, b, c, d, p = self._torsions[index]
        return [a, b, c, d, tuple(p)]

    def setTorsionParameters(self, index, particle1, particle2, particle3, particle4, parameters=()):
        self._torsions[index] = [int(particle1), int(particle2), int(particle3), int(particle4), [float(md_value(p)) for p in parameters]]

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def updateParametersInContext(self, context):
        """Upload the per-torsion parameters again (the atoms and the number of torsions must not have changed)."""
        context._engine.update_force_parameters(self)


class CustomExternalForce(Force, _GlobalParams):
    """A force on single particles with any energy text in their coordinates x, y, z (as the positions give them: never periodic)."""

    def __init__(self, energy):
        Force.__init__(self)
        self._init_globals()
        self._energy = energy
        self._pnames = []
        self._particles = []
        self._derivs = []

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = energy

    def addPerParticleParameter(self, name):
        self._pnames.append(name)
        return len(self._pnames) - 1

    def getNumPerParticleParameters(self):
        return len(self._pnames)

    def getPerParticleParameterName(self, index):
        return self._pnames[index]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)

    def addParticle(self, particle, parameters=()):
        self._particles.append([int(particle), [float(md_value(p)) for p in parameters]])
        return len(self._particles) - 1

    def getNumParticles(self):
        return len(self._particles)

    def getParticleParameters(self, index):
        i, p = self._particles[index]
        return [i, tuple(p)]

    def setParticleParameters(self, index, particle, parameters=()):
        self._particles[index] = [int(particle), [float(md_value(p)) for p in parameters]]

    def updateParametersInContext(self, context):
        """Upload the per-particle parameters again (the atoms and the number of particles must not have changed)."""
        context._engine.update_force_parameters(self)


class _CompoundBonds(Force, _GlobalParams):
    """What CustomCompoundBondForce and CustomCentroidBondForce share: the energy text, per-bond and global parameters, the bonds
    (each a list of particles or groups plus parameters), stored tabulated functions and derivative names (both refused at
    translation), the periodic flag."""

    def __init__(self, number, energy):
        Force.__init__(self)
        self._init_globals()
        self._n = int(number)
        self._energy = energy
        self._bnames = []
        self._bonds = []           # [[slot entries], [parameters]]
        self._derivs = []
        self._functions = []
        self._periodic = False

    def getEnergyFunction(self):
        return self._energy

    def setEnergyFunction(self, energy):
        self._energy = energy

    def addPerBondParameter(self, name):
        self._bnames.append(name)
        return len(self._bnames) - 1

    def getNumPerBondParameters(self):
        return len(self._bnames)

    def getPerBondParameterName(self, index):
        return self._bnames[index]

    def addEnergyParameterDerivative(self, name):
        self._derivs.append(name)

    def getNumEnergyParameterDerivatives(self):
        return len(self._derivs)

    def addTabulatedFunction(self, name, function):
        self._functions.append((str(name), function))
        return len(self._functions) - 1

    def getNumTabulatedFunctions(self):
        return len(self._functions)

    def _row(self, members, parameters):
        members = [int(m) for m in members]
        if len(members) != self._n:
            raise OpenMMException('%s: a bond takes %d %s (%d given)' % (self.__class__.__name__, self._n, self._unit, len(members)))
        return [members, [float(md_value(p)) for p in parameters]]

    def addBond(self, members, parameters=()):
        self._bonds.append(self._row(members, parameters))
        return len(self._bonds) - 1

    def getNumBonds(self):
        return len(self._bonds)

    def getBondParameters(self, index):
        members, p = self._bonds[index]
        return [tuple(members), tuple(p)]

    def setBondParameters(self, index, members, parameters=()):
        self._bonds[index] = self._row(members, parameters)

    def setUsesPeriodicBoundaryConditions(self, periodic):
        self._periodic = bool(periodic)

    def usesPeriodicBoundaryConditions(self):
        return self._periodic

    def updateParametersInContext(self, context):
        """Upload the per-bond parameters (and group weights) again; the members and the number of bonds must not have changed."""
        context._engine.update_force_parameters(self)


class CustomCompoundBondForce(_CompoundBonds):
    """Bonds over N particles p1 .. pN with any energy text in x1, y1, z1 .. zN (raw coordinates), distance(pa,pb), angle(pa,pb,pc)
    and dihedral(pa,pb,pc,pd), per-bond and global parameters."""
    _unit = 'particles'

    def __init__(self, numParticles, energy):
        _CompoundBonds.__init__(self, numParticles, energy)

    def getNumParticlesPerBond(self):
        return self._n


class CustomCentroidBondForce(_CompoundBonds):
    """Bonds over N groups g1 .. gN, each the weighted centre of a set of particles; the text is CustomCompoundBondForce's with g
    names, x1 .. the coordinates of the centre of group 1."""
    _unit = 'groups'

    def __init__(self, numGroups, energy):
        _CompoundBonds.__init__(self, numGroups, energy)
        self._groups = []           # [[particles], [weights]]; no weights: the particles' masses

    def getNumGroupsPerBond(self):
        return self._n

    def addGroup(self, particles, weights=()):
        particles, weights = [int(p) for p in particles], [float(md_value(w)) for w in (weights or ())]
        if weights and len(weights) != len(particles):
            raise OpenMMException('CustomCentroidBondForce: a group needs one weight per particle, or none (the masses)')
        self._groups.append([particles, weights])
        return len(self._groups) - 1

    def getNumGroups(self):
        return len(self._groups)

    def getGroupParameters(self, index):
        particles, weights = self._groups[index]
        return [tuple(particles), tuple(weights)]

    def setGroupParameters(self, index, particles, weights=()):
        particles, weights = [int(p) for p in particles], [float(md_value(w)) for w in (weights or ())]
        if weights and len(weights) != len(particles):
            raise OpenMMException('CustomCentroidBondForce: a group needs one weight per particle, or none (the masses)')
        self._groups[index] = [particles, weights]


class CMMotionRemover(Force):
    """Accepted and ignored (removes centre-of-mass motion in OpenMM; no energy)."""

    def __init__(self, frequency=1):
        Force.__init__(self)
        self._frequency = frequency


class MonteCarloBarostat(Force):
    """openmm.MonteCarloBarostat: isotropic Monte Carlo volume moves at constant pressure [OpenMM: MonteCarloBarostatImpl.cpp].
    Every `frequency` steps the Context scales the centres of its molecules (Context.getMolecules()) and the box by
    s = ((V + dV) / V)^(1/3), dV uniform in +-volumeScale, and keeps the move with probability min(1, exp(-w / kT)),
    w = dE + P dV - N_molecules kT ln((V + dV) / V); a rejected move restores positions and box bit for bit.  volumeScale starts at
    1 % of the volume and follows the acceptance rate (below 25 % of ten attempts: / 1.1, above 75 %: x 1.1, at most 0.3 V).
    The attempt is made where the step program has its UpdateContextState step -- here: before the step (Engine.step), which is the
    same thing for every program that neither moves x nor reads a force or an energy ahead of that step; other programs are refused
    when the Context is created.  The random numbers are numpy's (default_rng(seed); seed 0: entropy), not OpenMM's stream: one draw
    for dV per attempt, one for the Metropolis test only when w > 0.  No energy of its own; the engine skips it like CMMotionRemover."""

    def __init__(self, defaultPressure, defaultTemperature, frequency=25):
        Force.__init__(self)
        self.setDefaultPressure(defaultPressure)
        self.setDefaultTemperature(defaultTemperature)
        self.setFrequency(frequency)
        self._seed = 0

    @staticmethod
    def Pressure():
        return 'MonteCarloPressure'

    @staticmethod
    def Temperature():
        return 'MonteCarloTemperature'

    def getDefaultPressure(self):
        return Quantity(self._pressure, _unit.bar)

    def setDefaultPressure(self, pressure):
        self._pressure = float(pressure.value_in_unit(_unit.bar) if isinstance(pressure, Quantity) else pressure)

    def getDefaultTemperature(self):
        return Quantity(self._temperature, _unit.kelvin)

    def setDefaultTemperature(self, temperature):
        self._temperature = float(md_value(temperature, _unit.kelvin))

    def getFrequency(self):
        return self._frequency

    def setFrequency(self, frequency):
        """Steps between two attempts; 0 disables the barostat."""
        if int(frequency) < 0:
            raise OpenMMException('MonteCarloBarostat: the frequency must not be negative')
        self._frequency = int(frequency)

    def getRandomNumberSeed(self):
        return self._seed

    def setRandomNumberSeed(self, seed):
        self._seed = int(seed)

    def usesPeriodicBoundaryConditions(self):
        return False


# ------------------------------------------------------------------------------------------------ virtual sites
class VirtualSite:
    """openmm.VirtualSite: a massless particle whose position is computed from other particles (System.setVirtualSite)."""
    _kind = -1

    def __init__(self, particles, weights):
        self._particles = tuple(int(p) for p in particles)
        self._weights = tuple(float(w) for w in weights)

    def getNumParticles(self):
        return len(self._particles)

    def getParticle(self, particle):
        return self._particles[particle]


class TwoParticleAverageSite(VirtualSite):
    """s = w1 r1 + w2 r2"""
    _kind = 0

    def __init__(self, particle1, particle2, weight1, weight2):
        super().__init__((particle1, particle2), (weight1, weight2))

    def getWeight(self, particle):
        return self._weights[particle]


class ThreeParticleAverageSite(VirtualSite):
    """s = w1 r1 + w2 r2 + w3 r3"""
    _kind = 1

    def __init__(self, particle1, particle2, particle3, weight1, weight2, weight3):
        super().__init__((particle1, particle2, particle3), (weight1, weight2, weight3))

    def getWeight(self, particle):
        return self._weights[particle]


class OutOfPlaneSite(VirtualSite):
    """s = r1 + w12 r12 + w13 r13 + wCross (r12 x r13), r12 = r2 - r1, r13 = r3 - r1"""
    _kind = 2

    def __init__(self, particle1, particle2, particle3, weight12, weight13, weightCross):
        super().__init__((particle1, particle2, particle3), (weight12, weight13, weightCross))

    def getWeight12(self):
        return self._weights[0]

    def getWeight13(self):
        return self._weights[1]

    def getWeightCross(self):
        return self._weights[2]


class LocalCoordinatesSite(VirtualSite):
    """Exists so that a script that names it fails with a message of its own: the HIP path has no such site."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError('LocalCoordinatesSite is not supported by the HIP path (TwoParticleAverageSite, '
                                  'ThreeParticleAverageSite and OutOfPlaneSite are)')


def check_virtual_sites(system):
    """What OpenMM checks when a Context is created over a System with virtual sites or massless particles."""
    n = system.getNumParticles()
    sites = getattr(system, '_vsites', {})
    for index, site in sorted(sites.items()):
        if system._masses[index] != 0.0:
            raise OpenMMException('Virtual site %d has nonzero mass (%g)' % (index, system._masses[index]))
        for k in range(site.getNumParticles()):
            p = site.getParticle(k)
            if not 0 <= p < n:
                raise OpenMMException('Virtual site %d: particle index %d is out of range' % (index, p))
            if p in sites:
                raise OpenMMException('Virtual site %d depends on particle %d, which is a virtual site itself' % (index, p))
            if p == index or p in [site.getParticle(j) for j in range(k)]:
                raise OpenMMException('Virtual site %d names particle %d twice' % (index, p))
    for p1, p2, _ in system._constraints:
        for p in (p1, p2):
            if p in sites:
                raise OpenMMException('A constraint cannot involve a virtual site (particle %d)' % p)
            if 0 <= p < n and system._masses[p] == 0.0:
                raise OpenMMException('A constraint cannot involve a massless particle (particle %d)' % p)


# ------------------------------------------------------------------------------------------------ system
class System:
    def __init__(self):
        self._masses = []
        self._forces = []
        self._box = None
        self._constraints = []
        self._vsites = {}

    def setVirtualSite(self, index, virtualSite):
        index = int(index)
        if not 0 <= index < len(self._masses):
            raise OpenMMException('setVirtualSite: particle index %d is out of range' % index)
        if not isinstance(virtualSite, VirtualSite):
            raise TypeError('setVirtualSite: a VirtualSite is expected')
        self._vsites[index] = virtualSite

    def isVirtualSite(self, index):
        return int(index) in self._vsites

    def getVirtualSite(self, index):
        if int(index) not in self._vsites:
            raise OpenMMException('This particle is not a virtual site')
        return self._vsites[int(index)]

    def addParticle(self, mass):
        self._masses.append(float(md_value(mass)))
        return len(self._masses) - 1

    def getNumParticles(self):
        return len(self._masses)

    def getParticleMass(self, index):
        return Quantity(self._masses[index], _unit.dalton)

    def setParticleMass(self, index, mass):
        self._masses[index] = float(md_value(mass))

    def addForce(self, force):
        self._forces.append(force)
        return len(self._forces) - 1

    def getNumForces(self):
        return len(self._forces)

    def getForce(self, index):
        return self._forces[index]

    def getForces(self):
        return list(self._forces)

    def removeForce(self, index):
        del self._forces[index]

    def getNumConstraints(self):
        return len(self._constraints)

    def addConstraint(self, p1, p2, distance):
        self._constraints.append((int(p1), int(p2), float(md_value(distance))))
        return len(self._constraints) - 1

    def setDefaultPeriodicBoxVectors(self, a, b, c):
        vecs = []
        for v in (a, b, c):
            v = md_value(v)
            vecs.append(tuple(float(md_value(x)) for x in v))
        self._box = tuple(vecs)

    def getDefaultPeriodicBoxVectors(self):
        if self._box is None:
            raise OpenMMException('System has no periodic box')
        return [Quantity(Vec3(*v), nm) for v in self._box]

    def usesPeriodicBoundaryConditions(self):
        return any(f.usesPeriodicBoundaryConditions() for f in self._forces)

    def _copy_from(self, other):
        clone = copy.deepcopy(other)
        self.__dict__.update(clone.__dict__)


# ------------------------------------------------------------------------------------------------ integrators
class Integrator:
    def __init__(self, stepSize):
        self._dt = float(md_value(stepSize))
        self._context = None
        self._seed = 0

    def getConstraintTolerance(self):
        return getattr(self, '_ctol', 1e-5)

    def setConstraintTolerance(self, tol):
        self._ctol = float(tol)

    def getStepSize(self):
        return Quantity(self._dt, _unit.picosecond)

    def setStepSize(self, stepSize):
        self._dt = float(md_value(stepSize))
        if self._context is not None:
            self._context._engine.invalidate_program()

    def setRandomNumberSeed(self, seed):
        self._seed = int(seed)

    def getRandomNumberSeed(self):
        return self._seed

    def step(self, steps):
        if self._context is None:
            raise OpenMMException('This Integrator is not bound to a context!')
        self._context._engine.step(int(steps))


class _StockIntegrator(Integrator):
    """OpenMM's stock integrators: the engine runs their step as `EVAL ; STOCK` -- one launch for the whole post-force update
    (csrc/stock.hip) -- or, with its `stock_native` switch off, as the CustomIntegrator program `_program` returns."""
    _stock_kind = None              # backend.STOCK_*

    def __init__(self, stepSize, temperature=0.0, frictionCoeff=0.0):
        Integrator.__init__(self, stepSize)
        self._temperature = float(md_value(temperature))
        self._friction = float(md_value(frictionCoeff))

    def _changed(self):
        if self._context is not None:
            self._context._engine.invalidate_program()

    def setConstraintTolerance(self, tol):
        Integrator.setConstraintTolerance(self, tol)
        if self._context is not None:
            self._context._engine.set_constraint_tolerance(self._ctol)

    def setRandomNumberSeed(self, seed):
        Integrator.setRandomNumberSeed(self, seed)
        self._changed()

    def _kT(self):
        return _unit.BOLTZMANN_CONSTANT_kB._value * self._temperature

    def _new_program(self):
        prog = CustomIntegrator(self._dt)
        prog._seed = self._seed
        prog._ctol = self.getConstraintTolerance()
        prog.addUpdateContextState()
        return prog

    @staticmethod
    def _leapfrog_tail(prog):
        """x0 <- x ; x <- x + dt v ; constrain ; v <- (x - x0)/dt: how the leapfrog kinds end."""
        prog.addComputePerDof('x0', 'x')
        prog.addComputePerDof('x', 'x+dt*v')
        prog.addConstrainPositions()
        prog.addComputePerDof('v', '(x-x0)/dt')


class _ThermostatedIntegrator(_StockIntegrator):
    def __init__(self, temperature, frictionCoeff, stepSize):
        _StockIntegrator.__init__(self, stepSize, temperature, frictionCoeff)
        if self._temperature < 0 or self._friction < 0:
            raise OpenMMException('%s: the temperature and the friction coefficient must not be negative' % type(self).__name__)

    def getTemperature(self):
        return Quantity(self._temperature, _unit.kelvin)

    def setTemperature(self, temperature):
        self._temperature = float(md_value(temperature))
        self._changed()

    def getFriction(self):
        return Quantity(self._friction, _unit.dimensionless / _unit.picosecond)

    def setFriction(self, frictionCoeff):
        self._friction = float(md_value(frictionCoeff))
        self._changed()


class VerletIntegrator(_StockIntegrator):
    """openmm.VerletIntegrator(stepSize): leapfrog Verlet.  (With step size 0 it serves the reference's static energy checks.)"""
    _stock_kind = 0

    def __init__(self, stepSize):
        _StockIntegrator.__init__(self, stepSize)

    def _program(self):
        prog = self._new_program()
        prog.addPerDofVariable('x0', 0)
        prog.addComputePerDof('v', 'v+dt*f/m')
        self._leapfrog_tail(prog)
        return prog


class LangevinMiddleIntegrator(_ThermostatedIntegrator):
    """openmm.LangevinMiddleIntegrator(temperature, frictionCoeff, stepSize): the LFMiddle discretisation (Zhang et al. 2019)."""
    _stock_kind = 1

    def _program(self):
        prog = self._new_program()
        prog.addGlobalVariable('kT', self._kT())
        prog.addGlobalVariable('friction', self._friction)
        prog.addPerDofVariable('x1', 0)
        prog.addComputePerDof('v', 'v+dt*f/m')
        prog.addConstrainVelocities()
        prog.addComputePerDof('x', 'x+0.5*dt*v')
        prog.addComputePerDof('v', 'z*v + sqrt(kT*(1 - z*z)/mass)*gaussian; mass=m; z=exp(-(1.0*dt)*friction)')
        prog.addComputePerDof('x', 'x+0.5*dt*v')
        prog.addComputePerDof('x1', 'x')
        prog.addConstrainPositions()
        prog.addComputePerDof('v', 'v+(x-x1)/dt')
        return prog


class LangevinIntegrator(_ThermostatedIntegrator):
    """openmm.LangevinIntegrator(temperature, frictionCoeff, stepSize): the leapfrog Langevin scheme of OpenMM before 7.5's default."""
    _stock_kind = 2

    def _program(self):
        prog = self._new_program()
        vscale = math.exp(-self._friction * self._dt)
        prog.addGlobalVariable('kT', self._kT())
        prog.addGlobalVariable('vscale', vscale)
        prog.addGlobalVariable('fscale', (1.0 - vscale) / self._friction if self._friction > 0 else self._dt)
        prog.addPerDofVariable('x0', 0)
        prog.addComputePerDof('v', 'vscale*v+fscale*f/m+sqrt(kT*(1-vscale*vscale)/m)*gaussian')
        self._leapfrog_tail(prog)
        return prog


class BrownianIntegrator(_ThermostatedIntegrator):
    """openmm.BrownianIntegrator(temperature, frictionCoeff, stepSize): overdamped dynamics; the velocities are (x' - x)/dt."""
    _stock_kind = 3

    def __init__(self, temperature, frictionCoeff, stepSize):
        _ThermostatedIntegrator.__init__(self, temperature, frictionCoeff, stepSize)
        if not self._friction > 0:
            raise OpenMMException('BrownianIntegrator: the friction coefficient must be positive')

    def setFriction(self, frictionCoeff):
        if not float(md_value(frictionCoeff)) > 0:
            raise OpenMMException('BrownianIntegrator: the friction coefficient must be positive')
        _ThermostatedIntegrator.setFriction(self, frictionCoeff)

    def _program(self):
        prog = self._new_program()
        prog.addGlobalVariable('fscale', self._dt / self._friction)
        prog.addGlobalVariable('noisevar', 2.0 * self._kT() * self._dt / self._friction)
        prog.addPerDofVariable('x0', 0)
        prog.addComputePerDof('x0', 'x')
        prog.addComputePerDof('x', 'x+fscale*f/m+sqrt(noisevar/m)*gaussian')
        prog.addConstrainPositions()
        prog.addComputePerDof('v', '(x-x0)/dt')
        return prog


class DrudeLangevinIntegrator(LangevinIntegrator):
    """openmm.DrudeLangevinIntegrator(temperature, frictionCoeff, drudeTemperature, drudeFrictionCoeff, stepSize): the leapfrog
    Langevin scheme with two thermostats -- every Drude pair of the System's one DrudeForce is thermalised at `temperature` in its
    centre of mass and at `drudeTemperature` in its relative coordinate -- and an optional hard wall on the pair distance.  The engine
    runs the step as `EVAL ; DRUDE_STEP`, one launch for the whole post-force update (csrc/drude.hip); there is no
    op-by-op form of it (`_program` is the plain Langevin step, which the engine uses for its checks only)."""
    _drude = True

    def __init__(self, temperature, frictionCoeff, drudeTemperature, drudeFrictionCoeff, stepSize):
        LangevinIntegrator.__init__(self, temperature, frictionCoeff, stepSize)
        self._drude_temperature = float(md_value(drudeTemperature))
        self._drude_friction = float(md_value(drudeFrictionCoeff))
        self._max_drude_distance = 0.0
        if self._drude_temperature < 0 or self._drude_friction < 0:
            raise OpenMMException('DrudeLangevinIntegrator: the Drude temperature and friction coefficient must not be negative')

    def getDrudeTemperature(self):
        return Quantity(self._drude_temperature, _unit.kelvin)

    def setDrudeTemperature(self, temperature):
        self._drude_temperature = float(md_value(temperature))
        self._changed()

    def getDrudeFriction(self):
        return Quantity(self._drude_friction, _unit.dimensionless / _unit.picosecond)

    def setDrudeFriction(self, frictionCoeff):
        self._drude_friction = float(md_value(frictionCoeff))
        self._changed()

    def getMaxDrudeDistance(self):
        return Quantity(self._max_drude_distance, nm)

    def setMaxDrudeDistance(self, distance):
        distance = float(md_value(distance))
        if distance < 0:
            raise OpenMMException('DrudeLangevinIntegrator: the maximum Drude distance must not be negative')
        self._max_drude_distance = distance
        self._changed()

    def _drude_kT(self):
        return _unit.BOLTZMANN_CONSTANT_kB._value * self._drude_temperature

    def _bound(self):
        if self._context is None:
            raise OpenMMException('This Integrator is not bound to a context!')
        return self._context._engine

    def computeSystemTemperature(self):
        """The temperature of the ordinary atoms and of the pairs' centres of mass: one read of the stored velocities."""
        return Quantity(self._bound().drude_temperatures()[0], _unit.kelvin)

    def computeDrudeTemperature(self):
        """The temperature of the pairs' relative motion: one read of the stored velocities."""
        return Quantity(self._bound().drude_temperatures()[1], _unit.kelvin)



class CustomIntegrator(Integrator):
    ComputeGlobal, ComputePerDof, ComputeSum, ConstrainPositions, ConstrainVelocities, UpdateContextState, \
        IfBlock, WhileBlock, EndBlock = range(9)

    def __init__(self, stepSize):
        Integrator.__init__(self, stepSize)
        self._gnames, self._gvalues = [], []
        self._pnames, self._pvalues = [], []
        self._steps = []
        self._kinetic = None

    # variables
    def addGlobalVariable(self, name, initialValue):
        self._gnames.append(name)
        self._gvalues.append(float(md_value(initialValue)))
        return len(self._gnames) - 1

    def getNumGlobalVariables(self):
        return len(self._gnames)

    def getGlobalVariableName(self, index):
        return self._gnames[index]

    def getGlobalVariable(self, index):
        return self._gvalues[index]

    def getGlobalVariableByName(self, name):
        return self._gvalues[self._gnames.index(name)]

    def setGlobalVariable(self, index, value):
        self._gvalues[index] = float(md_value(value))
        if self._context is not None:
            self._context._engine.invalidate_program()

    def setGlobalVariableByName(self, name, value):
        self.setGlobalVariable(self._gnames.index(name), value)

    def addPerDofVariable(self, name, initialValue):
        self._pnames.append(name)
        self._pvalues.append(float(md_value(initialValue)))
        return len(self._pnames) - 1

    def getNumPerDofVariables(self):
        return len(self._pnames)

    def getPerDofVariableName(self, index):
        return self._pnames[index]

    def getPerDofVariableByName(self, name):
        idx = self._pnames.index(name)
        if self._context is not None:
            return self._context._engine.get_per_dof(name)
        n = getattr(self, '_n_hint', 0)
        return [Vec3(self._pvalues[idx], self._pvalues[idx], self._pvalues[idx]) for _ in range(n)]

    def getPerDofVariable(self, index):
        return self.getPerDofVariableByName(self._pnames[index])

    def setPerDofVariableByName(self, name, values):
        if self._context is not None:
            self._context._engine.set_per_dof(name, values)

    # program
    def _add(self, kind, target='', expr=''):
        self._steps.append((kind, target, expr))
        return len(self._steps) - 1

    def addComputeGlobal(self, variable, expression):
        return self._add(self.ComputeGlobal, variable, expression)

    def addComputePerDof(self, variable, expression):
        return self._add(self.ComputePerDof, variable, expression)

    def addComputeSum(self, variable, expression):
        return self._add(self.ComputeSum, variable, expression)

    def addConstrainPositions(self):
        return self._add(self.ConstrainPositions)

    def addConstrainVelocities(self):
        return self._add(self.ConstrainVelocities)

    def addUpdateContextState(self):
        return self._add(self.UpdateContextState)

    def beginIfBlock(self, condition):
        return self._add(self.IfBlock, '', condition)

    def beginWhileBlock(self, condition):
        return self._add(self.WhileBlock, '', condition)

    def endBlock(self):
        return self._add(self.EndBlock)

    def setKineticEnergyExpression(self, expression):
        """The per-DOF expression whose sum State.getKineticEnergy() reports (default: m*v*v/2)."""
        self._kinetic = expression
        if self._context is not None:
            self._context._engine.invalidate_program()

    def getKineticEnergyExpression(self):
        return self._kinetic if self._kinetic is not None else 'm*v*v/2'

    def getNumComputations(self):
        return len(self._steps)

    def getComputationStep(self, index):
        return list(self._steps[index])


# ------------------------------------------------------------------------------------------------ platform / context
class Platform:
    _warned = set()

    def __init__(self, name='HIP'):
        self._name = name
        self._props = {}

    @staticmethod
    def getPlatformByName(name):
        """Only one platform exists here: the hand-written HIP path on MI355X.  Scripts written for
        the reference ask for 'Reference'/'CPU'/'CUDA'/'OpenCL'; they get the HIP platform (there is no
        CPU fallback) and `getName()` says so."""
        return Platform('HIP')

    @staticmethod
    def getNumPlatforms():
        return 1

    @staticmethod
    def getPlatform(index):
        return Platform('HIP')

    def getName(self):
        return self._name

    def setPropertyDefaultValue(self, name, value):
        self._props[name] = value

    def getPropertyDefaultValue(self, name):
        return self._props.get(name, '')


class State:
    def __init__(self, energy=None, kinetic=None, forces=None, positions=None, velocities=None, box=None, time=0.0):
        self._e, self._k, self._f, self._x, self._v, self._box, self._t = energy, kinetic, forces, positions, velocities, box, time

    def getPotentialEnergy(self):
        if self._e is None:
            raise OpenMMException('Invoked getPotentialEnergy() on a State which does not contain energies.')
        return Quantity(self._e, kjmol)

    def getKineticEnergy(self):
        if self._k is None:
            raise OpenMMException('Invoked getKineticEnergy() on a State which does not contain energies.')
        return Quantity(self._k, kjmol)

    def _vecs(self, arr, u, asNumpy):
        if arr is None:
            raise OpenMMException('State does not contain the requested data.')
        return Quantity(arr if asNumpy else [Vec3(*r) for r in arr.tolist()], u)

    def getForces(self, asNumpy=False):
        return self._vecs(self._f, kjmol / nm, asNumpy)

    def getPositions(self, asNumpy=False):
        return self._vecs(self._x, nm, asNumpy)

    def getVelocities(self, asNumpy=False):
        return self._vecs(self._v, nm / _unit.picosecond, asNumpy)

    def getPeriodicBoxVectors(self):
        if self._box is None:          # a Context in free space (NoCutoff / CutoffNonPeriodic)
            return None
        return [Quantity(Vec3(*v), nm) for v in self._box]

    def getTime(self):
        return Quantity(self._t, _unit.picosecond)

    def getEnergyParameterDerivatives(self):
        if getattr(self, '_derivatives', None) is None:
            raise OpenMMException('Invoked getEnergyParameterDerivatives() on a State which does not contain parameter derivatives.')
        return dict(self._derivatives)


def _as_array(values, n, what):
    v = md_value(values)
    if isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], Quantity):
        v = [md_value(r) for r in v]
    arr = np.array(v, dtype=np.float64)
    if arr.shape != (n, 3):
        raise OpenMMException('Called %s() on a Context with the wrong number of %s' % (what, what[3:].lower()))
    return arr


def molecules_of(system):
    """The molecules of a System: connected components of its bond graph (Context.getMolecules)."""
    n = system.getNumParticles()
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    pairs = [(c[0], c[1]) for c in system._constraints]
    for force in system.getForces():
        if isinstance(force, (HarmonicBondForce, CustomBondForce)):
            pairs += [(b[0], b[1]) for b in force._bonds]
        elif isinstance(force, (HarmonicAngleForce, CustomAngleForce)):
            pairs += [(r[0], r[1]) for r in force._angles] + [(r[1], r[2]) for r in force._angles]
        elif isinstance(force, (PeriodicTorsionForce, CustomTorsionForce, RBTorsionForce)):
            pairs += [(r[0], r[1]) for r in force._torsions] + [(r[1], r[2]) for r in force._torsions] + \
                     [(r[2], r[3]) for r in force._torsions]
        elif isinstance(force, CMAPTorsionForce):              # both dihedrals of every term, each as a torsion
            pairs += [(r[k], r[k + 1]) for r in force._torsions for k in (1, 2, 3, 5, 6, 7)]
        elif isinstance(force, CustomCompoundBondForce):       # consecutive particles, as an angle or torsion (a centroid bond joins nothing)
            pairs += [(a, b) for members, _ in force._bonds for a, b in zip(members[:-1], members[1:])]
        elif isinstance(force, DrudeForce):                    # a Drude particle hangs on its parent: a box move must not tear them apart
            pairs += [(r[0], r[1]) for r in force._particles if 0 <= r[0] < n and 0 <= r[1] < n]
    # (a virtual site belongs to the molecule of its parents, as in OpenMM's getMolecules)
    pairs += [(index, site.getParticle(k)) for index, site in sorted(getattr(system, '_vsites', {}).items())
              for k in range(site.getNumParticles()) if 0 <= site.getParticle(k) < n]
    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    groups = {}
    for i in range(n):
        groups.setdefault(find(i), []).append(i)
    return [groups[r] for r in sorted(groups)]


class Context:
    def __init__(self, system, integrator, platform=None, properties=None):
        from ..engine import Engine
        if integrator._context is not None:
            raise OpenMMException('This Integrator is already bound to a context')
        self._system = system
        self._integrator = integrator
        self._platform = platform or Platform('HIP')
        self._engine = Engine(system, integrator, properties or {})
        integrator._context = self

    def getSystem(self):
        return self._system

    def getIntegrator(self):
        return self._integrator

    def getPlatform(self):
        return self._platform

    def setPositions(self, positions):
        self._engine.set_positions(_as_array(positions, self._system.getNumParticles(), 'setPositions'))

    def setVelocities(self, velocities):
        self._engine.set_velocities(_as_array(velocities, self._system.getNumParticles(), 'setVelocities'))

    def setVelocitiesToTemperature(self, temperature, randomSeed=None):
        """Maxwell-Boltzmann velocities from numpy's generator (OpenMM's own RNG stream is not
        reproduced: SURVEY.md 8c G13 'parity unpinned')."""
        T = float(md_value(temperature))
        rng = np.random.default_rng(randomSeed)
        m = np.array(self._system._masses)
        kT = _unit.BOLTZMANN_CONSTANT_kB._value * T
        v = rng.normal(size=(len(m), 3)) * np.sqrt(kT / np.where(m > 0, m, 1.0))[:, None]
        v[m <= 0] = 0.0
        # multi-rank runs integrate every atom on every rank: all ranks must hold the SAME velocities, also when no seed
        # was given (each process would draw its own from OS entropy) -- rank 0's draw is broadcast
        v = self._engine.broadcast_from_rank0(v)
        self._engine.set_velocities(v)
        self._engine.apply_velocity_constraints()     # as OpenMM does after drawing the velocities

    def applyConstraints(self, tol=None):
        """Move the positions onto the constraint surface (reference = the current positions)."""
        self._engine.apply_constraints()

    def applyVelocityConstraints(self, tol=None):
        self._engine.apply_velocity_constraints()

    def computeVirtualSites(self):
        """Put every virtual site where its parents' current positions say (a no-op for a System without sites)."""
        self._engine.compute_virtual_sites()

    def setParameter(self, name, value):
        if name == MonteCarloBarostat.Pressure() and isinstance(value, Quantity):
            value = value.value_in_unit(_unit.bar)        # (the parameter is a number of bar, as in OpenMM)
        self._engine.set_parameter(name, float(md_value(value)))

    def getParameter(self, name):
        return self._engine.get_parameter(name)

    def getParameters(self):
        return dict(self._engine.parameters)

    def setPeriodicBoxVectors(self, a, b, c):
        """A new (orthorhombic) box for the live Context; the positions stay as they are, as in OpenMM."""
        vecs = [[float(md_value(x)) for x in md_value(v)] for v in (a, b, c)]
        for i in range(3):
            for j in range(3):
                if i != j and abs(vecs[i][j]) > 1e-12:
                    raise InputError('only orthorhombic periodic boxes are supported by the HIP path')
        self._engine.set_box([vecs[0][0], vecs[1][1], vecs[2][2]])

    def setState(self, state):
        """Box, then positions and velocities (those the State carries) of another Context's State."""
        if state._box is not None:
            self.setPeriodicBoxVectors(*state._box)
        if state._x is not None:
            self._engine.set_positions(state._x)
        if state._v is not None:
            self._engine.set_velocities(state._v)

    def getMolecules(self):
        """Connected components of the bond graph (bonds of the bonded forces + constraints), as OpenMM's
        Context.getMolecules(): a list of lists of atom indices, each in increasing order."""
        return molecules_of(self._system)

    def getState(self, getPositions=False, getVelocities=False, getForces=False, getEnergy=False,
                 getParameters=False, enforcePeriodicBox=False, groups=-1, getParameterDerivatives=False):
        if isinstance(groups, (set, list, tuple, frozenset)):
            mask = 0
            for g in groups:
                mask |= 1 << int(g)
        else:
            mask = int(groups) & 0xFFFFFFFF
        state = self._engine.get_state(getPositions, getVelocities, getForces, getEnergy, mask)
        if getParameterDerivatives:
            # the parameters some force asked for with addEnergyParameterDerivative (e.g. AlchemicalSystem, systems.py:390)
            names = []
            for force in self._system.getForces():
                for name in getattr(force, '_derivs', ()):
                    if name not in names:
                        names.append(name)
            state._derivatives = {name: self._engine.energy_derivative(name) for name in names}
        return state

    def reinitialize(self, preserveState=False):
        self._engine.reinitialize(preserveState)


class MinimizationReporter:
    """openmm.MinimizationReporter (OpenMM 8.1): subclass it and override report(); an instance handed to
    LocalEnergyMinimizer.minimize / Simulation.minimizeEnergy is called once per L-BFGS iteration."""

    def report(self, iteration, x, grad, args):
        """iteration: 0, 1, ...; x, grad: flat sequences of 3N numbers (nm, kJ/mol/nm); args: 'system energy', 'restraint energy'
        (kJ/mol), 'restraint strength' (kJ/mol/nm^2), 'max constraint error' (relative).  Return True to stop the minimisation."""
        return False


class LocalEnergyMinimizer:
    """openmm.LocalEnergyMinimizer: L-BFGS on the Context's potential energy, positions left in the Context.  The vectors and the
    energy evaluations stay on the GPU (csrc/minimize.hip, Engine.minimize)."""

    @staticmethod
    def minimize(context, tolerance=10.0, maxIterations=0, reporter=None):
        """tolerance: RMS force at which to stop, a Quantity of energy / length or a number of kJ/mol/nm; maxIterations = 0: until
        converged."""
        if isinstance(tolerance, Quantity):
            tolerance = md_value(tolerance, kjmol / nm)
        tolerance, maxIterations = float(tolerance), int(maxIterations)
        if not tolerance > 0:
            raise OpenMMException('LocalEnergyMinimizer: the tolerance must be positive')
        if maxIterations < 0:
            raise OpenMMException('LocalEnergyMinimizer: maxIterations must not be negative')
        if reporter is not None and not callable(getattr(reporter, 'report', None)):
            raise TypeError('LocalEnergyMinimizer: reporter must be a MinimizationReporter')
        context._engine.minimize(tolerance, maxIterations, reporter)


from . import app  # noqa: E402,F401
