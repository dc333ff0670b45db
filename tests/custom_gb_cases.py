"""Models and references of the CustomGBForce tests (csrc/custom_gb.hip).  Every model is restated here in closed form in torch fp64 on
the CPU -- from its formulas, not by parsing its texts, so a mistake of the compiler shows as another number -- and its forces come
from torch.autograd, as in tests/gb_cases.py.  Units nm, kJ/mol, e.

obc2-text    OBC2 as a CustomGBForce: the texts of atomsmm_amd.customgb.GBSAOBC2Force with the engulfed-sphere term, so that
             gb_cases.evaluate (the definition of GBSAOBCForce) is its reference and gb_cases.n5 takes every branch.  Parameters q,
             or = R - 0.009, sr = S or; I of type ParticlePairNoExclusions, B of type SingleParticle; self and surface terms, and the
             pair term -pre q1 q2 / f of type ParticlePairNoExclusions.

chain-table  a synthetic model, each piece one mechanism (parameters t = a type index 0 .. 2, a in [0.5, 1.5], c = the charge; globals
             kappa, eps0; W a Discrete2DFunction 3 x 3 that is NOT symmetric, S a Continuous1DFunction on [0, 8] nm):
               V (ParticlePair, with exclusions)   sum_j W(t1, t2) a2 S(r) / (1 + kappa r)        asymmetric; both tables; a global
               P (SingleParticle)                  a + 0.3 V^2 / (1 + V^2)
               Q (SingleParticle)                  eps0 sqrt(1 + P^2 + 0.5 V)                     reads P AND V: a two-level Jacobian
               ParticlePair term                   c1 c2 exp(-r / (Q1 + Q2)) / (r + P1 P2)       reads both atoms' values
               ParticlePairNoExclusions term       0.05 exp(-kappa r) / r                        r only; a global
               SingleParticle term                 0.5 c^2 / Q + 0.1 V P
             No text has a step, select, min, max, abs, floor or ceil, so none has a kink.  The two places where a table could make
             one: S is 0 outside [0, 8] nm and every distance of every case is below 4.4 nm (margin 3.6 nm; chain_force asserts 6);
             W is read at rint(t) and every t is a whole number exactly (margin 0.5).  W, a, S are positive, so V > 0 and the square
             root's argument exceeds 1.
"""
import numpy as np
import torch

from atomsmm_amd import customgb, expr as X, openmm, tables as T

import gb_cases as G

KAPPA, EPS0 = 0.7, 1.3
W_VALUES = [0.9, 1.4, 0.6, 0.7, 1.1, 1.3, 1.5, 0.8, 1.0]          # W(x, y) = values[x + 3 y]: W(0, 1) = 0.7 != W(1, 0) = 1.4
S_LO, S_HI, S_KNOTS = 0.0, 8.0, 33
S_VALUES = [float(np.exp(-0.45 * x) * (1.0 + 0.15 * np.sin(2.1 * x)) + 0.2) for x in np.linspace(S_LO, S_HI, S_KNOTS)]

V_TEXT = 'W(t1,t2)*a2*S(r)/(1+kappa*r)'
P_TEXT = 'a+0.3*V^2/(1+V^2)'
Q_TEXT = 'eps0*sqrt(1+P^2+0.5*V)'
PAIR_TEXT = 'c1*c2*exp(-r/(Q1+Q2))/(r+P1*P2)'
FAR_TEXT = '0.05*exp(-kappa*r)/r'
SINGLE_TEXT = '0.5*c^2/Q+0.1*V*P'


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------------------------ obc2-text
def obc2_force(case, rc=None, **kw):
    force = customgb.GBSAOBC2Force(case['charge'], case['radius'], case['scale'], engulfed=True, **kw)
    if rc:
        force.setNonbondedMethod(force.CutoffNonPeriodic)
        force.setCutoffDistance(rc)
    return force


def obc2_reference(case, rc=None, **kw):
    """gb_cases.evaluate plus the computed values [I, B]: the Born integral as gb_cases restates it, summed here once more."""
    out = G.evaluate(case, rc, **kw)
    x = _t(case['positions'])
    rho = _t(case['radius']) - G.OFFSET
    s = _t(case['scale']) * rho
    integral = G._born_integral(*G._geometry(x, x, 0, rc), rho, s)
    out['values'] = np.stack([integral.numpy(), out['born']])
    return out


# ------------------------------------------------------------------------------------ chain-table
def chain_parameters(case):
    """(t, a, c) per atom from the case: the type index by position in the case, a from the radius, c the charge."""
    n = len(case['positions'])
    return np.stack([np.arange(n) % 3, 5.0 * np.asarray(case['radius']) * (1.0 + 0.02 * (np.arange(n) % 7)), np.asarray(case['charge'])], axis=1).astype(np.float64)


def chain_exclusions(n):
    """(3 m, 3 m + 1) and (3 m, 3 m + 2): the bonds of a water where the case is one."""
    return [(i, i + d) for i in range(0, n, 3) for d in (1, 2) if i + d < n]


def chain_force(case, rc=None, exclusions=None, kappa=KAPPA, eps0=EPS0):
    n = len(case['positions'])
    d = case['positions'][:, None, :] - case['positions'][None, :, :]
    assert np.sqrt((d * d).sum(-1)).max() < S_HI - 2.0          # no distance near the end of S's range
    force = openmm.CustomGBForce()
    for name in ('t', 'a', 'c'):
        force.addPerParticleParameter(name)
    force.addGlobalParameter('kappa', kappa)
    force.addGlobalParameter('eps0', eps0)
    force.addTabulatedFunction('W', openmm.Discrete2DFunction(3, 3, W_VALUES))
    force.addTabulatedFunction('S', openmm.Continuous1DFunction(S_VALUES, S_LO, S_HI))
    force.addComputedValue('V', V_TEXT, force.ParticlePair)
    force.addComputedValue('P', P_TEXT, force.SingleParticle)
    force.addComputedValue('Q', Q_TEXT, force.SingleParticle)
    force.addEnergyTerm(PAIR_TEXT, force.ParticlePair)
    force.addEnergyTerm(FAR_TEXT, force.ParticlePairNoExclusions)
    force.addEnergyTerm(SINGLE_TEXT, force.SingleParticle)
    for row in chain_parameters(case):
        force.addParticle(list(row))
    for i, j in (chain_exclusions(n) if exclusions is None else exclusions):
        force.addExclusion(i, j)
    if rc:
        force.setNonbondedMethod(force.CutoffNonPeriodic)
        force.setCutoffDistance(rc)
    return force


def _spline(r, values, lo, hi):
    """The natural cubic spline through `values` (the coefficients of atomsmm_amd.tables, the interval arithmetic restated), in torch."""
    coef = _t(T.spline_coefficients(values, lo, hi))
    nx = len(values)
    h = (hi - lo) / (nx - 1)
    k = torch.clamp(torch.floor((r.detach() - lo) / h), 0, nx - 2).long()
    u = (r - lo) - k.to(torch.float64) * h
    a, b, c, d = (coef[:, j][k] for j in range(4))
    return a + u * (b + u * (c + u * d))


def chain_reference(case, rc=None, exclusions=None, kappa=KAPPA, eps0=EPS0, parameters=None, w_values=None, s_values=None, want_forces=True):
    """dict(energy, forces, values = [V, P, Q]) of the chain-table model, in one graph."""
    n = len(case['positions'])
    par = chain_parameters(case) if parameters is None else np.asarray(parameters, dtype=np.float64)
    t, a, c = par[:, 0].astype(np.int64), _t(par[:, 1]), _t(par[:, 2])
    w = _t(W_VALUES if w_values is None else w_values)
    x = _t(case['positions']).clone().requires_grad_(want_forces)
    r, part = G._geometry(x, x, 0, rc)
    allowed = part.clone()
    for i, j in (chain_exclusions(n) if exclusions is None else exclusions):
        allowed[i, j] = allowed[j, i] = False
    zero = torch.zeros_like(r)
    wij = w[torch.as_tensor(t)[:, None] + 3 * torch.as_tensor(t)[None, :]]
    f = wij * a[None, :] * _spline(r, S_VALUES if s_values is None else s_values, S_LO, S_HI) / (1.0 + kappa * r)
    V = torch.where(allowed, f, zero).sum(1)
    P = a + 0.3 * V ** 2 / (1.0 + V ** 2)
    Q = eps0 * torch.sqrt(1.0 + P ** 2 + 0.5 * V)
    pair = c[:, None] * c[None, :] * torch.exp(-r / (Q[:, None] + Q[None, :])) / (r + P[:, None] * P[None, :])
    far = 0.05 * torch.exp(-kappa * r) / r
    energy = 0.5 * torch.where(allowed, pair, zero).sum() + 0.5 * torch.where(part, far, zero).sum() + (0.5 * c ** 2 / Q + 0.1 * V * P).sum()
    out = dict(energy=energy.item(), values=np.stack([V.detach().numpy(), P.detach().numpy(), Q.detach().numpy()]))
    if want_forces:
        (grad,) = torch.autograd.grad(energy, x)
        out['forces'] = -grad.numpy()
    return out


MODELS = {'obc2-text': (obc2_force, obc2_reference), 'chain-table': (chain_force, chain_reference)}


# ------------------------------------------------------------------------------------ a force object onto a backend context
def compiled(force):
    """expr.compile_custom_gb of a CustomGBForce object."""
    names = [force.getPerParticleParameterName(k) for k in range(force.getNumPerParticleParameters())]
    gnames = [force.getGlobalParameterName(k) for k in range(force.getNumGlobalParameters())]
    functions = list(force._functions)
    return X.compile_custom_gb(names, gnames, [tuple(v) for v in force._values], [tuple(t) for t in force._terms],
                               T.declared(functions) if functions else None)


def create_on(ctx, force, globals_=None):
    """The force on a backend context, as the engine translates it: its id."""
    progs = compiled(force)
    n = force.getNumParticles()
    params = np.array(force._particles, dtype=np.float64).reshape(n, -1)
    values = [force.getGlobalParameterDefaultValue(k) for k in range(force.getNumGlobalParameters())] if globals_ is None else globals_
    rc = force.getCutoffDistance()._value if force.getNonbondedMethod() == force.CutoffNonPeriodic else 0.0
    fid = ctx.custom_gb_create(force.getNumComputedValues(), progs.types, [(p.code, p.consts) for p in progs.programs], values,
                               np.ascontiguousarray(params.T), np.array(force._exclusions, dtype=np.int32).reshape(-1, 2), rc)
    if force._functions:
        ctx.custom_gb_set_tables(fid, [T.device_table(fn) for _, fn in force._functions])
    return fid
