"""Three generalized-Born models as CustomGBForce objects, written from the published formulas: Hawkins-Cramer-Truhlar (HCT), and the
two Onufriev-Bashford-Case rescalings OBC1 and OBC2.

    GBSAHCTForce / GBSAOBC1Force / GBSAOBC2Force(charge, radius, scale, soluteDielectric=1.0, solventDielectric=78.3, SA='ACE')

charge (e), radius (nm) and scale per particle.  The per-particle parameters are q, the offset radius `or` = radius - 0.009 and the
scaled radius `sr` = scale * or.  The computed values:

    I = sum_j step(r + sr2 - or1) / 2 (1/L - 1/U + (r - sr2^2/r)(1/U^2 - 1/L^2)/4 + log(L/U)/(2 r)),  U = r + sr2, L = max(or1, |r - sr2|)
    B = 1/(1/or - I)                                                          HCT
    B = 1/(1/or - tanh(a psi - b psi^2 + c psi^3)/radius),  psi = I or        OBC1: (0.8, 0, 2.909125); OBC2: (1, 0.8, 4.85)

and the energy terms: the self term -K/2 (1/eps_in - 1/eps_out) q^2/B, the surface term 4 pi SA (radius + 0.14)^2 (radius/B)^6 (SA =
'ACE': 2.25936 kJ/mol/nm^2; a number: that energy; None: no term) and the pair term -K (1/eps_in - 1/eps_out) q1 q2/f with
f = sqrt(r^2 + B1 B2 exp(-r^2/(4 B1 B2))).  Both pair texts are ParticlePairNoExclusions, as OpenMM's GBSAOBCForce takes all pairs.
K = 138.935456, the constant of every Coulomb term of this package.

engulfed=True adds the term 2 (1/or1 - 1/L) to the integrand where or1 < sr2 - r (particle 1 lies inside the scaled sphere of
particle 2), which OpenMM's GBSAOBCForce has and its CustomGBForce texts leave out.

GBn and GBn2 need the published neck tables: supply them to a CustomGBForce of your own as a Discrete2DFunction.
"""
import math

from . import openmm as mm

KC = 138.935456
OFFSET, PROBE = 0.009, 0.14
ACE = 2.25936           # kJ/mol/nm^2
RESCALING = dict(OBC1=(0.8, 0.0, 2.909125), OBC2=(1.0, 0.8, 4.85))


def integral_text(engulfed=False):
    """The text of the pair integral I."""
    inner = '1/L-1/U+0.25*(r-sr2^2/r)*(1/(U^2)-1/(L^2))+0.5*log(L/U)/r'
    if engulfed:
        inner += '+2*step(sr2-r-or1)*(1/or1-1/L)'
    return 'step(r+sr2-or1)*0.5*(%s); U=r+sr2; L=max(or1,D); D=abs(r-sr2)' % inner


def born_radius_text(model):
    """The text of the Born radius B from I."""
    if model == 'HCT':
        return '1/(1/or-I)'
    a, b, c = RESCALING[model]
    return '1/(1/or-tanh(%r*psi-%r*psi^2+%r*psi^3)/radius); psi=I*or; radius=or+%r' % (a, b, c, OFFSET)


def _force(model, charge, radius, scale, soluteDielectric, solventDielectric, SA, engulfed):
    if not len(charge) == len(radius) == len(scale):
        raise ValueError('charge, radius and scale need one entry per particle')
    force = mm.CustomGBForce()
    for name in ('q', 'or', 'sr'):
        force.addPerParticleParameter(name)
    force.addGlobalParameter('solventDielectric', solventDielectric)
    force.addGlobalParameter('soluteDielectric', soluteDielectric)
    force.addComputedValue('I', integral_text(engulfed), force.ParticlePairNoExclusions)
    force.addComputedValue('B', born_radius_text(model), force.SingleParticle)
    factor = '%r*(1/soluteDielectric-1/solventDielectric)' % KC
    force.addEnergyTerm('-0.5*%s*q^2/B' % factor, force.SingleParticle)
    if SA is not None:
        energy = ACE if SA == 'ACE' else float(SA)
        force.addEnergyTerm('%r*(radius+%r)^2*(radius/B)^6; radius=or+%r' % (4.0 * math.pi * energy, PROBE, OFFSET), force.SingleParticle)
    force.addEnergyTerm('-%s*q1*q2/f; f=sqrt(r^2+B1*B2*exp(-r^2/(4*B1*B2)))' % factor, force.ParticlePairNoExclusions)
    for q, R, S in zip(charge, radius, scale):
        rho = float(R) - OFFSET
        force.addParticle([float(q), rho, float(S) * rho])
    return force


def GBSAHCTForce(charge, radius, scale, soluteDielectric=1.0, solventDielectric=78.3, SA='ACE', engulfed=False):
    return _force('HCT', charge, radius, scale, soluteDielectric, solventDielectric, SA, engulfed)


def GBSAOBC1Force(charge, radius, scale, soluteDielectric=1.0, solventDielectric=78.3, SA='ACE', engulfed=False):
    return _force('OBC1', charge, radius, scale, soluteDielectric, solventDielectric, SA, engulfed)


def GBSAOBC2Force(charge, radius, scale, soluteDielectric=1.0, solventDielectric=78.3, SA='ACE', engulfed=False):
    return _force('OBC2', charge, radius, scale, soluteDielectric, solventDielectric, SA, engulfed)
