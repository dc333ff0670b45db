"""Inputs of the generalized-Born tests (GBSAOBCForce, csrc/gb.hip) and an fp64 restatement of the definition in torch on the CPU.

The restatement is written from the definition (include/atomsmm_hip.h: amm_gb_create), not from the kernels, and its forces come
from torch.autograd: nobody derived them by hand.  Units nm, kJ/mol, e.

    rho_i = R_i - 0.009, s_j = S_j rho_j; a pair (i, j), i != j, takes part when there is no cutoff or r^2 < rc^2
    I_i = 1/2 sum_j h(r_ij; rho_i, s_j) over the pairs that take part and have rho_i < r + s_j
    L = 1/max(rho_i, |r - s_j|), U = 1/(r + s_j)
    h = L - U + r (U^2 - L^2)/4 + ln(U/L)/(2 r) + s_j^2 (L^2 - U^2)/(4 r)   [+ 2 (1/rho_i - L) when rho_i < s_j - r]
    Psi = I rho, B = 1/(1/rho - tanh(Psi - 0.8 Psi^2 + 4.85 Psi^3)/R)
    E_pol = -1/2 K (1/eps_in - 1/eps_out) sum_{i,j} q_i q_j / f_ij (ordered pairs that take part, and i = j)
    f_ij = sqrt(r^2 + B_i B_j exp(-r^2/(4 B_i B_j)));  E_SA = 4 pi gamma sum_i (R_i + 0.14)^2 (R_i/B_i)^6
"""
import math

import numpy as np
import torch

from free_space_cases import d1527, s33  # noqa: F401  (re-exported: the cases are cut as there)

KC = 138.935456
OFFSET, PROBE = 0.009, 0.14
ALPHA, BETA, GAMMA = 1.0, 0.8, 4.85
EPS_IN, EPS_OUT, SA = 1.0, 78.3, 2.25936
ROWS = 512          # rows per block of the blocked evaluation (memory: ROWS x n doubles per intermediate)


def radii_by_mass(mass):
    """(R, S) per atom from its mass: hydrogen, carbon, nitrogen, everything else."""
    mass = np.asarray(mass, dtype=np.float64)
    R = np.where(mass < 2, 0.12, np.where(mass < 13, 0.17, np.where(mass < 15, 0.155, 0.15)))
    S = np.where(mass < 2, 0.85, np.where(mass < 13, 0.72, np.where(mass < 15, 0.79, 0.85)))
    return R, S


def with_radii(case):
    R, S = radii_by_mass(case['mass'])
    return dict(positions=np.ascontiguousarray(case['positions'], dtype=np.float64), charge=np.asarray(case['charge'], dtype=np.float64),
                radius=R, scale=S, mass=np.asarray(case['mass'], dtype=np.float64))


def d4608(spcfw):
    """The whole 1536-atom q-SPC-FW box and two copies shifted by one and two box edges along x: 18 tiles of 256."""
    shift = np.zeros(3)
    shift[0] = spcfw['box'][0]
    pos = np.concatenate([spcfw['positions'] + k * shift for k in range(3)])
    return with_radii(dict(positions=pos, charge=np.tile(spcfw['charge'], 3), mass=np.tile(spcfw['mass'], 3)))


def n5():
    """Five atoms that take every branch of h: atom 1 is engulfed by atom 0, the pair (0 <- 1) does not count, the pairs (0, 2) and
    (2, 3) take the rho side of the max, atom 4 lies outside a 1.0 nm cutoff."""
    return dict(positions=np.array([[0, 0, 0], [0.03, 0, 0], [0.35, 0.02, -0.01], [0.35, 0.20, 0], [2, 2, 2]], dtype=np.float64),
                charge=np.array([0.6, -0.4, -0.5, 0.3, 1.0]), radius=np.array([0.30, 0.10, 0.17, 0.12, 0.2]),
                scale=np.array([1.0, 0.8, 0.72, 0.85, 0.8]), mass=np.array([12.0, 1.0, 12.0, 1.0, 16.0]))


def tiny(n):
    """n = 1: one ion; n = 2: one pair at 0.31 nm."""
    pos = np.array([[0.1, 0.2, 0.3], [0.35, 0.05, 0.42]])[:n]
    return dict(positions=pos, charge=np.array([-0.8, 0.4])[:n], radius=np.array([0.15, 0.12])[:n], scale=np.array([0.85, 0.85])[:n],
                mass=np.array([16.0, 1.0])[:n])


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _geometry(x_rows, x_all, first_row, rc):
    """(r with 1 where the pair does not take part, mask of the pairs that take part) of rows first_row.. against all atoms."""
    d = x_rows[:, None, :] - x_all[None, :, :]
    r2 = (d * d).sum(-1)
    rows = torch.arange(first_row, first_row + x_rows.shape[0])
    part = rows[:, None] != torch.arange(x_all.shape[0])[None, :]            # the diagonal is left out by index
    if rc is not None and rc > 0:
        part = part & (r2 < rc * rc)
    return torch.sqrt(torch.where(part, r2, torch.ones_like(r2))), part


def _born_integral(r, part, rho_rows, s_all):
    rho = rho_rows[:, None]
    s = s_all[None, :]
    U = 1.0 / (r + s)
    L = 1.0 / torch.maximum(rho.expand_as(r), (r - s).abs())
    h = L - U + 0.25 * r * (U * U - L * L) + torch.log(U / L) / (2 * r) + s * s / (4 * r) * (L * L - U * U)
    h = h + torch.where(rho < s - r, 2.0 * (1.0 / rho - L), torch.zeros_like(r))
    counts = part & (rho < r + s)
    return 0.5 * torch.where(counts, h, torch.zeros_like(h)).sum(1)


def _born_radius(I, rho, R):
    psi = I * rho
    return 1.0 / (1.0 / rho - torch.tanh(ALPHA * psi - BETA * psi ** 2 + GAMMA * psi ** 3) / R)


def _energy_rows(r, part, first_row, q, B, R, pre, sa):
    """(E_pol, E_SA) of rows first_row..: their ordered pairs, their diagonal terms and their surface terms."""
    rows = slice(first_row, first_row + r.shape[0])
    D = B[rows, None] * B[None, :]
    r2 = r * r
    f = torch.sqrt(r2 + D * torch.exp(-r2 / (4 * D)))
    pair = torch.where(part, q[rows, None] * q[None, :] / f, torch.zeros_like(f)).sum()
    e_pol = -0.5 * pre * (pair + (q[rows] ** 2 / B[rows]).sum())
    e_sa = 4 * math.pi * sa * ((R[rows] + PROBE) ** 2 * (R[rows] / B[rows]) ** 6).sum()
    return e_pol, e_sa


def evaluate_direct(case, rc=None, eps_in=EPS_IN, eps_out=EPS_OUT, sa=SA, charge=None, want_forces=True):
    """The definition in one graph: dict(e_pol, e_sa, energy, born, forces).  For small cases (memory: ~40 n x n arrays)."""
    x = _t(case['positions']).clone().requires_grad_(want_forces)
    q = _t(case['charge'] if charge is None else charge)
    R, S = _t(case['radius']), _t(case['scale'])
    rho = R - OFFSET
    s = S * rho
    r, part = _geometry(x, x, 0, rc)
    B = _born_radius(_born_integral(r, part, rho, s), rho, R)
    e_pol, e_sa = _energy_rows(r, part, 0, q, B, R, KC * (1 / eps_in - 1 / eps_out), sa)
    out = dict(e_pol=e_pol.item(), e_sa=e_sa.item(), energy=(e_pol + e_sa).item(), born=B.detach().numpy().copy())
    if want_forces:
        (grad,) = torch.autograd.grad(e_pol + e_sa, x)
        out['forces'] = -grad.numpy()
    return out


def evaluate(case, rc=None, eps_in=EPS_IN, eps_out=EPS_OUT, sa=SA, charge=None, want_forces=True):
    """The same numbers in blocks of ROWS rows, so that 4608 atoms fit: the Born radii first; then E(x, B) block by block with
    autograd for dE/dx at fixed radii and dE/dB; then dB/dI by autograd of the per-atom function; then every block of the Born integral
    again, back-propagated with g = dE/dI.  Every derivative is autograd's; only the chain rule that joins the stages is written out."""
    n = len(case['positions'])
    x = _t(case['positions']).clone().requires_grad_(want_forces)
    q = _t(case['charge'] if charge is None else charge)
    R, S = _t(case['radius']), _t(case['scale'])
    rho = R - OFFSET
    s = S * rho
    pre = KC * (1 / eps_in - 1 / eps_out)
    with torch.no_grad():
        I = torch.cat([_born_integral(*_geometry(x[a:a + ROWS], x, a, rc), rho[a:a + ROWS], s) for a in range(0, n, ROWS)])
    I = I.clone().requires_grad_(want_forces)
    B_of_I = _born_radius(I, rho, R)
    B = B_of_I.detach().clone().requires_grad_(want_forces)
    e_pol = e_sa = 0.0
    for a in range(0, n, ROWS):
        r, part = _geometry(x[a:a + ROWS], x, a, rc)
        p, t = _energy_rows(r, part, a, q, B, R, pre, sa)
        if want_forces:
            (p + t).backward()                       # x.grad: dE/dx at fixed radii; B.grad: dE/dB
        e_pol += p.item()
        e_sa += t.item()
    out = dict(e_pol=e_pol, e_sa=e_sa, energy=e_pol + e_sa, born=B.detach().numpy().copy())
    if want_forces:
        (g,) = torch.autograd.grad(B_of_I, I, grad_outputs=B.grad)          # dE/dI
        for a in range(0, n, ROWS):
            r, part = _geometry(x[a:a + ROWS], x, a, rc)
            _born_integral(r, part, rho[a:a + ROWS], s).backward(g[a:a + ROWS])
        out['forces'] = -x.grad.numpy()
    return out
