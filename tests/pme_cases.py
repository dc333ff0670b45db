"""The checker of the PME reciprocal-space tests: smooth particle-mesh Ewald restated in plain numpy on a GIVEN mesh, and the
seeded cases it is run on.  Nothing here is a test; tests/test_pme_host.py checks the checker (against OpenMM's literals, against
80-bit arithmetic, against its own energy's gradient, against an explicit Ewald sum, and for its sensitivity to six planted errors)
and tests/test_gpu_pme.py checks the kernels of csrc/pme.hip against the checker.

The algorithm is the one the header comment of csrc/pme.hip states (Essmann et al., J. Chem. Phys. 103, 8577, with OpenMM's
conventions): cardinal B-splines of order 5, Q = the charges spread on the mesh, S = FFT(Q),

    E_rec = 1/2 sum_m eterm(m) |S(m)|^2,   eterm(m) = Kc exp(-pi^2 m^2 / alpha^2) / (pi V m^2 B(m)),   eterm(0) = 0,
    E_self = -Kc alpha / sqrt(pi) sum q^2  (no neutralising-background term),
    F_i = -q_i sum_mesh grad(w w w)(i, p) phi(p),   phi = inverse FFT(eterm S) (the convolution of Q with the pair potential).

None of it is the kernels' arithmetic: the spline weights come from the Cox-de Boor definition of M_n, evaluated where the
definition says (w[k] = M_5(fr + 4 - k), dw[k] = M_4(fr + 4 - k) - M_4(fr + 3 - k)), the moduli from a direct sum, the transforms
from np.fft with explicit axes, the frequencies from np.fft.fftfreq.  On a given mesh smooth PME is a finite, exactly specified
computation, so the kernels must agree with this file up to what their 2^-42 fixed-point mesh rounds away -- and `quant` is a
model of exactly that rounding, from which the GPU tests derive their tolerances (tolerances()).

The steps are methods of one class so that a test can plant an error in a copy (a subclass that overrides one step).
"""
import functools

import numpy as np

ORDER = 5
KC = 138.935456
ALPHA = 2.6                          # 1/nm
QUANT = 2.0 ** 42                    # the kernels' fixed-point scale (PME_FIXED_SCALE)


def cardinal_bspline(n, u):
    """M_n(u), the cardinal B-spline of order n (support [0, n]), by the Cox-de Boor recursion from the hat function M_2."""
    if n == 2:
        return np.where((u >= 0) & (u <= 2), 1 - np.abs(u - 1), 0 * u)
    return (u * cardinal_bspline(n - 1, u) + (n - u) * cardinal_bspline(n - 1, u - 1)) / (n - 1)


class PmeReference:
    """pme_reference() as an object: one method per step of the algorithm."""

    def __init__(self, dtype=np.float64, quant=None):
        self.T = np.dtype(dtype).type
        self.quant = quant
        self.pi = 4 * np.arctan(self.T(1))

    # -- per axis: the mesh points an atom touches, its weights on them and their derivatives with respect to the scaled coordinate
    def locate(self, x, L, K):
        t = x / L
        t = (t - np.floor(t)) * K            # (t - floor(t) can round to 1: the index then wraps through the modulo below)
        ti = np.floor(t)
        return ti.astype(np.int64) % K, t - ti

    def axis_terms(self, axis, x, L, K):
        """points [n][5], w [n][5], dw [n][5] of one axis."""
        idx, fr = self.locate(x, L, K)
        u = fr[:, None] + self.T(ORDER - 1) - np.arange(ORDER).astype(self.T)[None, :]
        w = cardinal_bspline(ORDER, u)
        dw = cardinal_bspline(ORDER - 1, u) - cardinal_bspline(ORDER - 1, u - 1)
        return (idx[:, None] + np.arange(ORDER)[None, :]) % K, w, dw

    # -- reciprocal space
    def moduli(self, axis, K):
        """|sum_k M_5(k + 1) exp(2 pi i m k / K)|^2 for m = 0 .. K - 1, values below 1e-7 replaced by their neighbours' mean."""
        k = np.arange(ORDER - 1)
        knots = cardinal_bspline(ORDER, (k + 1).astype(self.T))
        arg = 2 * self.pi * (np.outer(np.arange(K), k) % K).astype(self.T) / K
        mod = (np.cos(arg) @ knots) ** 2 + (np.sin(arg) @ knots) ** 2
        small = mod < 1e-7
        return np.where(small, (np.roll(mod, 1) + np.roll(mod, -1)) / 2, mod)

    def frequencies(self, axis, K):
        """The integer frequency of every stored index: folded to (-K/2, K/2] on x and y, the non-negative half on z."""
        if axis == 2:
            return np.arange(K // 2 + 1)
        return np.rint(np.fft.fftfreq(K, 1.0 / K)).astype(np.int64)

    def plane_weights(self, Kz):
        """How often a stored kz plane counts in the sum over all m: twice, but for kz = 0 and, on an even mesh, kz = Kz / 2."""
        w = np.full(Kz // 2 + 1, 2.0)
        w[0] = 1.0
        if Kz % 2 == 0:
            w[-1] = 1.0
        return w.astype(self.T)

    def eterm(self, box, alpha, K, Kc):
        T = self.T
        h = [self.frequencies(a, K[a]).astype(T) / box[a] for a in range(3)]
        m2 = h[0][:, None, None] ** 2 + h[1][None, :, None] ** 2 + h[2][None, None, :] ** 2
        m2[0, 0, 0] = 1
        b = [self.moduli(a, K[a]) for a in range(3)]
        B = b[0][:, None, None] * b[1][None, :, None] * b[2][None, None, :K[2] // 2 + 1]
        et = T(Kc) * np.exp(-self.pi * self.pi * m2 / (T(alpha) * T(alpha))) / (self.pi * box[0] * box[1] * box[2] * m2 * B)
        et[0, 0, 0] = 0
        return et

    def force_charge(self, q):
        """The charge that multiplies an atom's mesh gradient."""
        return q

    # -- the whole computation; pos [n][3], q [n] hold charged atoms only
    def evaluate(self, pos, box, q, alpha, K, Kc, want_forces=True):
        T = self.T
        pos, box, q = np.asarray(pos).astype(T), np.asarray(box).astype(T), np.asarray(q).astype(T)
        K = [int(k) for k in K]
        n = len(q)
        pts, w, dw = zip(*(self.axis_terms(a, pos[:, a], box[a], K[a]) for a in range(3)))
        flat = ((pts[0][:, :, None, None] * K[1] + pts[1][:, None, :, None]) * K[2] + pts[2][:, None, None, :]).reshape(-1)
        c = q[:, None, None, None] * w[0][:, :, None, None] * w[1][:, None, :, None] * w[2][:, None, None, :]
        if self.quant:
            c = np.rint(c * T(self.quant)) / T(self.quant)
        Q = np.zeros(K[0] * K[1] * K[2], dtype=T)
        np.add.at(Q, flat, c.reshape(-1))
        S = np.fft.rfftn(Q.reshape(K), axes=(0, 1, 2))
        et = self.eterm(box, alpha, K, Kc)
        e_rec = (self.plane_weights(K[2])[None, None, :] * et * (S.real ** 2 + S.imag ** 2)).sum() / 2
        e_self = -T(Kc) * T(alpha) / np.sqrt(self.pi) * (q * q).sum()
        if not want_forces:
            return e_rec, e_self, None
        phi = np.fft.irfftn(S * et, s=K, axes=(0, 1, 2)).astype(T) * T(K[0] * K[1] * K[2])
        g = phi.reshape(-1)[flat].reshape(n, ORDER, ORDER, ORDER)
        grad = np.stack([np.einsum('ia,ib,ic,iabc->i', dw[0], w[1], w[2], g) * K[0] / box[0],
                         np.einsum('ia,ib,ic,iabc->i', w[0], dw[1], w[2], g) * K[1] / box[1],
                         np.einsum('ia,ib,ic,iabc->i', w[0], w[1], dw[2], g) * K[2] / box[2]], axis=1)
        return e_rec, e_self, -self.force_charge(q)[:, None] * grad


def run_reference(model, pos, box, q, alpha, K, Kc=KC, want_forces=True):
    """`model` (a PmeReference or a mutated copy) on all atoms: only the charged ones cost anything, the others get a zero row --
    unless the model itself hands them a charge to gather with (a planted error)."""
    pos, q = np.asarray(pos, dtype=np.float64), np.asarray(q, dtype=np.float64)
    live = model.force_charge(q) != 0
    e_rec, e_self, f = model.evaluate(pos[live], box, q[live], alpha, K, Kc, want_forces)
    if not want_forces:
        return e_rec, e_self, None
    F = np.zeros((len(q), 3), dtype=model.T)
    F[live] = f
    return e_rec, e_self, F


def pme_reference(pos, box, q, alpha, K, Kc, dtype=np.float64, quant=None):
    """(E_rec, E_self, F [n][3]) of smooth PME, order 5, on the mesh K[0] x K[1] x K[2]; quant = 2**42 rounds every spread
    contribution q wx wy wz to a multiple of 1 / quant, as a fixed-point mesh does."""
    return run_reference(PmeReference(dtype, quant), pos, box, q, alpha, K, Kc)


def tolerances(pos, box, q, alpha, K, Kc=KC):
    """What a GPU test compares with and how closely, from the reference alone.  F, E: the exact reference (E = E_rec + E_self);
    F_q, E_q: the quantised one; dF = max|F_q - F|, dE = |E_q - E|: what one realisation of the 2^-42 rounding moves;
    tol_F = 4 dF + 256 eps max|F| and tol_E = 4 dE + 256 eps (E_rec + |E_self|): four times that (the kernels' rounding is another
    realisation of the same pattern; the factor is headroom for its max-norm) plus a floor for the two transforms and the
    reduction of the energy in double precision."""
    er, es, F = pme_reference(pos, box, q, alpha, K, Kc)
    erq, esq, Fq = pme_reference(pos, box, q, alpha, K, Kc, quant=QUANT)
    eps = np.finfo(np.float64).eps
    fmax = np.abs(F).max()
    dF, dE = np.abs(Fq - F).max(), abs((erq + esq) - (er + es))
    return dict(F=F, E=er + es, E_rec=er, E_self=es, F_q=Fq, E_q=erq + esq, fmax=fmax, dF=dF, dE=dE,
                tol_F=4 * dF + 256 * eps * fmax, tol_E=4 * dE + 256 * eps * (er + abs(es)))


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# Meshes chosen from the constants of csrc/pme.hip and device_utils.h (test_pme_host.py reads them out of the sources and asserts
# that the table still straddles them): PME_TILE 8, PME_ORDER 5 (tile + halo = 12), PME_LDS_BINS 4096, KEEP 32 (x 256 threads =
# 8192 tiles), 1024 blocks of 256 atoms.
BOX = (2.0, 2.3, 1.9)                # nm: three different edges
N_SMALL = 144                        # 128 charged, 16 with q = 0
MESHES = {
    'atomic': (10, 11, 9),             # some K < 12: device atomics; odd and even axes, no Nyquist plane
    'one_tile_halo': (12, 12, 12),     # the smallest tiled mesh: every point is covered by two tiles per axis through the wrap
    'ragged': (13, 20, 27),            # no axis a multiple of 8, odd Kx and Kz
    'aligned': (16, 24, 32),           # multiples of 8
    'global_bins': (136, 136, 129),    # 17^3 = 4913 tiles: the global-counter binning kernels
    'long_scan': (168, 168, 161),      # 21^3 = 9261 tiles: the scan keeps nothing in registers
    'many_blocks': (20, 13, 27),       # 262 400 atoms: 1025 blocks in the binning kernels, thousands of atoms per tile
}
MANY_SIDE = 64                       # many_blocks: 64^3 uncharged atoms on a jittered lattice ...
MANY_CHARGED = 256                   # ... and 256 charged ones, one in every 1025 of the atom order
CASES = sorted(MESHES)
EDGE_ATOMS = {                       # name -> index among the charged atoms of a case (the same in every case)
    'origin': 0, 'far corner': 1, 'minus 1e-18': 2, 'whole boxes outside': 3, 'boxes away': 4, 'on a node': 5, 'below a node': 6}


def edge_positions(box, K):
    """The seven atoms every case carries (EDGE_ATOMS), for the box and mesh at hand."""
    L = np.asarray(box, dtype=np.float64)
    node = L * np.array([5, 7, K[2] - 1]) / np.asarray(K)
    return np.array([
        [0.0, 0.0, 0.0],
        L,
        [-1e-18, 0.3 * L[1], 0.6 * L[2]],          # t - floor(t) rounds to 1: the index wraps through the modulo
        [2 * L[0], -1 * L[1], 3 * L[2]],           # a whole number of boxes from the origin
        [-3.4 * L[0], 4.2 * L[1], -4.7 * L[2]],    # three to five boxes away in each direction
        node,                                      # on a mesh node (to the rounding of 5 L / K)
        node - 1e-13,                              # 1e-13 nm below it
    ])


def charges(rng, n, zero_every=9, zero_from=0):
    q = rng.uniform(-1.0, 1.0, n)
    q[np.abs(q) < 0.05] = 0.5                      # (a charged atom is clearly charged)
    q[zero_from::zero_every] = 0.0
    return q


def small_positions(rng, n, box, K, q):
    """Random positions over three boxes per axis; the first seven charged atoms are the edge atoms."""
    pos = rng.uniform(-1.0, 2.0, (n, 3)) * np.asarray(box)
    pos[np.flatnonzero(q)[:len(EDGE_ATOMS)]] = edge_positions(box, K)
    return pos


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """dict(name, K, box, alpha, Kc, q [n], pos [n][3]), the same arrays at every call (treat them as read-only).  seed > 0: other
    positions and charges on the same mesh."""
    K = MESHES[name]
    rng = np.random.default_rng([CASES.index(name), seed, 20240917])
    box = np.array(BOX)
    if name == 'many_blocks':
        n = MANY_SIDE ** 3 + MANY_CHARGED
        stride = n // MANY_CHARGED
        charged = np.arange(MANY_CHARGED) * stride + 3
        q = np.zeros(n)
        q[charged] = charges(rng, MANY_CHARGED, zero_every=10 ** 9, zero_from=10 ** 9)
        pos = np.empty((n, 3))
        cell = np.stack(np.meshgrid(*[np.arange(MANY_SIDE)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
        pos[q == 0] = (cell + 0.5 + rng.uniform(-0.4, 0.4, cell.shape)) / MANY_SIDE * box
        pos[charged] = small_positions(rng, MANY_CHARGED, box, K, np.ones(MANY_CHARGED))
    else:
        n = N_SMALL
        q = charges(rng, n)
        pos = small_positions(rng, n, box, K, q)
    for a in (q, pos, box):
        a.setflags(write=False)
    return dict(name=name, K=K, box=box, alpha=ALPHA, Kc=KC, q=q, pos=pos)


def one_tile_positions(c, seed=1):
    """Every atom of case c in the mesh cells [8, min(16, K)) of each axis: one tile of the tiled spread, all the others empty."""
    rng = np.random.default_rng([seed, 77])
    K = np.asarray(c['K'], dtype=np.float64)
    lo, hi = 8.0 / K, np.minimum(16.0, K) / K
    frac = lo + (hi - lo) * rng.uniform(0.01, 0.99, (len(c['q']), 3))
    return frac * c['box']


@functools.lru_cache(maxsize=None)
def case_tolerances(name):
    """tolerances() of a case's own positions and charges: computed once, shared by the tests that need it, never written to."""
    c = case(name)
    t = tolerances(c['pos'], c['box'], c['q'], c['alpha'], c['K'], c['Kc'])
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def ewald_k_sum(pos, box, q, alpha, kmax, Kc=KC):
    """(E, F) of the reciprocal-space Ewald sum itself, over every integer vector with |component| <= kmax but 0."""
    pos, box, q = np.asarray(pos, dtype=np.float64), np.asarray(box, dtype=np.float64), np.asarray(q, dtype=np.float64)
    r = np.arange(-kmax, kmax + 1)
    M = np.stack(np.meshgrid(r, r, r, indexing='ij'), axis=-1).reshape(-1, 3)
    h = M[(M != 0).any(axis=1)] / box
    m2 = (h * h).sum(axis=1)
    ph = 2 * np.pi * pos @ h.T
    Sr, Si = q @ np.cos(ph), q @ np.sin(ph)
    a = Kc * np.exp(-np.pi ** 2 * m2 / alpha ** 2) / (np.pi * box.prod() * m2)
    return 0.5 * (a * (Sr * Sr + Si * Si)).sum(), 2 * np.pi * q[:, None] * (((np.sin(ph) * Sr - np.cos(ph) * Si) * a) @ h)
