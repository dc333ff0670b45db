"""Reference for the CMAP tests: energy and forces of CMAPTorsionForce terms in numpy fp64, independent of atomsmm_amd.tables and of
the 16-coefficient form the device reads.

The interpolant is evaluated as what it is defined to be, the tensor-product periodic cubic spline through the map, with
scipy.interpolate.CubicSpline(bc_type='periodic'): spline along phi through every psi column at the term's phi (value and first
derivative), then spline along psi through those values.  energy[i + size * j] is the map at phi = 2 pi i / size, psi = 2 pi j / size.

Dihedrals follow PeriodicTorsionForce's convention: with F = x1 - x2, G = x2 - x3, H = x4 - x3, A = F x G, B = H x G the angle is
atan2((B x A) . G / |G|, A . B); its Cartesian gradient is written out below and checked against central differences in
tests/test_cmap_host.py."""
import numpy as np
from scipy.interpolate import CubicSpline

TWO_PI = 2.0 * np.pi


def as_grid(size, energy):
    """f[i, j]: the map at phi index i, psi index j."""
    return np.asarray(energy, dtype=np.float64).reshape(size, size).T


class MapSpline:
    """The tensor-product periodic cubic spline through one map."""

    def __init__(self, size, energy):
        self.size = int(size)
        f = as_grid(self.size, energy)
        self.x = np.arange(self.size + 1) * (TWO_PI / self.size)
        self.along_phi = CubicSpline(self.x, np.concatenate([f, f[:1]], axis=0), axis=0, bc_type='periodic')     # one spline per psi column

    def _along_psi(self, values):
        return CubicSpline(self.x, np.append(values, values[0]), bc_type='periodic')

    def __call__(self, phi, psi):
        """(E, dE/dphi, dE/dpsi) at angles in radians (any branch)."""
        phi, psi = np.mod(phi, TWO_PI), np.mod(psi, TWO_PI)
        through_values = self._along_psi(self.along_phi(phi))
        through_slopes = self._along_psi(self.along_phi(phi, 1))
        return float(through_values(psi)), float(through_slopes(psi)), float(through_values(psi, 1))


def min_image(d, box):
    return d if box is None else d - box * np.rint(d / box)


def dihedral(x, atoms, box=None):
    """(angle, gradient[4][3]) of the dihedral over the four atoms."""
    a, b, c, d = (x[k] for k in atoms)
    F, G, H = min_image(a - b, box), min_image(b - c, box), min_image(d - c, box)
    A, Bv = np.cross(F, G), np.cross(H, G)
    g = np.linalg.norm(G)
    angle = np.arctan2(np.dot(np.cross(Bv, A), G) / g, np.dot(A, Bv))
    a2, b2, fg, hg = np.dot(A, A), np.dot(Bv, Bv), np.dot(F, G), np.dot(H, G)
    gi = -g / a2 * A
    gl = g / b2 * Bv
    gj = g / a2 * A + fg / (a2 * g) * A - hg / (b2 * g) * Bv
    gk = -g / b2 * Bv - fg / (a2 * g) * A + hg / (b2 * g) * Bv
    return angle, np.stack([gi, gj, gk, gl])


def evaluate(positions, maps, terms, box=None, want_forces=True):
    """maps: [(size, energy)]; terms: rows (map, a1, a2, a3, a4, b1, b2, b3, b4).  Returns dict(energy, forces, angles)."""
    x = np.asarray(positions, dtype=np.float64)
    box = None if box is None else np.asarray(box, dtype=np.float64)
    splines = [MapSpline(size, energy) for size, energy in maps]
    energy, forces, angles = 0.0, np.zeros_like(x), []
    for row in terms:
        m, first, second = int(row[0]), [int(k) for k in row[1:5]], [int(k) for k in row[5:9]]
        phi, gphi = dihedral(x, first, box)
        psi, gpsi = dihedral(x, second, box)
        e, de_dphi, de_dpsi = splines[m](phi, psi)
        energy += e
        angles.append((phi, psi))
        if want_forces:
            for k in range(4):          # (np.add.at in spirit: an atom may appear in both dihedrals, or twice in one term)
                forces[first[k]] -= de_dphi * gphi[k]
                forces[second[k]] -= de_dpsi * gpsi[k]
    return dict(energy=energy, forces=forces, angles=np.array(angles).reshape(-1, 2))


# ------------------------------------------------------------------------------------ inputs
def random_map(size, seed, lo=1.0, hi=3.0):
    """Values in [lo, hi] kJ/mol: totals stay far from zero."""
    return size, np.random.default_rng(seed).uniform(lo, hi, size * size)


def chain(rng, n, start=None, bond=0.15):
    """n atoms joined by bonds of about `bond` nm in random directions that never fold back: no degenerate dihedral."""
    x = [np.zeros(3) if start is None else np.asarray(start, dtype=np.float64)]
    step = np.array([1.0, 0.0, 0.0])
    for _ in range(n - 1):
        while True:
            trial = rng.normal(size=3)
            trial /= np.linalg.norm(trial)
            if abs(np.dot(trial, step)) < 0.8:          # at least 37 degrees off the previous bond, either way
                break
        step = trial
        x.append(x[-1] + bond * rng.uniform(0.9, 1.1) * step)
    return np.array(x)


def disjoint_terms(n_terms, seed, n_maps=2, centre=2.0, spread=1.0):
    """n_terms terms over disjoint sets of eight atoms (two separate four-atom chains each), maps assigned alternately."""
    rng = np.random.default_rng(seed)
    pos, terms = [], []
    for t in range(n_terms):
        for _ in range(2):
            pos.append(chain(rng, 4, start=centre + rng.uniform(-spread, spread, 3)))
        terms.append([t % n_maps] + list(range(8 * t, 8 * t + 8)))
    return np.concatenate(pos), np.array(terms, dtype=np.int64)


def backbone(n_atoms, seed, n_maps=2, start=(1.0, 1.0, 1.0)):
    """A chain of n_atoms atoms with the backbone pattern (k .. k+3, k+1 .. k+4): n_atoms - 4 terms, an inner atom in up to eight
    records."""
    rng = np.random.default_rng(seed)
    pos = chain(rng, n_atoms, start=start)
    terms = [[k % n_maps, k, k + 1, k + 2, k + 3, k + 1, k + 2, k + 3, k + 4] for k in range(n_atoms - 4)]
    return pos, np.array(terms, dtype=np.int64)


def place_dihedral(phi, psi, bond=0.15, bend=np.deg2rad(111.0)):
    """Five atoms a-b-c-d-e with dihedral(a, b, c, d) = phi and dihedral(b, c, d, e) = psi to rounding, built atom by atom from bond
    length, bond angle and torsion (the usual internal-to-Cartesian step)."""
    def add(p1, p2, p3, torsion):
        bc = p3 - p2
        bc /= np.linalg.norm(bc)
        n = np.cross(p2 - p1, bc)
        n /= np.linalg.norm(n)
        m = np.cross(n, bc)
        d2 = np.array([-bond * np.cos(bend), bond * np.sin(bend) * np.cos(torsion), bond * np.sin(bend) * np.sin(torsion)])
        return p3 + d2[0] * bc + d2[1] * m + d2[2] * n

    a = np.array([0.0, 0.0, 0.0])
    b = np.array([bond, 0.0, 0.0])
    c = b + bond * np.array([-np.cos(bend), np.sin(bend), 0.0])
    d = add(a, b, c, phi)
    e = add(b, c, d, psi)
    return np.array([a, b, c, d, e])
