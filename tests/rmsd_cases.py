"""The checker of the RMSDForce tests: the definition restated in 50-digit arithmetic (mpmath), and seeded generators of references
and positions.  Nothing here is a test; tests/test_rmsd_host.py checks the checker against itself and tests/test_gpu_rmsd.py the
kernels against the checker.

    c = sum x_i / N,  y'_i = y_i - sum y / N,  M = sum y'_i x_i^T,  Horn's symmetric 4 x 4 matrix of M, the eigenvector of its largest
    eigenvalue as the quaternion of the proper rotation R,  d_i = x_i - c - R y'_i,
    energy = rmsd = sqrt(sum |d_i|^2 / N),  force on i = -d_i / (N rmsd);  sum |d_i|^2 / N < 1e-20 nm^2: energy 0, zero rows.
"""
import mpmath
import numpy as np

DIGITS = 50
GUARD = 1e-20                       # nm^2
SIGMA = (1.0, 0.6, 0.35)            # nm: the anisotropic blob
OFFSET = (3.0, -2.0, 2.5)           # nm: where its centre lies


def horn_matrix(M):
    """Horn's matrix of M[a][b] = sum y'_a x_b: its top eigenvector (q0, qx, qy, qz) rotates y' onto x."""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    return [[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
            [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
            [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
            [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]]


def rotation_of(q):
    q0, q1, q2, q3 = q
    return [[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
            [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
            [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]]


def evaluate(positions, reference, particles=None, want_forces=True):
    """dict(energy, forces [n][3] (rows outside the selection zero), gap = (l1 - l2) / |l1| of Horn's matrix, rg = the radius of
    gyration of the selected reference): positions and reference are [n][3] float64 for every particle, read exactly."""
    positions = np.asarray(positions, dtype=np.float64)
    reference = np.asarray(reference, dtype=np.float64)
    sel = list(range(len(positions))) if particles is None or len(particles) == 0 else [int(p) for p in particles]
    N = len(sel)
    with mpmath.workdps(DIGITS):
        mp = mpmath.mpf
        x = [[mp(float(v)) for v in positions[i]] for i in sel]
        y = [[mp(float(v)) for v in reference[i]] for i in sel]
        c = [mpmath.fsum(r[a] for r in x) / N for a in range(3)]
        ym = [mpmath.fsum(r[a] for r in y) / N for a in range(3)]
        yc = [[r[a] - ym[a] for a in range(3)] for r in y]
        M = [[mpmath.fsum(yc[i][a] * x[i][b] for i in range(N)) for b in range(3)] for a in range(3)]
        values, vectors = mpmath.eigsy(mpmath.matrix(horn_matrix(M)))
        order = sorted(range(4), key=lambda k: values[k])
        top, second = values[order[3]], values[order[2]]
        gap = float((top - second) / abs(top)) if top != 0 else 0.0
        q = [vectors[k, order[3]] for k in range(4)]
        norm = mpmath.sqrt(mpmath.fsum(v * v for v in q))
        R = rotation_of([v / norm for v in q])
        d = [[x[i][a] - c[a] - mpmath.fsum(R[a][b] * yc[i][b] for b in range(3)) for a in range(3)] for i in range(N)]
        msd = mpmath.fsum(v * v for r in d for v in r) / N
        rg = float(mpmath.sqrt(mpmath.fsum(v * v for r in yc for v in r) / N))
        forces = np.zeros((len(positions), 3))
        if msd < mp(GUARD):
            return dict(energy=0.0, forces=forces, gap=gap, rg=rg)
        rmsd = mpmath.sqrt(msd)
        if want_forces:
            for k, i in enumerate(sel):
                forces[i] = [float(-d[k][a] / (N * rmsd)) for a in range(3)]
        return dict(energy=float(rmsd), forces=forces, gap=gap, rg=rg)


def kabsch_rmsd(positions, reference):
    """numpy's answer by the SVD of the covariance with the determinant correction (proper rotations only)."""
    x = np.asarray(positions, dtype=np.float64)
    y = np.asarray(reference, dtype=np.float64)
    x = x - x.mean(axis=0)
    y = y - y.mean(axis=0)
    U, S, Vt = np.linalg.svd(y.T @ x)
    sign = np.sign(np.linalg.det(U @ Vt))
    msd = ((x * x).sum() + (y * y).sum() - 2.0 * (S[0] + S[1] + sign * S[2])) / len(x)
    return float(np.sqrt(max(msd, 0.0)))


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return np.array(rotation_of(q), dtype=np.float64)


def blob(n, seed, offset=OFFSET, sigma=SIGMA):
    """The reference: an anisotropic Gaussian blob away from the origin, [n][3] nm."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * np.asarray(sigma) + np.asarray(offset, dtype=np.float64)


def rigid_image(reference, seed):
    """The reference rotated about its centre by a random proper rotation and translated by about a nanometre."""
    rng = np.random.default_rng(seed + 7919)
    R = random_rotation(rng)
    centre = reference.mean(axis=0)
    return (reference - centre) @ R.T + centre + rng.uniform(-1.0, 1.0, 3)


def displaced(reference, seed, noise):
    """A rigid image of the reference plus Gaussian noise of `noise` nm per coordinate."""
    rng = np.random.default_rng(seed + 104729)
    return rigid_image(reference, seed) + noise * rng.normal(size=reference.shape)


def mirror_case(n, seed, noise=0.02):
    """(reference, positions): the positions are the mirror image z -> -z of the reference plus noise."""
    ref = blob(n, seed)
    rng = np.random.default_rng(seed + 15485863)
    return ref, ref * np.array([1.0, 1.0, -1.0]) + noise * rng.normal(size=ref.shape)


def line_case(n, seed, noise=0.05):
    """(reference, positions): n atoms on one straight line; the positions are the line rotated and shifted, with noise ALONG it."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(-2.0, 2.0, n))
    u = np.array([0.48, -0.6, 0.64])                 # a unit vector
    ref = np.asarray(OFFSET) + t[:, None] * u
    w = random_rotation(rng) @ u
    pos = np.array([-1.0, 4.0, 0.5]) + (t + noise * rng.normal(size=n))[:, None] * w
    return ref, pos
