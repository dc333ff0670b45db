"""The checker of the GayBerneForce tests: the definition restated in 50-digit arithmetic (mpmath), forces by central differences of
that energy, and seeded case generators.  Nothing here is a test; tests/test_gayberne_host.py checks the checker against closed forms
and tests/test_gpu_gayberne.py the kernels against the checker.

    frame of i:  x^ = d1 / |d1|, d1 = r_i - r_x;  y^ = normalize(d2 - x^ (x^ . d2)), d2 = r_i - r_y;  z^ = x^ x y^;  A_i = rows x^ y^ z^
                 (no x-particle: the identity; no y-particle: any unit vector perpendicular to x^; minimum images when periodic)
    G_i = A_i^T diag(a^2, b^2, c^2) A_i,  B_i = A_i^T diag(ex^-1/2, ey^-1/2, ez^-1/2) A_i,  s_i = (a b + c^2) sqrt(a b),  a b c = sx/2 sy/2 sz/2
    pair:  G12 = G_1 + G_2,  B12 = B_1 + B_2,  sigma12 = (r^T G12^-1 r^ / 2)^-1/2,  h12 = r - sigma12,  rho = sigma / (h12 + sigma),
           U = 4 eps (rho^12 - rho^6),  eta = (2 s_1 s_2 / det G12)^1/2,  chi = (2 r^T B12^-1 r^)^2,  E = U eta chi S(r)
    sigma = (sigma_1 + sigma_2) / 2, eps = sqrt(eps_1 eps_2) unless an exception gives both; eps = 0: the pair is skipped;
    r >= r_c contributes nothing; S = 1 - 10 t^3 + 15 t^4 - 6 t^5, t = (r - r_s) / (r_c - r_s) between r_s and r_c.

A case is a `spec` -- dict(particles=[(sigma, eps, xparticle, yparticle, sx, sy, sz, ex, ey, ez)], exceptions=[(i, j, sigma, eps)],
method=0 / 1 / 2, cutoff, switch (None: no switching function), box (None or three edges)) -- and positions [n][3].

The gradient costs two energies per coordinate, each over the pairs of the ellipsoids whose centre or frame the coordinate moves:
about 12 N^2 pair energies for N uniaxial ellipsoids with a marker each.  Cases above a few dozen ellipsoids are therefore RECORDED
(scripts/record_gayberne_goldens.py writes tests/golden/data/gayberne_*.npz from `evaluate`); the host test recomputes a sample of
their rows."""
import functools
import os

import mpmath
import numpy as np

DIGITS = 50
STEP = '1e-20'                      # nm: the central difference's step
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'data')
NO_CUTOFF, CUTOFF_NONPERIODIC, CUTOFF_PERIODIC = 0, 1, 2


# ------------------------------------------------------------------------------------ the definition, 50 digits
def _mp(v):
    return mpmath.mpf(float(v))


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _image(d, box):
    if box is None:
        return d
    return [d[k] - box[k] * mpmath.nint(d[k] / box[k]) for k in range(3)]


def frame_of(spec, x, i, flips=(1, 1)):
    """A_i as rows [x^, y^, z^] (mpf) of particle i at the mpf positions x.  flips: signs put on d1 and d2 (the energy must not care)."""
    _, _, xp, yp = spec['particles'][i][:4]
    one, zero = mpmath.mpf(1), mpmath.mpf(0)
    if xp < 0:
        return [[one, zero, zero], [zero, one, zero], [zero, zero, one]]
    box = spec['box'] if spec['method'] == CUTOFF_PERIODIC else None
    d1 = [flips[0] * v for v in _image([x[i][k] - x[xp][k] for k in range(3)], box)]
    n1 = mpmath.sqrt(_dot(d1, d1))
    xh = [v / n1 for v in d1]
    if yp >= 0:
        d2 = [flips[1] * v for v in _image([x[i][k] - x[yp][k] for k in range(3)], box)]
    else:
        # any vector that is not parallel to x^: the coordinate axis x^ has the least of
        k = min(range(3), key=lambda a: abs(xh[a]))
        d2 = [one if a == k else zero for a in range(3)]
    t = _dot(xh, d2)
    u = [d2[k] - xh[k] * t for k in range(3)]
    nu = mpmath.sqrt(_dot(u, u))
    yh = [v / nu for v in u]
    return [xh, yh, _cross(xh, yh)]


def _sandwich(A, diag):
    """A^T diag A for the rows A."""
    return [[A[0][a] * diag[0] * A[0][b] + A[1][a] * diag[1] * A[1][b] + A[2][a] * diag[2] * A[2][b] for b in range(3)] for a in range(3)]


def record_of(spec, x, i, flips=(1, 1)):
    """(centre, G_i, B_i, s_i) of particle i."""
    _, _, _, _, sx, sy, sz, ex, ey, ez = spec['particles'][i]
    a, b, c = _mp(sx) / 2, _mp(sy) / 2, _mp(sz) / 2
    A = frame_of(spec, x, i, flips)
    G = _sandwich(A, [a * a, b * b, c * c])
    Bm = _sandwich(A, [1 / mpmath.sqrt(_mp(ex)), 1 / mpmath.sqrt(_mp(ey)), 1 / mpmath.sqrt(_mp(ez))])
    return list(x[i]), G, Bm, (a * b + c * c) * mpmath.sqrt(a * b)


def _det3(M):
    return (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
            + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))


def quad_inverse(M, v):
    """v^T M^-1 v by Cramer's rule, and det M."""
    det = _det3(M)
    w = []
    for k in range(3):
        Mk = [[v[a] if b == k else M[a][b] for b in range(3)] for a in range(3)]
        w.append(_det3(Mk) / det)
    return _dot(v, w), det


def pair_terms(spec, rec1, rec2, sigma, eps):
    """dict(E, r, sigma12, ratio = (h12 + sigma) / sigma, rho, U, eta, chi, S) of one pair, or None when it lies at or beyond the cutoff."""
    box = spec['box'] if spec['method'] == CUTOFF_PERIODIC else None
    d = _image([rec2[0][k] - rec1[0][k] for k in range(3)], box)
    r = mpmath.sqrt(_dot(d, d))
    S = mpmath.mpf(1)
    if spec['method'] != NO_CUTOFF:
        rc = _mp(spec['cutoff'])
        if r >= rc:
            return None
        if spec.get('switch') is not None and r > _mp(spec['switch']):
            t = (r - _mp(spec['switch'])) / (rc - _mp(spec['switch']))
            S = 1 - 10 * t ** 3 + 15 * t ** 4 - 6 * t ** 5
    rh = [v / r for v in d]
    G12 = [[rec1[1][a][b] + rec2[1][a][b] for b in range(3)] for a in range(3)]
    B12 = [[rec1[2][a][b] + rec2[2][a][b] for b in range(3)] for a in range(3)]
    q, detG = quad_inverse(G12, rh)
    p, _ = quad_inverse(B12, rh)
    sigma12 = 1 / mpmath.sqrt(q / 2)
    h12 = r - sigma12
    rho = sigma / (h12 + sigma)
    U = 4 * eps * (rho ** 12 - rho ** 6)
    eta = mpmath.sqrt(2 * rec1[3] * rec2[3] / detG)
    chi = (2 * p) ** 2
    return dict(E=U * eta * chi * S, r=r, sigma12=sigma12, ratio=(h12 + sigma) / sigma, rho=rho, U=U, eta=eta, chi=chi, S=S)


def mixing(spec):
    """dict (i, j) -> (sigma, eps) in mpf of every pair i < j that interacts (eps > 0), and the sorted list of particles in any."""
    parts = spec['particles']
    over = {(min(i, j), max(i, j)): (s, e) for i, j, s, e in spec.get('exceptions', [])}
    live = [i for i, p in enumerate(parts) if p[1] > 0.0]
    live = sorted(set(live) | {m for key, (_, e) in over.items() if e > 0.0 for m in key})
    out = {}
    for a in range(len(live)):
        for b in range(a + 1, len(live)):
            i, j = live[a], live[b]
            if (i, j) in over:
                s, e = over[(i, j)]
                if e > 0.0:
                    out[(i, j)] = (_mp(s), _mp(e))
            elif parts[i][1] > 0.0 and parts[j][1] > 0.0:
                out[(i, j)] = ((_mp(parts[i][0]) + _mp(parts[j][0])) / 2, mpmath.sqrt(_mp(parts[i][1]) * _mp(parts[j][1])))
    return out, live


def energy(spec, positions, flips=None):
    """The total energy (mpf) and the list of the interacting pairs' terms [(i, j, terms)].  flips: {particle: (sign of d1, sign of d2)}."""
    flips = flips or {}
    with mpmath.workdps(DIGITS):
        x = [[_mp(v) for v in row] for row in np.asarray(positions, dtype=np.float64)]
        mix, live = mixing(spec)
        recs = {i: record_of(spec, x, i, flips.get(i, (1, 1))) for i in live}
        pairs = []
        for (i, j), (s, e) in mix.items():
            t = pair_terms(spec, recs[i], recs[j], s, e)
            if t is not None:
                pairs.append((i, j, t))
        return mpmath.fsum(t['E'] for _, _, t in pairs), pairs


def evaluate(spec, positions, rows=None, totals=True):
    """dict(energy, forces [n][3], min_ratio, max_rho, n_pairs): the energy of the definition and its negative gradient by central
    differences with the step 1e-20 at 50 digits.  rows: only these particles' force rows (the others stay NaN).  totals=False: the
    force rows alone -- no pass over all pairs, the energy comes back NaN."""
    positions = np.asarray(positions, dtype=np.float64)
    n = len(positions)
    with mpmath.workdps(DIGITS):
        h = mpmath.mpf(STEP)
        x = [[_mp(v) for v in row] for row in positions]
        mix, live = mixing(spec)
        recs = {i: record_of(spec, x, i) for i in live}
        partners = {i: [] for i in live}
        terms = {}
        for (i, j), (s, e) in mix.items():
            t = pair_terms(spec, recs[i], recs[j], s, e) if totals else None
            if t is not None:
                terms[(i, j)] = t
            if t is not None or not totals:
                partners[i].append(j)
                partners[j].append(i)
        total = mpmath.fsum(t['E'] for t in terms.values()) if totals else mpmath.nan
        # whom a particle moves: itself, and the ellipsoids whose x- or y-particle it is
        moves = {p: set() for p in range(n)}
        for i in live:
            moves[i].add(i)
            for m in spec['particles'][i][2:4]:
                if m >= 0:
                    moves[m].add(i)
        forces = np.full((n, 3), np.nan)
        for p in (range(n) if rows is None else rows):
            touched = sorted(moves[p])
            keys = sorted({(min(i, j), max(i, j)) for i in touched for j in partners[i]})
            for k in range(3):
                side = []
                for sign in (1, -1):
                    keep = x[p][k]
                    x[p][k] = keep + sign * h
                    moved = dict(recs)
                    for i in touched:
                        moved[i] = record_of(spec, x, i)
                    x[p][k] = keep
                    acc = []
                    for i, j in keys:
                        t = pair_terms(spec, moved[i], moved[j], *mix[(i, j)])
                        acc.append(t['E'] if t is not None else mpmath.mpf(0))
                    side.append(mpmath.fsum(acc))
                forces[p, k] = float(-(side[0] - side[1]) / (2 * h))
        ratios = [float(t['ratio']) for t in terms.values()]
        rhos = [float(t['rho']) for t in terms.values()]
        return dict(energy=float(total), forces=forces, min_ratio=min(ratios) if ratios else float('inf'),
                    max_rho=max(rhos) if rhos else 0.0, n_pairs=len(terms))


# ------------------------------------------------------------------------------------ the same contact ratios in fp64, all pairs at once
def _mixing_float(spec):
    with mpmath.workdps(DIGITS):
        mix, live = mixing(spec)
        return {k: (float(s), float(e)) for k, (s, e) in mix.items()}, live


def ratios_float(spec, positions, tables=None):
    """(h12 + sigma) / sigma of every interacting pair inside the cutoff in numpy fp64 -- only to PLACE a case (settle); what a test
    asserts comes from the 50-digit `evaluate`.  tables: what _mixing_float(spec) returned, to save making it again."""
    pos = np.asarray(positions, dtype=np.float64)
    box = np.asarray(spec['box'], dtype=np.float64) if spec['method'] == CUTOFF_PERIODIC else None

    def image(d):
        return d if box is None else d - box * np.rint(d / box)
    mix, live = tables or _mixing_float(spec)
    G = {}
    for i in live:
        _, _, xp, yp, sx, sy, sz = spec['particles'][i][:7]
        if xp < 0:
            A = np.eye(3)
        else:
            xh = image(pos[i] - pos[xp])
            xh = xh / np.linalg.norm(xh)
            d2 = image(pos[i] - pos[yp]) if yp >= 0 else np.eye(3)[int(np.argmin(np.abs(xh)))]
            u = d2 - xh * (xh @ d2)
            yh = u / np.linalg.norm(u)
            A = np.array([xh, yh, np.cross(xh, yh)])
        G[i] = A.T @ np.diag([0.25 * sx * sx, 0.25 * sy * sy, 0.25 * sz * sz]) @ A
    if not mix:
        return np.zeros(0)
    keys = sorted(mix)
    ii, jj = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    sig = np.array([mix[k][0] for k in keys])
    Gall = np.zeros((len(pos), 3, 3))
    for i in live:
        Gall[i] = G[i]
    d = image(pos[jj] - pos[ii])
    r = np.linalg.norm(d, axis=1)
    rh = d / r[:, None]
    w = np.linalg.solve(Gall[ii] + Gall[jj], rh[:, :, None])[:, :, 0]
    sigma12 = 1.0 / np.sqrt(0.5 * np.einsum('ka,ka->k', rh, w))
    ratio = (r - sigma12 + sig) / sig
    return ratio if spec['method'] == NO_CUTOFF else ratio[r < spec['cutoff']]


def settle(spec, positions, centres, target=0.85):
    """Scale the configuration about the origin -- every centre, its markers keeping their offsets -- until the closest contact of
    `ratios_float` is `target` (bisection on the scale; a free-space case).  centres[p]: the ellipsoid particle p rides on (itself
    for an ellipsoid)."""
    pos = np.asarray(positions, dtype=np.float64)
    centres = np.asarray(centres)
    offset = pos - pos[centres]

    def at(scale):
        return pos[centres] * scale + offset
    tables = _mixing_float(spec)
    lo, hi = 0.2, 5.0
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        if ratios_float(spec, at(mid), tables).min() < target:
            lo = mid
        else:
            hi = mid
    return at(hi)


# ------------------------------------------------------------------------------------ generators
SIGMA, EPS = 0.3, 1.5
UNIAXIAL = (0.5, 0.3, 0.3, 1.0, 2.0, 2.0)          # sx sy sz ex ey ez: a prolate ellipsoid, side-by-side deeper than end-to-end
OBLATE = (0.2, 0.45, 0.45, 2.5, 0.8, 0.8)
BIAXIAL = (0.5, 0.36, 0.25, 0.8, 1.4, 2.2)
SPHERE = (0.3, 0.3, 0.3, 1.0, 1.0, 1.0)
MARKER = (SIGMA, 0.0, -1, -1) + SPHERE             # an axis particle: epsilon 0, it never interacts


def spec_of(particles, exceptions=(), method=NO_CUTOFF, cutoff=1.0, switch=None, box=None):
    return dict(particles=[tuple(p) for p in particles], exceptions=[tuple(e) for e in exceptions], method=method, cutoff=cutoff,
                switch=switch, box=None if box is None else tuple(float(v) for v in box))


def force_of(spec):
    """The openmm.GayBerneForce of a spec."""
    from atomsmm_amd import openmm
    force = openmm.GayBerneForce()
    for p in spec['particles']:
        force.addParticle(*p)
    for e in spec['exceptions']:
        force.addException(*e)
    force.setNonbondedMethod(spec['method'])
    force.setCutoffDistance(spec['cutoff'])
    if spec['switch'] is not None:
        force.setUseSwitchingFunction(True)
        force.setSwitchingDistance(spec['switch'])
    return force


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def fluid(n, seed, shape=UNIAXIAL, spacing=0.55, jitter=0.04, target=0.85, biaxial_every=0, place=True):
    """n ellipsoids on a jittered cubic lattice in free space, each with a marker 0.1 nm away in a random direction; particle 2k is
    the MARKER of ellipsoid k and particle 2k + 1 the ellipsoid, so that no active index equals its particle index.  Every
    `biaxial_every`-th ellipsoid is biaxial with a second marker appended behind all pairs.  Settled to the closest contact `target`
    (place=False: left on the lattice -- for a recorded case, whose settled positions are in its file).
    Returns (spec, positions, ellipsoid particles)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    grid = np.array([(a, b, c) for a in range(side) for b in range(side) for c in range(side)], dtype=np.float64)[:n]
    centres = (grid - grid.mean(axis=0)) * spacing + rng.uniform(-jitter, jitter, size=(n, 3))
    axes = unit_vectors(rng, n)
    particles, pos, rides = [], [], []
    for k in range(n):
        particles.append(MARKER)
        pos.append(centres[k] - 0.1 * axes[k])
        rides.append(2 * k + 1)
        particles.append((SIGMA, EPS * (1.0 + 0.25 * (k % 3)), 2 * k, -1) + tuple(shape))
        pos.append(centres[k])
        rides.append(2 * k + 1)
    if biaxial_every:
        for k in range(0, n, biaxial_every):
            # about 60 degrees off d1: the frame rolls when the x-marker moves
            side_dir = np.cross(axes[k], unit_vectors(rng, 1)[0])
            side_dir /= np.linalg.norm(side_dir)
            d2 = 0.12 * (0.5 * axes[k] + np.sqrt(0.75) * side_dir)
            particles.append(MARKER)
            pos.append(centres[k] - d2)
            rides.append(2 * k + 1)
            particles[2 * k + 1] = particles[2 * k + 1][:3] + (len(particles) - 1,) + BIAXIAL
    spec = spec_of(particles)
    pos = np.array(pos)
    if n > 1 and place:
        pos = settle(spec, pos, rides, target)
    return spec, pos, [2 * k + 1 for k in range(n)]


def golden_path(name):
    return os.path.join(GOLDEN, 'gayberne_%s.npz' % name)


@functools.lru_cache(maxsize=None)
def golden(name):
    """The recorded answer of `evaluate` for a large case: dict(positions, energy, forces, min_ratio, max_rho, n_pairs)."""
    with np.load(golden_path(name)) as z:
        out = {k: (z[k].copy() if z[k].ndim else z[k].item()) for k in z.files}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def exceptions_72(place=True):
    """72 ellipsoids: row 0 holds 70 exceptions (every third an override, the others epsilon 0), ellipsoid 1 one override with
    ellipsoid 71, ellipsoid 2 none besides row 0's."""
    spec, pos, ell = fluid(72, 172, place=place)
    ex = []
    for k in range(1, 71):
        ex.append((ell[0], ell[k], 0.28 + 0.0005 * k, 0.9 + 0.01 * k) if k % 3 == 0 else (ell[k], ell[0], 0.3, 0.0))
    ex.append((ell[71], ell[1], 0.33, 2.5))
    spec['exceptions'] = ex
    return spec, pos, ell


# the recorded cases: name -> generator(place) of (spec, positions, ellipsoid particles)
RECORDED = {
    'n63': lambda place=True: fluid(63, 163, place=place), 'n64': lambda place=True: fluid(64, 164, biaxial_every=5, place=place),
    'n65': lambda place=True: fluid(65, 165, place=place), 'n129': lambda place=True: fluid(129, 229, shape=OBLATE, spacing=0.5, place=place),
    'n257': lambda place=True: fluid(257, 357, biaxial_every=16, place=place), 'exc72': exceptions_72,
}


@functools.lru_cache(maxsize=None)
def recorded(name):
    """(spec, positions, ellipsoid particles, the recorded answer) of a recorded case, the positions those of its file."""
    spec, _, ell = RECORDED[name](place=False)
    out = golden(name)
    return spec, out['positions'], ell, out
