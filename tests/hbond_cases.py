"""TEST INFRASTRUCTURE (checker only) of the hydrogen-bond force (csrc/hbond.hip): texts of CustomHbondForce, layouts of donors and
acceptors, the pairs that survive on the host, and the way to the 50-digit reference of tests/compound_cases.py.

A hydrogen-bond text over d1 d2 d3 a1 a2 a3 is rewritten to a compound-bond text over p1 .. p6 (d1..d3 -> p1..p3, a1..a3 -> p4..p6) with
a regular expression; a surviving (donor, acceptor) pair is then one bond of six particles with the donor's parameters followed by
the acceptor's, and compound_cases.exact_bond -- the text at 50 digits, forces by mpmath.diff in the atoms' own coordinates -- is the
reference.  It shares neither the compiler, the interpreter, the analytic gradients, the all-pairs scan nor the gather.

The pairs that survive are enumerated here in fp64: not excluded, and |x_d1 - x_a1| (minimum image when periodic) below the cutoff.

Inputs to avoid (`usable`): a pair within 1e-6 nm of the cutoff, and what compound_cases.usable avoids (angles within 1e-3 of 0 or
pi, dihedrals with a nearly collinear triple or within 1e-3 of the cut of atan2).  A test that filters asserts that it kept at least
95 % of the surviving pairs (`MIN_KEPT`); the seeds below are chosen so that the reference alone meets that, and
tests/test_hbond_host.py checks it on the CPU.
"""
import re

import numpy as np

import compound_cases as C

MIN_KEPT = C.MIN_KEPT
CUTOFF_MARGIN = 1e-6
_PARTICLE = re.compile(r'\b([da])([123])\b')

_V16 = ('kd*(distance(d1,a1)-r0)^2 + 0.3*kd*(distance(d2,a1)-r0)^2 + 0.2*(distance(d1,a2)-r0)^2 + 0.1*(distance(d3,a3)-r0)^2'
        ' + 0.1*(distance(d2,a2)-r0)^2 + 0.05*(distance(d2,d1)-0.1)^2 + 0.05*(distance(a1,a2)-0.1)^2 + 0.02*distance(d3,a1)'
        ' + ka*((angle(d2,d1,a1)-t0)^2 + 0.5*(angle(d1,a1,a2)-t0)^2 + 0.2*(angle(d3,d1,a1)-t0)^2 + 0.2*(angle(d1,a1,a3)-t0)^2'
        ' + 0.1*(angle(d2,a1,a2)-t0)^2)'
        ' + kt*(cos(dihedral(d2,d1,a1,a2)-phi) + 0.5*cos(2*dihedral(d3,d1,a1,a3)) + 0.25*cos(dihedral(d3,d2,d1,a1)))')

# name -> text, per-donor names, per-acceptor names, globals, the slots (0 .. 5) the text names
TEXTS = {
    'distance': dict(text='k*(distance(d1,a1)-r0)^2', dnames=[], anames=[], globals=dict(k=40.0, r0=0.3)),                         # V = 1
    'three': dict(text='k*(distance(d1,a1)-r0)^2*(1+cos(angle(d2,d1,a1)))*(2+cos(dihedral(d2,d1,a1,a2)-phi))', dnames=[], anames=[],
                  globals=dict(k=25.0, r0=0.3, phi=0.7)),                                                                            # V = 3
    'sixteen': dict(text=_V16, dnames=['kd', 'r0'], anames=['ka', 't0'], globals=dict(kt=3.0, phi=0.4)),                            # V = 16
    'parameters': dict(text='kd*ka*scale*(distance(d1,a1)-r0)^2*(1.5+cos(angle(d2,d1,a1)-t0))', dnames=['kd', 'r0'], anames=['ka', 't0'],
                       globals=dict(scale=1.2)),                                                                                    # V = 2
    'distance-angle': dict(text='eps*((s/distance(d1,a1))^12-(s/distance(d1,a1))^10)*cos(angle(d2,d1,a1))^2', dnames=[], anames=[],
                           globals=dict(eps=2.0, s=0.19)),                                                                           # V = 2
    'with-dihedral': dict(text='eps*((s/distance(d1,a1))^12-(s/distance(d1,a1))^10)*cos(angle(d2,d1,a1))^2*(1+0.5*cos(dihedral(d2,d1,a1,a2)))',
                          dnames=[], anames=[], globals=dict(eps=2.0, s=0.19)),                                                      # V = 3
}
N_VARIABLES = {'distance': 1, 'three': 3, 'sixteen': 16, 'parameters': 2, 'distance-angle': 2, 'with-dihedral': 3}
PARAMETER_RANGE = dict(kd=(5.0, 20.0), ka=(1.0, 4.0), r0=(0.25, 0.4), t0=(1.6, 2.4))


def compound_text(text):
    """The text over p1 .. p6: d1..d3 -> p1..p3, a1..a3 -> p4..p6."""
    return _PARTICLE.sub(lambda m: 'p%d' % (int(m.group(2)) + (3 if m.group(1) == 'a' else 0)), text)


def compound_case(name, gvalues=None):
    """The case of tests/compound_cases.py that restates text `name`: six particles, the donor's then the acceptor's parameters."""
    case = TEXTS[name]
    return dict(n=6, text=compound_text(case['text']), names=case['dnames'] + case['anames'],
                globals=dict(case['globals'] if gvalues is None else gvalues), kinks=lambda v, p, g: [])


def named_slots(name):
    """The slots 0 .. 5 that text `name` reads."""
    return sorted({s for _, (_, slots) in C.variables_in(compound_text(TEXTS[name]['text']))[1].items() for s in slots})


def parameters(name, count, side, seed):
    """[count][parameters] of the donors (side 'd') or the acceptors ('a') of text `name`, drawn from a fixed seed."""
    names = TEXTS[name]['dnames' if side == 'd' else 'anames']
    rng = np.random.default_rng(seed + (17 if side == 'a' else 0))
    return np.array([[rng.uniform(*PARAMETER_RANGE[p]) for p in names] for _ in range(count)], dtype=np.float64).reshape(count, len(names))


def layout(n_donors, n_acceptors, edge, seed, min_distance=0.12, place=None):
    """(positions [3 (D + A)][3], donors [D][3], acceptors [A][3]): three atoms of its own per donor and per acceptor -- the first
    uniformly in a cube of `edge`, or where place(rng, t, is_acceptor) puts it (no two atoms closer than min_distance under the
    minimum image of `edge`), the second and third 0.1 and 0.16 nm off in random directions.  Atoms 3 t .. 3 t + 2 belong to donor t;
    the acceptors follow."""
    rng = np.random.default_rng(seed)
    n = n_donors + n_acceptors
    pos = np.zeros((3 * n, 3))
    placed = np.zeros((0, 3))
    for t in range(n):
        while True:
            first = rng.uniform(0.0, edge, 3) if place is None else np.asarray(place(rng, t, t >= n_donors), dtype=np.float64)
            arms = rng.normal(size=(2, 3))
            arms = arms / np.linalg.norm(arms, axis=1)[:, None] * np.array([[0.1], [0.16]])
            trio = np.stack([first, first + arms[0], first + arms[1]])
            d = np.linalg.norm(trio[1] - trio[2])
            if d < 0.08:
                continue
            if len(placed):
                delta = placed[None, :, :] - trio[:, None, :]
                delta -= edge * np.rint(delta / edge)
                if np.sqrt((delta ** 2).sum(axis=2)).min() < min_distance:
                    continue
            break
        pos[3 * t:3 * t + 3] = trio
        placed = np.concatenate([placed, trio])
    idx = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return pos, idx[:n_donors].copy(), idx[n_donors:].copy()


def water_layout(n_mol, edge, seed):
    """(positions [3 n_mol][3], donors [2 n_mol][3], acceptors [n_mol][3], exclusions) of a water-like box: molecule m is O = 3 m,
    H = 3 m + 1, 3 m + 2 on a jittered grid; each H is a donor (H, O, -1) -- so every O is d2 of two donors -- and each O an
    acceptor (O, H1, H2); the pairs within a molecule are excluded."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n_mol ** (1.0 / 3.0)))
    cell = edge / side
    grid = np.array([(i, j, k) for i in range(side) for j in range(side) for k in range(side)], dtype=np.float64)[:n_mol]
    pos = np.zeros((3 * n_mol, 3))
    donors, acceptors, excl = [], [], []
    for m in range(n_mol):
        o = (grid[m] + 0.5) * cell + rng.uniform(-0.25, 0.25, 3) * max(cell - 0.25, 0.0)
        a = rng.normal(size=3)
        a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3))
        b /= np.linalg.norm(b)
        half = 0.5 * 1.9106
        pos[3 * m] = o
        pos[3 * m + 1] = o + 0.1 * (np.cos(half) * a + np.sin(half) * b)
        pos[3 * m + 2] = o + 0.1 * (np.cos(half) * a - np.sin(half) * b)
        donors += [[3 * m + 1, 3 * m, -1], [3 * m + 2, 3 * m, -1]]
        acceptors.append([3 * m, 3 * m + 1, 3 * m + 2])
        excl += [(2 * m, m), (2 * m + 1, m)]
    return pos, np.array(donors, dtype=np.int32), np.array(acceptors, dtype=np.int32), excl


def first_distances(pos, donors, acceptors, box=None):
    """|x_d1 - x_a1| of every (donor, acceptor) pair in fp64, [D][A]; the minimum image when a box is given."""
    d = np.asarray(pos)[np.asarray(donors)[:, 0]][:, None, :] - np.asarray(pos)[np.asarray(acceptors)[:, 0]][None, :, :]
    if box is not None:
        d = d - np.asarray(box) * np.rint(d / np.asarray(box))
    return np.sqrt((d ** 2).sum(axis=2))


def survivors(pos, donors, acceptors, exclusions=(), cutoff=None, box=None):
    """The (donor, acceptor) pairs that are not excluded and lie inside the cutoff (None: all), in donor-major order."""
    r = first_distances(pos, donors, acceptors, box)
    keep = np.ones(r.shape, dtype=bool) if cutoff is None else r < cutoff
    for d, a in exclusions:
        keep[d, a] = False
    return [(int(d), int(a)) for d, a in zip(*np.nonzero(keep))]


def members_of(donors, acceptors, pair):
    """The six atoms of a pair for the reference; a slot at -1 takes the first atom of its side (no variable reads it)."""
    d, a = np.asarray(donors)[pair[0]], np.asarray(acceptors)[pair[1]]
    return [int(x) if x >= 0 else int(d[0]) for x in d] + [int(x) if x >= 0 else int(a[0]) for x in a]


def usable(name, pos, donors, acceptors, pair, params, cutoff=None, box=None):
    """True when the pair is none of the inputs to avoid."""
    if cutoff is not None:
        r = first_distances(pos, np.asarray(donors)[[pair[0]]], np.asarray(acceptors)[[pair[1]]], box)[0, 0]
        if abs(r - cutoff) < CUTOFF_MARGIN:
            return False
    return C.usable(compound_case(name), pos, members_of(donors, acceptors, pair), params, box)


def margin_ok(pos, donors, acceptors, cutoff, box=None):
    """No pair of the layout within CUTOFF_MARGIN of the cutoff (the host's and the kernel's lists then agree)."""
    return not (np.abs(first_distances(pos, donors, acceptors, box) - cutoff) < CUTOFF_MARGIN).any()


def reference(name, pos, donors, acceptors, dpar, apar, pairs, box=None, gvalues=None):
    """(energy, forces [n][3], pairs kept, pairs looked at) of the 50-digit reference over the usable pairs of `pairs`."""
    case = compound_case(name, gvalues)
    rows, params = [], []
    for d, a in pairs:
        p = list(dpar[d]) + list(apar[a])
        if usable(name, pos, donors, acceptors, (d, a), p, None, box):
            rows.append(((d, a), members_of(donors, acceptors, (d, a))))
            params.append(p)
    energies, forces = C.bond_sum(case, [m for _, m in rows], params, pos, box)
    # (an atom that stands in for a slot at -1 collects zeros only)
    e, f = C.total(energies, forces, len(pos))
    return e, f, [p for p, _ in rows], len(pairs)


# ------------------------------------------------------------------------------------------------ the layouts of the cutoff tests
CUTOFF_EDGE, CUTOFF = 2.5, 0.9


def _ball(rng, centre, radius):
    v = rng.normal(size=3)
    return np.asarray(centre) + v / np.linalg.norm(v) * radius * rng.uniform() ** (1.0 / 3.0)


def _place_none(rng, t, acceptor):          # two clusters half a box diagonal apart
    return _ball(rng, (1.85, 1.85, 1.85) if acceptor else (0.6, 0.6, 0.6), 0.4)


def _place_few(rng, t, acceptor):           # donors in a slab at the face x = 0, acceptors in two slabs about 0.8 nm from it on either side
    y, z = rng.uniform(0.0, CUTOFF_EDGE, 2)
    if not acceptor:
        return (rng.uniform(0.05, 0.2), y, z)
    return (rng.uniform(0.9, 1.1) if t % 2 else rng.uniform(1.65, 1.85), y, z)


def _place_all(rng, t, acceptor):
    return _ball(rng, (1.25, 1.25, 1.25), 0.38)


CUTOFF_LAYOUTS = {'none': (_place_none, 0.05), 'three-percent': (_place_few, 0.12), 'twenty-percent': (None, 0.12), 'all': (_place_all, 0.05)}


def cutoff_layout(rate, n_donors=130, n_acceptors=130, seed=31):
    """(positions, donors, acceptors) for the 2.5 nm box and the 0.9 nm cutoff with survival near 0 % (two distant clusters), near 3 %
    (slabs on either side of a face: half of the survivors straddle it), 20 % (uniform) or 100 % (one cluster)."""
    place, closest = CUTOFF_LAYOUTS[rate]
    return layout(n_donors, n_acceptors, CUTOFF_EDGE, seed, min_distance=closest, place=place)
