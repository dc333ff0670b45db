"""The topology zoo of the bond-list tests: small periodic systems, each built to sit on ONE guard of amm_bonded_finalize_impl
(csrc/bonded.hip) or of the scheduler's bond-list rules (csrc/run_ops.hip), with the layout it was built for written next to it.

Guards of amm_bonded_finalize_impl, and the case that sits on each (every case also exists with its atoms renumbered by a fixed
permutation, `<name>~`, so that component slots differ from index order; a shuffled case never has mol3_ok):

  G = max_comp <= 4 ? 4 : 8          Z5 (4 atoms, G = 4) | Z6-7 (5 atoms, G = 8)
  terms_ok: max_comp <= 8            Z7-8 (8 atoms, term lanes) | Z7-9 (9 atoms: no term tables, and rule 2 declines)
  terms_ok: nref > 0                 Z10-none (no term at all)
  terms_ok: terms per comp <= G      G = 4: Z2 (4 terms, ok) | Z3 (5 terms), Z5 (6 terms);  G = 8: Z6-7, Z6-8 (ok) | Z6-9 (9 terms)
  mol3_ok: G == 4, 3 ncomp == n      Z1, Z2 (ok) | Z4-ion (a 1-atom component: 3 ncomp != n)
  mol3_ok: atoms 3c, 3c+1, 3c+2      Z4-interleaved (two waters whose indices interleave), every shuffled case
  mol3_ok: kinds 2..7 absent         Z4-ljc (one BOND_LJC term in one water)
  n_gterms: gterm >= terms_from      every case runs with the default (8192: record walk only) and with option terms_from = 1
  mixed_ok: n_gterms > 0, !terms_ok  Z8-* with terms_from = 1 (mixed) | the same at the default (not mixed) | Z1 (terms_ok: not mixed)
  mixed_ok: small = <= 4 atoms,      Z8-equal holds a 4-atom chain with 4 terms (small) | Z5's chains have 6 terms: no small component,
            <= 4 terms                  nsc == 0, not mixed although n_gterms > 0 and !terms_ok
  mixed_ok: 2 small_atoms >= n       Z8-above (2 x 270 > 289) | Z8-equal (2 x 19 == 38) | Z8-below (2 x 16 < 35: not mixed)
  an atom without records            Z4-ion, Z10-half (every other molecule is three atoms without a term), Z10-none

Not reachable, by construction (so no case):
  * `nrec_of[a] >= 12` under terms_ok.  It is tested while terms are being numbered, and a term whose number reaches G has already
    cleared terms_ok one statement earlier; so when the test runs the component holds at most G <= 8 terms, each of which names an
    atom at most once per role (arity <= 4, and a term that named one atom twice would have zero displacement -- the zoo has none), so
    an atom has at most 8 records < 12.  The same count makes `nrec_of[i] <= 4` of mol3_ok always true (G == 4: at most 4 terms).
  * `++nrec_of > 12` in the mixed branch for a component that is still small: a small component has at most 4 terms, so at most 4
    records per atom; the test can only clear `small` of a component that `> 4 terms` cleared already.
  * `nt >= 1 << 26` and the index-range refusal are argument checks, not layouts (tests/test_gpu_api.py).

Guards of the scheduler's bond-list rules (tests/test_gpu_bonded_layouts.py, (c)): rule 2 takes n x {K, M, E, K} when max_comp <= 8
(every case but Z7-9 and Z8-*), rule 3 one iteration per launch above that (Z7-9, Z8-*); rule 5 takes E, K, K, M when n_gterms > 0
(terms_from = 1), and its launch is k_mixed_eval_kicks where mixed_ok (Z8-above, Z8-equal), k_terms_gather_kicks elsewhere.

FINDING (fixtures).  Before this zoo no test ran k_inner_lanes<8, *, true, ...> (G = 8 with term lanes): it needs a set whose largest
component has 5..8 atoms and no component more than 8 terms.  The suite's bond-list sets were TIP3P water (3 atoms: G = 4),
emim-BCN4 (19 atoms: no term tables), heaq in water (the solute is one large component) and methane in water (5 atoms, but 4 bonds
+ 6 angles = 10 terms: G = 8 WITHOUT term lanes).  Z6-7, Z6-8 and Z7-8 are the first; Z6-8 also runs the BATH instantiation.

Geometries.  Molecules are built from internal coordinates (bond = r0 (1 +- 0.15), angle = theta0 +- 0.25 inside [0.5, pi - 0.5],
dihedral uniform), so that the "usable" filter (bonds within 30 % of r0, angles and both triples of a dihedral 0.3 rad from
collinear, phi 1e-3 from the atan2 cut) keeps what it draws: the zoo draws 1149 molecules and keeps every one (the filter must keep
90 %: tests/test_bonded_cases_host.py).

TOLERANCE (measured).  The unit of a force error is S_i = sum over the terms at atom i of |F_t,i|, that of an energy error sum |E_t|,
both from the mpmath reference.  W_FORCE_CPU / W_ENERGY_CPU below are the worst deviation of the plain fp64 restatement
(bonded_ref.term_np) from the reference over the atoms / cases of the zoo in those units: entries 0..7 the part of each kind, entry
8 all kinds together.  A GPU result may differ from the reference by MARGIN = 16 times entry 8, and at an atom that carries only
some of the kinds by 16 times the sum of their entries (the restatement keeps each kind's part below its entry), if that is less.  The harmonic bond dominates
(r - r0 loses eps r / |r - r0|; the zoo's bonds come within 1e-4 of r0 and some atoms have little else pulling on them).  What the
MI355X gave in the same units is recorded beside them (W_FORCE_MI355X, W_ENERGY_MI355X: the worst over test (a) of
tests/test_gpu_bonded_layouts.py, all kinds together).
"""
import numpy as np

BOND, ANGLE, LJC, NEAR, TORSION, EWALD, VIR_H, VIR_LJ = range(8)
ARITY = (2, 3, 2, 2, 4, 2, 2, 2)
MARGIN = 16.0
#               BOND     ANGLE    LJC      NEAR     TORSION  EWALD    VIR_H    VIR_LJ   all
W_FORCE_CPU = (1.2e-13, 7.0e-15, 5.0e-16, 2.8e-14, 4.0e-15, 9.0e-15, 4.2e-15, 8.0e-16, 1.2e-13)
W_ENERGY_CPU = (7.0e-16, 6.5e-17, 5.2e-18, 6.5e-17, 1.4e-17, 1.9e-18, 2.0e-17, 3.2e-19, 7.5e-16)
W_FORCE_MI355X = 9.3e-14      # the worst case is Z9 (all kinds); every other case stays below 4.6e-14
#                               (Z9's atoms without a harmonic bond: 1.3e-14, against bounds of 1.2e-13 .. 2.1e-13 from their own kinds)
W_ENERGY_MI355X = 6.7e-16
FORCE_BOUND, ENERGY_BOUND = MARGIN * W_FORCE_CPU[8], MARGIN * W_ENERGY_CPU[8]


class Case:
    def __init__(self, name, n, box, x, terms, periodic, expect, expect_tf1, note=''):
        self.name, self.n, self.box, self.note = name, int(n), np.asarray(box, dtype=np.float64), note
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        assert self.x.shape == (self.n, 3)
        # the library lays records and term slots down kind by kind, terms of a kind in the order they were added
        self.terms = sorted(terms, key=lambda t: t[0])
        self.periodic = tuple(bool(p) for p in periodic)
        self.expect, self.expect_tf1 = dict(expect), dict(expect_tf1)
        rng = np.random.default_rng([7, self.n])
        self.mass = rng.choice([1.008, 12.011, 15.9994], self.n)
        self.v = rng.normal(size=(self.n, 3)) * np.sqrt(2.494 / self.mass)[:, None]

    def kind_arrays(self, kind):
        idx = np.array([a for k, a, _ in self.terms if k == kind], dtype=np.int32).reshape(-1, ARITY[kind])
        par = np.array([p for k, _, p in self.terms if k == kind], dtype=np.float64)
        return idx, par

    def shuffled(self):
        """the same system with its atoms renumbered by a fixed permutation (atom i becomes perm[i])"""
        perm = np.random.default_rng([11, self.n]).permutation(self.n)
        x = np.empty_like(self.x)
        x[perm] = self.x
        terms = [(k, tuple(int(perm[a]) for a in at), p) for k, at, p in self.terms]
        e0, e1 = dict(self.expect, mol3_ok=0), dict(self.expect_tf1, mol3_ok=0)
        c = Case(self.name + '~', self.n, self.box, x, terms, self.periodic, e0, e1, self.note)
        c.mass = np.empty_like(self.mass); c.mass[perm] = self.mass
        c.v = np.empty_like(self.v); c.v[perm] = self.v
        c.perm = perm
        return c


# ------------------------------------------------------------------------------------------------ the finalize rules, restated
def layout(n, terms, terms_from=8192):
    """What amm_bonded_finalize_impl decides for `terms` [(kind, atoms, params)] in (kind, term) order on n atoms: the dict that
    backend.HipContext.bonded_stats returns."""
    comp = list(range(n))

    def find(a):
        while comp[a] != a:
            a = comp[a]
        return a

    for _, at, _ in terms:
        for b in at[1:]:
            ra, rb = find(at[0]), find(b)
            if ra != rb:
                comp[max(ra, rb)] = min(ra, rb)
    roots = sorted({find(i) for i in range(n)})
    members = {r: [i for i in range(n) if find(i) == r] for r in roots}
    nterm = {r: 0 for r in roots}
    for _, at, _ in terms:
        nterm[find(at[0])] += 1
    ncomp, max_comp = len(roots), max(len(m) for m in members.values())
    G = 4 if max_comp <= 4 else 8
    terms_ok = max_comp <= 8 and len(terms) > 0 and all(v <= G for v in nterm.values())
    mol3 = terms_ok and G == 4 and 3 * ncomp == n and all(members[r] == [3 * c, 3 * c + 1, 3 * c + 2] for c, r in enumerate(roots)) \
        and all(k < 2 for k, _, _ in terms)
    n_gterms = len(terms) if len(terms) >= terms_from else 0
    small = [r for r in roots if len(members[r]) <= 4 and nterm[r] <= 4]
    small_atoms = sum(len(members[r]) for r in small)
    mixed = n_gterms > 0 and not terms_ok and len(small) > 0 and 2 * small_atoms >= n
    return dict(ncomp=ncomp, max_comp=max_comp, terms_ok=int(terms_ok), G=G, mol3_ok=int(mol3), mixed_ok=int(mixed), n_gterms=n_gterms,
                n_sc=len(small) if mixed else 0)


# ------------------------------------------------------------------------------------------------ geometry
DRAWN = {'drawn': 0, 'kept': 0}


def _rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    a, b, c, d = q
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def _place(p0, p1, p2, r, theta, phi):
    """the atom bonded to p2 at distance r, angle theta with p1, dihedral phi with p0 (natural extension reference frame)"""
    bc = (p2 - p1) / np.linalg.norm(p2 - p1)
    nrm = np.cross(p1 - p0, bc)
    nrm /= np.linalg.norm(nrm)
    m = np.cross(nrm, bc)
    d = np.array([-r * np.cos(theta), r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi)])
    return p2 + d[0] * bc + d[1] * m + d[2] * nrm


def draw_chain(rng, natoms, r0=0.12, theta0=1.9):
    x = np.zeros((natoms, 3))
    r = lambda: r0 * (1.0 + rng.uniform(-0.15, 0.15))
    th = lambda: float(np.clip(theta0 + rng.uniform(-0.25, 0.25), 0.5, np.pi - 0.5))
    if natoms > 1:
        x[1] = [r(), 0, 0]
    if natoms > 2:
        t, rr = th(), r()
        x[2] = x[1] + rr * np.array([-np.cos(t), np.sin(t), 0])
    for k in range(3, natoms):
        x[k] = _place(x[k - 3], x[k - 2], x[k - 1], r(), th(), rng.uniform(-np.pi, np.pi))
    return x


def angle_of(a, b, c):
    d1, d2 = a - b, c - b
    return float(np.arctan2(np.linalg.norm(np.cross(d1, d2)), d1 @ d2))


def dihedral_of(a, b, c, d):
    b1, b2, b3 = b - a, c - b, d - c
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    return float(np.arctan2(np.linalg.norm(b2) * (b1 @ n2), n1 @ n2))


def usable(x, terms):
    """the filter of the well-conditioned zoo over one molecule (local atom numbers)"""
    for kind, at, p in terms:
        if kind == BOND:
            r = np.linalg.norm(x[at[0]] - x[at[1]])
            if abs(r - p[0]) > 0.3 * p[0]:
                return False
        elif kind == ANGLE:
            if not 0.3 <= angle_of(x[at[0]], x[at[1]], x[at[2]]) <= np.pi - 0.3:
                return False
        elif kind == TORSION:
            for tri in ((0, 1, 2), (1, 2, 3)):
                if not 0.3 <= angle_of(*(x[at[q]] for q in tri)) <= np.pi - 0.3:
                    return False
            if np.pi - abs(dihedral_of(*(x[a] for a in at))) < 1e-3:
                return False
    return True


def draw_usable(rng, natoms, terms, **kw):
    while True:
        x = draw_chain(rng, natoms, **kw)
        DRAWN['drawn'] += 1
        if usable(x, terms):
            DRAWN['kept'] += 1
            return x


def lattice(nmol, spacing=0.75):
    side = int(np.ceil(nmol ** (1.0 / 3.0)))
    g = (np.arange(side) + 0.5) * spacing
    c = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3)[:nmol]
    return c, np.full(3, side * spacing)


# ------------------------------------------------------------------------------------------------ molecule templates (local numbering)
KB, KA = 3.0e5, 450.0
HH = 2 * 0.12 * np.sin(1.9 / 2)


def _bonds(n):
    return [(BOND, (i, i + 1), (0.12, KB * (1 + 0.1 * (i % 3)))) for i in range(n - 1)]


def _angles(n, count=None):
    out = [(ANGLE, (i, i + 1, i + 2), (1.9, KA * (1 + 0.2 * (i % 2)))) for i in range(n - 2)]
    return out if count is None else out[:count]


def _torsions(n, count=None):
    out = [(TORSION, (i, i + 1, i + 2, i + 3), (float(1 + i % 3), (0.0, np.pi, 1.1)[i % 3], 4.0 + i)) for i in range(n - 3)]
    return out if count is None else out[:count]


WATER = [(BOND, (0, 1), (0.12, KB)), (BOND, (0, 2), (0.12, 1.1 * KB)), (ANGLE, (1, 0, 2), (1.9, KA))]            # centre in slot 0
TRI4 = [(BOND, (1, 0), (0.12, KB)), (BOND, (1, 2), (0.12, 1.1 * KB)), (BOND, (0, 2), (HH, 0.2 * KB)), (ANGLE, (0, 1, 2), (1.9, KA))]   # centre in slot 1
TRI5 = TRI4 + [(ANGLE, (1, 0, 2), (0.62, 0.5 * KA))]
CHAIN4 = _bonds(4) + _angles(4) + _torsions(4)                       # 3 + 2 + 1 = 6 terms
CHAIN4_SMALL = _bonds(4) + _angles(4, 1)                             # 3 + 1 = 4 terms: a small component of a mixed set
CHAIN5 = {7: _bonds(5) + _angles(5), 8: _bonds(5) + _angles(5) + _torsions(5, 1), 9: _bonds(5) + _angles(5) + _torsions(5)}
CHAIN8 = _bonds(8) + _angles(8, 1)                                   # 7 + 1 = 8 terms on 8 atoms
CHAIN9 = _bonds(9) + _angles(9, 2)
CHAIN19 = _bonds(19) + _angles(19) + _torsions(19)


def water_geometry(rng, terms):
    """a three-site molecule as a chain H - O - H, renumbered to where `terms` has its centre"""
    centre = [at for k, at, _ in terms if k == ANGLE][0][1]
    x = draw_chain(rng, 3)                           # chain order: end, centre, end
    order = [0, 1, 2]
    order.remove(centre)
    out = np.empty((3, 3))
    out[centre], out[order[0]], out[order[1]] = x[1], x[0], x[2]
    return out


def assemble(name, mols, periodic=(False,) * 8, expect=None, expect_tf1=None, seed=0, note='', spacing=0.75):
    """mols: [(natoms, terms in local numbering, geometry function or None)]; molecules on a lattice, randomly turned."""
    rng = np.random.default_rng([3, seed, len(mols)])
    centres, box = lattice(len(mols), spacing)
    xs, terms, base = [], [], 0
    for (natoms, tl, geom), c in zip(mols, centres):
        if geom is not None:
            while True:
                x = geom(rng, tl)
                DRAWN['drawn'] += 1
                if usable(x, tl):
                    DRAWN['kept'] += 1
                    break
        else:
            x = draw_usable(rng, natoms, tl)
        x = (x - x.mean(0)) @ _rotation(rng).T + c
        xs.append(x)
        terms += [(k, tuple(base + a for a in at), p) for k, at, p in tl]
        base += natoms
    x = np.concatenate(xs)
    exp0 = dict(expect, n_gterms=0, mixed_ok=0, n_sc=0)
    exp1 = dict(expect, n_gterms=len(terms))
    exp1.update(expect_tf1 or {})
    return Case(name, base, box, x, terms, periodic, exp0, exp1, note)


def _stats(ncomp, max_comp, terms_ok, G, mol3_ok=0, mixed_ok=0, n_sc=0):
    return dict(ncomp=ncomp, max_comp=max_comp, terms_ok=terms_ok, G=G, mol3_ok=mol3_ok, mixed_ok=mixed_ok, n_sc=n_sc)


def build_zoo():
    W = (3, WATER, water_geometry)
    zoo = []
    # Z1: 91 waters = 273 atoms, 364 lanes of G = 4 (the last block ends at lane 108)
    zoo.append(assemble('Z1', [W] * 91, expect=_stats(91, 3, 1, 4, mol3_ok=1), seed=1))
    zoo.append(assemble('Z2', [(3, TRI4, water_geometry)] * 91, expect=_stats(91, 3, 1, 4, mol3_ok=1), seed=2))
    zoo.append(assemble('Z3', [(3, TRI5, water_geometry)] * 91, expect=_stats(91, 3, 0, 4), seed=3))
    # Z4: one condition of mol3_ok each
    z = assemble('Z4-interleaved', [W] * 91, expect=_stats(91, 3, 1, 4), seed=4)
    swap = np.arange(z.n)
    swap[:6] = [0, 2, 4, 1, 3, 5]                     # water 0 takes the indices 0, 2, 4 and water 1 the indices 1, 3, 5
    x = np.empty_like(z.x)
    x[swap] = z.x
    zoo.append(Case(z.name, z.n, z.box, x, [(k, tuple(int(swap[a]) for a in at), p) for k, at, p in z.terms], z.periodic, z.expect, z.expect_tf1))
    zoo.append(assemble('Z4-ion', [W] * 90 + [(1, [], None)], expect=_stats(91, 3, 1, 4), seed=5))
    zoo.append(assemble('Z4-ljc', [W] * 45 + [(3, WATER + [(LJC, (1, 2), (0.17, 0.1, 0.2))], water_geometry)] + [W] * 45,
                        expect=_stats(91, 3, 1, 4), seed=6))
    # Z5: 67 four-site chains with 6 terms: G = 4 without term lanes; no small component (6 > 4 terms), so never mixed
    zoo.append(assemble('Z5', [(4, CHAIN4, None)] * 67, expect=_stats(67, 4, 0, 4), seed=7))
    # Z6: 55 five-site chains = 275 atoms, 440 lanes of G = 8
    for nt in (7, 8, 9):
        zoo.append(assemble('Z6-%d' % nt, [(5, CHAIN5[nt], None)] * 55, expect=_stats(55, 5, int(nt <= 8), 8), seed=8 + nt))
    zoo.append(assemble('Z7-8', [(8, CHAIN8, None)] * 35, expect=_stats(35, 8, 1, 8), seed=20, spacing=1.1))
    zoo.append(assemble('Z7-9', [(9, CHAIN9, None)] * 31, expect=_stats(31, 9, 0, 8), seed=21, spacing=1.2))
    # Z8: waters + one 19-atom chain; small components are the waters (3 atoms, 3 terms) and, in -equal and -below, one 4-atom chain
    big = (19, CHAIN19, None)
    zoo.append(assemble('Z8-above', [W] * 45 + [big] + [W] * 45, expect=_stats(91, 19, 0, 8), expect_tf1=dict(mixed_ok=1, n_sc=90), seed=30, spacing=1.0))
    zoo.append(assemble('Z8-equal', [W] * 2 + [big] + [W] * 3 + [(4, CHAIN4_SMALL, None)], expect=_stats(7, 19, 0, 8),
                        expect_tf1=dict(mixed_ok=1, n_sc=6), seed=31, spacing=1.6))
    zoo.append(assemble('Z8-below', [W] * 2 + [big] + [W] * 2 + [(4, CHAIN4_SMALL, None)], expect=_stats(6, 19, 0, 8), seed=32, spacing=1.6))
    zoo.append(build_z9())
    # Z10: no term at all; every other molecule without a term
    zoo.append(assemble('Z10-none', [(1, [], None)] * 70, expect=_stats(70, 1, 0, 4), seed=40))
    zoo.append(assemble('Z10-half', [W, (3, [], None)] * 45, expect=_stats(45 + 135, 3, 1, 4), seed=41))
    return zoo


Z9_PERIODIC = (True, False, False, True, True, True, True, False)


def build_z9():
    """All eight kinds in one set, the periodic flag differing per kind; a box of exactly 3 nm.  Molecules of the periodic kinds
    (chains: bonds + torsion + a BOND_NEAR end-to-end pair; pairs: BOND_EWALD_EXCL + BOND_VIRIAL_HARMONIC at r = 0.05 .. 0.3 nm) have
    atoms moved by whole box edges, so their terms straddle the faces; molecules of the other kinds (angle + BOND_LJC +
    BOND_VIRIAL_LJ) stay whole.  One periodic bond has its x displacement at L/2 - 1 ulp."""
    rng = np.random.default_rng(99)
    L = 3.0
    per = [(BOND, (0, 1), (0.12, KB)), (BOND, (1, 2), (0.12, KB)), (BOND, (2, 3), (0.12, 1.2 * KB)),
           (TORSION, (0, 1, 2, 3), (2.0, 1.1, 6.0)), (NEAR, (0, 3), (-0.2, 0.28, 0.4))]
    non = [(ANGLE, (0, 1, 2), (1.9, KA)), (LJC, (0, 2), (0.15, 0.18, 0.3)), (VIR_LJ, (0, 1), (0.0, 0.11, 0.25)), (LJC, (1, 2), (-0.1, 0.1, 0.2))]
    xs, terms, base = [], [], 0
    centres, _ = lattice(64, 0.74)
    for m, c in enumerate(centres[:61]):
        which = m % 3
        if which == 0:
            tl = per
            x = draw_usable(rng, 4, [t for t in per if t[0] != NEAR])
        elif which == 1:
            tl = non
            x = draw_usable(rng, 3, non)
        else:
            r = 0.05 + 0.25 * (m // 3) / 19.0
            tl = [(EWALD, (0, 1), (-0.35,)), (VIR_H, (0, 1), (0.1, 800.0))]
            x = np.array([[0.0, 0, 0], [r, 0, 0]])
        x = (x - x.mean(0)) @ _rotation(rng).T + c
        if which != 1:
            x = x + L * rng.integers(-1, 2, size=x.shape)           # whole box edges, per atom and axis
        xs.append(x)
        terms += [(k, tuple(base + a for a in at), p) for k, at, p in tl]
        base += len(x)
    # the pair at L/2 - 1 ulp: 0 and nextafter(1.5, 0) are exact, and so is their difference
    xs.append(np.array([[0.0, 2.9, 2.9], [np.nextafter(1.5, 0.0), 2.9, 2.9]]))
    terms.append((BOND, (base, base + 1), (1.45, 500.0)))
    base += 2
    x = np.concatenate(xs)
    ncomp = 61 + 1
    exp = _stats(ncomp, 4, 0, 4)                    # a chain has 5 terms > G = 4: no term lanes
    return Case('Z9', base, np.full(3, L), x, terms, Z9_PERIODIC, dict(exp, n_gterms=0), dict(exp, n_gterms=len(terms), mixed_ok=1, n_sc=41),
                note='all kinds')


_ZOO = None


def zoo():
    """{name: Case}: the eighteen systems and their shuffled twins, built once"""
    global _ZOO
    if _ZOO is None:
        plain = build_zoo()
        _ZOO = {}
        for c in plain:
            _ZOO[c.name] = c
            _ZOO[c.name + '~'] = c.shuffled()
    return _ZOO


NAMES = ['Z1', 'Z2', 'Z3', 'Z4-interleaved', 'Z4-ion', 'Z4-ljc', 'Z5', 'Z6-7', 'Z6-8', 'Z6-9', 'Z7-8', 'Z7-9', 'Z8-above', 'Z8-equal',
         'Z8-below', 'Z9', 'Z10-none', 'Z10-half']
ALL_NAMES = [n + s for n in NAMES for s in ('', '~')]

_REFS = {}


def reference(name):
    """the mpmath reference of a case, computed once per process; a shuffled case takes its twin's, renumbered"""
    import bonded_ref
    if name not in _REFS:
        if name.endswith('~'):
            _REFS[name] = reference(name[:-1]).permuted(zoo()[name].perm)
        else:
            _REFS[name] = bonded_ref.Reference(zoo()[name])
    return _REFS[name]
