"""tests/vsite_ref.py -- numpy fp64 restatement of virtual-site placement and force spreading as csrc/vsite.hip states them.
TEST INFRASTRUCTURE ONLY.

A site table is four arrays: site [ns] (atom index of each site), kind [ns], parents [ns][3] (-1 pads a site of two parents) and
weights [ns][3]:

  AVERAGE2      s = w1 r1 + w2 r2                              f_k += w_k f
  AVERAGE3      s = w1 r1 + w2 r2 + w3 r3                      f_k += w_k f
  OUT_OF_PLANE  s = r1 + w12 r12 + w13 r13 + wc (r12 x r13)    f2 += w12 f + wc (r13 x f) ; f3 += w13 f + wc (f x r12) ;
                r12 = r2 - r1, r13 = r3 - r1                   f1 += f - (the f2 and f3 parts)

Differences of positions are plain (no minimum image), every operation is one numpy operation in the kernel's order, so that place()
rounds as the kernel does.  spread() adds to every parent its entries in the order of the sites, as the kernel's lanes do, and
zeroes the sites' rows."""
import numpy as np

AVERAGE2, AVERAGE3, OUT_OF_PLANE = range(3)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]],
                    axis=1)


def table(sites):
    """[(site, kind, parents, weights), ...] -> the four arrays."""
    ns = len(sites)
    site = np.array([s[0] for s in sites], dtype=np.int32).reshape(ns)
    kind = np.array([s[1] for s in sites], dtype=np.int32).reshape(ns)
    parents = np.full((ns, 3), -1, dtype=np.int32)
    weights = np.zeros((ns, 3))
    for row, (_, _, p, w) in enumerate(sites):
        parents[row, :len(p)] = p
        weights[row, :len(w)] = w
    return site, kind, parents, weights


def site_positions(x, site, kind, parents, weights):
    """The positions of the sites, [ns][3], from their parents' rows of x."""
    r1, r2 = x[parents[:, 0]], x[parents[:, 1]]
    r3 = x[np.maximum(parents[:, 2], 0)]
    w = weights
    # average sites: ((w1 r1) + (w2 r2)) [+ (w3 r3)]
    avg2 = w[:, 0:1] * r1 + w[:, 1:2] * r2
    avg3 = avg2 + w[:, 2:3] * r3
    # out of plane: ((r1 + w12 r12) + w13 r13) + wc (r12 x r13)
    r12, r13 = r2 - r1, r3 - r1
    oop = ((r1 + w[:, 0:1] * r12) + w[:, 1:2] * r13) + w[:, 2:3] * _cross(r12, r13)
    k = kind[:, None]
    return np.where(k == AVERAGE2, avg2, np.where(k == AVERAGE3, avg3, oop))


def place(x, site, kind, parents, weights):
    """A copy of x with the sites' rows computed from their parents'."""
    out = np.array(x, dtype=np.float64, copy=True)
    if len(site):
        out[site] = site_positions(out, site, kind, parents, weights)
    return out


def shares(x, f_site, kind, parents, weights):
    """The three parents' shares [3][ns][3] of the forces f_site [ns][3] on the sites."""
    w = weights
    r1, r2 = x[parents[:, 0]], x[parents[:, 1]]
    r3 = x[np.maximum(parents[:, 2], 0)]
    r12, r13 = r2 - r1, r3 - r1
    f2 = w[:, 0:1] * f_site + w[:, 2:3] * _cross(r13, f_site)
    f3 = w[:, 1:2] * f_site + w[:, 2:3] * _cross(f_site, r12)
    f1 = (f_site - f2) - f3
    oop = np.stack([f1, f2, f3])
    avg = np.stack([w[:, 0:1] * f_site, w[:, 1:2] * f_site, w[:, 2:3] * f_site])
    return np.where((kind == OUT_OF_PLANE)[None, :, None], oop, avg)


def spread(x, f, site, kind, parents, weights):
    """A copy of f in which every site's row went to the site's parents (J^T f at x) and is 0."""
    out = np.array(f, dtype=np.float64, copy=True)
    if not len(site):
        return out
    g = shares(x, out[site], kind, parents, weights)
    for s in range(len(site)):                      # (the order of the sites: the order in which a parent's lane adds its entries)
        for role in range(2 if kind[s] == AVERAGE2 else 3):
            out[parents[s, role]] += g[role, s]
    out[site] = 0.0
    return out
