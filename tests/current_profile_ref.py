"""Restatement of kmcf_current_profile (include/kmcfield.h) in numpy, on top of current_map_ref.pair_list: the current
through x-planes per cell and pair kind from the DIRECT pair definition (a counted pair r -> s is added to plane k iff
q(r) <= k < q(s)), the node-keyed form the device uses (per-node sums of the pairs that leave the node's slab, binned by
cell and slab, prefix over k), the per-atom current vector, and per output the quantities the bounds are made of.

Bounds.  Profile entry (c, k, t): 2**-52 * (n_pairs + n_atoms + n_planes) * sum |I|, the sum and the two counts over the
counted pairs of (c, t) whose left end has q <= k and over their left ends: every addend of any way to form the entry is
one of those |I|, and that many additions are made in whatever order (first order, like the current map's bound).
Vector component of atom a: n_a * 2**-52 * sum_s |I_as d_as|, two summation orders of the same n_a terms."""
import numpy as np

import current_map_ref as R

EPS = R.EPS


def slabs(planes, x):
    """q(a): number of planes X_k <= x_a (an atom on a plane lies to its right)."""
    return np.searchsorted(np.asarray(planes, np.float64), np.asarray(x, np.float64), side="right").astype(np.int64)


def atom_cells(n_atom, atom_site, site_cell, n_cells):
    """cell(a) = site_cell[atom_site[a]], everything outside [0, n_cells) mapped to n_cells; None: all in cell 0."""
    if site_cell is None:
        assert n_cells == 1
        return np.zeros(n_atom, np.int64)
    c = np.asarray(site_cell, np.int64)[np.asarray(atom_site, np.int64)[:n_atom]]
    return np.where((c >= 0) & (c < n_cells), c, n_cells)


def _round_away(f):
    """C's round(): halves away from zero (np.round sends them to the even neighbour)."""
    r = np.round(f)
    tie = np.abs(f - np.trunc(f)) == 0.5
    return np.where(tie, np.trunc(f) + np.sign(f), r)


def displacement(xyz, a, s, lattice=None):
    """d_as of atoms a -> s: plain differences, or with lattice = (Lx, Ly, Lz) the minimum image in y and z."""
    d = xyz[s] - xyz[a]
    if lattice is not None:
        for ax in (1, 2):
            f = d[:, ax] / lattice[ax]
            f = f - _round_away(f)
            d[:, ax] = f * lattice[ax]
    return d


def counted(pairs, m):
    """(a, s, I_as, is_tunnel) of the counted pairs: both ends atoms.  I = g * (m[r] - m[c]), two rounded operations."""
    r, c, g, tn = pairs
    m = np.asarray(m, np.float64)
    keep = (r >= 2) & (c >= 2)
    r, c, g, tn = r[keep], c[keep], g[keep], tn[keep]
    return r - 2, c - 2, g * (m[r] - m[c]), tn


def _bucket(cell, a, s, n_cells):
    return np.where((cell[a] == cell[s]) & (cell[a] < n_cells), cell[a], n_cells)


def profile_direct(pairs, m, x, planes, cell, n_cells):
    """F[c, k, t] straight from the definition, and its bound.  x: per atom; cell: atom_cells()."""
    a, s, i, tn = counted(pairs, m)
    q = slabs(planes, x)
    P = len(planes)
    left = q[a] < q[s]                                    # only the left end counts a pair
    a, s, i, tn = a[left], s[left], i[left], tn[left]
    key = _bucket(cell, a, s, n_cells) * 2 + tn
    nk = (n_cells + 1) * 2
    F = np.zeros((nk, P))
    for k in range(P):
        sel = (q[a] <= k) & (k < q[s])
        F[:, k] = np.bincount(key[sel], i[sel], nk)
    # the bound: pairs of (c, t) whose left end has q <= k (whether or not they still cross k), and their left ends
    flat = key * (P + 1) + q[a]
    n_pairs = np.bincount(flat, minlength=nk * (P + 1)).reshape(nk, P + 1).cumsum(1)[:, :P]
    s_abs = np.bincount(flat, np.abs(i), nk * (P + 1)).reshape(nk, P + 1).cumsum(1)[:, :P]
    ends = np.unique(key * (len(x) + 1) + a)
    flat_e = (ends // (len(x) + 1)) * (P + 1) + q[ends % (len(x) + 1)]
    n_atoms = np.bincount(flat_e, minlength=nk * (P + 1)).reshape(nk, P + 1).cumsum(1)[:, :P]
    bound = EPS * (n_pairs + n_atoms + P) * s_abs
    shape = (n_cells + 1, 2, P)
    return dict(F=F.reshape(shape).transpose(0, 2, 1).copy(), bound=bound.reshape(shape).transpose(0, 2, 1).copy(),
                n_crossing=int(len(a)))


def profile_nodes(pairs, m, x, planes, cell, n_cells):
    """The node-keyed form: S_a[t][same / rest] over a's counted pairs with q(s) != q(a), summed by (cell or rest, slab),
    prefix over k."""
    a, s, i, tn = counted(pairs, m)
    q = slabs(planes, x)
    P, na = len(planes), len(x)
    out = q[a] != q[s]
    a, s, i, tn = a[out], s[out], i[out], tn[out]
    same = _bucket(cell, a, s, n_cells) < n_cells
    F = np.zeros((n_cells + 1, P, 2))
    for t in (0, 1):
        for is_same in (True, False):
            sel = (tn == bool(t)) & (same == is_same)
            S = np.bincount(a[sel], i[sel], na)
            key = (cell if is_same else np.full(na, n_cells)) * (P + 1) + q
            B = np.bincount(key, S, (n_cells + 1) * (P + 1)).reshape(n_cells + 1, P + 1)
            F[:, :, t] += B.cumsum(1)[:, :P]
    return F


def total(F):
    """TOTAL[k] in the order the header fixes: c ascending, (F[c][k][0] + F[c][k][1]) each."""
    tot = np.zeros(F.shape[1])
    for c in range(F.shape[0]):
        tot = tot + (F[c, :, 0] + F[c, :, 1])
    return tot


def flux_stats(F):
    tot = total(F)
    return dict(flux_min=float(tot.min()), flux_max=float(tot.max()), plane_min=int(np.argmin(tot)), plane_max=int(np.argmax(tot)))


def vector(pairs, m, xyz, lattice=None):
    """J[a] = 1/2 sum_s (g (m_r - m_s)) * d_as per atom (n_atom x 3) and its bound n_a 2**-52 sum |I d|."""
    a, s, i, tn = counted(pairs, m)
    na = len(xyz)
    term = i[:, None] * displacement(np.asarray(xyz, np.float64), a, s, lattice)
    J = np.stack([0.5 * np.bincount(a, term[:, k], na) for k in range(3)], 1)
    n = np.bincount(a, minlength=na)
    bound = np.stack([n * EPS * np.bincount(a, np.abs(term[:, k]), na) for k in range(3)], 1)
    return dict(J=J, bound=bound, n=n)


def to_sites(N, atom_site, v):
    """Site array of a per-atom array: zero, then out[atom_site[a]] = v[a] for the atoms with a row (all but the last)."""
    out = np.zeros(N, v.dtype)
    na = len(atom_site) - 1
    out[np.asarray(atom_site)[:na]] = v[:na]
    return out
