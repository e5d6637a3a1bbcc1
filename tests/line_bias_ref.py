"""numpy restatement of the per-line bias of the K solve (kmcf_k_assemble_contacts, include/kmcfield.h) and the shared
inputs of tests/test_line_bias_ref.py (CPU) and tests/test_gpu_line_bias.py.

Site classes: bit 0 metal, bit 1 uncharged vacancy; G_ij = high_G iff (cls_i & cls_j) != 0, else low_G.
rhs_i = sum over the contact sites j of row i's left, then right, contact pattern of G_ij * V_j -- here as rounded
products added one by one in pattern order; the device adds in the same order with one fused multiply-add per entry, so
the two differ by at most n_i * 2^-52 * S_i, S_i = sum |G_ij V_j| (n_i roundings of at most 2^-53 S_i on either side)."""
import functools

import numpy as np

O_EL, VACANCY = 3, 2
EPS = 2.0 ** -52


def site_classes(element, charge, metals):
    cls = np.isin(element, metals).astype(np.uint8)
    cls[(np.asarray(element) == VACANCY) & (np.asarray(charge) == 0)] |= 2
    return cls


def contact_patterns(d):
    """(left_row_ptr, left_col, right_row_ptr, right_col): for every interface row the contact sites closer than
    nn_dist, ascending, numbered inside their contact block (the layout of kmcf_kstate_pattern, which = 1 / 2)."""
    from scipy.spatial import cKDTree
    N, NL, xyz, r = d["N"], d["N_contact"], d["xyz"], d["nn_dist"]
    assert d["pbc"] == 0
    mid = xyz[NL:N - NL]
    out = []
    for block in (xyz[:NL], xyz[N - NL:]):
        near = cKDTree(block).query_ball_point(mid, r * (1 + 1e-9))
        rp, col = np.zeros(len(mid) + 1, np.int32), []
        for i, js in enumerate(near):
            js = sorted(j for j in js if np.sqrt(((mid[i] - block[j]) ** 2).sum()) < r)
            col.extend(js)
            rp[i + 1] = len(col)
        out += [rp, np.asarray(col, np.int32)]
    return tuple(out)


def contact_rhs(left_rp, left_col, right_rp, right_col, cls, NL, V, high_G, low_G, row0=0):
    """(rhs, n, S) for the rows of the patterns (interface rows row0 ...): the sum in the contract's order, the number of
    entries and the sum of the |terms| of every row."""
    n_rows = len(left_rp) - 1
    n_int = len(cls) - 2 * NL
    rhs, cnt, S = np.zeros(n_rows), np.zeros(n_rows, np.int64), np.zeros(n_rows)
    for i in np.flatnonzero((np.diff(left_rp) > 0) | (np.diff(right_rp) > 0)):
        ci = cls[NL + row0 + i]
        sites = list(left_col[left_rp[i]:left_rp[i + 1]]) + [NL + n_int + j for j in right_col[right_rp[i]:right_rp[i + 1]]]
        acc = 0.0
        for s in sites:
            term = (high_G if (ci & cls[s]) else low_G) * V[s]
            acc = acc + term
            S[i] += abs(term)
        rhs[i], cnt[i] = acc, len(sites)
    return rhs, cnt, S


def k_matrix(row_ptr, col, left_rp, left_col, right_rp, right_col, cls, NL, high_G, low_G):
    """K over ALL interface rows (scipy CSR) from the interface pattern (global interface columns) and the contact
    patterns: off-diagonals -G_ij, diagonal = sum of the row's conductances to interface, left and right neighbours."""
    import scipy.sparse as sp
    n = len(row_ptr) - 1
    n_int = len(cls) - 2 * NL
    assert n == n_int
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    ci = cls[NL:NL + n]
    off = rows != col
    g = np.where((ci[rows] & ci[col]) != 0, high_G, low_G) * off
    diag = np.bincount(rows, weights=g, minlength=n)
    for rp, cl, base in ((left_rp, left_col, 0), (right_rp, right_col, NL + n_int)):
        rr = np.repeat(np.arange(n), np.diff(rp))
        gc = np.where((ci[rr] & cls[base + cl]) != 0, high_G, low_G)
        diag += np.bincount(rr, weights=gc, minlength=n)
    assert np.count_nonzero(~off) == n                 # the pattern holds every row's diagonal entry
    data = -g
    data[~off] = diag
    return sp.csr_matrix((data, col, row_ptr), shape=(n, n)), diag


def scaled_residual(K, diag, b, phi):
    """sqrt(r . D^-1 r / b . b) of the true residual r = b - K phi."""
    r = b - K @ phi
    return float(np.sqrt((r * r / diag).sum() / (b * b).sum()))


@functools.lru_cache(maxsize=None)
def crossbar_case():
    """The device under test, once per session: synth_crossbar_40nm(tiles=1), its contact patterns and the element array
    in which every third interface site next to the left and next to the right contact is rewritten to oxygen, so that
    contact pairs of both conductance classes occur (all of them are metal-metal in the device as carved)."""
    import kmcfield_amd as km
    d = km.structure.synth_crossbar_40nm(tiles=1)
    NL = d["N_contact"]
    lrp, lcol, rrp, rcol = contact_patterns(d)
    el = d["element"].copy()
    for rp in (lrp, rrp):
        adjacent = np.flatnonzero(np.diff(rp) > 0)
        el[NL + adjacent[::3]] = O_EL
    d = dict(d, element=el)
    return dict(d=d, left_rp=lrp, left_col=lcol, right_rp=rrp, right_col=rcol)


def random_contact_values(d, seed=20241):
    """N-vector, zero in the interface, every contact slot its own value in [-8, 8] from a fixed seed."""
    NL = d["N_contact"]
    rng = np.random.default_rng(seed)
    v = np.zeros(d["N"])
    v[:NL] = rng.uniform(-8, 8, NL)
    v[d["N"] - NL:] = rng.uniform(-8, 8, NL)
    return v
