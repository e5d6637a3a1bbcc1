"""Plain dense reference of the T path under periodic y-z boundaries (kmcf_initialize_sparsity_T_pbc, csrc/kmcf_tstate.hip)
and the synthetic periodic devices it is tested on.  numpy only: no oracle, no ctypes, no GPU.

TRefPbc is tests/tpath_ref.py::TRef with ONE thing replaced: the matrix D of atom-atom distances is the library's
minimum image (include/kmcfield.h above kmcf_compute_cutoff_list_pbc), formed by tests/pbc_ref.py::dist with its c_round
(the C round, half away from zero -- np.round goes to even).  Everything downstream of D -- neighbour bonds D < nn_dist,
the ground flag, the pair rule Dt > nn_dist, the WKB values, M, the Jacobi diagonal -- is TRef's construction, restated
here line for line (tpath_ref.py itself is not edited), and every method (as_csr, imacro, power, tunnel_csr, edges, ...)
is inherited.  D_open keeps the open-boundary matrix next to it: what the cases are built for is counted on the two.

Cases (tpath_pbc_case(name)): the cubic 2.5 A lattice of tpath_ref, periods (ny, nz) * 2.5, so the crystal closes on
itself.  Counts as asserted by tests/test_tpath_pbc_ref.py (BUILT_FOR_PBC):

  pbc_nt_65           4 x 4 cross-section, L = 10, nn_dist 3.5: two cells of nn_dist per period -> the brute-force pattern
                      path.  2.5 / 10 is exact: every wrapped distance is exact.  65 points: a second mask word holding
                      one.  iy 0 <-> 2 is exactly half a period (fy = +-0.5: round goes away from zero on both sides, the
                      two orders of a pair land on -5 and +5).  Two vacancies of one layer at iy 0 and iy 3, 0.1 eV apart:
                      7.5 A and a tunnel pair under the open distance, 2.5 A and a neighbour bond under the minimum image.
  pbc_group_178       6 x 6 x 18, L = 15, nn_dist 3.5: four cells per period -> the wrapped cell grid.  Three block rows
                      with KMCF_SUB_STRIP = 2.  The ground atom (iy = iz = 5 of the last layer) has two neighbours through
                      the faces.  2.5 / 15 is inexact: wrapped distances carry rounding (test: nothing within 1e-9 A of
                      nn_dist).
  pbc_distance_edges  8 x 8 cross-section, L = 20, nn_dist 5.0: four cells of width exactly the cutoff, fy = k / 8 exact.
                      iy 0 <-> 6 (and iz likewise) is EXACTLY nn_dist through a face: neither a neighbour (d < nn_dist)
                      nor a tunnel pair (d > nn_dist); three pairs of vacancies 0.1 eV apart are placed there.
"""
import functools

import numpy as np

import pbc_ref as P
import tpath_ref as R
from tpath_ref import DEFECT, H_BAR, LD, N_EL, OXYGEN_DEFECT, Q_E, TI_EL, VACANCY, _lattice, _set_points, _vacancy

A_LAT = R.A_LAT


def min_image_matrix(pos, L):
    """D[i][j] = the library's minimum-image distance of atoms i and j, every operation as pbc_ref.dist writes it."""
    x, y, z = np.asarray(pos, np.float64).T
    return P.dist(x[:, None], y[:, None], z[:, None], x[None, :], y[None, :], z[None, :], (0.0, float(L[1]), float(L[2])))


class TRefPbc(R.TRef):
    """TRef on the minimum-image distance matrix.  Attributes as TRef, plus L (the lattice, periods L[1], L[2]) and
    D_open / Dt_open (the open-boundary distances of the same atoms / tunnel points)."""

    def __init__(self, xyz, element, charge, cb, metals, n1, layers, x_lo, x_hi, par, L):
        p = self.par = dict(par)
        self.L = tuple(float(v) for v in L)
        xyz = np.asarray(xyz, np.float64)
        element = np.asarray(element)
        # ---- atoms
        self.atom_site = np.flatnonzero((element != DEFECT) & (element != OXYGEN_DEFECT)).astype(np.int32)
        s = self.atom_site
        self.N_site = len(element)
        self.N_atom = Na = len(s)
        self.Nsub = n = Na + 1
        self.pos, self.el = xyz[s], element[s]
        self.ch, self.cb = np.asarray(charge)[s], np.asarray(cb, np.float64)[s]
        self.metals, self.n1, self.layers, self.x_lo, self.x_hi = np.asarray(metals), n1, layers, x_lo, x_hi
        x, y, z = self.pos.T
        dx, dy, dz = x[None, :] - x[:, None], y[None, :] - y[:, None], z[None, :] - z[:, None]
        self.D_open = np.sqrt(dx * dx + dy * dy + dz * dz)
        self.D = D = min_image_matrix(self.pos, self.L)                   # THE difference to TRef
        nn, hi, lo, loop = p["nn_dist"], p["high_G"], p["low_G"], p["loop_G"]
        eye = np.eye(n, dtype=bool)
        # ---- neighbour operator
        na = Na - 1
        metal = np.isin(self.el, self.metals)
        cvac = (self.el == VACANCY) & (self.ch == 0)
        near = (D[:na, :na] < nn) & ~eye[2:, 2:]
        both = (metal[:na, None] & metal[None, :na]) | (cvac[:na, None] & cvac[None, :na])
        G = np.zeros((n, n))
        G[2:, 2:] = np.where(near, np.where(both, hi, lo), 0.0)
        node = np.arange(n)
        ext = (node >= 2) & (node > (n + 1) - n1)
        inj = (node >= 2) & (node < n1 + 2)
        G[0, ext] = G[ext, 0] = hi
        G[1, inj] = G[inj, 1] = hi
        G[0, 1] = G[1, 0] = loop
        ground = np.zeros(n)
        ground[0] = hi
        ground[2:][D[:na, Na - 1] < nn] = hi                              # through the faces too
        self.ground = ground
        self.diag_neigh = (ground.astype(LD) + G.astype(LD).sum(1)).astype(np.float64)
        self.A_pattern = (G > 0) | eye
        self.A = -G
        self.A[eye] = self.diag_neigh
        self.rhs = np.zeros(n)
        self.rhs[0], self.rhs[1] = -loop * p["Vd"], loop * p["Vd"]
        # ---- tunnel points (x is not periodic: the window and the index rules are TRef's)
        a = np.arange(Na)
        window = np.isin(self.el, (TI_EL, N_EL)) & (x > x_lo) & (x < x_hi)
        self.tunnel_idx = t = np.flatnonzero(((self.el == VACANCY) | window) & (a >= 1) & (a <= Na - 2)).astype(np.int32)
        self.n_t = nt = len(t)
        self.is_vac = v = self.el[t] == VACANCY
        self.is_metal_p = m = metal[t] & (t > (layers - 1) * n1) & (t < Na - (layers - 1) * n1)
        # ---- pair rule
        teye = np.eye(nt, dtype=bool)
        self.Dt = Dt = D[np.ix_(t, t)]
        self.Dt_open = self.D_open[np.ix_(t, t)]
        cbt = self.cb[t]
        self.dE = dE = np.abs(cbt[:, None] - cbt[None, :])
        self.c2t = c2t = (v[:, None] & m[None, :]) | (m[:, None] & v[None, :])
        self.pair_kind = kind = ((v[:, None] & v[None, :]) | c2t | (m[:, None] & m[None, :])) & ~teye
        self.pair = pair = kind & (Dt > nn) & (dE > p["tol"])
        self.S_pattern = pair | teye
        # ---- WKB values
        E1 = Q_E * p["V0"]
        self.E2 = E2 = E1 - dE
        i, j = np.nonzero(pair)
        den = np.where(c2t[i, j], dE[i, j], np.abs(E1 - E2[i, j])).astype(LD)
        prefac = LD(-(np.sqrt(2 * p["m_e"]) / H_BAR) * (2.0 / 3.0))
        e2 = E2[i, j]
        area = np.power(LD(E1), LD(1.5)) - np.where(e2 > 0, np.power(np.maximum(e2, 0).astype(LD), LD(1.5)), LD(0))
        val = np.where(e2 == 0, LD(0), -np.exp(prefac * ((1e-10 * Dt[i, j]).astype(LD) / den) * area))
        S = np.zeros((nt, nt), LD)
        S[i, j] = val
        self.diag_tunnel = (-S.sum(1)).astype(np.float64)
        self.S = S.astype(np.float64)
        self.S[i[(e2 == 0) & c2t[i, j]], j[(e2 == 0) & c2t[i, j]]] = -0.0
        self.S[teye] = self.diag_tunnel
        # ---- merged operator and the Jacobi diagonal
        self.sub_rows = rows = t + 2
        self.M = self.A.astype(LD)
        S[teye] = -S.sum(1)
        self.M[np.ix_(rows, rows)] += S
        d = self.diag_neigh.astype(LD)
        d[rows] += S[teye]
        self.diag = d.astype(np.float64)
        self.dinv = (1 / d).astype(np.float64)

    def open_pair(self):
        """the pair rule under the open distance (what kmcf_initialize_sparsity_T's state assembles)"""
        p = self.par
        return self.pair_kind & (self.Dt_open > p["nn_dist"]) & (self.dE > p["tol"])

    def wrap_bond_rows(self):
        """matrix rows (nodes) that hold at least one bond through a face"""
        na, nn = self.N_atom - 1, self.par["nn_dist"]
        wrap = (self.D[:na, :na] < nn) & ~(self.D_open[:na, :na] < nn)
        return np.flatnonzero(wrap.any(1)) + 2

    def edges_pbc(self):
        """What the periodic cases are built for, counted on this system (pairs once, i < j)."""
        p, nt, Na, t = self.par, self.n_t, self.N_atom, self.tunnel_idx
        nn, na = p["nn_dist"], Na - 1
        aup = np.triu(np.ones((na, na), bool), 1)
        up = np.triu(np.ones((nt, nt), bool), 1)
        Dn, Dn0 = self.D[:na, :na], self.D_open[:na, :na]
        pr = self.pair & up
        hot = self.pair_kind & (self.dE > p["tol"]) & up
        y, z = self.pos[t, 1], self.pos[t, 2]
        half = (np.abs(y[:, None] - y[None, :]) == 0.5 * self.L[1]) | (np.abs(z[:, None] - z[None, :]) == 0.5 * self.L[2])
        cells = P.cells_per_period(self.L, nn)
        span = self.pos.max(0) - self.pos.min(0)
        grid = min(cells) >= 3 and span[1] < self.L[1] and span[2] < self.L[2]
        return dict(
            N_atom=Na, n_t=nt, nnz_tunnel=int(self.S_pattern.sum()), block_rows=(nt + 63) // 64, remainder=nt % 64,
            wrap_bonds=int(((Dn < nn) & ~(Dn0 < nn) & aup).sum()),
            wrap_tunnel_pairs=int((pr & (self.Dt != self.Dt_open)).sum()),
            open_pair_now_neighbour=int((self.open_pair() & (self.Dt < nn) & up).sum()),
            open_pair_now_nothing=int((self.open_pair() & ~self.pair & ~(self.Dt < nn) & up).sum()),
            pairs_at_half_period=int((pr & half).sum()),
            ground_neighbours_through_face=int(((self.D[:na, Na - 1] < nn) & ~(self.D_open[:na, Na - 1] < nn)).sum()),
            ground_neighbours=int((self.D[:na, Na - 1] < nn).sum()),
            d_at_nn_through_face=int((hot & (self.Dt == nn) & (self.Dt_open != nn)).sum()),
            atoms_at_nn_through_face=int(((Dn == nn) & (Dn0 != nn) & aup).sum()),
            cells_per_period=cells, pattern_path="cells" if grid else "brute")

    def margin_to_nn(self):
        """smallest |d - nn_dist| over the atom pairs and over the candidate tunnel pairs that are NOT exactly at nn_dist"""
        nn = self.par["nn_dist"]
        na = self.N_atom - 1
        d = np.r_[self.D[:na, :self.N_atom][~np.eye(na, self.N_atom, dtype=bool)], self.Dt[self.pair_kind]]
        d = d[d != nn]
        return float(np.abs(d - nn).min())


# ------------------------------------------------------------------------------------------------ periodic devices
def _periodic(d):
    d["L"] = (d["xyz"][:, 0].max() + A_LAT, d["ny"] * A_LAT, d["nz"] * A_LAT)
    return d


def _case_pbc_nt_65():
    d = _periodic(_lattice(31, 4, 4, 7))
    lyr = d["layers"] + 3
    a = _vacancy(d, (lyr, 0, 1), charge=0)
    b = _vacancy(d, (lyr, 3, 1), charge=2)
    d["cb"][b] = d["cb"][a] + 0.1 * Q_E                                    # (same layer: the smooth edge alone would not pass tol)
    return _set_points(d, 65, [a, b])


def _case_pbc_group_178():
    d = _periodic(_set_points(_lattice(27, 6, 6, 12), 178))
    d["knobs"] = {"KMCF_SUB_STRIP": "2"}
    return d


def _case_pbc_distance_edges():
    """nn_dist = 5 A on an 8 x 8 cross-section of period 20 A: iy 0 <-> 6 is 15 A apart in the open device and EXACTLY
    5.0 through the face (fy = 0.75 -> -0.25, dy = -5, all exact).  Three pairs of vacancies 0.1 eV apart sit there (two
    through the y face, one through the z face).
    Pairs one ulp either side of nn_dist through a face are left out: they cannot be built with exact arithmetic.  One ulp
    of 5.0 is 2^-50.  The wrapped component is L (fy - round fy) with L = 20: it is exact only where the offset over 20 is
    a dyadic fraction, i.e. for offsets that are multiples of 5 2^k, so a wrapped leg moves the distance by multiples
    of 5 2^k, never by 2^-50; and the 3-4-5 triangle of tpath_ref's open case needs a wrapped leg of 3 or 4, i.e. an
    offset of 16 or 17, and 16 / 20, 17 / 20 are not floating-point numbers.  (The open one-ulp pairs are in
    tpath_ref's distance_edges, which the periodic entry point runs unchanged with pbc = 0.)"""
    d = _periodic(_lattice(32, 8, 8, 7, p_vac=0.1))
    d["par"]["nn_dist"] = 5.0
    L0 = d["layers"]
    keep = []
    for lyr, ka, kb in ((L0 + 1, (0, 2), (6, 2)), (L0 + 3, (1, 5), (7, 5)), (L0 + 5, (3, 0), (3, 6))):
        a = _vacancy(d, (lyr,) + ka, charge=0)
        b = _vacancy(d, (lyr,) + kb, charge=2)
        d["cb"][b] = d["cb"][a] + 0.1 * Q_E
        keep += [a, b]
    return _set_points(d, 180, keep)


CASES_PBC = ("pbc_nt_65", "pbc_group_178", "pbc_distance_edges")

# What each case exists for: asserted against TRefPbc.edges_pbc() by tests/test_tpath_pbc_ref.py.
BUILT_FOR_PBC = {
    "pbc_nt_65": dict(N_atom=208, n_t=65, nnz_tunnel=3471, block_rows=2, remainder=1, wrap_bonds=102, wrap_tunnel_pairs=398,
                      open_pair_now_neighbour=1, pairs_at_half_period=762, ground_neighbours_through_face=2, ground_neighbours=5,
                      d_at_nn_through_face=0, cells_per_period=(2, 2), pattern_path="brute"),
    "pbc_group_178": dict(N_atom=648, n_t=178, nnz_tunnel=27932, block_rows=3, remainder=50, wrap_bonds=214, wrap_tunnel_pairs=4683,
                          open_pair_now_neighbour=0, pairs_at_half_period=4252, ground_neighbours_through_face=2, ground_neighbours=5,
                          d_at_nn_through_face=0, cells_per_period=(4, 4), pattern_path="cells"),
    "pbc_distance_edges": dict(N_atom=832, n_t=180, nnz_tunnel=23388, block_rows=3, remainder=52, wrap_bonds=1692, wrap_tunnel_pairs=3906,
                               open_pair_now_neighbour=19, open_pair_now_nothing=3, pairs_at_half_period=2769,
                               ground_neighbours_through_face=10, ground_neighbours=17, d_at_nn_through_face=3,
                               atoms_at_nn_through_face=414, cells_per_period=(4, 4), pattern_path="cells"),
}
# counts that must not be zero in a case (the edge the table of the module docstring names for it)
NONZERO_PBC = {
    "pbc_nt_65": ("wrap_bonds", "wrap_tunnel_pairs", "open_pair_now_neighbour", "pairs_at_half_period", "ground_neighbours_through_face"),
    "pbc_group_178": ("wrap_bonds", "wrap_tunnel_pairs", "ground_neighbours_through_face"),
    "pbc_distance_edges": ("wrap_bonds", "wrap_tunnel_pairs", "d_at_nn_through_face"),
}


@functools.lru_cache(maxsize=None)
def tpath_pbc_case(name):
    """dict as tpath_ref.tpath_case, plus L (lattice: x extent, Ly, Lz) and built_for = BUILT_FOR_PBC[name]; read-only."""
    d = {"pbc_nt_65": _case_pbc_nt_65, "pbc_group_178": _case_pbc_group_178, "pbc_distance_edges": _case_pbc_distance_edges}[name]()
    d = {k: v for k, v in d.items() if k not in ("lat", "extra_site", "seed", "ny", "nz", "n_oxide")}
    d.update(name=name, metals=R.METALS.copy(), built_for=BUILT_FOR_PBC[name])
    R._ro(d["xyz"], d["element"], d["charge"], d["cb"], d["metals"])
    return d


def ref_pbc_of(case, Vd=None, charge=None, cb=None, L=None):
    par = dict(case["par"])
    if Vd is not None:
        par["Vd"] = Vd
    return TRefPbc(case["xyz"], case["element"], case["charge"] if charge is None else charge, case["cb"] if cb is None else cb,
                   case["metals"], case["n1"], case["layers"], case["x_lo"], case["x_hi"], par, case["L"] if L is None else L)


@functools.lru_cache(maxsize=None)
def case_ref_pbc(name, Vd=None):
    """The periodic reference system of a case (built once per process; treat as read-only), optionally at another bias."""
    return ref_pbc_of(tpath_pbc_case(name), Vd=Vd)


# ------------------------------------------------------------------------------------------------ natural-order PCG
def _seq_dot(a, b):
    return float(np.cumsum(a * b)[-1])                                    # cumsum adds strictly left to right


def pcg_natural(ref, tol, max_it):
    """Plain float64 Jacobi-PCG on the float64 entries of ref.M from a zero start, every sum in natural order (a row's
    products in ascending column order, a dot product in ascending row order), stopping as the library does: while
    r.z / b.b > tol^2.  Returns (x, iterations)."""
    M64 = ref.M.astype(np.float64)
    pattern = M64 != 0
    n, width = len(M64), int(pattern.sum(1).max())
    # rows padded to one width (entries in ascending column order, then zeros: adding 0.0 changes nothing)
    pcol, pval = np.zeros((n, width), np.int64), np.zeros((n, width))
    for i in range(n):
        c = np.flatnonzero(pattern[i])
        pcol[i, :len(c)], pval[i, :len(c)] = c, M64[i, c]

    def spmv(v):
        prod = pval * v[pcol]
        acc = np.zeros(n)
        for k in range(width):                                           # a row's k-th product onto its sum: left to right
            acc += prod[:, k]
        return acc

    dinv = 1.0 / np.diag(M64)
    b = ref.rhs.astype(np.float64)
    x = np.zeros_like(b)
    r = b.copy()
    z = r * dinv
    bb, rz = _seq_dot(b, b), _seq_dot(r, z)
    p = z.copy()
    k = 0
    while rz / bb > tol * tol and k < max_it:
        Ap = spmv(p)
        a = rz / _seq_dot(p, Ap)
        x += a * p
        r -= a * Ap
        z = r * dinv
        rz_new = _seq_dot(r, z)
        p = (rz_new / rz) * p + z
        rz = rz_new
        k += 1
    return x, k


@functools.lru_cache(maxsize=None)
def pcg_natural_case(name, Vd, tol):
    ref = case_ref_pbc(name, Vd)
    x, k = pcg_natural(ref, tol, 20000)
    x.flags.writeable = False
    return x, k
