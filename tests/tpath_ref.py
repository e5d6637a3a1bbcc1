"""Plain dense reference of the T path (current solve, csrc/kmcf_tstate.hip) and the synthetic devices it is tested on.
numpy only: no oracle, no ctypes, no GPU.

What is restated is what the DEVICE is specified to compute (the formulation of the reference's GPU kernels,
src/current_solver_gpu.cu and src/initialize_sparsity_T.cu, which oracle/kmcf_oracle_T.c cites line by line) -- written
from the formulas, not from that file, as dense N x N arrays: every pair of atoms gets its distance, every pair of
tunnel points its rule and its WKB value, no cell list, no CSR, no loops over rows.  Sums are accumulated in
np.longdouble, so that no order of addition is built in.  tests/test_tpath_ref.py holds this file and the oracle to each
other on every case below and asserts what each case is built for; tests/test_gpu_tpath_synthetic.py holds the library
to this file.

Nodes: 0 extraction, 1 injection, 2 + a for atom a = 0 .. N_atom - 2.  The last atom is the ground node and is cut:
every atom within nn_dist of it carries +high_G on its diagonal, as does node 0.

Cases (tpath_case(name); cubic lattice of spacing 2.5 A, x-ordered, Ti contacts of 3 layers, interstitial DEFECT / OD
sites interleaved so that atom index != site index).  Counts as printed by `pytest tests/test_tpath_ref.py -s`:

  case            N_atom  n_t  block nnz  what it places on an edge (TRef.edges() counts)
  nt_0               208    0          0  no vacancy, empty contact window: no block at all
  nt_1               208    1          1  one vacancy: a lone diagonal (points_without_pair=1)
  nt_2               208    2          4  two vacancies 10 A and 0.5 eV apart: 2 x 2 (E2_pos=1)
  nt_63              208   63       3237  one mask word, one tile, one point short (E2_neg=411, E2_pos=1176, c2t_pairs=950)
  nt_64              208   64       3350  exactly one mask word and one tile (E2_neg=426, E2_pos=1217, c2t_pairs=980)
  nt_65              208   65       3463  a second word / block row holding one point (E2_neg=442, E2_pos=1257, c2t_pairs=1010)
  nt_128             312  128      14146  two full block rows (4 x 6 cross-section; E2_neg=1068, E2_pos=5941)
  nt_129             312  129      14373  a third block row holding one point; KMCF_SUB_STRIP=2: strips of 2 and 1 in row 0
  energy_edges       208   70       4142  dE_at_tol=15, dE_just_above_tol=3, dE_zero=164, E2_zero=10 (3 contact-to-trap),
                                          E2_neg_ulp=4, E2_pos_ulp=4, E2_neg=552, E2_pos=1474
  distance_edges     211   66       3390  nn_dist = 5 A: d_at_nn=15, d_ulp_below_nn=1, d_ulp_above_nn=1 (pairs that pass the
                                          other rules), atoms_at_nn=384 (pairs of atoms at exactly nn_dist)
  window_edges       208  100       5734  x_at_lo=15, x_ulp_above_lo=1, x_at_hi=13, x_ulp_below_hi=1; atoms 32 and 176 points
                                          but not "metal_p", 33 and 175 are; atom 0, the ground atom and one neighbour of it
                                          vacancies; vacancy neighbours: 26 charged-neutral, 18 neutral-neutral;
                                          points_without_pair=19
  group_178          648  178      27932  6 x 6 x (3 + 12 + 3): three block rows, remainder 50 (E2_neg=2699, E2_pos=11178)
"""
import functools

import numpy as np

DEFECT, OXYGEN_DEFECT, VACANCY, O_EL, HF_EL, NI_EL, TI_EL, PT_EL, N_EL = range(9)      # src/utils.h:37-44
Q_E = 1.60217663e-19                     # src/initialize_sparsity_T.cu:5
H_BAR = 1.054571817e-34                  # :6
METALS = np.array([TI_EL, N_EL], np.int32)
PAR = dict(nn_dist=3.5, Vd=2.0, high_G=1e5, low_G=1e-8, loop_G=1e7, tol=Q_E * 0.01, m_e=0.85 * 9.11e-31, V0=1.6)
A_LAT = 2.5
LD = np.longdouble


def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


def csr_of(pattern, values):
    """(row_ptr, col, val) of the entries of a dense boolean pattern, columns ascending."""
    r, c = np.nonzero(pattern)
    row_ptr = np.r_[0, np.cumsum(pattern.sum(1))].astype(np.int64)
    return row_ptr, c.astype(np.int32), values[r, c]


class TRef:
    """Everything one step of the current solve assembles, dense.  Attributes (float64 unless said otherwise):
    atom_site, el, ch, cb, pos (the atom arrays); A, A_pattern, diag_neigh, rhs (neighbour operator);
    tunnel_idx, is_vac, is_metal_p; pair_kind, pair, S_pattern, S, diag_tunnel; M (longdouble), diag, dinv;
    Dt, dE, E2, c2t (per pair of tunnel points: distance, |CB_i - CB_j|, E1 - |dCB|, contact-to-trap)."""

    def __init__(self, xyz, element, charge, cb, metals, n1, layers, x_lo, x_hi, par):
        p = self.par = dict(par)
        xyz = np.asarray(xyz, np.float64)
        element = np.asarray(element)
        # ---- atoms: every site that is neither kind of interstitial, in site order
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
        self.D = D = np.sqrt(dx * dx + dy * dy + dz * dz)                 # the expression as the kernels write it
        nn, hi, lo, loop = p["nn_dist"], p["high_G"], p["low_G"], p["loop_G"]
        eye = np.eye(n, dtype=bool)
        # ---- neighbour operator: conductances G >= 0 between the nodes, A = diag(row sums + ground) - G
        na = Na - 1
        metal = np.isin(self.el, self.metals)
        cvac = (self.el == VACANCY) & (self.ch == 0)                      # only an UNCHARGED vacancy conducts
        near = (D[:na, :na] < nn) & ~eye[2:, 2:]
        both = (metal[:na, None] & metal[None, :na]) | (cvac[:na, None] & cvac[None, :na])
        G = np.zeros((n, n))
        G[2:, 2:] = np.where(near, np.where(both, hi, lo), 0.0)
        node = np.arange(n)
        ext = (node >= 2) & (node > (n + 1) - n1)                         # the last layer's atoms, the ground atom cut off
        inj = (node >= 2) & (node < n1 + 2)                               # the first layer's atoms
        G[0, ext] = G[ext, 0] = hi
        G[1, inj] = G[inj, 1] = hi
        G[0, 1] = G[1, 0] = loop
        ground = np.zeros(n)
        ground[0] = hi
        ground[2:][D[:na, Na - 1] < nn] = hi                              # whatever the two atoms are
        self.diag_neigh = (ground.astype(LD) + G.astype(LD).sum(1)).astype(np.float64)
        self.A_pattern = (G > 0) | eye
        self.A = -G
        self.A[eye] = self.diag_neigh
        self.rhs = np.zeros(n)
        self.rhs[0], self.rhs[1] = -loop * p["Vd"], loop * p["Vd"]
        # ---- tunnel points: a vacancy of any charge, or a Ti / N atom strictly inside the x window; never atom 0,
        # never the ground atom
        a = np.arange(Na)
        window = np.isin(self.el, (TI_EL, N_EL)) & (x > x_lo) & (x < x_hi)
        self.tunnel_idx = t = np.flatnonzero(((self.el == VACANCY) | window) & (a >= 1) & (a <= Na - 2)).astype(np.int32)
        self.n_t = nt = len(t)
        self.is_vac = v = self.el[t] == VACANCY
        self.is_metal_p = m = metal[t] & (t > (layers - 1) * n1) & (t < Na - (layers - 1) * n1)
        # ---- pair rule
        teye = np.eye(nt, dtype=bool)
        self.Dt = Dt = D[np.ix_(t, t)]
        cbt = self.cb[t]
        self.dE = dE = np.abs(cbt[:, None] - cbt[None, :])
        self.c2t = c2t = (v[:, None] & m[None, :]) | (m[:, None] & v[None, :])
        self.pair_kind = kind = ((v[:, None] & v[None, :]) | c2t | (m[:, None] & m[None, :])) & ~teye
        self.pair = pair = kind & (Dt > nn) & (dE > p["tol"])
        self.S_pattern = pair | teye
        # ---- WKB values.  E1 = q V0, E2 = E1 - |dCB| (float64: the branch is taken on these numbers);
        # E2 > 0: -exp(prefac (d / den) (E1^1.5 - E2^1.5)), E2 < 0: -exp(prefac (d / den) E1^1.5), E2 == 0: 0.0,
        # den = |E1 - E2|.  The contact-to-trap branch is written there as an integration over the energy window
        # with a step dE = q * 0.01 * 1e10, far above any window: its loop runs ONCE, with den = |dCB| and
        # 0 + value as the sum (so -0.0 at E2 == 0).  That is the specified behaviour, not something to repair.
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

    # CSR views (what the library hands out)
    def neighbour_csr(self):
        return csr_of(self.A_pattern, self.A)

    def tunnel_csr(self):
        return csr_of(self.S_pattern, self.S)

    def as_csr(self):
        """The system under the attribute names of oracle.TSystem (row_ptr, col, val, sub_row_ptr, ...), so that one
        comparison serves both restatements."""
        import types
        rp, col, val = self.neighbour_csr()
        srp, scol, sval = self.tunnel_csr()
        return types.SimpleNamespace(Nsub=self.Nsub, N_atom=self.N_atom, n_t=self.n_t, row_ptr=rp, col=col, val=val, diag_neigh=self.diag_neigh,
                                     rhs=self.rhs, tunnel_idx=self.tunnel_idx, sub_row_ptr=srp, sub_col=scol, sub_val=sval,
                                     diag_tunnel=self.diag_tunnel, dinv=self.dinv, sub_rows=self.sub_rows, atom_site=self.atom_site,
                                     atom_element=self.el)

    def imacro_terms(self, m):
        c = np.flatnonzero(self.A_pattern[1] & (np.arange(self.Nsub) >= 2))
        m = np.asarray(m, np.float64)
        return self.A[1, c].astype(LD) * (m[c].astype(LD) - LD(m[1]))

    def imacro(self, m):
        """Injected current on potentials m (N_atom + 2 entries, already scaled by G0): over the entries of row 1
        with column node >= 2, sum of X[1][c] (m[c] - m[1])."""
        return float(self.imacro_terms(m).sum())

    def imacro_scale(self, m):
        """sum |X[1][c] m[1]| over ALL entries of row 1: what the 1e-11 bar of tests/test_gpu_tpath.py is relative to."""
        return float(np.abs(self.A[1, self.A_pattern[1]] * np.asarray(m)[1]).sum())

    def power(self, m, Vd, alpha, sentinel=-7.0):
        """(site_power, shifted m).  m: N_atom + 2 potentials already scaled by G0; heating shifts all of them by
        |min m[2:]|.  For atom rows r and atom columns c != r, of the neighbour part and of the tunnel part:
        ical = X[r][c] (m[r] - m[c]); ineg = -ical where ical < 0 under Vd > 0 or ical > 0 under Vd < 0, else 0;
        P[r] = sum_c ineg m[c] - (sum_c ineg) m[r], here as sum_c ineg (m[c] - m[r]) with every term formed in
        longdouble (the same number, without the cancellation).  site_power[site of a] = -alpha P for non-metal atoms
        a; every other site keeps the sentinel."""
        Na, na = self.N_atom, self.N_atom - 1
        m = np.array(m, np.float64)
        assert len(m) == Na + 2
        m = m + abs(m[2:].min())
        mm = m[2:self.Nsub]
        Xn = self.A[2:, 2:].copy()
        Xn[np.eye(na, dtype=bool)] = 0.0
        Xt = np.zeros((na, na))
        St = self.S.copy()
        St[np.eye(self.n_t, dtype=bool)] = 0.0
        Xt[np.ix_(self.tunnel_idx, self.tunnel_idx)] = St
        P = np.zeros(na, LD)
        dm = mm[:, None] - mm[None, :]                                    # m[r] - m[c], float64 as the kernels form it
        for X in (Xn, Xt):
            ical = X * dm
            neg = (ical < 0) if Vd > 0 else ((ical > 0) if Vd < 0 else np.zeros_like(ical, bool))
            ineg = np.where(neg, -ical, 0.0).astype(LD)
            P += (ineg * (mm[None, :].astype(LD) - mm[:, None].astype(LD))).sum(1)
        pw = np.full(self.N_site, sentinel)
        write = ~np.isin(self.el[:na], self.metals)
        pw[self.atom_site[:na][write]] = (-alpha * P[write]).astype(np.float64)
        return pw, m

    def edges(self):
        """What the cases are built for, counted on this system (pairs counted once, i < j)."""
        p, nt, Na, t = self.par, self.n_t, self.N_atom, self.tunnel_idx
        up = np.triu(np.ones((nt, nt), bool), 1)
        far = self.pair_kind & (self.Dt > p["nn_dist"]) & up             # pairs on which the energy rule decides
        hot = self.pair_kind & (self.dE > p["tol"]) & up                 # pairs on which the distance rule decides
        nn = p["nn_dist"]
        pr = self.pair & up
        x = self.pos[:, 0]
        inner = (np.arange(Na) >= 1) & (np.arange(Na) <= Na - 2) & np.isin(self.el, (TI_EL, N_EL))
        aup = np.triu(np.ones((Na - 1, Na - 1), bool), 1)
        Dn = self.D[:Na - 1, :Na - 1]
        vac = self.el == VACANCY
        vv = vac[:Na - 1, None] & vac[None, :Na - 1] & (Dn < nn) & aup
        q0 = self.ch[:Na - 1] == 0
        lo_i, hi_i = (self.layers - 1) * self.n1, Na - (self.layers - 1) * self.n1
        info = {int(a): (bool(self.is_vac[k]), bool(self.is_metal_p[k])) for k, a in enumerate(t)}
        return dict(
            N_atom=Na, n_t=nt, nnz_tunnel=int(self.S_pattern.sum()), block_rows=(nt + 63) // 64, remainder=nt % 64,
            dE_at_tol=int((far & (self.dE == p["tol"])).sum()),
            dE_just_above_tol=int((far & (self.dE > p["tol"]) & (self.dE <= p["tol"] * (1 + 4e-16))).sum()),
            dE_zero=int((far & (self.dE == 0)).sum()),
            E2_zero=int((pr & (self.E2 == 0)).sum()), E2_zero_c2t=int((pr & (self.E2 == 0) & self.c2t).sum()),
            E2_neg=int((pr & (self.E2 < 0)).sum()), E2_pos=int((pr & (self.E2 > 0)).sum()),
            E2_neg_ulp=int((pr & (self.E2 < 0) & (self.E2 > -1e-33)).sum()),
            E2_pos_ulp=int((pr & (self.E2 > 0) & (self.E2 < 1e-33)).sum()),
            c2t_pairs=int((pr & self.c2t).sum()),
            d_at_nn=int((hot & (self.Dt == nn)).sum()), d_ulp_below_nn=int((hot & (self.Dt == np.nextafter(nn, 0))).sum()),
            d_ulp_above_nn=int((hot & (self.Dt == np.nextafter(nn, np.inf))).sum()),
            atoms_at_nn=int(((Dn == nn) & aup).sum()),
            x_at_lo=int((inner & (x == self.x_lo)).sum()), x_ulp_above_lo=int((inner & (x == np.nextafter(self.x_lo, np.inf))).sum()),
            x_at_hi=int((inner & (x == self.x_hi)).sum()), x_ulp_below_hi=int((inner & (x == np.nextafter(self.x_hi, -np.inf))).sum()),
            idx_lo_edge=info.get(lo_i), idx_lo_next=info.get(lo_i + 1), idx_hi_edge=info.get(hi_i), idx_hi_prev=info.get(hi_i - 1),
            atom0_vacancy=bool(vac[0]), last_atom_vacancy=bool(vac[Na - 1]),
            ground_neighbour_vacancies=int((vac[:Na - 1] & (self.D[:Na - 1, Na - 1] < nn)).sum()),
            vac_neighbours_charged_neutral=int((vv & (q0[:, None] != q0[None, :])).sum()),
            vac_neighbours_neutral_neutral=int((vv & q0[:, None] & q0[None, :]).sum()),
            points_without_pair=int((self.S_pattern.sum(1) == 1).sum()))


# ------------------------------------------------------------------------------------------------ synthetic devices
def _lattice(seed, ny, nz, n_oxide, n_contact=3, p_vac=0.25, extras=None):
    """The cubic device of tests/test_oracle_T.py::small_device, with a map (layer, iy, iz) -> site and, per layer,
    extra vacancy sites (dx, y, z) appended behind the layer's lattice sites (0 <= dx < a / 2 keeps the x order)."""
    a = A_LAT
    rng = np.random.default_rng(seed)
    xyz, el, lat, extra_site = [], [], {}, []
    nl = 2 * n_contact + n_oxide
    for l in range(nl):
        oxide = n_contact <= l < n_contact + n_oxide
        for iy in range(ny):
            for iz in range(nz):
                lat[(l, iy, iz)] = len(el)
                xyz.append((l * a, iy * a, iz * a))
                el.append((VACANCY if rng.random() < p_vac else (HF_EL if (l + iy + iz) % 2 else O_EL)) if oxide else TI_EL)
        for e in (extras or {}).get(l, ()):
            extra_site.append(len(el))
            xyz.append((l * a + e[0], e[1], e[2]))
            el.append(VACANCY)
        if oxide:
            for iy in range(ny - 1):
                xyz.append((l * a + a / 2, iy * a + a / 2, a / 2))
                el.append(OXYGEN_DEFECT if rng.random() < 0.3 else DEFECT)
    xyz, el = np.array(xyz), np.array(el, np.int32)
    charge = np.where(el == VACANCY, np.where(rng.random(len(el)) < 0.5, 2, 0), 0).astype(np.int32)
    x = xyz[:, 0]
    x0, x1 = (n_contact - 1) * a, (n_contact + n_oxide) * a
    cb = Q_E * (1.0 - 2.0 * np.clip((x - x0) / (x1 - x0), 0, 1)) + Q_E * 0.003 * rng.standard_normal(len(x)) * ((x > x0) & (x < x1))
    return dict(xyz=xyz, element=el, charge=charge, cb=cb, n1=ny * nz, layers=n_contact, lat=lat, extra_site=extra_site,
                n_oxide=n_oxide, ny=ny, nz=nz, seed=seed, x_lo=(n_contact - 1) * a - 0.1, x_hi=(n_contact + n_oxide) * a + 0.1,
                par=dict(PAR), knobs={})


def _oxide_sites(d):
    L = d["layers"]
    return [d["lat"][(l, iy, iz)] for l in range(L, L + d["n_oxide"]) for iy in range(d["ny"]) for iz in range(d["nz"])]


def _count_points(d):
    el, x = d["element"], d["xyz"][:, 0]
    atom = np.flatnonzero((el != DEFECT) & (el != OXYGEN_DEFECT))
    e, xa = el[atom][1:-1], x[atom][1:-1]
    return int(((e == VACANCY) | (np.isin(e, (TI_EL, N_EL)) & (xa > d["x_lo"]) & (xa < d["x_hi"]))).sum())


def _set_points(d, target, keep=()):
    """Turn oxide lattice sites into vacancies, or vacancies into oxygen, in a fixed shuffled order until the device has
    exactly `target` tunnel points.  Sites in `keep` are left alone."""
    rng = np.random.default_rng(1000 + d["seed"])
    sites = [s for s in _oxide_sites(d) if s not in set(keep)]
    for s in rng.permutation(sites):
        n = _count_points(d)
        if n == target:
            break
        if n < target and d["element"][s] != VACANCY:
            d["element"][s], d["charge"][s] = VACANCY, 2 * int(rng.integers(0, 2))
        elif n > target and d["element"][s] == VACANCY:
            d["element"][s], d["charge"][s] = O_EL, 0
    assert _count_points(d) == target, (_count_points(d), target)
    return d


def _vacancy(d, key, charge=0, cb=None):
    s = d["lat"][key]
    d["element"][s], d["charge"][s] = VACANCY, charge
    if cb is not None:
        d["cb"][s] = cb
    return s


def _case_nt_small(k):
    d = _lattice(21, 4, 4, 7, p_vac=0.0)
    d["x_lo"], d["x_hi"] = 1e9, -1e9                                       # an empty window: no metal tunnel point
    for key in [(4, 1, 1), (8, 2, 2)][:k]:                                 # two vacancies 10 A and 0.5 eV apart
        _vacancy(d, key, charge=2 * (key[0] == 8))
    return d


def _case_nt(n, ny=4, nz=4, n_oxide=7, seed=22):
    return _set_points(_lattice(seed, ny, nz, n_oxide), n)


def _case_energy_edges():
    """Sixteen vacancies two lattice steps apart (5 A > nn_dist: every pair of them is a candidate) and two contact
    atoms get conduction-band edges that are exact multiples of tol or sit on q V0."""
    d = _lattice(23, 4, 4, 7)
    tol, E1 = d["par"]["tol"], Q_E * d["par"]["V0"]
    up, dn = np.inf, -np.inf
    cbs = [0.0, tol, 2 * tol, np.nextafter(2 * tol, up), 0.0, E1, np.nextafter(E1, up), np.nextafter(E1, dn), 2 * E1, 0.5 * E1,
           -tol, 4 * tol, E1 + tol, -E1, 8 * tol, tol]
    L = d["layers"]
    keys = [(l, iy, iz) for l in (L, L + 2, L + 4, L + 6) for iy in (0, 2) for iz in (0, 2)]
    keep = [_vacancy(d, k, charge=2 * (n % 2), cb=c) for n, (k, c) in enumerate(zip(keys, cbs))]
    # contact-to-trap on the same edges: two Ti atoms of the layer next to the oxide (atom index > (layers - 1) n1)
    for key, c in (((L - 1, 1, 1), 0.0), ((L - 1, 3, 3), tol)):
        d["cb"][d["lat"][key]] = c
        keep.append(d["lat"][key])
    return _set_points(d, 70, keep)                                        # (two mask words, as it happens)


def _case_distance_edges():
    """nn_dist = 5 A: two lattice steps are EXACTLY nn_dist, and so is the offset (0, 4, 3) of an extra vacancy from the
    lattice vacancy at y = z = 0 of its layer; two more extras sit at (0, 4 -+ 2^-50, 3), where the distance as the
    kernels form it (9 + (16 -+ 2^-47), no rounding in any step; sqrt: 5 -+ 0.8 ulp) is the neighbour of 5.0 in
    float64 on either side."""
    e = 2.0 ** -50
    L = 3
    d = _lattice(24, 4, 4, 7, extras={L + 1: [(0.0, 4.0, 3.0)], L + 3: [(0.0, 4.0 + e, 3.0)], L + 5: [(0.0, 4.0 - e, 3.0)]})
    d["par"]["nn_dist"] = 5.0
    keep = []
    for l, s in zip((L + 1, L + 3, L + 5), d["extra_site"]):
        p = _vacancy(d, (l, 0, 0), charge=0)
        d["charge"][s] = 2
        d["cb"][s] = d["cb"][p] + 0.1 * Q_E                                # (same layer: the smooth edge alone would not pass tol)
        keep.append(p)
    return _set_points(d, 66, keep)


def _case_window_edges():
    d = _lattice(25, 4, 4, 7)
    a, L, nl = A_LAT, 3, 13
    lat, x = d["lat"], d["xyz"][:, 0]
    d["x_lo"], d["x_hi"] = 1 * a, (nl - 1) * a                             # ON the second and on the last layer of atoms
    x[lat[(1, 2, 1)]] = np.nextafter(1 * a, np.inf)                        # one ulp inside
    x[lat[(nl - 1, 1, 2)]] = np.nextafter((nl - 1) * a, -np.inf)
    # (atoms (layers - 1) n1 and N_atom - (layers - 1) n1 -- the first atoms of layers 2 and 11 -- lie inside the window:
    # tunnel points that are not "metal_p"; their index neighbours 33 and N_atom - 33 are)
    s0, sl = lat[(0, 0, 0)], lat[(nl - 1, 3, 3)]
    d["element"][s0] = d["element"][sl] = VACANCY                         # atom 0 and the ground atom: never tunnel points
    d["element"][lat[(nl - 1, 3, 2)]] = VACANCY                           # the ground atom's neighbour: a point, +high_G on its diagonal
    d["charge"][lat[(nl - 1, 3, 2)]] = 2
    keep = [_vacancy(d, (L + 2, 1, 1), 0), _vacancy(d, (L + 2, 1, 2), 2), _vacancy(d, (L + 2, 2, 1), 0),    # neutral next to charged
            _vacancy(d, (L + 3, 1, 1), 0)]                                                                   # and next to neutral
    return _set_points(d, 100, keep)


CASES = ("nt_0", "nt_1", "nt_2", "nt_63", "nt_64", "nt_65", "nt_128", "nt_129", "energy_edges", "distance_edges", "window_edges",
         "group_178")

# What each case exists for: asserted against TRef.edges() by tests/test_tpath_ref.py (a case that lost its edge fails
# there).  Keys not listed are not constrained.
BUILT_FOR = {
    "nt_0": dict(n_t=0, nnz_tunnel=0),
    "nt_1": dict(n_t=1, nnz_tunnel=1),
    "nt_2": dict(n_t=2, nnz_tunnel=4),
    "nt_63": dict(n_t=63, block_rows=1, remainder=63),
    "nt_64": dict(n_t=64, block_rows=1, remainder=0),
    "nt_65": dict(n_t=65, block_rows=2, remainder=1),
    "nt_128": dict(n_t=128, block_rows=2, remainder=0),
    "nt_129": dict(n_t=129, block_rows=3, remainder=1),
    "energy_edges": dict(n_t=70, dE_at_tol=15, dE_just_above_tol=3, dE_zero=164, E2_zero=10, E2_zero_c2t=3, E2_neg_ulp=4, E2_pos_ulp=4,
                         E2_neg=552, E2_pos=1474),
    "distance_edges": dict(n_t=66, d_at_nn=15, d_ulp_below_nn=1, d_ulp_above_nn=1, atoms_at_nn=384),
    "window_edges": dict(n_t=100, x_at_lo=15, x_ulp_above_lo=1, x_at_hi=13, x_ulp_below_hi=1, idx_lo_edge=(False, False),
                         idx_lo_next=(False, True), idx_hi_edge=(False, False), idx_hi_prev=(False, True), atom0_vacancy=True,
                         last_atom_vacancy=True, ground_neighbour_vacancies=1, vac_neighbours_charged_neutral=26,
                         vac_neighbours_neutral_neutral=18, points_without_pair=19),
    "group_178": dict(N_atom=648, n_t=178, block_rows=3, remainder=50),
}


@functools.lru_cache(maxsize=None)
def tpath_case(name):
    """dict(xyz, element, charge, cb, n1, layers, x_lo, x_hi, par, metals, knobs, built_for); arrays read-only."""
    if name in ("nt_0", "nt_1", "nt_2"):
        d = _case_nt_small(int(name[3:]))
    elif name in ("nt_63", "nt_64", "nt_65"):
        d = _case_nt(int(name[3:]))
    elif name in ("nt_128", "nt_129"):
        d = _case_nt(int(name[3:]), ny=4, nz=6, seed=26)
        d["knobs"] = {"KMCF_SUB_STRIP": "2"}                               # ragged strips: the test runs with and without
    elif name == "energy_edges":
        d = _case_energy_edges()
    elif name == "distance_edges":
        d = _case_distance_edges()
    elif name == "window_edges":
        d = _case_window_edges()
    elif name == "group_178":
        d = _set_points(_lattice(27, 6, 6, 12), 178)
        d["knobs"] = {"KMCF_SUB_STRIP": "2"}
    else:
        raise KeyError(name)
    d = {k: v for k, v in d.items() if k not in ("lat", "extra_site", "seed", "ny", "nz", "n_oxide")}
    d.update(name=name, metals=METALS.copy(), built_for=BUILT_FOR[name])
    _ro(d["xyz"], d["element"], d["charge"], d["cb"], d["metals"])
    return d


@functools.lru_cache(maxsize=None)
def case_ref(name, Vd=None):
    """The reference system of a case (built once per process; treat as read-only), optionally at another bias."""
    return ref_of(tpath_case(name), Vd=Vd)


def ref_of(case, Vd=None, charge=None, cb=None):
    par = dict(case["par"])
    if Vd is not None:
        par["Vd"] = Vd
    return TRef(case["xyz"], case["element"], case["charge"] if charge is None else charge, case["cb"] if cb is None else cb,
                case["metals"], case["n1"], case["layers"], case["x_lo"], case["x_hi"], par)


def other_state(case):
    """(charge, cb) that differ from the case's: what a FIRST assembly runs on, so that the compared second one finds
    grown buffers, another pattern in the masks and other values behind it."""
    rng = np.random.default_rng(99)
    charge = np.where(case["element"] == VACANCY, 2 - case["charge"], 0).astype(np.int32)
    cb = case["cb"][::-1] * 0.5 + Q_E * 0.05 * rng.standard_normal(len(case["cb"]))
    return charge, cb


def potentials(ref, Vd, seed=1):
    """A prescribed potential vector over the Nsub nodes (volts): a smooth profile plus noise, as in tests/test_gpu_tpath.py."""
    rng = np.random.default_rng(seed)
    return Vd * (0.5 + 0.5 * np.cos(np.arange(ref.Nsub) * 0.05)) + 1e-3 * rng.standard_normal(ref.Nsub)
