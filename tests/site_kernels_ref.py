"""Plain references for the kernels that feed the solver every KMC step, and the synthetic inputs they are tested on:
the pairwise ("gridless") Poisson term (csrc/kmcf_pairwise.hip), the charge rule, the K / CB-edge value assembly and
the global heat update (csrc/kmcf_kstate.hip).  numpy / scipy only, no GPU.

Each reference restates ONE operation as directly as possible -- direct distances instead of a cell list, a loop over
rows instead of lanes, integer counts instead of value sums, math.fsum instead of a tree -- so that it shares no
structure with the kernel it judges.  tests/test_site_kernels_ref.py pins the references to the CPU oracle on the 5 nm
device and asserts the conditions every input below is built for; tests/test_gpu_site_kernels.py holds the library to
them.  Inputs are built once per process (lru_cache) and handed out read-only."""
import functools
import math
import zlib

import numpy as np
from scipy.spatial import cKDTree
from scipy.special import erfc

Q_E = 1.60217663e-19                    # gpu_solvers.h:323
OXYGEN_DEFECT, VACANCY = 1, 2           # src/utils.h:37-44
OXIDE_TYPES = (3, 4)                    # any type that is neither a defect, a vacancy nor in the metal list
SCAN_TILE = 2048                        # flags per block of the compaction scan (KMCF_SCAN_TILE, csrc/kmcf_block.hpp)
CUTOFF = 20.0
SENTINEL = 123.0


def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


# ------------------------------------------------------------------------------------------------ pairwise term
def site_charged_pairs(xyz, charge, reach):
    """(i, j, dist) of every pair (site i, charged site j != i) with dist <= reach: candidates from a k-d tree, the
    distance itself recomputed from the coordinates as sqrt(dx^2 + dy^2 + dz^2)."""
    xyz = np.asarray(xyz, np.float64)
    charged = np.flatnonzero(np.asarray(charge) != 0)
    if len(charged) == 0:
        z = np.zeros(0, np.int64)
        return z, z, np.zeros(0)
    D = cKDTree(xyz).sparse_distance_matrix(cKDTree(xyz[charged]), reach * (1 + 1e-9), output_type="coo_matrix")
    i, j = D.row.astype(np.int64), charged[D.col]
    keep = i != j
    i, j = i[keep], j[keep]
    d = xyz[j] - xyz[i]
    dist = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    keep = dist <= reach
    return i[keep], j[keep], dist[keep]


def pairwise_ref(xyz, charge, sigma, k, cutoff):
    """(want, S, n) per site: want_i = sum over charged j != i with dist < cutoff of q_j erfc(r / (sigma sqrt 2)) k q / r,
    r = 1e-10 dist; S_i the same sum over absolute values (float64); n_i the number of terms.
    Each term is the float64 expression as written, with scipy's erfc; the terms of a site are ACCUMULATED in
    np.longdouble, so that no order of addition is built into the reference.  (What float64 leaves in a term is the
    rounding of erfc's argument, which weighs 2 x^2 times in erfc for large x -- 33 times at 20 A, x = 4 -- on terms
    that are 1e-8 of a nearest-neighbour term.)"""
    N = len(xyz)
    charge = np.asarray(charge)
    i, j, dist = site_charged_pairs(xyz, charge, cutoff)
    m = dist < cutoff
    i, j, dist = i[m], j[m], dist[m]
    r = 1e-10 * dist
    term = charge[j].astype(np.float64) * erfc(r / (sigma * np.sqrt(2.0))) * k * Q_E / r
    order = np.argsort(i, kind="stable")
    i, term = i[order], term[order]
    n = np.bincount(i, minlength=N).astype(np.int64)
    want = np.zeros(N, np.longdouble)
    S = np.zeros(N)
    if len(i):
        first = np.flatnonzero(np.r_[True, i[1:] != i[:-1]])
        want[i[first]] = np.add.reduceat(term.astype(np.longdouble), first)
        S[i[first]] = np.add.reduceat(np.abs(term), first)
    return want, S, n


def cutoff_margin(xyz, charge, cutoff=CUTOFF):
    """(smallest |dist / cutoff - 1| over the pairs (site, charged site) near the cutoff, number of pairs at exactly it)"""
    _, _, dist = site_charged_pairs(xyz, charge, cutoff * 1.001)
    rel = np.abs(dist / cutoff - 1.0)
    return (float(rel.min()) if len(rel) else np.inf), int((dist == cutoff).sum())


def cell_order(xyz, cutoff=CUTOFF):
    """(order, cells per axis): the sites sorted by cutoff-sized cell, cell id (cx ncy + cy) ncz + cz counted from the
    lowest coordinate, ascending site id inside a cell -- the order the compaction of csrc/kmcf_pairwise.hip scans in."""
    xyz = np.asarray(xyz, np.float64)
    c = np.floor((xyz - xyz.min(0)) * (1.0 / cutoff)).astype(np.int64)
    nc = np.floor((xyz.max(0) - xyz.min(0)) * (1.0 / cutoff)).astype(np.int64) + 1
    c = np.minimum(c, nc - 1)
    cid = (c[:, 0] * nc[1] + c[:, 1]) * nc[2] + c[:, 2]
    return np.argsort(cid, kind="stable"), tuple(int(v) for v in nc)


def _lattice(nx, ny, nz, a=4.0):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g.astype(np.float64) * a, g


TILE_EDGE_SIZES = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)       # a scan tile one item short, exactly full, one item over
TILE_EDGE = tuple("tile_edge@%d" % n for n in TILE_EDGE_SIZES)


@functools.lru_cache(maxsize=None)
def tile_edge_sites(N):
    """(xyz, order) of the cases at the edge of a scan tile, shared by the pairwise, gap and chain tests: N sites drawn from
    a 13 x 13 x 13 lattice of 4 A, jittered by 0.3 A, ids shuffled -- 3 x 3 x 3 cells of CUTOFF, a dozen sites or more in the
    last one.  order = cell_order(xyz)[0]: order[-1] is the site at the LAST position of the cell order, the item whose
    list position comes out of every count before it and whose run ends at the list's total.  Read-only."""
    rng = np.random.default_rng(4000 + N)
    g, _ = _lattice(13, 13, 13)
    xyz = g[rng.choice(len(g), N, replace=False)] + rng.uniform(-0.3, 0.3, (N, 3))
    order, nc = cell_order(xyz)
    assert nc == (3, 3, 3)
    return _ro(xyz, order)


PAIRWISE_CASES = ("thin", "thin_uncharged", "one_cell", "one_site", "seventeen", "cube", "lattice_cutoffs", "large",
                  "large_tail") + TILE_EDGE
ON_LATTICE = ("thin", "thin_uncharged", "lattice_cutoffs")
LARGE = ("large", "large_tail")


@functools.lru_cache(maxsize=None)
def pairwise_case(name):
    """dict(xyz, charge, slices [(displ, count), ...]) of one pairwise input, read-only."""
    if name in ("thin", "thin_uncharged"):          # 1029 x 2 x 2 at 4 A: thinner than one cutoff in y and z
        xyz, g = _lattice(1029, 2, 2)
        charge = np.where(g.sum(1) % 2 == 0, 2, -2).astype(np.int32)
        if name == "thin_uncharged":
            charge[:] = 0
        slices = [(0, len(xyz))]
    elif name == "one_cell":
        rng = np.random.default_rng(21)
        xyz = rng.random((300, 3)) * 15.0
        charge = np.zeros(300, np.int32)
        charge[rng.choice(300, 100, replace=False)] = rng.choice([-2, 2], 100)
        slices = [(0, 300)]
    elif name == "one_site":
        xyz, charge, slices = np.array([[1.5, -2.0, 7.25]]), np.array([2], np.int32), [(0, 1)]
    elif name == "seventeen":
        xyz = np.random.default_rng(22).random((17, 3)) * 12.0
        charge = np.zeros(17, np.int32)
        charge[16] = -2
        slices = [(0, 17)]
    elif name == "cube":
        rng = np.random.default_rng(23)
        N = 6000
        xyz = rng.random((N, 3)) * 70.0
        charge = np.zeros(N, np.int32)
        idx = rng.choice(N, 3 * N // 10, replace=False)
        charge[idx] = rng.choice([-2, 2], len(idx))
        slices = [(0, N), (0, 0), (N - 1, 1), (1237, 1001)]
    elif name == "lattice_cutoffs":
        rng = np.random.default_rng(24)
        xyz, _ = _lattice(16, 16, 16)
        N = len(xyz)
        charge = np.zeros(N, np.int32)
        idx = rng.choice(N, N // 5, replace=False)
        charge[idx] = rng.choice([-2, 2], len(idx))
        slices = [(0, N)]
    elif name in LARGE:                              # 83 x 81 x 80 jittered lattice: 263 scan tiles
        rng = np.random.default_rng(11)
        g, _ = _lattice(83, 81, 80)
        N = len(g)
        xyz = g + rng.uniform(-0.3, 0.3, g.shape)
        charge = np.zeros(N, np.int32)
        if name == "large":
            idx = rng.choice(N, N // 100, replace=False)
            charge[idx] = rng.choice([-2, 2], len(idx))
        else:                                        # charges on the last 3000 sites of the cell order only
            tail = cell_order(xyz)[0][-3000:]
            charge[tail] = np.where(np.arange(3000) % 3 == 0, -2, 2)
        slices = [(0, N)]
    elif name in TILE_EDGE:                          # one charged site: the one at the last position of the cell order
        xyz, order = tile_edge_sites(int(name.split("@")[1]))
        charge = np.zeros(len(xyz), np.int32)
        charge[order[-1]] = 2
        slices = [(0, len(xyz))]
    else:
        raise KeyError(name)
    _ro(xyz, charge)
    return dict(name=name, xyz=xyz, charge=charge, slices=slices, N=len(xyz))


@functools.lru_cache(maxsize=None)
def pairwise_reference(name, sigma, k):
    return _ro(*pairwise_ref(pairwise_case(name)["xyz"], pairwise_case(name)["charge"], sigma, k, CUTOFF))


# ------------------------------------------------------------------------------------------------ charge rule
def charge_ref(element, charge_in, neigh_rows, metals, displ):
    """update_charge on rows [displ, displ + len(neigh_rows)): row r lists the neighbours of site displ + r.  A vacancy is
    neutral if a listed neighbour is a metal or at least two are vacancies, else +2; an oxygen defect is neutral next to
    a metal, else -2; every other site keeps its charge.  Entries < 0 are skipped."""
    element = np.asarray(element)
    out = np.array(charge_in, np.int32, copy=True)
    metals = [int(m) for m in metals]
    neigh_rows = np.asarray(neigh_rows)
    for r in range(neigh_rows.shape[0]):
        i = displ + r
        e = int(element[i])
        if e != VACANCY and e != OXYGEN_DEFECT:
            continue
        listed = [int(element[j]) for j in neigh_rows[r] if j >= 0]
        metal = any(en in metals for en in listed)
        if e == VACANCY:
            out[i] = 0 if (metal or sum(en == VACANCY for en in listed) >= 2) else 2
        else:
            out[i] = 0 if metal else -2
    return out


# crafted rows: (centre element, {slot: neighbour kind}, every other slot, expected charge); kinds "M" the LAST entry of
# the metal list, "V" vacancy, "O" oxide, None -1.  Slots >= nn are dropped with the row (see charge_case).
def _crafted(nn):
    rows = [(VACANCY, {nn - 1: "M"}, "O", 0), (OXYGEN_DEFECT, {nn - 1: "M"}, "O", 0),       # the deciding metal in the last slot
            (VACANCY, {}, None, 2), (OXYGEN_DEFECT, {}, None, -2),                          # a row of all -1
            (VACANCY, {}, "O", 2), (OXYGEN_DEFECT, {}, "O", -2),
            (VACANCY, {min(3, nn - 1): "V"}, "O", 2), (OXYGEN_DEFECT, {min(3, nn - 1): "V"}, "O", -2),   # exactly one vacancy
            (VACANCY, {nn - 1: "M"}, None, 0), (VACANCY, {0: "V"}, None, 2)]
    if nn > 12:                                     # exactly two vacancies, held by lanes 3 and 12
        rows += [(VACANCY, {3: "V", 12: "V"}, "O", 0), (OXYGEN_DEFECT, {3: "V", 12: "V"}, "O", -2),
                 (VACANCY, {3: "V", 12: "V"}, None, 0)]
    if nn > 16:                                     # slot 16: lane 0's second pass
        rows += [(VACANCY, {16: "M"}, "O", 0), (OXYGEN_DEFECT, {16: "M"}, "O", 0), (VACANCY, {0: "V", 16: "V"}, "O", 0),
                 (VACANCY, {16: "V"}, "O", 2)]
    return rows


CHARGE_CASES = {   # name: (N, nn, row_count, displ, number of metal types, first crafted row)
    "nn1": (400, 1, 300, 0, 1, 0), "nn15": (400, 15, 300, 0, 2, 0), "nn16": (400, 16, 300, 0, 3, 0),
    "nn17": (400, 17, 300, 0, 1, 0), "nn52": (400, 52, 300, 0, 2, 0),
    "rows1_last_slot": (300, 52, 1, 0, 3, 0), "rows1_slot16": (300, 52, 1, 0, 3, 13), "rows16": (300, 52, 16, 0, 2, 0),
    "rows17": (300, 52, 17, 0, 1, 0), "displ123": (500, 52, 300, 123, 3, 0), "displ123_nn17": (500, 17, 17, 123, 2, 0),
    "stride": (40000, 17, 40000, 0, 2, 0),
}
METAL_LISTS = {1: (6,), 2: (6, 8), 3: (9, 6, 8)}


@functools.lru_cache(maxsize=None)
def charge_case(name):
    """dict(element, neigh (row_count x nn: the slice's rows only, indices anywhere in the device), metals, displ,
    row_count, nn, N, crafted [(site, expected charge), ...], want: charge_ref on input charges of 7), read-only."""
    N, nn, row_count, displ, n_metals, first = CHARGE_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    metals = METAL_LISTS[n_metals]
    kinds = np.array(list(metals) + [OXYGEN_DEFECT, VACANCY] + list(OXIDE_TYPES))
    weight = np.array([0.12 / n_metals] * n_metals + [0.25, 0.33] + [0.15, 0.15])
    element = rng.choice(kinds, N, p=weight / weight.sum()).astype(np.int32)
    # three sites of known type OUTSIDE the slice where there is room, else at its far end, for the crafted rows to name
    spare = [s for s in range(N) if not displ <= s < displ + row_count][-3:] if N - row_count >= 3 else [N - 3, N - 2, N - 1]
    site_of = {"M": spare[0], "V": spare[1], "O": spare[2]}
    element[spare[0]], element[spare[1]], element[spare[2]] = metals[-1], VACANCY, OXIDE_TYPES[0]
    # random rows: few listed neighbours (1 .. 4 of the nn slots), so that every outcome of the rule occurs often
    neigh = rng.integers(0, N, (row_count, nn)).astype(np.int32)
    keep = rng.random((row_count, nn)) < rng.integers(1, 5, (row_count, 1)) / nn
    neigh[~keep] = -1
    crafted = []
    rows = _crafted(nn)
    rows = rows[first:] + rows[:first]
    for r, (centre, slots, other, expect) in enumerate(rows):
        site = displ + r
        if r >= row_count or site in spare:
            break
        element[site] = centre
        neigh[r] = -1 if other is None else site_of[other]
        for s, kind in slots.items():
            neigh[r, s] = site_of[kind]
        crafted.append((site, expect))
    want = charge_ref(element, np.full(N, 7, np.int32), neigh, metals, displ)
    _ro(element, neigh, want)
    return dict(name=name, element=element, neigh=neigh, metals=np.array(metals, np.int32), displ=displ,
                row_count=row_count, nn=nn, N=N, crafted=crafted, want=want)


# ------------------------------------------------------------------------------------------------ K / CB values
def site_classes(element, charge, metals):
    """(metal, uncharged vacancy) per site"""
    element, charge = np.asarray(element), np.asarray(charge)
    return np.isin(element, np.asarray(metals)), (element == VACANCY) & (charge == 0)


def k_values_ref(row_ptr, col, left, right, element, charge, metals, high_G, low_G, Vd, N_left, n_interface, cb):
    """dict(val, diag, dinv, rhs, left, right) from the three patterns: (row_ptr, col) the interface block with
    block-local columns, left / right = (row_ptr, col) of the contact blocks.  Off-diagonals -high_G or -low_G by the
    class rule (K: both metal or both uncharged vacancy; CB: either metal); the diagonal from INTEGER counts,
    (count_high high_G + count_low low_G) over the interface, left and right entries, so that it is exact up to the
    final three roundings; rhs = left VL + right VR with VL = -Vd/2, VR = +Vd/2 (K) and the signs swapped (CB)."""
    metal, uvac = site_classes(element, charge, metals)
    n = n_interface

    def high(i, j):
        return (metal[i] | metal[j]) if cb else ((metal[i] & metal[j]) | (uvac[i] & uvac[j]))

    def counts(rp, cl, col0, skip_diag):
        rows = np.repeat(np.arange(n), np.diff(rp))
        cl = np.asarray(cl, np.int64)[:rp[-1]]
        h = high(N_left + rows, col0 + cl)
        live = (cl != rows) if skip_diag else np.ones(len(cl), bool)
        nh = np.bincount(rows[live & h], minlength=n)
        nl = np.bincount(rows[live & ~h], minlength=n)
        return rows, cl, h, nh, nl

    rows, cl, h, nh, nl = counts(np.asarray(row_ptr), col, N_left, True)
    _, _, _, lh, ll = counts(np.asarray(left[0]), left[1], 0, False)
    _, _, _, rh, rl = counts(np.asarray(right[0]), right[1], N_left + n, False)
    d = nh.astype(np.float64) * high_G + nl.astype(np.float64) * low_G
    l = lh.astype(np.float64) * high_G + ll.astype(np.float64) * low_G
    r = rh.astype(np.float64) * high_G + rl.astype(np.float64) * low_G
    tot = d + l + r
    val = np.where(h, -high_G, -low_G)
    on_diag = cl == rows
    val[on_diag] = tot[rows[on_diag]]
    VL, VR = (Vd / 2, -Vd / 2) if cb else (-Vd / 2, Vd / 2)
    return dict(val=val, diag=tot, dinv=1.0 / tot, rhs=l * VL + r * VR, left=l, right=r, off_diagonal=~on_diag)


def neighbor_rows(xyz, nn_dist, nn):
    """the first nn sites j != i with dist < nn_dist in ascending j, -1 padding (the library's neighbour list)"""
    xyz = np.asarray(xyz, np.float64)
    N = len(xyz)
    out = np.full((N, nn), -1, np.int32)
    for i, lst in enumerate(cKDTree(xyz).query_ball_point(xyz, nn_dist, return_sorted=True)):
        lst = [j for j in lst if j != i and np.linalg.norm(xyz[j] - xyz[i]) < nn_dist][:nn]
        out[i, :len(lst)] = lst
    return out


def box_pattern(xyz, L, pbc, cutoff, row0, n_rows, col0, n_cols):
    """(row_ptr, col) of rows [row0, row0 + n_rows) x columns [col0, col0 + n_cols), block-local ascending columns:
    dist < cutoff, minimum image in y and z under pbc (valid while cutoff < L / 2 and the sites lie in [0, L))."""
    xyz = np.asarray(xyz, np.float64)
    box = [1e6, L[1], L[2]] if pbc else None
    D = cKDTree(xyz[row0:row0 + n_rows], boxsize=box).sparse_distance_matrix(
        cKDTree(xyz[col0:col0 + n_cols], boxsize=box), cutoff, output_type="coo_matrix")
    # (explicit zeros -- the diagonal -- are entries of the COO result; pairs AT the cutoff do not occur off-lattice)
    order = np.lexsort((D.col, D.row))
    rows, cols = D.row[order], D.col[order]
    keep = D.data[order] < cutoff
    rows, cols = rows[keep], cols[keep]
    rp = np.zeros(n_rows + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n_rows), out=rp[1:])
    return rp, cols.astype(np.int32)


K_DEVICES = ("sparse", "dense")
K_BOX = np.array([60.0, 21.0, 21.0])
K_NN_DIST, K_CONTACT = 3.5, 60
K_PARAMS = dict(Vd=5.0, high_G=1.0, low_G=1e-8)           # the 5 nm device's conductances
K_CHARGE_NN_DIST, K_CHARGE_NN = 1.6, 20                   # the neighbour list the charges come from (see k_device)


@functools.lru_cache(maxsize=None)
def k_device(name):
    """A synthetic device for the value assembly: random sites in a 60 x 21 x 21 A box sorted by x, 60 contact sites
    per side.  "sparse": about 4000 sites, 27 entries per row; "dense": about 45 entries per row and, under pbc = 1,
    none above 64 (sites of longer rows are taken out again), so that a 64-row tile would hold more than the 2040
    entries a tile may have.
    Elements: 30 % metal (two types), 40 % vacancies, the rest oxide and oxygen defects, mixed along every row.  The
    charges follow from the charge rule on a SHORT neighbour list (1.6 A, 20 slots: 2.4 / 4 neighbours on average),
    under which a part of the vacancies stays charged -- with the 3.5 A list nearly every vacancy here has a metal
    neighbour and no charged vacancy would be left.  charge2 (the vacancies' charges flipped between 0 and +2) is a
    second, different state for the assembly that runs BEFORE the one that is compared."""
    rng = np.random.default_rng({"sparse": 31, "dense": 32}[name])
    N0 = {"sparse": 4000, "dense": 6500}[name]
    xyz = rng.random((N0, 3)) * K_BOX
    if name == "dense":
        while True:
            t = cKDTree(xyz, boxsize=[1e6, K_BOX[1], K_BOX[2]])
            length = np.array([len(v) for v in t.query_ball_point(xyz, K_NN_DIST)])
            if length.max() <= 64:
                break
            xyz = np.delete(xyz, np.flatnonzero(length > 64)[::2], axis=0)
    xyz = xyz[np.argsort(xyz[:, 0], kind="stable")]
    N = len(xyz)
    metals = (6, 8)
    kinds = np.array([6, 8, VACANCY, OXYGEN_DEFECT, 3, 4])
    element = rng.choice(kinds, N, p=[0.15, 0.15, 0.40, 0.10, 0.10, 0.10]).astype(np.int32)
    neigh = neighbor_rows(xyz, K_CHARGE_NN_DIST, K_CHARGE_NN)
    charge = charge_ref(element, np.zeros(N, np.int32), neigh, metals, 0)
    charge2 = charge.copy()
    vac = element == VACANCY
    charge2[vac] = 2 - charge[vac]
    _ro(xyz, element, neigh, charge, charge2)
    return dict(name=name, xyz=xyz, element=element, charge=charge, charge2=charge2, neigh=neigh, N=N, NL=K_CONTACT,
                n=N - 2 * K_CONTACT, metals=np.array(metals, np.int32), lattice=K_BOX, **K_PARAMS)


def k_patterns(dev, pbc):
    """the three patterns of a k_device by box_pattern: (interface, left, right), each (row_ptr, col)"""
    NL, n, xyz, L = dev["NL"], dev["n"], dev["xyz"], dev["lattice"]
    return (box_pattern(xyz, L, pbc, K_NN_DIST, NL, n, NL, n), box_pattern(xyz, L, pbc, K_NN_DIST, NL, n, 0, NL),
            box_pattern(xyz, L, pbc, K_NN_DIST, NL, n, NL + n, NL))


def k_pair_shares(dev, row_ptr, col, charge):
    """shares of the interface off-diagonals that join metal-metal, uncharged vacancy-uncharged vacancy, metal-uncharged
    vacancy, and a charged vacancy with anything"""
    NL, n = dev["NL"], dev["n"]
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    col = np.asarray(col)[:row_ptr[-1]]
    off = rows != col
    i, j = NL + rows[off], NL + col[off]
    metal, uvac = site_classes(dev["element"], charge, dev["metals"])
    cvac = (dev["element"] == VACANCY) & (np.asarray(charge) != 0)
    return dict(metal_metal=float((metal[i] & metal[j]).mean()), uvac_uvac=float((uvac[i] & uvac[j]).mean()),
                metal_uvac=float(((metal[i] & uvac[j]) | (uvac[i] & metal[j])).mean()),
                cvac_any=float((cvac[i] | cvac[j]).mean()))


def window_tiles(row_ptr, col, max_rows=64, max_entries=2040, max_cols=1024):
    """End row of every tile the window plan cuts from a CSR in the INTERNAL row order (kmcf_matrix_sum_plan): whole
    rows while the tile holds at most 64 rows, 2040 entries and 1024 distinct columns.  Returns (ends, closed_by) with
    closed_by in {"rows", "entries", "columns", "end"}.
    A restatement of plan_window (csrc/kmcf_spmv.hip) for a matrix that expects value codes: row_cap = 8 WIN_U,
    cap = 256 WIN_U - WIN_U, wmax = 256 WIN_WQ with WIN_U = 8, WIN_WQ = 4 -- change the defaults here with them.  The
    library reports these cuts nowhere (kmcf_matrix_row_order gives the row-per-lane tiles); the GPU test checks the
    number of tiles against the plan's under KMCF_SPMV_SELL=0."""
    n = len(row_ptr) - 1
    ends, why = [], []
    r = 0
    while r < n:
        e, seen = r, set()
        reason = "end"
        while e < n:
            if e - r >= max_rows:
                reason = "rows"
                break
            if row_ptr[e + 1] - row_ptr[r] > max_entries:
                reason = "entries"
                break
            new = seen | set(col[row_ptr[e]:row_ptr[e + 1]].tolist())
            if len(new) > max_cols:
                reason = "columns"
                break
            seen = new
            e += 1
        assert e > r, "a row alone exceeds a tile"
        ends.append(e)
        why.append(reason)
        r = e
    return np.array(ends), why


# ------------------------------------------------------------------------------------------------ global heat
HEAT_SIZES = (0, 1, 255, 257, 262144, 524291)
HEAT_ARGS = dict(a=0.999, b=0.3, steps=100.0, C=1e-15, small_step=1e-12)     # power term 0.01 .. 25 next to b = 0.3


def heat_global_ref(p, T, a, b, steps, C, small_step):
    """update_temp_global in closed form: c (1 - a^step) / (1 - a) + a^step T with c = b + P / C small_step, P the
    exactly rounded sum of the power (math.fsum) and step = int(steps)."""
    P = math.fsum(np.asarray(p, np.float64).tolist())
    step = int(steps)
    c = b + P / C * small_step
    return c * (1.0 - math.pow(a, float(step))) / (1.0 - a) + math.pow(a, float(step)) * T


def heat_bar(p, T, a, b, steps, C, small_step):
    """1e-13 on the terms before they cancel: the summation (first term) and the final addition (second)."""
    S = math.fsum(np.abs(np.asarray(p, np.float64)).tolist())
    g = abs((1.0 - a ** int(steps)) / (1.0 - a))
    return 1e-13 * (abs(b) + S * small_step / C) * g + 1e-13 * abs(a ** int(steps) * T)


@functools.lru_cache(maxsize=None)
def heat_power(N):
    """N power values of mixed sign, magnitudes 1e-15 .. 1e-6 (log-uniform), in pairs (m, -m (1 - 2e-3)) scattered over
    the vector (an odd N leaves the smallest without its partner): the sum cancels to about 1e-3 of the sum of the
    magnitudes."""
    rng = np.random.default_rng(40 + N % 97)
    m = np.sort(10.0 ** rng.uniform(-14.99, -6, (N + 1) // 2))[::-1]
    p = np.stack([m, -m * (1 - 2e-3)], 1).reshape(-1)[:N]
    return _ro(rng.permutation(p))
