"""The restatement kmcf_pair_correlation and kmcf_defect_correlation (csrc/kmcf_paircorr.hip) are held to: the contract of
include/kmcfield.h in plain numpy, and the inputs the tests run it on.  No GPU.

ALL pairs, in blocks of rows; the distance written out operation by operation (site_gap_pbc_ref.d2_exact: the open
difference, or the minimum image through pbc_ref.c_round); the table edge2 from the contract's own expression; the bin
from np.searchsorted(edge2, d2, side="right") - 1, capped at n_bins - 1; buckets and class pairs as defined; the counts
from the full symmetric matrix.  No cell list, no sqrt, nothing shared with the kernel.

tests/test_pair_corr_ref.py asserts what every input is built for; tests/test_gpu_pair_corr.py holds the library to this
file with np.array_equal on every output."""
import functools

import numpy as np

import pbc_ref as P
import site_gap_pbc_ref as GP
import site_gap_ref as GR

BLOCK = 256                                # rows per block of the all-pairs distance
MAX_CLASSES, MAX_BINS = 4, 256
STAT_KEYS = ("n_pairs_total", "n_members", "n_probes", "max_count", "max_count_site")


def table(r_max, n_bins):
    """(e, edge2): e[k] = r_max * k / n_bins (multiply, then divide), edge2[k] = e[k] * e[k], edge2[n_bins] = r_max * r_max"""
    r_max = np.float64(r_max)
    k = np.arange(n_bins + 1, dtype=np.float64)
    e = (r_max * k) / np.float64(n_bins)
    edge2 = e * e
    edge2[n_bins] = r_max * r_max
    return e, edge2


def bin_of(edge2, d2):
    """the largest k < n_bins with edge2[k] <= d2"""
    n_bins = len(edge2) - 1
    return np.minimum(np.searchsorted(edge2, d2, side="right") - 1, n_bins - 1)


def pair_index(p, q, n_classes):
    p, q = np.minimum(p, q), np.maximum(p, q)
    return p * n_classes - p * (p - 1) // 2 + (q - p)


def n_pairs(n_classes):
    return n_classes * (n_classes + 1) // 2


def pairs_within(xyz, cls, n_classes, r_max, L=None):
    """(i, j, d2) of every pair i < j of members with d2 <= r_max * r_max"""
    xyz = np.asarray(xyz, np.float64)
    cls = np.asarray(cls).astype(np.int64)
    mem = np.flatnonzero((cls >= 0) & (cls < n_classes))
    r2 = np.float64(r_max) * np.float64(r_max)
    I, J, D = [], [], []
    for s in range(0, len(mem), BLOCK):
        a = mem[s:s + BLOCK]
        d2 = GP.d2_exact(xyz, a[:, None], mem[None, :], L)
        ok = (d2 <= r2) & (a[:, None] < mem[None, :])
        ia, ib = np.nonzero(ok)
        I.append(a[ia]); J.append(mem[ib]); D.append(d2[ia, ib])
    cat = lambda l, t: np.concatenate(l) if l else np.zeros(0, t)
    return cat(I, np.int64), cat(J, np.int64), cat(D, np.float64)


def pair_correlation(xyz, cls, n_classes, r_max, n_bins, r_count=None, cell=None, n_cells=1, L=None):
    """dict(hist uint64 (n_cells + 1, n_pairs, n_bins), members int32 (n_cells + 1, n_classes), edge2, edges, counts int32
    (N, n_classes), stats: the integers of kmcf_pair_stats_t); L = (Lx, Ly, Lz): the minimum image, None: open"""
    xyz = np.asarray(xyz, np.float64)
    N = len(xyz)
    cls = np.asarray(cls).astype(np.int64)
    r_count = r_max if r_count is None else r_count
    cell = GR.cells_of(cell, n_cells, N)
    member = (cls >= 0) & (cls < n_classes)
    centre = member | (cls == n_classes)
    e, edge2 = table(r_max, n_bins)
    npair = n_pairs(n_classes)
    hist = np.zeros((n_cells + 1, npair, n_bins), np.uint64)
    i, j, d2 = pairs_within(xyz, cls, n_classes, r_max, L)
    ok = (cell[i] >= 0) & (cell[j] >= 0)
    i, j, d2 = i[ok], j[ok], d2[ok]
    bucket = np.where(cell[i] == cell[j], cell[i], n_cells)
    np.add.at(hist, (bucket, pair_index(cls[i], cls[j], n_classes), bin_of(edge2, d2)), np.uint64(1))
    members = np.zeros((n_cells + 1, n_classes), np.int32)
    mi = np.flatnonzero(member)
    np.add.at(members, (np.where(cell[mi] >= 0, cell[mi], n_cells), cls[mi]), 1)
    # the counts: the full symmetric matrix, a row per centre
    counts = np.zeros((N, n_classes), np.int32)
    rc2 = np.float64(r_count) * np.float64(r_count)
    cen = np.flatnonzero(centre)
    for s in range(0, len(cen), BLOCK):
        a = cen[s:s + BLOCK]
        d = GP.d2_exact(xyz, a[:, None], mi[None, :], L)
        near = (d <= rc2) & (a[:, None] != mi[None, :])
        for q in range(n_classes):
            counts[a, q] = (near & (cls[mi] == q)[None, :]).sum(1)
    tot = counts.sum(1)
    if len(cen):
        best = int(tot[cen].max())
        site = int(cen[tot[cen] == best].min())
    else:
        best, site = 0, -1
    stats = dict(n_pairs_total=int(hist.sum()), n_members=int(member.sum()), n_probes=int((centre & ~member).sum()), max_count=best,
                 max_count_site=site)
    return dict(hist=hist, members=members, edge2=edge2, edges=e, counts=counts, stats=stats)


def defect_classes(element, charge, probe_all):
    """the class rule of kmcf_defect_correlation: 0 neutral vacancy, 1 charged vacancy, 2 oxygen ion; others probe (3) or none (-1)"""
    element, charge = np.asarray(element), np.asarray(charge)
    cls = np.full(len(element), 3 if probe_all else -1, np.int32)
    cls[(element == P.VACANCY) & (charge == 0)] = 0
    cls[(element == P.VACANCY) & (charge != 0)] = 1
    cls[element == P.OXYGEN_DEFECT] = 2
    return cls


def pair_rdf(result, volume):
    """the contract of solvers.pair_rdf, written out once more: hist / (n_pq * shell_k / volume), buckets < n_cells"""
    hist, members, e = result["hist"], result["members"], result["edges"]
    n_cells, n_classes = hist.shape[0] - 1, members.shape[1]
    out = np.full((n_cells,) + hist.shape[1:], np.nan)
    for c in range(n_cells):
        for p in range(n_classes):
            for q in range(p, n_classes):
                Np, Nq = float(members[c, p]), float(members[c, q])
                n_pq = Np * Nq if p != q else Np * (Np - 1.0) / 2.0
                if n_pq == 0:
                    continue
                for k in range(hist.shape[2]):
                    shell = 4.0 / 3.0 * np.pi * (e[k + 1] ** 3 - e[k] ** 3)
                    out[c, int(pair_index(p, q, n_classes)), k] = float(hist[c, int(pair_index(p, q, n_classes)), k]) / (n_pq * shell / volume)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, cls, n_classes, cell (or None), n_cells, r_max, n_bins, r_count, cutoff = radius of the index, L)

SETTINGS = ((20.0, 20, 8.0), (20.0, 256, 20.0), (12.0, 7, 5.0))
RANDOM = tuple(P.RANDOM_CASES)             # p11, p23, p34, p52
EDGE_SETTINGS = ((7, 12.0), (20, 20.0), (256, 20.0), (13, 9.5))
SQRT_SPELLINGS = {"sqrt(d2) * (n / r)": lambda d2, n, r: np.sqrt(d2) * (np.float64(n) / np.float64(r)),
                  "sqrt(d2) / r * n": lambda d2, n, r: np.sqrt(d2) / np.float64(r) * np.float64(n),
                  "sqrt(d2) / (r / n)": lambda d2, n, r: np.sqrt(d2) / (np.float64(r) / np.float64(n))}


def _case(name, xyz, cls, n_classes, cell, n_cells, r_max, n_bins, r_count, L, cutoff=P.CUTOFF):
    xyz, cls = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(cls, np.int32)
    cell = None if cell is None else np.ascontiguousarray(cell, np.int32)
    for a in (xyz, cls) + (() if cell is None else (cell,)):
        a.flags.writeable = False
    return dict(name=name, xyz=xyz, cls=cls, n_classes=n_classes, cell=cell, n_cells=n_cells, r_max=float(r_max), n_bins=int(n_bins),
                r_count=float(r_count), L=np.array(L, np.float64), cutoff=float(cutoff))


def _random(base, k):
    """the sites of pbc_ref.pairwise_case(base): about 25 % each of three classes, 15 % probes, 10 % none; random cells in
    [-1, n_cells] (both ends: no valid cell)"""
    p = P.pairwise_case(base)
    N = p["N"]
    rng = np.random.default_rng(4100 + k)
    cls = rng.choice([0, 1, 2, 3, -1], N, p=[.25, .25, .25, .15, .10])
    n_cells = 3
    cell = rng.integers(-1, n_cells + 1, N)
    r_max, n_bins, r_count = SETTINGS[k]
    return _case("%s#%d" % (base, k), p["xyz"], cls, 3, cell, n_cells, r_max, n_bins, r_count, p["L"])


def _lattice_wrap():
    """3072 sites on a 4 A lattice, every site a member (class by the parity of the lattice indices' sum), one cell"""
    p = P.pairwise_case("lattice_wrap")
    g = np.rint(p["xyz"] / 4.0).astype(np.int64)
    return _case("lattice_wrap", p["xyz"], g.sum(1) % 2, 2, None, 1, 20.0, 20, 12.0, p["L"])


def _edge_probe_case(n_bins, r_max):
    """pairs along x: per row a member of class 0 at x = 0 and its partner of class 1 at dx = e[k] stepped by -4 .. +4 ulps
    (steps beyond r_max left out); the rows 40 A apart on a square grid in (y, z), so that a site's only partner within
    r_max is its own.  Every edge k = 1 .. n_bins; with 256 bins every second edge and the last one (3072 sites at most)."""
    e, _ = table(r_max, n_bins)
    ks = list(range(1, n_bins + 1))
    if len(ks) * 18 > 3072:
        ks = sorted(set(range(1, n_bins + 1, 2)) | {n_bins})
    dxs = []
    for k in ks:
        for u in range(-4, 5):
            dx = e[k]
            for _ in range(abs(u)):
                dx = np.nextafter(dx, np.inf if u > 0 else 0.0)
            if dx <= r_max:
                dxs.append(dx)
    rows = len(dxs)
    side = int(np.ceil(np.sqrt(rows)))
    r = np.arange(rows)
    y, z = 40.0 * (r // side), 40.0 * (r % side)
    xyz = np.zeros((2 * rows, 3))
    xyz[0::2, 1] = xyz[1::2, 1] = y
    xyz[0::2, 2] = xyz[1::2, 2] = z
    xyz[1::2, 0] = dxs
    cls = np.tile([0, 1], rows)
    assert len(xyz) <= 3072
    return _case("edge_probe@%d,%g" % (n_bins, r_max), xyz, cls, 2, None, 1, r_max, n_bins, r_max, (r_max + 8.0, 40.0 * side, 40.0 * side))


def _tile_edge(n):
    """n sites on a 4 A lattice of 16 x 16 sites per x plane, classes by site parity, two cells by the x plane's parity"""
    idx = np.arange(n)
    g = np.stack([idx // 256, (idx // 16) % 16, idx % 16], -1)
    return _case("tile_edge@%d" % n, g * 4.0, idx % 2, 2, (idx // 256) % 2, 2, 12.0, 7, 5.0, (4.0 * (g[:, 0].max() + 1), 64.0, 64.0))


def _centres(n):
    """2049 sites on the lattice of tile_edge, n of them centres (the first n // 2 + 1 members, the others probes): the 16
    centres per pass of a block of the walk and the 64 per block"""
    c = _tile_edge(2049)
    cls = np.full(2049, -1, np.int32)
    pick = np.linspace(0, 2048, n).astype(np.int64)
    cls[pick] = np.where(np.arange(n) <= n // 2, 0, 1)         # n_classes = 1: class 1 is the probe
    return _case("centres@%d" % n, c["xyz"], cls, 1, None, 1, 12.0, 7, 12.0, c["L"])


def _small(name):
    L = (16.0, 64.0, 64.0)
    pin = [(0.0, 0.0, 0.0), (8.0, 63.75, 63.75)]              # two sites of no class pin the index
    if name == "empty":
        xyz, cls, ncl = pin + [(4.0, 4.0, 4.0), (5.0, 4.0, 4.0)], [-1, -1, 7, -1], 3
    elif name == "single":
        xyz, cls, ncl = pin + [(4.0, 4.0, 4.0), (5.0, 4.0, 4.0), (4.0, 63.0, 4.0), (4.0, 40.0, 40.0)], [-1, -1, 0, 2, 2, 2], 2
    elif name == "dup":
        xyz, cls, ncl = pin + [(4.0, 4.0, 4.0), (4.0, 4.0, 4.0), (6.0, 4.0, 4.0)], [-1, -1, 1, 0, 2], 2
    else:
        ncl = 1 if name == "one_class" else 4
        rng = np.random.default_rng(5 + ncl)
        n = 300
        xyz = pin + [tuple(v) for v in rng.random((n, 3)) * np.array([12.0, 30.0, 30.0])]
        cls = [-1, -1] + list(rng.integers(0, ncl + 1, n))
    cell = None if name != "four_classes" else np.arange(len(cls)) % 3 - 1
    return _case(name, np.array(xyz, np.float64), cls, ncl, cell, 1 if cell is None else 2, 10.0, 5, 6.0, L, cutoff=16.0)


CENTRES = (15, 16, 17, 63, 64, 65)
SMALL = ("empty", "single", "dup", "one_class", "four_classes")
CASES = (tuple("%s#%d" % (b, k) for b in RANDOM for k in range(len(SETTINGS))) + ("lattice_wrap",)
         + tuple("edge_probe@%d,%g" % s for s in EDGE_SETTINGS) + tuple("tile_edge@%d" % n for n in (2047, 2048, 2049))
         + tuple("centres@%d" % n for n in CENTRES) + SMALL)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in SMALL:
        return _small(name)
    if name == "lattice_wrap":
        return _lattice_wrap()
    if name.startswith("edge_probe@"):
        n, r = name.split("@")[1].split(",")
        return _edge_probe_case(int(n), float(r))
    if name.startswith("tile_edge@"):
        return _tile_edge(int(name.split("@")[1]))
    if name.startswith("centres@"):
        return _centres(int(name.split("@")[1]))
    base, k = name.split("#")
    return _random(base, int(k))


def _freeze(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def reference(name, periodic=True):
    """pair_correlation() of an input, computed once per process and never modified"""
    c = case(name)
    return _freeze(pair_correlation(c["xyz"], c["cls"], c["n_classes"], c["r_max"], c["n_bins"], c["r_count"], c["cell"], c["n_cells"],
                                    c["L"] if periodic else None))


# ---- defects: the stubs() box of site_gap_pbc_ref with some vacancies charged and a few oxygen ions ----------------------------
DEFECT_SETTING = (10.0, 16, 6.0)


@functools.lru_cache(maxsize=None)
def defects():
    s = GP.stubs()
    element, charge = s["element"].copy(), s["charge"].copy()
    charge[s["left"][::2]] = 2                                  # every second vacancy of the left stump charged
    rng = np.random.default_rng(77)
    oxy = np.flatnonzero(element == P.O_EL)
    ions = rng.choice(oxy, 12, replace=False)
    element[ions] = P.OXYGEN_DEFECT
    charge[ions] = -2
    cell = (s["xyz"][:, 0] > 0.5 * (s["xyz"][:, 0].min() + s["xyz"][:, 0].max())).astype(np.int32)
    for a in (element, charge, cell):
        a.flags.writeable = False
    return dict(s, element=element, charge=charge, cell=cell, n_cells=2)


@functools.lru_cache(maxsize=None)
def defects_reference(probe_all, periodic=True):
    d = defects()
    r_max, n_bins, r_count = DEFECT_SETTING
    cls = defect_classes(d["element"], d["charge"], probe_all)
    return _freeze(dict(pair_correlation(d["xyz"], cls, 3, r_max, n_bins, r_count, d["cell"], d["n_cells"], d["L"] if periodic else None),
                        cls=cls))
