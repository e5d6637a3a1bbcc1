"""The restatement kmcf_site_set_gap_pbc and kmcf_filament_gap_pbc (csrc/kmcf_gap.hip, the periodic gp_search_kernel) are held to:
the contract of include/kmcfield.h in plain numpy, and the inputs the tests run it on.  No GPU.

ALL pairs (a, b) of a gap cell, in blocks of A sites; the distance written out operation by operation --
    dx = x[a] - x[b];  fy = (y[a] - y[b]) / Ly;  fy = fy - round(fy);  dy = fy * Ly   (z likewise; pbc_ref.c_round)
    d2 = (dx*dx + dy*dy) + dz*dz
-- the test d2 <= r_max*r_max, and lexsort((b, a, d2)): smallest d2, then smallest a, then smallest b.  No cell list and
nothing shared with the kernel.  L = None is the open-boundary distance of kmcf_site_set_gap; the result then equals
site_gap_ref.site_set_gap (asserted in tests/test_site_gap_pbc_ref.py).

For the 5 nm cell (6 000 x 8 000 pairs) propose="tree" lets a k-d tree over the nine (y, z) shifted copies of B propose
the pairs within the nearest approach it finds (times 1 + 1e-9, plus 1e-9 A: far more than the tree's distance and the
contract's can differ); the exact arithmetic above decides among them.  The minimum image is never farther than any
other image, so a pair at the exact minimum is among the proposals.

tests/test_site_gap_pbc_ref.py asserts what every input is built for; tests/test_gpu_site_gap_pbc.py holds the library to
this file, array_equal on every field (gap: within 1 ulp of sqrt(gap2))."""
import functools

import numpy as np

import pbc_ref as P
import site_gap_ref as GR

BLOCK = 512                                # A sites per block of the all-pairs distance


def fold(va, vb, period):
    """(minimum-image difference va - vb, the number of periods taken out) along one periodic axis"""
    f = (va - vb) / period
    n = P.c_round(f)
    f = f - n
    return f * period, n


def d2_exact(xyz, a, b, L=None):
    """the contract's d2 of the pairs (a, b) (broadcast); L None: open boundaries"""
    dx = xyz[a, 0] - xyz[b, 0]
    if L is None:
        dy, dz = xyz[a, 1] - xyz[b, 1], xyz[a, 2] - xyz[b, 2]
    else:
        dy, dz = fold(xyz[a, 1], xyz[b, 1], L[1])[0], fold(xyz[a, 2], xyz[b, 2], L[2])[0]
    return (dx * dx + dy * dy) + dz * dz


def crossings(xyz, a, b, L):
    """(ny, nz): periods taken out of y[a] - y[b] and z[a] - z[b]; non-zero: the pair is nearest across that face"""
    return int(fold(xyz[a, 1], xyz[b, 1], L[1])[1]), int(fold(xyz[a, 2], xyz[b, 2], L[2])[1])


def _proposals(xyz, A, B, r_max, L):
    """(a, b) candidate pairs from a k-d tree over shifted copies of B, without duplicates; None: no B within reach"""
    from scipy.spatial import cKDTree
    shifts = [(sy, sz) for sy in (-1, 0, 1) for sz in (-1, 0, 1)] if L is not None else [(0, 0)]
    pts = np.concatenate([xyz[B] + np.array([0.0, sy * L[1], sz * L[2]]) for sy, sz in shifts]) if L is not None else xyz[B]
    ids = np.tile(B, len(shifts))
    tree = cKDTree(pts)
    R = r_max * (1 + 1e-9) + 1e-9
    d, _ = tree.query(xyz[A], k=1, distance_upper_bound=R)
    if not np.isfinite(d.min()):
        return None
    rad = min(R, d.min() * (1 + 1e-9) + 1e-9)
    near = A[d <= rad]
    lists = tree.query_ball_point(xyz[near], rad)
    a = np.repeat(near, [len(l) for l in lists])
    b = ids[np.concatenate([np.asarray(l, np.int64) for l in lists])]
    pairs = np.unique(np.stack([a, b], axis=1), axis=0)
    return pairs[:, 0], pairs[:, 1]


def nearest_pair(xyz, A, B, r_max, L=None, propose="all"):
    """(a, b, d2) of the contract for the site lists A, B of one gap cell, or None"""
    if len(A) == 0 or len(B) == 0:
        return None
    r2 = r_max * r_max
    if propose == "tree":
        got = _proposals(xyz, A, B, r_max, L)
        if got is None:
            return None
        a, b = got
        d2 = d2_exact(xyz, a, b, L)
        ok = d2 <= r2
        if not ok.any():
            return None
        a, b, d2 = a[ok], b[ok], d2[ok]
        k = np.lexsort((b, a, d2))[0]
        return int(a[k]), int(b[k]), float(d2[k])
    best = None
    for s in range(0, len(A), BLOCK):
        a = np.broadcast_to(A[s:s + BLOCK, None], (len(A[s:s + BLOCK]), len(B))).ravel()
        b = np.broadcast_to(B[None, :], (len(A[s:s + BLOCK]), len(B))).ravel()
        d2 = d2_exact(xyz, a, b, L)
        ok = np.flatnonzero(d2 <= r2)
        if len(ok) == 0:
            continue
        k = ok[np.lexsort((b[ok], a[ok], d2[ok]))[0]]
        got = (float(d2[k]), int(a[k]), int(b[k]))
        if best is None or got < best:
            best = got
    return None if best is None else (best[1], best[2], best[0])


def site_set_gap(xyz, side, r_max, cell=None, n_cells=1, L=None, propose="all"):
    """(gaps, stats): GAP_DTYPE records of the n_cells gap cells and the integer fields of kmcf_gap_stats_t, the pair
    distance the minimum image under L = (Lx, Ly, Lz) (L None: open boundaries)"""
    xyz = np.asarray(xyz, np.float64)
    r_max = float(r_max)
    N = len(xyz)
    side = np.asarray(side).astype(np.int64) & 3
    cell = GR.cells_of(cell, n_cells, N)
    gaps = np.zeros(n_cells, GR.GAP_DTYPE)
    gaps["gap"] = gaps["gap2"] = np.inf
    gaps["site_left"] = gaps["site_right"] = -1
    left, right = (side & 1) != 0, (side & 2) != 0
    for c in range(n_cells):
        here = cell == c
        A, B = np.flatnonzero(here & left), np.flatnonzero(here & right)
        gaps[c]["n_left"], gaps[c]["n_right"], gaps[c]["n_both"] = len(A), len(B), int((here & left & right).sum())
        gaps[c]["bridged"] = gaps[c]["n_both"] > 0
        got = nearest_pair(xyz, A, B, r_max, L, propose)
        if got is not None:
            a, b, d2 = got
            gaps[c]["gap2"], gaps[c]["gap"] = d2, np.sqrt(d2)
            gaps[c]["site_left"], gaps[c]["site_right"] = a, b
            gaps[c]["x_left"], gaps[c]["x_right"] = xyz[a, 0], xyz[b, 0]
    found = gaps["site_left"] >= 0
    stats = dict(n_left=int(left.sum()), n_right=int(right.sum()), n_both=int((left & right).sum()),
                 cells_bridged=int((gaps["bridged"] != 0).sum()), cells_open=int(((gaps["bridged"] == 0) & found).sum()),
                 cells_none=int(((gaps["bridged"] == 0) & ~found).sum()))
    return gaps, stats


def filament_gap(neigh, element, charge, metals, xyz, NL, NR, r_max, cell=None, n_cells=1, bins=None, L=None, propose="all"):
    """dict(gaps, stats, side, profile) of kmcf_filament_gap_pbc: the sides from the list as given (site_gap_ref.sides), the
    profile along x (site_gap_ref.profile: x is not periodic), the search under L"""
    xyz = np.asarray(xyz, np.float64)
    side, cls = GR.sides(neigh, element, charge, metals, xyz[:, 0], NL, NR)
    gaps, stats = site_set_gap(xyz, side, r_max, cell, n_cells, L, propose)
    prof = GR.profile(cls, side, cell, n_cells, xyz[:, 0], *bins) if bins is not None else None
    return dict(gaps=gaps, stats=stats, side=side, profile=prof)


def index_coords(c):
    """(coords, nc): index cell coordinates of every site under kmcf_compute_cutoff_list_pbc's rule (pbc = 1): x in cells of
    the cutoff from the smallest x; in y and z max(1, floor(L / cutoff)) cells that tile one period from the smallest
    coordinate"""
    xyz, L, cutoff = c["xyz"], c["L"], c["cutoff"]
    lo = xyz.min(axis=0)
    assert (xyz.max(axis=0)[1:] - lo[1:] < L[1:]).all()
    ncx = int(np.floor((xyz[:, 0].max() - lo[0]) * (1.0 / cutoff))) + 1
    ncy, ncz = P.cells_per_period(L, cutoff)
    nc = np.array([ncx, ncy, ncz])
    inv = np.array([1.0 / cutoff, ncy / L[1], ncz / L[2]])
    return np.clip(np.floor((xyz - lo) * inv).astype(np.int64), 0, nc - 1), nc


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, side, cell (or None), n_cells, r_max, cutoff = radius of the periodic index, L) and, where the
# answer holds by construction, pairs = [(a, b, d2) or None per gap cell].

R_MAX, R_SMALL = 20.0, 12.0
RANDOM = P.PAIRWISE_CASES                  # p11, p23, p34, p52, lattice_wrap


def _random(name, r_max, per_cell):
    """the sites of pbc_ref.pairwise_case(name); about 2 % of them in both sets, about per_cell sites per gap cell, some
    cell ids outside [0, n_cells)"""
    p = P.pairwise_case(name)
    N = p["N"]
    n_cells = N // per_cell
    rng = np.random.default_rng(2001)
    side = rng.choice(4, N, p=[.3, .34, .34, .02]).astype(np.int32)
    cell = rng.integers(-1, n_cells + 1, N).astype(np.int32)
    return dict(name=name, xyz=p["xyz"], side=side, cell=cell, n_cells=n_cells, r_max=r_max, cutoff=P.CUTOFF, L=p["L"])


def _exact(name, L, cutoff, r_max, sites, pairs, x_hi=8.0):
    """sites: [((x, y, z), side, gap cell)]; two sites of no set and no cell pin the index: one at the origin, one a
    quarter below the far corner of the period"""
    sites = list(sites) + [((0.0, 0.0, 0.0), 0, -1), ((x_hi, L[1] - 0.25, L[2] - 0.25), 0, -1)]
    xyz = np.array([s[0] for s in sites], np.float64)
    assert (xyz * 4 == np.round(xyz * 4)).all()                                 # multiples of 1/4: the arithmetic is exact
    cell = np.array([s[2] for s in sites], np.int32)
    return dict(name=name, xyz=xyz, side=np.array([s[1] for s in sites], np.int32), cell=cell, n_cells=int(cell.max()) + 1,
                r_max=float(r_max), cutoff=float(cutoff), L=np.array(L, np.float64), pairs=pairs)


A_, B_ = 1, 2
L64 = (16.0, 64.0, 64.0)


def _corner():
    """a in the first index cell of y and z, its nearest b in the last of both: (dx, dy, dz) = (-2, 2, 3) through both faces;
    the nearest b without the wrap is 8 away (d2 = r_max^2: it counts, and loses)"""
    return _exact("corner", L64, 16.0, 8.0,
                  [((4, 1, 1), A_, 0), ((6, 63, 62), B_, 0), ((4, 9, 1), B_, 0), ((4, 30, 30), A_, 0)], [(0, 1, 17.0)])


def _rim_wrap(r_max=5.0):
    """one pair (-3, 4, 0) apart through the y face: d2 = 25 exactly; the other b is 8 away"""
    return _exact("rim_wrap", L64, 16.0, r_max, [((4, 1, 4), A_, 0), ((7, 61, 4), B_, 0), ((4, 1, 12), B_, 0)],
                  [(0, 1, 25.0) if r_max >= 5.0 else None])


def _half():
    """Ly = 25: one index cell in y.  Two gap cells, each one pair exactly Ly / 2 apart in y, a above b in one and below in
    the other: fy = +-0.5 rounds away from zero, dy = -+12.5, d2 = 156.25 either way"""
    return _exact("half", (16.0, 25.0, 64.0), 16.0, 13.0,
                  [((2, 17.5, 4), A_, 0), ((2, 5, 4), B_, 0), ((2, 5, 10), A_, 1), ((2, 17.5, 10), B_, 1)],
                  [(0, 1, 156.25), (2, 3, 156.25)])


def _ties_wrap():
    """per gap cell two a and two b, all four pairs at d2 = 4 + 16 = 20, one b through the y face and one inside: the winner
    is the smallest a, then the smallest b -- the b through the wrap in cell 0, the b inside in cell 1"""
    sites = []
    for g, z in enumerate((8.0, 40.0)):
        bs = [((4, 62, z), B_, g), ((4, 6, z), B_, g)]
        sites += [((6, 2, z), A_, g), ((2, 2, z), A_, g)] + (bs if g == 0 else bs[::-1])
    return _exact("ties_wrap", L64, 16.0, 6.0, sites, [(0, 2, 20.0), (4, 6, 20.0)])


def _two_cells():
    """Ly = 32, cutoff 16: two index cells in y, each next to the other through BOTH faces.  Gap cell 0: a at y = 14, its
    nearest b at y = 18 through the inner face (y = 16); gap cell 1: a at y = 2, its nearest b at y = 30 through the outer,
    wrapped face.  Each a has a b of its own index cell 6 away, and r_max = 12 is below the 14 that separates each a from
    the face it does not look through: a bound taken to the wrong face prunes the winner's cell"""
    return _exact("two_cells", (16.0, 32.0, 64.0), 16.0, 12.0,
                  [((4, 14, 8), A_, 0), ((4, 18, 8), B_, 0), ((4, 8, 8), B_, 0),
                   ((4, 2, 40), A_, 1), ((4, 30, 40), B_, 1), ((4, 8, 40), B_, 1)], [(0, 1, 16.0), (3, 4, 16.0)])


def _second_image():
    """Ly = 16 < 2 r_max = 24: b lies 11 above a and its image 5 below, both within r_max.  One pair, one distance: d2 = 25;
    n_right stays 1"""
    return _exact("second_image", (16.0, 16.0, 64.0), 16.0, 12.0, [((4, 1, 8), A_, 0), ((4, 12, 8), B_, 0)], [(0, 1, 25.0)])


def _interior():
    """a periodic index whose winner is nowhere near a face: the periodic and the open answer are equal"""
    return _exact("interior", L64, 16.0, 8.0,
                  [((4, 30, 30), A_, 0), ((6, 33, 31), B_, 0), ((4, 36, 30), B_, 0), ((8, 24, 30), A_, 0)], [(0, 1, 14.0)])


EXACT = {"corner": _corner, "rim_wrap": _rim_wrap, "rim_wrap_below": lambda: _rim_wrap(float(np.nextafter(5.0, 0.0))),
         "half": _half, "ties_wrap": _ties_wrap, "two_cells": _two_cells, "second_image": _second_image, "interior": _interior}
SEARCH_CASES = tuple("%s@%g" % (n, r) for n in RANDOM for r in (R_MAX, R_SMALL)) + tuple(EXACT)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in EXACT:
        return EXACT[name]()
    base, r = name.split("@")
    return _random(base, float(r), 8 if float(r) == R_MAX else 12)


@functools.lru_cache(maxsize=None)
def reference(name, periodic=True):
    """site_set_gap() of an input, computed once per process and never modified"""
    c = case(name)
    gaps, stats = site_set_gap(c["xyz"], c["side"], c["r_max"], c["cell"], c["n_cells"], c["L"] if periodic else None)
    gaps.setflags(write=False)
    return gaps, stats


# ---- stubs: two filament stumps that face each other across the y face ---------------------------------------------------------
STUB_METAL = 9
STUB_R_MAX = 10.0
STUB_LEFT = [(gx, 4, 2) for gx in (1, 2, 3, 4)]          # (x, y, z) lattice indices: from the left plane on, at y index 4
STUB_RIGHT = [(gx, 0, 2) for gx in (7, 8, 9, 10)]        # three planes further in x, at y index 0, up to the right plane


@functools.lru_cache(maxsize=None)
def stubs():
    """pbc_ref.box() (12 x 5 x 6 sites at 2.5 A, jittered, period 12.5 x 15 A): the first and the last x plane metal (30
    contact sites each), every other site O except two chains of neutral vacancies.  dict(xyz, L, element, charge, metals,
    NL, NR, N, left, right: the chains' site ids, per, opn: the periodic and the open neighbour list)."""
    b = P.box()
    g = b["grid"]
    site = lambda t: int(np.flatnonzero((g == np.array(t)).all(axis=1))[0])
    element = np.full(b["N"], P.O_EL, np.int32)
    element[g[:, 0] == 0] = STUB_METAL
    element[g[:, 0] == 11] = STUB_METAL
    left, right = np.array([site(t) for t in STUB_LEFT]), np.array([site(t) for t in STUB_RIGHT])
    element[left] = element[right] = P.VACANCY
    per, opn = P.box_lists()
    return dict(xyz=b["xyz"], L=b["L"], element=element, charge=np.zeros(b["N"], np.int32), metals=np.array([STUB_METAL], np.int32),
                NL=30, NR=30, N=b["N"], left=left, right=right, per=per, opn=opn)
