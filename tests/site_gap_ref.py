"""The restatement kmcf_site_set_gap and kmcf_filament_gap (csrc/kmcf_gap.hip) are held to: the definitions of
include/kmcfield.h in plain numpy, with scipy.spatial.cKDTree only proposing candidate pairs, and the synthetic cases the
tests run it on.

Candidates: every pair the tree finds within r_max * (1 + 1e-9) could be taken; the set is narrowed first, without
changing the result, to the pairs within d_nn * (1 + 1e-9) of each other, d_nn being the smallest nearest-neighbour
distance the tree reports for the cell (capped at the radius above) -- a pair at the exact minimum is not farther apart
than that.  On the candidates: the exact arithmetic of the contract, d2 = (dx*dx + dy*dy) + dz*dz with every operation
rounded, the test d2 <= r_max*r_max, and lexsort((b, a, d2)): smallest d2, then smallest a, then smallest b.

tests/test_site_gap_ref.py pins this file with answers known by construction; tests/test_gpu_site_gap.py holds the library
to it, array_equal on every field (gap: within 1 ulp of sqrt(gap2))."""
import numpy as np
from scipy.spatial import cKDTree

import clusters_ref as CR
import site_kernels_ref as SK

GAP_DTYPE = np.dtype([("gap", np.float64), ("gap2", np.float64), ("x_left", np.float64), ("x_right", np.float64),
                      ("site_left", np.int32), ("site_right", np.int32), ("n_left", np.int32), ("n_right", np.int32),
                      ("n_both", np.int32), ("bridged", np.int32)])           # kmcf_gap_t
STAT_KEYS = ("n_left", "n_right", "n_both", "cells_bridged", "cells_open", "cells_none")
EXACT_FIELDS = tuple(n for n in GAP_DTYPE.names if n != "gap")


def d2_exact(xyz, a, b):
    dx, dy, dz = (xyz[a, k] - xyz[b, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def nearest_pair(xyz, A, B, r_max):
    """(a, b, d2) of the contract for the site lists A, B (one gap cell), or None"""
    if len(A) == 0 or len(B) == 0:
        return None
    tree = cKDTree(xyz[B])
    R = r_max * (1 + 1e-9)
    d, _ = tree.query(xyz[A], k=1, distance_upper_bound=R)
    if not np.isfinite(d.min()):
        return None
    rad = min(R, d.min() * (1 + 1e-9) + 1e-12)
    near = A[d <= rad]
    lists = tree.query_ball_point(xyz[near], rad)
    a = np.repeat(near, [len(l) for l in lists])
    b = B[np.concatenate([np.asarray(l, np.int64) for l in lists])]
    d2 = d2_exact(xyz, a, b)
    ok = d2 <= r_max * r_max
    if not ok.any():
        return None
    a, b, d2 = a[ok], b[ok], d2[ok]
    k = np.lexsort((b, a, d2))[0]
    return int(a[k]), int(b[k]), float(d2[k])


def cells_of(cell, n_cells, N):
    """gap cell per site, -1: none"""
    if cell is None:
        assert n_cells == 1
        return np.zeros(N, np.int64)
    cell = np.asarray(cell).astype(np.int64)
    return np.where((cell >= 0) & (cell < n_cells), cell, -1)


def site_set_gap(xyz, side, r_max, cell=None, n_cells=1):
    """(gaps, stats): GAP_DTYPE records of the n_cells gap cells, the integer fields of kmcf_gap_stats_t"""
    xyz = np.asarray(xyz, np.float64)
    r_max = float(r_max)
    N = len(xyz)
    side = np.asarray(side).astype(np.int64) & 3
    cell = cells_of(cell, n_cells, N)
    gaps = np.zeros(n_cells, GAP_DTYPE)
    gaps["gap"] = gaps["gap2"] = np.inf
    gaps["site_left"] = gaps["site_right"] = -1
    inside = cell >= 0
    for f, bit in (("n_left", (side & 1) != 0), ("n_right", (side & 2) != 0), ("n_both", side == 3)):
        gaps[f] = np.bincount(cell[inside & bit], minlength=n_cells)
    gaps["bridged"] = gaps["n_both"] > 0
    member = np.flatnonzero(inside & (side != 0))
    order = member[np.argsort(cell[member], kind="stable")]                    # ascending site id inside a cell
    bounds = np.searchsorted(cell[order], np.arange(n_cells + 1))
    for c in range(n_cells):
        sites = order[bounds[c]:bounds[c + 1]]
        got = nearest_pair(xyz, sites[(side[sites] & 1) != 0], sites[(side[sites] & 2) != 0], r_max)
        if got is not None:
            a, b, d2 = got
            gaps[c]["gap2"], gaps[c]["gap"] = d2, np.sqrt(d2)
            gaps[c]["site_left"], gaps[c]["site_right"] = a, b
            gaps[c]["x_left"], gaps[c]["x_right"] = xyz[a, 0], xyz[b, 0]
    found = gaps["site_left"] >= 0
    stats = dict(n_left=int(((side & 1) != 0).sum()), n_right=int(((side & 2) != 0).sum()), n_both=int((side == 3).sum()),
                 cells_bridged=int((gaps["bridged"] != 0).sum()), cells_open=int(((gaps["bridged"] == 0) & found).sum()),
                 cells_none=int(((gaps["bridged"] == 0) & ~found).sum()))
    return gaps, stats


def sides(neigh, element, charge, metals, x, NL, NR):
    """(side, cls): side[i] = touch of i's cluster for members, 0 for non-members"""
    label, table, _ = CR.clusters(neigh, element, charge, metals, x, NL, NR)
    touch = np.zeros(len(label), np.int32)
    touch[table["root"]] = table["touch"]
    member = label >= 0
    side = np.zeros(len(label), np.int32)
    side[member] = touch[label[member]]
    return side, CR.classes(element, charge, metals)


def profile(cls, side, cell, n_cells, x, n_bins, x_lo, x_hi):
    """(n_cells, n_bins, 3) counts of the conductive vacancies per gap cell, x bin and side 1 / 2 / 3"""
    x = np.asarray(x, np.float64)
    cell = cells_of(cell, n_cells, len(x))
    inv_w = n_bins / (float(x_hi) - float(x_lo))
    t = (x - float(x_lo)) * inv_w
    s = np.asarray(side).astype(np.int64) & 3
    ok = (np.asarray(cls) == CR.VAC) & (s != 0) & (cell >= 0) & (t >= 0) & (t < n_bins)
    out = np.zeros((n_cells, n_bins, 3), np.int32)
    np.add.at(out, (cell[ok], t[ok].astype(np.int64), s[ok] - 1), 1)
    return out


def filament_gap(neigh, element, charge, metals, xyz, NL, NR, r_max, cell=None, n_cells=1, bins=None):
    """dict(gaps, stats, side, profile) of kmcf_filament_gap"""
    xyz = np.asarray(xyz, np.float64)
    side, cls = sides(neigh, element, charge, metals, xyz[:, 0], NL, NR)
    gaps, stats = site_set_gap(xyz, side, r_max, cell, n_cells)
    prof = profile(cls, side, cell, n_cells, xyz[:, 0], *bins) if bins is not None else None
    return dict(gaps=gaps, stats=stats, side=side, profile=prof)


def constriction(prof_cell):
    """smallest side-3 count of one gap cell's profile (n_bins, 3) between its first and last bin that hold one; 0 if none"""
    s3 = np.asarray(prof_cell)[:, 2]
    nz = np.flatnonzero(s3)
    return int(s3[nz[0]:nz[-1] + 1].min()) if len(nz) else 0


# ---- synthetic cases ---------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, side, cell (or None), n_cells, r_max, cutoff = edge of the index cells) and what is known about it.

def index_coords(c):
    """index cell coordinates of every site under kmcf_compute_cutoff_list's rule"""
    xyz, inv = c["xyz"], 1.0 / c["cutoff"]
    lo = xyz.min(axis=0)
    nc = np.floor((xyz.max(axis=0) - lo) * inv).astype(np.int64) + 1
    return np.clip(np.floor((xyz - lo) * inv).astype(np.int64), 0, nc - 1), nc


def _shuffled(c, seed):
    """the same case with the site ids permuted"""
    perm = np.random.default_rng(seed).permutation(len(c["xyz"]))             # new id k holds old site perm[k]
    c["xyz"], c["side"] = np.ascontiguousarray(c["xyz"][perm]), c["side"][perm]
    if c["cell"] is not None:
        c["cell"] = c["cell"][perm]
    c["old_id"] = perm
    return c


def _planes():
    """36 A sites in the plane x = 0, 36 B sites in the plane x = 3, shifted by half a spacing in y: every pair of
    neighbours across has d2 = 9 + 1.25^2 exactly; an A site off the rim has two such B sites"""
    i, j = (g.ravel() for g in np.meshgrid(np.arange(6), np.arange(6), indexing="ij"))
    A = np.stack([np.zeros(36), 2.5 * i, 2.5 * j], axis=1)
    B = np.stack([np.full(36, 3.0), 2.5 * i + 1.25, 2.5 * j], axis=1)
    c = dict(name="planes", xyz=np.concatenate([A, B]), side=np.repeat(np.array([1, 2], np.int32), 36), cell=None, n_cells=1,
             r_max=4.0, cutoff=4.0, d2=9.0 + 1.5625)
    return _shuffled(c, 5)


RELATIONS = [(sx, sy, sz) for sx in (-1, 0, 1) for sy in (-1, 0, 1) for sz in (-1, 0, 1)]


def _straddle():
    """27 gap cells, one per relation of two index cells (same, 6 faces, 12 edges, 8 corners): the nearest pair (a, b) of
    gap cell g has b in the index cell at offset RELATIONS[g] from a's; a decoy of each set lies farther off"""
    edge = 5.0
    pts, side, cell, pairs = [], [], [], []
    for g, s in enumerate(RELATIONS):
        s = np.array(s, np.float64)
        o = edge * np.array([4 * g + 1, 1, 1], np.float64)
        a = o + 2.5 + 2.25 * s                                                  # a quarter from the faces it looks at
        if s.any():
            b, b2, a2 = a + 0.5 * s, a - 1.0 * s, a + 2.0 * s
        else:
            b, b2, a2 = a + np.array([0.5, 0, 0]), a + np.array([0, 1.5, 0]), a + np.array([2.0, 0, 0])
        k = len(pts)
        pts += [a, b, b2, a2]
        side += [1, 2, 2, 1]
        cell += [g] * 4
        pairs.append((k, k + 1, float(((a - b) ** 2).sum())))
    pts += [np.zeros(3), edge * np.array([4 * 27, 3, 3], np.float64) - 0.5]     # the corners of the index
    side += [0, 0]
    cell += [-1, -1]
    c = dict(name="straddle", xyz=np.array(pts), side=np.array(side, np.int32), cell=np.array(cell, np.int32), n_cells=27,
             r_max=5.0, cutoff=edge)
    c = _shuffled(c, 6)
    new_id = np.argsort(c["old_id"])
    c["pairs"] = [(int(new_id[a]), int(new_id[b]), d2) for a, b, d2 in pairs]
    return c


def _rim(r_max):
    """one pair (3, 4, 0) apart: d2 = 25 exactly; the other B sites lie inside the 27 index cells (edge 15) but farther than
    r_max"""
    a = np.array([20.0, 20.0, 20.0])
    far = [a + v for v in ([6.0, 0, 0], [0, -7.5, 2.0], [-9.0, 3.0, 3.0], [4.0, 4.0, 4.0], [0, 0, 13.0], [-5.0, -0.5, 0])]
    pts = [a, a + np.array([3.0, 4.0, 0.0])] + far + [np.zeros(3), np.full(3, 44.0)]
    side = [1, 2] + [2] * len(far) + [0, 0]
    return dict(name="rim", xyz=np.array(pts), side=np.array(side, np.int32), cell=None, n_cells=1, r_max=r_max, cutoff=15.0)


def _mixed():
    """20 000 random points in a box of 40, sides and gap cells drawn at random: 1000 gap cells, some sites in none, a few
    sites in both sets; the gap cells from 980 on hold no A site or no B site"""
    rng = np.random.default_rng(2024)
    N, n_cells = 20000, 1000
    xyz = rng.uniform(0.0, 40.0, (N, 3))
    u = rng.random(N)
    side = np.zeros(N, np.int32)
    side[u < 0.3] = 1
    side[(u >= 0.3) & (u < 0.6)] = 2
    side[u >= 0.999] = 3
    side[(u >= 0.6) & (u < 0.62)] = 4 + 8                                       # bits above 1 are ignored
    cell = rng.integers(0, n_cells, N).astype(np.int32)
    junk = rng.random(N) < 0.05
    cell[junk] = np.resize(np.array([-1, n_cells, -7, 5 * n_cells], np.int32), int(junk.sum()))
    side[(cell >= 990) & (cell < n_cells)] &= 1
    side[(cell >= 980) & (cell < 990)] &= 2
    return dict(name="mixed", xyz=xyz, side=side, cell=cell, n_cells=n_cells, r_max=4.5, cutoff=5.0)


def _dense():
    """3000 B sites and 600 A sites in ONE index cell (edge 5), three gap cells; two far sites make the index larger"""
    rng = np.random.default_rng(99)
    xyz = np.concatenate([rng.uniform(0.0, 4.9, (3600, 3)), np.array([[0.0, 0, 0], [12.0, 12.0, 12.0]])])
    side = np.concatenate([np.full(600, 1), np.full(3000, 2), [0, 0]]).astype(np.int32)
    cell = np.concatenate([rng.integers(0, 3, 3600), [-1, -1]]).astype(np.int32)
    return _shuffled(dict(name="dense", xyz=xyz, side=side, cell=cell, n_cells=3, r_max=0.5, cutoff=5.0), 7)


def index_positions(c):
    """position of every site in the index's cell order (cell id (cx ncy + cy) ncz + cz, ascending site id inside a cell):
    the order in which the compaction scans the flags, SCAN_TILE of them per tile"""
    coords, nc = index_coords(c)
    cid = (coords[:, 0] * nc[1] + coords[:, 1]) * nc[2] + coords[:, 2]
    pos = np.empty(len(cid), np.int64)
    pos[np.argsort(cid, kind="stable")] = np.arange(len(cid))
    return pos


def _large():
    """The 83 x 81 x 80 jittered lattice of the pairwise tests (537 840 sites, 263 scan tiles, index cells of 20 A), one gap
    cell.  Members only at the two ends of the cell order: from position 256 tiles on (a random third each A, B, none) and
    48 positions of the first tile -- the A and B counts of tiles 1 .. 255 are zero, so both totals and every offset of
    the last tiles hold what the scan carries from its first pass of 256 tiles into its second.  One B site of the last
    tile is moved to 0.3 A from an A site of the last tile: closer than two lattice sites can be (4 - 0.6 A), so
    pair = (a, b, d2) is the answer by construction.  (The record itself would survive a lost carry, which moves all
    those list positions alike: `large_two` is the case that notices.)"""
    xyz = SK.pairwise_case("large")["xyz"].copy()
    base = dict(xyz=xyz, cutoff=SK.CUTOFF)
    last = np.flatnonzero(index_positions(base) >= 262 * SK.SCAN_TILE)
    a, b = int(last[len(last) // 2]), int(last[len(last) // 2 + 1])             # two sites inside the last index cells
    xyz[b] = xyz[a] + np.array([0.3, 0.0, 0.0])
    pos = index_positions(base)                                                # (of the final coordinates)
    rng = np.random.default_rng(263)
    side = np.zeros(len(xyz), np.int32)
    ends = (pos >= 256 * SK.SCAN_TILE) | ((pos >= 1000) & (pos < 1048))
    side[ends] = rng.integers(0, 3, int(ends.sum()))
    side[a], side[b] = 1, 2
    return dict(name="large", xyz=xyz, side=side, cell=None, n_cells=1, r_max=SK.CUTOFF, cutoff=SK.CUTOFF,
                pair=(a, b, float(d2_exact(xyz, a, b))))


def _large_two():
    """`large` with TWO gap cells, so that a record depends on what the scan carries from its first pass of 256 tiles into
    its second: gap cell 0 = the positions below 256 tiles (its members: 48 positions of the first tile and a planted pair
    there), gap cell 1 = the positions from 256 tiles on, its planted pair (a1, b1) at the very start of tile 256.  With
    the carry lost, tile 256's first members are written to the list slots of the first tile's members: whichever write
    stays, one cell loses a site of its planted pair (device_search(carry=False) shows both outcomes)."""
    T = SK.SCAN_TILE
    xyz = SK.pairwise_case("large")["xyz"].copy()
    base = dict(xyz=xyz, cutoff=SK.CUTOFF)
    at = np.argsort(index_positions(base))                                      # site at every position
    a0, b0, a1, b1 = (int(at[p]) for p in (1010, 1011, 256 * T + 2, 256 * T + 3))
    xyz[b0] = xyz[a0] + np.array([0.3, 0.0, 0.0])
    xyz[b1] = xyz[a1] + np.array([0.3, 0.0, 0.0])
    pos = index_positions(base)                                                # (of the final coordinates)
    rng = np.random.default_rng(264)
    side = np.zeros(len(xyz), np.int32)
    first, tail = (pos >= 1000) & (pos < 1048), pos >= 256 * T
    side[first] = rng.integers(0, 3, int(first.sum()))                         # a third each: A, B, none
    side[tail] = rng.choice(np.array([0, 1, 2], np.int32), int(tail.sum()), p=[0.8, 0.1, 0.1])
    side[[a0, a1]], side[[b0, b1]] = 1, 2
    return dict(name="large_two", xyz=xyz, side=side, cell=(pos >= 256 * T).astype(np.int32), n_cells=2, r_max=SK.CUTOFF,
                cutoff=SK.CUTOFF, pairs=[(a0, b0, float(d2_exact(xyz, a0, b0))), (a1, b1, float(d2_exact(xyz, a1, b1)))])


def _tile_edge(N):
    """SK.tile_edge_sites(N) (N = 2047, 2048, 2049: a scan tile one item short, exactly full, one item over), one gap cell, a
    random third of the sites each A, B, none.  The B site b is the one at the LAST position of the index's cell order; the A
    site a at the position before it is moved to 0.35 A from b, towards the lower corner, closer than two lattice sites can be
    (4 - 0.6 A): pair = (a, b, d2) is the answer by construction, and it is lost if the last item of the scan is."""
    xyz, order = SK.tile_edge_sites(N)
    xyz = xyz.copy()
    a, b = int(order[-2]), int(order[-1])
    xyz[a] = xyz[b] - 0.2
    c = dict(name="tile_edge@%d" % N, xyz=xyz, cell=None, n_cells=1, r_max=SK.CUTOFF, cutoff=SK.CUTOFF)
    assert index_positions(c)[b] == N - 1                                      # (of the final coordinates)
    side = np.random.default_rng(270 + N).integers(0, 3, N).astype(np.int32)
    side[a], side[b] = 1, 2
    return dict(c, side=side, pair=(a, b, float(d2_exact(xyz, a, b))))


def device_search(c, carry=True, later_write_stays=True):
    """The compaction and search of csrc/kmcf_gap.hip restated step by step on the index's cell order -- per-tile counts of
    the A and B flags, their exclusive scan in passes of 256 tiles, the scatter into the member lists, the walk of the
    runs bpos[cell_start[..]] of the 27 index cells, the minimum per gap cell -- so that a defect of the scan can be put
    in: carry=False starts every pass of the scan from 0 (offsets and the total), and later_write_stays picks which of
    two writes to one list slot survives (ascending or descending tile).  Returns [(a, b, d2) or None per gap cell]."""
    T = SK.SCAN_TILE
    xyz, r2 = c["xyz"], c["r_max"] * c["r_max"]
    N = len(xyz)
    gcell = cells_of(c["cell"], c["n_cells"], N)
    coords, nc = index_coords(c)
    cid = (coords[:, 0] * nc[1] + coords[:, 1]) * nc[2] + coords[:, 2]
    order = np.argsort(cid, kind="stable")
    cell_start = np.searchsorted(cid[order], np.arange(int(nc.prod()) + 1))
    flags = np.where(gcell[order] >= 0, c["side"][order] & 3, 0)

    def positions(flag):                                                       # (list position of every slot, total)
        cnt = np.add.reduceat(flag.astype(np.int64), np.arange(0, N, T))
        off = np.zeros(len(cnt), np.int64)
        total = 0
        for p0 in range(0, len(cnt), 256):
            base = total if carry else 0
            off[p0:p0 + 256] = base + np.cumsum(cnt[p0:p0 + 256]) - cnt[p0:p0 + 256]
            total = base + int(cnt[p0:p0 + 256].sum())
        inside = np.cumsum(flag) - flag.astype(np.int64)
        inside = inside - np.repeat(inside[::T], T)[:N]
        return np.repeat(off, T)[:N] + inside, total

    def scatter(flag, where, total):
        t = np.flatnonzero(flag)
        if not later_write_stays:
            t = t[::-1]
        lst = np.full(max(total, int(where[t].max()) + 1 if len(t) else 0), -1, np.int64)
        lst[where[t]] = order[t]                                                # (a repeated index keeps the last value)
        return lst[:total]

    fa, fb = (flags & 1) != 0, (flags & 2) != 0
    apos, n_a = positions(fa)
    bpos, n_b = positions(fb)
    alist, bsite = scatter(fa, apos, n_a), scatter(fb, bpos, n_b)
    bpos = np.append(bpos, n_b)
    best = [None] * c["n_cells"]
    for a in alist[alist >= 0]:                                                # (-1: a slot below the total that nobody wrote)
        cx, cy, cz = coords[a]
        runs = []
        for ax in range(max(cx - 1, 0), min(cx + 1, nc[0] - 1) + 1):
            for ay in range(max(cy - 1, 0), min(cy + 1, nc[1] - 1) + 1):
                lo = (ax * nc[1] + ay) * nc[2] + max(cz - 1, 0)
                hi = (ax * nc[1] + ay) * nc[2] + min(cz + 1, nc[2] - 1)
                runs.append(np.arange(bpos[cell_start[lo]], min(bpos[cell_start[hi + 1]], n_b)))
        b = bsite[np.concatenate(runs)]
        b = b[b >= 0]
        b = b[gcell[b] == gcell[a]]
        d2 = d2_exact(xyz, a, b)
        for k in np.flatnonzero(d2 <= r2):
            got = (float(d2[k]), int(a), int(b[k]))
            if best[gcell[a]] is None or got < best[gcell[a]]:
                best[gcell[a]] = got
    return [None if g is None else (g[1], g[2], g[0]) for g in best]


BUILDERS = {"planes": _planes, "straddle": _straddle, "rim": lambda: _rim(5.0),
            "rim_below": lambda: _rim(float(np.nextafter(5.0, 0.0))), "mixed": _mixed, "dense": _dense, "large": _large,
            "large_two": _large_two, **{"tile_edge@%d" % n: (lambda n=n: _tile_edge(n)) for n in SK.TILE_EDGE_SIZES}}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def reference(name):
    """site_set_gap() of a synthetic case, computed once per process and never modified"""
    key = ("ref", name)
    if key not in _cache:
        c = case(name)
        gaps, stats = site_set_gap(c["xyz"], c["side"], c["r_max"], c["cell"], c["n_cells"])
        gaps.setflags(write=False)
        _cache[key] = (gaps, stats)
    return _cache[key]
