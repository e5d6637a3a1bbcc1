"""The restatement kmcf_site_set_chain_pbc and kmcf_filament_chain_pbc (csrc/kmcf_chain.hip, the periodic ch_search_kernel) are held
to: the contract of include/kmcfield.h in plain numpy, and the inputs the tests run it on.  No GPU.

Vertices, Kruskal, the rounds of Boruvka, the tree walk and the record types are those of tests/site_chain_ref.py; the pair
distance, `fold` and `crossings` are those of tests/site_gap_pbc_ref.py --
    dx = x[a] - x[b];  fy = (y[a] - y[b]) / Ly;  fy = fy - round(fy);  dy = fy * Ly   (z likewise; pbc_ref.c_round)
    d2 = (dx*dx + dy*dy) + dz*dz
What is restated here is the links under a lattice L = (Lx, Ly, Lz): a k-d tree over the nine (y, z)-shifted copies of a
group proposes the pairs within r_max * (1 + 1e-9) + 1e-9 (far more than the tree's distance and the contract's can
differ; the minimum image is never farther than any other image, so every counting pair is proposed); the proposals are
de-duplicated -- one pair, one row, however many of its images are near --; the exact d2 decides (d2 <= r_max*r_max),
lexsort((hi, lo, d2)), the first row per vertex pair is the link.  No cell list and nothing shared with the kernel.
L = None is the open-boundary search: the result then equals site_chain_ref.site_set_chain (asserted in
tests/test_site_chain_pbc_ref.py, which also asserts what every input below is built for)."""
import functools

import numpy as np
from scipy.spatial import cKDTree

import pbc_ref as P
import site_chain_ref as R
import site_gap_pbc_ref as GP

CHAIN_DTYPE, HOP_DTYPE = R.CHAIN_DTYPE, R.HOP_DTYPE
NONE, OPEN, CHAINED, BRIDGED = R.NONE, R.OPEN, R.CHAINED, R.BRIDGED
V_LEFT, V_RIGHT = R.V_LEFT, R.V_RIGHT
vertices, kruskal_path, boruvka_path, tree_path = R.vertices, R.kruskal_path, R.boruvka_path, R.tree_path
d2_exact, fold, crossings = GP.d2_exact, GP.fold, GP.crossings


def near_pairs(xyz, A, B, reach, L):
    """(a, b): the pairs of a in A and b in B of which some (y, z) image lies within `reach`, each pair once"""
    if len(A) == 0 or len(B) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    shifts = [(sy, sz) for sy in (-1, 0, 1) for sz in (-1, 0, 1)] if L is not None else [(0, 0)]
    pts = np.concatenate([xyz[B] + np.array([0.0, sy * L[1], sz * L[2]]) for sy, sz in shifts]) if L is not None else xyz[B]
    m = cKDTree(xyz[A]).sparse_distance_matrix(cKDTree(pts), reach, output_type="ndarray")
    a, b = A[m["i"]], B[m["j"] % len(B)]
    key = np.unique(a.astype(np.int64) * len(xyz) + b)
    return key // len(xyz), key % len(xyz)


def candidate_pairs(xyz, sites, vid, r_max, L):
    """(a, b) proposals between the cell's L, R and stone sites, and among its stones (a < b there); one row per pair"""
    reach = r_max * (1 + 1e-9) + 1e-9
    groups = [sites[vid == V_LEFT], sites[vid == V_RIGHT], sites[vid >= 0]]
    a, b = [], []
    for p, q in ((0, 1), (0, 2), (1, 2)):
        pa, pb = near_pairs(xyz, groups[p], groups[q], reach, L)
        a.append(pa)
        b.append(pb)
    pa, pb = near_pairs(xyz, groups[2], groups[2], reach, L)
    a.append(pa[pa < pb])
    b.append(pb[pa < pb])
    return np.concatenate(a), np.concatenate(b)


def cell_links(xyz, sites, vid, r_max, L=None):
    """site_chain_ref.cell_links under the lattice L: ((d2, a, b, va, vb) sorted by key, a < b, one row per linked vertex
    pair; the mask over `sites` of those with a site of another vertex within r_max)"""
    a, b = candidate_pairs(xyz, sites, vid, r_max, L)
    vertex = np.zeros(len(xyz), np.int64)
    vertex[sites] = vid
    va, vb = vertex[a], vertex[b]
    d2 = d2_exact(xyz, a, b, L)
    ok = (d2 <= r_max * r_max) & (va != vb)
    a, b, va, vb, d2 = a[ok], b[ok], va[ok], vb[ok], d2[ok]
    surface = np.isin(sites, np.concatenate([a, b]))
    swap = a > b
    a, b, va, vb = np.where(swap, b, a), np.where(swap, a, b), np.where(swap, vb, va), np.where(swap, va, vb)
    o = np.lexsort((b, a, d2))
    a, b, va, vb, d2 = a[o], b[o], va[o], vb[o], d2[o]
    lo, hi = np.minimum(va, vb) + 2, np.maximum(va, vb) + 2
    _, first = np.unique(lo * (len(xyz) + 2) + hi, return_index=True)
    first.sort()
    return (d2[first], a[first], b[first], va[first], vb[first]), surface


def cell_members(side, node, cell, n_cells):
    """per searched gap cell (both terminals, no site on both sides): (c, member sites, their vertex ids)"""
    node = np.asarray(node).astype(np.int64)
    side, own, stone, vcell = vertices(side, node, cell, n_cells)
    inside = own >= 0
    n_left = np.bincount(own[inside & ((side & 1) != 0)], minlength=n_cells)
    n_right = np.bincount(own[inside & ((side & 2) != 0)], minlength=n_cells)
    n_both = np.bincount(own[inside & (side == 3)], minlength=n_cells)
    for c in range(n_cells):
        if n_both[c] == 0 and n_left[c] > 0 and n_right[c] > 0:
            sites = np.flatnonzero(vcell == c)
            yield c, sites, np.where(stone[sites], node[sites], np.where(side[sites] == 1, V_LEFT, V_RIGHT))


def site_set_chain(xyz, side, node, r_max, cell=None, n_cells=1, max_hops=0, L=None, boruvka=False):
    """site_chain_ref.site_set_chain with the pair distance the minimum image under L = (Lx, Ly, Lz) (None: open
    boundaries): dict(chains, hops, paths, stats, rounds, links: the sorted links per searched cell)"""
    xyz = np.asarray(xyz, np.float64)
    r_max = float(r_max)
    node = np.asarray(node).astype(np.int64)
    side, own, stone, vcell = vertices(side, node, cell, n_cells)
    chains = np.zeros(n_cells, CHAIN_DTYPE)
    hops = np.zeros((n_cells, max_hops), HOP_DTYPE)
    hops["from"] = hops["to"] = -1
    hops["d2"] = np.inf
    inside = own >= 0
    chains["n_left"] = np.bincount(own[inside & ((side & 1) != 0)], minlength=n_cells)
    chains["n_right"] = np.bincount(own[inside & ((side & 2) != 0)], minlength=n_cells)
    n_both = np.bincount(own[inside & (side == 3)], minlength=n_cells)
    chains["n_stone_sites"] = np.bincount(vcell[stone], minlength=n_cells)
    homes = np.unique(node[stone], return_index=True)[1]
    chains["n_stones"] = np.bincount(vcell[np.flatnonzero(stone)[homes]], minlength=n_cells)
    chains["hop_max"] = chains["hop_max2"] = chains["direct2"] = np.inf
    chains["neck_from"] = chains["neck_to"] = -1
    chains["status"] = np.where(n_both > 0, BRIDGED, np.where((chains["n_left"] == 0) | (chains["n_right"] == 0), NONE, OPEN))
    for f in ("hop_max", "hop_max2", "direct2"):
        chains[f][n_both > 0] = 0.0
    paths, rounds, links_of, surface_sites = [None] * n_cells, [], {}, 0
    for c, sites, vid in cell_members(side, node, cell, n_cells):
        r = chains[c]
        links, surface = cell_links(xyz, sites, vid, r_max, L)
        links_of[c] = links
        surface_sites += int(surface.sum())
        direct = (np.minimum(links[3], links[4]) == V_RIGHT) & (np.maximum(links[3], links[4]) == V_LEFT)
        if direct.any():
            r["direct2"] = links[0][direct][0]
        path = kruskal_path(links)
        if boruvka:
            again, n = boruvka_path(links)
            assert again == path
            rounds.append(n)
        paths[c] = path
        if path is None:
            continue
        r["status"], r["n_hops"] = CHAINED, len(path)
        neck = max(path, key=lambda h: (h[2], min(h[0], h[1]), max(h[0], h[1])))
        r["hop_max2"], r["hop_max"] = neck[2], np.sqrt(neck[2])
        r["neck_from"], r["neck_to"] = neck[0], neck[1]
        length = 0.0
        for h in path:
            length += float(np.sqrt(h[2]))
        r["length"] = length
        for k, h in enumerate(path[:max_hops]):
            hops[c, k] = h
    st = chains["status"]
    stats = dict(cells_none=int((st == NONE).sum()), cells_open=int((st == OPEN).sum()), cells_chained=int((st == CHAINED).sum()),
                 cells_bridged=int((st == BRIDGED).sum()), n_stones=int(chains["n_stones"].sum()),
                 n_stone_sites=int(chains["n_stone_sites"].sum()), surface_sites=surface_sites)
    return dict(chains=chains, hops=hops, paths=paths, stats=stats, rounds=rounds, links=links_of)


def candidates_of(c):
    """(a, b): every proposed pair of every searched gap cell of an input"""
    a, b = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for _, sites, vid in cell_members(c["side"], c["node"], c["cell"], c["n_cells"]):
        pa, pb = candidate_pairs(c["xyz"], sites, vid, c["r_max"], c["L"])
        a.append(pa)
        b.append(pb)
    return np.concatenate(a), np.concatenate(b)


def stones_through_a_face(c):
    """the nodes of an input's stones that have sites on both sides of a y or z face: two of its sites are nearest to each
    other through the face"""
    xyz, L = c["xyz"], c["L"]
    node = np.asarray(c["node"]).astype(np.int64)
    _, _, stone, _ = vertices(c["side"], node, c["cell"], c["n_cells"])
    out = []
    for n in np.unique(node[stone]):
        s = np.flatnonzero(stone & (node == n))
        if len(s) < 2:
            continue
        a, b = np.meshgrid(s, s, indexing="ij")
        ny, nz = fold(xyz[a, 1], xyz[b, 1], L[1])[1], fold(xyz[a, 2], xyz[b, 2], L[2])[1]
        near = d2_exact(xyz, a, b, L) <= 16.0
        if (near & ((ny != 0) | (nz != 0))).any():
            out.append(int(n))
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, side, node, cell (or None), n_cells, r_max, cutoff = radius of the periodic index, L, max_hops) and,
# where the answer holds by construction, hops = [[(from, to, d2), ...] or None per gap cell].

L64 = (16.0, 64.0, 64.0)
_L, _R, _S = 1, 2, 0


def _exact(name, L, cutoff, r_max, sites, hops, x_hi=8.0, max_hops=8, shuffle=None):
    """sites: [((x, y, z), side, node, gap cell)]; two sites of no vertex and no cell pin the index: one at the origin, one a
    quarter below the far corner of the period.  Coordinates in multiples of 1/4 and periods that are powers of two (or
    differences of exactly half a period): the arithmetic of the listed hops is exact."""
    sites = list(sites) + [((0.0, 0.0, 0.0), 0, -1, -1), ((x_hi, L[1] - 0.25, L[2] - 0.25), 0, -1, -1)]
    xyz = np.array([s[0] for s in sites], np.float64)
    assert (xyz * 4 == np.round(xyz * 4)).all()
    cell = np.array([s[3] for s in sites], np.int32)
    c = dict(name=name, xyz=xyz, side=np.array([s[1] for s in sites], np.int32), node=np.array([s[2] for s in sites], np.int32),
             cell=cell, n_cells=int(cell.max()) + 1, r_max=float(r_max), cutoff=float(cutoff), L=np.array(L, np.float64),
             max_hops=max_hops)
    if shuffle is not None:
        c = R._shuffled(c, shuffle)
        hops = [None if h is None else R._renamed(c, h) for h in hops]
    c["hops"] = hops
    return c


def _wrap_ladder():
    """L at y = 1, R at y = 62.75, and between them THROUGH the y face the stones at y = 0.25 and y = 63.5: three hops of
    0.75; inside the cell L and R are 61.75 apart and the two stones 63.25"""
    z = 8.0
    return _exact("wrap_ladder", L64, 16.0, 1.0,
                  [((4, 1, z), _L, -1, 0), ((4, 0.25, z), _S, 7, 0), ((4, 63.5, z), _S, 3, 0), ((4, 62.75, z), _R, -1, 0),
                   ((4, 1, z + 1.5), _S, 5, 0), ((5.5, 63.5, z), _S, 6, 0)],
                  [[(0, 1, 0.5625), (1, 2, 0.5625), (2, 3, 0.5625)]], shuffle=21)


def _corner():
    """L in the first index cell of y and z, the stone in the last of both: (dx, dy, dz) = (-2, 2, 3) through both faces at
    once, d2 = 17; the stone is 3 from R; L - R are linked directly through both faces as well, at 4 + 25 + 9 = 38"""
    return _exact("corner", L64, 16.0, 8.0, [((4, 1, 1), _L, -1, 0), ((6, 63, 62), _S, 2, 0), ((6, 60, 62), _R, -1, 0)],
                  [[(0, 1, 17.0), (1, 2, 9.0)]])


def _wrap_detour():
    """site_chain_ref's `detour` with the stones beyond the y face: the direct link l1 - r1 inside the cell at exactly
    r_max^2 = 25 (3, 4, 0), and l0 - s1 - s2 - r0 with hops 3 (through the face), 3.5 and 3: hop_max2 = 12.25, direct2 = 25"""
    return _exact("wrap_detour", L64, 16.0, 5.0,
                  [((4, 1, 30), _L, -1, 0), ((4, 62, 30), _S, 0, 0), ((4, 62, 33.5), _S, 1, 0), ((4, 59, 33.5), _R, -1, 0),
                   ((4, 30, 30), _L, -1, 0), ((7, 34, 30), _R, -1, 0)],
                  [[(0, 1, 9.0), (1, 2, 12.25), (2, 3, 9.0)]], shuffle=22)


def _rim_wrap(r_max=5.0):
    """l0 - s1 - s2 with hops 3 and 4 inside the cell, and the last hop s2 - r0 (-3, 4, 0) through the y face: d2 = 25
    exactly.  r_max = 5: CHAINED; r_max just below: that hop is no link and nothing replaces it: OPEN.  More stones in the
    index cells around, farther than 5 from everything."""
    return _exact("rim_wrap" if r_max >= 5.0 else "rim_wrap_below", L64, 16.0, r_max,
                  [((4, 8, 4), _L, -1, 0), ((4, 5, 4), _S, 0, 0), ((4, 1, 4), _S, 1, 0), ((7, 61, 4), _R, -1, 0),
                   ((4, 20, 4), _S, 2, 0), ((4, 55, 10), _S, 3, 0), ((4, 1, 58), _S, 4, 0), ((4, 12, 12), _S, 5, 0)],
                  [[(0, 1, 9.0), (1, 2, 16.0), (2, 3, 25.0)] if r_max >= 5.0 else None])


def _half():
    """Ly = 25: one index cell in y.  Two gap cells, each with its first hop L - stone exactly Ly / 2 apart in y, L above
    the stone in one and below it in the other: fy = +-0.5 rounds away from zero, d2 = 156.25 from either end; the stone
    is 6 from R along x, and L - R (36 + 156.25) is beyond r_max = 13"""
    return _exact("half", (16.0, 25.0, 64.0), 16.0, 13.0,
                  [((2, 17.5, 4), _L, -1, 0), ((2, 5, 4), _S, 1, 0), ((8, 5, 4), _R, -1, 0),
                   ((2, 5, 10), _L, -1, 1), ((2, 17.5, 10), _S, 4, 1), ((8, 17.5, 10), _R, -1, 1)],
                  [[(0, 1, 156.25), (1, 2, 36.0)], [(3, 4, 156.25), (4, 5, 36.0)]])


def _second_image():
    """Ly = 16 < 2 r_max = 24: the stone lies 11 above L and its image 5 below, both within r_max: one link, d2 = 25; R is 4
    from the stone along z and linked to L directly at 25 + 16.  Every site is marked once: 3 surface sites"""
    return _exact("second_image", (16.0, 16.0, 64.0), 16.0, 12.0,
                  [((4, 1, 8), _L, -1, 0), ((4, 12, 8), _S, 1, 0), ((4, 12, 12), _R, -1, 0)], [[(0, 1, 25.0), (1, 2, 16.0)]])


def _self_image():
    """Ly = 16 = r_max: a one-site stone (16 from its own image) and a two-site stone whose sites at y = 2 and y = 14 are 4
    apart through the face (and 16 from their own images).  None of that is a link; the chain L - s - {t, u} - R has hops
    of 36, 37 and 36"""
    return _exact("self_image", (16.0, 16.0, 64.0), 16.0, 16.0,
                  [((4, 1, 8), _L, -1, 0), ((4, 1, 14), _S, 1, 0), ((4, 2, 20), _S, 5, 0), ((4, 14, 20), _S, 5, 0),
                   ((4, 14, 26), _R, -1, 0)], [[(0, 1, 36.0), (1, 2, 37.0), (3, 4, 36.0)]])


def _ties_wrap():
    """5 x 16 x 16 sites at 4 A in a period of 64: the plane x = 0 is L, x = 16 is R, every site between its own node;
    r_max = 4: every link has d2 = 16, a sixteenth of those in y or z through the wrap, and the chain is whatever the order
    of the site ids decides"""
    g = np.stack([a.ravel() for a in np.meshgrid(np.arange(5), np.arange(16), np.arange(16), indexing="ij")], axis=1)
    side = np.where(g[:, 0] == 0, _L, np.where(g[:, 0] == 4, _R, 0))
    c = _exact("ties_wrap", L64, 16.0, 4.0, [(tuple(4.0 * p), int(s), 0, 0) for p, s in zip(g, side)], [None], x_hi=16.0,
               shuffle=23)
    N = len(c["xyz"])
    c["node"] = np.where((c["side"] == 0) & (c["cell"] == 0), (np.arange(N) * 7 + 3) % N, -1).astype(np.int32)
    del c["hops"]
    return c


def _two_cells():
    """Ly = 32, cutoff 16: two index cells in y, each next to the other through BOTH faces.  Gap cell 0: L at y = 14, its
    stone at y = 18 through the inner face (y = 16); gap cell 1: L at y = 2, its stone at y = 30 through the outer, wrapped
    face.  Each R is 4 from the stone along x.  Each L has a stone of its own index cell 6 away, and r_max = 12 is below the
    14 that separates each L from the face it does not look through: a bound to the wrong face prunes the hop's cell"""
    return _exact("two_cells", (16.0, 32.0, 64.0), 16.0, 12.0,
                  [((4, 14, 8), _L, -1, 0), ((4, 18, 8), _S, 1, 0), ((8, 18, 8), _R, -1, 0), ((4, 8, 8), _S, 3, 0),
                   ((4, 2, 40), _L, -1, 1), ((4, 30, 40), _S, 5, 1), ((8, 30, 40), _R, -1, 1), ((4, 8, 40), _S, 7, 1)],
                  [[(0, 1, 16.0), (1, 2, 16.0)], [(4, 5, 16.0), (5, 6, 16.0)]])


def _one_cell():
    """Ly = Lz = 16 = cutoff: one index cell in y and in z, next to itself through every face.  L - stone through the y
    face, stone - R through the z face, 2 each; L - R directly through both at 8"""
    return _exact("one_cell", (16.0, 16.0, 16.0), 16.0, 6.0,
                  [((4, 1, 1), _L, -1, 0), ((4, 15, 1), _S, 2, 0), ((4, 15, 15), _R, -1, 0)], [[(0, 1, 4.0), (1, 2, 4.0)]])


def _wrapped_stone():
    """one stone of four sites 2 apart at y = 3, 1, 63, 61: it passes through the y face (the node is given; its home, the
    smallest id, lies below the face).  L is 3 from the site at y = 3, R is 3 from the site at y = 61: the chain enters the
    stone on one side of the face and leaves it on the other"""
    return _exact("wrapped_stone", L64, 16.0, 4.0,
                  [((4, 63, 8), _S, 5, 0), ((4, 6, 8), _L, -1, 0), ((4, 3, 8), _S, 5, 0), ((4, 1, 8), _S, 5, 0),
                   ((4, 61, 8), _S, 5, 0), ((4, 58, 8), _R, -1, 0)], [[(1, 2, 9.0), (4, 5, 9.0)]])


ZIGZAG_STONES = 230


def _zigzag_wrap():
    """Ly = 32 (two index cells), Lz = 16 (one): L, 230 one-site stones and R on a helix -- 2 further in y (mod 32) and a
    quarter further in x per site, every second one half up in z --: 231 hops of d2 = 4 + 1/16 + 1/4 that pass the y face
    14 times; a turn of the helix is 4 along x from the next, r_max = 2.5"""
    k = np.arange(ZIGZAG_STONES + 2)
    pts = np.stack([0.25 * k, (2.0 * k) % 32.0, 4.0 + 0.5 * (k % 2)], axis=1)
    side = np.zeros(len(k), np.int64)
    side[0], side[-1] = _L, _R
    c = _exact("zigzag_wrap", (64.0, 32.0, 16.0), 16.0, 2.5, [(tuple(p), int(s), 0, 0) for p, s in zip(pts, side)], [None],
               x_hi=0.25 * (len(k) + 2), max_hops=16, shuffle=24)
    N = len(c["xyz"])
    c["node"] = np.where((c["side"] == 0) & (c["cell"] == 0), np.arange(N), -1).astype(np.int32)
    c["hops"] = [[(int(c["new_id"][i]), int(c["new_id"][i + 1]), 4.3125) for i in range(ZIGZAG_STONES + 1)]]
    return c


def _interior():
    """`wrap_detour`'s sites around the middle of the period: nothing is near a face, periodic equals open"""
    return _exact("interior", L64, 16.0, 5.0,
                  [((4, 25, 30), _L, -1, 0), ((4, 22, 30), _S, 0, 0), ((4, 22, 33.5), _S, 1, 0), ((4, 19, 33.5), _R, -1, 0),
                   ((4, 36, 30), _L, -1, 0), ((7, 40, 30), _R, -1, 0)],
                  [[(0, 1, 9.0), (1, 2, 12.25), (2, 3, 9.0)]], shuffle=25)


EXACT = {"wrap_ladder": _wrap_ladder, "corner": _corner, "wrap_detour": _wrap_detour, "rim_wrap": _rim_wrap,
         "rim_wrap_below": lambda: _rim_wrap(float(np.nextafter(5.0, 0.0))), "half": _half, "second_image": _second_image,
         "self_image": _self_image, "ties_wrap": _ties_wrap, "two_cells": _two_cells, "one_cell": _one_cell,
         "wrapped_stone": _wrapped_stone, "zigzag_wrap": _zigzag_wrap, "interior": _interior}

R_MAX, R_SMALL = 20.0, 12.0
RANDOM = P.PAIRWISE_CASES                  # p11, p23, p34, p52, lattice_wrap: 1 x 1, 2 x 3, 3 x 4, 5 x 2, 3 x 3 cells in (y, z)
PER_CELL = 12                              # sites per gap cell, about
# name: (seed, reach of the union that forms the bodies, share of the near stone pairs it joins)
BODIES = {"p11": (3001, 4.0, 0.6), "p23": (3002, 4.0, 0.6), "p34": (3003, 4.0, 0.6), "p52": (3011, 4.0, 0.6),
          "lattice_wrap": (3005, 4.0, 0.3)}


def _random(name, r_max):
    """the sites of pbc_ref.pairwise_case(name): 46 % of them stones, 26 % each L and R, about 2 % on both sides; a random
    gap cell each, some ids outside [0, n_cells); the nodes: components of a random share of the stone pairs within 4 A
    under the minimum image, named by their largest site"""
    p = P.pairwise_case(name)
    N, xyz, L = p["N"], p["xyz"], p["L"]
    seed, reach, share = BODIES[name]
    rng = np.random.default_rng(seed)
    n_cells = N // PER_CELL
    side = rng.choice(4, N, p=[.46, .26, .26, .02]).astype(np.int32)
    cell = rng.integers(-1, n_cells + 1, N).astype(np.int32)
    stones = np.flatnonzero(side == 0)
    a, b = near_pairs(xyz, stones, stones, reach, L)
    keep = (a < b) & (d2_exact(xyz, a, b, L) <= reach * reach)
    a, b = a[keep], b[keep]
    take = rng.random(len(a)) < share
    uf = R._Union()
    for u, v in zip(a[take].tolist(), b[take].tolist()):
        uf.union(u, v)
    root = np.array([uf.find(int(s)) for s in stones])
    label = np.zeros(N, np.int64)
    np.maximum.at(label, root, stones)
    node = np.full(N, -1, np.int32)
    node[stones] = label[root]
    return dict(name="%s@%g" % (name, r_max), xyz=xyz, side=side, node=node, cell=cell, n_cells=n_cells, r_max=float(r_max),
                cutoff=P.CUTOFF, L=L, max_hops=8)


SEARCH_CASES = tuple("%s@%g" % (n, r) for n in RANDOM for r in (R_MAX, R_SMALL)) + tuple(EXACT)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in EXACT:
        return EXACT[name]()
    base, r = name.split("@")
    return _random(base, float(r))


@functools.lru_cache(maxsize=None)
def reference(name, periodic=True):
    """site_set_chain() of an input, computed once per process and never modified"""
    c = case(name)
    r = site_set_chain(c["xyz"], c["side"], c["node"], c["r_max"], c["cell"], c["n_cells"], c["max_hops"],
                       L=c["L"] if periodic else None, boruvka=True)
    r["chains"].setflags(write=False)
    r["hops"].setflags(write=False)
    return r
