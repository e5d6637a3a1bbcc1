"""The restatement kmcf_site_set_chain and kmcf_filament_chain (csrc/kmcf_chain.hip) are held to: the definitions of
include/kmcfield.h in plain numpy, with scipy.spatial.cKDTree only proposing candidate pairs, and the synthetic cases the
tests run it on.

Per gap cell: the vertices (L_c, R_c, the nodes whose home lies in the cell) and their sites; candidates are the pairs of
sites of DIFFERENT vertex kinds or different nodes that the tree finds within r_max * (1 + 1e-9) -- pairs inside one
terminal are never links, and an electrode has millions of them; on the candidates the exact arithmetic of the contract,
d2 = (dx*dx + dy*dy) + dz*dz with every operation rounded, the test d2 <= r_max*r_max, lexsort((hi, lo, d2)), the first
pair per vertex pair (the link), plain Kruskal on the links in that order, and the tree path from L_c to R_c.

boruvka_path restates the device's rounds (every component takes its smallest outgoing link; stop when a round takes none
or L and R are joined); tests/test_site_chain_ref.py shows that it returns Kruskal's hop list.  That file pins this one
with answers known by construction; tests/test_gpu_site_chain.py holds the library to it."""
import numpy as np
from scipy.spatial import cKDTree

import site_gap_ref as GR
import site_kernels_ref as SK

CHAIN_DTYPE = np.dtype([("hop_max", np.float64), ("hop_max2", np.float64), ("length", np.float64), ("direct2", np.float64),
                        ("status", np.int32), ("n_hops", np.int32), ("neck_from", np.int32), ("neck_to", np.int32),
                        ("n_stones", np.int32), ("n_stone_sites", np.int32), ("n_left", np.int32),
                        ("n_right", np.int32)])                                # kmcf_chain_t
HOP_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("d2", np.float64)])   # kmcf_hop_t
NONE, OPEN, CHAINED, BRIDGED = 0, 1, 2, 3
STAT_KEYS = ("cells_none", "cells_open", "cells_chained", "cells_bridged", "n_stones", "n_stone_sites", "surface_sites")
EXACT_FIELDS = tuple(n for n in CHAIN_DTYPE.names if n not in ("hop_max", "length"))
V_LEFT, V_RIGHT = -1, -2                                                       # vertex ids of the terminals; a stone's: its node

d2_exact = GR.d2_exact


def vertices(side, node, cell, n_cells):
    """(side & 3, own cell or -1, stone mask, vertex cell or -1 per site)"""
    N = len(side)
    side = np.asarray(side).astype(np.int64) & 3
    node = np.asarray(node).astype(np.int64)
    own = GR.cells_of(cell, n_cells, N)
    stone = (side == 0) & (node >= 0) & (node < N) & (own >= 0)
    home = np.full(N, N, np.int64)
    np.minimum.at(home, node[stone], np.flatnonzero(stone))
    vcell = np.full(N, -1, np.int64)
    term = ((side == 1) | (side == 2)) & (own >= 0)
    vcell[term] = own[term]
    vcell[stone] = own[home[node[stone]]]
    return side, own, stone, vcell


def cross_pairs(xyz, groups, r_max):
    """(a, b) site pairs within r_max * (1 + 1e-9) between different groups, and inside the last group (the stones)"""
    R = r_max * (1 + 1e-9)
    trees = [cKDTree(xyz[g]) if len(g) else None for g in groups]
    a, b = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for p in range(len(groups)):
        for q in range(p + 1, len(groups)):
            if trees[p] is None or trees[q] is None:
                continue
            m = trees[p].sparse_distance_matrix(trees[q], R, output_type="ndarray")
            a.append(groups[p][m["i"]])
            b.append(groups[q][m["j"]])
    if trees[-1] is not None:
        pr = trees[-1].query_pairs(R, output_type="ndarray")
        a.append(groups[-1][pr[:, 0]])
        b.append(groups[-1][pr[:, 1]])
    return np.concatenate(a), np.concatenate(b)


def cell_links(xyz, sites, vid, r_max):
    """The links of one cell: (d2, a, b, va, vb) arrays sorted by key, a < b, one row per linked vertex pair; and the mask
    over `sites` of those with a site of another vertex within r_max.  sites: the cell's member sites, vid: their vertices."""
    groups = [sites[vid == V_LEFT], sites[vid == V_RIGHT], sites[vid >= 0]]
    a, b = cross_pairs(xyz, groups, r_max)
    vertex = np.zeros(len(xyz), np.int64)
    vertex[sites] = vid
    va, vb = vertex[a], vertex[b]
    d2 = d2_exact(xyz, a, b)
    ok = (d2 <= r_max * r_max) & (va != vb)
    a, b, va, vb, d2 = a[ok], b[ok], va[ok], vb[ok], d2[ok]
    surface = np.isin(sites, np.concatenate([a, b]))
    swap = a > b
    a, b, va, vb = np.where(swap, b, a), np.where(swap, a, b), np.where(swap, vb, va), np.where(swap, va, vb)
    o = np.lexsort((b, a, d2))
    a, b, va, vb, d2 = a[o], b[o], va[o], vb[o], d2[o]
    lo, hi = np.minimum(va, vb) + 2, np.maximum(va, vb) + 2                    # (>= 0)
    _, first = np.unique(lo * (len(xyz) + 2) + hi, return_index=True)          # the smallest key per vertex pair
    first.sort()
    return (d2[first], a[first], b[first], va[first], vb[first]), surface


class _Union:
    def __init__(self):
        self.p = {}

    def find(self, x):
        p = self.p
        p.setdefault(x, x)
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.p[max(a, b)] = min(a, b)
        return True


def tree_path(edges, src, dst):
    """hops [(from, to, d2)] from src to dst in the forest `edges` [(d2, a, b, va, vb)], or None"""
    adj = {}
    for d2, a, b, va, vb in edges:
        adj.setdefault(va, []).append((vb, a, b, d2))
        adj.setdefault(vb, []).append((va, b, a, d2))
    prev, stack = {src: None}, [src]
    while stack:
        v = stack.pop()
        for w, a, b, d2 in adj.get(v, []):
            if w not in prev:
                prev[w] = (v, a, b, d2)
                stack.append(w)
    if dst not in prev:
        return None
    hops, v = [], dst
    while prev[v] is not None:
        u, a, b, d2 = prev[v]
        hops.append((a, b, d2))
        v = u
    return hops[::-1]


def _rows(links):
    return [(float(d), int(a), int(b), int(va), int(vb)) for d, a, b, va, vb in zip(*links)]


def kruskal_path(links, src=V_LEFT, dst=V_RIGHT):
    uf, edges = _Union(), []
    for row in _rows(links):
        if uf.union(row[3], row[4]):
            edges.append(row)
            if uf.find(src) == uf.find(dst):
                break
    return tree_path(edges, src, dst)


def boruvka_path(links, src=V_LEFT, dst=V_RIGHT, max_rounds=40):
    """(hops or None, rounds): the device's rounds on the sorted links"""
    rows, uf, edges, rounds = _rows(links), _Union(), set(), 0
    while rounds < max_rounds:
        rounds += 1
        best = {}
        for k, row in enumerate(rows):                                         # sorted: the first seen per component is its minimum
            ca, cb = uf.find(row[3]), uf.find(row[4])
            if ca != cb:
                best.setdefault(ca, k)
                best.setdefault(cb, k)
        if not best:
            break
        for k in set(best.values()):
            uf.union(rows[k][3], rows[k][4])
            edges.add(rows[k])
        if uf.find(src) == uf.find(dst):
            break
    return tree_path(sorted(edges), src, dst), rounds


def site_set_chain(xyz, side, node, r_max, cell=None, n_cells=1, max_hops=0, boruvka=False):
    """dict(chains: CHAIN_DTYPE records, hops: HOP_DTYPE (n_cells, max_hops), paths: the full hop list per cell (None: no
    chain), stats: the integer fields of kmcf_chain_stats_t the input decides, rounds: per searched cell with boruvka)"""
    xyz = np.asarray(xyz, np.float64)
    r_max = float(r_max)
    N = len(xyz)
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
    homes = np.unique(node[stone], return_index=True)[1]                       # first (smallest) stone site per node
    chains["n_stones"] = np.bincount(vcell[np.flatnonzero(stone)[homes]], minlength=n_cells)
    chains["hop_max"] = chains["hop_max2"] = chains["direct2"] = np.inf
    chains["neck_from"] = chains["neck_to"] = -1
    member = np.flatnonzero(vcell >= 0)
    order = member[np.argsort(vcell[member], kind="stable")]
    bounds = np.searchsorted(vcell[order], np.arange(n_cells + 1))
    paths, rounds, surface_sites = [None] * n_cells, [], 0
    for c in range(n_cells):
        r = chains[c]
        if n_both[c] > 0:
            r["status"], r["hop_max"], r["hop_max2"], r["direct2"] = BRIDGED, 0.0, 0.0, 0.0
            continue
        if r["n_left"] == 0 or r["n_right"] == 0:
            r["status"] = NONE
            continue
        sites = order[bounds[c]:bounds[c + 1]]
        vid = np.where(stone[sites], node[sites], np.where(side[sites] == 1, V_LEFT, V_RIGHT))
        links, surface = cell_links(xyz, sites, vid, r_max)
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
            r["status"] = OPEN
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
    return dict(chains=chains, hops=hops, paths=paths, stats=stats, rounds=rounds)


def sides_and_nodes(neigh, element, charge, metals, x, NL, NR):
    """(side, node) of kmcf_filament_chain: the touch of the site's cluster; its label where that cluster floats"""
    side, cls = GR.sides(neigh, element, charge, metals, x, NL, NR)
    label = GR.CR.clusters(neigh, element, charge, metals, x, NL, NR)[0]
    node = np.where((cls != 0) & (side == 0), label, -1).astype(np.int32)
    return side, node


# ---- synthetic cases ---------------------------------------------------------------------------------------------------------
# Each: dict(name, xyz, side, node, cell (or None), n_cells, r_max, cutoff = edge of the index cells, max_hops) and what is
# known about it.

def _case(name, pts, side, node, r_max, cutoff, cell=None, n_cells=1, max_hops=8, **known):
    return dict(name=name, xyz=np.array(pts, np.float64), side=np.array(side, np.int32), node=np.array(node, np.int32),
                cell=None if cell is None else np.array(cell, np.int32), n_cells=n_cells, r_max=float(r_max),
                cutoff=float(cutoff), max_hops=max_hops, **known)


def _shuffled(c, seed, keep_first=0):
    """the same case with the site ids permuted (the first keep_first keep theirs); c["new_id"][old] = new"""
    N = len(c["xyz"])
    perm = np.concatenate([np.arange(keep_first), keep_first + np.random.default_rng(seed).permutation(N - keep_first)])
    for k in ("xyz", "side", "node", "cell"):                                  # new id k holds old site perm[k]
        if c[k] is not None:
            c[k] = np.ascontiguousarray(c[k][perm])
    c["new_id"] = np.argsort(perm)
    return c


def _renamed(c, hops):
    return [(int(c["new_id"][a]), int(c["new_id"][b]), d2) for a, b, d2 in hops]


def _ladder():
    """one L site, stones at x = 3, 6, 9, one R site at x = 12; decoy stones farther than r_max from everything"""
    pts = [[0, 0, 0], [3, 0, 0], [6, 0, 0], [9, 0, 0], [12, 0, 0], [3, 4.5, 0], [6, -5, 0], [9, 0, 6], [17, 0, 0], [-5, 0, 0]]
    side = [1, 0, 0, 0, 2] + [0] * 5
    node = [-1, 7, 3, 9, -1, 1, 2, 4, 5, 6]                                      # labels are arbitrary values in [0, N)
    c = _case("ladder", pts, side, node, 4.0, 4.0)
    c = _shuffled(c, 11)
    c["hops"] = _renamed(c, [(0, 1, 9.0), (1, 2, 9.0), (2, 3, 9.0), (3, 4, 9.0)])
    return c


def _detour_points(last):
    """l0 - s1 - s2 - r0 with hops 3, 3.5 and |last|; a second pair l1, r1"""
    s2 = np.array([3.0, 3.5, 0.0])
    return [[0, 0, 0], [3, 0, 0], s2, s2 + np.array(last, np.float64), [40, 0, 0]]


def _detour():
    """the direct link l1 - r1 at exactly 5.0 = r_max (3, 4, 0), and the path l0 - s1 - s2 - r0 with hops 3, 3.5, 3: the
    chain takes the stones, hop_max2 = 12.25, direct2 = 25"""
    pts = _detour_points([3, 0, 0]) + [[43, 4, 0]]
    c = _case("detour", pts, [1, 0, 0, 2, 1, 2], [-1, 0, 1, -1, -1, -1], 5.0, 5.0)
    c = _shuffled(c, 12)
    c["hops"] = _renamed(c, [(0, 1, 9.0), (1, 2, 12.25), (2, 3, 9.0)])
    return c


def _rim(r_max):
    """`detour` without a direct link (l1 - r1 are 6 apart) and the last stone hop s2 - r0 at exactly 5.0 (3, 4, 0); index
    cells of 15 with more stones inside the 27 cells, farther than 5 from everything.  r_max = 5: CHAINED, 3 hops,
    hop_max2 = 25.  r_max just below 5: that hop is no link and nothing replaces it: OPEN."""
    pts = _detour_points([3, 4, 0]) + [[46, 0, 0], [20, 20, 20], [-6, 0, 0], [3, -9, 2], [12, 14, 3], [6, 7.5, 13]]
    side = [1, 0, 0, 2, 1, 2] + [0] * 5
    node = [-1, 0, 1, -1, -1, -1, 2, 3, 4, 5, 6]
    c = _case("rim" if r_max == 5.0 else "rim_below", pts, side, node, r_max, 15.0)
    c["hops"] = [(0, 1, 9.0), (1, 2, 12.25), (2, 3, 25.0)] if r_max == 5.0 else None
    return c


def _ties():
    """integer lattice 6 x 6 x 6, the plane x = 0 is L, x = 5 is R, every interior site its own node; r_max = 1: every link
    has d2 = 1 and the chain is whatever the order of the site ids decides"""
    g = np.stack([a.ravel() for a in np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")], axis=1)
    side = np.where(g[:, 0] == 0, 1, np.where(g[:, 0] == 5, 2, 0))
    c = _case("ties", g.astype(np.float64), side, np.zeros(216), 1.0, 2.0)
    c = _shuffled(c, 13)
    c["node"] = np.where(c["side"] == 0, (np.arange(216) * 7 + 3) % 216, -1).astype(np.int32)   # a permutation: own nodes
    return c


def _straddle():
    """27 gap cells, one per relation of two index cells (GR.RELATIONS): a (L) lies a quarter from the faces of its index
    cell, the stone m and b (R) in the index cell at that offset: the hop a - m crosses the relation (a finds m through it,
    m finds a through the opposite one), the hop m - b lies inside one cell; decoys of each kind lie farther off"""
    edge = 5.0
    pts, side, node, cell, hops = [], [], [], [], []
    for g, s in enumerate(GR.RELATIONS):
        s = np.array(s, np.float64) if any(s) else np.array([0.2, 0, 0])         # (same cell: a small step along x)
        o = edge * np.array([4 * g + 1, 1, 1], np.float64)
        a = o + 2.5 + 2.25 * np.array(GR.RELATIONS[g], np.float64)
        m, b = a + 0.4 * s, a + 0.8 * s
        k = len(pts)
        pts += [a, m, b, a - 1.0 * s, a + 2.0 * s, a + 1.5 * s]                  # ..., a decoy L, R and stone
        side += [1, 0, 2, 1, 2, 0]
        node += [-1, k + 1, -1, -1, -1, k + 5]
        cell += [g] * 6
        hops.append([(k, k + 1), (k + 1, k + 2)])
    pts += [np.zeros(3), edge * np.array([4 * 27, 3, 3], np.float64) - 0.5]     # the corners of the index
    side += [0, 0]
    node += [-1, -1]
    cell += [-1, -1]
    c = _case("straddle", pts, side, node, 5.0, edge, cell=cell, n_cells=27)
    xyz = c["xyz"]
    hops = [[(a, b, float(d2_exact(xyz, a, b))) for a, b in h] for h in hops]
    c = _shuffled(c, 14)
    c["node"] = np.where(c["node"] >= 0, c["new_id"][np.maximum(c["node"], 0)], -1).astype(np.int32)
    c["hops"] = [_renamed(c, h) for h in hops]
    return c


def _home(flipped):
    """two gap cells (y = 0 and y = 10), each an L site at x = 0 and an R site at x = 8, r_max = 4.5; ONE node with a stone
    site at x = 4 in each: it serves the cell of its smaller site id -- cell 0, or cell 1 once the two ids are swapped"""
    pts = [[4, 0, 0], [4, 10, 0], [0, 0, 0], [8, 0, 0], [0, 10, 0], [8, 10, 0]]
    if flipped:
        pts[0], pts[1] = pts[1], pts[0]
    cell = [1, 0, 0, 0, 1, 1] if flipped else [0, 1, 0, 0, 1, 1]
    c = _case("home_flipped" if flipped else "home", pts, [0, 0, 1, 2, 1, 2], [5, 5, -1, -1, -1, -1], 4.5, 5.0, cell=cell,
              n_cells=2)
    c["hops"] = [None, [(4, 0, 16.0), (0, 5, 16.0)]] if flipped else [[(2, 0, 16.0), (0, 3, 16.0)], None]
    return c


def _multi_site():
    """a row of 12 snake-shaped stones of 2 - 40 sites between an L and an R plate; consecutive stones approach each other
    at their ENDS (2.5 apart), and the smallest id of every stone is its middle site (ids 0 .. 11): the link of two stones
    is a minimum over members that are not the vertices' names"""
    rng = np.random.default_rng(15)
    sizes = [2, 40, 3, 17, 33, 5, 40, 2, 9, 26, 12, 7]
    stones, x = [], 2.5
    for n in sizes:
        k = np.arange(n)
        stones.append(np.stack([x + 1.0 * k, 0.6 * np.sin(0.9 * k), 0.5 * (k % 2)], axis=1))
        x += 1.0 * (n - 1) + 2.5
    plate = np.array([[0.0, y, z] for y in (-1.0, 0.0, 1.0) for z in (-1.0, 0.0, 1.0)])
    right = plate + np.array([x, 0.0, 0.0])
    middle = [s[len(s) // 2] for s in stones]
    rest = [np.delete(s, len(s) // 2, axis=0) for s in stones]
    label = (np.arange(len(sizes)) * 5 + 40)                                    # node labels: any values in [0, N)
    pts = np.concatenate([np.array(middle)] + rest + [plate, right])
    node = np.concatenate([label] + [np.full(len(r), l) for r, l in zip(rest, label)] + [np.full(18, -1)])
    side = np.concatenate([np.zeros(len(pts) - 18), np.full(9, 1), np.full(9, 2)])
    c = _case("multi_site", pts, side, node, 3.0, 4.0, max_hops=16)
    return _shuffled(c, 16, keep_first=len(sizes))


def _zigzag():
    """600 one-site stones 2 apart along x, every second one 0.7 up: 601 hops, the first of d2 = 4, the others 4 + 0.49"""
    n = 600
    xs = 2.0 * np.arange(1, n + 1)
    pts = np.concatenate([[[0.0, 0, 0]], np.stack([xs, 0.7 * (np.arange(n) % 2), np.zeros(n)], axis=1), [[2.0 * (n + 1), 0, 0]]])
    side = np.zeros(n + 2)
    side[0], side[-1] = 1, 2
    c = _case("zigzag", pts, side, np.zeros(n + 2), 2.5, 2.5, max_hops=16)
    c = _shuffled(c, 3)
    c["node"] = np.where(c["side"] == 0, np.arange(n + 2), -1).astype(np.int32)
    return c


def _statuses():
    """six gap cells 20 apart in y, r_max = 4: 0 NONE (no R site), 1 OPEN (a stone at x = 3 only; what would close the chain
    is a stone in no cell, a site whose node lies outside [0, N) and an R site in no cell), 2 CHAINED (stones at 3 and 6),
    3 BRIDGED (a site on both sides), 4 NONE (stones only), 5 CHAINED by its direct link; sides carry bits above 1"""
    rows = [  # x, region (y = 20 * region), gap cell, side, node
        (0, 0, 0, 1, -1), (3, 0, 0, 0, 1),
        (0, 1, 1, 1 | 4, -1), (3, 1, 1, 12, 2), (9, 1, 1, 2 | 8, -1), (6, 1, 1, 0, -5), (6.2, 1, 1, 0, 1000), (6.1, 1, -1, 0, 3),
        (6.3, 1, 9, 16, 4), (5.9, 1, 6, 2, -1), (5.8, 1, -2, 2, -1),
        (0, 2, 2, 1, -1), (3, 2, 2, 8, 12), (6, 2, 2, 0, 13), (9, 2, 2, 2, -1),
        (0, 3, 3, 1, -1), (3, 3, 3, 3, -1), (6, 3, 3, 0, 16), (9, 3, 3, 2, -1),
        (3, 4, 4, 0, 19), (6, 4, 4, 0, 19),
        (0, 5, 5, 1, -1), (3.5, 5, 5, 2 | 32, -1),
    ]
    pts = [[r[0], 20.0 * r[1], 0.0] for r in rows]
    c = _case("statuses", pts, [r[3] for r in rows], [r[4] for r in rows], 4.0, 5.0, cell=[r[2] for r in rows], n_cells=6)
    c["status"] = [NONE, OPEN, CHAINED, BRIDGED, NONE, CHAINED]
    c["n_hops"] = [0, 0, 3, 0, 0, 1]
    return c


def _mixed():
    """20 000 random points in a box of 40, 8 x 8 gap cells over y - z, L: x < 4, R: x > 36, 0.05 % of the sites on both
    sides, 60 % of the sites with a random node in [0, N / 2) -- a node's sites lie anywhere, most of them outside the gap
    cell of its home --, 3 % of the sites in no cell"""
    rng = np.random.default_rng(2025)
    N, n_cells, box = 20000, 64, 40.0
    xyz = rng.uniform(0.0, box, (N, 3))
    cy, cz = (np.minimum((xyz[:, k] / box * 8).astype(np.int64), 7) for k in (1, 2))
    cell = (cy * 8 + cz).astype(np.int32)
    side = np.zeros(N, np.int32)
    side[xyz[:, 0] < 4.0] = 1
    side[xyz[:, 0] > 36.0] = 2
    side[rng.random(N) > 0.9995] = 3
    node = np.where(rng.random(N) < 0.6, rng.integers(0, N // 2, N), -1).astype(np.int32)
    junk = rng.random(N) < 0.03
    cell[junk] = np.resize(np.array([-1, n_cells, -7], np.int32), int(junk.sum()))
    return dict(name="mixed", xyz=xyz, side=side, node=node, cell=cell, n_cells=n_cells, r_max=2.4, cutoff=5.0, max_hops=8)


def _large():
    """The 83 x 81 x 80 jittered lattice of the pairwise tests (537 840 sites, 263 scan tiles, index cells of 20 A) with
    members only at the two ends of the cell order, as GR's `large_two`: gap cell 0 = the positions below 256 tiles (its
    members: 48 positions of the first tile), gap cell 1 = the positions from 256 tiles on (a third of them members: L, R
    and stones of 50 nodes).  In each cell a chain a - m1 - m2 - b is planted with hops of 0.3 A, shorter than two lattice
    sites can be apart (4 - 0.6 A): the cell's chain by construction.  Both member lists (all members, surface members)
    depend on what the scan carries from its first pass of 256 tiles into its second."""
    T = SK.SCAN_TILE
    xyz = SK.pairwise_case("large")["xyz"].copy()
    base = dict(xyz=xyz, cutoff=SK.CUTOFF)
    at = np.argsort(GR.index_positions(base))                                   # site at every position
    plant = [[int(at[p + k]) for k in range(4)] for p in (1010, 256 * T + 2)]
    for a, m1, m2, b in plant:
        for k, s in enumerate((m1, m2, b)):
            xyz[s] = xyz[a] + np.array([0.3 * (k + 1), 0.0, 0.0])
    pos = GR.index_positions(base)                                             # (of the final coordinates)
    rng = np.random.default_rng(265)
    N = len(xyz)
    side, node = np.zeros(N, np.int32), np.full(N, -1, np.int32)
    first, tail = np.flatnonzero((pos >= 1000) & (pos < 1048)), np.flatnonzero(pos >= 256 * T)
    for idx, p in ((first, [0.25, 0.25, 0.25, 0.25]), (tail, [0.7, 0.1, 0.1, 0.1])):
        kind = rng.choice(4, len(idx), p=p)                                    # none, L, R, stone
        side[idx] = np.where(kind == 3, 0, kind)
        stones = idx[kind == 3]
        node[stones] = rng.integers(0, 50, len(stones)) + (100 if idx is tail else 0)
    for k, (a, m1, m2, b) in enumerate(plant):
        side[[a, m1, m2, b]] = [1, 0, 0, 2]
        node[[a, m1, m2, b]] = [-1, 200 + 2 * k, 201 + 2 * k, -1]
    hops = [[(p[k], p[k + 1], float(d2_exact(xyz, p[k], p[k + 1]))) for k in range(3)] for p in plant]
    return dict(name="large", xyz=xyz, side=side, node=node, cell=(pos >= 256 * T).astype(np.int32), n_cells=2,
                r_max=SK.CUTOFF, cutoff=SK.CUTOFF, max_hops=4, hops=hops)


def _tile_edge(N):
    """SK.tile_edge_sites(N) (N = 2047, 2048, 2049: a scan tile one item short, exactly full, one item over), one gap cell, a
    random quarter of the sites each L, R, stone (50 nodes), none, and r_max = 0.5 A: no two lattice sites are that close
    (4 - 0.6 A).  The stone s is the site at the LAST position of the index's cell order; the two sites before it become an
    L site l at 0.4 A from s in x and an R site r at 0.4 A from s in y, both towards the lower corner, 0.57 A apart: the only
    links are l - s and s - r, the only chain is l - s - r, and it is lost if the last item of the scan is."""
    xyz, order = SK.tile_edge_sites(N)
    xyz = xyz.copy()
    l, r, s = (int(v) for v in order[-3:])
    xyz[l] = xyz[s] - np.array([0.4, 0.0, 0.0])
    xyz[r] = xyz[s] - np.array([0.0, 0.4, 0.0])
    assert GR.index_positions(dict(xyz=xyz, cutoff=SK.CUTOFF))[s] == N - 1     # (of the final coordinates)
    rng = np.random.default_rng(280 + N)
    kind = rng.choice(4, N)                                                    # none, L, R, stone
    side = np.where(kind == 3, 0, kind).astype(np.int32)
    node = np.where(kind == 3, rng.integers(0, 50, N), -1).astype(np.int32)
    side[[l, s, r]] = [1, 0, 2]
    node[[l, s, r]] = [-1, 200, -1]
    hops = [(l, s, float(d2_exact(xyz, l, s))), (s, r, float(d2_exact(xyz, s, r)))]
    return dict(name="tile_edge@%d" % N, xyz=xyz, side=side, node=node, cell=None, n_cells=1, r_max=0.5, cutoff=SK.CUTOFF,
                max_hops=4, hops=hops)


BUILDERS = {"ladder": _ladder, "detour": _detour, "rim": lambda: _rim(5.0),
            "rim_below": lambda: _rim(float(np.nextafter(5.0, 0.0))), "ties": _ties, "straddle": _straddle,
            "home": lambda: _home(False), "home_flipped": lambda: _home(True), "multi_site": _multi_site, "zigzag": _zigzag,
            "statuses": _statuses, "mixed": _mixed, "large": _large,
            **{"tile_edge@%d" % n: (lambda n=n: _tile_edge(n)) for n in SK.TILE_EDGE_SIZES}}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def reference(name):
    """site_set_chain() of a synthetic case, computed once per process and never modified"""
    key = ("ref", name)
    if key not in _cache:
        c = case(name)
        r = site_set_chain(c["xyz"], c["side"], c["node"], c["r_max"], c["cell"], c["n_cells"], c["max_hops"], boruvka=True)
        r["chains"].setflags(write=False)
        r["hops"].setflags(write=False)
        _cache[key] = r
    return _cache[key]
