"""The restatement kmcf_conductive_clusters (csrc/kmcf_clusters.hip) is held to: the definitions of include/kmcfield.h in
plain numpy plus scipy.sparse.csgraph.connected_components, and the graphs the tests run it on.

The reference has no cluster analysis; the rule for which pairs conduct is its high_G rule (populate_T_dist: both sites
metal, or both uncharged vacancies).  tests/test_clusters_ref.py pins this file with answers known by construction;
tests/test_gpu_clusters.py holds the library to it, array_equal on every output."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

from events_graph_ref import ring_list

VACANCY, O_EL = 2, 3
METAL, VAC = 1, 2                       # KMCF_CLUSTER_METAL, KMCF_CLUSTER_VACANCY
TABLE_DTYPE = np.dtype([("root", np.int32), ("kind", np.int32), ("size", np.int32), ("touch", np.int32),
                        ("x_min", np.float64), ("x_max", np.float64)])
STAT_KEYS = ("members", "n_clusters", "n_metal_clusters", "n_vacancy_clusters", "n_bridging", "largest_vacancy",
             "largest_bridging")


def classes(element, charge, metals):
    """0 no member, 1 metal, 2 conductive vacancy"""
    element, charge = np.asarray(element), np.asarray(charge)
    metal = np.isin(element, np.asarray(metals))
    cls = np.where(metal, METAL, 0)
    cls[~metal & (element == VACANCY) & (charge == 0)] = VAC
    return cls


def listed_pairs(neigh):
    """(i, j) of every list entry that names a site: entries outside [0, N) are padding"""
    neigh = np.asarray(neigh)
    N = neigh.shape[0]
    ok = (neigh >= 0) & (neigh < N)
    i = np.broadcast_to(np.arange(N)[:, None], neigh.shape)[ok]
    return i.astype(np.int64), neigh[ok].astype(np.int64)


def clusters(neigh, element, charge, metals, x, NL, NR):
    """(label, table, stats): label[i] = smallest site id of i's cluster (-1: no member); table: TABLE_DTYPE rows sorted by
    root; stats: the integer fields of kmcf_cluster_stats_t without passes and ms."""
    neigh = np.asarray(neigh)
    N = neigh.shape[0]
    x = np.asarray(x, np.float64)
    cls = classes(element, charge, metals)
    i, j = listed_pairs(neigh)
    cond = (cls[i] != 0) & (cls[i] == cls[j])          # an entry in either row is an edge: the graph is undirected
    g = coo_matrix((np.ones(int(cond.sum()), np.int8), (i[cond], j[cond])), shape=(N, N))
    _, comp = connected_components(g, directed=False)
    member = cls != 0
    ids = np.arange(N)
    low = np.full(N, N, np.int64)                       # per component: smallest member id
    np.minimum.at(low, comp[member], ids[member])
    label = np.where(member, low[comp], -1).astype(np.int32)
    roots = np.flatnonzero(label == ids)
    table = np.zeros(len(roots), TABLE_DTYPE)
    table["root"] = roots
    table["kind"] = cls[roots]
    size = np.bincount(label[member], minlength=N)
    table["size"] = size[roots]
    xmin, xmax = np.full(N, np.inf), np.full(N, -np.inf)
    np.minimum.at(xmin, label[member], x[member])
    np.maximum.at(xmax, label[member], x[member])
    table["x_min"], table["x_max"] = xmin[roots], xmax[roots]
    touch = np.zeros(N, np.int32)                       # indexed by root
    metal = cls == METAL
    np.bitwise_or.at(touch, label[metal & (ids < NL)], 1)
    np.bitwise_or.at(touch, label[metal & (ids >= N - NR)], 2)
    for a, b in ((i, j), (j, i)):                       # vacancy a shares an entry with metal b, whichever row holds it
        m = (cls[a] == VAC) & (cls[b] == METAL)
        np.bitwise_or.at(touch, label[a[m]], touch[label[b[m]]])
    table["touch"] = touch[roots]
    vac = table[table["kind"] == VAC]
    bridging = vac[vac["touch"] == 3]
    stats = dict(members=int(member.sum()), n_clusters=len(table), n_metal_clusters=int((table["kind"] == METAL).sum()),
                 n_vacancy_clusters=len(vac), n_bridging=len(bridging),
                 largest_vacancy=int(vac["size"].max()) if len(vac) else 0,
                 largest_bridging=int(bridging["size"].max()) if len(bridging) else 0)
    return label, table, stats


# ---- synthetic graphs ----------------------------------------------------------------------------------------------------

METALS = np.array([5, 6, 8], np.int32)


def draw(N, seed):
    """element, charge, x: about a third of the sites metal, a third vacancies (a third of those charged), the rest oxygen;
    x on both sides of zero"""
    rng = np.random.default_rng(seed)
    u = rng.random(N)
    element = np.full(N, O_EL, np.int32)
    metal = u < 1 / 3
    element[metal] = METALS[rng.integers(0, len(METALS), int(metal.sum()))]
    vac = (u >= 1 / 3) & (u < 2 / 3)
    element[vac] = VACANCY
    charge = np.zeros(N, np.int32)
    charge[vac & (rng.random(N) < 1 / 3)] = 2
    return element, charge, rng.uniform(-25.0, 60.0, N)


def graph(name, neigh, seed, element=None, charge=None, NL=None, NR=None):
    neigh = np.ascontiguousarray(getattr(neigh, "neigh", neigh), np.int32)
    N, nn = neigh.shape
    el, ch, x = draw(N, seed)
    if element is not None:
        el = np.asarray(element, np.int32)
    if charge is not None:
        ch = np.asarray(charge, np.int32)
    return dict(name=name, N=N, nn=nn, neigh=neigh, element=el, charge=ch, metals=METALS, x=x,
                NL=max(N // 10, 1) if NL is None else NL, NR=max(N // 10, 1) if NR is None else NR)


def _path_shuffled():
    N = 1 << 17
    order = np.random.default_rng(17).permutation(N).astype(np.int32)      # order[k]: id of the k-th site along the path
    neigh = np.full((N, 2), -1, np.int32)
    neigh[order[1:], 0] = order[:-1]
    neigh[order[:-1], 1] = order[1:]
    c = graph("path_shuffled", neigh, 18, element=np.full(N, VACANCY), charge=np.zeros(N))
    c["ends"] = (int(order[0]), int(order[-1]))
    return c


ASYM_EDGES = 40


def _asym(one_way=True):
    """local7's list plus one-way entries a -> a + 1000 in the padding column, both ends forced into the same class (every
    a lies below 1100, so no site is an end of two such entries)"""
    base = ring_list(5013, [1, 2, 70], False, 7).neigh
    assert (base[:, 6] == -1).all()
    neigh = base.copy()
    el, ch, _ = draw(5013, 21)
    a_sites = np.random.default_rng(77).choice(np.arange(100, 1100, 5), size=ASYM_EDGES, replace=False)
    for n, a in enumerate(a_sites.tolist()):
        b = a + 1000
        if one_way:
            neigh[a, 6] = b
        el[[a, b]] = VACANCY if n % 2 else METALS[1]
        ch[[a, b]] = 0
    c = graph("asym", neigh, 21, element=el, charge=ch)
    c["one_way"] = [(a, a + 1000) for a in a_sites.tolist()]
    return c


def _junk():
    neigh = ring_list(5013, [1, 2, 70], False, 7).neigh.copy()
    N = neigh.shape[0]
    rng = np.random.default_rng(31)
    rows, cols = rng.integers(0, N, 50), rng.integers(0, 7, 50)
    neigh[rows, cols] = np.resize(np.array([N, N + 7, -5], np.int32), 50)
    return graph("junk", neigh, 3)


BUILDERS = {
    "tiny": lambda: graph("tiny", ring_list(5, [1], False, 2), 4, NL=1, NR=1),
    "none": lambda: graph("none", ring_list(300, [1, 2], False, 4), 5, element=np.full(300, O_EL), charge=np.zeros(300)),
    "one": lambda: graph("one", ring_list(4099, [1], True, 2), 6, element=np.full(4099, METALS[1]), charge=np.zeros(4099)),
    "path_shuffled": _path_shuffled,
    "pairs1": lambda: graph("pairs1", (np.arange(4098, dtype=np.int32) ^ 1)[:, None], 11),
    "nn70": lambda: graph("nn70", ring_list(7001, list(range(1, 36)), False, 70), 10),
    "scatter": lambda: graph("scatter", ring_list(600077, [1] + [24576 * k + 5 for k in range(1, 13)], True, 26), 12),
    "asym": _asym,
    "asym_without": lambda: _asym(one_way=False),
    "junk": _junk,
    "local7": lambda: graph("local7", ring_list(5013, [1, 2, 70], False, 7), 3),
}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def reference(name):
    """clusters() of a synthetic case, computed once per process and never modified"""
    key = ("ref", name)
    if key not in _cache:
        c = case(name)
        label, table, stats = clusters(c["neigh"], c["element"], c["charge"], c["metals"], c["x"], c["NL"], c["NR"])
        label.setflags(write=False)
        table.setflags(write=False)
        _cache[key] = (label, table, stats)
    return _cache[key]


# ---- devices ---------------------------------------------------------------------------------------------------------------

def cell_5nm(km, filament):
    """the uncarved 5 nm cell of the synthetic crossbar: 37 650 sites, contacts 576 + 576"""
    key = ("cell", filament)
    if key not in _cache:
        _cache[key] = km.structure.synth_crossbar_40nm(tiles=1, carve=False, filament=filament)
    return _cache[key]


def slab_sites(label, table, x, half_width=2.0):
    """sites of the (one) bridging filament whose x lies within half_width of the middle of its x range"""
    b = table[(table["kind"] == VAC) & (table["touch"] == 3)]
    assert len(b) == 1
    mid = 0.5 * (b["x_min"][0] + b["x_max"][0])
    return np.flatnonzero((label == b["root"][0]) & (np.abs(np.asarray(x) - mid) <= half_width))
