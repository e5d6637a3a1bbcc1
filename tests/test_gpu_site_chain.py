"""GPU: kmcf_site_set_chain and kmcf_filament_chain (csrc/kmcf_chain.hip) against the restatement of tests/site_chain_ref.py:
array_equal on every integer of every record, on hop_max2, direct2 and the hops; hop_max and length within an ulp per
term; the stats the input decides; the same bytes from a second call and from calls without stats or hop list.
Synthetic site sets (tests/test_site_chain_ref.py shows that they are what their names say); the 5 nm cell with a filament,
with it cut narrowly -- and one vacancy put into the cut --, cut widely, without one; a 2 x 2 crossbar; the argument checks."""
import ctypes as C
import time

import numpy as np
import pytest
from scipy.spatial import cKDTree

import clusters_ref as CR
import site_chain_ref as R
from test_gpu_site_gap import R_MAX, _Device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comm(km):
    c = km.solvers.KMC_comm(1, 2, 1, 1)
    c.connect()
    yield c
    c.close()


def _same(got, ref):
    chains, hops, st = got["chains"], got["hops"], got["stats"]
    print({k: st[k] for k in st if not k.startswith("ms_")}, "clusters %.3f ms, search %.3f ms" % (st["ms_clusters"], st["ms_search"]))
    for k in R.STAT_KEYS:
        assert st[k] == ref["stats"][k], (k, st[k], ref["stats"][k])
    for f in R.EXACT_FIELDS:
        assert np.array_equal(chains[f], ref["chains"][f]), (f, np.flatnonzero(chains[f] != ref["chains"][f])[:8])
    if hops is not None:
        for f in R.HOP_DTYPE.names:
            assert np.array_equal(hops[f], ref["hops"][f]), (f, np.argwhere(hops[f] != ref["hops"][f])[:8])
    # hop_max = sqrt(hop_max2): one rounding on either side.  length: n sqrt terms, each within an ulp of the reference's
    # and none larger than the sum, and n - 1 additions in the same order whose roundings can then differ by an ulp of
    # the sum each: 2 n ulp(length) bounds the difference.
    root = np.sqrt(ref["chains"]["hop_max2"])
    fin = np.isfinite(root)
    assert np.array_equal(np.isfinite(chains["hop_max"]), fin) and (chains["hop_max"][~fin] == np.inf).all()
    assert (np.abs(chains["hop_max"][fin] - root[fin]) <= np.spacing(root[fin])).all()
    want = ref["chains"]["length"]
    assert (np.abs(chains["length"] - want) <= 2 * ref["chains"]["n_hops"] * np.spacing(want)).all()
    total = int(ref["chains"]["n_hops"].sum())
    assert total <= st["forest_edges"] <= max(st["n_stones"] + 2 * len(chains) - 1, 0) and 1 <= st["rounds"] <= 40


class _Index:
    """a spatial index over a case's coordinates, with the case's cell edge"""

    def __init__(self, km, comm, c, lattice=None):
        import torch
        self.km, self.c = km, c
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        self.i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (f64(c["xyz"][:, k]) for k in range(3))
        self.side, self.node = self.i32(c["side"]), self.i32(c["node"])
        self.cell = self.i32(c["cell"]) if c["cell"] is not None else None
        self.handle = C.c_void_p()
        p, lib = km.solvers._ptr, km.lib.load()
        if lattice is None:
            km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                      float(c["cutoff"]), C.byref(self.handle)), "kmcf_compute_cutoff_list")
        else:
            lat = np.ascontiguousarray(lattice, np.float64)
            km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                          float(c["cutoff"]), lat.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                                          C.byref(self.handle)), "kmcf_compute_cutoff_list_pbc")

    def raw(self, **over):
        """the C entry itself with single arguments replaced: (rc, records, hops, stats)"""
        km, c, p = self.km, self.c, self.km.solvers._ptr
        max_hops = over.get("max_hops", c["max_hops"])
        n_cells = over.get("n_cells", c["n_cells"])
        chains = np.zeros(max(n_cells, 1), km.solvers.CHAIN_DTYPE)
        hops = np.zeros((max(n_cells, 1), max(max_hops, 1)), km.solvers.HOP_DTYPE)
        st = km.lib.ChainStats()
        a = dict(p=self.handle, x=p(self.x), y=p(self.y), z=p(self.z), side=p(self.side), node=p(self.node),
                 r_max=float(c["r_max"]), cell=p(self.cell), n_cells=n_cells,
                 chains=chains.ctypes.data_as(C.POINTER(km.lib.Chain)),
                 hops=hops.ctypes.data_as(C.POINTER(km.lib.Hop)) if max_hops > 0 else None, max_hops=max_hops, stats=C.byref(st))
        a.update(over)
        rc = km.lib.load().kmcf_site_set_chain(a["p"], a["x"], a["y"], a["z"], a["side"], a["node"], a["r_max"], a["cell"],
                                               a["n_cells"], a["chains"], a["hops"], a["max_hops"], a["stats"])
        return rc, chains, (hops if max_hops > 0 else None), st.as_dict()

    def chain(self, **over):
        rc, chains, hops, st = self.raw(**over)
        self.km.lib.check(rc, "kmcf_site_set_chain")
        return dict(chains=chains, hops=hops, stats=st)

    def refused(self, match, **over):
        rc = self.raw(**over)[0]
        msg = self.km.lib.load().kmcf_last_error().decode()
        assert rc == -1 and match in msg, (rc, msg)

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


CASES = ["ladder", "detour", "rim", "rim_below", "ties", "straddle", "home", "home_flipped", "multi_site", "zigzag", "statuses",
         "mixed", "large", "tile_edge@2047", "tile_edge@2048", "tile_edge@2049"]


@pytest.mark.parametrize("name", CASES)
def test_site_sets_match_the_restatement(km, comm, name):
    c, ref = R.case(name), R.reference(name)
    ix = _Index(km, comm, c)
    try:
        got = ix.chain()
        _same(got, ref)
        again = ix.chain()                                           # scratch reused: the same bytes
        assert got["chains"].tobytes() == again["chains"].tobytes() and got["hops"].tobytes() == again["hops"].tobytes()
        assert {k: v for k, v in got["stats"].items() if not k.startswith("ms_")} == \
               {k: v for k, v in again["stats"].items() if not k.startswith("ms_")}
        assert ix.chain(stats=None)["chains"].tobytes() == got["chains"].tobytes()
        assert ix.chain(max_hops=0)["chains"].tobytes() == got["chains"].tobytes()
        assert ix.chain(max_hops=0, stats=None)["chains"].tobytes() == got["chains"].tobytes()
        if name == "zigzag":
            assert got["stats"]["rounds"] >= 4 and got["chains"][0]["n_hops"] == 601 and got["hops"].shape == (1, 16)
        if name == "rim":                                           # ... and the same index with r_max just below the last hop
            _same(ix.chain(r_max=R.case("rim_below")["r_max"]), R.reference("rim_below"))
        if name == "detour":                                        # no node at all: the chain is the direct link
            none = ix.i32(np.full(len(c["xyz"]), -1))
            alone = ix.chain(node=ix.km.solvers._ptr(none))
            assert alone["chains"][0]["n_hops"] == 1 and alone["chains"][0]["hop_max2"] == 25.0 == alone["chains"][0]["direct2"]
    finally:
        ix.close()


def test_arguments_are_checked(km, comm):
    ix = _Index(km, comm, R.case("rim"))
    try:
        for k in ("x", "y", "z", "side", "node", "chains", "p"):
            ix.refused({"x": "d_x", "y": "d_y", "z": "d_z", "side": "d_site_side", "node": "d_site_node", "chains": "h_chains",
                        "p": "p is NULL"}[k], **{k: None})
        for bad in (float("nan"), float("inf"), 0.0, -1.0):
            ix.refused("r_max", r_max=bad)
        ix.refused("cutoff", r_max=float(np.nextafter(15.0, 16.0)))
        ix.refused("n_cells", n_cells=0)
        ix.refused("d_site_cell is NULL", n_cells=2)
        ix.refused("max_hops", max_hops=-1)
        ix.refused("h_hops is set", max_hops=0, hops=np.zeros(1, km.solvers.HOP_DTYPE).ctypes.data_as(C.POINTER(km.lib.Hop)))
        ix.refused("h_hops is NULL", hops=None)
        _same(ix.chain(r_max=15.0), R.site_set_chain(ix.c["xyz"], ix.c["side"], ix.c["node"], 15.0, max_hops=ix.c["max_hops"]))
    finally:
        ix.close()
    per = _Index(km, comm, R.case("rim"), lattice=[100.0, 100.0, 100.0])
    try:
        per.refused("periodic")
    finally:
        per.close()


# ---- the full call on devices ------------------------------------------------------------------------------------------------------

MAX_HOPS = 12


def _chain(dv, r_max=R_MAX, **kw):
    NL = dv.d["N_contact"]
    return dv.S.filament_chain(dv.comm, dv.buf, NL, NL, r_max, site_cell=dv.cell, n_cells=dv.n_cells, max_hops=MAX_HOPS, **kw)


def _restated(dv):
    d, NL = dv.d, dv.d["N_contact"]
    t = time.time()
    side, node = R.sides_and_nodes(dv.neigh, dv.buf.site_element.cpu().numpy(), dv.buf.site_charge.cpu().numpy(), d["metals"],
                                   d["xyz"][:, 0], NL, NL)
    ref = R.site_set_chain(d["xyz"], side, node, R_MAX, dv.cell, dv.n_cells, MAX_HOPS)
    print("restatement %.2f s" % (time.time() - t))
    return side, node, ref


def _check(dv):
    """the record against the restatement, and the relations to the gap on the same state"""
    got = _chain(dv)
    side, node, ref = _restated(dv)
    _same(got, ref)
    assert np.array_equal(got["side"].cpu().numpy(), side) and np.array_equal(got["node"].cpu().numpy(), node)
    gap = dv.run()["gaps"]
    ch = got["chains"]
    assert np.array_equal(ch["direct2"], gap["gap2"]) and (ch["hop_max2"] <= ch["direct2"]).all()
    assert np.array_equal(ch["n_left"], gap["n_left"]) and np.array_equal(ch["n_right"], gap["n_right"])
    assert np.array_equal(ch["status"] == R.BRIDGED, gap["bridged"] != 0)
    # no stones: one hop, the gap itself, wherever the gap found a pair between two different sites
    alone = dv.S.site_set_chain(dv.buf, got["side"], got["node"] * 0 - 1, R_MAX, site_cell=dv.cell, n_cells=dv.n_cells)["chains"]
    found = (gap["site_left"] >= 0) & (gap["bridged"] == 0)
    assert (alone["n_hops"][found] == 1).all() and np.array_equal(alone["hop_max2"][found], gap["gap2"][found])
    assert (alone["status"][~found & (gap["bridged"] == 0)] <= R.OPEN).all() and (alone["n_stones"] == 0).all()
    # the primitive on the sides and nodes the full call wrote: the same records
    again = dv.S.site_set_chain(dv.buf, got["side"], got["node"], R_MAX, site_cell=dv.cell, n_cells=dv.n_cells, max_hops=MAX_HOPS)
    assert again["chains"].tobytes() == ch.tobytes() and again["hops"].tobytes() == got["hops"].tobytes()
    return got, side


@pytest.fixture(scope="module")
def cell5(km):
    dv = _Device(km, CR.cell_5nm(km, 4.0))
    yield dv
    dv.close()


def test_cell_with_a_filament_is_bridged(cell5):
    cell5.buf.site_charge.copy_(cell5.charge0)
    got, _ = _check(cell5)
    r = got["chains"][0]
    assert (r["status"], r["n_hops"], r["hop_max2"], r["direct2"], r["n_left"], r["n_right"]) == (R.BRIDGED, 0, 0.0, 0.0, 5930, 8094)
    assert got["stats"]["cells_bridged"] == 1 and (got["hops"]["from"] == -1).all()


def stone_for_the_cut(d, neigh, cls, side, gap2):
    """a site that, turned into a conductive vacancy, floats (no listed neighbour is a member) and lies closer than the gap
    to both sides: the one whose farther side is nearest.  (site, d2 to the left side, d2 to the right side)"""
    xyz, NL = d["xyz"], d["N_contact"]
    members = cls != 0
    ok = np.ones(len(xyz), bool)
    ok[:NL] = ok[-NL:] = False
    ok &= ~members & ~np.isin(d["element"], d["metals"])
    listed = (neigh >= 0) & (neigh < len(xyz))
    ok &= ~(members[np.where(listed, neigh, 0)] & listed).any(axis=1)
    cand, reach, both = np.flatnonzero(ok), np.sqrt(gap2) * (1 + 1e-9), []
    trees = [cKDTree(xyz[side == bit]) for bit in (1, 2)]                      # (proposals only: the d2 below are exact)
    cand = cand[(trees[0].query(xyz[cand])[0] <= reach) & (trees[1].query(xyz[cand])[0] <= reach)]
    assert len(cand) > 0
    for bit in (1, 2):
        s = np.flatnonzero(side == bit)
        both.append(np.array([R.d2_exact(xyz, np.full(len(s), c), s).min() for c in cand]))
    far = np.maximum(both[0], both[1])
    k = int(np.argmin(far))
    assert far[k] < gap2, (far[k], gap2)
    return int(cand[k]), float(both[0][k]), float(both[1][k])


def test_cell_with_the_filament_cut(cell5):
    import torch
    cell5.cut(2.0)
    got, side = _check(cell5)
    r = got["chains"][0]
    assert r["status"] == R.CHAINED and r["direct2"] == 21.324007338524996 and got["stats"]["cells_chained"] == 1
    # one vacancy in the cut: a chain of two hops, both shorter than the gap
    d = cell5.d
    cls = CR.classes(cell5.buf.site_element.cpu().numpy(), cell5.buf.site_charge.cpu().numpy(), d["metals"])
    site, d2_left, d2_right = stone_for_the_cut(d, cell5.neigh, cls, side, r["direct2"])
    element0 = cell5.buf.site_element.clone()
    try:
        cell5.buf.site_element[site] = int(CR.VACANCY)
        cell5.buf.site_charge[site] = 0
        got, _ = _check(cell5)
        r = got["chains"][0]
        gap = cell5.run()["gaps"][0]
        assert gap["gap2"] == 21.324007338524996                     # the gap does not see the stone
        assert r["status"] == R.CHAINED and r["n_hops"] == 2 and r["hop_max"] < gap["gap"]
        assert got["hops"][0]["to"][0] == site == got["hops"][0]["from"][1]
        assert got["hops"][0]["d2"][:2].tolist() == [d2_left, d2_right] and r["hop_max2"] == max(d2_left, d2_right)
    finally:
        cell5.buf.site_element.copy_(element0)
        cell5.buf.site_charge.copy_(cell5.charge0)
    cell5.cut(12.0)
    got, _ = _check(cell5)
    assert got["chains"][0]["status"] in (R.OPEN, R.CHAINED) and np.isinf(got["chains"][0]["direct2"])


def test_cell_without_a_filament(km):
    dv = _Device(km, CR.cell_5nm(km, None))
    try:
        got, _ = _check(dv)
        r = got["chains"][0]
        assert (r["n_left"], r["n_right"]) == (5766, 7931) and np.isinf(r["direct2"]) and r["status"] in (R.OPEN, R.CHAINED)
    finally:
        dv.close()


def test_null_outputs_and_filament_arguments(cell5):
    cell5.cut(2.0)
    full = _chain(cell5)
    for kw in (dict(sides=False), dict(nodes=False), dict(sides=False, nodes=False)):
        r = _chain(cell5, **kw)
        assert r["chains"].tobytes() == full["chains"].tobytes() and r["hops"].tobytes() == full["hops"].tobytes()
        assert (r["side"] is None) == (kw.get("sides") is False) and (r["node"] is None) == (kw.get("nodes") is False)
    S, buf, NL = cell5.S, cell5.buf, cell5.d["N_contact"]
    with pytest.raises(S._L.KmcfError, match="r_max.*cutoff"):
        _chain(cell5, r_max=20.5)
    with pytest.raises(S._L.KmcfError, match="N_left_tot"):
        S.filament_chain(cell5.comm, buf, -1, NL, R_MAX)
    with pytest.raises(S._L.KmcfError, match="exceeds N"):
        S.filament_chain(cell5.comm, buf, buf.N_, 1, R_MAX)
    lib, p = S._L.load(), S._ptr
    chains = np.zeros(1, S.CHAIN_DTYPE)
    head = lambda **o: [o.get("idx", buf.cutoff_idx), o.get("nn", buf.nn_), o.get("neigh", p(buf.neigh_idx)),
                        o.get("element", p(buf.site_element)), o.get("charge", p(buf.site_charge)),
                        o.get("metals", p(buf.metal_types)), o.get("num_metals", buf.num_metal_types_), p(buf.site_x),
                        p(buf.site_y), p(buf.site_z), NL, o.get("NR", NL), R_MAX, None, 1,
                        chains.ctypes.data_as(C.POINTER(S._L.Chain)), None, 0, None, None, None]
    for match, o in (("d_neigh_idx", dict(neigh=None)), ("d_site_element", dict(element=None)), ("d_site_charge", dict(charge=None)),
                     ("nn", dict(nn=0)), ("num_metals", dict(num_metals=-1)), ("d_metals", dict(metals=None)),
                     ("N_right_tot", dict(NR=-2)), ("p is NULL", dict(idx=None))):
        assert lib.kmcf_filament_chain(*head(**o)) == -1 and match in lib.kmcf_last_error().decode(), match
    assert lib.kmcf_filament_chain(*head()) == 0 and chains.tobytes() == full["chains"].tobytes()


def test_crossbar_2x2_cells(km):
    d = km.structure.synth_crossbar_40nm(tiles=2, filament=4.0)
    cell = km.structure.crossbar_lines(d)[2]
    dv = _Device(km, d, cell=cell, n_cells=4)
    try:
        got, _ = _check(dv)
        assert got["chains"]["status"][0] == R.BRIDGED and (got["chains"]["status"][1:] != R.BRIDGED).all()
        assert (got["chains"]["n_left"] > 0).all() and (got["chains"]["n_right"] > 0).all()
    finally:
        dv.close()
