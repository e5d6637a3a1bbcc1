"""GPU: kmcf_site_set_gap and kmcf_filament_gap (csrc/kmcf_gap.hip) against the restatement of tests/site_gap_ref.py:
array_equal on every field of every record and on every integer of the stats; gap within 1 ulp of sqrt(gap2).  Synthetic
site sets on indices with small cells (ties, the 27 relations of index cells, the rim of r_max, 1000 random gap cells, one
crowded index cell); the 5 nm cell with a filament, with the filament cut narrowly and widely, without one; a 2 x 2
crossbar with its four cells.  tests/test_site_gap_ref.py pins the restatement and shows that the cases are what their
names say."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as CR
import site_gap_ref as GR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comm(km):
    c = km.solvers.KMC_comm(1, 2, 1, 1)
    c.connect()
    yield c
    c.close()


def _same(got, ref):
    gaps, st = got
    r_gaps, r_st = ref
    print({k: st[k] for k in GR.STAT_KEYS}, "clusters %.3f ms, search %.3f ms" % (st["ms_clusters"], st["ms_search"]))
    for k in GR.STAT_KEYS:
        assert st[k] == r_st[k], (k, st[k], r_st[k])
    for f in GR.EXACT_FIELDS:
        assert np.array_equal(gaps[f], r_gaps[f]), (f, np.flatnonzero(gaps[f] != r_gaps[f])[:8])
    root = np.sqrt(r_gaps["gap2"])
    fin = np.isfinite(root)
    assert np.array_equal(np.isfinite(gaps["gap"]), fin) and (gaps["gap"][~fin] == np.inf).all()
    assert (np.abs(gaps["gap"][fin] - root[fin]) <= np.spacing(root[fin])).all()


# ---- the search primitive on synthetic sets --------------------------------------------------------------------------------------

class _Index:
    """a spatial index over a case's coordinates, with the case's cell edge"""

    def __init__(self, km, comm, c):
        import torch
        self.km, self.c = km, c
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (f64(c["xyz"][:, k]) for k in range(3))
        self.side = i32(c["side"])
        self.cell = i32(c["cell"]) if c["cell"] is not None else None
        self.handle = C.c_void_p()
        p = km.solvers._ptr
        km.lib.check(km.lib.load().kmcf_compute_cutoff_list(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                            float(c["cutoff"]), C.byref(self.handle)), "kmcf_compute_cutoff_list")

    def gap(self, r_max=None, stats=True):
        """the C entry itself: (records, stats dict or None)"""
        km, c, p = self.km, self.c, self.km.solvers._ptr
        gaps = np.zeros(c["n_cells"], km.solvers.GAP_DTYPE)
        st = km.lib.GapStats()
        rc = km.lib.load().kmcf_site_set_gap(self.handle, p(self.x), p(self.y), p(self.z), p(self.side),
                                             float(c["r_max"] if r_max is None else r_max), p(self.cell), c["n_cells"],
                                             gaps.ctypes.data_as(C.POINTER(km.lib.Gap)), C.byref(st) if stats else None)
        km.lib.check(rc, "kmcf_site_set_gap")
        return gaps, (st.as_dict() if stats else None)

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


@pytest.mark.parametrize("name", ["planes", "straddle", "rim", "rim_below", "mixed", "dense", "large", "large_two",
                                  "tile_edge@2047", "tile_edge@2048", "tile_edge@2049"])
def test_site_sets_match_the_restatement(km, comm, name):
    ix = _Index(km, comm, GR.case(name))
    try:
        got = ix.gap()
        _same(got, GR.reference(name))
        again = ix.gap()                                             # scratch reused: the same bytes
        assert got[0].tobytes() == again[0].tobytes()
        assert ix.gap(stats=False)[0].tobytes() == got[0].tobytes()
        if name == "rim":                                           # ... and the same index with r_max just below the pair
            below = ix.gap(r_max=GR.case("rim_below")["r_max"])
            _same(below, GR.reference("rim_below"))
    finally:
        ix.close()


def test_r_max_above_the_cutoff_is_refused(km, comm):
    ix = _Index(km, comm, GR.case("rim"))
    try:
        with pytest.raises(km.lib.KmcfError, match="r_max.*cutoff"):
            ix.gap(r_max=float(np.nextafter(15.0, 16.0)))
        _same(ix.gap(r_max=15.0), GR.site_set_gap(ix.c["xyz"], ix.c["side"], 15.0))      # the cutoff itself is allowed
    finally:
        ix.close()


# ---- the full call on devices ------------------------------------------------------------------------------------------------------

R_MAX = 20.0


class _Device:
    """list from kmcf_neighbor_list, charges from kmcf_update_charge, index from kmcf_compute_cutoff_list"""

    def __init__(self, km, d, cell=None, n_cells=1):
        S = km.solvers
        self.S, self.d, self.cell, self.n_cells = S, d, cell, n_cells
        N, NL = d["N"], d["N_contact"]
        self.comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
        self.comm.connect()
        self.buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                                d["lattice"], d["metals"])
        S.compute_neighbor_list(self.comm, self.buf, 3.5, 52)
        S.compute_cutoff_list(self.comm, self.buf, 20.0)
        S.update_charge_gpu(self.buf.site_element, self.buf.site_charge, self.buf.neigh_idx, N, 52, self.buf.metal_types,
                            self.buf.num_metal_types_, self.comm.counts_events, self.comm.displs_events, self.comm)
        self.neigh = self.buf.neigh_idx.cpu().numpy().reshape(N, 52)
        self.charge0 = self.buf.site_charge.clone()

    def run(self, r_max=R_MAX, **kw):
        NL = self.d["N_contact"]
        return self.S.filament_gap(self.comm, self.buf, NL, NL, r_max, site_cell=self.cell, n_cells=self.n_cells, **kw)

    def restated(self, bins=None):
        d = self.d
        return GR.filament_gap(self.neigh, d["element"], self.buf.site_charge.cpu().numpy(), d["metals"], d["xyz"], d["N_contact"],
                               d["N_contact"], R_MAX, cell=self.cell, n_cells=self.n_cells, bins=bins)

    def check(self, bins=None):
        got, ref = self.run(bins=bins), self.restated(bins)
        _same((got["gaps"], got["stats"]), (ref["gaps"], ref["stats"]))
        assert np.array_equal(got["side"].cpu().numpy(), ref["side"])
        if bins is not None:
            assert got["profile"].dtype == np.int32 and np.array_equal(got["profile"], ref["profile"])
        return got, ref

    def cut(self, half_width):
        import torch
        d = self.d
        self.buf.site_charge.copy_(self.charge0)
        label, table, _ = CR.clusters(self.neigh, d["element"], self.charge0.cpu().numpy(), d["metals"], d["xyz"][:, 0],
                                      d["N_contact"], d["N_contact"])
        slab = CR.slab_sites(label, table, d["xyz"][:, 0], half_width)
        self.buf.site_charge[torch.as_tensor(slab, device="cuda")] = 2

    def close(self):
        self.buf.freeGPUmemory()
        self.comm.close()


@pytest.fixture(scope="module")
def cell5(km):
    dv = _Device(km, CR.cell_5nm(km, 4.0))
    yield dv
    dv.close()


BINS = (17, -1.0, 52.0)


def test_cell_with_a_filament_is_bridged(cell5):
    cell5.buf.site_charge.copy_(cell5.charge0)
    got, _ = cell5.check(bins=BINS)
    g = got["gaps"][0]
    assert (g["n_left"], g["n_right"], g["n_both"], g["bridged"], g["gap2"]) == (5930, 8094, 164, 1, 0.0)
    assert g["site_left"] == g["site_right"] and got["profile"][0][:, 2].sum() == 164
    assert GR.constriction(got["profile"][0]) >= 1


def test_cell_with_the_filament_cut(cell5):
    cell5.cut(2.0)
    got, _ = cell5.check(bins=BINS)
    g = got["gaps"][0]
    assert g["gap2"] == 21.324007338524996 and (g["site_left"], g["site_right"]) == (6145, 6204)
    assert (g["n_left"], g["n_right"], g["n_both"]) == (5848, 7999, 0) and got["stats"]["cells_open"] == 1
    assert got["profile"][0][:, 2].sum() == 0
    cell5.cut(12.0)
    got, _ = cell5.check()
    g = got["gaps"][0]
    assert (g["n_left"], g["n_right"], g["site_left"]) == (5815, 7972, -1) and got["stats"]["cells_none"] == 1


def test_cell_without_a_filament(km):
    dv = _Device(km, CR.cell_5nm(km, None))
    try:
        got, _ = dv.check()
        g = got["gaps"][0]
        assert (g["n_left"], g["n_right"], g["n_both"], g["site_left"]) == (5766, 7931, 0, -1) and np.isinf(g["gap"])
    finally:
        dv.close()


def test_null_outputs_and_two_calls(cell5):
    cell5.cut(2.0)
    full = cell5.run(bins=BINS)
    for kw in (dict(), dict(sides=False), dict(bins=BINS, sides=False)):
        r = cell5.run(**kw)
        assert r["gaps"].tobytes() == full["gaps"].tobytes()
        assert {k: r["stats"][k] for k in GR.STAT_KEYS} == {k: full["stats"][k] for k in GR.STAT_KEYS}
        assert (r["side"] is None) == (kw.get("sides") is False) and (r["profile"] is None) == ("bins" not in kw)
    again = cell5.run(bins=BINS)
    assert again["gaps"].tobytes() == full["gaps"].tobytes() and again["profile"].tobytes() == full["profile"].tobytes()
    assert bool((again["side"] == full["side"]).all())
    # the search primitive on the sides the full call wrote: the same records
    r = cell5.S.site_set_gap(cell5.buf, full["side"], R_MAX)
    assert r["gaps"].tobytes() == full["gaps"].tobytes()
    with pytest.raises(cell5.S._L.KmcfError, match="r_max.*cutoff"):
        cell5.run(r_max=20.5)


def test_clusters_and_pairwise_term_are_not_disturbed(cell5):
    S, buf, comm, NL = cell5.S, cell5.buf, cell5.comm, cell5.d["N_contact"]
    cell5.cut(2.0)

    def snapshot():
        cl = S.conductive_clusters(comm, buf, NL, NL)
        S.poisson_gridless_gpu(buf, comm)
        ints = {k: v for k, v in cl["stats"].items() if k != "ms"}
        return cl["label"].cpu().numpy().tobytes(), cl["clusters"].tobytes(), ints, buf.site_potential_charge.cpu().numpy().tobytes()

    before = snapshot()
    assert np.frombuffer(before[3], np.float64).any()               # the cut sites carry charge: the term is not zero
    cell5.run(bins=BINS)
    assert snapshot() == before


def test_crossbar_2x2_cells(km):
    d = km.structure.synth_crossbar_40nm(tiles=2, filament=4.0)
    cell = km.structure.crossbar_lines(d)[2]
    dv = _Device(km, d, cell=cell, n_cells=4)
    try:
        got, _ = dv.check(bins=BINS)
        assert got["gaps"]["bridged"].tolist() == [1, 0, 0, 0] and got["gaps"]["n_both"].tolist() == [161, 0, 0, 0]
        assert (got["stats"]["cells_bridged"], got["stats"]["cells_none"]) == (1, 3)
    finally:
        dv.close()
