"""GPU: kmcf_conductive_clusters (csrc/kmcf_clusters.hip) against the restatement of tests/clusters_ref.py, array_equal on
the labels, on every field of the table (x_min / x_max included) and on every integer of the stats: synthetic graphs from
5 sites to a path of 131 072 shuffled ids and 600 077 interleaved sites, nn from 1 to 70, one-way entries, out-of-range
entries; the 5 nm cell with a filament, without one and with the filament cut; a 2 x 2 crossbar with a filament.
tests/test_clusters_ref.py pins the restatement and shows that the graphs are what their names say."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as CR
import events_graph_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def comm(km):
    """one communicator for the whole file: its workspace is grown and reused across graphs of every size"""
    c = km.solvers.KMC_comm(1, 2, 1, 1)
    c.connect()
    yield c
    c.close()


class _Dev:
    def __init__(self, c):
        import torch
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.c = c
        self.neigh, self.el, self.ch, self.metals = i32(c["neigh"].reshape(-1)), i32(c["element"]), i32(c["charge"]), i32(c["metals"])
        self.x = torch.as_tensor(np.ascontiguousarray(c["x"], dtype=np.float64), device="cuda")


def _call(km, comm, dv, labels=True, max_clusters=None):
    """the C entry itself: (label or None, table or None, stats dict with passes and ms)"""
    import torch
    S, c = km.solvers, dv.c
    lib = km.lib.load()
    label = torch.full((c["N"],), -7, dtype=torch.int32, device="cuda") if labels else None
    table = np.zeros(max_clusters, S.CLUSTER_DTYPE) if max_clusters else None
    st = km.lib.ClusterStats()
    p = S._ptr
    rc = lib.kmcf_conductive_clusters(comm.handle, c["N"], c["nn"], p(dv.neigh), p(dv.el), p(dv.ch), p(dv.metals),
                                      len(c["metals"]), p(dv.x), c["NL"], c["NR"], p(label),
                                      table.ctypes.data_as(C.POINTER(km.lib.Cluster)) if max_clusters else None,
                                      max_clusters or 0, C.byref(st))
    km.lib.check(rc, "kmcf_conductive_clusters")
    return (label.cpu().numpy() if labels else None), table, st.as_dict()


def _full(km, comm, dv):
    _, _, st = _call(km, comm, dv, labels=False)
    return _call(km, comm, dv, max_clusters=max(st["n_clusters"], 1))


def _same(got, ref):
    label, table, st = got
    r_label, r_table, r_st = ref
    n = r_st["n_clusters"]
    print({k: st[k] for k in CR.STAT_KEYS}, "passes %d, %.3f ms" % (st["passes"], st["ms"]))
    for k in CR.STAT_KEYS:
        assert st[k] == r_st[k], (k, st[k], r_st[k])
    assert np.array_equal(label, r_label), "labels differ at %d sites" % int((label != r_label).sum())
    for f in CR.TABLE_DTYPE.names:
        assert np.array_equal(table[f][:n], r_table[f]), f
    assert np.array_equal(table[:n], r_table)


CASES = ["tiny", "none", "one", "path_shuffled", "pairs1", "nn70", "scatter", "asym", "junk"]


@pytest.mark.parametrize("name", CASES)
def test_synthetic_graph_matches_the_restatement(km, comm, name):
    c = CR.case(name)
    got = _full(km, comm, _Dev(c))
    _same(got, CR.reference(name))
    if name == "path_shuffled":
        assert got[0][c["ends"][0]] == 0 and got[0][c["ends"][1]] == 0
    if name == "none":
        assert got[2]["n_clusters"] == 0 and (got[0] == -1).all()
    if name == "one":
        assert got[1]["root"].tolist() == [0]


def test_passes_do_not_depend_on_the_input(km, comm):
    passes = [_call(km, comm, _Dev(CR.case(n)), labels=False)[2]["passes"] for n in ("tiny", "path_shuffled", "scatter")]
    assert passes[0] >= 1 and passes == [passes[0]] * 3, passes


def test_two_calls_return_the_same_bytes(km, comm):
    dv = _Dev(CR.case("scatter"))
    a, b = _full(km, comm, dv), _full(km, comm, dv)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert {k: a[2][k] for k in CR.STAT_KEYS} == {k: b[2][k] for k in CR.STAT_KEYS}


def test_null_outputs_prefix_and_untouched_inputs(km, comm):
    c = CR.case("junk")
    r_label, r_table, r_st = CR.reference("junk")
    dv = _Dev(c)
    before = [t.clone() for t in (dv.neigh, dv.el, dv.ch, dv.metals, dv.x)]
    ints = lambda st: {k: st[k] for k in CR.STAT_KEYS + ("passes",)}
    full = _full(km, comm, dv)
    for labels, cap in ((False, None), (True, None), (False, r_st["n_clusters"])):
        assert ints(_call(km, comm, dv, labels=labels, max_clusters=cap)[2]) == ints(full[2])
    cap = 100
    assert cap < r_st["n_clusters"]
    lib, S = km.lib.load(), km.solvers
    short = np.zeros(cap + 3, S.CLUSTER_DTYPE)                        # three entries behind the cap: they stay as they are
    short["root"] = -9
    p = S._ptr
    st2 = km.lib.ClusterStats()
    km.lib.check(lib.kmcf_conductive_clusters(comm.handle, c["N"], c["nn"], p(dv.neigh), p(dv.el), p(dv.ch), p(dv.metals),
                                              len(c["metals"]), p(dv.x), c["NL"], c["NR"], None,
                                              short.ctypes.data_as(C.POINTER(km.lib.Cluster)), cap, C.byref(st2)), "prefix")
    assert st2.n_clusters == r_st["n_clusters"]                       # the true count
    assert np.array_equal(short[:cap], r_table[:cap]) and (short["root"][cap:] == -9).all()
    assert np.all(np.diff(short["root"][:cap]) > 0)
    for t, b in zip((dv.neigh, dv.el, dv.ch, dv.metals, dv.x), before):
        assert bool((t == b).all())


def test_event_step_after_the_analysis_matches_the_oracle(km, oracle, comm):
    """local7 of tests/events_graph_ref.py: the analysis on the step's own communicator and arrays, then the step."""
    import torch
    S = km.solvers
    c, ref = G.case("local7"), G.reference(oracle, "local7")
    ev = S.KMC_comm(c["N"] - 2, c["N"] + 1, c["N"], c["N"])
    ev.connect()
    try:
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        cc = dict(N=c["N"], nn=c["nn"], neigh=c["neigh"], element=c["element"], charge=c["charge"],
                  metals=np.array([G.R.O_EL], np.int32), x=c["xyz"][:, 0], NL=50, NR=50)      # "metal": the oxygen sites
        dv = _Dev(cc)
        lay, pot = i32(c["lay"]), f64(c["pot"])
        y, z = f64(c["xyz"][:, 1]), f64(c["xyz"][:, 2])
        step = lambda rng: S.execute_kmc_step_mpi(ev, c["N"], ev.counts_events, ev.displs_events, c["nn"], dv.neigh, lay,
                                                  c["T_bg"], c["freq"], c["sigma"], c["k"], dv.x, y, z, pot, dv.el, dv.ch, rng,
                                                  c["layers"], max_events=c["max_events"], return_log=True)
        got = _full(km, ev, dv)
        _same(got, CR.clusters(cc["neigh"], cc["element"], cc["charge"], cc["metals"], cc["x"], 50, 50))
        t, n, log = step(S.RandomNumberGenerator(c["seed"]))
        assert n == ref["n"] and np.array_equal(log, ref["log"])
        assert np.array_equal(dv.el.cpu().numpy(), ref["el"]) and np.array_equal(dv.ch.cpu().numpy(), ref["ch"])
        assert t == pytest.approx(ref["t"], rel=1e-12)
        # ... and between two steps: the analysis of the stepped state, nothing of the step's workspace disturbed
        got = _full(km, ev, dv)
        _same(got, CR.clusters(cc["neigh"], ref["el"], ref["ch"], cc["metals"], cc["x"], 50, 50))
    finally:
        ev.close()


# ---- devices ---------------------------------------------------------------------------------------------------------------

class _Device:
    """list from kmcf_neighbor_list, charges from kmcf_update_charge"""

    def __init__(self, km, d):
        S = km.solvers
        self.S, self.d = S, d
        N, NL = d["N"], d["N_contact"]
        self.comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
        self.comm.connect()
        self.buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                                d["lattice"], d["metals"])
        S.compute_neighbor_list(self.comm, self.buf, 3.5, 52)
        S.update_charge_gpu(self.buf.site_element, self.buf.site_charge, self.buf.neigh_idx, N, 52, self.buf.metal_types,
                            self.buf.num_metal_types_, self.comm.counts_events, self.comm.displs_events, self.comm)

    def run(self):
        out = self.S.conductive_clusters(self.comm, self.buf, self.d["N_contact"], self.d["N_contact"])
        return out["label"].cpu().numpy(), out["clusters"], out["stats"]

    def restated(self):
        d, b = self.d, self.buf
        return CR.clusters(b.neigh_idx.cpu().numpy().reshape(d["N"], 52), d["element"], b.site_charge.cpu().numpy(), d["metals"],
                           d["xyz"][:, 0], d["N_contact"], d["N_contact"])

    def close(self):
        self.buf.freeGPUmemory()
        self.comm.close()


def test_cell_with_a_filament_and_with_the_filament_cut(km):
    import torch
    dv = _Device(km, CR.cell_5nm(km, 4.0))
    try:
        got, ref = dv.run(), dv.restated()
        _same(got, ref)
        st = got[2]
        assert (st["n_clusters"], st["n_metal_clusters"], st["n_vacancy_clusters"]) == (36, 2, 34)
        assert st["n_bridging"] == 1 and st["largest_bridging"] == 164
        b = got[1][got[1]["touch"] == 3]
        b = b[b["kind"] == CR.VAC]
        assert b["root"].tolist() == [2778]
        slab = CR.slab_sites(ref[0], ref[1], dv.d["xyz"][:, 0])
        assert len(slab) == 13
        dv.buf.site_charge[torch.as_tensor(slab, device="cuda")] = 2
        got = dv.run()
        _same(got, dv.restated())
        st = got[2]
        assert st["n_bridging"] == 0 and st["n_vacancy_clusters"] == 35 and st["largest_vacancy"] == 82
    finally:
        dv.close()


def test_cell_without_a_filament(km):
    dv = _Device(km, CR.cell_5nm(km, None))
    try:
        got = dv.run()
        _same(got, dv.restated())
        st = got[2]
        assert st["n_vacancy_clusters"] == 36 and st["largest_vacancy"] == 4 and st["n_bridging"] == 0
    finally:
        dv.close()


def test_crossbar_2x2_with_a_filament(km):
    d = km.structure.synth_crossbar_40nm(tiles=2, filament=4.0)
    assert d["N"] == 102832
    dv = _Device(km, d)
    try:
        got = dv.run()
        _same(got, dv.restated())
        st = got[2]
        assert st["n_metal_clusters"] == 4 and st["n_bridging"] == 1 and st["largest_bridging"] == 161
    finally:
        dv.close()
