"""CPU: the restatement of the conductive cluster analysis (tests/clusters_ref.py) on graphs whose answer is known by
construction and on the 5 nm cell with and without a filament, the conditions that keep the GPU test
(tests/test_gpu_clusters.py) meaningful, and the argument errors of kmcf_conductive_clusters (reached on a host-only
communicator: they are checked before anything needs a device)."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as CR

V, O, M = CR.VACANCY, CR.O_EL, int(CR.METALS[0])


def _rows(rows, nn):
    out = np.full((len(rows), nn), -1, np.int32)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def _table(rows):
    return np.array(rows, CR.TABLE_DTYPE)


def test_two_triangles_joined_through_a_charged_vacancy():
    neigh = _rows([[1, 2], [0, 2], [0, 1, 3], [2, 4], [3, 5, 6], [4, 6], [4, 5]], 3)
    x = np.array([-3.0, 1.0, 2.0, 3.0, 4.0, -7.5, 6.0])
    charge = np.array([0, 0, 0, 2, 0, 0, 0])
    label, table, stats = CR.clusters(neigh, np.full(7, V), charge, CR.METALS, x, 0, 0)
    assert label.tolist() == [0, 0, 0, -1, 4, 4, 4]
    assert np.array_equal(table, _table([(0, 2, 3, 0, -3.0, 2.0), (4, 2, 3, 0, -7.5, 6.0)]))
    assert stats == dict(members=6, n_clusters=2, n_metal_clusters=0, n_vacancy_clusters=2, n_bridging=0, largest_vacancy=3,
                         largest_bridging=0)
    # ... and through an uncharged one: a single cluster
    label, table, stats = CR.clusters(neigh, np.full(7, V), np.zeros(7, int), CR.METALS, x, 0, 0)
    assert label.tolist() == [0] * 7 and np.array_equal(table, _table([(0, 2, 7, 0, -7.5, 6.0)]))


def test_metal_vacancy_metal_line():
    neigh = _rows([[1], [0, 2], [1]], 2)
    x = np.array([-21.0, 0.5, 30.0])
    el = np.array([M, V, M])
    label, table, stats = CR.clusters(neigh, el, np.zeros(3, int), CR.METALS, x, 1, 1)
    assert label.tolist() == [0, 1, 2]                          # a metal-vacancy pair is no conductive edge
    assert np.array_equal(table, _table([(0, 1, 1, 1, -21.0, -21.0), (1, 2, 1, 3, 0.5, 0.5), (2, 1, 1, 2, 30.0, 30.0)]))
    assert stats == dict(members=3, n_clusters=3, n_metal_clusters=2, n_vacancy_clusters=1, n_bridging=1, largest_vacancy=1,
                         largest_bridging=1)
    _, table, stats = CR.clusters(neigh, el, np.zeros(3, int), CR.METALS, x, 0, 0)      # the metals hold no contact id
    assert table["touch"].tolist() == [0, 0, 0] and stats["n_bridging"] == 0
    _, table, _ = CR.clusters(neigh, el, np.zeros(3, int), CR.METALS, x, 1, 0)
    assert table["touch"].tolist() == [1, 1, 0]
    # the entry may stand in the metal's row only
    one_sided = _rows([[1], [], [1]], 2)
    _, table, _ = CR.clusters(one_sided, el, np.zeros(3, int), CR.METALS, x, 1, 1)
    assert table["touch"].tolist() == [1, 3, 2]


def test_one_way_edge_in_a_padding_column_joins_two_clusters():
    neigh = _rows([[1], [0], [3], [2]], 2)
    args = (np.full(4, V), np.zeros(4, int), CR.METALS, np.arange(4.0), 0, 0)
    label, table, _ = CR.clusters(neigh, *args)
    assert label.tolist() == [0, 0, 2, 2] and table["size"].tolist() == [2, 2]
    neigh[3, 1] = 1                                             # 3 lists 1; 1 does not list 3
    label, table, _ = CR.clusters(neigh, *args)
    assert label.tolist() == [0, 0, 0, 0] and np.array_equal(table, _table([(0, 2, 4, 0, 0.0, 3.0)]))


def test_out_of_range_entries_are_padding():
    neigh = _rows([[1, 4], [0, 9], [3, -5], [2, 4]], 2)
    label, _, _ = CR.clusters(neigh, np.full(4, V), np.zeros(4, int), CR.METALS, np.arange(4.0), 0, 0)
    assert label.tolist() == [0, 0, 2, 2]


# ---- the 5 nm cell ---------------------------------------------------------------------------------------------------------

def _device(km, oracle, filament):
    d = CR.cell_5nm(km, filament)
    assert d["N"] == 37650 and d["N_contact"] == 576
    neigh = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 3.5, 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), neigh, d["metals"])
    return d, neigh, charge


def _run(d, neigh, charge):
    return CR.clusters(neigh, d["element"], charge, d["metals"], d["xyz"][:, 0], d["N_contact"], d["N_contact"])


@pytest.fixture(scope="module")
def filament5(km, oracle):
    return _device(km, oracle, 4.0)


def test_cell_with_a_filament(filament5):
    d, neigh, charge = filament5
    label, table, stats = _run(d, neigh, charge)
    assert (stats["n_clusters"], stats["n_metal_clusters"], stats["n_vacancy_clusters"]) == (36, 2, 34)
    assert stats["n_bridging"] == 1 and stats["largest_bridging"] == 164 and stats["largest_vacancy"] == 164
    b = table[(table["kind"] == CR.VAC) & (table["touch"] == 3)]
    assert b["root"].tolist() == [2778] and b["size"].tolist() == [164]
    assert round(float(b["x_min"][0]), 4) == 0.0082 and round(float(b["x_max"][0]), 4) == 50.9657
    metal = table[table["kind"] == CR.METAL]
    assert sorted(metal["touch"].tolist()) == [1, 2]            # the electrodes do not share a cluster
    assert label[0] != label[d["N"] - 1] and label[0] == 0


def test_cell_without_a_filament(km, oracle):
    _, _, stats = _run(*_device(km, oracle, None))
    assert stats["n_vacancy_clusters"] == 36 and stats["largest_vacancy"] == 4 and stats["n_bridging"] == 0


def test_cell_with_the_filament_cut(filament5):
    d, neigh, charge = filament5
    label, table, _ = _run(d, neigh, charge)
    slab = CR.slab_sites(label, table, d["xyz"][:, 0])
    assert len(slab) == 13
    cut = charge.copy()
    cut[slab] = 2
    _, _, stats = _run(d, neigh, cut)
    assert stats["n_bridging"] == 0 and stats["n_vacancy_clusters"] == 35 and stats["largest_vacancy"] == 82


# ---- conditions of the GPU test ----------------------------------------------------------------------------------------------

def test_asym_one_way_entries_merge_clusters():
    """At least 10 of the one-way entries join two clusters that are separate without them."""
    c = CR.case("asym")
    without = CR.reference("asym_without")[0]
    label = CR.reference("asym")[0]
    merging = [(a, b) for a, b in c["one_way"] if without[a] != without[b]]
    print("asym: %d of %d one-way entries merge two clusters" % (len(merging), len(c["one_way"])))
    assert len(merging) >= 10
    assert all(label[a] == label[b] >= 0 for a, b in c["one_way"])
    assert CR.reference("asym")[2]["n_clusters"] < CR.reference("asym_without")[2]["n_clusters"]


def test_synthetic_cases_are_what_their_names_say():
    assert CR.reference("none")[2]["n_clusters"] == 0 and (CR.reference("none")[0] == -1).all()
    label, table, stats = CR.reference("one")
    assert stats["n_clusters"] == 1 and table["root"][0] == 0 and table["size"][0] == 4099 and table["touch"][0] == 3
    c = CR.case("path_shuffled")
    label, table, stats = CR.reference("path_shuffled")
    assert stats["n_clusters"] == 1 and label[c["ends"][0]] == 0 and label[c["ends"][1]] == 0 and table["size"][0] == 1 << 17
    label, table, stats = CR.reference("scatter")
    assert stats["n_clusters"] >= 100                           # many roots ...
    for kind in (CR.METAL, CR.VAC):                             # ... and one cluster per kind that runs through the whole id range
        t = table[table["kind"] == kind]
        sites = np.flatnonzero(label == t["root"][np.argmax(t["size"])])
        assert len(sites) > 100000 and sites.max() - sites.min() > 0.99 * len(label)
    for name in ("tiny", "pairs1", "nn70", "junk"):
        el = CR.case(name)["element"]
        assert CR.reference(name)[2]["n_clusters"] >= 1
        assert name == "tiny" or ((np.isin(el, CR.METALS).mean() > 0.25) and ((el == V).mean() > 0.25))
    x = CR.case("scatter")["x"]
    assert x.min() < 0 < x.max()                                 # extents on both sides of zero
    junk = CR.case("junk")["neigh"]
    assert ((junk >= junk.shape[0]) | (junk < -1)).sum() >= 40


# ---- argument errors: KMCF_ERR_ARG before the host-only-communicator check ---------------------------------------------------

ERR_ARG, ERR_STATE = -1, -4


def _args(h):
    """Well-formed arguments for a host-only communicator.  The device pointers are never dereferenced: every call here
    returns from the argument checks or from the host-only check behind them."""
    fake = C.c_void_p(64)
    return dict(c=h, N=100, nn=4, d_neigh_idx=fake, d_site_element=fake, d_site_charge=fake, d_metals=fake, num_metals=2,
                d_x=fake, N_left_tot=10, N_right_tot=10, d_site_label=fake, h_clusters=None, max_clusters=0, stats=None)


@pytest.mark.parametrize("change,want,word", [
    (dict(c=None), ERR_ARG, b"c is NULL"), (dict(d_neigh_idx=None), ERR_ARG, b"d_neigh_idx"),
    (dict(d_site_element=None), ERR_ARG, b"d_site_element"), (dict(d_site_charge=None), ERR_ARG, b"d_site_charge"),
    (dict(d_x=None), ERR_ARG, b"d_x"), (dict(N=0), ERR_ARG, b"N = 0"), (dict(N=-3), ERR_ARG, b"N = -3"),
    (dict(nn=0), ERR_ARG, b"nn = 0"), (dict(num_metals=-1), ERR_ARG, b"num_metals"),
    (dict(d_metals=None), ERR_ARG, b"d_metals"), (dict(N_left_tot=-1), ERR_ARG, b"N_left_tot"),
    (dict(N_right_tot=-1), ERR_ARG, b"N_right_tot"), (dict(N_left_tot=60, N_right_tot=41), ERR_ARG, b"N_left_tot + N_right_tot"),
    (dict(max_clusters=-1), ERR_ARG, b"max_clusters"), (dict(h_clusters=True), ERR_ARG, b"h_clusters"),
    (dict(), ERR_STATE, b"host-only"), (dict(d_metals=None, num_metals=0), ERR_STATE, b"host-only"),
    (dict(d_site_label=None, N_left_tot=50, N_right_tot=50), ERR_STATE, b"host-only")])
def test_argument_errors_on_a_host_only_communicator(km, change, want, word):
    lib = km.lib.load()
    h = C.c_void_p()
    km.lib.check(lib.kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    try:
        a = _args(h)
        a.update(change)
        table = (km.lib.Cluster * 4)()
        if a["h_clusters"] is True:
            a["h_clusters"] = table
        st = km.lib.ClusterStats()
        a["stats"] = C.byref(st)
        rc = lib.kmcf_conductive_clusters(*a.values())
        msg = lib.kmcf_last_error()
        assert rc == want and word in msg and b"kmcf_conductive_clusters" in msg, (rc, msg)
    finally:
        lib.kmcf_comm_destroy(h)


def test_python_struct_layout(km):
    assert C.sizeof(km.lib.Cluster) == 32 == CR.TABLE_DTYPE.itemsize == km.solvers.CLUSTER_DTYPE.itemsize
    assert CR.TABLE_DTYPE == km.solvers.CLUSTER_DTYPE
    assert [n for n, _ in km.lib.ClusterStats._fields_][:7] == list(CR.STAT_KEYS)
