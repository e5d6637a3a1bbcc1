"""CPU: the restatement of kmcf_pair_correlation (tests/pair_corr_ref.py) on inputs whose answer holds by construction, and
the conditions every input of tests/test_gpu_pair_corr.py is built for.

edge_probe, measured here (pairs whose sqrt-guessed bin differs from the table bin / pairs of the setting):
    (n_bins, r_max)      sqrt(d2) * (n / r)    sqrt(d2) / r * n    sqrt(d2) / (r / n)
    (7, 12)                    2 / 59               2 / 59               2 / 59
    (20, 20)                   0 / 176              2 / 176              0 / 176
    (256, 20)                 51 / 1157             0 / 1157             0 / 1157
    (13, 9.5)                  0 / 113              9 / 113              3 / 113
Every spelling is wrong on pairs of the case and every setting has a spelling that is wrong on it.  A spelling cannot be
wrong on EVERY setting: at (20, 20) n / r = r / n = 1 and e[k] = k exactly, sqrt(fl(dx * dx)) = dx for these dx, so the
first and the third spelling are floor(dx), which is the table bin (fl(dx * dx) < k * k for every double dx < k)."""
import numpy as np
import pytest

import pair_corr_ref as R
import pbc_ref as P
import site_gap_pbc_ref as GP


# ---- the restatement on answers that hold by construction ------------------------------------------------------------------------

def test_three_sites_on_a_line():
    xyz = np.array([[0.0, 0, 0], [3.0, 0, 0], [7.0, 0, 0], [3.0, 4.0, 0]])
    r = R.pair_correlation(xyz, [0, 1, 0, 2], 2, 5.0, 5, r_count=4.0)          # site 3 is a probe
    assert np.array_equal(r["edge2"], [0.0, 1.0, 4.0, 9.0, 16.0, 25.0])
    # pairs: (0,1) d2 = 9 -> bin 3, classes (0,1) -> index 1; (1,2) d2 = 16 -> bin 4, index 1; (0,2) d2 = 49: beyond
    want = np.zeros((2, 3, 5), np.uint64)
    want[0, 1, 3] = want[0, 1, 4] = 1
    assert np.array_equal(r["hist"], want)
    assert np.array_equal(r["members"], [[2, 1], [0, 0]])
    # counts within 4: site 0: {1}; site 1: {0, 2}; site 2: {1}; probe 3: {1} (d = 4), 0 and 2 are 5 away
    assert np.array_equal(r["counts"], [[0, 1], [2, 0], [0, 1], [0, 1]])
    assert r["stats"] == dict(n_pairs_total=2, n_members=3, n_probes=1, max_count=2, max_count_site=1)


def test_d2_on_r_max_counts_and_lands_in_the_last_bin():
    xyz = np.array([[0.0, 0, 0], [3.0, 4.0, 0]])
    r = R.pair_correlation(xyz, [0, 0], 1, 5.0, 7)
    assert r["hist"].sum() == 1 and r["hist"][0, 0, 6] == 1
    assert R.pair_correlation(xyz, [0, 0], 1, np.nextafter(5.0, 0.0), 7)["hist"].sum() == 0


def test_buckets():
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0], [3.0, 0, 0]])
    r = R.pair_correlation(xyz, [0, 0, 0, 0], 1, 1.5, 1, cell=[0, 0, 1, 5], n_cells=2)
    # (0,1) same cell 0; (1,2) different valid cells: rest; (2,3): site 3 has no valid cell: no bucket
    assert np.array_equal(r["hist"][:, 0, 0], [1, 0, 1])
    assert np.array_equal(r["members"][:, 0], [2, 1, 1])
    assert np.array_equal(r["counts"][:, 0], [1, 2, 2, 1])                       # the counts ignore the cells


def test_minimum_image_one_distance_per_pair():
    """Ly = 16 < 2 r_max: the partner lies 11 above and its image 5 below; one pair, d2 = 25"""
    xyz = np.array([[4.0, 1, 8], [4.0, 12, 8]])
    L = np.array([16.0, 16.0, 64.0])
    r = R.pair_correlation(xyz, [0, 0], 1, 12.0, 12, L=L)
    assert r["hist"].sum() == 1 and r["hist"][0, 0, 5] == 1 and np.array_equal(r["counts"][:, 0], [1, 1])
    assert R.pair_correlation(xyz, [0, 0], 1, 12.0, 12, L=None)["hist"][0, 0, 11] == 1


def test_class_pair_index():
    for n in range(1, 5):
        seen = [int(R.pair_index(p, q, n)) for p in range(n) for q in range(p, n)]
        assert seen == list(range(R.n_pairs(n)))
        assert all(R.pair_index(q, p, n) == R.pair_index(p, q, n) for p in range(n) for q in range(n))


# ---- the conditions on the inputs ----------------------------------------------------------------------------------------------

def test_every_case_fits_the_limits():
    for name in R.CASES:
        c = R.case(name)
        assert len(c["xyz"]) <= 3072 and c["r_max"] <= c["cutoff"] and 0 < c["r_count"] <= c["r_max"], name
        assert (c["xyz"].max(0)[1:] - c["xyz"].min(0)[1:] < c["L"][1:]).all(), name


@pytest.mark.parametrize("name", [n for n in R.CASES if n[0] == "p"])
def test_random_cases_take_the_general_path(name):
    c = R.case(name)
    base = name.split("#")[0]
    assert P.cells_per_period(c["L"]) == P.RANDOM_CASES[base][3]
    cls = c["cls"]
    share = [(cls == v).mean() for v in (0, 1, 2, 3, -1)]
    assert all(abs(s - w) < 0.05 for s, w in zip(share, (.25, .25, .25, .15, .10))), share
    assert c["cell"].min() == -1 and c["cell"].max() == c["n_cells"]
    for periodic in (True, False):
        r = R.reference(name, periodic)
        h = r["hist"]
        assert (h.sum(axis=2) > 0).all(), "every class pair in every bucket, the rest bucket included"
        i, j, d2 = R.pairs_within(c["xyz"], cls, 3, c["r_max"], c["L"] if periodic else None)
        assert len(i) > r["stats"]["n_pairs_total"] > 0                      # some pairs enter no bucket
        # pairs between r_count and r_max
        assert ((d2 > c["r_count"] ** 2) & (d2 <= c["r_max"] ** 2)).any() or c["r_count"] == c["r_max"]
        # in the index-cell order a centre meets partners of smaller and of larger id: both orders occur among the pairs
        # of every member that has at least two partners
        deg_lo, deg_hi = np.bincount(j, minlength=len(cls)), np.bincount(i, minlength=len(cls))
        assert ((deg_lo > 0) & (deg_hi > 0)).sum() > 100
    assert not np.array_equal(R.reference(name, True)["hist"], R.reference(name, False)["hist"])


def test_lattice_wrap_has_pairs_on_the_bin_edges():
    c = R.case("lattice_wrap")
    assert len(c["xyz"]) == 3072 and (c["r_max"], c["n_bins"], c["r_count"]) == (20.0, 20, 12.0)
    i, j, d2 = R.pairs_within(c["xyz"], c["cls"], c["n_classes"], c["r_max"], c["L"])
    _, edge2 = R.table(c["r_max"], c["n_bins"])
    on_edge = np.isin(d2, edge2)
    print("lattice_wrap: %d pairs within 20 A, %d on an entry of edge2, %d at r_max^2" % (len(d2), on_edge.sum(), (d2 == edge2[-1]).sum()))
    assert len(d2) == 667904 and on_edge.sum() == 103680
    assert on_edge.sum() >= 1000 and (d2 == edge2[-1]).any()
    r = R.reference("lattice_wrap")
    assert r["stats"]["n_pairs_total"] == len(d2)                                # one cell: every pair is counted
    # a pair on edge2[k], 0 < k < n_bins, belongs to bin k; on edge2[n_bins] to the last bin
    kb = R.bin_of(edge2, d2[on_edge])
    assert (edge2[kb] == d2[on_edge])[d2[on_edge] < edge2[-1]].all() and (kb[d2[on_edge] == edge2[-1]] == c["n_bins"] - 1).all()


def _edge_probe_differences(n_bins, r_max):
    c = R.case("edge_probe@%d,%g" % (n_bins, r_max))
    i, j, d2 = R.pairs_within(c["xyz"], c["cls"], 2, r_max, c["L"])
    assert len(d2) == len(c["xyz"]) // 2 and (j == i + 1).all()                 # each site's only partner is its own
    _, edge2 = R.table(r_max, n_bins)
    kb = R.bin_of(edge2, d2)
    return {nm: int((np.minimum(f(d2, n_bins, r_max).astype(np.int64), n_bins - 1) != kb).sum()) for nm, f in R.SQRT_SPELLINGS.items()}, len(d2)


def test_edge_probe_defeats_a_sqrt_binning_without_the_table():
    diff = {s: _edge_probe_differences(*s) for s in R.EDGE_SETTINGS}
    for s, (d, n) in diff.items():
        print("edge_probe %s: %d pairs, wrong by spelling: %s" % (s, n, d))
        assert any(d.values()), "no spelling is wrong at %s" % (s,)
    for nm in R.SQRT_SPELLINGS:
        assert any(d[nm] for d, _ in diff.values()), "%s is never wrong" % nm
    assert all(diff[(7, 12.0)][0].values())                                      # at (7, 12) every spelling is wrong
    # one such pair: bin 5 by the table, 6 by the first spelling
    dx = float.fromhex("0x1.4924924924924p+3")
    _, edge2 = R.table(12.0, 7)
    assert R.bin_of(edge2, np.array([dx * dx]))[0] == 5 and int(np.sqrt(dx * dx) * (7 / 12.0)) == 6
    c = R.case("edge_probe@7,12")
    assert dx in c["xyz"][:, 0]


def test_edge_probe_periodic_equals_open():
    for s in R.EDGE_SETTINGS:
        name = "edge_probe@%d,%g" % s
        assert np.array_equal(R.reference(name, True)["hist"], R.reference(name, False)["hist"])


def test_tile_edges():
    for n in (2047, 2048, 2049):
        c = R.case("tile_edge@%d" % n)
        assert len(c["xyz"]) == n and np.array_equal(c["cls"], np.arange(n) % 2)
        assert R.reference("tile_edge@%d" % n)["stats"]["n_members"] == n
    for n in R.CENTRES:
        r = R.reference("centres@%d" % n)
        assert r["stats"]["n_members"] + r["stats"]["n_probes"] == n and r["stats"]["n_probes"] > 0
    assert all(R.reference("centres@%d" % n)["stats"]["n_pairs_total"] > 0 for n in (16, 17, 63, 64, 65))


def test_small_cases():
    r = R.reference("empty")
    assert not r["hist"].any() and not r["members"].any() and not r["counts"].any()
    assert r["stats"] == dict(n_pairs_total=0, n_members=0, n_probes=0, max_count=0, max_count_site=-1)
    r, o = R.reference("single"), R.reference("single", False)
    assert not r["hist"].any() and r["stats"]["n_members"] == 1 and r["stats"]["n_probes"] == 3
    assert r["counts"][:, 0].tolist() == [0, 0, 0, 1, 1, 0] and o["counts"][:, 0].tolist() == [0, 0, 0, 1, 0, 0]   # one probe sees it through the y face
    r = R.reference("dup")
    assert r["hist"].sum() == 1 and r["hist"][0, int(R.pair_index(0, 1, 2)), 0] == 1      # d2 = 0: bin 0
    assert r["counts"].tolist() == [[0, 0], [0, 0], [1, 0], [0, 1], [1, 1]]
    assert R.reference("one_class")["hist"].shape[1] == 1 and R.reference("four_classes")["hist"].shape[1] == 10
    assert (R.reference("four_classes")["hist"].sum(axis=(0, 2)) > 0).all()


def test_defects_follow_the_class_rule():
    d = R.defects()
    for probe_all in (False, True):
        cls = R.defect_classes(d["element"], d["charge"], probe_all)
        vac = d["element"] == P.VACANCY
        assert (cls[vac & (d["charge"] == 0)] == 0).all() and (cls[vac & (d["charge"] != 0)] == 1).all()
        assert (cls[d["element"] == P.OXYGEN_DEFECT] == 2).all()
        other = ~vac & (d["element"] != P.OXYGEN_DEFECT)
        assert (cls[other] == (3 if probe_all else -1)).all() and other.sum() > 300
        assert all((cls == v).sum() >= 2 for v in (0, 1, 2))
        r = R.defects_reference(probe_all)
        assert r["stats"]["n_probes"] == (other.sum() if probe_all else 0) and r["stats"]["n_pairs_total"] > 0
    assert np.array_equal(R.defects_reference(False)["hist"], R.defects_reference(True)["hist"])       # probes are never partners
    assert not np.array_equal(R.defects_reference(True, True)["counts"], R.defects_reference(True, False)["counts"])


# ---- further assertions ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["p23#0", "p52#2", "lattice_wrap", "four_classes", "dup"])
def test_bins_add_up_to_the_pairs_of_a_bucket(name):
    c, r = R.case(name), R.reference(name)
    i, j, d2 = R.pairs_within(c["xyz"], c["cls"], c["n_classes"], c["r_max"], c["L"])
    import site_gap_ref as GR
    cell = GR.cells_of(c["cell"], c["n_cells"], len(c["xyz"]))
    ok = (cell[i] >= 0) & (cell[j] >= 0)
    bucket = np.where(cell[i] == cell[j], cell[i], c["n_cells"])[ok]
    assert np.array_equal(r["hist"].sum(axis=(1, 2)), np.bincount(bucket, minlength=c["n_cells"] + 1))


@pytest.mark.parametrize("name", ["p23#0", "four_classes", "one_class", "empty"])
def test_rdf_times_its_norm_returns_the_histogram(km, name):
    r = R.reference(name)
    vol = 987.25
    for g in (km.solvers.pair_rdf(r, vol), R.pair_rdf(r, vol)):
        n_cells, n_classes = r["hist"].shape[0] - 1, r["members"].shape[1]
        assert g.shape == (n_cells,) + r["hist"].shape[1:]
        e = r["edges"]
        shell = 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
        for c in range(n_cells):
            for p in range(n_classes):
                for q in range(p, n_classes):
                    Np, Nq = float(r["members"][c, p]), float(r["members"][c, q])
                    n_pq = Np * Nq if p != q else Np * (Np - 1) / 2
                    row = g[c, int(R.pair_index(p, q, n_classes))]
                    if n_pq == 0:
                        assert np.isnan(row).all()
                    else:
                        assert np.array_equal(np.rint(row * (n_pq * shell / vol)).astype(np.uint64), r["hist"][c, int(R.pair_index(p, q, n_classes))])
                        assert np.allclose(row * (n_pq * shell / vol), r["hist"][c, int(R.pair_index(p, q, n_classes))], rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("name", ["p11#0", "tile_edge@2049", "single"])
def test_periodic_restatement_without_a_lattice_is_the_open_one(name):
    c = R.case(name)
    a = R.pair_correlation(c["xyz"], c["cls"], c["n_classes"], c["r_max"], c["n_bins"], c["r_count"], c["cell"], c["n_cells"], L=None)
    b = R.reference(name, periodic=False)
    for k in ("hist", "members", "edge2", "counts"):
        assert np.array_equal(a[k], b[k])
    assert a["stats"] == b["stats"]
    # ... and d2_exact with L None is the plain difference
    i, j = np.array([0, 1]), np.array([2, 3])
    dx = c["xyz"][i] - c["xyz"][j]
    assert np.array_equal(GP.d2_exact(c["xyz"], i, j, None), (dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])


def test_python_surface(km):
    assert callable(km.solvers.pair_correlation) and callable(km.solvers.defect_correlation) and callable(km.solvers.pair_rdf)
    assert (km.solvers.PC_MAX_CLASSES, km.solvers.PC_MAX_BINS) == (R.MAX_CLASSES, R.MAX_BINS)
    assert [n for n, _ in km.lib.PairStats._fields_][:5] == list(R.STAT_KEYS)
