"""CPU: the restatement of the filament gap analysis (tests/site_gap_ref.py) on answers known by construction -- the 5 nm
cell with a filament, with the filament cut narrowly and widely, without a filament; the 2 x 2 crossbar's cells -- the
conditions that keep the GPU test (tests/test_gpu_site_gap.py) meaningful, the struct layout, and the argument errors of
kmcf_site_set_gap / kmcf_filament_gap that are reachable without an index (they are checked before the index is)."""
import ctypes as C

import numpy as np
import pytest

import clusters_ref as CR
import site_gap_ref as GR

R_MAX = 20.0


# ---- small sets --------------------------------------------------------------------------------------------------------------

def test_tie_break_smallest_a_then_smallest_b():
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 5, 0], [1.0, 5, 0], [0.0, 0, 1.0]])
    gaps, stats = GR.site_set_gap(xyz, [2, 1, 2, 1, 2], 3.0)                     # a in {1, 3}; b in {0, 2, 4}
    g = gaps[0]
    assert (g["site_left"], g["site_right"], g["gap2"], g["gap"]) == (1, 0, 1.0, 1.0)     # (1,0) (3,2) tie; (1,4) is farther
    assert (g["x_left"], g["x_right"]) == (1.0, 0.0) and (g["n_left"], g["n_right"], g["n_both"], g["bridged"]) == (2, 3, 0, 0)
    assert stats == dict(n_left=2, n_right=3, n_both=0, cells_bridged=0, cells_open=1, cells_none=0)
    gaps, _ = GR.site_set_gap(xyz, [2, 1, 2, 1, 2], 3.0, cell=[1, 1, 0, 0, 7], n_cells=2)
    assert gaps["site_left"].tolist() == [3, 1] and gaps["site_right"].tolist() == [2, 0] and gaps["n_right"].tolist() == [1, 1]


def test_a_site_in_both_sets_bridges_its_cell():
    xyz = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
    gaps, stats = GR.site_set_gap(xyz, [1, 2, 3], 0.25)
    g = gaps[0]
    assert (g["gap2"], g["site_left"], g["site_right"], g["n_left"], g["n_right"], g["n_both"], g["bridged"]) == (0.0, 2, 2, 2, 2, 1, 1)
    assert stats["cells_bridged"] == 1 and stats["cells_open"] == 0


def test_no_pair_within_r_max_and_sites_of_no_cell():
    xyz = np.array([[0.0, 0, 0], [3.0, 4.0, 0]])
    gaps, stats = GR.site_set_gap(xyz, [1, 2], np.nextafter(5.0, 0.0))
    g = gaps[0]
    assert np.isinf(g["gap"]) and np.isinf(g["gap2"]) and (g["site_left"], g["site_right"], g["x_left"], g["x_right"]) == (-1, -1, 0.0, 0.0)
    assert stats["cells_none"] == 1
    assert GR.site_set_gap(xyz, [1, 2], 5.0)[0][0]["gap2"] == 25.0             # d2 == r_max*r_max counts
    gaps, stats = GR.site_set_gap(xyz, [1, 2], 5.0, cell=[0, -1], n_cells=1)   # b belongs to no cell
    assert gaps[0]["site_left"] == -1 and (gaps[0]["n_left"], gaps[0]["n_right"]) == (1, 0)
    assert (stats["n_left"], stats["n_right"]) == (1, 1)                       # the device counts include it


def test_profile_bins():
    cls = np.array([2, 2, 2, 1, 2, 2])
    side = np.array([1, 3, 3, 3, 0, 2])
    x = np.array([0.0, 4.99, 5.0, 1.0, 1.0, 10.0])
    p = GR.profile(cls, side, None, 1, x, 2, 0.0, 10.0)
    assert p.tolist() == [[[1, 0, 1], [0, 0, 1]]]                              # metal, non-member and x == x_hi stay out
    assert GR.constriction(p[0]) == 1 and GR.constriction(np.zeros((4, 3), int)) == 0


# ---- the 5 nm cell -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def filament5(km, oracle):
    d = CR.cell_5nm(km, 4.0)
    neigh = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 3.5, 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), neigh, d["metals"])
    return d, neigh, charge


def _gap(d, neigh, charge, **kw):
    return GR.filament_gap(neigh, d["element"], charge, d["metals"], d["xyz"], d["N_contact"], d["N_contact"], R_MAX, **kw)


def _cut(d, neigh, charge, half_width):
    label, table, _ = CR.clusters(neigh, d["element"], charge, d["metals"], d["xyz"][:, 0], d["N_contact"], d["N_contact"])
    cut = charge.copy()
    cut[CR.slab_sites(label, table, d["xyz"][:, 0], half_width)] = 2
    return cut


def test_cell_with_a_filament_is_bridged(filament5):
    d, neigh, charge = filament5
    r = _gap(d, neigh, charge, bins=(10, 0.0, 51.0))
    g = r["gaps"][0]
    assert (g["n_left"], g["n_right"], g["n_both"], g["bridged"]) == (5930, 8094, 164, 1)
    assert g["gap2"] == 0.0 and g["site_left"] == g["site_right"] and r["side"][g["site_left"]] == 3
    assert g["site_left"] == int(np.flatnonzero(r["side"] == 3)[0])
    assert r["stats"] == dict(n_left=5930, n_right=8094, n_both=164, cells_bridged=1, cells_open=0, cells_none=0)
    assert r["profile"][0][:, 2].sum() == 164 and GR.constriction(r["profile"][0]) >= 1


def test_cell_with_the_filament_cut(filament5):
    d, neigh, charge = filament5
    r = _gap(d, neigh, _cut(d, neigh, charge, 2.0))
    g = r["gaps"][0]
    assert (g["n_left"], g["n_right"], g["n_both"], g["bridged"]) == (5848, 7999, 0, 0)
    assert g["gap2"] == 21.324007338524996 and (g["site_left"], g["site_right"]) == (6145, 6204)
    assert round(float(g["gap"]), 4) == 4.6178
    assert (g["x_left"], g["x_right"]) == (d["xyz"][6145, 0], d["xyz"][6204, 0])
    # a unique minimum: no other pair of the two sets is as close
    A, B = np.flatnonzero(r["side"] & 1), np.flatnonzero(r["side"] & 2)
    d2 = GR.d2_exact(d["xyz"], A[:, None], B[None, :])
    assert (d2 <= g["gap2"]).sum() == 1
    assert r["stats"]["cells_open"] == 1


def test_cell_with_the_filament_cut_widely_and_without_a_filament(km, oracle, filament5):
    d, neigh, charge = filament5
    g = _gap(d, neigh, _cut(d, neigh, charge, 12.0))["gaps"][0]
    assert (g["n_left"], g["n_right"], g["n_both"], g["site_left"]) == (5815, 7972, 0, -1) and np.isinf(g["gap"])
    d = CR.cell_5nm(km, None)
    neigh = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 3.5, 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), neigh, d["metals"])
    r = _gap(d, neigh, charge)
    g = r["gaps"][0]
    assert (g["n_left"], g["n_right"], g["n_both"], g["site_left"]) == (5766, 7931, 0, -1) and np.isinf(g["gap"])
    assert r["stats"]["cells_none"] == 1


def test_crossbar_2x2_cells(km, oracle):
    d = km.structure.synth_crossbar_40nm(tiles=2, filament=4.0)
    assert d["N"] == 102832 and d["N_contact"] == 1248
    neigh = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 3.5, 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), neigh, d["metals"])
    cell = km.structure.crossbar_lines(d)[2]
    assert np.bincount(cell[cell >= 0]).tolist() == [10509] * 4
    r = _gap(d, neigh, charge, cell=cell, n_cells=4)
    assert r["gaps"]["bridged"].tolist() == [1, 0, 0, 0] and r["gaps"]["n_both"].tolist() == [161, 0, 0, 0]
    assert r["gaps"]["site_left"].tolist()[1:] == [-1, -1, -1] and np.isinf(r["gaps"]["gap"][1:]).all()
    assert (r["stats"]["cells_bridged"], r["stats"]["cells_open"], r["stats"]["cells_none"]) == (1, 0, 3)


# ---- conditions of the GPU test ----------------------------------------------------------------------------------------------

def test_planes_ties_across_a_and_two_equidistant_b():
    c = GR.case("planes")
    g = GR.reference("planes")[0][0]
    A, B = np.flatnonzero(c["side"] == 1), np.flatnonzero(c["side"] == 2)
    d2 = GR.d2_exact(c["xyz"], A[:, None], B[None, :])
    assert d2.min() == c["d2"] == g["gap2"] == 10.5625
    at_min = d2 == d2.min()
    assert at_min.any(axis=1).sum() == 36                          # every a attains it ...
    assert g["site_left"] == A.min() and at_min[0].sum() == 2      # ... the smallest a with two b
    assert g["site_right"] == B[at_min[0]].min() and g["site_right"] != B[at_min[0]].max()
    coords, nc = GR.index_coords(c)
    assert nc.prod() >= 16                                         # the planes spread over many index cells ...
    assert tuple(coords[g["site_left"]]) != tuple(coords[A].min(axis=0))      # ... and the winner is not in the first


def test_straddle_covers_the_27_relations():
    c = GR.case("straddle")
    gaps, stats = GR.reference("straddle")
    coords, nc = GR.index_coords(c)
    seen = set()
    for g, (a, b, d2) in enumerate(c["pairs"]):
        assert (gaps[g]["site_left"], gaps[g]["site_right"], gaps[g]["gap2"]) == (a, b, d2)
        rel = tuple((coords[b] - coords[a]).tolist())
        assert rel == GR.RELATIONS[g]
        seen.add(rel)
        assert gaps[g]["n_left"] == 2 and gaps[g]["n_right"] == 2
    assert len(seen) == 27 and stats["cells_open"] == 27


def test_rim_is_counted_at_r_max_and_not_below():
    g = GR.reference("rim")[0][0]
    assert (g["gap2"], g["gap"], g["site_left"], g["site_right"]) == (25.0, 5.0, 0, 1)
    g = GR.reference("rim_below")[0][0]
    assert g["site_left"] == -1 and np.isinf(g["gap2"])
    c = GR.case("rim")
    assert c["r_max"] * 3 == c["cutoff"] and GR.case("rim_below")["r_max"] < 5.0
    coords, nc = GR.index_coords(c)
    B = np.flatnonzero(c["side"] == 2)
    assert (np.abs(coords[B] - coords[0]).max(axis=1) <= 1).all() and len(B) == 7      # candidates of the 27 cells, one within r_max
    assert (GR.d2_exact(c["xyz"], 0, B) > 25.0).sum() == 6


def test_mixed_holds_every_kind_of_cell():
    c = GR.case("mixed")
    gaps, stats = GR.reference("mixed")
    print("mixed:", stats)
    assert stats["cells_open"] >= 100 and stats["cells_none"] >= 20 and stats["cells_bridged"] >= 5
    assert stats["cells_open"] + stats["cells_none"] + stats["cells_bridged"] == c["n_cells"] == 1000
    assert ((gaps["n_left"] == 0) & (gaps["n_right"] > 0)).sum() >= 5 and ((gaps["n_right"] == 0) & (gaps["n_left"] > 0)).sum() >= 5
    cell = c["cell"]
    assert (cell == -1).sum() >= 100 and (cell >= 1000).sum() >= 100 and ((c["side"] & 3) == 3).sum() >= 5
    assert (c["side"] > 3).sum() >= 100
    assert GR.index_coords(c)[1].tolist() == [8, 8, 8]


def test_dense_fills_one_index_cell():
    c = GR.case("dense")
    coords, nc = GR.index_coords(c)
    member = c["side"] != 0
    assert (coords[member] == 0).all() and nc.tolist() == [3, 3, 3]
    assert (c["side"] == 2).sum() == 3000 and (c["side"] == 1).sum() == 600       # > 256 lanes' strides; > 16 A sites per block
    gaps, stats = GR.reference("dense")
    assert stats["cells_open"] == 3 and (gaps["gap2"] > 0).all()


def test_large_members_sit_at_the_two_ends_of_263_tiles_and_the_planted_pair_wins():
    c = GR.case("large")
    tile = GR.index_positions(c) // GR.SK.SCAN_TILE
    N = len(c["xyz"])
    assert N == 537840 and tile.max() == 262 and c["cutoff"] == c["r_max"] == 20.0
    for bit in (1, 2):                                             # A, B: per-tile counts as the compaction forms them
        cnt = np.bincount(tile[(c["side"] & bit) != 0], minlength=263)
        print("set %d: first tile %d, tiles 1..255 %d, tiles 256..262 %s" % (bit, cnt[0], cnt[1:256].sum(), cnt[256:].tolist()))
        assert cnt[0] >= 8 and cnt[1:256].sum() == 0 and (cnt[256:] >= 100).all()
    a, b, d2 = c["pair"]
    assert tile[a] == 262 and tile[b] == 262 and c["side"][a] == 1 and c["side"][b] == 2
    assert 0.0899 < d2 < 0.0901 and d2 == GR.d2_exact(c["xyz"], a, b)
    # no two other members come near that: the lattice leaves 4 - 0.6 A between any two sites, and b lies 0.3 A from one
    others = np.setdiff1d(np.flatnonzero(c["side"]), [b])
    d, _ = GR.cKDTree(c["xyz"][others]).query(c["xyz"][others], k=2)
    assert d[:, 1].min() >= 3.4
    assert np.sort(GR.cKDTree(c["xyz"][others]).query(c["xyz"][b], k=2)[0])[1] >= 3.1
    gaps, stats = GR.reference("large")
    g = gaps[0]
    assert (g["site_left"], g["site_right"], g["gap2"]) == (a, b, d2) and g["bridged"] == 0
    assert (g["x_left"], g["x_right"]) == (c["xyz"][a, 0], c["xyz"][b, 0])
    assert stats["cells_open"] == 1 and stats["n_both"] == 0
    assert stats["n_left"] == int((c["side"] == 1).sum()) and stats["n_right"] == int((c["side"] == 2).sum())
    assert 3000 <= stats["n_left"] <= 6000 and 3000 <= stats["n_right"] <= 6000


def test_large_two_has_a_record_that_depends_on_the_carry_of_the_scan():
    """`large` itself cannot tell a lost carry: its pair lies in the last tile, and without the carry every list position
    from tile 256 on moves down by the same amount.  `large_two` can: shown here on the step-by-step restatement of the
    device's compaction and search, first intact (it gives the restatement's records), then with every pass of the scan
    starting from 0, for either survivor of the two writes that then meet in one list slot."""
    c = GR.case("large_two")
    T = GR.SK.SCAN_TILE
    pos = GR.index_positions(c)
    tile = pos // T
    (a0, b0, d0), (a1, b1, d1) = c["pairs"]
    assert tile.max() == 262 and c["n_cells"] == 2 and np.array_equal(c["cell"], (tile >= 256).astype(np.int32))
    cnt = {bit: np.bincount(tile[(c["side"] & bit) != 0], minlength=263) for bit in (1, 2)}
    for bit in (1, 2):
        print("set %d: first tile %d, tiles 256..262 %s" % (bit, cnt[bit][0], cnt[bit][256:].tolist()))
        assert cnt[bit][0] >= 8 and cnt[bit][1:256].sum() == 0 and (cnt[bit][256:] >= 100).all()
    assert tile[a0] == 0 and tile[b0] == 0 and tile[a1] == 256 and tile[b1] == 256
    # the planted sites of cell 1 are among the first members of tile 256: as many as the first tile holds
    for site, bit in ((a1, 1), (b1, 2)):
        rank = int(((tile == 256) & ((c["side"] & bit) != 0) & (pos < pos[site])).sum())
        assert rank < cnt[bit][0], (rank, cnt[bit][0])
    assert 0.0899 < d0 < 0.0901 and 0.0899 < d1 < 0.0901
    gaps, stats = GR.reference("large_two")
    want = [(a0, b0, d0), (a1, b1, d1)]
    assert [(g["site_left"], g["site_right"], g["gap2"]) for g in gaps] == want and stats["cells_open"] == 2
    assert GR.device_search(c) == want
    for later in (True, False):
        broken = GR.device_search(c, carry=False, later_write_stays=later)
        print("scan without its carry, %s write stays:" % ("later" if later else "earlier"), broken)
        assert broken != want
        assert (broken[0] != want[0]) if later else (broken[1] != want[1])   # the cell whose members were overwritten


@pytest.mark.parametrize("N", GR.SK.TILE_EDGE_SIZES)
def test_tile_edge_answer_hangs_on_the_last_item_of_the_scan(N):
    c = GR.case("tile_edge@%d" % N)
    T = GR.SK.SCAN_TILE
    pos = GR.index_positions(c)
    a, b, d2 = c["pair"]
    assert len(c["xyz"]) == N and N in (T - 1, T, T + 1) and c["cutoff"] == c["r_max"] == 20.0
    assert pos[b] == N - 1 and c["side"][b] == 2 and c["side"][a] == 1
    assert 0.1199 < d2 < 0.1201 and d2 == GR.d2_exact(c["xyz"], a, b)
    # no two other sites come near that: the lattice leaves 4 - 0.6 A between any two, and a lies 0.35 A from one
    others = np.setdiff1d(np.arange(N), [a])
    assert GR.cKDTree(c["xyz"][others]).query(c["xyz"][others], k=2)[0][:, 1].min() >= 3.4
    for bit in (1, 2):
        assert ((c["side"] & bit) != 0).sum() >= 500
    gaps, stats = GR.reference(c["name"])
    g = gaps[0]
    assert (g["site_left"], g["site_right"], g["gap2"]) == (a, b, d2) and stats["cells_open"] == 1 and stats["n_both"] == 0
    assert GR.device_search(c) == [(a, b, d2)]
    # ... and without the last item the answer is another pair, farther apart
    lost = dict(c, side=np.where(np.arange(N) == b, 0, c["side"]))
    (a2, b2, d22), = GR.device_search(lost)
    assert b2 != b and d22 > 9.0


# ---- struct layout and argument errors ---------------------------------------------------------------------------------------

def test_python_struct_layout(km):
    assert C.sizeof(km.lib.Gap) == 56 == GR.GAP_DTYPE.itemsize == km.solvers.GAP_DTYPE.itemsize
    assert GR.GAP_DTYPE == km.solvers.GAP_DTYPE
    assert [n for n, _ in km.lib.Gap._fields_] == list(GR.GAP_DTYPE.names)
    assert [n for n, _ in km.lib.GapStats._fields_][:6] == list(GR.STAT_KEYS)


ERR_ARG = -1


def _set_args():
    """Well-formed arguments apart from the NULL index.  The device pointers are never dereferenced."""
    fake = C.c_void_p(64)
    return dict(p=None, d_x=fake, d_y=fake, d_z=fake, d_site_side=fake, r_max=5.0, d_site_cell=fake, n_cells=4, h_gaps=True,
                stats=None)


def _fil_args():
    fake = C.c_void_p(64)
    return dict(p=None, nn=52, d_neigh_idx=fake, d_site_element=fake, d_site_charge=fake, d_metals=fake, num_metals=2, d_x=fake,
                d_y=fake, d_z=fake, N_left_tot=10, N_right_tot=10, r_max=5.0, d_site_cell=fake, n_cells=4, h_gaps=True, n_bins=0,
                x_lo=0.0, x_hi=0.0, h_profile=None, d_site_side=None, stats=None)


COMMON = [(dict(), b"p is NULL"), (dict(d_x=None), b"d_x"), (dict(d_y=None), b"d_y"), (dict(d_z=None), b"d_z"),
          (dict(h_gaps=None), b"h_gaps"), (dict(r_max=float("nan")), b"r_max"), (dict(r_max=float("inf")), b"r_max"),
          (dict(r_max=0.0), b"r_max"), (dict(r_max=-1.0), b"r_max"), (dict(n_cells=0), b"n_cells"),
          (dict(d_site_cell=None), b"d_site_cell"), (dict(d_site_cell=None, n_cells=1), b"p is NULL")]


def _call(km, fn, a):
    lib = km.lib.load()
    gaps = (km.lib.Gap * 4)()
    prof = (C.c_int * 64)()
    a = dict(a)
    a["h_gaps"] = gaps if a["h_gaps"] is True else None
    if a.get("h_profile") is True:
        a["h_profile"] = prof
    rc = getattr(lib, fn)(*a.values())
    return rc, lib.kmcf_last_error()


@pytest.mark.parametrize("change,word", COMMON + [(dict(d_site_side=None), b"d_site_side")])
def test_site_set_gap_argument_errors_without_an_index(km, change, word):
    a = _set_args()
    a.update(change)
    rc, msg = _call(km, "kmcf_site_set_gap", a)
    assert rc == ERR_ARG and word in msg and b"kmcf_site_set_gap" in msg, (rc, msg)


@pytest.mark.parametrize("change,word", COMMON + [
    (dict(d_neigh_idx=None), b"d_neigh_idx"), (dict(d_site_element=None), b"d_site_element"),
    (dict(d_site_charge=None), b"d_site_charge"), (dict(nn=0), b"nn = 0"), (dict(num_metals=-1), b"num_metals"),
    (dict(d_metals=None), b"d_metals"), (dict(N_left_tot=-1), b"N_left_tot"), (dict(N_right_tot=-2), b"N_right_tot"),
    (dict(n_bins=-1), b"n_bins"), (dict(h_profile=True), b"h_profile"),
    (dict(h_profile=True, n_bins=8, x_lo=1.0, x_hi=1.0), b"x_hi"), (dict(h_profile=True, n_bins=8, x_lo=0.0, x_hi=1.0), b"p is NULL"),
    (dict(n_bins=8), b"p is NULL")])
def test_filament_gap_argument_errors_without_an_index(km, change, word):
    a = _fil_args()
    a.update(change)
    rc, msg = _call(km, "kmcf_filament_gap", a)
    assert rc == ERR_ARG and word in msg and b"kmcf_filament_gap" in msg, (rc, msg)
