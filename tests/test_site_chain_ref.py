"""CPU: the restatement of tests/site_chain_ref.py against answers known by construction, the conditions that make each
synthetic case what its name says, and Boruvka's rounds with the device's early stop against Kruskal's hop list."""
import numpy as np
import pytest

import site_chain_ref as R


def _paths(name):
    c, r = R.case(name), R.reference(name)
    known = c["hops"] if c["n_cells"] > 1 else [c["hops"]]
    return c, r, known


@pytest.mark.parametrize("name", ["ladder", "detour", "rim", "rim_below", "straddle", "home", "home_flipped", "large",
                                  "tile_edge@2047", "tile_edge@2048", "tile_edge@2049"])
def test_known_chains(name):
    c, r, known = _paths(name)
    assert len(known) == c["n_cells"]
    for k, (want, got) in enumerate(zip(known, r["paths"])):
        rec = r["chains"][k]
        if want is None:
            assert got is None and rec["status"] == R.OPEN and rec["n_hops"] == 0 and np.isinf(rec["hop_max2"])
            assert (rec["neck_from"], rec["neck_to"], rec["length"]) == (-1, -1, 0.0)
            continue
        assert [tuple(h) for h in got] == [tuple(h) for h in want], k
        assert rec["status"] == R.CHAINED and rec["n_hops"] == len(want)
        assert rec["hop_max2"] == max(h[2] for h in want) and rec["hop_max"] == np.sqrt(rec["hop_max2"])
        assert abs(rec["length"] - sum(np.sqrt(h[2]) for h in want)) <= 1e-12 * rec["length"]
        listed = r["hops"][k][:len(want)]
        assert [tuple(h) for h in listed.tolist()] == [tuple(h) for h in want[:c["max_hops"]]]
        assert (r["hops"][k][len(want):]["from"] == -1).all() and np.isinf(r["hops"][k][len(want):]["d2"]).all()


def test_ladder_and_detour_numbers():
    lad, det = R.reference("ladder")["chains"][0], R.reference("detour")["chains"][0]
    assert lad["n_hops"] == 4 and lad["hop_max2"] == 9.0 and np.isinf(lad["direct2"]) and lad["length"] == 12.0
    assert (lad["n_left"], lad["n_right"], lad["n_stones"], lad["n_stone_sites"]) == (1, 1, 8, 8)
    assert det["n_hops"] == 3 and det["hop_max2"] == 12.25 and det["direct2"] == 25.0 and det["length"] == 9.5
    assert R.case("detour")["r_max"] ** 2 == det["direct2"]                     # the direct link lies on the rim and counts


def test_rim_closes_and_opens():
    rim, below = R.reference("rim"), R.reference("rim_below")
    assert rim["chains"][0]["status"] == R.CHAINED and rim["chains"][0]["hop_max2"] == 25.0 == R.case("rim")["r_max"] ** 2
    assert below["chains"][0]["status"] == R.OPEN and R.case("rim_below")["r_max"] < 5.0
    assert below["stats"]["surface_sites"] == rim["stats"]["surface_sites"] - 1  # r0 has lost its only partner


def test_ties_many_links_at_the_bottleneck():
    c, r = R.case("ties"), R.reference("ties")
    rec = r["chains"][0]
    assert rec["status"] == R.CHAINED and rec["hop_max2"] == 1.0 and rec["n_hops"] >= 5
    side, own, stone, vcell = R.vertices(c["side"], c["node"], c["cell"], 1)
    sites = np.flatnonzero(vcell == 0)
    vid = np.where(stone[sites], c["node"][sites], np.where(side[sites] == 1, R.V_LEFT, R.V_RIGHT))
    links, _ = R.cell_links(c["xyz"], sites, vid, c["r_max"])
    assert int((links[0] == rec["hop_max2"]).sum()) >= 10
    assert all(h[2] == 1.0 for h in r["paths"][0])
    neck = max(r["paths"][0], key=lambda h: (min(h[0], h[1]), max(h[0], h[1])))
    assert (rec["neck_from"], rec["neck_to"]) == neck[:2]


def test_straddle_covers_the_27_relations():
    c = R.case("straddle")
    coords, _ = R.GR.index_coords(c)
    seen = set()
    for (a, m, _), (_, b, _) in c["hops"]:
        rel = tuple(int(v) for v in coords[m] - coords[a])
        assert tuple(int(v) for v in coords[b] - coords[a]) == rel
        seen.add(rel)
    assert seen == set(R.GR.RELATIONS)


def test_home_decides_the_cell():
    for name, cell in (("home", 0), ("home_flipped", 1)):
        rec = R.reference(name)["chains"]
        assert rec["status"].tolist() == ([R.CHAINED, R.OPEN] if cell == 0 else [R.OPEN, R.CHAINED])
        assert rec["n_stones"][cell] == 1 and rec["n_stone_sites"][cell] == 2 and rec["n_stones"][1 - cell] == 0
        assert rec["n_stone_sites"][1 - cell] == 0


def test_multi_site_links_are_not_at_the_smallest_ids():
    c, r = R.case("multi_site"), R.reference("multi_site")
    path = r["paths"][0]
    assert len(path) == 13 and r["chains"][0]["n_stones"] == 12 and r["chains"][0]["n_stone_sites"] == 196
    sizes = np.bincount(c["node"][c["node"] >= 0])
    assert sizes[sizes > 0].min() == 2 and sizes.max() == 40
    ends = [s for h in path for s in h[:2] if c["side"][s] == 0]
    assert sum(s >= 12 for s in ends) >= len(ends) - 4                          # the homes are the ids below 12


def test_zigzag_is_long_and_takes_rounds():
    c, r = R.case("zigzag"), R.reference("zigzag")
    rec = r["chains"][0]
    assert rec["n_hops"] == 601 and rec["hop_max2"] == 4.0 + 0.7 * 0.7 and abs(rec["hop_max2"] - 4.49) < 1e-12
    assert r["paths"][0][0][2] == 4.0 and r["rounds"][0] >= 4
    assert c["max_hops"] == 16 and (r["hops"][0]["from"] >= 0).all()


def test_statuses_all_occur():
    c, r = R.case("statuses"), R.reference("statuses")
    assert r["chains"]["status"].tolist() == c["status"] and r["chains"]["n_hops"].tolist() == c["n_hops"]
    assert set(c["status"]) == {R.NONE, R.OPEN, R.CHAINED, R.BRIDGED}
    b = r["chains"][3]
    assert (b["hop_max"], b["hop_max2"], b["direct2"], b["length"], b["neck_from"]) == (0.0, 0.0, 0.0, 0.0, -1)
    assert r["chains"][5]["direct2"] == 12.25 == r["chains"][5]["hop_max2"]
    assert r["chains"]["n_stones"].tolist() == [1, 1, 2, 1, 1, 0] and r["chains"]["n_stone_sites"].tolist() == [1, 1, 2, 1, 2, 0]
    assert (c["side"] > 3).sum() >= 4 and ((c["node"] >= len(c["xyz"])) | (c["node"] < -1)).sum() == 2
    assert ((c["cell"] < 0) | (c["cell"] >= c["n_cells"])).sum() == 4


def test_mixed_is_mixed():
    c, r = R.case("mixed"), R.reference("mixed")
    st = r["stats"]
    for k in ("cells_open", "cells_chained", "cells_bridged"):
        assert st[k] >= 0.1 * c["n_cells"], (k, st[k])
    assert r["chains"]["n_hops"].max() >= 8
    side, own, stone, vcell = R.vertices(c["side"], c["node"], c["cell"], c["n_cells"])
    assert int((stone & (vcell != own)).sum()) > 0
    chained = r["chains"]["status"] == R.CHAINED
    assert (r["chains"]["hop_max2"][chained] <= r["chains"]["direct2"][chained]).all()


def test_large_members_sit_at_both_ends_of_the_scan():
    c = R.case("large")
    side, own, stone, vcell = R.vertices(c["side"], c["node"], c["cell"], c["n_cells"])
    pos = R.GR.index_positions(c)[vcell >= 0]
    T = R.SK.SCAN_TILE
    assert (pos < T).sum() >= 20 and (pos >= 256 * T).sum() >= 1000
    between = (pos >= T) & (pos < 256 * T)
    assert between.sum() <= 3                                                   # (planted sites that moved into a later index cell)
    assert R.reference("large")["stats"]["surface_sites"] > 1000


@pytest.mark.parametrize("N", R.SK.TILE_EDGE_SIZES)
def test_tile_edge_chain_needs_the_last_item_of_the_scan(N):
    c, ref = R.case("tile_edge@%d" % N), R.reference("tile_edge@%d" % N)
    (l, s, d_ls), (s2, r, d_sr) = c["hops"]
    assert len(c["xyz"]) == N and N in (R.SK.SCAN_TILE - 1, R.SK.SCAN_TILE, R.SK.SCAN_TILE + 1) and s == s2
    assert R.GR.index_positions(c)[s] == N - 1 and c["node"][s] == 200 and (c["node"] == 200).sum() == 1
    assert (c["side"][l], c["side"][s], c["side"][r]) == (1, 0, 2)
    assert d_ls <= 0.25 and d_sr <= 0.25 and R.d2_exact(c["xyz"], l, r) > 0.25
    # no two other sites come near: the lattice leaves 4 - 0.6 A between any two
    others = np.setdiff1d(np.arange(N), [l, r])
    assert R.cKDTree(c["xyz"][others]).query(c["xyz"][others], k=2)[0][:, 1].min() >= 3.4
    for kind in (c["side"] == 1, c["side"] == 2, c["node"] >= 0):
        assert kind.sum() >= 400
    rec = ref["chains"][0]
    assert rec["status"] == R.CHAINED and rec["n_hops"] == 2 and np.isinf(rec["direct2"])
    assert ref["stats"]["surface_sites"] == 3
    # ... and without the stone at the last position there is no chain
    lost = R.site_set_chain(c["xyz"], c["side"], np.where(np.arange(N) == s, -1, c["node"]), c["r_max"], max_hops=4)
    assert lost["chains"][0]["status"] == R.OPEN


def test_boruvka_with_the_early_stop_returns_kruskals_hops():
    """random one-cell problems, a third of them on integer lattices (many tied d2): the same hop list"""
    rng = np.random.default_rng(1)
    total = chained = most_rounds = 0
    for trial in range(300):
        N = int(rng.integers(50, 400))
        xyz = rng.uniform(0, 20, (N, 3))
        if trial % 3 == 0:
            xyz = np.round(xyz)
        side = np.zeros(N, np.int64)
        side[xyz[:, 0] < 3] = 1
        side[xyz[:, 0] > 17] = 2
        node = np.where(rng.random(N) < 0.5, rng.integers(0, N, N) // 3 * 3, -1)
        cell = (xyz[:, 1] > 10).astype(np.int64)
        r = R.site_set_chain(xyz, side, node, float(rng.choice([2.5, 3.5, 5.0])), cell, 2, boruvka=True)   # (asserts equality)
        total += len(r["rounds"])
        chained += int((r["chains"]["status"] == R.CHAINED).sum())
        most_rounds = max([most_rounds] + r["rounds"])
    print(total, "problems,", chained, "chained, at most", most_rounds, "rounds")
    assert total >= 500 and chained >= 100 and most_rounds <= 40
