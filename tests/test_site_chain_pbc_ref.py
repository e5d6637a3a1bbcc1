"""CPU: the restatement of the periodic tunnelling chain (tests/site_chain_pbc_ref.py) and the conditions that keep the GPU
test (tests/test_gpu_site_chain_pbc.py) meaningful -- every input does what it was built for --; Boruvka's rounds under the
minimum image return Kruskal's hops; the pair distance is the same from both ends; the two new symbols and `periodic=`."""
import inspect
import os
import re

import numpy as np
import pytest

import pbc_ref as P
import site_chain_pbc_ref as CP
import site_chain_ref as R
import site_gap_pbc_ref as GP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN_CASES = ["ladder", "detour", "rim", "rim_below", "ties", "straddle", "home", "home_flipped", "multi_site", "zigzag",
              "statuses", "mixed", "large"]


# ---- symbols ---------------------------------------------------------------------------------------------------------------------

def test_the_two_symbols_are_exported_with_the_headers_signatures(km):
    lib = km.lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmcfield.h")).read(), flags=re.S)
    for name in ("kmcf_site_set_chain", "kmcf_filament_chain"):
        decl, decl_pbc = (re.search(r"int\s+%s\s*\(([^)]*)\)" % n, hdr) for n in (name, name + "_pbc"))
        assert decl and decl_pbc, name
        assert re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", decl_pbc.group(1))      # the parameter list of its counterpart
        res, args = km.lib.SIGNATURES[name + "_pbc"]
        assert (res, args) == km.lib.SIGNATURES[name] and len(args) == decl_pbc.group(1).count(",") + 1
        assert hasattr(lib, name + "_pbc")


def test_the_python_calls_accept_periodic(km):
    for f in (km.solvers.site_set_chain, km.solvers.filament_chain):
        p = inspect.signature(f).parameters
        assert "periodic" in p and p["periodic"].default is False, f.__name__


def test_no_document_calls_the_periodic_chain_a_later_change():
    for name in ("include/kmcfield.h", "README.md", "INTEGRATION.md", "DESIGN.md", "tools/kmc_loop.py"):
        text = re.sub(r"\s+", " ", open(os.path.join(ROOT, name)).read())
        for phrase in ("periodic form is a later change", "the search is non-periodic", "chain search is non-periodic and refuses"):
            assert phrase not in text, (name, phrase)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", OPEN_CASES)
def test_without_a_lattice_it_is_the_open_restatement(name):
    c, ref = R.case(name), R.reference(name)
    got = CP.site_set_chain(c["xyz"], c["side"], c["node"], c["r_max"], c["cell"], c["n_cells"], c["max_hops"], L=None)
    assert got["chains"].tobytes() == ref["chains"].tobytes() and got["hops"].tobytes() == ref["hops"].tobytes()
    assert got["stats"] == ref["stats"] and got["paths"] == ref["paths"]


def _all_candidates():
    for name in CP.SEARCH_CASES:
        c = CP.case(name)
        yield (name, c) + CP.candidates_of(c)


def test_the_distance_is_the_same_bits_from_both_ends():
    total = wrapped = 0
    for name, c, a, b in _all_candidates():
        ab, ba = CP.d2_exact(c["xyz"], a, b, c["L"]), CP.d2_exact(c["xyz"], b, a, c["L"])
        assert ab.tobytes() == ba.tobytes(), name
        assert len(np.unique(a * len(c["xyz"]) + b)) == len(a), name             # one pair, one row
        total += len(a)
        wrapped += int(((CP.fold(c["xyz"][a, 1], c["xyz"][b, 1], c["L"][1])[1] != 0)
                        | (CP.fold(c["xyz"][a, 2], c["xyz"][b, 2], c["L"][2])[1] != 0)).sum())
    print("candidate pairs", total, "of them through a face", wrapped)
    assert total >= 10000 and wrapped >= 1000


def test_candidates_hold_every_counting_pair():
    """all pairs of a small input against the tree's proposals"""
    for name in ("p11@20", "second_image", "self_image", "one_cell", "half"):
        c = CP.case(name)
        for _, sites, vid in CP.cell_members(c["side"], c["node"], c["cell"], c["n_cells"]):
            a, b = np.meshgrid(sites, sites, indexing="ij")
            va, vb = np.meshgrid(vid, vid, indexing="ij")
            ok = (a < b) & (va != vb) & (CP.d2_exact(c["xyz"], a, b, c["L"]) <= c["r_max"] ** 2)
            want = set(zip(a[ok].tolist(), b[ok].tolist()))
            pa, pb = CP.candidate_pairs(c["xyz"], sites, vid, c["r_max"], c["L"])
            got = set(zip(np.minimum(pa, pb).tolist(), np.maximum(pa, pb).tolist()))
            assert want <= got, name


# ---- Boruvka under the minimum image -----------------------------------------------------------------------------------------------

def test_boruvka_under_the_lattice_returns_kruskals_hops():
    rng = np.random.default_rng(4100)
    L = np.array([16.0, 16.0, 16.0])
    most, chained, through = 0, 0, 0
    for k in range(330):
        n = int(rng.integers(20, 90))
        if k % 3 == 0:                                                          # an integer lattice: ties everywhere
            xyz = rng.integers(0, 16, (n, 3)).astype(np.float64)
            r_max = float(rng.choice([2.0, 3.0, 4.0]))
        else:
            xyz = rng.random((n, 3)) * L
            r_max = float(rng.uniform(2.5, 6.0))
        kind = rng.choice(3, n, p=[0.8, 0.1, 0.1])
        kind[:2] = [1, 2]
        sites = np.arange(n)
        vid = np.where(kind == 1, CP.V_LEFT, np.where(kind == 2, CP.V_RIGHT, rng.integers(0, n, n)))
        links, _ = CP.cell_links(xyz, sites, vid, r_max, L)
        want = CP.kruskal_path(links)
        got, rounds = CP.boruvka_path(links)
        assert got == want and rounds <= 40, k
        most = max(most, rounds)
        if want:
            chained += 1
            through += any(CP.crossings(xyz, a, b, L) != (0, 0) for a, b, _ in want)
    print("330 problems: %d chained, %d with a hop through a face, at most %d rounds" % (chained, through, most))
    assert chained >= 100 and through >= 30


# ---- random inputs ---------------------------------------------------------------------------------------------------------------------

def _listed_crossings(c, ref):
    ny = nz = 0
    for h in ref["hops"].reshape(-1):
        if h["from"] >= 0:
            cy, cz = CP.crossings(c["xyz"], h["from"], h["to"], c["L"])
            ny, nz = ny + (cy != 0), nz + (cz != 0)
    return ny, nz


@pytest.mark.parametrize("name", [n for n in CP.SEARCH_CASES if "@" in n])
def test_random_cases_hold_what_they_are_built_for(name):
    c, ref, opn = CP.case(name), CP.reference(name), CP.reference(name, periodic=False)
    base = name.split("@")[0]
    N, st = len(c["xyz"]), ref["stats"]
    differ = int(sum(ref["chains"][k].tobytes() != opn["chains"][k].tobytes() for k in range(c["n_cells"])))
    ny, nz = _listed_crossings(c, ref)
    faces = CP.stones_through_a_face(c)
    print("%s: %d sites, %d gap cells, index cells %s; %s; %d records differ from open boundaries, listed hops through y %d, "
          "through z %d, %d stones through a face, rounds %d, longest chain %d hops"
          % (name, N, c["n_cells"], GP.index_coords(c)[1].tolist(), st, differ, ny, nz, len(faces), max(ref["rounds"]),
             ref["chains"]["n_hops"].max()))
    assert c["r_max"] in (20.0, 12.0) and c["r_max"] <= c["cutoff"] == 20.0 and c["max_hops"] == 8
    assert tuple(GP.index_coords(c)[1][1:]) == P.pairwise_case(base)["cells"]
    assert abs(((c["side"] & 3) == 3).mean() - 0.02) < 0.01
    assert (c["cell"] == -1).sum() >= 1 and (c["cell"] == c["n_cells"]).sum() >= 1
    for k in ("cells_none", "cells_open", "cells_chained", "cells_bridged"):
        assert st[k] >= 1, k
    assert differ >= 5
    searched = np.isin(ref["chains"]["status"], (CP.OPEN, CP.CHAINED))
    assert np.isinf(ref["chains"]["direct2"][searched]).any() and np.isfinite(ref["chains"]["direct2"][searched]).any()
    assert ny >= 3 and nz >= 3
    assert len(faces) >= 1
    assert max(ref["rounds"]) >= 2
    if c["r_max"] == CP.R_MAX:
        assert (ref["chains"]["n_hops"] >= 2).sum() >= 5


# ---- constructed cases: the answers hold by construction ----------------------------------------------------------------------------

def _known(name):
    c, ref = CP.case(name), CP.reference(name)
    for k, want in enumerate(c["hops"]):
        assert ref["paths"][k] == want, (name, k, ref["paths"][k], want)
        assert ref["chains"][k]["status"] == (CP.OPEN if want is None else CP.CHAINED)
    return c, ref, CP.reference(name, periodic=False)


def test_wrap_ladder_is_chained_only_under_the_lattice():
    c, ref, opn = _known("wrap_ladder")
    assert ref["chains"][0]["n_hops"] == 3 and opn["chains"][0]["status"] == CP.OPEN
    assert [CP.crossings(c["xyz"], a, b, c["L"])[0] != 0 for a, b, _ in c["hops"][0]] == [False, True, False]
    ys = sorted(c["xyz"][[h[0] for h in c["hops"][0]] + [c["hops"][0][-1][1]], 1])
    assert ys == [0.25, 1.0, 62.75, 63.5]


def test_corner_hop_crosses_both_faces():
    c, ref, opn = _known("corner")
    assert CP.crossings(c["xyz"], 0, 1, c["L"]) == (-1, -1) and ref["chains"][0]["hop_max2"] == 17.0
    assert ref["chains"][0]["direct2"] == 38.0 and opn["chains"][0]["status"] == CP.OPEN
    coords, nc = GP.index_coords(c)
    assert tuple(nc[1:]) == (4, 4) and tuple(coords[0][1:]) == (0, 0) and tuple(coords[1][1:]) == (3, 3)


def test_wrap_detour_takes_the_stones_beyond_the_face():
    c, ref, opn = _known("wrap_detour")
    r = ref["chains"][0]
    assert (r["hop_max2"], r["direct2"], r["n_hops"]) == (12.25, 25.0, 3) and c["r_max"] ** 2 == 25.0
    assert CP.crossings(c["xyz"], *c["hops"][0][0][:2], c["L"])[0] != 0
    o = opn["chains"][0]
    assert (o["n_hops"], o["hop_max2"], o["direct2"]) == (1, 25.0, 25.0)          # without the wrap: the direct link


def test_rim_wrap_closes_at_r_max_and_not_below():
    c, ref, opn = _known("rim_wrap")
    assert ref["chains"][0]["hop_max2"] == 25.0 == c["r_max"] ** 2 and CP.crossings(c["xyz"], 2, 3, c["L"]) == (-1, 0)
    assert opn["chains"][0]["status"] == CP.OPEN
    below, _, _ = _known("rim_wrap_below")
    assert below["r_max"] < 5.0 and np.array_equal(below["xyz"], c["xyz"]) and CP.reference("rim_wrap_below")["stats"]["cells_open"] == 1


def test_half_a_period_rounds_away_from_zero_from_both_ends():
    c, ref, _ = _known("half")
    xyz, L = c["xyz"], c["L"]
    assert GP.index_coords(c)[1][1] == 1 and L[1] == 25.0
    for (a, b), f in (((0, 1), 0.5), ((3, 4), -0.5)):
        assert (xyz[a, 1] - xyz[b, 1]) / L[1] == f and (xyz[b, 1] - xyz[a, 1]) / L[1] == -f
        assert CP.fold(xyz[a, 1], xyz[b, 1], L[1])[0] == -f * L[1] and CP.fold(xyz[b, 1], xyz[a, 1], L[1])[0] == f * L[1]
        assert CP.d2_exact(xyz, a, b, L) == CP.d2_exact(xyz, b, a, L) == 156.25
    assert ref["chains"]["hop_max2"].tolist() == [156.25, 156.25] and np.isinf(ref["chains"]["direct2"]).all()


def test_second_image_adds_no_link_and_no_mark():
    c, ref, opn = _known("second_image")
    assert c["L"][1] < 2 * c["r_max"] and GP.index_coords(c)[1][1] == 1
    assert R.d2_exact(c["xyz"], 0, 1) == 121.0 <= c["r_max"] ** 2                # both images of the stone within r_max of L
    assert len(ref["links"][0][0]) == 3 and ref["stats"]["surface_sites"] == 3 and ref["chains"][0]["n_stones"] == 1
    assert ref["chains"][0]["hop_max2"] == 25.0 and ref["chains"][0]["direct2"] == 41.0
    assert opn["chains"][0]["hop_max2"] == 121.0


def test_self_image_is_no_link():
    c, ref, _ = _known("self_image")
    assert c["L"][1] == c["r_max"] == 16.0
    assert CP.d2_exact(c["xyz"], 2, 3, c["L"]) == 16.0 and c["node"][2] == c["node"][3]      # one stone, 4 apart through the face
    links = ref["links"][0]
    assert (links[3] != links[4]).all() and len(links[0]) == 5                   # L-s, t-R, s-t, L-t, s-R
    assert ref["chains"][0]["n_stones"] == 2 and ref["chains"][0]["n_stone_sites"] == 3 and ref["stats"]["surface_sites"] == 5


def test_ties_wrap_every_link_has_one_d2():
    c, ref = CP.case("ties_wrap"), CP.reference("ties_wrap")
    d2, a, b = ref["links"][0][:3]
    assert (d2 == 16.0).all() and len(d2) >= 2000
    through = sum(CP.crossings(c["xyz"], i, j, c["L"]) != (0, 0) for i, j in zip(a.tolist(), b.tolist()))
    assert through >= 50
    r = ref["chains"][0]
    assert r["status"] == CP.CHAINED and r["n_hops"] >= 4 and r["hop_max2"] == 16.0 and np.isinf(r["direct2"])
    assert max(ref["rounds"]) >= 2


def test_two_cells_inner_and_outer_face():
    c, ref, opn = _known("two_cells")
    coords, nc = GP.index_coords(c)
    assert nc[1] == 2 and c["L"][1] / 2 >= c["cutoff"]
    for g, crossed in ((0, 0), (1, -1)):
        a, b, d2 = c["hops"][g][0]
        assert coords[a][1] == 0 and coords[b][1] == 1 and CP.crossings(c["xyz"], a, b, c["L"])[0] == crossed
        ya = c["xyz"][a, 1]
        assert max(ya - 0.0, 16.0 - ya) > c["r_max"] > np.sqrt(d2)             # the face the hop does NOT pass is out of reach
    assert opn["chains"][0]["n_hops"] == 2 and opn["chains"][1]["status"] == CP.OPEN      # open: nothing reaches round the period


def test_one_cell_in_y_and_z():
    c, ref, opn = _known("one_cell")
    assert tuple(GP.index_coords(c)[1][1:]) == (1, 1)
    assert CP.crossings(c["xyz"], 0, 1, c["L"]) == (-1, 0) and CP.crossings(c["xyz"], 1, 2, c["L"]) == (0, -1)
    assert ref["chains"][0]["direct2"] == 8.0 and opn["chains"][0]["status"] == CP.OPEN


def test_wrapped_stone_is_one_node_entered_and_left_on_different_sides():
    c, ref, _ = _known("wrapped_stone")
    r = ref["chains"][0]
    assert (r["n_stones"], r["n_stone_sites"], r["n_hops"]) == (1, 4, 2)
    ys = c["xyz"][c["node"] == 5, 1]
    assert sorted(ys) == [1.0, 3.0, 61.0, 63.0] and CP.stones_through_a_face(c) == [5]
    (a0, b0, _), (a1, b1, _) = c["hops"][0]
    assert c["xyz"][b0, 1] < 32.0 < c["xyz"][a1, 1] and c["node"][b0] == c["node"][a1] == 5


def test_zigzag_wrap_is_long_winds_and_takes_rounds():
    c, ref, opn = _known("zigzag_wrap")
    r = ref["chains"][0]
    coords, nc = GP.index_coords(c)
    assert r["n_hops"] == CP.ZIGZAG_STONES + 1 >= 200 and tuple(nc[1:]) == (2, 1) and c["max_hops"] == 16
    turns = sum(CP.crossings(c["xyz"], a, b, c["L"])[0] != 0 for a, b, _ in c["hops"][0])
    assert turns >= 5 and max(ref["rounds"]) >= 4 and opn["chains"][0]["status"] == CP.OPEN
    assert r["hop_max2"] == 4.3125


def test_interior_equals_the_open_answer():
    c, ref, opn = _known("interior")
    assert ref["chains"].tobytes() == opn["chains"].tobytes() and ref["hops"].tobytes() == opn["hops"].tobytes()
    assert ref["stats"] == opn["stats"]
    assert all(CP.crossings(c["xyz"], a, b, c["L"]) == (0, 0) for a, b, _ in c["hops"][0])


def test_every_radius_is_within_its_index():
    for name in CP.SEARCH_CASES:
        c = CP.case(name)
        assert 0.0 < c["r_max"] <= c["cutoff"], name
        assert ((c["node"] < len(c["xyz"])) | (c["side"] != 0)).all()
