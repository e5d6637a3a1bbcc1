"""CPU: the restatement of the periodic filament gap (tests/site_gap_pbc_ref.py) and the conditions that keep the GPU test
(tests/test_gpu_site_gap_pbc.py) meaningful -- every input does what it was built for -- the two new symbols, and the
argument errors of kmcf_site_set_gap_pbc / kmcf_filament_gap_pbc that are reachable without an index (the table of
tests/test_site_gap_ref.py)."""
import os
import re

import numpy as np
import pytest

import pbc_ref as P
import site_gap_pbc_ref as GP
import site_gap_ref as GR
import test_site_gap_ref as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- symbols and argument errors ---------------------------------------------------------------------------------------------

def test_the_two_symbols_are_exported_with_the_headers_signatures(km):
    lib = km.lib.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmcfield.h")).read(), flags=re.S)
    for name in ("kmcf_site_set_gap", "kmcf_filament_gap"):
        decl, decl_pbc = (re.search(r"int\s+%s\s*\(([^)]*)\)" % n, hdr) for n in (name, name + "_pbc"))
        assert decl and decl_pbc, name
        assert re.sub(r"\s+", " ", decl.group(1)) == re.sub(r"\s+", " ", decl_pbc.group(1))      # the parameter list of its counterpart
        res, args = km.lib.SIGNATURES[name + "_pbc"]
        assert (res, args) == km.lib.SIGNATURES[name] and len(args) == decl_pbc.group(1).count(",") + 1
        assert hasattr(lib, name + "_pbc")


SET_TABLE = TG.test_site_set_gap_argument_errors_without_an_index.pytestmark[0].args[1]
FIL_TABLE = TG.test_filament_gap_argument_errors_without_an_index.pytestmark[0].args[1]


def test_the_error_tables_are_those_of_the_plain_calls():
    assert len(SET_TABLE) == len(TG.COMMON) + 1 and len(FIL_TABLE) == len(TG.COMMON) + 13


@pytest.mark.parametrize("change,word", SET_TABLE)
def test_site_set_gap_pbc_argument_errors_without_an_index(km, change, word):
    a = TG._set_args()
    a.update(change)
    rc, msg = TG._call(km, "kmcf_site_set_gap_pbc", a)
    assert rc == TG.ERR_ARG and word in msg and b"kmcf_site_set_gap_pbc" in msg, (rc, msg)


@pytest.mark.parametrize("change,word", FIL_TABLE)
def test_filament_gap_pbc_argument_errors_without_an_index(km, change, word):
    a = TG._fil_args()
    a.update(change)
    rc, msg = TG._call(km, "kmcf_filament_gap_pbc", a)
    assert rc == TG.ERR_ARG and word in msg and b"kmcf_filament_gap_pbc" in msg, (rc, msg)


# ---- the restatement itself ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["planes", "straddle", "rim", "rim_below", "mixed", "dense"])
def test_without_a_lattice_it_is_the_open_restatement(name):
    c = GR.case(name)
    gaps, stats = GP.site_set_gap(c["xyz"], c["side"], c["r_max"], c["cell"], c["n_cells"], L=None)
    r_gaps, r_stats = GR.reference(name)
    assert stats == r_stats
    for f in GR.GAP_DTYPE.names:
        assert np.array_equal(gaps[f], r_gaps[f]), f


@pytest.mark.parametrize("name", ["p23@20", "lattice_wrap@12", "corner", "ties_wrap"])
def test_tree_proposals_give_the_all_pairs_answer(name):
    c = GP.case(name)
    gaps, stats = GP.site_set_gap(c["xyz"], c["side"], c["r_max"], c["cell"], c["n_cells"], c["L"], propose="tree")
    assert gaps.tobytes() == GP.reference(name)[0].tobytes() and stats == GP.reference(name)[1]


def test_fold_is_the_distance_of_pbc_ref():
    c = P.pairwise_case("p23")
    xyz, L = c["xyz"], c["L"]
    a, b = np.arange(0, 600)[:, None], np.arange(600, 1500)[None, :]
    d = P.dist(xyz[a, 0], xyz[a, 1], xyz[a, 2], xyz[b, 0], xyz[b, 1], xyz[b, 2], L)
    # (pbc_ref.dist adds dx*dx + dy*dy + dz*dz left to right, as the contract's d2 does: the same bits)
    assert np.array_equal(np.sqrt(GP.d2_exact(xyz, a, b, L)), d)
    assert (GP.fold(xyz[a, 1], xyz[b, 1], L[1])[1] != 0).sum() >= 1000


# ---- random cases ----------------------------------------------------------------------------------------------------------------

def _winner_crossings(c, gaps):
    ny = nz = 0
    for g in gaps[gaps["site_left"] >= 0]:
        cy, cz = GP.crossings(c["xyz"], g["site_left"], g["site_right"], c["L"])
        ny, nz = ny + (cy != 0), nz + (cz != 0)
    return ny, nz


@pytest.mark.parametrize("base", GP.RANDOM)
def test_random_cases_hold_what_they_are_built_for(base):
    name = "%s@%g" % (base, GP.R_MAX)
    c = GP.case(name)
    N = len(c["xyz"])
    gaps, stats = GP.reference(name)
    opn, _ = GP.reference(name, periodic=False)
    differ = int(sum(gaps[k].tobytes() != opn[k].tobytes() for k in range(c["n_cells"])))
    ny, nz = _winner_crossings(c, gaps)
    none = int((gaps["site_left"] < 0).sum())
    print("%s: %d sites, %d gap cells, index cells %s; %d records differ from open boundaries, winners across y %d, across z %d, "
          "no pair %d, %s" % (name, N, c["n_cells"], GP.index_coords(c)[1].tolist(), differ, ny, nz, none, stats))
    assert c["r_max"] == 20.0 and c["n_cells"] == N // 8 and c["cutoff"] == 20.0
    assert tuple(GP.index_coords(c)[1][1:]) == P.pairwise_case(base)["cells"]
    assert abs(((c["side"] & 3) == 3).mean() - 0.02) < 0.01
    assert (c["cell"] == -1).sum() >= 1 and (c["cell"] == c["n_cells"]).sum() >= 1
    assert differ >= 10
    assert ny >= 3 and nz >= 3
    assert none >= 5
    assert stats["cells_open"] >= 50
    assert stats["cells_bridged"] >= 5
    assert stats["cells_open"] + stats["cells_none"] + stats["cells_bridged"] == c["n_cells"]


@pytest.mark.parametrize("base", GP.RANDOM)
def test_second_radius(base):
    """r_max = 12 with about 12 sites per gap cell: no thresholds, the figures are printed"""
    name = "%s@%g" % (base, GP.R_SMALL)
    c = GP.case(name)
    gaps, stats = GP.reference(name)
    print(name, c["n_cells"], "gap cells, winners across (y, z)", _winner_crossings(c, gaps), stats)
    assert c["r_max"] == 12.0 and c["n_cells"] == len(c["xyz"]) // 12 and c["r_max"] < c["cutoff"]


# ---- constructed cases: the answers hold by construction -------------------------------------------------------------------------

def _records(name):
    c = GP.case(name)
    gaps, stats = GP.reference(name)
    for g, want in zip(gaps, c["pairs"]):
        if want is None:
            assert g["site_left"] == -1 and g["site_right"] == -1 and np.isinf(g["gap2"])
        else:
            assert (g["site_left"], g["site_right"], g["gap2"]) == want, (name, g, want)
    return c, gaps, GP.reference(name, periodic=False)[0]


def test_corner_crosses_both_faces():
    c, gaps, opn = _records("corner")
    a, b = gaps[0]["site_left"], gaps[0]["site_right"]
    assert GP.crossings(c["xyz"], a, b, c["L"]) == (-1, -1)
    coords, nc = GP.index_coords(c)
    assert nc[1] == 4 and nc[2] == 4 and tuple(coords[a][1:]) == (0, 0) and tuple(coords[b][1:]) == (3, 3)
    assert (opn[0]["site_right"], opn[0]["gap2"]) == (2, 64.0)                  # the open answer is another b


def test_rim_wrap_counts_at_r_max_and_not_below():
    c, gaps, opn = _records("rim_wrap")
    assert c["r_max"] * c["r_max"] == gaps[0]["gap2"] == 25.0 and GP.crossings(c["xyz"], 0, 1, c["L"]) == (-1, 0)
    assert opn[0]["site_left"] == -1
    below = GP.case("rim_wrap_below")
    _records("rim_wrap_below")
    assert below["r_max"] < 5.0 and np.array_equal(below["xyz"], c["xyz"]) and GP.reference("rim_wrap_below")[1]["cells_none"] == 1


def test_half_a_period_rounds_away_from_zero():
    c, gaps, _ = _records("half")
    xyz, L = c["xyz"], c["L"]
    assert GP.index_coords(c)[1][1] == 1 and L[1] == 25.0
    for (a, b), (f, n) in zip(((0, 1), (2, 3)), ((0.5, 1.0), (-0.5, -1.0))):
        assert (xyz[a, 1] - xyz[b, 1]) / L[1] == f and P.c_round(f) == n
        dy, taken = GP.fold(xyz[a, 1], xyz[b, 1], L[1])
        assert dy == -f * L[1] and taken == n
    assert gaps["gap2"].tolist() == [156.25, 156.25]


def test_ties_wrap_smallest_a_then_smallest_b():
    c, gaps, _ = _records("ties_wrap")
    for g in range(2):
        A = np.flatnonzero((c["cell"] == g) & (c["side"] == 1))
        B = np.flatnonzero((c["cell"] == g) & (c["side"] == 2))
        d2 = GP.d2_exact(c["xyz"], A[:, None], B[None, :], c["L"])
        assert d2.shape == (2, 2) and (d2 == 20.0).all()
        cross = [GP.crossings(c["xyz"], A[0], b, c["L"])[0] != 0 for b in B]
        assert sorted(cross) == [False, True]
        assert (gaps[g]["site_left"], gaps[g]["site_right"]) == (A.min(), B.min())
        assert cross[0] == (g == 0)                                             # the winner's b: through the wrap in cell 0, inside in cell 1
    assert c["xyz"][gaps[0]["site_left"], 0] > c["xyz"][gaps[0]["site_left"] + 1, 0]      # the smallest a is not the first in x


def test_two_cells_inner_and_outer_face():
    c, gaps, opn = _records("two_cells")
    coords, nc = GP.index_coords(c)
    assert nc[1] == 2 and c["L"][1] / 2 >= c["cutoff"]
    for g, crossed in ((0, 0), (1, -1)):
        a, b = gaps[g]["site_left"], gaps[g]["site_right"]
        assert coords[a][1] == 0 and coords[b][1] == 1 and GP.crossings(c["xyz"], a, b, c["L"])[0] == crossed
        ya = c["xyz"][a, 1]
        wrong_face = max(ya - 0.0, 16.0 - ya)                                   # the face the winner does NOT lie behind
        assert wrong_face > c["r_max"] > np.sqrt(gaps[g]["gap2"])
        own = np.flatnonzero((c["cell"] == g) & (c["side"] == 2) & (coords[:, 1] == 0))
        assert len(own) == 1 and GP.d2_exact(c["xyz"], a, own[0], c["L"]) == 36.0
    assert opn[0]["gap2"] == 16.0 and opn[1]["gap2"] == 36.0


def test_second_image_adds_no_pair():
    c, gaps, opn = _records("second_image")
    assert c["L"][1] < 2 * c["r_max"] and GP.index_coords(c)[1][1] == 1
    open_d2 = GR.d2_exact(c["xyz"], 0, 1)
    assert open_d2 == 121.0 <= c["r_max"] ** 2 and gaps[0]["gap2"] == 25.0     # both images within r_max; one distance
    assert (gaps[0]["n_left"], gaps[0]["n_right"]) == (1, 1) and GP.reference("second_image")[1]["cells_open"] == 1
    assert opn[0]["gap2"] == 121.0


def test_interior_equals_the_open_answer():
    c, gaps, opn = _records("interior")
    assert gaps.tobytes() == opn.tobytes() and GP.crossings(c["xyz"], 0, 1, c["L"]) == (0, 0)
    coords, nc = GP.index_coords(c)
    assert nc[1] == 4 and nc[2] == 4 and tuple(coords[0][1:]) == (1, 1)


# ---- stubs -------------------------------------------------------------------------------------------------------------------------

def test_stubs_face_each_other_across_the_y_face():
    s = GP.stubs()
    args = (s["element"], s["charge"], s["metals"], s["xyz"], s["NL"], s["NR"], GP.STUB_R_MAX)
    per = GP.filament_gap(s["per"], *args, L=s["L"], bins=(6, 0.0, 30.0))
    opn = GP.filament_gap(s["opn"], *args, L=None)
    g = per["gaps"][0]
    print("stubs: periodic", g, "open", opn["gaps"][0])
    assert (s["element"][:30] == GP.STUB_METAL).all() and (s["element"][-30:] == GP.STUB_METAL).all()
    assert (per["side"][s["left"]] == 1).all() and (per["side"][s["right"]] == 2).all()
    assert (per["side"][:30] == 1).all() and (per["side"][-30:] == 2).all() and (per["side"] != 0).sum() == 68
    assert np.array_equal(per["side"], opn["side"])                             # neither chain passes a face itself
    assert (g["site_left"], g["site_right"]) == (s["left"][-1], s["right"][0])
    assert 7.0 < g["gap"] < 9.0 and GP.crossings(s["xyz"], g["site_left"], g["site_right"], s["L"])[0] != 0
    assert (g["n_left"], g["n_right"], g["n_both"], g["bridged"]) == (34, 34, 0, 0)
    assert opn["gaps"][0]["site_left"] == -1 and opn["stats"]["cells_none"] == 1
    assert per["profile"].sum() == 8 and per["profile"][0][:, 2].sum() == 0
