"""CPU: the restatement of kmcf_field_sample (tests/field_sample_ref.py) on inputs whose answer holds by construction, and
the conditions every input of tests/test_gpu_field_sample.py is built for.

The bounds (tests/test_gpu_field_sample.py asserts the same of the library), n = count, eps = 2^-52:
    |wsum - fsum|  <= n eps sum(w)            |acc_f - fsum| <= n eps sum(w |v_f|)
    |mean - exact| <= (2 n + 4) eps sum(w |v_f|) / sum(w)
the first-order bound of a sum of n terms in any order, times two; the terms are the same bits on both sides."""
import numpy as np
import pytest

import field_sample_ref as R
import site_gap_pbc_ref as GP

EPS = R.EPS


def test_two_sites_by_hand():
    xyz = np.array([(0.0, 0.0, 0.0), (2.0, 0.0, 0.0)])
    r = R.field_sample(xyz, [(1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (5.0, 0.0, 0.0), (-2.0, 0.0, 0.0)], [[1.0, 3.0]], None, 2.0, 1, -1.0)
    assert list(r["count"]) == [2, 2, 0, 1] and list(r["nearest"]) == [0, 0, -1, 0]
    assert list(r["nearest_d2"]) == [1.0, 0.0, np.inf, 4.0]
    assert list(r["wsum"]) == [2 * 0.5625, 1.0, 0.0, 0.0]                      # (1 - 1/4)^2 twice; 1 and 0 (the rim); none; the rim
    assert list(r["out"][0]) == [2.0, 1.0, -1.0, -1.0]                         # the mean; the site itself; fill; fill (wsum == 0)
    assert r["stats"] == dict(n_points=4, n_empty=1, n_visits=5, n_members=2, max_count=2, max_count_point=0)
    raw = R.field_sample(xyz, [(1.0, 0.0, 0.0)], [[1.0, 3.0]], [0, 1], 2.0, 0)
    assert raw["out"][0, 0] == 3.0 * 0.5625 and raw["stats"]["n_members"] == 1 and raw["nearest"][0] == 1


def test_minimum_image_and_no_points():
    xyz = np.array([(0.0, 0.5, 0.5)])
    L = (10.0, 8.0, 8.0)
    per = R.field_sample(xyz, [(0.0, 7.5, 0.5), (0.0, 7.5 + 16.0, 0.5 - 8.0)], None, None, 2.0, 1, R.FILL, L)
    assert list(per["count"]) == [1, 1] and list(per["nearest_d2"]) == [1.0, 1.0]
    assert list(R.field_sample(xyz, [(0.0, 7.5, 0.5)], None, None, 2.0)["count"]) == [0]
    none = R.field_sample(xyz, np.zeros((0, 3)), [[1.0]], None, 2.0)
    assert none["stats"] == dict(n_points=0, n_empty=0, n_visits=0, n_members=0, max_count=0, max_count_point=-1)


def test_grid_points_are_z_fastest():
    p = R.grid_points((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (2, 3, 4))
    assert p.shape == (24, 3) and tuple(p[1]) == (1.0, 2.0, 5.0) and tuple(p[4]) == (1.0, 2.25, 3.0) and tuple(p[12]) == (1.5, 2.0, 3.0)


@pytest.mark.parametrize("name", tuple(R.RANDOM))
@pytest.mark.parametrize("periodic", [True, False])
def test_random_cases_are_what_they_are_built_for(name, periodic):
    c, r = R.case(name), R.reference(name, periodic)
    cnt = r["count"]
    assert 0.05 <= (cnt == 0).mean() <= 0.50, (cnt == 0).mean()
    assert cnt.max() >= 33 and (cnt == 1).any()
    ncy, ncz = R.RANDOM[name]
    assert int(np.floor(c["L"][1] / c["cutoff"])) == ncy and int(np.floor(c["L"][2] / c["cutoff"])) == ncz
    assert c["xyz"][:, 1].min() == 0.0 and c["xyz"][:, 2].min() == 0.0           # the origin of the periodic index
    assert np.ptp(c["xyz"][:, 1]) < c["L"][1] and np.ptp(c["xyz"][:, 2]) < c["L"][2]
    pts, lo, hi = c["points"], c["xyz"].min(0), c["xyz"].max(0)
    outside = ((pts < lo) | (pts > hi)).any(1)
    assert (outside & (cnt > 0)).sum() >= 20, "points outside the sites' box that reach boundary sites"
    assert (outside & (cnt == 0)).sum() >= 20, "points beyond reach"
    if periodic:
        Ly, Lz = c["L"][1], c["L"][2]
        out_period = (pts[:, 1] < 0) | (pts[:, 1] >= Ly) | (pts[:, 2] < 0) | (pts[:, 2] >= Lz)
        assert (out_period & (cnt > 0)).sum() >= 20, "points outside the period that reach sites through the minimum image"
        assert ((np.abs(pts[:, 1]) > 2.0 * Ly) & (cnt > 0)).any() and ((np.abs(pts[:, 2]) > 2.0 * Lz) & (cnt > 0)).any()
        assert np.abs(pts[:, 1]).max() <= 4.0 * Ly and np.abs(pts[:, 2]).max() <= 4.0 * Lz
        for y in (0.0, Ly, -Ly, 3.0 * Ly):
            for z in (0.0, Lz):
                assert ((pts[:, 1] == y) & (pts[:, 2] == z) & (cnt > 0)).any(), ("a point on the faces", y, z)
        # the wrap matters: the open distance gives another answer
        assert not np.array_equal(cnt, R.reference(name, False)["count"])


def test_cells_case_holds_the_member_counts():
    c = R.case("cells")
    per_cell = np.bincount(np.floor(c["xyz"][:, 0] / c["cutoff"]).astype(int), minlength=len(R.CELL_COUNTS))
    assert tuple(per_cell) == R.CELL_COUNTS and {0, 1, 15, 16, 17, 40} <= set(R.CELL_COUNTS)
    assert c["mask"].all()


@pytest.mark.parametrize("n", R.TILES)
def test_tile_cases(n):
    c = R.case("tile@%d" % n)
    assert len(c["xyz"]) == n and 0.4 < c["mask"].mean() < 0.6 and len(c["points"]) == 257
    assert R.reference("tile@%d" % n)["stats"]["n_members"] == int(c["mask"].sum())


@pytest.mark.parametrize("periodic", [True, False])
def test_lattice_case_is_exact_and_sits_on_the_rim(periodic):
    c, r = R.case("lattice"), R.reference("lattice", periodic, n_fields=8)
    assert c["radius"] == 4.0 and c["cutoff"] == 4.0
    pts, xyz, n = c["points"], c["xyz"], len(c["points"])
    mem = np.flatnonzero(c["mask"])
    both = np.concatenate([pts, xyz])
    d2 = GP.d2_exact(both, np.arange(n)[:, None], (n + mem)[None, :], c["L"] if periodic else None)
    assert (d2 == 16.0).sum() >= 8, "pairs exactly on the rim"
    assert (d2 == np.nextafter(16.0, np.inf)).sum() >= 8, "pairs at the next double above r2"
    on_rim = (d2 == 16.0).sum(1)
    within = (d2 <= 16.0).sum(1)
    assert np.array_equal(within, r["count"]) and (on_rim > 0).any()
    above = (d2 == np.nextafter(16.0, np.inf)).any(1)
    assert above.sum() >= 8 and (r["count"][above] == 0).all() and (r["nearest"][above] == -1).all()
    # rim-only points: counted, weight 0, the mean is the fill
    rim_only = (on_rim == within) & (within > 0)
    if rim_only.any():
        assert (r["wsum"][rim_only] == 0.0).all() and (r["out"][:, rim_only] == R.FILL).all()
    # ties of the nearest site go to the smallest id
    dmin = d2.min(1)
    ties = ((d2 == dmin[:, None]).sum(1) >= 2) & (dmin <= 16.0)
    assert ties.sum() >= 8
    first = mem[np.argmax(d2 == dmin[:, None], axis=1)]
    assert np.array_equal(r["nearest"][ties], first[ties])
    assert ((dmin == 0.0) & (r["nearest_d2"] == 0.0)).sum() >= 1, "a point on a site"
    # exact: every term is a multiple of 2^-12 of small size, so the sums carry no rounding: any order gives these bits
    assert np.array_equal(r["wsum"], r["wsum_fsum"]) and np.array_equal(r["acc"], r["acc_fsum"])
    assert np.array_equal(r["wsum"] * 4096.0, np.rint(r["wsum"] * 4096.0))
    assert np.array_equal(r["acc"] * 4096.0, np.rint(r["acc"] * 4096.0))
    if periodic:
        assert c["L"][1] == 16.0 and c["L"][2] == 16.0          # a power of two: the minimum image is exact
        assert (((pts[:, 1] < 0) | (pts[:, 1] >= 16.0)) & (r["count"] > 0)).any()


@pytest.mark.parametrize("name", R.CASES)
@pytest.mark.parametrize("periodic", [True, False])
def test_restatement_stays_within_the_bounds(name, periodic):
    """numpy's order against the correctly rounded sums; a constant field gives the constant as its mean"""
    r = R.reference(name, periodic, n_fields=8)
    n = r["count"].astype(np.float64)
    assert (np.abs(r["wsum"] - r["wsum_fsum"]) <= n * EPS * r["wsum_fsum"]).all()
    assert (np.abs(r["acc"] - r["acc_fsum"]) <= n[None, :] * EPS * r["wabs"]).all()
    ok = r["wsum"] > 0.0
    exact = r["acc_fsum"][:, ok] / r["wsum_fsum"][ok]
    bound = (2.0 * n[ok] + 4.0) * EPS * r["wabs"][:, ok] / r["wsum_fsum"][ok]
    assert (np.abs(r["out"][:, ok] - exact) <= bound).all()
    assert (r["out"][:, ~ok] == R.FILL).all()
    const = R.case(name)["values"][1, 0]
    assert (np.abs(r["out"][1, ok] - const) <= (2.0 * n[ok] + 4.0) * EPS * abs(const)).all()
    frac = np.abs(r["wsum"] - r["wsum_fsum"])[ok] / (n[ok] * EPS * r["wsum_fsum"][ok])
    print("%s, %s: numpy's order at %.3f of the bound on wsum" % (name, "periodic" if periodic else "open", frac.max()))


def test_variants():
    full = R.reference("r23", True)
    assert R.reference("r23", True, mask="none")["stats"]["n_visits"] == 0
    assert R.reference("r23", True, mask="ones")["stats"] == R.reference("r23", True, mask="null")["stats"]
    small = R.reference("r23", True, radius=R.SMALL_RADIUS)
    assert (small["count"] == 0).mean() > 0.5 and small["stats"]["n_visits"] > 0
    for n in R.N_POINTS:
        assert np.array_equal(R.reference("r23", True, n_points=n)["count"], full["count"][:n])
    assert set(R.FIELD_COUNTS) == {0, 1, 2, 3, 4, 5, 8}


def test_the_wrappers_exist(km):
    S = km.solvers
    assert callable(S.field_sample) and callable(S.field_grid) and callable(S.field_slice) and callable(S.sample_density)
    res = dict(out=np.array([2.0]), radius=3.0)
    assert np.array_equal(S.sample_density(res), R.sample_density([2.0], 3.0))
    assert np.isclose(S.sample_density(res, 1.0)[0], 2.0 * 105.0 / (32.0 * np.pi))
