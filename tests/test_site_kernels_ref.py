"""CPU: the references of tests/site_kernels_ref.py against the oracle on the 5 nm device (and, for the pairwise term, against
an all-pairs sum in 40-digit arithmetic), answers known by construction, and the conditions that keep the inputs of
tests/test_gpu_site_kernels.py meaningful -- asserted here, so that a later edit of a seed cannot silently empty a case."""
import math

import numpy as np
import pytest

import site_kernels_ref as R


# ------------------------------------------------------------------------------------------------ references
def test_pairwise_ref_matches_oracle_on_5nm(oracle, dev5, ref5):
    d = dev5
    want, S, n = R.pairwise_ref(d["xyz"], ref5["charge"], d["sigma"], d["k"], 20.0)
    orc = oracle.poisson_gridless(d["xyz"], ref5["charge"], d["sigma"], d["k"], 20.0)
    err = np.abs(orc - want.astype(np.float64))
    print("5 nm: max |oracle - ref| / S = %.3g, terms per site <= %d" % (float((err[S > 0] / S[S > 0]).max()), n.max()))
    assert np.all(err <= 1e-14 * S)
    assert np.all(orc[n == 0] == 0.0) and (n > 0).sum() > 30000
    assert np.all(S * (1 + 1e-12) >= np.abs(want.astype(np.float64)))


def test_pairwise_ref_matches_40_digit_all_pairs_sum():
    """Every term of every site evaluated by mpmath at 40 digits from the float64 inputs, all pairs, no tree: 1e-15 S_i.
    What a float64 term is off by is, above all, the rounding of erfc's argument times erfc's condition number
    c(x) = 2 x exp(-x^2) / (sqrt(pi) erfc x): 1.2 at 3 A, 8.6 at 10 A, 33 at the cutoff.  Relative to S_i a site's sum is
    then off by about (c_i + 2) 2^-53 with c_i the |term|-weighted mean of c, and 1e-15 = 9 * 2^-53 is what float64 terms
    can hold where c_i stays below 7: at sites that have a partner within some 9 A.  The 200 sites therefore fill a
    24 x 16 x 16 A box (c_i <= 5 asserted below; the box is longer than the cutoff, which still decides 800 pairs)."""
    mp = pytest.importorskip("mpmath")
    from scipy.special import erfc
    mp.mp.dps = 40
    rng = np.random.default_rng(7)
    N, sigma, k, cutoff = 200, 3.5e-10, 8.987552e9 / 23.0, 20.0
    xyz = rng.random((N, 3)) * np.array([24.0, 16.0, 16.0])
    charge = np.zeros(N, np.int32)
    idx = rng.choice(N, 60, replace=False)
    charge[idx] = rng.choice([-2, 2], 60)
    want, S, n = R.pairwise_ref(xyz, charge, sigma, k, cutoff)
    assert R.cutoff_margin(xyz, charge, cutoff)[0] > 1e-12
    i, _, dist = R.site_charged_pairs(xyz, charge, 100.0)
    assert (dist >= cutoff).sum() > 500 and n.min() >= 1
    near = dist < cutoff
    x = 1e-10 * dist[near] / (sigma * np.sqrt(2.0))
    weight = erfc(x) / dist[near]
    cond = 2 * x * np.exp(-x * x) / (np.sqrt(np.pi) * erfc(x))
    c_site = np.bincount(i[near], weight * cond, N) / np.bincount(i[near], weight, N)
    assert c_site.max() <= 5.0, c_site.max()
    X = [[mp.mpf(float(v)) for v in row] for row in xyz]
    root2, q, kk, sg = mp.sqrt(2), mp.mpf(R.Q_E), mp.mpf(k), mp.mpf(sigma)
    worst = 0.0
    for i in range(N):
        tot, count = mp.mpf(0), 0
        for j in idx:
            if j == i:
                continue
            dist = mp.sqrt(sum((X[j][a] - X[i][a]) ** 2 for a in range(3)))
            if dist < cutoff:
                r = mp.mpf("1e-10") * dist
                tot += int(charge[j]) * mp.erfc(r / (sg * root2)) * kk * q / r
                count += 1
        assert count == n[i]
        err = abs(mp.mpf(float(want[i])) - tot)
        worst = max(worst, float(err / mp.mpf(float(S[i]))))
        assert err <= mp.mpf(1e-15) * mp.mpf(float(S[i])), i
    print("200 sites: max |ref - 40 digits| / S = %.3g, weighted condition number <= %.2f" % (worst, c_site.max()))


def test_charge_ref_matches_oracle_on_5nm(oracle, dev5, ref5):
    d = dev5
    got = R.charge_ref(d["element"], np.zeros(d["N"], np.int32), ref5["neigh"], d["metals"], 0)
    assert np.array_equal(got, ref5["charge"]) and int((got != 0).sum()) == 339
    # a slice with displ > 0: only its rows of the list, untouched sites keep the 7 they came with
    lo, cnt = 12345, 2000
    got = R.charge_ref(d["element"], np.full(d["N"], 7, np.int32), ref5["neigh"][lo:lo + cnt], d["metals"], lo)
    want = oracle.update_charge(d["element"], np.full(d["N"], 7, np.int32), ref5["neigh"][lo:lo + cnt], d["metals"], lo, lo + cnt)
    assert np.array_equal(got, want) and np.all(got[:lo] == 7) and np.all(got[lo + cnt:] == 7)


def test_k_values_ref_matches_oracle_on_5nm(oracle, dev5, ref5):
    d, ks, A = dev5, ref5["ks"], ref5["A"]
    got = R.k_values_ref(ks.row_ptr, ks.col, (ks.left_row_ptr, ks.left_col), (ks.right_row_ptr, ks.right_col), d["element"],
                         ref5["charge"], d["metals"], d["high_G"], d["low_G"], d["Vd"], ks.N_left, ks.n, cb=False)
    off = got["off_diagonal"]
    assert np.array_equal(got["val"][off], A["val"][off])
    for key in ("diag", "dinv", "rhs", "left", "right"):
        np.testing.assert_allclose(got[key], A[key], rtol=1e-14, atol=0, err_msg=key)
    np.testing.assert_allclose(got["val"][~off], A["val"][~off], rtol=1e-14)
    # the CB rule against the oracle's CB system (values and right-hand side: all it returns)
    _, _, B = oracle.update_CB_edge(ks, d["element"], d["metals"], d["high_G"], d["low_G"], d["Vd"], max_it=1)
    cb = R.k_values_ref(ks.row_ptr, ks.col, (ks.left_row_ptr, ks.left_col), (ks.right_row_ptr, ks.right_col), d["element"],
                        ref5["charge"], d["metals"], d["high_G"], d["low_G"], d["Vd"], ks.N_left, ks.n, cb=True)
    assert np.array_equal(cb["val"][off], B["val"][off])
    np.testing.assert_allclose(cb["val"][~off], B["val"][~off], rtol=1e-14)
    np.testing.assert_allclose(cb["rhs"], B["rhs"], rtol=1e-14)
    assert np.any(cb["rhs"] != 0) and np.array_equal(np.sign(cb["rhs"][cb["rhs"] != 0]), -np.sign(got["rhs"][cb["rhs"] != 0]))


def test_k_values_ref_on_a_chain_known_by_construction():
    """contact | metal - metal - uncharged V - uncharged V - charged V - oxide | contact, all on one row of neighbours"""
    M, V, O = 6, R.VACANCY, 3
    element = np.array([M, M, M, V, V, V, O, M])
    charge = np.array([0, 0, 0, 0, 0, 2, 0, 0])
    n = 6
    rp = np.array([0, 2, 5, 8, 11, 14, 16])
    col = np.array([0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5])
    left = (np.array([0, 1, 1, 1, 1, 1, 1]), np.array([0]))
    right = (np.array([0, 0, 0, 0, 0, 0, 1]), np.array([0]))
    H, Lo = 1.0, 1e-8
    k = R.k_values_ref(rp, col, left, right, element, charge, [M], H, Lo, 5.0, 1, n, cb=False)
    assert k["val"][k["off_diagonal"]].tolist() == [-H, -H, -Lo, -Lo, -H, -H, -Lo, -Lo, -Lo, -Lo]
    assert k["left"].tolist() == [H, 0, 0, 0, 0, 0] and k["right"].tolist() == [0, 0, 0, 0, 0, Lo]
    assert k["diag"].tolist() == [2 * H, H + Lo, H + Lo, H + Lo, 2 * Lo, 2 * Lo] and k["rhs"].tolist() == [-2.5 * H, 0, 0, 0, 0, 2.5 * Lo]
    c = R.k_values_ref(rp, col, left, right, element, charge, [M], H, Lo, 5.0, 1, n, cb=True)
    assert c["val"][c["off_diagonal"]].tolist() == [-H, -H, -H, -H, -Lo, -Lo, -Lo, -Lo, -Lo, -Lo]
    assert c["right"].tolist() == [0, 0, 0, 0, 0, H] and c["rhs"].tolist() == [2.5 * H, 0, 0, 0, 0, -2.5 * H]


def test_heat_global_ref_matches_oracle(oracle):
    rng = np.random.default_rng(5)
    p = rng.random(37650) * 1e-9
    args = (0.999, 0.3, 100.0, 1e-12, 1e-17)
    np.testing.assert_allclose(R.heat_global_ref(p, 300.0, *args), oracle.update_temperature_global(p, 300.0, *args), rtol=1e-13)
    q = R.heat_power(257)
    a = R.HEAT_ARGS
    args = (a["a"], a["b"], 100.9, a["C"], a["small_step"])
    np.testing.assert_allclose(R.heat_global_ref(q, 310.0, *args), oracle.update_temperature_global(q, 310.0, *args), rtol=1e-13)
    assert R.heat_global_ref(q, 310.0, *args) == R.heat_global_ref(q, 310.0, a["a"], a["b"], 100.0, a["C"], a["small_step"])
    zero = a["b"] * (1 - a["a"] ** 100) / (1 - a["a"]) + a["a"] ** 100 * 300.0
    assert R.heat_global_ref(np.zeros(0), 300.0, **a) == zero


# ------------------------------------------------------------------------------------------------ pairwise inputs
SIGMA, K = 3.5e-10, 8.987552e9 / 23.0          # (the conditions below do not depend on the two constants)


@pytest.mark.parametrize("name", R.PAIRWISE_CASES)
def test_pairwise_input_meets_its_conditions(name):
    c = R.pairwise_case(name)
    xyz, charge, N = c["xyz"], c["charge"], c["N"]
    margin, exact = R.cutoff_margin(xyz, charge)
    _, _, n = R.pairwise_reference(name, SIGMA, K)
    order, nc = R.cell_order(xyz)
    tiles = -(-N // R.SCAN_TILE)
    print("%s: N %d, %d charged, cells %s, %d scan tiles, nearest pair to the cutoff %.3g, %d at it, terms per site <= %d"
          % (name, N, int((charge != 0).sum()), nc, tiles, margin, exact, n.max() if N else 0))
    assert n.max() <= 1000
    for displ, count in c["slices"]:
        assert 0 <= displ and displ + count <= N
    if name in R.ON_LATTICE:
        assert np.array_equal(xyz, 4.0 * np.round(xyz / 4.0))
        if (charge != 0).any():
            assert exact >= 100
    else:
        assert margin >= 1e-12
    flags = (charge != 0)[order]
    per_tile = np.add.reduceat(flags.astype(int), np.arange(0, N, R.SCAN_TILE))
    if name == "thin":
        assert N == 2 * R.SCAN_TILE + 20 and nc[1:] == (1, 1) and per_tile.tolist() == [2048, 2048, 20]
        assert sorted(set(charge.tolist())) == [-2, 2] and (n > 0).all()
    if name == "thin_uncharged":
        assert not charge.any() and np.array_equal(xyz, R.pairwise_case("thin")["xyz"])
    if name == "one_cell":
        assert nc == (1, 1, 1) and int((charge != 0).sum()) == 100
        i, j, dist = R.site_charged_pairs(xyz, charge, 40.0)
        assert (dist > 20.0).sum() >= 20              # the cutoff decides inside the single cell too
    if name == "one_site":
        assert N == 1 and charge[0] != 0 and n[0] == 0
    if name == "seventeen":
        assert N == 17 and np.flatnonzero(charge).tolist() == [16] and n.tolist() == [1] * 16 + [0]
    if name == "cube":
        assert nc == (4, 4, 4) and int((charge != 0).sum()) == 1800 and (1237, 1001) in c["slices"]
    if name == "lattice_cutoffs":
        assert nc == (4, 4, 4) and N == 2 * R.SCAN_TILE
        i, j, dist = R.site_charged_pairs(xyz, charge, 20.0)
        at = np.abs(xyz[j[dist == 20.0]] - xyz[i[dist == 20.0]]) / 4.0
        kinds = {tuple(sorted(v)) for v in at.tolist()}
        assert kinds == {(0.0, 0.0, 5.0), (0.0, 3.0, 4.0)}
        assert (np.round(xyz[:, 0] / 4.0) % 5 == 0).sum() == 4 * 256      # planes 0, 5, 10, 15 lie on cell faces
    if name in R.LARGE:
        pos = np.empty(N, np.int64)
        pos[order] = np.arange(N)
        late = int((pos[charge != 0] >= 256 * R.SCAN_TILE).sum())
        print("   charged sites at cell-order positions >= 524288: %d" % late)
        assert tiles > 256 and late >= 100
        if name == "large_tail":
            assert int((charge != 0).sum()) == 3000 and pos[charge != 0].min() == N - 3000
            assert per_tile[:-2].sum() == 0 and per_tile[256:].sum() == 3000
            assert np.array_equal(xyz, R.pairwise_case("large")["xyz"])
    if name in R.TILE_EDGE:
        # the one charged site is the last item of the scan: of a tile one short, of a full tile, alone in a second tile;
        # every term of the result is its term
        assert N in R.TILE_EDGE_SIZES and nc == (3, 3, 3) and np.flatnonzero(flags).tolist() == [N - 1]
        assert per_tile.tolist() == ([1] if N <= R.SCAN_TILE else [0, 1])
        assert n.max() == 1 and (n > 0).sum() >= 100 and n[order[-1]] == 0
    # the zero pattern of the result is part of the bar: sites without a term exist wherever the case can have them
    if name in ("large", "large_tail", "one_site", "seventeen", "thin_uncharged") + R.TILE_EDGE:
        assert (n == 0).any()


# ------------------------------------------------------------------------------------------------ charge inputs
@pytest.mark.parametrize("name", sorted(R.CHARGE_CASES))
def test_charge_input_holds_its_crafted_rows(name):
    c = R.charge_case(name)
    N, nn, rows, displ = c["N"], c["nn"], c["row_count"], c["displ"]
    assert c["neigh"].shape == (rows, nn) and c["neigh"].max() < N and c["neigh"].min() >= -1
    assert len(c["crafted"]) == min(rows, len(R._crafted(nn)))
    for site, expect in c["crafted"]:
        assert c["want"][site] == expect, (site, expect)
    el, want = c["element"], c["want"]
    inside = np.zeros(N, bool)
    inside[displ:displ + rows] = True
    touched = inside & ((el == R.VACANCY) | (el == R.OXYGEN_DEFECT))
    assert np.all(want[~touched] == 7) and set(want[touched].tolist()) <= {0, 2, -2}
    assert int(c["metals"][-1]) in el.tolist()
    if rows >= 300:
        assert {0, 2, -2, 7} == set(want.tolist())
        if displ:
            far = c["neigh"][c["neigh"] >= 0]
            assert (far < displ).any() and (far >= displ + rows).any()       # the look-ups are global
            assert (want[:displ] == 7).all() and (el[:displ] == R.VACANCY).any()
    if name == "stride":
        assert rows > 2048 * 16
    if name == "rows1_slot16":
        assert c["neigh"][0, 16] >= 0 and (np.delete(c["neigh"][0], 16) != c["neigh"][0, 16]).all()


def test_charge_crafted_rows_cover_what_they_are_for():
    assert {c[1] for c in R.CHARGE_CASES.values()} == {1, 15, 16, 17, 52}
    assert {c[2] for c in R.CHARGE_CASES.values()} >= {1, 16, 17, 300}
    assert {c[4] for c in R.CHARGE_CASES.values()} == {1, 2, 3}
    rows = R._crafted(52)
    assert (R.VACANCY, {51: "M"}, "O", 0) in rows and (R.VACANCY, {16: "M"}, "O", 0) in rows
    assert (R.VACANCY, {3: "V", 12: "V"}, "O", 0) in rows and (R.OXYGEN_DEFECT, {3: "V", 12: "V"}, "O", -2) in rows
    assert (R.VACANCY, {3: "V"}, "O", 2) in rows and (R.VACANCY, {}, None, 2) in rows


# ------------------------------------------------------------------------------------------------ K inputs
@pytest.mark.parametrize("name", R.K_DEVICES)
def test_k_device_meets_its_conditions(oracle, name):
    dev = R.k_device(name)
    xyz, NL, n, L = dev["xyz"], dev["NL"], dev["n"], dev["lattice"]
    assert np.all(np.diff(xyz[:, 0]) >= 0) and np.all(xyz >= 0) and np.all(xyz < L)
    assert np.array_equal(dev["neigh"], oracle.neighbor_list(xyz[:, 0], xyz[:, 1], xyz[:, 2], R.K_CHARGE_NN_DIST, R.K_CHARGE_NN))
    assert (dev["neigh"][:, -1] == -1).all()                   # no row of the charge list is truncated
    for pbc in (0, 1):
        pats = R.k_patterns(dev, pbc)
        for (rp, col), (c0, nc) in zip(pats, ((NL, n), (0, NL), (NL + n, NL))):
            rp_o, col_o = oracle.pattern(xyz[:, 0], xyz[:, 1], xyz[:, 2], L, pbc, R.K_NN_DIST, n, nc, NL, c0)
            assert np.array_equal(rp, rp_o) and np.array_equal(col, col_o)
        rp, col = pats[0]
        length = np.diff(rp)
        print("%s pbc %d: %d rows, %.1f entries per row, longest %d, left %d, right %d contact entries"
              % (name, pbc, n, length.mean(), length.max(), len(pats[1][1]), len(pats[2][1])))
        assert length.min() >= 2 and len(pats[1][1]) > 100 and len(pats[2][1]) > 100
        if name == "dense":
            assert length.max() <= 64 and (length.mean() >= 40 if pbc else length.mean() >= 36)
            assert 64 * length.mean() > 1.15 * 2040                      # 64 average rows overflow a tile's entry limit
        shares = R.k_pair_shares(dev, rp, col, dev["charge"])
        print("   ", {k: round(v, 3) for k, v in shares.items()})
        assert min(shares.values()) >= 0.05, shares
    assert np.array_equal(dev["charge"], oracle.update_charge(dev["element"], np.zeros(dev["N"], np.int32), dev["neigh"], dev["metals"]))
    vac = dev["element"] == R.VACANCY
    assert np.array_equal(dev["charge2"][vac], 2 - dev["charge"][vac]) and np.array_equal(dev["charge2"][~vac], dev["charge"][~vac])


def test_window_tiles_on_hand_made_rows():
    rp = np.arange(0, 131 * 30, 30)                 # 130 rows of 30 entries: 64-row tiles (1920 entries)
    col = np.tile(np.arange(30), 130)
    ends, why = R.window_tiles(rp, col)
    assert ends.tolist() == [64, 128, 130] and why == ["rows", "rows", "end"]
    rp = np.arange(0, 101 * 45, 45)                 # 100 rows of 45: 45 rows make 2025 entries, 46 exceed 2040
    ends, why = R.window_tiles(rp, np.tile(np.arange(45), 100))
    assert ends.tolist() == [45, 90, 100] and why == ["entries", "entries", "end"]
    ends, why = R.window_tiles(rp, np.arange(4500))  # all columns distinct: 22 rows hold 990, 23 hold 1035 > 1024
    assert ends[0] == 22 and why[0] == "columns"


# ------------------------------------------------------------------------------------------------ heat inputs
@pytest.mark.parametrize("N", R.HEAT_SIZES)
def test_heat_power_cancels(N):
    p = R.heat_power(N)
    assert len(p) == N
    if N >= 255:
        mag = np.abs(p)
        assert mag.min() < 1e-14 and mag.max() > 1e-7 and 1e-15 <= mag.min() and mag.max() <= 1e-6
        ratio = abs(math.fsum(p.tolist())) / math.fsum(mag.tolist())
        assert 3e-4 <= ratio <= 3e-3, ratio
        assert (p > 0).sum() >= N // 2 and (p < 0).sum() >= N // 2 - 1
    a = R.HEAT_ARGS
    term = math.fsum(np.abs(p).tolist()) * a["small_step"] / a["C"]
    if N >= 255:
        assert 0.03 * a["b"] <= term <= 100 * a["b"]      # the power term is visible next to b, neither drowns the other
    assert R.heat_bar(p, 300.0, **a) > 0


def test_heat_sizes_straddle_the_grid_cap():
    assert {0, 1, 255, 257} <= set(R.HEAT_SIZES) and 262144 in R.HEAT_SIZES       # 1024 blocks of 256: the last size without a stride
    assert max(R.HEAT_SIZES) > 2 * 262144 and max(R.HEAT_SIZES) % 256 != 0
