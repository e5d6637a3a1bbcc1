"""CPU: the per-line bias helpers of structure.py (crossbar_lines, line_bias, bias_scheme), the numpy restatement of the
per-site contact right-hand side (tests/line_bias_ref.py) against a hand-built example, and the conditions the GPU
tests (tests/test_gpu_line_bias.py) rely on in their input."""
import numpy as np
import pytest

import line_bias_ref as R


@pytest.fixture(scope="module")
def case(km):
    return R.crossbar_case()


def test_crossbar_lines_counts_and_cells(km, case):
    d = case["d"]
    N, NL = d["N"], d["N_contact"]
    assert (N, NL) == (26444, 336)
    word, bit, cell = km.structure.crossbar_lines(d)
    assert word.shape == bit.shape == (NL,) and cell.shape == (N,)
    assert np.bincount(word).tolist() == [168, 168] and np.bincount(bit).tolist() == [168, 168]
    assert sorted(set(cell.tolist())) == [-1, 0, 1, 2, 3]
    # every site of a cell lies under one word stripe and one bit stripe (the rule synth_crossbar_40nm carves with)
    L, period = d["lattice"][1], d["lattice"][1] / 2
    y, z = d["xyz"][:, 1], d["xyz"][:, 2]
    inside = cell >= 0
    w, b = cell[inside] // 2, cell[inside] % 2
    assert np.all((z[inside] >= w * period) & (z[inside] < (w + 0.52) * period))
    assert np.all((y[inside] >= b * period) & (y[inside] < (b + 0.52) * period))
    outside = ~inside
    assert np.all(((z[outside] % period) >= 0.52 * period) | ((y[outside] % period) >= 0.52 * period))
    # the contact sites carry the line of the cells above / below them
    assert np.all(z[:NL] // period == word) and np.all(y[N - NL:] // period == bit)
    assert L == pytest.approx(51.15)
    with pytest.raises(ValueError):
        km.structure.crossbar_lines(km.structure.synth_small(tiles=1))       # uncarved: contacts between the stripes


@pytest.mark.parametrize("scheme, want", [("all", [1, 1, 1, 1]), ("half", [1, 1 / 2, 1 / 2, 0]),
                                          ("third", [1, 1 / 3, 1 / 3, -1 / 3])])
@pytest.mark.parametrize("select", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_scheme_cell_voltages(km, case, scheme, select, want):
    """Cell voltage = bit line - word line: the selected cell, the cell sharing its word line, the one sharing its bit
    line, the unselected one."""
    d = case["d"]
    V = 15.0
    N, NL = d["N"], d["N_contact"]
    v = km.structure.bias_scheme(d, scheme, select=select, V=V)
    word, bit, _ = km.structure.crossbar_lines(d)
    assert v.shape == (N,) and np.all(v[NL:N - NL] == 0.0)
    word_V = [set(v[:NL][word == l].tolist()) for l in range(2)]
    bit_V = [set(v[N - NL:][bit == l].tolist()) for l in range(2)]
    assert all(len(s) == 1 for s in word_V + bit_V)              # one value per line
    wv, bv = [s.pop() for s in word_V], [s.pop() for s in bit_V]
    w, b = select
    got = [bv[b] - wv[w], bv[1 - b] - wv[w], bv[b] - wv[1 - w], bv[1 - b] - wv[1 - w]]
    np.testing.assert_allclose(got, np.array(want) * V, rtol=1e-15, atol=1e-15)
    assert wv[w] == -V / 2 and bv[b] == V / 2                    # K's sign convention: left -, right +
    if scheme == "all":                                          # the scalar call's boundary condition
        assert np.all(v[:NL] == -V / 2) and np.all(v[N - NL:] == V / 2)


def test_line_bias_and_scheme_arguments(km, case):
    d = case["d"]
    v = km.structure.line_bias(d, [1.0, 2.0], [-3.0, 4.0])
    word, bit, _ = km.structure.crossbar_lines(d)
    NL = d["N_contact"]
    assert np.array_equal(v[:NL], np.array([1.0, 2.0])[word]) and np.array_equal(v[-NL:], np.array([-3.0, 4.0])[bit])
    assert km.structure.bias_scheme(d, "half", select=(1, 0))[0] in (0.0, -d["Vd"] / 2)      # V defaults to the device's Vd
    with pytest.raises(ValueError):
        km.structure.bias_scheme(d, "quarter", select=(0, 0), V=1.0)
    with pytest.raises(ValueError):
        km.structure.bias_scheme(d, "half", select=(0, 2), V=1.0)
    with pytest.raises(ValueError):
        km.structure.line_bias(d, [1.0, 2.0], [1.0])


def test_rhs_restatement_on_a_hand_built_example():
    """Three interface rows between two left and two right contact sites.  Sites: 0, 1 left | 2, 3, 4 interface | 5, 6
    right.  Row 0 touches left 0 and 1 and right 0, row 1 nothing, row 2 right 1 and (listed first) right 0."""
    NL = 2
    cls = np.array([1, 1, 1, 0, 2, 1, 2], np.uint8)             # metal, metal | metal, oxide, vacancy | metal, vacancy
    V = np.array([-3.0, 0.5, 0, 0, 0, 2.0, 7.0])
    left_rp, left_col = np.array([0, 2, 2, 2]), np.array([0, 1])
    right_rp, right_col = np.array([0, 1, 1, 3]), np.array([0, 0, 1])
    hi, lo = 1.0, 1e-8
    rhs, n, S = R.contact_rhs(left_rp, left_col, right_rp, right_col, cls, NL, V, hi, lo)
    dense = np.zeros((3, 7))                                     # G_ij against every site
    dense[0, [0, 1, 5]] = hi                                     # metal row: high to the three metal contacts
    dense[2, 5], dense[2, 6] = lo, hi                            # vacancy row: low to the metal, high to the vacancy
    want = np.array([(hi * -3.0 + hi * 0.5) + hi * 2.0, 0.0, lo * 2.0 + hi * 7.0])
    assert np.array_equal(rhs, want)
    np.testing.assert_allclose(rhs, dense @ V, rtol=1e-15)
    assert n.tolist() == [3, 0, 2]
    np.testing.assert_allclose(S, np.abs(dense) @ np.abs(V), rtol=1e-15)
    # the same rows as the second rank of a group sees them (its patterns start at its first row)
    rhs1, n1, _ = R.contact_rhs(left_rp[1:] - left_rp[1], left_col[2:], right_rp[1:] - right_rp[1], right_col[1:], cls, NL, V,
                                hi, lo, row0=1)
    assert np.array_equal(rhs1, want[1:]) and n1.tolist() == [0, 2]


def test_input_conditions_of_the_gpu_tests(km, case):
    d = case["d"]
    NL, N = d["N_contact"], d["N"]
    n_int = N - 2 * NL
    cls = R.site_classes(d["element"], np.zeros(N, np.int32), d["metals"])
    used = []
    for side, (rp, col, base) in enumerate(((case["left_rp"], case["left_col"], 0), (case["right_rp"], case["right_col"], NL + n_int))):
        assert len(rp) == n_int + 1 and len(col) == 1556
        length = np.diff(rp)
        assert np.count_nonzero(length) == 336 and length.max() <= 5
        rows = np.repeat(np.arange(n_int), length)
        high = (cls[NL + rows] & cls[base + col]) != 0
        assert high.any() and (~high).any(), "both conductance classes among the contact pairs of side %d" % side
        assert sorted(set(col.tolist())) == list(range(NL))     # every contact site is used
        used.append(length)
    both = used[0] + used[1]
    assert (both >= 2).any() and (both == 0).any()
    assert np.count_nonzero(both) == 672
    # the matrix of the restatement: symmetric M-matrix, strictly dominant exactly in the rows with contact entries
    charge = np.zeros(N, np.int32)
    rp, col = _interface_pattern(d)
    K, diag = R.k_matrix(rp, col, case["left_rp"], case["left_col"], case["right_rp"], case["right_col"],
                         R.site_classes(d["element"], charge, d["metals"]), NL, d["high_G"], d["low_G"])
    assert abs(K - K.T).max() == 0.0
    slack = np.asarray(K.sum(axis=1)).ravel()
    assert np.all(slack[both > 0] > 0) and np.abs(slack[both == 0]).max() <= 1e-12 * diag.max()


def _interface_pattern(d):
    from scipy.spatial import cKDTree
    NL, N, r = d["N_contact"], d["N"], d["nn_dist"]
    mid = d["xyz"][NL:N - NL]
    pairs = cKDTree(mid).query_pairs(r * (1 + 1e-9), output_type="ndarray")
    keep = np.sqrt(((mid[pairs[:, 0]] - mid[pairs[:, 1]]) ** 2).sum(axis=1)) < r
    i, j = pairs[keep, 0], pairs[keep, 1]
    n = len(mid)
    rows = np.concatenate([i, j, np.arange(n)])
    cols = np.concatenate([j, i, np.arange(n)])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=n), out=rp[1:])
    return rp, cols[order].astype(np.int32)


def test_abi_and_host_side_checks(km):
    """The two entry points are declared, bound and exported, and refuse a NULL argument by name before anything needs
    a device."""
    import os
    import re
    lib = km.lib.load()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmcfield.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("kmcf_k_assemble_contacts", "kmcf_background_potential_sparse_contacts"):
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert decl, name
        res, args = km.lib.SIGNATURES[name]
        assert len(args) == decl.group(1).count(",") + 1 and hasattr(lib, name)
    assert lib.kmcf_k_assemble_contacts(None, None, None, None, 2, None, 1.0, 1e-8) == -1
    assert b"kmcf_k_assemble_contacts: k is NULL" in lib.kmcf_last_error()
    assert lib.kmcf_background_potential_sparse_contacts(None, None, None, None, 2, None, 10, 2, 2, 1.0, 1e-8, None) == -1
    assert b"kmcf_background_potential_sparse_contacts: k is NULL" in lib.kmcf_last_error()
