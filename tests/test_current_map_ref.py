"""CPU: the restatement of kmcf_current_map (tests/current_map_ref.py) on a hand-written chain and on oracle devices
solved directly, and the C ABI of the call (symbol, argument errors, struct layout).  The GPU tests
(tests/test_gpu_current_map.py) hold the device against this restatement."""
import ctypes as C

import numpy as np
import pytest

import current_map_ref as R
from test_oracle_T import PAR, make_T, small_device

G0 = 2 * 3.8612e-5 * 1e-5


def test_three_resistor_chain():
    """injection node 1 -- atom 0 -- atom 1 -- extraction node 0, conductances 1, 2 (a tunnel pair), 4 and a loop entry
    (0, 1) that is no pair; potentials 7, 3, 1, 0 carry exactly 4 through every resistor."""
    # nodes: 0 extraction, 1 injection, 2 = atom 0, 3 = atom 1; neighbour rows with their diagonals
    rows = {0: {0: 104.0, 1: -100.0, 3: -4.0}, 1: {0: -100.0, 1: 101.0, 2: -1.0}, 2: {1: -1.0, 2: 1.0}, 3: {0: -4.0, 3: 4.0}}
    rp, col, val = [0], [], []
    for r in range(4):
        for c in sorted(rows[r]):
            col.append(c)
            val.append(rows[r][c])
        rp.append(len(col))
    tunnel = dict(tunnel_idx=np.array([0, 1]), row_ptr=np.array([0, 2, 4]), col=np.array([0, 1, 0, 1]),
                  val=np.array([2.0, -2.0, -2.0, 2.0]), first=0)
    m = np.array([0.0, 7.0, 3.0, 1.0])
    res = R.from_parts(4, rp, col, val, m, 0, tunnel)
    np.testing.assert_array_equal(res["through"], [2.0, 2.0, 4.0, 4.0])
    assert res["through"][2] == res["through"][3]
    np.testing.assert_array_equal(res["net"], [-4.0, 4.0, 0.0, 0.0])
    np.testing.assert_array_equal(res["tunnel"], [0.0, 0.0, 2.0, 2.0])
    np.testing.assert_array_equal(res["n"], [1, 1, 2, 2])                     # the (0, 1) entries are not counted
    assert res["pairs"] == 6
    # a third atom without a row (the cut ground atom): sites 5, 2 hold the two atoms, 9 keeps 0
    atom_site = np.array([5, 2, 9])
    np.testing.assert_array_equal(R.to_sites(10, atom_site, res["through"]), [0, 0, 4.0, 0, 0, 4.0, 0, 0, 0, 0])
    st = R.stats(res, atom_site)
    assert st == dict(i_injection=4.0, i_extraction=4.0, sum_through=8.0, sum_tunnel=4.0, max_through=4.0, max_site=5,
                      tunnel_pairs_walked=2)
    # only differences of m enter: a shift that is exact in floating point changes nothing
    res2 = R.from_parts(4, rp, col, val, m + 8.0, 0, tunnel)
    for k in ("through", "tunnel", "net"):
        np.testing.assert_array_equal(res[k], res2[k])


DEVICES = [dict(), dict(ny=2, nz=2, n_oxide_layers=3), dict(seed=3, ny=6, nz=5), dict(ny=8, nz=8, n_oxide_layers=9)]


@pytest.mark.parametrize("kw", DEVICES, ids=["default", "2x2x3", "seed3_6x5", "8x8x9"])
def test_oracle_devices_conserve_current(oracle, kw):
    """The merged operator solved by sparse LU: Kirchhoff's law at every atom away from the cut ground atom, the injected
    current equal to the oracle's I_macro, and the sum of all residuals zero (every pair is stored from both ends)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    d = small_device(**kw)
    x = d["xyz"][:, 0]
    T = make_T(oracle, d, x_lo=x.min() + 0.1, x_hi=x.max() - 0.1)
    assert T.n_t > 0
    M = T.merged_csr()
    m = np.zeros(T.N_atom + 2)
    m[:T.Nsub] = spl.spsolve(sp.csc_matrix(M), T.rhs) * G0
    res = R.from_tsystem(T, m)
    # the pairs are the off-diagonals of the merged operator minus (0, 1) / (1, 0)
    Mc = M.tocoo()
    off = (Mc.row != Mc.col) & ~((Mc.row < 2) & (Mc.col < 2))
    assert res["pairs"] == int(off.sum())
    np.testing.assert_array_equal(np.sort(res["r"]), np.sort(Mc.row[off]))
    # Kirchhoff: atoms farther than nn_dist from the last atom (the others carry the +high_G start value on the diagonal)
    pos = np.stack([T.ax, T.ay, T.az], 1)
    far = np.sqrt(((pos[:-1] - pos[-1]) ** 2).sum(1)) >= PAR["nn_dist"]
    net, th = res["net"][2:], res["through"][2:]
    worst = float((np.abs(net[far]) / np.maximum(th[far], 1e-300)).max())
    print("largest |net| / through at an interior atom: %.2e" % worst)
    assert np.all(np.abs(net[far]) <= 1e-7 * th[far]), worst
    assert (~far).any() and np.abs(net[~far]).max() > 1e-3 * th[~far].max()      # ... and there the residual is the current
    # injected current
    im = T.imacro(m)
    assert abs(res["net"][1] - im) <= res["n"][1] * R.EPS * res["S"][1], (res["net"][1], im)
    assert res["net"][1] > 0 and res["net"][0] < 0
    # antisymmetry: I_rc + I_cr = 0 exactly, so the sum of all residuals is rounding only
    assert abs(res["net"].sum()) <= res["pairs"] * R.EPS * res["S"].sum()
    # tunnel share is part of the whole
    assert np.all(res["tunnel"] <= res["through"]) and res["tunnel"].sum() > 0


def test_symbol_and_argument_errors(km):
    lib = km.lib.load()
    assert "kmcf_current_map" in km.lib.SIGNATURES and hasattr(lib, "kmcf_current_map")
    one = C.c_void_p(8)                                            # (never dereferenced: the NULL checks come first)
    assert lib.kmcf_current_map(None, one, one, None, None, None) == -1
    assert b"kmcf_current_map" in lib.kmcf_last_error() and b"state" in lib.kmcf_last_error()
    # the other two need a state to get that far: any non-NULL pointer will do, it is not looked at before the checks
    assert lib.kmcf_current_map(one, None, one, None, None, None) == -1
    assert b"d_atom_virtual_potentials" in lib.kmcf_last_error()
    assert lib.kmcf_current_map(one, one, None, None, None, None) == -1
    assert b"d_site_current" in lib.kmcf_last_error()


def test_stats_struct_has_the_c_layout(km):
    """kmcf_current_map_stats_t: five doubles, two ints, one float, padded to a multiple of 8."""
    St = km.lib.CurrentMapStats
    names = [n for n, _ in St._fields_]
    assert names == ["i_injection", "i_extraction", "sum_through", "sum_tunnel", "max_through", "max_site",
                     "tunnel_pairs_walked", "ms"]
    assert [getattr(St, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44, 48]
    assert C.sizeof(St) == 56
    # ... and the header declares the fields in this order
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmcfield.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} kmcf_current_map_stats_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(double|int|float)\s+(\w+)\s*;", body)
    assert [n for _, n in decl] == names
    ctype = {"double": C.c_double, "int": C.c_int, "float": C.c_float}
    assert [ctype[t] for t, _ in decl] == [t for _, t in St._fields_]
