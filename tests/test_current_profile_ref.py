"""CPU: the restatement of kmcf_current_profile (tests/current_profile_ref.py) on a hand-written chain and on oracle
devices solved directly, and the C ABI of the call (symbol, argument errors, struct layout).  The GPU tests
(tests/test_gpu_current_profile.py) hold the device against this restatement."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import current_map_ref as R
import current_profile_ref as PR
from test_current_map_ref import DEVICES, G0
from test_oracle_T import PAR, make_T, small_device

A_LAT = 2.5


def _chain():
    """injection node 1 -- atom 0 -- atom 1 -- atom 2 -- extraction node 0 at x = 0, 1, 2: conductances 1, 2, 2, 4, and a
    tunnel pair atom 0 -- atom 2 of conductance 1 that spans both planes x = 0.5, 1.5; potentials 7, 3, 2, 1, 0 carry
    exactly 4 through the device, 2 of it through the tunnel pair.  A fourth atom has no row."""
    rows = {0: {0: 104.0, 1: -100.0, 4: -4.0}, 1: {0: -100.0, 1: 101.0, 2: -1.0}, 2: {1: -1.0, 2: 3.0, 3: -2.0},
            3: {2: -2.0, 3: 4.0, 4: -2.0}, 4: {0: -4.0, 3: -2.0, 4: 6.0}}
    rp, col, val = [0], [], []
    for r in range(5):
        for c in sorted(rows[r]):
            col.append(c)
            val.append(rows[r][c])
        rp.append(len(col))
    tunnel = dict(tunnel_idx=np.array([0, 2]), row_ptr=np.array([0, 2, 4]), col=np.array([0, 1, 0, 1]),
                  val=np.array([1.0, -1.0, -1.0, 1.0]), first=0)
    m = np.array([0.0, 7.0, 3.0, 2.0, 1.0, 0.0])
    xyz = np.array([[0.0, 0.0, 0.0], [1.0, 0.75, 0.0], [2.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    return R.pair_list(rp, col, val, 0, tunnel), m, xyz


def test_four_resistor_chain_is_exact():
    pairs, m, xyz = _chain()
    x = xyz[:, 0]
    one = np.zeros(4, np.int64)
    for form in ("direct", "nodes"):
        f = (lambda *a: PR.profile_direct(*a)["F"]) if form == "direct" else PR.profile_nodes
        # one cell, planes between the atoms: 2 through the bonds, 2 through the tunnel pair, at both planes
        F = f(pairs, m, x, [0.5, 1.5], one, 1)
        np.testing.assert_array_equal(F, [[[2.0, 2.0], [2.0, 2.0]], [[0.0, 0.0], [0.0, 0.0]]])
        np.testing.assert_array_equal(PR.total(F), [4.0, 4.0])
        # cells 0, 1, 0: the bonds join different cells (rest), the tunnel pair stays inside cell 0
        F = f(pairs, m, x, [0.5, 1.5], np.array([0, 1, 0, 2]), 2)
        np.testing.assert_array_equal(F[0], [[0.0, 2.0], [0.0, 2.0]])
        np.testing.assert_array_equal(F[1], np.zeros((2, 2)))
        np.testing.assert_array_equal(F[2], [[2.0, 0.0], [2.0, 0.0]])
        # a plane ON atom 1 leaves it to the right; a plane left of everything and one right of everything count nothing
        F = f(pairs, m, x, [-1.0, 1.0, 5.0], one, 1)
        np.testing.assert_array_equal(F[0], [[0.0, 0.0], [2.0, 2.0], [0.0, 0.0]])
        # a plane on atom 2: only atom 2 is right of it
        F = f(pairs, m, x, [2.0], one, 1)
        np.testing.assert_array_equal(F[0], [[2.0, 2.0]])
    d = PR.profile_direct(pairs, m, x, [0.5, 1.5], one, 1)
    assert d["n_crossing"] == 3                                 # each pair once, from its left end
    assert PR.flux_stats(d["F"]) == dict(flux_min=4.0, flux_max=4.0, plane_min=0, plane_max=0)
    # the vector: J = 1/2 sum I d
    v = PR.vector(pairs, m, xyz)
    np.testing.assert_array_equal(v["J"][:, 0], [3.0, 2.0, 3.0, 0.0])
    np.testing.assert_array_equal(v["J"][:, 1], [0.75, 0.0, -0.75, 0.0])
    np.testing.assert_array_equal(v["J"][:, 2], np.zeros(4))
    np.testing.assert_array_equal(v["n"], [2, 2, 2, 0])
    assert v["J"][:, 0].sum() == 1.0 * PR.total(d["F"]).sum() == 8.0
    # period 1 in y: the image of atom 1 at y = -0.25 is the nearer one
    vp = PR.vector(pairs, m, xyz, lattice=(9.0, 1.0, 9.0))
    np.testing.assert_array_equal(vp["J"][:, 0], v["J"][:, 0])
    np.testing.assert_array_equal(vp["J"][:, 1], [-0.25, 0.0, 0.25, 0.0])
    # halves round away from zero, as C's round() does
    np.testing.assert_array_equal(PR._round_away(np.array([0.5, -0.5, 1.5, 2.5, 0.25, -0.75])), [1.0, -1.0, 2.0, 3.0, 0.0, -1.0])
    # sites: atoms 0 .. 2 have rows
    np.testing.assert_array_equal(PR.to_sites(6, np.array([5, 2, 0, 3]), v["J"][:, 0]), [3.0, 0, 2.0, 0, 0, 3.0])


@pytest.mark.parametrize("kw", DEVICES, ids=["default", "2x2x3", "seed3_6x5", "8x8x9"])
def test_oracle_devices(oracle, kw):
    """The merged operator solved by sparse LU, planes at every mid-layer."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    d = small_device(**kw)
    x = d["xyz"][:, 0]
    T = make_T(oracle, d, x_lo=x.min() + 0.1, x_hi=x.max() - 0.1)
    m = np.zeros(T.N_atom + 2)
    m[:T.Nsub] = spl.spsolve(sp.csc_matrix(T.merged_csr()), T.rhs) * G0
    tn = dict(tunnel_idx=T.tunnel_idx, row_ptr=T.sub_row_ptr, col=T.sub_col, val=T.sub_val, first=0)
    pairs = R.pair_list(T.row_ptr, T.col, T.val, 0, tn)
    res = R.node_sums(T.Nsub, *pairs, m)
    xyz = np.stack([T.ax, T.ay, T.az], 1)
    layers = np.unique(T.ax)
    np.testing.assert_allclose(np.diff(layers), A_LAT)
    planes = layers[:-1] + 0.5 * A_LAT
    P, na = len(planes), T.N_atom
    ny = kw.get("ny", 4)
    # 2 x 2 cells cut in y-z, and one cell
    cell4 = (2 * (T.ay >= 0.5 * ny * A_LAT - 0.5 * A_LAT) + (T.az >= 0.5 * kw.get("nz", 4) * A_LAT - 0.5 * A_LAT)).astype(np.int64)
    for cell, n_cells in ((np.zeros(na, np.int64), 1), (cell4, 4)):
        dr = PR.profile_direct(pairs, m, T.ax, planes, cell, n_cells)
        Fn = PR.profile_nodes(pairs, m, T.ax, planes, cell, n_cells)
        ratio = float((np.abs(Fn - dr["F"]) / np.maximum(dr["bound"], 1e-300)).max())
        print("%d cells: node form against direct form, largest difference %.3f of the bound" % (n_cells, ratio))
        assert np.all(np.abs(Fn - dr["F"]) <= dr["bound"])
        if n_cells == 1:
            assert not dr["F"][1].any() and not Fn[1].any()       # no rest with one cell
            one = dr
        else:
            assert np.abs(dr["F"][4]).max() > 0
            np.testing.assert_allclose(dr["F"].sum(0), one["F"].sum(0), rtol=0, atol=float(one["bound"].sum(0).max()))
    F, bound = one["F"], one["bound"]
    tot = PR.total(F)
    q = PR.slabs(planes, T.ax)
    # conservation: left of plane k all atoms bonded to a virtual node belong to node 1, right of it every atom with the
    # ground start value (those within nn_dist of the last atom) and every atom bonded to node 0
    r, c = pairs[0], pairs[1]
    inj, ext = c[r == 1] - 2, c[r == 0] - 2
    ground = np.nonzero(np.sqrt(((xyz[:-1] - xyz[-1]) ** 2).sum(1)) < PAR["nn_dist"])[0]
    net = res["net"][2:2 + na]
    checked = 0
    for k in range(P):
        if q[inj].max() <= k < min(q[ground].min(), q[ext].min()):
            left = q <= k
            tol = float(np.abs(net[left[:len(net)]]).sum()) + float(bound[:, k, :].sum())
            assert abs(tot[k] - res["net"][1]) <= tol, (k, tot[k], res["net"][1], tol)
            assert abs(tot[k] - res["net"][1]) <= 1e-6 * abs(res["net"][1])        # (and that is tight: the solve conserves)
            checked += 1
    assert checked >= P - 3 and checked >= 1, (checked, P)
    print("I = %.6e at %d of %d planes; total at the last plane %.6e" % (res["net"][1], checked, P, tot[-1]))
    # sum_a jx[a] = h sum_k F_total[k]
    v = PR.vector(pairs, m, xyz)
    lhs, rhs = math.fsum(v["J"][:, 0]), A_LAT * math.fsum(tot)
    tol = float(v["bound"][:, 0].sum()) + A_LAT * float(bound.sum())
    print("sum jx %.15e against h sum F %.15e (difference %.2e, bound %.2e)" % (lhs, rhs, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol and lhs > 0
    # tunnel share: exactly zero wherever no tunnel point lies on both sides
    qt = q[np.asarray(T.tunnel_idx)]
    share = []
    for k in range(P):
        both = (qt <= k).any() and (qt > k).any()
        if not both:
            assert not F[:, k, 1].any()
        share.append(F[0, k, 1] / tot[k])
    assert max(share) > 0.5
    print("tunnel share per plane: " + " ".join("%.3f" % s for s in share))


def _planes(*v):
    return (C.c_double * len(v))(*v)


def test_symbol_and_argument_errors(km):
    lib = km.lib.load()
    assert "kmcf_current_profile" in km.lib.SIGNATURES and hasattr(lib, "kmcf_current_profile")
    one = C.c_void_p(8)                                            # (never dereferenced: these checks come first)
    x3, out = _planes(0.5, 1.5, 2.5), (C.c_double * 64)()

    def call(t=one, pot=one, cell=None, n_cells=1, x=x3, n=3, prof=out, jx=None, jy=None, jz=None):
        return lib.kmcf_current_profile(t, pot, cell, n_cells, x, n, prof, jx, jy, jz, None)

    def err(name, **kw):
        assert call(**kw) == -1, kw                                # KMCF_ERR_ARG
        msg = lib.kmcf_last_error()
        assert b"kmcf_current_profile" in msg and name in msg, (kw, msg)

    err(b"(t)", t=None)
    err(b"d_atom_virtual_potentials", pot=None)
    err(b"h_plane_x", x=None)
    err(b"h_profile", prof=None)
    for n in (0, -1, 1025):
        err(b"n_planes", n=n)
    for n in (0, -1, 1025):
        err(b"n_cells", n_cells=n, cell=one)
    err(b"d_site_cell", n_cells=2)
    err(b"h_plane_x", x=_planes(0.5, float("nan"), 2.5))
    err(b"h_plane_x", x=_planes(0.5, float("inf"), 2.5))
    err(b"h_plane_x", x=_planes(0.5, 0.5, 2.5))
    err(b"h_plane_x", x=_planes(0.5, 2.5, 1.5))
    for some in (dict(jx=one), dict(jy=one), dict(jz=one), dict(jx=one, jy=one), dict(jx=one, jz=one), dict(jy=one, jz=one)):
        err(b"d_site_jx", **some)


def test_stats_struct_has_the_c_layout(km):
    """kmcf_current_profile_stats_t: five doubles, two ints, two floats."""
    St = km.lib.CurrentProfileStats
    names = [n for n, _ in St._fields_]
    assert names == ["i_injection", "i_extraction", "flux_min", "flux_max", "sum_jx", "plane_min", "plane_max", "ms_pairs", "ms_planes"]
    assert [getattr(St, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 44, 48, 52]
    assert C.sizeof(St) == 56
    # ... and the header declares the fields in this order (several declarators to a line)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmcfield.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} kmcf_current_profile_stats_t;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = [(t, n.strip()) for t, ns in re.findall(r"(double|int|float)\s+([\w\s,]+);", body) for n in ns.split(",")]
    assert [n for _, n in decl] == names
    ctype = {"double": C.c_double, "int": C.c_int, "float": C.c_float}
    assert [ctype[t] for t, _ in decl] == [t for _, t in St._fields_]
    # the prototype is there with its eleven parameters
    proto = re.search(r"int kmcf_current_profile\(([^;]*)\);", hdr).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", proto, flags=re.S).split(",")) == 11 == len(km.lib.SIGNATURES["kmcf_current_profile"][1])
