"""CPU: the dense T-path reference (tests/tpath_ref.py) against the oracle (oracle/kmcf_oracle_T.c) -- two restatements
of the same device formulation written apart from each other -- on every synthetic case, at the bars of
tests/test_gpu_tpath.py: integer work identical, neighbour off-diagonals identical, diagonals / preconditioner / rhs
rtol 1e-13, WKB values and the tunnel diagonal rtol 1e-10 with exact zeros exact, I_macro 1e-11 of its absolute terms,
power 1e-11 of its maximum.  Then what every case is built for (tpath_ref.BUILT_FOR; each count non-zero), and the
reference against itself."""
import numpy as np
import pytest

import tpath_ref as R

G0 = 2 * 3.8612e-5 * 1e-5


def _oracle_T(oracle, case, Vd=None):
    p = case["par"]
    return oracle.TSystem(case["xyz"], case["element"], case["charge"], case["cb"], case["metals"], p["nn_dist"], case["n1"], case["n1"],
                          case["layers"], p["Vd"] if Vd is None else Vd, p["high_G"], p["low_G"], p["loop_G"], p["tol"], p["m_e"], p["V0"],
                          x_lo=case["x_lo"], x_hi=case["x_hi"])


def _same_zeros(a, b):
    """entries that are exactly 0.0 in one are exactly +-0.0 in the other"""
    np.testing.assert_array_equal(a == 0, b == 0)


@pytest.mark.parametrize("name", R.CASES)
def test_reference_equals_oracle(oracle, name):
    case = R.tpath_case(name)
    ref = R.case_ref(name)
    T = _oracle_T(oracle, case)
    assert ref.N_atom == T.N_atom and ref.n_t == T.n_t
    np.testing.assert_array_equal(ref.atom_site, T.atom_site)
    np.testing.assert_array_equal(ref.tunnel_idx, T.tunnel_idx)
    rp, col, val = ref.neighbour_csr()
    np.testing.assert_array_equal(rp, T.row_ptr)
    np.testing.assert_array_equal(col, T.col)
    rows = np.repeat(np.arange(T.Nsub), np.diff(rp))
    off = col != rows
    np.testing.assert_array_equal(val[off], T.val[off])
    np.testing.assert_allclose(val[~off], T.val[~off], rtol=1e-13, atol=0)
    np.testing.assert_allclose(ref.diag_neigh, T.diag_neigh, rtol=1e-13, atol=0)
    np.testing.assert_allclose(ref.diag, T.diag, rtol=1e-13, atol=0)
    np.testing.assert_allclose(ref.dinv, T.dinv, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(ref.rhs, T.rhs)
    srp, scol, sval = ref.tunnel_csr()
    np.testing.assert_array_equal(srp, T.sub_row_ptr)
    np.testing.assert_array_equal(scol, T.sub_col)
    _same_zeros(sval, T.sub_val)
    np.testing.assert_allclose(sval, T.sub_val, rtol=1e-10, atol=0)
    _same_zeros(ref.diag_tunnel, T.diag_tunnel)
    np.testing.assert_allclose(ref.diag_tunnel, T.diag_tunnel, rtol=1e-10, atol=0)
    if len(sval):
        nz = T.sub_val != 0
        print("%s: WKB values agree within %.2e relative" % (name, float(np.abs(sval[nz] / T.sub_val[nz] - 1).max()) if nz.any() else 0.0))
    # merged operator: the oracle's split product against the dense longdouble M
    x = np.cos(np.arange(T.Nsub) * 0.7) + 1.5
    want = (ref.M @ x.astype(R.LD))
    bound = np.abs(ref.M) @ np.abs(x).astype(R.LD)
    assert np.all(np.abs(T.spmv(x) - want) <= 1e-13 * bound)
    # current and power on one prescribed potential vector, both signs of the bias
    for Vd in (case["par"]["Vd"], -case["par"]["Vd"]):
        Tv = T if Vd == case["par"]["Vd"] else _oracle_T(oracle, case, Vd)
        m = np.zeros(T.N_atom + 2)
        m[:T.Nsub] = R.potentials(ref, Vd) * G0
        im, imo = ref.imacro(m), Tv.imacro(m)
        assert abs(im - imo) <= 1e-11 * ref.imacro_scale(m), (im, imo)
        pw, ms = ref.power(m, Vd, 1.0)
        pwo = np.full(len(case["element"]), -7.0)
        mo = m.copy()
        Tv.power(mo, 1.0, pwo)
        np.testing.assert_array_equal(ms, mo)
        np.testing.assert_array_equal(pw == -7.0, pwo == -7.0)
        w = pw != -7.0
        assert w.any() and np.abs(pw - pwo).max() <= 1e-11 * np.abs(pw[w]).max()


_printed = set()


@pytest.mark.parametrize("name", R.CASES)
def test_case_is_built_for_its_edge(name):
    case = R.tpath_case(name)
    e = R.case_ref(name).edges()
    if name not in _printed:
        _printed.add(name)
        print("\n%s: %s" % (name, ", ".join("%s=%s" % kv for kv in e.items() if kv[1] not in (0, None, False))))
    assert e["N_atom"] <= 700
    want = case["built_for"]
    assert want, "a case without a stated purpose"
    for k, v in want.items():
        assert e[k] == v, (name, k, e[k], v)
        if name.endswith("_edges"):
            assert e[k], (name, k)      # every listed edge is there: no count is zero
    # atom index != site index in every case (the interstitials are interleaved)
    ref = R.case_ref(name)
    assert (ref.atom_site != np.arange(ref.N_atom)).any()
    # x-ordered atoms (what the contact rules by atom index assume): no atom lies left of an atom a layer before it
    x = ref.pos[:, 0]
    assert np.all(np.diff(x) > -1e-9)


@pytest.mark.parametrize("name", R.CASES)
def test_reference_against_itself(name):
    ref = R.case_ref(name)
    S = ref.S
    np.testing.assert_array_equal(S, S.T)                         # |dCB| and the distance are symmetric, so is the value
    np.testing.assert_array_equal(ref.S_pattern, ref.S_pattern.T)
    if ref.n_t:
        assert np.all(np.abs(S.astype(R.LD).sum(1)) <= 2e-16 * np.abs(S).astype(R.LD).sum(1))      # rows sum to zero (the diagonal was rounded once)
        assert np.all(np.diag(S) >= 0) and np.all(S[~np.eye(ref.n_t, dtype=bool)] <= 0)
    np.testing.assert_array_equal(ref.M, ref.M.T)
    np.testing.assert_array_equal(ref.A, ref.A.T)
    # a Kirchhoff matrix with the ground cut: weakly diagonally dominant, strictly in the rows that touch the ground
    offsum = np.abs(ref.M).sum(1) - np.abs(np.diag(ref.M))
    assert np.all(np.diag(ref.M) >= offsum * (1 - 1e-15))
    assert np.diag(ref.M)[0] > offsum[0]
    m = {}
    for Vd in (2.0, -2.0):
        m[Vd] = np.zeros(ref.N_atom + 2)
        m[Vd][:ref.Nsub] = R.potentials(ref, Vd) * G0
        pw, ms = ref.power(m[Vd], Vd, 1.0)
        w = pw != -7.0
        metal_sites = np.isin(ref.el, ref.metals)
        written = np.zeros(ref.N_site, bool)
        written[ref.atom_site[:-1][~metal_sites[:-1]]] = True
        np.testing.assert_array_equal(w, written)                 # metals, interstitials and the cut atom keep the sentinel
        assert np.all(pw[w] >= 0) and pw[w].max() > 0
        assert ms[2:].min() == 0 or m[Vd][2:].min() >= 0
    # the noise of the two vectors is the same and the profile mirrors: m(-Vd) = -m(Vd) + 2 noise; on the mirrored vector
    # itself the current flips exactly
    assert ref.imacro(-m[2.0]) == -ref.imacro(m[2.0])
    assert ref.imacro(m[2.0]) * ref.imacro(m[-2.0]) < 0
    pw_p, _ = ref.power(m[2.0], 2.0, 1.0)
    pw_n, _ = ref.power(-m[2.0], -2.0, 1.0)                       # mirrored potentials under the mirrored bias: the same heat
    w = pw_p != -7.0
    assert np.abs(pw_p[w] - pw_n[w]).max() <= 1e-10 * pw_p[w].max()       # (the two shifts round the differences differently)
    assert np.all(R.ref_of(R.tpath_case(name), Vd=-2.0).rhs == -ref.rhs)
