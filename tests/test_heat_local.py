"""CPU: the local heat solve's C ABI (kmcf_update_temperature_local) and the numpy restatement of its system
(tests/heat_local_ref.py) that the GPU tests hold the library to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import heat_local_ref as H
import site_kernels_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMCF_ERR_ARG = -1

PRM5 = dict(background_temp=300.0, k_th_metal=29.0, k_th_vacancies=5.0, k_th_non_vacancy=0.5, L_char=3.5e-10, c_p=1.92,
            A=51.15e-10 * 51.15e-10, t_ox=52.6838e-10, delta_t=1e-13)


def _header():
    hdr = open(os.path.join(ROOT, "include", "kmcfield.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_symbol_exported(km):
    lib = km.lib.load()
    assert hasattr(lib, "kmcf_update_temperature_local")
    assert "kmcf_update_temperature_local" in km.lib.SIGNATURES


def test_argtypes_match_header(km):
    hdr = _header()
    m = re.search(r"int\s+kmcf_update_temperature_local\s*\(([^)]*)\)", hdr)
    assert m, "prototype not found"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    res, args = km.lib.SIGNATURES["kmcf_update_temperature_local"]
    assert res is C.c_int and len(args) == len(params) == 15
    for p, a in zip(params, args):
        if "*" in p:
            assert a is C.c_void_p or hasattr(a, "_type_") and issubclass(a, C._Pointer), (p, a)
            if "kmcf_heat_params_t" in p:
                assert a._type_ is km.lib.HeatParams
            elif "kmcf_solve_stats_t" in p:
                assert a._type_ is km.lib.SolveStats
            elif p.startswith("double *h_"):
                assert a._type_ is C.c_double
            elif p.startswith("int *h_"):
                assert a._type_ is C.c_int
        elif p.startswith("int "):
            assert a is C.c_int, p
        elif p.startswith("double "):
            assert a is C.c_double, p
        else:
            raise AssertionError(p)
    # the parameter struct: same fields, same order, same types
    s = re.search(r"typedef struct \{([^}]*)\}\s*kmcf_heat_params_t;", hdr)
    fields = re.findall(r"(double|int)\s+(\w+);", s.group(1))
    got = [(n, t) for n, t in km.lib.HeatParams._fields_]
    assert [n for _, n in fields] == [n for n, _ in got]
    assert all((t == "double") == (ct is C.c_double) and (t == "int") == (ct is C.c_int) for (t, _), (_, ct) in zip(fields, got))


def test_null_state_is_refused_before_device_work(km):
    lib = km.lib.load()
    prm = km.solvers.heat_params()
    T_bg, steady = C.c_double(-1.0), C.c_int(-1)
    st = km.lib.SolveStats()
    rc = lib.kmcf_update_temperature_local(None, None, None, None, 0, None, None, 10, 1, 1, 1e-12, C.byref(prm),
                                           C.byref(T_bg), C.byref(steady), C.byref(st))
    assert rc == KMCF_ERR_ARG
    assert b"kmcf_update_temperature_local" in lib.kmcf_last_error() and b"null" in lib.kmcf_last_error()
    assert T_bg.value == -1.0 and steady.value == -1


@pytest.fixture(scope="module")
def sys5(oracle, dev5):
    d = dev5
    NL = d["N_contact"]
    ks = oracle.KSystem(d["xyz"], d["lattice"], d["pbc"], d["nn_dist"], NL, NL)
    nl = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], d["nn_dist"], 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), nl, d["metals"])
    cls = H.site_classes(d["element"], charge, d["metals"])
    Q = H.synthetic_power(d["element"], charge, d["metals"], 1e-8)
    return dict(ks=ks, cls=cls, Q=Q, d=d)


@pytest.mark.parametrize("step_time", [1e-13, 1.0])
def test_restatement_properties(sys5, step_time):
    ks, d = sys5["ks"], sys5["d"]
    T_old = np.full(d["N"], PRM5["background_temp"])
    s = H.heat_system(ks, sys5["cls"], PRM5, step_time, sys5["Q"], T_old)
    A = s["A"]
    assert s["steady"] == (step_time > 1e3 * PRM5["delta_t"])
    # the 5 nm conductances of the issue: 1.015e-8, 1.75e-9, 1.75e-10 W/K; C = 7.25e-24 J/K per site
    np.testing.assert_allclose(s["g"], [1.015e-8, 1.75e-9, 1.75e-10], rtol=1e-12)
    assert abs(s["C"] * ks.n - 2.646e-19) < 1e-21 and abs(s["C"] - 7.25e-24) < 1e-26
    # row sums = C/dt + gL + gR (the interface couplings cancel)
    rs = np.asarray(A.sum(axis=1)).ravel()
    np.testing.assert_allclose(rs, s["cdt"] + s["gL"] + s["gR"], rtol=0, atol=1e-12 * s["diag"].max())
    # symmetric, three distinct off-diagonal values, every diagonal positive
    assert abs(A - A.T).max() == 0.0
    off = A - __import__("scipy.sparse", fromlist=["diags"]).diags(A.diagonal())
    assert np.array_equal(np.unique(off.data[off.data != 0]), np.sort(-s["g"]))
    assert (A.diagonal() > 0).all()
    assert (s["gL"] > 0).sum() > 0 and (s["gR"] > 0).sum() > 0
    if s["steady"]:
        assert s["cdt"] == 0.0
    else:
        assert s["cdt"] == pytest.approx(7.251e-11, rel=1e-3)


# ------------------------------------------------------------------------------------------------ synthetic devices
# What tests/test_gpu_heat_synthetic.py rests on: the conditions its inputs are built for, that the two restatements
# agree, and that a plain float64 Jacobi-PCG to the library's stopping rule lies a factor 10 inside the GPU test's bar.


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def test_dictionary_codes_of_the_sets():
    assert set(H.HEAT_SETS) == set(H.HEAT_CODES)
    for kset, codes in H.HEAT_CODES.items():
        assert H.dictionary_codes(H.synth_params(kset)) == codes, kset
    assert sorted(len(set(c)) for c in H.HEAT_CODES.values()) == [1, 2, 2, 2, 3]
    assert H.HEAT_CODES["metal_eq_other"] == [0, 1, 0]


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("name", R.K_DEVICES)
def test_synthetic_device_holds_every_pair_class(name, pbc):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    dev = R.k_device(name)
    NL, n = dev["NL"], dev["n"]
    pats = H.synth_patterns(name, pbc)
    cls, cls2, Q, T_old = H.synth_inputs(name)
    assert np.array_equal(cls, H.site_classes(dev["element"], dev["charge"], dev["metals"]))
    assert not np.array_equal(cls, cls2) and (cls[NL:-NL] != cls2[NL:-NL]).sum() >= n // 10
    ref = H.heat_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], cls, H.synth_params("distinct"), 1e-15, Q, T_old, NL, n)
    cn, cl, cr = ref["counts"]
    share = cn.sum(0) / cn.sum()
    print("%s pbc %d: %d sites, metal-metal %.1f %%, vacancy-vacancy %.1f %%, other %.1f %% of %d off-diagonals; left %s, right %s"
          % (name, pbc, n, 100 * share[0], 100 * share[1], 100 * share[2], cn.sum(), cl.sum(0), cr.sum(0)))
    assert cn.sum() == ref["off_diagonal"].sum() and share.min() >= 0.05
    assert cl.sum(0).min() >= 10 and cr.sum(0).min() >= 10
    # one connected component, with rows on either contact
    rp, col = pats[0]
    ncomp, _ = connected_components(csr_matrix((np.ones(len(col)), col, rp), shape=(n, n)), directed=False)
    assert ncomp == 1
    assert (np.diff(pats[1][0]) > 0).any() and (np.diff(pats[2][0]) > 0).any()
    # no cancellation in any assembled quantity
    assert (Q >= 0).all() and (Q[NL:-NL] > 0).any() and (T_old > 0).all() and H.SYNTH_PRM["background_temp"] > 0
    assert np.all(T_old[:NL] == H.SENTINEL) and np.all(T_old[-NL:] == H.SENTINEL) and H.SENTINEL != H.SYNTH_PRM["background_temp"]
    assert np.ptp(T_old[NL:-NL]) > 1.0


@pytest.mark.parametrize("case", [c for c in H.synth_cases() if c[3] == "transient"], ids=lambda c: "-".join(map(str, c)))
def test_transient_step_makes_the_capacity_term_visible(case):
    name, pbc, kset, mode = case
    c = H.synth_case(*case)
    p, ref = c["p"], c["ref"]
    assert 0 < c["step_time"] <= 1e3 * p["delta_t"] and not ref["steady"]
    row_sum = (ref["diag"] - ref["cdt"]).astype(np.float64)
    ratio = float(ref["cdt"]) / np.median(row_sum)
    print("%s: C/dt = %.3g W/K, median row sum %.3g W/K, ratio %.2f" % (case, float(ref["cdt"]), np.median(row_sum), ratio))
    assert 0.1 <= ratio <= 10.0
    steady = H.synth_case(name, pbc, kset, "steady")
    assert steady["ref"]["steady"] and steady["ref"]["cdt"] == 0 and steady["step_time"] > 1e3 * p["delta_t"]


@pytest.mark.parametrize("case", H.synth_cases(), ids=lambda c: "-".join(map(str, c)))
def test_values_ref_agrees_with_the_restated_system(case):
    name, pbc = case[:2]
    c = H.synth_case(*case)
    ref, s = c["ref"], c["sys"]
    A = s["A"].tocsr()
    A.sort_indices()
    rp, col = H.synth_patterns(name, pbc)[0]
    assert np.array_equal(A.indptr, rp) and np.array_equal(A.indices, col)       # every pattern entry is a value of A
    off = ref["off_diagonal"]
    assert np.array_equal(A.data[off], ref["val"][off])
    assert ref["steady"] == s["steady"]
    worst = {"val diagonal": H.rel_error(A.data[~off], ref["diag"][ref["rows"][~off]]), "diag": H.rel_error(s["diag"], ref["diag"]),
             "rhs": H.rel_error(s["b"], ref["rhs"]), "left": H.rel_error(s["gL"], ref["left"]), "right": H.rel_error(s["gR"], ref["right"])}
    print(case, worst)
    # (heat_system adds a row's values one by one: up to 64 additions of positive terms, each 2^-53)
    assert max(worst.values()) <= 70 * 2.0 ** -53
    assert float(ref["cdt"]) == pytest.approx(s["cdt"], rel=1e-15)
    assert np.array_equal(ref["val"][~off], ref["diag"][ref["rows"][~off]].astype(np.float64))


@pytest.mark.parametrize("case", H.synth_cases(), ids=lambda c: "-".join(map(str, c)))
def test_float64_pcg_lands_on_the_direct_solve(case):
    name = case[0]
    c = H.synth_case(*case)
    NL = R.k_device(name)["NL"]
    p, s, T_ref = c["p"], c["sys"], c["T"]
    T0 = p["background_temp"]
    T_old = H.synth_inputs(name)[3]
    tol = H.SYNTH_CG["cg_tolerance"] / np.sqrt(s["g"].max())
    x, it = H.pcg_jacobi(s["A"].tocsr(), s["b"], T_old[NL:-NL], tol, H.SYNTH_CG["cg_max_iterations"])
    dT = np.abs(T_ref - T0).max()
    err = np.abs(x - T_ref[NL:-NL]).max()
    print("%s: %d iterations, max |T - T0| = %.4g K, |T_pcg - T_direct| = %.3g = %.2g of it" % (case, it, dT, err, err / dT))
    assert 0 < it < H.SYNTH_CG["cg_max_iterations"]
    assert dT > 1.0
    assert err <= 1e-9 * dT
