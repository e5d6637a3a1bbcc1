"""CPU: the local heat solve's C ABI (kmcf_update_temperature_local) and the numpy restatement of its system
(tests/heat_local_ref.py) that the GPU tests hold the library to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import heat_local_ref as H

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
