"""GPU: the local heat solve (kmcf_update_temperature_local) on the reference's 5 nm device against the scipy
restatement of its system (tests/heat_local_ref.py), its physics, its warm start, its rank groups, its argument
checks, and that it leaves K's solve exactly as it found it; once on the synthetic 40 nm crossbar."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import heat_local_ref as H

pytestmark = pytest.mark.gpu

PRM5 = dict(background_temp=300.0, k_th_metal=29.0, k_th_vacancies=5.0, k_th_non_vacancy=0.5, L_char=3.5e-10, c_p=1.92,
            A=51.15e-10 * 51.15e-10, t_ox=52.6838e-10, delta_t=1e-13)
STEADY, TRANSIENT = 1e-6, 1e-13          # step_time > 1e3 delta_t: steady state; else one backward-Euler step
Q_SCALE = 1e-8                           # W per vacancy site: tens of K of heating at 5 nm


def _params(km, **kw):
    p = dict(PRM5, cg_tolerance=1e-13, cg_max_iterations=20000)
    p.update(kw)
    return km.solvers.heat_params(**p)


def _setup(km, d, comm):
    S = km.solvers
    NL = d["N_contact"]
    buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                        buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
    return buf


def _heat(km, buf, d, step_time, prm, T_old, Q):
    import torch
    NL = d["N_contact"]
    buf.site_power = torch.as_tensor(np.asarray(Q, np.float64), device=buf.device)
    buf.site_temperature = torch.as_tensor(np.asarray(T_old, np.float64).copy(), device=buf.device)
    res = km.solvers.update_temperature_local_gpu(buf, d["N"], NL, NL, step_time, prm)
    return buf.site_temperature.cpu().numpy().copy(), res


@pytest.fixture(scope="module")
def h5(km, oracle, dev5):
    import torch
    assert torch.cuda.is_available()
    S = km.solvers
    d = dev5
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], rank=0, size=1, device=0)
    comm.connect()
    buf = _setup(km, d, comm)
    charge = buf.site_charge.cpu().numpy()
    ks = oracle.KSystem(d["xyz"], d["lattice"], d["pbc"], d["nn_dist"], NL, NL)
    cls = H.site_classes(d["element"], charge, d["metals"])
    Q = H.synthetic_power(d["element"], charge, d["metals"], Q_SCALE)
    T_old = np.full(d["N"], PRM5["background_temp"])
    T_old[NL:-NL] += 5.0 * np.sin(0.013 * np.arange(d["N"] - 2 * NL)) ** 2        # a previous field that is not flat
    yield dict(comm=comm, buf=buf, d=d, ks=ks, cls=cls, Q=Q, T_old=T_old, charge=charge, refs={})
    buf.freeGPUmemory()
    comm.close()


def _ref(h, step_time):
    """spsolve of the restated system (cached per mode)."""
    if step_time not in h["refs"]:
        s = H.heat_system(h["ks"], h["cls"], PRM5, step_time, h["Q"], h["T_old"])
        h["refs"][step_time] = (s, H.solve(s, PRM5["background_temp"], h["d"]["N"], h["d"]["N_contact"]))
    return h["refs"][step_time]


@pytest.mark.parametrize("step_time", [STEADY, TRANSIENT])
def test_agrees_with_restatement(km, h5, step_time):
    d, NL, T0 = h5["d"], h5["d"]["N_contact"], PRM5["background_temp"]
    s, T_ref = _ref(h5, step_time)
    T, res = _heat(km, h5["buf"], d, step_time, _params(km), h5["T_old"], h5["Q"])
    st = res["stats"]
    print("5 nm %s: %d iterations, assembly %.3f ms, solve %.3f ms, relres %.2e, max dT %.2f K" % (
        "steady" if res["steady"] else "transient", st["iterations"], st["ms_assembly"], st["ms_solve"], st["relres"],
        np.abs(T_ref - T0).max()))
    assert res["steady"] == (step_time > 1e3 * PRM5["delta_t"]) == s["steady"]
    assert st["converged"] == 1 and st["iterations"] > 0
    assert np.all(T[:NL] == T0) and np.all(T[-NL:] == T0)
    assert np.abs(T - T_ref).max() <= 1e-8 * np.abs(T_ref - T0).max()
    assert res["Global temperature [K]"] == pytest.approx(T[NL:-NL].mean(), rel=1e-14)
    assert float(h5["buf"].T_bg.item()) == res["Global temperature [K]"]
    # the system as assembled: diag, contact sums (the K vectors of the state now hold the heat system's)
    kv = km.solvers.k_vectors(h5["buf"])
    np.testing.assert_allclose(kv["left"], s["gL"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(kv["right"], s["gR"], rtol=1e-13, atol=0)
    np.testing.assert_allclose(kv["diag"], s["diag"], rtol=1e-13, atol=0)


@pytest.mark.parametrize("step_time", [STEADY, TRANSIENT])
def test_physics(km, h5, step_time):
    d, NL, T0 = h5["d"], h5["d"]["N_contact"], PRM5["background_temp"]
    N = d["N"]
    # no power, T_old = T0 everywhere: T = T0 exactly
    T, res = _heat(km, h5["buf"], d, step_time, _params(km), np.full(N, T0), np.zeros(N))
    assert np.all(T == T0) and res["Global temperature [K]"] == T0
    # Q >= 0: T >= T0 (maximum principle), and energy conservation
    s, _ = _ref(h5, step_time)
    T_old = np.full(N, T0) if step_time == STEADY else h5["T_old"]
    T, res = _heat(km, h5["buf"], d, step_time, _params(km), T_old, h5["Q"])
    dT = T - T0
    assert dT.min() >= -1e-9 * dT.max()
    Qi = h5["Q"][NL:-NL].sum()
    out = ((s["gL"] + s["gR"]) * dT[NL:-NL]).sum()
    if res["steady"]:
        assert abs(out - Qi) <= 1e-9 * Qi, (out, Qi)
    else:
        stored = (s["C"] * (T - T_old)[NL:-NL] / step_time).sum()
        assert abs(stored + out - Qi) <= 1e-9 * Qi, (stored, out, Qi)


def test_warm_start(km, h5):
    d = h5["d"]
    T1, r1 = _heat(km, h5["buf"], d, STEADY, _params(km), h5["T_old"], h5["Q"])
    T2, r2 = _heat(km, h5["buf"], d, STEADY, _params(km), T1, h5["Q"])
    assert r1["stats"]["iterations"] > 10 and r2["stats"]["iterations"] <= 1, (r1["stats"], r2["stats"])
    assert r2["stats"]["converged"] == 1
    assert np.abs(T2 - T1).max() <= 1e-10 * np.abs(T1 - PRM5["background_temp"]).max()


def test_zero_step_keeps_the_field(km, h5):
    d, NL = h5["d"], h5["d"]["N_contact"]
    T, res = _heat(km, h5["buf"], d, 0.0, _params(km), h5["T_old"], h5["Q"])
    assert not res["steady"] and res["stats"]["iterations"] == 0
    assert np.array_equal(T, h5["T_old"])


def _k_solves(km, d, comm, with_heat):
    """K solve, (local heat solve,) K solve: the second K solve's statistics and potential."""
    S = km.solvers
    NL = d["N_contact"]
    buf = _setup(km, d, comm)
    S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                      len(d["metals"]))
    heat = None
    if with_heat:
        Q = H.synthetic_power(d["element"], buf.site_charge.cpu().numpy(), d["metals"], Q_SCALE)
        heat = _heat(km, buf, d, STEADY, _params(km), np.full(d["N"], PRM5["background_temp"]), Q)
    # a later KMC step: the potential of the first solve is the start guess, the system is K's again
    st = S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                           d["nn_dist"], len(d["metals"]))
    S.sum_and_gather_potential(buf, NL, comm)
    v = buf.site_potential_boundary.cpu().numpy().copy()
    buf.freeGPUmemory()
    return st, v, heat


def _same_solve(a, b):
    (sa, va, _), (sb, vb, _) = a, b
    assert sa["iterations"] == sb["iterations"] and sa["bb"] == sb["bb"] and sa["rz"] == sb["rz"], (sa, sb)
    assert np.array_equal(va, vb)


@pytest.mark.parametrize("resident", [1, 0])
def test_k_solve_unchanged_one_rank(km, dev5, resident):
    d = dev5
    NL = d["N_contact"]
    S = km.solvers
    out = []
    for with_heat in (False, True):
        comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], options={"KMCF_CG_RESIDENT": str(resident)})
        comm.connect()
        out.append(_k_solves(km, d, comm, with_heat))
        comm.close()
    assert out[1][2][1]["stats"]["iterations"] > 0
    _same_solve(out[0], out[1])


def _group(km, d, P, fn):
    import torch
    S = km.solvers
    NL = d["N_contact"]
    comms = S.KMC_comm.loopback_group(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], size=P, device=0)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comms[r].connect()
            out[r] = fn(comms[r])
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(180)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish (deadlock?)"
    for c in comms:
        c.close()
    return out


@pytest.mark.parametrize("P", [2, 4])
def test_rank_groups(km, h5, P):
    d, T0 = h5["d"], PRM5["background_temp"]
    res = {}
    for step_time in (STEADY, TRANSIENT):
        T1, r1 = _heat(km, h5["buf"], d, step_time, _params(km), h5["T_old"], h5["Q"])

        def fn(comm):
            buf = _setup(km, d, comm)
            T, r = _heat(km, buf, d, step_time, _params(km), h5["T_old"], h5["Q"])
            buf.freeGPUmemory()
            return T, r

        out = _group(km, d, P, fn)
        for T, r in out:
            assert np.array_equal(T, out[0][0])
            assert r["steady"] == r1["steady"] and r["stats"]["converged"] == 1
            assert r["Global temperature [K]"] == out[0][1]["Global temperature [K]"]
        bar = 1e-10 * np.abs(T1 - T0).max()
        assert np.abs(out[0][0] - T1).max() <= bar
        assert abs(out[0][1]["Global temperature [K]"] - r1["Global temperature [K]"]) <= bar
        res[step_time] = [o[1]["stats"]["iterations"] for o in out]
    print("P = %d: iterations per rank %s" % (P, res))


def test_k_solve_unchanged_two_ranks(km, dev5):
    runs = [_group(km, dev5, 2, lambda comm, wh=wh: _k_solves(km, dev5, comm, wh)) for wh in (False, True)]
    for a, b in zip(*runs):
        _same_solve(a, b)


def test_bad_arguments(km, h5):
    import torch
    lib = km.lib.load()
    d, buf, NL = h5["d"], h5["buf"], h5["d"]["N_contact"]
    S, P = km.solvers, km.solvers._ptr
    buf.site_power = torch.zeros(d["N"], dtype=torch.float64, device=buf.device)
    buf.site_temperature = torch.full((d["N"],), 300.0, dtype=torch.float64, device=buf.device)

    def call(prm, N=d["N"], nl=NL, nr=NL, step_time=STEADY, power=True):
        rc = lib.kmcf_update_temperature_local(buf.K_distributed, P(buf.site_element), P(buf.site_charge),
                                               P(buf.metal_types), buf.num_metal_types_,
                                               P(buf.site_power) if power else None, P(buf.site_temperature), N, nl, nr,
                                               step_time, C.byref(prm), None, None, None)
        return rc, lib.kmcf_last_error().decode()

    for name in ("k_th_metal", "k_th_vacancies", "k_th_non_vacancy", "L_char", "c_p", "A", "t_ox", "delta_t"):
        for bad in (0.0, -1.0):
            rc, msg = call(_params(km, **{name: bad}))
            assert rc == -1 and (name + " =") in msg, (name, msg)
    rc, msg = call(_params(km), step_time=-1e-12)
    assert rc == -1 and "step_time" in msg
    for kw in (dict(N=d["N"] + 1), dict(nl=NL - 1), dict(nr=NL + 1)):
        rc, msg = call(_params(km), **kw)
        assert rc == -1 and "N/N_left/N_right" in msg, kw
    rc, msg = call(_params(km), power=False)
    assert rc == -1 and "null" in msg
    assert torch.all(buf.site_temperature == 300.0)        # nothing was touched


def test_40nm_once(km):
    S = km.solvers
    d = km.structure.synth_crossbar_40nm()
    N, NL = d["N"], d["N_contact"]
    T0 = PRM5["background_temp"]
    comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
    comm.connect()
    buf = _setup(km, d, comm)
    charge = buf.site_charge.cpu().numpy()
    Q = H.synthetic_power(d["element"], charge, d["metals"], Q_SCALE)
    Qi = Q[NL:-NL].sum()
    # the 40 nm device's area and the model's other constants (structures/40nm_crossbar/parameters.txt)
    prm = _params(km, A=102.3e-10 * 102.3e-10, cg_max_iterations=50000)
    for step_time in (STEADY, TRANSIENT):
        T_old = np.full(N, T0)
        t = time.perf_counter()
        T, res = _heat(km, buf, d, step_time, prm, T_old, Q)
        wall = time.perf_counter() - t
        st = res["stats"]
        gL, gR = np.zeros(N - 2 * NL), np.zeros(N - 2 * NL)      # the heat system's contact sums, caller's order
        dp = C.POINTER(C.c_double)
        km.lib.check(km.lib.load().kmcf_k_get_vectors(buf.K_distributed, None, None, None, gL.ctypes.data_as(dp),
                                                      gR.ctypes.data_as(dp)), "kmcf_k_get_vectors")
        dT = T - T0
        out = ((gL + gR) * dT[NL:-NL]).sum()
        stored = 0.0
        if not res["steady"]:
            C_site = prm.c_p * 1e6 * prm.A * prm.t_ox / (N - 2 * NL)
            stored = (C_site * (T - T_old)[NL:-NL] / step_time).sum()
        print("40 nm %s: %d iterations, assembly %.3f ms, solve %.3f ms, call %.1f ms, max dT %.3g K" % (
            "steady" if res["steady"] else "transient", st["iterations"], st["ms_assembly"], st["ms_solve"], wall * 1e3,
            dT.max()))
        assert st["converged"] == 1
        assert dT.min() >= -1e-9 * dT.max() and dT.max() > 0
        assert abs(stored + out - Qi) <= 1e-9 * Qi, (stored, out, Qi)
    buf.freeGPUmemory()
    comm.close()
