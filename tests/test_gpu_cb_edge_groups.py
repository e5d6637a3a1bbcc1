"""GPU: the conduction-band-edge solve (update_CB_edge_gpu_sparse) and the literal scaled CG (solve_sparse_CG_Jacobi)
on rank groups: in-process groups of 2 and 4 ranks on one GPU (one host thread per rank), host-loopback and peer-to-peer
transport, the Jacobi-PCG form and the scaled form (KMCF_CB_SCALED, a group knob), the single-reduction recurrence (a
group's default) and the reference's.

The oracle has no P-rank emulation of the absolute stopping rule, so a group is held to the oracle's one-rank
restatement by the tolerances of the one-rank tests (tests/test_gpu_cb_edge.py), not bit for bit.  What IS held bit for
bit: the ranks of a group among each other, the two transports against each other, and K's next solve with and without a
band-edge call in between."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EV = 1.60217663e-19
KMCF_ERR_STATE = -4
FORMS = {"pcg": {}, "scaled": {"KMCF_CB_SCALED": "1"}}
VARIANTS = {"cg1r": {}, "classic": {"KMCF_CG_VARIANT": "classic"}}        # cg1r: a group's default


def _transport(monkeypatch, name):
    """Connect-scope knobs of an in-process group come from the environment (it is connected at creation)."""
    if name == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")               # bound of every device-side wait
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)


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


def _cb(km, buf, d):
    NL = d["N_contact"]
    return km.solvers.update_CB_edge_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                                d["nn_dist"], len(d["metals"]))


def _run_threads(P, work, seconds):
    out, errs = [None] * P, []

    def guarded(r):
        try:
            out[r] = work(r)
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=guarded, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(seconds)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish (deadlock?)"
    return out


def _group(km, d, P, fn, options=None, seconds=240):
    """fn(comm) on every rank of an in-process group of P, each on its own host thread; options: one dict for all ranks
    or a function of the rank."""
    import torch
    S = km.solvers
    NL = d["N_contact"]
    comms = S.KMC_comm.loopback_group(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], size=P, device=0)

    def work(r):
        torch.cuda.set_device(0)
        for k, v in (options(r) if callable(options) else (options or {})).items():
            comms[r].set_option(k, v)
        comms[r].connect()
        return fn(comms[r])

    try:
        return _run_threads(P, work, seconds)
    finally:
        for c in comms:
            c.close()


def _two_calls(km, d, comm):
    """Cold band-edge call, the system it assembled, then a second call that starts from the first one's result."""
    buf = _setup(km, d, comm)
    try:
        st1 = _cb(km, buf, d)
        got = buf.site_CB_edge.cpu().numpy().copy()
        kv = km.solvers.k_vectors(buf)
        st2 = _cb(km, buf, d)
        got2 = buf.site_CB_edge.cpu().numpy().copy()
    finally:
        buf.freeGPUmemory()
    return dict(st1=st1, st2=st2, got=got, got2=got2, rhs=kv["rhs"], val=kv["val"])


def _one_rank_two_calls(km, d, form):
    S = km.solvers
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], options=FORMS[form])
    comm.connect()
    try:
        return _two_calls(km, d, comm)
    finally:
        comm.close()


@pytest.mark.parametrize("variant", ["cg1r", "classic"])
@pytest.mark.parametrize("form", ["pcg", "scaled"])
@pytest.mark.parametrize("P", [2, 4])
def test_group_band_edge(km, oracle, dev5, ref5, monkeypatch, P, form, variant):
    """Items 1-6 of the issue.  On the parent commit the group call raises KMCF_ERR_ARG ("single-rank solve").

    Warm start (the project has no bar): the second call starts from the first call's array, which is in J -- a
    start guess 1.6e-19 times the solution, as in the reference -- so it takes about as long as the cold one; the
    group may take no more iterations than one rank's second call plus max(3, 5 %) of the cold count."""
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    monkeypatch.delenv("KMCF_CG_VARIANT", raising=False)
    d = dev5
    NL, Vd = d["N_contact"], d["Vd"]
    ks = ref5["ks"]
    want, it_o, A = oracle.update_CB_edge(ks, d["element"], d["metals"], d["high_G"], d["low_G"], Vd)
    counts, displs = oracle.partition(ks.n, P)
    opts = dict(FORMS[form], **VARIANTS[variant])
    one = _one_rank_two_calls(km, d, form)
    slack = max(3, 0.05 * it_o)
    runs = {}
    for transport in ("loopback", "p2p"):
        _transport(monkeypatch, transport)
        out = _group(km, d, P, lambda comm: _two_calls(km, d, comm), options=opts)
        runs[transport] = out
        o0 = out[0]
        print("P = %d, %s, %s, %s: cold %d iterations (oracle %d, one rank %d), %.2f ms; second call %d (one rank %d), "
              "%.2f ms; max|got - want| / eV = %.2e" % (P, transport, form, variant, o0["st1"]["iterations"], it_o,
                                                        one["st1"]["iterations"], o0["st1"]["ms_solve"],
                                                        o0["st2"]["iterations"], one["st2"]["iterations"],
                                                        o0["st2"]["ms_solve"], np.abs(o0["got"] - want).max() / EV))
        for r, o in enumerate(out):
            # 1. returns, converged on every rank
            assert o["st1"]["converged"] == 1 and o["st2"]["converged"] == 1, (r, o["st1"], o["st2"])
            # 2. every site against the oracle's restatement
            got = o["got"]
            assert got.shape == (d["N"],)
            assert np.all(got[:NL] == Vd / 2 * EV) and np.all(got[-NL:] == -Vd / 2 * EV)
            assert np.abs(got - want).max() / EV <= 1e-9
            assert abs(o["st1"]["iterations"] - it_o) <= slack, (o["st1"]["iterations"], it_o)
            assert np.abs(got).max() <= Vd / 2 * EV * (1 + 1e-9)
            # 3. identical on all ranks
            assert np.array_equal(got, o0["got"]) and np.array_equal(o["got2"], o0["got2"])
            for st in ("st1", "st2"):
                assert o[st]["iterations"] == o0[st]["iterations"] and o[st]["rz"] == o0[st]["rz"], (r, st, o[st], o0[st])
            # 5. the assembled system of this rank's rows
            r0, nr = int(displs[r]), int(counts[r])
            e0, e1 = ks.row_ptr[r0], ks.row_ptr[r0 + nr]
            np.testing.assert_allclose(o["rhs"], A["rhs"][r0:r0 + nr], rtol=1e-14)
            if form == "scaled":
                np.testing.assert_allclose(o["val"], A["val_scaled"][e0:e1], rtol=1e-12, atol=1e-300)
            else:
                np.testing.assert_allclose(o["val"], A["val"][e0:e1], rtol=1e-14, atol=1e-300)
            # 6. warm start
            assert o["st2"]["iterations"] <= one["st2"]["iterations"] + max(3, 0.05 * one["st1"]["iterations"]), \
                (o["st2"]["iterations"], one["st2"]["iterations"], one["st1"]["iterations"])
            assert np.abs(o["got2"] - want).max() / EV <= 1e-9
    # 4. a group's iterates do not depend on its transport
    for a, b in zip(runs["loopback"], runs["p2p"]):
        assert np.array_equal(a["got"], b["got"]) and np.array_equal(a["got2"], b["got2"])
        for st in ("st1", "st2"):
            assert a[st]["iterations"] == b[st]["iterations"] and a[st]["rz"] == b[st]["rz"], (st, a[st], b[st])


def _k_solves(km, d, comm, with_cb):
    """K solve, (band-edge solve,) K assembly and solve: the second K solve's statistics and potential."""
    S = km.solvers
    NL = d["N_contact"]
    buf = _setup(km, d, comm)
    try:
        S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                          len(d["metals"]))
        cb = _cb(km, buf, d) if with_cb else None
        # a later KMC step: the potential of the first solve is the start guess, the system is K's again
        st = S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                               d["nn_dist"], len(d["metals"]))
        mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))
        tpb = mat.sum_plan(with_csr=False)["resident_tpb"]
        S.sum_and_gather_potential(buf, NL, comm)
        v = buf.site_potential_boundary.cpu().numpy().copy()
    finally:
        buf.freeGPUmemory()
    return dict(st=st, v=v, cb=cb, tpb=tpb)


@pytest.mark.parametrize("resident", [1, 0])
def test_k_solve_unchanged_two_ranks(km, dev5, monkeypatch, resident):
    """Item 7.  The scaled form leaves the matrix with many distinct values and no value codes; K's next assembly
    re-codes it before the group's cached resident plan is launched again (kmcf_cgr_solve re-validates and would fail
    with KMCF_ERR_STATE otherwise)."""
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    _transport(monkeypatch, "p2p")                        # (a group's resident launch needs the peer-to-peer transport)
    base = {"KMCF_CG_RESIDENT": str(resident), "KMCF_CGR_TIMEOUT_MS": "20000"}
    runs = {}
    for name, with_cb, extra in (("none", False, {}), ("pcg", True, FORMS["pcg"]), ("scaled", True, FORMS["scaled"])):
        runs[name] = _group(km, dev5, 2, lambda comm, w=with_cb: _k_solves(km, dev5, comm, w), options=dict(base, **extra))
    for o in runs["none"]:
        assert (o["tpb"] > 0) == bool(resident), o["tpb"]
    for name in ("pcg", "scaled"):
        for a, b in zip(runs["none"], runs[name]):
            assert b["cb"]["converged"] == 1 and b["cb"]["iterations"] > 0
            assert b["tpb"] == a["tpb"]
            sa, sb = a["st"], b["st"]
            assert sa["iterations"] == sb["iterations"] and sa["bb"] == sb["bb"] and sa["rz"] == sb["rz"], (name, sa, sb)
            assert sa["converged"] == sb["converged"] == 1
            assert np.array_equal(a["v"], b["v"]), name


def test_stale_resident_plan_is_refused_not_launched(km, dev5, ref5, monkeypatch):
    """Item 7, the path that IS reachable: a P = 2 group whose K solve ran resident, then the scaled band edge (the
    matrix now holds many distinct values and no codes), then a solve on the K matrix WITHOUT a new assembly.  The group's
    cached plan would launch on the codes of the system before; every rank gets KMCF_ERR_STATE instead, on the host,
    and after a K assembly the same state solves resident again."""
    import torch
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    _transport(monkeypatch, "p2p")
    S = km.solvers
    d = dev5
    NL = d["N_contact"]

    def fn(comm):
        buf = _setup(km, d, comm)
        try:
            args = (buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"], len(d["metals"]))
            st0 = S.background_potential_gpu_sparse(*args)
            mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))
            tpb = mat.sum_plan(with_csr=False)["resident_tpb"]
            cb = _cb(km, buf, d)
            n = mat.info()["rows_this_rank"]
            r = torch.ones(n, dtype=torch.float64, device="cuda")
            x = torch.zeros(n, dtype=torch.float64, device="cuda")
            dinv = torch.ones(n, dtype=torch.float64, device="cuda")
            err = None
            try:
                S.conjugate_gradient_jacobi(mat, r, x, dinv, 1e-10, 100)
            except km.lib.KmcfError as e:
                err = str(e)
            st1 = S.background_potential_gpu_sparse(*args)
            return dict(tpb=tpb, cb=cb, err=err, st0=st0, st1=st1, x=x.cpu().numpy())
        finally:
            buf.freeGPUmemory()

    out = _group(km, d, 2, fn, options={"KMCF_CB_SCALED": "1", "KMCF_CG_RESIDENT": "1", "KMCF_CGR_TIMEOUT_MS": "20000"})
    for o in out:
        assert o["tpb"] > 0 and o["cb"]["converged"] == 1
        assert o["err"] is not None and "(%d)" % KMCF_ERR_STATE in o["err"] and "resident plan" in o["err"], o["err"]
        assert np.all(o["x"] == 0.0)                                     # nothing was solved on stale codes
        assert o["st0"]["converged"] == 1 and o["st1"]["converged"] == 1 and o["st1"]["iterations"] <= o["st0"]["iterations"]


def test_ranks_that_disagree_on_the_form_are_refused_at_the_build(km, dev5, monkeypatch):
    """Item 8: KMCF_CB_SCALED chooses which collectives a rank enters, so it is a group knob.  (Peer-to-peer transport,
    like the disagreement case of tests/test_gpu_options.py: the build's table exchange carries the knob hashes.)"""
    import time
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    _transport(monkeypatch, "p2p")
    S = km.solvers
    d = dev5
    NL = d["N_contact"]

    def fn(comm):
        buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                           d["lattice"], d["metals"])
        t0 = time.time()
        try:
            S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
        except km.lib.KmcfError as e:
            return dict(error=str(e), seconds=time.time() - t0)
        buf.freeGPUmemory()
        return dict(error=None)

    out = _group(km, d, 2, fn, options=lambda r: {"KMCF_CB_SCALED": "1"} if r == 1 else {})
    for o in out:
        assert o["error"] is not None, "the build accepted ranks that disagree"
        assert "(%d)" % KMCF_ERR_STATE in o["error"] and "KMCF_CB_SCALED" in o["error"], o["error"]
        assert o["seconds"] < 30, o["seconds"]


@pytest.mark.parametrize("variant", ["cg1r", "classic"])
@pytest.mark.parametrize("transport", ["loopback", "p2p"])
@pytest.mark.parametrize("P", [2, 3])
def test_solve_sparse_CG_Jacobi_generic_csr_groups(km, oracle, monkeypatch, P, transport, variant):
    """Item 9: the library-level entry on a caller-supplied CSR matrix split over P ranks by kmcf_partition (the
    60 x 60 shifted Laplacian of tests/test_gpu_cb_edge.py): every rank leaves with its rows of the scaled matrix and of
    the scaled right-hand side, like one rank does."""
    import ctypes as C
    import scipy.sparse as sp
    import torch
    monkeypatch.delenv("KMCF_CG_VARIANT", raising=False)
    _transport(monkeypatch, transport)
    S = km.solvers
    nx = 60
    n = nx * nx
    T = sp.diags([-1, 2.3, -1], [-1, 0, 1], shape=(nx, nx))
    M = (sp.kron(sp.eye(nx), T) + sp.kron(T, sp.eye(nx))).tocsr()
    M.sort_indices()
    b = np.random.default_rng(11).standard_normal(n)
    val, bb, y = M.data.copy(), b.copy(), np.zeros(n)
    L = oracle.lib()
    L.orc_solve_sparse_CG_Jacobi.restype = C.c_int
    L.orc_solve_sparse_CG_Jacobi.argtypes = [C.c_int, oracle._ip, oracle._ip, oracle._dp, oracle._dp, oracle._dp, C.c_double, C.c_int]
    it_o = L.orc_solve_sparse_CG_Jacobi(n, M.indptr.astype(np.int32), M.indices.astype(np.int32), val, bb, y, 1e-14, 5000)
    counts, displs = S.KMC_comm.partition(n, P)
    comms = S.KMC_comm.loopback_group(n, n, n, n, size=P, device=0, options=VARIANTS[variant])

    def work(r):
        torch.cuda.set_device(0)
        comm = comms[r]
        comm.connect()
        r0, nr = int(displs[r]), int(counts[r])
        e0, e1 = M.indptr[r0], M.indptr[r0 + nr]
        mat = S.Distributed_matrix(comm, n, counts, displs, M.indices[e0:e1], M.indptr[r0:r0 + nr + 1] - e0, M.data[e0:e1])
        try:
            rhs = torch.as_tensor(b[r0:r0 + nr].copy(), device="cuda")
            x = torch.zeros(nr, dtype=torch.float64, device="cuda")
            st = S.solve_sparse_CG_Jacobi(mat, rhs, x, 1e-14, 5000)
            return dict(st=st, x=x.cpu().numpy(), rhs=rhs.cpu().numpy(), val=mat.get_values().copy())
        finally:
            mat.close()

    try:
        out = _run_threads(P, work, 120)
    finally:
        for c in comms:
            c.close()
    xs = np.concatenate([o["x"] for o in out])
    print("P = %d, %s, %s: %d iterations (oracle %d), %.2f ms, max|x - y| = %.2e" % (
        P, transport, variant, out[0]["st"]["iterations"], it_o, out[0]["st"]["ms_solve"], np.abs(xs - y).max()))
    for r, o in enumerate(out):
        r0, nr = int(displs[r]), int(counts[r])
        e0, e1 = M.indptr[r0], M.indptr[r0 + nr]
        assert o["st"]["converged"] == 1
        assert o["st"]["iterations"] == out[0]["st"]["iterations"] and o["st"]["rz"] == out[0]["st"]["rz"]
        assert abs(o["st"]["iterations"] - it_o) <= 2, (o["st"]["iterations"], it_o)
        np.testing.assert_allclose(o["rhs"], bb[r0:r0 + nr], rtol=1e-14)         # rhs scaled in place (:740)
        np.testing.assert_allclose(o["val"], val[e0:e1], rtol=1e-14)             # A scaled in place (:745)
    assert np.abs(xs - y).max() <= 1e-12
    assert np.abs(M @ xs - b).max() <= 1e-10
