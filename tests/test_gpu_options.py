"""GPU: options per communicator (kmcf_set_option).  Communicators of one process that are configured differently
without touching the process's environment, connect-scope knobs refused after the connect, an in-process group whose
ranks set their options from their own threads, a group whose ranks disagree on a group knob (refused at the matrix
build, on the host, before any solve), and the T path's tunnel-block storage chosen per communicator."""
import os
import threading
import time

import numpy as np
import pytest
from conftest import assert_solve_bit_identical

pytestmark = pytest.mark.gpu

KMCF_ERR_STATE = -4


def _k_system(km, d, comm):
    S = km.solvers
    NL = d["N_contact"]
    buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    return buf


def _one_rank(km, d, options=None):
    S = km.solvers
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], rank=0, size=1, device=0, options=options)
    comm.connect()
    return comm, _k_system(km, d, comm)


def test_two_communicators_differ_without_the_environment(km, dev5, ref5, oracle, monkeypatch):
    """One communicator with KMCF_CG_RESIDENT=0 and KMCF_CG_VARIANT=cg1r, one with the defaults (the reference's
    recurrence as one resident launch), a third with KMCF_SPMV_KIND=1 (the CSR stream kernel): three plans in one
    process, each solve bit-identical to the oracle adding in its order, and os.environ never touched."""
    import torch
    S = km.solvers
    d = dev5
    for k in ("KMCF_CG_RESIDENT", "KMCF_CG_VARIANT", "KMCF_SPMV_KIND"):
        monkeypatch.delenv(k, raising=False)
    env0 = dict(os.environ)
    A, ks = ref5["A"], ref5["ks"]
    lib = km.lib.load()
    made = []
    try:
        ca, ba = _one_rank(km, d, {"KMCF_CG_RESIDENT": "0", "KMCF_CG_VARIANT": "cg1r"})
        made.append((ca, ba))
        cb, bb = _one_rank(km, d)
        made.append((cb, bb))
        cc, bc = _one_rank(km, d, {"KMCF_SPMV_KIND": 1})
        made.append((cc, bc))
        assert ca.get_option("KMCF_CG_VARIANT") == ("cg1r", 2) and cb.get_option("KMCF_CG_VARIANT") == (None, 0)
        out = []
        for comm, buf in made:
            buf.site_charge.copy_(buf.site_charge.new_tensor(ref5["charge"]))
            S.k_assemble(buf, d["Vd"], d["high_G"], d["low_G"])
            mat = S.Distributed_matrix.from_handle(lib.kmcf_kstate_matrix(buf.K_distributed))
            r = torch.as_tensor(A["rhs"], device="cuda").clone()
            x = torch.zeros_like(r)
            dinv = torch.as_tensor(A["dinv"], device="cuda")
            st = S.conjugate_gradient_jacobi(mat, r, x, dinv, ref5["tol"], 10000)
            out.append(dict(mat=mat, st=st, x=x.cpu().numpy(), r=r.cpu().numpy(), plan=mat.sum_plan(), info=mat.info()))
        a, b, c = out
        assert a["plan"]["cg_variant"] == 1 and a["plan"]["resident_tpb"] == 0
        assert b["plan"]["cg_variant"] == 0 and b["plan"]["resident_tpb"] > 0
        assert a["info"]["spmv_kind"] == b["info"]["spmv_kind"] == 2 and c["info"]["spmv_kind"] == 1
        assert c["st"]["converged"] == 1 and c["st"]["relres"] <= ref5["tol"]     # (the device-order oracle: row-per-lane plans)
        for o, variant in ((a, "cg1r"), (b, "classic")):
            assert o["st"]["converged"] == 1 and o["st"]["relres"] <= ref5["tol"]
            orc = oracle.pcg_device_order(o["plan"], A["rhs"], np.zeros(ks.n), A["dinv"], ref5["tol"], 10000, variant=variant)
            assert_solve_bit_identical(o["st"], o["x"], o["r"] if variant == "cg1r" else None, orc)
        # the stream plan's SpMV under test_gpu_parity.py::test_spmv_matches_oracle's bars
        rng = np.random.default_rng(3)
        for xv in (np.ones(ks.n), rng.standard_normal(ks.n)):
            p = torch.as_tensor(xv, device="cuda")
            Ap = torch.empty_like(p)
            c["mat"].spmv(p, Ap)
            y = oracle.spmv(ks.row_ptr, ks.col, A["val"], xv)
            bound = oracle.spmv(ks.row_ptr, ks.col, np.abs(A["val"]), np.abs(xv))
            assert np.all(np.abs(Ap.cpu().numpy() - y) <= 1e-13 * bound + 1e-300)
    finally:
        for comm, buf in made:
            buf.freeGPUmemory()
            comm.close()
    assert dict(os.environ) == env0


def test_connect_scope_knob_is_refused_after_the_connect(km):
    S = km.solvers
    lib = km.lib.load()
    c = S.KMC_comm(100, 101, 100, 100, device=0, options={"KMCF_P2P_TIMEOUT_MS": "15000"})
    try:
        assert c.get_option("KMCF_P2P_TIMEOUT_MS") == ("15000", 2)
        c.connect()
        assert lib.kmcf_set_option(c.handle, b"KMCF_P2P_TIMEOUT_MS", b"2000") == KMCF_ERR_STATE
        assert "KMCF_P2P_TIMEOUT_MS" in lib.kmcf_last_error().decode()
        assert c.get_option("KMCF_P2P_TIMEOUT_MS") == ("15000", 2)
        c.set_option("KMCF_CG_VARIANT", "cg1r")           # comm scope: still settable
    finally:
        c.close()


def _group(km, d, P, options_of, stop_after_build=False):
    """P ranks of an in-process group, one thread each; rank r sets options_of(r) from its own thread."""
    import torch
    S = km.solvers
    NL = d["N_contact"]
    comms = S.KMC_comm.loopback_group(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], size=P, device=0)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            for k, v in options_of(r).items():
                comm.set_option(k, v)
            comm.connect()
            t0 = time.time()
            try:
                buf = _k_system(km, d, comm)
            except km.lib.KmcfError as e:
                out[r] = dict(error=str(e), seconds=time.time() - t0)
                return
            if stop_after_build:
                out[r] = dict(error=None)
                buf.freeGPUmemory()
                return
            S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                                buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
            st = S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                                   d["nn_dist"], len(d["metals"]), 0)
            mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))
            plan, kv = mat.sum_plan(), S.k_vectors(buf)
            S.sum_and_gather_potential(buf, NL, comm)             # every rank: the whole interface solution
            out[r] = dict(error=None, st=st, plan=plan, kv=kv,
                          charge=buf.site_charge.cpu().numpy().copy(), v=buf.site_potential_boundary.cpu().numpy().copy())
            buf.freeGPUmemory()
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(240)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish"
    for c in comms:
        c.close()
    return out


def test_group_options_set_per_rank_thread(km, dev5, ref5, oracle, monkeypatch):
    """A loopback group of two whose ranks set their options from their own threads, the same value on both: the
    reference's recurrence on the host loopback transport, then the single-reduction recurrence as one resident launch
    per rank on the peer-to-peer transport -- each bit-identical to the oracle's P = 2 emulation of that order.  Then
    rank 1 sets another KMCF_CG_VARIANT: the next matrix build refuses on BOTH ranks, on the host, in seconds."""
    d = dev5
    NL = d["N_contact"]
    ks = ref5["ks"]
    P = 2
    counts, displs = oracle.partition(ks.n, P)
    for k in ("KMCF_CG_VARIANT", "KMCF_CG_RESIDENT", "KMCF_EVENTS_PARTITIONED", "KMCF_P2P_DIRECT", "KMCF_CGR_TPB",
              "KMCF_CGR_G1", "KMCF_TRANSPORT"):
        monkeypatch.delenv(k, raising=False)
    # the reference's recurrence, host loopback transport
    out = _group(km, d, P, lambda r: {"KMCF_CG_VARIANT": "classic"})
    ranks = [oracle.DeviceRank(o["plan"]) for o in out]
    assert all(o["plan"]["cg_variant"] == 0 for o in out)
    rhs = np.concatenate([o["kv"]["rhs"] for o in out])
    dinv = np.concatenate([o["kv"]["dinv"] for o in out])
    orc = oracle.pcg_device_order_ranks(ranks, counts, displs, rhs, np.zeros(ks.n), dinv, ref5["tol"], 10000, variant="classic")
    for o in out:
        assert np.array_equal(o["charge"], ref5["charge"])
        assert o["st"]["converged"] == 1 and o["st"]["iterations"] == orc["iterations"]
        assert o["st"]["rz"] == orc["rz"] and o["st"]["bb"] == orc["bb"]
        assert np.array_equal(o["v"][NL:-NL], orc["x"])
    # single reduction, resident, peer-to-peer transport (a connect-scope knob: an in-process group is connected at
    # creation, so it comes from the environment)
    monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
    monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    opts = {"KMCF_CG_VARIANT": "cg1r", "KMCF_CG_RESIDENT": "1", "KMCF_CGR_TIMEOUT_MS": "20000"}
    out = _group(km, d, P, lambda r: opts)
    assert all(o["plan"]["cg_variant"] == 1 and o["plan"]["resident_tpb"] > 0 for o in out)
    ranks = [oracle.DeviceRank(o["plan"]) for o in out]
    rhs = np.concatenate([o["kv"]["rhs"] for o in out])
    dinv = np.concatenate([o["kv"]["dinv"] for o in out])
    orc = oracle.pcg_resident_ranks(ranks, counts, displs, rhs, np.zeros(ks.n), dinv, ref5["tol"], 10000)
    for o in out:
        assert o["st"]["converged"] == 1 and o["st"]["iterations"] == orc["iterations"]
        assert o["st"]["rz"] == orc["rz"] and o["st"]["bb"] == orc["bb"]
        np.testing.assert_array_equal(o["v"][NL:NL + ks.n], orc["x"])
    # disagreement: refused by the build's own exchange, before any solve
    out = _group(km, d, P, lambda r: dict(opts, KMCF_CG_VARIANT="classic" if r == 1 else "cg1r"), stop_after_build=True)
    for o in out:
        assert o["error"] is not None, "the build accepted ranks that disagree"
        assert "(%d)" % KMCF_ERR_STATE in o["error"] and "KMCF_CG_VARIANT" in o["error"], o["error"]
        assert o["seconds"] < 30, o["seconds"]


def test_tunnel_storage_per_communicator(km, monkeypatch):
    """The conducting 4 x 4 crossbar of test_gpu_conducting.py on two communicators of one process, KMCF_SUB_DENSE
    1 (dense symmetric tiles) and 2 (jagged tiles) as options: the storage t_info reports, and the current that
    test's environment-driven runs get (jagged and dense add the same sums: identical)."""
    from test_gpu_conducting import _current, _device
    S = km.solvers
    monkeypatch.delenv("KMCF_SUB_DENSE", raising=False)
    env0 = dict(os.environ)
    d = km.structure.synth_crossbar_40nm(tiles=4, filament=4.0)
    N, NL = d["N"], d["N_contact"]
    res = {}
    for dense in ("1", "2"):
        comm = S.KMC_comm(N - 2 * NL, N + 1, N, N, options={"KMCF_SUB_DENSE": dense})
        comm.connect()
        dev = _device(km, 4.0, comm=comm, d=d)
        try:
            im, il, st, info, bound = _current(dev, 1e-18, first=True, touch_env=False)
        finally:
            dev["buf"].freeGPUmemory()
            comm.close()
        assert st["converged"] == 1 and info["tunnel_points"] == 17722
        assert int(info["tunnel_dense"]) == int(dense)
        assert abs(im - il) <= max(bound * 1.01, 1e-25) and abs(im - il) <= 1e-8 * im, (im, il, bound)
        res[dense] = im
    assert res["1"] == res["2"]
    assert 3e-3 < res["1"] < 5e-3                     # (the environment-driven test: 3.8614e-3)
    assert dict(os.environ) == env0
