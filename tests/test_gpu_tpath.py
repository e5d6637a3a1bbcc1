"""GPU: the T path (current solve: Kirchhoff neighbour matrix with two virtual nodes + WKB tunnel sub-block,
split-operator Jacobi-PCG, I_macro, dissipated power) through the C ABI against oracle/kmcf_oracle_T.c.

PARITY UNPINNED: no reference fixture covers this path (tests/test_oracle_T.py says what pins the oracle).
Bars: integer work (atom list, both patterns, tunnel points) bit-exact; neighbour off-diagonals bit-exact,
diagonals / preconditioner rtol 1e-13; WKB values rtol 1e-10 (device exp/pow against glibc's through an exponent
of magnitude ~30); SpMV |dy| <= 1e-12 sum|a||x|; I_macro 1e-9 relative; power 1e-8 of its maximum.
Split PCG: against the oracle adding in the DEVICE's order on the system as assembled on the device
(oracle/kmcf_oracle_order.c: row-per-lane, boundary-row, long-row and tunnel-block kernels, rank-ordered sums):
iteration count and potentials IDENTICAL; against the oracle's natural order: iterates at 5 iterations 1e-10, the
converged solution's TRUE residual <= 3 x the oracle's own true residual.

small_device(seed=7) has 208 atoms and 62 tunnel points: one 64-bit mask word, one tile, one strip.  The block sizes
around the mask word and the tile, reverse bias and inputs ON the strict comparisons are in
tests/test_gpu_tpath_synthetic.py, against the dense reference of tests/tpath_ref.py."""
import threading

import os

import numpy as np
import pytest

from test_oracle_T import PAR, Q, TI, N_EL, small_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


G0 = 2 * 3.8612e-5 * 1e-5


def _make(km, torch, xyz, element, charge, cb, metals, n1, layers, comm, nn_dist=3.5):
    S = km.solvers
    N = len(element)
    buf = S.GPUBuffers(N, element, xyz[:, 0], xyz[:, 1], xyz[:, 2], 52, 3.5e-10, 1.0, [1, 1, 1], metals)
    buf.site_charge.copy_(torch.as_tensor(np.asarray(charge, np.int32)))
    buf.site_CB_edge = torch.as_tensor(np.asarray(cb, np.float64), device="cuda")
    S.initialize_sparsity_T(buf, 0, nn_dist, n1, n1, layers, comm)
    return buf


def _device_rank(km, oracle, buf, row0, dense=False, spread=False, strip=16):
    """What fixes one rank's summation order + the system as assembled on the device (for oracle.pcg_device_order_ranks).
    spread: the tunnel block's tiles are dealt to the ranks of the group (strip: tiles per strip, KMCF_SUB_STRIP)."""
    S = km.solvers
    mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
    plan, v, tn = mat.sum_plan(), S.t_vectors(buf), S.t_tunnel(buf)
    ns = len(tn["row_ptr"]) - 1
    sub = dict(grid=plan["sub_grid"], rows=tn["tunnel_idx"][tn["first"]:tn["first"] + ns] + 2 - row0, row_ptr=tn["row_ptr"],
               col=tn["col"], val=tn["val"], dense=dense or spread, spread=spread, strip=strip)
    return dict(rank=oracle.DeviceRank(plan, sub), rhs=v["rhs"], dinv=v["dinv"], ns=ns, variant="cg1r" if plan["cg_variant"] else "classic")


def _device_order_solve(oracle, parts, counts, displs, tol, max_it):
    ns = np.array([p["ns"] for p in parts], np.int64)
    return oracle.pcg_device_order_ranks([p["rank"] for p in parts], counts, displs, np.concatenate([p["rhs"] for p in parts]),
                                         np.zeros(int(displs[-1] + counts[-1])), np.concatenate([p["dinv"] for p in parts]), tol,
                                         max_it, variant=parts[0]["variant"], sub_counts=ns, sub_displs=np.cumsum(ns) - ns)


def _compare_assembly(S, buf, T, r0=0, nr=None, s_first=None):
    nr = T.Nsub if nr is None else nr
    rp, col = S.t_pattern(buf)
    want_rp = T.row_ptr[r0:r0 + nr + 1] - T.row_ptr[r0]
    np.testing.assert_array_equal(rp, want_rp)
    sl = slice(T.row_ptr[r0], T.row_ptr[r0 + nr])
    np.testing.assert_array_equal(col, T.col[sl])
    v = S.t_vectors(buf)
    rows = np.repeat(np.arange(r0, r0 + nr), np.diff(want_rp))
    offd = T.col[sl] != rows
    np.testing.assert_array_equal(v["val"][offd], T.val[sl][offd])                  # -high_G / -low_G / -loop_G
    np.testing.assert_allclose(v["val"][~offd], T.val[sl][~offd], rtol=1e-13)
    np.testing.assert_allclose(v["diag_neighbour"], T.diag_neigh[r0:r0 + nr], rtol=1e-13)
    np.testing.assert_array_equal(v["rhs"], T.rhs[r0:r0 + nr])
    tn = S.t_tunnel(buf)
    np.testing.assert_array_equal(tn["tunnel_idx"], T.tunnel_idx)
    s0 = tn["first"]
    ns = len(tn["row_ptr"]) - 1
    np.testing.assert_array_equal(tn["row_ptr"], T.sub_row_ptr[s0:s0 + ns + 1] - T.sub_row_ptr[s0])
    ssl = slice(T.sub_row_ptr[s0], T.sub_row_ptr[s0 + ns])
    np.testing.assert_array_equal(tn["col"], T.sub_col[ssl])
    np.testing.assert_allclose(tn["val"], T.sub_val[ssl], rtol=1e-10, atol=0)
    np.testing.assert_allclose(tn["diag"], T.diag_tunnel[s0:s0 + ns], rtol=1e-10)
    # preconditioner of the whole operator: rtol follows the tunnel diagonal where it contributes
    np.testing.assert_allclose(v["dinv"], T.dinv[r0:r0 + nr], rtol=1e-10)
    plain = np.ones(nr, bool)
    own = T.sub_rows[(T.sub_rows >= r0) & (T.sub_rows < r0 + nr)] - r0
    plain[own] = False
    np.testing.assert_allclose(v["dinv"][plain], T.dinv[r0:r0 + nr][plain], rtol=1e-13)
    return tn


def test_small_device_single_rank(km, oracle, torch):
    S = km.solvers
    d = small_device(seed=7)
    a = 2.5
    x_lo, x_hi = (d["layers"] - 1) * a - 0.1, (d["layers"] + 7) * a + 0.1
    metals = np.array([TI, N_EL], np.int32)
    T = oracle.TSystem(d["xyz"], d["element"], d["charge"], d["cb"], metals, PAR["nn_dist"], d["n1"], d["n1"], d["layers"],
                       PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], PAR["tol"], PAR["m_e"], PAR["V0"], x_lo, x_hi)
    comm = S.KMC_comm(T.Nsub, T.Nsub, len(d["element"]), len(d["element"]))
    comm.connect()
    buf = _make(km, torch, d["xyz"], d["element"], d["charge"], d["cb"], metals, d["n1"], d["layers"], comm)
    assert buf.N_atom_ == T.N_atom
    np.testing.assert_array_equal(S.t_atom_sites(buf), T.atom_site)
    prm = S.current_params(PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], G0, PAR["tol"], PAR["m_e"], PAR["V0"],
                           contact_x_lo=x_lo, contact_x_hi=x_hi)
    S.t_assemble(buf, prm)
    _compare_assembly(S, buf, T)
    # the split operator through the generic SpMV entry
    mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
    x = np.cos(np.arange(T.Nsub) * 0.7) + 1.5
    p = torch.as_tensor(x, device="cuda")
    Ap = torch.empty_like(p)
    mat.spmv(p, Ap)
    M = T.merged_csr()
    assert np.all(np.abs(Ap.cpu().numpy() - T.spmv(x)) <= 1e-12 * (abs(M) @ np.abs(x)))
    # current and power kernels on prescribed potentials (0 CG iterations leave the start vector untouched):
    # I_macro is a sum of differences of nearly equal potentials, so it is compared on identical inputs
    rng = np.random.default_rng(1)
    x0 = PAR["Vd"] * (0.5 + 0.5 * np.cos(np.arange(T.Nsub) * 0.05)) + 1e-3 * rng.standard_normal(T.Nsub)
    kw = dict(contact_x_lo=x_lo, contact_x_hi=x_hi)
    args = (d["n1"], d["n1"], d["layers"], PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], G0, PAR["tol"], PAR["nn_dist"],
            PAR["m_e"], PAR["V0"], 2)
    for heating in (False, True):
        buf.atom_virtual_potentials.zero_()
        buf.atom_virtual_potentials[:T.Nsub] = torch.as_tensor(x0, device="cuda")
        buf.site_power.fill_(-7.0)
        im, st = S.update_power_gpu_sparse_dist(buf, *args, heating, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=0, **kw)
        assert st["iterations"] == 0
        m = np.zeros(T.N_atom + 2)
        m[:T.Nsub] = x0 * G0
        imo = T.imacro(m)
        assert abs(im - imo) <= 1e-11 * np.abs(T.val[T.row_ptr[1]:T.row_ptr[2]] * m[1]).sum(), (im, imo)
        got = buf.atom_virtual_potentials.cpu().numpy()
        if not heating:
            np.testing.assert_array_equal(got, m)
            assert np.all(buf.site_power.cpu().numpy() == -7.0)
        else:
            pw = np.full(len(d["element"]), -7.0)
            T.power(m, 1.0, pw)                          # shifts m in place
            np.testing.assert_allclose(got, m, rtol=1e-15, atol=0)
            gp = buf.site_power.cpu().numpy()
            np.testing.assert_array_equal(gp == -7.0, pw == -7.0)
            assert np.abs(gp - pw).max() <= 1e-11 * np.abs(pw[pw != -7.0]).max()
    # the CG's wiring (split SpMV, preconditioner, dots): iterates after 5 iterations from zero
    buf.atom_virtual_potentials.zero_()
    im, st = S.update_power_gpu_sparse_dist(buf, *args, False, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=5, **kw)
    xo, ito, relo = T.solve(np.zeros(T.Nsub), 1e-30, 5)
    assert st["iterations"] == ito == 5
    got = buf.atom_virtual_potentials.cpu().numpy()[:T.Nsub] / G0
    assert np.abs(got - xo).max() <= 1e-10 * np.abs(xo).max()
    # converged solve: stopping rule, iteration count, warm restart
    buf.atom_virtual_potentials.zero_()
    im, st = S.update_power_gpu_sparse_dist(buf, d["n1"], d["n1"], d["layers"], PAR["Vd"], PAR["high_G"], PAR["low_G"],
                                            PAR["loop_G"], G0, PAR["tol"], PAR["nn_dist"], PAR["m_e"], PAR["V0"], 2, False, False,
                                            1.0, cg_tolerance=1e-13, cg_max_iterations=20000, contact_x_lo=x_lo, contact_x_hi=x_hi)
    xo, ito, relo = T.solve(np.zeros(T.Nsub), 1e-13, 20000)
    assert st["converged"] == 1 and st["relres"] <= 1e-13
    od = _device_order_solve(oracle, [_device_rank(km, oracle, buf, 0)], [T.Nsub], [0], 1e-13, 20000)
    assert st["iterations"] == od["iterations"], (st["iterations"], od["iterations"], ito)
    np.testing.assert_array_equal(buf.atom_virtual_potentials.cpu().numpy()[:T.Nsub], od["x"] * G0)
    assert abs(st["iterations"] - ito) <= max(3, 0.05 * ito), (st["iterations"], ito)      # natural order: a nearby count
    v = buf.atom_virtual_potentials.cpu().numpy()[:T.Nsub] / G0
    res = T.rhs - T.spmv(v)
    res_o = T.rhs - T.spmv(xo)
    assert np.linalg.norm(res) <= 3 * np.linalg.norm(res_o), (np.linalg.norm(res), np.linalg.norm(res_o))
    tight = np.r_[0, 1, 2 + np.nonzero(np.isin(T.atom_element[:-1], [TI, N_EL]))[0]]
    assert np.abs(v[tight] - xo[tight]).max() <= 2e-6 * np.abs(xo).max()
    assert im > 0
    buf.freeGPUmemory()
    comm.close()


def test_5nm_device(km, oracle, dev5, ref5, torch):
    """The reference's 5 nm device with solve_current on (BASELINE config 3's path at config 1's size):
    25 682-row neighbour matrix (two 578-entry virtual-node rows), 1913 tunnel points, 36 % dense block."""
    S = km.solvers
    d = dev5
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, 25682, d["N"], d["N"])
    comm.connect()
    buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    buf.site_charge.copy_(torch.as_tensor(ref5["charge"]))
    # conduction-band edge on the GPU (update_CB_edge_gpu_sparse); the oracle gets the same array so that the
    # |dE| > tol decisions of the tunnel pattern are taken on identical numbers
    S.update_CB_edge_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"], len(d["metals"]))
    cb = buf.site_CB_edge.cpu().numpy()
    high_G, low_G, loop_G = 1e5 * d["high_G"], d["low_G"], 1e7 * d["high_G"]      # src/kmc_main.cpp:294-296
    tol, m_e, V0 = Q * 0.01, 0.85 * 9.11e-31, 1.6
    T = oracle.TSystem(d["xyz"], d["element"], ref5["charge"], cb, d["metals"], d["nn_dist"], NL, NL, 10, d["Vd"], high_G, low_G,
                       loop_G, tol, m_e, V0)
    S.initialize_sparsity_T(buf, d["pbc"], d["nn_dist"], NL, NL, 10, comm)
    assert buf.N_atom_ == T.N_atom == 25681
    prm = S.current_params(d["Vd"], high_G, low_G, loop_G, G0, tol, m_e, V0)
    S.t_assemble(buf, prm)
    tn = _compare_assembly(S, buf, T)
    info = S.t_info(buf)
    assert info["tunnel_points"] == 1913 and info["nnz_tunnel"] == len(T.sub_col)
    minfo = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed)).info()
    assert minfo["spmv_kind"] == 2          # the virtual-node rows did not push the matrix off the window kernel
    # current and power on prescribed potentials (see test_small_device_single_rank)
    rng = np.random.default_rng(2)
    ax = d["xyz"][T.atom_site, 0]
    x0 = np.zeros(T.Nsub)
    x0[0], x0[1] = 0.0, d["Vd"]
    x0[2:] = d["Vd"] * np.clip(1 - ax[:-1] / 52.0, 0, 1) + 1e-3 * rng.standard_normal(T.N_atom - 1)
    args = (NL, NL, 10, d["Vd"], high_G, low_G, loop_G, G0, tol, d["nn_dist"], m_e, V0, len(d["metals"]))
    buf.atom_virtual_potentials.zero_()
    buf.atom_virtual_potentials[:T.Nsub] = torch.as_tensor(x0, device="cuda")
    im, st = S.update_power_gpu_sparse_dist(buf, *args, True, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=0)
    m = np.zeros(T.N_atom + 2)
    m[:T.Nsub] = x0 * G0
    imo = T.imacro(m)
    assert abs(im - imo) <= 1e-11 * np.abs(T.val[T.row_ptr[1]:T.row_ptr[2]] * m[1]).sum(), (im, imo)
    pw = np.zeros(d["N"])
    T.power(m, 1.0, pw)
    np.testing.assert_allclose(buf.atom_virtual_potentials.cpu().numpy(), m, rtol=1e-15, atol=0)
    gp = buf.site_power.cpu().numpy()
    assert np.abs(gp - pw).max() <= 1e-10 * np.abs(pw).max() and pw.max() > 0
    # the reference's benchmark setting: 100 iterations whatever the residual (current_solver_gpu.cu:1455-1456);
    # iterates of the two implementations agree while rounding has not yet been amplified (5 iterations checked)
    buf.atom_virtual_potentials.zero_()
    im, st = S.update_power_gpu_sparse_dist(buf, *args, False, False, 1.0)
    assert st["iterations"] == 100 and st["converged"] == 0
    buf.atom_virtual_potentials.zero_()
    im, st = S.update_power_gpu_sparse_dist(buf, *args, False, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=5)
    xo, ito, relo = T.solve(np.zeros(T.Nsub), 1e-30, 5)
    got = buf.atom_virtual_potentials.cpu().numpy()[:T.Nsub] / G0
    assert st["iterations"] == ito == 5 and np.abs(got - xo).max() <= 1e-10 * np.abs(xo).max()
    # converged (the reference's commented-out tolerance 1e-15 * N_atom), cold then warm
    buf.atom_virtual_potentials.zero_()
    im, st = S.update_power_gpu_sparse_dist(buf, *args, False, False, 1.0, cg_tolerance=1e-15 * T.N_atom, cg_max_iterations=2000)
    xo, ito, relo = T.solve(np.zeros(T.Nsub), 1e-15 * T.N_atom, 2000)
    # conductances from 1e7 (loop) to 1e-17 (far tunnel pairs): the Jacobi-PCG count moves with the summation
    # order of the dots by ~10 % here (349 in the device's order against 316 in the oracle's natural order; 2 % on
    # the K system, whose span is 1e8).  So the count is held to the oracle adding in the DEVICE's order: identical.
    od = _device_order_solve(oracle, [_device_rank(km, oracle, buf, 0)], [T.Nsub], [0], 1e-15 * T.N_atom, 2000)
    assert st["converged"] == 1 and st["iterations"] == od["iterations"], (st, od["iterations"], ito)
    np.testing.assert_array_equal(buf.atom_virtual_potentials.cpu().numpy()[:T.Nsub], od["x"] * G0)
    print("T 5 nm: %d iterations (oracle, device order: %d; natural order: %d), assembly %.3f ms, solve %.3f ms"
          % (st["iterations"], od["iterations"], ito, st["ms_assembly"], st["ms_solve"]))
    v = buf.atom_virtual_potentials.cpu().numpy() / G0
    assert abs(v[1] - d["Vd"]) < 1e-3 and abs(v[NL] - d["Vd"]) < 0.1          # the reference's sanity check (:2014-2020)
    # true residual: the recurrence stops at 2.6e-11; what rounding leaves between recurrence and true residual on a
    # system spanning 1e7 ... 1e-17 is the oracle's to say: the device may not be more than 3 x worse
    res = np.linalg.norm(T.rhs - T.spmv(v[:T.Nsub])) / np.linalg.norm(T.rhs)
    res_o = np.linalg.norm(T.rhs - T.spmv(xo)) / np.linalg.norm(T.rhs)
    print("T 5 nm: true residual %.3e (oracle, natural order: %.3e)" % (res, res_o))
    assert res <= 3 * res_o, (res, res_o)
    # the current from the loop side (Kirchhoff at the source node): equal to the reference's injection-side sum up to
    # that node's residual, G0 |r_1| <= G0 sqrt(T_11 r.z) -- here small against the current itself
    mm = buf.atom_virtual_potentials.cpu().numpy()
    i_loop = loop_G * (d["Vd"] * G0 - (mm[1] - mm[0]))
    assert abs(im - i_loop) <= G0 * np.sqrt((loop_G + NL * high_G) * st["rz"]) * 1.01, (im, i_loop)
    print("T 5 nm: I_macro %.6e (injection side), %.6e (loop side)" % (im, i_loop))
    assert im > 0
    buf.freeGPUmemory()
    comm.close()


def test_inprocess_builds_read_what_was_uploaded(km, oracle, torch):
    """Regression ("the flake of the in-process groups"): three host threads upload their site arrays from
    pageable memory and build their rows of T at once, round after round, on device memory that was filled with junk
    and handed back before every round -- so that a kernel reading an array as it was BEFORE its upload gets visibly
    wrong coordinates instead of last round's identical ones.  Before the set-up kernels moved to the caller's stream
    one round in eight built a wrong pattern."""
    S = km.solvers
    d = small_device(seed=11)
    metals = np.array([TI, N_EL], np.int32)
    a = 2.5
    x_lo, x_hi = (d["layers"] - 1) * a - 0.1, (d["layers"] + 7) * a + 0.1
    T = oracle.TSystem(d["xyz"], d["element"], d["charge"], d["cb"], metals, PAR["nn_dist"], d["n1"], d["n1"], d["layers"],
                       PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], PAR["tol"], PAR["m_e"], PAR["V0"], x_lo, x_hi)
    N, P = len(d["element"]), 3
    for rnd in range(16):
        junk = [torch.randint(0, 300, ((64 << 20) // 4,), dtype=torch.int32, device="cuda"),
                torch.rand((32 << 20) // 8, dtype=torch.float64, device="cuda") * 30.0]
        torch.cuda.synchronize()
        del junk
        torch.cuda.empty_cache()
        comms = S.KMC_comm.loopback_group(T.Nsub, T.Nsub, N, N, P)
        errs = []

        def work(r):
            try:
                torch.cuda.set_device(0)
                buf = _make(km, torch, d["xyz"], d["element"], d["charge"], d["cb"], metals, d["n1"], d["layers"], comms[r])
                r0, nr = int(comms[r].displs_T[r]), int(comms[r].counts_T[r])
                rp, col = S.t_pattern(buf)
                np.testing.assert_array_equal(rp, T.row_ptr[r0:r0 + nr + 1] - T.row_ptr[r0])
                np.testing.assert_array_equal(col, T.col[T.row_ptr[r0]:T.row_ptr[r0 + nr]])
                buf.freeGPUmemory()
            except Exception as e:  # pragma: no cover
                errs.append("round %d, rank %d: %s" % (rnd, r, str(e)[:600]))

        threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        for c in comms:
            c.close()
        assert not errs, "\n".join(errs)


@pytest.mark.parametrize("P,transport,storage", [(P, tr, stg) for P in (2, 3) for tr in ("loopback", "p2p") for stg in ("bitmap", "tiles")]
                         + [(5, "p2p", "tiles")])      # (five ranks: the first and the last own contact atoms only -- no tunnel point of their own, tiles all the same)
def test_small_device_multirank(km, oracle, torch, P, transport, storage, monkeypatch):
    """Row-partitioned T over an in-process group: halo exchange of the neighbour part, all-gather of the tunnel
    sub-vector, replicated current and power.  transport "loopback": host-synchronous exchanges, in order; "p2p": the
    device-side peer-to-peer protocol, where the sub-vector all-gather runs on the comm stream underneath the
    neighbour part of every SpMV (kmcf_subop_begin / _finish).  Same results, bit for bit (the oracle's device-order run
    does not know the transport).  storage "bitmap": every rank holds its rows of the tunnel block (bitmap + packed
    values); "tiles": the block as dense symmetric 64 x 64 tiles whose strips are dealt to the ranks (what a group gets for
    a block more than a quarter full; KMCF_SUB_DENSE=1 forces it at this size, strips of one tile so that every rank holds
    one), the ranks' partial sums all-gathered and added in rank order -- against the oracle walking the same tiles."""
    monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
    monkeypatch.setenv("KMCF_SUB_STRIP", "1")
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    S = km.solvers
    d = small_device(seed=11)
    a = 2.5
    x_lo, x_hi = (d["layers"] - 1) * a - 0.1, (d["layers"] + 7) * a + 0.1
    if P == 5:                                         # a window over the middle of the oxide only: the outer ranks own no tunnel point
        x_lo, x_hi = (d["layers"] + 1) * a - 0.1, (d["layers"] + 5) * a + 0.1
    metals = np.array([TI, N_EL], np.int32)
    T = oracle.TSystem(d["xyz"], d["element"], d["charge"], d["cb"], metals, PAR["nn_dist"], d["n1"], d["n1"], d["layers"],
                       PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], PAR["tol"], PAR["m_e"], PAR["V0"], x_lo, x_hi)
    N = len(d["element"])
    comms = S.KMC_comm.loopback_group(T.Nsub, T.Nsub, N, N, P)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            buf = _make(km, torch, d["xyz"], d["element"], d["charge"], d["cb"], metals, d["n1"], d["layers"], comm)
            prm = S.current_params(PAR["Vd"], PAR["high_G"], PAR["low_G"], PAR["loop_G"], G0, PAR["tol"], PAR["m_e"], PAR["V0"],
                                   contact_x_lo=x_lo, contact_x_hi=x_hi)
            S.t_assemble(buf, prm)
            r0, nr = int(comm.displs_T[r]), int(comm.counts_T[r])
            _compare_assembly(S, buf, T, r0, nr)
            assert S.t_info(buf)["tunnel_dense"] == (1 if storage == "tiles" else 0)
            buf.site_power.fill_(-7.0)
            im, st = S.update_power_gpu_sparse_dist(buf, d["n1"], d["n1"], d["layers"], PAR["Vd"], PAR["high_G"], PAR["low_G"],
                                                    PAR["loop_G"], G0, PAR["tol"], PAR["nn_dist"], PAR["m_e"], PAR["V0"], 2, True,
                                                    False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000, contact_x_lo=x_lo,
                                                    contact_x_hi=x_hi)
            out[r] = dict(im=im, st=st, v=buf.atom_virtual_potentials.cpu().numpy().copy(),
                          pw=buf.site_power.cpu().numpy().copy(), part=_device_rank(km, oracle, buf, r0, spread=storage == "tiles", strip=1),
                          r0=r0, nr=nr, info=S.t_info(buf))
            buf.freeGPUmemory()
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(180)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish"
    for c in comms:
        c.close()
    if storage == "tiles":                             # every rank holds a share of the tiles (strips of one tile: the first ranks, one each)
        nb = (out[0]["info"]["tunnel_points"] + 63) // 64
        held = [o["info"]["tunnel_bytes"] // 32768 for o in out]
        assert sum(held) == nb * (nb + 1) // 2 and min(held[:min(P, nb * (nb + 1) // 2)]) > 0, (held, nb)
        print("tunnel points per rank %s, tiles per rank %s" % ([o["info"]["tunnel_points_rank"] for o in out], held))
        if P == 5:
            assert min(o["info"]["tunnel_points_rank"] for o in out) == 0      # (the case this parameter is here for)
    xo, ito, relo = T.solve(np.zeros(T.Nsub), 1e-13, 20000)
    m = np.zeros(T.N_atom + 2)
    m[:T.Nsub] = xo * G0
    imo = T.imacro(m)
    pw = np.full(N, -7.0)
    T.power(m, 1.0, pw)
    # the oracle adding in the device's order over the P ranks: identical count and potentials (heating on: the
    # potentials were shifted by |min| after the scaling, current_solver_gpu.cu:2068-2071)
    od = _device_order_solve(oracle, [o["part"] for o in out], [o["nr"] for o in out], [o["r0"] for o in out], 1e-13, 20000)
    mo = od["x"] * G0
    mo = mo + abs(min(mo[2:].min(), 0.0))        # (the minimum runs over N_atom + 2 entries: the last one is never solved, 0)
    for o in out:
        assert o["st"]["converged"] == 1 and o["st"]["iterations"] == od["iterations"], (o["st"]["iterations"], od["iterations"], ito)
        np.testing.assert_array_equal(o["v"][:T.Nsub], mo)
        assert abs(o["st"]["iterations"] - ito) <= max(3, 0.05 * ito)
        assert (o["im"] > 0 or P == 5) and abs(o["im"] - out[0]["im"]) == 0     # (the narrowed window of the 5-rank case carries no current)
        np.testing.assert_array_equal(o["v"], out[0]["v"])             # replicated bit for bit
        np.testing.assert_array_equal(o["pw"], out[0]["pw"])
        np.testing.assert_array_equal(o["pw"] == -7.0, pw == -7.0)
        tight = np.r_[0, 1, 2 + np.nonzero(np.isin(T.atom_element[:-1], [TI, N_EL]))[0]]
        assert np.abs(o["v"][tight] - m[tight]).max() <= 2e-6 * np.abs(m).max()


@pytest.mark.parametrize("P", [2, 3])
def test_5nm_device_rank_group_holds_the_tunnel_block_as_tiles(km, oracle, dev5, ref5, torch, monkeypatch, P):
    """The reference's 5 nm device over a group of P ranks on the peer-to-peer transport with the tunnel block (1913 points,
    30 block rows) as dense symmetric tiles whose 44 strips are dealt to the ranks (kmcf_subop::spread; KMCF_SUB_DENSE=1
    forces it below 2048 points): every rank forms its partial of all sums from the strips it holds, the partials are
    all-gathered and added in rank order.  Held against the oracle walking the same tiles rank by rank -- iteration
    count and every potential identical -- and against the group holding the block as row slices (bitmap): the same
    current to the solver's tolerance, the same power pattern."""
    S = km.solvers
    d = dev5
    monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
    monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    par = dict(Vd=d["Vd"], high_G=1e5 * d["high_G"], low_G=d["low_G"], loop_G=1e7 * d["high_G"], tol=Q * 0.01, m_e=0.85 * 9.11e-31, V0=1.6)
    NL, xyz, element = d["N_contact"], d["xyz"], d["element"]
    cb = 1.60217663e-19 * d["Vd"] * (0.5 - np.clip(xyz[:, 0] / 52.0, 0, 1))
    N = len(element)
    na = int(np.isin(element, [0, 1], invert=True).sum())
    res = {}
    for storage in ("tiles", "bitmap"):
        monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
        comms = S.KMC_comm.loopback_group(na + 1, na + 1, N, N, P)
        out, errs = [None] * P, []

        def work(r):
            try:
                torch.cuda.set_device(0)
                comm = comms[r]
                buf = S.GPUBuffers(N, element, xyz[:, 0], xyz[:, 1], xyz[:, 2], 52, d["sigma"], d["k"], d["lattice"], d["metals"])
                buf.site_charge.copy_(torch.as_tensor(np.asarray(ref5["charge"], np.int32)))
                buf.site_CB_edge = torch.as_tensor(cb, device="cuda")
                S.initialize_sparsity_T(buf, 0, d["nn_dist"], NL, NL, 10, comm)
                prm = S.current_params(par["Vd"], par["high_G"], par["low_G"], par["loop_G"], G0, par["tol"], par["m_e"], par["V0"])
                S.t_assemble(buf, prm)
                info = S.t_info(buf)
                buf.atom_virtual_potentials.zero_()
                buf.site_power.zero_()
                im, st = S.update_power_gpu_sparse_dist(buf, NL, NL, 10, par["Vd"], par["high_G"], par["low_G"], par["loop_G"], G0, par["tol"],
                                                        d["nn_dist"], par["m_e"], par["V0"], len(d["metals"]), True, False, 1.0,
                                                        cg_tolerance=1e-13, cg_max_iterations=20000)
                r0, nr = int(comm.displs_T[r]), int(comm.counts_T[r])
                out[r] = dict(im=im, st=st, info=info, v=buf.atom_virtual_potentials.cpu().numpy().copy(), pw=buf.site_power.cpu().numpy().copy(),
                              part=_device_rank(km, oracle, buf, r0, spread=storage == "tiles") if storage == "tiles" else None, r0=r0, nr=nr)
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
        for o in out:
            assert o["st"]["converged"] == 1 and o["info"]["tunnel_points"] == 1913
            assert o["info"]["tunnel_dense"] == (1 if storage == "tiles" else 0)
            np.testing.assert_array_equal(o["v"], out[0]["v"])
            np.testing.assert_array_equal(o["pw"], out[0]["pw"])
            assert o["im"] == out[0]["im"]
        res[storage] = out
    tl, bm = res["tiles"], res["bitmap"]
    held = [o["info"]["tunnel_bytes"] // 32768 for o in tl]
    assert sum(held) == 30 * 31 // 2 and max(held) - min(held) <= 16, held             # 465 tiles, a strip's length apart at most
    n = na + 1
    od = _device_order_solve(oracle, [o["part"] for o in tl], [o["nr"] for o in tl], [o["r0"] for o in tl], 1e-13, 20000)
    mo = od["x"] * G0
    mo = mo + abs(min(mo[2:].min(), 0.0))
    assert tl[0]["st"]["iterations"] == od["iterations"], (tl[0]["st"]["iterations"], od["iterations"])
    np.testing.assert_array_equal(tl[0]["v"][:n], mo)
    print("T 5 nm over %d ranks, tunnel block as tiles (%s per rank): %d iterations (oracle in the device's order: %d; row slices: %d), "
          "I_macro %.9e against %.9e" % (P, held, tl[0]["st"]["iterations"], od["iterations"], bm[0]["st"]["iterations"], tl[0]["im"], bm[0]["im"]))
    assert abs(tl[0]["st"]["iterations"] - bm[0]["st"]["iterations"]) <= max(3, 0.1 * bm[0]["st"]["iterations"])
    # (two summation orders under one stopping rule: the source node's residual is what separates the currents -- 2e-5 of it here)
    assert abs(tl[0]["im"] - bm[0]["im"]) <= 1e-4 * abs(bm[0]["im"])
    assert np.abs(tl[0]["pw"] - bm[0]["pw"]).max() <= 1e-3 * np.abs(bm[0]["pw"]).max() + 1e-300
    np.testing.assert_array_equal(tl[0]["pw"] == 0, bm[0]["pw"] == 0)


@pytest.mark.parametrize("device", ["small", "5nm"])
def test_dense_symmetric_tunnel_block_matches_bitmap_and_oracle(km, oracle, dev5, ref5, torch, monkeypatch, device):
    """The tunnel block stored as dense symmetric 64 x 64 tiles (the upper block triangle once; what a > 50 % dense block
    of one rank gets, KMCF_SUB_DENSE=1 forces it here) against the bitmap + packed-values storage and the oracle:
    same values, same diagonal, same operator (to rounding: the two add in different orders), same solve, current and
    power.  The 40 nm test (tests/test_gpu_fullsize.py) runs this storage at full size through properties."""
    S = km.solvers
    if device == "small":
        d = small_device(seed=7)
        a = 2.5
        kw = dict(contact_x_lo=(d["layers"] - 1) * a - 0.1, contact_x_hi=(d["layers"] + 7) * a + 0.1)
        metals = np.array([TI, N_EL], np.int32)
        par = dict(PAR)
        n1, layers, xyz, element, charge, cb = d["n1"], d["layers"], d["xyz"], d["element"], d["charge"], d["cb"]
        lattice, sigma, kk, nmet = [1, 1, 1], 3.5e-10, 1.0, 2
    else:
        d = dev5
        kw = {}
        metals = d["metals"]
        par = dict(Vd=d["Vd"], high_G=1e5 * d["high_G"], low_G=d["low_G"], loop_G=1e7 * d["high_G"], tol=Q * 0.01, m_e=0.85 * 9.11e-31,
                   V0=1.6, nn_dist=d["nn_dist"])
        n1, layers, xyz, element, charge = d["N_contact"], 10, d["xyz"], d["element"], ref5["charge"]
        cb = 1.60217663e-19 * d["Vd"] * (0.5 - np.clip(xyz[:, 0] / 52.0, 0, 1))            # a smooth band edge: enough for a storage test
        lattice, sigma, kk, nmet = d["lattice"], d["sigma"], d["k"], len(d["metals"])
    N = len(element)
    res = {}
    for dense in (0, 1, 2):                  # bitmap + packed values | dense symmetric tiles | jagged symmetric tiles (entries only)
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        comm = S.KMC_comm(N, N, N, N)
        comm.connect()
        buf = S.GPUBuffers(N, element, xyz[:, 0], xyz[:, 1], xyz[:, 2], 52, sigma, kk, lattice, metals)
        buf.site_charge.copy_(torch.as_tensor(np.asarray(charge, np.int32)))
        buf.site_CB_edge = torch.as_tensor(np.asarray(cb, np.float64), device="cuda")
        na = int(np.isin(element, [0, 1], invert=True).sum())
        comm.counts_T, comm.displs_T = comm.partition(na + 1, 1)
        S.initialize_sparsity_T(buf, 0, par["nn_dist"], n1, n1, layers, comm)
        prm = S.current_params(par["Vd"], par["high_G"], par["low_G"], par["loop_G"], G0, par["tol"], par["m_e"], par["V0"], **kw)
        S.t_assemble(buf, prm)
        tn, v = S.t_tunnel(buf), S.t_vectors(buf)
        n = S.t_info(buf)["Nsub"]
        assert S.t_info(buf)["tunnel_dense"] == dense
        mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
        rng = np.random.default_rng(5)
        x = rng.standard_normal(n)
        p = torch.as_tensor(x, device="cuda")
        Ap = torch.empty_like(p)
        mat.spmv(p, Ap)
        args = (n1, n1, layers, par["Vd"], par["high_G"], par["low_G"], par["loop_G"], G0, par["tol"], par["nn_dist"], par["m_e"], par["V0"], nmet)
        buf.atom_virtual_potentials.zero_()
        buf.site_power.zero_()
        im, st = S.update_power_gpu_sparse_dist(buf, *args, True, False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000, **kw)
        # either storage against the oracle adding in ITS order (bitmap: a wave per row; tiles: strips, row and column
        # sums, four waves per block row): the same solve, bit for bit (heating on: potentials scaled, then shifted)
        od = _device_order_solve(oracle, [_device_rank(km, oracle, buf, 0, dense=bool(dense))], [n], [0], 1e-13, 20000)
        mo = od["x"] * G0
        mo = mo + abs(min(mo[2:].min(), 0.0))
        assert st["iterations"] == od["iterations"], (dense, st["iterations"], od["iterations"])
        np.testing.assert_array_equal(buf.atom_virtual_potentials.cpu().numpy()[:n], mo)
        res[dense] = dict(tn=tn, dinv=v["dinv"], Ap=Ap.cpu().numpy(), x=x, im=im, st=st, m=buf.atom_virtual_potentials.cpu().numpy().copy(),
                          pw=buf.site_power.cpu().numpy().copy(), n=n)
        buf.freeGPUmemory()
        comm.close()
    a, b = res[0], res[1]
    np.testing.assert_array_equal(a["tn"]["row_ptr"], b["tn"]["row_ptr"])
    np.testing.assert_array_equal(a["tn"]["col"], b["tn"]["col"])
    rows_of = np.repeat(np.arange(len(a["tn"]["row_ptr"]) - 1) + a["tn"]["first"], np.diff(a["tn"]["row_ptr"]))
    off = a["tn"]["col"] != rows_of
    np.testing.assert_array_equal(a["tn"]["val"][off], b["tn"]["val"][off])                                      # the same WKB values, bit for bit
    np.testing.assert_allclose(b["tn"]["val"][~off], a["tn"]["val"][~off], rtol=1e-12)                           # diagonal entries = -(row sums)
    np.testing.assert_allclose(b["tn"]["diag"], a["tn"]["diag"], rtol=1e-12)                                     # -(row sums): another order
    np.testing.assert_allclose(b["dinv"], a["dinv"], rtol=1e-12)
    # operator: |dy| <= 1e-12 * sum |a_ij x_j| with the sum bounded through the diagonal magnitudes
    scale = np.abs(1.0 / a["dinv"]) * np.abs(a["x"]).max() * 2
    assert np.all(np.abs(a["Ap"] - b["Ap"]) <= 1e-12 * scale), float((np.abs(a["Ap"] - b["Ap"]) / scale).max())
    assert a["st"]["converged"] == b["st"]["converged"] == 1
    assert abs(a["st"]["iterations"] - b["st"]["iterations"]) <= max(3, 0.1 * a["st"]["iterations"])
    metal = np.r_[0, 1]
    assert np.abs(a["m"][metal] - b["m"][metal]).max() <= 1e-6 * np.abs(a["m"]).max()
    assert np.abs(a["pw"] - b["pw"]).max() <= 1e-5 * np.abs(a["pw"]).max() + 1e-300
    np.testing.assert_array_equal(a["pw"] == 0, b["pw"] == 0)
    # the jagged tiles hold the dense tiles' entries and add them in the same order (an absent entry added 0.0 there):
    # everything identical, bit for bit -- values, diagonal, product, iterates, current, power
    c = res[2]
    for key in ("val", "diag", "row_ptr", "col"):
        np.testing.assert_array_equal(c["tn"][key], b["tn"][key])
    np.testing.assert_array_equal(c["dinv"], b["dinv"])
    np.testing.assert_array_equal(c["Ap"], b["Ap"])
    assert c["st"]["iterations"] == b["st"]["iterations"] and c["im"] == b["im"]
    np.testing.assert_array_equal(c["m"], b["m"])
    np.testing.assert_array_equal(c["pw"], b["pw"])


def test_in_process_builds_under_stress():
    """tools/tmulti_stress.py as a regression test: the four variants of test_small_device_multirank cycle
    after cycle in ONE process, device memory re-allocated and filled with junk in between -- the history in which an
    in-process group once built a T pattern from coordinates its kernels did not see yet.  The set-up
    kernels run on the caller's stream since then, and every set-up now compares what its kernels see with a
    synchronous host copy (KMCF_ERR_STATE on a mismatch: loud instead of a silently wrong pattern)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "tmulti_stress.py"), "10", "poison"], capture_output=True, text=True,
                         timeout=600, cwd=root)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "0 failures in 10 cycles" in out.stdout, out.stdout[-2000:]
