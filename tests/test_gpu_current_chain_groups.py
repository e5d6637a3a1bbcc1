"""GPU: the current chain of a bias point on a rank group with nothing handed in from a one-rank solve -- band edge
on the group, T assembly, current solve -- on the conducting 4 x 4-cell crossbar of tests/test_gpu_conducting.py; and the
band edge of the full synthetic 40 nm crossbar on a group of two against one-rank solves of the same device."""
import threading

import numpy as np
import pytest

from test_gpu_conducting import _current, _device

pytestmark = pytest.mark.gpu

EV = 1.60217663e-19


def _threads(P, work, seconds):
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
    assert all(o is not None for o in out), "a rank did not finish"
    return out


def test_conducting_crossbar_whole_chain_on_a_group(km, monkeypatch):
    """P = 2, peer-to-peer transport, NO band-edge array handed in: every rank calls update_CB_edge_gpu_sparse on the
    group and assembles T from the array that call left it with.  I_macro is identical on both ranks and within 1e-8
    relative of the one-rank chain's (the bar tests/test_gpu_conducting.py holds the group to with a one-rank band
    edge); the injection side equals the loop side within the residual bound, as there."""
    import torch
    S = km.solvers
    monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
    monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "60000")
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    d = km.structure.synth_crossbar_40nm(tiles=4, filament=4.0)
    N, NL = d["N"], d["N_contact"]
    N_atom = int(((d["element"] != 0) & (d["element"] != 1)).sum())
    P = 2
    monkeypatch.setenv("KMCF_SUB_DENSE", "1")
    one = _device(km, 4.0, d=d)
    try:
        i1, l1, st1, _, _ = _current(one, 1e-18, first=True, touch_env=False)
        cb1 = one["buf"].site_CB_edge.cpu().numpy().copy()
    finally:
        one["buf"].freeGPUmemory()
        one["comm"].close()
    monkeypatch.delenv("KMCF_SUB_DENSE", raising=False)           # the group: dense tiles dealt to the ranks (its default)
    comms = S.KMC_comm.loopback_group(N - 2 * NL, N_atom + 1, N, N, P)

    def work(r):
        torch.cuda.set_device(0)
        dev = _device(km, 4.0, comm=comms[r], d=d)
        try:
            res = _current(dev, 1e-18, first=True, touch_env=False)          # cb=None: the band edge is the group's
            return res + (dev["buf"].site_CB_edge.cpu().numpy().copy(),)
        finally:
            dev["buf"].freeGPUmemory()

    try:
        out = _threads(P, work, 600)
    finally:
        for c in comms:
            c.close()
    print("one rank: I_macro %.12e (%d iterations); group of 2: I_macro %.12e (%d iterations, %.1f ms), band edge max|group - one rank| / eV = %.2e"
          % (i1, st1["iterations"], out[0][0], out[0][2]["iterations"], out[0][2]["ms_solve"], np.abs(out[0][5] - cb1).max() / EV))
    for im, il, st, info, bound, cb in out:
        assert st["converged"] == 1 and info["tunnel_points"] == 17722 and info["tunnel_dense"] == 1
        assert im == out[0][0]
        assert np.array_equal(cb, out[0][5])
        assert abs(im - il) <= max(bound * 1.01, 1e-25) and abs(im - il) <= 1e-8 * im, (im, il, bound)
        assert abs(im - i1) <= 1e-8 * i1, (im, i1)


def test_band_edge_40nm_on_a_group_of_two(km, monkeypatch):
    """Full size, once: the synthetic 40 nm crossbar's band edge on a P = 2 loopback group against one-rank solves of the
    same device from the same zero start (loopback: two ranks' waiting kernels sharing one card at this size would
    measure the scheduler).  No accuracy bar exists at this size, so it is taken from the one-rank code in this test:
    d0 = max|pcg form - scaled form| / eV on one rank, two solves of one system that differ by rounding only and stop
    by the same rule -- which is also what a group solve and a one-rank solve are.  Required:
    max|group - one-rank pcg| / eV <= 2 d0 (d0 is a single sample of such a distance), iterations within max(3, 5 %)."""
    import torch
    S = km.solvers
    monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    d = km.structure.synth_crossbar_40nm()
    N, NL = d["N"], d["N_contact"]

    def solve(comm):
        buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                           d["lattice"], d["metals"])
        try:
            S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
            st = S.update_CB_edge_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                             len(d["metals"]))
            return st, buf.site_CB_edge.cpu().numpy().copy()
        finally:
            buf.freeGPUmemory()

    one = {}
    for form, opts in (("pcg", {}), ("scaled", {"KMCF_CB_SCALED": "1"})):
        comm = S.KMC_comm(N - 2 * NL, N + 1, N, N, options=opts)
        comm.connect()
        try:
            one[form] = solve(comm)
        finally:
            comm.close()
        assert one[form][0]["converged"] == 1
    d0 = np.abs(one["pcg"][1] - one["scaled"][1]).max() / EV
    P = 2
    comms = S.KMC_comm.loopback_group(N - 2 * NL, N + 1, N, N, P)

    def work(r):
        torch.cuda.set_device(0)
        comms[r].connect()
        return solve(comms[r])

    try:
        out = _threads(P, work, 900)
    finally:
        for c in comms:
            c.close()
    dist = np.abs(out[0][1] - one["pcg"][1]).max() / EV
    it1 = one["pcg"][0]["iterations"]
    print("40 nm band edge: one rank pcg %d iterations, %.1f ms; scaled %d iterations, %.1f ms; d0 = %.3e; group of 2 "
          "(loopback, one card): %d iterations, %.1f ms, max|group - one rank| / eV = %.3e"
          % (it1, one["pcg"][0]["ms_solve"], one["scaled"][0]["iterations"], one["scaled"][0]["ms_solve"], d0,
             out[0][0]["iterations"], out[0][0]["ms_solve"], dist))
    for st, cb in out:
        assert st["converged"] == 1
        assert st["iterations"] == out[0][0]["iterations"] and st["rz"] == out[0][0]["rz"]
        assert np.array_equal(cb, out[0][1])
        assert abs(st["iterations"] - it1) <= max(3, 0.05 * it1), (st["iterations"], it1)
        assert np.all(cb[:NL] == d["Vd"] / 2 * EV) and np.all(cb[-NL:] == -d["Vd"] / 2 * EV)
    assert dist <= 2 * d0, (dist, d0)
