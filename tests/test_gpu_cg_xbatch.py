"""GPU: the batched x update of the classic PCG loop (KMCF_CG_XBATCH = B: p_k in slot k % B of a ring of B buffers,
x += alpha p applied once in B iterations, csrc/kmcf_cg.hip) against the oracle in the device's summation order and
against B = 1, bit for bit: the batch applies the same operations to the same operands in the same order, so x, r, the
iteration count, r.z and b.b must be IDENTICAL for every B.

Matrices: symmetric positive-definite chains (1-D Laplacians with three coded off-diagonal values and a varying
diagonal) through the public matrix API, solved from a non-zero start guess as the loop of kernels
(KMCF_CG_RESIDENT=0) on the coded row-per-lane SpMV, which is what the device-order oracle restates.

Shapes (a vector block owns 512 rows, two per lane; the grid is capped at 2048 blocks):
  n = 3, 511       most lanes have no pair, the odd last row is block 0 / thread 0's;
  n = 512, 513     one block exactly, and one row more;
  n = 256*512+513  the second grid-stride step of the vector kernels -- in a child process with KMCF_DEVICE_SHARE=8
                   (read once per process), which caps the grid at 256 blocks: the path the 40 nm matrix takes at 2048.
Fixed iteration counts 1, 2, 3, 4, 5, 8, 9: the limit is reached with 0 ... B-1 and with B updates pending, which the
caller's output kernel (kmcf_pcg_jacobi: cg_out_kernel) or cg_x_kernel (the workspace loop, reached from the public
ABI through kmcf_solve_sparse_CG_Jacobi: unpreconditioned instance, absolute rule) then apply.  Solves that stop on
the relative rule after 4, 5, 6 and 7 iterations -- every residue mod 2, 3 and 4 -- flush in the loop head's stop
path; the tolerances are cut from the oracle's own r.z history and the oracle's count is asserted first.
kmcf_pcg_workspace (relative rule) and kmcf_jacobi_cg_workspace_absolute are internal: they are driven by the K solve
and the CB-edge solve of the 5 nm device, B = 2, 3, 4 against B = 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = (1, 2, 3, 4, 5, 8, 9)
BATCHES = (2, 3, 4)
OPTIONS = {"KMCF_CG_RESIDENT": "0", "KMCF_CG_VARIANT": "classic", "KMCF_SPMV_KIND": "2", "KMCF_SPMV_CODED": "1",
           "KMCF_SPMV_SELL": "1"}
BIG_SHARE, BIG_N = 8, 256 * 512 + 513


def _chain(n, diag=None):
    """CSR of a symmetric chain: a[i, i+1] = a[i+1, i] in {-1, -0.5, -0.25}, diagonal 2.5 ... 3.5 (or `diag`):
    strictly diagonally dominant, hence positive definite."""
    import scipy.sparse as sp
    off = np.array([-1.0, -0.5, -0.25])[np.arange(max(n - 1, 0)) % 3]
    d = np.full(n, float(diag)) if diag is not None else 2.5 + 0.25 * (np.arange(n) % 5)
    M = sp.diags([off, d, off], [-1, 0, 1], shape=(n, n)).tocsr()
    M.sort_indices()
    return M


def _vectors(n):
    rng = np.random.default_rng(1000 + n)
    return rng.standard_normal(n), 0.5 * rng.standard_normal(n)          # b, x0 (non-zero)


class _System:
    """One matrix on one communicator; KMCF_CG_XBATCH is set per solve (communicator scope: read at the next solve)."""

    def __init__(self, km, torch, n, diag=None):
        S = km.solvers
        self.km, self.torch, self.n = km, torch, n
        self.M = _chain(n, diag)
        self.b, self.x0 = _vectors(n)
        self.dinv = 1.0 / self.M.diagonal()
        self.comm = S.KMC_comm(n, n, n, n, options=OPTIONS)
        self.comm.connect()
        self.mat = S.Distributed_matrix(self.comm, n, [n], [0], self.M.indices, self.M.indptr, self.M.data)
        self.plan = self.mat.sum_plan()
        assert self.plan["sell_active"] and self.plan["resident_tpb"] == 0 and self.plan["cg_variant"] == 0, self.plan

    def batch(self, B):
        self.comm.set_option("KMCF_CG_XBATCH", B)
        assert self.comm.get_option("KMCF_CG_XBATCH") == (str(B), 2)

    def solve(self, tol=1e-30, max_it=0, fixed=0, precond=True):
        t = self.torch
        r = t.as_tensor(self.b.copy(), device="cuda")
        x = t.as_tensor(self.x0.copy(), device="cuda")
        di = t.as_tensor(self.dinv.copy(), device="cuda") if precond else None
        st = self.km.solvers.conjugate_gradient_jacobi(self.mat, r, x, di, tol, max_it, fixed_iters=fixed)
        return st, x.cpu().numpy(), r.cpu().numpy()

    def oracle(self, O, tol=1e-30, max_it=0, fixed=0, precond=True, **kw):
        return O.pcg_device_order(self.plan, self.b, self.x0, self.dinv if precond else None, tol, max_it,
                                  fixed_iters=fixed, **kw)

    def apply(self, v):
        t = self.torch
        p = t.as_tensor(v.copy(), device="cuda")
        Ap = t.full((self.n,), 7.0, dtype=t.float64, device="cuda")
        self.mat.spmv(p, Ap)
        return Ap.cpu().numpy()

    def close(self):
        self.mat.close()
        self.comm.close()


def _same(label, got, want, bad, stopped=True):
    """got / want: (st or oracle dict, x, r).  Everything identical, or a line per difference."""
    (sa, xa, ra), (sb, xb, rb) = got, want
    print("cg-xbatch %s: iterations %d / %d, rz %.17g / %.17g, max|dx| %.3e, max|dr| %.3e"
          % (label, sa["iterations"], sb["iterations"], sa["rz"], sb["rz"], float(np.abs(xa - xb).max()),
             float(np.abs(ra - rb).max()) if ra is not None and rb is not None else 0.0))
    # (`converged` only where a stopping rule decides the end: after a fixed count the library also reports what the
    #  rule would have said of the last r.z, the oracle whether its loop stopped on it)
    if sa["iterations"] != sb["iterations"] or (stopped and bool(sa["converged"]) != bool(sb["converged"])):
        bad.append("%s: iterations %d (converged %d), wanted %d (%d)" % (label, sa["iterations"], sa["converged"],
                                                                        sb["iterations"], sb["converged"]))
    if sa["rz"] != sb["rz"] or sa["bb"] != sb["bb"]:
        bad.append("%s: rz %.17g bb %.17g, wanted %.17g %.17g" % (label, sa["rz"], sa["bb"], sb["rz"], sb["bb"]))
    if not np.array_equal(xa, xb):
        bad.append("%s: x differs in %d rows, max %.3e" % (label, int((xa != xb).sum()), float(np.abs(xa - xb).max())))
    if ra is not None and rb is not None and not np.array_equal(ra, rb):
        bad.append("%s: r differs in %d rows, max %.3e" % (label, int((ra != rb).sum()), float(np.abs(ra - rb).max())))


def _orc3(orc):
    return orc, orc["x"], orc["r"]


def _fixed_counts(s, O, label, precond=True):
    """Every fixed iteration count at B = 1, 2, 3, 4 against the oracle and against B = 1 (kmcf_pcg_jacobi: what is
    pending at the limit is applied by cg_out_kernel)."""
    bad = []
    want = {k: _orc3(s.oracle(O, fixed=k, precond=precond)) for k in FIXED}
    base = {}
    for B in (1,) + BATCHES:
        s.batch(B)
        for k in FIXED:
            got = s.solve(fixed=k, precond=precond)
            _same("%s B=%d k=%d vs oracle" % (label, B, k), got, want[k], bad, stopped=False)
            if B == 1:
                base[k] = got
            else:
                _same("%s B=%d k=%d vs B=1" % (label, B, k), got, base[k], bad)
    return bad


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("n", [3, 511, 512, 513])
def test_fixed_iterations_match_oracle_and_unbatched(km, oracle, torch, n):
    s = _System(km, torch, n)
    try:
        bad = _fixed_counts(s, oracle, "n=%d" % n)
    finally:
        s.close()
    assert not bad, "\n".join(bad)


def test_unpreconditioned_instance(km, oracle, torch):
    s = _System(km, torch, 513)
    try:
        bad = _fixed_counts(s, oracle, "n=513 plain", precond=False)
    finally:
        s.close()
    assert not bad, "\n".join(bad)


def test_relative_stop_at_every_residue(km, oracle, torch):
    """The loop stops on r.z / b.b <= tol^2 after 4, 5, 6 and 7 iterations (0 ... B-1 mod B for B = 2, 3, 4): the loop
    head that sees the stop applies whatever is pending."""
    s = _System(km, torch, 513)
    try:
        bad = []
        hist = s.oracle(oracle, tol=1e-300, max_it=12, history=True)
        rz, bb = hist["rz_hist"], hist["bb"]
        assert hist["iterations"] == 12 and len(rz) >= 8
        seen = set()
        for stop in (4, 5, 6, 7):
            before = float(np.min(rz[:stop]))
            assert rz[stop] < before, (stop, rz[:stop + 1])               # (a tolerance between them exists)
            tol = float(np.sqrt(np.sqrt(rz[stop] * before) / bb))
            want = s.oracle(oracle, tol=tol, max_it=100)
            assert want["iterations"] == stop and want["converged"], (stop, want["iterations"])      # on the CPU first
            seen.add(stop)
            s.batch(1)
            base = s.solve(tol=tol, max_it=100)
            _same("stop=%d B=1 vs oracle" % stop, base, _orc3(want), bad)
            for B in BATCHES:
                s.batch(B)
                got = s.solve(tol=tol, max_it=100)
                _same("stop=%d B=%d vs oracle" % (stop, B), got, _orc3(want), bad)
                _same("stop=%d B=%d vs B=1" % (stop, B), got, base, bad)
        for B in BATCHES:
            assert {k % B for k in seen} == set(range(B))
    finally:
        s.close()
    assert not bad, "\n".join(bad)


def test_batched_then_unbatched_on_one_matrix(km, oracle, torch):
    """A batched solve moves the matrix's p through the ring; the next solve (B = 1) and kmcf_spmv must find the
    original buffer again."""
    s = _System(km, torch, 513)
    try:
        bad = []
        v = np.random.default_rng(5).standard_normal(s.n)
        y0 = s.apply(v)
        ref = oracle.spmv(s.M.indptr, s.M.indices, s.M.data, v)
        assert np.abs(y0 - ref).max() <= 1e-13 * (abs(s.M) @ np.abs(v)).max()
        want = _orc3(s.oracle(oracle, fixed=5))
        for B in (4, 1, 3, 1, 2, 1):
            s.batch(B)
            _same("B=%d k=5 in a row" % B, s.solve(fixed=5), want, bad, stopped=False)
            y = s.apply(v)
            if not np.array_equal(y, y0):
                bad.append("kmcf_spmv after a B=%d solve differs in %d rows" % (B, int((y != y0).sum())))
    finally:
        s.close()
    assert not bad, "\n".join(bad)


def test_workspace_loop_flushes_at_the_limit(km, oracle, torch):
    """kmcf_solve_sparse_CG_Jacobi: the loop on the workspace (no output kernel: cg_x_kernel applies what is pending at
    the limit), unpreconditioned, with the absolute stopping rule.  Diagonal 4: 1/sqrt(diag) = 0.5, so the scaling of
    A, b and the start guess is exact and the oracle can be given the scaled system as numbers."""
    S = km.solvers
    s = _System(km, torch, 513, diag=4.0)
    try:
        bad = []

        def run(max_it):
            s.mat.set_values(s.M.data)                               # (the solve scales A in place)
            rhs = torch.as_tensor(s.b.copy(), device="cuda")
            x = torch.as_tensor(s.x0.copy(), device="cuda")
            st = S.solve_sparse_CG_Jacobi(s.mat, rhs, x, 1e-14, max_it)
            return st, x.cpu().numpy(), None

        s.batch(1)
        run(1)
        plan = s.mat.sum_plan()                                      # the scaled values, the plan of the f64 kernel
        assert plan["sell_active"], plan
        assert np.array_equal(np.sort(np.unique(plan["val"])), np.array([-0.25, -0.125, -0.0625, 1.0]))
        base, want = {}, {}
        for k in FIXED + (5000,):
            o = oracle.pcg_device_order(plan, 0.5 * s.b, 2.0 * s.x0, None, 1e-14, k, check_mode=2)
            want[k] = (o, 0.5 * o["x"], None)
        assert want[5000][0]["converged"] and 9 < want[5000][0]["iterations"] < 5000
        for B in (1,) + BATCHES:
            s.batch(B)
            for k in FIXED + (5000,):
                got = run(k)
                _same("workspace B=%d max_it=%d vs oracle" % (B, k), got, want[k], bad, stopped=k == 5000)
                if B == 1:
                    base[k] = got
                else:
                    _same("workspace B=%d max_it=%d vs B=1" % (B, k), got, base[k], bad)
    finally:
        s.close()
    assert not bad, "\n".join(bad)


def test_k_and_cb_edge_solves_of_the_5nm_device(km, dev5, torch):
    """kmcf_pcg_workspace (K solve, relative rule) and kmcf_jacobi_cg_workspace_absolute (CB-edge solve, absolute
    rule) as loops of kernels: B = 2, 3, 4 against B = 1."""
    S = km.solvers
    d = dev5
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], rank=0, size=1, device=0,
                      options={"KMCF_CG_RESIDENT": "0", "KMCF_CG_VARIANT": "classic"})
    comm.connect()
    buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    guess = torch.as_tensor(0.25 * d["Vd"] * np.cos(np.arange(d["N"]) * 0.01), device="cuda")
    bad, base = [], {}
    try:
        for B in (1,) + BATCHES:
            comm.set_option("KMCF_CG_XBATCH", B)
            buf.site_potential_boundary.copy_(guess)
            st = S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                                   d["nn_dist"], len(d["metals"]), 0)
            k_run = (st, buf.site_potential_boundary.cpu().numpy(), None)
            buf.site_CB_edge = (0.5 * guess).clone()                 # (the CB-edge solve starts from the array's content)
            st = S.update_CB_edge_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                             len(d["metals"]))
            cb_run = (st, buf.site_CB_edge.cpu().numpy(), None)
            for name, run in (("K", k_run), ("CB", cb_run)):
                assert run[0]["converged"] == 1 and run[0]["iterations"] > 8, (name, run[0])
                if B == 1:
                    base[name] = run
                else:
                    _same("5 nm %s B=%d vs B=1" % (name, B), run, base[name], bad)
    finally:
        buf.freeGPUmemory()
        comm.close()
    assert not bad, "\n".join(bad)


def test_second_grid_stride_step_in_a_child_process():
    """n = 256 * 512 + 513 under KMCF_DEVICE_SHARE=8 (a process-wide knob, hence the child): the 256 blocks cover
    256 * 512 rows in their first step, block 0 takes a second one, block 1 a single pair, thread 0 the odd last row."""
    env = dict(os.environ, KMCF_DEVICE_SHARE=str(BIG_SHARE))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "big"], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "cg-xbatch big: ok" in out.stdout, out.stdout[-4000:]


def _big():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import torch
    import kmcfield_amd as km
    import kmcf_oracle as O
    assert torch.cuda.is_available() and os.environ.get("KMCF_DEVICE_SHARE") == str(BIG_SHARE)
    s = _System(km, torch, BIG_N)
    try:
        assert s.plan["vec_grid"] == 2048 // BIG_SHARE and BIG_N > 512 * s.plan["vec_grid"], s.plan["vec_grid"]
        bad = _fixed_counts(s, O, "n=%d" % BIG_N)
    finally:
        s.close()
    print("\n".join(bad) if bad else "cg-xbatch big: ok")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(_big() if sys.argv[1:] == ["big"] else 2)
