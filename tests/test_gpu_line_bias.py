"""GPU: per-line crossbar bias -- kmcf_k_assemble_contacts and kmcf_background_potential_sparse_contacts (one Dirichlet
value per contact site) on synth_crossbar_40nm(tiles=1) with every third contact-adjacent interface site rewritten to
oxygen (tests/line_bias_ref.py: crossbar_case), against the numpy restatement, the scalar entry points, every solver
path, in-process rank groups, the error contract and three supersteps of the KMC loop.

Bounds.  rhs: |rhs_i - ref_i| <= n_i 2^-52 S_i (order of addition and contraction only; tests/line_bias_ref.py).
Solve: sqrt(r . D^-1 r / b . b) of the TRUE residual, held to 10 x what the scalar entry point reaches on the same
device, element array and solver path (measured in the same test)."""
import threading

import numpy as np
import pytest

import line_bias_ref as R

pytestmark = pytest.mark.gpu

KMCF_ERR_ARG = -1
V_SELECT = 15.0
SELECT = (0, 1)


@pytest.fixture(scope="module")
def case(km):
    return R.crossbar_case()


def _comm(km, d, options=None):
    NL = d["N_contact"]
    comm = km.solvers.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], options=options)
    comm.connect()
    return comm


def _setup(km, d, comm):
    S = km.solvers
    buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], d["N_contact"], comm)
    S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                        buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
    return buf


def _fill(buf, v):
    import torch
    buf.site_potential_boundary.copy_(torch.as_tensor(v))
    torch.cuda.synchronize()


def _solve_contacts(km, buf, d, v):
    """whole array in (contact slots = boundary condition, interface = start guess), statistics and whole array out"""
    NL = d["N_contact"]
    _fill(buf, v)
    st = km.solvers.background_potential_gpu_sparse_contacts(buf, d["N"], NL, NL, d["high_G"], d["low_G"], len(d["metals"]))
    return st, buf.site_potential_boundary.cpu().numpy().copy()


def _solve_scalar(km, buf, d, Vd):
    NL = d["N_contact"]
    _fill(buf, np.zeros(d["N"]))
    st = km.solvers.background_potential_gpu_sparse(buf, d["N"], NL, NL, Vd, d["pbc"], d["high_G"], d["low_G"],
                                                    d["nn_dist"], len(d["metals"]))
    return st, buf.site_potential_boundary.cpu().numpy().copy()


def _uniform(d, Vd):
    NL = d["N_contact"]
    v = np.zeros(d["N"])
    v[:NL], v[d["N"] - NL:] = -Vd / 2, Vd / 2
    return v


def _ref_rhs(case, cls, V):
    d = case["d"]
    return R.contact_rhs(case["left_rp"], case["left_col"], case["right_rp"], case["right_col"], cls, d["N_contact"], V,
                         d["high_G"], d["low_G"])


@pytest.fixture(scope="module")
def one(km, case):
    """One rank, default options: the library's patterns and charges, the restatement's K, and the results the group
    tests compare with (rhs for random slots, potential of the half-select scheme and of the scalar call)."""
    S = km.solvers
    d = case["d"]
    NL, N = d["N_contact"], d["N"]
    comm = _comm(km, d)
    buf = _setup(km, d, comm)
    try:
        charge = buf.site_charge.cpu().numpy()
        cls = R.site_classes(d["element"], charge, d["metals"])
        rp, col = S.k_pattern(buf, 0)
        lrp, lcol = S.k_pattern(buf, 1)
        rrp, rcol = S.k_pattern(buf, 2)
        # the restatement's contact patterns (a KD tree on the host) are the library's
        assert np.array_equal(lrp, case["left_rp"]) and np.array_equal(lcol, case["left_col"])
        assert np.array_equal(rrp, case["right_rp"]) and np.array_equal(rcol, case["right_col"])
        K, diag = R.k_matrix(rp, col, lrp, lcol, rrp, rcol, cls, NL, d["high_G"], d["low_G"])
        v_rand = R.random_contact_values(d)
        import torch
        S.k_assemble_contacts(buf, torch.as_tensor(v_rand, device="cuda"), d["high_G"], d["low_G"])
        rhs_rand = S.k_vectors(buf)["rhs"].copy()
        v_half = km.structure.bias_scheme(d, "half", select=SELECT, V=V_SELECT)
        st_half, phi_half = _solve_contacts(km, buf, d, v_half)
        st_sc, phi_sc = _solve_scalar(km, buf, d, V_SELECT)
    finally:
        buf.freeGPUmemory()
        comm.close()
    return dict(cls=cls, K=K, diag=diag, v_rand=v_rand, rhs_rand=rhs_rand, v_half=v_half, phi_half=phi_half, phi_scalar=phi_sc,
                st_half=st_half, st_scalar=st_sc)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_rhs_parity_random_slots(km, case, one):
    """Check 1: every row of rhs against the restatement; rows without contact entries exactly 0.0; values, diagonal
    and 1/diag byte-identical to kmcf_k_assemble's."""
    import torch
    S = km.solvers
    d = case["d"]
    ref, n, Sabs = _ref_rhs(case, one["cls"], one["v_rand"])
    comm = _comm(km, d)
    buf = _setup(km, d, comm)
    try:
        V = torch.as_tensor(one["v_rand"], device="cuda")
        S.k_assemble_contacts(buf, V, d["high_G"], d["low_G"])
        got = S.k_vectors(buf)
        S.k_assemble_contacts(buf, V, d["high_G"], d["low_G"])
        again = S.k_vectors(buf)
        assert np.array_equal(V.cpu().numpy(), one["v_rand"])              # read, never written
        S.k_assemble(buf, d["Vd"], d["high_G"], d["low_G"])
        scalar = S.k_vectors(buf)
    finally:
        buf.freeGPUmemory()
        comm.close()
    rhs = got["rhs"]
    assert rhs.shape == ref.shape == (d["N"] - 2 * d["N_contact"],)
    err = np.abs(rhs - ref)
    bound = n * R.EPS * Sabs
    print("rhs: %d rows with entries, max |rhs - ref| / bound = %.3f, max |rhs| = %.3f" % (
        np.count_nonzero(n), (err[n > 0] / bound[n > 0]).max(), np.abs(rhs).max()))
    assert np.count_nonzero(n) == 672 and np.count_nonzero(ref) > 600
    assert np.all(err <= bound)
    assert np.all(_bits(rhs[n == 0]) == 0)                                  # exactly +0.0
    for key in ("val", "diag", "dinv", "left", "right"):
        assert np.array_equal(_bits(got[key]), _bits(scalar[key])), key
    for key in ("val", "diag", "dinv", "rhs"):
        assert np.array_equal(_bits(got[key]), _bits(again[key])), key       # two calls, the same bytes
    assert np.array_equal(_bits(rhs), _bits(one["rhs_rand"]))               # ... also from another state of the same device


def test_uniform_slots_reduce_to_the_scalar_call(km, case, one):
    """Check 2."""
    import torch
    S = km.solvers
    d = case["d"]
    NL, Vd = d["N_contact"], d["Vd"]
    v = _uniform(d, Vd)
    _, n, Sabs = _ref_rhs(case, one["cls"], v)
    comm = _comm(km, d)
    buf = _setup(km, d, comm)
    try:
        S.k_assemble(buf, Vd, d["high_G"], d["low_G"])
        scalar = S.k_vectors(buf)["rhs"].copy()
        S.k_assemble_contacts(buf, torch.as_tensor(v, device="cuda"), d["high_G"], d["low_G"])
        new = S.k_vectors(buf)["rhs"].copy()
        st, phi = _solve_contacts(km, buf, d, v)
        st_s, phi_s = _solve_scalar(km, buf, d, Vd)
    finally:
        buf.freeGPUmemory()
        comm.close()
    bound = n * R.EPS * Sabs
    err = np.abs(new - scalar)
    print("uniform slots: max |rhs - scalar rhs| / bound = %.3f; iterations %d (scalar %d); max |phi - scalar phi| = %.2e" % (
        (err[n > 0] / bound[n > 0]).max(), st["iterations"], st_s["iterations"], np.abs(phi[NL:-NL] - phi_s[NL:-NL]).max()))
    assert np.all(err <= bound) and np.all(new[n == 0] == 0.0) and np.all(scalar[n == 0] == 0.0)
    assert np.array_equal(_bits(phi[:NL]), _bits(v[:NL])) and np.array_equal(_bits(phi[-NL:]), _bits(v[-NL:]))
    assert st["converged"] == 1 and st_s["converged"] == 1


def _check_solve(case, one, v, phi, bar):
    """Check 3 for one solution: residual of the restatement's system and the maximum principle."""
    d = case["d"]
    NL = d["N_contact"]
    b, _, _ = _ref_rhs(case, one["cls"], v)
    res = R.scaled_residual(one["K"], one["diag"], b, phi[NL:-NL])
    contacts = np.concatenate([v[:NL], v[-NL:]])
    e = bar * np.abs(contacts).max()
    lo, hi = phi[NL:-NL].min(), phi[NL:-NL].max()
    return res, (lo >= contacts.min() - e and hi <= contacts.max() + e), (lo, hi, e)


PATHS = [("1", "classic"), ("1", "cg1r"), ("0", "classic"), ("0", "cg1r")]


@pytest.mark.parametrize("resident, variant", PATHS)
def test_solve_solves_its_system_on_every_path(km, case, one, resident, variant):
    """Checks 3 and 4: scheme "half", select (0, 1), V = 15 on the resident launch and the kernel loop, both
    recurrences.  The bar is 10 x the scalar entry point's value on the same path.

    Measured (MI355X), new / scalar: resident classic 2.22e-10 / 2.30e-10, resident cg1r 2.49e-10 / 1.99e-10, loop classic
    2.47e-10 / 2.02e-10, loop cg1r 2.46e-10 / 2.03e-10."""
    S = km.solvers
    d = case["d"]
    NL = d["N_contact"]
    v = one["v_half"]
    comm = _comm(km, d, options={"KMCF_CG_RESIDENT": resident, "KMCF_CG_VARIANT": variant})
    buf = _setup(km, d, comm)
    try:
        mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))
        st_s, phi_s = _solve_scalar(km, buf, d, V_SELECT)
        tpb = mat.sum_plan(with_csr=False)["resident_tpb"]
        st, phi = _solve_contacts(km, buf, d, v)
        st2, phi2 = _solve_contacts(km, buf, d, v)
    finally:
        buf.freeGPUmemory()
        comm.close()
    assert (tpb > 0) == (resident == "1"), tpb
    res_s, _, _ = _check_solve(case, one, _uniform(d, V_SELECT), phi_s, 0.0)
    bar = 10 * res_s
    res, inside, (lo, hi, e) = _check_solve(case, one, v, phi, bar)
    print("resident %s, %s: true scaled residual %.3e (scalar call %.3e, bar %.3e), %d iterations (scalar %d), "
          "phi in [%.9f, %.9f], e = %.2e" % (resident, variant, res, res_s, bar, st["iterations"], st_s["iterations"], lo, hi, e))
    assert st["converged"] == 1 and st_s["converged"] == 1
    assert res <= bar
    assert inside, (lo, hi, e)
    assert np.array_equal(_bits(phi[:NL]), _bits(v[:NL])) and np.array_equal(_bits(phi[-NL:]), _bits(v[-NL:]))
    assert np.array_equal(_bits(phi), _bits(phi2)) and st["iterations"] == st2["iterations"] and st["rz"] == st2["rz"]


# ---------------------------------------------------------------------------------------------- rank groups

def _transport(monkeypatch, name):
    """Connect-scope knobs of an in-process group come from the environment (it is connected at creation)."""
    if name == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")               # bound of every device-side wait
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)


def _group(km, d, P, fn, resident, seconds=240):
    import torch
    S = km.solvers
    NL = d["N_contact"]
    comms = S.KMC_comm.loopback_group(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"], size=P, device=0,
                                      options={"KMCF_CG_RESIDENT": resident, "KMCF_CGR_TIMEOUT_MS": "20000"})
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
    try:
        for t in threads:
            t.start()
        for t in threads:
            t.join(seconds)
        assert not errs, "\n".join(errs)
        assert all(o is not None for o in out), "a rank did not finish (deadlock?)"
    finally:
        for c in comms:
            c.close()
    return out


@pytest.mark.parametrize("P", [2, 3])
def test_rank_groups(km, case, one, monkeypatch, P):
    """Check 5.  The solve leaves every rank's own rows in its array, like the scalar call; the complete array on every
    rank is what kmcf_sum_and_gather_potential, the next stage of a step, makes of it -- for both entry points.
    The two transports are compared on the solver path they share, the loop of kernels (KMCF_CG_RESIDENT=0, as
    tests/test_gpu_multirank.py compares them: a group's resident launch exists on the peer-to-peer transport only and
    adds in another order); that launch is the third run."""
    import torch
    S = km.solvers
    d = case["d"]
    NL, N = d["N_contact"], d["N"]

    def fn(comm):
        buf = _setup(km, d, comm)
        try:
            S.k_assemble_contacts(buf, torch.as_tensor(one["v_rand"], device="cuda"), d["high_G"], d["low_G"])
            rhs = S.k_vectors(buf)["rhs"].copy()
            full = {}
            for name in ("half", "scalar"):
                if name == "half":
                    st, _ = _solve_contacts(km, buf, d, one["v_half"])
                else:
                    st, _ = _solve_scalar(km, buf, d, V_SELECT)
                buf.site_potential_charge.zero_()
                torch.cuda.synchronize()
                S.sum_and_gather_potential(buf, NL, comm)
                full[name] = (st, buf.site_potential_boundary.cpu().numpy().copy())
            mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))
            return dict(rhs=rhs, row0=int(comm.displs_K[comm.rank_K]), rows=int(comm.counts_K[comm.rank_K]),
                        tpb=mat.sum_plan(with_csr=False)["resident_tpb"], **full)
        finally:
            buf.freeGPUmemory()

    runs = {}
    for transport, resident in (("loopback", "0"), ("p2p", "0"), ("p2p", "1")):
        _transport(monkeypatch, transport)
        runs[transport, resident] = out = _group(km, d, P, fn, resident)
        dev = {}
        for name, want in (("half", one["phi_half"]), ("scalar", one["phi_scalar"])):
            dev[name] = max(float(np.abs(o[name][1][NL:-NL] - want[NL:-NL]).max()) for o in out)
        # the scalar call's slots are not the caller's: the comparison is over the interface
        print("P = %d, %s, resident %s: max |phi - one rank| new %.3e, scalar %.3e; iterations new %d (one rank %d), scalar %d (one rank %d)" % (
            P, transport, resident, dev["half"], dev["scalar"], out[0]["half"][0]["iterations"], one["st_half"]["iterations"],
            out[0]["scalar"][0]["iterations"], one["st_scalar"]["iterations"]))
        assert sum(o["rows"] for o in out) == N - 2 * NL
        for o in out:
            assert (o["tpb"] > 0) == (resident == "1"), (transport, resident, o["tpb"])      # the path that was asked for ran
            r0, nr = o["row0"], o["rows"]
            assert np.array_equal(_bits(o["rhs"]), _bits(one["rhs_rand"][r0:r0 + nr]))       # byte-identical per row
            st, phi = o["half"]
            assert st["converged"] == 1 and phi.shape == (N,)
            assert np.array_equal(_bits(phi), _bits(out[0]["half"][1]))                      # every rank: the complete array
            assert np.array_equal(_bits(phi[:NL]), _bits(one["v_half"][:NL])) and np.array_equal(_bits(phi[-NL:]), _bits(one["v_half"][-NL:]))
        assert dev["scalar"] > 0.0
        assert dev["half"] <= 10 * dev["scalar"]
    for a, b in zip(runs["loopback", "0"], runs["p2p", "0"]):
        assert np.array_equal(_bits(a["rhs"]), _bits(b["rhs"]))
        assert np.array_equal(_bits(a["half"][1]), _bits(b["half"][1]))                      # bit for bit between the transports
        assert a["half"][0]["iterations"] == b["half"][0]["iterations"] and a["half"][0]["rz"] == b["half"][0]["rz"]


# ---------------------------------------------------------------------------------------------- errors

def test_errors_name_the_argument_or_the_site(km, case, one):
    """Check 6."""
    import torch
    S = km.solvers
    d = case["d"]
    NL, N = d["N_contact"], d["N"]
    comm = _comm(km, d)
    buf = _setup(km, d, comm)
    args = (d["high_G"], d["low_G"], len(d["metals"]))

    def refused(f, *words):
        with pytest.raises(km.lib.KmcfError) as e:
            f()
        msg = str(e.value)
        assert "(%d)" % KMCF_ERR_ARG in msg, msg
        for w in words:
            assert w in msg, msg

    try:
        refused(lambda: S.k_assemble_contacts(buf, None, d["high_G"], d["low_G"]), "kmcf_k_assemble_contacts", "d_site_potential")
        keep = buf.site_potential_boundary
        buf.site_potential_boundary = None
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, *args), "d_site_potential_boundary")
        buf.site_potential_boundary = keep
        keep = buf.site_element
        buf.site_element = None
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, *args), "d_site_element")
        buf.site_element = keep
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N - 1, NL, NL, *args), "N/N_left_tot/N_right_tot", str(N - 1))
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL + 1, NL, *args), "N/N_left_tot/N_right_tot")
        # NaN in one left slot, inf in one right slot: the smaller site id is named, the slots stay as they are
        v = one["v_half"].copy()
        v[5], v[N - NL + 7] = np.nan, np.inf
        _fill(buf, v)
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, *args), "site 5 ", "not finite")
        after = buf.site_potential_boundary.cpu().numpy()
        assert np.array_equal(_bits(after[:NL]), _bits(v[:NL])) and np.array_equal(_bits(after[-NL:]), _bits(v[-NL:]))
        refused(lambda: S.k_assemble_contacts(buf, buf.site_potential_boundary, d["high_G"], d["low_G"]), "site 5 ")
        v[5] = 0.0                                               # ... and now the right slot alone
        _fill(buf, v)
        refused(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, *args), "site %d " % (N - NL + 7), "right contact slot 7")
        # afterwards a valid call succeeds, with the result of a state that never saw the bad values
        st, phi = _solve_contacts(km, buf, d, one["v_half"])
        assert st["converged"] == 1
        assert np.array_equal(_bits(phi), _bits(one["phi_half"]))
    finally:
        buf.freeGPUmemory()
        comm.close()


# ---------------------------------------------------------------------------------------------- loop

def _loop(km, d, steps, contacts, T=300.0):
    """charge -> K solve -> pairwise -> gather -> events, `steps` times.  contacts: N-vector whose contact slots drive
    the new call, or None for the scalar call at d["Vd"]."""
    import torch
    S = km.solvers
    NL, N = d["N_contact"], d["N"]
    comm = _comm(km, d)
    buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"], d["lattice"], d["metals"])
    try:
        S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
        S.compute_cutoff_list(comm, buf, 20.0)
        S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
        layers = km.structure.LAYERS
        xs = np.clip(d["xyz"][:, 0], layers[0]["start_x"], layers[-1]["end_x"])
        lay = torch.as_tensor(S.site_layers(xs, layers), device="cuda")
        rng = S.RandomNumberGenerator(km.structure.RND_SEED_KMC)
        if contacts is not None:
            _fill(buf, contacts)
        logs, times = [], []
        for _ in range(steps):
            S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                                buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
            if contacts is None:
                st = S.background_potential_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                                       len(d["metals"]))
            else:
                st = S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, d["high_G"], d["low_G"], len(d["metals"]))
            assert st["converged"] == 1
            S.poisson_gridless_gpu(buf, comm)
            S.sum_and_gather_potential(buf, NL, comm)
            t, nev, log = S.execute_kmc_step_mpi(comm, N, comm.counts_events, comm.displs_events, 52, buf.neigh_idx, lay, T, 10e13,
                                                 d["sigma"], d["k"], buf.site_x, buf.site_y, buf.site_z, buf.site_potential_charge,
                                                 buf.site_element, buf.site_charge, rng, layers, max_events=100000, return_log=True)
            assert nev == len(log)
            logs.append(log)
            times.append(t)
        slots = buf.site_potential_boundary.cpu().numpy()
        return logs, np.array(times), np.concatenate([slots[:NL], slots[-NL:]])
    finally:
        buf.freeGPUmemory()
        comm.close()


def test_three_supersteps(km, case):
    """Check 7, on the device as carved (the oxygen rewrite is for the conductance classes of the other tests)."""
    d = km.structure.synth_crossbar_40nm(tiles=1)
    NL, N = d["N_contact"], d["N"]
    v = km.structure.bias_scheme(d, "third", select=SELECT, V=V_SELECT)
    logs, times, slots = _loop(km, d, 3, v)
    _, _, cell = km.structure.crossbar_lines(d)
    n_events = [len(l) for l in logs]
    per_cell = [np.bincount(cell[l[:, 0]][cell[l[:, 0]] >= 0], minlength=4).tolist() for l in logs]
    print("scheme third: events per step %s, per cell %s, KMC times %s" % (n_events, per_cell, times))
    assert min(n_events) > 0 and np.all(times > 0)
    for log in logs:
        assert log.shape[1] == 3 and np.all((log[:, :2] >= 0) & (log[:, :2] < N))
    assert np.array_equal(_bits(slots), _bits(np.concatenate([v[:NL], v[-NL:]])))       # three solves later
    # scheme "all" through the new call is the scalar call: the same events under the same seed
    d15 = dict(d, Vd=V_SELECT)
    logs_a, times_a, _ = _loop(km, d15, 3, km.structure.bias_scheme(d15, "all", V=V_SELECT))
    logs_s, times_s, _ = _loop(km, d15, 3, None)
    print("scheme all against the scalar call: events %s / %s, max relative KMC time difference %.2e" % (
        [len(l) for l in logs_a], [len(l) for l in logs_s], np.abs(times_a / times_s - 1).max()))
    for a, s in zip(logs_a, logs_s):
        assert np.array_equal(a, s)
    np.testing.assert_allclose(times_a, times_s, rtol=1e-9)
