"""GPU: the T path (csrc/kmcf_tstate.hip) on the synthetic devices of tests/tpath_ref.py -- tunnel blocks of 0, 1, 2, 63,
64, 65, 128, 129 and 178 points, conduction-band edges ON tol and ON q V0, distances ON nn_dist, atoms ON the contact
window and ON the index bounds of the contact rule, both signs of the bias -- against the plain dense reference of that
file (numpy, longdouble sums; tests/test_tpath_ref.py holds it and the oracle to each other), in the three storage forms
of the block (KMCF_SUB_DENSE = 0 bitmap + packed values, 1 dense symmetric tiles, 2 jagged tiles) and dealt over a group.

Bars: those of tests/test_gpu_tpath.py (its docstring), none wider: integer work identical; neighbour off-diagonals
identical, diagonals rtol 1e-13; WKB values and tunnel diagonal rtol 1e-10 with exact zeros exact; SpMV
|dy_i| <= 1e-12 (|M| |x|)_i; I_macro 1e-11 of its absolute terms; power 1e-11 of its maximum; potentials after scale and
shift rtol 1e-15; converged solves identical to the oracle adding in the device's order, true residual (dense
longdouble M) <= 3 x the natural-order oracle's.

Every compared assembly is the SECOND on its state: the first runs on another band edge and charge vector
(tpath_ref.other_state), so that grown buffers hold another pattern's masks and values.  Every form gets a fresh device
-- except in (a'), where ONE state (one rank; one per rank of a group) goes through the forms in turn and must give a
fresh state's values bit for bit."""
import contextlib
import threading

import numpy as np
import pytest

import tpath_ref as R
from test_gpu_tpath import G0, _compare_assembly, _device_order_solve, _device_rank, _make
from test_oracle_T import N_EL, TI
from test_tpath_ref import _oracle_T

pytestmark = pytest.mark.gpu

STORAGE = {"bitmap": 0, "tiles": 1, "jagged": 2}
SOLVE_TOL = 1e-20


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _args(case, Vd):
    p = case["par"]
    return (case["n1"], case["n1"], case["layers"], Vd, p["high_G"], p["low_G"], p["loop_G"], G0, p["tol"], p["nn_dist"], p["m_e"], p["V0"], 2)


def _prm(S, case, Vd):
    p = case["par"]
    return S.current_params(Vd, p["high_G"], p["low_G"], p["loop_G"], G0, p["tol"], p["m_e"], p["V0"], contact_x_lo=case["x_lo"],
                            contact_x_hi=case["x_hi"])


def _first_assembly_then_state(S, torch, buf, case, Vd):
    """A first assembly on another state; then the case's own charge and band edge are put in place (not yet assembled).
    The first one runs with the contact window wide open: every contact atom is a tunnel point then, so the point arrays
    hold valid points BEHIND the n_t of the assembly that is compared (a read one past the last point finds a partner)."""
    charge, cb = R.other_state(case)
    buf.site_charge.copy_(torch.as_tensor(charge))
    buf.site_CB_edge = torch.as_tensor(cb, device="cuda")
    wide = dict(case, x_lo=-1e9, x_hi=1e9)
    S.t_assemble(buf, _prm(S, wide, Vd))
    assert S.t_info(buf)["tunnel_points"] > R.case_ref(case["name"]).n_t
    buf.site_charge.copy_(torch.as_tensor(np.array(case["charge"], np.int32)))
    buf.site_CB_edge = torch.as_tensor(np.array(case["cb"], np.float64), device="cuda")


@contextlib.contextmanager
def _device(km, torch, name, Vd=None, comm=None):
    """One communicator (unless given) and one set of buffers for a case, freed on the way out; the case's state in place
    behind a first assembly on another one.  Yields (S, buf, ref, kw): ref the dense reference at this bias."""
    S = km.solvers
    case = R.tpath_case(name)
    Vd = case["par"]["Vd"] if Vd is None else Vd
    ref = R.case_ref(name, Vd)
    own = comm is None
    if own:
        N = len(case["element"])
        comm = S.KMC_comm(ref.Nsub, ref.Nsub, N, N)
        comm.connect()
    buf = None
    try:
        buf = _make(km, torch, case["xyz"].copy(), case["element"].copy(), case["charge"], case["cb"], case["metals"].copy(), case["n1"], case["layers"], comm,
                    nn_dist=case["par"]["nn_dist"])
        assert buf.N_atom_ == ref.N_atom
        _first_assembly_then_state(S, torch, buf, case, Vd)
        yield S, buf, ref, dict(contact_x_lo=case["x_lo"], contact_x_hi=case["x_hi"])
    finally:
        if buf is not None:
            buf.freeGPUmemory()
        if own:
            comm.close()


def _m_of(ref, x0):
    m = np.zeros(ref.N_atom + 2)
    m[:ref.Nsub] = x0 * G0
    return m


# ------------------------------------------------------------------------------------------------ (a) assembly
@pytest.mark.parametrize("name,strip", [(n, None) for n in R.CASES] + [("nt_128", 2), ("nt_129", 2)])
def test_assembly_one_rank(km, torch, monkeypatch, name, strip):
    """kmcf_initialize_sparsity_T + kmcf_t_assemble against the dense reference, in each storage form; the forms against
    each other.  strip = 2 (KMCF_SUB_STRIP): ragged strips of tiles, block row 0 of three block rows: a strip of 2 and of 1."""
    case = R.tpath_case(name)
    if strip:
        monkeypatch.setenv("KMCF_SUB_STRIP", str(strip))
    res = {}
    for form, dense in STORAGE.items():
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        with _device(km, torch, name) as (S, buf, ref, kw):
            np.testing.assert_array_equal(S.t_atom_sites(buf), ref.atom_site)
            S.t_assemble(buf, _prm(S, case, case["par"]["Vd"]))
            tn = _compare_assembly(S, buf, ref.as_csr())
            info = S.t_info(buf)
            assert info["tunnel_points"] == ref.n_t and info["nnz_tunnel"] == int(ref.S_pattern.sum()), (form, info)
            assert info["tunnel_dense"] == (dense if ref.n_t > 0 else 0), (form, info)
            # exact zeros of the block (E2 == 0: in the pattern, value +-0.0) are exact zeros here
            np.testing.assert_array_equal(tn["val"] == 0, ref.tunnel_csr()[2] == 0)
            res[form] = dict(tn=tn, dinv=S.t_vectors(buf)["dinv"])
            if ref.n_t == 0:                                       # the empty block: assembly done, and the solve behind it runs
                buf.atom_virtual_potentials.zero_()
                im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, case["par"]["Vd"]), True, False, 1.0, cg_tolerance=1e-13,
                                                        cg_max_iterations=20000, **kw)
                assert st["converged"] == 1 and np.isfinite(im)           # (a current through low_G alone: its sign is rounding)
                assert np.all(np.isfinite(buf.atom_virtual_potentials.cpu().numpy()))
    a, b, c = res["bitmap"], res["tiles"], res["jagged"]
    for key in ("row_ptr", "col"):
        np.testing.assert_array_equal(a["tn"][key], b["tn"][key])
    rows_of = np.repeat(np.arange(len(a["tn"]["row_ptr"]) - 1) + a["tn"]["first"], np.diff(a["tn"]["row_ptr"]))
    off = a["tn"]["col"] != rows_of
    np.testing.assert_array_equal(a["tn"]["val"][off], b["tn"]["val"][off])                  # the same WKB values, bit for bit
    np.testing.assert_allclose(b["tn"]["val"][~off], a["tn"]["val"][~off], rtol=1e-12, atol=0)      # -(row sums): another order
    np.testing.assert_allclose(b["tn"]["diag"], a["tn"]["diag"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(b["dinv"], a["dinv"], rtol=1e-12, atol=0)
    for key in ("val", "diag", "row_ptr", "col"):                                                # jagged: the dense tiles' entries, same order
        np.testing.assert_array_equal(c["tn"][key], b["tn"][key])
    np.testing.assert_array_equal(c["dinv"], b["dinv"])


# ------------------------------------------------------------------------------------------------ (a') one state, form after form
def _assembled(S, buf, want, form, r0=0, nr=None):
    """The file's comparison of one assembly + what must be bit-identical between a fresh and a reused state."""
    tn = _compare_assembly(S, buf, want, r0, nr)
    info = S.t_info(buf)
    assert info["tunnel_dense"] == STORAGE[form], (form, info)
    return dict(val=tn["val"].copy(), diag=tn["diag"].copy(), dinv=S.t_vectors(buf)["dinv"].copy(), bytes=info["tunnel_bytes"])


def _same_as_fresh(got, fresh, what):
    for key in ("val", "diag", "dinv"):
        np.testing.assert_array_equal(got[key], fresh[key], err_msg="%s: %s differs from a fresh state's" % (what, key))
    assert got["bytes"] == fresh["bytes"], (what, got["bytes"], fresh["bytes"])


@pytest.mark.parametrize("name,strip", [("nt_129", 2), ("group_178", None)])
def test_one_state_through_the_storage_forms(km, torch, monkeypatch, name, strip):
    """ONE T state assembled as bitmap -> tiles -> jagged -> bitmap -> tiles (every other test gives each form a fresh
    device): after each assembly the comparison with the dense reference, the form reported, and tunnel values, tunnel
    diagonal and preconditioner bit-identical to a fresh state's in that form -- a flag, grid or pointer left behind by
    the form before would show.  Then one split SpMV (test_split_spmv's bound) and the power pass on prescribed
    potentials (test_current_and_power_on_prescribed_potentials' bars) on the state as the sequence left it."""
    case = R.tpath_case(name)
    Vd = case["par"]["Vd"]
    if strip:
        monkeypatch.setenv("KMCF_SUB_STRIP", str(strip))
    fresh = {}
    for form, dense in STORAGE.items():
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        with _device(km, torch, name) as (S, buf, ref, kw):
            S.t_assemble(buf, _prm(S, case, Vd))
            fresh[form] = _assembled(S, buf, ref.as_csr(), form)
    with _device(km, torch, name) as (S, buf, ref, kw):
        want = ref.as_csr()
        for k, form in enumerate(("bitmap", "tiles", "jagged", "bitmap", "tiles")):
            monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[form]))
            S.t_assemble(buf, _prm(S, case, Vd))
            _same_as_fresh(_assembled(S, buf, want, form), fresh[form], "assembly %d (%s)" % (k, form))
        # the split SpMV on the state as it stands (tiles)
        mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
        rng = np.random.default_rng(5)
        x = rng.standard_normal(ref.Nsub) + 3.0 * rng.random(ref.Nsub)
        p = torch.as_tensor(x, device="cuda")
        Ap = torch.empty_like(p)
        mat.spmv(p, Ap)
        err = np.abs(Ap.cpu().numpy() - ref.M @ x.astype(R.LD))
        bound = np.abs(ref.M) @ np.abs(x).astype(R.LD)
        assert np.all(err <= 1e-12 * bound), (int(np.argmax(err / bound)), float((err / bound).max()))
        # the power pass on prescribed potentials (0 iterations; it assembles once more, as tiles)
        x0 = R.potentials(ref, Vd)
        m = _m_of(ref, x0)
        buf.atom_virtual_potentials.zero_()
        buf.atom_virtual_potentials[:ref.Nsub] = torch.as_tensor(x0, device="cuda")
        buf.site_power.fill_(-7.0)
        im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), True, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=0, **kw)
        assert st["iterations"] == 0 and S.t_info(buf)["tunnel_dense"] == 1
        assert abs(im - ref.imacro(m)) <= 1e-11 * ref.imacro_scale(m), (im, ref.imacro(m))
        pw, ms = ref.power(m, Vd, 1.0)
        gp = buf.site_power.cpu().numpy()
        np.testing.assert_allclose(buf.atom_virtual_potentials.cpu().numpy(), ms, rtol=1e-15, atol=0)
        np.testing.assert_array_equal(gp == -7.0, pw == -7.0)
        w = pw != -7.0
        assert np.abs(gp - pw)[w].max() <= 1e-11 * np.abs(pw[w]).max(), float(np.abs(gp - pw)[w].max() / np.abs(pw[w]).max())
        assert (gp[w] != 0).any() and np.all(gp[w] >= 0)


def _group_through(km, torch, monkeypatch, name, P, forms):
    """One state per rank of a loopback group of P, assembled in each of `forms` in turn (the knob changes while all
    ranks wait at a barrier); per rank and assembly what _assembled returns."""
    S = km.solvers
    case = R.tpath_case(name)
    Vd = case["par"]["Vd"]
    ref = R.case_ref(name, Vd)
    want = ref.as_csr()
    N = len(case["element"])
    step = [0]

    def next_form():
        monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[forms[step[0]]]))
        step[0] += 1

    next_form()
    comms = S.KMC_comm.loopback_group(ref.Nsub, ref.Nsub, N, N, P)
    gate = threading.Barrier(P, action=next_form, timeout=120)
    out, errs = [[] for _ in range(P)], []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            with _device(km, torch, name, Vd, comm=comm) as (S_, buf, ref_, kw):
                r0, nr = int(comm.displs_T[r]), int(comm.counts_T[r])
                for k, form in enumerate(forms):
                    if k:
                        gate.wait()
                    S.t_assemble(buf, _prm(S, case, Vd))
                    out[r].append(_assembled(S, buf, want, form, r0, nr))
        except Exception as e:  # pragma: no cover
            import traceback
            gate.abort()
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(180)
    assert not errs, "\n".join(errs)
    assert all(len(o) == len(forms) for o in out), "a rank did not finish"
    for c in comms:
        c.close()
    return out


def test_group_states_through_the_storage_forms(km, torch, monkeypatch):
    """group_178 over three in-process ranks (loopback), strips of two tiles: one state per rank through tiles -> bitmap ->
    tiles, every assembly compared as in test_one_state_through_the_storage_forms, against fresh groups in each form."""
    monkeypatch.setenv("KMCF_SUB_STRIP", "2")
    monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    P, name = 3, "group_178"
    fresh = {form: _group_through(km, torch, monkeypatch, name, P, (form,)) for form in ("tiles", "bitmap")}
    assert sum(o[0]["bytes"] for o in fresh["tiles"]) == 6 * 32768                # really dealt: six tiles in all
    seq = ("tiles", "bitmap", "tiles")
    got = _group_through(km, torch, monkeypatch, name, P, seq)
    for r in range(P):
        for k, form in enumerate(seq):
            _same_as_fresh(got[r][k], fresh[form][r][0], "rank %d, assembly %d (%s)" % (r, k, form))


# ------------------------------------------------------------------------------------------------ (b) split SpMV
@pytest.mark.parametrize("form", list(STORAGE))
@pytest.mark.parametrize("name", R.CASES)
def test_split_spmv(km, torch, monkeypatch, name, form):
    """y = A_n x + P^T S P x through the generic SpMV entry against the dense longdouble M.  Two products in a row on
    vectors without structure: the sub-vector's pad behind the last point (64 nb - n_t positions, and the 4-word
    unroll's reach behind that) holds what the diagonal pass or the first product left there, and the second product
    meets it with other numbers -- a read behind the last point cannot cancel."""
    monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[form]))
    case = R.tpath_case(name)
    with _device(km, torch, name) as (S, buf, ref, kw):
        S.t_assemble(buf, _prm(S, case, case["par"]["Vd"]))
        mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
        rng = np.random.default_rng(5)
        absM = np.abs(ref.M)
        for scale in (1.0, 1e3):
            x = scale * (rng.standard_normal(ref.Nsub) + 3.0 * rng.random(ref.Nsub))
            p = torch.as_tensor(x, device="cuda")
            Ap = torch.empty_like(p)
            mat.spmv(p, Ap)
            got = Ap.cpu().numpy()
            want = ref.M @ x.astype(R.LD)
            bound = absM @ np.abs(x).astype(R.LD)
            err = np.abs(got - want)
            assert np.all(err <= 1e-12 * bound), (form, scale, int(np.argmax(err / bound)), float((err / bound).max()))


# ------------------------------------------------------------------------------------------------ (c) current and power
@pytest.mark.parametrize("form", list(STORAGE))
@pytest.mark.parametrize("Vd", [2.0, -2.0])
@pytest.mark.parametrize("name", ["group_178", "window_edges", "energy_edges"])
def test_current_and_power_on_prescribed_potentials(km, torch, monkeypatch, name, Vd, form):
    """0 CG iterations leave the start vector untouched: I_macro and the dissipated power of a prescribed field, under
    forward and REVERSE bias (the second branch of ineg, the signs of the right-hand side and of the current)."""
    monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[form]))
    case = R.tpath_case(name)
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        x0 = R.potentials(ref, Vd)
        m = _m_of(ref, x0)
        want_im = ref.imacro(m)
        for heating in (False, True):
            buf.atom_virtual_potentials.zero_()
            buf.atom_virtual_potentials[:ref.Nsub] = torch.as_tensor(x0, device="cuda")
            buf.site_power.fill_(-7.0)
            im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), heating, False, 1.0, cg_tolerance=1e-30, cg_max_iterations=0, **kw)
            assert st["iterations"] == 0
            np.testing.assert_array_equal(S.t_vectors(buf)["rhs"], ref.rhs)
            assert abs(im - want_im) <= 1e-11 * ref.imacro_scale(m), (im, want_im)
            assert (im < 0) == (Vd < 0) and (want_im < 0) == (Vd < 0), (im, want_im)
            got = buf.atom_virtual_potentials.cpu().numpy()
            gp = buf.site_power.cpu().numpy()
            if not heating:
                np.testing.assert_array_equal(got, m)
                assert np.all(gp == -7.0)
            else:
                pw, ms = ref.power(m, Vd, 1.0)
                np.testing.assert_allclose(got, ms, rtol=1e-15, atol=0)
                np.testing.assert_array_equal(gp == -7.0, pw == -7.0)
                w = pw != -7.0
                assert np.abs(gp - pw)[w].max() <= 1e-11 * np.abs(pw[w]).max(), float(np.abs(gp - pw)[w].max() / np.abs(pw[w]).max())
                assert (gp[w] != 0).any() and np.all(gp[w] >= 0)


@pytest.mark.parametrize("form", list(STORAGE))
def test_zero_bias(km, torch, monkeypatch, form):
    """Vd = 0 from a zero start (as tests/test_gpu_edge_cases.py::test_zero_rhs_and_converged_start for the K path):
    potentials exactly 0.0, I_macro 0.0, written power 0.0, nothing non-finite."""
    monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[form]))
    case = R.tpath_case("nt_65")
    with _device(km, torch, "nt_65", 0.0) as (S, buf, ref, kw):
        buf.atom_virtual_potentials.zero_()
        buf.site_power.fill_(-7.0)
        im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, 0.0), True, False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000, **kw)
        got = buf.atom_virtual_potentials.cpu().numpy()
        gp = buf.site_power.cpu().numpy()
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(gp)) and np.isfinite(im)
        assert np.all(got == 0.0) and im == 0.0
        pw, _ = ref.power(np.zeros(ref.N_atom + 2), 0.0, 1.0)
        np.testing.assert_array_equal(gp == -7.0, pw == -7.0)
        assert np.all(gp[gp != -7.0] == 0.0)
        assert st["iterations"] == 0                              # (b = 0: r.z / b.b is NaN, the loop never runs)


# ------------------------------------------------------------------------------------------------ (d) converged solve
@pytest.mark.parametrize("form", list(STORAGE))
@pytest.mark.parametrize("Vd", [2.0, -2.0])
@pytest.mark.parametrize("name", ["nt_64", "nt_65", "nt_129", "group_178"])
def test_converged_solve_one_rank(km, oracle, torch, monkeypatch, name, Vd, form):
    """The solve to SOLVE_TOL = 1e-20: identical to the oracle adding in the device's order, and -- apart from the oracle's
    orders -- a true residual on the dense longdouble M of at most 3 x the natural-order oracle's.
    Why 1e-20: on these systems the true residual follows the recurrence down to sqrt(r.z / b.b) ~ 2e-19 (|r|_2 ~ 1e-8 at
    |b|_2 = 2.8e7) and stays there, in every case and under both signs (the natural-order oracle: 2.3e-19 ... 2.8e-19 at
    1e-19 and at 1e-20).  Above that floor the residual at the stop is whatever the LAST iteration left, and one iteration
    takes a factor 2 ... 8 here: two summation orders that stop one iteration apart differ by more than 3 with nothing
    wrong in either (at 1e-13, nt_65: 7.8e-4 in natural order, 3.3e-3 in the device's -- an earlier form of this test).
    At the floor the factor measures what it is meant to: what rounding leaves."""
    dense = STORAGE[form]
    monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
    case = R.tpath_case(name)
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        n = ref.Nsub
        buf.atom_virtual_potentials.zero_()
        im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), False, False, 1.0, cg_tolerance=SOLVE_TOL, cg_max_iterations=20000, **kw)
        assert st["converged"] == 1 and st["relres"] <= SOLVE_TOL
        # the oracle adding in the device's order on the system as assembled on the device: identical
        od = _device_order_solve(oracle, [_device_rank(km, oracle, buf, 0, dense=bool(dense))], [n], [0], SOLVE_TOL, 20000)
        got = buf.atom_virtual_potentials.cpu().numpy()
        assert st["iterations"] == od["iterations"], (st["iterations"], od["iterations"])
        np.testing.assert_array_equal(got[:n], od["x"] * G0)
        assert (im < 0) == (Vd < 0) and im != 0
    # apart from the oracle's order: the true residual on the dense longdouble M, against the natural-order solve's
    T = _oracle_T(oracle, case, Vd)
    xo, ito, relo = T.solve(np.zeros(n), SOLVE_TOL, 20000)
    v = got[:n] / G0
    rhs = ref.rhs.astype(R.LD)
    res = float(np.sqrt((((rhs - ref.M @ v.astype(R.LD))) ** 2).sum()))
    res_o = float(np.sqrt((((rhs - ref.M @ xo.astype(R.LD))) ** 2).sum()))
    print("%s Vd %+g %s: %d iterations (natural order %d), true residual %.3e (natural order %.3e)" % (name, Vd, form, st["iterations"], ito, res, res_o))
    assert res <= 3 * res_o, (res, res_o)
    tight = np.r_[0, 1, 2 + np.nonzero(np.isin(ref.el[:-1], [TI, N_EL]))[0]]
    assert np.abs(v[tight] - xo[tight]).max() <= 2e-6 * np.abs(xo).max()


# ------------------------------------------------------------------------------------------------ (e) one rank group
@pytest.mark.parametrize("transport,storage", [(tr, stg) for tr in ("loopback", "p2p") for stg in ("bitmap", "tiles")])
def test_group_of_three(km, oracle, torch, monkeypatch, transport, storage):
    """group_178 (three block rows, six tiles) over three in-process ranks, strips of two tiles: two tiles on every rank.
    As tests/test_gpu_tpath.py::test_small_device_multirank, with the dense reference in the oracle's place."""
    P, name = 3, "group_178"
    monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
    monkeypatch.setenv("KMCF_SUB_STRIP", "2")
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    S = km.solvers
    case = R.tpath_case(name)
    Vd = case["par"]["Vd"]
    ref = R.case_ref(name, Vd)
    want = ref.as_csr()
    N = len(case["element"])
    comms = S.KMC_comm.loopback_group(ref.Nsub, ref.Nsub, N, N, P)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            with _device(km, torch, name, Vd, comm=comm) as (S_, buf, ref_, kw):
                S.t_assemble(buf, _prm(S, case, Vd))
                r0, nr = int(comm.displs_T[r]), int(comm.counts_T[r])
                _compare_assembly(S, buf, want, r0, nr)
                assert S.t_info(buf)["tunnel_dense"] == (1 if storage == "tiles" else 0)
                buf.atom_virtual_potentials.zero_()
                buf.site_power.fill_(-7.0)
                im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), True, False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000, **kw)
                out[r] = dict(im=im, st=st, v=buf.atom_virtual_potentials.cpu().numpy().copy(), pw=buf.site_power.cpu().numpy().copy(),
                              part=_device_rank(km, oracle, buf, r0, spread=storage == "tiles", strip=2), r0=r0, nr=nr, info=S.t_info(buf))
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
    if storage == "tiles":                                         # really dealt: more than one tile on at least two ranks
        held = [o["info"]["tunnel_bytes"] // 32768 for o in out]
        assert sum(held) == 6 and sum(h > 1 for h in held) >= 2, held
    od = _device_order_solve(oracle, [o["part"] for o in out], [o["nr"] for o in out], [o["r0"] for o in out], 1e-13, 20000)
    m = _m_of(ref, od["x"])
    want_im = ref.imacro(m)
    pw, ms = ref.power(m, Vd, 1.0)                                 # (heating on: potentials shifted by |min| after the scaling)
    w = pw != -7.0
    for o in out:
        assert o["st"]["converged"] == 1 and o["st"]["iterations"] == od["iterations"], (o["st"]["iterations"], od["iterations"])
        np.testing.assert_array_equal(o["v"][:ref.Nsub], ms[:ref.Nsub])
        np.testing.assert_array_equal(o["v"], out[0]["v"])         # replicated bit for bit
        np.testing.assert_array_equal(o["pw"], out[0]["pw"])
        assert o["im"] == out[0]["im"] and o["im"] > 0
        assert abs(o["im"] - want_im) <= 1e-11 * ref.imacro_scale(m), (o["im"], want_im)
        np.testing.assert_allclose(o["v"], ms, rtol=1e-15, atol=0)
        np.testing.assert_array_equal(o["pw"] == -7.0, pw == -7.0)
        assert np.abs(o["pw"] - pw)[w].max() <= 1e-11 * np.abs(pw[w]).max()
