"""GPU: the T path under periodic y-z boundaries (kmcf_initialize_sparsity_T_pbc) on the periodic devices of
tests/tpath_pbc_ref.py -- the brute-force and the wrapped-grid pattern path, pairs at exactly half a period, a pair that
is a tunnel pair in the open device and a neighbour bond through a face, pairs at exactly nn_dist through a face, the
ground atom's neighbours through the faces -- against the dense periodic reference of that file (TRefPbc: numpy,
longdouble sums; tests/test_tpath_pbc_ref.py asserts what every case is built for), in the three storage forms of the
block (KMCF_SUB_DENSE = 0 bitmap + packed values, 1 dense symmetric tiles, 2 jagged tiles) and dealt over rank groups.

This file mirrors tests/test_gpu_tpath_synthetic.py and its bars are that file's, none wider: patterns identical;
neighbour off-diagonals identical, diagonals rtol 1e-13; WKB values and tunnel diagonal rtol 1e-10 with exact zeros exact;
SpMV |dy_i| <= 1e-12 (|M| |x|)_i; I_macro 1e-11 of its absolute terms; power 1e-11 of its maximum; potentials after scale
and shift rtol 1e-15; converged solves identical to the oracle adding in the device's order, true residual (dense
longdouble M) <= 3 x a natural-order solve's.  Every compared assembly is the second on its state
(tpath_ref.other_state first).  The argument errors of the entry point need no device: tests/test_tpath_pbc_ref.py."""
import contextlib
import threading

import numpy as np
import pytest

import current_map_ref as CM
import tpath_pbc_ref as Q
import tpath_ref as R
from test_gpu_tpath import G0, _compare_assembly, _device_order_solve, _device_rank
from test_gpu_tpath_synthetic import SOLVE_TOL, STORAGE, _args, _first_assembly_then_state, _m_of, _prm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _make(km, torch, case, comm, periodic, pbc=1, lattice=None):
    """tests/test_gpu_tpath.py::_make with the case's lattice in the buffers and the periodic entry point."""
    S = km.solvers
    xyz = case["xyz"]
    N = len(case["element"])
    lat = list(case.get("L", (1.0, 1.0, 1.0))) if lattice is None else lattice
    buf = S.GPUBuffers(N, case["element"].copy(), xyz[:, 0].copy(), xyz[:, 1].copy(), xyz[:, 2].copy(), 52, 3.5e-10, 1.0, lat, case["metals"].copy())
    buf.site_charge.copy_(torch.as_tensor(np.asarray(case["charge"], np.int32)))
    buf.site_CB_edge = torch.as_tensor(np.asarray(case["cb"], np.float64), device="cuda")
    S.initialize_sparsity_T(buf, pbc, case["par"]["nn_dist"], case["n1"], case["n1"], case["layers"], comm, periodic=periodic)
    return buf


@contextlib.contextmanager
def _device(km, torch, name, Vd=None, comm=None, periodic=True, first=True):
    """One communicator (unless given) and one periodic T state for a case, freed on the way out; the case's state in
    place behind a first assembly on another one.  Yields (S, buf, ref, kw): ref the dense periodic reference."""
    S = km.solvers
    case = Q.tpath_pbc_case(name)
    Vd = case["par"]["Vd"] if Vd is None else Vd
    ref = Q.case_ref_pbc(name, Vd)
    own = comm is None
    if own:
        N = len(case["element"])
        comm = S.KMC_comm(ref.Nsub, ref.Nsub, N, N)
        comm.connect()
    buf = None
    try:
        buf = _make(km, torch, case, comm, periodic)
        assert buf.N_atom_ == ref.N_atom
        if first:
            _first_assembly_then_state(S, torch, buf, dict(case, name=name), Vd)
        yield S, buf, ref, dict(contact_x_lo=case["x_lo"], contact_x_hi=case["x_hi"])
    finally:
        if buf is not None:
            buf.freeGPUmemory()
        if own:
            comm.close()


@pytest.fixture(autouse=True)
def _case_ref_lookup(monkeypatch):
    """_first_assembly_then_state looks the case's point count up through tpath_ref.case_ref(name): serve the periodic
    cases from the periodic references (the open cases as before)."""
    open_ref = R.case_ref
    monkeypatch.setattr(R, "case_ref", lambda name, Vd=None: Q.case_ref_pbc(name, Vd) if name in Q.CASES_PBC else open_ref(name, Vd))


def _knobs(monkeypatch, case):
    for k, v in case["knobs"].items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ (1) assembly
@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_assembly_one_rank(km, torch, monkeypatch, name):
    """kmcf_initialize_sparsity_T_pbc + kmcf_t_assemble against TRefPbc in each storage form; the forms against each
    other by the equalities of test_gpu_tpath_synthetic.py::test_assembly_one_rank."""
    case = Q.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    res = {}
    for form, dense in STORAGE.items():
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        with _device(km, torch, name) as (S, buf, ref, kw):
            np.testing.assert_array_equal(S.t_atom_sites(buf), ref.atom_site)
            S.t_assemble(buf, _prm(S, case, case["par"]["Vd"]))
            tn = _compare_assembly(S, buf, ref.as_csr())
            info = S.t_info(buf)
            assert info["tunnel_points"] == ref.n_t and info["nnz_tunnel"] == int(ref.S_pattern.sum()), (form, info)
            assert info["tunnel_dense"] == dense, (form, info)
            np.testing.assert_array_equal(tn["val"] == 0, ref.tunnel_csr()[2] == 0)
            # the exported block is symmetric bit for bit: d(i, j) and d(j, i) are the same bits
            dense_S = np.zeros((ref.n_t, ref.n_t))
            rows = np.repeat(np.arange(ref.n_t), np.diff(tn["row_ptr"]))
            dense_S[rows, tn["col"]] = tn["val"]
            np.testing.assert_array_equal(dense_S, dense_S.T)
            res[form] = dict(tn=tn, dinv=S.t_vectors(buf)["dinv"])
    a, b, c = res["bitmap"], res["tiles"], res["jagged"]
    for key in ("row_ptr", "col"):
        np.testing.assert_array_equal(a["tn"][key], b["tn"][key])
    # The same WKB values, bit for bit, and the same -(row sums) on the diagonal: a periodic state adds a row's sum in ONE
    # order whatever the form (tunnel_rowsum_kernel) -- the bitmap's bytes, where the open forms agree to rtol 1e-12.
    np.testing.assert_array_equal(b["tn"]["val"], a["tn"]["val"])
    np.testing.assert_array_equal(b["tn"]["diag"], a["tn"]["diag"])
    np.testing.assert_array_equal(b["dinv"], a["dinv"])
    for key in ("val", "diag", "row_ptr", "col"):                                                # jagged: the dense tiles' entries, same order
        np.testing.assert_array_equal(c["tn"][key], b["tn"][key])
    np.testing.assert_array_equal(c["dinv"], b["dinv"])


# ------------------------------------------------------------------------------------------------ (2) what the state reports
@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_state_reports_its_geometry(km, torch, monkeypatch, name):
    """t_periodic gives back what was passed; the plain kmcf_initialize_sparsity_T on the same device gives pbc = 0 and a
    pattern with strictly fewer entries in exactly the rows that hold a bond through a face."""
    case = Q.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    with _device(km, torch, name, first=False) as (S, buf, ref, kw):
        pbc, lat = S.t_periodic(buf)
        assert pbc == 1
        np.testing.assert_array_equal(lat, np.asarray(case["L"], np.float64))
        rp_p, col_p = S.t_pattern(buf)
    with _device(km, torch, name, periodic=False, first=False) as (S, buf, ref, kw):
        pbc, lat = S.t_periodic(buf)
        assert pbc == 0 and np.all(lat == 0.0)
        rp_o, col_o = S.t_pattern(buf)
        op = R.ref_of(case)                                      # the open reference on the same device
        orp, ocol, _ = op.neighbour_csr()
        np.testing.assert_array_equal(rp_o, orp)
        np.testing.assert_array_equal(col_o, ocol)
    fewer = np.flatnonzero(np.diff(rp_o) < np.diff(rp_p))
    np.testing.assert_array_equal(fewer, ref.wrap_bond_rows())
    assert len(fewer) and np.all(np.diff(rp_o) <= np.diff(rp_p))


# ------------------------------------------------------------------------------------------------ (3) SpMV, current, power
@pytest.mark.parametrize("form", list(STORAGE))
@pytest.mark.parametrize("name", ["pbc_group_178", "pbc_distance_edges"])
def test_split_spmv_then_current_and_power(km, torch, monkeypatch, name, form):
    """y = A_n x + P^T S P x against the dense longdouble M (two products, as test_split_spmv); then I_macro and the
    dissipated power of prescribed potentials under Vd = +2 and -2 (0 CG iterations)."""
    monkeypatch.setenv("KMCF_SUB_DENSE", str(STORAGE[form]))
    case = Q.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    for Vd in (2.0, -2.0):
        with _device(km, torch, name, Vd) as (S, buf, ref, kw):
            if Vd > 0:
                S.t_assemble(buf, _prm(S, case, Vd))
                mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_tstate_matrix(buf.T_distributed))
                rng = np.random.default_rng(5)
                absM = np.abs(ref.M)
                for scale in (1.0, 1e3):
                    x = scale * (rng.standard_normal(ref.Nsub) + 3.0 * rng.random(ref.Nsub))
                    p = torch.as_tensor(x, device="cuda")
                    Ap = torch.empty_like(p)
                    mat.spmv(p, Ap)
                    err = np.abs(Ap.cpu().numpy() - ref.M @ x.astype(R.LD))
                    bound = absM @ np.abs(x).astype(R.LD)
                    print("%s %s x%g: SpMV worst %.3e of (|M||x|)_i" % (name, form, scale, float((err / bound).max())))
                    assert np.all(err <= 1e-12 * bound), (form, scale, int(np.argmax(err / bound)), float((err / bound).max()))
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
                print("%s %s Vd %+g: I_macro off by %.3e of its absolute terms" % (name, form, Vd, abs(im - want_im) / ref.imacro_scale(m)))
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
                    print("%s %s Vd %+g: power off by %.3e of its maximum" % (name, form, Vd, float(np.abs(gp - pw)[w].max() / np.abs(pw[w]).max())))
                    assert np.abs(gp - pw)[w].max() <= 1e-11 * np.abs(pw[w]).max()
                    assert (gp[w] != 0).any() and np.all(gp[w] >= 0)


# ------------------------------------------------------------------------------------------------ (4) converged solve
@pytest.mark.parametrize("form", list(STORAGE))
@pytest.mark.parametrize("name", ["pbc_nt_65", "pbc_group_178"])
def test_converged_solve_one_rank(km, oracle, torch, monkeypatch, name, form):
    """The solve to SOLVE_TOL = 1e-20: identical in iteration count and in every entry to the oracle adding in the
    device's order (fed by the device's own assembled CSR: it needs no periodic oracle), and a true residual on the dense
    longdouble M of at most 3 x that of tpath_pbc_ref.pcg_natural, a plain natural-order float64 Jacobi-PCG run to the same
    tolerance.  The tolerance, the factor and their reason:
    tests/test_gpu_tpath_synthetic.py::test_converged_solve_one_rank's docstring (at 1e-20 both solves sit on the floor that
    rounding leaves, where the factor compares what it is meant to)."""
    dense = STORAGE[form]
    monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
    case = Q.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    Vd = case["par"]["Vd"]
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        n = ref.Nsub
        buf.atom_virtual_potentials.zero_()
        im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), False, False, 1.0, cg_tolerance=SOLVE_TOL, cg_max_iterations=20000, **kw)
        assert st["converged"] == 1 and st["relres"] <= SOLVE_TOL
        strip = int(case["knobs"].get("KMCF_SUB_STRIP", 16))
        od = _device_order_solve(oracle, [_device_rank(km, oracle, buf, 0, dense=bool(dense), strip=strip)], [n], [0], SOLVE_TOL, 20000)
        got = buf.atom_virtual_potentials.cpu().numpy()
        assert st["iterations"] == od["iterations"], (st["iterations"], od["iterations"])
        np.testing.assert_array_equal(got[:n], od["x"] * G0)
        assert im > 0
    xo, ito = Q.pcg_natural_case(name, Vd, SOLVE_TOL)
    v = got[:n] / G0
    rhs = ref.rhs.astype(R.LD)
    res = float(np.sqrt((((rhs - ref.M @ v.astype(R.LD))) ** 2).sum()))
    res_o = float(np.sqrt((((rhs - ref.M @ xo.astype(R.LD))) ** 2).sum()))
    print("%s %s: %d iterations (natural order %d), true residual %.3e (natural order %.3e)" % (name, form, st["iterations"], ito, res, res_o))
    assert res <= 3 * res_o, (res, res_o)


# ------------------------------------------------------------------------------------------------ (5) rank groups
_ONE_RANK = {}


def _one_rank_assembly(km, torch, storage):
    """pbc_group_178 assembled on one rank (strips of two tiles), per storage form: what a group must reproduce."""
    if storage not in _ONE_RANK:
        name = "pbc_group_178"
        case = Q.tpath_pbc_case(name)
        with _device(km, torch, name) as (S, buf, ref, kw):
            S.t_assemble(buf, _prm(S, case, case["par"]["Vd"]))
            v, tn = S.t_vectors(buf), S.t_tunnel(buf)
            rp, col = S.t_pattern(buf)
            _ONE_RANK[storage] = dict(rp=rp, col=col, val=v["val"], diag_neighbour=v["diag_neighbour"], dinv=v["dinv"], rhs=v["rhs"],
                                      t_rp=tn["row_ptr"], t_col=tn["col"], t_val=tn["val"], t_diag=tn["diag"])
    return _ONE_RANK[storage]


@pytest.mark.parametrize("P,transport,storage", [(P, tr, stg) for P in (2, 3) for tr in ("loopback", "p2p") for stg in ("bitmap", "tiles")])
def test_rank_groups(km, oracle, torch, monkeypatch, P, transport, storage):
    """pbc_group_178 over in-process groups of 2 and 3, strips of two tiles: every rank's rows of the assembly are the
    one-rank state's bytes -- pattern, neighbour values and diagonal, right-hand side, tunnel pattern, every WKB value,
    and the entries that are SUMS: the tunnel diagonal -(row sum), stored in the block and exported, and 1 / diagonal --
    and the solve is identical to the oracle adding in the device's order.  (The sums: a periodic state held as tiles
    takes its row sums from the walk over the pair bitmap, tunnel_rowsum_kernel, a row's sum depending on the row alone,
    and a group gathers them.  The open state's sums of one application of the tiles depend on the deal -- tiles over
    three ranks: some diagonals one unit in the last place from the one-rank state's -- which is why this is asserted of
    the periodic state.)
    Bonds through a face join atoms of one x layer: no halo a group would not have in the open device's layers."""
    name = "pbc_group_178"
    monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
    monkeypatch.setenv("KMCF_SUB_STRIP", "2")
    monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    one = _one_rank_assembly(km, torch, storage)
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    S = km.solvers
    case = Q.tpath_pbc_case(name)
    Vd = case["par"]["Vd"]
    ref = Q.case_ref_pbc(name, Vd)
    want = ref.as_csr()
    N = len(case["element"])
    comms = S.KMC_comm.loopback_group(ref.Nsub, ref.Nsub, N, N, P)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            with _device(km, torch, name, Vd, comm=comm) as (S_, buf, ref_, kw):
                assert S.t_periodic(buf)[0] == 1
                S.t_assemble(buf, _prm(S, case, Vd))
                r0, nr = int(comm.displs_T[r]), int(comm.counts_T[r])
                tn = _compare_assembly(S, buf, want, r0, nr)
                assert S.t_info(buf)["tunnel_dense"] == (1 if storage == "tiles" else 0)
                v = S.t_vectors(buf)
                rp, col = S.t_pattern(buf)
                asm = dict(rp=rp, col=col, val=v["val"].copy(), diag_neighbour=v["diag_neighbour"].copy(), dinv=v["dinv"].copy(), rhs=v["rhs"].copy(),
                           t_rp=tn["row_ptr"], t_col=tn["col"], t_val=tn["val"].copy(), t_diag=tn["diag"].copy(), first=tn["first"])
                buf.atom_virtual_potentials.zero_()
                buf.site_power.fill_(-7.0)
                im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), True, False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000, **kw)
                out[r] = dict(im=im, st=st, v=buf.atom_virtual_potentials.cpu().numpy().copy(), pw=buf.site_power.cpu().numpy().copy(),
                              part=_device_rank(km, oracle, buf, r0, spread=storage == "tiles", strip=2), r0=r0, nr=nr, info=S.t_info(buf), asm=asm)
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
    if storage == "tiles":                                         # really dealt
        held = [o["info"]["tunnel_bytes"] // 32768 for o in out]
        assert sum(held) == 6 and sum(h > 0 for h in held) >= 2, held
    # every rank's rows: the one-rank state's bytes
    for o in out:
        a, r0, nr = o["asm"], o["r0"], o["nr"]
        e0, e1 = one["rp"][r0], one["rp"][r0 + nr]
        np.testing.assert_array_equal(a["rp"], one["rp"][r0:r0 + nr + 1] - e0)
        np.testing.assert_array_equal(a["col"], one["col"][e0:e1])
        np.testing.assert_array_equal(a["val"], one["val"][e0:e1])
        for key in ("diag_neighbour", "rhs"):
            np.testing.assert_array_equal(a[key], one[key][r0:r0 + nr])
        s0, ns = a["first"], len(a["t_rp"]) - 1
        t0, t1 = one["t_rp"][s0], one["t_rp"][s0 + ns]
        np.testing.assert_array_equal(a["t_rp"], one["t_rp"][s0:s0 + ns + 1] - t0)
        np.testing.assert_array_equal(a["t_col"], one["t_col"][t0:t1])
        np.testing.assert_array_equal(a["t_val"], one["t_val"][t0:t1])          # every WKB value, and the diagonal entries
        np.testing.assert_array_equal(a["t_diag"], one["t_diag"][s0:s0 + ns])
        np.testing.assert_array_equal(a["dinv"], one["dinv"][r0:r0 + nr])
    od = _device_order_solve(oracle, [o["part"] for o in out], [o["nr"] for o in out], [o["r0"] for o in out], 1e-13, 20000)
    m = _m_of(ref, od["x"])
    want_im = ref.imacro(m)
    pw, ms = ref.power(m, Vd, 1.0)
    w = pw != -7.0
    for o in out:
        assert o["st"]["converged"] == 1 and o["st"]["iterations"] == od["iterations"], (o["st"]["iterations"], od["iterations"])
        np.testing.assert_array_equal(o["v"][:ref.Nsub], ms[:ref.Nsub])
        np.testing.assert_array_equal(o["v"], out[0]["v"])         # replicated bit for bit
        np.testing.assert_array_equal(o["pw"], out[0]["pw"])
        assert o["im"] == out[0]["im"] and o["im"] > 0
        assert abs(o["im"] - want_im) <= 1e-11 * ref.imacro_scale(m), (o["im"], want_im)
        np.testing.assert_array_equal(o["pw"] == -7.0, pw == -7.0)
        assert np.abs(o["pw"] - pw)[w].max() <= 1e-11 * np.abs(pw[w]).max()


# ------------------------------------------------------------------------------------------------ (6) current map
def test_current_map_on_the_periodic_state(km, torch, monkeypatch):
    """solvers.current_map on the periodic state of pbc_group_178.  (i) Against current_map_ref.from_device -- the stored
    values of the storage in use against the map's fresh evaluation of every pair -- within that file's bound of two orders
    of addition, n_r 2^-52 S_r: a map that measured a pair with the open distance would miss it by orders of magnitude on
    every pair through a face.  (ii) Against from_parts on TRefPbc: the same pairs (the periodic pattern: bonds and tunnel
    pairs through the faces), and the node sums within the same bound, n_r 2^-52 S_r of the reference's own sums."""
    name = "pbc_group_178"
    case = Q.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    monkeypatch.setenv("KMCF_SUB_DENSE", "1")
    Vd = case["par"]["Vd"]
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        S.t_assemble(buf, _prm(S, case, Vd))
        m = _m_of(ref, R.potentials(ref, Vd))
        buf.atom_virtual_potentials.copy_(torch.as_tensor(m, device="cuda"))
        torch.cuda.synchronize()
        out = S.current_map(buf)
        got = dict(current=out["current"].cpu().numpy(), tunnel=out["tunnel"].cpu().numpy(), net=out["net"].cpu().numpy())
        dev = CM.from_device(S, buf, m)
        N, atom_site = len(case["element"]), ref.atom_site
        rp, col, val = ref.neighbour_csr()
        srp, scol, sval = ref.tunnel_csr()
        want = CM.from_parts(ref.Nsub, rp, col, val, m, 0, dict(tunnel_idx=ref.tunnel_idx, row_ptr=srp, col=scol, val=sval, first=0))
        assert out["stats"]["tunnel_pairs_walked"] == int(want["n_t"].sum()) == int(ref.S_pattern.sum()) - ref.n_t
        np.testing.assert_array_equal(dev["r"], want["r"])         # the same pairs, row by row
        np.testing.assert_array_equal(dev["n"], want["n"])
        for what, r in (("from_device", dev), ("from_parts on TRefPbc", want)):
            bound = CM.to_sites(N, atom_site, r["n"] * CM.EPS * r["S"])
            for key, node_key, f in (("current", "through", 0.5), ("tunnel", "tunnel", 0.5), ("net", "net", 1.0)):
                diff = np.abs(got[key] - CM.to_sites(N, atom_site, r[node_key]))
                worst = float((diff / np.maximum(f * bound, 1e-300)).max())
                print("%s %s: worst %.3f of the bound n_r 2^-52 S_r" % (what, key, worst))
                assert np.all(diff <= f * bound), (what, key, worst)
        assert (got["tunnel"] > 0).any() and np.all(got["current"][np.setdiff1d(np.arange(N), atom_site[:-1])] == 0)
        # the open map of the same device and field is another map
        st_p = out["stats"]
    with _device(km, torch, name, Vd, periodic=False) as (S, buf, ref, kw):
        S.t_assemble(buf, _prm(S, case, Vd))
        buf.atom_virtual_potentials.copy_(torch.as_tensor(m, device="cuda"))
        torch.cuda.synchronize()
        st_o = S.current_map(buf)["stats"]
        assert st_o["sum_through"] != st_p["sum_through"] and st_o["sum_tunnel"] != st_p["sum_tunnel"]


# ------------------------------------------------------------------------------------------------ (7) pbc = 0: the old entry point's bytes
def test_pbc_0_is_the_plain_entry_point(km, torch, monkeypatch):
    """kmcf_initialize_sparsity_T_pbc with pbc = 0 (h_lattice NULL, and a lattice that would wrap everything) on nt_129:
    pattern, neighbour values, tunnel export, dinv and the solved potentials are the bytes of kmcf_initialize_sparsity_T."""
    import ctypes as C
    name = "nt_129"
    case = R.tpath_case(name)
    _knobs(monkeypatch, case)
    S = km.solvers
    lib = km.lib.load()
    ref = R.case_ref(name)
    Vd = case["par"]["Vd"]
    N = len(case["element"])
    res = []
    for entry, lattice in (("plain", None), ("pbc0", None), ("pbc0", [30.0, 5.0, 5.0])):
        comm = S.KMC_comm(ref.Nsub, ref.Nsub, N, N)
        comm.connect()
        buf = _make(km, torch, case, comm, periodic=False, pbc=0)
        if entry == "pbc0":                                      # replace the state by one of the new entry point
            lib.kmcf_tstate_destroy(buf.T_distributed)
            h = C.c_void_p()
            cnt = np.ascontiguousarray(comm.counts_T, np.int32)
            dsp = np.ascontiguousarray(comm.displs_T, np.int32)
            ip = C.POINTER(C.c_int)
            lat = None if lattice is None else (C.c_double * 3)(*lattice)
            dptr = lambda t: C.c_void_p(t.data_ptr())
            km.lib.check(lib.kmcf_initialize_sparsity_T_pbc(comm.handle, dptr(buf.site_x), dptr(buf.site_y), dptr(buf.site_z), dptr(buf.site_element), N,
                                                            lat, 0, case["par"]["nn_dist"], case["n1"], case["n1"], case["layers"],
                                                            cnt.ctypes.data_as(ip), dsp.ctypes.data_as(ip), C.byref(h)), "kmcf_initialize_sparsity_T_pbc")
            buf.T_distributed = h
        try:
            assert S.t_periodic(buf)[0] == 0 and np.all(S.t_periodic(buf)[1] == 0.0)
            _first_assembly_then_state(S, torch, buf, case, Vd)
            buf.atom_virtual_potentials.zero_()
            buf.site_power.fill_(-7.0)
            im, st = S.update_power_gpu_sparse_dist(buf, *_args(case, Vd), True, False, 1.0, cg_tolerance=1e-13, cg_max_iterations=20000,
                                                    contact_x_lo=case["x_lo"], contact_x_hi=case["x_hi"])
            assert st["converged"] == 1
            v, tn = S.t_vectors(buf), S.t_tunnel(buf)
            rp, col = S.t_pattern(buf)
            res.append(dict(rp=rp, col=col, val=v["val"], diag=v["diag_neighbour"], dinv=v["dinv"], rhs=v["rhs"], t_idx=tn["tunnel_idx"],
                            t_rp=tn["row_ptr"], t_col=tn["col"], t_val=tn["val"], t_diag=tn["diag"], pot=buf.atom_virtual_potentials.cpu().numpy(),
                            pw=buf.site_power.cpu().numpy(), it=np.array([st["iterations"]]), im=np.array([im])))
        finally:
            buf.freeGPUmemory()
            comm.close()
    for other in res[1:]:
        for key, want in res[0].items():
            assert np.asarray(other[key]).tobytes() == np.asarray(want).tobytes(), key
