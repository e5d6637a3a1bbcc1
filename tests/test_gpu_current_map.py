"""GPU: kmcf_current_map (site-resolved current: through, tunnel share, Kirchhoff residual) against the numpy restatement
tests/current_map_ref.py built from the device's own exports.

Bar of every per-site comparison: |dev - ref| <= n_r * 2**-52 * S_r (x 1/2 for through and tunnel), n_r the pairs of the
node, S_r = sum |I_rc|: each I_rc is the same two rounded operations on both sides, only the order of the additions
differs (current_map_ref.py says why that is the bound of two orders).  Sites that hold no atom row are exactly 0.

Windows: the shapes are named by their tunnel point counts (91 = two mask words and a tail of 27; 20 = one partial word;
386 = seven words and a tail of 2); small_device gives these counts with the window x.min() + 0.1 .. x.max() - 0.1 (the
one tests/test_current_map_ref.py uses), so that window is used and the counts are asserted.  The narrower window of
tests/test_gpu_tpath.py (59 points on small_device(): less than one word) runs as one more shape."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import current_map_ref as R
from test_oracle_T import DEFECT, N_EL, O_EL, OD, PAR, Q, TI, VAC, small_device

pytestmark = pytest.mark.gpu

G0 = 2 * 3.8612e-5 * 1e-5
A_LAT = 2.5


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- cases
def _case_small(window="wide", vacancies="all", **kw):
    d = small_device(**kw)
    el, ch = d["element"].copy(), d["charge"].copy()
    if vacancies != "all":                                  # every vacancy (or all but one) turned to oxygen
        vac = np.nonzero(el == VAC)[0]
        keep = vac[len(vac) // 2:len(vac) // 2 + 1] if vacancies == "one" else vac[:0]
        gone = np.setdiff1d(vac, keep)
        el[gone] = O_EL
        ch[gone] = 0
    x = d["xyz"][:, 0]
    lo, hi = {"wide": (x.min() + 0.1, x.max() - 0.1), "tpath": ((d["layers"] - 1) * A_LAT - 0.1, (d["layers"] + 7) * A_LAT + 0.1),
              "middle": ((d["layers"] + 1) * A_LAT - 0.1, (d["layers"] + 5) * A_LAT + 0.1), "none": (1e9, -1e9)}[window]
    return dict(xyz=d["xyz"], element=el, charge=ch, cb=d["cb"], metals=np.array([TI, N_EL], np.int32), n1=d["n1"], layers=d["layers"],
                par=dict(PAR), lattice=[1, 1, 1], sigma=3.5e-10, k=1.0, win=dict(contact_x_lo=lo, contact_x_hi=hi),
                cg=dict(cg_tolerance=1e-13, cg_max_iterations=20000))


_CB5 = {}


def _cb_edge_5nm(km, torch, d, ref5):
    """The conduction-band edge of the 5 nm device as tests/test_gpu_tpath.py::test_5nm_device makes it: the oracle's
    charges, update_CB_edge_gpu_sparse on the K path.  Once per session."""
    if "cb" not in _CB5:
        S = km.solvers
        NL = d["N_contact"]
        comm = S.KMC_comm(d["N"] - 2 * NL, 25682, d["N"], d["N"])
        comm.connect()
        buf = S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"], d["lattice"], d["metals"])
        S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
        S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
        buf.site_charge.copy_(torch.as_tensor(ref5["charge"]))
        S.update_CB_edge_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"], len(d["metals"]))
        _CB5["cb"] = buf.site_CB_edge.cpu().numpy().copy()
        buf.freeGPUmemory()
        comm.close()
    return _CB5["cb"]


def _case_5nm(km, torch, dev5, ref5):
    d = dev5
    cb = _cb_edge_5nm(km, torch, d, ref5)
    par = dict(Vd=d["Vd"], high_G=1e5 * d["high_G"], low_G=d["low_G"], loop_G=1e7 * d["high_G"], tol=Q * 0.01, m_e=0.85 * 9.11e-31, V0=1.6,
               nn_dist=d["nn_dist"])
    return dict(xyz=d["xyz"], element=d["element"], charge=ref5["charge"], cb=cb, metals=d["metals"], n1=d["N_contact"], layers=10, par=par,
                lattice=d["lattice"], sigma=d["sigma"], k=d["k"], win={}, cg=dict(cg_tolerance=1e-13, cg_max_iterations=20000))


SHAPES = {
    "small_91": (lambda: _case_small(), 91),
    "small_59_tpath_window": (lambda: _case_small(window="tpath"), 59),
    "2x2x3_20": (lambda: _case_small(ny=2, nz=2, n_oxide_layers=3), 20),
    "no_points": (lambda: _case_small(window="none", vacancies="none"), 0),
    "one_point": (lambda: _case_small(window="none", vacancies="one"), 1),
}


def _n_atoms(case):
    return int(np.isin(case["element"], [DEFECT, OD], invert=True).sum())


def _open(km, torch, case, comm=None):
    S = km.solvers
    N, na = len(case["element"]), _n_atoms(case)
    if comm is None:
        comm = S.KMC_comm(na + 1, na + 1, N, N)
        comm.connect()
    xyz = case["xyz"]
    buf = S.GPUBuffers(N, case["element"], xyz[:, 0], xyz[:, 1], xyz[:, 2], 52, case["sigma"], case["k"], case["lattice"], case["metals"])
    buf.site_charge.copy_(torch.as_tensor(np.asarray(case["charge"], np.int32)))
    buf.site_CB_edge = torch.as_tensor(np.asarray(case["cb"], np.float64), device="cuda")
    S.initialize_sparsity_T(buf, 0, case["par"]["nn_dist"], case["n1"], case["n1"], case["layers"], comm)
    return comm, buf


def _params(S, case):
    p = case["par"]
    return S.current_params(p["Vd"], p["high_G"], p["low_G"], p["loop_G"], G0, p["tol"], p["m_e"], p["V0"], **case["win"])


def _update_power(S, buf, case, heating, **cg):
    p = case["par"]
    kw = dict(case["win"])
    kw.update(cg or case["cg"])
    return S.update_power_gpu_sparse_dist(buf, case["n1"], case["n1"], case["layers"], p["Vd"], p["high_G"], p["low_G"], p["loop_G"], G0,
                                          p["tol"], p["nn_dist"], p["m_e"], p["V0"], len(case["metals"]), bool(heating), False, 1.0, **kw)


def _upload(torch, buf, m):
    buf.atom_virtual_potentials.copy_(torch.as_tensor(np.ascontiguousarray(m, np.float64), device="cuda"))
    torch.cuda.synchronize()


def _map(S, buf):
    out = S.current_map(buf)
    return dict(current=out["current"].cpu().numpy(), tunnel=out["tunnel"].cpu().numpy(), net=out["net"].cpu().numpy(), stats=out["stats"])


def _random_field(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


def _site_bounds(N, atom_site, ref):
    return R.to_sites(N, atom_site, ref["n"] * R.EPS * ref["S"])


def _assert_within(got, ref, atom_site, what=""):
    """got: site arrays of the device; ref: node sums of the restatement (or of another device map's restatement)."""
    N = len(got["current"])
    bound = _site_bounds(N, atom_site, ref)
    worst = {}
    for key, node_key, f in (("current", "through", 0.5), ("tunnel", "tunnel", 0.5), ("net", "net", 1.0)):
        want = R.to_sites(N, atom_site, ref[node_key]) if "through" in ref else ref[key]
        diff = np.abs(got[key] - want)
        worst[key] = float((diff / np.maximum(f * bound, 1e-300)).max())
        bad = np.nonzero(diff > f * bound)[0]
        assert len(bad) == 0, "%s %s: %d sites beyond n_r 2^-52 S_r, worst %.3g of the bound (site %d: %.17g against %.17g)" % (
            what, key, len(bad), worst[key], bad[0], got[key][bad[0]], want[bad[0]])
    print("%s: largest |dev - ref| in units of the bound: through %.3f tunnel %.3f net %.3f" % (what, worst["current"], worst["tunnel"], worst["net"]))


def _assert_stats(got, ref, atom_site, n_atom, imacro=None, one_rank=True):
    st = got["stats"]
    na = len(atom_site) - 1
    assert abs(st["i_injection"] - ref["net"][1]) <= ref["n"][1] * R.EPS * ref["S"][1]
    assert abs(st["i_extraction"] + ref["net"][0]) <= ref["n"][0] * R.EPS * ref["S"][0]
    if imacro is not None:
        assert abs(st["i_injection"] - imacro) <= ref["n"][1] * R.EPS * ref["S"][1], (st["i_injection"], imacro)
    for key, arr in (("sum_through", got["current"]), ("sum_tunnel", got["tunnel"])):
        want = math.fsum(arr)
        assert abs(st[key] - want) <= n_atom * R.EPS * want, (key, st[key], want)
    th = got["current"][atom_site[:na]]
    k = int(np.argmax(th))                                         # the first maximum: the smallest site id among equals
    assert st["max_through"] == th[k] and st["max_site"] == atom_site[k], (st, th[k], atom_site[k])
    if one_rank:
        assert st["tunnel_pairs_walked"] == int(ref["n_t"].sum())
    assert st["ms"] > 0


# ---------------------------------------------------------------- one rank: shapes x fields
_SOLVED = {}      # shape -> (shift, atom_site, [(potentials, device map, restatement) without / with solve_heating])


@pytest.mark.parametrize("field", ["solved", "random"])
@pytest.mark.parametrize("shape", list(SHAPES) + ["5nm"])
def test_shapes_one_rank(km, torch, dev5, ref5, shape, field):
    S = km.solvers
    case, points = (_case_5nm(km, torch, dev5, ref5), 1913) if shape == "5nm" else (SHAPES[shape][0](), SHAPES[shape][1])
    comm, buf = _open(km, torch, case)
    try:
        na, N = buf.N_atom_, buf.N_
        atom_site = S.t_atom_sites(buf)
        if shape.startswith("small"):
            assert na == 208
        maps = []
        if field == "solved":
            # the device's own solve, without and with the |min| shift of solve_heating
            for heating in (0, 1):
                buf.atom_virtual_potentials.zero_()
                im, st = _update_power(S, buf, case, heating)
                assert st["converged"] == 1
                m = buf.atom_virtual_potentials.cpu().numpy().copy()
                got = _map(S, buf)
                ref = R.from_device(S, buf, m)
                _assert_within(got, ref, atom_site, "%s solved, heating %d" % (shape, heating))
                _assert_stats(got, ref, atom_site, na, imacro=im if heating == 0 else None)    # (I_macro is formed before the shift)
                maps.append((m, got, ref))
            (m0, g0, r0), (m1, g1, r1) = maps
            shift = abs(min(m0[2:].min(), 0.0))
            np.testing.assert_array_equal(m1, m0 + shift)          # what solve_heating did to the potentials
            _SOLVED[shape] = (shift, atom_site, maps)              # (for the two shift tests below)
        else:
            # every pair carries current; on a grid of 2**-20 a shift by 3 is exact, so it must drop out bit for bit
            m = _random_field(na + 2, 5)
            _upload(torch, buf, m)
            S.t_assemble(buf, _params(S, case))
            got = _map(S, buf)
            ref = R.from_device(S, buf, m)
            _assert_within(got, ref, atom_site, "%s random" % shape)
            _assert_stats(got, ref, atom_site, na)
            mq = np.round(m * 2.0 ** 20) / 2.0 ** 20
            _upload(torch, buf, mq)
            a = _map(S, buf)
            _upload(torch, buf, mq + 3.0)
            b = _map(S, buf)
            for key in ("current", "tunnel", "net"):
                np.testing.assert_array_equal(a[key], b[key])
            assert a["current"].max() > 0
            maps.append((m, got, ref))
        info = S.t_info(buf)
        assert info["tunnel_points"] == points, info
        for m, got, ref in maps:
            # nothing outside the atoms' sites; the last atom has no row
            rest = np.setdiff1d(np.arange(N), atom_site[:-1])
            for key in ("current", "tunnel", "net"):
                assert not got[key][rest].any()
            if points <= 1:                                        # no pair in the bitmap: the neighbour part alone
                assert not got["tunnel"].any() and got["stats"]["tunnel_pairs_walked"] == 0 and got["stats"]["sum_tunnel"] == 0.0
                assert info["nnz_tunnel"] == points
            else:
                assert got["tunnel"].max() > 0 and np.all(got["tunnel"] <= got["current"])
    finally:
        buf.freeGPUmemory()
        comm.close()


def _solved(request, shape):
    if shape not in _SOLVED:                                       # (run alone: make the maps now)
        request.getfixturevalue("km")
        test_shapes_one_rank(request.getfixturevalue("km"), request.getfixturevalue("torch"), request.getfixturevalue("dev5"),
                             request.getfixturevalue("ref5"), shape, "solved")
    return _SOLVED[shape]


def _shift_figures(shape, shift, atom_site, maps):
    """Largest difference of the two maps in units of the summation bound n_r 2**-52 S_r, on the device and in the
    restatement (numpy, fed the same two potential vectors)."""
    (m0, g0, r0), (m1, g1, r1) = maps
    N = len(g0["current"])
    bound = _site_bounds(N, atom_site, r0)
    out = {}
    for key, node_key, f in (("current", "through", 0.5), ("tunnel", "tunnel", 0.5), ("net", "net", 1.0)):
        out[key] = (float((np.abs(g1[key] - g0[key]) / np.maximum(f * bound, 1e-300)).max()),
                    float((np.abs(r1[node_key] - r0[node_key]) / np.maximum(f * r0["n"] * R.EPS * r0["S"], 1e-300)).max()))
    print("%s: shift %.3e; heating 1 against heating 0 in units of n_r 2^-52 S_r, device (restatement): through %.3f (%.3f) "
          "tunnel %.3f (%.3f) net %.3f (%.3f)" % ((shape, shift) + out["current"] + out["tunnel"] + out["net"]))
    return out


@pytest.mark.parametrize("shape", list(SHAPES) + ["5nm"])
def test_heating_shift_within_the_summation_bound(request, shape):
    """The maps of the device's own solve with solve_heating 0 and 1 (potentials m and fl(m + |min|)) agree within
    n_r * 2**-52 * S_r, the bar the feature's specification sets for this comparison.

    The bound covers two ORDERS OF ADDITION of the same terms; fl(m + shift) also rounds every potential by up to
    2**-53 |m|, which moves a term I_rc by up to g 2**-52 max|m|.  Whether that stays inside the bar depends on the
    potentials, so the figures are printed, for the device and for the numpy restatement fed the same two vectors.
    MEASURED (MI355X): shift 0 and identical bytes on small_91, small_59 and 2x2x3; no_points / one_point (shift
    2.4e-19): through 0.78 of the bar, net 0.98; the 5 nm device with the band edge of test_gpu_tpath.py::test_5nm_device
    (update_CB_edge_gpu_sparse; shift 3.4e-16): through 0.71 (restatement 0.74), net 0.77 (0.77).  The margin is not
    structural: with a synthetic band edge falling linearly in x instead (the one test_gpu_tpath.py's storage test uses,
    no case of this suite) the same device gave 3.5 x the bar at 58 of its sites, in the restatement 3.6 x, while device
    and restatement agreed within 0.28 of it on either vector.  test_heating_shift_within_its_own_rounding therefore
    also holds the two maps to the bound that includes the shift's rounding (0.2 of it at 5 nm), and the random-field
    tests shift by an amount that is exact in floating point and demand identical bytes."""
    shift, atom_site, maps = _solved(request, shape)
    (m0, g0, r0), (m1, g1, r1) = maps
    _shift_figures(shape, shift, atom_site, maps)
    _assert_within(g1, dict(n=r0["n"], S=r0["S"], current=g0["current"], tunnel=g0["tunnel"], net=g0["net"]), atom_site,
                   "%s heating 1 against heating 0" % shape)


@pytest.mark.parametrize("shape", list(SHAPES) + ["5nm"])
def test_heating_shift_within_its_own_rounding(request, shape):
    """The shift drops out up to what it does to the potentials themselves.  m1 = fl(m0 + shift) carries a relative
    rounding of 2**-53 per potential, so a difference m1[r] - m1[c] is off by at most 2 * 2**-53 * max|m1| from
    m0[r] - m0[c], a term I_rc by g_rc times that plus the roundings of the difference and the product on either side
    (2 * 2**-53 |I_rc| each); the additions add (n_r - 1) 2**-53 S_r per map.  Per node:
        |sum1 - sum0| <= (n_r + 2) 2**-52 max(S0_r, S1_r) + 2**-52 max|m1| sum_c g_rc
    (x 1/2 for through and tunnel).  A shift of exactly 0 must leave identical bytes."""
    shift, atom_site, maps = _solved(request, shape)
    (m0, g0, r0), (m1, g1, r1) = maps
    N = len(g0["current"])
    if shift == 0.0:
        for key in ("current", "tunnel", "net"):
            assert g1[key].tobytes() == g0[key].tobytes()
        return
    node_bound = (r0["n"] + 2) * R.EPS * np.maximum(r0["S"], r1["S"]) + R.EPS * np.abs(m1).max() * r0["G"]
    bound = R.to_sites(N, atom_site, node_bound)
    for key, f in (("current", 0.5), ("tunnel", 0.5), ("net", 1.0)):
        diff = np.abs(g1[key] - g0[key])
        print("%s %s: largest difference %.3f of the bound with the shift's rounding" % (shape, key, float((diff / np.maximum(f * bound, 1e-300)).max())))
        assert np.all(diff <= f * bound), key


# ---------------------------------------------------------------- storages of the tunnel block
def test_map_does_not_depend_on_the_storage(km, torch, monkeypatch):
    """386 points (seven mask words, a tail of 2) held as bitmap + values, dense tiles, jagged tiles: the map walks the
    bitmap and evaluates the pairs afresh, so the three maps are the same bytes; each is within the bound of the
    restatement built from the values that storage exports."""
    S = km.solvers
    case = _case_small(ny=8, nz=8, n_oxide_layers=9)
    res = {}
    for dense in (0, 1, 2):
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        comm, buf = _open(km, torch, case)
        try:
            atom_site = S.t_atom_sites(buf)
            buf.atom_virtual_potentials.zero_()
            im, st = _update_power(S, buf, case, 1)
            info = S.t_info(buf)
            assert info["tunnel_dense"] == dense and info["tunnel_points"] == 386 and buf.N_atom_ == 960
            out = []
            for m in (buf.atom_virtual_potentials.cpu().numpy().copy(), _random_field(buf.N_atom_ + 2, 9)):
                _upload(torch, buf, m)
                got = _map(S, buf)
                ref = R.from_device(S, buf, m)
                _assert_within(got, ref, atom_site, "storage %d" % dense)
                _assert_stats(got, ref, atom_site, buf.N_atom_)
                out.append((m, got))
            res[dense] = out
        finally:
            buf.freeGPUmemory()
            comm.close()
    # the random field is the same input for all three (the solved one differs by the storages' summation orders)
    for dense in (1, 2):
        np.testing.assert_array_equal(res[dense][1][0], res[0][1][0])
        for key in ("current", "tunnel", "net"):
            assert res[dense][1][1][key].tobytes() == res[0][1][1][key].tobytes(), (dense, key)
        for key in ("i_injection", "i_extraction", "sum_through", "sum_tunnel", "max_through", "max_site", "tunnel_pairs_walked"):
            assert res[dense][1][1]["stats"][key] == res[0][1][1]["stats"][key]


# ---------------------------------------------------------------- rank groups
@pytest.mark.parametrize("P,transport,storage", [(P, tr, stg) for P in (2, 3) for tr in ("loopback", "p2p") for stg in ("bitmap", "tiles")]
                         + [(5, "p2p", "tiles")])      # (five ranks, a window over the middle of the oxide: the outer ranks own no tunnel row)
def test_rank_groups(km, torch, P, transport, storage, monkeypatch):
    """small_device() over an in-process group (the cases of test_gpu_tpath.py::test_small_device_multirank): every rank
    forms the sums of its own rows, the per-node sums are all-gathered; all ranks return the same bytes and statistics,
    within the bound of the one-rank map."""
    S = km.solvers
    case = _case_small(window="middle" if P == 5 else "wide")
    fields = [_random_field(_n_atoms(case) + 2, 21), PAR["Vd"] * G0 * (0.5 + 0.5 * np.cos(np.arange(_n_atoms(case) + 2) * 0.05))]
    # one rank first (bitmap storage)
    monkeypatch.setenv("KMCF_SUB_DENSE", "0")
    monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    comm, buf = _open(km, torch, case)
    atom_site = S.t_atom_sites(buf)
    S.t_assemble(buf, _params(S, case))
    one = []
    for m in fields:
        _upload(torch, buf, m)
        got = _map(S, buf)
        ref = R.from_device(S, buf, m)
        _assert_within(got, ref, atom_site, "one rank")
        one.append((got, ref))
    buf.freeGPUmemory()
    comm.close()
    # the group
    monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
    monkeypatch.setenv("KMCF_SUB_STRIP", "1")
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    N, na = len(case["element"]), _n_atoms(case)
    comms = S.KMC_comm.loopback_group(na + 1, na + 1, N, N, P)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            _, b = _open(km, torch, case, comms[r])
            S.t_assemble(b, _params(S, case))
            info = S.t_info(b)
            assert info["tunnel_dense"] == (1 if storage == "tiles" else 0)
            maps = []
            for m in fields:
                _upload(torch, b, m)
                first = _map(S, b)
                again = _map(S, b)
                for key in ("current", "tunnel", "net"):
                    assert first[key].tobytes() == again[key].tobytes()
                maps.append(first)
            out[r] = dict(maps=maps, info=info)
            b.freeGPUmemory()
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
    rows = [o["info"]["tunnel_points_rank"] for o in out]
    print("tunnel rows per rank: %s" % rows)
    if P == 5:
        assert min(rows) == 0 and max(rows) > 0                    # (the case this parameter is here for)
    for f, (got1, ref1) in enumerate(one):
        for o in out:
            g = o["maps"][f]
            for key in ("current", "tunnel", "net"):
                assert g[key].tobytes() == out[0]["maps"][f][key].tobytes()
            for key in ("i_injection", "i_extraction", "sum_through", "sum_tunnel", "max_through", "max_site"):
                assert g["stats"][key] == out[0]["maps"][f]["stats"][key], key
            _assert_within(g, dict(n=ref1["n"], S=ref1["S"], current=got1["current"], tunnel=got1["tunnel"], net=got1["net"]), atom_site,
                           "P %d %s %s against one rank" % (P, transport, storage))
            _assert_within(g, ref1, atom_site, "P %d %s %s against the restatement" % (P, transport, storage))
            _assert_stats(g, ref1, atom_site, na, one_rank=False)
        # the pairs walked are each rank's own: together the one rank's
        assert sum(o["maps"][f]["stats"]["tunnel_pairs_walked"] for o in out) == got1["stats"]["tunnel_pairs_walked"]


# ---------------------------------------------------------------- statistics, determinism, untouched state, errors
def test_stats_determinism_and_untouched_state(km, torch):
    S = km.solvers
    case = _case_small()
    comm, buf = _open(km, torch, case)
    try:
        na, N = buf.N_atom_, buf.N_
        atom_site = S.t_atom_sites(buf)
        rng = np.random.default_rng(1)
        x0 = np.zeros(na + 2)
        x0[:na + 1] = PAR["Vd"] * (0.5 + 0.5 * np.cos(np.arange(na + 1) * 0.05)) + 1e-3 * rng.standard_normal(na + 1)

        def power(heating):
            _upload(torch, buf, x0)
            buf.site_power.fill_(-7.0)
            im, st = _update_power(S, buf, case, heating, cg_tolerance=1e-30, cg_max_iterations=0)
            assert st["iterations"] == 0
            return im, buf.atom_virtual_potentials.cpu().numpy().copy(), buf.site_power.cpu().numpy().copy()

        # i_injection = the I_macro the power update returned for the same potentials (heating off: no shift after it)
        im, m, pw = power(0)
        got = _map(S, buf)
        _assert_stats(got, R.from_device(S, buf, m), atom_site, na, imacro=im)
        assert im != 0.0
        im, m, pw = power(1)
        assert (pw != -7.0).any()
        tn = S.t_tunnel(buf)
        vec = S.t_vectors(buf)
        first = _map(S, buf)
        again = _map(S, buf)
        for key in ("current", "tunnel", "net"):                   # determinism: the same bytes
            assert first[key].tobytes() == again[key].tobytes()
        for key in first["stats"]:
            assert key == "ms" or first["stats"][key] == again["stats"][key]
        ref = R.from_device(S, buf, m)
        _assert_within(first, ref, atom_site, "prescribed potentials")
        _assert_stats(first, ref, atom_site, na)
        # the optional outputs may be left out
        only = S.current_map(buf, tunnel=False, net=False)
        assert only["tunnel"] is None and only["net"] is None
        assert only["current"].cpu().numpy().tobytes() == first["current"].tobytes()
        # untouched: potentials, site_power, the tunnel block, the matrix, and what the next power update gives
        np.testing.assert_array_equal(buf.atom_virtual_potentials.cpu().numpy(), m)
        np.testing.assert_array_equal(buf.site_power.cpu().numpy(), pw)
        tn2, vec2 = S.t_tunnel(buf), S.t_vectors(buf)
        for key in tn:
            np.testing.assert_array_equal(tn2[key], tn[key])
        for key in vec:
            np.testing.assert_array_equal(vec2[key], vec[key])
        im2, m2, pw2 = power(1)
        assert im2 == im
        np.testing.assert_array_equal(m2, m)
        np.testing.assert_array_equal(pw2, pw)
        # potentials given explicitly; all equal: no current anywhere, and the tie goes to the smallest site id
        flat = torch.full((na + 2,), 0.25, dtype=torch.float64, device="cuda")
        z = S.current_map(buf, potentials=flat)
        assert not z["current"].cpu().numpy().any() and not z["net"].cpu().numpy().any()
        assert z["stats"]["max_through"] == 0.0 and z["stats"]["max_site"] == atom_site[0]
        assert z["stats"]["i_injection"] == 0.0 and z["stats"]["sum_through"] == 0.0
    finally:
        buf.freeGPUmemory()
        comm.close()


def test_needs_an_assembled_state(km, torch):
    S = km.solvers
    case = _case_small(ny=2, nz=2, n_oxide_layers=3)
    comm, buf = _open(km, torch, case)
    try:
        lib = km.lib.load()
        out = torch.zeros(buf.N_, dtype=torch.float64, device="cuda")
        rc = lib.kmcf_current_map(buf.T_distributed, C.c_void_p(buf.atom_virtual_potentials.data_ptr()), C.c_void_p(out.data_ptr()),
                                  None, None, None)
        assert rc == -4 and b"kmcf_current_map" in lib.kmcf_last_error()                # KMCF_ERR_STATE
        with pytest.raises(km.lib.KmcfError):
            S.current_map(buf)
        S.t_assemble(buf, _params(S, case))
        assert S.current_map(buf)["stats"]["max_site"] >= 0
    finally:
        buf.freeGPUmemory()
        comm.close()
