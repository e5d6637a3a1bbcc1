"""GPU: periodic y-z boundaries in the neighbour list (kmcf_neighbor_list_pbc), the pairwise term
(kmcf_compute_cutoff_list_pbc + kmcf_poisson_gridless), the event rates (kmcf_events_set_lattice), and what becomes
periodic through them (clusters), against the brute-force restatements of tests/pbc_ref.py.  tests/test_pbc_ref.py
asserts, on the restatements alone, what every input is built for: margins to the cutoffs, pairs across the wrap in
every case, sums that a non-periodic kernel cannot reproduce.

  * neighbour list: equal to the restatement entry for entry (cell path, brute-force path, slices, truncated rows);
    pbc = 0 gives kmcf_neighbor_list's bytes; the periodic 5 nm cell gives the same list after a rigid shift in y and z.
  * pairwise term: per site |got - want| <= 1e-12 S_i (the bar and reference construction of test_gpu_site_kernels.py),
    sentinels outside the slice untouched, exactly +0.0 where a site has no term, two calls the same bytes, pbc = 0 the
    bytes of the non-periodic entry points, the error cases, kmcf_pairwise_periodic.
  * event rates: types equal, rates within 4 x the largest relative error of the SAME call with pbc = 0 against the
    non-periodic restatement on the same input (the parent arithmetic; the minimum image adds a few roundings to dist,
    hence the factor, as in test_gpu_events_thermal.py); wrap pairs' rates differ from the pbc = 0 rates; resetting the
    lattice restores a fresh communicator's bytes; one step against the restatement's selection.
  * clusters: a vacancy chain through the wrap is one cluster on the periodic list, two on the open one.
  * the gap search refuses a periodic index; tools/kmc_loop.py --workload 5nm-periodic runs.

Every test builds and frees its own communicator and buffers."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import pbc_ref as P
from test_pbc_ref import shifted_5nm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@contextlib.contextmanager
def _comm(km, N):
    c = km.solvers.KMC_comm(1, 2, N, N)
    c.connect()
    try:
        yield c
    finally:
        c.close()


def _i32(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.int32), device="cuda")


def _f64(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _coords(torch, xyz):
    return tuple(_f64(torch, xyz[:, a]) for a in range(3))


# ------------------------------------------------------------------------------------------------ neighbour list
def _list(km, torch, comm, xyz, L, pbc, nn_dist, nn, displ=0, count=None, entry="pbc"):
    lib, p = km.lib.load(), km.solvers._ptr
    N = len(xyz)
    count = N if count is None else count
    x, y, z = _coords(torch, xyz)
    out = torch.full((max(count, 1) * nn,), -7, dtype=torch.int32, device="cuda")
    if entry == "pbc":
        lat = None if L is None else np.ascontiguousarray(L, np.float64)
        km.lib.check(lib.kmcf_neighbor_list_pbc(comm.handle, p(x), p(y), p(z), N, None if lat is None else _dp(lat), pbc, nn_dist, nn,
                                                count, displ, p(out)), "kmcf_neighbor_list_pbc")
    else:
        km.lib.check(lib.kmcf_neighbor_list(comm.handle, p(x), p(y), p(z), N, nn_dist, nn, count, displ, p(out)), "kmcf_neighbor_list")
    return out.cpu().numpy()[:count * nn].reshape(count, nn)


@pytest.mark.parametrize("name", sorted(P.NEIGHBOR_CASES))
def test_neighbor_list_matches_brute_force(km, torch, name):
    c = P.pairwise_case(name)
    xyz, L, N, nn_dist = c["xyz"], c["L"], c["N"], P.NEIGHBOR_CASES[name]
    want, longest = P.neighbor_reference(name, nn_dist, P.NN)
    short, _ = P.neighbor_reference(name, nn_dist, P.NN_TRUNCATED)
    with _comm(km, N) as comm:
        got = _list(km, torch, comm, xyz, L, 1, nn_dist, P.NN)
        assert np.array_equal(got, want), "first at row %d" % int(np.flatnonzero((got != want).any(1))[0])
        assert np.array_equal(_list(km, torch, comm, xyz, L, 1, nn_dist, P.NN_TRUNCATED), short)          # rows cut at nn
        for displ, count in ((0, 0), (N - 1, 1), (N // 3 + 5, N // 4 + 3)):
            assert np.array_equal(_list(km, torch, comm, xyz, L, 1, nn_dist, P.NN, displ, count), want[displ:displ + count])
        # pbc = 0 through the new entry: the bytes of kmcf_neighbor_list, with or without a lattice
        opn = _list(km, torch, comm, xyz, None, 0, nn_dist, P.NN, entry="open")
        assert np.array_equal(_list(km, torch, comm, xyz, L, 0, nn_dist, P.NN), opn)
        assert np.array_equal(_list(km, torch, comm, xyz, None, 0, nn_dist, P.NN), opn)
        assert not np.array_equal(opn, want)
    print("%s: %d rows, longest %d, %d entries differ from the open list" % (name, N, longest, int((opn != want).sum())))


def test_neighbor_list_brute_force_path_and_errors(km, torch):
    """fewer than 3 cells of nn_dist fit the period in y: every pair is tested; rows longer than nn are cut"""
    c = P.pairwise_case(P.FALLBACK_CASE)
    want, longest = P.neighbor_reference(P.FALLBACK_CASE, P.FALLBACK_NN_DIST, P.FALLBACK_NN)
    lib = km.lib.load()
    with _comm(km, c["N"]) as comm:
        got = _list(km, torch, comm, c["xyz"], c["L"], 1, P.FALLBACK_NN_DIST, P.FALLBACK_NN)
        assert longest > P.FALLBACK_NN and np.array_equal(got, want)
        for L, pbc, word in ((None, 1, "h_lattice"), (c["L"], 2, "pbc"), ([45.0, 0.0, 30.0], 1, " y"), ([45.0, 25.0, np.nan], 1, " z"),
                             ([45.0, -25.0, 30.0], 1, " y"), ([45.0, 25.0, np.inf], 1, " z")):
            with pytest.raises(km.lib.KmcfError) as e:
                _list(km, torch, comm, c["xyz"], L, pbc, 3.5, P.NN)
            assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
    assert lib.kmcf_neighbor_list_pbc(None, None, None, None, 1, None, 0, 3.5, 4, 1, 0, None) == -1


def test_periodic_5nm_list_is_invariant_under_a_shift(km, torch):
    d = km.structure.periodic_5nm()
    N, L, nn_dist = d["N"], d["lattice"], d["nn_dist"]
    with _comm(km, N) as comm:
        t0 = time.perf_counter()
        a = _list(km, torch, comm, d["xyz"], L, 1, nn_dist, 52)
        ms = 1e3 * (time.perf_counter() - t0)
        b = _list(km, torch, comm, shifted_5nm(d), L, 1, nn_dist, 52)
        opn = _list(km, torch, comm, d["xyz"], L, 0, nn_dist, 52)
    n = (a >= 0).sum(1)
    print("periodic 5 nm: %d sites, %d list entries (%d open), rows %d .. %d, %.1f ms" % (N, int(n.sum()), int((opn >= 0).sum()), n.min(),
                                                                                        n.max(), ms))
    assert np.array_equal(a, b)
    assert int(n.sum()) == 2 * 479444 and n.min() == 10 and n.max() == 52 and int((opn >= 0).sum()) == 2 * 461392
    i, j, _ = km.structure.min_image_pairs(d["xyz"], L, nn_dist)
    rows = np.repeat(np.arange(N), n)
    assert np.array_equal(np.sort(np.r_[i, j] * N + np.r_[j, i]), rows.astype(np.int64) * N + a[a >= 0])


# ------------------------------------------------------------------------------------------------ pairwise term
@contextlib.contextmanager
def _index(km, torch, comm, xyz, L, pbc, entry="pbc"):
    lib, p = km.lib.load(), km.solvers._ptr
    x, y, z = _coords(torch, xyz)
    h = C.c_void_p()
    if entry == "pbc":
        lat = None if L is None else np.ascontiguousarray(L, np.float64)
        km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(x), p(y), p(z), len(xyz), P.CUTOFF, None if lat is None else _dp(lat),
                                                      pbc, C.byref(h)), "kmcf_compute_cutoff_list_pbc")
    else:
        km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(x), p(y), p(z), len(xyz), P.CUTOFF, C.byref(h)), "kmcf_compute_cutoff_list")
    try:
        yield h, (x, y, z)
    finally:
        lib.kmcf_pairwise_destroy(h)


def _pairwise(km, torch, h, xyz_d, charge, sigma, k, count, displ, N):
    lib, p = km.lib.load(), km.solvers._ptr
    pot = torch.full((N,), P.SENTINEL, dtype=torch.float64, device="cuda")
    km.lib.check(lib.kmcf_poisson_gridless(h, p(xyz_d[0]), p(xyz_d[1]), p(xyz_d[2]), p(charge), sigma, k, count, displ, p(pot)),
                 "kmcf_poisson_gridless")
    return pot.cpu().numpy()


@pytest.mark.parametrize("run", P.PAIRWISE_CASES)
def test_pairwise_term_matches_minimum_image_sum(km, dev5, torch, run):
    sigma, k = dev5["sigma"], dev5["k"]
    names = P.CHARGE_VARIANTS.get(run, (run,))
    first = P.pairwise_case(run)
    N, xyz, L = first["N"], first["xyz"], first["L"]
    lib = km.lib.load()
    with _comm(km, N) as comm, _index(km, torch, comm, xyz, L, 1) as (h, xyz_d):
        pbc, lat = C.c_int(-1), np.zeros(3)
        km.lib.check(lib.kmcf_pairwise_periodic(h, C.byref(pbc), _dp(lat)), "kmcf_pairwise_periodic")
        assert pbc.value == 1 and np.array_equal(lat, L)
        for name in names:
            c = P.pairwise_case(name)
            want, S, n = P.pairwise_reference(name, sigma, k)
            charge = _i32(torch, c["charge"])
            for displ, count in c["slices"]:
                got = _pairwise(km, torch, h, xyz_d, charge, sigma, k, count, displ, N)
                again = _pairwise(km, torch, h, xyz_d, charge, sigma, k, count, displ, N)
                sl = slice(displ, displ + count)
                err = np.abs(got[sl].astype(np.longdouble) - want[sl]).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rel = np.where(S[sl] > 0, err / S[sl], 0.0)
                print("%s rows [%d, %d): max |got - want| / S = %.3g, %d sites without a term"
                      % (name, displ, displ + count, rel.max() if count else 0.0, int((n[sl] == 0).sum())))
                assert np.all(got[:displ] == P.SENTINEL) and np.all(got[displ + count:] == P.SENTINEL)
                assert np.all(err <= 1e-12 * S[sl]), "site %d of the slice" % int(np.argmax(err - 1e-12 * S[sl]))
                lone = n[sl] == 0
                assert np.all(got[sl][lone] == 0.0) and not np.signbit(got[sl][lone]).any()
                assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("name", ["p23", "lattice_wrap"])
def test_pairwise_pbc0_is_the_non_periodic_index(km, dev5, torch, name):
    sigma, k = dev5["sigma"], dev5["k"]
    c = P.pairwise_case(name)
    N, xyz, L = c["N"], c["xyz"], c["L"]
    lib = km.lib.load()
    charge = _i32(torch, c["charge"])
    with _comm(km, N) as comm:
        with _index(km, torch, comm, xyz, None, 0, entry="open") as (h, xyz_d):
            base = _pairwise(km, torch, h, xyz_d, charge, sigma, k, N, 0, N)
            pbc = C.c_int(-1)
            km.lib.check(lib.kmcf_pairwise_periodic(h, C.byref(pbc), None), "kmcf_pairwise_periodic")
            assert pbc.value == 0
        for lattice in (L, None):
            with _index(km, torch, comm, xyz, lattice, 0) as (h, xyz_d):
                assert _pairwise(km, torch, h, xyz_d, charge, sigma, k, N, 0, N).tobytes() == base.tobytes()
                pbc, lat = C.c_int(-1), np.full(3, -1.0)
                km.lib.check(lib.kmcf_pairwise_periodic(h, C.byref(pbc), _dp(lat)), "kmcf_pairwise_periodic")
                assert pbc.value == 0 and np.array_equal(lat, L if lattice is not None else np.zeros(3))
    want, S, _ = P.pairwise_reference(name, sigma, k, False)
    assert np.all(np.abs(base.astype(np.longdouble) - want).astype(np.float64) <= 1e-12 * S)


def test_cutoff_list_pbc_error_cases(km, torch):
    c = P.pairwise_case("p11")
    xyz, L = c["xyz"], c["L"]
    lib = km.lib.load()
    span_y = float(xyz[:, 1].max() - xyz[:, 1].min())
    span_z = float(xyz[:, 2].max() - xyz[:, 2].min())
    with _comm(km, c["N"]) as comm:
        for lattice, pbc, word in ((None, 1, "h_lattice"), (L, 2, "pbc"), (L, -1, "pbc"),
                                   ([45.0, 0.0, 30.0], 1, " y"), ([45.0, -1.0, 30.0], 1, " y"), ([45.0, np.nan, 30.0], 1, " y"),
                                   ([45.0, np.inf, 30.0], 1, " y"), ([45.0, 25.0, 0.0], 1, " z"), ([45.0, 25.0, np.nan], 1, " z"),
                                   ([45.0, span_y, 30.0], 1, " y"), ([45.0, 25.0, span_z], 1, " z"), ([45.0, 25.0, 0.5 * span_z], 1, " z")):
            with pytest.raises(km.lib.KmcfError) as e:
                with _index(km, torch, comm, xyz, lattice, pbc):
                    pass
            assert "(-1)" in str(e.value) and word in str(e.value), str(e.value)
        with _index(km, torch, comm, xyz, [45.0, np.nextafter(span_y, 100.0), np.nextafter(span_z, 100.0)], 1):      # span < L: fine
            pass
    p = C.c_int()
    assert lib.kmcf_pairwise_periodic(None, C.byref(p), None) == -1 and b"kmcf_pairwise_periodic" in lib.kmcf_last_error()


# ------------------------------------------------------------------------------------------------ events
class _Box:
    """P.box() on the device with its periodic list"""

    def __init__(self, km, torch, dev5):
        self.km, self.S, self.torch = km, km.solvers, torch
        b = self.b = P.box()
        self.per, self.opn = P.box_lists()
        self.layers = km.structure.LAYERS
        self.lay = km.solvers.site_layers(b["xyz"][:, 0], self.layers)
        self.sigma, self.k, self.T_bg, self.freq = dev5["sigma"], dev5["k"], 300.0, 1e13
        self.xyz_d = _coords(torch, b["xyz"])
        self.neigh_d, self.lay_d, self.pot_d = _i32(torch, self.per.reshape(-1)), _i32(torch, self.lay), _f64(torch, b["pot"])
        self.reset()

    def reset(self):
        self.el, self.ch = _i32(self.torch, self.b["element"]), _i32(self.torch, self.b["charge"])

    def args(self, comm):
        N = self.b["N"]
        return (comm, N, comm.counts_events, comm.displs_events, P.BOX_NN, self.neigh_d, self.lay_d, self.T_bg, self.freq, self.sigma,
                self.k, *self.xyz_d, self.pot_d, self.el, self.ch)

    def rates(self, comm):
        return self.S.event_rates(*self.args(comm), self.layers)

    def ref(self, L):
        b = self.b
        return P.event_list(b["xyz"], self.per, self.lay, self.T_bg, self.freq, self.sigma, self.k, b["pot"], b["element"], b["charge"],
                            self.layers, L=L)


def _rel_err(got, want):
    live = want > 0
    assert np.array_equal(got == 0, want == 0)
    return float((np.abs(got[live] - want[live]) / want[live]).max())


def test_event_rates_take_the_minimum_image(km, dev5, torch):
    bx = _Box(km, torch, dev5)
    b, S = bx.b, km.solvers
    N = b["N"]
    wrap = P.wrap_slots(b["xyz"], bx.per, b["L"], P.BOX_NN_DIST)
    i = np.repeat(np.arange(N), P.BOX_NN).reshape(bx.per.shape)
    t_open, p_open = bx.ref(None)
    t_per, p_per = bx.ref(b["L"])
    with _comm(km, N) as fresh:
        typ_fresh, prob_fresh = bx.rates(fresh)
    with _comm(km, N) as comm:
        typ0, prob0 = bx.rates(comm)
        assert typ0.tobytes() == typ_fresh.tobytes() and prob0.tobytes() == prob_fresh.tobytes()
        err0 = _rel_err(prob0, p_open)                                    # the parent arithmetic on this input
        S.events_set_lattice(comm, b["L"], 1)
        typ1, prob1 = bx.rates(comm)
        S.events_reset(comm)                                              # does not clear the lattice
        typ1b, prob1b = bx.rates(comm)
        S.events_set_lattice(comm, None, 0)
        typ2, prob2 = bx.rates(comm)
        with pytest.raises(km.lib.KmcfError):
            S.events_set_lattice(comm, None, 1)
        for bad in ([36.0, 0.0, 15.0], [36.0, 12.5, -1.0], [36.0, np.nan, 15.0]):
            with pytest.raises(km.lib.KmcfError):
                S.events_set_lattice(comm, bad, 1)
        with pytest.raises(km.lib.KmcfError):
            S.events_set_lattice(comm, b["L"], 2)
        assert bx.rates(comm)[1].tobytes() == prob_fresh.tobytes()         # a refused call changes nothing
    assert km.lib.load().kmcf_events_set_lattice(None, None, 0) == -1
    assert np.array_equal(typ0, t_open) and np.array_equal(typ1, t_per)
    err1 = _rel_err(prob1, p_per)
    print("event rates, periodic box: %d live slots, %d across the wrap; largest relative error pbc 0 %.3e, pbc 1 %.3e (bar 4 x %.3e)"
          % (int((typ1 != P.EV_NULL).sum()), int((wrap & (typ1 != P.EV_NULL)).sum()), err0, err1, err0))
    assert err1 <= 4 * err0
    assert prob1b.tobytes() == prob1.tobytes() and typ1b.tobytes() == typ1.tobytes()
    assert typ2.tobytes() == typ_fresh.tobytes() and prob2.tobytes() == prob_fresh.tobytes()
    for et in (P.EV_REC, P.EV_VDIFF, P.EV_ODIFF):                         # (present: tests/test_pbc_ref.py)
        m = wrap & (typ1 == et) & (b["charge"][i] != 0) & (prob1 > 0) & (prob0 > 0)
        assert m.sum() >= 3 and np.all(prob1[m] != prob0[m])


def test_kmc_step_with_the_lattice_set(km, oracle, dev5, torch):
    bx = _Box(km, torch, dev5)
    b, S = bx.b, km.solvers
    cap, seed = 24, 3
    typ, prob = bx.ref(b["L"])
    u = oracle.mt_uniform_stream(seed, 2 * cap)
    t_r, n_r, log_r, el_r, ch_r, margins = P.kmc_step(bx.per, typ, prob, bx.freq, b["element"], b["charge"], u, cap)
    t_o, n_o, log_o = P.kmc_step(bx.per, *bx.ref(None), bx.freq, b["element"], b["charge"], u, cap)[:3]
    print("periodic step: %d events, smallest selection margin %.3g; the open-boundary rates select %s"
          % (n_r, margins.min(), "the same events" if np.array_equal(log_o, log_r) else "other events"))
    assert n_r >= 4 and margins.min() > 1e-9
    with _comm(km, b["N"]) as comm:
        S.events_set_lattice(comm, b["L"], 1)
        rng = S.RandomNumberGenerator(seed)
        t, n, log = S.execute_kmc_step_mpi(*bx.args(comm), rng, bx.layers, max_events=cap, return_log=True)
        el, ch = bx.el.cpu().numpy(), bx.ch.cpu().numpy()
        nxt = rng.getRandomNumber()
    assert n == n_r and np.array_equal(log, log_r)
    assert np.array_equal(el, el_r) and np.array_equal(ch, ch_r)
    assert t == pytest.approx(t_r, rel=1e-12)
    assert nxt == oracle.mt_uniform_stream(seed, 2 * n + 1)[-1]


# ------------------------------------------------------------------------------------------------ clusters, gap, loop
def test_vacancy_chain_through_the_wrap_is_one_cluster(km, dev5, torch):
    import clusters_ref as CR
    S = km.solvers
    b, ch = P.box(), P.chain()
    per, opn = P.box_lists()
    N = b["N"]
    metals = np.array([9], np.int32)
    with _comm(km, N) as comm:
        xyz = b["xyz"].copy()                  # (the inputs are read-only)
        buf = S.GPUBuffers(N, ch["element"].copy(), xyz[:, 0], xyz[:, 1], xyz[:, 2], P.BOX_NN, dev5["sigma"], dev5["k"], b["L"], metals)
        try:
            for pbc, lst, n_clusters in ((1, per, 1), (0, opn, 2)):
                S.compute_neighbor_list(comm, buf, P.BOX_NN_DIST, P.BOX_NN, pbc=pbc)
                assert np.array_equal(buf.neigh_idx.cpu().numpy().reshape(N, P.BOX_NN), lst)
                got = S.conductive_clusters(comm, buf, 0, 0)
                label, table, stats = CR.clusters(lst, ch["element"], ch["charge"], metals, b["xyz"][:, 0], 0, 0)
                assert got["stats"]["n_vacancy_clusters"] == n_clusters == stats["n_vacancy_clusters"]
                assert np.array_equal(got["label"].cpu().numpy(), label)
                for key in CR.TABLE_DTYPE.names:
                    assert np.array_equal(got["clusters"][key], table[key]), key
                for key in CR.STAT_KEYS:
                    assert got["stats"][key] == stats[key], key
        finally:
            buf.freeGPUmemory()


def test_gap_search_refuses_a_periodic_index(km, dev5, torch):
    S = km.solvers
    b = P.box()
    N = b["N"]
    with _comm(km, N) as comm:
        xyz = b["xyz"].copy()                  # (the inputs are read-only)
        buf = S.GPUBuffers(N, b["element"].copy(), xyz[:, 0], xyz[:, 1], xyz[:, 2], P.BOX_NN, dev5["sigma"], dev5["k"], b["L"],
                           np.array([9], np.int32))
        try:
            S.compute_neighbor_list(comm, buf, P.BOX_NN_DIST, P.BOX_NN, pbc=1)
            S.compute_cutoff_list(comm, buf, 20.0, pbc=1)
            side = _i32(torch, np.where(np.arange(N) % 2, 1, 2))
            with pytest.raises(km.lib.KmcfError) as e:
                S.site_set_gap(buf, side, 5.0)
            assert "(-1)" in str(e.value) and "periodic" in str(e.value), str(e.value)
            with pytest.raises(km.lib.KmcfError) as e:
                S.filament_gap(comm, buf, 0, 0, 5.0)
            assert "(-1)" in str(e.value) and "periodic" in str(e.value), str(e.value)
            S.poisson_gridless_gpu(buf, comm)                                # the index itself is fine
        finally:
            buf.freeGPUmemory()


def test_kmc_loop_periodic_workload():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kmc_loop.py"), "--workload", "5nm-periodic", "--steps", "2"],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "sites 37637" in out.stdout
    events = [int(n) for n in re.findall(r"events [0-9.]+ \((\d+) ev\)", out.stdout)]
    assert len(events) == 2 and sum(events) >= 1
    assert all(w in out.stdout for w in ("charge", "boundary", "pairwise", "gather"))
