"""GPU: the KMC event step (csrc/kmcf_events.hip) against oracle.kmc_step on the synthetic graphs of
tests/events_graph_ref.py, which reach what the 5 nm device and synth_small never do: the slow path's group loop, fast
and slow events inside one batch, the selection walk from memory, group sums read from memory, nn from 1 to 70, row counts
at the tree's boundaries, several full batches, a list that is not symmetric, a list without events, and the cache of the
symmetry verdict.  tests/test_events_graphs.py shows with the references alone that every case reaches what its name
says and that no selection lies within 1e-9 of a slot boundary: the device must give the oracle's log."""
import ctypes as C
import threading

import numpy as np
import pytest

import events_graph_ref as G
import events_thermal_ref as R

pytestmark = pytest.mark.gpu

KNOBS = ("KMCF_EV_TREL", "KMCF_EVENTS_PERSISTENT", "KMCF_EVENTS_FULLSCAN", "KMCF_EVENTS_PARTITIONED")
ERR_STATE = -4


@pytest.fixture(autouse=True)
def _clean_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


class _Dev:
    """One rank's device copy of a case; the neighbour list may live in a tensor the caller keeps (neigh=)."""

    def __init__(self, km, c, comm=None, neigh=None):
        import torch
        self.S, self.c = km.solvers, c
        self.own = comm is None
        if comm is None:
            comm = self.S.KMC_comm(max(c["N"] - 2, 1), c["N"] + 1, c["N"], c["N"])
            comm.connect()
        self.comm = comm
        self.f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        self.i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        r0, nr = int(comm.displs_events[comm.rank_events]), int(comm.counts_events[comm.rank_events])
        self.rows = slice(r0, r0 + nr)
        self.neigh = neigh if neigh is not None else self.i32(c["neigh"][self.rows].reshape(-1) if nr else np.full(1, -1))
        self.load(c)

    def load(self, c):
        """the site arrays, positions and potentials of case c (the neighbour tensor stays)"""
        self.c = c
        self.lay, self.pot = self.i32(c["lay"]), self.f64(c["pot"])
        self.x, self.y, self.z = (self.f64(c["xyz"][:, q]) for q in range(3))
        self.el, self.ch = self.i32(c["element"]), self.i32(c["charge"])

    def _args(self):
        c, m = self.c, self.comm
        return (m, c["N"], m.counts_events, m.displs_events, c["nn"], self.neigh, self.lay, c["T_bg"], c["freq"], c["sigma"],
                c["k"], self.x, self.y, self.z, self.pot, self.el, self.ch)

    def step(self, rng, max_events=None):
        return self.S.execute_kmc_step_mpi(*self._args(), rng, self.c["layers"], max_events=max_events or self.c["max_events"],
                                           return_log=True)

    def rates(self):
        return self.S.event_rates(*self._args(), self.c["layers"])

    def state(self):
        return self.el.cpu().numpy(), self.ch.cpu().numpy()

    def close(self):
        if self.own:
            self.comm.close()


def _same(oracle, dv, got, ref, rng=None):
    """count, log, final element / charge arrays equal; event time to 1e-12; two draws per event"""
    t, n, log = got
    assert n == ref["n"], (n, ref["n"])
    assert np.array_equal(log, ref["log"]), "first difference at event %d" % np.flatnonzero((log != ref["log"]).any(axis=1))[0]
    el, ch = dv.state()
    assert np.array_equal(el, ref["el"]) and np.array_equal(ch, ref["ch"])
    assert t == pytest.approx(ref["t"], rel=1e-12)
    if rng is not None:
        assert rng.getRandomNumber() == oracle.mt_uniform_stream(dv.c["seed"], 2 * n + 1)[-1]


def _run(km, oracle, name, callback=False):
    c, ref = G.case(name), G.reference(oracle, name)
    dv = _Dev(km, c)
    try:
        rng = km.solvers.RandomNumberGenerator(c["seed"])
        got = dv.step(rng.getRandomNumber if callback else rng)
        _same(oracle, dv, got, ref, rng)
    finally:
        dv.close()


@pytest.mark.parametrize("name", G.SYMMETRIC_CASES)
def test_default_path_matches_the_oracle(km, oracle, name):
    _run(km, oracle, name)


@pytest.mark.parametrize("variant", ["three_launches", "fullscan", "callback"])
@pytest.mark.parametrize("name", ["local7", "nn63", "mixed", "many"])
def test_other_paths_match_the_oracle(km, oracle, name, variant, monkeypatch):
    """KMCF_EVENTS_PERSISTENT=0: three launches per event; KMCF_EVENTS_FULLSCAN=1: the full pass per event; a callback
    generator: batches of one event."""
    if variant == "three_launches":
        monkeypatch.setenv("KMCF_EVENTS_PERSISTENT", "0")
    if variant == "fullscan":
        monkeypatch.setenv("KMCF_EVENTS_FULLSCAN", "1")
    _run(km, oracle, name, callback=variant == "callback")


@pytest.mark.parametrize("trel", [1, 64])
def test_mixed_under_a_shrunk_claim_range(km, oracle, trel, monkeypatch):
    """KMCF_EV_TREL: the slow events are those whose span reaches the value.  64 tiles: at least 10 slow and 10 fast events
    in the batch; 1 tile: every event is slow (rows i +- 70 never share a tile), the 5 nm test's setting on this graph."""
    fp = G.footprint(G.case("mixed")["neigh"], G.reference(oracle, "mixed")["log"])
    slow = G.slow_events(fp, trel)
    print("mixed, KMCF_EV_TREL=%d: slow / fast %d / %d" % (trel, slow.sum(), (~slow).sum()))
    assert slow.sum() >= 10
    if trel == 64:
        assert (~slow).sum() >= 10
    monkeypatch.setenv("KMCF_EV_TREL", str(trel))
    _run(km, oracle, "mixed")


@pytest.mark.parametrize("name", ["local7", "nn63", "nn70"])
def test_event_rates(km, name):
    """kmcf_event_rates: the types of events_thermal_ref.event_list; rates against the numpy.longdouble restatement within 4 x
    the error the f64 restatement itself shows against it (the factor of tests/test_gpu_events_thermal.py: a device exp /
    erfc an ulp or two off libm)."""
    c = G.case(name)
    dv = _Dev(km, c)
    try:
        typ, prob = dv.rates()
    finally:
        dv.close()
    t0, p0 = G.rates(c)
    assert typ.shape == (c["N"], c["nn"]) and np.array_equal(typ, t0)
    ii, cc, p_ld = G.rates_longdouble(c)
    live = np.zeros(typ.shape, bool)
    live[ii, cc] = True
    assert (prob[~live] == 0).all() and (prob[live] > 0).all()
    err_ref = float((np.abs(p0[ii, cc] - p_ld) / p_ld).max())
    err_dev = float((np.abs(prob[ii, cc] - p_ld) / p_ld).max())
    print("%s: %d live slots; relative rate error against longdouble: device %.3e, f64 restatement %.3e (bar 4 x)" % (
        name, len(ii), err_dev, err_ref))
    assert err_dev <= 4 * err_ref


def _run_group(km, oracle, name, P):
    """P ranks = P host threads on the loopback transport (tests/test_gpu_multirank.py::_run_ranks); every rank's result"""
    import torch
    c, ref = G.case(name), G.reference(oracle, name)
    comms = km.solvers.KMC_comm.loopback_group(max(c["N"] - 2, 1), c["N"] + 1, c["N"], c["N"], size=P, device=0)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comms[r].connect()
            dv = _Dev(km, c, comm=comms[r])
            rng = km.solvers.RandomNumberGenerator(c["seed"])
            got = dv.step(rng)
            out[r] = (dv, got, rng)
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    try:
        assert not errs, "\n".join(errs)
        assert all(o is not None for o in out), "a rank did not finish"
        for dv, got, rng in out:
            _same(oracle, dv, got, ref, rng)
    finally:
        for m in comms:
            m.close()
    return comms


@pytest.mark.parametrize("name,P,partitioned", [("local7", 3, False), ("local7", 3, True), ("local7", 4, True),
                                                ("tiny", 4, True), ("tiny", 6, True)])
def test_rank_groups(km, oracle, name, P, partitioned, monkeypatch):
    """Replicated (every rank steps the gathered list) and KMCF_EVENTS_PARTITIONED=1 (the reference's scheme): every rank
    ends with the oracle's log and state.  local7 on 4 ranks: uneven shares; tiny on 6: the last rank holds no row."""
    if partitioned:
        monkeypatch.setenv("KMCF_EVENTS_PARTITIONED", "1")
    comms = _run_group(km, oracle, name, P)
    counts = comms[0].counts_events
    if (name, P) == ("local7", 4):
        assert len(set(counts.tolist())) > 1
    if (name, P) == ("tiny", 6):
        assert counts[-1] == 0


def test_list_that_is_not_symmetric(km, oracle):
    """asym: local7 plus one-way edges.  The library must notice and take the full pass; a walk through the lists of i and j
    leaves the oracle's log within 20 events (tests/test_events_graphs.py::test_asym_has_teeth)."""
    _run(km, oracle, "asym")


@pytest.mark.parametrize("fullscan", [False, True])
def test_list_without_events(km, fullscan, monkeypatch):
    """Every site O: KMCF_ERR_STATE, "no event could be selected", no event counted, site arrays untouched.  (The two paths
    draw a different number of uniforms before they give up: the generator's position is unspecified, include/kmcfield.h.)"""
    if fullscan:
        monkeypatch.setenv("KMCF_EVENTS_FULLSCAN", "1")
    c = dict(G.case("local7"))
    c["element"] = np.full(c["N"], R.O_EL, np.int32)
    c["charge"] = np.zeros(c["N"], np.int32)
    dv = _Dev(km, c)
    lib = km.lib.load()
    try:
        S = km.solvers
        rng = S.RandomNumberGenerator(1)
        m = dv.comm
        cnt, dsp = np.asarray(m.counts_events, np.int32), np.asarray(m.displs_events, np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        E = [np.array([l[key] for l in c["layers"]]) for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        t, nev = C.c_double(-1.0), C.c_int(-1)
        ptr = lambda x: C.c_void_p(x.data_ptr())
        rc = lib.kmcf_execute_kmc_step(m.handle, c["N"], ip(cnt), ip(dsp), c["nn"], ptr(dv.neigh), ptr(dv.lay), c["T_bg"], c["freq"],
                                       c["sigma"], c["k"], ptr(dv.x), ptr(dv.y), ptr(dv.z), ptr(dv.pot), ptr(dv.el), ptr(dv.ch),
                                       5, dp(E[0]), dp(E[1]), dp(E[2]), dp(E[3]), C.cast(lib.kmcf_rng_next, C.c_void_p), rng.handle,
                                       64, C.byref(t), C.byref(nev), None)
        assert rc == ERR_STATE, (rc, lib.kmcf_last_error())
        assert b"no event could be selected" in lib.kmcf_last_error()
        assert nev.value == 0
        el, ch = dv.state()
        assert np.array_equal(el, c["element"]) and np.array_equal(ch, c["charge"])
    finally:
        dv.close()


def _second_step(km, oracle, dv):
    """asym's site arrays beside whatever list dv holds, one step, against asym's oracle"""
    c, ref = G.case("asym"), G.reference(oracle, "asym")
    dv.load(c)
    rng = km.solvers.RandomNumberGenerator(c["seed"])
    _same(oracle, dv, dv.step(rng), ref, rng)


def test_verdict_cache_list_changed_in_place(km, oracle):
    """One communicator, one device tensor: a step on local7's (symmetric) list, then asym's list copied into the SAME tensor.
    The symmetry verdict is kept per address (include/kmcfield.h, kmcf_execute_kmc_step): kmcf_events_reset between the two
    drops it, and the second step takes the full pass the list needs."""
    c = G.case("local7")
    dv = _Dev(km, c)
    try:
        rng = km.solvers.RandomNumberGenerator(c["seed"])
        _same(oracle, dv, dv.step(rng), G.reference(oracle, "local7"), rng)
        addr = dv.neigh.data_ptr()
        dv.neigh.copy_(dv.i32(G.case("asym")["neigh"].reshape(-1)))
        assert dv.neigh.data_ptr() == addr
        km.solvers.events_reset(dv.comm)
        _second_step(km, oracle, dv)
    finally:
        dv.close()


def test_one_communicator_through_every_path(km, oracle, monkeypatch):
    """ONE communicator whose workspace changes shape and path between steps (every other test opens a fresh one per case).
    ring7_7001 and nn70 have the same N: the persistent path (its tree and pinned block are allocated), nn70 (nn changes:
    the cache is rebuilt; nn > 63: three launches, their device batch buffers), then ring7_7001 on the full pass, on three
    launches and on the persistent path again -- a workspace that holds the buffers of all three paths --, and once more
    after kmcf_events_reset.  Every step against oracle.kmc_step."""
    ring, wide = G.case("ring7_7001"), G.case("nn70")
    assert ring["N"] == wide["N"] and ring["nn"] <= G.NN_PERSISTENT < wide["nn"]
    dv = _Dev(km, ring)
    lists = {"ring7_7001": dv.neigh, "nn70": dv.i32(wide["neigh"].reshape(-1))}

    def step(name, knob=None):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        if knob:
            monkeypatch.setenv(*knob)
        c = G.case(name)
        dv.neigh = lists[name]
        dv.load(c)
        rng = km.solvers.RandomNumberGenerator(c["seed"])
        _same(oracle, dv, dv.step(rng), G.reference(oracle, name), rng)

    try:
        step("ring7_7001")
        step("nn70")
        step("ring7_7001", ("KMCF_EVENTS_FULLSCAN", "1"))
        step("ring7_7001", ("KMCF_EVENTS_PERSISTENT", "0"))
        step("ring7_7001")
        km.solvers.events_reset(dv.comm)
        step("ring7_7001")
    finally:
        dv.close()


def test_verdict_cache_list_at_another_address(km, oracle):
    """... and asym's list in a new tensor while the old one is alive: another address, a fresh verdict by itself."""
    c = G.case("local7")
    dv = _Dev(km, c)
    try:
        rng = km.solvers.RandomNumberGenerator(c["seed"])
        _same(oracle, dv, dv.step(rng), G.reference(oracle, "local7"), rng)
        old = dv.neigh
        dv.neigh = dv.i32(G.case("asym")["neigh"].reshape(-1))
        assert dv.neigh.data_ptr() != old.data_ptr()
        _second_step(km, oracle, dv)
    finally:
        dv.close()
