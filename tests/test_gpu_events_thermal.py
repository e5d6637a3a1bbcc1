"""GPU: thermally coupled event rates (kmcf_event_rates, kmcf_execute_kmc_step_thermal) against the
numpy restatement tests/events_thermal_ref.py, whose agreement with the C oracle tests/test_events_thermal.py holds.

The workload of the rate and sequence tests is the hot spot of test_events_thermal.py::test_hot_spot_workload_conditions
(structure.synth_small(tiles=1), potentials of the oracle's K solve plus the pairwise term, T_bg 300 K, a 2000 K spot in
the oxide): that test shows on the restatement alone that the thermal logs leave the T_BG log within three events and that
no selection lies within 1e-9 of a slot boundary, so the device must reproduce the restatement's log exactly.

Rates.  Measured on an MI355X on this workload (printed by test_rates_match_the_restatement): the largest relative
difference between the device's and numpy's rates in KMCF_RATE_T_BG -- the arithmetic the thermal modes leave
unchanged -- is what exp, erfc and sqrt of the two sides round differently, scaled by the exponent's size; the thermal
modes are held to four times that figure, whatever it is (nothing is fixed in advance)."""
import threading

import numpy as np
import pytest

import events_thermal_ref as R

pytestmark = pytest.mark.gpu

MODES = {"ekin": R.EKIN, "site": R.T_SITE}


@pytest.fixture(scope="module")
def small(km, oracle):
    w = R.small_workload(km, oracle)
    w["ref"] = {}
    return w


def _ref_step(oracle, w, mode, T=None, T_bg=None, max_events=None):
    """the restatement's step (cached per mode on the hot spot)"""
    d = w["d"]
    key = mode if T is None else None
    if key is not None and key in w["ref"]:
        return w["ref"][key]
    cap = max_events or w["max_events"]
    u = oracle.mt_uniform_stream(w["seed"], 2 * cap)
    out = R.kmc_step(d["xyz"], w["neigh"], w["lay"], w["T_bg"] if T_bg is None else T_bg, w["freq"], d["sigma"], d["k"], w["pot"],
                     d["element"], w["charge"], w["layers"], u, T=w["T_hot"] if T is None else T, mode=mode, max_events=cap)
    if key is not None:
        w["ref"][key] = out
    return out


class _Dev:
    """One rank's device copy of a workload dict(d, neigh, charge, lay, pot, layers)."""

    def __init__(self, km, w, comm=None):
        import torch
        self.km, self.w, self.S = km, w, km.solvers
        d = w["d"]
        self.N = d["N"]
        self.own = comm is None
        if comm is None:
            comm = self.S.KMC_comm(self.N - 2 * d["N_contact"], self.N + 1, self.N, self.N)
            comm.connect()
        self.comm = comm
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.f64 = f64
        r0, nr = int(comm.displs_events[comm.rank_events]), int(comm.counts_events[comm.rank_events])
        self.rows = slice(r0, r0 + nr)
        self.neigh = i32(np.asarray(w["neigh"])[self.rows].reshape(-1))          # this rank's count * nn slots
        self.lay, self.pot = i32(w["lay"]), f64(w["pot"])
        self.x, self.y, self.z = (f64(d["xyz"][:, q]) for q in range(3))
        self.reset()

    def reset(self):
        import torch
        d = self.w["d"]
        self.el = torch.as_tensor(np.ascontiguousarray(d["element"], dtype=np.int32), device="cuda")
        self.ch = torch.as_tensor(np.ascontiguousarray(self.w["charge"], dtype=np.int32), device="cuda")

    def _args(self, T_bg):
        w, d, c = self.w, self.w["d"], self.comm
        return (c, self.N, c.counts_events, c.displs_events, 52, self.neigh, self.lay, T_bg, w["freq"], d["sigma"], d["k"],
                self.x, self.y, self.z, self.pot, self.el, self.ch)

    def rates(self, mode, T=None, T_bg=None):
        return self.S.event_rates(*self._args(self.w["T_bg"] if T_bg is None else T_bg), self.w["layers"],
                                  site_temperature=None if T is None else self.f64(T), rate_mode=mode)

    def step(self, rng, mode=None, T=None, T_bg=None, max_events=None):
        """mode None: kmcf_execute_kmc_step as before this feature"""
        kw = {} if mode is None else dict(site_temperature=None if T is None else self.f64(T), rate_mode=mode)
        return self.S.execute_kmc_step_mpi(*self._args(self.w["T_bg"] if T_bg is None else T_bg), rng, self.w["layers"],
                                           max_events=max_events or self.w["max_events"], return_log=True, **kw)

    def state(self):
        return self.el.cpu().numpy(), self.ch.cpu().numpy()

    def close(self):
        if self.own:
            self.comm.close()


@pytest.fixture(scope="module")
def dev_small(km, small):
    dv = _Dev(km, small)
    yield dv
    dv.close()


def _rel_err(got, want):
    live = want > 0
    assert np.array_equal(got == 0, want == 0)
    return float((np.abs(got[live] - want[live]) / want[live]).max())


def _rate_bar(dv, w):
    """Largest relative rate error of KMCF_RATE_T_BG against the restatement: the bar of the thermal modes is 4 x this."""
    d = w["d"]
    dv.reset()                           # (steps of earlier tests have executed events on the device copy)
    typ, prob = dv.rates("bg")
    t0, p0, _ = R.event_list(d["xyz"], w["neigh"], w["lay"], w["T_bg"], w["freq"], d["sigma"], d["k"], w["pot"], d["element"],
                             w["charge"], w["layers"])
    assert np.array_equal(typ, t0)
    return _rel_err(prob, p0)


def test_rates_match_the_restatement(km, small, dev_small):
    w, d, dv = small, small["d"], dev_small
    err0 = _rate_bar(dv, w)
    print("event rates, hot-spot workload: %d live slots; largest relative error KMCF_RATE_T_BG %.3e" % (
        int((dv.rates("bg")[0] != R.EV_NULL).sum()), err0))
    for name, mode in MODES.items():
        typ, prob = dv.rates(name, T=w["T_hot"])
        t1, p1, _ = R.event_list(d["xyz"], w["neigh"], w["lay"], w["T_bg"], w["freq"], d["sigma"], d["k"], w["pot"], d["element"],
                                 w["charge"], w["layers"], T=w["T_hot"], mode=mode)
        assert typ.shape == (d["N"], 52) and np.array_equal(typ, t1)
        err = _rel_err(prob, p1)
        print("  mode %-4s: largest relative error %.3e (bar 4 x %.3e)" % (name, err, err0))
        assert err <= 4 * err0
        assert not np.array_equal(prob, dv.rates("bg")[1])               # the field is read
    assert np.array_equal(dv.rates(2, T=w["T_hot"])[1], dv.rates("site", T=w["T_hot"])[1])      # 0 / 1 / 2 are accepted too


def test_uniform_field_is_bit_identical_to_t_bg(km, oracle, small, dev_small):
    """T == T_bg everywhere: EA - kB * 0 and kB * T_bg are the T_BG operands, so both thermal modes give its bits -- the
    rates, and a step that is kmcf_execute_kmc_step's in every output."""
    w, dv = small, dev_small
    S = km.solvers
    T = np.full(w["d"]["N"], w["T_bg"])
    t0, p0 = dv.rates("bg")
    for name in MODES:
        t1, p1 = dv.rates(name, T=T)
        assert np.array_equal(t1, t0) and np.array_equal(p1, p0)
    dv.reset()
    rng = S.RandomNumberGenerator(w["seed"])
    base = dv.step(rng)
    el0, ch0 = dv.state()
    nxt0 = rng.getRandomNumber()
    assert base[1] >= 100
    for name, field in (("bg", T), ("ekin", T), ("site", T)):       # (all three through kmcf_execute_kmc_step_thermal)
        dv.reset()
        rng = S.RandomNumberGenerator(w["seed"])
        t, n, log = dv.step(rng, mode=name, T=field)
        el, ch = dv.state()
        assert n == base[1] and np.array_equal(log, base[2]) and t == base[0]
        assert np.array_equal(el, el0) and np.array_equal(ch, ch0)
        assert rng.getRandomNumber() == nxt0


def test_uniform_t_site_matches_the_oracle_5nm(km, oracle, dev5, ref5):
    """Mode 2 with T == 600 K and T_bg = 300 K is the oracle's step at 600 K (7 events; 3 at 300 K)."""
    d = dev5
    NL = d["N_contact"]
    pot = oracle.poisson_gridless(d["xyz"], ref5["charge"], d["sigma"], d["k"])
    pot[NL:NL + ref5["ks"].n] += ref5["x"]
    layers = km.structure.LAYERS
    w = dict(d=d, neigh=ref5["neigh"], charge=ref5["charge"], lay=km.solvers.site_layers(d["xyz"][:, 0], layers), pot=pot,
             layers=layers, T_bg=300.0, freq=10e13, seed=1, max_events=4096)
    t_o, n_o, log_o, el_o, ch_o = oracle.kmc_step(d["xyz"], w["neigh"], w["lay"], 600.0, w["freq"], d["sigma"], d["k"], pot,
                                                  d["element"], w["charge"], layers, oracle.mt_state(1), max_events=4096)
    assert n_o == 7
    dv = _Dev(km, w)
    try:
        rng = km.solvers.RandomNumberGenerator(1)
        t, n, log = dv.step(rng, mode="site", T=np.full(d["N"], 600.0))
        el, ch = dv.state()
        assert n == n_o and np.array_equal(log, log_o)
        assert np.array_equal(el, el_o) and np.array_equal(ch, ch_o)
        assert t == pytest.approx(t_o, rel=1e-12)
        assert rng.getRandomNumber() == oracle.mt_uniform_stream(1, 2 * n + 1)[-1]
        dv.reset()
        assert dv.step(km.solvers.RandomNumberGenerator(1))[1] == 3
    finally:
        dv.close()


def _check_against_ref(ref, got, state):
    t_r, n_r, log_r, el_r, ch_r, _ = ref
    t, n, log = got
    assert n == n_r and np.array_equal(log, log_r)
    assert np.array_equal(state[0], el_r) and np.array_equal(state[1], ch_r)
    assert t == pytest.approx(t_r, rel=1e-12)


@pytest.mark.parametrize("path", ["default", "fullscan", "callback", "three_launches"])
@pytest.mark.parametrize("name", ["ekin", "site"])
def test_hot_spot_event_sequence(km, oracle, small, dev_small, name, path, monkeypatch):
    """Same potentials, same field, same generator state in: the restatement's (i, j, type) log, final element / charge
    state, event time to 1e-12, two draws per event -- on every path of the event loop behind the build kernel."""
    w, dv = small, dev_small
    monkeypatch.delenv("KMCF_EV_TREL", raising=False)
    monkeypatch.delenv("KMCF_EVENTS_PERSISTENT", raising=False)
    monkeypatch.delenv("KMCF_EVENTS_FULLSCAN", raising=False)
    if path == "fullscan":
        monkeypatch.setenv("KMCF_EVENTS_FULLSCAN", "1")
    if path == "three_launches":
        monkeypatch.setenv("KMCF_EVENTS_PERSISTENT", "0")
    ref = _ref_step(oracle, w, MODES[name])
    assert 100 <= ref[1] < w["max_events"] and ref[5].min() > 1e-9
    dv.reset()
    rng = km.solvers.RandomNumberGenerator(w["seed"])
    got = dv.step(rng.getRandomNumber if path == "callback" else rng, mode=name, T=w["T_hot"])
    _check_against_ref(ref, got, dv.state())
    assert got[0] >= 1 / w["freq"]
    assert rng.getRandomNumber() == oracle.mt_uniform_stream(w["seed"], 2 * got[1] + 1)[-1]


@pytest.mark.parametrize("name", ["ekin", "site"])
@pytest.mark.parametrize("partitioned", [False, True])
def test_rank_group_gives_the_one_rank_log(km, oracle, small, dev_small, partitioned, name, monkeypatch):
    """Two ranks in one process (loopback transport): replicated (every rank runs the whole list on the whole-device
    field) and with KMCF_EVENTS_PARTITIONED=1 (a rank's slots read T at global site ids): the restatement's log, that
    is the one rank's (test_hot_spot_event_sequence), on both ranks."""
    import torch
    w, d = small, small["d"]
    if partitioned:
        monkeypatch.setenv("KMCF_EVENTS_PARTITIONED", "1")
    else:
        monkeypatch.delenv("KMCF_EVENTS_PARTITIONED", raising=False)
    monkeypatch.delenv("KMCF_EVENTS_FULLSCAN", raising=False)
    monkeypatch.delenv("KMCF_EVENTS_PERSISTENT", raising=False)
    P = 2
    ref = _ref_step(oracle, w, MODES[name])
    bar = 4 * _rate_bar(dev_small, w)                   # the one-rank tests' bar (test_rates_match_the_restatement)
    comms = km.solvers.KMC_comm.loopback_group(d["N"] - 2 * d["N_contact"], d["N"] + 1, d["N"], d["N"], size=P, device=0)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comms[r].connect()
            dv = _Dev(km, w, comm=comms[r])
            typ, prob = dv.rates(name, T=w["T_hot"])
            rng = km.solvers.RandomNumberGenerator(w["seed"])
            got = dv.step(rng, mode=name, T=w["T_hot"])
            out[r] = dict(got=got, state=dv.state(), nxt=rng.getRandomNumber(), typ=typ, prob=prob, rows=dv.rows)
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish"
    for c in comms:
        c.close()
    t1, p1, _ = R.event_list(d["xyz"], w["neigh"], w["lay"], w["T_bg"], w["freq"], d["sigma"], d["k"], w["pot"], d["element"],
                             w["charge"], w["layers"], T=w["T_hot"], mode=MODES[name])
    for o in out:
        _check_against_ref(ref, o["got"], o["state"])
        assert o["nxt"] == oracle.mt_uniform_stream(w["seed"], 2 * ref[1] + 1)[-1]
        assert np.array_equal(o["typ"], t1[o["rows"]])                      # kmcf_event_rates: this rank's rows
        assert _rel_err(o["prob"], p1[o["rows"]]) <= bar                    # (a rank's slots read T at GLOBAL site ids)
    assert out[0]["rows"].stop == out[1]["rows"].start and out[1]["rows"].stop == d["N"]


def test_unusable_temperature_is_refused_before_any_event(km, oracle, small, dev_small):
    """One zero in the field, at a site that owns a non-null event: KMCF_ERR_ARG naming it; site arrays and generator
    untouched.  The same zero at a site without events is not looked at."""
    w, dv = small, dev_small
    S = km.solvers
    d = w["d"]
    _, _, site = R.event_list(d["xyz"], w["neigh"], w["lay"], w["T_bg"], w["freq"], d["sigma"], d["k"], w["pot"], d["element"],
                              w["charge"], w["layers"], T=w["T_hot"], mode=R.T_SITE)
    owners = np.unique(site[site >= 0])
    idle = np.setdiff1d(np.arange(d["N"]), owners)
    assert len(owners) > 2 and len(idle) > 0
    for bad_value in (0.0, -1.0, float("nan"), float("inf")):
        for name in MODES:
            T = w["T_hot"].copy()
            T[owners[len(owners) // 2]] = bad_value
            T[owners[-1]] = bad_value                                 # the FIRST such site is named
            dv.reset()
            rng = S.RandomNumberGenerator(w["seed"])
            with pytest.raises(km.lib.KmcfError) as e:
                dv.step(rng, mode=name, T=T)
            assert "(-1)" in str(e.value) and "site %d " % owners[len(owners) // 2] in str(e.value), str(e.value)
            el, ch = dv.state()
            assert np.array_equal(el, d["element"]) and np.array_equal(ch, w["charge"])
            assert rng.getRandomNumber() == S.RandomNumberGenerator(w["seed"]).getRandomNumber()
            with pytest.raises(km.lib.KmcfError):
                dv.rates(name, T=T)
    T = w["T_hot"].copy()
    T[idle] = 0.0
    dv.reset()
    assert dv.step(S.RandomNumberGenerator(w["seed"]), mode="site", T=T)[1] == _ref_step(oracle, w, R.T_SITE)[1]
    T[owners[0]] = 0.0
    dv.reset()
    assert dv.step(S.RandomNumberGenerator(w["seed"]), mode="bg", T=T)[1] >= 1     # mode 0 never reads the field


def test_electro_thermal_chain(km, oracle, small, dev_small):
    """The whole chain on one rank, conducting 4 x 4 crossbar (the device of tests/test_gpu_conducting.py): charge, K
    solve, pairwise, gather -> CB edge -> power with heating -> local heat solve (steady state) -> a thermal step in
    KMCF_RATE_T_SITE on the solved field.  The field is not flat; the restatement, fed with the downloaded potential,
    temperature, element and charge, gives the same 32 events and the same rates."""
    import torch
    import test_gpu_conducting as TC
    S = km.solvers
    dev = TC._device(km, 4.0)
    d, buf, comm = dev["d"], dev["buf"], dev["comm"]
    N, NL = d["N"], d["N_contact"]
    layers = km.structure.LAYERS
    try:
        S.compute_cutoff_list(comm, buf, 20.0)
        st = S.background_potential_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"], len(d["metals"]), 0)
        assert st["converged"] == 1
        S.poisson_gridless_gpu(buf, comm)
        S.sum_and_gather_potential(buf, NL, comm)
        im, il, st_t, info, bound = TC._current(dev, 1e-15, first=True, touch_env=False)       # CB edge, then power with heating
        assert st_t["converged"] == 1 and im > 0 and float(buf.site_power.max()) > 0
        T0 = 300.0
        prm = S.heat_params(background_temp=T0, A=(4 * 51.15e-10) ** 2, cg_tolerance=1e-13, cg_max_iterations=50000)
        res = S.update_temperature_local_gpu(buf, N, NL, NL, 1e-6, prm)
        assert res["steady"] and res["stats"]["converged"] == 1
        T = buf.site_temperature.cpu().numpy().copy()
        print("chain: I_macro %.4e, max power %.3e W, field %.3f .. %.3f K" % (im, float(buf.site_power.max()), T.min(), T.max()))
        assert np.all(np.isfinite(T)) and T[NL:-NL].max() > T0 and T.min() > 0
        pot = buf.site_potential_charge.cpu().numpy().copy()
        el0, ch0 = buf.site_element.cpu().numpy().copy(), buf.site_charge.cpu().numpy().copy()
        neigh = buf.neigh_idx.cpu().numpy().reshape(N, 52)
        xs = np.clip(d["xyz"][:, 0], layers[0]["start_x"], layers[-1]["end_x"])
        lay = S.site_layers(xs, layers)
        freq, cap = 10e13, 32
        u = oracle.mt_uniform_stream(1, 2 * cap)
        ref = R.kmc_step(d["xyz"], neigh, lay, T0, freq, d["sigma"], d["k"], pot, el0, ch0, layers, u, T=T, mode=R.T_SITE, max_events=cap)
        assert ref[1] == cap and ref[5].min() > 1e-9, (ref[1], ref[5].min())
        lay_d = torch.as_tensor(lay, device="cuda")
        args = (comm, N, comm.counts_events, comm.displs_events, 52, buf.neigh_idx, lay_d, T0, freq, d["sigma"], d["k"], buf.site_x,
                buf.site_y, buf.site_z, buf.site_potential_charge, buf.site_element, buf.site_charge)
        # rates on the solved field, within the bar measured on the hot-spot workload's unchanged arithmetic
        # (test_rates_match_the_restatement)
        t1, p1, _ = R.event_list(d["xyz"], neigh, lay, T0, freq, d["sigma"], d["k"], pot, el0, ch0, layers, T=T, mode=R.T_SITE)
        t0, p0, _ = R.event_list(d["xyz"], neigh, lay, T0, freq, d["sigma"], d["k"], pot, el0, ch0, layers)
        typ0, prob0 = S.event_rates(*args, layers)
        typ, prob = S.event_rates(*args, layers, site_temperature=buf.site_temperature, rate_mode="site")
        assert np.array_equal(typ0, t0) and np.array_equal(typ, t1)
        bar, err0, err = _rate_bar(dev_small, small), _rel_err(prob0, p0), _rel_err(prob, p1)
        print("chain: largest relative rate error KMCF_RATE_T_BG %.3e, KMCF_RATE_T_SITE %.3e (bar 4 x %.3e, hot-spot workload)" % (err0, err, bar))
        assert err <= 4 * bar
        rng = S.RandomNumberGenerator(1)
        got = S.execute_kmc_step_mpi(*args, rng, layers, max_events=cap, return_log=True, site_temperature=buf.site_temperature,
                                     rate_mode="site")
        assert got[1] == cap and np.array_equal(got[2], ref[2])
        assert np.array_equal(buf.site_element.cpu().numpy(), ref[3]) and np.array_equal(buf.site_charge.cpu().numpy(), ref[4])
        assert got[0] == pytest.approx(ref[0], rel=1e-12)
        assert rng.getRandomNumber() == oracle.mt_uniform_stream(1, 2 * cap + 1)[-1]
    finally:
        buf.freeGPUmemory()
        comm.close()
