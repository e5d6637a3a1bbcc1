"""CPU: the restatement the thermal event step is held to (tests/events_thermal_ref.py) against the C oracle, the
conditions that keep the GPU sequence test meaningful, and the argument errors of the two new entry points (reached on
a host-only communicator: they are checked before anything needs a device)."""
import ctypes as C

import numpy as np
import pytest

import events_thermal_ref as R


@pytest.fixture(scope="module")
def fields5(oracle, dev5, ref5):
    d = dev5
    NL = d["N_contact"]
    pot = oracle.poisson_gridless(d["xyz"], ref5["charge"], d["sigma"], d["k"])
    pot[NL:NL + ref5["ks"].n] += ref5["x"]
    return pot


@pytest.fixture(scope="module")
def work5(km, dev5, ref5, fields5):
    layers = km.structure.LAYERS
    return dict(d=dev5, neigh=ref5["neigh"], charge=ref5["charge"], lay=km.solvers.site_layers(dev5["xyz"][:, 0], layers),
                pot=fields5, layers=layers)


@pytest.fixture(scope="module")
def small(km, oracle):
    return R.small_workload(km, oracle)


def _oracle_step(oracle, w, T_bg, layers=None, seed=1, freq=1e14, max_events=4096):
    d = w["d"]
    return oracle.kmc_step(d["xyz"], w["neigh"], w["lay"], T_bg, freq, d["sigma"], d["k"], w["pot"], d["element"],
                           w["charge"], layers or w["layers"], oracle.mt_state(seed), max_events=max_events)


def _ref_step(oracle, w, T_bg, T=None, mode=R.T_BG, seed=1, freq=1e14, max_events=4096):
    d = w["d"]
    u = oracle.mt_uniform_stream(seed, 2 * max_events)
    return R.kmc_step(d["xyz"], w["neigh"], w["lay"], T_bg, freq, d["sigma"], d["k"], w["pot"], d["element"], w["charge"],
                      w["layers"], u, T=T, mode=mode, max_events=max_events)


def _same(ref, orc):
    t, n, log, el, ch, _ = ref
    t_o, n_o, log_o, el_o, ch_o = orc
    assert n == n_o and np.array_equal(log, log_o)
    assert np.array_equal(el, el_o) and np.array_equal(ch, ch_o)
    assert t == pytest.approx(t_o, rel=1e-14)


@pytest.mark.parametrize("which,T,events", [("5nm", 77.0, 2), ("5nm", 300.0, 3), ("5nm", 600.0, 7),
                                            ("small", 77.0, 267), ("small", 300.0, 294), ("small", 600.0, 337)])
def test_restatement_reproduces_the_oracle(oracle, work5, small, which, T, events):
    """Uniform field: every mode of the restatement is the oracle's step at that temperature."""
    w = work5 if which == "5nm" else small
    orc = _oracle_step(oracle, w, T)
    assert orc[1] == events
    _same(_ref_step(oracle, w, T), orc)
    N = w["d"]["N"]
    _same(_ref_step(oracle, w, T, T=np.full(N, T), mode=R.EKIN), orc)          # T[s] == T_bg: Ekin = 0
    _same(_ref_step(oracle, w, 300.0, T=np.full(N, T), mode=R.T_SITE), orc)    # T_bg plays no part in T_SITE


@pytest.mark.parametrize("which,dT", [("5nm", 300.0), ("small", 150.0)])
def test_ekin_with_a_uniform_field_lowers_every_layer_energy(oracle, work5, small, which, dT):
    """EKIN, T = T_bg + dT everywhere: EA - kB dT in every branch = the oracle with every layer energy lowered by kB dT."""
    w = work5 if which == "5nm" else small
    lowered = [dict(l, **{key: l[key] - R.KB * dT for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")}) for l in w["layers"]]
    orc = _oracle_step(oracle, w, 300.0, layers=lowered)
    ref = _ref_step(oracle, w, 300.0, T=np.full(w["d"]["N"], 300.0 + dT), mode=R.EKIN)
    assert ref[1] >= 1 and ref[5].min() > 1e-9        # (E - kB dT - Eg against E - Eg - kB dT: an ulp apart, far from any boundary)
    _same(ref, orc)
    assert orc[0] != _oracle_step(oracle, w, 300.0)[0]                         # ... and the term changes the rates


def test_hot_spot_workload_conditions(oracle, small):
    """What the GPU sequence test (tests/test_gpu_events_thermal.py) relies on, asserted on the restatement alone: the
    thermal logs leave the T_BG log within the first three events, the step ends by itself, and no selection comes
    within 1e-9 (relative to the total rate) of a slot boundary -- rounding differences between device and numpy
    (exp, erfc, the order of the sums: ~1e-13 relative) cannot move a selection."""
    w = small
    assert w["d"]["N"] == 37650 and w["d"]["Vd"] == 15.0
    T = w["T_hot"]
    assert T.min() >= 300.0 and 1900.0 < T.max() <= 2000.0
    base = _ref_step(oracle, w, 300.0)
    for mode, name in ((R.EKIN, "EKIN"), (R.T_SITE, "T_SITE")):
        t, n, log, el, ch, margins = _ref_step(oracle, w, 300.0, T=T, mode=mode)
        m = min(n, base[1])
        diff = np.flatnonzero((log[:m] != base[2][:m]).any(axis=1))
        first = int(diff[0]) if len(diff) else m
        print("%s: %d events, first difference from the T_BG log at event %d, smallest margin %.2e" % (name, n, first, margins.min()))
        assert first < 3
        assert 1 <= n < w["max_events"] and t >= 1 / w["freq"]
        assert margins.min() > 1e-9
    assert base[5].min() > 1e-9


# ---- argument errors: KMCF_ERR_ARG before the host-only-communicator check -------------------------------------------

ERR_ARG, ERR_STATE = -1, -4


def _host_comm(km):
    h = C.c_void_p()
    km.lib.check(km.lib.load().kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    return h


def _step_args(h, T_bg=300.0):
    """Well-formed arguments of kmcf_execute_kmc_step for a host-only communicator.  The device pointers are never
    dereferenced: every call here returns from the argument checks or from the host-only check behind them."""
    ip = lambda n: (C.c_int * n)()
    dp = lambda n: (C.c_double * n)()
    fake = C.c_void_p(64)
    cnt, dsp = ip(1), ip(1)
    cnt[0] = 4
    t, nev = C.c_double(-1.0), C.c_int(-1)
    keep = (cnt, dsp, dp(5), dp(5), dp(5), dp(5), t, nev)
    return keep, [h, 4, cnt, dsp, 52, fake, fake, T_bg, 1e14, 3.5e-10, 1.0, fake, fake, fake, fake, fake, fake,
                  5, keep[2], keep[3], keep[4], keep[5]]


@pytest.mark.parametrize("mode,field,T_bg,want,word", [
    (3, True, 300.0, ERR_ARG, b"rate_mode"), (-1, True, 300.0, ERR_ARG, b"rate_mode"),
    (1, False, 300.0, ERR_ARG, b"d_site_temperature"), (2, False, 300.0, ERR_ARG, b"d_site_temperature"),
    (0, True, 0.0, ERR_ARG, b"T_bg"), (2, True, -5.0, ERR_ARG, b"T_bg"), (1, True, float("nan"), ERR_ARG, b"T_bg"),
    (0, False, 300.0, ERR_STATE, b"host-only"), (1, True, 300.0, ERR_STATE, b"host-only"), (2, True, 300.0, ERR_STATE, b"host-only")])
def test_thermal_argument_errors_on_a_host_only_communicator(km, mode, field, T_bg, want, word):
    lib = km.lib.load()
    h = _host_comm(km)
    try:
        T = C.c_void_p(64) if field else None
        keep, a = _step_args(h, T_bg)
        rng = km.solvers.RandomNumberGenerator(1)
        fn = C.cast(lib.kmcf_rng_next, C.c_void_p)
        rc = lib.kmcf_execute_kmc_step_thermal(*a, fn, rng.handle, 16, C.byref(keep[6]), C.byref(keep[7]), None, T, mode)
        assert rc == want and word in lib.kmcf_last_error(), (rc, lib.kmcf_last_error())
        assert b"kmcf_execute_kmc_step_thermal" in lib.kmcf_last_error()
        assert rng.getRandomNumber() == km.solvers.RandomNumberGenerator(1).getRandomNumber()      # nothing drawn
        rc = lib.kmcf_event_rates(*a, T, mode, None, None)
        assert rc == want and word in lib.kmcf_last_error(), (rc, lib.kmcf_last_error())
        assert b"kmcf_event_rates" in lib.kmcf_last_error()
    finally:
        lib.kmcf_comm_destroy(h)


def test_python_rate_mode_names(km):
    S = km.solvers
    assert S.RATE_MODES == {"bg": 0, "ekin": 1, "site": 2}
    assert [S._rate_mode(m) for m in ("bg", "ekin", "site", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    with pytest.raises(ValueError):
        S._rate_mode("hot")
