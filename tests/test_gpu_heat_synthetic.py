"""GPU: the local heat solve (kmcf_update_temperature_local) off the 5 nm fixture, on the synthetic devices of
tests/site_kernels_ref.py, against the value-by-value restatement of its system (heat_local_ref.heat_values_ref: integer
class counts in np.longdouble) and scipy's direct solve (tests/test_heat_local.py asserts what the inputs are built for).

  * assembly on BOTH walks (the tiles of the coded window plan; row-wise after KMCF_SPMV_CODED=0 + replan), which one ran
    read from the library: off-diagonals bit-equal to the reference, diag / 1/diag / rhs / left / right and the diagonal
    entries within 16 * 2^-53 (at most nine roundings on any path -- k L, count g, two adds per sum, C/dt's five, three
    adds, the division -- all terms positive), the two walks bit-equal to each other.  sparse x pbc 0 / 1 x five
    conductivity sets (3, 2, 2, 2 and 1 dictionary codes) x steady / transient; dense x the distinct and the all-equal set.
    Every compared assembly is the SECOND of two different ones on the same state.
  * long rows (KMCF_LONG_ROW below the longest row): the row-wise walk with value codes present, for the heat system
    and, in the same state, for K and the band edge.
  * solution and bookkeeping of every such call: 1e-8 of the heating against the direct solve, converged, the interface
    mean, the energy balance, the contacts at T0 whatever the caller left there; a step of length 0.
  * the mode switch at step_time == 1e3 delta_t exactly, a sequence of dictionaries of 3, 2, 1, 3 codes on one state
    followed by a K solve, and rank groups of 2 and 3 with uneven partitions (each rank's rows bit-equal to one rank's).

Every test builds and frees its own communicators and buffers."""
import contextlib
import threading
import time

import numpy as np
import pytest

import heat_local_ref as H
import site_kernels_ref as R
from test_gpu_heat_local import _same_solve
from test_gpu_site_kernels import _check_system as _check_k_system

pytestmark = pytest.mark.gpu

BAR = 16 * 2.0 ** -53
VECTORS = ("diag", "dinv", "rhs", "left", "right")
OTHER_MODE = {"steady": "transient", "transient": "steady"}
PLAN_KNOBS = ("KMCF_SPMV_KIND", "KMCF_SPMV_CODED", "KMCF_SPMV_SELL", "KMCF_SPMV_SELL_ROWS", "KMCF_SPMV_SELLV", "KMCF_CB_SCALED",
              "KMCF_LONG_ROW", "KMCF_CG_RESIDENT")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture
def clean_env(monkeypatch):
    for key in PLAN_KNOBS:
        monkeypatch.delenv(key, raising=False)
    return monkeypatch


def _dev_i32(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.int32), device="cuda")       # (a copy: the inputs are read-only)


@contextlib.contextmanager
def _state(km, torch, name, pbc, comm=None, options=None):
    """A K state of a k_device with the charges of dev["charge"]; the communicator is made (and closed) here unless given."""
    S = km.solvers
    dev = R.k_device(name)
    N, NL, n = dev["N"], dev["NL"], dev["n"]
    xyz = dev["xyz"]
    own = comm is None
    if own:
        comm = S.KMC_comm(n, N + 1, N, N, options=options)
        comm.connect()
    buf = None
    try:
        # (copies: the devices are read-only; sigma and k belong to the pairwise term, which nothing here runs)
        buf = S.GPUBuffers(N, np.array(dev["element"]), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]),
                           R.K_CHARGE_NN, 1.0, 1.0, dev["lattice"], dev["metals"])
        S.initialize_sparsity_K(buf, pbc, R.K_NN_DIST, NL, comm)
        st = dict(buf=buf, comm=comm, dev=dev, name=name, pbc=pbc, charge=_dev_i32(torch, dev["charge"]),
                  charge2=_dev_i32(torch, dev["charge2"]),
                  mat=S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed)))
        buf.site_charge.copy_(st["charge"])
        yield st
    finally:
        if buf is not None:
            buf.freeGPUmemory()
        if own:
            comm.close()


def _heat(km, torch, st, p, step_time):
    """one call with the caller's arrays set afresh (the contacts of T_old hold a sentinel): (T, result)"""
    dev, buf = st["dev"], st["buf"]
    _, _, Q, T_old = H.synth_inputs(st["name"])
    buf.site_power = torch.as_tensor(np.array(Q), device=buf.device)
    buf.site_temperature = torch.as_tensor(np.array(T_old), device=buf.device)
    prm = km.solvers.heat_params(**p, **H.SYNTH_CG)
    res = km.solvers.update_temperature_local_gpu(buf, dev["N"], dev["NL"], dev["NL"], step_time, prm)
    return buf.site_temperature.cpu().numpy().copy(), res


def _second_of_two(km, torch, st, kset, mode, prior):
    """The call that counts, after a DIFFERENT assembly on the same state: a heat call on charge2 with another
    conductivity set in the other mode (prior == "heat"), or K's assembly on charge2.  Returns (T, result, vectors)."""
    S, buf, dev = km.solvers, st["buf"], st["dev"]
    buf.site_charge.copy_(st["charge2"])
    if prior == "heat":
        other = "all_equal" if kset == "distinct" else "distinct"
        _heat(km, torch, st, H.synth_params(other), H.SYNTH_STEP[OTHER_MODE[mode]])
    else:
        S.k_assemble(buf, dev["Vd"], dev["high_G"], dev["low_G"])
    buf.site_charge.copy_(st["charge"])
    T, res = _heat(km, torch, st, H.synth_params(kset), H.SYNTH_STEP[mode])
    return T, res, S.k_vectors(buf)


def _walk(st):
    """which assembly walk the library takes on this state now, from what it reports (kmcf_update_temperature_local:
    tiles when the matrix runs a coded kernel and every row is short, else row-wise)"""
    info = st["mat"].info()
    n_short = st["mat"].row_order()[1]
    rows = info["rows_this_rank"]
    coded = info["spmv_coded"] >= 1
    walk = "tile" if (info["spmv_kind"] == 2 and coded and n_short == rows) else ("row+codes" if coded else "row")
    return walk, "spmv_kind %d, spmv_coded %d, %d of %d rows short" % (info["spmv_kind"], info["spmv_coded"], n_short, rows)


def _check_system(tag, kv, ref):
    """off-diagonals bit-equal, everything else within BAR of the long-double reference; the worst errors"""
    off = ref["off_diagonal"]
    worst = {key: H.rel_error(kv[key], ref[key]) for key in VECTORS}
    worst["val diagonal"] = H.rel_error(kv["val"][~off], ref["diag"][ref["rows"][~off]])
    wrong = int((kv["val"][off] != ref["val"][off]).sum())
    print("%s: largest relative error %s; %d of %d off-diagonals differ"
          % (tag, ", ".join("%s %.3g" % kv_ for kv_ in worst.items()), wrong, int(off.sum())))
    assert wrong == 0, "%s: %d off-diagonals differ" % (tag, wrong)
    for key, w in worst.items():
        assert w <= BAR, "%s %s: %.3g" % (tag, key, w)


def _check_solution(tag, name, case, T, res, T_bg):
    """the field against the direct solve and the call's bookkeeping (T_bg: what the wrapper left in the buffers)"""
    NL = R.k_device(name)["NL"]
    p, s, T_ref, step_time = case["p"], case["sys"], case["T"], case["step_time"]
    T0 = p["background_temp"]
    _, _, Q, T_old = H.synth_inputs(name)
    stt = res["stats"]
    dT = np.abs(T_ref - T0).max()
    err = np.abs(T - T_ref).max()
    Qi = Q[NL:-NL].sum()
    out = ((s["gL"] + s["gR"]) * (T - T0)[NL:-NL]).sum()
    stored = 0.0 if s["steady"] else (s["C"] * (T - T_old)[NL:-NL] / step_time).sum()
    print("%s: %d iterations, relres %.2e, assembly %.3f ms, solve %.3f ms, max dT %.4g K, |T - T_ref| = %.2g of it, "
          "energy balance %.2g of the power" % (tag, stt["iterations"], stt["relres"], stt["ms_assembly"], stt["ms_solve"], dT,
                                                err / dT, abs(stored + out - Qi) / Qi))
    assert res["steady"] == s["steady"] == case["ref"]["steady"]
    assert stt["converged"] == 1 and stt["iterations"] > 0
    assert np.all(T[:NL] == T0) and np.all(T[-NL:] == T0)              # the caller left a sentinel there
    assert err <= 1e-8 * dT
    assert res["Global temperature [K]"] == pytest.approx(T[NL:-NL].mean(), rel=1e-14)
    assert T_bg == res["Global temperature [K]"]
    assert abs(stored + out - Qi) <= 1e-9 * Qi, (stored, out, Qi)


def _same_patterns(km, st):
    pats = [km.solvers.k_pattern(st["buf"], which) for which in range(3)]
    for (rp, col), (rp_r, col_r) in zip(pats, H.synth_patterns(st["name"], st["pbc"])):
        assert np.array_equal(rp, rp_r) and np.array_equal(col, col_r)


# ------------------------------------------------------------------------------------------------ (a), (b), (d)
CASES_AB = [("sparse", pbc, k) for pbc in (0, 1) for k in H.HEAT_SETS] + \
           [("dense", pbc, k) for pbc in (0, 1) for k in ("distinct", "all_equal")]


@pytest.mark.parametrize("name,pbc,kset", CASES_AB)
def test_assembly_and_solution_on_both_walks(km, torch, clean_env, name, pbc, kset):
    t_start = time.perf_counter()
    got = {}
    with _state(km, torch, name, pbc) as st:
        _same_patterns(km, st)
        n = st["dev"]["n"]
        for walk in ("tile", "row"):
            if walk == "row":                                  # replanned without value codes: the row-wise kernel
                clean_env.setenv("KMCF_SPMV_CODED", "0")
                assert st["mat"].replan()["spmv_coded"] == 0
            for mode, prior in (("steady", "heat"), ("transient", "k")):
                case = H.synth_case(name, pbc, kset, mode)
                T, res, kv = _second_of_two(km, torch, st, kset, mode, prior)
                ran, why = _walk(st)
                tag = "%s pbc %d %s %s, %s walk (%s)" % (name, pbc, kset, mode, ran, why)
                assert ran == walk, tag
                _check_system(tag, kv, case["ref"])
                _check_solution(tag, name, case, T, res, float(st["buf"].T_bg.item()))
                got[walk, mode] = kv
            if walk == "tile":
                plan = st["mat"].sum_plan()
                assert plan["n_short"] == n and plan["long_items"] == 0
                ends, closed = R.window_tiles(plan["row_ptr"], plan["col"])
                print("   %d window tiles closed by %s" % (len(ends), {w: closed.count(w) for w in sorted(set(closed))}))
                if name == "dense":                            # tiles close at the entry limit, not at 64 rows
                    assert closed.count("entries") >= len(ends) // 2 and np.diff(np.r_[0, ends]).min() < 64
                else:
                    assert closed.count("rows") >= len(ends) // 2
    # the two walks: the same integer counts, the same additions, the same values
    for mode in ("steady", "transient"):
        for key in VECTORS + ("val",):
            assert np.array_equal(got["row", mode][key], got["tile", mode][key]), (mode, key)
    print("%s pbc %d %s: %.2f s" % (name, pbc, kset, time.perf_counter() - t_start))


# ------------------------------------------------------------------------------------------------ (c) long rows
LONG_ROW = 40


def test_long_rows_take_the_row_walk_with_codes_present(km, torch, clean_env):
    """Rows beyond KMCF_LONG_ROW sit behind the short ones and outside the tiles: the heat system, K and the band edge
    are then assembled row-wise INTO the value codes of the coded plan."""
    S = km.solvers
    name, pbc = "dense", 1
    t_start = time.perf_counter()
    clean_env.setenv("KMCF_LONG_ROW", str(LONG_ROW))
    with _state(km, torch, name, pbc) as st:
        _same_patterns(km, st)
        dev, buf = st["dev"], st["buf"]
        N, NL, n = dev["N"], dev["NL"], dev["n"]
        length = np.diff(H.synth_patterns(name, pbc)[0][0])
        for kset in ("distinct", "metal_eq_other"):
            for mode, prior in (("steady", "heat"), ("transient", "k")):
                case = H.synth_case(name, pbc, kset, mode)
                T, res, kv = _second_of_two(km, torch, st, kset, mode, prior)
                ran, why = _walk(st)
                plan = st["mat"].sum_plan(with_csr=False)
                tag = "long rows, %s %s, %s walk (%s, %d long-row items)" % (kset, mode, ran, why, plan["long_items"])
                assert ran == "row+codes", tag
                assert plan["n_short"] == int((length <= LONG_ROW).sum()) and 0 < plan["n_short"] < n and plan["long_items"] > 0
                _check_system(tag, kv, case["ref"])
                _check_solution(tag, name, case, T, res, float(st["buf"].T_bg.item()))
        # K and the band edge in the same corner, against k_values_ref with the bars of test_value_assembly_on_synthetic_devices
        pats = H.synth_patterns(name, pbc)
        Vd, hi, lo = dev["Vd"], dev["high_G"], dev["low_G"]
        ref = {cb: R.k_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], dev["element"], dev["charge"], dev["metals"],
                                  hi, lo, Vd, NL, n, cb) for cb in (False, True)}
        for ch in (st["charge2"], st["charge"]):
            buf.site_charge.copy_(ch)
            S.k_assemble(buf, Vd, hi, lo)
        assert _walk(st)[0] == "row+codes"
        _check_k_system("long rows, K, row-wise with codes", S.k_vectors(buf), ref[False])
        stt = S.update_CB_edge_gpu_sparse(buf, N, NL, NL, Vd, pbc, hi, lo, R.K_NN_DIST, len(dev["metals"]))
        print("   CB solve: %d iterations, %.2f ms" % (stt["iterations"], stt["ms_solve"]))
        assert _walk(st)[0] == "row+codes"                  # (a coded matrix: the band edge's values stay unscaled)
        _check_k_system("long rows, CB, row-wise with codes", S.k_vectors(buf), ref[True])
    print("long rows: %.2f s" % (time.perf_counter() - t_start))


# ------------------------------------------------------------------------------------------------ (d) a step of length 0
def test_zero_step_sets_the_contacts_and_nothing_else(km, torch, clean_env):
    """include/kmcfield.h: step_time == 0 assembles and solves nothing -- the interface slice comes back as it was, the
    contacts are set to background_temp all the same, the statistics are zero with converged = 1, and the state keeps
    the system it held."""
    name, pbc = "sparse", 0
    with _state(km, torch, name, pbc) as st:
        NL = st["dev"]["NL"]
        T_old = H.synth_inputs(name)[3]
        p = H.synth_params("distinct")
        _heat(km, torch, st, p, H.SYNTH_STEP["transient"])
        before = km.solvers.k_vectors(st["buf"])
        T, res = _heat(km, torch, st, H.synth_params("all_equal"), 0.0)
        after = km.solvers.k_vectors(st["buf"])
        assert not res["steady"] and res["stats"]["iterations"] == 0 and res["stats"]["converged"] == 1
        assert np.all(T_old[:NL] == H.SENTINEL) and np.all(T[:NL] == p["background_temp"]) and np.all(T[-NL:] == p["background_temp"])
        assert np.array_equal(T[NL:-NL], T_old[NL:-NL])
        assert res["Global temperature [K]"] == pytest.approx(T_old[NL:-NL].mean(), rel=1e-14)
        assert float(st["buf"].T_bg.item()) == res["Global temperature [K]"]
        for key in before:
            assert np.array_equal(before[key], after[key]), key


# ------------------------------------------------------------------------------------------------ (e) mode boundary
def test_mode_switch_is_strict_at_1e3_delta_t(km, torch, clean_env):
    name, pbc, kset = "sparse", 0, "distinct"
    dev = R.k_device(name)
    NL, n = dev["NL"], dev["n"]
    p = H.synth_params(kset)
    pats = H.synth_patterns(name, pbc)
    cls, _, Q, T_old = H.synth_inputs(name)
    at = np.float64(1e3) * np.float64(p["delta_t"])
    above = np.nextafter(at, np.inf)
    assert above > at and float(above) > 1e3 * p["delta_t"] >= float(at)
    with _state(km, torch, name, pbc) as st:
        for step_time, steady in ((at, False), (above, True), (at, False)):
            ref = H.heat_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], cls, p, step_time, Q, T_old, NL, n)
            assert ref["steady"] == steady and (ref["cdt"] == 0) == steady
            T, res = _heat(km, torch, st, p, float(step_time))
            kv = km.solvers.k_vectors(st["buf"])
            assert res["steady"] == ref["steady"] and res["stats"]["converged"] == 1
            _check_system("step_time %.17g (%s)" % (step_time, "steady" if steady else "transient"), kv, ref)
            # diag carries C/dt exactly in the transient mode: the steady diagonal is beyond the bar from it
            free = H.heat_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], cls, p, 1.0, Q, T_old, NL, n)
            with_c = H.rel_error(kv["diag"], free["diag"]) > BAR
            assert with_c == (not steady)


# ------------------------------------------------------------------------------------------------ (f) dictionaries in sequence
SEQUENCE = (("distinct", "steady"), ("metal_eq_vacancy", "transient"), ("all_equal", "steady"), ("distinct", "transient"))


@pytest.mark.parametrize("resident", [0, 1])
def test_dictionary_sequence_on_one_state(km, torch, clean_env, resident):
    """3, 2, 1 and 3 dictionary codes in turn on one state (the row-per-lane kernel changes its instance with the
    dictionary's size), then K: every call as on a fresh state, K's solve as on a state that never solved for heat."""
    S = km.solvers
    name, pbc = "sparse", 1
    dev = R.k_device(name)
    N, NL = dev["N"], dev["NL"]
    options = {"KMCF_CG_RESIDENT": str(resident)}
    t_start = time.perf_counter()

    def call(st, kset, mode):
        T, res = _heat(km, torch, st, H.synth_params(kset), H.SYNTH_STEP[mode])
        return T, res, S.k_vectors(st["buf"])

    def k_solve(st):
        buf = st["buf"]
        S.k_assemble(buf, dev["Vd"], dev["high_G"], dev["low_G"])
        stt = S.background_potential_gpu_sparse(buf, N, NL, NL, dev["Vd"], pbc, dev["high_G"], dev["low_G"], R.K_NN_DIST,
                                                len(dev["metals"]))
        S.sum_and_gather_potential(buf, NL, st["comm"])
        return stt, buf.site_potential_boundary.cpu().numpy().copy(), None

    fresh = {}
    for kset, mode in SEQUENCE:
        with _state(km, torch, name, pbc, options=options) as st:
            fresh[kset, mode] = call(st, kset, mode)
    with _state(km, torch, name, pbc, options=options) as st:
        k_alone = k_solve(st)
    with _state(km, torch, name, pbc, options=options) as st:
        for kset, mode in SEQUENCE:
            T, res, kv = call(st, kset, mode)
            ran, why = _walk(st)
            assert ran == "tile", why
            T_f, res_f, kv_f = fresh[kset, mode]
            print("resident %d, %s %s after the others: %d iterations (%d on a fresh state), %s"
                  % (resident, kset, mode, res["stats"]["iterations"], res_f["stats"]["iterations"], why))
            _check_system("%s %s in sequence" % (kset, mode), kv, H.synth_case(name, pbc, kset, mode)["ref"])
            for key in kv:
                assert np.array_equal(kv[key], kv_f[key]), (kset, mode, key)
            assert np.array_equal(T, T_f)
            assert res["stats"]["iterations"] == res_f["stats"]["iterations"] and res["stats"]["bb"] == res_f["stats"]["bb"]
            assert res["Global temperature [K]"] == res_f["Global temperature [K]"]
        k_after = k_solve(st)
    assert k_alone[0]["iterations"] > 0 and k_alone[0]["converged"] == 1
    _same_solve(k_alone, k_after)
    print("dictionary sequence, resident %d: K solve %d iterations, %.2f s" % (resident, k_alone[0]["iterations"],
                                                                             time.perf_counter() - t_start))


# ------------------------------------------------------------------------------------------------ (g) rank groups
GROUP_CALLS = [(k, m) for k in ("distinct", "metal_eq_other") for m in ("steady", "transient")]


def _uneven(n, P):
    """row counts that differ from rank to rank (and from kmcf_partition's even split)"""
    counts = np.full(P, n // P, np.int32)
    counts[0] -= 101
    counts[-1] += 101 + n % P
    if P > 2:
        counts[1] += 37
        counts[-1] -= 37
    assert counts.sum() == n and len(set(counts.tolist())) == P and counts.min() > 0
    return counts, np.r_[0, np.cumsum(counts)[:-1]].astype(np.int32)


@pytest.mark.parametrize("P", [2, 3])
def test_rank_groups_assemble_one_ranks_rows(km, torch, clean_env, P):
    S = km.solvers
    name, pbc = "sparse", 1
    dev = R.k_device(name)
    N, NL, n = dev["N"], dev["NL"], dev["n"]
    cls, _, Q, T_old = H.synth_inputs(name)
    counts, displs = _uneven(n, P)
    t_start = time.perf_counter()

    def calls(st):
        out = {}
        for kset, mode in GROUP_CALLS:
            T, res = _heat(km, torch, st, H.synth_params(kset), H.SYNTH_STEP[mode])
            out[kset, mode] = (T, res, S.k_vectors(st["buf"]), _walk(st), float(st["buf"].T_bg.item()))
        return out, [S.k_pattern(st["buf"], which) for which in range(3)]

    with _state(km, torch, name, pbc) as st:
        one, _ = calls(st)
    comms = S.KMC_comm.loopback_group(n, N + 1, N, N, size=P, device=0)
    for c in comms:
        c.counts_K, c.displs_K = counts.copy(), displs.copy()
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comms[r].connect()
            with _state(km, torch, name, pbc, comm=comms[r]) as st:
                out[r] = calls(st)
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(180)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish (deadlock?)"
    for c in comms:
        c.close()

    for kset, mode in GROUP_CALLS:
        T1, res1, kv1, _, _ = one[kset, mode]
        p, step_time = H.synth_params(kset), H.SYNTH_STEP[mode]
        T0 = p["background_temp"]
        for r in range(P):
            (T, res, kv, (ran, why), _), pats = out[r][0][kset, mode], out[r][1]
            r0, nr = int(displs[r]), int(counts[r])
            assert len(pats[0][0]) == nr + 1 and len(kv["diag"]) == nr
            # the system: this rank's rows of the one-rank run, byte for byte
            for key in VECTORS:
                assert np.array_equal(kv[key], kv1[key][r0:r0 + nr]), (kset, mode, r, key)
            ref = H.heat_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], cls, p, step_time, Q, T_old, NL, n, row0=r0)
            _check_system("P = %d rank %d rows [%d, %d) %s %s, %s walk (%s)" % (P, r, r0, r0 + nr, kset, mode, ran, why), kv, ref)
            assert res["stats"]["converged"] == 1 and res["steady"] == res1["steady"]
            assert np.array_equal(T, out[0][0][kset, mode][0])
            assert res["Global temperature [K]"] == out[0][0][kset, mode][1]["Global temperature [K]"]
        bar = 1e-10 * np.abs(T1 - T0).max()
        Tg = out[0][0][kset, mode][0]
        print("P = %d %s %s: iterations %s (one rank %d), |T - T_one_rank| = %.2g of the heating"
              % (P, kset, mode, [out[r][0][kset, mode][1]["stats"]["iterations"] for r in range(P)],
                 res1["stats"]["iterations"], np.abs(Tg - T1).max() / np.abs(T1 - T0).max()))
        assert np.abs(Tg - T1).max() <= bar
        _check_solution("P = %d %s %s, rank 0's field" % (P, kset, mode), name, H.synth_case(name, pbc, kset, mode), Tg,
                        out[0][0][kset, mode][1], out[0][0][kset, mode][4])
    print("P = %d: %.2f s" % (P, time.perf_counter() - t_start))

