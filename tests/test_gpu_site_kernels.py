"""GPU: the kernels that feed the solver every KMC step, off the 5 nm fixture, each against its plain reference of
tests/site_kernels_ref.py (tests/test_site_kernels_ref.py pins the references and asserts what every input is built for).

  * pairwise term (kmcf_compute_cutoff_list + kmcf_poisson_gridless): per site |got - want| <= 1e-12 S_i with S_i the
    site's own sum of absolute terms (the project's 1e-12 of test_gpu_parity.py, no longer against the device-wide
    maximum), exactly 0.0 where no charged site lies within the cutoff, the sentinel outside the requested slice.
    Devices thinner than a cutoff, a single cell, full / empty / barely begun scan tiles, pairs AT the cutoff, sites on
    cell faces, slices, 263 scan tiles (the carry across passes of 256 tiles, once with every earlier tile empty), and
    the only charged site as the last item of the scan with 2047, 2048 and 2049 sites (tile_edge@N).
  * charge rule (kmcf_update_charge): hand-written neighbour rows, equal to charge_ref on the whole vector.
  * K / CB-edge value assembly: two synthetic devices x pbc 0 / 1 x both rules x both kernels (tiles, row-wise):
    off-diagonals bit-equal to k_values_ref, vectors and diagonal entries rtol 1e-14 (test_k_assembly_matches_oracle's
    bars), the two kernels bit-equal to each other, every compared result the SECOND of two different assemblies.
  * global heat (kmcf_update_temperature_global): N from 0 to 524 291 (the grid strides beyond 262 144), 1e-13 on the
    terms before they cancel.

Every test builds and frees its own communicator and buffers."""
import contextlib
import ctypes as C
import time

import numpy as np
import pytest

import site_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@contextlib.contextmanager
def _comm(km, *rows):
    c = km.solvers.KMC_comm(*rows)
    c.connect()
    try:
        yield c
    finally:
        c.close()


def _i32(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.int32), device="cuda")       # (a copy: the inputs are read-only)


def _f64(torch, a):
    return torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")


# ------------------------------------------------------------------------------------------------ pairwise term
PAIRWISE_RUNS = {"thin": ("thin", "thin_uncharged"), "one_cell": ("one_cell",), "one_site": ("one_site",),
                 "seventeen": ("seventeen",), "cube": ("cube",), "lattice_cutoffs": ("lattice_cutoffs",),
                 "large": ("large", "large_tail"),           # (one cutoff list per run: the sites are the same)
                 **{name: (name,) for name in R.TILE_EDGE}}  # the only charged site: the last item of the compaction's scan


@pytest.mark.parametrize("run", sorted(PAIRWISE_RUNS))
def test_pairwise_term_matches_direct_sum(km, dev5, torch, run):
    lib, p = km.lib.load(), km.solvers._ptr
    sigma, k = dev5["sigma"], dev5["k"]
    names = PAIRWISE_RUNS[run]
    first = R.pairwise_case(names[0])
    N, xyz = first["N"], first["xyz"]
    with _comm(km, 1, 2, N, 1) as comm:
        x, y, z = (_f64(torch, xyz[:, a]) for a in range(3))
        h = C.c_void_p()
        km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(x), p(y), p(z), N, R.CUTOFF, C.byref(h)), "kmcf_compute_cutoff_list")
        try:
            for name in names:
                c = R.pairwise_case(name)
                assert c["xyz"] is xyz or np.array_equal(c["xyz"], xyz)
                want, S, n = R.pairwise_reference(name, sigma, k)
                charge = _i32(torch, c["charge"])
                for displ, count in c["slices"]:
                    pot = torch.full((N,), R.SENTINEL, dtype=torch.float64, device="cuda")
                    t0 = time.perf_counter()
                    km.lib.check(lib.kmcf_poisson_gridless(h, p(x), p(y), p(z), p(charge), sigma, k, count, displ, p(pot)),
                                 "kmcf_poisson_gridless")
                    ms = 1e3 * (time.perf_counter() - t0)
                    got = pot.cpu().numpy()
                    sl = slice(displ, displ + count)
                    err = np.abs(got[sl].astype(np.longdouble) - want[sl]).astype(np.float64)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        rel = np.where(S[sl] > 0, err / S[sl], 0.0)
                    print("%s rows [%d, %d): max |got - want| / S = %.3g, %d sites without a term, %.2f ms"
                          % (name, displ, displ + count, rel.max() if count else 0.0, int((n[sl] == 0).sum()), ms))
                    assert np.all(got[:displ] == R.SENTINEL) and np.all(got[displ + count:] == R.SENTINEL)
                    assert np.all(err <= 1e-12 * S[sl]), "site %d of the slice" % int(np.argmax(err - 1e-12 * S[sl]))
                    lone = n[sl] == 0
                    assert np.all(got[sl][lone] == 0.0) and not np.signbit(got[sl][lone]).any()
        finally:
            lib.kmcf_pairwise_destroy(h)


# ------------------------------------------------------------------------------------------------ charge rule
@pytest.mark.parametrize("name", sorted(R.CHARGE_CASES))
def test_charge_rule_on_hand_written_rows(km, torch, name):
    lib, p = km.lib.load(), km.solvers._ptr
    c = R.charge_case(name)
    with _comm(km, 1, 2, 1, c["N"]) as comm:
        el, neigh, metals = _i32(torch, c["element"]), _i32(torch, c["neigh"].reshape(-1)), _i32(torch, c["metals"])
        charge = torch.full((c["N"],), 7, dtype=torch.int32, device="cuda")
        count, displ = np.array([c["row_count"]], np.int32), np.array([c["displ"]], np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        t0 = time.perf_counter()
        km.lib.check(lib.kmcf_update_charge(comm.handle, p(el), p(charge), p(neigh), c["N"], c["nn"], p(metals), len(c["metals"]),
                                            ip(count), ip(displ)), "kmcf_update_charge")
        ms = 1e3 * (time.perf_counter() - t0)
        got = charge.cpu().numpy()
    bad = np.flatnonzero(got != c["want"])
    print("%s: %d rows of %d slots from site %d, %d sites differ, %.2f ms" % (name, c["row_count"], c["nn"], c["displ"], len(bad), ms))
    for site, expect in c["crafted"]:
        assert got[site] == expect, "crafted row of site %d: got %d, expected %d" % (site, got[site], expect)
    assert len(bad) == 0, "first at site %d: got %d, want %d" % (bad[0], got[bad[0]], c["want"][bad[0]])


# ------------------------------------------------------------------------------------------------ K / CB values
def _rel(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(want != 0, r, np.where(got == want, 0.0, np.inf)))) if len(want) else 0.0


def _check_system(tag, got, ref, scaled=False):
    """the project's bars of test_k_assembly_matches_oracle.  scaled: the solve left A scaled in place by D^-1/2 and the
    scaling vector 1 / sqrt(diag) in dinv (the literal CB form, what a matrix without value codes runs), so the unscaled
    values are out of reach: dinv is held to 1 / sqrt(diag) of the reference at the same 1e-14, the values to
    val dis_i dis_j of the reference within 16 * 2^-53 -- sqrt, the division and the two products are each correctly
    rounded on both sides, 6 roundings each way"""
    off = ref["off_diagonal"]
    worst = {}
    for key in ("diag", "dinv", "rhs", "left", "right"):
        want = ref["dis"] if scaled and key == "dinv" else ref[key]
        worst[key] = _rel(got[key], want)
        np.testing.assert_allclose(got[key], want, rtol=1e-14, atol=0, err_msg="%s %s" % (tag, key))
    if scaled:
        worst["val (scaled)"] = _rel(got["val"], ref["val_scaled"])
        np.testing.assert_allclose(got["val"], ref["val_scaled"], rtol=16 * 2.0 ** -53, atol=0, err_msg=tag)
    else:
        assert np.array_equal(got["val"][off], ref["val"][off]), "%s: %d off-diagonals differ" % (tag, int((got["val"][off] != ref["val"][off]).sum()))
        worst["val diagonal"] = _rel(got["val"][~off], ref["val"][~off])
        np.testing.assert_allclose(got["val"][~off], ref["val"][~off], rtol=1e-14, atol=0, err_msg=tag)
    print("%s: largest relative error %s" % (tag, ", ".join("%s %.2g" % kv for kv in worst.items())))


@pytest.mark.parametrize("pbc", [0, 1])
@pytest.mark.parametrize("name", R.K_DEVICES)
def test_value_assembly_on_synthetic_devices(km, dev5, torch, monkeypatch, name, pbc):
    S = km.solvers
    dev = R.k_device(name)
    N, NL, n = dev["N"], dev["NL"], dev["n"]
    xyz, Vd, hi, lo = dev["xyz"], dev["Vd"], dev["high_G"], dev["low_G"]
    for key in ("KIND", "CODED", "SELL", "SELL_ROWS", "SELLV"):
        monkeypatch.delenv("KMCF_SPMV_" + key, raising=False)
    monkeypatch.delenv("KMCF_CB_SCALED", raising=False)
    t_start = time.perf_counter()
    with _comm(km, n, N + 1, N, N) as comm:
        buf = S.GPUBuffers(N, dev["element"], xyz[:, 0], xyz[:, 1], xyz[:, 2], R.K_CHARGE_NN, dev5["sigma"], dev5["k"],
                           dev["lattice"], dev["metals"])
        try:
            # charges by the library's rule on the library's list: the state the CPU conditions were asserted on
            S.compute_neighbor_list(comm, buf, R.K_CHARGE_NN_DIST, R.K_CHARGE_NN)
            S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                                buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
            assert np.array_equal(buf.site_charge.cpu().numpy(), dev["charge"])
            charge, charge2 = _i32(torch, dev["charge"]), _i32(torch, dev["charge2"])
            S.initialize_sparsity_K(buf, pbc, R.K_NN_DIST, NL, comm)
            pats = [S.k_pattern(buf, which) for which in range(3)]
            ref = {cb: R.k_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], dev["element"], dev["charge"], dev["metals"],
                                      hi, lo, Vd, NL, n, cb) for cb in (False, True)}
            rows = np.repeat(np.arange(n), np.diff(pats[0][0]))
            dis = 1.0 / np.sqrt(ref[True]["diag"])
            ref[True]["dis"], ref[True]["val_scaled"] = dis, ref[True]["val"] * dis[rows] * dis[pats[0][1]]
            mat = S.Distributed_matrix.from_handle(km.lib.load().kmcf_kstate_matrix(buf.K_distributed))

            def assemble_K():                  # twice in a row with different charges; the second one counts
                for ch in (charge2, charge):
                    buf.site_charge.copy_(ch)
                    S.k_assemble(buf, Vd, hi, lo)
                return S.k_vectors(buf)

            def assemble_CB():                 # (the state then holds the CB system: kmcf_update_CB_edge_sparse)
                st = S.update_CB_edge_gpu_sparse(buf, N, NL, NL, Vd, pbc, hi, lo, R.K_NN_DIST, len(dev["metals"]))
                print("   CB solve: %d iterations, %.2f ms" % (st["iterations"], st["ms_solve"]))
                return S.k_vectors(buf)

            # ---- default plan: the tile kernel
            tile = {False: assemble_K()}
            info = mat.info()                                     # (a matrix counts as coded once an assembly wrote its codes)
            assert info["spmv_kind"] == 2 and info["spmv_coded"] >= 1, info
            _, n_short, lane_tile_ends = mat.row_order()
            assert n_short == n                                   # all rows are short: the tiles cover every row
            plan = mat.sum_plan()
            ends, why = R.window_tiles(plan["row_ptr"], plan["col"])
            tile_rows = np.diff(np.r_[0, ends])
            print("%s pbc %d: %d rows, %.1f entries per row, %d tiles closed by %s, row-per-lane tiles of %d .. %d rows"
                  % (name, pbc, n, len(pats[0][1]) / n, len(ends), {w: why.count(w) for w in sorted(set(why))},
                     np.diff(np.r_[0, lane_tile_ends]).min() if len(lane_tile_ends) else 0,
                     np.diff(np.r_[0, lane_tile_ends]).max() if len(lane_tile_ends) else 0))
            if name == "dense":                                   # tiles close at the entry limit, not at 64 rows
                assert why.count("entries") >= len(ends) // 2 and tile_rows.min() < 64
            else:
                assert why.count("rows") >= len(ends) // 2
            _check_system("%s pbc %d K, tiles" % (name, pbc), tile[False], ref[False])
            tile[True] = assemble_CB()                            # the CB codes over K's
            _check_system("%s pbc %d CB, tiles" % (name, pbc), tile[True], ref[True])
            again = assemble_K()                                  # ... and K's over the CB system's
            for key in tile[False]:
                assert np.array_equal(again[key], tile[False][key]), key

            # ---- replanned without value codes, fresh assembly: the row-wise kernel
            monkeypatch.setenv("KMCF_SPMV_CODED", "0")
            assert mat.replan()["spmv_coded"] == 0
            row = {False: assemble_K()}
            assert mat.info()["spmv_coded"] == 0
            _check_system("%s pbc %d K, row-wise" % (name, pbc), row[False], ref[False])
            row[True] = assemble_CB()
            _check_system("%s pbc %d CB, row-wise" % (name, pbc), row[True], ref[True], scaled=True)
            # the two kernels: the same integer counts, the same three additions
            for key in ("val", "diag", "dinv", "rhs", "left", "right"):
                assert np.array_equal(row[False][key], tile[False][key]), "K " + key
            for key in ("diag", "rhs", "left", "right"):          # (the row-wise CB solve scaled val and dinv in place)
                assert np.array_equal(row[True][key], tile[True][key]), "CB " + key
            # ---- coded again, without the row-per-lane layout: the plan then reports its WINDOW tiles (the ones the tile
            # kernel walks; with the layout, spmv_tiles counts the row-per-lane tiles), and the tile kernel runs once more
            monkeypatch.delenv("KMCF_SPMV_CODED")
            monkeypatch.setenv("KMCF_SPMV_SELL", "0")
            mat.replan()
            third = assemble_K()
            info = mat.info()
            assert info["spmv_coded"] == 1 and info["spmv_tiles"] == len(ends), (info, len(ends))
            for key in tile[False]:
                assert np.array_equal(third[key], tile[False][key]), key
            monkeypatch.delenv("KMCF_SPMV_SELL")
            mat.replan()
        finally:
            buf.freeGPUmemory()
    print("%s pbc %d: %.2f s" % (name, pbc, time.perf_counter() - t_start))


# ------------------------------------------------------------------------------------------------ global heat
@pytest.mark.parametrize("N,steps", [(N, 100.0) for N in R.HEAT_SIZES] + [(257, 100.9)])      # (100.9 truncates to 100)
def test_global_heat_beyond_the_grid_cap(km, torch, N, steps):
    S = km.solvers
    p = R.heat_power(N)
    args = dict(R.HEAT_ARGS, steps=steps)
    want = R.heat_global_ref(p, 300.0, **args)
    bar = R.heat_bar(p, 300.0, **args)
    with _comm(km, 1, 2, 1, 1) as comm:
        # (N = 0: a buffer the kernel must not read -- the entry point takes no null pointer)
        power = _f64(torch, p) if N else torch.full((4,), 1e30, dtype=torch.float64, device="cuda")
        T = torch.tensor([300.0], dtype=torch.float64, device="cuda")
        t0 = time.perf_counter()
        S.update_temperatureglobal_gpu(power, T, N, args["a"], args["b"], args["steps"], args["C"], args["small_step"], comm)
        ms = 1e3 * (time.perf_counter() - t0)
        got = T.item()
    print("N %d, steps %s: T %.15g, |T - T_ref| = %.3g, bar %.3g, %.2f ms" % (N, steps, got, abs(got - want), bar, ms))
    assert abs(got - want) <= bar
    if N == 0:
        a, b = args["a"], args["b"]
        assert want == b * (1 - a ** 100) / (1 - a) + a ** 100 * 300.0
    if steps != 100.0:
        assert want == R.heat_global_ref(p, 300.0, **dict(args, steps=100.0))
