"""GPU: the event rate census (kmcf_event_census, csrc/kmcf_census.hip) against the numpy restatement of
tests/event_census_ref.py, fed with the (type, prob) that solvers.event_rates returns on the same inputs -- the same build
kernel, so every integer, every selection and every row sum must be EQUAL, and a bucket's rate_sum of n terms lies within
n * 2^-52 * fsum (all terms are non-negative: the first-order bound of any order of addition).  The cases and what each is
built for: tests/event_census_cases.py, shown on the references alone by tests/test_event_census_ref.py."""
import contextlib

import numpy as np
import pytest

import event_census_cases as K
import event_census_ref as CR
import events_thermal_ref as R
import stream_order_cases as SO
import test_gpu_stream_order as T
from test_gpu_events_graphs import _Dev

pytestmark = pytest.mark.gpu

torch, filler = T.torch, T.filler           # the fixtures of the stream order protocol


class _Case:
    """a case on the device with its cell map; census / rates on the rows [displ, displ + count)"""

    def __init__(self, km, name, T_bg=300.0):
        self.km, self.S, self.c = km, km.solvers, K.case(name, T_bg)
        self.dv = _Dev(km, self.c)
        self.cell = self.dv.i32(K.cell_map(self.c["N"]))

    def _args(self, count, displ):
        c, dv = self.c, self.dv
        count = c["N"] - displ if count is None else count
        neigh = dv.neigh[displ * c["nn"]:(displ + count) * c["nn"]] if count else dv.neigh      # (no rows: never read)
        return (dv.comm, c["N"], [count], [displ], c["nn"], neigh, dv.lay, c["T_bg"], c["freq"], c["sigma"], c["k"], dv.x, dv.y, dv.z,
                dv.pot, dv.el, dv.ch, c["layers"])

    def census(self, count=None, displ=0, cells=False, rows=True, **kw):
        return self.S.event_census(*self._args(count, displ), site_cell=self.cell if cells else None,
                                   n_cells=K.N_CELLS if cells else 1, bins=K.BINS, rows=rows, **kw)

    def rates(self, count=None, displ=0, **kw):
        return self.S.event_rates(*self._args(count, displ), **kw)

    def reference(self, count=None, displ=0, cells=False, **kw):
        c = self.c
        count = c["N"] - displ if count is None else count
        typ, prob = self.rates(count, displ, **kw)
        return CR.census(typ, prob, c["neigh"][displ:displ + count], c["lay"], len(c["layers"]), displ=displ,
                         cell=K.cell_map(c["N"]) if cells else None, n_cells=K.N_CELLS if cells else 1, bins=K.BINS)

    def close(self):
        self.dv.close()


@contextlib.contextmanager
def _case(km, name, T_bg=300.0):
    cs = _Case(km, name, T_bg)
    try:
        yield cs
    finally:
        cs.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _agree(got, ref, what):
    """got: solvers.event_census; ref: the restatement.  Returns the largest fraction of the sum bound."""
    frac = CR.assert_tables_agree(got["table"], ref["table"], ref["n_terms"], what)
    assert (got["table"]["reserved"] == 0).all()
    assert np.array_equal(got["spectrum"], ref["spectrum"]), what
    if got["row_rate"] is not None:
        assert np.array_equal(got["row_best"].cpu().numpy(), ref["row_best"]), what
        assert np.array_equal(_bits(got["row_rate"].cpu().numpy()), _bits(ref["row_rate"])), what
    g, r = got["stats"], ref["stats"]
    for f in ("slots", "n_events", "n_zero", "n_nan", "n_type", "rows_live", "max_i", "max_j", "max_type"):
        assert g[f] == r[f], (what, f, g[f], r[f])
    assert _bits(g["rate_max"]) == _bits(r["rate_max"]), what
    host = CR.stats_from_table(got["table"])                # the header's formulas on the RETURNED table: exact
    assert _bits(g["rate_type"]).tolist() == _bits(host["rate_type"]).tolist(), what
    assert _bits(g["rate_total"]) == _bits(host["rate_total"]) and _bits(g["dt_mean"]) == _bits(host["dt_mean"]), what
    assert g["ms_build"] > 0 and g["ms_census"] > 0 or g["slots"] == 0
    return frac


def _same_bytes(a, b):
    assert a["table"].tobytes() == b["table"].tobytes() and a["spectrum"].tobytes() == b["spectrum"].tobytes()
    assert a["row_rate"].cpu().numpy().tobytes() == b["row_rate"].cpu().numpy().tobytes()
    assert a["row_best"].cpu().numpy().tobytes() == b["row_best"].cpu().numpy().tobytes()
    strip = lambda s: {k: (_bits(v).tolist() if isinstance(v, (float, list)) else v) for k, v in s.items() if not k.startswith("ms")}
    assert strip(a["stats"]) == strip(b["stats"])


@pytest.mark.parametrize("T_bg", K.TEMPERATURES)
@pytest.mark.parametrize("name", K.CASES)
def test_census_matches_the_restatement(km, name, T_bg):
    with _case(km, name, T_bg) as cs:
        for cells in (False, True):
            got, ref = cs.census(cells=cells), cs.reference(cells=cells)
            frac = _agree(got, ref, "%s at %g K, cells %s" % (name, T_bg, cells))
            print("%s at %g K, %s: %d events in %d buckets (largest %d), %d zero, %d live rows; rate_sum: largest fraction of the "
                  "bound n * 2^-52 * fsum %.3f; build %.3f ms, census %.3f ms" % (
                      name, T_bg, "3 cells + rest" if cells else "one cell", got["stats"]["n_events"],
                      int((got["table"]["n_events"] > 0).sum()), int(got["table"]["n_events"].max()), got["stats"]["n_zero"],
                      got["stats"]["rows_live"], frac, got["stats"]["ms_build"], got["stats"]["ms_census"]))
        if name == "empty":
            assert got["stats"]["n_events"] == 0 and got["stats"]["dt_mean"] == np.inf and got["stats"]["max_i"] == -1
        assert cs.census(rows=False)["row_rate"] is None


@pytest.mark.parametrize("name, T_bg", [("mixed", 10.0), ("dense", 300.0)])
def test_two_calls_return_the_same_bytes(km, name, T_bg):
    with _case(km, name, T_bg) as cs:
        a = cs.census(cells=True)
        cs.S.events_reset(cs.dv.comm)                       # drops the census's scratch: the next call allocates again
        b, c = cs.census(cells=True), cs.census(cells=True)
        _same_bytes(a, b)
        _same_bytes(b, c)


@pytest.mark.parametrize("T_bg", K.TEMPERATURES)
@pytest.mark.parametrize("name", ["mixed", "dense"])
def test_merged_slices_are_the_whole(km, name, T_bg):
    pieces = K.slices(name)
    displ, count = pieces[0][1], sum(n for n, _ in pieces)
    with _case(km, name, T_bg) as cs:
        whole = cs.census(count, displ, cells=True)
        ref = cs.reference(count, displ, cells=True)
        _agree(whole, ref, name)
        parts = [cs.census(n, d, cells=True) for n, d in pieces]
        for (n, d), p in zip(pieces, parts):
            _agree(p, cs.reference(n, d, cells=True), "%s rows [%d, +%d)" % (name, d, n))
        merged = cs.S.event_census_merge(parts)
    CR.assert_tables_agree(merged["table"], whole["table"], ref["n_terms"], name)
    assert np.array_equal(merged["spectrum"], whole["spectrum"])
    assert merged["row_rate"].cpu().numpy().tobytes() == whole["row_rate"].cpu().numpy().tobytes()
    assert merged["row_best"].cpu().numpy().tobytes() == whole["row_best"].cpu().numpy().tobytes()
    for f in ("slots", "n_events", "n_zero", "n_nan", "n_type", "rows_live", "rate_max", "max_i", "max_j", "max_type"):
        assert merged["stats"][f] == whole["stats"][f], f
    assert abs(merged["stats"]["rate_total"] - whole["stats"]["rate_total"]) <= CR.sum_bound(ref["stats"]["n_events"],
                                                                                             ref["stats"]["rate_total"])
    # count == 0: KMCF_OK, everything zero, dt_mean +infinity
    with _case(km, "tiny") as cs:
        z = cs.census(0, 2, cells=True)
    assert not z["table"]["n_events"].any() and not z["table"]["rate_sum"].any() and (z["table"]["max_i"] == -1).all()
    assert not z["spectrum"].any() and z["stats"]["slots"] == 0 and z["stats"]["dt_mean"] == np.inf and z["row_rate"].numel() == 0


def test_thermal_modes(km):
    import torch as th
    with _case(km, "mixed") as cs:
        c = cs.c
        base = cs.census(cells=True)
        flat = th.full((c["N"],), c["T_bg"], dtype=th.float64, device="cuda")
        for mode in ("ekin", "site"):
            _same_bytes(base, cs.census(cells=True, site_temperature=flat, rate_mode=mode))
        field = 300.0 + 60.0 * np.random.default_rng(5).random(c["N"])
        Td = cs.dv.f64(field)
        for mode in ("ekin", "site"):
            got = cs.census(cells=True, site_temperature=Td, rate_mode=mode)
            _agree(got, cs.reference(cells=True, site_temperature=Td, rate_mode=mode), "mixed, mode %s" % mode)
            assert got["table"]["rate_sum"].tobytes() != base["table"]["rate_sum"].tobytes()
        typ, _, site = R.event_list(c["xyz"], c["neigh"], c["lay"], c["T_bg"], c["freq"], c["sigma"], c["k"], c["pot"], c["element"],
                                    c["charge"], c["layers"])
        bad = int(site[typ != R.EV_NULL].max())             # a site that owns an event
        for value in (0.0, -5.0, float("nan")):
            field_bad = field.copy()
            field_bad[bad] = value
            with pytest.raises(km.lib.KmcfError) as e:
                cs.census(cells=True, site_temperature=cs.dv.f64(field_bad), rate_mode="site")
            assert "(-1)" in str(e.value) and "kmcf_event_census: the temperature of site %d is not finite or not > 0" % bad in str(e.value)
        _same_bytes(base, cs.census(cells=True))            # a refused call leaves nothing behind


def test_nan_potential_at_one_live_site(km):
    with _case(km, "pairs1") as cs:
        c = cs.c
        typ, _ = K.rates("pairs1")
        row = int(np.flatnonzero(K.live_rows(typ))[3])
        pot = c["pot"].copy()
        pot[row] = np.nan
        cs.dv.pot = cs.dv.f64(pot)
        got, ref = cs.census(cells=True), cs.reference(cells=True)
        _agree(got, ref, "pairs1 with a NaN potential")
    n_nan = got["stats"]["n_nan"]
    print("NaN potential at site %d: %d of %d events have a NaN rate" % (row, n_nan, got["stats"]["n_events"]))
    assert n_nan >= 1 and n_nan == ref["stats"]["n_nan"]
    assert np.isfinite(got["table"]["rate_sum"]).all() and np.isfinite(got["table"]["rate_max"]).all()
    assert np.isfinite(got["stats"]["rate_total"]) and np.isfinite(got["stats"]["rate_max"])
    assert int(got["spectrum"].sum()) == got["stats"]["n_events"] - n_nan
    assert np.isfinite(got["row_rate"].cpu().numpy()).all()


@pytest.mark.parametrize("name", ["mixed", "asym"])
def test_census_leaves_the_step_alone(km, name):
    """a step behind a census (cells, rows, another temperature in between) is the step of a fresh communicator"""
    out = []
    for with_census in (True, False):
        with _case(km, name) as cs:
            rng = km.solvers.RandomNumberGenerator(cs.c["seed"])
            if with_census:
                cs.census(cells=True)
            first = cs.dv.step(rng)
            if with_census:
                cs.census(cells=False)                      # between two steps: the step's workspace exists
            second = cs.dv.step(rng)
            out.append((first, second, cs.dv.state(), rng.getRandomNumber()))
    (a1, a2, sa, ra), (b1, b2, sb, rb) = out
    for a, b in ((a1, b1), (a2, b2)):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2])
    assert a1[1] > 0 and np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1]) and ra == rb


class _Census(T._Events):
    """the census in the stream order protocol: the staged arrays of the event_rates case, the table as the output"""

    def call(self):
        S, h, m = self.ctx.S, self.h, self.comm_
        self.res = S.event_census(m, h["N"], m.counts_events, m.displs_events, h["nn"], self.neigh, self.lay, h["T_bg"], h["freq"], h["sigma"],
                                  h["k"], self.x, self.y, self.z, self.pot, self.el, self.ch, h["layers"], site_temperature=self.temp,
                                  rate_mode="site", rows=True)

    def read(self):
        r = self.res
        return dict(table=r["table"], spectrum=r["spectrum"], row_rate=r["row_rate"], row_best=r["row_best"], stats=r["stats"])


@pytest.mark.parametrize("stream", ["default", "side"])
def test_census_waits_for_the_callers_stream(km, torch, filler, stream):
    c = dict(SO.case("event_rates"), name="event_census")
    T._run_case(_Census, km, torch, filler, c, stream == "side", key="event_census")


@contextlib.contextmanager
def _device(km, d, periodic):
    """the 5 nm device after the first charge update and potential (the stages of tools/kmc_loop.py in front of the events)"""
    import torch as th
    S = km.solvers
    N, NL = d["N"], d["N_contact"]
    comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
    comm.connect()
    buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"], d["lattice"], d["metals"])
    try:
        pbc = 1 if periodic else 0
        S.compute_neighbor_list(comm, buf, d["nn_dist"], 52, pbc=pbc)
        S.compute_cutoff_list(comm, buf, 20.0, pbc=pbc)
        S.events_set_lattice(comm, d["lattice"], pbc)
        S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
        layers = km.structure.LAYERS
        lay_h = S.site_layers(d["xyz"][:, 0], layers)
        lay = th.as_tensor(lay_h, device="cuda")
        S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types, buf.num_metal_types_,
                            comm.counts_events, comm.displs_events, comm)
        S.background_potential_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"], len(d["metals"]), 0)
        S.poisson_gridless_gpu(buf, comm)
        S.sum_and_gather_potential(buf, NL, comm)
        args = (comm, N, comm.counts_events, comm.displs_events, 52, buf.neigh_idx, lay, 300.0, 10e13, d["sigma"], d["k"], buf.site_x,
                buf.site_y, buf.site_z, buf.site_potential_charge, buf.site_element, buf.site_charge, layers)
        yield S, args, buf.neigh_idx.cpu().numpy().reshape(N, 52), np.asarray(lay_h), len(layers)
    finally:
        buf.freeGPUmemory()
        comm.close()


@pytest.mark.parametrize("periodic", [False, True])
def test_5nm_device_open_and_periodic(km, dev5, periodic):
    d = km.structure.periodic_5nm("init") if periodic else dev5
    with _device(km, d, periodic) as (S, args, neigh, lay, L):
        typ, prob = S.event_rates(*args)
        got = S.event_census(*args, bins=K.BINS, rows=True)
        if periodic:                                        # the lattice counts: the open-boundary rates are others
            S.events_set_lattice(args[0], None, 0)
            assert S.event_census(*args, bins=K.BINS)["table"]["rate_sum"].tobytes() != got["table"]["rate_sum"].tobytes()
    ref = CR.census(typ, prob, neigh, lay, L, bins=K.BINS)
    frac = _agree(got, ref, "5 nm%s" % (" periodic" if periodic else ""))
    assert got["stats"]["n_events"] == int((typ != R.EV_NULL).sum()) > 0
    print("5 nm%s: %d events of %d slots, %d live rows, rate_total %.6e, dt_mean %.4e s; fraction of the sum bound %.3f; build %.3f ms, "
          "census %.3f ms" % (" periodic" if periodic else "", got["stats"]["n_events"], got["stats"]["slots"], got["stats"]["rows_live"],
                              got["stats"]["rate_total"], got["stats"]["dt_mean"], frac, got["stats"]["ms_build"], got["stats"]["ms_census"]))
