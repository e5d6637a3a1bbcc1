"""CPU: the numpy restatement of the event census (tests/event_census_ref.py) against a plain Python loop, and the
conditions on the inputs of tests/test_gpu_event_census.py, shown with the references alone: zero rates and tied maxima
at 10 K, all four event types, more than 256 compaction tiles, live slots on both sides of a tile boundary, nn above the
persistent step's limit, a slice boundary inside a run of live rows, a rest bucket that is not empty.  And the host
combination rule (solvers.event_census_merge) on tables the restatement computed."""
import numpy as np
import pytest

import event_census_cases as K
import event_census_ref as CR
import events_thermal_ref as R


def _same_exact(a, b):
    for f in CR.BUCKET.names:
        assert np.array_equal(a[f].view(np.uint64) if a[f].dtype == np.float64 else a[f],
                              b[f].view(np.uint64) if b[f].dtype == np.float64 else b[f]), f


@pytest.mark.parametrize("T_bg", K.TEMPERATURES)
@pytest.mark.parametrize("name", ["tiny", "pairs1"])
def test_restatement_equals_the_plain_loop(name, T_bg):
    c = K.case(name, T_bg)
    typ, prob = K.rates(name, T_bg)
    cell = K.cell_map(c["N"])
    ref = K.reference(name, T_bg, cells=True)
    table, max_slot, spectrum = CR.census_loop(typ, prob, c["neigh"], c["lay"], len(c["layers"]), cell=cell, n_cells=K.N_CELLS,
                                               bins=K.BINS)
    _same_exact(ref["table"], table)
    assert np.array_equal(ref["max_slot"], max_slot) and np.array_equal(ref["spectrum"], spectrum)
    rate, best = CR.row_loop(typ, prob)
    assert np.array_equal(ref["row_rate"].view(np.uint64), rate.view(np.uint64)) and np.array_equal(ref["row_best"], best)
    assert ref["stats"]["n_events"] == int((typ != R.EV_NULL).sum()) == int(ref["spectrum"].sum())
    assert ref["stats"]["rows_live"] == int(K.live_rows(typ).sum())


@pytest.mark.parametrize("name, n_zero, n_top", [("pairs1", 18, 32), ("mixed", 129, 298), ("asym", 33, 308)])
def test_10_K_holds_zero_rates_and_tied_maxima(name, n_zero, n_top):
    typ, prob = K.rates(name, 10.0)
    live = typ != R.EV_NULL
    assert int((prob[live] == 0.0).sum()) == n_zero
    assert prob.max() == 1e214 and int((prob[live] == 1e214).sum()) == n_top
    ref = K.reference(name, 10.0, cells=True)
    # some bucket's maximum is attained by more than one of its slots: the smallest slot id decides
    c = K.case(name)
    slot = np.flatnonzero(live.reshape(-1))
    tied_inside = 0
    t = ref["table"]
    for idx in zip(*np.nonzero(ref["max_slot"] >= 0)):
        i = slot // c["nn"]
        cell = K.cell_map(c["N"])[i]
        cell = np.where((cell < 0) | (cell >= K.N_CELLS), K.N_CELLS, cell)
        j = c["neigh"].reshape(-1)[slot]
        members = (cell == idx[0]) & (c["lay"][j] == idx[1]) & (typ.reshape(-1)[slot] == idx[2])
        hits = slot[members & (prob.reshape(-1)[slot] == t[idx]["rate_max"])]
        assert hits.min() == ref["max_slot"][idx]
        tied_inside += len(hits) > 1
    assert tied_inside >= 1


def test_conditions_on_the_inputs():
    typ, _ = K.rates("mixed")
    assert set(np.unique(typ).tolist()) == {0, 1, 2, 3, 4}                           # all four event types at 300 K
    assert typ.size > 9.6e6 and (typ.size + K.SCAN_TILE - 1) // K.SCAN_TILE > 256    # the scan kernel's second pass
    typ, _ = K.rates("dense")
    assert (typ.reshape(-1)[[2047, 2048, 2049]] != R.EV_NULL).all()                  # both sides of a tile boundary
    assert int((typ != R.EV_NULL).sum()) == 79986 and set(np.unique(typ).tolist()) == {0, 4}
    assert K.reference("dense")["table"]["n_events"].max() > 15000                   # buckets of tens of thousands of terms
    assert K.reference("dense", cells=True)["table"]["n_events"].max() > 3000        # (thousands with the cell map)
    assert not (K.rates("empty")[0] != R.EV_NULL).any()
    assert K.case("nn64")["nn"] == 64 and K.case("nn70")["nn"] == 70 and "nn64" in K.CASES and "nn70" in K.CASES
    for name in ("mixed", "dense"):
        live = K.live_rows(K.rates(name)[0])
        pieces = K.slices(name)
        for (count, displ), (_, nxt) in zip(pieces[:-1], pieces[1:]):
            assert displ > 0 and displ + count == nxt
        assert any(live[d - 1] and live[d] for _, d in pieces[1:])      # a cut inside a run of live rows (dense: 255 | 256)
        assert all(count % 16 for count, _ in pieces)
    for name in K.CASES:
        if name != "empty":
            assert K.reference(name, cells=True)["table"][K.N_CELLS]["n_events"].sum() > 0, name    # the rest bucket


@pytest.mark.parametrize("T_bg", K.TEMPERATURES)
@pytest.mark.parametrize("name", ["mixed", "dense"])
def test_merge_of_the_slices_is_the_whole(km, name, T_bg):
    pieces = K.slices(name)
    displ, count = pieces[0][1], sum(n for n, _ in pieces)
    whole = K.reference(name, T_bg, cells=True, count=count, displ=displ)
    parts = [K.reference(name, T_bg, cells=True, count=n, displ=d) for n, d in pieces]
    for p in parts + [whole]:
        p["stats"].update(ms_build=0.0, ms_census=0.0)
    merged = km.solvers.event_census_merge(parts)
    CR.assert_tables_agree(merged["table"], whole["table"], whole["n_terms"], name)
    assert np.array_equal(merged["spectrum"], whole["spectrum"])
    assert np.array_equal(merged["row_rate"], whole["row_rate"]) and np.array_equal(merged["row_best"], whole["row_best"])
    for f in ("slots", "n_events", "n_zero", "n_nan", "n_type", "rows_live", "rate_max", "max_i", "max_j", "max_type"):
        assert merged["stats"][f] == whole["stats"][f], f
    assert abs(merged["stats"]["rate_total"] - whole["stats"]["rate_total"]) <= CR.sum_bound(whole["stats"]["n_events"],
                                                                                             whole["stats"]["rate_total"])
