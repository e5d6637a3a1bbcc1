"""numpy restatement of kmcf_event_census (include/kmcfield.h): from the (type, prob) of an event list --
events_thermal_ref.event_list on the CPU, solvers.event_rates on the GPU -- the table per (cell, layer, type), the
spectrum of the binary exponents, the row outputs and the statistics.  Sums come from math.fsum (the correctly rounded
sum): the yardstick a device sum in any order lies within n * 2^-52 * fsum of, n the bucket's number of terms, since all
terms are non-negative.  Everything else is exact: integers, selections (the bits of one slot's rate) and the row sums,
which one accumulator adds in slot order."""
import math

import numpy as np

EV_NULL = 4
BUCKET = np.dtype([("n_events", np.int64), ("rate_sum", np.float64), ("rate_max", np.float64), ("max_i", np.int32),
                   ("max_j", np.int32), ("n_zero", np.int32), ("reserved", np.int32)])
DEFAULT_BINS = (64, -128, 16)


def bin_of(p, n_bins, e_lo, e_step):
    """the spectrum's bin of a rate that is not NaN"""
    bits = int(np.float64(p).view(np.uint64))
    be = (bits >> 52) & 0x7ff
    if be == 0:
        return 0
    if be == 0x7ff:
        return n_bins - 1
    return min(max((be - 1023 - e_lo) // e_step, 0), n_bins - 1)         # (Python's // is the floor)


def stats_from_table(table):
    """what the header forms from the table: integer sums; rate_type[t] over cell ascending, then layer ascending, from
    0.0; rate_total = ((r0 + r1) + r2) + r3; dt_mean"""
    n_type, rate_type = [0] * 4, [0.0] * 4
    for t in range(4):
        r = 0.0
        for c in range(table.shape[0]):
            for l in range(table.shape[1]):
                r += float(table[c, l, t]["rate_sum"])
        rate_type[t] = r
        n_type[t] = int(table[:, :, t]["n_events"].sum())
    total = ((rate_type[0] + rate_type[1]) + rate_type[2]) + rate_type[3]
    return dict(n_type=n_type, rate_type=rate_type, n_events=int(table["n_events"].sum()), n_zero=int(table["n_zero"].sum()),
                rate_total=total, dt_mean=math.inf if total == 0 else 1 / total)


def census(typ, prob, neigh, layer, num_layers, displ=0, cell=None, n_cells=1, bins=DEFAULT_BINS):
    """typ, prob, neigh: the (count, nn) rows [displ, displ + count) of the list; layer, cell: per site of the whole device.
    Returns dict(table (n_cells + 1, num_layers, 4) of BUCKET, max_slot and n_terms of the same shape (slot id of the
    maximum, -1: none; non-NaN terms of rate_sum), spectrum (4, n_bins) or None, row_rate, row_best, stats)."""
    typ, prob, neigh = np.asarray(typ), np.asarray(prob, np.float64), np.asarray(neigh)
    count, nn = typ.shape
    layer = np.asarray(layer)
    table = np.zeros((n_cells + 1, num_layers, 4), BUCKET)
    table["max_i"] = table["max_j"] = -1
    max_slot = np.full(table.shape, -1, np.int64)
    n_terms = np.zeros(table.shape, np.int64)
    slot = np.flatnonzero(typ.reshape(-1) != EV_NULL)
    i = displ + slot // nn
    j = neigh.reshape(-1)[slot].astype(np.int64)
    ty = typ.reshape(-1)[slot].astype(np.int64)
    p = prob.reshape(-1)[slot]
    lay = layer[j].astype(np.int64)
    assert ((lay >= 0) & (lay < num_layers)).all()
    if cell is None:
        assert n_cells == 1
        ce = np.zeros(len(slot), np.int64)
    else:
        ce = np.asarray(cell)[i].astype(np.int64)
        ce = np.where((ce < 0) | (ce >= n_cells), n_cells, ce)
    key = (ce * num_layers + lay) * 4 + ty
    order = np.argsort(key, kind="stable")                  # ascending slot id inside a key
    bounds = np.flatnonzero(np.diff(key[order])) + 1
    nan = np.isnan(p)
    for grp in np.split(order, bounds) if len(order) else []:
        b = table.reshape(-1)[int(key[grp[0]])]             # (a view into table)
        num = grp[~nan[grp]]
        b["n_events"] = len(grp)
        b["n_zero"] = int((p[num] == 0.0).sum())
        b["rate_sum"] = math.fsum(p[num].tolist())
        n_terms.reshape(-1)[int(key[grp[0]])] = len(num)
        if len(num):
            first = num[np.flatnonzero(p[num] == p[num].max())[0]]
            b["rate_max"], b["max_i"], b["max_j"] = p[first], i[first], j[first]
            max_slot.reshape(-1)[int(key[grp[0]])] = slot[first]
    spectrum = None
    if bins is not None and bins[0] > 0:
        spectrum = np.zeros((4, bins[0]), np.int64)
        for t, q in zip(ty[~nan].tolist(), p[~nan].tolist()):
            spectrum[t, bin_of(q, *bins)] += 1
    # rows: one accumulator in slot order (numpy's cumsum adds sequentially: the bits of the plain loop, see row_loop)
    ev = (typ != EV_NULL) & ~np.isnan(prob)
    row_rate = np.cumsum(np.where(ev, prob, 0.0), axis=1)[:, -1] if count else np.zeros(0)
    masked = np.where(ev, prob, -1.0)
    row_best = np.where(ev.any(axis=1), masked.argmax(axis=1), -1).astype(np.int32) if count else np.zeros(0, np.int32)
    stats = stats_from_table(table)
    stats.update(slots=count * nn, n_nan=int(nan.sum()), rows_live=int((typ != EV_NULL).any(axis=1).sum()) if count else 0,
                 rate_max=0.0, max_i=-1, max_j=-1, max_type=-1)
    cand = np.flatnonzero(max_slot.reshape(-1) >= 0)
    if len(cand):
        flat = table.reshape(-1)
        top = flat["rate_max"][cand].max()
        tied = cand[flat["rate_max"][cand] == top]
        win = tied[np.argmin(max_slot.reshape(-1)[tied])]
        stats.update(rate_max=float(flat[win]["rate_max"]), max_i=int(flat[win]["max_i"]), max_j=int(flat[win]["max_j"]),
                     max_type=int(win % 4))
    return dict(table=table, max_slot=max_slot, n_terms=n_terms, spectrum=spectrum, row_rate=row_rate, row_best=row_best,
                stats=stats)


def row_loop(typ, prob):
    """the row outputs by the plain loop: (row_rate, row_best)"""
    count, nn = typ.shape
    rate, best = np.zeros(count), np.full(count, -1, np.int32)
    for r in range(count):
        acc, top = 0.0, None
        for s in range(nn):
            q = float(prob[r, s])
            if typ[r, s] == EV_NULL or q != q:
                continue
            acc += q
            if top is None or q > top:
                top, best[r] = q, s
        rate[r] = acc
    return rate, best


def census_loop(typ, prob, neigh, layer, num_layers, displ=0, cell=None, n_cells=1, bins=DEFAULT_BINS):
    """census() by one plain Python loop over the slots: the table (sums by fsum), max_slot, the spectrum"""
    count, nn = typ.shape
    table = np.zeros((n_cells + 1, num_layers, 4), BUCKET)
    table["max_i"] = table["max_j"] = -1
    max_slot = np.full(table.shape, -1, np.int64)
    terms = {}
    spectrum = np.zeros((4, bins[0]), np.int64)
    for r in range(count):
        for s in range(nn):
            t = int(typ[r, s])
            if t == EV_NULL:
                continue
            i, j, q = displ + r, int(neigh[r, s]), float(prob[r, s])
            c = 0 if cell is None else int(cell[i])
            c = n_cells if c < 0 or c >= n_cells else c
            idx = (c, int(layer[j]), t)
            b = table[idx]
            b["n_events"] += 1
            if q != q:
                continue
            terms.setdefault(idx, []).append(q)
            b["n_zero"] += q == 0.0
            if max_slot[idx] < 0 or q > b["rate_max"]:
                b["rate_max"], b["max_i"], b["max_j"] = q, i, j
                max_slot[idx] = r * nn + s
            spectrum[t, bin_of(q, *bins)] += 1
    for idx, v in terms.items():
        table[idx]["rate_sum"] = math.fsum(v)
    return table, max_slot, spectrum


def sum_bound(n_terms, fsum):
    """n * 2^-52 * fsum: the first-order bound of a sum of n non-negative terms in any order"""
    return n_terms * 2.0 ** -52 * fsum


def assert_tables_agree(got, ref, n_terms, what=""):
    """every integer and every maximum equal; rate_sum within the bound.  Returns the largest fraction of the bound."""
    for f in ("n_events", "n_zero", "max_i", "max_j"):
        assert np.array_equal(got[f], ref[f]), (what, f, np.flatnonzero((got[f] != ref[f]).reshape(-1))[:8])
    assert np.array_equal(got["rate_max"].view(np.uint64), ref["rate_max"].view(np.uint64)), (what, "rate_max")
    err = np.abs(got["rate_sum"] - ref["rate_sum"])
    bound = sum_bound(n_terms, ref["rate_sum"])
    assert np.isfinite(got["rate_sum"]).all() and (err <= bound).all(), (what, "rate_sum", float(err.max()))
    frac = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)
    return float(frac.max()) if frac.size else 0.0
