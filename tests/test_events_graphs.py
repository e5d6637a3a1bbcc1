"""CPU: the synthetic graphs of tests/events_graph_ref.py are what their names say -- shown with the two references alone
(the C oracle and the numpy restatement), never with the library.  tests/test_gpu_events_graphs.py then demands the
oracle's log of the device: the smallest margin of every case is > 1e-9 (the bar of tests/test_events_thermal.py; sums in
another order differ at 1e-15), so a kernel that is right cannot pick another slot."""
import numpy as np
import pytest

import events_graph_ref as G
import events_thermal_ref as R


def _stats(oracle, name):
    """(case, oracle reference, margins, footprint); the restatement must give the oracle's log (the two largest cases:
    the log is replayed, which checks every logged slot against u * total and its type)"""
    c, ref = G.case(name), G.reference(oracle, name)
    u = oracle.mt_uniform_stream(c["seed"], 2 * max(ref["n"], 1))
    if name in G.REPLAYED or not c["symmetric"]:
        m = G.margins(c, ref["log"], u)
    else:
        t, n, log, el, ch, m = G.restated_step(oracle, c)
        assert n == ref["n"] and np.array_equal(log, ref["log"])
        assert np.array_equal(el, ref["el"]) and np.array_equal(ch, ref["ch"])
        assert t == pytest.approx(ref["t"], rel=1e-14)
        if c["N"] <= 100000:
            assert np.allclose(G.margins(c, log, u), m, rtol=1e-6, atol=1e-12)   # the replay measures what the restatement does
    fp = G.footprint(c["neigh"], ref["log"])
    slow = G.slow_events(fp)
    print("%s: N %d nn %d, %d events, types %s, smallest margin %.2e, slow / fast %d / %d" % (
        name, c["N"], c["nn"], ref["n"], np.bincount(ref["log"][:, 2], minlength=5)[:4].tolist(), m.min(), slow.sum(), (~slow).sum()))
    return c, ref, m, fp


def _common(name, c, ref, m, min_types=3):
    lo, hi = G.WINDOWS.get(name, (20, 400))
    assert lo <= ref["n"] <= hi, ref["n"]
    assert m.min() > 1e-9
    assert (ref["log"][:, 2] < R.EV_NULL).all()
    if name != "many_capped":
        assert ref["n"] < c["max_events"] and ref["t"] >= 1 / c["freq"]            # the step ends by itself
    assert len(np.unique(ref["log"][:, 2])) >= min_types


@pytest.mark.parametrize("name", ["pairs1", "chain2", "local7", "nn63", "nn64", "nn70", "ring7_7001", "many", "many_capped"])
def test_small_graphs(oracle, name):
    c, ref, m, fp = _stats(oracle, name)
    _common(name, c, ref, m)
    nt, nst, ng = G.tree_shape(c["N"])
    assert nst <= G.EV_STMAX and ng <= G.EV_GLDS and not G.slow_events(fp).any()
    valid = (c["neigh"] >= 0).sum(axis=1)
    if name == "pairs1":
        assert c["nn"] == 1 and np.array_equal(c["neigh"][:, 0], np.arange(c["N"]) ^ 1)
    if name == "chain2":
        assert c["nn"] == 2 and valid[0] == 1 and valid[-1] == 1 and (valid[1:-1] == 2).all()
    if name == "local7":
        assert c["N"] % G.EV_RT and (c["neigh"][:, 6] == -1).all() and valid.max() == 6
    if name == "nn63":
        assert c["nn"] == G.NN_PERSISTENT and (valid == 63).all()                  # n_aff = 2 nn + 2 = 128 = EV_AFF
    if name in ("nn64", "nn70"):
        assert c["nn"] > G.NN_PERSISTENT                                           # three launches per event
    if name == "ring7_7001":
        assert c["N"] == G.case("nn70")["N"] and c["nn"] <= G.NN_PERSISTENT and nt > 1     # nn70's rows, on the persistent path
    if name == "many":
        assert ref["n"] > (4 + 8 + 16 + 32 + 64 + 128 + 256) + G.EV_BMAX           # batches of 4 .. 256, one of 512, into a second of 512
        assert len(np.unique(ref["log"][:, 2])) == 4
    if name == "many_capped":
        full = G.reference(oracle, "many")
        assert ref["n"] == 777 and np.array_equal(ref["log"], full["log"][:777])   # 508 events in batches of 4 .. 256, then one of 269


def test_tiny(oracle):
    """Less than one tile, one supertile, one group.  Two planted sites: the defect's generation and one hop of the vacancy."""
    c, ref, m, fp = _stats(oracle, "tiny")
    _common("tiny", c, ref, m, min_types=1)
    assert c["N"] < G.EV_RT and G.tree_shape(c["N"]) == (1, 1, 1)
    assert set(ref["log"][:, 2].tolist()) <= {R.EV_GEN, R.EV_VDIFF}


@pytest.mark.parametrize("N", [8192, 8193, 16384 + 129])
def test_edge_group(oracle, N):
    """8192: the last tile, supertile and group are full; 8193 and 16384 + 129: the last group, supertile and tile hold one
    row.  An event in the last row; beyond one group also an event whose i and j straddle rows 8191 | 8192."""
    name = "edge_group_%d" % N
    c, ref, m, fp = _stats(oracle, name)
    _common(name, c, ref, m)
    assert c["N"] == N and (N % G.GROUP_ROWS == 0 or N % (G.EV_RT * G.EV_ST) == 1)
    log = ref["log"]
    assert ((log[:, 0] == N - 1) | (log[:, 1] == N - 1)).any()
    if N > G.GROUP_ROWS:
        lo, hi = np.minimum(log[:, 0], log[:, 1]), np.maximum(log[:, 0], log[:, 1])
        assert ((lo < G.GROUP_ROWS) & (hi >= G.GROUP_ROWS)).any()


def test_scatter(oracle):
    c, ref, m, fp = _stats(oracle, "scatter")
    _common("scatter", c, ref, m)
    assert G.slow_events(fp).all()
    assert (fp[:, 1] > 16).sum() >= 10 and (fp[:, 2] >= 64).sum() >= 10
    print("scatter: up to %d touched groups" % fp[:, 1].max())


def test_mixed(oracle):
    c, ref, m, fp = _stats(oracle, "mixed")
    _common("mixed", c, ref, m)
    slow = G.slow_events(fp)
    changes = int((slow[1:] != slow[:-1]).sum())
    print("mixed: %d changes of path between consecutive events" % changes)
    assert slow.sum() >= 10 and (~slow).sum() >= 10 and changes >= 10
    assert ref["n"] <= G.EV_BMAX                  # (one step; the batches grow 4, 8, 16, ...: both paths inside the later ones)
    # a shrunk claim range (KMCF_EV_TREL): 64 tiles keep the split; at 1 tile every event spans more than the range,
    # since rows i +- 70 are always two tiles or more apart
    s64 = G.slow_events(fp, 64)
    assert s64.sum() >= 10 and (~s64).sum() >= 10
    assert G.slow_events(fp, 1).all()


@pytest.mark.parametrize("name", ["no_st", "no_glds"])
def test_walks_from_memory(oracle, name):
    c, ref, m, fp = _stats(oracle, name)
    _common(name, c, ref, m, min_types=2 if name == "no_glds" else 3)
    nt, nst, ng = G.tree_shape(c["N"])
    if name == "no_st":
        assert nst > G.EV_STMAX and ng <= G.EV_GLDS
    else:
        assert ng == G.EV_GLDS + 1
    groups = np.unique(ref["log"][:, :2] // G.GROUP_ROWS)
    assert len(groups) >= 8 and ng - 1 in groups


def test_asym_has_teeth(oracle):
    """On the list that is not symmetric a zero-out through the lists of i and j leaves the oracle's log within the first
    20 events: a library that trusted a verdict "symmetric" here would be caught."""
    c, ref, m, fp = _stats(oracle, "asym")
    _common("asym", c, ref, m)
    assert not c["symmetric"] and G.case("local7")["symmetric"]
    assert c["neigh"].shape == G.case("local7")["neigh"].shape
    u = oracle.mt_uniform_stream(c["seed"], 2 * c["max_events"])
    lw = G.listwise_step(c, u, max_events=20)
    k = min(len(lw), ref["n"])
    diff = np.flatnonzero((lw[:k] != ref["log"][:k]).any(axis=1))
    assert len(diff) and diff[0] < 20
    print("asym: the list-wise zero-out leaves the oracle's log at event %d" % diff[0])
    # on a symmetric list the two are the same step
    s = G.case("local7")
    assert np.array_equal(G.listwise_step(s, u), G.reference(oracle, "local7")["log"])


@pytest.mark.parametrize("name", ["local7", "nn63", "nn70"])
def test_longdouble_rates_set_the_scale(name):
    """The longdouble restatement the device's rates are held to agrees with the f64 one to a few hundred ulp at most
    (the exponent E_A / kT, up to ~200, multiplies the rounding of its operands)."""
    c = G.case(name)
    ii, cc, p_ld = G.rates_longdouble(c)
    typ, p = G.rates(c)
    assert len(ii) == (typ != R.EV_NULL).sum() >= 100
    err = float((np.abs(p[ii, cc] - p_ld) / p_ld).max())
    print("%s: %d live slots, f64 restatement against longdouble: %.3e" % (name, len(ii), err))
    assert 0 < err < 1e-12
