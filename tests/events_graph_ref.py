"""Synthetic neighbour graphs that drive the KMC event step (csrc/kmcf_events.hip) to the edges of its sum tree, and the
numpy tools that prove, with the references alone, that each graph reaches what its name says.

The event step only needs a neighbour list, positions, potentials and site states: no real device.  Every case here is a
small dict that oracle.kmc_step, events_thermal_ref.kmc_step and solvers.execute_kmc_step_mpi all accept (see step_args /
oracle_step).  tests/test_events_graphs.py (CPU) checks the conditions on the inputs; tests/test_gpu_events_graphs.py
holds the library to the oracle on them."""
import numpy as np

import events_thermal_ref as R

# Mirrored from csrc/kmcf_events.hip (the constexpr block in front of event_batch_kernel): rows per tile, tiles per group,
# tiles per supertile, range of the tile claim table, group sums kept in LDS, supertile sums kept in LDS, events per
# batch; and the largest nn the persistent kernel takes (execute_kmc_step_impl: "nn <= 63", EV_AFF = 2 * 63 + 2).
EV_RT = 32
EV_GROUP = 256
EV_ST = 4
EV_TREL = 2048
EV_GLDS = 512
EV_STMAX = 12800
EV_BMAX = 512
NN_PERSISTENT = 63
GROUP_ROWS = EV_RT * EV_GROUP

VACANCY_K, DEFECT_K, ION_K = 0, 1, 2          # kinds of planted sites


def tree_shape(N):
    """(tiles, supertiles, groups) of the row-aligned tree of an N-row list."""
    n_tiles = (N + EV_RT - 1) // EV_RT
    return n_tiles, (n_tiles + EV_ST - 1) // EV_ST, (n_tiles + EV_GROUP - 1) // EV_GROUP


def is_symmetric(neigh):
    """every listed neighbour j of i lists i back, and no row lists a site twice"""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    v = neigh >= 0
    i = np.broadcast_to(np.arange(N, dtype=np.int64)[:, None], neigh.shape)[v]
    j = neigh[v].astype(np.int64)
    a, b = i * N + j, j * N + i                    # the pairs as listed and turned round: the same set
    if (a[1:] < a[:-1]).any():
        a.sort()
    b.sort()
    return bool((a[1:] != a[:-1]).all()) and np.array_equal(a, b)


def _pack(cols, nn):
    """rows of candidate ids (-1: none) -> valid entries ascending and first, duplicates dropped, padded with -1 to nn"""
    big = np.iinfo(np.int64).max
    a = np.where(cols >= 0, cols, big).astype(np.int64)
    a.sort(axis=1)
    dup = np.zeros(a.shape, bool)
    dup[:, 1:] = a[:, 1:] == a[:, :-1]
    a[dup] = big
    a.sort(axis=1)
    assert a.shape[1] <= nn or (a[:, nn:] == big).all(), "a row holds more than nn neighbours"
    out = np.full((a.shape[0], nn), -1, np.int32)
    w = min(nn, a.shape[1])
    out[:, :w] = np.where(a[:, :w] == big, -1, a[:, :w])
    return out


def ring_list(N, offsets, wrap, nn, only=None):
    """Site i lists i +- o for every offset o (modulo N with wrap, else entries out of range are dropped).  only: a
    boolean mask per offset-row, offsets[k] is used from sites with only[k][i] (the caller keeps that symmetric)."""
    i = np.arange(N, dtype=np.int64)[:, None]
    o = np.asarray(offsets, np.int64)[None, :]
    cols = np.concatenate([i - o, i + o], axis=1)
    if wrap:
        cols %= N
    else:
        cols[(cols < 0) | (cols >= N)] = -1
    if only is not None:
        m = np.concatenate([only, only], axis=1)
        cols[~m] = -1
    cols[cols == i] = -1
    out = _pack(cols, nn)
    assert is_symmetric(out)
    return Symmetric(out)


class Symmetric:
    """a list that has passed is_symmetric (graph_case does not check it a second time)"""

    def __init__(self, neigh):
        self.neigh = neigh


def make_layers():
    return [dict(E_gen_0=0.9 + 0.05 * l, E_rec_1=0.3, E_diff_2=0.6 + 0.05 * l, E_diff_3=0.5) for l in range(5)]


def graph_case(name, neigh, n_hot, seed, force=(), pot_set=None, max_events=4096, pair_ions=True, hot_rows=None):
    """Everything a step needs.  All sites are O with charge 0 and a potential from N(0, 0.02 V); n_hot random sites (and
    the sites of `force`: (site, kind, shift)) become a vacancy (+2), a defect or an oxygen ion (-2) whose potential is
    moved by U(-0.2, 1.2) V (ions: the other way), which makes some of their events hot (E_A < 0) and leaves others cold.
    pair_ions: half of the planted ions get a vacancy or a defect on one listed neighbour, so that recombination and ion
    diffusion occur.  hot_rows: half of the random sites are drawn from these rows instead of from all."""
    symmetric = isinstance(neigh, Symmetric) or is_symmetric(neigh)
    neigh = np.ascontiguousarray(neigh.neigh if isinstance(neigh, Symmetric) else neigh, np.int32)
    N, nn = neigh.shape
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0.0, 50.0, (N, 3))
    element = np.full(N, R.O_EL, np.int32)
    charge = np.zeros(N, np.int32)
    pot = rng.normal(0.0, 0.02, N)
    lay = rng.integers(0, 5, N).astype(np.int32)
    sites = rng.choice(N, size=min(n_hot, N), replace=False) if n_hot else np.zeros(0, np.int64)
    if hot_rows is not None and n_hot:
        half = len(sites) // 2
        sites[:half] = rng.choice(np.asarray(hot_rows), size=half, replace=False)
    kinds = rng.integers(0, 3, len(sites))
    shifts = rng.uniform(-0.2, 1.2, len(sites))
    planted = {}

    def plant(s, kind, shift):
        s = int(s)
        if s in planted:
            return False
        planted[s] = kind
        if kind == VACANCY_K:
            element[s], charge[s] = R.VACANCY, 2
            pot[s] += shift
        elif kind == DEFECT_K:
            element[s], charge[s] = R.DEFECT, 0
            pot[s] += shift
        else:
            element[s], charge[s] = R.OXYGEN_DEFECT, -2
            pot[s] -= shift
        return True

    for s, kind, shift in force:
        plant(s, kind, shift)
    for s, kind, shift in zip(sites, kinds, shifts):
        if plant(s, kind, shift) and kind == ION_K and pair_ions and rng.random() < 0.5:
            row = neigh[s][neigh[s] >= 0]
            if len(row):
                plant(row[rng.integers(len(row))], int(rng.integers(0, 2)), rng.uniform(-0.2, 1.2))
    for s, v in (pot_set or {}).items():
        pot[s] = v
    return dict(name=name, N=N, nn=nn, neigh=neigh, xyz=xyz, element=element, charge=charge, lay=lay, pot=pot,
                layers=make_layers(), T_bg=300.0, freq=1e14, sigma=3.5e-10, k=8.987552e9 / 23, seed=1, max_events=max_events,
                symmetric=symmetric)


def oracle_step(oracle, c, max_events=None):
    """oracle.kmc_step on a case: (t, n, log, element_after, charge_after)"""
    return oracle.kmc_step(c["xyz"], c["neigh"], c["lay"], c["T_bg"], c["freq"], c["sigma"], c["k"], c["pot"], c["element"],
                           c["charge"], c["layers"], oracle.mt_state(c["seed"]), max_events=max_events or c["max_events"])


def rates(c):
    """(type, prob) of events_thermal_ref.event_list in KMCF_RATE_T_BG"""
    typ, prob, _ = R.event_list(c["xyz"], c["neigh"], c["lay"], c["T_bg"], c["freq"], c["sigma"], c["k"], c["pot"], c["element"],
                                c["charge"], c["layers"])
    return typ, prob


def rates_longdouble(c):
    """The rates of the live slots by the formula of events_thermal_ref.event_list (KMCF_RATE_T_BG) in numpy.longdouble:
    (rows, columns, prob).  The constants are the doubles of the formula; the screened self-interaction, whose erfc numpy
    lacks in that type, is formed by mpmath at 30 digits from the same doubles."""
    import mpmath
    LD = np.longdouble
    mp = mpmath.mp.clone()
    mp.dps = 30
    typ, _ = rates(c)
    ii, cc = np.nonzero(typ != R.EV_NULL)
    jj = c["neigh"][ii, cc]
    et = typ[ii, cc]
    pot, ch, lay = c["pot"].astype(LD), c["charge"].astype(np.int64), c["lay"]
    E = [np.array([l[key] for l in c["layers"]], LD) for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]

    def v_solve(i, j, q):
        d2 = sum((mp.mpf(float(c["xyz"][j, a])) - mp.mpf(float(c["xyz"][i, a]))) ** 2 for a in range(3))
        r = mp.mpf(1e-10) * mp.sqrt(d2)
        v = q * mp.erfc(r / (mp.mpf(c["sigma"]) * mp.sqrt(2))) * mp.mpf(c["k"]) * mp.mpf(R.Q) / r
        return LD(mp.nstr(v, 25))

    dpot = pot[ii] - pot[jj]
    ci, cj = ch[ii], ch[jj]
    EA = np.zeros(len(ii), LD)
    for n in range(len(ii)):
        i, j, t = int(ii[n]), int(jj[n]), int(et[n])
        if t == R.EV_GEN:
            EA[n] = E[0][lay[j]] - 2 * dpot[n]
        elif t == R.EV_REC:
            cs = int(ci[n] - cj[n])
            EA[n] = E[1][lay[j]] - cs * (dpot[n] + int(np.sign(cs) * (abs(cs) // 2)) * v_solve(i, j, 2))
        elif t == R.EV_VDIFF:
            siv = v_solve(i, j, int(ci[n])) if ci[n] != 0 else LD(0)
            EA[n] = E[2][lay[j]] - int(ci[n] - cj[n]) * (dpot[n] + siv)
        else:
            siv = v_solve(i, j, 2) if ci[n] != 0 else LD(0)
            EA[n] = E[3][lay[j]] - int(ci[n] - cj[n]) * (dpot[n] - siv)
    prob = LD(c["freq"]) * (1 / (np.exp(EA / (LD(R.KB) * LD(c["T_bg"]))) + LD(R.EPSILON)))
    return ii, cc, prob


def restated_step(oracle, c, max_events=None):
    cap = max_events or c["max_events"]
    u = oracle.mt_uniform_stream(c["seed"], 2 * cap)
    return R.kmc_step(c["xyz"], c["neigh"], c["lay"], c["T_bg"], c["freq"], c["sigma"], c["k"], c["pot"], c["element"],
                      c["charge"], c["layers"], u, max_events=cap)


def _zero_listwise(flat, prob, typ, nn, i, j):
    """the zero-out of the library's fast path: rows i and j, and in the rows they list the slots that point to i or j"""
    for s in (i, j):
        row = flat[s * nn:(s + 1) * nn]
        for n in row[row >= 0]:
            sl = slice(n * nn, (n + 1) * nn)
            hit = (flat[sl] == i) | (flat[sl] == j)
            prob[sl][hit] = 0.0
            typ[sl][hit] = R.EV_NULL
        live = slice(s * nn, (s + 1) * nn)
        prob[live][row >= 0] = 0.0
        typ[live][row >= 0] = R.EV_NULL


def _zero_full(flat, prob, typ, nn, i, j):
    """zero_out_events_split as the oracle states it: every slot whose row or entry is i or j"""
    dead = (flat == i) | (flat == j)
    dead[i * nn:(i + 1) * nn] |= flat[i * nn:(i + 1) * nn] >= 0
    dead[j * nn:(j + 1) * nn] |= flat[j * nn:(j + 1) * nn] >= 0
    prob[dead] = 0.0
    typ[dead] = R.EV_NULL


def margins(c, log, uniforms):
    """Replay of a log: for every event the distance of u * total from the nearest boundary of the logged slot in the
    cumulative sum, relative to the total (events_thermal_ref.kmc_step's margins, without its per-event cumsum over all
    slots: the partial sum up to the logged slot, zero-out through the lists where they are symmetric).  A logged slot
    that does not hold u * total gives a negative margin; a logged type that is not the slot's raises."""
    typ, prob = rates(c)
    nn = c["nn"]
    typ, prob, flat = typ.reshape(-1).copy(), prob.reshape(-1).copy(), c["neigh"].reshape(-1)
    zero = _zero_listwise if c["symmetric"] else _zero_full
    out = []
    for n, (i, j, et) in enumerate(np.asarray(log).tolist()):
        col = np.flatnonzero(flat[i * nn:(i + 1) * nn] == j)
        assert len(col) == 1, "logged pair (%d, %d) is not one slot" % (i, j)
        idx = i * nn + int(col[0])
        assert typ[idx] == et, "event %d: logged type %d, slot type %d" % (n, et, typ[idx])
        total = prob.sum()
        number = uniforms[2 * n] * total
        lo = prob[:idx].sum()
        out.append(min(number - lo, lo + prob[idx] - number) / total)
        zero(flat, prob, typ, nn, i, j)
    return np.array(out)


def listwise_step(c, uniforms, max_events=None):
    """The numpy step with the fast path's zero-out (through the lists of i and j only): the log.  Equal to the oracle's
    on a symmetric list; on a list that is not symmetric it keeps slots alive that the oracle kills."""
    cap = max_events or c["max_events"]
    typ, prob = rates(c)
    nn = c["nn"]
    typ, prob, flat = typ.reshape(-1).copy(), prob.reshape(-1).copy(), c["neigh"].reshape(-1)
    log, t, n = [], 0.0, 0
    while t < 1 / c["freq"] and n < cap:
        cum = np.cumsum(prob)
        total = cum[-1]
        idx = min(int(np.searchsorted(cum, uniforms[2 * n] * total, side="right")), len(cum) - 1)
        i, j = idx // nn, int(flat[idx])
        log.append((i, j, int(typ[idx])))
        _zero_listwise(flat, prob, typ, nn, i, j)
        t = -np.log(uniforms[2 * n + 1]) / total
        n += 1
    return np.array(log, np.int32).reshape(-1, 3)


def footprint(neigh, log):
    """Per event the rows the kernel touches (the valid neighbours of i and of j, i and j): (span, groups, distance) --
    largest minus smallest touched tile, number of distinct groups, largest minus smallest touched group."""
    out = np.zeros((len(log), 3), np.int64)
    for n, (i, j, _) in enumerate(np.asarray(log).tolist()):
        rows = np.concatenate([neigh[i], neigh[j], [i, j]])
        tiles = rows[rows >= 0] // EV_RT
        groups = tiles // EV_GROUP
        out[n] = tiles.max() - tiles.min(), len(np.unique(groups)), groups.max() - groups.min()
    return out


def slow_events(fp, trel=EV_TREL):
    """the events that leave the claim range: span >= trel tiles or distance >= 64 groups"""
    return (fp[:, 0] >= trel) | (fp[:, 2] >= 64)


# ---- the cases ---------------------------------------------------------------------------------------------------------

def _pairs1():
    N = 4098
    neigh = (np.arange(N, dtype=np.int32) ^ 1)[:, None]
    return graph_case("pairs1", neigh, 90, 11)


def _edge(N, seed):
    # hot pairs in the last row and across the boundary of the first group (rows 8191 | 8192): a vacancy far above its
    # neighbours; the neighbour across the boundary far below the others, so that slot carries the row's rate
    # (N = 8193: row 8192 is the last row AND the far side of the boundary -- one event does both)
    force = [(N - 1, VACANCY_K, 1.2)] if N - 1 != GROUP_ROWS else []
    pot_set = {}
    if N > GROUP_ROWS:
        force.append((GROUP_ROWS - 1, VACANCY_K, 1.2))
        pot_set[GROUP_ROWS] = -0.5
    return graph_case("edge_group_%d" % N, ring_list(N, [1, 2, 70], False, 6), 60, seed, force=force, pot_set=pot_set)


def _mixed():
    N = 600077
    far = (np.arange(N) % 1000 < 10)[:, None]
    near = np.ones((N, 1), bool)
    only = np.concatenate([near, near, near] + [far] * 5, axis=1)
    neigh = ring_list(N, [1, 2, 70] + [99000 * k for k in range(1, 6)], False, 16, only=only)
    return graph_case("mixed", neigh, 100, 5, hot_rows=np.flatnonzero(far[:, 0]))


def _asym():
    """local7 plus one-way edges a -> b in the padding column (the last column is no longer sorted into the row): a is an
    ion, b a vacancy 1000 rows on that does not list a.  The recombination a -> b is hot and b has hot hops of its own:
    once b hops, the oracle's pass kills a -> b, a walk through b's lists does not find it."""
    base = ring_list(5013, [1, 2, 70], False, 7).neigh
    assert (base[:, 6] == -1).all()
    neigh = base.copy()
    rng = np.random.default_rng(77)
    a_sites = rng.choice(np.arange(100, 3900, 5), size=40, replace=False)
    force = []
    for a in a_sites.tolist():
        b = a + 1000
        neigh[a, 6] = b
        force += [(a, ION_K, -0.6), (b, VACANCY_K, 1.0)]    # E_A of a -> b and of b's hops: both about -1.3 eV
    c = graph_case("asym", neigh, 30, 7, force=force)
    assert not c["symmetric"]
    return c


def _no(name, N, seed):
    return graph_case(name, ring_list(N, [1, 1000], False, 4), 60, seed, force=[(N - 1, VACANCY_K, 1.2)])


def _many(max_events):
    return graph_case("many" if max_events == 4096 else "many_capped", ring_list(20011, [1, 33, 4100], True, 6), 2600, 3,
                      max_events=max_events)


BUILDERS = {
    "pairs1": _pairs1,
    "chain2": lambda: graph_case("chain2", ring_list(4099, [1], False, 2), 60, 2),
    "local7": lambda: graph_case("local7", ring_list(5013, [1, 2, 70], False, 7), 60, 3),
    "tiny": lambda: graph_case("tiny", ring_list(5, [1], False, 2), 0, 4, force=[(1, DEFECT_K, 1.0), (3, VACANCY_K, 0.1)]),
    "edge_group_8192": lambda: _edge(8192, 5),
    "edge_group_8193": lambda: _edge(8193, 6),
    "edge_group_16513": lambda: _edge(16384 + 129, 7),
    "nn63": lambda: graph_case("nn63", ring_list(9006, list(range(1, 32)) + [4503], True, 63), 60, 8),
    "nn64": lambda: graph_case("nn64", ring_list(7001, list(range(1, 33)), True, 64), 60, 9),
    "nn70": lambda: graph_case("nn70", ring_list(7001, list(range(1, 36)), False, 70), 60, 10),
    # nn70's N with local7's list: the two share one communicator in test_one_communicator_through_every_path
    "ring7_7001": lambda: graph_case("ring7_7001", ring_list(7001, [1, 2, 70], False, 7), 60, 14),
    "scatter": lambda: graph_case("scatter", ring_list(600077, [1] + [24576 * k + 5 for k in range(1, 13)], True, 26), 60, 11),
    "mixed": _mixed,
    "many": lambda: _many(4096),
    "many_capped": lambda: _many(777),
    "no_st": lambda: _no("no_st", 1700003, 12),
    "no_glds": lambda: _no("no_glds", 4200031, 13),
    "asym": _asym,
}
SYMMETRIC_CASES = [n for n in BUILDERS if n != "asym"]
REPLAYED = ("no_st", "no_glds")               # the two largest: the oracle's log is replayed instead of restated
WINDOWS = {"many": (1100, 4096), "many_capped": (777, 777), "tiny": (1, 3)}      # events per step; the others: 20 .. 400
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


def reference(oracle, name):
    """dict(t, n, log, el, ch) of the oracle's step on a case, computed once per process and never modified"""
    key = ("ref", name)
    if key not in _cache:
        t, n, log, el, ch = oracle_step(oracle, case(name))
        for a in (log, el, ch):
            a.setflags(write=False)
        _cache[key] = dict(t=t, n=n, log=log, el=el, ch=ch)
    return _cache[key]
