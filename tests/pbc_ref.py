"""Plain numpy restatements for the periodic (y, z) paths -- kmcf_neighbor_list_pbc, kmcf_compute_cutoff_list_pbc +
kmcf_poisson_gridless, the event list after kmcf_events_set_lattice -- and the inputs they are tested on.  No GPU.

Everything here is brute force: all pairs, the distance written out operation for operation as include/kmcfield.h
states it, no cell list and no k-d tree, so that nothing is shared with the kernels it judges (nor with
structure.min_image_pairs, which tests/test_pbc_ref.py compares it with).  tests/test_pbc_ref.py asserts the conditions
every input is built for; tests/test_gpu_pbc.py holds the library to the restatements.  Inputs are built once per process
(lru_cache) and handed out read-only."""
import functools

import numpy as np
from scipy.special import erfc

Q_E = 1.60217663e-19                    # gpu_solvers.h:323
CUTOFF = 20.0
SENTINEL = 123.0
DEFECT, OXYGEN_DEFECT, VACANCY, O_EL = 0, 1, 2, 3
EV_GEN, EV_REC, EV_VDIFF, EV_ODIFF, EV_NULL = 0, 1, 2, 3, 4
KB = 8.617333262e-5
EPSILON = 1e-200


def _ro(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


# ------------------------------------------------------------------------------------------------ distance
def c_round(f):
    """C round(): half away from zero.  trunc, then one step where the (exact) remainder reaches a half."""
    f = np.asarray(f, np.float64)
    r = np.trunc(f)
    return r + np.where(np.abs(f - r) >= 0.5, np.sign(f), 0.0)


def dist(x1, y1, z1, x2, y2, z2, L=None):
    """L = (Lx, Ly, Lz): the reference's four-argument site_dist with pbc = 1 (src/gpu_solvers.h:287-319), every operation
    as written there; L None: the open-boundary expression of the pairwise and event kernels, (x2 - x1) etc."""
    if L is None:
        dx, dy, dz = x2 - x1, y2 - y1, z2 - z1
        return np.sqrt(dx * dx + dy * dy + dz * dz)
    dx = x1 - x2
    fy = (y1 - y2) / L[1]
    fy = fy - c_round(fy)
    dy = fy * L[1]
    fz = (z1 - z2) / L[2]
    fz = fz - c_round(fz)
    dz = fz * L[2]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def dist_matrix(xyz, cols, L=None):
    """dist(site i, site cols[c]) for every site i: N x len(cols)"""
    a, b = np.asarray(xyz, np.float64), np.asarray(xyz, np.float64)[cols]
    return dist(a[:, None, 0], a[:, None, 1], a[:, None, 2], b[None, :, 0], b[None, :, 1], b[None, :, 2], L)


# ------------------------------------------------------------------------------------------------ neighbour list
def neighbor_rows(xyz, L, nn_dist, nn):
    """(list, longest row): the first nn sites j != i with dist < nn_dist in ascending j, -1 padding"""
    N = len(xyz)
    D = dist_matrix(xyz, np.arange(N), L)
    near = D < nn_dist
    near[np.arange(N), np.arange(N)] = False
    out = np.full((N, nn), -1, np.int32)
    for i in range(N):
        lst = np.flatnonzero(near[i])[:nn]
        out[i, :len(lst)] = lst
    return out, int(near.sum(1).max())


def neighbor_stats(xyz, L, nn_dist):
    """dict(margin: smallest |dist / nn_dist - 1| over all pairs, wrap: pairs listed under the minimum image but not
    without it, longest: the longest row)"""
    N = len(xyz)
    D, D0 = dist_matrix(xyz, np.arange(N), L), dist_matrix(xyz, np.arange(N), None)
    off = ~np.eye(N, dtype=bool)
    return dict(margin=float(np.abs(D[off] / nn_dist - 1.0).min()), wrap=int(((D < nn_dist) & ~(D0 < nn_dist) & off).sum()) // 2,
                longest=int(((D < nn_dist) & off).sum(1).max()))


# ------------------------------------------------------------------------------------------------ pairwise term
def pairwise_ref(xyz, charge, L, sigma, k, cutoff=CUTOFF):
    """(want, S, n) per site, the terms written as in site_kernels_ref.pairwise_ref: want_i = sum over charged j != i with
    dist < cutoff of q_j erfc(r / (sigma sqrt 2)) k q / r, r = 1e-10 dist, each term the float64 expression with scipy's
    erfc, a site's terms ACCUMULATED in np.longdouble; S_i the float64 sum of their absolute values; n_i their number.
    dist: the minimum image under L, the open-boundary distance with L None."""
    charge = np.asarray(charge)
    N = len(xyz)
    cols = np.flatnonzero(charge != 0)
    D = dist_matrix(xyz, cols, L)
    m = D < cutoff
    m[cols, np.arange(len(cols))] = False                       # j == i
    r = 1e-10 * np.where(m, D, 1.0)
    term = np.where(m, charge[cols].astype(np.float64)[None, :] * erfc(r / (sigma * np.sqrt(2.0))) * k * Q_E / r, 0.0)
    want = term.astype(np.longdouble).sum(1) if len(cols) else np.zeros(N, np.longdouble)
    S = np.abs(term).sum(1) if len(cols) else np.zeros(N)
    return want, S, m.sum(1).astype(np.int64)


def pairwise_stats(xyz, charge, L, cutoff=CUTOFF):
    """dict(margin: smallest |dist / cutoff - 1| over the (site, charged site) pairs NOT at exactly the cutoff, exact: pairs at
    exactly it, wrap: pairs inside the cutoff under the minimum image but not without it)"""
    cols = np.flatnonzero(np.asarray(charge) != 0)
    D, D0 = dist_matrix(xyz, cols, L), dist_matrix(xyz, cols, None)
    D[cols, np.arange(len(cols))] = np.inf
    rel = np.abs(D / cutoff - 1.0)
    return dict(margin=float(rel[D != cutoff].min()), exact=int((D == cutoff).sum()), wrap=int(((D < cutoff) & ~(D0 < cutoff)).sum()))


def cells_per_period(L, cutoff=CUTOFF):
    """cells of the periodic index in (y, z): max(1, floor(L / cutoff))"""
    return tuple(max(1, int(np.floor(L[a] / cutoff))) for a in (1, 2))


# name: (N, box (x extent, Ly, Lz), seed, cells in (y, z))
RANDOM_CASES = {"p11": (600, (45.0, 25.0, 30.0), 32, (1, 1)), "p23": (1500, (45.0, 45.0, 65.0), 33, (2, 3)),
                "p34": (3000, (45.0, 60.0, 85.0), 34, (3, 4)), "p52": (3000, (30.0, 104.0, 47.0), 35, (5, 2))}
PAIRWISE_CASES = tuple(RANDOM_CASES) + ("lattice_wrap",)
# further charge vectors on a case's sites (one index serves them): a single charged site, site 0 on the face y = 0 --
# itself and every site beyond the cutoff are left without a term -- and no charged site at all
CHARGE_VARIANTS = {"p23": ("p23", "p23_one", "p23_none")}
NEIGHBOR_CASES = {"p11": 3.5, "p34": 3.5, "p52": 3.5, "lattice_wrap": 4.1}          # name: nn_dist
NN = 16                                  # slots of the full lists: above the longest row (asserted <= 11)
NN_TRUNCATED = 4
# p11 once more with a reach of which fewer than 3 cells fit a period (floor(25 / 9) = 2): the list's brute-force path
FALLBACK_CASE, FALLBACK_NN_DIST, FALLBACK_NN = "p11", 9.0, 64


@functools.lru_cache(maxsize=None)
def pairwise_case(name):
    """dict(xyz, charge, L, slices [(displ, count), ...], N, cells) of one periodic input, read-only: 30 % of the sites
    charged +-2; random cases: uniform in the box, the first four sites pinned to y = 0, y = nextafter(Ly, 0), z = 0,
    z = nextafter(Lz, 0) (the faces of the period: first and last cell, the clamp of the cell coordinate).
    lattice_wrap: 12 x 16 x 16 sites at 4 A in a period of 64 A -- all arithmetic exact, pairs at exactly 20.0 (4 x (3, 4, 0),
    4 x (0, 0, 5)), many across the wrap."""
    if name in ("p23_one", "p23_none"):
        base = pairwise_case("p23")
        charge = np.zeros(base["N"], np.int32)
        if name == "p23_one":
            charge[0] = -2
        return dict(base, name=name, charge=_ro(charge), slices=[(0, base["N"])])
    if name == "lattice_wrap":
        rng = np.random.default_rng(31)
        g = np.stack(np.meshgrid(np.arange(12), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
        xyz = g.astype(np.float64) * 4.0
        L = np.array([48.0, 64.0, 64.0])
        N = len(xyz)
        slices = [(0, N)]
    else:
        N, box, seed, _ = RANDOM_CASES[name]
        rng = np.random.default_rng(seed)
        L = np.array(box)
        xyz = rng.random((N, 3)) * L
        xyz[0, 1], xyz[1, 1] = 0.0, np.nextafter(L[1], 0.0)
        xyz[2, 2], xyz[3, 2] = 0.0, np.nextafter(L[2], 0.0)
        slices = [(0, N), (0, 0), (N - 1, 1), (N // 3 + 5, N // 4 + 3)]
    charge = np.zeros(N, np.int32)
    idx = rng.choice(N, 3 * N // 10, replace=False)
    charge[idx] = rng.choice([-2, 2], len(idx))
    _ro(xyz, charge, L)
    return dict(name=name, xyz=xyz, charge=charge, L=L, slices=slices, N=N, cells=cells_per_period(L))


@functools.lru_cache(maxsize=None)
def pairwise_reference(name, sigma, k, periodic=True):
    c = pairwise_case(name)
    return _ro(*pairwise_ref(c["xyz"], c["charge"], c["L"] if periodic else None, sigma, k))


@functools.lru_cache(maxsize=None)
def neighbor_reference(name, nn_dist, nn):
    c = pairwise_case(name)
    rows, longest = neighbor_rows(c["xyz"], c["L"], nn_dist, nn)
    return _ro(rows), longest


# ------------------------------------------------------------------------------------------------ event list
def _v_solve(r, charge, sigma, k):
    return charge * erfc(r / (sigma * np.sqrt(2.0))) * k * Q_E / r


def event_list(xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, L=None):
    """(type uint8, prob float64) of shape neigh.shape: the rate formulas of events_thermal_ref.event_list in the
    background-temperature mode, the pair distance taken from dist() above (L None: open boundaries)."""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    xyz = np.asarray(xyz, np.float64)
    layer, pot, element, charge = np.asarray(layer), np.asarray(pot, np.float64), np.asarray(element), np.asarray(charge)
    E = [np.array([l[key] for l in layers], np.float64) for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]
    i = np.repeat(np.arange(N), nn).reshape(N, nn)
    valid = (neigh >= 0) & (neigh < N)
    j = np.where(valid, neigh, 0)
    d = 1e-10 * dist(xyz[i, 0], xyz[i, 1], xyz[i, 2], xyz[j, 0], xyz[j, 1], xyz[j, 2], L)
    d = np.where(valid & (d > 0), d, 1.0)
    ei, ej, ci, cj = element[i], element[j], charge[i].astype(np.int64), charge[j].astype(np.int64)
    dpot = pot[i] - pot[j]
    lj = layer[j]
    typ = np.full(neigh.shape, EV_NULL, np.uint8)
    EA = np.zeros(neigh.shape)
    m = valid & (ei == DEFECT) & (ej == O_EL)                                   # generation
    EA = np.where(m, E[0][lj] - 2 * dpot - 0, EA)
    typ[m] = EV_GEN
    m = valid & (ei == OXYGEN_DEFECT) & (ej == VACANCY)                         # recombination (cs / 2 towards zero)
    cs = ci - cj
    half = np.sign(cs) * (np.abs(cs) // 2)
    EA = np.where(m, E[1][lj] - cs * (dpot + half * _v_solve(d, 2, sigma, k)) - 0, EA)
    typ[m] = EV_REC
    m = valid & (ei == VACANCY) & (ej == O_EL)                                  # vacancy diffusion
    siv = np.where(ci != 0, _v_solve(d, ci, sigma, k), 0.0)
    EA = np.where(m, E[2][lj] - (ci - cj) * (dpot + siv) - 0, EA)
    typ[m] = EV_VDIFF
    m = valid & (ei == OXYGEN_DEFECT) & (ej == DEFECT)                          # ion diffusion
    siv = np.where(ci != 0, _v_solve(d, 2, sigma, k), 0.0)
    EA = np.where(m, E[3][lj] - (ci - cj) * (dpot - siv) - 0, EA)
    typ[m] = EV_ODIFF
    live = typ != EV_NULL
    with np.errstate(over="ignore"):
        prob = np.where(live, freq * (1 / (np.exp(EA / (KB * T_bg)) + EPSILON)), 0.0)
    return typ, prob


def kmc_step(neigh, typ, prob, freq, element, charge, uniforms, max_events):
    """The step of events_thermal_ref.kmc_step on a given event list: (event_time, n_events, log[n, 3], element_after,
    charge_after, margins[n])."""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    typ, prob = typ.reshape(-1).copy(), prob.reshape(-1).copy()
    flat = neigh.reshape(-1)
    el, ch = np.array(element, np.int32), np.array(charge, np.int32)
    log, margins = [], []
    t, n = 0.0, 0
    while t < 1 / freq and n < max_events:
        cum = np.cumsum(prob)
        total = cum[-1]
        number = uniforms[2 * n] * total
        idx = min(int(np.searchsorted(cum, number, side="right")), len(cum) - 1)
        lo = cum[idx - 1] if idx > 0 else 0.0
        margins.append(min(number - lo, cum[idx] - number) / total)
        i, j, et = idx // nn, int(flat[idx]), int(typ[idx])
        log.append((i, j, et))
        if et == EV_GEN:
            el[i], el[j], ch[i], ch[j] = OXYGEN_DEFECT, VACANCY, -2, 2
        elif et == EV_REC:
            el[i], el[j], ch[i], ch[j] = DEFECT, O_EL, 0, 0
        elif et in (EV_VDIFF, EV_ODIFF):
            el[i], el[j] = el[j], el[i]
            ch[i], ch[j] = ch[j], ch[i]
        dead = (flat == i) | (flat == j)
        dead[i * nn:(i + 1) * nn] |= flat[i * nn:(i + 1) * nn] >= 0
        dead[j * nn:(j + 1) * nn] |= flat[j * nn:(j + 1) * nn] >= 0
        prob[dead] = 0.0
        typ[dead] = EV_NULL
        t = -np.log(uniforms[2 * n + 1]) / total
        n += 1
    return t, n, np.array(log, np.int32).reshape(-1, 3), el, ch, np.array(margins)


# ------------------------------------------------------------------------------------------------ small periodic box
BOX_NN_DIST, BOX_NN = 3.5, 20
BOX_CHAIN = (3, 4, 0, 1)                 # y indices of the vacancy chain of box(): it leaves at y = Ly and re-enters at y = 0


@functools.lru_cache(maxsize=None)
def box():
    """A 12 x 5 x 6 lattice at 2.5 A, jittered by +-0.3 A, in a period of 12.5 x 15 A; x from 0.3 A on, across the interface
    and oxide layers of structure.LAYERS.  Every site has its six lattice neighbours within 3.5 A, those of the first
    and last plane in y and z across the wrap.  Elements: 40 % O, 20 % each of defect, oxygen defect (-2) and vacancy
    (+2, every fifth one neutral), so that recombination, vacancy-diffusion and ion-diffusion pairs lie across the wrap
    (asserted in tests/test_pbc_ref.py).  dict(xyz, L, element, charge, pot, N, grid), read-only."""
    rng = np.random.default_rng(36)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(5), np.arange(6), indexing="ij"), -1).reshape(-1, 3)
    xyz = g * 2.5 + rng.uniform(-0.3, 0.3, g.shape) + np.array([0.6, 0.3, 0.3])
    L = np.array([36.0, 12.5, 15.0])
    N = len(xyz)
    element = rng.choice([O_EL, DEFECT, OXYGEN_DEFECT, VACANCY], N, p=[0.4, 0.2, 0.2, 0.2]).astype(np.int32)
    charge = np.where(element == OXYGEN_DEFECT, -2, np.where(element == VACANCY, 2, 0)).astype(np.int32)
    vac = np.flatnonzero(element == VACANCY)
    charge[vac[::5]] = 0
    pot = rng.uniform(-0.4, 0.4, N)
    _ro(xyz, L, element, charge, pot, g)
    return dict(xyz=xyz, L=L, element=element, charge=charge, pot=pot, N=N, grid=g)


@functools.lru_cache(maxsize=None)
def box_lists():
    """(periodic list, open list) of box(), BOX_NN slots"""
    b = box()
    return neighbor_rows(b["xyz"], b["L"], BOX_NN_DIST, BOX_NN)[0], neighbor_rows(b["xyz"], None, BOX_NN_DIST, BOX_NN)[0]


def wrap_slots(xyz, neigh, L, nn_dist):
    """mask of the list slots whose pair is a neighbour only under the minimum image"""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    i = np.repeat(np.arange(N), nn).reshape(N, nn)
    j = np.where(neigh >= 0, neigh, 0)
    d0 = dist(xyz[i, 0], xyz[i, 1], xyz[i, 2], xyz[j, 0], xyz[j, 1], xyz[j, 2], None)
    return (neigh >= 0) & ~(d0 < nn_dist)


@functools.lru_cache(maxsize=None)
def chain():
    """box() with every site O except a chain of four neutral vacancies along y at grid (5, *, 2), y indices BOX_CHAIN:
    dict(element, charge, sites: the chain's site ids in chain order)."""
    b = box()
    g = b["grid"]
    element = np.full(b["N"], O_EL, np.int32)
    sites = np.array([int(np.flatnonzero((g[:, 0] == 5) & (g[:, 1] == yy) & (g[:, 2] == 2))[0]) for yy in BOX_CHAIN])
    element[sites] = VACANCY
    charge = np.zeros(b["N"], np.int32)
    _ro(element, charge, sites)
    return dict(element=element, charge=charge, sites=sites)
