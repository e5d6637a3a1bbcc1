"""numpy / scipy restatement of the event rates and of the KMC step ("Thermally coupled event rates"):
the reference the tests hold kmcf_event_rates and kmcf_execute_kmc_step_thermal to.

    EA  : the activation energy of build_event_list (src/kmc_events.cu:128-207)
    s   : the site whose temperature counts: j for generation, i for recombination and the two diffusions
    T_BG   P = freq / (exp(EA / (kB T_bg)) + 1e-200)
    EKIN   P = freq / (exp((EA - kB (T[s] - T_bg)) / (kB T_bg)) + 1e-200)
    T_SITE P = freq / (exp(EA / (kB T[s])) + 1e-200)

The step: cumulative sum of the rates, first slot whose cumulative rate exceeds u * total, execute, zero every slot that
touches i or j, t = -log(u') / total, until t >= 1 / freq or max_events.  The uniforms are the caller's (the tests draw
them from oracle.mt_uniform_stream)."""
import numpy as np

DEFECT, OXYGEN_DEFECT, VACANCY, O_EL = 0, 1, 2, 3
EV_GEN, EV_REC, EV_VDIFF, EV_ODIFF, EV_NULL = 0, 1, 2, 3, 4
T_BG, EKIN, T_SITE = 0, 1, 2
KB = 8.617333262e-5
EPSILON = 1e-200
Q = 1.60217663e-19


def _v_solve(r, charge, sigma, k):
    from scipy.special import erfc
    return charge * erfc(r / (sigma * np.sqrt(2.0))) * k * Q / r


def event_list(xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, T=None, mode=T_BG):
    """(type uint8, prob float64, site int32), each of shape neigh.shape; site = s of every slot (-1 on null slots)."""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    layer, pot, element, charge = np.asarray(layer), np.asarray(pot, np.float64), np.asarray(element), np.asarray(charge)
    # every event needs element[i] != O_EL: only those rows are evaluated (the same arithmetic per slot; lists of millions
    # of rows with a few hundred live ones would otherwise spend seconds in erfc), the others are null
    rows = np.flatnonzero(element != O_EL)
    if len(rows) < N:
        t, p, s = _event_list_rows(rows, xyz, neigh[rows], layer, T_bg, freq, sigma, k, pot, element, charge, layers, T, mode)
        typ, prob, site = np.full((N, nn), EV_NULL, np.uint8), np.zeros((N, nn)), np.full((N, nn), -1, np.int32)
        typ[rows], prob[rows], site[rows] = t, p, s
        return typ, prob, site
    return _event_list_rows(np.arange(N), xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, T, mode)


def _event_list_rows(rows, xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, T, mode):
    """event_list for the rows `rows` of the list; neigh holds these rows only, its entries are site ids"""
    N, nn = len(element), neigh.shape[1]
    E = [np.array([l[key] for l in layers], np.float64) for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]
    i = np.repeat(rows, nn).reshape(len(rows), nn)
    valid = (neigh >= 0) & (neigh < N)
    j = np.where(valid, neigh, 0)
    d = xyz[j] - xyz[i]
    dist = 1e-10 * np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    dist = np.where(valid & (dist > 0), dist, 1.0)
    ei, ej, ci, cj = element[i], element[j], charge[i].astype(np.int64), charge[j].astype(np.int64)
    dpot = pot[i] - pot[j]
    lj = layer[j]
    typ = np.full(neigh.shape, EV_NULL, np.uint8)
    EA = np.zeros(neigh.shape)
    # generation
    m = valid & (ei == DEFECT) & (ej == O_EL)
    EA = np.where(m, E[0][lj] - 2 * dpot - 0, EA)
    typ[m] = EV_GEN
    gen = m
    # recombination (charge_state / 2: C integer division, towards zero)
    m = valid & (ei == OXYGEN_DEFECT) & (ej == VACANCY)
    cs = ci - cj
    half = np.sign(cs) * (np.abs(cs) // 2)
    EA = np.where(m, E[1][lj] - cs * (dpot + half * _v_solve(dist, 2, sigma, k)) - 0, EA)
    typ[m] = EV_REC
    # vacancy diffusion
    m = valid & (ei == VACANCY) & (ej == O_EL)
    siv = np.where(ci != 0, _v_solve(dist, ci, sigma, k), 0.0)
    EA = np.where(m, E[2][lj] - (ci - cj) * (dpot + siv) - 0, EA)
    typ[m] = EV_VDIFF
    # ion diffusion
    m = valid & (ei == OXYGEN_DEFECT) & (ej == DEFECT)
    siv = np.where(ci != 0, _v_solve(dist, 2, sigma, k), 0.0)
    EA = np.where(m, E[3][lj] - (ci - cj) * (dpot - siv) - 0, EA)
    typ[m] = EV_ODIFF
    live = typ != EV_NULL
    site = np.where(live, np.where(gen, j, i), -1).astype(np.int32)
    with np.errstate(over="ignore"):
        if mode == T_BG:
            arg = EA / (KB * T_bg)
        else:
            Ts = np.asarray(T, np.float64)[np.where(live, site, 0)]
            if mode == EKIN:
                arg = (EA - KB * (Ts - T_bg)) / (KB * T_bg)
            elif mode == T_SITE:
                arg = EA / (KB * Ts)
            else:
                raise ValueError(mode)
        prob = np.where(live, freq * (1 / (np.exp(arg) + EPSILON)), 0.0)
    return typ, prob, site


def kmc_step(xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, uniforms, T=None, mode=T_BG,
             max_events=4096):
    """Returns (event_time, n_events, log[n, 3], element_after, charge_after, margins[n]).  margins: for every event,
    the distance of u * total from the nearest boundary between two slots of the cumulative sum, relative to total."""
    neigh = np.asarray(neigh)
    N, nn = neigh.shape
    typ, prob, _ = event_list(xyz, neigh, layer, T_bg, freq, sigma, k, pot, element, charge, layers, T, mode)
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


def hot_spot(xyz, T0=300.0, dT=1700.0, width=10.0, x0=25.0):
    """T = T0 + dT exp(-r^2 / (2 width^2)), r [A] from (x0, mean y, mean z)."""
    c = np.array([x0, xyz[:, 1].mean(), xyz[:, 2].mean()])
    r2 = ((xyz - c) ** 2).sum(axis=1)
    return T0 + dT * np.exp(-r2 / (2.0 * width ** 2))


def small_workload(km, oracle):
    """structure.synth_small(tiles=1) with the potentials of the oracle's K solve plus the pairwise term (as fields5 of
    tests/test_kmc_events.py builds them for the 5 nm device): dict(d, neigh, charge, lay, pot, layers, T_hot)."""
    d = km.structure.synth_small(tiles=1)
    NL, layers = d["N_contact"], km.structure.LAYERS
    ks = oracle.KSystem(d["xyz"], d["lattice"], d["pbc"], d["nn_dist"], NL, NL)
    neigh = oracle.neighbor_list(d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], d["nn_dist"], 52)
    charge = oracle.update_charge(d["element"], np.zeros(d["N"], np.int32), neigh, d["metals"])
    A = oracle.assemble_K(ks, d["element"], charge, d["metals"], d["high_G"], d["low_G"], d["Vd"])
    x, _, _ = oracle.pcg_jacobi(ks.row_ptr, ks.col, A["val"], A["rhs"], np.zeros(ks.n), A["dinv"], 1e-14 * ks.n, 10000)
    pot = oracle.poisson_gridless(d["xyz"], charge, d["sigma"], d["k"])
    pot[NL:NL + ks.n] += x
    xs = np.clip(d["xyz"][:, 0], layers[0]["start_x"], layers[-1]["end_x"])
    lay = km.solvers.site_layers(xs, layers)
    return dict(d=d, neigh=neigh, charge=charge, lay=lay, pot=pot, layers=layers, T_hot=hot_spot(d["xyz"]),
                T_bg=300.0, freq=1e14, seed=1, max_events=4096)
