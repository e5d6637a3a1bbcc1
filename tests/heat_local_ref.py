"""numpy / scipy restatement of the local heat system ("Local heat solve"): the reference the tests hold
kmcf_update_temperature_local to.  Interface rows on the K pattern of oracle.KSystem, contact sites at T0.

    g_ij = kappa(i, j) * L_char,  kappa = k_th_metal (both metal) | k_th_vacancies (both uncharged vacancies) |
                                          k_th_non_vacancy (any other pair)
    (C/dt + sum_j g_ij + gL_i + gR_i) T_i - sum_j g_ij T_j = (C/dt) T_old_i + Q_i + (gL_i + gR_i) T0
    C = c_p 1e6 A t_ox / N_interface; steady state (no C/dt terms) when step_time > 1e3 delta_t."""
import numpy as np

VACANCY = 2


def site_classes(element, charge, metals):
    """bit 0: metal, bit 1: uncharged vacancy (the classes of K's high_G rule)."""
    element = np.asarray(element)
    cls = np.isin(element, np.asarray(metals)).astype(np.uint8)
    cls |= (((element == VACANCY) & (np.asarray(charge) == 0)).astype(np.uint8) << 1)
    return cls


def conductances(p):
    return np.array([p["k_th_metal"], p["k_th_vacancies"], p["k_th_non_vacancy"]]) * p["L_char"]


def pair_g(ci, cj, g):
    both = ci & cj
    return np.where(both & 1, g[0], np.where(both & 2, g[1], g[2]))


def heat_system(ks, cls, p, step_time, site_power, T_old):
    """dict(A (scipy CSR, interface rows), b, gL, gR, cdt, C, steady, g) of one call."""
    import scipy.sparse as sp
    n, NL = ks.n, ks.N_left
    g = conductances(p)
    rp, col = np.asarray(ks.row_ptr), np.asarray(ks.col)
    rows = np.repeat(np.arange(n), np.diff(rp))
    off = rows != col
    r_off, c_off = rows[off], col[off]
    g_off = pair_g(cls[NL + r_off], cls[NL + c_off], g)
    d_int = np.bincount(r_off, weights=g_off, minlength=n)

    def contact_sum(crp, ccol, site0):
        crp = np.asarray(crp)
        cr = np.repeat(np.arange(n), np.diff(crp))
        return np.bincount(cr, weights=pair_g(cls[NL + cr], cls[site0 + np.asarray(ccol)], g), minlength=n)

    gL = contact_sum(ks.left_row_ptr, ks.left_col, 0)
    gR = contact_sum(ks.right_row_ptr, ks.right_col, NL + n)
    C = p["c_p"] * 1e6 * p["A"] * p["t_ox"] / n
    steady = step_time > 1e3 * p["delta_t"]
    cdt = 0.0 if steady else C / step_time
    diag = cdt + d_int + gL + gR
    A = sp.csr_matrix((np.concatenate([-g_off, diag]), (np.concatenate([r_off, np.arange(n)]),
                                                         np.concatenate([c_off, np.arange(n)]))), shape=(n, n))
    T0 = p["background_temp"]
    b = cdt * np.asarray(T_old)[NL:NL + n] + np.asarray(site_power)[NL:NL + n] + (gL + gR) * T0
    return dict(A=A, b=b, gL=gL, gR=gR, cdt=cdt, C=C, steady=steady, g=g, diag=diag, d_int=d_int)


def solve(sysd, T0, N, NL):
    """Whole field: the interface solved directly, contacts at T0."""
    import scipy.sparse.linalg as sla
    T = np.full(N, float(T0))
    T[NL:NL + sysd["A"].shape[0]] = sla.spsolve(sysd["A"].tocsc(), sysd["b"])
    return T


def synthetic_power(element, charge, metals, scale=1.0):
    """Deterministic source: positive on the vacancy sites (more on uncharged ones), zero elsewhere [W]."""
    element = np.asarray(element)
    q = np.zeros(len(element))
    vac = element == VACANCY
    idx = np.nonzero(vac)[0]
    q[idx] = 1.0 + 0.5 * np.cos(0.37 * idx) + (np.asarray(charge)[idx] == 0)
    return q * scale
