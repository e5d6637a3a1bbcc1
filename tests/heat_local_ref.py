"""numpy / scipy restatement of the local heat system ("Local heat solve"): the reference the tests hold
kmcf_update_temperature_local to.  Interface rows on the K pattern of oracle.KSystem, contact sites at T0.

    g_ij = kappa(i, j) * L_char,  kappa = k_th_metal (both metal) | k_th_vacancies (both uncharged vacancies) |
                                          k_th_non_vacancy (any other pair)
    (C/dt + sum_j g_ij + gL_i + gR_i) T_i - sum_j g_ij T_j = (C/dt) T_old_i + Q_i + (gL_i + gR_i) T0
    C = c_p 1e6 A t_ox / N_interface; steady state (no C/dt terms) when step_time > 1e3 delta_t.

heat_system + solve are the SOLUTION's reference (float64, scipy's direct solve).  heat_values_ref restates the assembled
system value by value from integer class counts in np.longdouble, for the synthetic devices of site_kernels_ref.k_device
(synth_case); tests/test_heat_local.py asserts that the two agree and the conditions the synthetic cases are built for,
tests/test_gpu_heat_synthetic.py holds the library to them."""
import functools
import types

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


# ------------------------------------------------------------------------------------------------ the system, value by value
def pair_class(ci, cj):
    """0 both metal, 1 both uncharged vacancies, 2 any other pair"""
    both = np.asarray(ci) & np.asarray(cj)
    return np.where(both & 1, 0, np.where(both & 2, 1, 2))


def steady_mode(step_time, p):
    """the mode switch as the header states it, in float64: strictly beyond 1e3 delta_t"""
    return bool(np.float64(step_time) > np.float64(1e3) * np.float64(p["delta_t"]))


def heat_values_ref(row_ptr, col, left, right, cls, p, step_time, site_power, T_old, N_left, n, row0=0):
    """dict(val, diag, dinv, rhs, left, right, off_diagonal, rows, cdt, steady) of one call, in the caller's row order, in
    the shape of site_kernels_ref.k_values_ref: (row_ptr, col) the interface rows [row0, row0 + len(row_ptr) - 1) with
    block-local (global interface) columns, left / right = (row_ptr, col) of the contact blocks of the same rows, cls the
    site classes of the whole device (site_classes), n the number of interface sites of the device.
    Off-diagonals: -(k_th_class * L_char) in float64, ONE correctly rounded product (what the host forms).  Vectors: from
    INTEGER class counts per row in np.longdouble -- diag = C/dt + sum_c n_c g_c over the interface, left and right
    entries, rhs = C/dt T_old + Q + (gL + gR) T0, dinv = 1 / diag, g_c and C/dt themselves formed in np.longdouble --
    and returned in np.longdouble; val (float64) holds diag rounded once on its diagonal entries."""
    LD = np.longdouble
    cls = np.asarray(cls)
    rp = np.asarray(row_ptr)
    nr = len(rp) - 1
    site = N_left + row0 + np.arange(nr)
    kth = np.array([p["k_th_metal"], p["k_th_vacancies"], p["k_th_non_vacancy"]], np.float64)
    g64 = kth * np.float64(p["L_char"])
    g = kth.astype(LD) * LD(p["L_char"])

    def counts(rp_, col_, site0, skip_diag):
        rp_ = np.asarray(rp_)
        rows = np.repeat(np.arange(nr), np.diff(rp_))
        c = np.asarray(col_, np.int64)[:rp_[-1]]
        k = pair_class(cls[site[rows]], cls[site0 + c])
        live = (c != row0 + rows) if skip_diag else np.ones(len(c), bool)
        cnt = np.stack([np.bincount(rows[live & (k == q)], minlength=nr) for q in range(3)], 1)
        return rows, c, k, cnt

    rows, c, k, cn = counts(rp, col, N_left, True)
    _, _, _, cl = counts(left[0], left[1], 0, False)
    _, _, _, cr = counts(right[0], right[1], N_left + n, False)
    assert cn.dtype.kind == "i" and cl.dtype.kind == "i" and cr.dtype.kind == "i"
    d, gl, gr = (cnt.astype(LD) @ g for cnt in (cn, cl, cr))
    steady = steady_mode(step_time, p)
    cdt = LD(0) if steady else LD(p["c_p"]) * LD(1e6) * LD(p["A"]) * LD(p["t_ox"]) / LD(n) / LD(step_time)
    tot = cdt + d + gl + gr
    rhs = cdt * np.asarray(T_old, np.float64)[site].astype(LD) + np.asarray(site_power, np.float64)[site].astype(LD) \
        + (gl + gr) * LD(p["background_temp"])
    on_diag = c == row0 + rows
    val = -g64[k]
    val[on_diag] = tot[rows[on_diag]].astype(np.float64)
    return dict(val=val, diag=tot, dinv=LD(1) / tot, rhs=rhs, left=gl, right=gr, off_diagonal=~on_diag, rows=rows,
                cdt=cdt, steady=steady, counts=(cn, cl, cr), pair_class=k)


def rel_error(got, want):
    """largest |got - want| / |want| in np.longdouble; where want is 0 (a row without contact entries, a steady row
    without power) got must be exactly 0, else the error is infinite"""
    got, want = np.asarray(got).astype(np.longdouble), np.asarray(want).astype(np.longdouble)
    if got.size == 0:
        return 0.0
    zero = want == 0
    err = np.abs(got - want) / np.where(zero, 1, np.abs(want))
    return float(np.where(zero, np.where(got == 0, 0.0, np.inf), err).max())


def pattern_system(pats, N_left):
    """the three patterns ((row_ptr, col) of interface, left, right) as the object heat_system reads"""
    (rp, col), (lrp, lcol), (rrp, rcol) = pats
    return types.SimpleNamespace(n=len(rp) - 1, N_left=N_left, row_ptr=rp, col=col, left_row_ptr=lrp, left_col=lcol,
                                 right_row_ptr=rrp, right_col=rcol)


def pcg_jacobi(A, b, x0, tol, max_iterations):
    """plain float64 Jacobi-PCG to the library's stopping rule sqrt(r.z / b.b) <= tol: (x, iterations)"""
    dinv = 1.0 / A.diagonal()
    x = np.array(x0, np.float64)
    r = b - A @ x
    z = dinv * r
    q = z.copy()
    rz, bb = r @ z, b @ b
    it = 0
    while np.sqrt(rz / bb) > tol and it < max_iterations:
        Aq = A @ q
        alpha = rz / (q @ Aq)
        x += alpha * q
        r -= alpha * Aq
        z = dinv * r
        rz_new = r @ z
        q = z + (rz_new / rz) * q
        rz = rz_new
        it += 1
    return x, it


# ------------------------------------------------------------------------------------------------ synthetic cases
# The 5 nm device's thermal constants on the synthetic devices of site_kernels_ref.k_device (a 60 x 21 x 21 A box):
# A = 21 A x 21 A, t_ox = 60 A.
SYNTH_PRM = dict(background_temp=300.0, L_char=3.5e-10, c_p=1.92, A=21e-10 * 21e-10, t_ox=60e-10, delta_t=1e-13)
# conductivity sets (k_th_metal, k_th_vacancies, k_th_non_vacancy) and the dictionary codes of the three pair classes:
# equal conductivities share a code, codes are handed out in class order
HEAT_SETS = {"distinct": (29.0, 5.0, 0.5), "metal_eq_vacancy": (29.0, 29.0, 0.5), "metal_eq_other": (0.5, 5.0, 0.5),
             "vacancy_eq_other": (29.0, 5.0, 5.0), "all_equal": (0.5, 0.5, 0.5)}
HEAT_CODES = {"distinct": [0, 1, 2], "metal_eq_vacancy": [0, 0, 1], "metal_eq_other": [0, 1, 0],
              "vacancy_eq_other": [0, 1, 1], "all_equal": [0, 0, 0]}
# step_time > 1e3 delta_t = 1e-10 s: steady state.  The transient step makes C/dt comparable to a row's conductance sum
# (C = 5.08e-20 J/K over 3880 .. 6370 sites, C/dt about 1e-8 W/K; at 1e-13 s it would be 1 % of the largest g)
SYNTH_STEP = {"steady": 1e-6, "transient": 1e-15}
SYNTH_Q_SCALE = 1e-8
SYNTH_CG = dict(cg_tolerance=1e-13, cg_max_iterations=20000)
SENTINEL = 123.0                                  # what the caller leaves in the contact slots of site_temperature


def synth_cases():
    """(device, pbc, conductivity set, mode) of every call the GPU tests compare: sparse x every set, dense x the
    distinct and the all-equal set, and the two-code set of the long-row test on dense under pbc 1"""
    out = [("sparse", pbc, k, m) for pbc in (0, 1) for k in HEAT_SETS for m in SYNTH_STEP]
    out += [("dense", pbc, k, m) for pbc in (0, 1) for k in ("distinct", "all_equal") for m in SYNTH_STEP]
    out += [("dense", 1, "metal_eq_other", m) for m in SYNTH_STEP]
    return out


def synth_params(kset):
    km, kv, ko = HEAT_SETS[kset]
    return dict(SYNTH_PRM, k_th_metal=km, k_th_vacancies=kv, k_th_non_vacancy=ko)


def dictionary_codes(p):
    """the code of each pair class: distinct values of -g in class order (kmcf_update_temperature_local's dictionary)"""
    g = conductances(p)
    seen, codes = [], []
    for v in g:
        if v not in seen:
            seen.append(v)
        codes.append(seen.index(v))
    return codes


@functools.lru_cache(maxsize=None)
def synth_patterns(name, pbc):
    import site_kernels_ref as R
    return R.k_patterns(R.k_device(name), pbc)


@functools.lru_cache(maxsize=None)
def synth_inputs(name):
    """(cls, cls2, Q, T_old) of a k_device: classes under charge and charge2, the source, the previous field (not flat on
    the interface, SENTINEL on the contacts), read-only"""
    import site_kernels_ref as R
    dev = R.k_device(name)
    NL, N = dev["NL"], dev["N"]
    cls = site_classes(dev["element"], dev["charge"], dev["metals"])
    cls2 = site_classes(dev["element"], dev["charge2"], dev["metals"])
    Q = synthetic_power(dev["element"], dev["charge"], dev["metals"], SYNTH_Q_SCALE)
    T_old = np.full(N, SENTINEL)
    T_old[NL:-NL] = SYNTH_PRM["background_temp"] + 5.0 * np.sin(0.013 * np.arange(N - 2 * NL)) ** 2
    for a in (cls, cls2, Q, T_old):
        a.flags.writeable = False
    return cls, cls2, Q, T_old


@functools.lru_cache(maxsize=None)
def synth_case(name, pbc, kset, mode):
    """One call on a synthetic device, computed once per process and handed out read-only:
    dict(p, step_time, ref: heat_values_ref, sys: heat_system, T: spsolve's field with the contacts at T0)."""
    import site_kernels_ref as R
    dev = R.k_device(name)
    NL, n, N = dev["NL"], dev["n"], dev["N"]
    pats = synth_patterns(name, pbc)
    cls, _, Q, T_old = synth_inputs(name)
    p, step_time = synth_params(kset), SYNTH_STEP[mode]
    ref = heat_values_ref(pats[0][0], pats[0][1], pats[1], pats[2], cls, p, step_time, Q, T_old, NL, n)
    s = heat_system(pattern_system(pats, NL), cls, p, step_time, Q, T_old)
    T = solve(s, p["background_temp"], N, NL)
    T.flags.writeable = False
    return dict(p=p, step_time=step_time, ref=ref, sys=s, T=T)
