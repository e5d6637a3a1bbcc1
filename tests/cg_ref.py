"""A plain reference for CG tests: textbook (Jacobi-)PCG in numpy, the small seeded systems to run it on, and the bars
a device solve of them is to be held to.  tests/test_cg_ref.py holds the conditions these inputs and bars must meet;
tests/test_gpu_cg_paths.py compares every SpMV path's solve with them.

The reference is the recurrence of dist_conjugate_gradient.cpp:149-276 written down once more, row sums and dot
products in the order numpy adds them, in the precision the caller names: np.longdouble (64-bit mantissa on x86: the
reference) or np.float64 (only to measure how far a correct f64 run in ANOTHER summation order lies from it).  The
single-reduction recurrence (cg1r) gives the same iterates in exact arithmetic, so this one serves both."""
import numpy as np

U = 2.0 ** -53                     # unit roundoff of the device's arithmetic
VALUES3 = np.array([-1.0, -0.125, -3.0])                    # <= 3 distinct off-diagonals: row per lane, coded
VALUES5 = np.array([-1.0, -0.125, -3.0, -0.5, -2.0])        # 4 ... 62: coded window kernel


def _matvec(M, dtype):
    ip, ix, d = M.indptr, M.indices, M.data.astype(dtype)
    assert np.all(np.diff(ip) > 0), "every row holds its diagonal"
    return lambda v: np.add.reduceat(d * v[ix], ip[:-1])


def pcg_reference(M, b, x0, dinv, k, dtype, alpha_scale=None, beta_scale=None):
    """k iterations of PCG on the scipy CSR matrix M from x0; dinv = 1 / diag (Jacobi) or None (no preconditioner).
    Returns dict(alpha=[k], rz=[k + 1] (rz[0] before the first iteration, rz[j] after iteration j), x=[k], r=[k]
    (after each iteration), bb, res=[k + 1] (sqrt(rz / bb): what the loop compares with its tolerance)).
    alpha_scale = {j: s}: iteration j (1-based) takes s * alpha instead of alpha (beta_scale: s * beta) -- the
    sensitivity checks' deliberately wrong run."""
    mv = _matvec(M, dtype)
    b = np.asarray(b).astype(dtype)
    x = np.asarray(x0).astype(dtype)
    di = None if dinv is None else np.asarray(dinv).astype(dtype)
    r = b - mv(x)
    z = r if di is None else di * r
    p = z.copy()
    rz = (r * z).sum()
    out = dict(alpha=[], rz=[rz], x=[], r=[], bb=(b * b).sum())
    for j in range(1, k + 1):
        Ap = mv(p)
        a = rz / (p * Ap).sum()
        if alpha_scale and j in alpha_scale:
            a = a * dtype(alpha_scale[j])
        x = x + a * p
        r = r - a * Ap
        z = r if di is None else di * r
        rzn = (r * z).sum()
        be = rzn / rz
        if beta_scale and j in beta_scale:
            be = be * dtype(beta_scale[j])
        p = z + be * p
        rz = rzn
        out["alpha"].append(a)
        out["rz"].append(rz)
        out["x"].append(x)
        out["r"].append(r)
    out["res"] = [float(np.sqrt(v / out["bb"])) for v in out["rz"]]
    return out


def iterations_to(ref, tol):
    """Iterations a solve to the relative tolerance tol takes: the first j with sqrt(rz[j] / bb) <= tol."""
    for j, v in enumerate(ref["res"]):
        if v <= tol:
            return j
    raise AssertionError("the reference was not run far enough for tolerance %g" % tol)


def count_tolerance(ref, floor=1e-10):
    """The tolerance of an iteration-count check on a system whose PCG TERMINATES (count_rhs): the stopping iteration j
    is the first whose residual lies below `floor` (what an f64 recurrence leaves of a long-double residual of 1e-17 is
    its own rounding, so such a residual counts as `floor`), and the tolerance the geometric mean of floor and the
    smallest earlier residual, at most 10 x floor: a step length off by 1e-5 must still be seen.
    Returns (tol, j, margin): floor * margin <= tol and tol * margin <= res[i] for every i < j."""
    res = ref["res"]
    j = next(i for i, v in enumerate(res) if v < floor)
    above = min(res[:j])
    tol = float(floor * min(np.sqrt(above / floor), 10.0))
    return tol, j, float(min(tol / floor, above / tol))


def count_conditions(ref, tol, floor=1e-10):
    """The threshold condition of a count check, from the reference alone: (iterations the reference takes to tol,
    factor by which its residual there lies below tol, factor by which every earlier one lies above)."""
    res = ref["res"]
    j = iterations_to(ref, tol)
    return j, tol / max(res[j], floor), min(res[:j]) / tol


def _finish(P, rng_v, values):
    """Symmetric values on the symmetric 0/1 pattern P (strict upper triangle drawn, mirrored), then the diagonal:
    1.5 x the row's off-diagonal absolute sum + 1 + uniform[0, 1)."""
    import scipy.sparse as sp
    U_ = sp.triu(P, 1).tocsr()
    U_.sort_indices()
    d_rand = rng_v.random(P.shape[0])
    if values is None:
        U_.data = -(0.1 + 3.0 * rng_v.random(U_.nnz))
        assert len(np.unique(U_.data)) > 62
    else:
        U_.data = rng_v.choice(np.asarray(values), U_.nnz)
    M = (U_ + U_.T).tocsr()
    off = np.abs(M).sum(1).A1
    M = (M + sp.diags(1.5 * off + 1.0 + d_rand)).tocsr()
    M.sort_indices()
    return M


def _pattern(n, kmax, reach, long_row, seed):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(n):
        k = int(rng.integers(1, kmax + 1))
        c = np.arange(max(0, i - reach), min(n, i + reach + 1))
        c = rng.choice(c[c != i], size=min(k, len(c) - 1), replace=False)
        rows += [i] * len(c)
        cols += list(c)
    if long_row is not None:
        c = rng.choice(n, 700, replace=False)
        c = c[c != long_row]
        rows += [long_row] * len(c)
        cols += list(c)
    P = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    return ((P + P.T) > 0).astype(float).tocsr()


def ragged(n, values=VALUES3, long_row=True, seed=7):
    """n rows of 1 to 32 drawn off-diagonal entries within +-200 of the diagonal (more after symmetrisation), with
    long_row one row and column (row 11) of about 700 entries: beyond KMCF_LONG_ROW = 384.  values: the set the
    off-diagonals are drawn from, or None for all distinct; the PATTERN depends on (n, long_row, seed) only, so
    set_values moves one matrix object between the value sets."""
    P = _pattern(n, 32, 200, 11 if long_row else None, seed)
    return _finish(P, np.random.default_rng(seed + 1000), values)


def tiny(values=VALUES3, seed=3):
    """40 rows of 1 to 6 drawn off-diagonal entries: fewer rows, tiles and chunks than any kernel's smallest grid
    has blocks, so most blocks of every pass contribute a partial of nothing."""
    P = _pattern(40, 6, 12, None, seed)
    return _finish(P, np.random.default_rng(seed + 1000), values)


def first_step_inputs(M, jacobi=True, seed=5):
    """(x0, b): x0 = 0 and a right-hand side whose FIRST search direction lies in [1, 1.25]: with q uniform there,
    b = diag * q for the Jacobi solve and b = q without preconditioner.  With the builders' diagonal dominance every
    row's term p_i (A p)_i of p0.Ap0 is then positive and of comparable size."""
    n = M.shape[0]
    q = 1.0 + 0.25 * np.random.default_rng(seed).random(n)
    return np.zeros(n), (M.diagonal() * q if jacobi else q)


def first_direction(M, b, jacobi=True):
    """(p0, dinv) of a solve of b from x0 = 0: the first search direction as f64 arithmetic forms it, fl(dinv * b) or b
    (dinv = None), so that x1 / p0 = alpha0 in every entry of an f64 run, to its two roundings."""
    if not jacobi:
        return b.copy(), None
    dinv = 1.0 / M.diagonal()
    return dinv * b, dinv


def first_step_terms(M, p0):
    """In long double: (row terms p_i (A p)_i of p0.Ap0, |p|^T |A| |p| / p^T A p)."""
    ld = np.longdouble
    p = p0.astype(ld)
    t = p * _matvec(M, ld)(p)
    Mabs = abs(M)
    return t, float((p * _matvec(Mabs, ld)(p)).sum() / t.sum())


def alpha0_bar(M, p0):
    """Relative bound of the first step length: 2 (n + L) u |p|^T|A||p| / p^T A p, L = longest row -- the standard
    bound of a dot product of n terms over row sums of <= L terms, twice (p.Ap and r.z; r.z alone has no cancellation)."""
    L = int(np.diff(M.indptr).max())
    return 2.0 * (M.shape[0] + L) * U * first_step_terms(M, p0)[1]


def rel_max(a, ref):
    """Relative max-norm distance of a from the (long double) ref."""
    return float(np.abs(np.asarray(a).astype(np.longdouble) - ref).max() / np.abs(ref).max())


def rel(a, ref):
    return float(abs(np.longdouble(a) - ref) / abs(ref))


SYSTEMS = {"ragged": lambda values: ragged(6000, values),
           "ragged_nolong": lambda values: ragged(6000, values, long_row=False), "tiny": tiny}
VALUE_SETS = {"v3": VALUES3, "v5": VALUES5, "f64": None}
K_STEPS = (1, 2, 5)
_cache = {}


def system(name, values, jacobi):
    """One test system with everything the checks need, computed once per process and never written to:
    M, x0, b, p0, dinv (None without preconditioner), ref (long double, 25 iterations), f64 (the float64 run, 5
    iterations), a0bar (the first step's bar), and the count check's right-hand side cb, its reference cref and
    (tol, stop, margin)."""
    key = (name, values, bool(jacobi))
    if key not in _cache:
        M = SYSTEMS[name](VALUE_SETS[values])
        x0, b = first_step_inputs(M, jacobi)
        p0, dinv = first_direction(M, b, jacobi)
        ref = pcg_reference(M, b, x0, dinv, 25, np.longdouble)
        f64 = pcg_reference(M, b, x0, dinv, max(K_STEPS), np.float64)
        cb = count_rhs(M, jacobi)
        cref = pcg_reference(M, cb, x0, dinv, 12, np.longdouble)
        tol, stop, margin = count_tolerance(cref)
        s = dict(name=name, values=values, jacobi=bool(jacobi), M=M, x0=x0, b=b, p0=p0, dinv=dinv, ref=ref, f64=f64,
                 cb=cb, cref=cref, tol=tol, stop=stop, margin=margin, a0bar=alpha0_bar(M, p0),
                 L=int(np.diff(M.indptr).max()))
        for v in (x0, b, p0, cb) + (() if dinv is None else (dinv,)):       # (shared between tests: nobody writes to them)
            v.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def step_bars(s, k, factor=16.0):
    """Bars of the iterates after k iterations: factor x the distance of the float64 numpy run from the long-double
    reference (relative max-norm for x and r, relative error for r.z).  The device works at the same unit roundoff in
    another summation order; the factor covers the spread between orders and nothing more.
    A caution from the CPU: that distance is ONE draw of a rounding error.  numpy's r.z lies below u / 5 on four of
    the eighteen systems, and float64 runs that merely add in another order (rows permuted, strided dot products) lay
    up to 85 x further out for r.z and 56 x for r (x: 11 x at most), in 10 of 162 comparisons.  Two derived bounds
    were worked out in its place and are not used: worst-case dot-product constants (n u) carried through the
    recurrence, or through its exact first-order sensitivities, give 1e-8 ... 1e-5 for r after 5 iterations, blind
    to a step length off by 1e-9."""
    ref, f64 = s["ref"], s["f64"]
    out = dict(x=factor * rel_max(f64["x"][k - 1], ref["x"][k - 1]), r=factor * rel_max(f64["r"][k - 1], ref["r"][k - 1]),
               rz=factor * rel(f64["rz"][k], ref["rz"][k]))
    if k == 1:
        # Measured on an MI355X: r1.z1 of a correct solve (alpha0 2.3 u off, every other figure within its bar) lies
        # 4.4 u from the reference on ragged / v5 / Jacobi, where numpy's own run happens to lie 0.14 u from it: 32.3 x.
        # As the issue provides for this case, r1.z1 takes the derived bound of the first step instead.
        out["rz"] = first_step_bars(s)["rz"]
    return out


def step_distance(s, k, x, r, rz):
    """(x, r, rz) distances of a run's iterates after k iterations from the long-double reference, as step_bars measures."""
    ref = s["ref"]
    return dict(x=rel_max(x, ref["x"][k - 1]), r=rel_max(r, ref["r"][k - 1]), rz=rel(rz, ref["rz"][k]))


def count_rhs(M, jacobi=True, m=5):
    """A right-hand side for an iteration-count check on ANY symmetric positive definite M.  (With a generic
    right-hand side the tests' matrices lower the residual by a steady factor of about 3 per iteration, and no
    tolerance lies a factor 2 from both its neighbours.)  b = D^(1/2) V c with V = m eigenvectors of the Jacobi-scaled
    D^(-1/2) M D^(-1/2) from both ends of its spectrum (D = I without preconditioner).  PCG from x0 = 0 then ends at
    iteration m with a residual drop of many orders -- if its step lengths are right; a wrong p.Ap leaves components
    behind and the loop goes on."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    n = M.shape[0]
    m = min(m, n - 1)
    d = M.diagonal() if jacobi else np.ones(n)
    S = sp.diags(1.0 / np.sqrt(d))
    B = (S @ M @ S).tocsr()
    if n <= 64:
        w, V = np.linalg.eigh(B.toarray())
        pick = list(range((m + 1) // 2)) + list(range(n - m // 2, n))
        w, V = w[pick], V[:, pick]
    else:
        w, V = spl.eigsh(B, k=m, which="BE", tol=0, v0=np.ones(n), maxiter=200000)
    c = 1.0 / (1.0 + np.arange(V.shape[1]))
    V = V * np.sign(V[np.abs(V).argmax(0), np.arange(V.shape[1])])      # (a sign convention: eigenvectors come with either)
    return np.sqrt(d) * (V @ c)


def count_case(M, jacobi=True):
    """(reference, tolerance, iterations) of a count check on M with count_rhs: ref["b"] is the right-hand side."""
    b = count_rhs(M, jacobi)
    ref = pcg_reference(M, b, np.zeros(M.shape[0]), 1.0 / M.diagonal() if jacobi else None, 12, np.longdouble)
    ref["b"] = b
    tol, stop, _ = count_tolerance(ref)
    return ref, tol, stop


def first_step_bars(s):
    """Relative bars of the scalars a one-iteration solve returns, from the long-double reference, in the style of
    alpha0_bar.  bb = b.b: n squares of one sign, 2 n u.  rz = r1.z1 with r1 = b - alpha0 A p0, where b and alpha0 A p0
    cancel: entry i of r1 carries (L_i + 2) u (|b_i| + alpha0 (|A||p0|)_i) from its row sum, product and difference and
    e alpha0 |A p0|_i from a step length off by e = alpha0_bar; then |d rz| <= sum w_i (2 |r_i| d_i + d_i^2) + (n + 2) u rz
    with w = dinv (or 1)."""
    ld = np.longdouble
    M, ref = s["M"], s["ref"]
    n = M.shape[0]
    a, r1, p = ref["alpha"][0], ref["r"][0], s["p0"].astype(ld)
    Ap = _matvec(M, ld)(p)
    absAp = _matvec(abs(M), ld)(p)
    w = np.ones(n, ld) if s["dinv"] is None else s["dinv"].astype(ld)
    d = (np.diff(M.indptr) + 2) * U * (np.abs(s["b"]).astype(ld) + a * absAp) + s["a0bar"] * a * np.abs(Ap)
    rz = ref["rz"][1]
    return dict(bb=2.0 * n * U, rz=float(((w * (2 * np.abs(r1) * d + d * d)).sum() + (n + 2) * U * rz) / rz))

