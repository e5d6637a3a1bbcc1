"""Small seeded SPD systems that put the register-resident PCG launch (csrc/kmcf_cgr.hip) at its own edges, with the
plan each of them must run under.  tests/test_cgr_cases_ref.py holds the conditions that make a GPU comparison on them
mean something (CPU only); tests/test_gpu_cgr_synthetic.py runs them.

Every matrix stays on the coded row-per-lane path -- the only one cgr_plan accepts: one rank, rows of at most 64
off-diagonal entries, no long row, off-diagonal values from a set of 1, 2 or 3, the diagonal of cg_ref._finish.  What
the library will make of a pattern is restated here from its code (restate_plan: the greedy tile cut of sell_cut_tile
and the lane order of sell_lane_order; expected_resident: the arithmetic of cgr_plan), so that a case can say on the
CPU which tile, window stretch, block and reduction group it is about -- and the GPU test can hold the library's own
plan to that before it compares anything.

Families (system(family, key) builds one, once per process; nobody writes to what it returns):
  "inst"   one matrix per (NQ, ND) instance: longest row exactly 32 / 52 / 64 entries (NQ = 8 / 13 / 16) with two and
           with three values, and one with a single value (runs as ND = 2, second value 0); 64-, 128-, 256-row tiles.
  "win"    256-row tiles; tile 2 (rows 512 ... 767, built with test_gpu_sell_packed._tile_rows / _pool and mirrored)
           has exactly 0, 256, 257, 512, 513 or 767 columns outside itself: nwq = 0, 1, 2, 2, 3, 3 stretches of the
           kernel's window.  "w0" ends in a tile of ONE row, "w256" in a tile of 100 rows (two waves without a row).
  "sib"    five 256-row tiles in which named rows reference the first row of their block, its last row and the first
           row of the next block, for two and for four tiles per block.
  "blocks" a banded matrix of n_tiles 64-row tiles (KMCF_SPMV_SELL_ROWS=64): the block counts of the flat and of
           the two-hop reduction."""
import numpy as np

import cg_ref as R

LD = np.longdouble
ECAP = 1024 - 256 - 1              # columns outside a tile's own rows (sell_plan_params: slot 1023 is the padding's target)
SELL_NQ = (8, 13, 16)              # KMCF_SELL_NQ: steps of 4 entries a lane holds in registers
COUNT_ROWS_MAX = 1500              # count checks need an eigen-solve (cg_ref.count_rhs): small systems only


# ---------------------------------------------------------------------------------------------------------------------
# the library's plan, restated

def restate_plan(M, row_cap, ecap=ECAP):
    """(tiles, perm) the library makes of the CSR matrix M with KMCF_SPMV_SELL_ROWS = row_cap, from its code:
    kmcf_sell_refine_order cuts tiles greedily in the caller's row order (sell_cut_tile: rows are added while the tile
    holds at most row_cap rows and references at most ecap columns that are not -- yet -- rows of it) and puts each
    tile's rows into lane order (sell_lane_order: stable sort by off-diagonal count, longest first, then every group of
    64 by index).  perm[i] = caller's row of internal row i; tiles = [(first internal row, rows, window)] with window =
    the tile's outside columns as INTERNAL ids in ascending order: window slot 256 + q, stretch q // 256, lane q % 256."""
    n = M.shape[0]
    ip, ix = M.indptr, M.indices
    cols = [ix[ip[i]:ip[i + 1]][ix[ip[i]:ip[i + 1]] != i] for i in range(n)]
    perm = np.arange(n)
    cuts, start = [], 0
    while start < n:
        e, ext, ref, rows = start, 0, set(), set()
        while e < n and e - start < row_cap:
            nxt = ext - (1 if e in ref else 0)
            new = [int(c) for c in cols[e] if c not in ref]
            nxt += sum(1 for c in new if c not in rows)
            if nxt > ecap:
                break
            ref.update(new)
            rows.add(e)
            ext = nxt
            e += 1
        assert e > start
        ln = np.array([len(cols[i]) for i in range(start, e)])
        order = np.argsort(-ln, kind="stable")
        order = np.concatenate([np.sort(order[t:t + 64]) for t in range(0, len(order), 64)])
        perm[start:e] = start + order
        cuts.append((start, e - start, sorted(ref - rows)))
        start = e
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return [(r0, nr, np.sort(inv[out]) if len(out) else np.zeros(0, np.int64)) for r0, nr, out in cuts], perm


def expected_resident(n_tiles, tpb=None, g1=None):
    """(resident_tpb, resident_g1, blocks, groups) of cgr_plan for a matrix of n_tiles <= 1024 tiles whose blocks all
    fit the device: KMCF_CGR_TPB = tpb (None: the smallest of 1 / 2 / 4 that keeps the grid within 256 blocks),
    KMCF_CGR_G1 = g1 (None: 0 = flat up to 256 blocks, else 16); groups of at least 2 and at most 64 blocks, doubled
    until at most 64 groups are left."""
    if tpb is None:
        tpb = next(t for t in (1, 2, 4) if (n_tiles + t - 1) // t <= 256)
    nb = (n_tiles + tpb - 1) // tpb
    if g1 is None:
        g1 = 0 if nb <= 256 else 16
    if g1 != 0 or nb > 256:
        g1 = max(2, min(64, g1))
        while (nb + g1 - 1) // g1 > 64:
            g1 *= 2
        assert g1 <= 64
    return tpb, g1, nb, ((nb + g1 - 1) // g1 if g1 else 1)


# ---------------------------------------------------------------------------------------------------------------------
# builders

def _sym(n, pairs):
    import scipy.sparse as sp
    pairs = np.array(sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b}))
    P = sp.csr_matrix((np.ones(len(pairs)), (pairs[:, 0], pairs[:, 1])), shape=(n, n))
    return ((P + P.T) > 0).astype(float).tocsr()


def _pairs(P):
    C = P.tocoo()
    return {(int(a), int(b)) for a, b in zip(C.row, C.col) if a < b}


def instance(L, nvals, n, seed):
    """n rows of 1 to 10 drawn entries within +-60 (more after mirroring), and ONE row (n // 3) filled up to exactly L
    off-diagonal entries: the longest, so that kmcf_sell_instance takes NQ = 8 / 13 / 16 for L = 32 / 52 / 64."""
    pairs = _pairs(R._pattern(n, 10, 60, None, seed))
    i0 = n // 3
    have = {b if a == i0 else a for a, b in pairs if i0 in (a, b)}
    rng = np.random.default_rng(seed + 500)
    cand = [c for c in range(i0 - 60, i0 + 61) if c != i0 and c not in have]
    for c in rng.choice(cand, size=L - len(have), replace=False):
        pairs.add((min(i0, int(c)), max(i0, int(c))))
    P = _sym(n, pairs)
    M = R._finish(P, np.random.default_rng(seed + 1000), R.VALUES3[:nvals])
    last = int(M.indices[M.indptr[i0]:M.indptr[i0 + 1]].max())
    return M, dict(long_row=i0, edges=[(i0, last)] if L == 64 else [])


WIN_TILE = 2                       # the tile the window cases are about


def window(nout, tail, seed):
    """Five 256-row tiles (+ a tail of `tail` rows); tile 2 references exactly `nout` columns outside itself.  Its rows
    come from test_gpu_sell_packed._tile_rows with a pool of _pool (nout = 767: backward=True, every row at least two
    pool columns and every pool column once, so that the running count of the greedy cut -- pool columns so far +
    later rows of the tile already referenced -- stays within the cap); nobody else references the tile, so mirroring
    leaves its outside columns what the pool is.  The other rows: 1 to 5 drawn entries within +-30."""
    from test_gpu_sell_packed import _pool, _tile_rows
    n, r0, nr = 5 * 256 + tail, 256 * WIN_TILE, 256
    rng = np.random.default_rng(seed)
    pairs = {(a, b) for a, b in _pairs(R._pattern(n, 5, 30, None, seed + 1)) if not (r0 <= a < r0 + nr or r0 <= b < r0 + nr)}
    pool = _pool(rng, n, r0, nr, nout) if nout else []
    if nout == ECAP:
        ln = [6] * nr
        for i in range(10, 17):
            ln[i] = 4              # pool columns per row: 6, 5, 4, then 3 (2 in these seven): 767 in all
    else:
        ln = [[6, 7, 8, 9][k] for k in rng.integers(4, size=nr)]
    tr = _tile_rows(rng, r0, ln, pool, 3, backward=nout == ECAP)
    for i, row in enumerate(tr):
        pairs |= {(min(r0 + i, c), max(r0 + i, c)) for c, _ in row[:-1]}
    M = R._finish(_sym(n, pairs), np.random.default_rng(seed + 1000), R.VALUES3)
    return M, dict(pool=np.asarray(pool, np.int64))


def window_edges(M, tiles, perm):
    """One entry of tile 2 per stretch of its window: (row, column) in the caller's numbering for the LAST column of
    every stretch (ranks 255, 511, ... and the window's last)."""
    r0, nr, win = tiles[WIN_TILE]
    out = []
    for q in range((len(win) + 255) // 256):
        c = int(perm[win[min(256 * q + 255, len(win) - 1)]])
        i = next(int(perm[t]) for t in range(r0, r0 + nr) if c in M.indices[M.indptr[perm[t]]:M.indptr[perm[t] + 1]])
        out.append((i, c))
    return out


SIB_TILES = 5
# (row, column, tiles per block, what the column is to the row's block)
SIB_EDGES = [(868, 512, 2, "first"), (612, 1023, 2, "last"), (869, 1024, 2, "next"),
             (356, 0, 2, "first"), (101, 511, 2, "last"), (358, 512, 2, "next"),
             (613, 0, 4, "first"), (100, 1023, 4, "last"), (869, 1024, 4, "next")]


def siblings():
    """Five 256-row tiles whose rows are already in lane order (perm = identity): wave w of every tile is a ring in which
    each row references its 8 / 6 / 4 / 2 nearest on either side (16 / 12 / 8 / 4 entries), row t of a tile references
    row t of the tiles before and after (1 or 2 more), and the entries of SIB_EDGES add at most 2 to a row -- the waves'
    lengths stay 4 apart."""
    n = 256 * SIB_TILES
    pairs = set()
    for T in range(SIB_TILES):
        for w, k in enumerate((8, 6, 4, 2)):
            g0 = 256 * T + 64 * w
            pairs |= {(g0 + j, g0 + (j + d) % 64) for j in range(64) for d in range(1, k + 1)}
        if T + 1 < SIB_TILES:
            pairs |= {(256 * T + t, 256 * T + 256 + t) for t in range(256)}
    base = {(min(a, b), max(a, b)) for a, b in pairs}
    for i, c, _, _ in SIB_EDGES:
        assert (min(i, c), max(i, c)) not in base
        pairs.add((i, c))
    M = R._finish(_sym(n, pairs), np.random.default_rng(4100), R.VALUES3)
    return M, dict(edges=sorted({(i, c) for i, c, _, _ in SIB_EDGES}))


def banded(n_tiles, seed=61):
    """64 n_tiles rows of 1 to 4 drawn entries within +-6: with 64-row tiles every tile is cut by its row count."""
    M = R._finish(R._pattern(64 * n_tiles, 4, 6, None, seed), np.random.default_rng(seed + 1000), R.VALUES3)
    return M, {}


# key -> (L, values, rows, tile rows, seed)
INSTANCES = {"nq8-nd2": (32, 2, 700, 64, 11), "nq8-nd3": (32, 3, 900, 128, 12), "nq13-nd2": (52, 2, 1500, 256, 13),
             "nq13-nd3": (52, 3, 500, 64, 14), "nq16-nd2": (64, 2, 1100, 128, 15), "nq16-nd3": (64, 3, 1300, 256, 16),
             "nq8-one-value": (32, 1, 1000, 256, 17)}
# key -> (outside columns of tile 2, rows of the tail tile)
WINDOWS = {"w0": (0, 1), "w256": (256, 100), "w257": (257, 0), "w512": (512, 0), "w513": (513, 0), "w767": (767, 0)}
BLOCK_TILES = (1, 3, 5, 64, 65, 128, 129, 256, 257)
# (tiles, KMCF_CGR_TPB): one tile per block at every count; partly filled last blocks; fewer tiles than a block holds
BLOCK_CASES = [(t, 1) for t in BLOCK_TILES] + [(5, 4), (257, 4), (3, 2), (65, 2), (1, 4), (3, 4)]
# (tiles, KMCF_CGR_G1, resident_g1, groups) at one tile per block
G1_CASES = [(256, 4, 4, 64), (257, 4, 8, 33), (257, 2, 8, 33), (257, 64, 64, 5), (65, 64, 64, 2)]

_cache = {}


def system(family, key, jacobi=True):
    """The case as cg_ref.system returns one (M, x0 = 0, b, p0, dinv, ref, f64, a0bar, L; cb, cref, tol, stop, margin
    where the system has at most COUNT_ROWS_MAX rows), and: rows (KMCF_SPMV_SELL_ROWS), tiles / perm (restate_plan),
    edges ((row, column) entries the case is about), extra (the builder's notes)."""
    ck = (family, key, bool(jacobi))
    if ck in _cache:
        return _cache[ck]
    if family == "inst":
        L, nvals, n, rows, seed = INSTANCES[key]
        M, extra = instance(L, nvals, n, seed)
    elif family == "win":
        M, extra = window(WINDOWS[key][0], WINDOWS[key][1], 300 + WINDOWS[key][0])
        rows = 256
    elif family == "sib":
        M, extra = siblings()
        rows = 256
    else:
        M, extra = banded(int(key))
        rows = 64
    tiles, perm = restate_plan(M, rows)
    if family == "win":
        extra["edges"] = window_edges(M, tiles, perm)
    s = make_system(M, jacobi, count=M.shape[0] <= COUNT_ROWS_MAX)
    s.update(name="%s/%s" % (family, key), rows=rows, tiles=tiles, perm=perm, edges=extra.get("edges", []), extra=extra)
    _cache[ck] = s
    return s


def make_system(M, jacobi=True, x0=None, count=True, b=None):
    """cg_ref.system's dict for the matrix M (x0: a start vector instead of 0; then p0 is the reference's own first
    direction and a0bar is not defined)."""
    n = M.shape[0]
    z, bb = R.first_step_inputs(M, jacobi)
    b = bb if b is None else b
    p0, dinv = R.first_direction(M, b, jacobi)
    start = z if x0 is None else x0
    s = dict(M=M, jacobi=bool(jacobi), x0=start, b=b, p0=p0, dinv=dinv, L=int(np.diff(M.indptr).max()),
             ref=R.pcg_reference(M, b, start, dinv, 25, LD), f64=R.pcg_reference(M, b, start, dinv, max(R.K_STEPS), np.float64))
    s["a0bar"] = R.alpha0_bar(M, p0) if x0 is None else None
    if count:
        s["cb"] = R.count_rhs(M, jacobi)
        s["cref"] = R.pcg_reference(M, s["cb"], z, dinv, 12, LD)
        s["tol"], s["stop"], s["margin"] = R.count_tolerance(s["cref"])
    for v in (s["x0"], s["b"], s["p0"]) + ((s["cb"],) if count else ()) + (() if dinv is None else (dinv,)):
        v.setflags(write=False)
    return s


START_STOP = ("inst", "nq16-nd3")  # the system of test_start_and_stop: 1300 rows, 256-row tiles
SOLVED_TOL = 1e-10                 # tolerance of the solve that starts from the solution


def start_vector(s):
    """A start vector of the size of the solution, nowhere zero to rounding."""
    return np.random.default_rng(77).standard_normal(s["M"].shape[0])


def solution(s):
    """The long-double solution of the system, rounded to double (PCG run until its residual is below 1e-18)."""
    if "solution" not in s:
        ref = R.pcg_reference(s["M"], s["b"], np.zeros(s["M"].shape[0]), s["dinv"], 80 if s["jacobi"] else 700, LD)
        assert ref["res"][-1] <= 1e-18, ref["res"][-1]
        s["solution"] = np.asarray(ref["x"][-1], np.float64)
        s["solution"].setflags(write=False)
    return s["solution"]


ORDERS = 8                         # permuted row orders of order_spread


def order_spread(s, k):
    """How far float64 runs that merely ADD IN ANOTHER ORDER lie from the long-double reference after k iterations:
    numpy's run of the system with rows and columns permuted (ORDERS seeded permutations; row sums and dot products
    then add their terms in another order), the largest distance per quantity, measured as cg_ref.step_distance does."""
    key = ("spread", k)
    if key not in s:
        M, n = s["M"], s["M"].shape[0]
        worst = dict(x=0.0, r=0.0, rz=0.0)
        for seed in range(ORDERS):
            p = np.random.default_rng(1000 + seed).permutation(n)
            inv = np.argsort(p)
            Mp = M[p][:, p].tocsr()
            Mp.sort_indices()
            f = R.pcg_reference(Mp, s["b"][p], s["x0"][p], None if s["dinv"] is None else s["dinv"][p], k, np.float64)
            d = R.step_distance(s, k, f["x"][k - 1][inv], f["r"][k - 1][inv], f["rz"][k])
            worst = {q: max(worst[q], d[q]) for q in worst}
        s[key] = worst
    return s[key]


def rz_bar_from_r(s, k, r_bar):
    """A bound of r.z that follows from the bar r itself is held to: every entry of r within r_bar x max|r| of the
    reference's, and a dot product of n terms of one sign: |d rz| <= sum w_i (2 |r_i| d + d^2) + (n + 2) u rz, w = dinv
    or 1 (the form of cg_ref.first_step_bars, for a start vector that bound is not derived for)."""
    r, rz = s["ref"]["r"][k - 1], s["ref"]["rz"][k]
    n = len(r)
    w = np.ones(n, LD) if s["dinv"] is None else s["dinv"].astype(LD)
    d = LD(r_bar) * np.abs(r).max()
    return float(((w * (2 * np.abs(r) * d + d * d)).sum() + (n + 2) * R.U * rz) / rz)


def step_bars(s, k):
    """(bars, derived): cg_ref.step_bars -- 16 x the distance of numpy's float64 run from the reference -- with the one
    provision that docstring asks for: numpy's distance is ONE draw of a rounding error, and where it is a lucky one
    the bar says nothing.  Decided on the CPU, from the reference alone: if a float64 numpy run of the SAME system in
    a permuted row order (order_spread) lies beyond the bar of r.z, r.z takes its derived first-step bound
    (cg_ref.first_step_bars; from a start vector x0 != 0, which that bound is not derived for, rz_bar_from_r -- there
    also after ONE iteration).  derived: the quantities whose bar is a derived one."""
    ref, f64 = s["ref"], s["f64"]
    bars = dict(x=16.0 * R.rel_max(f64["x"][k - 1], ref["x"][k - 1]), r=16.0 * R.rel_max(f64["r"][k - 1], ref["r"][k - 1]),
                rz=16.0 * R.rel(f64["rz"][k], ref["rz"][k]))
    zero_start = s["a0bar"] is not None
    derived = []
    if k == 1 or order_spread(s, k)["rz"] > bars["rz"]:
        bars["rz"] = R.first_step_bars(s)["rz"] if zero_start else rz_bar_from_r(s, k, bars["r"])
        derived.append("rz")
    if zero_start:
        mine = R.step_bars(s, k)
        assert all(bars[q] == mine[q] for q in bars if q not in derived or k == 1)
    return bars, derived


def count_from(s, x0):
    """The count check started from x0: b = A x0 + cg_ref.count_rhs, so that the first residual is that right-hand
    side to rounding; dict(b, ref, tol, stop, margin) from the reference's own run of it."""
    b = s["cb"] + s["M"] @ x0
    ref = R.pcg_reference(s["M"], b, x0, s["dinv"], 12, LD)
    tol, stop, margin = R.count_tolerance(ref)
    return dict(b=b, ref=ref, tol=tol, stop=stop, margin=margin)


def lost_entry_ratio(s, i, c):
    """The reference WITHOUT the entry (i, c), one iteration: distance of its r from the true reference's r (relative
    max-norm, as check (b) measures it) over the bar check (b) holds r to after one iteration."""
    M = s["M"].copy()
    lo, hi = M.indptr[i], M.indptr[i + 1]
    j = lo + int(np.searchsorted(M.indices[lo:hi], c))
    assert M.indices[j] == c and c != i
    M.data[j] = 0.0
    bad = R.pcg_reference(M, s["b"], s["x0"], s["dinv"], 1, LD)
    return float(R.rel_max(bad["r"][0], s["ref"]["r"][0]) / R.step_bars(s, 1)["r"])


def lost_row_ratio(s):
    """The smallest change of alpha0 that losing ONE row's term of p0.Ap0 makes, over alpha0's bar."""
    t, _ = R.first_step_terms(s["M"], s["p0"])
    return float((t / (t.sum() - t)).min() / s["a0bar"])
