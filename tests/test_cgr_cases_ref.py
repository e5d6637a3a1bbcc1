"""CPU: the conditions the systems of tests/cgr_cases.py must meet for tests/test_gpu_cgr_synthetic.py to mean something,
asserted on the long-double reference and on the restated plan alone.

  - every matrix is what cgr_plan accepts (symmetric, dominant diagonal, rows <= 64 entries, 1 / 2 / 3 values) and
    has the longest row its (NQ, ND) instance needs;
  - the tiles, windows, blocks and reduction groups a case is about follow from its pattern (cgr_cases.restate_plan,
    cgr_cases.expected_resident: the library's greedy cut, lane order and cgr_plan's arithmetic, restated);
  - ONE lost entry at an edge (a sibling column, a column of each window stretch, the 64th entry of a row) moves r
    after one iteration by more than 100 x the bar the GPU test holds r to; ONE lost row of p0.Ap0 moves alpha0 by more
    than 4 x its bar; the count checks' tolerances lie a factor >= 2 from the reference's residuals.
Every figure is printed (pytest -s)."""
import numpy as np
import pytest

import cg_ref as R
import cgr_cases as G

LD = np.longdouble
ALL = [("inst", k) for k in G.INSTANCES] + [("win", k) for k in G.WINDOWS] + [("sib", "sib")] + [("blocks", "5")]


def _offdiag(M):
    return M.data[M.indices != np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))]


@pytest.mark.parametrize("family,key", ALL + [("blocks", str(t)) for t in (65, 257)], ids=lambda v: str(v))
def test_matrices_qualify(family, key):
    s = G.system(family, key)
    M = s["M"]
    assert abs(M - M.T).max() == 0
    d = M.diagonal()
    off = np.abs(M).sum(1).A1 - d
    assert np.all(d >= 1.5 * off + 1.0) and np.all(d < 1.5 * off + 2.0)          # (cg_ref._finish's diagonal)
    lens = np.diff(M.indptr) - 1
    vals = np.unique(_offdiag(M))
    want = G.INSTANCES[key][1] if family == "inst" else 3
    print("cgr-cases %s: %d rows, longest %d, shortest %d, %d values" % (s["name"], M.shape[0], lens.max(), lens.min(), len(vals)))
    assert lens.max() <= 64 and lens.min() >= 0          # (a row of its diagonal alone is a row like any other)
    assert len(vals) == want and set(vals) <= set(R.VALUES3)
    if family == "inst":
        L, _, n, rows, _ = G.INSTANCES[key]
        assert M.shape[0] == n and 300 <= n <= 1500
        assert lens.max() == L and lens[s["extra"]["long_row"]] == L
        assert next(q for q in G.SELL_NQ if 4 * q >= lens.max()) == {32: 8, 52: 13, 64: 16}[L]
        assert len(np.unique(lens)) > 8                                            # (waves of different step counts)


def test_instances_cover_the_table():
    got = {(next(q for q in G.SELL_NQ if 4 * q >= L), 2 if nv <= 2 else 3) for L, nv, _, _, _ in G.INSTANCES.values()}
    assert got == {(q, d) for q in G.SELL_NQ for d in (2, 3)}
    assert sorted(nv for _, nv, _, _, _ in G.INSTANCES.values()).count(1) == 1
    assert {r for _, _, _, r, _ in G.INSTANCES.values()} == {64, 128, 256}


@pytest.mark.parametrize("key", list(G.INSTANCES))
def test_instance_tiles(key):
    """Reach 60: no tile comes near the cap of outside columns, every tile is cut by its row count; the lane order is
    a real permutation wherever a tile has more than one wave (rows of mixed lengths)."""
    s = G.system("inst", key)
    n, rows = s["M"].shape[0], s["rows"]
    sizes = [nr for _, nr, _ in s["tiles"]]
    print("cgr-cases %s: intended %d tiles of %d rows, restated %d, windows <= %d columns" %
          (s["name"], -(-n // rows), rows, len(sizes), max(len(w) for _, _, w in s["tiles"])))
    assert sizes == [rows] * (n // rows) + ([n % rows] if n % rows else [])
    assert max(len(w) for _, _, w in s["tiles"]) < G.ECAP
    assert (rows == 64) == np.array_equal(s["perm"], np.arange(n))     # (a 64-row tile is ONE wave, kept in index order)
    assert np.array_equal(np.sort(s["perm"]), np.arange(n))


@pytest.mark.parametrize("key", list(G.WINDOWS))
def test_window_counts(key):
    """Tile 2 has exactly the intended number of outside columns (its pool), every tile is cut at 256 rows (the tail
    apart), and the edge entries name one column per stretch: the last of each."""
    s = G.system("win", key)
    nout, tail = G.WINDOWS[key]
    sizes = [nr for _, nr, _ in s["tiles"]]
    r0, nr, win = s["tiles"][G.WIN_TILE]
    print("cgr-cases %s: intended %d outside columns, restated %d; tiles %s; stretches %d; edge entries %s"
          % (s["name"], nout, len(win), sizes, (len(win) + 255) // 256, s["edges"]))
    assert sizes == [256] * 5 + ([tail] if tail else [])
    assert (r0, nr) == (512, 256) and len(win) == nout
    assert np.array_equal(np.sort(s["perm"][win]), s["extra"]["pool"])
    assert len(s["edges"]) == {0: 0, 256: 1, 257: 2, 512: 2, 513: 3, 767: 3}[nout]
    inv = np.argsort(s["perm"])
    for q, (i, c) in enumerate(s["edges"]):
        assert 512 <= i < 768 and s["M"][i, c] != 0
        rank = int(np.searchsorted(win, inv[c]))
        assert win[rank] == inv[c] and rank // 256 == q and rank == min(256 * q + 255, nout - 1)
    assert all(len(w) <= G.ECAP for _, _, w in s["tiles"])


def test_window_tail_tiles():
    """A tile of a single row; a tile of 100 rows: waves 2 and 3 hold nothing."""
    assert G.system("win", "w0")["tiles"][-1][1] == 1
    assert G.system("win", "w256")["tiles"][-1][1] == 100


def test_sibling_columns():
    """perm is the identity, five tiles of 256 rows; every entry of SIB_EDGES references, from ANOTHER tile, the first
    row of the row's block, the last row of the block, or the first row of the next block."""
    s = G.system("sib", "sib")
    n = s["M"].shape[0]
    assert [nr for _, nr, _ in s["tiles"]] == [256] * G.SIB_TILES and np.array_equal(s["perm"], np.arange(n))
    for i, c, tpb, what in G.SIB_EDGES:
        assert s["M"][i, c] != 0 and i // 256 != c // 256
        rb0 = i // (256 * tpb) * 256 * tpb
        rb1 = min(rb0 + 256 * tpb, n)
        assert c == {"first": rb0, "last": rb1 - 1, "next": rb1}[what] and rb1 < n
        # (first / last: a sibling tile's row, read from LDS; next: outside the block, through the granules)
        assert (rb0 <= c < rb1) == (what != "next")
        print("cgr-cases sib: tpb %d row %d -> column %d = %s row of block [%d, %d)" % (tpb, i, c, what, rb0, rb1))
    assert {(t, w) for _, _, t, w in G.SIB_EDGES} == {(t, w) for t in (2, 4) for w in ("first", "last", "next")}


@pytest.mark.parametrize("nt", G.BLOCK_TILES)
def test_block_tiles(nt):
    s = G.system("blocks", str(nt))
    sizes = [nr for _, nr, _ in s["tiles"]]
    print("cgr-cases blocks/%d: intended %d tiles of 64 rows, restated %d (%d rows)" % (nt, nt, len(sizes), s["M"].shape[0]))
    assert sizes == [64] * nt and s["M"].shape[0] == 64 * nt <= 16448


def test_block_and_group_tables():
    """What cgr_plan makes of the block and G1 tables (expected_resident restates it): the lane and wave edges of the flat
    reduction, the two-hop default at 257 blocks, partly filled last blocks, fewer tiles than a block holds, exactly
    64 groups (no doubling), 65 (doubled), a partial last group, groups of 64."""
    flat = sorted(G.expected_resident(t, b)[2] for t, b in G.BLOCK_CASES if G.expected_resident(t, b)[1] == 0)
    assert {1, 64, 65, 128, 129, 256} <= set(flat)
    assert G.expected_resident(257, 1) == (1, 16, 257, 17) and 257 % 16 != 0
    for t, b in [(5, 4), (257, 4), (3, 2), (65, 2)]:
        assert t % b == 1                                   # ONE active tile in the last block
    assert G.expected_resident(1, 4)[2] == 1 and G.expected_resident(3, 4)[2] == 1
    for t, knob, g1, groups in G.G1_CASES:
        got = G.expected_resident(t, 1, knob)
        print("cgr-cases g1: %d tiles, KMCF_CGR_G1=%d -> g1 %d, %d groups (last of %d blocks)" % (t, knob, got[1], got[3], t - (got[3] - 1) * got[1]))
        assert got == (1, g1, t, groups)
    assert (256 + 3) // 4 == 64 and (257 + 3) // 4 == 65 and 257 - 4 * 64 == 1
    for t in (1, 286, 881, 1024):
        assert G.expected_resident(t)[0] == (1 if t <= 256 else 2 if t <= 512 else 4) and G.expected_resident(t)[1] == 0


@pytest.mark.parametrize("family,key", ALL, ids=lambda v: str(v))
def test_sensitivity(family, key):
    """One lost edge entry against the bar of r after one iteration (>= 100); one lost row of p0.Ap0 against alpha0's
    bar (>= 4); the reference's r is the true residual."""
    for jacobi in ((True, False) if (family, key) == G.START_STOP else (True,)):
        s = G.system(family, key, jacobi)
        row = G.lost_row_ratio(s)
        ratios = [G.lost_entry_ratio(s, i, c) for i, c in s["edges"]]
        print("cgr-cases %s%s: lost row / alpha0 bar %.3g; lost edge entry / r bar %s"
              % (s["name"], "" if jacobi else "/plain", row, " ".join("%.3g" % v for v in ratios) or "-"))
        assert row >= 4.0
        assert all(v >= 100.0 for v in ratios), ratios
        true_r = s["b"].astype(LD) - R._matvec(s["M"], LD)(s["ref"]["x"][4])
        assert np.abs(true_r - s["ref"]["r"][4]).max() <= 1e-16 * np.abs(s["b"]).max()
    if family == "inst":
        assert (len(s["edges"]) == 1) == (G.INSTANCES[key][0] == 64)


@pytest.mark.parametrize("family,key", ALL, ids=lambda v: str(v))
def test_count_margins(family, key):
    """The tolerance of every count check lies a factor >= 2 from the reference's residuals on both sides."""
    for jacobi in ((True, False) if (family, key) == G.START_STOP else (True,)):
        s = G.system(family, key, jacobi)
        assert s["M"].shape[0] <= G.COUNT_ROWS_MAX
        j, below, above = R.count_conditions(s["cref"], s["tol"])
        print("cgr-cases %s%s: count %d, tolerance %.3g, margin %.3g (below %.3g, above %.3g)"
              % (s["name"], "" if jacobi else "/plain", s["stop"], s["tol"], s["margin"], below, above))
        assert j == s["stop"] and j >= 3 and s["margin"] >= 2.0 and below >= 2.0 and above >= 2.0


def test_start_vectors():
    """test_start_and_stop's inputs: a random start vector leaves a first residual of the size of b; the long-double
    solution rounded to double leaves one below the tolerance of that test by many orders."""
    for jacobi in (True, False):
        s = G.system(*G.START_STOP, jacobi)
        x0 = G.start_vector(s)
        sx = G.make_system(s["M"], jacobi, x0=x0, count=False)
        assert 0.1 <= sx["ref"]["res"][0] <= 30.0
        xs = G.solution(s)
        ss = G.make_system(s["M"], jacobi, x0=xs, count=False)
        print("cgr-cases start/%s: res[0] from random x0 %.3g, from the rounded solution %.3g" % ("jacobi" if jacobi else "plain", sx["ref"]["res"][0], ss["ref"]["res"][0]))
        assert ss["ref"]["res"][0] <= 1e-15 and G.SOLVED_TOL >= 1e5 * ss["ref"]["res"][0]
        cs = G.count_from(s, x0)
        j, below, above = R.count_conditions(cs["ref"], cs["tol"])
        print("cgr-cases start/%s: count from x0 %d, tolerance %.3g, margin %.3g" % ("jacobi" if jacobi else "plain", cs["stop"], cs["tol"], cs["margin"]))
        assert j == cs["stop"] and j >= 3 and cs["margin"] >= 2.0 and below >= 2.0 and above >= 2.0


@pytest.mark.parametrize("family,key", ALL + [("blocks", "257")], ids=lambda v: str(v))
def test_step_bars(family, key):
    """cgr_cases.step_bars: r.z keeps 16 x numpy's distance unless a permuted-order float64 run of the same system lies
    beyond that (printed: how far such runs reach, in units of numpy's distance); x and r always keep it.  With the
    bars as they then stand, a step length off by 1e-9 in iteration 1 or 5 still misses them after 5 iterations."""
    s = G.system(family, key)
    for k in R.K_STEPS:
        bars, derived = G.step_bars(s, k)
        plain = R.step_bars(s, k)
        spread = G.order_spread(s, k)
        print("cgr-cases %s: k=%d permuted float64 runs reach x %.1f r %.1f rz %.1f x numpy's distance (bar 16); derived: %s"
              % (s["name"], k, *(16.0 * spread[q] / plain[q] if k > 1 or q != "rz" else 0.0 for q in ("x", "r", "rz")), ",".join(derived) or "-"))
        assert bars["x"] == plain["x"] and bars["r"] == plain["r"]
        assert (bars["rz"] == plain["rz"]) if "rz" not in derived or k == 1 else (bars["rz"] == R.first_step_bars(s)["rz"] > plain["rz"])
        assert ("rz" in derived) == (k == 1 or spread["rz"] > plain["rz"])
    bars, _ = G.step_bars(s, 5)
    for j in (1, 5):
        bad = R.pcg_reference(s["M"], s["b"], s["x0"], s["dinv"], 5, LD, alpha_scale={j: 1.0 + 1e-9})
        dist = R.step_distance(s, 5, bad["x"][4], bad["r"][4], bad["rz"][5])
        assert any(dist[q] > bars[q] for q in ("x", "r", "rz")), (j, dist, bars)
