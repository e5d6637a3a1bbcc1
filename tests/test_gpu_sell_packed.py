"""GPU: the packed entry stream of the coded row-per-lane kernel (five 12-bit fields per 8-byte word, the default)
against the 16-bit stream (KMCF_SELL_PACK=0 + replan), bit for bit: the two stream the same entries in the same
order, so every y[row], every p.Ap partial and with them every CG iterate must be identical.

Matrices as in tests/test_gpu_spmv_edge.py (KMCF_SPMV_KIND=2, <= 3 distinct off-diagonal values), made of whole tiles:
with KMCF_SPMV_SELL_ROWS=256 the planner cuts a tile every 256 rows (each tile here stays within the cap of 767
columns outside its own rows), sorts its rows by length and deals them to four waves.  Window slot of a column: its
lane for one of the tile's own rows, else 256 + its rank among the tile's outside columns.  Slot 1023 is never a
column -- it is the padding's target, the cap keeps it free -- so the largest field of a real entry is
(2 << 10) | 1022; the field arithmetic up to 0xFFF is tests/test_sell_pack_cpu.py's.

Every product is compared twice: for a random x bit for bit between the two settings and to 1e-14 |A| |x| against
the plain sum; for an x of small dyadic numbers, where every product and sum is exact in any order, against
_dense_apply with the tolerance of test_tiny_matrices."""
import numpy as np
import pytest

from test_gpu_spmv_edge import _csr, _dense_apply

pytestmark = pytest.mark.gpu

VALS = np.array([-1.0, -0.125, -3.0])
TILE = 256
CAP = 1024 - TILE - 1            # outside columns of a tile


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _env(monkeypatch, resident="0"):
    for k in ("KMCF_SELL_PACK", "KMCF_SPMV_SELL_SORT", "KMCF_SELL_NT", "KMCF_LONG_ROW", "KMCF_CG_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(KMCF_SPMV_KIND="2", KMCF_SPMV_CODED="1", KMCF_SPMV_SELL="1", KMCF_SPMV_SELL_ROWS="256",
                     KMCF_CG_RESIDENT=resident).items():
        monkeypatch.setenv(k, v)


def _tile_rows(rng, r0, lengths, pool, nvals, backward=False):
    """Rows r0 ... of one tile: row i gets lengths[i] off-diagonal entries -- columns of the tile itself and, where a
    pool is given, of the pool (every pool column is used, so the tile's outside columns ARE the pool) -- in column
    order, then the diagonal.  backward: only earlier rows of the tile are referenced (the planner counts a later
    row's column as an outside one until that row joins the tile; a tile AT the cap must not go beyond it on the way)."""
    nr = len(lengths)
    own = np.arange(r0, r0 + nr)
    rows, used = [], 0
    for i, ln in enumerate(lengths):
        cand = own[:i] if backward else own[own != r0 + i]
        n_out = min(ln // 2, len(pool)) if len(pool) else 0
        if ln - n_out > len(cand):
            n_out = ln - len(cand)
        assert n_out <= len(pool)
        out = [pool[(used + q) % len(pool)] for q in range(n_out)]
        used += n_out
        cols = sorted(set(out)) + sorted(rng.choice(cand, size=ln - len(set(out)), replace=False))
        assert len(cols) == ln and len(set(cols)) == ln
        rows.append([(int(c), float(VALS[rng.integers(nvals)])) for c in sorted(cols)] + [(r0 + i, 1000.0 + i % 7)])
    assert used >= len(pool), "the tile does not reference its whole pool"
    return rows


def _pool(rng, n, r0, nr, size):
    outside = np.concatenate([np.arange(0, r0), np.arange(r0 + nr, n)])
    return np.sort(rng.choice(outside, size=size, replace=False))


def _matrix(name, nvals=3):
    """name -> (rows, expected tile sizes)."""
    rng = np.random.default_rng(29)
    some = [0, 1, 4, 5, 6, 9, 10, 11, 15, 16, 27, 33]
    if name == "lengths":
        # one tile, 193 rows: the 64 longest 64/60/53/52 entries (13 steps of 5; 16 of 4), the next 64 16/15/11/10
        # (4 steps), the next 64 9/6/5/4/1 (2 steps), and a wave of a single row, without entries; no outside column
        ln = [[64, 60, 53, 52][i % 4] for i in range(64)] + [[16, 15, 11, 10][i % 4] for i in range(64)] + \
             [[9, 6, 5, 4, 1][i % 5] for i in range(64)] + [0]
        ln = list(rng.permutation(ln))
        return _tile_rows(rng, 0, ln, [], nvals), [len(ln)]
    if name == "two":
        sizes = [TILE, 100]
    elif name == "three":
        sizes = [TILE, TILE, 230]
    elif name == "nine":
        sizes = [TILE] * 8 + [77]
    else:
        raise KeyError(name)
    n = sum(sizes)
    rows = []
    for t, nr in enumerate(sizes):
        r0 = TILE * t
        ln = [some[k] for k in rng.integers(len(some), size=nr)]
        ln[int(rng.integers(nr))] = 64
        full = name == "nine" and t == 4
        if name == "nine" and t == 0:
            pool = []                                       # a tile without outside columns
        elif full:
            pool = _pool(rng, n, r0, nr, CAP)               # the full window: slots 256 ... 1022 are columns
            ln = [max(v, 12) for v in ln]
        elif name == "three" and t == 1:
            pool = _pool(rng, n, r0, nr, 460)
            ln = [max(v, 9) for v in ln]
        else:
            ln = [max(v, 4) for v in ln[:nr // 2]] + ln[nr // 2:]
            pool = _pool(rng, n, r0, nr, min(60 + 40 * t, n - nr, sum(v // 2 for v in ln)))
        tr = _tile_rows(rng, r0, ln, pool, nvals, backward=full)
        if name == "three" and t == 1:
            # fields 0x555 and 0xAAA: slot 0x155 = 341 is outside column 85 of the tile, slot 0x2AA = 682 is column 426;
            # the value code of an entry is the rank of its value's first appearance, so one row per pair of values
            # holds (code 1, slot 341), (code 2, slot 682) alternating in its 2nd ... 7th entries, whatever the ranks
            a, b = int(pool[341 - TILE]), int(pool[682 - TILE])
            k = 0
            for va in VALS[:nvals]:
                for vb in VALS[:nvals]:
                    i = 10 + k
                    k += 1
                    keep = [e for e in tr[i][:-1] if e[0] not in (a, b, r0 + i + 1)]
                    tr[i] = [(r0 + i + 1, float(VALS[0]))] + [(a, float(va)), (b, float(vb))] * 3 + keep + [tr[i][-1]]
        outside = {c for r in tr for c, v in r if not r0 <= c < r0 + nr}
        assert outside == set(int(c) for c in pool), (name, t)
        rows += tr
    return rows, sizes


def _open(km, rows):
    S = km.solvers
    indptr, indices, data = _csr(rows)
    n = len(rows)
    comm = S.KMC_comm(n, n, n, n)
    comm.connect()
    return comm, S.Distributed_matrix(comm, n, [n], [0], indices, indptr, data), (indptr, indices, data)


def _apply(torch, mat, x):
    p = torch.as_tensor(x, device="cuda")
    Ap = torch.full((len(x),), 7.0, dtype=torch.float64, device="cuda")
    mat.spmv(p, Ap)
    return Ap.cpu().numpy()


def _vectors(n):
    rng = np.random.default_rng(3)
    return rng.standard_normal(n), rng.integers(-16, 17, size=n) / 16.0


def _check_products(torch, mat, csr, label):
    """The products of the current plan for both x; returns them for the comparison between the settings."""
    indptr, indices, data = csr
    n = len(indptr) - 1
    xr, xd = _vectors(n)
    yr, yd = _apply(torch, mat, xr), _apply(torch, mat, xd)
    import scipy.sparse as sp
    # (copies: scipy sorts the arrays it is given in place when it merges duplicates for abs())
    M = sp.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(n, n))
    err = np.abs(yr - M @ xr)
    bound = 1e-14 * (abs(M) @ np.abs(xr)) + 1e-300
    print("sell-packed %s: max error / bound %.3f" % (label, float((err / bound).max())))
    assert np.all(err <= bound), label
    np.testing.assert_allclose(yd, _dense_apply(indptr, indices, data, xd), rtol=1e-14, atol=1e-14, err_msg=label)
    return yr, yd


def _both_settings(torch, monkeypatch, mat, csr, label, tiles=None):
    """Products under the default (packed) and under KMCF_SELL_PACK=0 after a replan: bit for bit the same."""
    monkeypatch.delenv("KMCF_SELL_PACK", raising=False)
    ip = mat.replan()
    assert ip["spmv_kind"] == 2 and ip["spmv_coded"] == 2, ip
    if tiles is not None:
        assert list(mat.sum_plan(with_csr=False)["tile_rows"]) == list(tiles), label
    packed = _check_products(torch, mat, csr, label + "/packed")
    monkeypatch.setenv("KMCF_SELL_PACK", "0")
    i16 = mat.replan()
    assert i16["spmv_kind"] == 2 and i16["spmv_coded"] == 2 and i16["spmv_tiles"] == ip["spmv_tiles"], i16
    plain = _check_products(torch, mat, csr, label + "/16-bit")
    monkeypatch.delenv("KMCF_SELL_PACK", raising=False)
    for a, b in zip(packed, plain):
        np.testing.assert_array_equal(a, b, err_msg=label)
    print("sell-packed %s: streamed 2-byte units %d packed, %d as 16-bit entries" % (label, ip["spmv_stream_entries"], i16["spmv_stream_entries"]))
    return ip, i16


def test_row_lengths(km, torch, monkeypatch):
    """Rows of 0, 1, 4, 5, 6, 9, 10, 11, 15, 16, 52, 53, 60 and 64 entries in one tile whose four waves run 13, 4, 2 and 0
    steps (one wave: a single row); no outside column."""
    _env(monkeypatch)
    rows, sizes = _matrix("lengths")
    comm, mat, csr = _open(km, rows)
    try:
        ip, i16 = _both_settings(torch, monkeypatch, mat, csr, "lengths", sizes)
        assert ip["spmv_window_cols"] == 0
        assert ip["spmv_stream_entries"] == (13 + 4 + 2 + 0) * 64 * 4          # words x 4 two-byte units
        assert i16["spmv_stream_entries"] == (16 + 4 + 3 + 0) * 64 * 4
    finally:
        mat.close()
        comm.close()


def test_a_65th_entry_declines(km, torch, monkeypatch):
    """A row of 65 off-diagonal entries: no row-per-lane layout, packed or not -- the coded window kernel runs."""
    _env(monkeypatch)
    rng = np.random.default_rng(7)
    n = 300
    rows = _tile_rows(rng, 0, [65] + [5] * (n - 1), [], 2)
    comm, mat, csr = _open(km, rows)
    try:
        for pack in (None, "0"):
            if pack is None:
                monkeypatch.delenv("KMCF_SELL_PACK", raising=False)
            else:
                monkeypatch.setenv("KMCF_SELL_PACK", pack)
            info = mat.replan()
            assert info["spmv_kind"] == 2 and info["spmv_coded"] == 1, info
            _check_products(torch, mat, csr, "65 entries/pack=%s" % pack)
    finally:
        mat.close()
        comm.close()


@pytest.mark.parametrize("nvals", [1, 2, 3])
def test_dictionaries(km, torch, monkeypatch, nvals):
    """One, two and three distinct values (the ND = 2 and ND = 3 instances) on three tiles (a pair and the odd tail), with
    the rows whose 2nd ... 7th fields alternate 0x555 / 0xAAA."""
    _env(monkeypatch)
    rows, sizes = _matrix("three", nvals)
    comm, mat, csr = _open(km, rows)
    try:
        assert len(np.unique([v for r in rows for c, v in r[:-1]])) == nvals
        ip, i16 = _both_settings(torch, monkeypatch, mat, csr, "three tiles, %d values" % nvals, sizes)
        assert ip["spmv_stream_entries"] < i16["spmv_stream_entries"]
    finally:
        mat.close()
        comm.close()


@pytest.mark.parametrize("name", ["two", "nine"])
def test_tile_counts_and_windows(km, torch, monkeypatch, name):
    """Two tiles (one pair, no tail) and nine (more tiles than XCD groups, fewer than blocks a chip holds); of the nine,
    tile 0 has no outside column and tile 4 the cap of them: its window is full, slot 1022 a column."""
    _env(monkeypatch)
    rows, sizes = _matrix(name)
    comm, mat, csr = _open(km, rows)
    try:
        ip, _ = _both_settings(torch, monkeypatch, mat, csr, name, sizes)
        if name == "nine":
            first = TILE * 4
            outside = {c for r in rows[first:first + TILE] for c, v in r if not first <= c < first + TILE}
            assert len(outside) == CAP
            assert not [c for r in rows[:TILE] for c, v in r if c >= TILE]
    finally:
        mat.close()
        comm.close()


def test_refresh_after_set_values(km, torch, monkeypatch):
    """set_values with two values swapped on half of the entries: the packed stream's codes are rewritten in place (its
    slots stay), the product again matches the 16-bit path bit for bit, get_values returns what was set."""
    _env(monkeypatch)
    rows, sizes = _matrix("three")
    comm, mat, csr = _open(km, rows)
    try:
        indptr, indices, data = csr
        _check_products(torch, mat, csr, "before set_values")            # the packed stream holds the first codes
        rng = np.random.default_rng(11)
        new = data.copy()
        half = rng.random(len(data)) < 0.5
        a, b = half & (data == VALS[0]), half & (data == VALS[1])
        new[a], new[b] = VALS[1], VALS[0]
        assert a.sum() > 500 and b.sum() > 500
        mat.set_values(new)
        assert mat.info()["spmv_coded"] == 2
        csr2 = (indptr, indices, new)
        first = _check_products(torch, mat, csr2, "after set_values")    # refreshed, not replanned
        np.testing.assert_array_equal(mat.get_values(), new)
        _both_settings(torch, monkeypatch, mat, csr2, "after set_values + replan", sizes)
        again = _check_products(torch, mat, csr2, "after set_values, packed")
        for p, q in zip(first, again):
            np.testing.assert_array_equal(p, q)
        np.testing.assert_array_equal(mat.get_values(), new)
    finally:
        mat.close()
        comm.close()


@pytest.mark.parametrize("resident", ["0", "1"])
def test_recurrence(km, torch, monkeypatch, resident):
    """Three fixed PCG iterations on the 3-tile matrix: x, r and r.z identical between the two settings -- the p.Ap
    partials' check.  resident=1: the register-resident launch, which reads the 16-bit stream under either setting
    (its codes are refreshed for it even where the packed stream serves the SpMV calls before)."""
    _env(monkeypatch, resident)
    rows, sizes = _matrix("three")
    comm, mat, csr = _open(km, rows)
    try:
        indptr, indices, data = csr
        n = len(rows)
        b = np.random.default_rng(13).standard_normal(n)
        dinv = 1.0 / np.array([r[-1][1] for r in rows])
        out = {}
        for pack in (None, "0"):
            if pack is None:
                monkeypatch.delenv("KMCF_SELL_PACK", raising=False)
            else:
                monkeypatch.setenv("KMCF_SELL_PACK", pack)
            info = mat.replan()
            assert info["spmv_coded"] == 2, info
            tpb = mat.sum_plan(with_csr=False)["resident_tpb"]                 # the path the solve below takes, not assumed
            print("sell-packed recurrence resident=%s pack=%s: resident_tpb %d" % (resident, pack, tpb))
            assert tpb > 0 if resident == "1" else tpb == 0, tpb
            _apply(torch, mat, b)                                      # an SpMV call first: the loop's stream is in use
            r = torch.as_tensor(b.copy(), device="cuda")
            x = torch.zeros_like(r)
            st = km.solvers.conjugate_gradient_jacobi(mat, r, x, torch.as_tensor(dinv, device="cuda"), 1e-30, 0, fixed_iters=3)
            assert st["iterations"] == 3, st
            out[pack] = (x.cpu().numpy(), r.cpu().numpy(), st["rz"], st["bb"])
        print("sell-packed recurrence resident=%s: rz %.17g / %.17g" % (resident, out[None][2], out["0"][2]))
        np.testing.assert_array_equal(out[None][0], out["0"][0])
        np.testing.assert_array_equal(out[None][1], out["0"][1])
        assert out[None][2] == out["0"][2] and out[None][3] == out["0"][3]
        assert np.all(np.isfinite(out[None][0])) and np.abs(out[None][0]).max() > 0
        # ... and three iterations did what three iterations do: the residual of the plain recurrence in float64
        import scipy.sparse as sp
        M = sp.csr_matrix((data.copy(), indices.copy(), indptr.copy()), shape=(n, n))
        xk, rk = np.zeros(n), b.copy()
        z = dinv * rk
        p = z.copy()
        rz = rk @ z
        for _ in range(3):
            Ap = M @ p
            al = rz / (p @ Ap)
            xk += al * p
            rk -= al * Ap
            z = dinv * rk
            rz, rz0 = rk @ z, rz
            p = z + (rz / rz0) * p
        # (diagonal 1000, off-diagonal row sums <= 192: condition number < 2, three iterations keep float64's accuracy)
        np.testing.assert_allclose(out[None][0], xk, rtol=1e-9, atol=1e-12)
    finally:
        mat.close()
        comm.close()
