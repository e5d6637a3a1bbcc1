"""GPU: kmcf_site_gradient (csrc/kmcf_gradient.hip) against the float64 restatement of tests/site_gradient_ref.py, every
output of every case:
  integers and flags (full, drop_to, the counts, every site id of the cell table and the stats): equal;
  drop: within 8 * 2^-52 * drop_ref;
  g: per site and component within C * B_i, B_i = 2^-52 n_i S_i (1 + n_i / lam_min) / lam_min, C = 4 * max(1, r_ref) = 4
     (r_ref = 0.059: tests/test_site_gradient_ref.py);
  g_max / drop_max: the maximum of the device's OWN per-site outputs bit for bit, the ids the smallest that attain it, and
     within the bars above of the restatement's.
Where the field a case prescribes ties the |g| of many sites (the linear field, the periodic lattice: see
tests/test_site_gradient_ref.py, which checks the conditions on every input), g_site must lie among the restatement's tied
ids instead of being equal to its choice; nothing else and no site is left out.

Measured on an MI355X, worst |g - g_ref| / B_i over a case: 0.044 (potential of the 5 nm device), 0.032 (linear field),
0.031 (masked), 0.037 / 0.025 (jittered lattice, nn = 4 / 52), at most 0.016 on the random clouds: a hundredth of the bar
(DESIGN.md 3.14)."""
import ctypes as C

import numpy as np
import pytest

import site_gradient_ref as R

pytestmark = pytest.mark.gpu

G_ID_EQUAL_BY_CONSTRUCTION = {"ties1", "ties2"}     # the two copies run through the same additions on the device too


@pytest.fixture(scope="module")
def comm(km):
    c = km.solvers.KMC_comm(1, 2, 1, 1)
    c.connect()
    yield c
    c.close()


def _buffers(km, d, nn=52):
    S = km.solvers
    return S.GPUBuffers(d["N"], d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], nn, d["sigma"], d["k"],
                        d["lattice"], d["metals"])


@pytest.fixture(scope="module")
def neigh5(km, dev5):
    """the 5 nm device's own kmcf_neighbor_list, nn = 52"""
    S, d = km.solvers, dev5
    comm = S.KMC_comm(d["N"] - 2 * d["N_contact"], d["N"] + 1, d["N"], d["N"])
    comm.connect()
    buf = _buffers(km, d)
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    nl = buf.neigh_idx.cpu().numpy().reshape(d["N"], 52)
    comm.close()
    return nl


def _dev(a, dtype):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


def _run(km, comm, c, pbc=None, lattice="case", site=True, tables=True):
    """the C entry itself on a case: dict of numpy outputs (site arrays prefilled with junk: every entry must be written)"""
    import torch
    lib, p = km.lib.load(), km.solvers._ptr
    N = c["N"]
    neigh = _dev(c["neigh"].reshape(-1), np.int32)
    x, y, z = (_dev(c["xyz"][:, k], np.float64) for k in range(3))
    value, mask, cell = _dev(c["value"], np.float64), _dev(c["mask"], np.int32), _dev(c["cell"], np.int32)
    lat = c["lattice"] if isinstance(lattice, str) else lattice
    latp = None if lat is None else np.ascontiguousarray(lat, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    f = lambda: torch.full((N,), float("nan"), dtype=torch.float64, device="cuda") if site else None
    i = lambda: torch.full((N,), -7, dtype=torch.int32, device="cuda") if site else None
    gx, gy, gz, drop, to, full = f(), f(), f(), f(), i(), i()
    cells = np.zeros(c["n_cells"], km.solvers.GRADIENT_CELL_DTYPE)
    st = km.lib.GradientStats()
    rc = lib.kmcf_site_gradient(comm.handle, N, c["nn"], p(neigh), p(x), p(y), p(z), latp, c["pbc"] if pbc is None else pbc,
                                p(value), p(mask), p(cell), c["n_cells"], p(gx), p(gy), p(gz), p(drop), p(to), p(full),
                                cells.ctypes.data_as(C.POINTER(km.lib.GradientCell)) if tables else None,
                                C.byref(st) if tables else None)
    km.lib.check(rc, "kmcf_site_gradient")
    out = dict(cells=cells, stats=st.as_dict())
    if site:
        out.update({k: t.cpu().numpy() for k, t in dict(gx=gx, gy=gy, gz=gz, drop=drop, drop_to=to, full=full).items()})
    return out


def _same_bytes(a, b):
    keys = [k for k in a if k not in ("stats",)]
    return (all(a[k].tobytes() == b[k].tobytes() for k in keys)
            and {k: v for k, v in a["stats"].items() if k != "ms"} == {k: v for k, v in b["stats"].items() if k != "ms"})


def _check(name, ref, got):
    """every output of the device against the restatement; returns the device's worst err_i / B_i"""
    c, out, r_cells, r_st = ref
    st, cells = got["stats"], got["cells"]
    N, n_cells = c["N"], c["n_cells"]
    # per site: integers equal, drop within 8 ulp-units, g within the bar
    assert np.array_equal(got["full"], out["full"]), np.flatnonzero(got["full"] != out["full"])[:5]
    assert np.array_equal(got["drop_to"], out["drop_to"]), np.flatnonzero(got["drop_to"] != out["drop_to"])[:5]
    assert np.all(np.abs(got["drop"] - out["drop"]) <= 8 * R.EPS * out["drop"])
    B = R.bound(out)
    ratio = R.error_ratio(got, out, B)
    for key in ("gx", "gy", "gz"):
        err = np.abs(got[key] - out[key])
        assert np.all(err <= R.C_DEVICE * B), (key, int(np.argmax(err - R.C_DEVICE * B)), float(err.max()))
    print("%s: N %d nn %d, worst |g - g_ref| / B = %.4f (bar %g), %.4f ms" % (name, N, c["nn"], ratio, R.C_DEVICE, st["ms"]))
    # counts
    for k in ("n_sites", "n_full", "n_degenerate", "pairs"):
        assert st[k] == r_st[k], (k, st[k], r_st[k])
    assert np.array_equal(cells["n_sites"], r_cells["n_sites"]) and np.array_equal(cells["n_full"], r_cells["n_full"])
    # maxima: a selection from the device's own outputs, bit for bit, smallest ids
    own = dict(gm=np.sqrt((got["gx"] * got["gx"] + got["gy"] * got["gy"]) + got["gz"] * got["gz"]), drop=got["drop"],
               drop_to=got["drop_to"], full=got["full"], n=out["n"], inn=out["inn"])
    o_cells, o_st = R.tables(own, c["cell"], n_cells)
    for k in ("g_max", "g_site", "drop_max", "drop_from", "drop_to"):
        assert st[k] == o_st[k], (k, st[k], o_st[k])
        assert np.array_equal(cells[k], o_cells[k]), (k, cells[k], o_cells[k])
    # ... and against the restatement's: the values within the bars, the ids equal (g_site among the tied ids where the
    # prescribed field ties)
    rows = R.maxima_rows(out, c["cell"], n_cells)
    cell_of = np.zeros(N, np.int64) if c["cell"] is None else c["cell"].astype(np.int64)
    for row in range(n_cells + 1):
        d, r = (st, r_st) if row == n_cells else (cells[row], r_cells[row])
        sel = out["inn"] if row == n_cells else out["inn"] & (cell_of == row)
        assert abs(d["drop_max"] - r["drop_max"]) <= 8 * R.EPS * r["drop_max"]
        assert (d["drop_from"], d["drop_to"]) == (r["drop_from"], r["drop_to"]), (row, d["drop_from"], r["drop_from"])
        slack = np.sqrt(3.0) * R.C_DEVICE * (B[sel].max() if sel.any() else 0.0)
        assert abs(d["g_max"] - r["g_max"]) <= slack, (row, d["g_max"], r["g_max"])
        tied, close = rows[(row, "g")]
        if name in G_ID_EQUAL_BY_CONSTRUCTION or r["g_max"] == 0.0 or (len(tied) <= 1 and len(close) == 0):
            assert d["g_site"] == r["g_site"], (row, d["g_site"], r["g_site"])
        else:
            assert d["g_site"] in tied or d["g_site"] in close, (row, d["g_site"])
    return ratio


# ---------------------------------------------------------------- 1: linear field on the real device
def test_linear_field_on_the_5nm_device(km, comm, dev5, neigh5):
    ref = R.reference("linear5", dev5, neigh5)
    c, out = ref[0], ref[1]
    got = _run(km, comm, c)
    _check("linear5", ref, got)
    B = R.bound(out)
    assert got["stats"]["n_full"] == 37650 and got["full"].all()
    for k, key in enumerate(("gx", "gy", "gz")):                        # g = a at every site
        assert np.all(np.abs(got[key] - R.LINEAR_A[k]) <= (R.C_DEVICE + 1) * B), key
    # drop = max |a . u| over the counted pairs; the coincident pair contributes nothing
    assert got["stats"]["pairs"] == int((c["neigh"] >= 0).sum()) - 2
    assert np.all(got["drop"] <= np.linalg.norm(R.LINEAR_A) * (1 + 1e-9)) and got["drop"].min() > 0
    assert _same_bytes(got, _run(km, comm, c))                          # two calls, the same bytes


# ---------------------------------------------------------------- 2, 3, 7: small synthetic inputs
@pytest.mark.parametrize("name", ["jitter52", "jitter4", "plane", "line5", "single", "two", "ties1", "ties2"])
def test_synthetic_input_matches_the_restatement(km, comm, name):
    ref = R.reference(name)
    got = _run(km, comm, ref[0])
    _check(name, ref, got)
    if name in ("plane", "line5", "single", "two"):
        assert not got["full"].any() and not got["gx"].any() and not got["gy"].any() and not got["gz"].any()
    if name == "ties2":                                                 # the cells: smallest ids, out-of-range sites
        cells, st = got["cells"], got["stats"]
        assert cells["g_max"][0] == cells["g_max"][1] and cells["g_site"][1] == cells["g_site"][0] + 27
        assert cells["drop_max"][0] == cells["drop_max"][1] and st["g_site"] < 27 and st["drop_from"] < 27
        assert st["n_sites"] == 54 and cells["n_sites"].tolist() == [25, 26]
        one = _run(km, comm, R.reference("ties1")[0])
        for k in ("gx", "gy", "gz", "drop", "drop_to", "full"):         # the cells change no site output
            assert one[k].tobytes() == got[k].tobytes(), k
        assert {k: v for k, v in one["stats"].items() if k != "ms"} == {k: v for k, v in st.items() if k != "ms"}


# ---------------------------------------------------------------- 4: launch edges
@pytest.mark.parametrize("N", R.LAUNCH_N)
def test_launch_edges(km, comm, N):
    for nn in R.LAUNCH_NN:
        name = "cloud_%d_%d" % (N, nn)
        ref = R.reference(name)
        _check(name, ref, _run(km, comm, ref[0]))


def test_outputs_may_be_left_out(km, comm):
    ref = R.reference("cloud_65_17")
    full = _run(km, comm, ref[0])
    only_tables = _run(km, comm, ref[0], site=False)
    assert only_tables["cells"].tobytes() == full["cells"].tobytes()
    assert {k: v for k, v in only_tables["stats"].items() if k != "ms"} == {k: v for k, v in full["stats"].items() if k != "ms"}
    only_site = _run(km, comm, ref[0], tables=False)
    for k in ("gx", "gy", "gz", "drop", "drop_to", "full"):
        assert only_site[k].tobytes() == full[k].tobytes(), k


# ---------------------------------------------------------------- 5: periodic
def test_periodic_lattice(km, comm):
    S = km.solvers
    ref = R.reference("pbc_sin")
    c = ref[0]
    # the list the cases use is the library's periodic list
    d = dict(N=c["N"], element=np.full(c["N"], 3, np.int32), xyz=c["xyz"], sigma=1.0, k=1.0, lattice=c["lattice"], metals=[5])
    buf = _buffers(km, d, 8)
    own = S.KMC_comm(1, 2, 1, c["N"])                                   # (kmcf_neighbor_list builds this rank's event rows)
    own.connect()
    S.compute_neighbor_list(own, buf, 3.0, 8, pbc=1)
    own.close()
    assert np.array_equal(buf.neigh_idx.cpu().numpy().reshape(c["N"], 8), c["neigh"])
    _check("pbc_sin", ref, _run(km, comm, c))
    # a field linear in x: (a_x, 0, 0) within the bar at every site, the faces included
    lin = R.reference("pbc_linx")
    g = _run(km, comm, lin[0])
    _check("pbc_linx", lin, g)
    B = R.bound(lin[1])
    assert np.all(np.abs(g["gx"] - R.PBC_AX) <= (R.C_DEVICE + 1) * B) and np.all(np.abs(g["gy"]) <= (R.C_DEVICE + 1) * B)
    assert np.all(np.abs(g["gz"]) <= (R.C_DEVICE + 1) * B)
    # the same input with pbc = 0: the restatement without the image, and not the periodic result at the y faces
    opn = R.reference("pbc_sin_open")
    o = _run(km, comm, opn[0])
    _check("pbc_sin_open", opn, o)
    p = _run(km, comm, c)
    iy = np.rint(c["xyz"][:, 1] / R.PBC_A - 0.3).astype(int)
    face = (iy == 0) | (iy == 3)
    assert np.all(np.abs(o["gy"][face] - p["gy"][face]) > 0.1) and np.array_equal(o["gy"][~face], p["gy"][~face])
    # with pbc = 0 the bytes do not depend on h_lattice
    assert _same_bytes(o, _run(km, comm, opn[0], lattice=None))
    assert _same_bytes(o, _run(km, comm, opn[0], lattice=np.array([1.0, float("nan"), -3.0])))


# ---------------------------------------------------------------- 6: mask
def test_masked_5nm_device(km, comm, dev5, neigh5):
    ref = R.reference("mask5", dev5, neigh5)
    c, out = ref[0], ref[1]
    got = _run(km, comm, c)
    _check("mask5", ref, got)
    off = c["mask"] == 0
    assert off.sum() == dev5["N"] - got["stats"]["n_sites"] > 0
    for k, v in (("gx", 0.0), ("gy", 0.0), ("gz", 0.0), ("drop", 0.0), ("drop_to", -1), ("full", 0)):
        assert np.all(got[k][off] == v), k
    assert not off[got["drop_to"][got["drop_to"] >= 0]].any()           # no masked-out neighbour is ever the drop's end
    assert got["stats"]["pairs"] < R.reference("linear5", dev5, neigh5)[3]["pairs"]


# ---------------------------------------------------------------- 8: Python surface
def test_field_map_on_the_5nm_device(km, dev5):
    import torch
    S, d = km.solvers, dev5
    NL = d["N_contact"]
    comm = S.KMC_comm(d["N"] - 2 * NL, d["N"] + 1, d["N"], d["N"])
    comm.connect()
    buf = _buffers(km, d)
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    S.compute_cutoff_list(comm, buf)
    S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_, buf.metal_types,
                        buf.num_metal_types_, comm.counts_events, comm.displs_events, comm)
    S.background_potential_gpu_sparse(buf, d["N"], NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"], d["nn_dist"],
                                      len(d["metals"]), 0)
    S.poisson_gridless_gpu(buf, comm)
    fm = S.field_map(comm, buf)
    pot = (buf.site_potential_boundary + buf.site_potential_charge).cpu().numpy()
    assert np.array_equal(fm["potential"].cpu().numpy(), pot)
    c = R._case(buf.neigh_idx.cpu().numpy().reshape(d["N"], 52), d["xyz"], pot)
    out = R.site_gradient(c["neigh"], c["xyz"], c["value"])
    r_cells, r_st = R.tables(out, None, 1)
    got = dict(cells=fm["cells"], stats=fm["stats"])
    for k, e in (("gx", "Ex"), ("gy", "Ey"), ("gz", "Ez")):
        got[k] = fm[k].cpu().numpy()
        assert np.array_equal(fm[e].cpu().numpy(), -got[k]), e           # E = -g
    got.update(drop=fm["drop"].cpu().numpy(), drop_to=fm["drop_to"].cpu().numpy(), full=fm["full"].cpu().numpy())
    _check("field_map", (c, out, r_cells, r_st), got)
    # the cell table: the dtype is the C struct, and it round-trips
    cells = fm["cells"]
    assert cells.dtype == S.GRADIENT_CELL_DTYPE and cells.dtype.itemsize == C.sizeof(km.lib.GradientCell)
    back = np.frombuffer(cells.tobytes(), S.GRADIENT_CELL_DTYPE)
    assert np.array_equal(back, cells) and back["g_site"][0] == fm["stats"]["g_site"]
    as_c = km.lib.GradientCell.from_buffer_copy(cells.tobytes())
    assert (as_c.n_sites, as_c.g_max, as_c.drop_from, as_c.drop_to) == (cells["n_sites"][0], cells["g_max"][0],
                                                                         cells["drop_from"][0], cells["drop_to"][0])
    # the largest |E| exceeds the mean field |Vd| / (x extent of the interface)
    xi = d["xyz"][NL:-NL, 0]
    mean_field = abs(d["Vd"]) / float(xi.max() - xi.min())
    print("largest |E| %.4f V/A at site %d, mean field %.4f V/A, ratio %.2f" % (fm["stats"]["g_max"], fm["stats"]["g_site"],
                                                                               mean_field, fm["stats"]["g_max"] / mean_field))
    assert fm["stats"]["g_max"] > mean_field
    buf.freeGPUmemory()
    comm.close()
