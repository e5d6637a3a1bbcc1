"""GPU: kmcf_current_profile (current through x-planes per cell and pair kind, per-site current vector) against the numpy
restatement tests/current_profile_ref.py built from the device's own exports (pattern, values, tunnel block).

Bars (current_profile_ref.py derives them): profile entry (c, k, t): 2**-52 (n_pairs + n_atoms + n_planes) sum |I| over the
counted pairs of (c, t) whose left end has q <= k; vector component of atom a: n_a 2**-52 sum_s |I_as d_as|.  Where a bar is
zero (no such pair) the device must return exactly 0.  The largest ratio of every comparison is printed; measured on the
MI355X over all cases: profile at most 0.066 of its bar (5 nm device 0.001), vector at most 0.136 (5 nm device)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import current_map_ref as R
import current_profile_ref as PR
import tpath_pbc_ref as QP
import tpath_ref as TR
from test_gpu_current_map import (A_LAT, G0, SHAPES, _case_5nm, _case_small, _n_atoms, _open, _params, _random_field, _update_power,
                                  _upload)
from test_oracle_T import PAR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------- the comparison
def _pairs(S, buf, row0=0):
    rp, col = S.t_pattern(buf)
    return R.pair_list(rp, col, S.t_vectors(buf)["val"], row0, S.t_tunnel(buf))


def _call(S, torch, buf, planes, site_cell, n_cells, vector):
    sc = None if site_cell is None else torch.as_tensor(np.ascontiguousarray(site_cell, np.int32), device="cuda")
    out = S.current_profile(buf, planes, site_cell=sc, n_cells=n_cells, vector=vector)
    if vector:
        out["J"] = np.stack([out[k].cpu().numpy() for k in ("jx", "jy", "jz")], 1)
    return out


def _reference(pairs, m, xyz_atoms, atom_site, planes, site_cell, n_cells, lattice=None):
    na = len(atom_site)
    cell = PR.atom_cells(na, atom_site, site_cell, n_cells)
    return dict(prof=PR.profile_direct(pairs, m, xyz_atoms[:, 0], planes, cell, n_cells), vec=PR.vector(pairs, m, xyz_atoms, lattice),
                nodes=R.node_sums(na + 1, *pairs, m))


def _assert_profile(got, ref, what):
    F, want, bound = got["profile"], ref["prof"]["F"], ref["prof"]["bound"]
    assert F.shape == want.shape
    diff = np.abs(F - want)
    ratio = float((diff / np.maximum(bound, 1e-300)).max())
    print("%s: profile, largest |dev - ref| %.3f of the bound (%d crossing pairs, %d entries)" % (what, ratio, ref["prof"]["n_crossing"], F.size))
    bad = np.argwhere(diff > bound)
    assert len(bad) == 0, "%s: %d profile entries beyond the bound, worst %.3g of it, first (c, k, t) = %s: %.17g against %.17g" % (
        what, len(bad), ratio, tuple(bad[0]), F[tuple(bad[0])], want[tuple(bad[0])])
    return ratio


def _assert_vector(got, ref, N, atom_site, what):
    ratio = 0.0
    for k, name in enumerate("xyz"):
        want, bound = PR.to_sites(N, atom_site, ref["vec"]["J"][:, k]), PR.to_sites(N, atom_site, ref["vec"]["bound"][:, k])
        diff = np.abs(got["J"][:, k] - want)
        ratio = max(ratio, float((diff / np.maximum(bound, 1e-300)).max()))
        bad = np.nonzero(diff > bound)[0]
        assert len(bad) == 0, "%s j%s: %d sites beyond n_a 2^-52 sum |I d|, worst %.3g of the bound (site %d: %.17g against %.17g)" % (
            what, name, len(bad), ratio, bad[0], got["J"][bad[0], k], want[bad[0]])
    rest = np.setdiff1d(np.arange(N), atom_site[:-1])              # nothing outside the atoms' sites; the last atom has no row
    assert not got["J"][rest].any()
    print("%s: vector, largest |dev - ref| %.3f of the bound" % (what, ratio))
    return ratio


def _assert_stats(got, ref, atom_site, vector):
    st, nodes = got["stats"], ref["nodes"]
    want = PR.flux_stats(got["profile"])                           # from the returned profile, in the order the header fixes
    for key in want:
        assert st[key] == want[key], (key, st[key], want[key])
    assert abs(st["i_injection"] - nodes["net"][1]) <= nodes["n"][1] * R.EPS * nodes["S"][1]
    assert abs(st["i_extraction"] + nodes["net"][0]) <= nodes["n"][0] * R.EPS * nodes["S"][0]
    if vector:
        jx = got["J"][:, 0]
        assert abs(st["sum_jx"] - math.fsum(jx)) <= len(atom_site) * R.EPS * float(np.abs(jx).sum())
    else:
        assert st["sum_jx"] == 0.0 and got["jx"] is None and got["jy"] is None and got["jz"] is None
    assert st["ms_pairs"] > 0 and st["ms_planes"] > 0


def _check(S, torch, buf, xyz, m, planes, site_cell, n_cells, what, lattice=None, pairs=None, atom_site=None):
    """Both calls (with and without the vector) against the restatement; returns (with vector, reference)."""
    atom_site = S.t_atom_sites(buf) if atom_site is None else atom_site
    pairs = _pairs(S, buf) if pairs is None else pairs
    ref = _reference(pairs, m, np.asarray(xyz, np.float64)[atom_site], atom_site, planes, site_cell, n_cells, lattice)
    with_v = _call(S, torch, buf, planes, site_cell, n_cells, True)
    without = _call(S, torch, buf, planes, site_cell, n_cells, False)
    # vector on or off: the same profile and statistics, byte for byte
    assert with_v["profile"].tobytes() == without["profile"].tobytes(), what
    for key in ("i_injection", "i_extraction", "flux_min", "flux_max", "plane_min", "plane_max"):
        assert with_v["stats"][key] == without["stats"][key], (what, key)
    _assert_profile(with_v, ref, what)
    _assert_vector(with_v, ref, buf.N_, atom_site, what)
    _assert_stats(with_v, ref, atom_site, True)
    _assert_stats(without, ref, atom_site, False)
    if site_cell is None:
        assert np.all(with_v["profile"][1] == 0.0) and not np.signbit(with_v["profile"][1]).any(), what      # the rest: exactly 0.0
    return with_v, ref


def _mid_planes(x, at_most=64):
    u = np.unique(np.round(np.asarray(x, np.float64), 9))
    mids = 0.5 * (u[:-1] + u[1:])
    if len(mids) > at_most:
        mids = mids[np.round(np.linspace(0, len(mids) - 1, at_most)).astype(int)]
    return mids


def _cells_2x2(xyz):
    y, z = xyz[:, 1], xyz[:, 2]
    return (2 * (y > 0.5 * (y.min() + y.max())) + (z > 0.5 * (z.min() + z.max()))).astype(np.int32)


def _configs(xyz, N):
    """(name, planes, site_cell, n_cells) on a device of small_device()'s lattice: layers at multiples of A_LAT."""
    x = xyz[:, 0]
    mids = np.arange(int(round(x.max() / A_LAT))) * A_LAT + 0.5 * A_LAT
    c4 = _cells_2x2(xyz)
    odd = c4.copy()
    odd[::5] = -1
    odd[1::7] = 4
    odd[2::11] = 1 << 30
    odd[3::13] = -(1 << 31)
    return [("mid-layers, 2 x 2 cells", mids, c4, 4),
            ("one plane", mids[len(mids) // 2:len(mids) // 2 + 1], None, 1),
            ("planes on the layers", np.arange(int(round(x.max() / A_LAT)) + 1) * A_LAT, None, 1),
            ("planes left of every atom", x.min() - np.array([3.0, 2.0, 1e-9]), c4, 4),
            ("300 planes, 1 cell", np.linspace(x.min() - 1.0, x.max() + 1.0, 300), np.zeros(N, np.int32), 1),
            ("3 planes, 130 cells", mids[[1, len(mids) // 2, len(mids) - 2]], (np.arange(N) % 130).astype(np.int32), 130),
            ("cells with -1 and >= n_cells", mids, odd, 4)]


# ---------------------------------------------------------------- one rank: shapes x fields
@pytest.mark.parametrize("field", ["solved", "random"])
@pytest.mark.parametrize("shape", list(SHAPES) + ["5nm"])
def test_shapes_one_rank(km, torch, dev5, ref5, shape, field):
    S = km.solvers
    case, points = (_case_5nm(km, torch, dev5, ref5), 1913) if shape == "5nm" else (SHAPES[shape][0](), SHAPES[shape][1])
    comm, buf = _open(km, torch, case)
    try:
        na, N = buf.N_atom_, buf.N_
        xyz = np.asarray(case["xyz"], np.float64)
        if field == "solved":
            buf.atom_virtual_potentials.zero_()
            im, st = _update_power(S, buf, case, 0)
            assert st["converged"] == 1
            m = buf.atom_virtual_potentials.cpu().numpy().copy()
        else:
            m = _random_field(na + 2, 5)
            _upload(torch, buf, m)
            S.t_assemble(buf, _params(S, case))
        assert S.t_info(buf)["tunnel_points"] == points
        atom_site, pairs = S.t_atom_sites(buf), _pairs(S, buf)
        if shape == "5nm":
            xa = xyz[atom_site, 0]
            configs = [("64 planes, one cell", np.linspace(xa.min(), xa.max(), 66)[1:-1], None, 1)]
        else:
            configs = _configs(xyz, N)
        for name, planes, site_cell, n_cells in configs:
            what = "%s %s, %s" % (shape, field, name)
            got, ref = _check(S, torch, buf, xyz, m, planes, site_cell, n_cells, what, pairs=pairs, atom_site=atom_site)
            F = got["profile"]
            assert F.shape == (n_cells + 1, len(planes), 2)
            if points <= 1:                                        # no pair in the bitmap: every tunnel entry is exactly 0.0
                assert np.all(F[:, :, 1] == 0.0) and not np.signbit(F[:, :, 1]).any()
            if name == "planes left of every atom":
                assert np.all(F == 0.0) and not np.signbit(F).any()
                assert got["stats"]["flux_min"] == 0.0 and got["stats"]["flux_max"] == 0.0
                assert got["stats"]["plane_min"] == 0 and got["stats"]["plane_max"] == 0          # the lowest index among equals
            elif name == "mid-layers, 2 x 2 cells":
                assert np.abs(F[:4]).max() > 0
                if points > 1:
                    assert np.abs(F[4, :, 1]).max() > 0            # tunnel pairs cross the cells: the rest is exercised
            elif name == "cells with -1 and >= n_cells":
                assert np.abs(F[4]).max() > 0
            elif name == "planes on the layers":
                # an atom on a plane lies to its right: plane l * a sees what the mid-layer plane (l - 1/2) a sees
                mid = _call(S, torch, buf, planes[1:] - 0.5 * A_LAT, None, 1, False)["profile"]
                assert mid.tobytes() == F[:, 1:].tobytes()
                assert not F[:, 0].any()                           # nothing lies left of the first layer
        if field == "solved":
            st = got["stats"]
            print("%s solved: i_injection %.9e, total forward current %.9e (plane %d) .. %.9e (plane %d)"
                  % (shape, st["i_injection"], st["flux_min"], st["plane_min"], st["flux_max"], st["plane_max"]))
    finally:
        buf.freeGPUmemory()
        comm.close()


# ---------------------------------------------------------------- mask word edges, periodic state
@pytest.mark.parametrize("name", ["nt_63", "nt_64", "nt_65", "nt_129"])
def test_mask_word_edges(km, torch, monkeypatch, name):
    """The synthetic T path cases whose tunnel point counts sit at the edges of a 64-bit mask word, random potentials."""
    from test_gpu_tpath_synthetic import _device, _prm
    case = TR.tpath_case(name)
    Vd = case["par"]["Vd"]
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        S.t_assemble(buf, _prm(S, case, Vd))
        assert S.t_info(buf)["tunnel_points"] == int(name[3:])
        m = _random_field(buf.N_atom_ + 2, 31)
        _upload(torch, buf, m)
        xyz = np.asarray(case["xyz"], np.float64)
        atom_site = S.t_atom_sites(buf)
        got, _ = _check(S, torch, buf, xyz, m, _mid_planes(xyz[atom_site, 0]), _cells_2x2(xyz), 4, name)
        assert np.abs(got["profile"][:, :, 1]).max() > 0
        _check(S, torch, buf, xyz, m, _mid_planes(xyz[atom_site, 0], 3), None, 1, name + ", one cell")


def test_periodic_state(km, torch, monkeypatch):
    """pbc_nt_65 on the periodic T state: the profile and J against the restatement with the minimum image; the device
    has pairs through a face, and there the restatement with open displacements is another vector."""
    from test_gpu_tpath_pbc import _device, _knobs
    from test_gpu_tpath_synthetic import _prm
    name = "pbc_nt_65"
    open_ref = TR.case_ref
    monkeypatch.setattr(TR, "case_ref", lambda n, Vd=None: QP.case_ref_pbc(n, Vd) if n in QP.CASES_PBC else open_ref(n, Vd))
    case = QP.tpath_pbc_case(name)
    _knobs(monkeypatch, case)
    Vd = case["par"]["Vd"]
    with _device(km, torch, name, Vd) as (S, buf, ref, kw):
        S.t_assemble(buf, _prm(S, case, Vd))
        assert S.t_periodic(buf)[0] == 1
        m = _random_field(buf.N_atom_ + 2, 32)
        _upload(torch, buf, m)
        xyz, L = np.asarray(case["xyz"], np.float64), [float(v) for v in case["L"]]
        atom_site, pairs = S.t_atom_sites(buf), _pairs(S, buf)
        planes = _mid_planes(xyz[atom_site, 0])
        got, ref_p = _check(S, torch, buf, xyz, m, planes, _cells_2x2(xyz), 4, name, lattice=L, pairs=pairs, atom_site=atom_site)
        # pairs through a face: the open displacement is another one
        a, s, i, tn = PR.counted(pairs, m)
        xa = xyz[atom_site]
        through = np.abs(PR.displacement(xa, a, s, L) - PR.displacement(xa, a, s)).max(1) > 1e-9
        assert through.any()
        ref_o = PR.vector(pairs, m, xa)
        moved = np.unique(a[through])
        far = np.zeros(buf.N_, bool)
        for k in (1, 2):
            open_sites = PR.to_sites(buf.N_, atom_site, ref_o["J"][:, k])
            bound = PR.to_sites(buf.N_, atom_site, ref_p["vec"]["bound"][:, k])
            far |= np.abs(got["J"][:, k] - open_sites) > bound
        assert far[atom_site[moved]].any()
        print("%s: %d of %d counted pairs pass a face (%d of them tunnel pairs); the open restatement misses J at %d sites"
              % (name, int(through.sum()), len(a), int((through & tn).sum()), int(far.sum())))


# ---------------------------------------------------------------- storages of the tunnel block
def test_profile_does_not_depend_on_the_storage(km, torch, monkeypatch):
    """386 points held as bitmap + values, dense tiles, jagged tiles: the call walks the bitmap and evaluates the pairs
    afresh, so profile and J are the same bytes; each is within the bounds of the restatement built from the values that
    storage exports."""
    S = km.solvers
    case = _case_small(ny=8, nz=8, n_oxide_layers=9)
    xyz = np.asarray(case["xyz"], np.float64)
    res = {}
    for dense in (0, 1, 2):
        monkeypatch.setenv("KMCF_SUB_DENSE", str(dense))
        comm, buf = _open(km, torch, case)
        try:
            m = _random_field(buf.N_atom_ + 2, 9)
            _upload(torch, buf, m)
            S.t_assemble(buf, _params(S, case))
            info = S.t_info(buf)
            assert info["tunnel_dense"] == dense and info["tunnel_points"] == 386 and buf.N_atom_ == 960
            name, planes, site_cell, n_cells = _configs(xyz, buf.N_)[0]
            res[dense], _ = _check(S, torch, buf, xyz, m, planes, site_cell, n_cells, "storage %d" % dense)
        finally:
            buf.freeGPUmemory()
            comm.close()
    for dense in (1, 2):
        assert res[dense]["profile"].tobytes() == res[0]["profile"].tobytes(), dense
        assert res[dense]["J"].tobytes() == res[0]["J"].tobytes(), dense
        for key in res[0]["stats"]:
            assert key.startswith("ms_") or res[dense]["stats"][key] == res[0]["stats"][key], (dense, key)


# ---------------------------------------------------------------- rank groups
@pytest.mark.parametrize("P,transport,storage", [(P, tr, stg) for P in (2, 3) for tr in ("loopback", "p2p") for stg in ("bitmap", "tiles")])
def test_rank_groups(km, torch, P, transport, storage, monkeypatch):
    """small_91 over an in-process group, set up as test_gpu_current_map.py::test_rank_groups: every rank matches the
    restatement (built from the one-rank state's exports) within the bounds, all ranks return the same bytes."""
    S = km.solvers
    case = _case_small()
    xyz = np.asarray(case["xyz"], np.float64)
    N, na = len(case["element"]), _n_atoms(case)
    fields = [_random_field(na + 2, 21), PAR["Vd"] * G0 * (0.5 + 0.5 * np.cos(np.arange(na + 2) * 0.05))]
    name, planes, site_cell, n_cells = _configs(xyz, N)[0]
    monkeypatch.setenv("KMCF_SUB_DENSE", "0")
    monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    comm, buf = _open(km, torch, case)
    atom_site = S.t_atom_sites(buf)
    S.t_assemble(buf, _params(S, case))
    pairs = _pairs(S, buf)
    refs = [_reference(pairs, m, xyz[atom_site], atom_site, planes, site_cell, n_cells) for m in fields]
    buf.freeGPUmemory()
    comm.close()
    monkeypatch.setenv("KMCF_SUB_DENSE", "1" if storage == "tiles" else "0")
    monkeypatch.setenv("KMCF_SUB_STRIP", "1")
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    comms = S.KMC_comm.loopback_group(na + 1, na + 1, N, N, P)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            _, b = _open(km, torch, case, comms[r])
            S.t_assemble(b, _params(S, case))
            assert S.t_info(b)["tunnel_dense"] == (1 if storage == "tiles" else 0)
            res = []
            for m in fields:
                _upload(torch, b, m)
                first = _call(S, torch, b, planes, site_cell, n_cells, True)
                again = _call(S, torch, b, planes, site_cell, n_cells, True)
                assert first["profile"].tobytes() == again["profile"].tobytes() and first["J"].tobytes() == again["J"].tobytes()
                res.append(first)
            out[r] = res
            b.freeGPUmemory()
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(180)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish"
    for c in comms:
        c.close()
    for f, ref in enumerate(refs):
        for r, o in enumerate(out):
            g = o[f]
            what = "P %d %s %s rank %d field %d" % (P, transport, storage, r, f)
            assert g["profile"].tobytes() == out[0][f]["profile"].tobytes() and g["J"].tobytes() == out[0][f]["J"].tobytes(), what
            for key in g["stats"]:
                assert key.startswith("ms_") or g["stats"][key] == out[0][f]["stats"][key], (what, key)
            _assert_profile(g, ref, what)
            _assert_vector(g, ref, N, atom_site, what)
            _assert_stats(g, ref, atom_site, True)


# ---------------------------------------------------------------- determinism, untouched state, statistics, errors
def test_determinism_and_untouched_state(km, torch):
    S = km.solvers
    case = _case_small()
    xyz = np.asarray(case["xyz"], np.float64)
    comm, buf = _open(km, torch, case)
    try:
        na, N = buf.N_atom_, buf.N_
        x0 = np.zeros(na + 2)
        x0[:na + 1] = PAR["Vd"] * (0.5 + 0.5 * np.cos(np.arange(na + 1) * 0.05)) + 1e-3 * np.random.default_rng(1).standard_normal(na + 1)

        def power():
            _upload(torch, buf, x0)
            buf.site_power.fill_(-7.0)
            im, st = _update_power(S, buf, case, 1, cg_tolerance=1e-30, cg_max_iterations=0)
            return im, buf.atom_virtual_potentials.cpu().numpy().copy(), buf.site_power.cpu().numpy().copy()

        im, m, pw = power()
        tn, vec = S.t_tunnel(buf), S.t_vectors(buf)
        name, planes, site_cell, n_cells = _configs(xyz, N)[0]

        def cmap():
            o = S.current_map(buf)
            return [o[k].cpu().numpy().tobytes() for k in ("current", "tunnel", "net")] + [{k: v for k, v in o["stats"].items() if k != "ms"}]

        before = cmap()
        first, ref = _check(S, torch, buf, xyz, m, planes, site_cell, n_cells, "prescribed potentials")
        again = _call(S, torch, buf, planes, site_cell, n_cells, True)
        assert first["profile"].tobytes() == again["profile"].tobytes() and first["J"].tobytes() == again["J"].tobytes()
        for key in first["stats"]:
            assert key.startswith("ms_") or first["stats"][key] == again["stats"][key]
        # a smaller and a larger profile in between do not disturb the next call (the output buffers only grow)
        _call(S, torch, buf, planes[:2], None, 1, False)
        _call(S, torch, buf, np.linspace(-1.0, 40.0, 700), (np.arange(N) % 9).astype(np.int32), 9, True)
        third = _call(S, torch, buf, planes, site_cell, n_cells, True)
        assert first["profile"].tobytes() == third["profile"].tobytes() and first["J"].tobytes() == third["J"].tobytes()
        assert cmap() == before                                    # the current map before and after: the same bytes
        # the current map's i_injection is the profile's
        assert first["stats"]["i_injection"] == before[3]["i_injection"] and first["stats"]["i_extraction"] == before[3]["i_extraction"]
        # untouched: potentials, site_power, the tunnel block, the matrix, and what the next power update gives
        np.testing.assert_array_equal(buf.atom_virtual_potentials.cpu().numpy(), m)
        np.testing.assert_array_equal(buf.site_power.cpu().numpy(), pw)
        tn2, vec2 = S.t_tunnel(buf), S.t_vectors(buf)
        for key in tn:
            np.testing.assert_array_equal(tn2[key], tn[key])
        for key in vec:
            np.testing.assert_array_equal(vec2[key], vec[key])
        im2, m2, pw2 = power()
        assert im2 == im
        np.testing.assert_array_equal(m2, m)
        np.testing.assert_array_equal(pw2, pw)
        # potentials given explicitly; all equal: no current anywhere, and ties go to the lowest plane
        flat = torch.full((na + 2,), 0.25, dtype=torch.float64, device="cuda")
        z = S.current_profile(buf, planes, potentials=flat, vector=True)
        assert not z["profile"].any() and not z["jx"].cpu().numpy().any()
        assert z["stats"]["flux_min"] == 0.0 and z["stats"]["flux_max"] == 0.0 and z["stats"]["plane_min"] == 0 and z["stats"]["plane_max"] == 0
        assert z["stats"]["i_injection"] == 0.0 and z["stats"]["sum_jx"] == 0.0
        # a tie that is not at plane 0: two planes in one gap between layers see the same pairs
        two = _call(S, torch, buf, np.array([planes[0], planes[4] - 0.1, planes[4] + 0.1]), None, 1, False)
        tot = PR.total(two["profile"])
        assert tot[1] == tot[2] and tot[1] != tot[0]
        assert two["stats"]["plane_max" if tot[1] > tot[0] else "plane_min"] == 1
    finally:
        buf.freeGPUmemory()
        comm.close()


def test_needs_an_assembled_state(km, torch):
    S = km.solvers
    case = _case_small(ny=2, nz=2, n_oxide_layers=3)
    comm, buf = _open(km, torch, case)
    try:
        lib = km.lib.load()
        x, out = (C.c_double * 2)(1.0, 2.0), (C.c_double * 8)()
        rc = lib.kmcf_current_profile(buf.T_distributed, C.c_void_p(buf.atom_virtual_potentials.data_ptr()), None, 1, x, 2, out, None, None, None,
                                      None)
        assert rc == -4 and b"kmcf_current_profile" in lib.kmcf_last_error()                # KMCF_ERR_STATE
        with pytest.raises(km.lib.KmcfError):
            S.current_profile(buf, [1.0, 2.0])
        S.t_assemble(buf, _params(S, case))
        assert S.current_profile(buf, [1.0, 2.0])["profile"].shape == (2, 2, 2)
    finally:
        buf.freeGPUmemory()
        comm.close()


# ---------------------------------------------------------------- the conducting 4 x 4 crossbar
def test_conducting_crossbar(km, torch):
    """structure.synth_crossbar_40nm(tiles=4, filament=4.0), set up as tests/test_gpu_conducting.py's one-rank case
    (17 722 tunnel points): cells from crossbar_lines, 32 planes between the contact blocks.  The restatement is out of
    reach here (1.4e8 pairs), so only what can be derived is held: (i) conservation with the device's own site_net: at every
    plane with all atoms bonded to the injection node on its left and the atoms bonded to the extraction node or carrying
    the ground start value on its right, |F_total[k] - i_injection| <= sum over the atoms left of k of |net_a| + bound;
    (ii) cells + rest add up to the one-cell profile within the bound.  bound: the profile bound with its counts and sums
    replaced by upper limits the current map gives, 2**-52 (pairs + atoms + planes) * 2 sum_through.  Which cell carries
    the current is printed, not asserted."""
    from test_gpu_conducting import _current, _device
    dev = _device(km, 4.0)
    try:
        S, d, buf = dev["S"], dev["d"], dev["buf"]
        N, NL = d["N"], d["N_contact"]
        im, il, st, info, _ = _current(dev, 1e-15, first=True)
        assert info["tunnel_points"] == 17722 and st["converged"] == 1
        cells = np.ascontiguousarray(km.structure.crossbar_lines(d)[2], np.int32)
        n_cells = int(cells.max()) + 1
        x_l, x_r = float(d["xyz"][:NL, 0].max()), float(d["xyz"][N - NL:, 0].min())
        planes = x_l + (x_r - x_l) * np.arange(1, 33) / 33
        cm = S.current_map(buf)
        got = _call(S, torch, buf, planes, cells, n_cells, True)
        one = _call(S, torch, buf, planes, None, 1, False)
        F, ps = got["profile"], got["stats"]
        assert ps["i_injection"] == cm["stats"]["i_injection"] and ps["i_injection"] > 0
        want = PR.flux_stats(F)
        for key in want:
            assert ps[key] == want[key], key
        atom_site = S.t_atom_sites(buf)
        na = len(atom_site)
        rp, col = S.t_pattern(buf)
        pairs_all = cm["stats"]["tunnel_pairs_walked"] + len(col)
        bound = R.EPS * (pairs_all + na + len(planes)) * 2.0 * cm["stats"]["sum_through"]
        # (ii) cells + rest against one cell
        diff = np.abs(F.sum(0) - one["profile"][0])
        print("cells + rest against the one-cell profile: largest difference %.3e, bound %.3e" % (diff.max(), bound))
        assert np.all(diff <= bound) and np.all(one["profile"][1] == 0.0)
        # (i) conservation
        xa = np.asarray(d["xyz"], np.float64)[atom_site]
        q = PR.slabs(planes, xa[:, 0])
        inj, ext = col[rp[1]:rp[2]], col[rp[0]:rp[1]]
        inj, ext = inj[inj >= 2] - 2, ext[ext >= 2] - 2
        ground = np.nonzero(np.sqrt(((xa[:-1] - xa[-1]) ** 2).sum(1)) < d["nn_dist"])[0]
        net_a = np.abs(cm["net"].cpu().numpy()[atom_site[:-1]])
        tot = PR.total(F)
        checked, worst = 0, 0.0
        for k in range(len(planes)):
            if q[inj].max() <= k < min(q[ground].min(), q[ext].min()):
                tol = float(net_a[q[:-1] <= k].sum()) + bound
                worst = max(worst, abs(tot[k] - ps["i_injection"]) / tol)
                assert abs(tot[k] - ps["i_injection"]) <= tol, (k, tot[k], ps["i_injection"], tol)
                checked += 1
        assert checked >= len(planes) - 2, checked                # (the planes lie between the contact blocks)
        print("conservation at %d planes: largest |F_total - i_injection| %.3f of (sum |net_a| + bound); flux %.9e .. %.9e, I_macro %.9e"
              % (checked, worst, ps["flux_min"], ps["flux_max"], im))
        mid = len(planes) // 2
        for c in range(n_cells + 1):
            t = F[c].sum(1)
            print("  %-7s I(plane %d) %+.6e  tunnel share %.4f" % ("rest" if c == n_cells else "cell %d" % c, mid, t[mid],
                                                                   F[c, mid, 1] / t[mid] if t[mid] != 0 else 0.0))
        print("  device time: pairs %.3f ms, planes %.3f ms (with the vector; without: %.3f, %.3f); current map %.3f ms"
              % (ps["ms_pairs"], ps["ms_planes"], one["stats"]["ms_pairs"], one["stats"]["ms_planes"], cm["stats"]["ms"]))
        assert abs(ps["sum_jx"]) > 0
    finally:
        dev["buf"].freeGPUmemory()
        dev["comm"].close()
