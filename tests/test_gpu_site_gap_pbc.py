"""GPU: kmcf_site_set_gap_pbc and kmcf_filament_gap_pbc (csrc/kmcf_gap.hip, the periodic gp_search_kernel) against the restatement of
tests/site_gap_pbc_ref.py: array_equal on every field of every record and on every integer of the stats; gap within 1 ulp of
sqrt(gap2); a second call the same bytes.  Random site sets on periodic indices of (1,1), (2,3), (3,4), (5,2) and (3,3)
cells in (y, z) at two radii; constructed sets on exact lattices (corner, rim, half a period, ties, two cells, second image,
interior); two filament stumps that face each other across the y face; the periodic 5 nm cell with a filament through its
corner, whole and cut.  On a non-periodic index the _pbc calls return the bytes of the plain calls; the pairwise term and
the cluster analysis are not disturbed; tools/kmc_loop.py --workload 5nm-periodic --gap runs.
tests/test_site_gap_pbc_ref.py shows that the inputs are what their names say.

Every test builds and frees its own communicator."""
import contextlib
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clusters_ref as CR
import pbc_ref as P
import site_gap_pbc_ref as GP
import site_gap_ref as GR
from test_gpu_site_gap import _same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@contextlib.contextmanager
def _comm(km, N):
    c = km.solvers.KMC_comm(1, 2, N, N)
    c.connect()
    try:
        yield c
    finally:
        c.close()


# ---- the search primitive ------------------------------------------------------------------------------------------------------

class _Index:
    """a spatial index over a case's coordinates with the case's cutoff: periodic with the case's lattice, or open"""

    def __init__(self, km, comm, c, periodic=True):
        import torch
        self.km, self.c = km, c
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (f64(c["xyz"][:, k]) for k in range(3))
        self.side = i32(c["side"])
        self.cell = i32(c["cell"]) if c["cell"] is not None else None
        self.handle = C.c_void_p()
        p, lib = km.solvers._ptr, km.lib.load()
        if periodic:
            lat = np.ascontiguousarray(c["L"], np.float64)
            km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                          float(c["cutoff"]), lat.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                                          C.byref(self.handle)), "kmcf_compute_cutoff_list_pbc")
        else:
            km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                      float(c["cutoff"]), C.byref(self.handle)), "kmcf_compute_cutoff_list")

    def gap(self, entry="kmcf_site_set_gap_pbc", r_max=None, stats=True):
        """the C entry itself: (records, stats dict or None)"""
        km, c, p = self.km, self.c, self.km.solvers._ptr
        gaps = np.zeros(c["n_cells"], km.solvers.GAP_DTYPE)
        st = km.lib.GapStats()
        rc = getattr(km.lib.load(), entry)(self.handle, p(self.x), p(self.y), p(self.z), p(self.side),
                                           float(c["r_max"] if r_max is None else r_max), p(self.cell), c["n_cells"],
                                           gaps.ctypes.data_as(C.POINTER(km.lib.Gap)), C.byref(st) if stats else None)
        km.lib.check(rc, entry)
        return gaps, (st.as_dict() if stats else None)

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


@pytest.mark.parametrize("name", GP.SEARCH_CASES)
def test_site_sets_match_the_restatement(km, name):
    c = GP.case(name)
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c)
        try:
            got = ix.gap()
            _same(got, GP.reference(name))
            again = ix.gap()                                         # scratch reused: the same bytes
            assert got[0].tobytes() == again[0].tobytes()
            assert ix.gap(stats=False)[0].tobytes() == got[0].tobytes()
            if name == "rim_wrap":                                  # ... and the same index with r_max just below the pair
                _same(ix.gap(r_max=GP.case("rim_wrap_below")["r_max"]), GP.reference("rim_wrap_below"))
            with pytest.raises(km.lib.KmcfError, match="periodic"):   # the plain call still refuses this index
                ix.gap(entry="kmcf_site_set_gap")
            with pytest.raises(km.lib.KmcfError, match="r_max.*cutoff"):
                ix.gap(r_max=float(np.nextafter(c["cutoff"], np.inf)))
        finally:
            ix.close()


def test_on_a_non_periodic_index_the_bytes_of_the_plain_call(km):
    c = dict(GR.case("mixed"), L=np.array([40.0, 40.0, 40.0]))
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c, periodic=False)
        try:
            plain = ix.gap(entry="kmcf_site_set_gap")
            _same(plain, GR.reference("mixed"))
            got = ix.gap()
            assert got[0].tobytes() == plain[0].tobytes()
            assert {k: got[1][k] for k in GR.STAT_KEYS} == {k: plain[1][k] for k in GR.STAT_KEYS}
        finally:
            ix.close()
        # kmcf_compute_cutoff_list_pbc with pbc = 0: the same index, the same bytes
        h = C.c_void_p()
        p, lib = km.solvers._ptr, km.lib.load()
        lat = np.ascontiguousarray(c["L"], np.float64)
        km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(ix.x), p(ix.y), p(ix.z), len(c["xyz"]), float(c["cutoff"]),
                                                      lat.ctypes.data_as(C.POINTER(C.c_double)), 0, C.byref(h)),
                     "kmcf_compute_cutoff_list_pbc")
        ix.handle = h
        try:
            assert ix.gap()[0].tobytes() == plain[0].tobytes()
        finally:
            ix.close()


# ---- the full call ---------------------------------------------------------------------------------------------------------------

class _Device:
    """buffers with a neighbour list and a spatial index, both periodic (pbc = 1) or both open"""

    def __init__(self, km, comm, xyz, element, L, metals, nn_dist, nn, pbc, sigma=3.5e-10, k=1.0):
        S = km.solvers
        self.S, self.comm, self.N = S, comm, len(xyz)
        xyz = np.array(xyz)                     # (the inputs are read-only)
        self.buf = S.GPUBuffers(self.N, np.array(element), xyz[:, 0], xyz[:, 1], xyz[:, 2], nn, sigma, k, L, metals)
        S.compute_neighbor_list(comm, self.buf, nn_dist, nn, pbc=pbc)
        S.compute_cutoff_list(comm, self.buf, 20.0, pbc=pbc)
        self.neigh = self.buf.neigh_idx.cpu().numpy().reshape(self.N, nn)

    def close(self):
        self.buf.freeGPUmemory()


def _check(got, ref, bins):
    _same((got["gaps"], got["stats"]), (ref["gaps"], ref["stats"]))
    assert np.array_equal(got["side"].cpu().numpy(), ref["side"])
    if bins is not None:
        assert got["profile"].dtype == np.int32 and np.array_equal(got["profile"], ref["profile"])


STUB_BINS = (7, -0.5, 30.5)


def test_stubs_across_the_y_face(km):
    s = GP.stubs()
    args = (s["element"], s["charge"], s["metals"], s["xyz"], s["NL"], s["NR"], GP.STUB_R_MAX)
    with _comm(km, s["N"]) as comm:
        dv = _Device(km, comm, s["xyz"], s["element"], s["L"], s["metals"], P.BOX_NN_DIST, P.BOX_NN, 1)
        try:
            assert np.array_equal(dv.neigh, s["per"])
            run = lambda **kw: dv.S.filament_gap(comm, dv.buf, s["NL"], s["NR"], GP.STUB_R_MAX, periodic=True, **kw)
            full = run(bins=STUB_BINS)
            ref = GP.filament_gap(s["per"], *args, L=s["L"], bins=STUB_BINS)
            _check(full, ref, STUB_BINS)
            g = full["gaps"][0]
            assert (g["site_left"], g["site_right"]) == (s["left"][-1], s["right"][0]) and 7.0 < g["gap"] < 9.0
            for kw in (dict(), dict(sides=False), dict(bins=STUB_BINS, sides=False)):         # NULL outputs
                r = run(**kw)
                assert r["gaps"].tobytes() == full["gaps"].tobytes()
                assert {k: r["stats"][k] for k in GR.STAT_KEYS} == {k: full["stats"][k] for k in GR.STAT_KEYS}
                assert (r["side"] is None) == (kw.get("sides") is False) and (r["profile"] is None) == ("bins" not in kw)
            again = run(bins=STUB_BINS)
            assert again["gaps"].tobytes() == full["gaps"].tobytes() and again["profile"].tobytes() == full["profile"].tobytes()
            # the search primitive on the sides the full call wrote
            r = dv.S.site_set_gap(dv.buf, full["side"], GP.STUB_R_MAX, periodic=True)
            assert r["gaps"].tobytes() == full["gaps"].tobytes()
            with pytest.raises(km.lib.KmcfError, match="periodic"):
                dv.S.filament_gap(comm, dv.buf, s["NL"], s["NR"], GP.STUB_R_MAX)
        finally:
            dv.close()
        # open list, open index: no pair within r_max -- through the _pbc call and through the plain one
        dv = _Device(km, comm, s["xyz"], s["element"], s["L"], s["metals"], P.BOX_NN_DIST, P.BOX_NN, 0)
        try:
            assert np.array_equal(dv.neigh, s["opn"])
            ref = GP.filament_gap(s["opn"], *args, L=None, bins=STUB_BINS)
            got = dv.S.filament_gap(comm, dv.buf, s["NL"], s["NR"], GP.STUB_R_MAX, bins=STUB_BINS, periodic=True)
            _check(got, ref, STUB_BINS)
            assert got["gaps"][0]["site_left"] == -1 and got["stats"]["cells_none"] == 1
            plain = dv.S.filament_gap(comm, dv.buf, s["NL"], s["NR"], GP.STUB_R_MAX, bins=STUB_BINS)
            assert plain["gaps"].tobytes() == got["gaps"].tobytes() and plain["profile"].tobytes() == got["profile"].tobytes()
            assert bool((plain["side"] == got["side"]).all())
        finally:
            dv.close()


R_MAX = 20.0
BINS = (17, -1.0, 52.0)
FILAMENT_RADIUS = 4.0


def _periodic_5nm_with_a_filament(km):
    """structure.periodic_5nm("init") with every oxygen site within 4 A (minimum image) of the line through the cell's
    corner (smallest y, smallest z) turned into a vacancy: a filament along x that passes both periodic faces"""
    d = km.structure.periodic_5nm("init")
    xyz, L = d["xyz"], d["lattice"]
    dy, _ = GP.fold(xyz[:, 1], xyz[:, 1].min(), L[1])
    dz, _ = GP.fold(xyz[:, 2], xyz[:, 2].min(), L[2])
    inside = dy * dy + dz * dz <= FILAMENT_RADIUS ** 2
    element = d["element"].copy()
    element[inside & (element == km.structure.O_EL)] = km.structure.VACANCY
    return d, element


def test_periodic_5nm_cell_with_a_filament_whole_and_cut(km):
    import torch
    d, element = _periodic_5nm_with_a_filament(km)
    N, NL, L, xyz = d["N"], d["N_contact"], d["lattice"], d["xyz"]
    S = km.solvers
    comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
    comm.connect()
    try:
        dv = _Device(km, comm, xyz, element, L, d["metals"], d["nn_dist"], 52, 1, d["sigma"], d["k"])
        try:
            buf = dv.buf
            S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, N, 52, buf.metal_types, buf.num_metal_types_,
                                comm.counts_events, comm.displs_events, comm)
            charge0 = buf.site_charge.cpu().numpy()
            label, table, _ = CR.clusters(dv.neigh, element, charge0, d["metals"], xyz[:, 0], NL, NL)
            x = xyz[:, 0]
            fil = table[(table["kind"] == CR.VAC) & (table["touch"] == 3)]
            assert len(fil) == 1 and fil["size"][0] >= 100
            mid = 0.5 * (fil["x_min"][0] + fil["x_max"][0])
            high = GP.fold(xyz[:, 1], xyz[:, 1].min(), L[1])[1] != 0             # the half of the period below the y face
            for half_width in (None, 2.0, "skew"):
                charge = charge0.copy()
                if half_width is not None:                           # the cut of tests/test_site_gap_ref.py
                    charge[CR.slab_sites(label, table, x, 2.0)] = 2
                if half_width == "skew":
                    # within 8 A of the cut the left stump keeps only its sites below the y face, the right stump only those
                    # above it: the stumps face each other through the face
                    charge[(label == fil["root"][0]) & (np.abs(x - mid) <= 8.0) & (((x < mid) & ~high) | ((x > mid) & high))] = 2
                buf.site_charge.copy_(torch.as_tensor(charge, device="cuda"))
                got = S.filament_gap(comm, buf, NL, NL, R_MAX, bins=BINS, periodic=True)
                ref = GP.filament_gap(dv.neigh, element, charge, d["metals"], xyz, NL, NL, R_MAX, bins=BINS, L=L, propose="tree")
                opn = GP.site_set_gap(xyz, ref["side"], R_MAX, L=None, propose="tree")[0]
                g = got["gaps"][0]
                print("periodic 5 nm, cut %s: %s; open-boundary distance on the same sides: gap2 %r (%d-%d); clusters %.3f ms, "
                      "search %.3f ms" % (half_width, g, opn[0]["gap2"], opn[0]["site_left"], opn[0]["site_right"],
                                          got["stats"]["ms_clusters"], got["stats"]["ms_search"]))
                _check(got, ref, BINS)
                if half_width is None:
                    assert g["bridged"] == 1 and g["gap2"] == 0.0 and g["n_both"] >= 100
                    both = np.flatnonzero(ref["side"] == 3)
                    cy = GP.fold(xyz[both, 1], xyz[:, 1].min(), L[1])[1]
                    assert (cy != 0).any() and (cy == 0).any()      # the filament lies on both sides of the y face
                else:
                    assert g["bridged"] == 0 and g["site_left"] >= 0 and g["gap"] > 0.0
                if half_width == "skew":
                    assert GP.crossings(xyz, g["site_left"], g["site_right"], L)[0] != 0 and g["gap2"] < opn[0]["gap2"]
                again = S.filament_gap(comm, buf, NL, NL, R_MAX, bins=BINS, periodic=True)
                assert again["gaps"].tobytes() == got["gaps"].tobytes() and again["profile"].tobytes() == got["profile"].tobytes()
        finally:
            dv.close()
    finally:
        comm.close()


def test_pairwise_term_and_clusters_are_not_disturbed(km, dev5):
    import torch
    S = km.solvers
    c = P.pairwise_case("p34")
    s = GP.case("p34@20")
    N = c["N"]
    rng = np.random.default_rng(77)
    element = rng.choice([P.O_EL, P.VACANCY, 9], N, p=[0.5, 0.4, 0.1]).astype(np.int32)
    with _comm(km, N) as comm:
        dv = _Device(km, comm, c["xyz"], element, c["L"], np.array([9], np.int32), 3.5, P.NN, 1, dev5["sigma"], dev5["k"])
        try:
            buf = dv.buf
            buf.site_charge.copy_(torch.as_tensor(np.array(c["charge"]), device="cuda"))

            def snapshot():
                cl = S.conductive_clusters(comm, buf, 0, 0)
                S.poisson_gridless_gpu(buf, comm)
                ints = {k: v for k, v in cl["stats"].items() if k != "ms"}
                return (cl["label"].cpu().numpy().tobytes(), cl["clusters"].tobytes(), ints,
                        buf.site_potential_charge.cpu().numpy().tobytes())

            before = snapshot()
            assert np.frombuffer(before[3], np.float64).any() and before[2]["n_clusters"] >= 10
            side = torch.as_tensor(np.array(s["side"]), device="cuda")
            r = S.site_set_gap(buf, side, R_MAX, site_cell=s["cell"], n_cells=s["n_cells"], periodic=True)
            _same((r["gaps"], r["stats"]), GP.reference("p34@20"))
            S.filament_gap(comm, buf, 0, 0, R_MAX, site_cell=s["cell"], n_cells=s["n_cells"], bins=(8, 0.0, 45.0), periodic=True)
            assert snapshot() == before
        finally:
            dv.close()


def test_kmc_loop_periodic_workload_with_the_gap():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kmc_loop.py"), "--workload", "5nm-periodic", "--gap", "20",
                          "--steps", "2"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "sites 37637" in out.stdout
    steps = [l for l in out.stdout.splitlines() if re.search(r"events [0-9.]+ \(\d+ ev\)", l)]
    assert len(steps) == 2 and all(re.search(r"\| gap [0-9.]+\+[0-9.]+ \[0: ", l) for l in steps), steps
