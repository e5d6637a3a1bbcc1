"""GPU: kmcf_pair_correlation and kmcf_defect_correlation (csrc/kmcf_paircorr.hip) against the restatement of
tests/pair_corr_ref.py: np.array_equal on hist, members, edge2, every entry of the count rows (prefilled with junk on the
device) and every integer of the stats -- no tolerance anywhere; a second call on reused scratch, a call with stats = NULL
and a call with d_site_count = NULL the same bytes.  Every case on a periodic index; the random cases at their first
setting, the lattice, the edge probes, the tile edges and the small cases also on an open index over the same
coordinates, each against its own reference.  The Python wrappers, pair_rdf and defect_correlation (probe_all 0 and 1,
periodic and open); the pairwise term and kmcf_site_set_gap on the same index are not disturbed; tools/kmc_loop.py
--pair-correlation runs; the stream ordering contract with the protocol of tests/test_gpu_stream_order.py.
tests/test_pair_corr_ref.py shows that the inputs are what their names say.

Every test builds and frees its own communicator."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pair_corr_ref as R
import pbc_ref as P
import site_gap_pbc_ref as GP
from test_gpu_site_gap_pbc import _comm, _Device
from test_gpu_stream_order import _Filler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK = -77
OPEN_TOO = tuple(n for n in R.CASES if not (n[0] == "p" and not n.endswith("#0")))


class _Index:
    """a spatial index over a case's coordinates with the case's cutoff: periodic with the case's lattice, or open"""

    def __init__(self, km, comm, c, periodic=True):
        import torch
        self.km, self.c, self.torch = km, c, torch
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (f64(c["xyz"][:, k]) for k in range(3))
        self.cls = i32(c["cls"])
        self.cell = i32(c["cell"]) if c["cell"] is not None else None
        self.handle = C.c_void_p()
        p, lib = km.solvers._ptr, km.lib.load()
        N = len(c["xyz"])
        if periodic:
            lat = np.ascontiguousarray(c["L"], np.float64)
            km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(self.x), p(self.y), p(self.z), N, float(c["cutoff"]),
                                                          lat.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(self.handle)),
                         "kmcf_compute_cutoff_list_pbc")
        else:
            km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(self.x), p(self.y), p(self.z), N, float(c["cutoff"]),
                                                      C.byref(self.handle)), "kmcf_compute_cutoff_list")

    def call(self, stats=True, counts=True, r_max=None, cls=None):
        """the C entry itself: dict(hist, members, edge2, counts (numpy or None), stats (dict or None))"""
        km, c, p, torch = self.km, self.c, self.km.solvers._ptr, self.torch
        N, ncl, nb, nc = len(c["xyz"]), c["n_classes"], c["n_bins"], c["n_cells"]
        hist = np.full((nc + 1, R.n_pairs(ncl), nb), 0xdead, np.uint64)
        members = np.full((nc + 1, ncl), JUNK, np.int32)
        edge2 = np.full(nb + 1, -1.0)
        cnt = torch.full((N, ncl), JUNK, dtype=torch.int32, device="cuda") if counts else None
        st = km.lib.PairStats()
        rc = km.lib.load().kmcf_pair_correlation(self.handle, p(self.x), p(self.y), p(self.z), p(self.cls if cls is None else cls), ncl,
                                                 float(c["r_max"] if r_max is None else r_max), nb, float(c["r_count"]), p(self.cell),
                                                 nc, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 members.ctypes.data_as(C.POINTER(C.c_int)),
                                                 edge2.ctypes.data_as(C.POINTER(C.c_double)), p(cnt), C.byref(st) if stats else None)
        km.lib.check(rc, "kmcf_pair_correlation")
        return dict(hist=hist, members=members, edge2=edge2, counts=cnt.cpu().numpy() if counts else None,
                    stats=st.as_dict() if stats else None)

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


def _same(got, ref, what=""):
    """every output equal, no tolerance"""
    for k in ("hist", "members", "edge2"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (what, k, int((got[k] != ref[k]).sum()))
    if got["counts"] is not None:
        g = got["counts"].cpu().numpy() if hasattr(got["counts"], "cpu") else got["counts"]
        assert g.dtype == np.int32 and np.array_equal(g, ref["counts"]), (what, "counts", np.flatnonzero((g != ref["counts"]).any(1))[:8])
    if got["stats"] is not None:
        assert {k: got["stats"][k] for k in R.STAT_KEYS} == ref["stats"], (what, got["stats"], ref["stats"])


def _bytes(r):
    return tuple(r[k].tobytes() for k in ("hist", "members", "edge2"))


@pytest.mark.parametrize("name", R.CASES)
def test_cases_match_the_restatement(km, name):
    c = R.case(name)
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False) if name in OPEN_TOO else (True,):
            ref = R.reference(name, periodic)
            ix = _Index(km, comm, c, periodic)
            try:
                got = ix.call()
                print("%s, %s index: %d pairs, %d members, %d probes, max count %d at %d, %.3f ms" % (
                    name, "periodic" if periodic else "open", got["stats"]["n_pairs_total"], got["stats"]["n_members"],
                    got["stats"]["n_probes"], got["stats"]["max_count"], got["stats"]["max_count_site"], got["stats"]["ms"]))
                _same(got, ref, (name, periodic))
                again = ix.call()                                        # scratch reused: the same bytes
                assert _bytes(again) == _bytes(got) and again["counts"].tobytes() == got["counts"].tobytes()
                assert {k: again["stats"][k] for k in R.STAT_KEYS} == {k: got["stats"][k] for k in R.STAT_KEYS}
                bare = ix.call(stats=False)
                assert _bytes(bare) == _bytes(got) and bare["counts"].tobytes() == got["counts"].tobytes()
                bare = ix.call(counts=False)
                assert _bytes(bare) == _bytes(got)
                assert {k: bare["stats"][k] for k in R.STAT_KEYS} == {k: got["stats"][k] for k in R.STAT_KEYS}
                with pytest.raises(km.lib.KmcfError, match="r_max.*cutoff"):
                    ix.call(r_max=float(np.nextafter(c["cutoff"], np.inf)))
            finally:
                ix.close()


def test_periodic_and_open_references_differ_where_the_wrap_matters():
    """(what the two kinds of index are told apart by)"""
    for name in ("p34#0", "lattice_wrap"):
        assert not np.array_equal(R.reference(name, True)["hist"], R.reference(name, False)["hist"])
        assert not np.array_equal(R.reference(name, True)["counts"], R.reference(name, False)["counts"])


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------

def _buffers(km, comm, c, periodic):
    S = km.solvers
    xyz, N = c["xyz"], len(c["xyz"])
    buf = S.GPUBuffers(N, np.zeros(N, np.int32), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]), 1, 1.0, 1.0,
                       np.array(c["L"]) if periodic else [1.0, 1.0, 1.0], np.array([6], np.int32))
    S.compute_cutoff_list(comm, buf, c["cutoff"], pbc=1 if periodic else 0)
    return buf


@pytest.mark.parametrize("name, periodic", [("p23#0", True), ("p23#2", False), ("four_classes", True), ("one_class", False)])
def test_python_wrapper_and_rdf(km, name, periodic):
    import torch
    c, ref = R.case(name), R.reference(name, periodic)
    S = km.solvers
    with _comm(km, len(c["xyz"])) as comm:
        buf = _buffers(km, comm, c, periodic)
        try:
            cls = torch.as_tensor(np.array(c["cls"]), device="cuda")
            got = S.pair_correlation(buf, cls, c["n_classes"], c["r_max"], c["n_bins"], r_count=c["r_count"], site_cell=c["cell"],
                                     n_cells=c["n_cells"], counts=True)
            assert got["hist"].shape == (c["n_cells"] + 1, R.n_pairs(c["n_classes"]), c["n_bins"]) and got["hist"].dtype == np.uint64
            _same(got, ref, name)
            assert np.array_equal(got["edges"], ref["edges"])
            bare = S.pair_correlation(buf, cls, c["n_classes"], c["r_max"], c["n_bins"], r_count=c["r_count"], site_cell=c["cell"],
                                      n_cells=c["n_cells"])
            assert bare["counts"] is None and _bytes(bare) == _bytes(got)
            # r_count defaults to r_max
            full = S.pair_correlation(buf, cls, c["n_classes"], c["r_max"], c["n_bins"], site_cell=c["cell"], n_cells=c["n_cells"],
                                      counts=True)
            want = R.pair_correlation(c["xyz"], c["cls"], c["n_classes"], c["r_max"], c["n_bins"], None, c["cell"], c["n_cells"],
                                      c["L"] if periodic else None)
            _same(full, want, name)
            vol = 1234.5
            g, w = S.pair_rdf(got, vol), R.pair_rdf(ref, vol)
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w))
            assert np.allclose(g[~np.isnan(g)], w[~np.isnan(w)], rtol=1e-13, atol=0.0)
        finally:
            buf.freeGPUmemory()


@pytest.mark.parametrize("pbc", [1, 0])
def test_defect_correlation(km, pbc):
    import torch
    d = R.defects()
    r_max, n_bins, r_count = R.DEFECT_SETTING
    S = km.solvers
    with _comm(km, d["N"]) as comm:
        dv = _Device(km, comm, d["xyz"], d["element"], d["L"], d["metals"], P.BOX_NN_DIST, P.BOX_NN, pbc)
        try:
            dv.buf.site_charge.copy_(torch.as_tensor(np.array(d["charge"]), device="cuda"))
            for probe_all in (False, True):
                ref = R.defects_reference(probe_all, bool(pbc))
                got = S.defect_correlation(comm, dv.buf, r_max, n_bins, r_count=r_count, site_cell=d["cell"], n_cells=d["n_cells"],
                                           counts=True, probe_all=probe_all, classes=True)
                _same(got, ref, ("defects", pbc, probe_all))
                assert np.array_equal(got["site_class"].cpu().numpy(), ref["cls"])
                assert got["stats"]["n_probes"] == (int((ref["cls"] == 3).sum()) if probe_all else 0)
                bare = S.defect_correlation(comm, dv.buf, r_max, n_bins, r_count=r_count, site_cell=d["cell"], n_cells=d["n_cells"],
                                            probe_all=probe_all)
                assert bare["site_class"] is None and bare["counts"] is None and _bytes(bare) == _bytes(got)
                # the classes it wrote, through the primitive
                prim = S.pair_correlation(dv.buf, got["site_class"], 3, r_max, n_bins, r_count=r_count, site_cell=d["cell"],
                                          n_cells=d["n_cells"], counts=True)
                assert _bytes(prim) == _bytes(got) and bool((prim["counts"] == got["counts"]).all())
        finally:
            dv.close()


def test_pairwise_term_and_gap_are_not_disturbed(km, dev5):
    import torch
    S = km.solvers
    c, s, pc = P.pairwise_case("p34"), GP.case("p34@20"), R.case("p34#0")
    N = c["N"]
    rng = np.random.default_rng(78)
    element = rng.choice([P.O_EL, P.VACANCY, P.OXYGEN_DEFECT, 9], N, p=[0.4, 0.4, 0.1, 0.1]).astype(np.int32)
    with _comm(km, N) as comm:
        dv = _Device(km, comm, c["xyz"], element, c["L"], np.array([9], np.int32), 3.5, P.NN, 1, dev5["sigma"], dev5["k"])
        try:
            buf = dv.buf
            buf.site_charge.copy_(torch.as_tensor(np.array(c["charge"]), device="cuda"))
            side = torch.as_tensor(np.array(s["side"]), device="cuda")

            def snapshot():
                S.poisson_gridless_gpu(buf, comm)
                r = S.site_set_gap(buf, side, 20.0, site_cell=s["cell"], n_cells=s["n_cells"], periodic=True)
                ints = {k: v for k, v in r["stats"].items() if not k.startswith("ms")}
                return buf.site_potential_charge.cpu().numpy().tobytes(), r["gaps"].tobytes(), ints

            before = snapshot()
            assert np.frombuffer(before[0], np.float64).any()
            cls = torch.as_tensor(np.array(pc["cls"]), device="cuda")
            got = S.pair_correlation(buf, cls, 3, pc["r_max"], pc["n_bins"], r_count=pc["r_count"], site_cell=pc["cell"],
                                     n_cells=pc["n_cells"], counts=True)
            _same(got, R.reference("p34#0"))
            S.defect_correlation(comm, buf, 20.0, 32, counts=True, probe_all=True)
            assert snapshot() == before
        finally:
            dv.close()


def test_kmc_loop_periodic_workload_with_the_pair_correlation():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kmc_loop.py"), "--workload", "5nm-periodic", "--steps", "1",
                          "--pair-correlation", "20"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "sites 37637" in out.stdout
    lines = out.stdout.splitlines()
    assert len([l for l in lines if re.search(r"pairs cell 0: V0 \d+ V\+ \d+ ion \d+ \| V-V ", l)]) == 1, lines
    assert len([l for l in lines if re.search(r"pairs device: \d+ pairs, \d+ defects, \d+ probes \| densest site \d+ \(\d+ defects", l)]) == 1


# ---- stream ordering -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def filler():
    import torch
    f = _Filler(torch)
    print("filler: %.1f ms on the device (%.1f ms to launch)" % (f.ms, f.launch_ms))
    assert f.ms >= 10.0, "the filler lasts %.2f ms" % f.ms
    return f


_SIDE = []


@pytest.mark.parametrize("stream", ["default", "side"])
def test_call_waits_for_the_callers_stream(km, filler, stream):
    """A decoy class array (all none) sits on the device; the true classes are copied behind the filler on the caller's
    stream; stream.query() is False before and True after the call; the outputs equal the synchronised reference."""
    import contextlib
    import torch
    name = "p23#0"
    c, ref = R.case(name), R.reference(name)
    assert ref["stats"]["n_pairs_total"] > 0
    if stream == "side" and not _SIDE:
        _SIDE.append(torch.cuda.Stream())
    side = _SIDE[0] if stream == "side" else None
    with _comm(km, len(c["xyz"])) as comm:
        if side is not None:
            km.lib.check(km.lib.load().kmcf_comm_set_caller_stream(comm.handle, side.cuda_stream), "kmcf_comm_set_caller_stream")
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            st = torch.cuda.current_stream()
            ix = _Index(km, comm, c)
            try:
                decoy = torch.full((len(c["xyz"]),), -1, dtype=torch.int32, device="cuda")
                true = ix.cls
                torch.cuda.synchronize()
                empty = ix.call(cls=decoy)                      # the decoy's own answer (and the scratch is allocated)
                assert empty["stats"]["n_members"] == 0 and not empty["hist"].any()
                torch.cuda.synchronize()
                filler.queue()
                decoy.copy_(true, non_blocking=True)
                marker = torch.cuda.Event()
                marker.record(st)
                busy = st.query()
                got = ix.call(cls=decoy)
                reached, done = marker.query(), st.query()
                assert busy is False, "the caller's stream was idle at the call: the filler is too short"
                assert reached is True, "the call returned before the work queued on the caller's stream had finished"
                assert done is True, "the call returned with work pending on the caller's stream"
                _same(got, ref, (name, stream))
            finally:
                ix.close()
        if side is not None:
            km.lib.check(km.lib.load().kmcf_comm_set_caller_stream(comm.handle, None), "kmcf_comm_set_caller_stream")
