"""GPU: kmcf_field_sample and kmcf_field_grid (csrc/kmcf_fieldsample.hip) against the restatement of
tests/field_sample_ref.py.  On every case: count, nearest, nearest_d2 and every integer of the stats equal; with n = count
and eps = 2^-52
    |wsum - fsum|  <= n eps sum(w)            |acc_f - fsum| <= n eps sum(w |v_f|)
    |mean - exact| <= (2 n + 4) eps sum(w |v_f|) / sum(w)
(derived: the first-order bound of a sum of n terms in any order, times two; the terms are the same bits on both sides);
on the exact lattice case every output, doubles included, np.array_equal.  Outputs are prefilled with junk on the device; a
second call on reused scratch, a call with stats = NULL and calls with any one output NULL return the same bytes.  The
largest fraction of a bound that was met is printed per test (DESIGN.md 3.17 records it).
tests/test_field_sample_ref.py shows that the inputs are what their names say.

Every test builds and frees its own communicator."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import field_sample_ref as R
import pair_corr_ref as PC
import pbc_ref as P
import site_gap_pbc_ref as GP
from test_gpu_site_gap_pbc import _comm, _Device
from test_gpu_stream_order import _Filler

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JUNK_I, JUNK_F = -77, -123.5
OUTPUTS = ("out", "wsum", "count", "nearest", "nearest_d2")
EPS = R.EPS


class _Index:
    """a spatial index over a case's sites with the case's cutoff: periodic with the case's lattice, or open"""

    def __init__(self, km, comm, c, periodic=True):
        import torch
        self.km, self.c, self.torch = km, c, torch
        self.f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        self.i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (self.f64(c["xyz"][:, k]) for k in range(3))
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

    def call(self, pts, values, mask, radius, normalize, fill=R.FILL, stats=True, skip=(), grid=None):
        """the C entry itself (grid = (origin, spacing, dims): kmcf_field_grid): dict of numpy arrays (None where the output
        was passed as NULL) and stats (dict or None).  pts, values and mask may be device tensors"""
        km, p, torch = self.km, self.km.solvers._ptr, self.torch
        dev = lambda a, conv: a if a is None or torch.is_tensor(a) else conv(a)
        values, mask = dev(values, self.f64), dev(mask, self.i32)
        nf = 0 if values is None else int(values.shape[0])
        n = int(np.prod(grid[2])) if grid is not None else (int(pts.shape[1]) if torch.is_tensor(pts) else len(pts))
        o = dict(out=torch.full((nf, n), JUNK_F, dtype=torch.float64, device="cuda") if nf else None,
                 wsum=torch.full((n,), JUNK_F, dtype=torch.float64, device="cuda"),
                 count=torch.full((n,), JUNK_I, dtype=torch.int32, device="cuda"),
                 nearest=torch.full((n,), JUNK_I, dtype=torch.int32, device="cuda"),
                 nearest_d2=torch.full((n,), JUNK_F, dtype=torch.float64, device="cuda"))
        for k in skip:
            o[k] = None
        st = km.lib.SampleStats()
        tail = (float(radius), int(normalize), float(fill), p(o["out"]), p(o["wsum"]), p(o["count"]), p(o["nearest"]),
                p(o["nearest_d2"]), C.byref(st) if stats else None)
        head = (self.handle, p(self.x), p(self.y), p(self.z), p(mask), nf, p(values))
        lib = km.lib.load()
        if grid is not None:
            og, hg, dg = (np.ascontiguousarray(grid[0], np.float64), np.ascontiguousarray(grid[1], np.float64),
                          np.ascontiguousarray(grid[2], np.int32))
            rc = lib.kmcf_field_grid(*head, og.ctypes.data_as(C.POINTER(C.c_double)), hg.ctypes.data_as(C.POINTER(C.c_double)),
                                     dg.ctypes.data_as(C.POINTER(C.c_int)), *tail)
            km.lib.check(rc, "kmcf_field_grid")
        else:
            if torch.is_tensor(pts):
                px, py, pz = pts
            else:
                px, py, pz = (self.f64(np.asarray(pts, np.float64).reshape(-1, 3)[:, k]) for k in range(3))
            nz = (lambda t: p(t)) if n else (lambda t: None)
            rc = lib.kmcf_field_sample(*head, n, nz(px), nz(py), nz(pz), *tail)
            km.lib.check(rc, "kmcf_field_sample")
        got = {k: (v.cpu().numpy() if v is not None else None) for k, v in o.items()}
        got["stats"] = st.as_dict() if stats else None
        return got

    def variant(self, name, **kw):
        pts, values, mask, radius, normalize = R.variant(name, **kw)
        return dict(pts=pts, values=values, mask=mask, radius=radius, normalize=normalize)

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


def _ints(st):
    return {k: st[k] for k in R.STAT_KEYS}


def _bytes(r, keys=OUTPUTS):
    return tuple(None if r[k] is None else r[k].tobytes() for k in keys)


_WORST = {"wsum": 0.0, "acc": 0.0, "mean": 0.0}


def _check(got, ref, normalize, what="", exact=False):
    """the integers equal, the doubles within the derived bounds (exact: equal); returns nothing, notes the fractions"""
    for k in ("count", "nearest"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], ref[k]), (what, k, np.flatnonzero(got[k] != ref[k])[:8])
    assert np.array_equal(got["nearest_d2"], ref["nearest_d2"]), (what, "nearest_d2")
    if got["stats"] is not None:
        assert _ints(got["stats"]) == ref["stats"], (what, got["stats"], ref["stats"])
    nf = 0 if got["out"] is None else len(got["out"])
    assert nf == len(ref["acc"])
    if exact:
        assert np.array_equal(got["wsum"], ref["wsum"]), (what, "wsum")
        if nf:
            assert np.array_equal(got["out"], ref["out"]), (what, "out", np.argwhere(got["out"] != ref["out"])[:8])
        return
    n = ref["count"].astype(np.float64)
    bound = n * EPS * ref["wsum_fsum"]
    err = np.abs(got["wsum"] - ref["wsum_fsum"])
    assert (err <= bound).all(), (what, "wsum", float((err - bound).max()))
    assert np.array_equal(got["wsum"] == 0.0, ref["wsum"] == 0.0)
    pos = bound > 0
    if pos.any():
        _WORST["wsum"] = max(_WORST["wsum"], float((err[pos] / bound[pos]).max()))
    if not nf:
        return
    ok = ref["wsum"] > 0.0
    if normalize:
        assert (got["out"][:, ~ok] == R.FILL).all(), (what, "fill")
        exact_mean = ref["acc_fsum"][:, ok] / ref["wsum_fsum"][ok]
        bound = (2.0 * n[ok] + 4.0) * EPS * ref["wabs"][:, ok] / ref["wsum_fsum"][ok]
        err, key = np.abs(got["out"][:, ok] - exact_mean), "mean"
    else:
        bound = n[None, :] * EPS * ref["wabs"]
        err, key = np.abs(got["out"] - ref["acc_fsum"]), "acc"
    assert (err <= bound).all(), (what, key, np.argwhere(err > bound)[:8])
    pos = bound > 0
    if pos.any():
        _WORST[key] = max(_WORST[key], float((err[pos] / bound[pos]).max()))


def _report(what):
    print("%s: largest fraction of the bounds so far: wsum %.3f, acc %.3f, mean %.3f" % (what, _WORST["wsum"], _WORST["acc"], _WORST["mean"]))


@pytest.mark.parametrize("name", R.CASES)
def test_cases_match_the_restatement(km, name):
    """every case on a periodic and on an open index over the same coordinates, 3 fields, normalised; a second call, a call
    without stats and calls with one output NULL each: the same bytes; a radius above the cutoff is refused"""
    c = R.case(name)
    exact = name == "lattice"
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False):
            ref = R.reference(name, periodic)
            ix = _Index(km, comm, c, periodic)
            try:
                v = ix.variant(name)
                got = ix.call(**v)
                st = got["stats"]
                print("%s, %s index: %d points, %d empty, %d visits, %d members, max count %d at %d, %.3f ms" % (
                    name, "periodic" if periodic else "open", st["n_points"], st["n_empty"], st["n_visits"], st["n_members"],
                    st["max_count"], st["max_count_point"], st["ms"]))
                _check(got, ref, 1, (name, periodic), exact)
                again = ix.call(**v)                                     # scratch reused: the same bytes
                assert _bytes(again) == _bytes(got) and _ints(again["stats"]) == _ints(got["stats"])
                assert _bytes(ix.call(stats=False, **v)) == _bytes(got)
                for k in OUTPUTS[1:]:
                    rest = tuple(o for o in OUTPUTS if o != k)
                    bare = ix.call(skip=(k,), **v)
                    assert bare[k] is None and _bytes(bare, rest) == _bytes(got, rest) and _ints(bare["stats"]) == _ints(got["stats"])
                raw = ix.call(**dict(v, normalize=0))
                _check(raw, R.reference(name, periodic, normalize=0), 0, (name, periodic, "raw"), exact)
                with pytest.raises(km.lib.KmcfError, match="radius.*cutoff"):
                    ix.call(**dict(v, radius=float(np.nextafter(c["cutoff"], np.inf))))
            finally:
                ix.close()
    _report(name)


@pytest.mark.parametrize("periodic", [True, False])
def test_lattice_with_eight_fields_is_exact(km, periodic):
    c = R.case("lattice")
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c, periodic)
        try:
            for normalize in (1, 0):
                got = ix.call(**ix.variant("lattice", n_fields=8, normalize=normalize))
                _check(got, R.reference("lattice", periodic, n_fields=8, normalize=normalize), normalize, ("lattice", periodic), exact=True)
        finally:
            ix.close()


@pytest.mark.parametrize("n_points", R.N_POINTS)
def test_group_edges_in_the_points(km, n_points):
    c = R.case("r23")
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False):
            ix = _Index(km, comm, c, periodic)
            try:
                got = ix.call(**ix.variant("r23", n_points=n_points))
                _check(got, R.reference("r23", periodic, n_points=n_points), 1, ("r23", periodic, n_points))
                if n_points == 0:
                    assert got["stats"]["ms"] == 0.0
            finally:
                ix.close()


@pytest.mark.parametrize("n_fields", R.FIELD_COUNTS)
@pytest.mark.parametrize("normalize", [1, 0])
def test_field_counts_and_normalisation(km, n_fields, normalize):
    """every bucket of the walk kernel (0, 1, 2, 4, 8 accumulators) and both sides of each edge"""
    c = R.case("r32")
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False):
            ix = _Index(km, comm, c, periodic)
            try:
                got = ix.call(**ix.variant("r32", n_fields=n_fields, normalize=normalize))
                assert (got["out"] is None) == (n_fields == 0)
                _check(got, R.reference("r32", periodic, n_fields=n_fields, normalize=normalize), normalize, ("r32", periodic, n_fields))
            finally:
                ix.close()
    _report("fields %d" % n_fields)


@pytest.mark.parametrize("name", ["r14", "r44"])
def test_masks_and_small_radius(km, name):
    c = R.case(name)
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False):
            ix = _Index(km, comm, c, periodic)
            try:
                res = {}
                for mask in ("none", "ones", "null"):
                    res[mask] = ix.call(**ix.variant(name, mask=mask))
                    _check(res[mask], R.reference(name, periodic, mask=mask), 1, (name, periodic, mask))
                none = res["none"]
                assert not none["count"].any() and (none["nearest"] == -1).all() and (none["out"] == R.FILL).all()
                assert np.isinf(none["nearest_d2"]).all() and not none["wsum"].any() and none["stats"]["n_members"] == 0
                assert _bytes(res["ones"]) == _bytes(res["null"]) and _ints(res["ones"]["stats"]) == _ints(res["null"]["stats"])
                small = ix.call(**ix.variant(name, radius=R.SMALL_RADIUS))
                _check(small, R.reference(name, periodic, radius=R.SMALL_RADIUS), 1, (name, periodic, "small radius"))
                assert small["stats"]["n_empty"] > small["stats"]["n_points"] // 2
            finally:
                ix.close()


GRID = ((-2.3, -1.7, 0.1), (4.3, 0.9, 1.1), (9, 11, 13))


@pytest.mark.parametrize("periodic", [True, False])
def test_grid_returns_the_bytes_of_the_sample_on_its_points(km, periodic):
    c = R.case("r23")
    pts = R.grid_points(*GRID)
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c, periodic)
        try:
            v = ix.variant("r23", n_fields=5)
            sample = ix.call(**dict(v, pts=pts))
            grid = ix.call(**dict(v, pts=None), grid=GRID)
            assert _bytes(grid) == _bytes(sample) and _ints(grid["stats"]) == _ints(sample["stats"])
            ref = R.field_sample(c["xyz"], pts, v["values"], v["mask"], v["radius"], 1, R.FILL, c["L"] if periodic else None)
            _check(grid, ref, 1, ("grid", periodic))
            assert ref["stats"]["n_visits"] > 0 and ref["stats"]["n_empty"] > 0
        finally:
            ix.close()


def test_nan_propagates_only_where_reached(km):
    c = R.case("r23")
    site = int(np.flatnonzero(c["mask"])[5])
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c, True)
        try:
            ref = R.reference("r23", True, nan_site=site)
            clean = R.reference("r23", True)
            got = ix.call(**ix.variant("r23", nan_site=site))
            hit = np.isnan(ref["out"][0])
            assert 0 < hit.sum() < len(hit) and not np.isnan(ref["out"][1:]).any()
            assert np.array_equal(np.isnan(got["out"][0]), hit) and not np.isnan(got["out"][1:]).any()
            assert np.array_equal(got["count"], clean["count"]) and np.array_equal(got["nearest"], clean["nearest"])
            base = ix.call(**ix.variant("r23"))
            assert np.array_equal(got["out"][0][~hit], base["out"][0][~hit]) and np.array_equal(got["out"][1:], base["out"][1:])
            assert np.array_equal(got["wsum"], base["wsum"])
        finally:
            ix.close()


def test_point_errors_carry_their_message(km):
    c = R.case("r23")
    with _comm(km, len(c["xyz"])) as comm:
        for periodic in (True, False):
            ix = _Index(km, comm, c, periodic)
            try:
                v = ix.variant("r23", n_points=40)
                for bad in (np.nan, np.inf, -np.inf):
                    pts = np.array(v["pts"])
                    pts[17, 2] = bad
                    pts[5, 0] = bad
                    with pytest.raises(km.lib.KmcfError, match=r"kmcf_field_sample: point 5 has a coordinate that is not finite"):
                        ix.call(**dict(v, pts=pts))
                pts = np.array(v["pts"])
                pts[3, 1] = 1001.0 * c["L"][1]
                pts[9, 2] = -1001.0 * c["L"][2]
                if periodic:
                    with pytest.raises(km.lib.KmcfError, match=r"kmcf_field_sample: point 3 lies further than 1000 periods"):
                        ix.call(**dict(v, pts=pts))
                else:
                    far = ix.call(**dict(v, pts=pts))
                    assert far["count"][3] == 0 and far["count"][9] == 0
                pts[3, 1], pts[9, 2] = 999.0 * c["L"][1], -999.0 * c["L"][2]         # inside the limit: served
                ref = R.field_sample(c["xyz"], pts, v["values"], v["mask"], v["radius"], 1, R.FILL, c["L"] if periodic else None)
                _check(ix.call(**dict(v, pts=pts)), ref, 1, ("999 periods", periodic))
                _check(ix.call(**v), R.reference("r23", periodic, n_points=40), 1, ("after the errors", periodic))
            finally:
                ix.close()


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------

def _buffers(km, comm, c, periodic):
    S = km.solvers
    xyz, N = c["xyz"], len(c["xyz"])
    buf = S.GPUBuffers(N, np.zeros(N, np.int32), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]), 1, 1.0, 1.0,
                       np.array(c["L"]) if periodic else [1.0, 1.0, 1.0], np.array([6], np.int32))
    S.compute_cutoff_list(comm, buf, c["cutoff"], pbc=1 if periodic else 0)
    return buf


@pytest.mark.parametrize("periodic", [True, False])
def test_python_wrappers(km, periodic):
    c = R.case("r32")
    S = km.solvers
    L = c["L"] if periodic else None
    with _comm(km, len(c["xyz"])) as comm:
        buf = _buffers(km, comm, c, periodic)
        try:
            host = lambda r: dict({k: (None if r[k] is None else r[k].cpu().numpy().reshape(-1) if k != "out" else
                                       r[k].cpu().numpy().reshape(len(r[k]), -1)) for k in OUTPUTS}, stats=r["stats"])
            got = S.field_sample(buf, c["points"], c["values"][:3], mask=c["mask"], fill=R.FILL)      # radius: the cutoff
            assert got["radius"] == c["cutoff"] and got["out"].shape == (3, len(c["points"]))
            _check(host(got), R.reference("r32", periodic), 1, "field_sample")
            raw = S.field_sample(buf, c["points"], c["values"][2], mask=None, radius=4.0, normalize=False)
            ref = R.field_sample(c["xyz"], c["points"], c["values"][2:3], None, 4.0, 0, L=L)
            _check(host(raw), ref, 0, "field_sample raw")
            assert np.array_equal(S.sample_density(raw).cpu().numpy(), R.sample_density(raw["out"].cpu().numpy(), 4.0))
            bare = S.field_sample(buf, c["points"])
            assert bare["out"] is None and np.array_equal(bare["count"].cpu().numpy(), R.reference("r32", periodic, mask="null")["count"])
            assert S.field_sample(buf, np.zeros((0, 3)), c["values"][:2])["stats"]["n_points"] == 0
            assert np.isnan(S.field_sample(buf, [[500.0, 0.0, 0.0]], c["values"][:1])["out"].cpu().numpy()).all()   # fill: nan
            # the grid, with labels
            labels = (np.arange(len(c["xyz"])) % 7).astype(np.int32)
            g = S.field_grid(buf, GRID[0], GRID[1], GRID[2], c["values"][:2], mask=c["mask"], fill=R.FILL, labels=labels)
            ref = R.field_sample(c["xyz"], R.grid_points(*GRID), c["values"][:2], c["mask"], c["cutoff"], 1, R.FILL, L)
            assert g["out"].shape == (2,) + GRID[2] and g["count"].shape == GRID[2] and g["dims"] == GRID[2]
            _check(host(g), ref, 1, "field_grid")
            want = np.where(ref["nearest"] >= 0, labels[np.maximum(ref["nearest"], 0)], -1).reshape(GRID[2])
            assert np.array_equal(g["labels"].cpu().numpy(), want) and (want == -1).any() and (want >= 0).any()
            # a slice: one voxel thick, across the sites' bounding box
            s = S.field_slice(buf, "x", 2.5, 1.5, values=c["values"][:1], fill=R.FILL)
            lo, hi = c["xyz"].min(0), c["xyz"].max(0)
            dims = (1, int(np.floor((hi[1] - lo[1]) / 1.5)) + 1, int(np.floor((hi[2] - lo[2]) / 1.5)) + 1)
            assert s["dims"] == dims
            ref = R.field_sample(c["xyz"], R.grid_points((2.5, lo[1], lo[2]), (1.5, 1.5, 1.5), dims), c["values"][:1], None, c["cutoff"],
                                 1, R.FILL, L)
            _check(host(s), ref, 1, "field_slice")
            # an index whose cutoff radius the buffers do not know: the default radius is refused in words, a given one served
            buf.cutoff_radius = None
            with pytest.raises(AssertionError, match="cutoff radius"):
                S.field_sample(buf, c["points"])
            again = S.field_sample(buf, c["points"], radius=c["cutoff"])
            assert np.array_equal(again["count"].cpu().numpy(), bare["count"].cpu().numpy())
        finally:
            buf.freeGPUmemory()


def test_pairwise_term_gap_and_pair_correlation_are_not_disturbed(km, dev5):
    import torch
    S = km.solvers
    c, s, pc = P.pairwise_case("p34"), GP.case("p34@20"), PC.case("p34#0")
    N = c["N"]
    rng = np.random.default_rng(78)
    element = rng.choice([P.O_EL, P.VACANCY, P.OXYGEN_DEFECT, 9], N, p=[0.4, 0.4, 0.1, 0.1]).astype(np.int32)
    with _comm(km, N) as comm:
        dv = _Device(km, comm, c["xyz"], element, c["L"], np.array([9], np.int32), 3.5, P.NN, 1, dev5["sigma"], dev5["k"])
        try:
            buf = dv.buf
            buf.site_charge.copy_(torch.as_tensor(np.array(c["charge"]), device="cuda"))
            side = torch.as_tensor(np.array(s["side"]), device="cuda")
            cls = torch.as_tensor(np.array(pc["cls"]), device="cuda")

            def snapshot():
                S.poisson_gridless_gpu(buf, comm)
                r = S.site_set_gap(buf, side, 20.0, site_cell=s["cell"], n_cells=s["n_cells"], periodic=True)
                ints = {k: v for k, v in r["stats"].items() if not k.startswith("ms")}
                q = S.pair_correlation(buf, cls, 3, pc["r_max"], pc["n_bins"], r_count=pc["r_count"], site_cell=pc["cell"],
                                       n_cells=pc["n_cells"], counts=True)
                return (buf.site_potential_charge.cpu().numpy().tobytes(), r["gaps"].tobytes(), ints, q["hist"].tobytes(),
                        q["members"].tobytes(), q["counts"].cpu().numpy().tobytes())

            before = snapshot()
            assert np.frombuffer(before[0], np.float64).any()
            pts = rng.random((300, 3)) * np.array(c["L"]) * 1.5 - 5.0
            values = rng.standard_normal((3, N))
            got = S.field_sample(buf, pts, values, mask=(element == P.VACANCY), radius=9.0, fill=R.FILL)
            ref = R.field_sample(c["xyz"], pts, values, element == P.VACANCY, 9.0, 1, R.FILL, c["L"])
            host = dict({k: got[k].cpu().numpy() for k in OUTPUTS}, stats=got["stats"])
            _check(host, ref, 1, "p34")
            S.field_grid(buf, (0.0, 0.0, 0.0), 4.0, (8, 8, 8), values)
            assert snapshot() == before
        finally:
            dv.close()


def test_kmc_loop_with_the_field_grid(tmp_path):
    out_file = str(tmp_path / "grid.npz")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kmc_loop.py"), "--workload", "5nm", "--steps", "1",
                          "--field-grid", "2.0", "--field-grid-radius", "6", "--field-grid-out", out_file],
                         capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    pat = r"field grid cell 0: \d+ x \d+ x \d+ voxels of 2 A, radius 6 A \| \d+ visits, \d+ empty \| potential .* V \| densest voxel .* \| [\d.]+ ms"
    assert len([l for l in lines if re.search(pat, l)]) == 1, lines
    z = np.load(out_file)
    assert z["potential"].ndim == 3 and z["potential"].shape == z["element"].shape == z["vacancy_density"].shape
    assert (z["vacancy_density"] >= 0).all() and z["element"].max() > 0


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
@pytest.mark.parametrize("decoy", ["values", "points", "mask"])
def test_call_waits_for_the_callers_stream(km, filler, stream, decoy):
    """A decoy (value rows of zeros, points far out, a mask of zeros) sits on the device; the true array is copied over it
    behind the filler on the caller's stream; stream.query() is False before and True after the call; the outputs are the
    synchronised reference's."""
    import contextlib
    import torch
    name = "r23"
    c, ref = R.case(name), R.reference(name)
    assert ref["stats"]["n_visits"] > 0
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
                v = ix.variant(name)
                true = dict(values=ix.f64(v["values"]), mask=ix.i32(v["mask"]),
                            points=torch.stack([ix.f64(v["pts"][:, k]) for k in range(3)]).contiguous())
                live = {k: t.clone() for k, t in true.items()}
                if decoy == "points":
                    live["points"].fill_(1e4)
                else:
                    live[decoy].zero_()
                args = dict(v, values=live["values"], mask=live["mask"], pts=live["points"])
                torch.cuda.synchronize()
                first = ix.call(**args)                          # the decoy's own answer (and the scratch is allocated)
                assert first["stats"]["n_visits"] == 0 if decoy != "values" else not first["out"][:, ref["wsum"] > 0].any()
                torch.cuda.synchronize()
                filler.queue()
                live[decoy].copy_(true[decoy], non_blocking=True)
                marker = torch.cuda.Event()
                marker.record(st)
                busy = st.query()
                got = ix.call(**args)
                reached, done = marker.query(), st.query()
                assert busy is False, "the caller's stream was idle at the call: the filler is too short"
                assert reached is True, "the call returned before the work queued on the caller's stream had finished"
                assert done is True, "the call returned with work pending on the caller's stream"
                _check(got, ref, 1, (name, stream, decoy))
            finally:
                ix.close()
        if side is not None:
            km.lib.check(km.lib.load().kmcf_comm_set_caller_stream(comm.handle, None), "kmcf_comm_set_caller_stream")
