"""GPU: every compute entry point keeps the stream ordering contract of include/kmcfield.h -- its work is ordered behind
everything the caller has queued on the caller's stream (torch's default stream, or the one declared with
kmcf_comm_set_caller_stream), and it returns with its streams synchronised.

Protocol, the same for every entry point (inputs: tests/stream_order_cases.py; tests/test_stream_order_cases.py holds the
decoys to their safety rules on the CPU):

  reference   on a fresh state the true inputs are uploaded, torch.cuda.synchronize(), the call, every output kept as
              bytes; once more with the decoy inputs.  The two references must differ in at least one output, or the
              case could not tell a library that waited from one that did not, and fails.
  staged call on another fresh state the decoys are put in the device arrays and synchronised; on the caller's stream a
              filler of FILLER_COUNT small kernels on a scratch tensor is queued and, behind it, the device-to-device
              copies that overwrite the decoys with the true values; stream.query() is False; the call; stream.query()
              is True; the outputs are read on the caller's stream, with no torch.cuda.synchronize().  Every output
              equals the true reference bit for bit, and no call returns an error.

Every case runs twice: on torch's default stream with no caller stream declared, and inside torch.cuda.stream(side) with
side = torch.cuda.Stream() -- torch creates it non-blocking, so nothing the null stream does waits for it -- declared on
every communicator of the case.

The filler: FILLER_COUNT launches of `scratch += c` on FILLER_ELEMS doubles.  Measured once per module with torch
events, as a synchronised run of its own, printed, and held to at least 10 ms; the query() assertions around every call
are what keep a too-short filler from passing silently.  On the MI355X: 33.3 ms on the device, 7.5 ms to launch (with
2 097 152 doubles: 9.3 ms and 6.3 ms -- the queue drained nearly as fast as it was filled, so the vector grew, not the count).

Besides stream.query(), an event recorded at the end of the caller's queue right before the call has completed when the
call returns: that is "the call returned only after the work ordered behind the caller's queue" without the library's
own use of the stream.  Both are asserted, on both streams.  (stream.query() on torch's default stream -- the legacy null
stream -- also sees what the LIBRARY puts there: a hipMemset of a new buffer used to stay there past the return of
kmcf_background_potential_sparse, kmcf_initialize_sparsity_T and a first kmcf_current_profile)

Also here: KMCF_ENTER_ALWAYS (set with kmcf_set_option) gives the reference bytes with an idle and with a busy caller
stream; after kmcf_comm_set_caller_stream(c, side) and then (c, None) the default stream is the caller's again; and a
group of two in-process ranks, each with a side stream of its own, on the loopback and on the peer-to-peer transport."""
import contextlib
import ctypes as C
import threading
import time

import numpy as np
import pytest

import stream_order_cases as SO

pytestmark = pytest.mark.gpu

FILLER_ELEMS = 1 << 23
FILLER_COUNT = 1500
FILLER_MIN_MS = 10.0
SENTINEL = 123.0


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class _Filler:
    def __init__(self, torch):
        self.scratch = torch.zeros(FILLER_ELEMS, dtype=torch.float64, device="cuda")
        self.queue()                                        # (warm-up: the kernel is loaded)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        self.queue()
        e1.record()
        self.launch_ms = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        self.ms = e0.elapsed_time(e1)

    def queue(self):
        """FILLER_COUNT small kernels on torch's current stream; touches nothing but the scratch tensor"""
        for _ in range(FILLER_COUNT):
            self.scratch.add_(1e-3)


@pytest.fixture(scope="module")
def filler(torch):
    f = _Filler(torch)
    print("filler: %d launches on %d doubles take %.1f ms on the device (%.1f ms to launch)" % (FILLER_COUNT, FILLER_ELEMS, f.ms, f.launch_ms))
    assert f.ms >= FILLER_MIN_MS, "the filler lasts %.2f ms: raise FILLER_COUNT" % f.ms
    return f


# ------------------------------------------------------------------------------------------------ plumbing
class _Ctx:
    """what a state is built with: the package, torch, and the caller stream to declare on every communicator"""

    def __init__(self, km, torch, side=None, options=None):
        self.km, self.torch, self.S, self.lib, self.side, self.options = km, torch, km.solvers, km.lib.load(), side, options

    def declare(self, comm, stream):
        self.km.lib.check(self.lib.kmcf_comm_set_caller_stream(comm.handle, None if stream is None else stream.cuda_stream),
                          "kmcf_comm_set_caller_stream")

    def comm(self, *rows):
        c = self.S.KMC_comm(*rows, options=self.options)
        c.connect()
        if self.side is not None:
            self.declare(c, self.side)
        return c

    def f64(self, a):
        return self.torch.as_tensor(np.array(a, dtype=np.float64), device="cuda")

    def i32(self, a):
        return self.torch.as_tensor(np.array(a, dtype=np.int32), device="cuda")


def _xyz(x, y, z):
    return [(x, 0), (y, 1), (z, 2)]


def _part(a, col, like):
    a = a if col is None else a[:, col]
    return np.ascontiguousarray(a).reshape(tuple(like.shape))


def _norm(v):
    """an output as bytes (dicts and sequences element by element; timings are no output)"""
    if isinstance(v, dict):
        return tuple((k, _norm(x)) for k, x in sorted(v.items()) if not k.startswith("ms"))
    if isinstance(v, (list, tuple)):
        return tuple(_norm(x) for x in v)
    if hasattr(v, "cpu") and hasattr(v, "numpy"):
        v = v.cpu().numpy()
    if v is None:
        return b"none"
    a = np.ascontiguousarray(v)
    return (a.dtype.str, a.shape, a.tobytes())


class _State:
    """One fresh state of a case.  stage: {key of the case's arrays: [(device tensor, column of the host array or None)]};
    call(): the library call(s) under test, nothing else; read(): every output (device tensors are read with .cpu(), on
    torch's current stream); close()."""

    def __init__(self, ctx, c):
        self.ctx, self.c, self.h = ctx, c, c["host"]
        self.comms, self.stage, self.closers = [], {}, []

    def comm(self, *rows):
        c = self.ctx.comm(*rows)
        self.comms.append(c)
        return c

    def close(self):
        for f in self.closers[::-1]:
            f()
        for c in self.comms:
            c.close()


def _load(ctx, st, which):
    torch = ctx.torch
    for key, s in st.c["arrays"].items():
        for t, col in st.stage[key]:
            t.copy_(torch.as_tensor(_part(getattr(s, which), col, t).copy()))
    torch.cuda.synchronize()


@contextlib.contextmanager
def _on(torch, side):
    if side is None:
        yield torch.cuda.current_stream()
    else:
        with torch.cuda.stream(side):
            yield side


def _reference(make, ctx, c, which):
    st = make(ctx, c)
    try:
        _load(ctx, st, which)
        st.call()
        return _norm(st.read())
    finally:
        st.close()


def _staged(make, ctx, c, filler):
    torch = ctx.torch
    with _on(torch, ctx.side) as stream:
        st = make(ctx, c)
        try:
            _load(ctx, st, "decoy")
            src = [(t, torch.as_tensor(_part(s.true, col, t).copy(), device="cuda")) for key, s in c["arrays"].items() for t, col in st.stage[key]]
            torch.cuda.synchronize()
            filler.queue()
            for t, s in src:
                t.copy_(s, non_blocking=True)
            marker = torch.cuda.Event()
            marker.record(stream)                            # the end of the caller's queue as it stands at the call
            busy = stream.query()
            st.call()
            reached, done = marker.query(), stream.query()
            assert busy is False, "the caller's stream was idle at the call: the filler is too short"
            assert reached is True, "the call returned before the work queued on the caller's stream had finished"
            assert done is True, "the call returned with work pending on the caller's stream"
            return _norm(st.read())                          # (no torch.cuda.synchronize(): read on the caller's stream)
        finally:
            st.close()


_SIDE = []


def _side(torch, k=0):
    """The declared streams of this file: one for the one-rank cases, one more per rank of the group.  torch hands out a
    different stream of its pool at every torch.cuda.Stream(); each one that has carried work keeps a hardware queue, and
    the in-process groups of the suite need their streams' queues to themselves (tests/conftest.py)."""
    while len(_SIDE) <= k:
        _SIDE.append(torch.cuda.Stream())
    return _SIDE[k]


def _differing(a, b):
    return [k for (k, x), (_, y) in zip(a, b) if x != y]


_REFS = {}


def _references(make, km, torch, c, key=None):
    """(true, decoy) reference outputs of a case, computed once per module and never modified"""
    key = key or c["name"]
    if key not in _REFS:
        ctx = _Ctx(km, torch)
        true, decoy = _reference(make, ctx, c, "true"), _reference(make, ctx, c, "decoy")
        assert _differing(true, decoy), "%s: the decoy inputs give the true inputs' outputs: the case proves nothing" % key
        _REFS[key] = (true, decoy)
    return _REFS[key]


def _run_case(make, km, torch, filler, c, side, options=None, key=None):
    true, decoy = _references(make, km, torch, c, key)
    stream = _side(torch) if side else None
    got = _staged(make, _Ctx(km, torch, stream, options), c, filler)
    bad, told = _differing(got, true), _differing(true, decoy)
    print("%s on %s: %d outputs, %s differ from the true reference; the decoy reference differs in %s"
          % (key or c["name"], "a declared side stream" if side else "torch's default stream", len(true), bad or "none", told))
    assert not bad, "%s: %s differ from the synchronised reference (%s the decoy's)" % (
        c["name"], bad, "equal to" if got == decoy else "not")


# ------------------------------------------------------------------------------------------------ plain vectors
class _Vec(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, S, torch = self.h, ctx.S, ctx.torch
        n = h["n"]
        self.comm_ = self.comm(n, n, n, n)
        self.mat = S.Distributed_matrix(self.comm_, n, [n], [0], h["col"], h["row_ptr"], h["val"])
        self.closers.append(self.mat.close)
        z = lambda: torch.zeros(n, dtype=torch.float64, device="cuda")
        self.t = dict(p=z(), b=z(), x0=z(), dinv=torch.ones(n, dtype=torch.float64, device="cuda"), a1=z(), a2=z(),
                      idx=torch.arange(n, dtype=torch.int32, device="cuda"), out=torch.full((n,), SENTINEL, dtype=torch.float64, device="cuda"))
        self.stage = {k: [(self.t[k], None)] for k in c["arrays"]}
        self.res = {}
        name = c["name"]
        if name.startswith("pcg_jacobi"):
            plan = self.mat.sum_plan(with_csr=False)
            assert (plan["resident_tpb"] > 0) == name.endswith("resident"), plan      # the path the case is named after
        torch.cuda.synchronize()

    def call(self):
        S, t, n, name = self.ctx.S, self.t, self.h["n"], self.c["name"]
        if name == "spmv":
            self.mat.spmv(t["p"], t["out"])
        elif name.startswith("pcg_jacobi"):
            self.res["stats"] = S.conjugate_gradient_jacobi(self.mat, t["b"], t["x0"], t["dinv"], 1e-10, 500)
        elif name == "solve_sparse_CG_Jacobi":
            self.res["stats"] = S.solve_sparse_CG_Jacobi(self.mat, t["b"], t["x0"], tol=1e-12, max_iterations=500)
        elif name == "pack":
            S.pack_gpu(self.comm_, t["out"], t["a1"], t["idx"], n)
        elif name == "unpack":
            S.unpack_gpu(self.comm_, t["out"], t["a1"], t["idx"], n)
        elif name == "unpack_add":
            S.unpack_add(self.comm_, t["a2"], t["a1"], t["idx"], n)
        elif name == "elementwise_vector_vector":
            S.elementwise_vector_vector(self.comm_, t["a1"], t["a2"], t["out"], n)
        elif name == "matrix_values":
            # host-side values: kmcf_matrix_set_values / _get_values and the replan copy d_val synchronously; the SpMV behind
            # them reads what they left, and the staged vector
            self.mat.set_values(self.h["val2"])
            self.res["values"] = self.mat.get_values().copy()
            self.mat.replan()
            self.mat.spmv(t["p"], t["out"])
        else:
            raise KeyError(name)

    def read(self):
        t = self.t
        return dict(self.res, out=t["out"], x=t["x0"], r=t["b"], a2=t["a2"])


# ------------------------------------------------------------------------------------------------ K path
K_LEVEL = {"neighbor_list": 0, "neighbor_list_pbc": 0, "initialize_sparsity_K": 0, "update_temperature_global": 0, "update_charge": 1,
           "filament_gap": 3, "filament_chain": 3}        # (every other K case: 2, the K state)


class _K(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, S, torch = self.h, ctx.S, ctx.torch
        N, NL = h["N"], h["NL"]
        name = c["name"]
        level = K_LEVEL.get(name, 2)
        self.comm_ = self.comm(h["n"], N + 1, N, N)
        buf = self.buf = S.GPUBuffers(N, np.array(h["element"]), np.array(h["xyz"][:, 0]), np.array(h["xyz"][:, 1]), np.array(h["xyz"][:, 2]),
                                      h["nn"], SO.SIGMA, SO.K_COULOMB, h["lattice"], h["metals"])
        self.closers.append(buf.freeGPUmemory)
        buf.site_charge.copy_(ctx.i32(h["charge"]))
        buf.site_temperature = torch.full((N,), 300.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        if level == 1:
            S.compute_neighbor_list(self.comm_, buf, h["nn_dist_charge"], h["nn"])
        if level == 2:
            S.initialize_sparsity_K(buf, 0, h["nn_dist"], NL, self.comm_)
        if level == 3:
            S.compute_neighbor_list(self.comm_, buf, h["nn_dist"], 52)
            S.compute_cutoff_list(self.comm_, buf, h["cutoff"])
        where = dict(xyz=_xyz(buf.site_x, buf.site_y, buf.site_z), element=[(buf.site_element, None)], charge=[(buf.site_charge, None)],
                     pot=[(buf.site_potential_boundary, None)], pot_charge=[(buf.site_potential_charge, None)],
                     power=[(buf.site_power, None)], T_old=[(buf.site_temperature, None)], T_bg=[(buf.T_bg, None)])
        if "neigh" in c["arrays"]:
            where["neigh"] = [(buf.neigh_idx, None)]
        self.stage = {k: where[k] for k in c["arrays"]}
        self.res = {}
        torch.cuda.synchronize()

    def call(self):
        S, h, buf, comm, name = self.ctx.S, self.h, self.buf, self.comm_, self.c["name"]
        N, NL, Vd, hi, lo = h["N"], h["NL"], h["Vd"], h["high_G"], h["low_G"]
        if name == "neighbor_list":
            S.compute_neighbor_list(comm, buf, h["nn_dist_charge"], h["nn"])
        elif name == "neighbor_list_pbc":
            S.compute_neighbor_list(comm, buf, h["nn_dist_charge"], h["nn"], pbc=1)
        elif name == "initialize_sparsity_K":
            S.initialize_sparsity_K(buf, 0, h["nn_dist"], NL, comm)
        elif name == "update_charge":
            S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, N, h["nn"], buf.metal_types, buf.num_metal_types_,
                                comm.counts_events, comm.displs_events, comm)
        elif name == "k_assemble":
            S.k_assemble(buf, Vd, hi, lo)
        elif name == "k_assemble_contacts":
            S.k_assemble_contacts(buf, buf.site_potential_boundary, hi, lo)
        elif name == "background_potential_sparse":
            self.res["stats"] = S.background_potential_gpu_sparse(buf, N, NL, NL, Vd, 0, hi, lo, h["nn_dist"], len(h["metals"]))
        elif name == "background_potential_sparse_contacts":
            self.res["stats"] = S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, hi, lo, len(h["metals"]))
        elif name == "update_CB_edge_sparse":
            self.res["stats"] = S.update_CB_edge_gpu_sparse(buf, N, NL, NL, Vd, 0, hi, lo, h["nn_dist"], len(h["metals"]))
        elif name == "sum_and_gather_potential":
            S.sum_and_gather_potential(buf, NL, comm)
        elif name == "update_temperature_global":
            g = h["global_heat"]
            S.update_temperatureglobal_gpu(buf.site_power, buf.T_bg, N, g["a"], g["b"], g["steps"], g["C"], g["small_step"], comm)
        elif name == "update_temperature_local":
            # (the C entry itself: the wrapper fills buf.T_bg behind the call, which is work of the caller's on its stream)
            L, p, prm = self.ctx.km.lib, S._ptr, S.heat_params(**h["heat"])
            st, T_bg, steady = L.SolveStats(), C.c_double(0.0), C.c_int(0)
            L.check(self.ctx.lib.kmcf_update_temperature_local(buf.K_distributed, p(buf.site_element), p(buf.site_charge), p(buf.metal_types),
                                                               buf.num_metal_types_, p(buf.site_power), p(buf.site_temperature), N, NL, NL,
                                                               h["heat_step"], C.byref(prm), C.byref(T_bg), C.byref(steady), C.byref(st)),
                    "kmcf_update_temperature_local")
            self.res["result"] = dict(T_bg=T_bg.value, steady=steady.value, stats=st.as_dict())
        elif name == "filament_gap":
            self.res["gap"] = S.filament_gap(comm, buf, NL, NL, h["r_max"], bins=(8, 0.0, 60.0))
        elif name == "filament_chain":
            self.res["chain"] = S.filament_chain(comm, buf, NL, NL, h["r_max"], max_hops=8)
        else:
            raise KeyError(name)

    def read(self):
        S, buf, name = self.ctx.S, self.buf, self.c["name"]
        out = dict(self.res)
        if name.startswith("neighbor_list"):
            out["neigh_idx"] = buf.neigh_idx
        elif name == "initialize_sparsity_K":
            out["patterns"] = [S.k_pattern(buf, which) for which in range(3)]
        elif name == "update_charge":
            out["charge"] = buf.site_charge
        elif name.startswith("k_assemble"):
            out["system"] = S.k_vectors(buf)                  # (its matrix values: kmcf_matrix_get_values right behind the assembly)
        elif name.startswith("background_potential") or name == "sum_and_gather_potential":
            out.update(boundary=buf.site_potential_boundary, charge_term=buf.site_potential_charge)
        elif name == "update_CB_edge_sparse":
            out["cb"] = buf.site_CB_edge
        elif name == "update_temperature_global":
            out["T_bg"] = buf.T_bg
        elif name == "update_temperature_local":
            out.update(T=buf.site_temperature)
        return out


# ------------------------------------------------------------------------------------------------ pairwise term
class _Pairwise(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, torch = self.h, ctx.torch
        N = h["N"]
        self.comm_ = self.comm(1, 2, N, N)
        self.x, self.y, self.z = (ctx.f64(h["xyz"][:, a]) for a in range(3))
        self.charge = ctx.i32(h["charge"])
        self.pot = torch.full((N,), SENTINEL, dtype=torch.float64, device="cuda")
        self.handle = None
        self.closers.append(lambda: self.handle is not None and ctx.lib.kmcf_pairwise_destroy(self.handle))
        where = dict(xyz=_xyz(self.x, self.y, self.z), charge=[(self.charge, None)])
        self.stage = {k: where[k] for k in c["arrays"]}
        torch.cuda.synchronize()
        if c["name"].startswith("poisson"):
            self.index()

    def index(self):
        ctx, h, p = self.ctx, self.h, self.ctx.S._ptr
        hd = C.c_void_p()
        if h["lattice"] is None:
            ctx.km.lib.check(ctx.lib.kmcf_compute_cutoff_list(self.comm_.handle, p(self.x), p(self.y), p(self.z), h["N"], h["cutoff"], C.byref(hd)),
                             "kmcf_compute_cutoff_list")
        else:
            lat = np.ascontiguousarray(h["lattice"], np.float64)
            ctx.km.lib.check(ctx.lib.kmcf_compute_cutoff_list_pbc(self.comm_.handle, p(self.x), p(self.y), p(self.z), h["N"], h["cutoff"],
                                                                  lat.ctypes.data_as(C.POINTER(C.c_double)), 1, C.byref(hd)),
                             "kmcf_compute_cutoff_list_pbc")
        self.handle = hd

    def poisson(self):
        ctx, h, p = self.ctx, self.h, self.ctx.S._ptr
        ctx.km.lib.check(ctx.lib.kmcf_poisson_gridless(self.handle, p(self.x), p(self.y), p(self.z), p(self.charge), h["sigma"], h["k"],
                                                       h["N"], 0, p(self.pot)), "kmcf_poisson_gridless")

    def call(self):
        if self.c["name"].startswith("poisson"):
            self.poisson()
        else:
            self.index()

    def read(self):
        if not self.c["name"].startswith("poisson"):
            self.poisson()              # what the index is good for: the term it gives on the coordinates now in place
        return dict(potential=self.pot)


# ------------------------------------------------------------------------------------------------ T path
class _T(_State):
    def __init__(self, ctx, c):
        from test_gpu_tpath import G0
        super().__init__(ctx, c)
        h, S, torch = self.h, ctx.S, ctx.torch
        case, N, name = h["case"], h["N"], c["name"]
        p = case["par"]
        self.comm_ = self.comm(h["Nsub"], h["Nsub"], N, N)
        xyz = case["xyz"]
        buf = self.buf = S.GPUBuffers(N, np.array(case["element"]), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]), 52, 3.5e-10, 1.0,
                                      [1, 1, 1], np.array(case["metals"]))
        self.closers.append(buf.freeGPUmemory)
        buf.site_charge.copy_(ctx.i32(case["charge"]))
        buf.site_CB_edge = ctx.f64(case["cb"])
        self.pot = torch.zeros(h["N_atom"] + 2, dtype=torch.float64, device="cuda")
        buf.atom_virtual_potentials = torch.zeros(h["N_atom"] + 2, dtype=torch.float64, device="cuda")     # (or the wrapper allocates it behind the call)
        self.cell = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.prm = S.current_params(h["Vd"], p["high_G"], p["low_G"], p["loop_G"], G0, p["tol"], p["m_e"], p["V0"],
                                    contact_x_lo=case["x_lo"], contact_x_hi=case["x_hi"])
        self.power_args = (case["n1"], case["n1"], case["layers"], h["Vd"], p["high_G"], p["low_G"], p["loop_G"], G0, p["tol"], p["nn_dist"],
                           p["m_e"], p["V0"], 2, True, False, 1.0)
        self.power_kw = dict(cg_tolerance=1e-13, cg_max_iterations=20000, contact_x_lo=case["x_lo"], contact_x_hi=case["x_hi"])
        torch.cuda.synchronize()
        if name != "initialize_sparsity_T":
            self.init()
            assert buf.N_atom_ == h["N_atom"]
        if name in ("current_map", "current_profile"):
            S.t_assemble(buf, self.prm)
        if name == "current_profile":
            # a first call grows the profile's buffers, and a call that allocates waits for more than the contract asks:
            # one synchronised call with the same planes and cells, so that the call under test allocates nothing
            S.current_profile(buf, h["planes"], site_cell=self.cell, n_cells=h["n_cells"], potentials=self.pot, vector=True)
        where = dict(xyz=_xyz(buf.site_x, buf.site_y, buf.site_z), element=[(buf.site_element, None)], charge=[(buf.site_charge, None)],
                     cb=[(buf.site_CB_edge, None)], potentials=[(self.pot, None)], cell=[(self.cell, None)])
        self.stage = {k: where[k] for k in c["arrays"]}
        self.res = {}
        torch.cuda.synchronize()

    def init(self):
        case = self.h["case"]
        self.ctx.S.initialize_sparsity_T(self.buf, 0, case["par"]["nn_dist"], case["n1"], case["n1"], case["layers"], self.comm_)

    def call(self):
        S, buf, name, h = self.ctx.S, self.buf, self.c["name"], self.h
        if name == "initialize_sparsity_T":
            self.init()
        elif name == "t_assemble":
            S.t_assemble(buf, self.prm)
        elif name == "update_power_sparse":
            self.res["imacro"], self.res["stats"] = S.update_power_gpu_sparse_dist(buf, *self.power_args, **self.power_kw)
        elif name == "current_map":
            self.res["map"] = S.current_map(buf, potentials=self.pot)
        elif name == "current_profile":
            self.res["profile"] = S.current_profile(buf, h["planes"], site_cell=self.cell, n_cells=h["n_cells"], potentials=self.pot, vector=True)
        else:
            raise KeyError(name)

    def read(self):
        S, buf, name = self.ctx.S, self.buf, self.c["name"]
        out = dict(self.res)
        if name == "initialize_sparsity_T":
            out.update(pattern=S.t_pattern(buf), atoms=S.t_atom_sites(buf), info=S.t_info(buf))
        elif name == "t_assemble":
            out.update(vectors=S.t_vectors(buf), tunnel=S.t_tunnel(buf), info=S.t_info(buf))
        elif name == "update_power_sparse":
            out.update(potentials=buf.atom_virtual_potentials, power=buf.site_power)
        return out


# ------------------------------------------------------------------------------------------------ events
class _Events(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, torch = self.h, ctx.torch
        N = h["N"]
        self.comm_ = self.comm(max(N - 2, 1), N + 1, N, N)
        self.neigh, self.lay = ctx.i32(h["neigh"].reshape(-1)), ctx.i32(h["lay"])
        self.x, self.y, self.z = (ctx.f64(h["xyz"][:, q]) for q in range(3))
        self.el, self.ch, self.pot = ctx.i32(h["element"]), ctx.i32(h["charge"]), ctx.f64(h["pot"])
        self.temp = torch.full((N,), 300.0, dtype=torch.float64, device="cuda")
        self.rng = ctx.S.RandomNumberGenerator(h["seed"])      # the same seed in every run
        where = dict(element=[(self.el, None)], charge=[(self.ch, None)], pot=[(self.pot, None)], temperature=[(self.temp, None)])
        self.stage = {k: where[k] for k in c["arrays"]}
        self.res = {}
        torch.cuda.synchronize()

    def call(self):
        S, h, m, name = self.ctx.S, self.h, self.comm_, self.c["name"]
        args = (m, h["N"], m.counts_events, m.displs_events, h["nn"], self.neigh, self.lay, h["T_bg"], h["freq"], h["sigma"], h["k"],
                self.x, self.y, self.z, self.pot, self.el, self.ch)
        if name == "event_rates":
            self.res["type"], self.res["rate"] = S.event_rates(*args, h["layers"], site_temperature=self.temp, rate_mode="site")
        elif name == "execute_kmc_step":
            self.res["time"], self.res["events"], self.res["log"] = S.execute_kmc_step_mpi(*args, self.rng, h["layers"], max_events=h["max_events"],
                                                                                         return_log=True)
        elif name == "execute_kmc_step_thermal":
            self.res["time"], self.res["events"], self.res["log"] = S.execute_kmc_step_mpi(
                *args, self.rng, h["layers"], max_events=h["max_events"], return_log=True, site_temperature=self.temp, rate_mode="site")
        else:
            raise KeyError(name)

    def read(self):
        return dict(self.res, element=self.el, charge=self.ch)


# ------------------------------------------------------------------------------------------------ analyses
class _Clusters(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, torch = self.h, ctx.torch
        self.comm_ = self.comm(1, 2, 1, 1)
        self.neigh, self.el, self.ch, self.metals = ctx.i32(h["neigh"].reshape(-1)), ctx.i32(h["element"]), ctx.i32(h["charge"]), ctx.i32(h["metals"])
        self.x = ctx.f64(h["x"])
        self.label = torch.full((h["N"],), -7, dtype=torch.int32, device="cuda")
        self.stage = dict(element=[(self.el, None)], charge=[(self.ch, None)], x=[(self.x, None)])
        torch.cuda.synchronize()

    def call(self):
        ctx, h, p = self.ctx, self.h, self.ctx.S._ptr
        self.table = np.zeros(h["N"], ctx.S.CLUSTER_DTYPE)
        st = ctx.km.lib.ClusterStats()
        ctx.km.lib.check(ctx.lib.kmcf_conductive_clusters(self.comm_.handle, h["N"], h["nn"], p(self.neigh), p(self.el), p(self.ch), p(self.metals),
                                                          len(h["metals"]), p(self.x), h["NL"], h["NR"], p(self.label),
                                                          self.table.ctypes.data_as(C.POINTER(ctx.km.lib.Cluster)), h["N"], C.byref(st)),
                         "kmcf_conductive_clusters")
        self.stats = st.as_dict()

    def read(self):
        return dict(label=self.label, table=self.table, stats=self.stats)


class _SiteSet(_State):
    """kmcf_site_set_gap / _chain and their _pbc forms on an index built from the case's coordinates"""

    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, S, torch = self.h, ctx.S, ctx.torch
        N = len(h["xyz"])
        self.comm_ = self.comm(1, 2, N, N)
        xyz = h["xyz"]
        lattice = h["lattice"] if h["periodic"] else [1.0, 1.0, 1.0]
        buf = self.buf = S.GPUBuffers(N, np.zeros(N, np.int32), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]), 1, 1.0, 1.0,
                                      lattice, np.array([6], np.int32))
        self.closers.append(buf.freeGPUmemory)
        torch.cuda.synchronize()
        S.compute_cutoff_list(self.comm_, buf, h["cutoff"], pbc=1 if h["periodic"] else 0)
        self.side = torch.zeros(N, dtype=torch.int32, device="cuda")
        self.node = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        self.cell = torch.zeros(N, dtype=torch.int32, device="cuda") if h["cell"] is not None else None
        where = dict(side=[(self.side, None)], node=[(self.node, None)], cell=[(self.cell, None)])
        self.stage = {k: where[k] for k in c["arrays"]}
        torch.cuda.synchronize()

    def call(self):
        S, h = self.ctx.S, self.h
        if "chain" in self.c["name"]:
            self.res = S.site_set_chain(self.buf, self.side, self.node, h["r_max"], site_cell=self.cell, n_cells=h["n_cells"],
                                        max_hops=h["max_hops"], periodic=h["periodic"])
        else:
            self.res = S.site_set_gap(self.buf, self.side, h["r_max"], site_cell=self.cell, n_cells=h["n_cells"], periodic=h["periodic"])

    def read(self):
        return self.res


class _Gradient(_State):
    def __init__(self, ctx, c):
        super().__init__(ctx, c)
        h, S, torch = self.h, ctx.S, ctx.torch
        N, xyz = h["N"], h["xyz"]
        self.comm_ = self.comm(1, 2, 1, 1)
        buf = self.buf = S.GPUBuffers(N, np.zeros(N, np.int32), np.array(xyz[:, 0]), np.array(xyz[:, 1]), np.array(xyz[:, 2]), h["nn"], 1.0, 1.0,
                                      [1.0, 1.0, 1.0], np.array([6], np.int32))
        buf.neigh_idx = ctx.i32(h["neigh"].reshape(-1))
        self.value = torch.zeros(N, dtype=torch.float64, device="cuda")
        self.stage = dict(xyz=_xyz(buf.site_x, buf.site_y, buf.site_z), value=[(self.value, None)])
        torch.cuda.synchronize()

    def call(self):
        self.res = self.ctx.S.site_gradient(self.comm_, self.buf, self.value)

    def read(self):
        return self.res


FAMILIES = [(_Vec, ("spmv", "pcg_jacobi/loop", "pcg_jacobi/resident", "solve_sparse_CG_Jacobi", "pack", "unpack", "unpack_add",
                    "elementwise_vector_vector", "matrix_values")),
            (_Pairwise, ("compute_cutoff_list", "compute_cutoff_list_pbc", "poisson_gridless/seventeen", "poisson_gridless/cube")),
            (_T, ("initialize_sparsity_T", "t_assemble", "update_power_sparse", "current_map", "current_profile")),
            (_Events, ("event_rates", "execute_kmc_step", "execute_kmc_step_thermal")),
            (_Clusters, ("conductive_clusters",)), (_Gradient, ("site_gradient",)),
            (_SiteSet, ("site_set_gap", "site_set_chain", "site_set_gap_pbc", "site_set_chain_pbc"))]
MAKERS = {name: maker for maker, names in FAMILIES for name in names}
MAKERS.update({name: _K for name in SO.CASES if name not in MAKERS})


def _knobs(monkeypatch, name):
    """the two PCG cases force their path through the knobs of tests/test_gpu_cgr_synthetic.py; every other case runs
    the library's own choice"""
    if name.startswith("pcg_jacobi"):
        from test_gpu_cgr_synthetic import _force
        _force(monkeypatch, SO.case(name)["host"]["rows"], "classic", resident="1" if name.endswith("resident") else "0")


@pytest.mark.parametrize("stream", ["default", "side"])
@pytest.mark.parametrize("name", SO.CASES)
def test_entry_point_waits_for_the_callers_stream(km, torch, filler, monkeypatch, name, stream):
    _knobs(monkeypatch, name)
    t0 = time.perf_counter()
    _run_case(MAKERS[name], km, torch, filler, SO.case(name), side=stream == "side")
    print("%s, %s stream: %.2f s" % (name, stream, time.perf_counter() - t0))


# ------------------------------------------------------------------------------------------------ KMCF_ENTER_ALWAYS
@pytest.mark.parametrize("name", ["update_charge", "poisson_gridless/cube", "spmv"])
def test_enter_always_gives_the_reference_bytes(km, torch, filler, name):
    """KMCF_ENTER_ALWAYS (INTEGRATION.md's remedy where the idle test of the caller's stream is not trusted), set per
    communicator with kmcf_set_option: the reference bytes with an idle caller stream and with the filler in flight."""
    c, make = SO.case(name), MAKERS[name]
    true, _ = _references(make, km, torch, c)
    opt = {"KMCF_ENTER_ALWAYS": "1"}
    ctx = _Ctx(km, torch, options=opt)
    st = make(ctx, c)
    try:
        assert st.comms[0].get_option("KMCF_ENTER_ALWAYS") == ("1", 2)
    finally:
        st.close()
    assert _reference(make, ctx, c, "true") == true, "idle caller stream"
    for side in (False, True):
        _run_case(make, km, torch, filler, c, side=side, options=opt)


# ------------------------------------------------------------------------------------------------ switching back
def test_default_stream_is_the_callers_again_after_a_reset(km, torch, filler):
    """kmcf_comm_set_caller_stream(c, side), then (c, None): a call with work queued on torch's default stream is ordered
    behind it again (the side stream, idle, is no longer asked)."""
    c, make = SO.case("spmv"), MAKERS["spmv"]
    true, _ = _references(make, km, torch, c)
    side = _side(torch)

    def make_and_switch(ctx, c):
        st = make(ctx, c)
        ctx.declare(st.comms[0], side)
        with torch.cuda.stream(side):                        # one call on the side stream, idle: the declared stream is in use
            st.call()
        ctx.declare(st.comms[0], None)
        st.t["out"].fill_(SENTINEL)
        torch.cuda.synchronize()
        return st

    got = _staged(make_and_switch, _Ctx(km, torch), c, filler)
    assert not _differing(got, true)


# ------------------------------------------------------------------------------------------------ a group of two ranks
_GROUP_FILLERS = []


def _group_run(km, torch, filler, staged):
    """kmcf_spmv and one kmcf_pcg_jacobi on two in-process ranks, each on a side stream of its own, declared on its own
    communicator; staged: every rank's slices hold decoys at the call, the true values are queued behind a filler."""
    from test_gpu_multirank import _tridiagonal
    S = km.solvers
    g = SO.group()
    n, P, arr = g["host"]["n"], g["host"]["P"], g["arrays"]
    M = _tridiagonal(n)
    counts, displs = S.KMC_comm.partition(n, P)
    comms = S.KMC_comm.loopback_group(n, n, n, n, size=P, device=0)
    out, errs = [None] * P, []
    while len(_GROUP_FILLERS) < P - 1:
        _GROUP_FILLERS.append(_Filler(torch))
    fillers = [filler] + _GROUP_FILLERS                      # (a scratch tensor per rank: the ranks run at the same time)

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            comm.connect()
            side = _side(torch, 1 + r)
            km.lib.check(km.lib.load().kmcf_comm_set_caller_stream(comm.handle, side.cuda_stream), "kmcf_comm_set_caller_stream")
            r0, nr = int(displs[r]), int(counts[r])
            sl = slice(r0, r0 + nr)
            sub = M[r0:r0 + nr]
            dev = lambda a: torch.as_tensor(np.array(a[sl]), device="cuda")
            with torch.cuda.stream(side):
                mat = S.Distributed_matrix(comm, n, counts, displs, sub.indices, sub.indptr, sub.data)
                dinv = dev(1.0 / M.diagonal())
                first = "decoy" if staged else "true"
                p, b, x0 = (dev(getattr(arr[k], first)) for k in ("p", "b", "x0"))
                src = [dev(arr[k].true) for k in ("p", "b", "x0")]
                Ap = torch.empty_like(p)
                torch.cuda.synchronize()
                res = {}
                for what in ("spmv", "pcg"):
                    if staged:
                        fillers[r].queue()
                        for t, s in zip((p,) if what == "spmv" else (b, x0), src[:1] if what == "spmv" else src[1:]):
                            t.copy_(s, non_blocking=True)
                        res[what + "_busy"] = side.query()
                    if what == "spmv":
                        mat.spmv(p, Ap)
                    else:
                        res["stats"] = S.conjugate_gradient_jacobi(mat, b, x0, dinv, 1e-12, 500)
                    if staged:
                        res[what + "_done"] = side.query()
                res.update(Ap=Ap.cpu().numpy(), x=x0.cpu().numpy(), r=b.cpu().numpy(), transport=comm.transport())
                mat.close()
            km.lib.check(km.lib.load().kmcf_comm_set_caller_stream(comm.handle, None), "kmcf_comm_set_caller_stream")
            out[r] = res
        except Exception as e:  # pragma: no cover
            import traceback
            errs.append("rank %d: %s\n%s" % (r, e, traceback.format_exc()))

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(P)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish (deadlock?)"
    for c in comms:
        c.close()
    return out


@pytest.mark.parametrize("transport", ["loopback", "p2p"])
def test_group_of_two_ranks_on_side_streams(km, torch, filler, monkeypatch, transport):
    """The halo pack kernel and the puts read p on another stream than the compute stream: they wait for the caller's
    queue as well.  Only vector values are staged; the control flow is shared through the all-reduced scalars."""
    monkeypatch.setenv("KMCF_CG_RESIDENT", "0")
    if transport == "p2p":
        monkeypatch.setenv("KMCF_TRANSPORT", "p2p")
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    ref = _group_run(km, torch, filler, staged=False)
    got = _group_run(km, torch, filler, staged=True)
    for r, (a, b) in enumerate(zip(got, ref)):
        print("rank %d on %s: %d iterations, busy %s / %s, done %s / %s" % (r, a["transport"], a["stats"]["iterations"], a["spmv_busy"],
                                                                              a["pcg_busy"], a["spmv_done"], a["pcg_done"]))
        assert ("p2p" in a["transport"]) == (transport == "p2p"), a["transport"]
        assert a["spmv_busy"] is False and a["pcg_busy"] is False, "the filler is too short"
        assert a["spmv_done"] is True and a["pcg_done"] is True
        for k in ("Ap", "x", "r"):
            assert a[k].tobytes() == b[k].tobytes(), "rank %d: %s differs from the synchronised group's" % (r, k)
        assert _norm(a["stats"]) == _norm(b["stats"])
