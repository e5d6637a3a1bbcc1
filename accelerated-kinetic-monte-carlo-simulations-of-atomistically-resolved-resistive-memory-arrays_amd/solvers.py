"""Host-side mirror of the reference's call surface for the field-solve path.

Names, argument meaning and side effects follow src/gpu_solvers.h:36-263,
src/gpu_buffers.h, src/KMC_comm.h and dist_iterative/ so that the parity tests
read like calls into the reference.  Every function forwards to the C ABI of
libkmcfield.so (include/kmcfield.h); torch is used only to own device memory
and (optionally) to bootstrap the RCCL communicator.  No compute happens here
and nothing falls back to the CPU.
"""
import ctypes as C

import numpy as np
import torch

from . import lib as _L


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device tensors must be contiguous CUDA tensors"
    return C.c_void_p(t.data_ptr())


def _ia(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def _da(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


class KMC_comm:
    """Partition tables of src/KMC_comm.h:225-289 (split=false: every module uses
    all ranks) plus this rank's libkmcfield communicator."""

    def __init__(self, nrows_K, nrows_T, nrows_pairwise, nrows_events, rank=0, size=1, device=0, _handle=None,
                 options=None):
        self.lib = _L.load()
        self.rank_K = self.rank_events = self.rank_pairwise = rank
        self.size_K = self.size_events = self.size_pairwise = size
        self.counts_K, self.displs_K = self.partition(nrows_K, size)
        self.rank_T, self.size_T = rank, size                      # the reference forces comm_T off (KMC_comm.h:243)
        self.counts_T, self.displs_T = self.partition(nrows_T, size)
        self.counts_pairwise, self.displs_pairwise = self.partition(nrows_pairwise, size)
        self.counts_events, self.displs_events = self.partition(nrows_events, size)
        self.device = device
        self.loopback = _handle is not None
        if _handle is None:
            h = C.c_void_p()
            _L.check(self.lib.kmcf_comm_create(C.byref(h), device, size, rank), "kmcf_comm_create")
            _handle = h
        self.handle = _handle
        for key, value in (options or {}).items():       # (before connect(): connect-scope knobs apply)
            self.set_option(key, value)

    @classmethod
    def loopback_group(cls, nrows_K, nrows_T, nrows_pairwise, nrows_events, size, device=0, options=None):
        """All `size` ranks of an in-process test group on one GPU (kmcf_comm_create_loopback); each
        returned KMC_comm must be driven by its own host thread.  options: one dict for every rank, or a list of
        per-rank dicts (KMC_comm.set_option).  The group is connected at creation, so its connect-scope knobs
        (KMCF_TRANSPORT, ...) come from the environment."""
        if options is None or isinstance(options, dict):
            options = [options] * size
        assert len(options) == size, "options: one dict, or one per rank"
        lib = _L.load()
        arr = (C.c_void_p * size)()
        _L.check(lib.kmcf_comm_create_loopback(arr, device, size), "kmcf_comm_create_loopback")
        return [cls(nrows_K, nrows_T, nrows_pairwise, nrows_events, rank=r, size=size, device=device,
                    _handle=C.c_void_p(arr[r]), options=options[r]) for r in range(size)]

    def set_option(self, key, value):
        """kmcf_set_option: a KMCF_* knob on this communicator only (value None: back to the environment).
        Flags take "1" / "0"; numbers may be given as int or float."""
        v = None if value is None else str(value).encode()
        _L.check(self.lib.kmcf_set_option(self.handle, key.encode(), v), "kmcf_set_option(%s)" % key)

    def get_option(self, key):
        """(effective value or None if the library decides, source): 0 default, 1 environment, 2 set here."""
        buf = C.create_string_buffer(256)
        src = self.lib.kmcf_get_option(self.handle, key.encode(), buf, len(buf))
        if src < 0:
            _L.check(src, "kmcf_get_option(%s)" % key)
        v = buf.value.decode()
        return (v if src else None), src

    @staticmethod
    def option_table():
        """kmcf_option_info: [(name, values, scope 0 comm / 1 connect / 2 process, group)] in the library's order."""
        lib = _L.load()
        out, i = [], 0
        name, values, scope, group = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int()
        while lib.kmcf_option_info(i, C.byref(name), C.byref(values), C.byref(scope), C.byref(group)) == 0:
            out.append((name.value.decode(), values.value.decode(), scope.value, bool(group.value)))
            i += 1
        return out

    @staticmethod
    def partition(nrows, size):
        lib = _L.load()
        counts = np.zeros(size, np.int32)
        displs = np.zeros(size, np.int32)
        _L.check(lib.kmcf_partition(int(nrows), int(size), counts.ctypes.data_as(C.POINTER(C.c_int)),
                                    displs.ctypes.data_as(C.POINTER(C.c_int))), "kmcf_partition")
        return counts, displs

    def connect(self, dist=None):
        """Bootstrap RCCL: rank 0 creates the unique id, torch.distributed (any
        backend) broadcasts its 128 bytes, every rank joins.  No-op for 1 rank."""
        if self.size_K == 1 or self.loopback:
            _L.check(self.lib.kmcf_comm_connect(self.handle, None), "kmcf_comm_connect")
            return
        assert dist is not None and dist.is_initialized(), "multi-rank groups need torch.distributed for bootstrap"
        buf = (C.c_char * _L.KMCF_UNIQUE_ID_BYTES)()
        if self.rank_K == 0:
            _L.check(self.lib.kmcf_comm_unique_id(buf), "kmcf_comm_unique_id")
        t = torch.tensor(list(bytes(buf)), dtype=torch.uint8)
        use_cuda = dist.get_backend() == "nccl"
        if use_cuda:
            t = t.cuda(self.device)
        dist.broadcast(t, src=0)
        raw = bytes(t.cpu().tolist())
        _L.check(self.lib.kmcf_comm_connect(self.handle, C.create_string_buffer(raw, len(raw))), "kmcf_comm_connect")

    def connect_p2p(self, dist):
        """Bootstrap the peer-to-peer transport WITHOUT RCCL (kmcf_comm_p2p_export / _import): every rank exports
        the IPC handle of its window, the host program all-gathers them (here: torch.distributed, any backend), every
        rank maps its peers.  Used where RCCL cannot run (several ranks on one GPU) and by tests."""
        _L.check(self.lib.kmcf_comm_connect(self.handle, None), "kmcf_comm_connect")
        nb = 64   # KMCF_P2P_HANDLE_BYTES
        buf = (C.c_char * nb)()
        _L.check(self.lib.kmcf_comm_p2p_export(self.handle, buf), "kmcf_comm_p2p_export")
        mine = torch.tensor(list(bytes(buf)), dtype=torch.uint8)
        parts = [torch.zeros(nb, dtype=torch.uint8) for _ in range(self.size_K)]
        dist.all_gather(parts, mine)
        raw = b"".join(bytes(t.tolist()) for t in parts)
        _L.check(self.lib.kmcf_comm_p2p_import(self.handle, C.create_string_buffer(raw, len(raw))), "kmcf_comm_p2p_import")

    def transport(self):
        return self.lib.kmcf_comm_transport(self.handle).decode()

    def rccl_ranks(self):
        return int(self.lib.kmcf_comm_rccl_ranks(self.handle))

    def select_transport(self, use_p2p):
        _L.check(self.lib.kmcf_comm_select_transport(self.handle, 1 if use_p2p else 0), "kmcf_comm_select_transport")

    def sync(self):
        _L.check(self.lib.kmcf_comm_sync(self.handle), "kmcf_comm_sync")

    def close(self):
        if self.handle:
            self.lib.kmcf_comm_destroy(self.handle)
            self.handle = None


class GPUBuffers:
    """Device SoA of src/gpu_buffers.h:12-162 (the members the K path touches).
    Arrays are torch CUDA tensors; K_distributed is the libkmcfield K state."""

    def __init__(self, N, site_element, site_x, site_y, site_z, nn, sigma, k, lattice, metals, device=0,
                 site_power=None, T_bg=300.0):
        dev = torch.device("cuda", device)
        self.device = dev
        self.N_ = int(N)
        self.nn_ = int(nn)
        self.num_metal_types_ = len(metals)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.site_element = torch.as_tensor(np.asarray(site_element, np.int32), **i32)
        self.site_x = torch.as_tensor(np.asarray(site_x, np.float64), **f64)
        self.site_y = torch.as_tensor(np.asarray(site_y, np.float64), **f64)
        self.site_z = torch.as_tensor(np.asarray(site_z, np.float64), **f64)
        self.site_charge = torch.zeros(N, **i32)
        self.site_potential_boundary = torch.zeros(N, **f64)
        self.site_potential_charge = torch.zeros(N, **f64)
        self.site_power = torch.zeros(N, **f64) if site_power is None else torch.as_tensor(site_power, **f64)
        self.T_bg = torch.tensor([T_bg], **f64)
        self.metal_types = torch.as_tensor(np.asarray(metals, np.int32), **i32)
        self.lattice_host = np.asarray(lattice, np.float64)
        self.sigma, self.k = float(sigma), float(k)
        self.neigh_idx = None
        self.cutoff_idx = None         # kmcf_pairwise* (replaces cutoff_idx / cutoff_window)
        self.cutoff_radius = None      # ... and the cutoff radius it was built with (compute_cutoff_list)
        self.K_distributed = None      # kmcf_kstate* (K_distributed + K_p_distributed + contact patterns)
        self.T_distributed = None      # kmcf_tstate* (T_distributed + T_p_distributed + atom_* arrays)
        self.site_CB_edge = None
        self.site_temperature = None   # kmcf_update_temperature_local (created on first use)
        self.atom_virtual_potentials = None   # N_atom + 2 doubles, allocated by initialize_sparsity_T
        self.N_atom_ = 0

    def freeGPUmemory(self):
        if self.T_distributed is not None:
            _L.load().kmcf_tstate_destroy(self.T_distributed)
            self.T_distributed = None
        if self.K_distributed is not None:
            _L.load().kmcf_kstate_destroy(self.K_distributed)
            self.K_distributed = None
        if self.cutoff_idx is not None:
            _L.load().kmcf_pairwise_destroy(self.cutoff_idx)
            self.cutoff_idx = self.cutoff_radius = None


# --------------------------------------------------------------------------
# gpu_solvers.h surface
# --------------------------------------------------------------------------

def compute_neighbor_list(kmc_comm, gpubuf, nn_dist=3.5, max_num_neighbors=52, pbc=0):
    """compute_neighbor_list (gpu_solvers.h:43; src/neighbor_lists_gpu.cu:252-292).  pbc = 1: the minimum image in y and z
    with the periods of gpubuf.lattice_host (kmcf_neighbor_list_pbc); the default is kmcf_neighbor_list."""
    lib = _L.load()
    count = int(kmc_comm.counts_events[kmc_comm.rank_events])
    displ = int(kmc_comm.displs_events[kmc_comm.rank_events])
    gpubuf.neigh_idx = torch.empty(max(count, 1) * max_num_neighbors, dtype=torch.int32, device=gpubuf.device)
    gpubuf.nn_ = max_num_neighbors
    if pbc:
        lat, latp = _da(gpubuf.lattice_host)
        _L.check(lib.kmcf_neighbor_list_pbc(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                            gpubuf.N_, latp, int(pbc), float(nn_dist), max_num_neighbors, count, displ,
                                            _ptr(gpubuf.neigh_idx)), "kmcf_neighbor_list_pbc")
        return
    _L.check(lib.kmcf_neighbor_list(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                    gpubuf.N_, float(nn_dist), max_num_neighbors, count, displ,
                                    _ptr(gpubuf.neigh_idx)), "kmcf_neighbor_list")


def initialize_sparsity_K(gpubuf, pbc, nn_dist, num_atoms_contact, kmc_comm):
    """initialize_sparsity_K (gpu_solvers.h:53; src/iterative_solvers_gpu.cu:262-488)."""
    lib = _L.load()
    h = C.c_void_p()
    lat, latp = _da(gpubuf.lattice_host)
    cnt, cntp = _ia(kmc_comm.counts_K)
    dsp, dspp = _ia(kmc_comm.displs_K)
    _L.check(lib.kmcf_initialize_sparsity_K(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y),
                                            _ptr(gpubuf.site_z), latp, gpubuf.N_, int(pbc), float(nn_dist),
                                            int(num_atoms_contact), cntp, dspp, C.byref(h)),
             "kmcf_initialize_sparsity_K")
    gpubuf.K_distributed = h


def update_charge_gpu(site_element, site_charge, neigh_idx, N, nn, metals, num_metals, count, displ, kmc_comm):
    """update_charge_gpu (gpu_solvers.h:149; src/potential_solver_gpu.cu:66-85)."""
    lib = _L.load()
    cnt, cntp = _ia(count)
    dsp, dspp = _ia(displ)
    _L.check(lib.kmcf_update_charge(kmc_comm.handle, _ptr(site_element), _ptr(site_charge), _ptr(neigh_idx),
                                    int(N), int(nn), _ptr(metals), int(num_metals), cntp, dspp), "kmcf_update_charge")


def background_potential_gpu_sparse(gpubuf, N, N_left_tot, N_right_tot, Vd, pbc, high_G, low_G, nn_dist,
                                    num_metals, kmc_step_count=0):
    """background_potential_gpu_sparse (gpu_solvers.h:162; src/potential_solver_gpu.cu:846-1128).
    Returns the solve statistics (the reference prints the iteration count on rank 0)."""
    lib = _L.load()
    st = _L.SolveStats()
    _L.check(lib.kmcf_background_potential_sparse(gpubuf.K_distributed, _ptr(gpubuf.site_element),
                                                  _ptr(gpubuf.site_charge), _ptr(gpubuf.metal_types), int(num_metals),
                                                  _ptr(gpubuf.site_potential_boundary), int(N), int(N_left_tot),
                                                  int(N_right_tot), float(Vd), float(high_G), float(low_G),
                                                  C.byref(st)), "kmcf_background_potential_sparse")
    return st.as_dict()


def background_potential_gpu_sparse_contacts(gpubuf, N, N_left_tot, N_right_tot, high_G, low_G, num_metals):
    """kmcf_background_potential_sparse_contacts: the K solve with one Dirichlet value per contact site.  The contact
    slots [0, N_left_tot) and [N - N_right_tot, N) of gpubuf.site_potential_boundary are the boundary condition (fill
    them once, e.g. from structure.bias_scheme; they are read, never written), its interface slice is the start guess
    and receives the solution.  Returns the solve statistics."""
    lib = _L.load()
    st = _L.SolveStats()
    _L.check(lib.kmcf_background_potential_sparse_contacts(gpubuf.K_distributed, _ptr(gpubuf.site_element),
                                                           _ptr(gpubuf.site_charge), _ptr(gpubuf.metal_types),
                                                           int(num_metals), _ptr(gpubuf.site_potential_boundary), int(N),
                                                           int(N_left_tot), int(N_right_tot), float(high_G), float(low_G),
                                                           C.byref(st)), "kmcf_background_potential_sparse_contacts")
    return st.as_dict()


def update_CB_edge_gpu_sparse(gpubuf, N, N_left_tot, N_right_tot, Vd, pbc, high_G, low_G, nn_dist, num_metals):
    """update_CB_edge_gpu_sparse (gpu_solvers.h:143; src/potential_solver_gpu.cu:673-772): writes
    gpubuf.site_CB_edge [J]."""
    lib = _L.load()
    if getattr(gpubuf, "site_CB_edge", None) is None:
        gpubuf.site_CB_edge = torch.zeros(gpubuf.N_, dtype=torch.float64, device=gpubuf.device)
    st = _L.SolveStats()
    _L.check(lib.kmcf_update_CB_edge_sparse(gpubuf.K_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                            _ptr(gpubuf.metal_types), int(num_metals), _ptr(gpubuf.site_CB_edge),
                                            int(N), int(N_left_tot), int(N_right_tot), float(Vd), float(high_G),
                                            float(low_G), C.byref(st)), "kmcf_update_CB_edge_sparse")
    return st.as_dict()


def initialize_sparsity_T(gpubuf, pbc, nn_dist, num_source_inj, num_ground_ext, num_layers_contact, kmc_comm, periodic=False):
    """initialize_sparsity_T (gpu_solvers.h:57; src/initialize_sparsity_T.cu:948-1154).  kmc_comm.counts_T must
    partition N_atom + 1 rows (src/kmc_main.cpp:165-171); pbc is accepted and, like the reference's T kernels,
    not used (they call the non-periodic site_dist_gpu overload).  periodic=True with pbc == 1:
    kmcf_initialize_sparsity_T_pbc with the periods of gpubuf.lattice_host -- neighbour pattern, ground flag, tunnel
    block and current map take the minimum image in y and z (include/kmcfield.h).  periodic=True with any other pbc
    builds the OPEN state without a warning (a caller's pbc = 0 device has no periods to take): t_periodic(gpubuf) is how
    to find out which state was built."""
    lib = _L.load()
    if gpubuf.T_distributed is not None:
        lib.kmcf_tstate_destroy(gpubuf.T_distributed)
        gpubuf.T_distributed = None
    h = C.c_void_p()
    cnt, cntp = _ia(kmc_comm.counts_T)
    dsp, dspp = _ia(kmc_comm.displs_T)
    if periodic and int(pbc) == 1:
        lat, latp = _da(gpubuf.lattice_host)
        _L.check(lib.kmcf_initialize_sparsity_T_pbc(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                                    _ptr(gpubuf.site_element), gpubuf.N_, latp, 1, float(nn_dist),
                                                    int(num_source_inj), int(num_ground_ext), int(num_layers_contact), cntp, dspp,
                                                    C.byref(h)), "kmcf_initialize_sparsity_T_pbc")
    else:
        _L.check(lib.kmcf_initialize_sparsity_T(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                                _ptr(gpubuf.site_element), gpubuf.N_, float(nn_dist), int(num_source_inj),
                                                int(num_ground_ext), int(num_layers_contact), cntp, dspp, C.byref(h)),
                 "kmcf_initialize_sparsity_T")
    gpubuf.T_distributed = h
    info = t_info(gpubuf)
    gpubuf.N_atom_ = info["N_atom"]
    if gpubuf.atom_virtual_potentials is None or gpubuf.atom_virtual_potentials.numel() != info["N_atom"] + 2:
        gpubuf.atom_virtual_potentials = torch.zeros(info["N_atom"] + 2, dtype=torch.float64, device=gpubuf.device)


def current_params(Vd, high_G, low_G, loop_G, G0, tol, m_e, V0, alpha_disp=1.0, solve_heating=False,
                   cg_tolerance=None, cg_max_iterations=100, N_atom=None, contact_x_lo=-4.2, contact_x_hi=52.65):
    """kmcf_current_params_t.  Defaults = what the reference hard-codes: cg tolerance 1e-30 * N_atom and 100
    iterations (src/current_solver_gpu.cu:1455-1456), contact window -4.2 .. 52.65 A (initialize_sparsity_T.cu:645)."""
    if cg_tolerance is None:
        cg_tolerance = 1e-30 * (N_atom or 1)
    return _L.CurrentParams(float(Vd), float(high_G), float(low_G), float(loop_G), float(G0), float(tol), float(m_e),
                            float(V0), float(alpha_disp), float(contact_x_lo), float(contact_x_hi), float(cg_tolerance),
                            int(cg_max_iterations), int(bool(solve_heating)))


def t_assemble(gpubuf, params):
    """Assembly half of update_power_gpu_sparse_dist (src/current_solver_gpu.cu:1496-1632)."""
    _L.check(_L.load().kmcf_t_assemble(gpubuf.T_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                       _ptr(gpubuf.site_CB_edge), _ptr(gpubuf.metal_types), gpubuf.num_metal_types_,
                                       C.byref(params)), "kmcf_t_assemble")


def update_power_gpu_sparse_dist(gpubuf, num_source_inj, num_ground_ext, num_layers_contact, Vd, high_G, low_G, loop_G,
                                 G0, tol, nn_dist, m_e, V0, num_metals, solve_heating_local, solve_heating_global,
                                 alpha_disp, cg_tolerance=None, cg_max_iterations=100, contact_x_lo=-4.2,
                                 contact_x_hi=52.65):
    """update_power_gpu_sparse_dist (gpu_solvers.h:212; src/current_solver_gpu.cu:1430-1855).  Returns
    (imacro, solve statistics); gpubuf.atom_virtual_potentials and gpubuf.site_power are updated in place."""
    lib = _L.load()
    prm = current_params(Vd, high_G, low_G, loop_G, G0, tol, m_e, V0, alpha_disp,
                         bool(solve_heating_local or solve_heating_global), cg_tolerance, cg_max_iterations,
                         gpubuf.N_atom_, contact_x_lo, contact_x_hi)
    st = _L.SolveStats()
    im = C.c_double(0.0)
    _L.check(lib.kmcf_update_power_sparse(gpubuf.T_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                          _ptr(gpubuf.site_CB_edge), _ptr(gpubuf.metal_types), int(num_metals),
                                          _ptr(gpubuf.atom_virtual_potentials), _ptr(gpubuf.site_power), C.byref(prm),
                                          C.byref(im), C.byref(st)), "kmcf_update_power_sparse")
    return im.value, st.as_dict()


def current_map(gpubuf, potentials=None, tunnel=True, net=True):
    """kmcf_current_map: where the current of a potential field flows (definitions: include/kmcfield.h).  Call it after
    update_power_gpu_sparse_dist (or t_assemble, with potentials of your own: N_atom + 2 doubles on the device; default
    gpubuf.atom_virtual_potentials).  Returns dict(current: N doubles per site, tunnel / net: the same or None, stats)."""
    pot = gpubuf.atom_virtual_potentials if potentials is None else potentials
    assert pot is None or pot.numel() == gpubuf.N_atom_ + 2, "potentials: N_atom + 2 doubles"
    f64 = dict(dtype=torch.float64, device=gpubuf.device)
    cur = torch.empty(gpubuf.N_, **f64)
    tun = torch.empty(gpubuf.N_, **f64) if tunnel else None
    nt = torch.empty(gpubuf.N_, **f64) if net else None
    st = _L.CurrentMapStats()
    _L.check(_L.load().kmcf_current_map(gpubuf.T_distributed, _ptr(pot), _ptr(cur), _ptr(tun), _ptr(nt), C.byref(st)),
             "kmcf_current_map")
    return dict(current=cur, tunnel=tun, net=nt, stats=st.as_dict())


def current_profile(gpubuf, planes, site_cell=None, n_cells=1, potentials=None, vector=False):
    """kmcf_current_profile: the current through x-planes per cell and kind, and the per-site current vector
    (definitions: include/kmcfield.h).  planes: strictly ascending x values (host); site_cell: N ints on the device or
    None (one cell).  Returns dict(profile: ndarray [n_cells + 1, n_planes, 2] -- the last cell index is the rest, the
    last axis neighbour / tunnel pairs --, jx / jy / jz: N doubles per site on the device or None, stats)."""
    pot = gpubuf.atom_virtual_potentials if potentials is None else potentials
    assert pot is None or pot.numel() == gpubuf.N_atom_ + 2, "potentials: N_atom + 2 doubles"
    assert site_cell is None or (site_cell.numel() == gpubuf.N_ and site_cell.dtype == torch.int32), "site_cell: N int32"
    x = np.ascontiguousarray(planes, np.float64).reshape(-1)
    n_cells = int(n_cells)
    prof = np.zeros((max(n_cells, 0) + 1, len(x), 2))
    f64 = dict(dtype=torch.float64, device=gpubuf.device)
    jx, jy, jz = (torch.empty(gpubuf.N_, **f64) for _ in range(3)) if vector else (None, None, None)
    st = _L.CurrentProfileStats()
    dp = C.POINTER(C.c_double)
    _L.check(_L.load().kmcf_current_profile(gpubuf.T_distributed, _ptr(pot), _ptr(site_cell), n_cells, x.ctypes.data_as(dp),
                                            len(x), prof.ctypes.data_as(dp), _ptr(jx), _ptr(jy), _ptr(jz), C.byref(st)),
             "kmcf_current_profile")
    return dict(profile=prof, jx=jx, jy=jy, jz=jz, stats=st.as_dict())


def t_periodic(gpubuf):
    """kmcf_tstate_periodic: (pbc, lattice) the T state was built with -- (0, zeros) for a state of the plain call."""
    pbc, lat = C.c_int(-1), np.zeros(3)
    _L.check(_L.load().kmcf_tstate_periodic(gpubuf.T_distributed, C.byref(pbc), lat.ctypes.data_as(C.POINTER(C.c_double))),
             "kmcf_tstate_periodic")
    return pbc.value, lat


def t_info(gpubuf):
    info = _L.TStateInfo()
    _L.check(_L.load().kmcf_tstate_info(gpubuf.T_distributed, C.byref(info)), "kmcf_tstate_info")
    return {k: getattr(info, k) for k, _ in info._fields_}


def t_pattern(gpubuf):
    """(row_ptr, col) of this rank's rows of the T neighbour matrix, global columns."""
    lib = _L.load()
    n = t_info(gpubuf)["rows_this_rank"]
    nnz = C.c_int64()
    rp = np.zeros(n + 1, np.int32)
    _L.check(lib.kmcf_tstate_pattern(gpubuf.T_distributed, rp.ctypes.data_as(C.POINTER(C.c_int)), None, C.byref(nnz)),
             "kmcf_tstate_pattern")
    col = np.zeros(max(nnz.value, 1), np.int32)
    _L.check(lib.kmcf_tstate_pattern(gpubuf.T_distributed, rp.ctypes.data_as(C.POINTER(C.c_int)),
                                     col.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nnz)), "kmcf_tstate_pattern")
    return rp, col[:nnz.value]


def t_atom_sites(gpubuf):
    a = np.zeros(t_info(gpubuf)["N_atom"], np.int32)
    _L.check(_L.load().kmcf_tstate_atom_sites(gpubuf.T_distributed, a.ctypes.data_as(C.POINTER(C.c_int))),
             "kmcf_tstate_atom_sites")
    return a


def t_vectors(gpubuf):
    """After t_assemble: dict(val, diag_neighbour, dinv, rhs) of this rank's rows (caller order)."""
    lib = _L.load()
    info = t_info(gpubuf)
    n = info["rows_this_rank"]
    out = {k: np.zeros(max(n, 1)) for k in ("diag_neighbour", "dinv", "rhs")}
    dp = C.POINTER(C.c_double)
    _L.check(lib.kmcf_tstate_get_vectors(gpubuf.T_distributed, out["diag_neighbour"].ctypes.data_as(dp),
                                         out["dinv"].ctypes.data_as(dp), out["rhs"].ctypes.data_as(dp)),
             "kmcf_tstate_get_vectors")
    out = {k: v[:n] for k, v in out.items()}
    val = np.zeros(max(info["nnz_neighbour"], 1))
    _L.check(lib.kmcf_matrix_get_values(lib.kmcf_tstate_matrix(gpubuf.T_distributed), val.ctypes.data_as(dp)),
             "kmcf_matrix_get_values")
    out["val"] = val[:info["nnz_neighbour"]]
    return out


def t_tunnel(gpubuf):
    """After t_assemble: dict(tunnel_idx, row_ptr, col, val, diag) of this rank's rows of the tunnel sub-block."""
    lib = _L.load()
    info = t_info(gpubuf)
    nt, ns, nnz = info["tunnel_points"], info["tunnel_points_rank"], info["nnz_tunnel"]
    tidx = np.zeros(max(nt, 1), np.int32)
    rp = np.zeros(ns + 1, np.int32)
    col = np.zeros(max(nnz, 1), np.int32)
    val = np.zeros(max(nnz, 1))
    diag = np.zeros(max(ns, 1))
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    _L.check(lib.kmcf_tstate_get_tunnel(gpubuf.T_distributed, tidx.ctypes.data_as(ip), rp.ctypes.data_as(ip),
                                        col.ctypes.data_as(ip), val.ctypes.data_as(dp), diag.ctypes.data_as(dp)),
             "kmcf_tstate_get_tunnel")
    return dict(tunnel_idx=tidx[:nt], row_ptr=rp, col=col[:nnz], val=val[:nnz], diag=diag[:ns], first=info["tunnel_first"])


def sum_and_gather_potential(gpubuf, num_atoms_first_layer, kmc_comm):
    """sum_and_gather_potential (gpu_solvers.h:181; src/potential_solver_gpu.cu:1130-1151) including the
    MPI_Gatherv of the solution done by the caller in the reference (src/kmc_main.cpp:367-384)."""
    lib = _L.load()
    cp = dp = None
    if getattr(gpubuf, "cutoff_idx", None) is not None:     # the pairwise term is in use: gather its rows too
        c_, cp = _ia(kmc_comm.counts_pairwise)
        d_, dp = _ia(kmc_comm.displs_pairwise)
    _L.check(lib.kmcf_sum_and_gather_potential(gpubuf.K_distributed, _ptr(gpubuf.site_potential_boundary),
                                               _ptr(gpubuf.site_potential_charge), gpubuf.N_,
                                               int(num_atoms_first_layer), cp, dp), "kmcf_sum_and_gather_potential")


def compute_cutoff_list(kmc_comm, gpubuf, cutoff_radius=20.0, pbc=0):
    """compute_cutoff_list (gpu_solvers.h:46; src/neighbor_lists_gpu.cu:293-372).  gpubuf.cutoff_idx becomes
    the opaque spatial index that replaces the reference's N x N_cutoff index list.  pbc = 1: a periodic index with the
    periods of gpubuf.lattice_host (kmcf_compute_cutoff_list_pbc), on which poisson_gridless_gpu takes the minimum image;
    the default is kmcf_compute_cutoff_list."""
    lib = _L.load()
    h = C.c_void_p()
    if pbc:
        lat, latp = _da(gpubuf.lattice_host)
        _L.check(lib.kmcf_compute_cutoff_list_pbc(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                                  gpubuf.N_, float(cutoff_radius), latp, int(pbc), C.byref(h)),
                 "kmcf_compute_cutoff_list_pbc")
        gpubuf.cutoff_idx, gpubuf.cutoff_radius = h, float(cutoff_radius)
        return
    _L.check(lib.kmcf_compute_cutoff_list(kmc_comm.handle, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y),
                                          _ptr(gpubuf.site_z), gpubuf.N_, float(cutoff_radius), C.byref(h)),
             "kmcf_compute_cutoff_list")
    gpubuf.cutoff_idx, gpubuf.cutoff_radius = h, float(cutoff_radius)


def poisson_gridless_gpu(gpubuf, kmc_comm):
    """poisson_gridless_gpu (gpu_solvers.h:173; src/potential_solver_gpu.cu:1620-1655): the rows of this
    rank of site_potential_charge."""
    lib = _L.load()
    r = kmc_comm.rank_pairwise
    _L.check(lib.kmcf_poisson_gridless(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                       _ptr(gpubuf.site_charge), gpubuf.sigma, gpubuf.k,
                                       int(kmc_comm.counts_pairwise[r]), int(kmc_comm.displs_pairwise[r]),
                                       _ptr(gpubuf.site_potential_charge)), "kmcf_poisson_gridless")


def update_temperatureglobal_gpu(site_power, T_bg, N, a_coeff, b_coeff, number_steps, C_thermal, small_step,
                                 kmc_comm):
    """update_temperatureglobal_gpu (gpu_solvers.h:231; src/heat_solver_gpu.cu:53-70)."""
    lib = _L.load()
    _L.check(lib.kmcf_update_temperature_global(kmc_comm.handle, _ptr(site_power), _ptr(T_bg), int(N),
                                                float(a_coeff), float(b_coeff), float(number_steps),
                                                float(C_thermal), float(small_step)),
             "kmcf_update_temperature_global")


def heat_params(background_temp=300.0, k_th_metal=29.0, k_th_vacancies=5.0, k_th_non_vacancy=0.5, L_char=3.5e-10,
                c_p=1.92, A=51.15e-10 * 51.15e-10, t_ox=52.6838e-10, delta_t=1e-13, cg_tolerance=1e-12,
                cg_max_iterations=20000):
    """kmcf_heat_params_t.  Defaults = the "Local thermal model" block of the 5 nm device's parameters.txt; the
    stopping rule (cg_tolerance, cg_max_iterations) is the library's own (local heat solve)."""
    return _L.HeatParams(float(background_temp), float(k_th_metal), float(k_th_vacancies), float(k_th_non_vacancy),
                         float(L_char), float(c_p), float(A), float(t_ox), float(delta_t), float(cg_tolerance),
                         int(cg_max_iterations))


def update_temperature_local_gpu(gpubuf, N, N_left_tot, N_right_tot, step_time, params, num_metals=None):
    """The solve_heating_local branch of Device::updateTemperature (src/heat_solver.cpp:76-98) as a sparse solve
    (kmcf_update_temperature_local): gpubuf.site_temperature (N doubles, created at background_temp on first use) is
    the previous field on entry and the new one, replicated on every rank, on return; gpubuf.site_power is the source.
    Returns {"Global temperature [K]": T_bg, "steady": bool, "stats": solve statistics}."""
    lib = _L.load()
    if getattr(gpubuf, "site_temperature", None) is None:
        gpubuf.site_temperature = torch.full((gpubuf.N_,), float(params.background_temp), dtype=torch.float64,
                                             device=gpubuf.device)
    nm = gpubuf.num_metal_types_ if num_metals is None else int(num_metals)
    st = _L.SolveStats()
    T_bg = C.c_double(0.0)
    steady = C.c_int(0)
    _L.check(lib.kmcf_update_temperature_local(gpubuf.K_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                               _ptr(gpubuf.metal_types), nm, _ptr(gpubuf.site_power),
                                               _ptr(gpubuf.site_temperature), int(N), int(N_left_tot), int(N_right_tot),
                                               float(step_time), C.byref(params), C.byref(T_bg), C.byref(steady),
                                               C.byref(st)), "kmcf_update_temperature_local")
    gpubuf.T_bg.fill_(T_bg.value)
    return {"Global temperature [K]": T_bg.value, "steady": bool(steady.value), "stats": st.as_dict()}


class RandomNumberGenerator:
    """RandomNumberGenerator of src/random_num.h: std::mt19937 + uniform_real_distribution<double>(0, 1)."""

    def __init__(self, seed=1):
        self.lib = _L.load()
        h = C.c_void_p()
        _L.check(self.lib.kmcf_rng_create(int(seed), C.byref(h)), "kmcf_rng_create")
        self.handle = h

    def setSeed(self, seed):
        self.lib.kmcf_rng_destroy(self.handle)
        h = C.c_void_p()
        _L.check(self.lib.kmcf_rng_create(int(seed), C.byref(h)), "kmcf_rng_create")
        self.handle = h

    def getRandomNumber(self):
        return self.lib.kmcf_rng_next(self.handle)


def site_layers(site_x, layers):
    """KMCProcess::KMCProcess (src/KMCProcess.cpp:33-50): the LAST layer whose [start_x, end_x] holds x."""
    site_x = np.asarray(site_x)
    lay = np.full(len(site_x), 1000, np.int32)
    for j, l in enumerate(layers):
        lay[(l["start_x"] <= site_x) & (site_x <= l["end_x"])] = j
    if lay.max() >= 1000:
        raise ValueError("a site is not inside the device (KMCProcess.cpp:45-48)")
    return lay


RATE_MODES = {"bg": 0, "ekin": 1, "site": 2}     # KMCF_RATE_T_BG, KMCF_RATE_EKIN, KMCF_RATE_T_SITE


def _rate_mode(rate_mode):
    if isinstance(rate_mode, str):
        if rate_mode not in RATE_MODES:
            raise ValueError("rate_mode %r: one of %s or 0 / 1 / 2" % (rate_mode, " | ".join(RATE_MODES)))
        return RATE_MODES[rate_mode]
    return int(rate_mode)


def _layer_energies(layers):
    return [_da([l[key] for l in layers]) for key in ("E_gen_0", "E_rec_1", "E_diff_2", "E_diff_3")]


def execute_kmc_step_mpi(kmc_comm, N, count, displs, nn, neigh_idx, site_layer, T_bg, freq, sigma, k, posx, posy, posz,
                         site_potential_charge, site_element, site_charge, rng, layers, max_events=1 << 20,
                         return_log=False, site_temperature=None, rate_mode="bg"):
    """execute_kmc_step_mpi (gpu_solvers.h:250; src/kmc_events.cu:333-563).  T_bg, freq, sigma, k are host
    scalars here.  layers: list of dicts with E_gen_0, E_rec_1, E_diff_2, E_diff_3 (copytoConstMemory).
    Returns the event time (and, with return_log, the number of events and their (i, j, type) rows).
    site_temperature (N doubles on the device, e.g. gpubuf.site_temperature after update_temperature_local_gpu) with
    rate_mode "ekin" | "site" (or 1 | 2): thermally coupled rates, kmcf_execute_kmc_step_thermal.  The defaults
    ("bg", no field) are kmcf_execute_kmc_step.
    The library keeps its verdict on a neighbour list per address: after writing into neigh_idx in place, or when a new list
    may sit where torch's caching allocator freed an old one, call events_reset(kmc_comm) before the next step."""
    lib = _L.load()
    mode = _rate_mode(rate_mode)
    cnt, cntp = _ia(count)
    dsp, dspp = _ia(displs)
    (eg, egp), (er, erp), (ev, evp), (eo, eop) = _layer_energies(layers)
    t = C.c_double()
    nev = C.c_int()
    cap = min(int(max_events), 1 << 16) if return_log else 0
    log = np.zeros(max(3 * cap, 1), np.int32)
    if callable(rng):
        # any uniform [0, 1) source, like the reference's RandomNumberGenerator& (one host round trip per event:
        # a foreign generator cannot be drawn ahead and rewound)
        keep = C.CFUNCTYPE(C.c_double, C.c_void_p)(lambda _user: float(rng()))
        fn, user = C.cast(keep, C.c_void_p), None
    else:
        fn, user = C.cast(lib.kmcf_rng_next, C.c_void_p), rng.handle
    args = (kmc_comm.handle, int(N), cntp, dspp, int(nn), _ptr(neigh_idx), _ptr(site_layer),
            float(T_bg), float(freq), float(sigma), float(k), _ptr(posx), _ptr(posy),
            _ptr(posz), _ptr(site_potential_charge), _ptr(site_element), _ptr(site_charge),
            len(layers), egp, erp, evp, eop, fn, user,
            cap if return_log else int(max_events), C.byref(t), C.byref(nev),
            log.ctypes.data_as(C.POINTER(C.c_int)) if return_log else None)
    if mode == 0 and site_temperature is None:
        _L.check(lib.kmcf_execute_kmc_step(*args), "kmcf_execute_kmc_step")
    else:
        _L.check(lib.kmcf_execute_kmc_step_thermal(*args, _ptr(site_temperature), mode), "kmcf_execute_kmc_step_thermal")
    if return_log:
        return t.value, nev.value, log[:3 * nev.value].reshape(-1, 3).copy()
    return t.value


def events_reset(kmc_comm):
    """kmcf_events_reset: drop the event step's workspace, the symmetry verdict of the neighbour list and a replicated
    group's gathered lists; the next step works them out again.  In a group: every rank, between the same two steps."""
    _L.check(_L.load().kmcf_events_reset(kmc_comm.handle), "kmcf_events_reset")


def events_set_lattice(kmc_comm, lattice, pbc):
    """kmcf_events_set_lattice: the pair distance of the event rates on this communicator from now on -- pbc = 1: minimum
    image in y and z with the periods lattice[1], lattice[2]; pbc = 0 (lattice may be None): the open-boundary default.
    events_reset does not clear it.  In a group: every rank alike."""
    latp = None
    if lattice is not None:
        lat, latp = _da(lattice)
    _L.check(_L.load().kmcf_events_set_lattice(kmc_comm.handle, latp, int(pbc)), "kmcf_events_set_lattice")


def event_rates(kmc_comm, N, count, displs, nn, neigh_idx, site_layer, T_bg, freq, sigma, k, posx, posy, posz,
                site_potential_charge, site_element, site_charge, layers, site_temperature=None, rate_mode="bg"):
    """kmcf_event_rates: the event list the step would build for this rank's rows, nothing executed.  Returns (type, prob): uint8 EVENTTYPE codes and float64 rates,
    both of shape (count[rank], nn)."""
    lib = _L.load()
    cnt, cntp = _ia(count)
    dsp, dspp = _ia(displs)
    (eg, egp), (er, erp), (ev, evp), (eo, eop) = _layer_energies(layers)
    rows = int(cnt[kmc_comm.rank_events])
    typ = np.zeros((rows, int(nn)), np.uint8)
    prob = np.zeros((rows, int(nn)), np.float64)
    _L.check(lib.kmcf_event_rates(kmc_comm.handle, int(N), cntp, dspp, int(nn), _ptr(neigh_idx), _ptr(site_layer),
                                  float(T_bg), float(freq), float(sigma), float(k), _ptr(posx), _ptr(posy), _ptr(posz),
                                  _ptr(site_potential_charge), _ptr(site_element), _ptr(site_charge), len(layers),
                                  egp, erp, evp, eop, _ptr(site_temperature), _rate_mode(rate_mode),
                                  typ.ctypes.data_as(C.POINTER(C.c_ubyte)), prob.ctypes.data_as(C.POINTER(C.c_double))),
             "kmcf_event_rates")
    return typ, prob


CENSUS_DTYPE = np.dtype([("n_events", np.int64), ("rate_sum", np.float64), ("rate_max", np.float64), ("max_i", np.int32),
                         ("max_j", np.int32), ("n_zero", np.int32), ("reserved", np.int32)])      # kmcf_census_bucket_t
EVENT_NAMES = ("gen", "rec", "vdiff", "odiff")      # EVENTTYPE 0..3


def event_census(kmc_comm, N, count, displs, nn, neigh_idx, site_layer, T_bg, freq, sigma, k, posx, posy, posz,
                 site_potential_charge, site_element, site_charge, layers, site_temperature=None, rate_mode="bg",
                 site_cell=None, n_cells=1, bins=(64, -128, 16), rows=False):
    """kmcf_event_census: the event list of this rank's rows (the one event_rates returns) reduced on the device to rates
    per cell, layer and event type; nothing executed, nothing drawn (definitions: include/kmcfield.h).  site_cell: int32
    device tensor of N cell ids (outside [0, n_cells): the rest, cell index n_cells) or None with n_cells = 1.
    bins = (n_bins, e_lo, e_step): the spectrum of the rates' binary exponents, None or n_bins = 0 for none.  rows: also
    the sum and the best slot per row, as device tensors.
    Returns dict(table: CENSUS_DTYPE array of shape (n_cells + 1, num_layers, 4), spectrum: int64 (4, n_bins) or None,
    row_rate / row_best: float64 / int32 device tensors of count[rank] entries or None, stats: dict)."""
    lib = _L.load()
    cnt, cntp = _ia(count)
    dsp, dspp = _ia(displs)
    (eg, egp), (er, erp), (ev, evp), (eo, eop) = _layer_energies(layers)
    n_rows = int(cnt[kmc_comm.rank_events])
    n_bins, e_lo, e_step = (0, 0, 1) if bins is None else (int(b) for b in bins)
    table = np.zeros((int(n_cells) + 1, len(layers), 4), CENSUS_DTYPE)
    spectrum = np.zeros((4, n_bins), np.int64) if n_bins > 0 else None
    row_rate = row_best = None
    if rows:
        dev = neigh_idx.device
        row_rate = torch.empty(n_rows, dtype=torch.float64, device=dev)
        row_best = torch.empty(n_rows, dtype=torch.int32, device=dev)
    st = _L.CensusStats()
    _L.check(lib.kmcf_event_census(kmc_comm.handle, int(N), cntp, dspp, int(nn), _ptr(neigh_idx), _ptr(site_layer),
                                   float(T_bg), float(freq), float(sigma), float(k), _ptr(posx), _ptr(posy), _ptr(posz),
                                   _ptr(site_potential_charge), _ptr(site_element), _ptr(site_charge), len(layers),
                                   egp, erp, evp, eop, _ptr(site_temperature), _rate_mode(rate_mode),
                                   _ptr(site_cell), int(n_cells), table.ctypes.data_as(C.POINTER(_L.CensusBucket)),
                                   n_bins, e_lo, e_step,
                                   spectrum.ctypes.data_as(C.POINTER(C.c_int64)) if spectrum is not None else None,
                                   _ptr(row_rate), _ptr(row_best), C.byref(st)),
             "kmcf_event_census")
    return dict(table=table, spectrum=spectrum, row_rate=row_rate, row_best=row_best, stats=st.as_dict())


def census_stats_from_table(table):
    """The statistics kmcf_event_census forms from its table, by the header's formulas: integer sums, rate_type[t] over cell
    ascending then layer ascending from 0.0, rate_total = ((r0 + r1) + r2) + r3, dt_mean (the overall maximum needs the
    slots of the maxima and is not formed here)."""
    n_type, rate_type = [0] * 4, [0.0] * 4
    for t in range(4):
        r = 0.0
        for c in range(table.shape[0]):
            for l in range(table.shape[1]):
                r += float(table[c, l, t]["rate_sum"])
        rate_type[t] = r
        n_type[t] = int(table[:, :, t]["n_events"].sum())
    total = ((rate_type[0] + rate_type[1]) + rate_type[2]) + rate_type[3]
    return dict(n_type=n_type, rate_type=rate_type, n_events=int(table["n_events"].sum()), n_zero=int(table["n_zero"].sum()),
                rate_total=total, dt_mean=float("inf") if total == 0 else 1 / total)


def event_census_merge(results):
    """The host combination of the censuses of a partitioned group's ranks (or of (count, displ) slices), in list order =
    ascending rows: integers add, sums add in list order, a maximum goes to the larger rate and among equal rates stays
    with the earlier result (its slot id is the smaller one).  Row outputs are concatenated.  Returns a result dict like
    event_census; stats are formed from the merged table, ms_build / ms_census add up."""
    results = list(results)
    first = results[0]
    table = first["table"].copy()
    spectrum = None if first["spectrum"] is None else first["spectrum"].copy()
    best = dict(rate_max=first["stats"]["rate_max"], max_i=first["stats"]["max_i"], max_j=first["stats"]["max_j"],
                max_type=first["stats"]["max_type"])
    for r in results[1:]:
        t = r["table"]
        table["n_events"] += t["n_events"]
        table["n_zero"] += t["n_zero"]
        table["rate_sum"] = table["rate_sum"] + t["rate_sum"]
        take = (t["max_i"] >= 0) & ((table["max_i"] < 0) | (t["rate_max"] > table["rate_max"]))
        for f in ("rate_max", "max_i", "max_j"):
            table[f] = np.where(take, t[f], table[f])
        if spectrum is not None:
            spectrum += r["spectrum"]
        s = r["stats"]
        if s["max_i"] >= 0 and (best["max_i"] < 0 or s["rate_max"] > best["rate_max"]):
            best = dict(rate_max=s["rate_max"], max_i=s["max_i"], max_j=s["max_j"], max_type=s["max_type"])
    stats = census_stats_from_table(table)
    stats.update(best)
    for key in ("slots", "n_nan", "rows_live", "ms_build", "ms_census"):
        stats[key] = sum(r["stats"][key] for r in results)

    def cat(key):
        parts = [r[key] for r in results]
        if any(p is None for p in parts):
            return None
        return torch.cat(parts) if isinstance(parts[0], torch.Tensor) else np.concatenate(parts)

    return dict(table=table, spectrum=spectrum, row_rate=cat("row_rate"), row_best=cat("row_best"), stats=stats)


# K-state inspection helpers used by the parity tests --------------------------------

CLUSTER_DTYPE = np.dtype([("root", np.int32), ("kind", np.int32), ("size", np.int32), ("touch", np.int32),
                          ("x_min", np.float64), ("x_max", np.float64)])      # kmcf_cluster_t


def conductive_clusters(kmc_comm, gpubuf, N_left_tot, N_right_tot, labels=True):
    """kmcf_conductive_clusters on the buffers' whole-device neighbour list: connected components of the metal sites and
    of the uncharged vacancies under the high_G rule (definitions: include/kmcfield.h).  Call it after
    update_charge_gpu.  Returns dict(label: int32 device tensor of N entries (-1: no member) or None, clusters: numpy
    structured array (root, kind, size, touch, x_min, x_max) sorted by root, stats: dict).  Two calls: the count, then
    the table."""
    lib = _L.load()
    N = gpubuf.N_
    assert gpubuf.neigh_idx is not None and gpubuf.neigh_idx.numel() == N * gpubuf.nn_, \
        "conductive_clusters needs the neighbour list of the whole device"
    label = torch.empty(N, dtype=torch.int32, device=gpubuf.device) if labels else None
    st = _L.ClusterStats()
    head = (kmc_comm.handle, N, gpubuf.nn_, _ptr(gpubuf.neigh_idx), _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
            _ptr(gpubuf.metal_types), gpubuf.num_metal_types_, _ptr(gpubuf.site_x), int(N_left_tot), int(N_right_tot))
    _L.check(lib.kmcf_conductive_clusters(*head, _ptr(label), None, 0, C.byref(st)), "kmcf_conductive_clusters")
    table = np.zeros(st.n_clusters, CLUSTER_DTYPE)
    if st.n_clusters:
        ms_count = st.ms
        _L.check(lib.kmcf_conductive_clusters(*head, _ptr(label), table.ctypes.data_as(C.POINTER(_L.Cluster)), len(table),
                                              C.byref(st)), "kmcf_conductive_clusters")
        assert st.n_clusters == len(table)
        st.ms += ms_count
    return dict(label=label, clusters=table, stats=st.as_dict())


GAP_DTYPE = np.dtype([("gap", np.float64), ("gap2", np.float64), ("x_left", np.float64), ("x_right", np.float64),
                      ("site_left", np.int32), ("site_right", np.int32), ("n_left", np.int32), ("n_right", np.int32),
                      ("n_both", np.int32), ("bridged", np.int32)])           # kmcf_gap_t


def _gap_cells(gpubuf, site_cell, n_cells):
    if site_cell is None:
        assert n_cells == 1, "n_cells = %d needs site_cell" % n_cells
        return None
    if not torch.is_tensor(site_cell):
        site_cell = torch.as_tensor(np.ascontiguousarray(site_cell, dtype=np.int32), device=gpubuf.device)
    assert site_cell.dtype == torch.int32 and site_cell.numel() == gpubuf.N_, "site_cell: N int32 entries"
    return site_cell


def site_set_gap(gpubuf, site_side, r_max, site_cell=None, n_cells=1, periodic=False):
    """kmcf_site_set_gap on the buffers' spatial index (gpubuf.cutoff_idx, compute_cutoff_list): per gap cell the nearest
    pair (a, b) of the sites with side bit 0 and the sites with side bit 1 within r_max (definitions:
    include/kmcfield.h).  site_side: int32 device tensor of N entries; site_cell: int32 tensor or array of N entries
    (values outside [0, n_cells): no cell), or None with n_cells == 1.  periodic=True: kmcf_site_set_gap_pbc, which takes
    the minimum image in y and z on a periodic index (compute_cutoff_list with pbc = 1) and is the plain call on any
    other; the default refuses a periodic index.  Returns dict(gaps: numpy structured array GAP_DTYPE of n_cells
    records, stats: dict)."""
    assert gpubuf.cutoff_idx is not None, "site_set_gap needs the spatial index: compute_cutoff_list first"
    assert site_side.dtype == torch.int32 and site_side.numel() == gpubuf.N_, "site_side: N int32 entries"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    gaps = np.zeros(int(n_cells), GAP_DTYPE)
    st = _L.GapStats()
    name = "kmcf_site_set_gap_pbc" if periodic else "kmcf_site_set_gap"
    _L.check(getattr(_L.load(), name)(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                      _ptr(site_side), float(r_max), _ptr(cell), int(n_cells),
                                      gaps.ctypes.data_as(C.POINTER(_L.Gap)), C.byref(st)), name)
    return dict(gaps=gaps, stats=st.as_dict())


def filament_gap(kmc_comm, gpubuf, N_left_tot, N_right_tot, r_max, site_cell=None, n_cells=1, bins=None, sides=True,
                 periodic=False):
    """kmcf_filament_gap: how close the conductive matter attached to the left electrode comes to the matter attached to
    the right one, per gap cell (definitions: include/kmcfield.h).  Call it after update_charge_gpu and
    compute_cutoff_list, on the communicator the index was built with.  bins: None or (n_bins, x_lo, x_hi) for the
    profile of the conductive vacancies along x.  periodic=True: kmcf_filament_gap_pbc -- the minimum image in y and z on
    a periodic index (compute_cutoff_list with pbc = 1; build the list with compute_neighbor_list(pbc=1) as well, so that
    the clusters wrap too), the plain call on any other; the default refuses a periodic index.  Returns dict(gaps: numpy
    structured array GAP_DTYPE of n_cells records, profile: int32 array (n_cells, n_bins, 3) -- last axis: side 1, 2, 3 -- or None, side: int32 device tensor of N
    entries or None, stats: dict)."""
    N = gpubuf.N_
    assert gpubuf.cutoff_idx is not None, "filament_gap needs the spatial index: compute_cutoff_list first"
    assert gpubuf.neigh_idx is not None and gpubuf.neigh_idx.numel() == N * gpubuf.nn_, \
        "filament_gap needs the neighbour list of the whole device"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    gaps = np.zeros(int(n_cells), GAP_DTYPE)
    n_bins, x_lo, x_hi = (int(bins[0]), float(bins[1]), float(bins[2])) if bins is not None else (0, 0.0, 0.0)
    profile = np.zeros((int(n_cells), n_bins, 3), np.int32) if bins is not None else None
    side = torch.empty(N, dtype=torch.int32, device=gpubuf.device) if sides else None
    st = _L.GapStats()
    name = "kmcf_filament_gap_pbc" if periodic else "kmcf_filament_gap"
    _L.check(getattr(_L.load(), name)(gpubuf.cutoff_idx, gpubuf.nn_, _ptr(gpubuf.neigh_idx), _ptr(gpubuf.site_element),
                                      _ptr(gpubuf.site_charge), _ptr(gpubuf.metal_types), gpubuf.num_metal_types_,
                                      _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z), int(N_left_tot),
                                      int(N_right_tot), float(r_max), _ptr(cell), int(n_cells),
                                      gaps.ctypes.data_as(C.POINTER(_L.Gap)), n_bins, x_lo, x_hi,
                                      profile.ctypes.data_as(C.POINTER(C.c_int)) if profile is not None else None,
                                      _ptr(side), C.byref(st)), name)
    return dict(gaps=gaps, profile=profile, side=side, stats=st.as_dict())


CHAIN_DTYPE = np.dtype([("hop_max", np.float64), ("hop_max2", np.float64), ("length", np.float64), ("direct2", np.float64),
                        ("status", np.int32), ("n_hops", np.int32), ("neck_from", np.int32), ("neck_to", np.int32),
                        ("n_stones", np.int32), ("n_stone_sites", np.int32), ("n_left", np.int32),
                        ("n_right", np.int32)])                                # kmcf_chain_t
HOP_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("d2", np.float64)])   # kmcf_hop_t
CHAIN_NONE, CHAIN_OPEN, CHAIN_CHAINED, CHAIN_BRIDGED = 0, 1, 2, 3


def _chain_out(n_cells, max_hops):
    chains = np.zeros(int(n_cells), CHAIN_DTYPE)
    hops = np.zeros((int(n_cells), int(max_hops)), HOP_DTYPE) if max_hops else None
    return chains, hops, (hops.ctypes.data_as(C.POINTER(_L.Hop)) if hops is not None else None)


def site_set_chain(gpubuf, site_side, site_node, r_max, site_cell=None, n_cells=1, max_hops=0, periodic=False):
    """kmcf_site_set_chain on the buffers' spatial index (gpubuf.cutoff_idx, compute_cutoff_list): per gap cell the chain
    of hops from the sites with side bit 0 to the sites with side bit 1 through the floating bodies of site_node whose
    largest hop is as small as any chain's (definitions: include/kmcfield.h).  site_side, site_node: int32 device tensors
    of N entries (a node outside [0, N): none); site_cell as in site_set_gap.  periodic=True: kmcf_site_set_chain_pbc, which
    takes the minimum image in y and z on a periodic index (compute_cutoff_list with pbc = 1) and is the plain call on any
    other; the default refuses a periodic index.  Returns dict(chains: numpy structured array CHAIN_DTYPE of n_cells
    records, hops: HOP_DTYPE array (n_cells, max_hops) or None with max_hops == 0, stats: dict)."""
    assert gpubuf.cutoff_idx is not None, "site_set_chain needs the spatial index: compute_cutoff_list first"
    for name, t in (("site_side", site_side), ("site_node", site_node)):
        assert t.dtype == torch.int32 and t.numel() == gpubuf.N_, name + ": N int32 entries"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    chains, hops, hp = _chain_out(n_cells, max_hops)
    st = _L.ChainStats()
    name = "kmcf_site_set_chain_pbc" if periodic else "kmcf_site_set_chain"
    _L.check(getattr(_L.load(), name)(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                      _ptr(site_side), _ptr(site_node), float(r_max), _ptr(cell), int(n_cells),
                                      chains.ctypes.data_as(C.POINTER(_L.Chain)), hp, int(max_hops), C.byref(st)), name)
    return dict(chains=chains, hops=hops, stats=st.as_dict())


def filament_chain(kmc_comm, gpubuf, N_left_tot, N_right_tot, r_max, site_cell=None, n_cells=1, max_hops=0, sides=True,
                   nodes=True, periodic=False):
    """kmcf_filament_chain: the stepping-stone chain between the matter attached to the left electrode and the matter
    attached to the right one through the floating conductive clusters, per gap cell (definitions: include/kmcfield.h).
    Call it after update_charge_gpu and compute_cutoff_list, on the communicator the index was built with.
    periodic=True: kmcf_filament_chain_pbc -- the minimum image in y and z on a periodic index (compute_cutoff_list with
    pbc = 1; build the list with compute_neighbor_list(pbc=1) as well, so that a body that passes a face is one node), the
    plain call on any other; the default refuses a periodic index.  Returns dict(chains, hops (or None), side / node:
    int32 device tensors of N entries or None, stats: dict)."""
    N = gpubuf.N_
    assert gpubuf.cutoff_idx is not None, "filament_chain needs the spatial index: compute_cutoff_list first"
    assert gpubuf.neigh_idx is not None and gpubuf.neigh_idx.numel() == N * gpubuf.nn_, \
        "filament_chain needs the neighbour list of the whole device"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    chains, hops, hp = _chain_out(n_cells, max_hops)
    side = torch.empty(N, dtype=torch.int32, device=gpubuf.device) if sides else None
    node = torch.empty(N, dtype=torch.int32, device=gpubuf.device) if nodes else None
    st = _L.ChainStats()
    name = "kmcf_filament_chain_pbc" if periodic else "kmcf_filament_chain"
    _L.check(getattr(_L.load(), name)(gpubuf.cutoff_idx, gpubuf.nn_, _ptr(gpubuf.neigh_idx), _ptr(gpubuf.site_element),
                                      _ptr(gpubuf.site_charge), _ptr(gpubuf.metal_types), gpubuf.num_metal_types_,
                                      _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z), int(N_left_tot),
                                      int(N_right_tot), float(r_max), _ptr(cell), int(n_cells),
                                      chains.ctypes.data_as(C.POINTER(_L.Chain)), hp, int(max_hops), _ptr(side), _ptr(node),
                                      C.byref(st)), name)
    return dict(chains=chains, hops=hops, side=side, node=node, stats=st.as_dict())


GRADIENT_CELL_DTYPE = np.dtype([("n_sites", np.int32), ("n_full", np.int32), ("g_max", np.float64), ("g_site", np.int32),
                                ("drop_max", np.float64), ("drop_from", np.int32), ("drop_to", np.int32)],
                               align=True)                                     # kmcf_gradient_cell_t


def site_gradient(kmc_comm, gpubuf, value, mask=None, site_cell=None, n_cells=1, periodic=False, nn=None):
    """kmcf_site_gradient on the buffers' whole-device neighbour list: per site the least-squares gradient of `value` over
    the counted pairs of its row and the largest bond drop, with the maxima per cell (definitions: include/kmcfield.h).
    value: N doubles on the device; mask: int32 device tensor of N entries (0: the site is left out) or None; site_cell:
    int32 tensor or array of N entries (values outside [0, n_cells): no cell), or None with n_cells == 1.  periodic=True:
    the minimum image in y and z with the periods of gpubuf.lattice_host (build the list with compute_neighbor_list(pbc=1)
    as well).  nn: slots per row of gpubuf.neigh_idx (default gpubuf.nn_).  Returns dict(gx, gy, gz, drop: N doubles,
    drop_to, full: N int32, all on the device; cells: numpy structured array GRADIENT_CELL_DTYPE of n_cells records;
    stats: dict)."""
    N = gpubuf.N_
    nn = gpubuf.nn_ if nn is None else int(nn)
    assert gpubuf.neigh_idx is not None and gpubuf.neigh_idx.numel() == N * nn, \
        "site_gradient needs the neighbour list of the whole device (N * nn entries)"
    assert value.dtype == torch.float64 and value.numel() == N, "value: N doubles"
    assert mask is None or (mask.dtype == torch.int32 and mask.numel() == N), "mask: N int32 entries"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    f64 = dict(dtype=torch.float64, device=gpubuf.device)
    i32 = dict(dtype=torch.int32, device=gpubuf.device)
    gx, gy, gz, drop = (torch.empty(N, **f64) for _ in range(4))
    drop_to, full = torch.empty(N, **i32), torch.empty(N, **i32)
    cells = np.zeros(int(n_cells), GRADIENT_CELL_DTYPE)
    st = _L.GradientStats()
    lat, latp = _da(gpubuf.lattice_host)
    _L.check(_L.load().kmcf_site_gradient(kmc_comm.handle, N, nn, _ptr(gpubuf.neigh_idx), _ptr(gpubuf.site_x),
                                          _ptr(gpubuf.site_y), _ptr(gpubuf.site_z), latp, 1 if periodic else 0, _ptr(value),
                                          _ptr(mask), _ptr(cell), int(n_cells), _ptr(gx), _ptr(gy), _ptr(gz), _ptr(drop),
                                          _ptr(drop_to), _ptr(full), cells.ctypes.data_as(C.POINTER(_L.GradientCell)),
                                          C.byref(st)), "kmcf_site_gradient")
    return dict(gx=gx, gy=gy, gz=gz, drop=drop, drop_to=drop_to, full=full, cells=cells, stats=st.as_dict())


def field_map(kmc_comm, gpubuf, potential=None, mask=None, site_cell=None, n_cells=1, periodic=False, nn=None):
    """The electric field at every site: site_gradient of the site potential the events read -- site_potential_boundary +
    site_potential_charge (background_potential_gpu_sparse and poisson_gridless_gpu first), or `potential` (N doubles on
    the device) -- and E = -g.  Returns site_gradient's dict with Ex, Ey, Ez (N doubles on the device) and `potential`
    added; g_max in cells and stats is the largest |E|, drop the largest potential difference per length of a bond."""
    pot = gpubuf.site_potential_boundary + gpubuf.site_potential_charge if potential is None else potential
    out = site_gradient(kmc_comm, gpubuf, pot, mask=mask, site_cell=site_cell, n_cells=n_cells, periodic=periodic, nn=nn)
    out.update(Ex=-out["gx"], Ey=-out["gy"], Ez=-out["gz"], potential=pot)
    return out


PC_MAX_CLASSES, PC_MAX_BINS = 4, 256           # KMCF_PC_MAX_CLASSES, KMCF_PC_MAX_BINS
DEFECT_CLASSES = ("V0", "V+", "ion")           # the classes of kmcf_defect_correlation; 3: probe


def _pair_out(n_classes, n_bins, n_cells, r_max, r_count, counts, gpubuf):
    n_pairs = n_classes * (n_classes + 1) // 2
    hist = np.zeros((int(n_cells) + 1, n_pairs, int(n_bins)), np.uint64)
    members = np.zeros((int(n_cells) + 1, n_classes), np.int32)
    edge2 = np.zeros(int(n_bins) + 1, np.float64)
    cnt = torch.empty((gpubuf.N_, n_classes), dtype=torch.int32, device=gpubuf.device) if counts else None
    return hist, members, edge2, cnt, float(r_max if r_count is None else r_count)


def _pair_result(hist, members, edge2, r_max, n_bins, cnt, st, **more):
    edges = float(r_max) * np.arange(int(n_bins) + 1, dtype=np.float64) / float(int(n_bins))
    return dict(hist=hist, members=members, edge2=edge2, edges=edges, counts=cnt, stats=st.as_dict(), **more)


def pair_correlation(gpubuf, site_class, n_classes, r_max, n_bins, r_count=None, site_cell=None, n_cells=1, counts=False):
    """kmcf_pair_correlation on the buffers' spatial index (gpubuf.cutoff_idx, compute_cutoff_list; open or periodic: the
    distance is the index's own): per bucket and class pair the histogram of the pair distances up to r_max, the members
    per cell and class, and (counts=True) per centre the members of every class within r_count (default r_max)
    (definitions: include/kmcfield.h).  site_class: int32 device tensor of N entries -- [0, n_classes) member, n_classes
    probe, anything else no part; site_cell as in site_set_gap.  Returns dict(hist: uint64 (n_cells + 1, n_pairs, n_bins),
    members: int32 (n_cells + 1, n_classes), edge2: the table of squared bin edges, edges: r_max * k / n_bins, counts:
    int32 device tensor (N, n_classes) or None, stats: dict)."""
    assert gpubuf.cutoff_idx is not None, "pair_correlation needs the spatial index: compute_cutoff_list first"
    assert site_class.dtype == torch.int32 and site_class.numel() == gpubuf.N_, "site_class: N int32 entries"
    assert 1 <= int(n_classes) <= PC_MAX_CLASSES and 1 <= int(n_bins) <= PC_MAX_BINS
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    hist, members, edge2, cnt, r_count = _pair_out(int(n_classes), n_bins, n_cells, r_max, r_count, counts, gpubuf)
    st = _L.PairStats()
    _L.check(_L.load().kmcf_pair_correlation(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                             _ptr(site_class), int(n_classes), float(r_max), int(n_bins), r_count, _ptr(cell),
                                             int(n_cells), hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                             members.ctypes.data_as(C.POINTER(C.c_int)),
                                             edge2.ctypes.data_as(C.POINTER(C.c_double)), _ptr(cnt), C.byref(st)),
             "kmcf_pair_correlation")
    return _pair_result(hist, members, edge2, r_max, n_bins, cnt, st)


def defect_correlation(kmc_comm, gpubuf, r_max, n_bins, r_count=None, site_cell=None, n_cells=1, counts=False, probe_all=False,
                       classes=False):
    """kmcf_defect_correlation: pair_correlation with the three classes of DEFECT_CLASSES taken from gpubuf.site_element
    and gpubuf.site_charge -- neutral vacancies, charged vacancies, oxygen ions; probe_all: every other site is a probe (a
    centre of the counts), otherwise it takes no part.  Call it after update_charge_gpu and compute_cutoff_list, on the
    communicator the index was built with.  classes=True: also returns the classes as formed (`site_class`, int32 device
    tensor of N entries).  Returns pair_correlation's dict."""
    assert gpubuf.cutoff_idx is not None, "defect_correlation needs the spatial index: compute_cutoff_list first"
    cell = _gap_cells(gpubuf, site_cell, n_cells)
    hist, members, edge2, cnt, r_count = _pair_out(3, n_bins, n_cells, r_max, r_count, counts, gpubuf)
    cls = torch.empty(gpubuf.N_, dtype=torch.int32, device=gpubuf.device) if classes else None
    st = _L.PairStats()
    _L.check(_L.load().kmcf_defect_correlation(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z),
                                               _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge), 1 if probe_all else 0,
                                               float(r_max), int(n_bins), r_count, _ptr(cell), int(n_cells),
                                               hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               members.ctypes.data_as(C.POINTER(C.c_int)),
                                               edge2.ctypes.data_as(C.POINTER(C.c_double)), _ptr(cnt), _ptr(cls), C.byref(st)),
             "kmcf_defect_correlation")
    return _pair_result(hist, members, edge2, r_max, n_bins, cnt, st, site_class=cls)


def pair_class_index(p, q, n_classes):
    """index of the class pair {p, q} in the histogram's second axis"""
    p, q = min(p, q), max(p, q)
    return p * n_classes - p * (p - 1) // 2 + (q - p)


def pair_rdf(result, volume):
    """The pair distribution g(r) of a pair_correlation result against a random arrangement, host-only numpy: per cell
    c < n_cells, class pair and bin, hist / (n_pq * shell_k / volume) with n_pq = N_p N_q for p != q and N_p (N_p - 1) / 2
    for p == q (N_p: the cell's members of class p), shell_k = 4/3 pi (e[k+1]^3 - e[k]^3); nan where n_pq == 0.  volume:
    a cell's volume (a number, or one per cell).  Returns float64 (n_cells, n_pairs, n_bins)."""
    hist, members, e = np.asarray(result["hist"]), np.asarray(result["members"]), np.asarray(result["edges"], np.float64)
    n_cells, n_classes = hist.shape[0] - 1, members.shape[1]
    shell = 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
    vol = np.broadcast_to(np.asarray(volume, np.float64), (n_cells,))
    out = np.full((n_cells,) + hist.shape[1:], np.nan)
    for c in range(n_cells):
        for p in range(n_classes):
            for q in range(p, n_classes):
                n_pq = float(members[c, p]) * float(members[c, q]) if p != q else float(members[c, p]) * (float(members[c, p]) - 1.0) / 2.0
                if n_pq > 0:
                    k = pair_class_index(p, q, n_classes)
                    out[c, k] = hist[c, k].astype(np.float64) / (n_pq * shell / vol[c])
    return out


FS_MAX_FIELDS = 8                              # KMCF_FS_MAX_FIELDS


def _fs_inputs(gpubuf, values, mask, radius):
    """(values as a contiguous (n_fields, N) double tensor or None, n_fields, mask, radius) of field_sample / field_grid"""
    assert gpubuf.cutoff_idx is not None, "field sampling needs the spatial index: compute_cutoff_list first"
    N = gpubuf.N_
    if values is not None:
        if not torch.is_tensor(values):
            values = torch.as_tensor(np.ascontiguousarray(values, dtype=np.float64), device=gpubuf.device)
        values = values.reshape(-1, N).contiguous()
        assert values.dtype == torch.float64 and 1 <= values.shape[0] <= FS_MAX_FIELDS, "values: 1 ... 8 rows of N doubles"
    if mask is not None:
        if not torch.is_tensor(mask):
            mask = torch.as_tensor(np.ascontiguousarray(mask, dtype=np.int32), device=gpubuf.device)
        assert mask.dtype == torch.int32 and mask.numel() == N, "mask: N int32 entries"
    if radius is None:
        assert getattr(gpubuf, "cutoff_radius", None) is not None, \
            "radius=None takes the index's cutoff radius, which compute_cutoff_list records: pass radius= for an index attached otherwise"
        radius = gpubuf.cutoff_radius
    radius = float(radius)
    return values, 0 if values is None else int(values.shape[0]), mask, radius


def _fs_outputs(gpubuf, n_fields, n):
    dev = gpubuf.device
    return (torch.empty((n_fields, n), dtype=torch.float64, device=dev) if n_fields else None,
            torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
            torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev))


def field_sample(gpubuf, points, values=None, mask=None, radius=None, normalize=True, fill=float("nan")):
    """kmcf_field_sample on the buffers' spatial index (gpubuf.cutoff_idx, compute_cutoff_list; open or periodic: the
    distance is the index's own): the site fields `values` ((n_fields, N) or (N,) doubles, tensor or array; None: no field)
    at the points ((n_points, 3) doubles, tensor or array), gathered from the sites with mask != 0 (all with mask None)
    within `radius` (default: the index's cutoff) with the weight (1 - d2 / radius^2)^2 (definitions: include/kmcfield.h).
    normalize: the weighted mean, `fill` where no weight was met; otherwise the raw weighted sum (sample_density).
    Returns dict(out: (n_fields, n_points) doubles or None, wsum, count (int32), nearest (int32 site id, -1 none),
    nearest_d2, stats: dict), the arrays on the device."""
    values, n_fields, mask, radius = _fs_inputs(gpubuf, values, mask, radius)
    if not torch.is_tensor(points):
        points = torch.as_tensor(np.ascontiguousarray(points, dtype=np.float64), device=gpubuf.device)
    assert points.dtype == torch.float64 and points.dim() == 2 and points.shape[1] == 3, "points: (n_points, 3) doubles"
    n = int(points.shape[0])
    px, py, pz = (points[:, k].contiguous() for k in range(3))
    out, wsum, count, nearest, nd2 = _fs_outputs(gpubuf, n_fields, n)
    st = _L.SampleStats()
    nz = lambda t: _ptr(t) if n else None
    _L.check(_L.load().kmcf_field_sample(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z), _ptr(mask),
                                         n_fields, _ptr(values), n, nz(px), nz(py), nz(pz), radius, 1 if normalize else 0,
                                         float(fill), _ptr(out), _ptr(wsum), _ptr(count), _ptr(nearest), _ptr(nd2), C.byref(st)),
             "kmcf_field_sample")
    return dict(out=out, wsum=wsum, count=count, nearest=nearest, nearest_d2=nd2, radius=radius, stats=st.as_dict())


def field_grid(gpubuf, origin, spacing, dims, values=None, mask=None, radius=None, normalize=True, fill=float("nan"), labels=None):
    """kmcf_field_grid: field_sample on the points origin + (i, j, k) * spacing of a grid of dims = (nx, ny, nz) voxels
    (spacing: three numbers or one).  Returns field_sample's dict with the arrays shaped (n_fields, nx, ny, nz) and
    (nx, ny, nz), and origin, spacing, dims; labels (an int32 site array: element, cluster label, cell id): also
    `labels` = labels[nearest], -1 where a voxel has no site within radius."""
    values, n_fields, mask, radius = _fs_inputs(gpubuf, values, mask, radius)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(origin, np.float64), (3,)))
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(spacing, np.float64), (3,)))
    d = np.ascontiguousarray(np.asarray(dims, np.int32).reshape(3))
    n = int(np.prod(d.astype(np.int64)))
    assert (d >= 1).all() and n < 2 ** 31, "dims: three counts >= 1 with a product below 2^31"
    out, wsum, count, nearest, nd2 = _fs_outputs(gpubuf, n_fields, n)
    st = _L.SampleStats()
    _L.check(_L.load().kmcf_field_grid(gpubuf.cutoff_idx, _ptr(gpubuf.site_x), _ptr(gpubuf.site_y), _ptr(gpubuf.site_z), _ptr(mask),
                                       n_fields, _ptr(values), o.ctypes.data_as(C.POINTER(C.c_double)),
                                       h.ctypes.data_as(C.POINTER(C.c_double)), d.ctypes.data_as(C.POINTER(C.c_int)), radius,
                                       1 if normalize else 0, float(fill), _ptr(out), _ptr(wsum), _ptr(count), _ptr(nearest),
                                       _ptr(nd2), C.byref(st)), "kmcf_field_grid")
    shape = tuple(int(v) for v in d)
    res = dict(out=out.reshape((n_fields,) + shape) if n_fields else None, wsum=wsum.reshape(shape), count=count.reshape(shape),
               nearest=nearest.reshape(shape), nearest_d2=nd2.reshape(shape), radius=radius, origin=o, spacing=h, dims=shape,
               stats=st.as_dict())
    if labels is not None:
        if not torch.is_tensor(labels):
            labels = torch.as_tensor(np.ascontiguousarray(labels, dtype=np.int32), device=gpubuf.device)
        assert labels.dtype == torch.int32 and labels.numel() == gpubuf.N_, "labels: N int32 entries"
        near = res["nearest"].long()
        res["labels"] = torch.where(near >= 0, labels.reshape(-1)[near.clamp(min=0)], torch.full_like(res["nearest"], -1))
    return res


def field_slice(gpubuf, axis, position, spacing, **kw):
    """field_grid on a one-voxel-thick grid across the sites' bounding box: the plane `axis` (0, 1, 2 or "x", "y", "z") =
    position, voxels of `spacing` along the other two axes, from the box's lower corner to its upper one."""
    axis = "xyz".index(axis) if isinstance(axis, str) else int(axis)
    xyz = (gpubuf.site_x, gpubuf.site_y, gpubuf.site_z)
    lo = np.array([float(t.min()) for t in xyz])
    hi = np.array([float(t.max()) for t in xyz])
    h = float(spacing)
    dims = np.floor((hi - lo) / h).astype(np.int64) + 1
    lo[axis], dims[axis] = float(position), 1
    return field_grid(gpubuf, lo, h, dims, **kw)


def sample_density(result, radius=None):
    """The number density (per volume of the coordinates' unit) of a raw sum -- field_sample / field_grid with
    normalize=False on a 0 / 1 field: out * 105 / (32 pi radius^3), the inverse of the weight's volume integral.  Host-only
    arithmetic on whatever array type `out` is; radius defaults to the result's own."""
    r = float(result["radius"] if radius is None else radius)
    return result["out"] * (105.0 / (32.0 * np.pi * r ** 3))


def k_assemble(gpubuf, Vd, high_G, low_G):
    lib = _L.load()
    _L.check(lib.kmcf_k_assemble(gpubuf.K_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                 _ptr(gpubuf.metal_types), gpubuf.num_metal_types_, float(Vd), float(high_G),
                                 float(low_G)), "kmcf_k_assemble")


def k_assemble_contacts(gpubuf, site_potential, high_G, low_G):
    """kmcf_k_assemble_contacts: K assembly whose right-hand side takes one Dirichlet value per contact site from the
    contact slots of site_potential (N doubles on the device, layout of site_potential_boundary)."""
    lib = _L.load()
    _L.check(lib.kmcf_k_assemble_contacts(gpubuf.K_distributed, _ptr(gpubuf.site_element), _ptr(gpubuf.site_charge),
                                          _ptr(gpubuf.metal_types), gpubuf.num_metal_types_, _ptr(site_potential),
                                          float(high_G), float(low_G)), "kmcf_k_assemble_contacts")


def k_pattern(gpubuf, which=0):
    lib = _L.load()
    mat = Distributed_matrix.from_handle(lib.kmcf_kstate_matrix(gpubuf.K_distributed))
    n = mat.info()["rows_this_rank"]
    nnz = C.c_int64()
    _L.check(lib.kmcf_kstate_pattern(gpubuf.K_distributed, which, None, None, C.byref(nnz)), "kmcf_kstate_pattern")
    rp = np.zeros(n + 1, np.int32)
    col = np.zeros(max(nnz.value, 1), np.int32)
    _L.check(lib.kmcf_kstate_pattern(gpubuf.K_distributed, which, rp.ctypes.data_as(C.POINTER(C.c_int)),
                                     col.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nnz)), "kmcf_kstate_pattern")
    return rp, col[:nnz.value]


def k_vectors(gpubuf):
    lib = _L.load()
    mat = Distributed_matrix.from_handle(lib.kmcf_kstate_matrix(gpubuf.K_distributed))
    n = mat.info()["rows_this_rank"]
    out = {k: np.zeros(max(n, 1)) for k in ("diag", "dinv", "rhs", "left", "right")}
    p = {k: v.ctypes.data_as(C.POINTER(C.c_double)) for k, v in out.items()}
    _L.check(lib.kmcf_k_get_vectors(gpubuf.K_distributed, p["diag"], p["dinv"], p["rhs"], p["left"], p["right"]),
             "kmcf_k_get_vectors")
    out = {k: v[:n] for k, v in out.items()}
    out["val"] = mat.get_values()
    return out


# --------------------------------------------------------------------------
# dist_iterative surface
# --------------------------------------------------------------------------

class Distributed_matrix:
    """Distributed_matrix + its Distributed_vector (dist_iterative/dist_objects.h:11-36, 69-233).
    Construct from the rows of this rank in CSR with GLOBAL column indices (ctor 1, :158-167)."""

    def __init__(self, kmc_comm, matrix_size, counts, displacements, col_indices_in, row_ptr_in, data_in):
        self.lib = _L.load()
        self.owned = True
        h = C.c_void_p()
        cnt, cntp = _ia(counts)
        dsp, dspp = _ia(displacements)
        rp, rpp = _ia(row_ptr_in)
        ci, cip = _ia(col_indices_in)
        dp = None
        if data_in is not None:
            dv, dp = _da(data_in)
        _L.check(self.lib.kmcf_matrix_create_csr(kmc_comm.handle, int(matrix_size), cntp, dspp, rpp, cip, dp,
                                                 C.byref(h)), "kmcf_matrix_create_csr")
        self.handle = h

    @classmethod
    def split_sparse(cls, kmc_comm, matrix_size, counts, displacements, col_indices_in, row_ptr_in, data_in,
                     subblock_size, count_subblock, displ_subblock, subblock_global_rows,
                     sub_row_ptr, sub_col_indices, sub_data):
        """Distributed_matrix + Distributed_subblock_sparse (dist_objects.h:52-65): the operator
        A_neighbour + P^T A_sub P of conjugate_gradient_jacobi_split_sparse, merged at build time."""
        self = cls.__new__(cls)
        self.lib = _L.load()
        self.owned = True
        h = C.c_void_p()
        a = [_ia(v) for v in (counts, displacements, row_ptr_in, col_indices_in, count_subblock, displ_subblock,
                              subblock_global_rows, sub_row_ptr, sub_col_indices)]
        dv, dp = _da(data_in)
        sv, sp_ = _da(sub_data)
        _L.check(self.lib.kmcf_matrix_create_split_sparse(kmc_comm.handle, int(matrix_size), a[0][1], a[1][1], a[2][1],
                                                          a[3][1], dp, int(subblock_size), a[4][1], a[5][1], a[6][1],
                                                          a[7][1], a[8][1], sp_, C.byref(h)),
                 "kmcf_matrix_create_split_sparse")
        self.handle = h
        return self

    @classmethod
    def from_handle(cls, handle):
        self = cls.__new__(cls)
        self.lib = _L.load()
        self.handle = C.c_void_p(handle) if not isinstance(handle, C.c_void_p) else handle
        self.owned = False
        return self

    def info(self):
        inf = _L.MatrixInfo()
        _L.check(self.lib.kmcf_matrix_info(self.handle, C.byref(inf)), "kmcf_matrix_info")
        return {k: getattr(inf, k) for k, _ in inf._fields_}

    def row_order(self):
        """kmcf_matrix_row_order: (perm, n_short, tile_ends) of the internal row order."""
        n = self.info()["rows_this_rank"]
        perm = np.zeros(max(n, 1), np.int32)
        ns, nt = C.c_int(0), C.c_int(0)
        _L.check(self.lib.kmcf_matrix_row_order(self.handle, perm.ctypes.data_as(C.POINTER(C.c_int)), C.byref(ns), None,
                                                C.byref(nt)), "kmcf_matrix_row_order")
        ends = np.zeros(max(nt.value, 1), np.int32)
        _L.check(self.lib.kmcf_matrix_row_order(self.handle, None, None, ends.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nt)),
                 "kmcf_matrix_row_order")
        return perm[:n], ns.value, ends[:nt.value]

    def sum_plan(self, with_csr=True):
        """kmcf_matrix_sum_plan: the integers that fix the summation order of the solver kernels, the row-per-lane
        tiles and (with_csr) the CSR in the internal order -- what the CPU oracle needs to add in the device's order."""
        pl = _L.SumPlan()
        _L.check(self.lib.kmcf_matrix_sum_plan(self.handle, C.byref(pl), None, None, None, None, None), "kmcf_matrix_sum_plan")
        out = {k: getattr(pl, k) for k, _ in pl._fields_ if k != "reserved"}
        nt, n, nnz = max(pl.sell_tiles, 1), pl.rows, int(self.info()["nnz"])
        first, rows = np.zeros(nt, np.int32), np.zeros(nt, np.int32)
        rp = np.zeros(n + 1, np.int32)
        col = np.zeros(max(nnz, 1), np.int32)
        val = np.zeros(max(nnz, 1))
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        _L.check(self.lib.kmcf_matrix_sum_plan(self.handle, None, ip(first), ip(rows), ip(rp) if with_csr else None,
                                               ip(col) if with_csr else None,
                                               val.ctypes.data_as(C.POINTER(C.c_double)) if with_csr else None),
                 "kmcf_matrix_sum_plan")
        out["tile_first"], out["tile_rows"] = first[:pl.sell_tiles], rows[:pl.sell_tiles]
        if with_csr:
            out["row_ptr"], out["col"], out["val"] = rp, col[:nnz], val[:nnz]
        out["perm"] = self.row_order()[0]
        gid = np.zeros(max(pl.halo_cols, 1), np.int32)
        _L.check(self.lib.kmcf_matrix_halo_columns(self.handle, ip(gid)), "kmcf_matrix_halo_columns")
        out["halo_gid"] = gid[:pl.halo_cols]
        return out

    def neighbours(self):
        """[(rank, nnz, cols_per_neighbour, rows_per_neighbour), ...] starting with self."""
        out = []
        for k in range(self.info()["number_of_neighbours"]):
            r, nnz, nc, nr = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            _L.check(self.lib.kmcf_matrix_neighbour(self.handle, k, C.byref(r), C.byref(nnz), C.byref(nc), None,
                                                    C.byref(nr), None), "kmcf_matrix_neighbour")
            cols = np.zeros(max(nc.value, 1), np.int32)
            rows = np.zeros(max(nr.value, 1), np.int32)
            _L.check(self.lib.kmcf_matrix_neighbour(self.handle, k, None, None, None,
                                                    cols.ctypes.data_as(C.POINTER(C.c_int)), None,
                                                    rows.ctypes.data_as(C.POINTER(C.c_int))), "kmcf_matrix_neighbour")
            out.append(dict(rank=r.value, nnz=nnz.value, cols=cols[:nc.value], rows=rows[:nr.value]))
        return out

    def set_values(self, data):
        dv, dp = _da(data)
        _L.check(self.lib.kmcf_matrix_set_values(self.handle, dp), "kmcf_matrix_set_values")

    def get_values(self):
        out = np.zeros(max(self.info()["nnz"], 1))
        _L.check(self.lib.kmcf_matrix_get_values(self.handle, out.ctypes.data_as(C.POINTER(C.c_double))),
                 "kmcf_matrix_get_values")
        return out[:self.info()["nnz"]]

    def spmv(self, p, Ap):
        """dspmv::gpu_packing_cam (dist_iterative/dist_spmv_gpu_packing.cpp:106-228)."""
        _L.check(self.lib.kmcf_spmv(self.handle, _ptr(p), _ptr(Ap)), "kmcf_spmv")

    def replan(self):
        """kmcf_spmv_replan: re-plan the SpMV from the effective KMCF_SPMV_* values -- the communicator's options, else
        the environment (measurement aid)."""
        _L.check(self.lib.kmcf_spmv_replan(self.handle), "kmcf_spmv_replan")
        return self.info()

    def spmv_bench(self, reps, with_dot=True):
        ms = C.c_float()
        _L.check(self.lib.kmcf_spmv_bench(self.handle, int(reps), 1 if with_dot else 0, C.byref(ms)),
                 "kmcf_spmv_bench")
        return ms.value

    def comm_bench(self, kind, reps):
        """ms for `reps` x {0: all-reduce of 3 doubles, 1: halo exchange, 2: SpMV kernels without exchange}."""
        ms = C.c_float()
        _L.check(self.lib.kmcf_comm_bench(self.handle, int(kind), int(reps), C.byref(ms)), "kmcf_comm_bench")
        return ms.value

    def close(self):
        if self.owned and self.handle:
            self.lib.kmcf_matrix_destroy(self.handle)
            self.handle = None


def conjugate_gradient_jacobi(A_distributed, r_local_d, x_local_d, diag_inv_local_d, relative_tolerance,
                              max_iterations, fixed_iters=0):
    """iterative_solver::conjugate_gradient_jacobi (dist_iterative/dist_conjugate_gradient.cpp:149-276).
    r_local_d: rhs in / residual out; x_local_d: start guess in / solution out."""
    st = _L.SolveStats()
    _L.check(A_distributed.lib.kmcf_pcg_jacobi(A_distributed.handle, _ptr(r_local_d), _ptr(x_local_d),
                                               _ptr(diag_inv_local_d), float(relative_tolerance),
                                               int(max_iterations), int(fixed_iters), C.byref(st)), "kmcf_pcg_jacobi")
    return st.as_dict()


def conjugate_gradient(A_distributed, r_local_d, x_local_d, relative_tolerance, max_iterations, fixed_iters=0):
    """iterative_solver::conjugate_gradient (dist_conjugate_gradient.cpp:17-121): no preconditioner."""
    return conjugate_gradient_jacobi(A_distributed, r_local_d, x_local_d, None, relative_tolerance, max_iterations,
                                     fixed_iters)


def solve_sparse_CG_Jacobi(A_distributed, d_rhs, d_x, tol=1e-14, max_iterations=50000):
    """solve_sparse_CG_Jacobi (src/iterative_solvers_gpu.cu:716-887): A and rhs are scaled in place."""
    st = _L.SolveStats()
    _L.check(A_distributed.lib.kmcf_solve_sparse_CG_Jacobi(A_distributed.handle, _ptr(d_rhs), _ptr(d_x), float(tol),
                                                           int(max_iterations), C.byref(st)),
             "kmcf_solve_sparse_CG_Jacobi")
    return st.as_dict()


def pack_gpu(kmc_comm, packed_buffer, unpacked_buffer, indices, number_of_elements):
    _L.check(_L.load().kmcf_pack(kmc_comm.handle, _ptr(packed_buffer), _ptr(unpacked_buffer), _ptr(indices),
                                 int(number_of_elements)), "kmcf_pack")


def unpack_gpu(kmc_comm, unpacked_buffer, packed_buffer, indices, number_of_elements):
    _L.check(_L.load().kmcf_unpack(kmc_comm.handle, _ptr(unpacked_buffer), _ptr(packed_buffer), _ptr(indices),
                                   int(number_of_elements)), "kmcf_unpack")


def unpack_add(kmc_comm, unpacked_buffer, packed_buffer, indices, number_of_elements):
    _L.check(_L.load().kmcf_unpack_add(kmc_comm.handle, _ptr(unpacked_buffer), _ptr(packed_buffer), _ptr(indices),
                                       int(number_of_elements)), "kmcf_unpack_add")


def elementwise_vector_vector(kmc_comm, array1, array2, result, size):
    _L.check(_L.load().kmcf_elementwise_vector_vector(kmc_comm.handle, _ptr(array1), _ptr(array2), _ptr(result),
                                                      int(size)), "kmcf_elementwise_vector_vector")
