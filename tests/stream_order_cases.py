"""Inputs of the stream ordering tests (tests/test_gpu_stream_order.py), plain numpy.

The GPU tests call an entry point while the device arrays it reads still hold a DECOY and the copies that put the TRUE
values in place are queued, behind a filler, on the caller's stream.  A library that orders its work behind the caller's
queue (include/kmcfield.h, "stream ordering contract") computes from the true values; one that does not reads the decoy.
So a decoy must be an input the entry point accepts as it stands -- a library that fails to wait must compute a wrong
answer, never read out of bounds -- and it must differ enough from the true array that the answer shows it.

case(name) returns dict(name, host: the host arguments (identical in both sets), arrays: {key: Staged}).  A Staged holds
the true array, the decoy, and the rule the decoy is held to (tests/test_stream_order_cases.py asserts them all):

  coords   (N, 3) doubles; finite, inside the true bounding box axis by axis
  element  int32; values of the element enum (src/utils.h:37-44: 0 .. 8)
  charge   int32; values the charge rule can produce (-2, 0, +2)
  finite   doubles; finite
  positive doubles; finite and > 0 (a Jacobi preconditioner)
  neigh    (rows, nn) int32; -1 or a site index below N
  perm     int32; a permutation of 0 .. n - 1
  values   int32; the true array's values in another order (side bits, node names, cell ids: any value is legal, and a
           permuted array keeps the value set the entry point was built for)

Every decoy has the true array's shape and dtype and differs from it in at least 10 % of its entries.  Nothing here is
new physics: the inputs are those of site_kernels_ref, pbc_ref, tpath_ref, events_graph_ref, clusters_ref, site_gap_ref,
site_chain_ref, their periodic forms, site_gradient_ref, heat_local_ref and cgr_cases."""
import functools
import types

import numpy as np

ELEMENTS = tuple(range(9))               # DEFECT, OXYGEN_DEFECT, VACANCY, O, Hf, Ni, Ti, Pt, N
CHARGES = (-2, 0, 2)
MIN_DIFFERENT = 0.10
KINDS = ("coords", "element", "charge", "finite", "positive", "neigh", "perm", "values")


class Staged:
    def __init__(self, kind, true, decoy, **rule):
        assert kind in KINDS, kind
        self.kind, self.rule = kind, rule
        dtype = np.float64 if kind in ("coords", "finite", "positive") else np.int32
        self.true = np.ascontiguousarray(true, dtype=dtype)
        self.decoy = np.ascontiguousarray(decoy, dtype=dtype)
        self.true.setflags(write=False)
        self.decoy.setflags(write=False)


def violations(s):
    """what a Staged breaks of its rule, as a list of sentences (empty: a safe decoy)"""
    t, d, bad = s.true, s.decoy, []
    if t.shape != d.shape or t.dtype != d.dtype:
        return ["shape or dtype differ: %s %s against %s %s" % (t.shape, t.dtype, d.shape, d.dtype)]
    different = float(np.mean(t != d)) if t.size else 0.0
    if different < MIN_DIFFERENT:
        bad.append("only %.1f %% of the entries differ" % (100 * different))
    if s.kind == "coords":
        if not np.isfinite(d).all():
            bad.append("a coordinate is not finite")
        elif (d.min(axis=0) < t.min(axis=0)).any() or (d.max(axis=0) > t.max(axis=0)).any():
            bad.append("outside the true bounding box")
    elif s.kind == "element":
        if not np.isin(d, ELEMENTS).all():
            bad.append("an element outside the enum")
    elif s.kind == "charge":
        if not np.isin(d, CHARGES).all():
            bad.append("a charge the rule cannot produce")
    elif s.kind in ("finite", "positive"):
        if not np.isfinite(d).all():
            bad.append("a value is not finite")
        if s.kind == "positive" and not (d > 0).all():
            bad.append("a value is not positive")
    elif s.kind == "neigh":
        if d.ndim != 2 or ((d < -1) | (d >= s.rule["N"])).any():
            bad.append("an index outside [-1, N)")
    elif s.kind == "perm":
        if not np.array_equal(np.sort(d), np.arange(s.rule["n"])):
            bad.append("not a permutation")
    elif s.kind == "values":
        if not np.array_equal(np.sort(d, axis=None), np.sort(t, axis=None)):
            bad.append("not the true array's values in another order")
    return bad


# ------------------------------------------------------------------------------------------------ decoy builders
def decoy_coords(xyz, seed, keep_x=True):
    """The same positions under another numbering.  keep_x (devices whose sites are sorted by x and whose contacts are the
    first and last sites): the (y, z) pairs are dealt again among the sites that share an x value -- on a lattice the set
    of positions stays what it was, no two sites coincide -- or, where no two sites share an x, among all sites.  Without
    keep_x the whole rows are dealt again."""
    xyz = np.asarray(xyz, np.float64)
    rng = np.random.default_rng(seed)
    out = xyz.copy()
    if not keep_x:
        return xyz[rng.permutation(len(xyz))]
    _, group, counts = np.unique(xyz[:, 0], return_inverse=True, return_counts=True)
    if counts.max() == 1:
        out[:, 1:] = xyz[rng.permutation(len(xyz)), 1:]
        return out
    for g in np.flatnonzero(counts > 1):
        rows = np.flatnonzero(group == g)
        out[rows, 1:] = xyz[rng.permutation(rows), 1:]
    return out


def permuted(a, seed, among=None):
    """a's values dealt again (among the entries of the index set `among` only, where given)"""
    a = np.asarray(a)
    rng = np.random.default_rng(seed)
    out = a.copy()
    if among is None:
        return a[rng.permutation(len(a))]
    among = np.asarray(among)
    out[among] = a[rng.permutation(among)]
    return out


def other_doubles(a, seed, lo=None, hi=None):
    """finite doubles in the true array's range, none equal to the true entry but by chance"""
    a = np.asarray(a, np.float64)
    rng = np.random.default_rng(seed)
    lo = float(a.min()) if lo is None else lo
    hi = float(a.max()) if hi is None else hi
    if hi <= lo:
        hi = lo + 1.0
    return rng.uniform(lo, hi, a.shape)


# ------------------------------------------------------------------------------------------------ plain vectors
VEC_TILES = 48                           # cgr_cases.banded: 64 rows per tile, 3072 rows
SIGMA, K_COULOMB = 3.5e-10, 8.987552e9 / 23


@functools.lru_cache(maxsize=None)
def _vectors():
    import cgr_cases as G
    M, _ = G.banded(VEC_TILES)
    M = M.tocsr()
    M.sort_indices()
    n = M.shape[0]
    rng = np.random.default_rng(401)
    dinv = 1.0 / M.diagonal()
    v = {k: rng.standard_normal(n) + 2.0 for k in ("p", "b", "x0", "a1", "a2", "p_d", "b_d", "x0_d", "a1_d", "a2_d")}
    idx, idx_d = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    host = dict(n=n, row_ptr=M.indptr.astype(np.int32), col=M.indices.astype(np.int32), val=M.data.copy(), rows=64,
                val2=M.data * np.where(M.indices == np.repeat(np.arange(n), np.diff(M.indptr)), 2.0, 1.0))
    return host, dict(
        p=Staged("finite", v["p"], v["p_d"]), b=Staged("finite", v["b"], v["b_d"]), x0=Staged("finite", v["x0"], v["x0_d"]),
        dinv=Staged("positive", dinv, dinv * rng.uniform(0.5, 1.5, n)),
        a1=Staged("finite", v["a1"], v["a1_d"]), a2=Staged("finite", v["a2"], v["a2_d"]),
        idx=Staged("perm", idx, idx_d, n=n))


def _vec(name, keys):
    host, arrays = _vectors()
    return dict(name=name, host=host, arrays={k: arrays[k] for k in keys})


# ------------------------------------------------------------------------------------------------ K path
@functools.lru_cache(maxsize=None)
def _kdev():
    import heat_local_ref as H
    import site_kernels_ref as R
    dev = R.k_device("sparse")
    N, NL, el = dev["N"], dev["NL"], dev["element"]
    xyz_d = decoy_coords(dev["xyz"], 402)
    el_d = permuted(el, 403)
    neigh = R.neighbor_rows(dev["xyz"], R.K_CHARGE_NN_DIST, R.K_CHARGE_NN)
    rng = np.random.default_rng(404)
    # a potential in the layout of site_potential_boundary: one Dirichlet value per contact site, a start guess between them
    pot = np.linspace(-dev["Vd"] / 2, dev["Vd"] / 2, N) + 0.05 * rng.standard_normal(N)
    pot_d = np.linspace(dev["Vd"] / 2, -dev["Vd"] / 2, N) + 0.05 * rng.standard_normal(N)
    _, _, Q, T_old = H.synth_inputs("sparse")
    T_d = np.array(T_old)
    T_d[NL:-NL] = H.SYNTH_PRM["background_temp"] + 5.0 * np.cos(0.013 * np.arange(N - 2 * NL)) ** 2
    host = dict(N=N, NL=NL, n=dev["n"], nn=R.K_CHARGE_NN, nn_dist_charge=R.K_CHARGE_NN_DIST, nn_dist=R.K_NN_DIST,
                metals=dev["metals"], lattice=dev["lattice"], Vd=dev["Vd"], high_G=dev["high_G"], low_G=dev["low_G"],
                xyz=dev["xyz"], element=el, charge=dev["charge"], heat=dict(H.synth_params("distinct"), **H.SYNTH_CG),
                heat_step=H.SYNTH_STEP["transient"], global_heat=dict(R.HEAT_ARGS), r_max=R.CUTOFF, cutoff=R.CUTOFF)
    arrays = dict(
        xyz=Staged("coords", dev["xyz"], xyz_d), element=Staged("element", el, el_d),
        charge=Staged("charge", dev["charge"], dev["charge2"]),
        neigh=Staged("neigh", neigh, np.full_like(neigh, -1), N=N),
        pot=Staged("finite", pot, pot_d), pot_charge=Staged("finite", 0.1 * rng.standard_normal(N), 0.1 * rng.standard_normal(N)),
        power=Staged("finite", Q, np.roll(Q, N // 3) * 1.5), T_old=Staged("finite", T_old, T_d),
        T_bg=Staged("finite", [300.0], [345.0]))
    return host, arrays


def _k(name, keys):
    host, arrays = _kdev()
    return dict(name=name, host=host, arrays={k: arrays[k] for k in keys})


# ------------------------------------------------------------------------------------------------ pairwise term
def _pairwise(name, source, keys):
    if source == "p11":
        import pbc_ref as P
        c = P.pairwise_case("p11")
        lattice = np.asarray(c["L"], np.float64)
    else:
        import site_kernels_ref as R
        c = R.pairwise_case(source)
        lattice = None
    N = c["N"]
    rng = np.random.default_rng(405)
    charge_d = rng.choice(np.array(CHARGES, np.int32), N, p=[0.3, 0.4, 0.3])
    arrays = dict(xyz=Staged("coords", c["xyz"], decoy_coords(c["xyz"], 406, keep_x=False)),
                  charge=Staged("charge", c["charge"], charge_d))
    host = dict(N=N, cutoff=20.0, lattice=lattice, sigma=SIGMA, k=K_COULOMB, xyz=c["xyz"], charge=c["charge"])
    return dict(name=name, host=host, arrays={k: arrays[k] for k in keys})


# ------------------------------------------------------------------------------------------------ T path
@functools.lru_cache(maxsize=None)
def _tdev():
    import tpath_ref as T
    c = T.tpath_case("nt_65")
    el, N = c["element"], len(c["element"])
    inner = np.flatnonzero(~np.isin(el, c["metals"]))          # every site that is no contact metal: the oxide and its interstitials
    el_d = permuted(el, 407, among=inner)
    atoms = lambda e: int(((e != T.DEFECT) & (e != T.OXYGEN_DEFECT)).sum())
    assert atoms(el_d) == atoms(el)                            # N_atom, and with it the row partition, is a host argument
    charge_d, cb_d = T.other_state(c)
    Vd = c["par"]["Vd"]
    Nsub = atoms(el) + 1
    pots = []
    for seed in (1, 2):
        m = np.zeros(atoms(el) + 2)
        m[:Nsub] = T.potentials(types.SimpleNamespace(Nsub=Nsub), Vd, seed)
        pots.append(m)
    cell = (c["xyz"][:, 1] > np.median(c["xyz"][:, 1])).astype(np.int32)
    host = dict(case=c, N=N, N_atom=atoms(el), Nsub=Nsub, Vd=Vd, planes=T.A_LAT * (np.arange(3, 10) + 0.25), n_cells=2)
    arrays = dict(xyz=Staged("coords", c["xyz"], decoy_coords(c["xyz"], 408)), element=Staged("element", el, el_d),
                  charge=Staged("charge", c["charge"], charge_d), cb=Staged("finite", c["cb"], cb_d),
                  potentials=Staged("finite", pots[0], pots[1][::-1].copy()), cell=Staged("values", cell, permuted(cell, 409)))
    return host, arrays


def _t(name, keys):
    host, arrays = _tdev()
    return dict(name=name, host=host, arrays={k: arrays[k] for k in keys})


# ------------------------------------------------------------------------------------------------ events
EVENTS_N = 1500


@functools.lru_cache(maxsize=None)
def _events():
    import events_graph_ref as G
    neigh = G.ring_list(EVENTS_N, [1, 2, 70], False, 7)
    c = G.graph_case("stream_order_1500", neigh, 400, 31, max_events=256)
    d = G.graph_case("stream_order_1500_decoy", neigh, 400, 32, max_events=256)
    assert np.array_equal(c["neigh"], d["neigh"])              # (positions and layers are not staged: the true case's)
    rng = np.random.default_rng(410)
    host = dict(c)
    arrays = dict(element=Staged("element", c["element"], d["element"]), charge=Staged("charge", c["charge"], d["charge"]),
                  pot=Staged("finite", c["pot"], d["pot"]),
                  temperature=Staged("finite", 300.0 + 60.0 * rng.random(EVENTS_N), 300.0 + 60.0 * rng.random(EVENTS_N)))
    return host, arrays


def _ev(name, keys):
    host, arrays = _events()
    return dict(name=name, host=host, arrays={k: arrays[k] for k in keys})


# ------------------------------------------------------------------------------------------------ analyses
def _clusters():
    import clusters_ref as CR
    c = CR.case("pairs1")
    el_d, ch_d, _ = CR.draw(c["N"], 411)
    return dict(name="conductive_clusters", host=c,
                arrays=dict(element=Staged("element", c["element"], el_d), charge=Staged("charge", c["charge"], ch_d),
                            x=Staged("finite", c["x"], permuted(c["x"], 412))))


def _site_set(name, module, source, periodic):
    c = __import__(module).case(source)
    # (the coordinates stay: the index of the search was built from them, and a search on other coordinates than its
    # index's is no input the entry point is specified for)
    arrays = dict(side=Staged("values", c["side"], permuted(c["side"], 414)))
    if "node" in c:
        arrays["node"] = Staged("values", c["node"], permuted(c["node"], 415))
    if c["cell"] is not None:
        arrays["cell"] = Staged("values", c["cell"], permuted(c["cell"], 416))
    host = dict(c, lattice=np.asarray(c["L"], np.float64) if periodic else None, periodic=periodic)
    return dict(name=name, host=host, arrays=arrays)


def _gradient():
    import site_gradient_ref as GR
    c = GR.case("jitter52")
    return dict(name="site_gradient", host=c,
                arrays=dict(xyz=Staged("coords", c["xyz"], decoy_coords(c["xyz"], 417, keep_x=False)),
                            value=Staged("finite", c["value"], other_doubles(c["value"], 418))))


# ------------------------------------------------------------------------------------------------ the table
BUILDERS = {
    # plain vectors
    "spmv": lambda: _vec("spmv", ("p",)),
    "pcg_jacobi/loop": lambda: _vec("pcg_jacobi/loop", ("b", "x0", "dinv")),
    "pcg_jacobi/resident": lambda: _vec("pcg_jacobi/resident", ("b", "x0", "dinv")),
    "solve_sparse_CG_Jacobi": lambda: _vec("solve_sparse_CG_Jacobi", ("b", "x0")),
    "pack": lambda: _vec("pack", ("a1", "idx")),
    "unpack": lambda: _vec("unpack", ("a1", "idx")),
    "unpack_add": lambda: _vec("unpack_add", ("a1", "a2", "idx")),
    "elementwise_vector_vector": lambda: _vec("elementwise_vector_vector", ("a1", "a2")),
    "matrix_values": lambda: _vec("matrix_values", ("p",)),
    # K path
    "neighbor_list": lambda: _k("neighbor_list", ("xyz",)),
    "neighbor_list_pbc": lambda: _k("neighbor_list_pbc", ("xyz",)),
    "initialize_sparsity_K": lambda: _k("initialize_sparsity_K", ("xyz",)),
    "update_charge": lambda: _k("update_charge", ("element", "charge", "neigh")),
    "k_assemble": lambda: _k("k_assemble", ("element", "charge")),
    "k_assemble_contacts": lambda: _k("k_assemble_contacts", ("element", "charge", "pot")),
    "background_potential_sparse": lambda: _k("background_potential_sparse", ("element", "charge", "pot")),
    "background_potential_sparse_contacts": lambda: _k("background_potential_sparse_contacts", ("element", "charge", "pot")),
    "update_CB_edge_sparse": lambda: _k("update_CB_edge_sparse", ("element", "charge")),
    "sum_and_gather_potential": lambda: _k("sum_and_gather_potential", ("pot", "pot_charge")),
    "update_temperature_global": lambda: _k("update_temperature_global", ("power", "T_bg")),
    "update_temperature_local": lambda: _k("update_temperature_local", ("power", "T_old")),
    "filament_gap": lambda: _k("filament_gap", ("element", "charge")),
    "filament_chain": lambda: _k("filament_chain", ("element", "charge")),
    # pairwise term
    "compute_cutoff_list": lambda: _pairwise("compute_cutoff_list", "cube", ("xyz",)),
    "compute_cutoff_list_pbc": lambda: _pairwise("compute_cutoff_list_pbc", "p11", ("xyz",)),
    "poisson_gridless/seventeen": lambda: _pairwise("poisson_gridless/seventeen", "seventeen", ("charge",)),
    "poisson_gridless/cube": lambda: _pairwise("poisson_gridless/cube", "cube", ("charge",)),
    # T path
    "initialize_sparsity_T": lambda: _t("initialize_sparsity_T", ("xyz", "element")),
    "t_assemble": lambda: _t("t_assemble", ("charge", "cb")),
    "update_power_sparse": lambda: _t("update_power_sparse", ("charge", "cb")),
    "current_map": lambda: _t("current_map", ("potentials",)),
    "current_profile": lambda: _t("current_profile", ("potentials", "cell")),
    # events
    "event_rates": lambda: _ev("event_rates", ("element", "charge", "pot", "temperature")),
    "execute_kmc_step": lambda: _ev("execute_kmc_step", ("element", "charge", "pot")),
    "execute_kmc_step_thermal": lambda: _ev("execute_kmc_step_thermal", ("element", "charge", "pot", "temperature")),
    # analyses
    "conductive_clusters": _clusters,
    "site_set_gap": lambda: _site_set("site_set_gap", "site_gap_ref", "straddle", False),
    "site_set_chain": lambda: _site_set("site_set_chain", "site_chain_ref", "straddle", False),
    "site_set_gap_pbc": lambda: _site_set("site_set_gap_pbc", "site_gap_pbc_ref", "p11@12", True),
    "site_set_chain_pbc": lambda: _site_set("site_set_chain_pbc", "site_chain_pbc_ref", "p11@12", True),
    "site_gradient": _gradient,
}
# The set-up entry points that copy the caller's coordinates to the host with synchronous copies: they wait for the caller's
# stream on the host (kmcf_enter_setup).  Each stages its coordinates.
SETUP = ("neighbor_list", "neighbor_list_pbc", "initialize_sparsity_K", "compute_cutoff_list", "compute_cutoff_list_pbc")
CASES = tuple(BUILDERS)
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = BUILDERS[name]()
    return _cache[name]


# ------------------------------------------------------------------------------------------------ the group
GROUP_N, GROUP_P = 2000, 2


@functools.lru_cache(maxsize=None)
def group():
    """the vectors of the two-rank group: whole-system arrays, each rank stages its own slice"""
    rng = np.random.default_rng(419)
    n = GROUP_N
    f = lambda: rng.standard_normal(n) + 2.0
    return dict(name="group", host=dict(n=n, P=GROUP_P),
                arrays=dict(p=Staged("finite", f(), f()), b=Staged("finite", f(), f()), x0=Staged("finite", f(), f())))
