"""GPU: kmcf_site_set_chain_pbc and kmcf_filament_chain_pbc (csrc/kmcf_chain.hip, the periodic ch_search_kernel) against the
restatement of tests/site_chain_pbc_ref.py, in the sense of `_same` of tests/test_gpu_site_chain.py: array_equal on every
integer, hop_max2, direct2, the hops and the input-decided stats (surface sites included); hop_max within 1 ulp, length
within 2 n ulp; a second call the same bytes.  Random site sets on periodic indices of (1,1), (2,3), (3,4), (5,2) and (3,3)
cells in (y, z) at two radii; constructed sets on exact lattices; direct2 against gap2 of kmcf_site_set_gap_pbc; on a
non-periodic index the bytes of the plain calls; the argument checks; two stumps and a floating body across the y face of
a small box; the periodic 5 nm cell with a filament through its corner, whole, cut, with a vacancy in the cut, without one;
tools/kmc_loop.py --workload 5nm-periodic --chain.  tests/test_site_chain_pbc_ref.py shows that the inputs are what their
names say.

Every test builds and frees its own communicator."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import clusters_ref as CR
import pbc_ref as P
import site_chain_pbc_ref as CP
import site_chain_ref as R
import site_gap_pbc_ref as GP
from test_gpu_site_chain import _same
from test_gpu_site_gap_pbc import _Device, _comm, _periodic_5nm_with_a_filament

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SET, SET_PBC, FIL, FIL_PBC = "kmcf_site_set_chain", "kmcf_site_set_chain_pbc", "kmcf_filament_chain", "kmcf_filament_chain_pbc"


def _ints(st):
    return {k: v for k, v in st.items() if not k.startswith("ms_")}


# ---- the search primitive ------------------------------------------------------------------------------------------------------

class _Index:
    """a spatial index over a case's coordinates with the case's cutoff: pbc = 1 with the case's lattice, the same call with
    pbc = 0, or (pbc None) kmcf_compute_cutoff_list"""

    def __init__(self, km, comm, c, pbc=1):
        import torch
        self.km, self.c = km, c
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
        self.i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device="cuda")
        self.x, self.y, self.z = (f64(c["xyz"][:, k]) for k in range(3))
        self.side, self.node = self.i32(c["side"]), self.i32(c["node"])
        self.cell = self.i32(c["cell"]) if c["cell"] is not None else None
        self.handle = C.c_void_p()
        p, lib = km.solvers._ptr, km.lib.load()
        if pbc is None:
            km.lib.check(lib.kmcf_compute_cutoff_list(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                      float(c["cutoff"]), C.byref(self.handle)), "kmcf_compute_cutoff_list")
        else:
            lat = np.ascontiguousarray(c.get("L", [1000.0, 1000.0, 1000.0]), np.float64)
            km.lib.check(lib.kmcf_compute_cutoff_list_pbc(comm.handle, p(self.x), p(self.y), p(self.z), len(c["xyz"]),
                                                          float(c["cutoff"]), lat.ctypes.data_as(C.POINTER(C.c_double)), pbc,
                                                          C.byref(self.handle)), "kmcf_compute_cutoff_list_pbc")

    def raw(self, entry=SET_PBC, **over):
        """the C entry itself with single arguments replaced: (rc, records, hops, stats)"""
        km, c, p = self.km, self.c, self.km.solvers._ptr
        max_hops = over.get("max_hops", c["max_hops"])
        n_cells = over.get("n_cells", c["n_cells"])
        chains = np.zeros(max(n_cells, 1), km.solvers.CHAIN_DTYPE)
        hops = np.zeros((max(n_cells, 1), max(max_hops, 1)), km.solvers.HOP_DTYPE)
        st = km.lib.ChainStats()
        a = dict(p=self.handle, x=p(self.x), y=p(self.y), z=p(self.z), side=p(self.side), node=p(self.node),
                 r_max=float(c["r_max"]), cell=p(self.cell), n_cells=n_cells,
                 chains=chains.ctypes.data_as(C.POINTER(km.lib.Chain)),
                 hops=hops.ctypes.data_as(C.POINTER(km.lib.Hop)) if max_hops > 0 else None, max_hops=max_hops, stats=C.byref(st))
        a.update(over)
        rc = getattr(km.lib.load(), entry)(a["p"], a["x"], a["y"], a["z"], a["side"], a["node"], a["r_max"], a["cell"],
                                           a["n_cells"], a["chains"], a["hops"], a["max_hops"], a["stats"])
        return rc, chains, (hops if max_hops > 0 else None), st.as_dict()

    def chain(self, entry=SET_PBC, **over):
        rc, chains, hops, st = self.raw(entry, **over)
        self.km.lib.check(rc, entry)
        return dict(chains=chains, hops=hops, stats=st)

    def refused(self, entry, match, **over):
        rc = self.raw(entry, **over)[0]
        msg = self.km.lib.load().kmcf_last_error().decode()
        assert rc == -1 and match in msg and entry + ":" in msg, (rc, msg)
        return msg

    def gap2(self, r_max=None):
        """gap2 per cell of kmcf_site_set_gap_pbc on the same index and sides"""
        km, c, p = self.km, self.c, self.km.solvers._ptr
        gaps = np.zeros(c["n_cells"], km.solvers.GAP_DTYPE)
        km.lib.check(km.lib.load().kmcf_site_set_gap_pbc(self.handle, p(self.x), p(self.y), p(self.z), p(self.side),
                                                         float(c["r_max"] if r_max is None else r_max), p(self.cell),
                                                         c["n_cells"], gaps.ctypes.data_as(C.POINTER(km.lib.Gap)), None),
                     "kmcf_site_set_gap_pbc")
        return gaps["gap2"]

    def close(self):
        self.km.lib.load().kmcf_pairwise_destroy(self.handle)


@pytest.mark.parametrize("name", CP.SEARCH_CASES)
def test_site_sets_match_the_restatement(km, name):
    c, ref = CP.case(name), CP.reference(name)
    with _comm(km, len(c["xyz"])) as comm:
        ix = _Index(km, comm, c)
        try:
            got = ix.chain()
            _same(got, ref)
            again = ix.chain()                                       # scratch reused: the same bytes
            assert got["chains"].tobytes() == again["chains"].tobytes() and got["hops"].tobytes() == again["hops"].tobytes()
            assert _ints(got["stats"]) == _ints(again["stats"])
            assert ix.chain(stats=None)["chains"].tobytes() == got["chains"].tobytes()
            assert ix.chain(max_hops=0)["chains"].tobytes() == got["chains"].tobytes()
            assert ix.chain(max_hops=0, stats=None)["chains"].tobytes() == got["chains"].tobytes()
            # direct2 is the gap's gap2 on the same index and sides, +infinity included
            assert np.array_equal(got["chains"]["direct2"], ix.gap2())
            if name == "zigzag_wrap":
                assert got["stats"]["rounds"] >= 4 and got["chains"][0]["n_hops"] == CP.ZIGZAG_STONES + 1
                assert got["hops"].shape == (1, 16)
            if name == "rim_wrap":                                  # ... and the same index with r_max just below the last hop
                below = CP.case("rim_wrap_below")["r_max"]
                _same(ix.chain(r_max=below), CP.reference("rim_wrap_below"))
                assert np.isinf(ix.gap2(below)).all()
            if name == "wrap_detour":                               # no node at all: the chain is the direct link
                none = ix.i32(np.full(len(c["xyz"]), -1))
                alone = ix.chain(node=km.solvers._ptr(none))["chains"][0]
                assert alone["n_hops"] == 1 and alone["hop_max2"] == 25.0 == alone["direct2"]
            msg = ix.refused(SET, "periodic")                       # the plain call still refuses this index
            assert SET_PBC in msg
            ix.refused(SET_PBC, "cutoff", r_max=float(np.nextafter(c["cutoff"], np.inf)))
        finally:
            ix.close()


OPEN_CASES = ["ladder", "detour", "rim", "rim_below", "ties", "straddle", "home", "home_flipped", "multi_site", "zigzag",
              "statuses", "mixed", "large"]


@pytest.mark.parametrize("name", OPEN_CASES)
def test_on_a_non_periodic_index_the_bytes_of_the_plain_call(km, name):
    c = R.case(name)
    with _comm(km, 1) as comm:
        plain = None
        for pbc in (None, 0):                                        # kmcf_compute_cutoff_list; ..._pbc with pbc = 0
            ix = _Index(km, comm, c, pbc=pbc)
            try:
                if plain is None:
                    plain = ix.chain(SET)
                    _same(plain, R.reference(name))
                got = ix.chain(SET_PBC)
                assert got["chains"].tobytes() == plain["chains"].tobytes() and got["hops"].tobytes() == plain["hops"].tobytes()
                assert _ints(got["stats"]) == _ints(plain["stats"])
                assert ix.chain(SET)["chains"].tobytes() == plain["chains"].tobytes()
            finally:
                ix.close()


def test_arguments_are_checked(km):
    c = CP.case("rim_wrap")
    with _comm(km, len(c["xyz"])) as comm:
        for ix in (_Index(km, comm, c), _Index(km, comm, c, pbc=None)):
            try:
                for k in ("x", "y", "z", "side", "node", "chains", "p"):
                    ix.refused(SET_PBC, {"x": "d_x", "y": "d_y", "z": "d_z", "side": "d_site_side", "node": "d_site_node",
                                         "chains": "h_chains", "p": "p is NULL"}[k], **{k: None})
                for bad in (float("nan"), float("inf"), 0.0, -1.0):
                    ix.refused(SET_PBC, "r_max", r_max=bad)
                ix.refused(SET_PBC, "cutoff", r_max=float(np.nextafter(16.0, 17.0)))
                ix.refused(SET_PBC, "n_cells", n_cells=0)
                ix.refused(SET_PBC, "d_site_cell is NULL", n_cells=2, cell=None)
                ix.refused(SET_PBC, "max_hops", max_hops=-1)
                ix.refused(SET_PBC, "h_hops is set", max_hops=0,
                           hops=np.zeros(1, km.solvers.HOP_DTYPE).ctypes.data_as(C.POINTER(km.lib.Hop)))
                ix.refused(SET_PBC, "h_hops is NULL", hops=None)
                # the order of the checks is the plain call's: the first bad argument is named
                ix.refused(SET_PBC, "d_site_side", side=None, x=None, r_max=-1.0)
                ix.refused(SET_PBC, "d_x", x=None, r_max=-1.0, p=None)
            finally:
                ix.close()
        ix = _Index(km, comm, c)
        try:                                                         # the cutoff itself is allowed
            _same(ix.chain(r_max=16.0), CP.site_set_chain(c["xyz"], c["side"], c["node"], 16.0, c["cell"], c["n_cells"],
                                                          c["max_hops"], L=c["L"]))
        finally:
            ix.close()


# ---- the full call ---------------------------------------------------------------------------------------------------------------

MAX_HOPS = 12


def _restated(neigh, element, charge, metals, xyz, NL, NR, r_max, L):
    t = time.time()
    side, node = R.sides_and_nodes(neigh, element, charge, metals, xyz[:, 0], NL, NR)
    ref = CP.site_set_chain(xyz, side, node, r_max, None, 1, MAX_HOPS, L=L)
    print("restatement %.2f s" % (time.time() - t))
    return side, node, ref


def _full(got, side, node, ref):
    _same(got, ref)
    assert np.array_equal(got["side"].cpu().numpy(), side) and np.array_equal(got["node"].cpu().numpy(), node)


def _filament_head(S, buf, NL, r_max, chains, o):
    p = S._ptr
    return [o.get("idx", buf.cutoff_idx), o.get("nn", buf.nn_), o.get("neigh", p(buf.neigh_idx)),
            o.get("element", p(buf.site_element)), o.get("charge", p(buf.site_charge)), o.get("metals", p(buf.metal_types)),
            o.get("num_metals", buf.num_metal_types_), p(buf.site_x), p(buf.site_y), p(buf.site_z), o.get("n_left", NL),
            o.get("n_right", NL), o.get("r_max", r_max), None, o.get("n_cells", 1), chains.ctypes.data_as(C.POINTER(S._L.Chain)), None,
            o.get("max_hops", 0), None, None, None]


BODY = [(5, 4, 3), (5, 0, 3)]            # (x, y, z) lattice indices of site_gap_pbc_ref.stubs(): neighbours through the y face


def test_stubs_and_a_floating_body_across_the_y_face(km):
    """site_gap_pbc_ref.stubs() -- two vacancy stumps 7.73 A apart through the y face -- and two more neutral vacancies, one
    on either side of that face and adjacent through it, next to neither stump: under the periodic list ONE floating body
    that touches the face, about 3.5 A from the left stump on one side and 5.6 A from the right stump on the other"""
    import torch
    s = GP.stubs()
    g = P.box()["grid"]
    body = [int(np.flatnonzero((g == np.array(t)).all(axis=1))[0]) for t in BODY]
    element = s["element"].copy()
    element[body] = P.VACANCY
    xyz, L, NL, NR, r_max = s["xyz"], s["L"], s["NL"], s["NR"], GP.STUB_R_MAX
    args = (element, s["charge"], s["metals"], xyz, NL, NR, r_max, L)
    with _comm(km, s["N"]) as comm:
        dv = _Device(km, comm, xyz, element, L, s["metals"], P.BOX_NN_DIST, P.BOX_NN, 1)
        try:
            S, buf = dv.S, dv.buf
            assert np.array_equal(dv.neigh, s["per"])
            run = lambda **kw: S.filament_chain(comm, buf, NL, NR, r_max, max_hops=MAX_HOPS, periodic=True, **kw)
            full = run()
            side, node, ref = _restated(s["per"], *args)
            _full(full, side, node, ref)
            r, hops = full["chains"][0], full["hops"][0]
            print("stubs with a body:", r, hops[:r["n_hops"]])
            assert node[body[0]] == node[body[1]] >= 0 and (node >= 0).sum() == 2
            assert (r["status"], r["n_hops"], r["n_stones"], r["n_stone_sites"]) == (R.CHAINED, 2, 1, 2)
            # it enters the body on one side of the face and leaves it on the other
            assert (hops["to"][0], hops["from"][1]) == tuple(body) and r["hop_max2"] < r["direct2"]
            gap = S.filament_gap(comm, buf, NL, NR, r_max, periodic=True)["gaps"][0]
            assert r["direct2"] == gap["gap2"] and 7.0 < gap["gap"] < 9.0
            for kw in (dict(sides=False), dict(nodes=False), dict(sides=False, nodes=False)):     # NULL outputs
                q = run(**kw)
                assert q["chains"].tobytes() == full["chains"].tobytes() and q["hops"].tobytes() == full["hops"].tobytes()
            # the primitive on the sides and nodes the full call wrote; and with every node -1: one hop, the periodic gap
            again = S.site_set_chain(buf, full["side"], full["node"], r_max, max_hops=MAX_HOPS, periodic=True)
            assert again["chains"].tobytes() == full["chains"].tobytes() and again["hops"].tobytes() == full["hops"].tobytes()
            alone = S.site_set_chain(buf, full["side"], full["node"] * 0 - 1, r_max, max_hops=MAX_HOPS, periodic=True)
            a = alone["chains"][0]
            assert (a["n_hops"], a["n_stones"], a["hop_max2"]) == (1, 0, gap["gap2"])
            assert (alone["hops"][0]["from"][0], alone["hops"][0]["to"][0]) == (gap["site_left"], gap["site_right"])
            with pytest.raises(km.lib.KmcfError, match="periodic.*kmcf_filament_chain_pbc"):
                S.filament_chain(comm, buf, NL, NR, r_max)
            with pytest.raises(km.lib.KmcfError, match="periodic.*kmcf_site_set_chain_pbc"):
                S.site_set_chain(buf, full["side"], full["node"], r_max)
            # the argument checks of the full call, by the name of the _pbc call
            lib, chains = S._L.load(), np.zeros(1, S.CHAIN_DTYPE)
            for match, o in (("d_neigh_idx", dict(neigh=None)), ("d_site_element", dict(element=None)),
                             ("d_site_charge", dict(charge=None)), ("nn", dict(nn=0)), ("num_metals", dict(num_metals=-1)),
                             ("d_metals", dict(metals=None)), ("N_left_tot", dict(n_left=-1)), ("N_right_tot", dict(n_right=-2)),
                             ("exceeds N", dict(n_left=s["N"], n_right=1)), ("r_max", dict(r_max=float("nan"))),
                             ("cutoff", dict(r_max=20.5)), ("n_cells", dict(n_cells=0)), ("max_hops", dict(max_hops=-1)),
                             ("h_hops is NULL", dict(max_hops=3)), ("p is NULL", dict(idx=None))):
                assert lib.kmcf_filament_chain_pbc(*_filament_head(S, buf, NL, r_max, chains, o)) == -1, match
                msg = lib.kmcf_last_error().decode()
                assert match in msg and FIL_PBC + ":" in msg, msg
            assert lib.kmcf_filament_chain_pbc(*_filament_head(S, buf, NL, r_max, chains, {})) == 0
            assert chains.tobytes() == full["chains"].tobytes()
            # the open list with the periodic index: the body is cut in two at the face, the distances stay periodic
            S.compute_neighbor_list(comm, buf, P.BOX_NN_DIST, P.BOX_NN, pbc=0)
            assert np.array_equal(buf.neigh_idx.cpu().numpy().reshape(s["N"], P.BOX_NN), s["opn"])
            cut = run()
            side_o, node_o, ref_o = _restated(s["opn"], *args)
            _full(cut, side_o, node_o, ref_o)
            assert node_o[body[0]] != node_o[body[1]] and cut["chains"][0]["n_stones"] == 2
            assert cut["chains"].tobytes() != full["chains"].tobytes()
        finally:
            dv.close()
        # open list, open index through the _pbc call: the plain call's bytes, no pair within r_max
        dv = _Device(km, comm, xyz, element, L, s["metals"], P.BOX_NN_DIST, P.BOX_NN, 0)
        try:
            got = dv.S.filament_chain(comm, dv.buf, NL, NR, r_max, max_hops=MAX_HOPS, periodic=True)
            plain = dv.S.filament_chain(comm, dv.buf, NL, NR, r_max, max_hops=MAX_HOPS)
            assert got["chains"].tobytes() == plain["chains"].tobytes() and got["hops"].tobytes() == plain["hops"].tobytes()
            side_o, node_o, ref_o = _restated(s["opn"], *args[:-1], None)
            _full(got, side_o, node_o, ref_o)
            assert np.isinf(got["chains"][0]["direct2"])
        finally:
            dv.close()


R_MAX = 20.0


def _stone_site(d, element, neigh, cls, side, L, reach2, through_a_face):
    """How the site is found: among the sites that are neither contact, metal nor member and have no member among their
    listed neighbours (turned into a neutral vacancy such a site floats: a one-site stone), those with a site of the left
    side AND a site of the right side within sqrt(reach2) under the minimum image; of these the one whose farther side is
    nearest.  through_a_face: only sites whose nearest pair to one of the sides is nearest through a y or z face.
    (site, d2 to the left side, d2 to the right side)"""
    xyz, NL, N = d["xyz"], d["N_contact"], len(d["xyz"])
    members = cls != 0
    ok = np.ones(N, bool)
    ok[:NL] = ok[-NL:] = False
    ok &= ~members & ~np.isin(element, d["metals"])
    listed = (neigh >= 0) & (neigh < N)
    ok &= ~(members[np.where(listed, neigh, 0)] & listed).any(axis=1)
    cand = np.flatnonzero(ok)
    best, faces = [], []
    for bit in (1, 2):
        a, b = CP.near_pairs(xyz, cand, np.flatnonzero(side == bit), np.sqrt(reach2) * (1 + 1e-9) + 1e-9, L)
        d2 = CP.d2_exact(xyz, a, b, L)
        o = np.lexsort((b, d2, a))
        a, b, d2 = a[o], b[o], d2[o]
        first = np.unique(a, return_index=True)[1]                              # the nearest site of this side per candidate
        m = np.full(N, np.inf)
        m[a[first]] = d2[first]
        f = np.zeros(N, bool)
        f[a[first]] = [GP.crossings(xyz, i, j, L) != (0, 0) for i, j in zip(a[first].tolist(), b[first].tolist())]
        best.append(m)
        faces.append(f)
    far = np.maximum(best[0], best[1])
    if through_a_face:
        far[~(faces[0] | faces[1])] = np.inf
    k = int(np.argmin(far))
    assert far[k] < reach2, (far[k], reach2)
    return k, float(best[0][k]), float(best[1][k])


def test_periodic_5nm_cell_with_a_filament_whole_cut_and_with_a_stone(km):
    """structure.periodic_5nm with a filament along x through the corner of the cell (it lies on both sides of both
    periodic faces).  States, as tests/test_gpu_site_chain.py has them on the open device: the filament whole; cut
    narrowly; the narrow cut with one vacancy placed in it; cut widely; no filament (all of it charged).  And one more: the
    stumps of the narrow cut trimmed so that they face each other through the y face (the `skew` state of
    tests/test_gpu_site_gap_pbc.py), with one vacancy placed so that the chain passes that face."""
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
            high = GP.fold(xyz[:, 1], xyz[:, 1].min(), L[1])[1] != 0
            narrow = CR.slab_sites(label, table, x, 2.0)
            skew = (label == fil["root"][0]) & (np.abs(x - mid) <= 8.0) & (((x < mid) & ~high) | ((x > mid) & high))

            def state(el, charge):
                buf.site_element.copy_(torch.as_tensor(el, device="cuda"))
                buf.site_charge.copy_(torch.as_tensor(charge, device="cuda"))
                got = S.filament_chain(comm, buf, NL, NL, R_MAX, max_hops=MAX_HOPS, periodic=True)
                side, node, ref = _restated(dv.neigh, el, charge, d["metals"], xyz, NL, NL, R_MAX, L)
                _full(got, side, node, ref)
                gap = S.filament_gap(comm, buf, NL, NL, R_MAX, periodic=True)["gaps"]
                ch = got["chains"]
                assert np.array_equal(ch["direct2"], gap["gap2"]) and (ch["hop_max2"] <= ch["direct2"]).all()
                assert np.array_equal(ch["n_left"], gap["n_left"]) and np.array_equal(ch["n_right"], gap["n_right"])
                assert np.array_equal(ch["status"] == R.BRIDGED, gap["bridged"] != 0)
                again = S.filament_chain(comm, buf, NL, NL, R_MAX, max_hops=MAX_HOPS, periodic=True)
                assert again["chains"].tobytes() == ch.tobytes() and again["hops"].tobytes() == got["hops"].tobytes()
                print(ch[0], got["hops"][0][:min(ch[0]["n_hops"], MAX_HOPS)])
                return got, side, gap[0]

            def with_a_stone(charge, side, gap, through_a_face):
                cls = CR.classes(element, charge, d["metals"])
                site, d2_left, d2_right = _stone_site(d, element, dv.neigh, cls, side, L, gap["gap2"], through_a_face)
                el = element.copy()
                el[site] = int(CR.VACANCY)
                ch = charge.copy()
                ch[site] = 0
                got, _, gap1 = state(el, ch)
                r, hops = got["chains"][0], got["hops"][0]
                assert gap1["gap2"] == gap["gap2"]                   # the gap does not see the stone
                assert r["status"] == R.CHAINED and r["n_hops"] == 2 and r["hop_max"] < gap["gap"]
                assert hops["to"][0] == site == hops["from"][1]
                assert hops["d2"][:2].tolist() == [d2_left, d2_right] and r["hop_max2"] == max(d2_left, d2_right)
                return [GP.crossings(xyz, h["from"], h["to"], L) != (0, 0) for h in hops[:2]]

            # the filament whole: BRIDGED
            got, _, _ = state(element, charge0)
            r = got["chains"][0]
            assert (r["status"], r["n_hops"], r["hop_max2"], r["direct2"]) == (R.BRIDGED, 0, 0.0, 0.0)
            assert got["stats"]["cells_bridged"] == 1 and (got["hops"]["from"] == -1).all()
            # cut narrowly; and one vacancy in the cut
            charge = charge0.copy()
            charge[narrow] = 2
            got, side, gap = state(element, charge)
            assert got["chains"][0]["status"] == R.CHAINED and 0.0 < gap["gap2"] < R_MAX ** 2
            with_a_stone(charge, side, gap, False)
            # the stumps face each other through the y face; one vacancy so that the chain passes it
            charge[skew] = 2
            got, side, gap = state(element, charge)
            assert GP.crossings(xyz, gap["site_left"], gap["site_right"], L)[0] != 0
            assert any(with_a_stone(charge, side, gap, True))
            # cut widely; no filament
            charge = charge0.copy()
            charge[CR.slab_sites(label, table, x, 12.0)] = 2
            got, _, _ = state(element, charge)
            assert got["chains"][0]["status"] in (R.OPEN, R.CHAINED) and np.isinf(got["chains"][0]["direct2"])
            charge = charge0.copy()
            charge[label == fil["root"][0]] = 2
            got, _, _ = state(element, charge)
            r = got["chains"][0]
            assert np.isinf(r["direct2"]) and r["status"] in (R.OPEN, R.CHAINED) and r["n_left"] > 0 and r["n_right"] > 0
        finally:
            dv.close()
    finally:
        comm.close()


def test_kmc_loop_periodic_workload_with_the_chain():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kmc_loop.py"), "--workload", "5nm-periodic", "--chain", "20",
                          "--chain-hops", "4", "--steps", "2"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "sites 37637" in out.stdout
    steps = [l for l in out.stdout.splitlines() if re.search(r"events [0-9.]+ \(\d+ ev\)", l)]
    assert len(steps) == 2 and all(re.search(r"\| chain [0-9.]+\+[0-9.]+ \(\d+ rounds, \d+ surface\) \[0: ", l) for l in steps), steps
