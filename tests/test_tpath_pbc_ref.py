"""CPU: the periodic dense T-path reference (tests/tpath_pbc_ref.py) against itself and against the open reference
(tests/tpath_ref.py): what every periodic case is built for (BUILT_FOR_PBC; a case that loses its edge fails here), the
open system reproduced where no pair reaches a face, symmetry, row sums, and the distance of every pair from nn_dist
that keeps rounding from deciding a pattern entry.  tests/test_gpu_tpath_pbc.py holds the library to this reference."""
import numpy as np
import pytest

import tpath_pbc_ref as Q
import tpath_ref as R

_printed = set()


@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_case_is_built_for_its_edge(name):
    case = Q.tpath_pbc_case(name)
    ref = Q.case_ref_pbc(name)
    e = ref.edges_pbc()
    if name not in _printed:
        _printed.add(name)
        print("\n%s: %s" % (name, ", ".join("%s=%s" % kv for kv in e.items())))
    assert e["N_atom"] <= 832
    want = case["built_for"]
    for key in ("wrap_bonds", "wrap_tunnel_pairs", "open_pair_now_neighbour", "pairs_at_half_period", "ground_neighbours_through_face",
                "d_at_nn_through_face", "pattern_path"):
        assert key in want, (name, key)
    for k, v in want.items():
        assert e[k] == v, (name, k, e[k], v)
    for k in Q.NONZERO_PBC[name]:
        assert e[k], (name, k)
    # the periods close the crystal: (ny, nz) lattice steps, and the atoms do not span one
    span = ref.pos.max(0) - ref.pos.min(0)
    assert case["L"][1] == span[1] + R.A_LAT and case["L"][2] == span[2] + R.A_LAT
    # atom index != site index, x-ordered atoms (as tests/test_tpath_ref.py asserts of the open cases)
    assert (ref.atom_site != np.arange(ref.N_atom)).any()
    assert np.all(np.diff(ref.pos[:, 0]) > -1e-9)


def test_pbc_nt_65_places_its_pair():
    """The explicit pair: vacancies of one layer at iy 0 and iy 3 -- a tunnel pair at 7.5 A in the open device, a neighbour
    bond at 2.5 A and NO tunnel pair under the minimum image; and the half-period pairs see round() go away from zero."""
    ref = Q.case_ref_pbc("pbc_nt_65")
    up = np.triu(np.ones((ref.n_t, ref.n_t), bool), 1)
    i, j = np.nonzero(ref.open_pair() & (ref.Dt < ref.par["nn_dist"]) & up)
    assert len(i) == 1
    assert ref.Dt_open[i[0], j[0]] == 7.5 and ref.Dt[i[0], j[0]] == 2.5 and not ref.pair[i[0], j[0]]
    a, b = ref.tunnel_idx[i[0]], ref.tunnel_idx[j[0]]
    assert ref.A_pattern[a + 2, b + 2] and ref.A[a + 2, b + 2] == -ref.par["low_G"]      # charged next to neutral
    assert Q.P.c_round(0.5) == 1.0 and Q.P.c_round(-0.5) == -1.0 and np.round(0.5) == 0.0
    y = ref.pos[:, 1]
    k, l = np.nonzero((y[:, None] - y[None, :] == 5.0) & (ref.pos[:, 0][:, None] == ref.pos[:, 0][None, :]) &
                      (ref.pos[:, 2][:, None] == ref.pos[:, 2][None, :]))
    assert len(k) and np.all(ref.D[k, l] == 5.0) and np.all(ref.D[l, k] == 5.0)


@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_periods_beyond_reach_reproduce_the_open_reference(name):
    """No pair reaches a face under a huge period, so TRefPbc must be TRef on the same device.  With periods of 2^30 A
    (1.07e9) the division and the product back are exact and EVERYTHING is reproduced bit for bit.  With periods of 1e9
    the round trip (dy / 1e9) * 1e9 rounds twice and may land one ulp from dy (distances within two ulps): all integer
    work is identical, the neighbour operator is identical, the WKB values agree to the distance's ulp through the
    exponent (~30): rtol 1e-13."""
    case = Q.tpath_pbc_case(name)
    want = R.ref_of(case)
    got = Q.ref_pbc_of(case, L=(2.0 ** 30,) * 3)
    for key in ("D", "A", "A_pattern", "diag_neigh", "rhs", "tunnel_idx", "pair", "S_pattern", "S", "diag_tunnel", "M", "diag", "dinv"):
        np.testing.assert_array_equal(getattr(got, key), getattr(want, key), err_msg=key)
    np.testing.assert_array_equal(got.D, got.D_open)
    got = Q.ref_pbc_of(case, L=(1e9,) * 3)
    for key in ("A", "A_pattern", "diag_neigh", "rhs", "tunnel_idx", "pair", "S_pattern"):
        np.testing.assert_array_equal(getattr(got, key), getattr(want, key), err_msg=key)
    assert np.all(np.abs(got.D - want.D) <= 2 * np.spacing(want.D))
    for key in ("S", "diag_tunnel", "dinv"):
        np.testing.assert_allclose(getattr(got, key), getattr(want, key), rtol=1e-13, atol=0, err_msg=key)
    assert np.all(np.abs(got.M - want.M) <= 1e-13 * np.abs(want.M))


@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_reference_against_itself(name):
    ref = Q.case_ref_pbc(name)
    np.testing.assert_array_equal(ref.D, ref.D.T)                 # d(i, j) and d(j, i): the same bits
    np.testing.assert_array_equal(ref.S, ref.S.T)
    np.testing.assert_array_equal(ref.S_pattern, ref.S_pattern.T)
    np.testing.assert_array_equal(ref.A, ref.A.T)
    np.testing.assert_array_equal(ref.M, ref.M.T)
    assert np.all(ref.D <= ref.D_open)                            # the minimum image is never the longer one ...
    assert (ref.D < ref.D_open).any()
    assert np.all(np.abs(ref.pos[:, None, 0] - ref.pos[None, :, 0]) <= ref.D)      # ... and x is not periodic
    # row sums of M are the ground terms: +high_G in row 0 and in the rows of the ground atom's neighbours, through the
    # faces too; every other row sums to zero (to the rounding of its diagonal)
    rows = ref.M.sum(1)
    scale = np.abs(ref.M).sum(1)
    assert np.all(np.abs(rows - ref.ground.astype(R.LD)) <= 4e-16 * scale)
    na, Na, nn = ref.N_atom - 1, ref.N_atom, ref.par["nn_dist"]
    through = np.flatnonzero((ref.D[:na, Na - 1] < nn) & ~(ref.D_open[:na, Na - 1] < nn))
    assert len(through) and np.all(ref.ground[through + 2] == ref.par["high_G"])
    assert int((ref.ground != 0).sum()) == 1 + ref.edges_pbc()["ground_neighbours"]
    # tunnel block: rows sum to zero, signs
    S = ref.S
    assert np.all(np.abs(S.astype(R.LD).sum(1)) <= 2e-16 * np.abs(S).astype(R.LD).sum(1))
    assert np.all(np.diag(S) >= 0) and np.all(S[~np.eye(ref.n_t, dtype=bool)] <= 0)
    # the open system on the same device is another system: fewer bonds, other WKB values (and, where a pair's status
    # changes, another tunnel pattern)
    op = R.ref_of(Q.tpath_pbc_case(name))
    assert op.A_pattern.sum() < ref.A_pattern.sum() and np.all(ref.A_pattern[op.A_pattern])
    assert (op.S != ref.S).any()
    e = ref.edges_pbc()
    assert (op.S_pattern != ref.S_pattern).any() == bool(e["open_pair_now_neighbour"] + e["open_pair_now_nothing"])


@pytest.mark.parametrize("name", Q.CASES_PBC)
def test_no_pair_within_1e_9_of_nn_dist(name):
    """Where a wrapped distance carries rounding (pbc_group_178: 2.5 / 15 is inexact) no atom pair and no candidate tunnel
    pair may lie within 1e-9 A of nn_dist: neither a fused multiply-add under the kernel's sqrt nor the last bit of a
    division may decide a pattern entry.  The exact cases may hold pairs AT nn_dist (pbc_distance_edges does, through the
    faces, by exact arithmetic); every other pair keeps the margin there too."""
    ref = Q.case_ref_pbc(name)
    assert ref.margin_to_nn() > 1e-9, ref.margin_to_nn()
    nn, na = ref.par["nn_dist"], ref.N_atom - 1
    at = int((ref.D[:na, :ref.N_atom] == nn).sum()) + int((ref.Dt[ref.pair_kind] == nn).sum())
    if name == "pbc_group_178":
        assert at == 0
    if name == "pbc_distance_edges":
        assert at > 0


def test_natural_order_pcg_converges():
    """pcg_natural (the yardstick of the GPU test's residual bar) reaches the tolerance and solves the dense system."""
    for name in ("pbc_nt_65", "pbc_group_178"):
        ref = Q.case_ref_pbc(name, 2.0)
        x, k = Q.pcg_natural_case(name, 2.0, 1e-20)
        assert 0 < k < 20000
        rhs = ref.rhs.astype(R.LD)
        res = float(np.sqrt(((rhs - ref.M @ x.astype(R.LD)) ** 2).sum()))
        assert res <= 1e-14 * float(np.sqrt((rhs ** 2).sum())), (name, res)


# ---- argument errors of the periodic entry point: KMCF_ERR_ARG before the host-only-communicator check --------------------
ERR_ARG, ERR_STATE = -1, -4


@pytest.mark.parametrize("pbc,lattice,want,word", [
    (2, [30.0, 10.0, 10.0], ERR_ARG, b"pbc = 2"), (-1, [30.0, 10.0, 10.0], ERR_ARG, b"pbc = -1"), (1, None, ERR_ARG, b"h_lattice is NULL"),
    (1, [30.0, 0.0, 10.0], ERR_ARG, b"period in y"), (1, [30.0, -10.0, 10.0], ERR_ARG, b"period in y"),
    (1, [30.0, np.inf, 10.0], ERR_ARG, b"period in y"), (1, [30.0, np.nan, 10.0], ERR_ARG, b"period in y"),
    (1, [30.0, 10.0, 0.0], ERR_ARG, b"period in z"), (1, [30.0, 10.0, np.nan], ERR_ARG, b"period in z"),
    (1, [30.0, 10.0, -np.inf], ERR_ARG, b"period in z"),
    # well-formed geometry: the call gets as far as kmcf_initialize_sparsity_T's own refusal of a host-only communicator
    (1, [30.0, 10.0, 10.0], ERR_STATE, b"host-only"), (0, None, ERR_STATE, b"host-only"), (0, [30.0, -1.0, np.nan], ERR_STATE, b"host-only")])
def test_argument_errors_on_a_host_only_communicator(km, pbc, lattice, want, word):
    """The device pointers are never dereferenced: every call returns from the argument checks or from the host-only check
    behind them.  The geometry errors name the _pbc call and the axis; pbc = 0 reads no lattice at all."""
    import ctypes as C
    lib = km.lib.load()
    h = C.c_void_p()
    km.lib.check(lib.kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    try:
        fake = C.c_void_p(64)
        cnt, dsp = (C.c_int * 1)(101), (C.c_int * 1)(0)
        lat = None if lattice is None else (C.c_double * 3)(*lattice)
        out = C.c_void_p()
        rc = lib.kmcf_initialize_sparsity_T_pbc(h, fake, fake, fake, fake, 100, lat, pbc, 3.5, 16, 16, 3, cnt, dsp, C.byref(out))
        msg = lib.kmcf_last_error()
        assert rc == want and word in msg, (rc, msg)
        if want == ERR_ARG:
            assert b"kmcf_initialize_sparsity_T_pbc" in msg, msg
        assert not out.value
    finally:
        lib.kmcf_comm_destroy(h)
    p = C.c_int()
    assert lib.kmcf_tstate_periodic(None, C.byref(p), None) == ERR_ARG and b"kmcf_tstate_periodic" in lib.kmcf_last_error()
