"""CPU: the conditions the inputs and bars of tests/cg_ref.py must meet, asserted on the reference alone.

GPU tests of the solver's scalars (first step length, iterates after 1, 2 and 5 iterations, iteration count) against
tests/cg_ref.py can only see a wrong p.Ap if the INPUTS make every row count: a row whose share of p0.Ap0 is tiny, a
bar looser than what one lost row changes, or a tolerance next to a residual would let a kernel that drops a partial
pass.  Each condition below closes one of these doors, for every system of cg_ref.SYSTEMS."""
import numpy as np
import pytest

import cg_ref as R

LD = np.longdouble
CASES = [(name, v, jac) for name in R.SYSTEMS for v in R.VALUE_SETS for jac in (True, False)]


@pytest.fixture(params=CASES, ids=lambda c: "%s-%s-%s" % (c[0], c[1], "jacobi" if c[2] else "plain"))
def sysm(request):
    return R.system(*request.param)


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is no wider than float64 here: no reference"


def test_builders():
    """Symmetric, diagonal >= 1.5 x the off-diagonal absolute sum, the value sets the kernels' dictionaries need on ONE
    pattern, a long row beyond KMCF_LONG_ROW = 384 and every other row within the row-per-lane kernels' 64 entries."""
    for name in R.SYSTEMS:
        Ms = {v: R.system(name, v, True)["M"] for v in R.VALUE_SETS}
        for v, M in Ms.items():
            assert abs(M - M.T).max() == 0
            d = M.diagonal()
            off = np.abs(M).sum(1).A1 - d
            assert np.all(d >= 1.5 * off) and np.all(d > 0)
            assert np.array_equal(M.indptr, Ms["v3"].indptr) and np.array_equal(M.indices, Ms["v3"].indices)
            offv = M.data[M.indices != np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))]
            nd = len(np.unique(offv))
            assert {"v3": nd == 3, "v5": nd == 5, "f64": nd > 62}[v], (name, v, nd)      # (62 = KMCF_DICT_MAX)
        lens = np.sort(np.diff(Ms["v3"].indptr) - 1)
        if name == "ragged":
            assert Ms["v3"].shape[0] == 6000 and lens[-1] > 384 + 300 and lens[-2] <= 64 and lens[0] >= 1
        elif name == "ragged_nolong":              # (the peer-to-peer group's: its direct halo protocol takes no long rows)
            assert Ms["v3"].shape[0] == 6000 and lens[-1] <= 64 and lens[0] >= 1
        else:
            assert Ms["v3"].shape[0] == 40 and lens[-1] <= 64


def test_reference_solves_the_system(sysm):
    """The reference is a PCG: its recurrence residual is the true one, and it converges."""
    s = sysm
    ref, M = s["ref"], s["M"]
    mv = R._matvec(M, LD)
    for k in (1, 5, 25):
        true_r = s["b"].astype(LD) - mv(ref["x"][k - 1])
        assert np.abs(true_r - ref["r"][k - 1]).max() <= 1e-16 * np.abs(s["b"]).max()
    assert ref["res"][25] <= (1e-10 if s["jacobi"] else 1e-4) and ref["res"][0] > 0.05
    # the first search direction is p0: x1 = alpha0 p0
    assert np.abs(ref["x"][0] / s["p0"].astype(LD) - ref["alpha"][0]).max() <= 2 * R.U * ref["alpha"][0]
    assert s["p0"].min() >= 1.0 - 4 * R.U and s["p0"].max() <= 1.25 + 4 * R.U


def test_row_share(sysm):
    """Every row's term of p0.Ap0 is positive and at least 1 / (100 n) of the sum."""
    t, gamma = R.first_step_terms(sysm["M"], sysm["p0"])
    n = len(t)
    assert t.min() > 0 and float(t.min() / t.sum()) >= 1.0 / (100 * n)
    assert gamma < 10.0                      # |p|^T|A||p| / p^T A p: the bars below scale with it


def test_alpha0_sees_one_lost_row_or_block(sysm):
    """alpha0 = r0.z0 / p0.Ap0 without any one row's term, any one aligned 64-row block's or 256-row block's: it moves
    by at least 1000 x the bar alpha0 is held to (cg_ref.alpha0_bar)."""
    s = sysm
    t, _ = R.first_step_terms(s["M"], s["p0"])
    pAp = t.sum()
    bar = s["a0bar"]
    assert bar <= 1e-11
    for width in (1, 64, 256):
        lost = np.add.reduceat(t, np.arange(0, len(t), width))
        if len(lost) == 1:                      # (fewer rows than the block: nothing is left of p0.Ap0)
            continue
        moved = lost / (pAp - lost)             # relative change of alpha0
        assert float(moved.min()) >= 1000.0 * bar, (width, float(moved.min()), bar)
        # ... and so does one term counted twice
        assert float((lost / (pAp + lost)).min()) >= 1000.0 * bar


@pytest.mark.parametrize("j", [1, 2, 3, 4, 5])
def test_k_step_bar_sees_a_step_length_off_by_1e_9(sysm, j):
    """The reference with iteration j's alpha scaled by (1 + 1e-9) misses the bars of the iterates after 5 iterations."""
    s = sysm
    bad = R.pcg_reference(s["M"], s["b"], s["x0"], s["dinv"], 5, LD, alpha_scale={j: 1.0 + 1e-9})
    dist = R.step_distance(s, 5, bad["x"][4], bad["r"][4], bad["rz"][5])
    bars = R.step_bars(s, 5)
    assert any(dist[q] > bars[q] for q in ("x", "r", "rz")), (dist, bars)


def test_count_tolerance_lies_between_two_residuals(sysm):
    """The tolerance of the count check: the reference's residual at the stopping iteration lies below it by a factor
    >= 2, every earlier one above it by a factor >= 2 -- and the count is one that depends on the step lengths: at
    least 3 iterations, and a first step length off by 1e-5 (one lost row moves it by more) changes it."""
    s = sysm
    j, below, above = R.count_conditions(s["cref"], s["tol"])
    assert j == s["stop"] and j >= 3
    assert below >= 2.0 and above >= 2.0, (below, above)
    bad = R.pcg_reference(s["M"], s["cb"], s["x0"], s["dinv"], 12, LD, alpha_scale={1: 1.0 + 1e-5})
    assert next((i for i, v in enumerate(bad["res"]) if v <= s["tol"]), None) != j       # (later, or not within 12)
    # the float64 run of the same system stops there too
    f64 = R.pcg_reference(s["M"], s["cb"], s["x0"], s["dinv"], 12, np.float64)
    assert R.iterations_to(f64, s["tol"]) == j


def test_count_rhs_on_the_older_tests_matrices():
    """The matrices of test_generic_csr_spmv_and_cg, test_generic_matrix_value_coding and
    test_multirank_generic_matrix_small_and_empty_ranks with cg_ref.count_rhs: the same threshold condition (with their
    own right-hand sides these lower the residual by a steady factor of about 3 per iteration: no tolerance lies a
    factor 2 from both its neighbours)."""
    import test_gpu_edge_cases as E
    import test_gpu_multirank as G
    import test_gpu_spmv_formats as F
    mats = [E._random_spd(5000, np.random.default_rng(9), lr) for lr in (False, True)]
    mats.append(F._banded(20000, np.random.default_rng(11), np.array([-1.0, -1e-8, -0.25])))
    mats += [G._tridiagonal(n) for n in (10, 3, 2000)]
    for M in mats:
        ref, tol, stop = R.count_case(M)
        j, below, above = R.count_conditions(ref, tol)
        assert j == stop and j >= min(3, M.shape[0] - 1) and below >= 2.0 and above >= 2.0, (M.shape, j, below, above)


def test_first_step_bars_see_one_lost_row(sysm):
    """bb and the returned r.z of the one-iteration solve: bars far below what a step length without one row's term
    does to r1.z1 (and the float64 run passes them)."""
    s = sysm
    bars = R.first_step_bars(s)
    assert bars["bb"] <= 2e-12 and bars["rz"] <= 1e-8
    t, _ = R.first_step_terms(s["M"], s["p0"])
    worst = 1.0 + float(t.min() / (t.sum() - t.min()))            # alpha0 without the smallest row term
    bad = R.pcg_reference(s["M"], s["b"], s["x0"], s["dinv"], 1, LD, alpha_scale={1: worst})
    assert R.rel(bad["rz"][1], s["ref"]["rz"][1]) >= 1000.0 * bars["rz"]
    f64 = s["f64"]
    assert R.rel(f64["rz"][1], s["ref"]["rz"][1]) <= bars["rz"] and R.rel(f64["bb"], s["ref"]["bb"]) <= bars["bb"]
