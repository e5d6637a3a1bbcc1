"""GPU: the register-resident PCG launch (csrc/kmcf_cgr.hip) on the synthetic systems of tests/cgr_cases.py -- tile
shapes, (NQ, ND) instances, window stretches, sibling columns, block counts, reduction groups, start vectors, stopping
rules and the state a launch leaves for the next -- off the 5 nm K matrix, which fixes one instance, 128-row tiles and
x0 = 0 for every other test of this launch.

Every knob that bears on the path is set (_force), and before anything is compared the library's own plan is held to
what the case is about (_plan): resident_tpb, resident_g1, the tiles and the row order against their CPU restatement
(cgr_cases.restate_plan / expected_resident), sell_active, sell_ident, cg_variant.  A case that ran the loop of kernels,
another tile shape or another reduction tree fails there.  Each solve is then held to

  a. the oracle adding in the device's order (oracle.pcg_device_order on the library's own plan), bit for bit:
     iteration count, x, r, r.z, b.b, converged -- both recurrences;
  b. the long-double reference computed from the CALLER's CSR (tests/cg_ref.py): checks (a), (b), (c) of
     tests/test_gpu_cg_paths.py, restated (_check) with the bars of cg_ref and no other tolerance -- r.z takes its
     derived first-step bound where cgr_cases.step_bars shows on the CPU that numpy's own distance is a lucky draw;
  c. the loop of kernels on the same matrix object (KMCF_CG_RESIDENT=0 + replan): the count solve stops where the
     reference does, x after five iterations lies within the bar of (b).

tests/test_cgr_cases_ref.py shows on the CPU that one lost edge entry moves r by more than 100 x its bar and one lost
row alpha0 by more than 4 x its bar.  Every case prints its plan and its ratios; the module's last test prints the
worst ratio per test (DESIGN.md section 5 quotes them)."""
import numpy as np
import pytest

import cg_ref as R
import cgr_cases as G
from conftest import assert_solve_bit_identical

pytestmark = pytest.mark.gpu

LD = np.longdouble
VARIANTS = ("classic", "cg1r")
TPBS = (1, 2, 4)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _force(monkeypatch, rows, variant, tpb=None, g1=None, resident="1", delay=None):
    """Every knob that bears on the path, explicitly (None: unset, the library's default)."""
    delay = None if delay is None else str(delay)
    knobs = dict(KMCF_SPMV_KIND="2", KMCF_SPMV_CODED="1", KMCF_SPMV_SELL="1", KMCF_SPMV_SELLV="1", KMCF_SPMV_SELL_ROWS=str(rows),
                 KMCF_SPMV_SELL_SORT=None, KMCF_SPMV_NT=None, KMCF_SELL_NT=None, KMCF_SELL_PACK=None, KMCF_LONG_ROW=None,
                 KMCF_CG_VARIANT=variant, KMCF_CG_XBATCH=None, KMCF_CG_RESIDENT=resident,
                 KMCF_CGR_TPB=None if tpb is None else str(tpb), KMCF_CGR_G1=None if g1 is None else str(g1),
                 KMCF_CGR_DELAY=delay, KMCF_CGR_RDELAY=delay, KMCF_CGR_ADAPT=delay, KMCF_CGR_TIMEOUT_MS=None,
                 KMCF_CGR_CLASSIC_TILES=None, KMCF_DEVICE_SHARE=None, KMCF_FORCE_COMM=None, KMCF_TRANSPORT=None)
    for k, v in knobs.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


class _Case:
    """One matrix object of the system s under forced knobs; closes what it opened."""

    def __init__(self, km, torch, monkeypatch, s, variant, tpb=None, g1=None, delay=None):
        self.km, self.torch, self.monkeypatch, self.s, self.variant, self.tpb, self.g1 = km, torch, monkeypatch, s, variant, tpb, g1
        _force(monkeypatch, s["rows"], variant, tpb, g1, delay=delay)
        S = km.solvers
        M = s["M"]
        n = M.shape[0]
        self.comm = S.KMC_comm(n, n, n, n)
        self.comm.connect()
        self.mat = S.Distributed_matrix(self.comm, n, [n], [0], M.indices, M.indptr, M.data)
        self.label = "%s/%s/tpb=%s/g1=%s" % (s["name"], variant, tpb, g1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.mat.close()
        self.comm.close()

    def plan(self):
        """The library's plan, held to the case BEFORE any comparison; returns it (with the CSR: the oracle's input)."""
        s = self.s
        plan = self.mat.sum_plan()
        tpb, g1, blocks, groups = G.expected_resident(len(s["tiles"]), self.tpb, self.g1)
        print("cgr %s: plan resident_tpb %d resident_g1 %d tiles %d (expected %d / %d / %d: %d blocks, %d groups) sell_active %d "
              "sell_ident %d cg_variant %d" % (self.label, plan["resident_tpb"], plan["resident_g1"], len(plan["tile_rows"]), tpb, g1,
                                               len(s["tiles"]), blocks, groups, plan["sell_active"], plan["sell_ident"], plan["cg_variant"]))
        assert plan["resident_tpb"] == tpb and plan["resident_g1"] == g1, (plan["resident_tpb"], plan["resident_g1"], tpb, g1)
        assert list(plan["tile_rows"]) == [nr for _, nr, _ in s["tiles"]] and list(plan["tile_first"]) == [r0 for r0, _, _ in s["tiles"]]
        assert plan["sell_active"] == 1 and plan["sell_ident"] == 1
        assert plan["cg_variant"] == (1 if self.variant == "cg1r" else 0)
        assert plan["n_short"] == plan["rows"] == s["M"].shape[0] and plan["halo_cols"] == 0 and plan["long_items"] == 0
        assert np.array_equal(plan["perm"], s["perm"]), "the row order is not the restated one"
        info = self.mat.info()
        assert info["spmv_kind"] == 2 and info["spmv_coded"] == 2 and info["spmv_tiles"] == len(s["tiles"]), info
        assert info["spmv_window_cols"] == sum(len(w) for _, _, w in s["tiles"]), info["spmv_window_cols"]
        return plan

    def solve(self, b, x0, dinv, tol, max_it, fixed=0):
        torch = self.torch
        r = torch.as_tensor(np.array(b, dtype=np.float64), device="cuda")
        x = torch.as_tensor(np.array(x0, dtype=np.float64), device="cuda")
        di = None if dinv is None else torch.as_tensor(np.array(dinv), device="cuda")
        st = self.km.solvers.conjugate_gradient_jacobi(self.mat, r, x, di, tol, max_it, fixed_iters=fixed)
        return st, x.cpu().numpy(), r.cpu().numpy()

    def solve_a(self, oracle, plan, b, x0, dinv, tol, max_it, fixed=0, what=""):
        """One solve, held to the device-order oracle bit for bit (check a); returns (st, x, r, oracle's result)."""
        st, x, r = self.solve(b, x0, dinv, tol, max_it, fixed)
        orc = oracle.pcg_device_order(plan, b, x0, dinv, tol, max_it, fixed_iters=fixed, variant=self.variant)
        print("cgr %s: %s iterations %d (oracle %d) converged %d rz %.17g (oracle %.17g) relres %.3e"
              % (self.label, what, st["iterations"], orc["iterations"], st["converged"], st["rz"], orc["rz"], st["relres"]))
        assert_solve_bit_identical(st, x, r, orc)
        return st, x, r, orc

    def runs(self, oracle, plan, steps=R.K_STEPS, count=True):
        """The solves of check (b), each also through check (a): k fixed iterations for every k, then the count solve."""
        s = self.s
        out = {k: self.solve_a(oracle, plan, s["b"], s["x0"], s["dinv"], 1e-30, 0, k, "fixed %d:" % k)[:3] for k in steps}
        if count:
            out["count"] = self.solve_a(oracle, plan, s["cb"], np.zeros(len(s["cb"])), s["dinv"], s["tol"], 100, 0, "count:")[:3]
        return out

    def loop(self, bad):
        """Check (c): the loop of kernels on this matrix object."""
        s = self.s
        _force(self.monkeypatch, s["rows"], self.variant, self.tpb, self.g1, resident="0")
        self.mat.replan()
        plan = self.mat.sum_plan(with_csr=False)
        assert plan["resident_tpb"] == 0 and plan["sell_active"] == 1 and plan["cg_variant"] == (1 if self.variant == "cg1r" else 0), plan
        st, _, _ = self.solve(s["cb"], np.zeros(len(s["cb"])), s["dinv"], s["tol"], 100)
        st5, x5, _ = self.solve(s["b"], s["x0"], s["dinv"], 1e-30, 0, 5)
        dist, bar = R.rel_max(x5, s["ref"]["x"][4]), G.step_bars(s, 5)[0]["x"]
        print("cgr %s: loop of kernels: count %d (reference %d), x after 5 iterations off by %.2e (bar %.2e)"
              % (self.label, st["iterations"], s["stop"], dist, bar))
        if st["iterations"] != s["stop"] or st["converged"] != 1:
            bad.append("loop: solve to %.3e took %d iterations (converged %d), the reference takes %d" % (s["tol"], st["iterations"], st["converged"], s["stop"]))
        if st5["iterations"] != 5 or not dist <= bar:
            bad.append("loop: x after 5 iterations off by %.3e, bar %.3e" % (dist, bar))


WORST = {}          # test -> worst measured ratio of check (b), printed by the last test of the module


def _check(s, runs, label, test, steps=R.K_STEPS):
    """Checks (a), (b), (c) of tests/test_gpu_cg_paths.py on the results of _Case.runs, restated from that module's
    _check with ONE difference: the bars of (b) come from cgr_cases.step_bars, which hands r.z its derived bound where a
    permuted-order float64 run on the CPU shows numpy's own distance to be a lucky draw.  Every figure is printed
    before anything is asserted."""
    ref, bad = s["ref"], []
    # a. first step
    st, x1, _ = runs[1]
    a0 = x1 / s["p0"]
    spread = float((a0.max() - a0.min()) / np.spacing(a0.min()))
    err = float(np.abs(a0.astype(LD) - ref["alpha"][0]).max() / ref["alpha"][0])
    fb = R.first_step_bars(s)
    e_bb, e_rz = R.rel(st["bb"], ref["bb"]), R.rel(st["rz"], ref["rz"][1])
    print("cgr %s: alpha0 %.17g err %.2e (bar %.2e) spread %.1f ulp; bb err %.2e (bar %.2e); rz1 err %.2e (bar %.2e)"
          % (label, float(a0[0]), err, s["a0bar"], spread, e_bb, fb["bb"], e_rz, fb["rz"]))
    if st["iterations"] != 1:
        bad.append("fixed_iters=1 ran %d iterations" % st["iterations"])
    if not spread <= 2.0:
        bad.append("alpha0 = x1 / p0 differs between entries by %.1f ulp" % spread)
    if not err <= s["a0bar"]:
        bad.append("alpha0 off by %.3e, bar %.3e" % (err, s["a0bar"]))
    if not e_bb <= fb["bb"]:
        bad.append("bb off by %.3e, bar %.3e" % (e_bb, fb["bb"]))
    if not e_rz <= fb["rz"]:
        bad.append("r.z after one iteration off by %.3e, bar %.3e" % (e_rz, fb["rz"]))
    # b. iterates
    for k in steps:
        st, x, r = runs[k]
        if st["iterations"] != k:
            bad.append("fixed_iters=%d ran %d iterations" % (k, st["iterations"]))
        bad += _iterates(s, k, x, r, st["rz"], label, test)
    # c. count
    st = runs["count"][0]
    print("cgr %s: count %d (reference %d, tolerance %.2e, relres %.2e)" % (label, st["iterations"], s["stop"], s["tol"], st["relres"]))
    if st["iterations"] != s["stop"] or st["converged"] != 1:
        bad.append("solve to %.3e: %d iterations (converged %d), the reference takes %d" % (s["tol"], st["iterations"], st["converged"], s["stop"]))
    return bad


def _iterates(s, k, x, r, rz, label, test, only=("x", "r", "rz")):
    """Check (b) after k iterations; the ratio printed and recorded is device distance / float64-numpy distance (the
    bar of 16 where the bar is not a derived one)."""
    ref, f64 = s["ref"], s["f64"]
    dist = R.step_distance(s, k, x, r, rz)
    bars, derived = G.step_bars(s, k)
    f64d = dict(x=R.rel_max(f64["x"][k - 1], ref["x"][k - 1]), r=R.rel_max(f64["r"][k - 1], ref["r"][k - 1]), rz=R.rel(f64["rz"][k], ref["rz"][k]))
    ratio = {q: dist[q] / f64d[q] if f64d[q] > 0 else (0.0 if dist[q] == 0 else np.inf) for q in only}
    for q in only:
        key = test + (" (derived bar)" if q in derived else "")
        WORST[key] = max(WORST.get(key, 0.0), ratio[q])
    print("cgr %s: k=%d distance / float64's  %s   (distances %s; bars %s; derived: %s; permuted float64 runs reach %s)"
          % (label, k, "  ".join("%s %.2f" % (q, ratio[q]) for q in only), " ".join("%.2e" % dist[q] for q in only),
             " ".join("%.2e" % bars[q] for q in only), ",".join(derived) or "-",
             " ".join("%.2f" % (G.order_spread(s, k)[q] / f64d[q] if f64d[q] > 0 else np.inf) for q in only)))
    return ["k=%d: %s off by %.3e, bar %.3e (%.1f x float64's distance)" % (k, q, dist[q], bars[q], ratio[q]) for q in only if not dist[q] <= bars[q]]


def _edge_rows(s, r1, label, bad):
    """r after ONE iteration, row by row on the rows that hold the case's edge entries, to the bar check (b) holds r to
    (relative to the reference's largest entry: that check's norm)."""
    ref = s["ref"]["r"][0]
    bar = G.step_bars(s, 1)[0]["r"]
    scale = float(np.abs(ref).max())
    for i in sorted({i for i, _ in s["edges"]}):
        err = float(abs(LD(r1[i]) - ref[i])) / scale
        print("cgr %s: edge row %d: r1 off by %.2e (bar %.2e)" % (label, i, err, bar))
        if not err <= bar:
            bad.append("edge row %d: r after one iteration off by %.3e, bar %.3e" % (i, err, bar))


def _full(km, torch, monkeypatch, oracle, s, variant, tpb, test, edges=False):
    """Checks (a), (b), (c) on one system at one launch shape."""
    with _Case(km, torch, monkeypatch, s, variant, tpb) as c:
        plan = c.plan()
        runs = c.runs(oracle, plan)
        bad = _check(s, runs, c.label, test)
        if edges:
            assert s["edges"] or s["name"] == "win/w0"
            _edge_rows(s, runs[1][2], c.label, bad)
        c.loop(bad)
    assert not bad, "\n".join([c.label] + bad)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tpb", (None,) + TPBS, ids=lambda t: "tpb=%s" % t)
@pytest.mark.parametrize("key", list(G.INSTANCES))
def test_instances(km, torch, monkeypatch, oracle, key, tpb, variant):
    """The six (NQ, ND) instances and the one-value dictionary, at 64-, 128- and 256-row tiles, at the planner's own
    choice of tiles per block and at 1 / 2 / 4."""
    s = G.system("inst", key)
    _full(km, torch, monkeypatch, oracle, s, variant, tpb, "instances", edges=bool(s["edges"]))


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tpb", TPBS, ids=lambda t: "tpb=%s" % t)
@pytest.mark.parametrize("key", list(G.WINDOWS))
def test_window_stretches(km, torch, monkeypatch, oracle, key, tpb, variant):
    """A tile of 0, 256, 257, 512, 513 and 767 outside columns (0 ... 3 stretches of the window, the last one holding one
    column, all or all but one), a last tile of one row and one of 100; r of the rows that read the last column of
    every stretch, row by row."""
    _full(km, torch, monkeypatch, oracle, G.system("win", key), variant, tpb, "window_stretches", edges=True)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("tpb", TPBS, ids=lambda t: "tpb=%s" % t)
def test_sibling_columns(km, torch, monkeypatch, oracle, tpb, variant):
    """Rows that reference the first and the last row of their block (another tile of it: from LDS where a block holds
    several tiles) and the first row of the next block (through the granules), for blocks of two and of four tiles;
    with one tile per block all of them travel through the granules."""
    _full(km, torch, monkeypatch, oracle, G.system("sib", "sib"), variant, tpb, "sibling_columns", edges=True)


def _sums(km, torch, monkeypatch, oracle, nt, tpb, g1, variant, test):
    """Block and group tables: check (a) at five fixed iterations and at a tolerance solve; check (b) for b.b and r.z
    (after one iteration to their derived bars, after five to 16 x float64's distance); b.b of an all-ones b is n."""
    s = G.system("blocks", str(nt))
    n = s["M"].shape[0]
    with _Case(km, torch, monkeypatch, s, variant, tpb, g1) as c:
        plan = c.plan()
        st1 = c.solve_a(oracle, plan, s["b"], s["x0"], s["dinv"], 1e-30, 0, 1, "fixed 1:")[0]
        st5 = c.solve_a(oracle, plan, s["b"], s["x0"], s["dinv"], 1e-30, 0, 5, "fixed 5:")[0]
        stt = c.solve_a(oracle, plan, s["b"], s["x0"], s["dinv"], 1e-9, 100, 0, "to 1e-9:")[0]
        ones = c.solve_a(oracle, plan, np.ones(n), np.zeros(n), s["dinv"], 1e-30, 0, 1, "ones:")[0]
    ref, fb = s["ref"], R.first_step_bars(s)
    e_bb, e_rz1 = R.rel(st1["bb"], ref["bb"]), R.rel(st1["rz"], ref["rz"][1])
    print("cgr %s: bb err %.2e (bar %.2e); rz1 err %.2e (bar %.2e); solve to 1e-9: %d iterations (reference %d); bb of ones %.17g"
          % (c.label, e_bb, fb["bb"], e_rz1, fb["rz"], stt["iterations"], R.iterations_to(ref, 1e-9), ones["bb"]))
    bad = _iterates(s, 5, ref["x"][4], ref["r"][4], st5["rz"], c.label, test, only=("rz",))
    assert e_bb <= fb["bb"] and e_rz1 <= fb["rz"] and not bad, bad
    assert st5["bb"] == st1["bb"] == stt["bb"]
    assert stt["converged"] == 1 and stt["relres"] <= 1e-9
    assert ones["bb"] == float(n)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nt,tpb", G.BLOCK_CASES, ids=lambda v: str(v))
def test_block_counts(km, torch, monkeypatch, oracle, nt, tpb, variant):
    """1, 3, 5, 64, 65, 128, 129, 256 blocks of one 64-row tile (flat reduction: the lane and wave edges of 'lane l of
    wave w reads block 64 w + l'), 257 (two hops, 17 groups of 16, the last of one block); last blocks of ONE active tile
    out of two or four; fewer tiles than a block holds."""
    _sums(km, torch, monkeypatch, oracle, nt, tpb, None, variant, "block_counts")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("nt,g1,want,groups", G.G1_CASES, ids=lambda v: str(v))
def test_group_reduction(km, torch, monkeypatch, oracle, nt, g1, want, groups, variant):
    """KMCF_CGR_G1 on 256, 257 and 65 blocks: exactly 64 groups (no doubling), 65 (doubled to 33 of 8), a request of 2
    (doubled twice), groups of 64 with a partial last one."""
    assert G.expected_resident(nt, 1, g1) == (1, want, nt, groups)
    _sums(km, torch, monkeypatch, oracle, nt, 1, g1, variant, "group_reduction")


@pytest.mark.parametrize("scenario", ["x0-random", "x0-solution", "b-zero", "max-it"])
@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "plain"])
@pytest.mark.parametrize("variant", VARIANTS)
def test_start_and_stop(km, torch, monkeypatch, oracle, variant, jacobi, scenario):
    """One matrix of 1300 rows in 256-row tiles (the planner's launch: one tile per block), with the Jacobi
    preconditioner and without (dinv = None: A.dinv == nullptr in the kernel).

    b-zero (b = 0, x0 = 0, tolerance 1e-10): both the resident launch and the loop of kernels return iterations = 0 and
    converged = 1 -- the loop condition r.z / b.b > tol^2 is 0 / 0 > tol^2, false, in both, as in the oracle -- with x
    and r exactly 0.  relres = sqrt(r.z / b.b) was NaN on both paths until pcg_collect learnt to report 0 for 0 / 0."""
    s = G.system(*G.START_STOP, jacobi)
    n = s["M"].shape[0]
    zero = np.zeros(n)
    bad = []
    with _Case(km, torch, monkeypatch, s, variant) as c:
        plan = c.plan()
        if scenario == "x0-random":
            sx = G.make_system(s["M"], jacobi, x0=G.start_vector(s), count=False)
            for k in R.K_STEPS:
                st, x, r, _ = c.solve_a(oracle, plan, sx["b"], sx["x0"], sx["dinv"], 1e-30, 0, k, "x0 random, fixed %d:" % k)
                bad += _iterates(sx, k, x, r, st["rz"], c.label, "start_and_stop")
            # the count solve from x0: b = A x0 + the count check's right-hand side, so that r0 is that right-hand side
            cs = G.count_from(s, sx["x0"])
            st = c.solve_a(oracle, plan, cs["b"], sx["x0"], sx["dinv"], cs["tol"], 100, 0, "x0 random, count:")[0]
            print("cgr %s: x0 random: count %d (reference %d, tolerance %.2e)" % (c.label, st["iterations"], cs["stop"], cs["tol"]))
            assert st["iterations"] == cs["stop"] and st["converged"] == 1
        elif scenario == "x0-solution":
            xs = G.solution(s)
            st, x, _, _ = c.solve_a(oracle, plan, s["b"], xs, s["dinv"], G.SOLVED_TOL, 100, 0, "x0 = solution:")
            moved, bar = float(np.abs(x - xs).max() / np.abs(xs).max()), G.step_bars(s, 5)[0]["x"]
            print("cgr %s: x0 = solution: %d iterations, x moved by %.2e (bar %.2e)" % (c.label, st["iterations"], moved, bar))
            assert st["iterations"] in (0, 1) and st["converged"] == 1 and moved <= bar
        elif scenario == "b-zero":
            st, x, r, _ = c.solve_a(oracle, plan, zero, zero, s["dinv"], 1e-10, 100, 0, "b = 0:")
            _force(monkeypatch, s["rows"], variant, resident="0")
            c.mat.replan()
            assert c.mat.sum_plan(with_csr=False)["resident_tpb"] == 0
            lst, lx, lr = c.solve(zero, zero, s["dinv"], 1e-10, 100)
            print("cgr %s: b = 0: resident %r, loop %r" % (c.label, st, lst))
            for name, t, xv, rv in (("resident", st, x, r), ("loop", lst, lx, lr)):
                assert not xv.any() and not rv.any(), name
                assert all(np.isfinite(t[q]) for q in ("iterations", "converged", "bb", "rz", "relres")), (name, t)
                assert (t["iterations"], t["converged"], t["bb"], t["rz"], t["relres"]) == (0, 1, 0.0, 0.0, 0.0), (name, t)
        else:
            st, x, r, orc = c.solve_a(oracle, plan, s["b"], s["x0"], s["dinv"], 1e-30, 7, 0, "max_it 7:")
            print("cgr %s: max_it 7: relres %.17g, oracle %.17g, reference %.17g" % (c.label, st["relres"], orc["relres"], s["ref"]["res"][7]))
            assert st["iterations"] == 7 and st["converged"] == 0
            assert st["relres"] == orc["relres"]
            np.testing.assert_allclose(st["relres"], s["ref"]["res"][7], rtol=1e-12)
    assert not bad, "\n".join([c.label] + bad)


@pytest.mark.parametrize("variant", VARIANTS)
def test_back_to_back(km, torch, monkeypatch, oracle, variant):
    """ONE matrix object (129 tiles of 64 rows, two per block: 65 blocks, the last of one tile), one resident plan, no
    replan in between: fixed 1, 2 and 3 iterations (publication and reduction counts of both parities), a tolerance
    solve, three tolerance solves with max_it = 1 000 000 000, set_values to other values of the same three-value set
    and back.  Every solve is bit-identical to the stateless oracle for its own inputs: nothing a launch leaves in the
    granule buffers, the slots or the sequence word reaches the next.
    The second and third of the max_it = 1e9 solves take the clearing branch of kmcf_cgr_solve: the host's bound of
    the sequence number advances by 3 max_it + 16 per solve whatever the solve used, and the branch is taken once
    bound + 3 max_it + 32 > 0xf0000000 -- 3e9 + 32 < 0xf0000000 = 4 026 531 840 for the first (not taken), 6e9 + 48
    beyond it for the second and, the bound restarting at 0 + 3e9 + 16, for the third.  This is derived from the code
    and not observed: the test cannot see which branch ran.  The three solve to 1e-6, 1e-8 and 1e-10, so each runs longer
    than the one before (asserted): the third, its sequence numbers starting over, passes through the numbers the
    second ended on -- where a branch that forgot its memsets would have left that solve's granules, in the buffers
    of the same parity.  The first polls are not delayed here (KMCF_CGR_DELAY = KMCF_CGR_RDELAY = KMCF_CGR_ADAPT = 0): a
    poll that comes before the writer is what would take such a granule for the new one.  Whether one does is a race;
    a launch that passes has not been shown to clear its buffers."""
    s = G.system("blocks", "129")
    n = s["M"].shape[0]
    zero = np.zeros(n)
    M2 = R._finish(s["M"].astype(bool).astype(float).tocsr(), np.random.default_rng(99), R.VALUES3)
    assert np.array_equal(M2.indices, s["M"].indices) and np.array_equal(M2.indptr, s["M"].indptr) and np.any(M2.data != s["M"].data)
    rng = np.random.default_rng(5)
    with _Case(km, torch, monkeypatch, s, variant, tpb=2, delay=0) as c:
        plan = c.plan()
        for k in (1, 2, 3):
            c.solve_a(oracle, plan, s["b"], zero, s["dinv"], 1e-30, 0, k, "fixed %d:" % k)
        c.solve_a(oracle, plan, s["b"], zero, s["dinv"], 1e-9, 100, 0, "tolerance:")
        its = []
        for q, tol in enumerate((1e-6, 1e-8, 1e-10)):
            st = c.solve_a(oracle, plan, rng.standard_normal(n), zero, s["dinv"], tol, 1_000_000_000, 0, "max_it 1e9 (%d):" % q)[0]
            assert st["converged"] == 1
            its.append(st["iterations"])
        assert 3 <= its[0] < its[1] < its[2] <= 60, its
        c.mat.set_values(M2.data)
        plan2 = c.mat.sum_plan()
        assert plan2["resident_tpb"] == 2 and plan2["sell_active"] == 1 and np.array_equal(plan2["perm"], plan["perm"])
        assert not np.array_equal(plan2["val"], plan["val"])
        assert np.array_equal(c.mat.get_values(), M2.data)
        st = c.solve_a(oracle, plan2, s["b"], zero, 1.0 / M2.diagonal(), 1e-9, 100, 0, "after set_values:")[0]
        assert st["converged"] == 1
        c.mat.set_values(s["M"].data)
        plan3 = c.plan()
        assert np.array_equal(plan3["val"], plan["val"])
        c.solve_a(oracle, plan3, s["b"], zero, s["dinv"], 1e-30, 0, 2, "values set back, fixed 2:")
        st = c.solve_a(oracle, plan3, s["b"], zero, s["dinv"], 1e-9, 100, 0, "values set back, tolerance:")[0]
        assert st["converged"] == 1


def test_zz_report_measured_ratios():
    """Prints the worst ratio of check (b) per test over the cases that ran (DESIGN.md section 5 quotes them)."""
    for key in sorted(WORST):
        print("cgr worst ratio %s: %.2f" % (key, WORST[key]))
