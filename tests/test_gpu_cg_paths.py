"""GPU: the fused p.Ap partial sums and the CG iterates of every interior SpMV kernel, against a plain reference.

kmcf_interior_path picks one of six kernels for the interior rows (vec, stream, window, coded window, row per lane
coded, row per lane f64).  Inside a solve each of them also produces p.Ap partials (DOT), on a rank group in an
instance that skips the boundary rows, some in a nontemporal instance; the boundary pass, the long-row kernel and the
consumer's partial counts complete the sum.  A wrong p.Ap is a wrong step length: the solve stays consistent
(x += a p, r -= a Ap for any a) and still converges on a well-conditioned matrix, only later -- so convergence and a
final residual do not see it.  Here the scalars themselves are held to tests/cg_ref.py (long double):

  a. the first step length alpha0 = x1 / p0, entry by entry, with b.b and the returned r.z, to a-priori rounding bounds;
  b. x, r and r.z after 1, 2 and 5 iterations, to 16 x the distance of numpy's float64 run from the reference (r.z
     after ONE iteration to the derived bound of (a): cg_ref.step_bars says why);
  c. the iteration count of a solve whose tolerance lies a factor >= 2 from the reference's residuals on both sides;
  d. all of it again after every step of a walk of ONE matrix object through the paths (set_values, kmcf_spmv_replan).

tests/test_cg_ref.py holds the inputs to the conditions that make these checks see one lost row.  The path of every
case is read back from the library (kmcf_matrix_info, kmcf_matrix_sum_plan), never assumed.  The solves run as the
loop of kernels (KMCF_CG_RESIDENT=0; the resident launch has tests/test_gpu_cgr_synthetic.py).  Rank groups are
the in-process loopback group on one GPU; several GPUs stay unmeasured here.

Every case prints its ratios of (b), device distance / float64-numpy distance (bar: 16), and the module's last test
the worst per path; DESIGN.md section 5 ("What holds the solver's scalars") records them."""
import threading

import numpy as np
import pytest

import cg_ref as R

pytestmark = pytest.mark.gpu

LD = np.longdouble
# path -> (value set of the matrix, KMCF_SPMV_* knobs that force it, what kmcf_matrix_info must then say)
PATHS = {
    "vec": dict(values="f64", env=dict(KIND=0), kind=0, coded=0, lane=False),
    "stream": dict(values="f64", env=dict(KIND=1), kind=1, coded=0, lane=False),
    "window": dict(values="f64", env=dict(KIND=2, SELLV=0), kind=2, coded=0, lane=False),
    "wcode": dict(values="v5", env=dict(KIND=2), kind=2, coded=1, lane=False),         # 5 values: beyond the lane kernel's 3
    "sell": dict(values="v3", env=dict(KIND=2), kind=2, coded=2, lane=True),
    "sellv": dict(values="f64", env=dict(KIND=2, SELLV=1), kind=2, coded=0, lane=True),
}
VARIANTS = ("classic", "cg1r")
WORST = {}          # path -> worst measured ratio of check (b), printed by the last test of the module


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _force(monkeypatch, env, variant, nt=None):
    """Every knob that bears on the path, explicitly: the session's environment decides nothing here."""
    knobs = dict(KMCF_SPMV_KIND=None, KMCF_SPMV_CODED="1", KMCF_SPMV_SELL="1", KMCF_SPMV_SELLV="1",
                 KMCF_SPMV_SELL_ROWS=None, KMCF_SPMV_SELL_SORT=None, KMCF_SPMV_NT=None, KMCF_SELL_NT=None,
                 KMCF_LONG_ROW=None, KMCF_CG_VARIANT=variant, KMCF_CG_RESIDENT="0")
    knobs.update({"KMCF_SPMV_" + k: str(v) for k, v in env.items()})
    knobs.update(nt or {})
    for k, v in knobs.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)


def _path_errors(path, variant, info, plan, long_row, label):
    """What the library says it runs, against what the case is about."""
    spec, bad = PATHS[path], []
    if info["spmv_kind"] != spec["kind"] or info["spmv_coded"] != spec["coded"]:
        bad.append("%s: spmv_kind %d coded %d, wanted %d / %d" % (label, info["spmv_kind"], info["spmv_coded"], spec["kind"], spec["coded"]))
    if (info["spmv_stream_entries"] > 0) != (spec["lane"] or path == "wcode"):
        bad.append("%s: spmv_stream_entries %d" % (label, info["spmv_stream_entries"]))
    if bool(plan["sell_active"]) != spec["lane"]:
        bad.append("%s: sell_active %d" % (label, plan["sell_active"]))
    if (plan["long_items"] > 0) != long_row:
        bad.append("%s: long_items %d" % (label, plan["long_items"]))
    if plan["resident_tpb"] != 0 or plan["cg_variant"] != (1 if variant == "cg1r" else 0):
        bad.append("%s: resident_tpb %d cg_variant %d" % (label, plan["resident_tpb"], plan["cg_variant"]))
    return bad


def _solve(km, torch, mat, b, dinv, tol, max_it, fixed):
    r = torch.as_tensor(np.array(b), device="cuda")
    x = torch.zeros_like(r)
    di = None if dinv is None else torch.as_tensor(np.array(dinv), device="cuda")
    st = km.solvers.conjugate_gradient_jacobi(mat, r, x, di, tol, max_it, fixed_iters=fixed)
    return st, x.cpu().numpy(), r.cpu().numpy()


def _runs(km, torch, mat, s, sl=slice(None), steps=R.K_STEPS):
    """The solves of one case on one rank (rows sl): k iterations from x0 = 0 for every k, then the count solve."""
    dinv = None if s["dinv"] is None else s["dinv"][sl]
    out = {k: _solve(km, torch, mat, s["b"][sl], dinv, 1e-30, 0, k) for k in steps}
    out["count"] = _solve(km, torch, mat, s["cb"][sl], dinv, s["tol"], 100, 0)
    return out


def _check(s, runs, label, path, steps=R.K_STEPS):
    """Checks (a), (b), (c) of the module docstring on the (gathered) results of _runs; every figure is printed before
    anything is asserted."""
    ref, bad = s["ref"], []
    # a. first step
    st, x1, _ = runs[1]
    a0 = x1 / s["p0"]
    spread = float((a0.max() - a0.min()) / np.spacing(a0.min()))
    err = float(np.abs(a0.astype(LD) - ref["alpha"][0]).max() / ref["alpha"][0])
    fb = R.first_step_bars(s)
    e_bb, e_rz = R.rel(st["bb"], ref["bb"]), R.rel(st["rz"], ref["rz"][1])
    print("cg-paths %s: alpha0 %.17g err %.2e (bar %.2e) spread %.1f ulp; bb err %.2e (bar %.2e); rz1 err %.2e (bar %.2e)"
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
        dist, bars = R.step_distance(s, k, x, r, st["rz"]), R.step_bars(s, k)
        f64d = dict(bars)                          # 16 x the float64 run's distance, also where the bar is a derived one
        if k == 1:
            f64d["rz"] = 16.0 * R.rel(s["f64"]["rz"][1], s["ref"]["rz"][1])
        ratio = {q: 16.0 * dist[q] / f64d[q] if f64d[q] > 0 else (0.0 if dist[q] == 0 else np.inf) for q in dist}
        WORST[path] = max(WORST.get(path, 0.0), *ratio.values())
        print("cg-paths %s: k=%d distance / float64's  x %.2f  r %.2f  rz %.2f   (distances %.2e %.2e %.2e)"
              % (label, k, ratio["x"], ratio["r"], ratio["rz"], dist["x"], dist["r"], dist["rz"]))
        if st["iterations"] != k:
            bad.append("fixed_iters=%d ran %d iterations" % (k, st["iterations"]))
        for q in ("x", "r", "rz"):
            if not dist[q] <= bars[q]:
                bad.append("k=%d: %s off by %.3e, bar %.3e (%.1f x float64's distance)"
                           % (k, q, dist[q], bars[q], ratio[q]))
    # c. count
    st = runs["count"][0]
    print("cg-paths %s: count %d (reference %d, tolerance %.2e, relres %.2e)" % (label, st["iterations"], s["stop"], s["tol"], st["relres"]))
    if st["iterations"] != s["stop"] or st["converged"] != 1:
        bad.append("solve to %.3e: %d iterations (converged %d), the reference takes %d" % (s["tol"], st["iterations"], st["converged"], s["stop"]))
    return bad


def _single(km, torch, monkeypatch, path, variant, jacobi, sysname, nt=None):
    S = km.solvers
    s = R.system(sysname, PATHS[path]["values"], jacobi)
    _force(monkeypatch, PATHS[path]["env"], variant, nt)
    M = s["M"]
    n = M.shape[0]
    comm = S.KMC_comm(n, n, n, n)
    comm.connect()
    mat = S.Distributed_matrix(comm, n, [n], [0], M.indices, M.indptr, M.data)
    label = "%s/%s/%s/%s%s" % (sysname, path, variant, "jacobi" if jacobi else "plain", "/nt" if nt else "")
    try:
        bad = _path_errors(path, variant, mat.info(), mat.sum_plan(with_csr=False), sysname == "ragged", label)
        for k, v in (nt or {}).items():
            if comm.get_option(k) != (v, 1):
                bad.append("%s = %r" % (k, comm.get_option(k)))
        assert not bad, bad                      # (the wrong kernel: nothing below would be about this case)
        bad = _check(s, _runs(km, torch, mat, s), label, path)
    finally:
        mat.close()
        comm.close()
    assert not bad, "\n".join([label] + bad)


@pytest.mark.parametrize("jacobi", [True, False], ids=["jacobi", "plain"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("sysname", ["ragged", "tiny"])
def test_one_rank(km, torch, monkeypatch, sysname, path, variant, jacobi):
    """Six paths x two recurrences x {Jacobi, none}: ragged(6000) with its long row (several blocks per pass, the
    long-row partial) and tiny() (40 rows: most blocks of every pass contribute nothing)."""
    _single(km, torch, monkeypatch, path, variant, jacobi, sysname)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("path,knob", [("stream", "KMCF_SPMV_NT"), ("window", "KMCF_SPMV_NT"), ("sell", "KMCF_SELL_NT")])
@pytest.mark.parametrize("sysname", ["ragged", "tiny"])
def test_one_rank_nontemporal(km, torch, monkeypatch, sysname, path, knob, variant):
    """The nontemporal instances (matrices beyond the caches get them by themselves) on the same small systems."""
    _single(km, torch, monkeypatch, path, variant, True, sysname, nt={knob: "1"})


# the walk of check (d): (name, knobs of the replan or None, value set to set or None) -- from the largest interior grid
# (vec: a block per 16 rows) over stream chunks and window tiles to the row-per-lane tiles, and back
WALK = [("vec", dict(KIND=0), None), ("stream", dict(KIND=1), None), ("window", dict(KIND=2, SELLV=0), None),
        ("wcode", None, "v5"), ("sell", None, "v3"), ("sellv", dict(KIND=2, SELLV=1), "f64"), ("sell", None, "v3"),
        ("wcode", dict(KIND=2, SELL=0), None), ("window", dict(KIND=2, CODED=0, SELLV=0), None), ("stream", dict(KIND=1), None),
        ("vec", dict(KIND=0), None)]


@pytest.mark.parametrize("variant", VARIANTS)
def test_replan_walk_on_one_matrix(km, torch, monkeypatch, variant):
    """(d) ONE matrix object moved through the paths by kmcf_spmv_replan and set_values, a first step (a) and a count
    solve (c) after every move: partial counts of the wrong grid and partials left by a larger grid show here."""
    S = km.solvers
    values = "f64"
    s = R.system("ragged", values, True)
    _force(monkeypatch, WALK[0][1], variant)
    M = s["M"]
    n = M.shape[0]
    comm = S.KMC_comm(n, n, n, n)
    comm.connect()
    # (created with few distinct values: the plan's hint, without which no later replan cuts tiles for the coded kernels)
    mat = S.Distributed_matrix(comm, n, [n], [0], M.indices, M.indptr, R.system("ragged", "v3", True)["M"].data)
    mat.set_values(M.data)
    bad = []
    try:
        for step, (path, env, newvalues) in enumerate(WALK):
            if env is not None:
                _force(monkeypatch, env, variant)
                mat.replan()
            if newvalues is not None:
                values = newvalues
                s = R.system("ragged", values, True)
                mat.set_values(s["M"].data)
            label = "walk/%s/%d:%s(%s)" % (variant, step, path, values)
            wrong = _path_errors(path, variant, mat.info(), mat.sum_plan(with_csr=False), True, label)
            assert not wrong, wrong
            np.testing.assert_array_equal(mat.get_values(), s["M"].data)
            bad += [label + ": " + m for m in _check(s, _runs(km, torch, mat, s, steps=(1,)), label, path, steps=(1,))]
    finally:
        mat.close()
        comm.close()
    assert not bad, "\n".join(bad)


GROUPS = {"loopback-2": (2, None, [2500, 3500]), "loopback-3": (3, None, [1500, 2600, 1900]), "p2p-2": (2, "p2p", [3300, 2700])}


# every path and recurrence on every group (the peer-to-peer group's cg1r iteration: fused, the all-reduce inside the
# update kernel) -- and the other two transports of that iteration, each with a sequence rule of its own after the loop:
# the all-reduce in a 1-block kernel in front of the fused update, and the staged halo with a separate peer-to-peer
# reduction.  The chain of solves of _runs -- three ended by their limit, then one stopped -- is what those rules see.
P2P_KNOBS = {"": {}, "-arsplit": dict(KMCF_P2P_AR="split"), "-staged": dict(KMCF_P2P_DIRECT="0")}
RANK_CASES = [pytest.param(g, p, v, "", id="%s-%s-%s" % (g, p, v)) for g in GROUPS for p in PATHS for v in VARIANTS]
RANK_CASES += [pytest.param("p2p-2", "sell", "cg1r", k, id="p2p-2-sell-cg1r" + k) for k in ("-arsplit", "-staged")]


@pytest.mark.parametrize("group,path,variant,p2p_knobs", RANK_CASES)
def test_rank_group(km, torch, monkeypatch, group, path, variant, p2p_knobs):
    """The same system over P ranks of an in-process group, uneven partition: the interior kernels' instances that skip
    boundary rows, the boundary pass (vec kernel; on the peer-to-peer transport the halo kernel) and the long row on
    rank 0 each add their partials.  (a) - (c) on the gathered vectors; every rank returns the same scalars.  The
    peer-to-peer group takes the system without the long row: its direct halo protocol does not run with one.
    Its cg1r iteration runs once per transport: fused with the all-reduce inside the update kernel (the default),
    fused with KMCF_P2P_AR=split, and with the staged halo (KMCF_P2P_DIRECT=0) and a separate peer-to-peer reduction."""
    S = km.solvers
    P, transport, counts = GROUPS[group]
    sysname = "ragged" if transport is None else "ragged_nolong"
    s = R.system(sysname, PATHS[path]["values"], True)
    _force(monkeypatch, PATHS[path]["env"], variant)
    monkeypatch.setenv("KMCF_LOOPBACK_TIMEOUT_S", "30")
    for k in ("KMCF_P2P_AR", "KMCF_P2P_DIRECT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in P2P_KNOBS[p2p_knobs].items():
        monkeypatch.setenv(k, v)
    if transport:
        monkeypatch.setenv("KMCF_TRANSPORT", transport)
        monkeypatch.setenv("KMCF_P2P_TIMEOUT_MS", "20000")     # ranks are Python threads: their host-side set-up can be seconds apart
    else:
        monkeypatch.delenv("KMCF_TRANSPORT", raising=False)
    M = s["M"]
    n = M.shape[0]
    displs = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int32)
    assert sum(counts) == n and len(set(counts)) == P
    comms = S.KMC_comm.loopback_group(n, n, n, n, size=P, device=0)
    out, errs = [None] * P, []

    def work(r):
        try:
            torch.cuda.set_device(0)
            comm = comms[r]
            comm.connect()
            r0, nr = int(displs[r]), int(counts[r])
            sub = M[r0:r0 + nr]
            mat = S.Distributed_matrix(comm, n, counts, displs, sub.indices, sub.indptr, sub.data)
            res = dict(transport=comm.transport(), info=mat.info(), plan=mat.sum_plan(with_csr=False))
            res["knobs"] = {k: comm.get_option(k) for k in P2P_KNOBS[p2p_knobs]}
            res["runs"] = _runs(km, torch, mat, s, slice(r0, r0 + nr))
            mat.close()
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
    label = "%s/%s/%s%s" % (group, path, variant, p2p_knobs)
    bad = []
    for r, o in enumerate(out):
        assert o["transport"] == ("p2p (in-process group)" if transport else "loopback"), o["transport"]
        assert o["knobs"] == {k: (v, 1) for k, v in P2P_KNOBS[p2p_knobs].items()}, o["knobs"]
        bad += _path_errors(path, variant, o["info"], o["plan"], sysname == "ragged" and r == 0, "%s rank %d" % (label, r))
        if not (o["info"]["boundary_rows"] > 0 and o["info"]["halo_cols"] > 0 and o["plan"]["boundary_grid"] > 0):
            bad.append("rank %d: boundary_rows %d halo_cols %d" % (r, o["info"]["boundary_rows"], o["info"]["halo_cols"]))
    assert not bad, bad
    runs = {}
    for key in list(R.K_STEPS) + ["count"]:
        sts = [o["runs"][key][0] for o in out]
        for st in sts[1:]:
            if (st["iterations"], st["bb"], st["rz"]) != (sts[0]["iterations"], sts[0]["bb"], sts[0]["rz"]):
                bad.append("%s: ranks disagree: %r / %r" % (key, sts[0], st))
        runs[key] = (sts[0], np.concatenate([o["runs"][key][1] for o in out]), np.concatenate([o["runs"][key][2] for o in out]))
    bad += _check(s, runs, label, path)
    assert not bad, "\n".join([label] + bad)


def test_zz_report_measured_ratios():
    """Prints the worst ratio of check (b) per path over the cases that ran (DESIGN.md section 5 quotes them)."""
    for path in PATHS:
        if path in WORST:
            print("cg-paths worst ratio %s: %.2f" % (path, WORST[path]))
