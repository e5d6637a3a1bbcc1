#!/usr/bin/env python3
"""Full per-step loop of the reference's main (src/kmc_main.cpp:328-500) on the library: charge update,
boundary (K) solve, pairwise term, sum/gather, KMC events -- with the per-module wall times the reference
prints into output<size>_<rank>.txt ("Z - calculation time - ...").

    python tools/kmc_loop.py [--workload 5nm|5nm-periodic|40nm|conducting] [--steps 6] [--T 300] [--current] [--rate-mode bg|ekin|site]
                             [--clusters] [--current-map] [--current-profile N] [--scheme all|half|third --select W,B] [--gap R]
                             [--chain R [--chain-hops K]] [--field-map] [--event-census] [--pair-correlation R [--pair-bins N]]

--current adds the electro-thermal stages after the potential and before the events: conduction-band edge, current
solve with heating (site_power), local heat solve (site_temperature); --rate-mode ekin | site lets the event rates read
that field (kmcf_execute_kmc_step_thermal).  Workload `conducting`: the 4 x 4 crossbar with a vacancy filament of
tests/test_gpu_conducting.py, whose current is a property of the device.  Workload `5nm-periodic`: the 5 nm example as the
periodic cell it is (structure.periodic_5nm, pbc = 1 in y and z): neighbour list, K pattern, the spatial index of the pairwise
term and the pair distance of the event rates all take the minimum image, and with --current so does the T state of the
current solve (kmcf_initialize_sparsity_T_pbc: neighbour bonds and the ground flag through the faces, the tunnel block's
pair rule and WKB distance, the current map); the step line is the one of `5nm`.  --clusters runs the conductive cluster analysis
(kmcf_conductive_clusters) after the charge update of every step: whether a filament bridges the electrodes, without a
current solve; the step line gains `clusters <ms> (<vacancy clusters> vac, largest <sites>, bridging <filaments>)`, the
time in milliseconds of device time.  --current-map (with --current) runs the site-resolved current map (kmcf_current_map)
after the power update of every step: the step line gains `current map <ms> (tunnel share <sum_tunnel / sum_through>, max
<max_through> at site <max_site>)`, the time again in milliseconds of device time.  --current-profile N (with --current) runs
the current profile (kmcf_current_profile) next to it: N planes equally spaced strictly between the x of the left and the
right contact blocks, cells from structure.crossbar_lines on the crossbar workloads (one cell otherwise).  Below the step line
it prints, per cell and for the rest, the current through the middle plane, its tunnel share and the range of planes whose
tunnel share exceeds one half, then `flux <flux_min> .. <flux_max> against I_macro <I_macro>` and the two device times.  --scheme all | half | third with --select W,B
(the synthetic crossbars only) drives the array per line instead of with one scalar Vd: the contact slots of the potential
array are filled once by structure.bias_scheme (selected word line -Vd/2, selected bit line +Vd/2, the others by the scheme),
the boundary solve is kmcf_background_potential_sparse_contacts, and the step line gains `events per cell [c0 c1 ...]`: the
events of the step whose first site lies under crossing word * n_lines + bit.  The band-edge and current stages of --current
still see the scalar Vd.  --gap R runs the filament gap analysis (kmcf_filament_gap; on `5nm-periodic`
kmcf_filament_gap_pbc: periodic clusters, minimum-image distance) after the charge update of every step:
how close the conductive matter attached to the left electrode comes to the matter attached to the right one, searched up
to R angstrom (at most 20, the cell edge of the spatial index), per cell of structure.crossbar_lines on the crossbar
workloads.  The step line gains `gap <ms clusters>+<ms search> [<cell>: <gap> A (<site_left>-<site_right>) L <n_left> R
<n_right> | <cell>: bridged (<n_both> sites) L .. R .. | <cell>: none L .. R ..]`; with --clusters a bridged cell also shows
`constriction <sites>`: the smallest number of filament vacancies in a slice of 3.2 angstrom along x.  --chain R runs the
tunnelling-chain analysis (kmcf_filament_chain; on `5nm-periodic` kmcf_filament_chain_pbc: periodic clusters, minimum-image
hops) next to it: per cell the chain of hops from the left side to the right
side through the floating conductive clusters whose longest hop is as short as any chain's, hops of at most R angstrom
(at most 20).  The step line gains `chain <ms clusters>+<ms search>
(<rounds> rounds, <surface sites> surface) [<cell>: <hops> hops, longest <hop_max> A (<from>-<to>), length <length> A,
direct <sqrt(direct2)> A, <stones> stones | <cell>: bridged | <cell>: open, .. stones | <cell>: none]`; --chain-hops K also
lists the first K hops of every chain as `<from>-<to> <hop> A`.  --field-map runs the site gradient map
(kmcf_site_gradient through solvers.field_map) on the potential the events read, after the sum / gather of every step: below
the step line it prints, per cell of structure.crossbar_lines on the crossbar workloads (one cell otherwise), `field <cell>:
|E| max <V/A> at site <site> = <ratio> x mean | drop <V/A> (<from>-<to>) | <full>/<sites> full` -- the mean field is
|Vd| / (x extent of the interface) -- and the device time; with --current the same for the site temperature of the heat
solve (`grad T`, K/A, no ratio).  On `5nm-periodic` the displacement is the minimum image.  --event-census runs the event
rate census (kmcf_event_census) before the event step of every superstep, in the step's rate mode: the forecast of the step
from the rates of every possible event, nothing executed.  Cells from structure.crossbar_lines on the crossbar workloads (one
cell otherwise).  Below the step line it prints, per cell and for the rest, `census cell <c>: rate <sum> (<share of the
total>) | gen <..> rec <..> vdiff <..> odiff <..> | max <rate> (<i>-<j>, <type>)` -- with --scheme also `| realised <share of
the step's events that fell into the cell>` next to the forecast share -- then `census device: rate_total <..> dt_mean <..> |
rows_live <..> n_zero <..> | build <ms> census <ms>`, the two device times.  --pair-correlation R [--pair-bins N] runs the
defect pair correlation (kmcf_defect_correlation; the distance is the spatial index's own, the minimum image on `5nm-periodic`)
after the event step of every superstep, up to R angstrom (at most 20) in N bins (default 20), every other site a probe of the
counts.  Cells from structure.crossbar_lines on the crossbar workloads (one cell otherwise).  Below the step line it prints,
per cell and for the rest, `pairs cell <c>: V0 <n> V+ <n> ion <n> | V-V first <lo>-<hi> A peak <lo>-<hi> A (<pairs>) | V-ion
first .. peak ..` -- V-V: the three vacancy-vacancy class pairs added, V-ion: the two vacancy-ion ones; first: the first
non-empty bin, peak: the fullest one (the first among equals) -- then `pairs device: <pairs> pairs, <members> defects,
<probes> probes | densest site <site> (<count> defects within R) | <ms> ms`.  --field-grid H [--field-grid-radius R] samples,
after the last step, site fields on a grid of spacing H angstrom (kmcf_field_grid through solvers.field_grid; radius R, at
most and by default 20) over the bounding box of every cell of structure.crossbar_lines on the crossbar workloads (one cell
otherwise): the potential the events read as a weighted mean, the neutral vacancies as a number density
(solvers.sample_density) and the element of the nearest site.  Per cell it prints `field grid cell <c>: <nx> x <ny> x <nz>
voxels of H A, radius R A | <visits> visits, <empty> empty | potential <min> .. <max> V | densest voxel (<i>, <j>, <k>)
<density> V0/A^3 (<n> neutral vacancies within reach) | <ms> ms + <ms> ms`; nothing is written unless --field-grid-out
FILE.npz names a file (potential, vacancy_density, element, count, origin, spacing; `_cell<c>` appended with several cells).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import kmcfield_amd as km  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="5nm", choices=["5nm", "5nm-periodic", "40nm", "conducting"])
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--T", type=float, default=300.0)
    ap.add_argument("--max-events", type=int, default=100000)
    ap.add_argument("--event-stats", action="store_true", help="locality of the selected rows (supertiles of 128 rows)")
    ap.add_argument("--current", action="store_true", help="CB edge, current solve with heating and local heat solve in every step")
    ap.add_argument("--rate-mode", default="bg", choices=["bg", "ekin", "site"],
                    help="event rates: T_bg only | the reference's Ekin term | Boltzmann factor at the site's temperature")
    ap.add_argument("--clusters", action="store_true",
                    help="conductive cluster analysis after every charge update: vacancy clusters, the largest, bridging filaments")
    ap.add_argument("--current-map", action="store_true",
                    help="site-resolved current map after every power update (needs --current): tunnel share, the busiest site")
    ap.add_argument("--current-profile", type=int, default=0, metavar="N",
                    help="current through N x-planes between the contacts per crossbar cell and pair kind (needs --current)")
    ap.add_argument("--scheme", default=None, choices=["all", "half", "third"],
                    help="per-line bias of the crossbar (synthetic workloads): all cells selected | V/2 scheme | V/3 scheme")
    ap.add_argument("--select", default="0,0", help="W,B: the selected word line and bit line of --scheme")
    ap.add_argument("--gap", type=float, default=None, metavar="R",
                    help="filament gap analysis after every charge update, searched up to R angstrom (<= 20): gap, pair and "
                         "counts per crossbar cell; with --clusters also the constriction of a bridging filament")
    ap.add_argument("--chain", type=float, default=None, metavar="R",
                    help="tunnelling-chain analysis after every charge update, hops of at most R angstrom (<= 20): the "
                         "stepping-stone chain between the electrode sides per crossbar cell, its longest hop and length")
    ap.add_argument("--chain-hops", type=int, default=0, metavar="K", help="with --chain: list the first K hops of every chain")
    ap.add_argument("--event-census", action="store_true",
                    help="event rate census before every event step: rate per crossbar cell and event type, the fastest event, "
                         "the mean residence time; with --scheme the realised share of the step's events next to the forecast")
    ap.add_argument("--field-map", action="store_true",
                    help="site gradient map of the potential after every sum / gather: largest |E| and bond drop per crossbar "
                         "cell, against the mean field; with --current also of the site temperature")
    ap.add_argument("--pair-correlation", type=float, default=None, metavar="R",
                    help="defect pair correlation after every step, up to R angstrom (<= 20): defect counts per crossbar cell, "
                         "first and fullest bin of the vacancy-vacancy and vacancy-ion distances, the densest site")
    ap.add_argument("--pair-bins", type=int, default=20, metavar="N", help="with --pair-correlation: bins of the histograms (<= 256)")
    ap.add_argument("--field-grid", type=float, default=None, metavar="H",
                    help="after the last step: the potential the events read, the neutral-vacancy density and the element of "
                         "the nearest site on a grid of spacing H angstrom over every crossbar cell's box")
    ap.add_argument("--field-grid-radius", type=float, default=None, metavar="R",
                    help="with --field-grid: the sampling radius in angstrom (at most and by default the cell edge of the spatial index)")
    ap.add_argument("--field-grid-out", default=None, metavar="FILE.npz",
                    help="with --field-grid: write the grids (potential, vacancy_density, element, count, origin, spacing per cell)")
    a = ap.parse_args()
    periodic = a.workload == "5nm-periodic"
    if a.field_grid is not None and not (np.isfinite(a.field_grid) and a.field_grid > 0.0):
        ap.error("--field-grid %g: the spacing is > 0" % a.field_grid)
    if a.field_grid_radius is not None and (a.field_grid is None or not a.field_grid_radius > 0.0):
        ap.error("--field-grid-radius R: R > 0, with --field-grid")
    if a.field_grid_out is not None and a.field_grid is None:
        ap.error("--field-grid-out needs --field-grid")
    if a.scheme and a.workload in ("5nm", "5nm-periodic"):
        ap.error("--scheme needs a crossbar with lines: --workload 40nm or conducting")
    if a.current_map and not a.current:
        ap.error("--current-map needs --current (the map reads the potentials of the current solve)")
    if a.current_profile and not a.current:
        ap.error("--current-profile needs --current (the profile reads the potentials of the current solve)")
    if not 0 <= a.current_profile <= 1024:
        ap.error("--current-profile N: 1 ... 1024 planes")
    if a.gap is not None and not 0.0 < a.gap <= 20.0:
        ap.error("--gap %g: the search radius is > 0 and at most 20 (the cell edge of the spatial index)" % a.gap)
    if a.chain is not None and not 0.0 < a.chain <= 20.0:
        ap.error("--chain %g: the hop length is > 0 and at most 20 (the cell edge of the spatial index)" % a.chain)
    if a.pair_correlation is not None and not 0.0 < a.pair_correlation <= 20.0:
        ap.error("--pair-correlation %g: the radius is > 0 and at most 20 (the cell edge of the spatial index)" % a.pair_correlation)
    if not 1 <= a.pair_bins <= 256:
        ap.error("--pair-bins N: 1 ... 256 bins")
    if a.chain_hops < 0 or (a.chain_hops and a.chain is None):
        ap.error("--chain-hops K: K >= 0, with --chain")
    if a.rate_mode != "bg" and not a.current:
        ap.error("--rate-mode %s needs --current (the heat solve provides the site temperatures)" % a.rate_mode)
    S = km.solvers
    if a.workload == "5nm":
        d = km.structure.load_device_5nm("init")
    elif periodic:
        d = km.structure.periodic_5nm("init")
    elif a.workload == "conducting":
        d = km.structure.synth_crossbar_40nm(tiles=4, filament=4.0)
    else:
        d = km.structure.synth_crossbar_40nm()
    N, NL = d["N"], d["N_contact"]
    t0 = time.perf_counter()
    comm = S.KMC_comm(N - 2 * NL, N + 1, N, N)
    comm.connect()
    buf = S.GPUBuffers(N, d["element"], d["xyz"][:, 0], d["xyz"][:, 1], d["xyz"][:, 2], 52, d["sigma"], d["k"],
                       d["lattice"], d["metals"])
    pbc = 1 if periodic else 0                # (the other workloads keep the reference GPU path's open list and pairwise term)
    S.compute_neighbor_list(comm, buf, d["nn_dist"], 52, pbc=pbc)
    S.compute_cutoff_list(comm, buf, 20.0, pbc=pbc)
    if a.field_grid_radius is not None and a.field_grid_radius > buf.cutoff_radius:
        ap.error("--field-grid-radius %g: at most %g, the cell edge of the spatial index" % (a.field_grid_radius, buf.cutoff_radius))
    S.events_set_lattice(comm, d["lattice"], pbc)
    S.initialize_sparsity_K(buf, d["pbc"], d["nn_dist"], NL, comm)
    layers = km.structure.LAYERS
    xs = d["xyz"][:, 0]
    if a.workload not in ("5nm", "5nm-periodic"):      # the synthetic crossbar shares the 5 nm stack along x
        xs = np.clip(xs, layers[0]["start_x"], layers[-1]["end_x"])
    lay = torch.as_tensor(S.site_layers(xs, layers), device="cuda")
    rng = S.RandomNumberGenerator(km.structure.RND_SEED_KMC)
    if a.current:
        # the atoms of the current solve are invariant under KMC events: one pattern per run (src/kmc_main.cpp:273)
        N_atom = int(((d["element"] != 0) & (d["element"] != 1)).sum())
        comm.counts_T, comm.displs_T = comm.partition(N_atom + 1, comm.size_T)
        S.initialize_sparsity_T(buf, d["pbc"], d["nn_dist"], NL, NL, 10, comm, periodic=periodic)
        q_e = 1.60217663e-19
        high_G_T, loop_G, G0 = 1e5 * d["high_G"], 1e7 * d["high_G"], 2 * 3.8612e-5 * 1e-5
        side = float(d["lattice"][1]) * 1e-10
        heat = S.heat_params(background_temp=a.T, A=side * side, cg_tolerance=1e-12, cg_max_iterations=50000)
    cell_of_site = None
    if a.scheme:
        try:
            select = tuple(int(t) for t in a.select.split(","))
            assert len(select) == 2
            contacts = km.structure.bias_scheme(d, a.scheme, select=select)
        except (AssertionError, ValueError) as e:
            ap.error("--select %s: %s" % (a.select, str(e) or "W,B expected"))
        cell_of_site = km.structure.crossbar_lines(d)[2]
        buf.site_potential_boundary.copy_(torch.as_tensor(contacts))      # once: the solve reads the slots, never writes them
    prof_cells, n_prof_cells, prof_planes = None, 1, None
    if a.current_profile:
        x_l, x_r = float(d["xyz"][:NL, 0].max()), float(d["xyz"][N - NL:, 0].min())       # the facing ends of the contact blocks
        prof_planes = x_l + (x_r - x_l) * np.arange(1, a.current_profile + 1) / (a.current_profile + 1)
        if a.workload not in ("5nm", "5nm-periodic"):
            cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
            prof_cells, n_prof_cells = torch.as_tensor(np.ascontiguousarray(cells, np.int32), device="cuda"), int(cells.max()) + 1
    gap_cells, n_gap_cells, gap_bins = None, 1, None
    if a.gap is not None or a.chain is not None:
        if a.workload not in ("5nm", "5nm-periodic"):
            cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
            gap_cells, n_gap_cells = torch.as_tensor(cells, device="cuda"), int(cells.max()) + 1
        if a.clusters and a.gap is not None:
            x_lo, x_hi = float(d["xyz"][:, 0].min()), float(d["xyz"][:, 0].max()) + 1e-6
            gap_bins = (int(np.ceil((x_hi - x_lo) / 3.2)), x_lo, x_hi)
    field_cells, n_field_cells, mean_field = None, 1, 0.0
    if a.field_map:
        if a.workload not in ("5nm", "5nm-periodic"):
            cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
            field_cells, n_field_cells = torch.as_tensor(np.ascontiguousarray(cells, np.int32), device="cuda"), int(cells.max()) + 1
        x_if = d["xyz"][NL:N - NL, 0]
        mean_field = abs(d["Vd"]) / float(x_if.max() - x_if.min())

    census_cells, n_census_cells = None, 1
    if a.event_census and a.workload not in ("5nm", "5nm-periodic"):
        cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
        census_cells, n_census_cells = torch.as_tensor(np.ascontiguousarray(cells, np.int32), device="cuda"), int(cells.max()) + 1

    pair_cells, n_pair_cells = None, 1
    if a.pair_correlation is not None and a.workload not in ("5nm", "5nm-periodic"):
        cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
        pair_cells, n_pair_cells = torch.as_tensor(np.ascontiguousarray(cells, np.int32), device="cuda"), int(cells.max()) + 1

    def pair_lines():
        """the per-cell lines of one defect pair correlation"""
        pc = S.defect_correlation(comm, buf, a.pair_correlation, a.pair_bins, site_cell=pair_cells, n_cells=n_pair_cells,
                                  probe_all=True)
        e, h, m, st_p = pc["edges"], pc["hist"], pc["members"], pc["stats"]
        ix = lambda p, q: S.pair_class_index(p, q, 3)

        def summary(row):
            nz = np.flatnonzero(row)
            if not len(nz):
                return "none"
            k = int(np.argmax(row))
            return "first %.2f-%.2f A peak %.2f-%.2f A (%d)" % (e[nz[0]], e[nz[0] + 1], e[k], e[k + 1], int(row[k]))
        out = []
        for c in range(n_pair_cells + 1):
            vv = h[c, ix(0, 0)] + h[c, ix(0, 1)] + h[c, ix(1, 1)]
            vi = h[c, ix(0, 2)] + h[c, ix(1, 2)]
            out.append("  pairs %s: V0 %d V+ %d ion %d | V-V %s | V-ion %s" % (
                "rest" if c == n_pair_cells else "cell %d" % c, m[c, 0], m[c, 1], m[c, 2], summary(vv), summary(vi)))
        out.append("  pairs device: %d pairs, %d defects, %d probes | densest site %d (%d defects within %g A) | %.3f ms" % (
            st_p["n_pairs_total"], st_p["n_members"], st_p["n_probes"], st_p["max_count_site"], st_p["max_count"], a.pair_correlation,
            st_p["ms"]))
        return out

    def census_lines(cs, log):
        """the per-cell lines of one census; log: the step's (i, j, type) rows, for the realised shares of --scheme"""
        t, st_c = cs["table"], cs["stats"]
        realised = None
        if a.scheme and len(log):
            cells = cell_of_site[log[:, 0]]
            cells = np.where((cells < 0) | (cells >= n_census_cells), n_census_cells, cells)
            realised = np.bincount(cells, minlength=n_census_cells + 1) / len(log)
        out = []
        for c in range(n_census_cells + 1):
            by_type = [sum(float(t[c, l, ty]["rate_sum"]) for l in range(t.shape[1])) for ty in range(4)]
            rate = ((by_type[0] + by_type[1]) + by_type[2]) + by_type[3]
            top, ty_top = t[c, 0, 0], 0
            for l in range(t.shape[1]):
                for ty in range(4):
                    b = t[c, l, ty]
                    if b["max_i"] >= 0 and (top["max_i"] < 0 or b["rate_max"] > top["rate_max"]):
                        top, ty_top = b, ty
            out.append("  census %s: rate %.5e (%.4f) | gen %.4e rec %.4e vdiff %.4e odiff %.4e | max %.5e (%d-%d, %s)%s" % (
                "rest" if c == n_census_cells else "cell %d" % c, rate, rate / st_c["rate_total"] if st_c["rate_total"] > 0 else 0.0,
                *by_type, top["rate_max"], top["max_i"], top["max_j"], S.EVENT_NAMES[ty_top] if top["max_i"] >= 0 else "none",
                "" if realised is None else " | realised %.4f" % realised[c]))
        out.append("  census device: rate_total %.6e dt_mean %.5e | rows_live %d n_zero %d | build %.3f ms census %.3f ms" % (
            st_c["rate_total"], st_c["dt_mean"], st_c["rows_live"], st_c["n_zero"], st_c["ms_build"], st_c["ms_census"]))
        return out

    def gradient_lines(what, unit, value, scale):
        """the per-cell lines of one site field"""
        fn = S.field_map if scale > 0 else S.site_gradient              # (|E| = |g|: the tables are the same)
        gm = fn(comm, buf, value, site_cell=field_cells, n_cells=n_field_cells, periodic=periodic)
        out = []
        for c, r in enumerate(gm["cells"]):
            ratio = " = %.2f x mean" % (r["g_max"] / scale) if scale > 0 else ""
            out.append("  %s cell %d: max %.5e %s at site %d%s | drop %.5e %s (%d-%d) | %d/%d full" % (
                what, c, r["g_max"], unit, r["g_site"], ratio, r["drop_max"], unit, r["drop_from"], r["drop_to"], r["n_full"],
                r["n_sites"]))
        st_g = gm["stats"]
        out.append("  %s device: max %.5e %s at site %d | %d pairs, %d degenerate sites | %.3f ms" % (
            what, st_g["g_max"], unit, st_g["g_site"], st_g["pairs"], st_g["n_degenerate"], st_g["ms"]))
        return out

    comm.sync()
    print("init [s] %.3f  (sites %d)" % (time.perf_counter() - t0, N))
    kmc_time = 0.0
    freq = 10e13
    for step in range(a.steps):
        def timed(f):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = f()
            comm.sync()
            torch.cuda.synchronize()
            return time.perf_counter() - t, r
        tc, _ = timed(lambda: S.update_charge_gpu(buf.site_element, buf.site_charge, buf.neigh_idx, buf.N_, buf.nn_,
                                                  buf.metal_types, buf.num_metal_types_, comm.counts_events,
                                                  comm.displs_events, comm))
        clusters = ""
        if a.clusters:
            cs = S.conductive_clusters(comm, buf, NL, NL, labels=False)["stats"]
            clusters = " | clusters %.3f (%d vac, largest %d, bridging %d)" % (cs["ms"], cs["n_vacancy_clusters"],
                                                                                  cs["largest_vacancy"], cs["n_bridging"])
        if a.gap is not None:
            gp = S.filament_gap(comm, buf, NL, NL, a.gap, site_cell=gap_cells, n_cells=n_gap_cells, bins=gap_bins, sides=False,
                                periodic=periodic)
            cells = []
            for c, g in enumerate(gp["gaps"]):
                if g["bridged"]:
                    what = "bridged (%d sites)" % g["n_both"]
                    if gap_bins is not None:
                        s3 = gp["profile"][c][:, 2]
                        nz = np.flatnonzero(s3)
                        what += " constriction %d" % (s3[nz[0]:nz[-1] + 1].min() if len(nz) else 0)
                elif g["site_left"] >= 0:
                    what = "%.4f A (%d-%d)" % (g["gap"], g["site_left"], g["site_right"])
                else:
                    what = "none"
                cells.append("%d: %s L %d R %d" % (c, what, g["n_left"], g["n_right"]))
            clusters += " | gap %.3f+%.3f [%s]" % (gp["stats"]["ms_clusters"], gp["stats"]["ms_search"], " | ".join(cells))
        if a.chain is not None:
            ch = S.filament_chain(comm, buf, NL, NL, a.chain, site_cell=gap_cells, n_cells=n_gap_cells, max_hops=a.chain_hops,
                                  sides=False, nodes=False, periodic=periodic)
            cells = []
            for c, r in enumerate(ch["chains"]):
                if r["status"] == S.CHAIN_BRIDGED:
                    what = "bridged"
                elif r["status"] == S.CHAIN_CHAINED:
                    what = "%d hops, longest %.4f A (%d-%d), length %.4f A, direct %.4f A, %d stones" % (
                        r["n_hops"], r["hop_max"], r["neck_from"], r["neck_to"], r["length"], np.sqrt(r["direct2"]), r["n_stones"])
                    for h in ch["hops"][c][:min(r["n_hops"], a.chain_hops)] if a.chain_hops else ():
                        what += ", %d-%d %.4f A" % (h["from"], h["to"], np.sqrt(h["d2"]))
                elif r["status"] == S.CHAIN_OPEN:
                    what = "open, %d stones" % r["n_stones"]
                else:
                    what = "none"
                cells.append("%d: %s" % (c, what))
            st_c = ch["stats"]
            clusters += " | chain %.3f+%.3f (%d rounds, %d surface) [%s]" % (st_c["ms_clusters"], st_c["ms_search"], st_c["rounds"],
                                                                            st_c["surface_sites"], " | ".join(cells))
        if a.scheme:
            tb, st = timed(lambda: S.background_potential_gpu_sparse_contacts(buf, N, NL, NL, d["high_G"], d["low_G"],
                                                                              len(d["metals"])))
        else:
            tb, st = timed(lambda: S.background_potential_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"],
                                                                     d["low_G"], d["nn_dist"], len(d["metals"]), step))
        tp, _ = timed(lambda: S.poisson_gridless_gpu(buf, comm))
        tg, _ = timed(lambda: S.sum_and_gather_potential(buf, NL, comm))
        # (site_potential_charge now holds boundary + charge: the potential the events read; |g| of it is |E|)
        field_lines = gradient_lines("field |E|", "V/A", buf.site_potential_charge, mean_field) if a.field_map else []
        thermal = {}
        if a.current:
            tcb, st_cb = timed(lambda: S.update_CB_edge_gpu_sparse(buf, N, NL, NL, d["Vd"], d["pbc"], d["high_G"], d["low_G"],
                                                                   d["nn_dist"], len(d["metals"])))
            tpw, (imacro, st_t) = timed(lambda: S.update_power_gpu_sparse_dist(
                buf, NL, NL, 10, d["Vd"], high_G_T, d["low_G"], loop_G, G0, q_e * 0.01, d["nn_dist"], 0.85 * 9.11e-31, 1.6,
                len(d["metals"]), True, False, 1.0, cg_tolerance=1e-15 * N_atom, cg_max_iterations=40000))
            if a.current_map:
                cm = S.current_map(buf, tunnel=False, net=False)["stats"]
                clusters += " | current map %.3f (tunnel share %.4f, max %.4e at site %d)" % (
                    cm["ms"], cm["sum_tunnel"] / cm["sum_through"] if cm["sum_through"] > 0 else 0.0, cm["max_through"], cm["max_site"])
            profile_lines = []
            if a.current_profile:
                cp = S.current_profile(buf, prof_planes, site_cell=prof_cells, n_cells=n_prof_cells)
                F, mid = cp["profile"], a.current_profile // 2
                for c in range(n_prof_cells + 1):
                    tot = F[c].sum(1)
                    share = np.divide(F[c][:, 1], tot, out=np.zeros_like(tot), where=tot != 0)
                    tun = np.flatnonzero(share > 0.5)
                    profile_lines.append("  %-7s I(plane %d) %+.4e  tunnel share %.4f  tunnels at planes %s" % (
                        "rest" if c == n_prof_cells else "cell %d" % c, mid, tot[mid], share[mid],
                        "%d..%d (x %.2f..%.2f A, %d planes)" % (tun[0], tun[-1], prof_planes[tun[0]], prof_planes[tun[-1]], len(tun)) if len(tun) else "none"))
                ps = cp["stats"]
                profile_lines.append("  flux %.6e (plane %d) .. %.6e (plane %d) against I_macro %.6e | pairs %.3f ms, planes %.3f ms" % (
                    ps["flux_min"], ps["plane_min"], ps["flux_max"], ps["plane_max"], imacro, ps["ms_pairs"], ps["ms_planes"]))
            th, ht = timed(lambda: S.update_temperature_local_gpu(buf, N, NL, NL, 1e-6, heat))      # steady state
            if a.field_map:
                field_lines += gradient_lines("grad T", "K/A", buf.site_temperature, 0.0)
            if a.rate_mode != "bg":
                thermal = dict(site_temperature=buf.site_temperature, rate_mode=a.rate_mode)
        census = None
        if a.event_census:
            census = S.event_census(comm, N, comm.counts_events, comm.displs_events, 52, buf.neigh_idx, lay, a.T, freq, d["sigma"],
                                    d["k"], buf.site_x, buf.site_y, buf.site_z, buf.site_potential_charge, buf.site_element,
                                    buf.site_charge, layers, site_cell=census_cells, n_cells=n_census_cells, **thermal)
        te, ev = timed(lambda: S.execute_kmc_step_mpi(comm, N, comm.counts_events, comm.displs_events, 52, buf.neigh_idx,
                                                      lay, a.T, freq, d["sigma"], d["k"], buf.site_x, buf.site_y,
                                                      buf.site_z, buf.site_potential_charge, buf.site_element,
                                                      buf.site_charge, rng, layers, max_events=a.max_events,
                                                      return_log=True, **thermal))
        kmc_time += ev[0]
        if a.scheme:
            cells = cell_of_site[ev[2][:, 0]]
            clusters += " | events per cell [%s]" % " ".join(str(c) for c in np.bincount(cells[cells >= 0], minlength=cell_of_site.max() + 1))
        if a.event_stats and ev[1] > 0:
            # where the selection walk lands: how often a recently used supertile (128 consecutive rows of the event list)
            # is selected again -- what a small cache of row sums in LDS would hit
            import collections
            st_ = ev[2][:, 0] // 128
            line = "  events: %d, distinct supertiles %d" % (len(st_), len(set(st_.tolist())))
            for cap in (16, 64, 256):
                lru, hits = collections.OrderedDict(), 0
                for q in st_.tolist():
                    if q in lru:
                        hits += 1
                        lru.move_to_end(q)
                    else:
                        lru[q] = 1
                        if len(lru) > cap:
                            lru.popitem(last=False)
                line += ", LRU-%d hit rate %.2f" % (cap, hits / len(st_))
            print(line, flush=True)
        if census is not None:
            field_lines = field_lines + census_lines(census, ev[2])
        if a.pair_correlation is not None:
            field_lines = field_lines + pair_lines()
        if a.current:
            print("step %d: charge %.6f | boundary %.6f (%d it) | pairwise %.6f | gather %.6f | CB edge %.6f (%d it) | "
                  "power %.6f (%d it, I_macro %.4e) | heat %.6f (%d it, max T %.2f K) | events[%s] %.6f (%d ev) | "
                  "superstep %.6f | KMC time %.5e%s" % (step + 1, tc, tb, st["iterations"], tp, tg, tcb, st_cb["iterations"], tpw,
                                                         st_t["iterations"], imacro, th, ht["stats"]["iterations"],
                                                         float(buf.site_temperature.max()), a.rate_mode, te, ev[1],
                                                         tc + tb + tp + tg + tcb + tpw + th + te, kmc_time, clusters), flush=True)
            for line in profile_lines + field_lines:
                print(line, flush=True)
            continue
        print("step %d: charge %.6f | boundary %.6f (%d it) | pairwise %.6f | gather %.6f | events %.6f (%d ev) | "
              "superstep %.6f | KMC time %.5e%s" % (step + 1, tc, tb, st["iterations"], tp, tg, te, ev[1],
                                                     tc + tb + tp + tg + te, kmc_time, clusters), flush=True)
        for line in field_lines:
            print(line, flush=True)
    if a.field_grid is not None:
        # (site_potential_charge: boundary + charge as of the last step's sum / gather -- the potential its events read)
        h, radius = a.field_grid, buf.cutoff_radius if a.field_grid_radius is None else a.field_grid_radius
        if a.workload in ("5nm", "5nm-periodic"):
            cells = np.zeros(N, np.int32)
        else:
            cells = km.structure.crossbar_lines(d)[2] if cell_of_site is None else cell_of_site
        neutral = ((buf.site_element == km.structure.VACANCY) & (buf.site_charge == 0)).to(torch.int32)
        ones = torch.ones(1, N, dtype=torch.float64, device="cuda")
        saved = {}
        for c in range(int(cells.max()) + 1):
            box = d["xyz"][cells == c]
            lo, hi = box.min(0), box.max(0)
            dims = np.floor((hi - lo) / h).astype(np.int64) + 1
            pot = S.field_grid(buf, lo, h, dims, buf.site_potential_charge, radius=radius, labels=buf.site_element)
            vac = S.field_grid(buf, lo, h, dims, ones, mask=neutral, radius=radius, normalize=False)
            dens = S.sample_density(vac)[0]
            v = pot["out"][0]
            seen = ~torch.isnan(v)
            k = int(torch.argmax(dens))
            ijk = np.unravel_index(k, tuple(int(n) for n in dims))
            st_f = pot["stats"]
            print("  field grid cell %d: %d x %d x %d voxels of %g A, radius %g A | %d visits, %d empty | potential %s V | "
                  "densest voxel (%d, %d, %d) %.4e V0/A^3 (%d neutral vacancies within reach) | %.3f ms + %.3f ms" % (
                      c, dims[0], dims[1], dims[2], h, radius, st_f["n_visits"], st_f["n_empty"],
                      "%.6f .. %.6f" % (float(v[seen].min()), float(v[seen].max())) if bool(seen.any()) else "none",
                      ijk[0], ijk[1], ijk[2], float(dens.reshape(-1)[k]), int(vac["count"].reshape(-1)[k]), st_f["ms"],
                      vac["stats"]["ms"]), flush=True)
            if a.field_grid_out is not None:
                tag = "" if int(cells.max()) == 0 else "_cell%d" % c
                saved.update({"potential" + tag: v.cpu().numpy(), "vacancy_density" + tag: dens.cpu().numpy(),
                              "element" + tag: pot["labels"].cpu().numpy(), "count" + tag: pot["count"].cpu().numpy(),
                              "origin" + tag: lo, "spacing" + tag: np.float64(h)})
        if a.field_grid_out is not None:
            np.savez(a.field_grid_out, **saved)
    buf.freeGPUmemory()
    comm.close()


if __name__ == "__main__":
    main()
