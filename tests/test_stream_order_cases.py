"""CPU: the inputs of the stream ordering tests (tests/stream_order_cases.py) meet the conditions their docstring states.

A decoy is what a library that failed to wait for the caller's stream would read.  It has to be harmless -- indices in
range, elements of the enum, charges of the charge rule, coordinates inside the true bounding box, finite numbers -- and
it has to differ from the true array in at least 10 % of its entries.  Sizes are host arguments and belong to neither
set.  That the ANSWER differs between the two sets is asserted on the GPU, on the two synchronised reference runs."""
import numpy as np
import pytest

import stream_order_cases as SO


@pytest.mark.parametrize("name", SO.CASES + ("group",))
def test_decoys_are_safe_and_different(name):
    c = SO.group() if name == "group" else SO.case(name)
    assert c["arrays"], "a case stages at least one array"
    for key, s in c["arrays"].items():
        assert s.true.shape == s.decoy.shape and s.true.dtype == s.decoy.dtype, key
        assert not s.true.flags.writeable and not s.decoy.flags.writeable, key
        share = float(np.mean(s.true != s.decoy))
        print("%s %s (%s): %d entries, %.0f %% differ" % (name, key, s.kind, s.true.size, 100 * share))
        assert SO.violations(s) == [], (name, key)
        # the true array meets the decoy's rule as well (but for the share that differs)
        own = SO.violations(SO.Staged(s.kind, s.decoy, s.true, **s.rule))
        assert [v for v in own if "differ" not in v] == [], (name, key, own)


def test_the_rules_reject_what_they_are_there_for():
    """violations() is the check: hold it to one broken decoy per rule"""
    n = 50
    f = np.linspace(1.0, 2.0, n)
    xyz = np.stack([f, f[::-1], f * 2], axis=1)
    far = xyz[::-1].copy()
    far[0, 2] = 99.0
    nan = f[::-1].copy()
    nan[3] = np.nan
    neg = f[::-1].copy()
    neg[3] = -1.0
    i = np.arange(n, dtype=np.int32)
    broken = [SO.Staged("coords", xyz, far), SO.Staged("coords", xyz, np.where(np.arange(n)[:, None] == 2, np.inf, xyz[::-1])),
              SO.Staged("element", i % 9, (i + 1) % 9 + (i == 7) * 9), SO.Staged("charge", (i % 3 - 1) * 2, ((i + 1) % 3 - 1) * 2 + (i == 0)),
              SO.Staged("finite", f, nan), SO.Staged("positive", f, neg),
              SO.Staged("neigh", np.full((n, 2), -1), np.where(i[:, None] == 4, n, 0) * np.ones((1, 2), np.int32), N=n),
              SO.Staged("neigh", np.full((n, 2), -1), np.full((n, 2), -2), N=n),
              SO.Staged("perm", i, np.r_[i[::-1][:-1], 1], n=n), SO.Staged("values", i, i[::-1] + (i == 0)),
              SO.Staged("finite", f, np.r_[f[:46], f[46:] + 1.0]),                 # 8 % of the entries differ
              SO.Staged("finite", f, f[:-1])]
    for s in broken:
        assert SO.violations(s), (s.kind, s.decoy[:8])
    assert SO.violations(SO.Staged("finite", f, f[::-1])) == []
    assert SO.violations(SO.Staged("perm", i, i[::-1], n=n)) == []


def test_host_arguments_are_shared_and_decoy_coordinates_keep_the_contacts():
    """Both sets of a case are built around ONE dict of host arguments.  The devices whose contacts are the first and last
    sites in x order keep every x where it was; the T device keeps its atom count, of which the row partition is made."""
    import tpath_ref as T
    for name in ("initialize_sparsity_K", "neighbor_list", "initialize_sparsity_T"):
        s = SO.case(name)["arrays"]["xyz"]
        assert np.array_equal(s.true[:, 0], s.decoy[:, 0]), name
        assert np.array_equal(np.sort(s.true[:, 1]), np.sort(s.decoy[:, 1])) and np.array_equal(np.sort(s.true[:, 2]), np.sort(s.decoy[:, 2]))
    t = SO.case("initialize_sparsity_T")
    el = t["arrays"]["element"]
    atoms = lambda e: np.flatnonzero((e != T.DEFECT) & (e != T.OXYGEN_DEFECT))
    assert len(atoms(el.true)) == len(atoms(el.decoy)) == t["host"]["N_atom"]
    assert not np.array_equal(atoms(el.true), atoms(el.decoy))              # ... and another set of atoms: the pattern shows it
    metal = np.isin(el.true, t["host"]["case"]["metals"])
    assert np.array_equal(el.true[metal], el.decoy[metal])
    # on the lattice the decoy is the same set of positions: no two sites coincide
    xyz = t["arrays"]["xyz"]
    as_set = lambda a: sorted(map(tuple, a.tolist()))
    assert as_set(xyz.true) == as_set(xyz.decoy) and len(set(map(tuple, xyz.decoy.tolist()))) == len(xyz.decoy)
    # the periodic index refuses sites that span a whole period: the decoy spans what the true sites span
    p = SO.case("compute_cutoff_list_pbc")
    span = p["arrays"]["xyz"].decoy.max(axis=0) - p["arrays"]["xyz"].decoy.min(axis=0)
    assert (span[1:] < p["host"]["lattice"][1:]).all()


def test_the_table_names_every_entry_point_of_the_issue():
    want = {"spmv", "pcg_jacobi/loop", "pcg_jacobi/resident", "solve_sparse_CG_Jacobi", "pack", "unpack", "unpack_add",
            "elementwise_vector_vector", "neighbor_list", "neighbor_list_pbc", "initialize_sparsity_K", "update_charge",
            "k_assemble", "k_assemble_contacts", "background_potential_sparse", "background_potential_sparse_contacts",
            "update_CB_edge_sparse", "sum_and_gather_potential", "update_temperature_global", "update_temperature_local",
            "compute_cutoff_list", "compute_cutoff_list_pbc", "poisson_gridless/seventeen", "poisson_gridless/cube",
            "initialize_sparsity_T", "t_assemble", "update_power_sparse", "current_map", "current_profile", "event_rates",
            "execute_kmc_step", "execute_kmc_step_thermal", "conductive_clusters", "site_set_gap", "filament_gap",
            "site_set_chain", "filament_chain", "site_set_gap_pbc", "site_set_chain_pbc", "site_gradient", "matrix_values"}
    assert want == set(SO.CASES)
    assert set(SO.SETUP) <= set(SO.CASES)
    for name in SO.SETUP:                                  # the host copy these make is of the coordinates: staged in each
        assert SO.case(name)["arrays"]["xyz"].kind == "coords", name
    assert SO.case("execute_kmc_step")["host"]["N"] < 2000
