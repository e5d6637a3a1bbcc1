"""CPU: what the inputs of tests/pbc_ref.py are built for, asserted on the restatements alone, and the periodic 5 nm cell
of structure.periodic_5nm().  tests/test_gpu_pbc.py relies on every condition here.

  * no (site, charged site) pair within 1e-9 (relative) of the cutoff, except the exact ones of lattice_wrap, which `<`
    must exclude: a kernel that forms the distance with other roundings still takes the same set;
  * every case has pairs that only the minimum image brings inside the cutoff, and the periodic and the open-boundary sums
    differ by more than 1e-6 S at most sites: a non-periodic kernel cannot pass;
  * the cells of the periodic index are the ones each case is named for;
  * the neighbour lists: margin, wrap pairs, longest row below the slots of the full list and above the truncated one.

Bars on margins come from the arithmetic, not from the inputs: a distance is a handful of correctly rounded operations,
relative error a few 1e-16; 1e-9 leaves seven orders."""
import numpy as np
import pytest

import pbc_ref as P


@pytest.fixture(scope="module")
def st(km):
    return km.structure


def test_c_round_is_half_away_from_zero():
    f = np.array([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 0.0, 3.0, -7.2, 7.7])
    assert np.array_equal(P.c_round(f), [1, -1, 2, 3, -3, 0, -0.0, 0, 3, -7, 8])
    assert not np.array_equal(np.round(f), P.c_round(f))            # numpy rounds half to even


def test_distance_is_the_minimum_image():
    L = np.array([10.0, 8.0, 6.0])
    d = P.dist(1.0, 0.5, 0.25, 4.0, 7.5, 5.75, L)                    # dy = -7 -> 1, dz = -5.5 -> 0.5; x is not periodic
    assert d == np.sqrt(9.0 + 1.0 + 0.25)
    assert P.dist(0.0, 0.0, 0.0, 9.0, 0.0, 0.0, L) == 9.0
    assert P.dist(0.0, 0.0, 0.0, 0.0, 4.0, 3.0, L) == 5.0            # exactly half a period: |dy| = L / 2 either way
    assert P.dist(1.0, 0.5, 0.25, 4.0, 7.5, 5.75, None) == np.sqrt(9.0 + 49.0 + 5.5 ** 2)


@pytest.mark.parametrize("name", P.PAIRWISE_CASES)
def test_pairwise_case_conditions(dev5, name):
    c = P.pairwise_case(name)
    xyz, L = c["xyz"], c["L"]
    assert c["cells"] == (P.RANDOM_CASES[name][3] if name in P.RANDOM_CASES else (3, 3))
    assert np.all(xyz.min(0) >= 0) and np.all(xyz.max(0)[1:] - xyz.min(0)[1:] < L[1:])
    s = P.pairwise_stats(xyz, c["charge"], L)
    want, S, n = P.pairwise_reference(name, dev5["sigma"], dev5["k"])
    open_want, _, open_n = P.pairwise_reference(name, dev5["sigma"], dev5["k"], False)
    differ = float((np.abs((want - open_want).astype(np.float64)) > 1e-6 * S).mean())
    print("%s: %d sites, cells %s, margin %.3g, %d pairs at the cutoff, %d wrap pairs, periodic != open at %.0f %% of the sites"
          % (name, c["N"], c["cells"], s["margin"], s["exact"], s["wrap"], 100 * differ))
    assert int((c["charge"] != 0).sum()) == 3 * c["N"] // 10
    assert s["margin"] >= 1e-9
    assert 17000 <= s["wrap"] <= 110000
    assert differ > 0.5 and np.all(n >= open_n)
    if name == "lattice_wrap":
        assert s["exact"] > 20000
        # ... many of them across the wrap: at exactly the cutoff under the minimum image only
        cols = np.flatnonzero(c["charge"] != 0)
        D, D0 = P.dist_matrix(xyz, cols, L), P.dist_matrix(xyz, cols, None)
        assert int(((D == P.CUTOFF) & (D0 != P.CUTOFF)).sum()) > 5000
    else:
        assert s["exact"] == 0
        assert xyz[0, 1] == 0.0 and xyz[1, 1] == np.nextafter(L[1], 0.0) and xyz[2, 2] == 0.0 and xyz[3, 2] == np.nextafter(L[2], 0.0)
        N = c["N"]
        assert c["slices"][:3] == [(0, N), (0, 0), (N - 1, 1)]
        d, cnt = c["slices"][3]
        assert 0 < d and d + cnt < N and cnt % 16 != 0
    if name == "p11":                     # a second image inside the cutoff: the period is shorter than two cutoffs
        assert L[1] < 2 * P.CUTOFF and L[2] < 2 * P.CUTOFF
    if name == "p34":
        assert L[1] / 3 == P.CUTOFF


def test_charge_variants_leave_sites_without_a_term(dev5):
    one = P.pairwise_case("p23_one")
    want, S, n = P.pairwise_reference("p23_one", dev5["sigma"], dev5["k"])
    assert n[0] == 0 and 100 < int((n == 0).sum()) < one["N"] - 100 and n.max() == 1
    _, _, open_n = P.pairwise_reference("p23_one", dev5["sigma"], dev5["k"], False)
    assert int((n > open_n).sum()) > 50                                 # partners of site 0 across the face y = 0
    want, S, n = P.pairwise_reference("p23_none", dev5["sigma"], dev5["k"])
    assert not n.any() and not S.any() and not want.any()


@pytest.mark.parametrize("name", sorted(P.NEIGHBOR_CASES))
def test_neighbor_case_conditions(name):
    c = P.pairwise_case(name)
    s = P.neighbor_stats(c["xyz"], c["L"], P.NEIGHBOR_CASES[name])
    print("%s, nn_dist %.1f: margin %.3g, %d wrap pairs, longest row %d" % (name, P.NEIGHBOR_CASES[name], s["margin"], s["wrap"], s["longest"]))
    assert s["margin"] >= 1e-9 and s["wrap"] > 50
    assert P.NN_TRUNCATED < s["longest"] <= 11 < P.NN
    assert all(int(np.floor(c["L"][a] / P.NEIGHBOR_CASES[name])) >= 3 for a in (1, 2))        # the cell path


def test_fallback_case_conditions():
    c = P.pairwise_case(P.FALLBACK_CASE)
    s = P.neighbor_stats(c["xyz"], c["L"], P.FALLBACK_NN_DIST)
    print("fallback: margin %.3g, %d wrap pairs, longest row %d" % (s["margin"], s["wrap"], s["longest"]))
    assert int(np.floor(c["L"][1] / P.FALLBACK_NN_DIST)) < 3                                  # fewer than 3 cells in y
    assert s["margin"] >= 1e-9 and s["wrap"] > 1000
    assert P.FALLBACK_NN < s["longest"] <= 160                                               # truncated, below the list's capacity


def test_box_has_every_event_type_across_the_wrap(st, dev5):
    b = P.box()
    per, opn = P.box_lists()
    s = P.neighbor_stats(b["xyz"], b["L"], P.BOX_NN_DIST)
    assert s["margin"] >= 1e-9 and s["longest"] < P.BOX_NN and s["wrap"] > 100
    assert b["xyz"][:, 0].min() > st.LAYERS[1]["start_x"] and b["xyz"][:, 0].max() < st.LAYERS[2]["end_x"]
    wrap = P.wrap_slots(b["xyz"], per, b["L"], P.BOX_NN_DIST)
    lay = np.zeros(b["N"], np.int32)
    typ, prob = P.event_list(b["xyz"], per, lay, 300.0, 1e13, dev5["sigma"], dev5["k"], b["pot"], b["element"], b["charge"], st.LAYERS,
                             L=b["L"])
    t0, p0 = P.event_list(b["xyz"], per, lay, 300.0, 1e13, dev5["sigma"], dev5["k"], b["pot"], b["element"], b["charge"], st.LAYERS)
    assert np.array_equal(typ, t0)
    i = np.repeat(np.arange(b["N"]), P.BOX_NN).reshape(per.shape)
    for et in (P.EV_REC, P.EV_VDIFF, P.EV_ODIFF):
        m = wrap & (typ == et) & (b["charge"][i] != 0) & (prob > 0) & (p0 > 0)
        print("event type %d: %d wrap slots with a distance-dependent rate" % (et, int(m.sum())))
        assert m.sum() >= 3 and np.all(prob[m] != p0[m])
    assert (typ == P.EV_GEN).any()


def test_chain_crosses_the_wrap(st):
    import clusters_ref as CR
    b, ch = P.box(), P.chain()
    per, opn = P.box_lists()
    s = ch["sites"]
    y = b["xyz"][s, 1]
    assert y[1] > y[0] > y[3] > y[2]                                   # leaves at the top, re-enters at the bottom
    for a, c in zip(s[:-1], s[1:]):
        assert c in per[a] and a in per[c]
    assert s[2] not in opn[s[1]] and s[1] not in opn[s[2]]
    metals = np.array([9], np.int32)
    _, table, stats = CR.clusters(per, ch["element"], ch["charge"], metals, b["xyz"][:, 0], 0, 0)
    assert stats["n_vacancy_clusters"] == 1 and table["size"].tolist() == [4]
    _, table, stats = CR.clusters(opn, ch["element"], ch["charge"], metals, b["xyz"][:, 0], 0, 0)
    assert stats["n_vacancy_clusters"] == 2 and table["size"].tolist() == [2, 2]


def test_periodic_5nm_numbers(st):
    d0, d = st.load_device_5nm("init"), st.periodic_5nm()
    N, NL = d["N"], d["N_contact"]
    assert d0["N"] == 37650 and N == 37637 and d["pbc"] == 1 and len(d["dropped"]) == 13
    assert d["dropped"].min() == 5760 and d["dropped"].max() == 29435
    assert NL <= d["dropped"].min() and d["dropped"].max() < d0["N"] - NL
    assert np.array_equal(d["xyz"][:NL], d0["xyz"][:NL]) and np.array_equal(d["xyz"][-NL:], d0["xyz"][-NL:])
    assert np.array_equal(d["element"][:NL], d0["element"][:NL]) and np.array_equal(d["element"][-NL:], d0["element"][-NL:])
    assert len(d["element"]) == N and len(d["potential_snap6"]) == N
    L, nn = d["lattice"], d["nn_dist"]
    # before: 13 sites duplicate another one under the minimum image, the open list has 461 392 pairs
    i0, j0, dist0 = st.min_image_pairs(d0["xyz"], L, 0.5)
    assert np.array_equal(np.unique(j0), d["dropped"]) and len(np.unique(np.r_[i0, j0])) == 26
    i, j, dist = st.min_image_pairs(d["xyz"], L, nn)
    assert len(st.min_image_pairs(d["xyz"], L, 0.5)[0]) == 0
    count = np.bincount(np.r_[i, j], minlength=N)
    margin = float(np.abs(dist / nn - 1.0).min())
    x, y, z = d["xyz"].T
    open_pairs = int((P.dist(x[i], y[i], z[i], x[j], y[j], z[j]) < nn).sum())
    print("periodic 5 nm: %d pairs (%d without the wrap), neighbours %d .. %d, margin %.3g" % (len(i), open_pairs, count.min(), count.max(), margin))
    assert len(i) == 479444 and open_pairs == 461392 and len(i) - open_pairs == 18052
    assert count.min() == 10 and count.max() == 52
    assert margin >= 1e-9
    # the structure's cell list and the restatement's distance agree on every listed pair
    assert np.array_equal(dist, P.dist(x[i], y[i], z[i], x[j], y[j], z[j], L))
    # a rigid shift in y and z, re-wrapped into the cell: the same set of pairs
    sh = shifted_5nm(d)
    i2, j2, dist2 = st.min_image_pairs(sh, L, nn)
    assert np.array_equal(i2, i) and np.array_equal(j2, j)
    assert float(np.abs(dist2 / nn - 1.0).min()) >= 1e-9
    assert sh[:, 1].min() >= 0 and sh[:, 1].max() < L[1] and sh[:, 2].min() >= 0 and sh[:, 2].max() < L[2]
    assert int(((sh[:, 1] != y) | (sh[:, 2] != z)).sum()) == N


def shifted_5nm(d, shift=(17.3, 40.1)):
    """the sites of periodic_5nm() shifted by (0, 17.3, 40.1) and wrapped back into [0, L)"""
    out = d["xyz"].copy()
    for a, s in zip((1, 2), shift):
        v = out[:, a] + s
        out[:, a] = np.where(v >= d["lattice"][a], v - d["lattice"][a], v)
    return out
