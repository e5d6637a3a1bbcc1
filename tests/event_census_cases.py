"""The cases of the event census tests (tests/test_event_census_ref.py on the CPU, tests/test_gpu_event_census.py on the
device): the synthetic graphs of tests/events_graph_ref.py plus

    dense   a ring list, N = 20 000, nn = 8, odd offsets only, with wrap: even sites DEFECT, odd sites O, so that every
            slot of an even row is a generation event -- buckets with tens of thousands of terms.  Under that pattern
            alone rows 255 and 256 are never both live, so slot 2047 (the last of compaction tile 0) could not be live
            next to 2048 and 2049: site 255 is a DEFECT and site 262 an O as well, which makes slot 7 of row 255 (-> 262)
            and slots 0 and 1 of row 256 (-> 249, 251) live.  79 986 live slots.
    empty   every site O: a list without events

cell maps with three cells plus sites outside every cell (both below 0 and above n_cells - 1), and rows cut as
(count, displ) slices with displ > 0 and counts that are no multiple of 16."""
import numpy as np

import event_census_ref as CR
import events_graph_ref as G
import events_thermal_ref as R

CASES = ("tiny", "pairs1", "chain2", "asym", "mixed", "nn63", "nn64", "nn70", "edge_group_8193", "dense", "empty")
TEMPERATURES = (300.0, 10.0)
N_CELLS = 3
BINS = CR.DEFAULT_BINS
SCAN_TILE = 2048                    # csrc/kmcf_block.hpp: KMCF_SCAN_TILE, slots per compaction tile


def _dense():
    N = 20000
    c = G.graph_case("dense", G.ring_list(N, [1, 3, 5, 7], True, 8), 0, 21)
    c["element"][0::2] = R.DEFECT
    c["element"][255], c["element"][262] = R.DEFECT, R.O_EL
    return c


BUILDERS = dict(G.BUILDERS)
BUILDERS["dense"] = _dense
BUILDERS["empty"] = lambda: G.graph_case("empty", G.ring_list(3001, [1, 2], False, 4), 0, 22)
_cache = {}


def case(name, T_bg=300.0):
    """the case at a background temperature (the arrays are shared, never modified)"""
    if name not in _cache:
        _cache[name] = G.case(name) if name in G.BUILDERS else BUILDERS[name]()
    c = dict(_cache[name])
    c["T_bg"] = T_bg
    return c


def rates(name, T_bg=300.0):
    """(type, prob) of events_thermal_ref.event_list, once per process"""
    key = ("rates", name, T_bg)
    if key not in _cache:
        typ, prob = G.rates(case(name, T_bg))
        typ.setflags(write=False)
        prob.setflags(write=False)
        _cache[key] = (typ, prob)
    return _cache[key]


def cell_map(N):
    """three cells of N / 3 consecutive sites; every 7th site lies below every cell (-1), every 11th above (5)"""
    s = np.arange(N, dtype=np.int64)
    cell = (s * N_CELLS // N).astype(np.int32)
    cell[s % 7 == 3] = -1
    cell[s % 11 == 5] = 5
    return cell


def live_rows(typ):
    return (np.asarray(typ) != R.EV_NULL).any(axis=1)


def slices(name):
    """(count, displ) pieces of consecutive rows, displ > 0, whose inner boundary cuts a run of live rows"""
    if name == "dense":
        return [(253, 3), (9999, 256), (9745, 10255)]
    typ, _ = rates(name)
    live = live_rows(typ)
    N = len(live)
    both = np.flatnonzero(live[1:] & live[:-1]) + 1         # rows r with r - 1 live too
    cut = int(both[np.searchsorted(both, N // 2)])
    return [(cut - 77, 77), (N - cut - 5, cut)]


def reference(name, T_bg=300.0, cells=False, count=None, displ=0, typ_prob=None):
    """the restatement on the rows [displ, displ + count) of a case; typ_prob: the list to restate (default: the CPU's)"""
    c = case(name, T_bg)
    typ, prob = typ_prob if typ_prob is not None else (a[displ:displ + (c["N"] if count is None else count)] for a in rates(name, T_bg))
    count = c["N"] - displ if count is None else count
    return CR.census(typ, prob, c["neigh"][displ:displ + count], c["lay"], len(c["layers"]), displ=displ,
                     cell=cell_map(c["N"]) if cells else None, n_cells=N_CELLS if cells else 1, bins=BINS)
