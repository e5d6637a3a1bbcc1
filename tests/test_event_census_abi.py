"""CPU: the C ABI of kmcf_event_census on a host-only communicator -- the symbol, the size of a bucket, every KMCF_ERR_ARG
arm before anything needs a device (kmcf_last_error names the argument), and KMCF_ERR_STATE for valid arguments."""
import ctypes as C

import pytest

ERR_ARG, ERR_STATE = -1, -4
FAKE = 64           # a device pointer that is never dereferenced: every call returns from the checks


def _host_comm(km):
    h = C.c_void_p()
    km.lib.check(km.lib.load().kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    return h


def _call(km, h, **over):
    """kmcf_event_census with well-formed arguments, some replaced: (rc, message)"""
    L = km.lib
    lib = L.load()
    n_cells, n_bins = over.get("n_cells", 3), over.get("n_bins", 8)
    cnt, dsp = (C.c_int * 1)(over.get("count", 4)), (C.c_int * 1)(over.get("displ", 0))
    E = [(C.c_double * 8)() for _ in range(4)]
    table = (L.CensusBucket * ((max(n_cells, 0) + 1) * 8 * 4))()
    spectrum = (C.c_int64 * (4 * max(n_bins, 1)))()
    st = L.CensusStats()
    a = dict(c=h, N=over.get("N", 4), h_count=cnt, h_displs=dsp, nn=52, neigh=FAKE, layer=FAKE, T_bg=300.0, freq=1e14, sigma=3.5e-10,
             k=1.0, x=FAKE, y=FAKE, z=FAKE, pot=FAKE, element=FAKE, charge=FAKE, num_layers=5, E0=E[0], E1=E[1], E2=E[2], E3=E[3],
             T=None, rate_mode=0, cell=FAKE, n_cells=n_cells, h_table=table, n_bins=n_bins, e_lo=-128, e_step=16,
             h_spectrum=spectrum, row_rate=None, row_best=None, stats=C.byref(st))
    a.update({k: v for k, v in over.items() if k in a and k not in ("n_cells", "n_bins", "N")})
    rc = lib.kmcf_event_census(*a.values())
    return rc, lib.kmcf_last_error() or b""


def test_symbol_and_struct_sizes(km):
    lib = km.lib.load()
    assert hasattr(lib, "kmcf_event_census") and "kmcf_event_census" in km.lib.SIGNATURES
    assert C.sizeof(km.lib.CensusBucket) == 40 and km.solvers.CENSUS_DTYPE.itemsize == 40
    assert [km.solvers.CENSUS_DTYPE.fields[n][1] for n, _ in km.lib.CensusBucket._fields_] == \
        [getattr(km.lib.CensusBucket, n).offset for n, _ in km.lib.CensusBucket._fields_]
    assert C.sizeof(km.lib.CensusStats) == 4 * 8 + 4 * 8 + 4 * 8 + 2 * 8 + 8 + 4 * 4 + 2 * 4


@pytest.mark.parametrize("over, word", [
    (dict(rate_mode=3), b"rate_mode"), (dict(rate_mode=1), b"d_site_temperature"), (dict(T_bg=0.0), b"T_bg"),
    (dict(neigh=None), b"null argument"), (dict(E2=None), b"null argument"), (dict(h_count=None), b"null argument"),
    (dict(num_layers=0), b"bad sizes"), (dict(num_layers=9), b"bad sizes"), (dict(nn=0), b"bad sizes"), (dict(freq=0.0), b"bad sizes"),
    (dict(h_table=None), b"h_table"),
    (dict(n_cells=0), b"n_cells"), (dict(n_cells=1025), b"n_cells"),
    (dict(cell=None), b"d_site_cell"),
    (dict(n_bins=-1), b"n_bins"), (dict(n_bins=257), b"n_bins"),
    (dict(h_spectrum=None), b"h_spectrum"), (dict(e_step=0), b"e_step"),
    (dict(n_bins=0), b"h_spectrum"),
    (dict(count=1 << 26, N=1 << 26), b"count * nn"), (dict(count=5), b"h_count"),
])
def test_argument_errors_before_the_device(km, over, word):
    h = _host_comm(km)
    try:
        rc, msg = _call(km, h, **over)
        assert rc == ERR_ARG and word in msg and b"kmcf_event_census" in msg, (rc, msg)
    finally:
        km.lib.load().kmcf_comm_destroy(h)


@pytest.mark.parametrize("over", [dict(), dict(cell=None, n_cells=1), dict(n_bins=0, h_spectrum=None), dict(stats=None),
                                  dict(rate_mode=2, T=FAKE), dict(n_cells=1024, n_bins=256)])
def test_valid_arguments_reach_the_host_only_check(km, over):
    h = _host_comm(km)
    try:
        rc, msg = _call(km, h, **over)
        assert rc == ERR_STATE and b"host-only" in msg and b"kmcf_event_census" in msg, (rc, msg)
    finally:
        km.lib.load().kmcf_comm_destroy(h)
