"""CPU: the C ABI of kmcf_pair_correlation and kmcf_defect_correlation -- the symbols, the size of the stats, and every
KMCF_ERR_ARG arm that needs no device (kmcf_last_error names the argument and the call).  The arguments are checked before
the index is, so the calls are made without one: well-formed arguments end at "p is NULL".  The one arm that needs an
index -- r_max above its cutoff radius -- is in tests/test_gpu_pair_corr.py."""
import ctypes as C

import pytest

ERR_ARG = -1
FAKE = C.c_void_p(64)       # a device pointer that is never dereferenced: every call returns from the checks


def _host_comm(km):
    h = C.c_void_p()
    km.lib.check(km.lib.load().kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    return h


def _args(fn):
    """well-formed arguments apart from the NULL index"""
    a = dict(p=None, d_x=FAKE, d_y=FAKE, d_z=FAKE)
    if fn == "kmcf_pair_correlation":
        a.update(d_site_class=FAKE, n_classes=3)
    else:
        a.update(d_site_element=FAKE, d_site_charge=FAKE, probe_all=1)
    a.update(r_max=10.0, n_bins=16, r_count=5.0, d_site_cell=FAKE, n_cells=4, h_hist=True, h_members=True, h_edge2=True, d_site_count=None)
    if fn == "kmcf_defect_correlation":
        a.update(d_site_class_out=None)
    a.update(stats=None)
    return a


def _call(km, fn, change):
    lib = km.lib.load()
    a = _args(fn)
    a.update(change)
    hist, members, edge2 = (C.c_uint64 * 8)(), (C.c_int * 8)(), (C.c_double * 8)()
    for k, buf in (("h_hist", hist), ("h_members", members), ("h_edge2", edge2)):
        a[k] = buf if a[k] is True else None
    h = _host_comm(km)                      # (a host-only communicator in the process: nothing here may need a device)
    try:
        rc = getattr(lib, fn)(*a.values())
        return rc, lib.kmcf_last_error() or b""
    finally:
        lib.kmcf_comm_destroy(h)


def test_symbols_and_struct(km):
    lib = km.lib.load()
    for fn in ("kmcf_pair_correlation", "kmcf_defect_correlation"):
        assert hasattr(lib, fn) and fn in km.lib.SIGNATURES
    assert len(km.lib.SIGNATURES["kmcf_pair_correlation"][1]) == 16 and len(km.lib.SIGNATURES["kmcf_defect_correlation"][1]) == 18
    assert C.sizeof(km.lib.PairStats) == 32
    assert [(n, getattr(km.lib.PairStats, n).offset) for n, _ in km.lib.PairStats._fields_] == [
        ("n_pairs_total", 0), ("n_members", 8), ("n_probes", 12), ("max_count", 16), ("max_count_site", 20), ("ms", 24)]


COMMON = [(dict(), b"p is NULL"), (dict(d_x=None), b"d_x"), (dict(d_y=None), b"d_y"), (dict(d_z=None), b"d_z"),
          (dict(h_hist=None), b"h_hist"), (dict(h_members=None), b"h_members"),
          (dict(n_bins=0), b"n_bins"), (dict(n_bins=257), b"n_bins"), (dict(n_bins=256), b"p is NULL"),
          (dict(r_max=float("nan")), b"r_max"), (dict(r_max=float("inf")), b"r_max"), (dict(r_max=0.0), b"r_max"),
          (dict(r_max=-1.0), b"r_max"),
          (dict(r_count=float("nan")), b"r_count"), (dict(r_count=float("inf")), b"r_count"), (dict(r_count=0.0), b"r_count"),
          (dict(r_count=-2.0), b"r_count"), (dict(r_count=10.5), b"r_count"), (dict(r_count=10.0), b"p is NULL"),
          (dict(n_cells=0), b"n_cells"), (dict(n_cells=-3), b"n_cells"), (dict(d_site_cell=None), b"d_site_cell"),
          (dict(d_site_cell=None, n_cells=1), b"p is NULL"),
          (dict(h_edge2=None), b"p is NULL"),
          (dict(n_cells=(1 << 24) // (6 * 16), n_bins=16), b"2^24"), (dict(n_cells=(1 << 24) // (6 * 16) - 1, n_bins=16), b"p is NULL")]


@pytest.mark.parametrize("change,word", COMMON + [
    (dict(d_site_class=None), b"d_site_class"), (dict(n_classes=0), b"n_classes"), (dict(n_classes=5), b"n_classes"),
    (dict(n_classes=4), b"p is NULL"), (dict(n_classes=1), b"p is NULL"),
    (dict(n_classes=4, n_bins=256, n_cells=(1 << 24) // 2560), b"2^24"),
    (dict(n_classes=4, n_bins=256, n_cells=(1 << 24) // 2560 - 1), b"p is NULL")])
def test_pair_correlation_argument_errors_without_an_index(km, change, word):
    rc, msg = _call(km, "kmcf_pair_correlation", change)
    assert rc == ERR_ARG and word in msg and b"kmcf_pair_correlation" in msg, (rc, msg)


@pytest.mark.parametrize("change,word", COMMON + [
    (dict(d_site_element=None), b"d_site_element"), (dict(d_site_charge=None), b"d_site_charge"), (dict(probe_all=0), b"p is NULL")])
def test_defect_correlation_argument_errors_without_an_index(km, change, word):
    rc, msg = _call(km, "kmcf_defect_correlation", change)
    assert rc == ERR_ARG and word in msg and b"kmcf_defect_correlation" in msg, (rc, msg)
