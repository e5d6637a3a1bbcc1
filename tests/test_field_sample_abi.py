"""CPU: the C ABI of kmcf_field_sample and kmcf_field_grid -- the symbols, the size and layout of the stats, and every
KMCF_ERR_ARG arm that needs no device (kmcf_last_error names the argument and the call).  The arguments are checked before
the index is, so the calls are made without one: well-formed arguments end at "p is NULL".  The arms that need an index or
a device -- a radius above the cutoff radius, a point that is not finite or too far out -- are in
tests/test_gpu_field_sample.py."""
import ctypes as C

import pytest

ERR_ARG = -1
FAKE = C.c_void_p(64)       # a device pointer that is never dereferenced: every call returns from the checks
NAN, INF = float("nan"), float("inf")


def _host_comm(km):
    h = C.c_void_p()
    km.lib.check(km.lib.load().kmcf_comm_create(C.byref(h), -1, 1, 0), "comm")
    return h


def _args(fn):
    """well-formed arguments apart from the NULL index"""
    a = dict(p=None, d_x=FAKE, d_y=FAKE, d_z=FAKE, d_site_mask=FAKE, n_fields=3, d_values=FAKE)
    if fn == "kmcf_field_sample":
        a.update(n_points=100, d_px=FAKE, d_py=FAKE, d_pz=FAKE)
    else:
        a.update(h_origin=(0.0, 0.0, 0.0), h_spacing=(1.0, 0.5, 2.0), h_dims=(4, 5, 6))
    a.update(radius=6.0, normalize=1, fill=0.0, d_out=FAKE, d_wsum=FAKE, d_count=FAKE, d_nearest=FAKE, d_nearest_d2=FAKE, stats=None)
    return a


def _call(km, fn, change):
    lib = km.lib.load()
    a = _args(fn)
    a.update(change)
    for k, t in (("h_origin", C.c_double), ("h_spacing", C.c_double), ("h_dims", C.c_int)):
        if a.get(k) is not None:
            a[k] = (t * 3)(*a[k])
    if a["stats"] is True:
        a["stats"] = C.byref(km.lib.SampleStats())
    h = _host_comm(km)                      # (a host-only communicator in the process: nothing here may need a device)
    try:
        rc = getattr(lib, fn)(*a.values())
        return rc, lib.kmcf_last_error() or b""
    finally:
        lib.kmcf_comm_destroy(h)


def test_symbols_and_struct(km):
    lib = km.lib.load()
    for fn in ("kmcf_field_sample", "kmcf_field_grid"):
        assert hasattr(lib, fn) and fn in km.lib.SIGNATURES
    assert len(km.lib.SIGNATURES["kmcf_field_sample"][1]) == 20 and len(km.lib.SIGNATURES["kmcf_field_grid"][1]) == 19
    assert C.sizeof(km.lib.SampleStats) == 40
    assert [(n, getattr(km.lib.SampleStats, n).offset) for n, _ in km.lib.SampleStats._fields_] == [
        ("n_points", 0), ("n_empty", 8), ("n_visits", 16), ("n_members", 24), ("max_count", 28), ("max_count_point", 32), ("ms", 36)]
    assert km.solvers.FS_MAX_FIELDS == 8


NO_OUTPUT = dict(n_fields=0, d_values=None, d_out=None, d_wsum=None, d_count=None, d_nearest=None, d_nearest_d2=None)
COMMON = [(dict(), b"p is NULL"), (dict(d_x=None), b"d_x"), (dict(d_y=None), b"d_y"), (dict(d_z=None), b"d_z"),
          (dict(d_site_mask=None), b"p is NULL"),
          (dict(n_fields=-1), b"n_fields"), (dict(n_fields=9), b"n_fields"), (dict(n_fields=8), b"p is NULL"),
          (dict(d_values=None), b"d_values"), (dict(d_out=None), b"d_out"),
          (dict(n_fields=0), b"d_values"), (dict(n_fields=0, d_values=None), b"d_out"),
          (dict(n_fields=0, d_values=None, d_out=None), b"p is NULL"),
          (dict(radius=NAN), b"radius"), (dict(radius=INF), b"radius"), (dict(radius=0.0), b"radius"), (dict(radius=-6.0), b"radius"),
          (dict(normalize=2), b"normalize"), (dict(normalize=-1), b"normalize"), (dict(normalize=0), b"p is NULL"),
          (dict(fill=NAN), b"p is NULL"), (dict(fill=NAN, normalize=0), b"p is NULL"), (dict(fill=INF), b"p is NULL"),
          (NO_OUTPUT, b"every output is NULL"), (dict(NO_OUTPUT, stats=True), b"p is NULL"), (dict(NO_OUTPUT, d_count=FAKE), b"p is NULL"),
          (dict(d_wsum=None, d_count=None, d_nearest=None, d_nearest_d2=None), b"p is NULL")]


@pytest.mark.parametrize("change,word", COMMON + [
    (dict(n_points=-1), b"n_points"), (dict(d_px=None), b"d_px"), (dict(d_py=None), b"d_py"), (dict(d_pz=None), b"d_pz"),
    (dict(n_points=0), b"p is NULL"), (dict(n_points=0, d_px=None, d_py=None, d_pz=None), b"p is NULL"),
    (dict(n_points=2 ** 31 - 1), b"p is NULL")])
def test_field_sample_argument_errors_without_an_index(km, change, word):
    rc, msg = _call(km, "kmcf_field_sample", change)
    assert rc == ERR_ARG and word in msg and b"kmcf_field_sample" in msg, (rc, msg)


@pytest.mark.parametrize("change,word", COMMON + [
    (dict(h_origin=None), b"h_origin"), (dict(h_spacing=None), b"h_spacing"), (dict(h_dims=None), b"h_dims"),
    (dict(h_origin=(0.0, NAN, 0.0)), b"h_origin[1]"), (dict(h_origin=(0.0, 0.0, -INF)), b"h_origin[2]"),
    (dict(h_spacing=(0.0, 1.0, 1.0)), b"h_spacing[0]"), (dict(h_spacing=(1.0, -1.0, 1.0)), b"h_spacing[1]"),
    (dict(h_spacing=(1.0, 1.0, NAN)), b"h_spacing[2]"), (dict(h_spacing=(1.0, INF, 1.0)), b"h_spacing[1]"),
    (dict(h_dims=(0, 1, 1)), b"h_dims[0]"), (dict(h_dims=(1, -2, 1)), b"h_dims[1]"), (dict(h_dims=(1, 1, 0)), b"h_dims[2]"),
    (dict(h_dims=(1, 1, 1)), b"p is NULL"),
    (dict(h_dims=(2048, 1024, 1024)), b"2^31"), (dict(h_dims=(2 ** 31 - 1, 2, 1)), b"2^31"),
    (dict(h_dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)), b"2^31"),
    (dict(h_dims=(2047, 1024, 1024)), b"p is NULL"), (dict(h_dims=(2 ** 31 - 1, 1, 1)), b"p is NULL")])
def test_field_grid_argument_errors_without_an_index(km, change, word):
    rc, msg = _call(km, "kmcf_field_grid", change)
    assert rc == ERR_ARG and word in msg and b"kmcf_field_grid" in msg, (rc, msg)
