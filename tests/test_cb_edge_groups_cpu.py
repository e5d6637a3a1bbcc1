"""CPU: what the band-edge solve on rank groups adds to the host side.  KMCF_CB_SCALED chooses which collectives a
rank enters (the scaled form exchanges 1/sqrt(diag) through the halo), so the option table reports it as a group knob;
and kmcf_solve_sparse_CG_Jacobi, which no longer refuses communicators of several ranks, still refuses a host-only
matrix with KMCF_ERR_STATE on any of them."""
import ctypes as C

import numpy as np
import pytest

KMCF_ERR_STATE = -4


def test_cb_scaled_is_a_group_knob(km):
    table = {t[0]: t for t in km.solvers.KMC_comm.option_table()}
    name, values, scope, group = table["KMCF_CB_SCALED"]
    assert group is True
    assert scope == 0                    # still read per call on the communicator
    assert values == "0 / 1"


@pytest.mark.parametrize("P", [1, 2])
def test_scaled_cg_refuses_a_host_only_matrix(km, P):
    S = km.solvers
    lib = km.lib.load()
    n = 12
    counts, displs = S.KMC_comm.partition(n, P)
    for r in range(P):
        comm = S.KMC_comm(n, n, n, n, rank=r, size=P, device=-1)          # device -1: host-only planning
        r0, nr = int(displs[r]), int(counts[r])
        rows = np.arange(r0, r0 + nr)
        col = np.stack([np.maximum(rows - 1, 0), rows, np.minimum(rows + 1, n - 1)], axis=1)
        col = [np.unique(c) for c in col]
        rp = np.concatenate([[0], np.cumsum([len(c) for c in col])]).astype(np.int32)
        m = S.Distributed_matrix(comm, n, counts, displs, np.concatenate(col).astype(np.int32), rp, None)
        b = np.ones(max(nr, 1))
        x = np.zeros(max(nr, 1))
        dp = C.POINTER(C.c_double)
        rc = lib.kmcf_solve_sparse_CG_Jacobi(m.handle, b.ctypes.data_as(dp), x.ctypes.data_as(dp), 1e-14, 100, None)
        assert rc == KMCF_ERR_STATE, rc
        assert "host-only" in lib.kmcf_last_error().decode()
        assert np.all(b == 1.0) and np.all(x == 0.0)                      # nothing was touched
        m.close()
        comm.close()
