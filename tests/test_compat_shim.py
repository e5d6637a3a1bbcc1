"""CPU: include/kmcfield_compat.hpp -- the drop-in definitions of the reference's gpu_solvers.h entry points --
must compile against the REFERENCE's own headers (gpu_solvers.h, gpu_buffers.h, KMC_comm.h, utils.h).  Runs only
where the reference checkout exists ($KMCF_REFERENCE, default /root/reference: the build container); the GPU
box has no reference, so the test is skipped there.  Syntax / type check only (hipcc -fsyntax-only): nothing
of the reference is built or linked."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("KMCF_REFERENCE", "/root/reference")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROCM_INC = "/opt/rocm/include"
MPI_INC = os.environ.get("KMCF_MPI_INCLUDE", "/opt/conda/include")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="reference checkout not present")
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.skipif(not os.path.exists(os.path.join(MPI_INC, "mpi.h")), reason="no mpi.h for the reference headers")
def test_compat_shim_compiles_against_reference_headers(tmp_path):
    tu = tmp_path / "kmcfield_backend.cpp"
    tu.write_text('#include "kmcfield_compat.hpp"\n')
    legacy = ["hipblas", "hipsolver", "hipsparse", "rocsparse", "rocblas", "hipcub", "rocm_smi"]   # ROCm 5 include style
    cmd = [HIPCC, "-fsyntax-only", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(REF, "src"),
           "-I" + os.path.join(REF, "dist_iterative"), "-I" + MPI_INC] + ["-I%s/%s" % (ROCM_INC, d) for d in legacy] + \
          ["-Wno-deprecated-declarations", "-Wno-unused-result", str(tu)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "error" not in r.stderr, r.stderr[-4000:]
    # every gpu_solvers.h function src/kmc_main.cpp calls is defined by the shim
    shim = open(os.path.join(ROOT, "include", "kmcfield_compat.hpp")).read()
    for name in ("compute_neighbor_list", "compute_cutoff_list", "initialize_sparsity_K", "initialize_sparsity_CB",
                 "initialize_sparsity_T", "update_CB_edge_gpu_sparse", "update_charge_gpu", "background_potential_gpu_sparse",
                 "poisson_gridless_gpu", "sum_and_gather_potential", "update_power_gpu_sparse_dist",
                 "update_temperatureglobal_gpu", "execute_kmc_step_mpi", "copytoConstMemory"):
        assert ("\n%s(" % name) in shim.replace("void ", "\n").replace("double ", "\n"), name
    # not a reference entry point: the reset a host program calls when it changes a neighbour list in place
    assert "kmcf_events_reset(comm_of(comm))" in shim
