/*
 * kmcfield.h -- C ABI of libkmcfield: MI355X-native (gfx950) field solve for
 * DeviceKMC: on-device K-matrix assembly + distributed Jacobi-PCG over a 1-D
 * row-partitioned CSR matrix.
 *
 * Every entry point cites the reference interface it replaces
 * (paths relative to the reference checkout).  All pointers named d_* are
 * DEVICE pointers on the communicator's GPU, h_* are HOST pointers.  Values
 * and vectors are double, indices / charges / ELEMENT are 32-bit int
 * (ELEMENT is a plain enum, src/utils.h:37-44).
 *
 * Error convention: every function returns KMCF_OK (0) or a negative code and
 * records a message retrievable with kmcf_last_error(); nothing calls exit()
 * (the reference aborts: src/utils.h:145-154, dist_iterative/cudaerrchk.h:12-75).
 * The C++ shim in kmcfield_compat.hpp restores abort-on-error for drop-in use.
 *
 * Stream ordering contract: device work of the library runs on its own non-blocking
 * HIP streams.  On entry every compute function orders its stream after everything the
 * caller has queued so far on the caller's stream -- the legacy null stream (what the
 * reference's kernels and plain hipMemcpy use, and PyTorch's default stream) unless
 * kmcf_comm_set_caller_stream() named another -- so buffers written by kernels or
 * asynchronous copies still in flight are complete before the library reads them.  On
 * return every function has synchronised its streams: results are visible to any stream
 * (the reference's contract, hipDeviceSynchronize at dist_conjugate_gradient.cpp:271).
 * Work queued on OTHER streams than the declared one must be synchronised by the caller.
 *
 * Threads: calls on different communicators may run concurrently (the members of an
 * in-process group are driven by one thread each); calls on ONE communicator, including
 * kmcf_set_option and kmcf_get_option, must not overlap.
 *
 * Process model: one process per GPU.  A kmcf_comm is this process's member of
 * the solver group (the reference's MPI communicator comm_K, src/KMC_comm.h:
 * 132-289).  Multi-rank groups exchange halos and dot products with RCCL.
 */
#ifndef KMCFIELD_H
#define KMCFIELD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMCF_OK 0
#define KMCF_ERR_ARG (-1)      /* bad argument / shape mismatch                */
#define KMCF_ERR_HIP (-2)      /* a HIP runtime call failed                    */
#define KMCF_ERR_COMM (-3)     /* RCCL failure or communicator not connected   */
#define KMCF_ERR_STATE (-4)    /* call order violated (e.g. solve before assemble) */
#define KMCF_ERR_NOMEM (-5)

#define KMCF_UNIQUE_ID_BYTES 256   /* two RCCL unique ids: halo communicator + reduction communicator */

typedef struct kmcf_comm kmcf_comm;     /* one rank of the solver group                  */
typedef struct kmcf_matrix kmcf_matrix; /* Distributed_matrix + Distributed_vector       */
typedef struct kmcf_kstate kmcf_kstate; /* what initialize_sparsity_K leaves in GPUBuffers */

const char *kmcf_last_error(void);
int kmcf_version(void);

/* ---------------------------------------------------------------------- */
/* Communicator (replaces MPI_Comm comm_K + select_gpu, src/kmc_main.cpp:   */
/* 72-91, src/KMC_comm.h:225-289).                                          */
/* ---------------------------------------------------------------------- */
int kmcf_comm_create(kmcf_comm **out, int device, int nranks, int rank);
/* rank 0 calls kmcf_comm_unique_id, the host program distributes the KMCF_UNIQUE_ID_BYTES
 * (torch.distributed / MPI_Bcast), then every rank calls kmcf_comm_connect.
 * A 1-rank group needs neither. */
int kmcf_comm_unique_id(void *h_id /* KMCF_UNIQUE_ID_BYTES */);
int kmcf_comm_connect(kmcf_comm *c, const void *h_id /* KMCF_UNIQUE_ID_BYTES */);
int kmcf_comm_destroy(kmcf_comm *c);
/* Test transport: all `nranks` members of an in-process group on ONE device (out: array of nranks
 * communicators, each to be driven by its own host thread).  Collectives are host-synchronous
 * device copies; exists because RCCL refuses two ranks on one GPU, so that the multi-rank logic
 * (halo maps, boundary pass, reductions) can be exercised on a 1-GPU box.  Not a performance path. */
int kmcf_comm_create_loopback(kmcf_comm **out, int device, int nranks);
/* Peer-to-peer transport (csrc/kmcf_p2p.hip): the CG's all-reduces and halo exchanges done by kernels over
 * IPC-mapped peer windows instead of one RCCL call each.  KMCF_TRANSPORT=p2p|auto makes kmcf_comm_connect set it up
 * over the RCCL communicator (auto: RCCL stays if set-up or self-test fail).  Without RCCL (kmcf_comm_connect with a
 * NULL id on a multi-rank group): every rank calls kmcf_comm_p2p_export, the host program all-gathers the
 * KMCF_P2P_HANDLE_BYTES of every rank in rank order, every rank calls kmcf_comm_p2p_import.  All waits are bounded
 * (KMCF_P2P_TIMEOUT_MS, default 2000): a peer that never arrives yields KMCF_ERR_COMM, not a hang. */
#define KMCF_P2P_HANDLE_BYTES 64
int kmcf_comm_p2p_export(kmcf_comm *c, void *h_handle /* KMCF_P2P_HANDLE_BYTES */);
int kmcf_comm_p2p_import(kmcf_comm *c, const void *h_handles /* nranks x KMCF_P2P_HANDLE_BYTES */);
const char *kmcf_comm_transport(const kmcf_comm *c);   /* "single", "loopback", "rccl", "p2p ..." */
/* Switch a group that has BOTH transports up (KMCF_TRANSPORT=p2p|auto over RCCL, or an in-process group) between
 * them; collective (every rank, same value), between solves.  Matrices built while the peer-to-peer transport was
 * active work on either. */
int kmcf_comm_select_transport(kmcf_comm *c, int use_p2p);
/* Ranks the RCCL communicator itself reports (ncclCommCount): 0 when no RCCL communicator is connected (one rank,
 * in-process groups, groups bootstrapped through the host program), -1 on an RCCL error.  The reference's benchmark
 * prints MPI_Comm_size the same way (dist_iterative_test/main_test_cg.cpp:94-118). */
int kmcf_comm_rccl_ranks(const kmcf_comm *c);
int kmcf_comm_sync(kmcf_comm *c);            /* wait for the solver streams      */
void *kmcf_comm_stream(kmcf_comm *c);        /* hipStream_t of the compute stream */
/* Declares the hipStream_t the caller queues its own device work on (NULL = legacy null
 * stream, the default); see "Stream ordering contract" above. */
int kmcf_comm_set_caller_stream(kmcf_comm *c, void *hip_stream);

/* Options per communicator: the KMCF_* knobs of INTEGRATION.md set on one communicator instead of the process's
 * environment.  A value set here wins over the environment on this communicator only and takes effect where the
 * environment would: at the next plan, solve, wait or set-up (matrices already planned keep their plan).  Connect-scope
 * knobs (KMCF_TRANSPORT, KMCF_FORCE_COMM, KMCF_P2P_WINDOW_MB, KMCF_P2P_TIMEOUT_MS, KMCF_LOOPBACK_TIMEOUT_S) are
 * settable until kmcf_comm_connect / kmcf_comm_p2p_export; in-process groups are connected at creation, so theirs come
 * from the environment.  Group knobs must be set alike on every rank: kmcf_matrix_build and a group's resident plan
 * compare them and refuse with KMCF_ERR_STATE.  Host-only communicators (device -1) accept options too.
 * key: the environment name ("KMCF_SPMV_KIND").  Flags ("set" in the table): "1" sets, "0" masks the environment.
 * value NULL: drop this communicator's override (back to the environment / the library's default).
 * KMCF_ERR_ARG: unknown key, value outside the knob's spec, or a process-wide knob (kmcf_last_error says which
 * and lists the accepted values).  KMCF_ERR_STATE: a connect-time knob on a connected communicator. */
int kmcf_set_option(kmcf_comm *c, const char *key, const char *value);
/* Effective value into buf (empty: the library decides).  Returns 0 default, 1 environment, 2 set on c, <0 error. */
int kmcf_get_option(const kmcf_comm *c, const char *key, char *buf, int buflen);
/* Enumerate the table: name, accepted values, scope (0 comm, 1 connect, 2 process), group flag. */
int kmcf_option_info(int index, const char **name, const char **values, int *scope, int *group);

/* Block-row partition rule of the reference (src/KMC_comm.h:249-263,
 * dist_iterative_test/utils.cpp:3-23). */
int kmcf_partition(int nrows, int nranks, int *h_counts, int *h_displs);

/* ---------------------------------------------------------------------- */
/* Distributed CSR matrix (Distributed_matrix ctor 1, dist_iterative/        */
/* dist_objects.h:158-167, dist_matrix.cpp:5-69; Distributed_vector          */
/* dist_vector.cpp:3-42).  Input: the rows of this rank, GLOBAL column ids.  */
/* The matrix must be structurally symmetric (dist_matrix.cpp:3).            */
/* ---------------------------------------------------------------------- */
int kmcf_matrix_create_csr(kmcf_comm *c, int matrix_size, const int *h_counts, const int *h_displs,
                           const int *h_row_ptr, const int *h_col_global, const double *h_val,
                           kmcf_matrix **out);
int kmcf_matrix_destroy(kmcf_matrix *m);

/* "Split sparse" operator of the T-matrix path, A = A_neighbour + P^T A_sub P
 * (conjugate_gradient_jacobi_split_sparse + dspmv_split_sparse::spmm_split_sparse1/2/3,
 * dist_iterative/dist_conjugate_gradient_split_sparse.cpp:18-182, dist_spmv_split_sparse.cpp;
 * Distributed_subblock_sparse, dist_objects.h:52-65).  The sub-block (rows = this rank's
 * count_sub[rank] tunnel rows, columns = GLOBAL sub indices 0..subblock_size) is merged into
 * the row-partitioned CSR at build time; kmcf_spmv / kmcf_pcg_jacobi then apply as usual
 * (no per-SpMV all-gather of the sub-vector).  h_sub_global_rows[s] = global matrix row of
 * sub index s for ALL ranks (the reference all-gathers them once,
 * src/initialize_sparsity_T.cu:752-786). */
int kmcf_matrix_create_split_sparse(kmcf_comm *c, int matrix_size, const int *h_counts, const int *h_displs,
                                    const int *h_row_ptr, const int *h_col_global, const double *h_val,
                                    int subblock_size, const int *h_count_sub, const int *h_displ_sub,
                                    const int *h_sub_global_rows, const int *h_sub_row_ptr,
                                    const int *h_sub_col, const double *h_sub_val, kmcf_matrix **out);

typedef struct {
    int matrix_size;          /* global rows                                        */
    int rows_this_rank;
    int64_t nnz;              /* of this rank, all blocks                           */
    int number_of_neighbours; /* includes self (dist_objects.h:83)                  */
    int halo_cols;            /* sum over k>=1 of nnz_cols_per_neighbour[k]         */
    int send_rows;            /* sum over k>=1 of nnz_rows_per_neighbour[k]         */
    int boundary_rows;        /* local rows that reference a halo column            */
    int spmv_kind;            /* 0 vec, 1 stream, 2 window (LDS-staged x window)    */
    int spmv_coded;           /* values currently dictionary-coded (2 B/nnz): 1 window kernel, 2 row-per-lane kernel */
    int spmv_tiles;           /* window / row-per-lane kernel: number of tiles      */
    int64_t spmv_window_cols; /* the same: sum of the tiles' window sizes           */
    int64_t spmv_stream_entries; /* coded kernels: 16-bit entries streamed per launch; row-per-lane kernels (coded, or
                                    spmv_coded==0 with f64 values): entries per launch, padding included; else 0.
                                    Where the coded row-per-lane kernel streams its entries packed (five 12-bit fields
                                    per 8-byte word, KMCF_SELL_PACK): the streamed bytes / 2, so that 2 B times this
                                    field stays the bytes a launch reads */
} kmcf_matrix_info_t;
int kmcf_matrix_info(const kmcf_matrix *m, kmcf_matrix_info_t *info);

/* Halo lists for inspection (cols_per_neighbour / rows_per_neighbour,
 * dist_matrix.cpp:390-487).  k in [0, number_of_neighbours); pass NULL to query
 * sizes.  *neighbour_rank = neighbours[k]. */
int kmcf_matrix_neighbour(const kmcf_matrix *m, int k, int *neighbour_rank, int *nnz_block,
                          int *ncols, int *h_cols, int *nrows, int *h_rows);

/* Internal row order for inspection (no reference counterpart: the reference keeps the caller's order).
 * h_perm[i] = caller's local row stored as internal row i (rows_this_rank entries; NULL: skip).  The rows longer
 * than KMCF_LONG_ROW come last; *n_short = number of rows before them.  h_tile_end: end row (exclusive, internal
 * order) of every tile of the row-per-lane SpMV layout, *n_tiles of them (pass NULL to query the count; 0 when
 * the order was not refined for that layout). */
int kmcf_matrix_row_order(const kmcf_matrix *m, int *h_perm, int *n_short, int *h_tile_end, int *n_tiles);

/* Summation order of the solver kernels for inspection (no reference counterpart).  The CG's dot products and the
 * SpMV's row sums are deterministic: one partial per block, blocks and lanes added in a fixed order that depends
 * only on the quantities below.  tests/ feed them to the CPU oracle, which then adds in the same order and must
 * reproduce the device's iterates bit for bit (oracle/kmcf_oracle_order.c). */
typedef struct {
    int rows, n_short, halo_cols;
    int vec_grid;           /* blocks of the CG's vector kernels = r.z / b.b partials                           */
    int sell_active;        /* 1: the row-per-lane coded kernel computes the short rows (else: see spmv_kind)    */
    int sell_ident;         /* 1: lane t of a tile owns internal row first + t                                   */
    int sell_grid;          /* its blocks = p.Ap partials of the interior pass                                   */
    int sell_tiles;
    int boundary_grid, boundary_lpr, boundary_rows;   /* separate pass over the rows that touch the halo (0: none) */
    int long_items;         /* chunks of the long-row kernel (0: none)                                           */
    int sub_grid;           /* blocks of the tunnel sub-block operator (0: none)                                 */
    int cg_variant;         /* recurrence a solve on this matrix runs now: 0 classic (reference order), 1 single-reduction */
    int resident_tpb;       /* > 0: the solve runs as ONE register-resident launch (kmcf_cgr.hip); tiles per block        */
    int resident_g1;        /* ... blocks per group of its two-stage reduction                                          */
    int reserved[1];
} kmcf_sum_plan_t;
/* h_tile_first / h_tile_rows: first internal row and row count of every row-per-lane tile (sell_tiles entries each;
 * NULL: skip).  h_row_ptr / h_col / h_val: the CSR as stored (internal row order, entries of a row in creation
 * order, own columns as internal row ids, halo columns as rows + halo slot; NULL: skip). */
int kmcf_matrix_sum_plan(const kmcf_matrix *m, kmcf_sum_plan_t *plan, int *h_tile_first, int *h_tile_rows,
                         int *h_row_ptr, int *h_col, double *h_val);

/* Global column of every halo slot (halo_cols entries; column n_loc + h of the stored CSR is global column h_gid[h]). */
int kmcf_matrix_halo_columns(const kmcf_matrix *m, int *h_gid);

/* Overwrite the values (same order as the CSR given at creation). */
int kmcf_matrix_set_values(kmcf_matrix *m, const double *h_val);
/* Copy the values back (creation order). */
int kmcf_matrix_get_values(const kmcf_matrix *m, double *h_val);

/* Ap = A p, distributed: halo pack + exchange overlapped with the interior
 * rows, then boundary rows (dspmv::gpu_packing_cam, dist_iterative/
 * dist_spmv_gpu_packing.cpp:106-228).  d_p, d_Ap: rows_this_rank doubles.
 * Synchronous (returns after the result is visible). */
int kmcf_spmv(kmcf_matrix *m, const double *d_p, double *d_Ap);

/* Timing helper for the roofline line: runs `reps` SpMVs (with_dot != 0: the
 * CG variant with the fused p.Ap partial) on the compute stream bracketed by HIP
 * events on that stream; *ms_total receives the elapsed time. */
int kmcf_spmv_bench(kmcf_matrix *m, int reps, int with_dot, float *ms_total);

/* Re-plans the SpMV of an existing matrix from the effective KMCF_SPMV_* values -- its communicator's options
 * (kmcf_set_option), else the environment -- (KIND 0 vec / 1 stream (CSR) / 2 window, CODED 0/1, SELL ...) and
 * re-codes its current values.  Measurement aid: bench.py times
 * the CSR kernel on the same matrix with it (the `roofline_csr` block); tests compare the kernels. */
int kmcf_spmv_replan(kmcf_matrix *m);

/* Diagnostic for multi-rank runs (collective: same arguments on every rank):
 * times `reps` repetitions of one piece of a distributed CG iteration on the
 * compute stream -- kind 0: the all-reduce of the 3 fused scalars, 1: the halo
 * exchange alone (pack, send/recv, wait), 2: the SpMV kernels alone (interior
 * + boundary rows, no exchange), 3 (split operators only): pack + all-gather of
 * the tunnel sub-vector + the wait for it. */
int kmcf_comm_bench(kmcf_matrix *m, int kind, int reps, float *ms_total);

typedef struct {
    int iterations;       /* CG iterations executed (reference prints K = iterations+1) */
    int converged;        /* 1 if the stopping rule was met                             */
    double relres;        /* sqrt(rz/bb), dist_conjugate_gradient.cpp:273                */
    double bb;            /* ||b||^2 (all ranks)                                        */
    double rz;            /* last r.z                                                   */
    float ms_solve;       /* device time (HIP events, compute stream): of the CG loop; kmcf_pcg_jacobi: of everything
                           * the call enqueued (vectors in, r = b - A x0, the iterations, vectors out) */
    float ms_assembly;    /* device time of the assembly kernels (K solve only)         */
} kmcf_solve_stats_t;

/* Jacobi-PCG (iterative_solver::conjugate_gradient_jacobi, dist_iterative/
 * dist_conjugate_gradient.cpp:149-276).  d_r: rhs in, residual out; d_x: start
 * guess in, solution out; d_diag_inv: 1/diag (NULL = unpreconditioned CG,
 * conjugate_gradient :17-121).  Stop when r.z/(b.b) <= tol^2 or after max_it
 * iterations; fixed_iters > 0 runs exactly that many (bench mode). */
int kmcf_pcg_jacobi(kmcf_matrix *m, double *d_r, double *d_x, const double *d_diag_inv,
                    double relative_tolerance, int max_iterations, int fixed_iters,
                    kmcf_solve_stats_t *stats);

/* Symmetric-scaled CG (solve_sparse_CG_Jacobi, src/
 * iterative_solvers_gpu.cu:716-887): solves D^-1/2 A D^-1/2 y = D^-1/2 b with
 * an absolute stop ||r||^2 <= tol^2 (tol 1e-14, max 50000 there); A values and
 * rhs are scaled IN PLACE like the reference.  On a rank group (every rank
 * calls it, d_rhs / d_x being its rows): 1/sqrt(diag) of the neighbours' rows
 * comes in by one halo exchange, every rank scales its own rows a_ij s_i s_j
 * and its slice of rhs and guess, the group runs plain CG with its recurrence
 * (KMCF_CG_VARIANT) under the same rule.  Afterwards kmcf_matrix_get_values
 * returns this rank's rows of the scaled matrix, d_rhs holds its scaled rows,
 * d_x its rows of the solution; `stats` are the group's (the time is the
 * rank's own). */
int kmcf_solve_sparse_CG_Jacobi(kmcf_matrix *m, double *d_rhs, double *d_x,
                                double tol, int max_iterations, kmcf_solve_stats_t *stats);

/* Small vector kernels of dist_iterative/utils_cg.cu (:4-111, :323-336). */
int kmcf_pack(kmcf_comm *c, double *d_packed, const double *d_unpacked, const int *d_indices, int n);
int kmcf_unpack(kmcf_comm *c, double *d_unpacked, const double *d_packed, const int *d_indices, int n);
int kmcf_unpack_add(kmcf_comm *c, double *d_unpacked, const double *d_packed, const int *d_indices, int n);
int kmcf_elementwise_vector_vector(kmcf_comm *c, const double *d_a, const double *d_b, double *d_out, int n);

/* ---------------------------------------------------------------------- */
/* K path                                                                    */
/* ---------------------------------------------------------------------- */

/* initialize_sparsity_K (src/iterative_solvers_gpu.cu:262-488): pattern of K
 * restricted to the interface sites [N_contact, N - N_contact) for the rows of
 * this rank + left/right contact patterns, built with a cell list instead of
 * the reference's O(n_loc*N) scan.  d_x/d_y/d_z: N site coordinates;
 * h_lattice[3]; counts/displs: row partition of the N - 2*N_contact interface
 * rows (kmc_comm.counts_K / displs_K). */
int kmcf_initialize_sparsity_K(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z,
                               const double *h_lattice, int N, int pbc, double nn_dist, int N_contact,
                               const int *h_counts, const int *h_displs, kmcf_kstate **out);
int kmcf_kstate_destroy(kmcf_kstate *k);
kmcf_matrix *kmcf_kstate_matrix(kmcf_kstate *k);   /* gpubuf.K_distributed */

/* Pattern export for tests (global interface column ids, ascending per row);
 * which: 0 = K rows of this rank, 1 = left contact block, 2 = right contact
 * block.  Pass h_col = NULL to query *nnz. */
int kmcf_kstate_pattern(const kmcf_kstate *k, int which, int *h_row_ptr, int *h_col, int64_t *nnz);

/* update_charge_gpu (src/potential_solver_gpu.cu:12-85): writes the charges of
 * the rows [displ[rank], displ[rank]+count[rank]) and all-gathers them. */
int kmcf_update_charge(kmcf_comm *c, const int *d_site_element, int *d_site_charge, const int *d_neigh_idx,
                       int N, int nn, const int *d_metals, int num_metals,
                       const int *h_count, const int *h_displ);

/* K value assembly only (the first half of background_potential_gpu_sparse,
 * src/potential_solver_gpu.cu:888-1042 with kernels :246-285, :323-367,
 * :438-454, :774-830): fills the CSR values, diagonal, 1/diag and rhs. */
int kmcf_k_assemble(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                    const int *d_metals, int num_metals, double Vd, double high_G, double low_G);
/* Copies of the assembled per-row vectors (rows_this_rank each; NULL to skip). */
int kmcf_k_get_vectors(const kmcf_kstate *k, double *h_diag, double *h_dinv, double *h_rhs,
                       double *h_left, double *h_right);

/* background_potential_gpu_sparse (src/potential_solver_gpu.cu:846-1128):
 * assembly + PCG (tol 1e-14*N_interface, max_it 10000, :885-886), solution
 * written in place into d_site_potential_boundary[N_left + displ ...] whose
 * previous content is the initial guess. */
int kmcf_background_potential_sparse(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                                     const int *d_metals, int num_metals,
                                     double *d_site_potential_boundary,
                                     int N, int N_left_tot, int N_right_tot, double Vd,
                                     double high_G, double low_G, kmcf_solve_stats_t *stats);

/* Per-line bias: one Dirichlet value per contact site instead of one scalar Vd.
 *
 * K assembly with one Dirichlet value per contact site.  d_site_potential: N doubles, whole
 * device, same layout as site_potential_boundary; only its contact slots [0, N_left) and
 * [N - N_right, N) are read, and nothing is written to it.  Values, diagonal and 1/diag are
 * those of kmcf_k_assemble (they do not depend on the bias); rhs[i] = sum over the contact
 * sites j in row i's left and right contact patterns (kmcf_kstate_pattern, which = 1, 2) of
 * G_ij * V[j], G_ij by the K rule (high_G iff both sites are metals or both uncharged
 * vacancies).  Order of addition, part of the contract: one accumulator per row starting at
 * 0.0, left entries in pattern order, then right entries in pattern order, each step one
 * fused multiply-add.  The result depends on the input alone: two calls give the same bytes,
 * and a row's rhs is the same bytes whatever the rank count and transport.  A row without
 * contact entries gets exactly 0.0.  With every left slot at -Vd/2 and every right slot at
 * +Vd/2 the system is that of kmcf_k_assemble(Vd) up to the rounding of the sums.
 * KMCF_ERR_ARG before anything needs a device: a NULL argument (kmcf_last_error names it).
 * KMCF_ERR_ARG after the call's one synchronisation: a contact value is not finite;
 * kmcf_last_error names the smallest such site id.  The contact slots are untouched then,
 * and the assembled rhs is unspecified (call again with finite values). */
int kmcf_k_assemble_contacts(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                             const int *d_metals, int num_metals, const double *d_site_potential,
                             double high_G, double low_G);

/* kmcf_background_potential_sparse with the contact values taken from the array itself: the
 * contact slots of d_site_potential_boundary are the boundary condition (read, never
 * written), its interface slice is the start guess and receives the solution (this rank's
 * rows, as in the scalar call; kmcf_sum_and_gather_potential replicates them).  Same
 * tolerance (1e-14 * N_interface), same max_it, same solver paths (register-resident launch
 * or kernel loop, either recurrence, one rank or a group).  On a group every rank passes its
 * own whole-device array with identical contact slots.  Downstream nothing changes:
 * kmcf_sum_and_gather_potential adds the whole array, contact slots included, into
 * site_potential_charge.  The band-edge and current solves still take a scalar Vd.
 * KMCF_ERR_ARG before anything needs a device (kmcf_last_error names the argument): NULL
 * argument, N / N_left_tot / N_right_tot other than the pattern's.  KMCF_ERR_COMM:
 * communicator not connected.  KMCF_ERR_ARG at the call's final synchronisation (no extra
 * host round trip on the good path): a contact value is not finite, kmcf_last_error names
 * the smallest such site id; the contact slots are untouched and the interface slice is
 * unspecified.  On a group every rank returns the same verdict. */
int kmcf_background_potential_sparse_contacts(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                                              const int *d_metals, int num_metals, double *d_site_potential_boundary,
                                              int N, int N_left_tot, int N_right_tot,
                                              double high_G, double low_G, kmcf_solve_stats_t *stats);

/* update_CB_edge_gpu_sparse (src/potential_solver_gpu.cu:575-772): Laplace solve for the
 * conduction-band edge on the K pattern: G = high_G if EITHER site is a metal (:289-319),
 * contacts at +Vd/2 (left) / -Vd/2 (right), solve_sparse_CG_Jacobi (tol 1e-14), boundary
 * fill and scaling by eV_to_J = 1.60217663e-19.  d_site_CB_edge: N doubles, in/out (its
 * interface slice is the start guess, :732).  Overwrites the K values of the state (the
 * next kmcf_k_assemble refills them).  On a rank group (every rank calls it with its own
 * whole-device array): each rank assembles and solves its rows of the K partition, the
 * stopping rule is read on the group's all-reduced r.z, the interface slices are
 * all-gathered, and every rank returns with the complete array, contacts filled and in J;
 * `stats` are the group's (the time is the rank's own).  The solve is a loop of kernels:
 * a register-resident plan of K and its buffers are not touched.  KMCF_CB_SCALED (a group
 * knob) chooses the literal scaled form. */
int kmcf_update_CB_edge_sparse(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                               const int *d_metals, int num_metals, double *d_site_CB_edge, int N,
                               int N_left_tot, int N_right_tot, double Vd, double high_G, double low_G,
                               kmcf_solve_stats_t *stats);

/* The MPI_Gatherv of the solution (src/kmc_main.cpp:367-384) + the two
 * MPI_Bcast + sum_AB_into_A of sum_and_gather_potential
 * (src/potential_solver_gpu.cu:1130-1151): replicates the interface solution
 * on every rank and does site_potential_charge += site_potential_boundary.
 * h_counts_pairwise / h_displs_pairwise (kmc_comm.counts_pairwise, displs_pairwise;
 * may be NULL): the rows of site_potential_charge each rank computed with
 * kmcf_poisson_gridless, all-gathered first (the MPI_Gatherv of src/kmc_main.cpp:
 * 405-425 + the MPI_Bcast of potential_solver_gpu.cu:1139-1142). */
int kmcf_sum_and_gather_potential(kmcf_kstate *k, double *d_site_potential_boundary,
                                  double *d_site_potential_charge, int N, int num_atoms_first_layer,
                                  const int *h_counts_pairwise, const int *h_displs_pairwise);

/* ---------------------------------------------------------------------- */
/* Short-range pairwise Poisson term                           */
/* ---------------------------------------------------------------------- */
typedef struct kmcf_pairwise kmcf_pairwise;

/* compute_cutoff_list (src/neighbor_lists_gpu.cu:293-372; cutoff 20 A there): one-off
 * spatial index of the sites; replaces the N x N_cutoff index list (gpubuf.cutoff_idx). */
int kmcf_compute_cutoff_list(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                             double cutoff_radius, kmcf_pairwise **out);
int kmcf_pairwise_destroy(kmcf_pairwise *p);

/* Periodic boundaries in y and z (the simulator's `pbc` parameter).  ONE distance applies to everything periodic in
 * this library -- the K pattern (kmcf_initialize_sparsity_K), kmcf_neighbor_list_pbc, the index below and the event
 * step after kmcf_events_set_lattice -- the reference's four-argument site_dist (src/gpu_solvers.h:287-319):
 *     dx = x1 - x2;   fy = (y1 - y2) / Ly;  fy -= round(fy);  dy = fy * Ly;   z like y;   dist = sqrt(dx*dx + dy*dy + dz*dz)
 * with Ly = h_lattice[1], Lz = h_lattice[2] and round() the C round (half away from zero); x is never periodic.  Only
 * the minimum image counts: where a period is shorter than two cutoffs, a second image inside the cutoff is NOT added.
 * With pbc == 0 every function keeps the open-boundary expression (and result bytes) of its non-periodic entry point.
 *
 * kmcf_compute_cutoff_list_pbc: the spatial index with pbc and the periods remembered.  pbc == 0: exactly the index of
 * kmcf_compute_cutoff_list (h_lattice may be NULL).  pbc == 1: x as before; in y the cells tile [min y, min y + Ly)
 * exactly, max(1, floor(Ly / cutoff)) cells of width >= cutoff; z likewise.  kmcf_poisson_gridless on such an index sums
 * over the charged j != i whose minimum-image distance is < cutoff (same term, no atomics, same bytes on every call).
 * KMCF_ERR_ARG, kmcf_last_error naming the axis: pbc outside 0 / 1; with pbc == 1 a NULL h_lattice, a period that is
 * not finite or <= 0 (both before anything needs a device), or sites that span a whole period (max - min >= L) on a
 * periodic axis -- wrap them into one cell first. */
int kmcf_compute_cutoff_list_pbc(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                                 double cutoff_radius, const double *h_lattice /* 3, host */, int pbc, kmcf_pairwise **out);
/* Inspection: *pbc and (h_lattice may be NULL) the three lattice values the index was built with (zeros if none). */
int kmcf_pairwise_periodic(const kmcf_pairwise *p, int *pbc, double *h_lattice /* 3, may be NULL */);

/* poisson_gridless_gpu (src/potential_solver_gpu.cu:1620-1655): for the sites
 * [displ, displ+count): site_potential_charge[i] = sum over charged sites j != i within
 * the cutoff of q_j erfc(r/(sigma sqrt 2)) k q / r  (v_solve_gpu, src/gpu_solvers.h:321-329).
 * "Within the cutoff" is the open-boundary distance on an index of kmcf_compute_cutoff_list, the minimum-image
 * distance on a periodic index of kmcf_compute_cutoff_list_pbc. */
int kmcf_poisson_gridless(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                          const int *d_site_charge, double sigma, double k, int count, int displ,
                          double *d_site_potential_charge);

/* ---------------------------------------------------------------------- */
/* KMC event step                                              */
/* ---------------------------------------------------------------------- */
/* std::mt19937 + std::uniform_real_distribution<double>(0,1): the reference's
 * RandomNumberGenerator (src/random_num.h).  kmcf_rng_next has the callback signature
 * kmcf_execute_kmc_step takes, so a host program may pass its own generator instead. */
typedef struct kmcf_rng kmcf_rng;
int kmcf_rng_create(unsigned int seed, kmcf_rng **out);
double kmcf_rng_next(void *rng);
int kmcf_rng_destroy(kmcf_rng *r);

/* execute_kmc_step_mpi (src/kmc_events.cu:333-563): builds the (site, neighbour) event list of
 * this rank's sites [displs[rank], +count[rank]) (build_event_list_split :128-207), then draws
 * events -- residence-time algorithm: first slot whose cumulative rate exceeds u*total, execute
 * (:284-331), zero the events touching the pair (:237-256), t = -log(u')/total -- until the last
 * drawn t reaches 1/freq; *event_time = that last t (the reference's return value), *n_events the
 * number of executed events, h_event_log (may be NULL; 3*max_events ints) the (i, j, type) triples.
 * d_neigh_idx: this rank's count*nn neighbour slots.  Layer energies: copytoConstMemory
 * (src/kmc_events.cu:565-571).  T_bg, freq, sigma, k: host scalars (device scalars in the reference).
 * ELEMENT / EVENTTYPE codes: src/utils.h:37-60.  Every rank must pass a generator in the same state.
 * The neighbour list is read as a constant of the run: the communicator keeps, per address d_neigh_idx and N, what
 * it has worked out about the list (whether it is symmetric, which decides how an event's slots are zeroed; a
 * replicated group's gathered copy of all ranks' lists).  While the communicator lives, the CONTENTS of a list at a
 * given address must not change without a call of kmcf_events_reset -- a list rewritten in place, or another list
 * that an allocator places at a freed list's address, is otherwise stepped with the old list's verdict and copy.
 * KMCF_ERR_STATE, "no event could be selected": no slot holds a rate (e.g. every site is O_EL) when an event is due.
 * The events executed before are counted and logged; the generator's position is unspecified after this error (the
 * paths draw a different number of uniforms before they give up). */
int kmcf_execute_kmc_step(kmcf_comm *c, int N, const int *h_count, const int *h_displs, int nn,
                          const int *d_neigh_idx, const int *d_site_layer, double T_bg, double freq,
                          double sigma, double k, const double *d_x, const double *d_y, const double *d_z,
                          const double *d_site_potential_charge, int *d_site_element, int *d_site_charge,
                          int num_layers, const double *h_E_gen, const double *h_E_rec,
                          const double *h_E_Vdiff, const double *h_E_Odiff,
                          double (*next_random)(void *), void *rng_user, int max_events,
                          double *event_time, int *n_events, int *h_event_log);

/* Drops what the communicator keeps for the event step between calls (workspace, the symmetry verdict of the
 * neighbour list, a replicated group's gathered lists): the next step works everything out again from the list it
 * is given.  For callers that change a neighbour list in place or reuse its memory; in a group, every rank calls it
 * between the same two steps.  Costs one symmetry pass and the allocations on the next step, nothing per step. */
int kmcf_events_reset(kmcf_comm *c);

/* Geometry of the pair distance that enters self_int_V in the event rates, for every later kmcf_execute_kmc_step,
 * kmcf_execute_kmc_step_thermal and kmcf_event_rates on this communicator.  pbc == 1: the minimum-image distance above
 * with Ly = h_lattice[1], Lz = h_lattice[2] (copied; pass the list of kmcf_neighbor_list_pbc, whose wrap pairs are the
 * ones this matters for).  pbc == 0 (the default of a new communicator; h_lattice may be NULL): the open-boundary
 * distance -- the kernels, and the bytes, of a communicator that never called this.  Nothing else in the step changes.
 * kmcf_events_reset does not clear the setting, kmcf_comm_destroy does.  In a group every rank sets it alike; this is
 * NOT checked.  KMCF_ERR_ARG: NULL c, pbc outside 0 / 1, NULL h_lattice or a period not finite or <= 0 with pbc == 1. */
int kmcf_events_set_lattice(kmcf_comm *c, const double *h_lattice /* 3, host; may be NULL with pbc == 0 */, int pbc);

/* Rate modes of the thermal step.  EA: the activation energy kmcf_execute_kmc_step forms; s: the site whose
 * temperature counts -- j for generation, i for recombination, vacancy diffusion and ion diffusion. */
#define KMCF_RATE_T_BG   0   /* P = freq / (exp(EA / (kB T_bg)) + 1e-200): kmcf_execute_kmc_step's rates          */
#define KMCF_RATE_EKIN   1   /* the reference's commented term: EA -= kB (T[s] - T_bg), then as KMCF_RATE_T_BG    */
#define KMCF_RATE_T_SITE 2   /* Boltzmann factor at the site's own temperature: exp(EA / (kB T[s]))              */

/* kmcf_execute_kmc_step with event rates that read the site temperatures (the field
 * kmcf_update_temperature_local leaves on every rank): d_site_temperature, N doubles, whole device (a
 * partitioned group's ranks read it at global site ids, like the potential).  A field equal to T_bg
 * everywhere gives, in both thermal modes, the bits of KMCF_RATE_T_BG.  Rates are fixed for the step.
 * rate_mode KMCF_RATE_T_BG: d_site_temperature may be NULL and is never read; the call is kmcf_execute_kmc_step.
 * KMCF_ERR_ARG (checked before anything needs a device): rate_mode outside 0..2, NULL field in mode 1 or 2,
 * T_bg <= 0.  KMCF_ERR_ARG before any event executes (site arrays and generator untouched, *n_events 0):
 * a temperature that is not finite or not > 0 at the site s of a non-null event slot; kmcf_last_error
 * names the first such site. */
int kmcf_execute_kmc_step_thermal(kmcf_comm *c, int N, const int *h_count, const int *h_displs, int nn,
                                  const int *d_neigh_idx, const int *d_site_layer, double T_bg, double freq,
                                  double sigma, double k, const double *d_x, const double *d_y, const double *d_z,
                                  const double *d_site_potential_charge, int *d_site_element, int *d_site_charge,
                                  int num_layers, const double *h_E_gen, const double *h_E_rec,
                                  const double *h_E_Vdiff, const double *h_E_Odiff,
                                  double (*next_random)(void *), void *rng_user, int max_events,
                                  double *event_time, int *n_events, int *h_event_log,
                                  const double *d_site_temperature, int rate_mode);

/* Inspection, like kmcf_kstate_pattern: builds the event list of this rank's rows [displs[rank], +count[rank])
 * in the given rate mode and copies it out; executes nothing, draws nothing, keeps nothing.
 * h_type: count*nn bytes (EVENTTYPE codes), h_prob: count*nn doubles; either may be NULL.
 * Errors as kmcf_execute_kmc_step_thermal. */
int kmcf_event_rates(kmcf_comm *c, int N, const int *h_count, const int *h_displs, int nn,
                     const int *d_neigh_idx, const int *d_site_layer, double T_bg, double freq,
                     double sigma, double k, const double *d_x, const double *d_y, const double *d_z,
                     const double *d_site_potential_charge, const int *d_site_element,
                     const int *d_site_charge, int num_layers, const double *h_E_gen,
                     const double *h_E_rec, const double *h_E_Vdiff, const double *h_E_Odiff,
                     const double *d_site_temperature, int rate_mode,
                     unsigned char *h_type, double *h_prob);

/* Event rate census: the list kmcf_event_rates returns for this rank's rows [displs[rank], +count[rank]) in the given rate
 * mode (the same build kernel, the same bits; it honours kmcf_events_set_lattice), reduced on the device to rates per cell,
 * layer and event type.  Executes nothing, draws nothing; a local operation without collectives.  Arguments up to
 * rate_mode: those of kmcf_event_rates.  Slot id = (i - displ) * nn + s.  An EVENT is a slot whose type is not NULL_EVENT
 * (4); its rate is the list's event_prob.
 * Bucket of an event (i, j, type): cell = d_site_cell[i] (the row's site), layer = d_site_layer[j] (the layer whose
 * energy entered the rate); h_table[((cell * num_layers) + layer) * 4 + type].  A cell value outside [0, n_cells) goes to
 * the REST, cell index n_cells (the convention of kmcf_current_profile).  d_site_cell == NULL (n_cells must be 1): every
 * site in cell 0.  Layers must lie in [0, num_layers), as the step requires; an event whose layer does not is left out of
 * the table, the spectrum, n_nan and with them every statistic except slots and rows_live (the row outputs keep it).
 * Nothing is stored outside the table for any input.
 * Per bucket: n_events and n_zero exact.  rate_sum: the sum of the bucket's rates that are not NaN, no atomics on doubles;
 * ORDER OF ADDITION: the events of the list in ascending slot id are numbered p = 0 ... n - 1 and cut into S pieces of
 * ceil(n / S) consecutive events, S = min(max(count * nn / 32768, 1), max(65536 / buckets, 1), 64).  Within a piece that
 * starts at p0, thread t of 256 adds the bucket's events with (p - p0) % 256 == t in ascending p to an accumulator that
 * starts at 0.0, then the xor butterfly inside each wavefront of 64 and (w0 + w1) + (w2 + w3); the pieces' sums are added
 * in ascending order to an accumulator that starts at 0.0.  The input alone fixes it: two calls on the same input return
 * the same bytes.  rate_max: the bits of one slot's rate, the largest that is not NaN; among equal rates the smallest slot
 * id (a bucket whose events all have rate 0.0: 0.0 with the pair of its first slot).  A NaN rate enters n_events and
 * stats->n_nan and nothing else.
 * Spectrum (n_bins in 0..256; 0: none, h_spectrum NULL): for a normal rate P, e = ((bits of P >> 52) & 0x7ff) - 1023, bin
 * floor((e - e_lo) / e_step) clamped into [0, n_bins - 1]; 0.0 and subnormals: bin 0; +infinity: the last bin; NaN: no
 * bin.  h_spectrum[type * n_bins + bin]: exact counts over all cells.
 * Row outputs (device, optional): d_row_rate[r] the sum of the non-NaN rates of row displ + r, in slot order by one
 * accumulator from 0.0; d_row_best[r] the slot s of the row's largest rate, the first among equals, -1 when the row has
 * no event whose rate is a number.  Rows without events: 0.0 and -1.
 * stats (host, formed from the table): rate_type[t] = sum over cell ascending, then layer ascending, of rate_sum, from
 * 0.0; rate_total = ((r0 + r1) + r2) + r3; dt_mean = 1 / rate_total (+infinity for 0); the maximum by the bucket rule.
 * In a partitioned group every rank gets the census of its own rows; tables combine on the host (integers add, sums add
 * in rank order, maxima by the rule above).
 * Keeps scratch of its own on the communicator (15 bytes per slot: type, rate, the live slots and their keys), freed by
 * kmcf_comm_destroy and dropped by kmcf_events_reset; reads and writes nothing of the event step's workspace.  Enters
 * like every entry point (stream ordering contract) and synchronises once, at its end.  count[rank] == 0: KMCF_OK, table,
 * spectrum and stats zeroed (the table's and the stats' site ids -1, as for any empty bucket), dt_mean +infinity.  A
 * list without events is no error.
 * KMCF_ERR_ARG before anything needs a device (kmcf_last_error names the argument): the checks of kmcf_event_rates,
 * count * nn >= 2^31 - 1 (slot ids are int32, as in the step's gather), rows outside [0, N), NULL h_table, n_cells
 * outside 1..1024, NULL d_site_cell with n_cells != 1, n_bins outside 0..256,
 * n_bins > 0 with NULL h_spectrum or e_step < 1, h_spectrum with n_bins == 0.  KMCF_ERR_STATE: host-only communicator,
 * after these.  KMCF_ERR_ARG at the final synchronisation: an unusable temperature in a thermal mode, message and
 * verdict of kmcf_event_rates; the outputs are unspecified then. */
typedef struct {            /* one per bucket, 40 bytes */
    int64_t n_events;       /* non-null slots of the bucket                                   */
    double  rate_sum;       /* sum of their rates                                             */
    double  rate_max;       /* largest rate (0.0 when the bucket has no candidate)            */
    int     max_i, max_j;   /* its slot's site pair, -1 / -1 when none                        */
    int     n_zero;         /* events of the bucket whose rate is exactly 0.0                 */
    int     reserved;
} kmcf_census_bucket_t;

typedef struct {
    int64_t slots, n_events, n_zero, n_nan;    /* count * nn; non-null slots; rate == 0.0; rate is NaN */
    int64_t n_type[4];  double rate_type[4];   /* per EVENTTYPE 0..3 */
    double  rate_total, dt_mean;               /* dt_mean = 1 / rate_total, +infinity when rate_total == 0 */
    double  rate_max;  int max_i, max_j, max_type;   /* over all buckets; -1 ids when none */
    int     rows_live;                         /* rows with at least one non-null slot */
    float   ms_build, ms_census;               /* device time (HIP events): the build kernel / everything behind it */
} kmcf_census_stats_t;

int kmcf_event_census(kmcf_comm *c, int N, const int *h_count, const int *h_displs, int nn,
                      const int *d_neigh_idx, const int *d_site_layer, double T_bg, double freq,
                      double sigma, double k, const double *d_x, const double *d_y, const double *d_z,
                      const double *d_site_potential_charge, const int *d_site_element,
                      const int *d_site_charge, int num_layers, const double *h_E_gen,
                      const double *h_E_rec, const double *h_E_Vdiff, const double *h_E_Odiff,
                      const double *d_site_temperature, int rate_mode,
                      const int *d_site_cell /* N, or NULL */, int n_cells,
                      kmcf_census_bucket_t *h_table /* (n_cells + 1) * num_layers * 4, required */,
                      int n_bins, int e_lo, int e_step, int64_t *h_spectrum /* 4 * n_bins, or NULL with n_bins == 0 */,
                      double *d_row_rate /* count[rank] doubles, or NULL */, int *d_row_best /* count[rank] ints, or NULL */,
                      kmcf_census_stats_t *stats /* or NULL */);

/* ---------------------------------------------------------------------- */
/* Conductive clusters: the filament as a graph (no reference counterpart)   */
/* ---------------------------------------------------------------------- */
/* Connected components of the sites that conduct, by the reference's own high_G rule (populate_T_dist,
 * src/current_solver_gpu.cu:1227-1241; class 1 / class 2 of the K rule).
 * Members: site i is METAL if site_element[i] is in the metal list, a CONDUCTIVE VACANCY if site_element[i] == VACANCY
 * (2) and site_charge[i] == 0; no other site is a member.
 * Conductive edge (i, j): j appears in row i of the neighbour list OR i appears in row j (rows truncated at nn make
 * lists one-sided), and both sites are metal or both are conductive vacancies (a metal-vacancy pair gets low_G).
 * Cluster: a connected component of the members under conductive edges.  Its label and `root` is its smallest site id;
 * non-members get label -1; a member without a conductive edge is a cluster of size 1.  kind: 1 metal, 2 vacancy.
 * touch: a metal cluster has bit 0 (left) if it holds a site id < N_left_tot, bit 1 (right) if it holds a site id
 * >= N - N_right_tot; a vacancy cluster has a bit if one of its sites shares a neighbour-list entry (either direction)
 * with a metal site whose cluster has that bit.  A vacancy cluster with touch == 3 is a bridging filament.
 * x_min / x_max: over the cluster's sites, from d_x, exact.  Every output is independent of the execution order: two
 * calls on the same input return the same bytes. */
#define KMCF_CLUSTER_METAL   1
#define KMCF_CLUSTER_VACANCY 2
typedef struct { int root, kind, size, touch; double x_min, x_max; } kmcf_cluster_t;   /* 32 bytes */
typedef struct {
    int members, n_clusters, n_metal_clusters, n_vacancy_clusters;
    int n_bridging;             /* vacancy clusters with touch == 3                         */
    int largest_vacancy;        /* size of the largest vacancy cluster (0: none)            */
    int largest_bridging;       /* size of the largest bridging filament (0: none)          */
    int passes;                 /* kernel launches that walk neighbour rows: a constant of the implementation */
    float ms;                   /* device time of everything the call enqueued (HIP events) */
} kmcf_cluster_stats_t;

/* A LOCAL operation on the WHOLE-device list (N rows, -1 padded; an entry >= N or < -1 is ignored as padding): no
 * collectives.  In a rank group every rank that wants the result calls it on its own copy of the whole list;
 * partitioned lists are out of scope.  Nothing is kept between calls but buffers on the communicator (freed by
 * kmcf_comm_destroy); no verdict about the list is cached, so the list and the site arrays may change between calls.
 * Call it after kmcf_update_charge: the classes read the charges.
 * d_site_label: N ints out, may be NULL.  h_clusters: the table sorted by root ascending, may be NULL; when
 * n_clusters > max_clusters the first max_clusters entries are written and stats->n_clusters still reports the true
 * count (query with h_clusters == NULL, then size the buffer).  stats may be NULL.
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL c, list, element, charge or
 * d_x; N <= 0; nn <= 0; num_metals < 0, or num_metals > 0 with NULL d_metals; N_left_tot < 0, N_right_tot < 0 or
 * N_left_tot + N_right_tot > N; max_clusters < 0, or h_clusters set with max_clusters == 0.
 * KMCF_ERR_STATE: host-only communicator. */
int kmcf_conductive_clusters(kmcf_comm *c, int N, int nn, const int *d_neigh_idx /* N*nn, -1 padded */,
                             const int *d_site_element, const int *d_site_charge,
                             const int *d_metals, int num_metals, const double *d_x,
                             int N_left_tot, int N_right_tot,
                             int *d_site_label /* N ints out; may be NULL */,
                             kmcf_cluster_t *h_clusters /* may be NULL */, int max_clusters,
                             kmcf_cluster_stats_t *stats /* may be NULL */);

/* ---------------------------------------------------------------------- */
/* Filament gap: nearest approach of the two electrode sides (no reference   */
/* counterpart)                                                              */
/* ---------------------------------------------------------------------- */
/* In the high-resistance state no filament bridges the device; what then sets the resistance is the tunnelling gap: how
 * close the conductive matter attached to the left electrode comes to the matter attached to the right one.
 * Sets: A = sites with side bit 0, B = sites with side bit 1; a site may be in both.  kmcf_site_set_gap takes the sides
 * as given (d_site_side; bits above 1 are ignored).  kmcf_filament_gap derives them: side[i] = touch of i's cluster,
 * exactly as kmcf_conductive_clusters defines touch, for members -- metal and vacancy clusters alike -- and 0 for
 * non-members.
 * Cell: d_site_cell[i] in [0, n_cells) is the gap cell of site i (for a crossbar: structure.crossbar_lines'
 * cell_of_site); any other value: the site belongs to no cell and enters no pair.  d_site_cell NULL requires
 * n_cells == 1 and puts every site in cell 0.
 * Pair of cell c: (a, b) with a in A, b in B, both in cell c; a == b is allowed.  dx = x[a] - x[b], likewise dy, dz;
 * d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to double (no fused multiply-add); the distance is non-periodic, and
 * these two calls refuse a periodic index (kmcf_compute_cutoff_list_pbc with pbc == 1) with KMCF_ERR_ARG: their pruning by
 * the distances to the cell faces does not carry over to wrapped cells.  kmcf_site_set_gap_pbc / kmcf_filament_gap_pbc
 * (below) take the minimum image on such an index.
 * A pair counts iff d2 <= r_max*r_max, that product formed in double.
 * Result per cell: the pair with the smallest d2; among equal d2 the smallest a, then the smallest b.  A site in both sets
 * gives gap2 = 0 through the pair (a, a).  gap2, the two sites, x_left / x_right and the counts are exact; gap =
 * sqrt(gap2).  Every output is independent of the execution order: two calls on the same input return the same bytes.
 * Profile (kmcf_filament_gap): inv_w = n_bins / (x_hi - x_lo) is computed once on the host; a conductive vacancy
 * (cluster kind 2) of cell c with side s in {1, 2, 3} and t = (x[i] - x_lo) * inv_w, 0 <= t < n_bins, adds 1 to
 * h_profile[(c*n_bins + (int)t)*3 + s-1].  The smallest side-3 count along x is the filament's constriction. */
typedef struct {            /* 56 bytes */
    double gap, gap2;       /* gap = sqrt(gap2); +infinity: no pair within r_max           */
    double x_left, x_right; /* x of site_left / site_right (0.0 when there is no pair)     */
    int site_left, site_right;   /* the pair, -1 when none                                  */
    int n_left, n_right, n_both; /* sites of this cell with side bit 0 / bit 1 / both bits  */
    int bridged;                 /* n_both > 0                                              */
} kmcf_gap_t;
typedef struct {
    int n_left, n_right, n_both;                 /* whole device, cell -1 included */
    int cells_bridged, cells_open, cells_none;   /* n_both > 0 / not bridged, a pair within r_max / not bridged, no pair */
    float ms_clusters, ms_search;                /* device time (HIP events): cluster pass and sides / everything behind */
} kmcf_gap_stats_t;

/* Both are LOCAL operations on WHOLE-device arrays of the index's N sites (kmcf_compute_cutoff_list; the coordinates are
 * the ones it was built from): no collectives, and nothing is kept between calls but scratch buffers on the index (freed
 * by kmcf_pairwise_destroy).  kmcf_poisson_gridless's lists are not touched.  r_max is at most the index's cutoff radius:
 * the 27 index cells around a site then hold every partner.  h_gaps: n_cells records out.  stats may be NULL.
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL coordinates, d_site_side
 * (kmcf_site_set_gap), h_gaps or p; r_max not finite, <= 0, or larger than the index's cutoff radius; n_cells < 1, or
 * NULL d_site_cell with n_cells != 1. */
int kmcf_site_set_gap(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                      const int *d_site_side /* N: bit 0 left set, bit 1 right set */, double r_max,
                      const int *d_site_cell /* N, or NULL */, int n_cells,
                      kmcf_gap_t *h_gaps /* n_cells */, kmcf_gap_stats_t *stats /* or NULL */);

/* The cluster pass of kmcf_conductive_clusters on the communicator of the index (call it after kmcf_update_charge),
 * the sides, then the search.  h_profile: n_cells*n_bins*3 ints out, or NULL (n_bins, x_lo, x_hi are then not used
 * beyond the check n_bins >= 0).  d_site_side: N ints out, or NULL.
 * KMCF_ERR_ARG as above, and: NULL list, element or charge; n_bins < 0; h_profile set with n_bins == 0 or with
 * x_hi <= x_lo; nn <= 0; num_metals < 0, or num_metals > 0 with NULL d_metals; N_left_tot < 0, N_right_tot < 0 or
 * N_left_tot + N_right_tot > N of the index. */
int kmcf_filament_gap(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                      const int *d_site_charge, const int *d_metals, int num_metals,
                      const double *d_x, const double *d_y, const double *d_z,
                      int N_left_tot, int N_right_tot, double r_max,
                      const int *d_site_cell, int n_cells, kmcf_gap_t *h_gaps,
                      int n_bins, double x_lo, double x_hi, int *h_profile /* n_cells*n_bins*3, or NULL */,
                      int *d_site_side /* N out, or NULL */, kmcf_gap_stats_t *stats);

/* The same two analyses under periodic y-z boundaries.  Parameter lists, outputs, argument checks and their order are
 * those of kmcf_site_set_gap / kmcf_filament_gap (kmcf_last_error names the _pbc call); the one difference: a periodic
 * index is accepted.
 * On a non-periodic index (kmcf_compute_cutoff_list, or kmcf_compute_cutoff_list_pbc with pbc == 0) they launch the
 * kernels of the plain calls and return their bytes.
 * On a periodic index (kmcf_compute_cutoff_list_pbc with pbc == 1) the pair distance is the library's one minimum image,
 * Ly and Lz being the periods the index was built with:
 *     dx = x[a] - x[b]
 *     fy = (y[a] - y[b]) / Ly;  fy -= round(fy);  dy = fy * Ly        (z likewise; round = C round, half away from zero)
 *     d2 = (dx*dx + dy*dy) + dz*dz
 * every operation rounded to double: no fused multiply-add, the division an IEEE division (no reciprocal multiply).  x is
 * never periodic.  A pair has ONE distance, the minimum image: where a period is shorter than 2 r_max, a second image
 * within r_max adds no pair.
 * Everything else is the contract above: A and B from the side bits, a == b allowed (gap2 = 0); gap cells from
 * d_site_cell; a pair counts iff d2 <= r_max*r_max; the winner has the smallest d2, then the smallest a, then the
 * smallest b; r_max is at most the index's cutoff radius; the profile along x, the counts and the stats are unchanged
 * (x is not periodic); gap = sqrt(gap2) is formed on the host; one synchronisation per call; two calls on the same input
 * return the same bytes.
 * kmcf_filament_gap_pbc derives the sides from the list it is given: pass the list of kmcf_neighbor_list_pbc (pbc == 1,
 * the same periods) so that the clusters are periodic as well.  This is not checked (as with kmcf_events_set_lattice):
 * an open list under a periodic distance gives open clusters measured across the wrap. */
int kmcf_site_set_gap_pbc(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                          const int *d_site_side /* N: bit 0 left set, bit 1 right set */, double r_max,
                          const int *d_site_cell /* N, or NULL */, int n_cells,
                          kmcf_gap_t *h_gaps /* n_cells */, kmcf_gap_stats_t *stats /* or NULL */);
int kmcf_filament_gap_pbc(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                          const int *d_site_charge, const int *d_metals, int num_metals,
                          const double *d_x, const double *d_y, const double *d_z,
                          int N_left_tot, int N_right_tot, double r_max,
                          const int *d_site_cell, int n_cells, kmcf_gap_t *h_gaps,
                          int n_bins, double x_lo, double x_hi, int *h_profile /* n_cells*n_bins*3, or NULL */,
                          int *d_site_side /* N out, or NULL */, kmcf_gap_stats_t *stats);

/* ---------------------------------------------------------------------- */
/* Tunnelling chain: the stepping-stone path between the electrode sides     */
/* through floating bodies (no reference counterpart)                        */
/* ---------------------------------------------------------------------- */
/* The gap ignores everything attached to neither electrode.  Floating vacancy clusters and metal islands carry the
 * trap-assisted tunnelling current of the high-resistance state: it hops left side, stone, stone, ..., right side, and
 * the longest hop decides it.  Per gap cell these calls report the chain of hops whose longest hop is as short as any
 * chain's.
 * Inputs per site.  side: bit 0 left, bit 1 right, higher bits ignored (as in kmcf_site_set_gap).  node: the id of the
 * floating body the site belongs to; any value outside [0, N) means none.  cell: the gap cell through d_site_cell /
 * n_cells exactly as in the gap calls (NULL requires n_cells == 1; a value outside [0, n_cells): the site is in no cell).
 * Terminals of gap cell c.  L_c = the sites with side bit 0 whose own cell is c, R_c the same with bit 1.  A site with
 * both bits makes the cell BRIDGED.
 * Stones.  A stone site has (side & 3) == 0, a valid node and a valid own cell.  The home of node n is the smallest site
 * id among its stone sites; the whole node belongs to the gap cell of its home, and ALL its stone sites take part in that
 * cell wherever they lie: a floating body is one object and is counted once.  The vertices of cell c are L_c, R_c and the
 * nodes whose home cell is c.
 * Pair distance.  d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to double, no fused multiply-add; non-periodic.  A
 * pair counts iff d2 <= r_max*r_max, that product formed in double.  r_max is at most the index's cutoff radius.
 * Link.  Two different vertices u, v of one cell are linked iff a pair (a in u, b in v) counts; the link's pair is the one
 * with the smallest key (d2, min(a,b), max(a,b)).  Keys of different links differ, so the links are totally ordered.
 * Chain of cell c.  The path between L_c and R_c in the minimum spanning forest of the cell's link graph under that order
 * -- what Kruskal's algorithm produces on the links sorted by key; the keys being unique, the path is unique.  It is the
 * path whose largest hop is as small as any path's.  Hops are reported oriented from L to R as (from, to, d2).
 * direct2 is the d2 of the link L_c - R_c and is bit-equal to gap2 of kmcf_site_set_gap on the same sides.  Where that
 * link ties with another pair of the same d2, the site pair may differ from the gap's: the gap breaks ties by (a, b), this
 * contract by (min, max).
 * Determinism: every output except the times depends on the input alone; two calls on the same input return the same bytes.
 * Cost: the first search round looks at every member's whole neighbourhood within r_max, electrode bulk included; the
 * later rounds run on the surface members only (those with a site of another vertex within r_max).  Measured on the 40 nm
 * crossbar (1.6e6 sites, 2.4e5 members): the search takes 2.1 ms at r_max = 20 next to a cluster pass of
 * 4.7 ms -- round 1 is the larger part of the search but does not dominate the call, which stays within 1.5 cluster passes
 * at every radius up to the cutoff.  An index with a smaller cutoff, built for this call alone (kmcf_compute_cutoff_list
 * with cutoff = r_max = 8, say), makes the search cheaper still: 0.8 ms against 1.4 ms at r_max = 8 on the 20 A index. */
#define KMCF_CHAIN_NONE    0   /* L_c or R_c is empty                                   */
#define KMCF_CHAIN_OPEN    1   /* both non-empty, no path                               */
#define KMCF_CHAIN_CHAINED 2   /* a path exists                                         */
#define KMCF_CHAIN_BRIDGED 3   /* a site with both bits: n_hops = 0, hop_max2 = direct2 = 0 */
typedef struct {            /* 64 bytes */
    double hop_max, hop_max2;    /* largest d2 on the chain (+infinity unless CHAINED or BRIDGED); hop_max = sqrt(hop_max2) */
    double length;               /* sum of sqrt(d2) over the hops, added in chain order on the host; 0.0 without a hop */
    double direct2;              /* d2 of the link L_c - R_c, +infinity if they are not linked     */
    int status, n_hops;          /* KMCF_CHAIN_*; the true number of hops (also beyond max_hops)   */
    int neck_from, neck_to;      /* the hop with the largest key, -1 when there is none            */
    int n_stones, n_stone_sites; /* vertices / sites of the stones assigned to this cell           */
    int n_left, n_right;         /* as in kmcf_gap_t                                               */
} kmcf_chain_t;
typedef struct { int from, to; double d2; } kmcf_hop_t;   /* 16 bytes */
typedef struct {
    int cells_none, cells_open, cells_chained, cells_bridged;
    int n_stones, n_stone_sites;    /* whole device: the stones assigned to a cell                                    */
    int surface_sites;              /* members of the search (sites of the vertices of OPEN / CHAINED cells) that have a
                                       site of another vertex of their cell within r_max                               */
    int rounds, forest_edges;       /* search rounds run; spanning-forest edges found before the search stopped        */
    float ms_clusters, ms_search;   /* device time (HIP events), as in kmcf_gap_stats_t                                */
} kmcf_chain_stats_t;

/* LOCAL operations on WHOLE-device arrays of the index's N sites, as the gap calls; scratch lives on the index (freed by
 * kmcf_pairwise_destroy).  h_chains: n_cells records out.  h_hops[c*max_hops + k] holds hop k of cell c for
 * k < min(n_hops, max_hops); the rest of a cell's slots are {-1, -1, +infinity}; h_hops may be NULL when max_hops == 0.
 * stats may be NULL.  One synchronisation per search round (a flag read) and one at the end.
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL coordinates, d_site_side,
 * d_site_node, h_chains or p; r_max not finite, <= 0, or larger than the index's cutoff radius; n_cells < 1, or NULL
 * d_site_cell with n_cells != 1; max_hops < 0, h_hops set with max_hops == 0 or NULL with max_hops > 0; a periodic index
 * (kmcf_site_set_chain_pbc / kmcf_filament_chain_pbc below take it; the message names that call).  KMCF_ERR_STATE: the
 * search did not stop within 40 rounds. */
int kmcf_site_set_chain(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                        const int *d_site_side /* N */, const int *d_site_node /* N */, double r_max,
                        const int *d_site_cell /* N, or NULL */, int n_cells,
                        kmcf_chain_t *h_chains /* n_cells */, kmcf_hop_t *h_hops /* n_cells*max_hops, or NULL */,
                        int max_hops, kmcf_chain_stats_t *stats /* or NULL */);

/* The cluster pass of kmcf_conductive_clusters (as kmcf_filament_gap runs it), then: side[i] = touch of i's cluster for
 * members and 0 for non-members; node[i] = the cluster label of i for the members of clusters with touch 0, metal and
 * vacancy clusters alike, and -1 for every other site; then the search above.  d_site_side, d_site_node: N ints out, or
 * NULL.  KMCF_ERR_ARG as above, and the list / metals / contact-count checks of kmcf_filament_gap. */
int kmcf_filament_chain(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                        const int *d_site_charge, const int *d_metals, int num_metals,
                        const double *d_x, const double *d_y, const double *d_z,
                        int N_left_tot, int N_right_tot, double r_max,
                        const int *d_site_cell, int n_cells, kmcf_chain_t *h_chains,
                        kmcf_hop_t *h_hops /* n_cells*max_hops, or NULL */, int max_hops,
                        int *d_site_side /* N out, or NULL */, int *d_site_node /* N out, or NULL */,
                        kmcf_chain_stats_t *stats);

/* The same two analyses under periodic y-z boundaries.  Parameter lists, outputs, argument checks and their order are
 * those of kmcf_site_set_chain / kmcf_filament_chain (kmcf_last_error names the _pbc call); the one difference: a
 * periodic index is accepted.
 * On a non-periodic index (kmcf_compute_cutoff_list, or kmcf_compute_cutoff_list_pbc with pbc == 0) they launch the
 * kernels of the plain calls and return their bytes.
 * On a periodic index (kmcf_compute_cutoff_list_pbc with pbc == 1) the pair distance is the library's one minimum image,
 * as in kmcf_site_set_gap_pbc, Ly and Lz being the periods the index was built with:
 *     dx = x[a] - x[b]
 *     fy = (y[a] - y[b]) / Ly;  fy -= round(fy);  dy = fy * Ly        (z likewise; round = C round, half away from zero)
 *     d2 = (dx*dx + dy*dy) + dz*dz
 * every operation rounded to double: no fused multiply-add, the division an IEEE division.  x is never periodic.
 * Symmetry.  d2(a, b) and d2(b, a) are the same bits: division, round, subtraction and product are odd in the difference,
 * and the squares remove the sign.  The two ends of a link therefore see one key, which the search relies on.
 * One distance per pair.  Where a period is shorter than 2 r_max, a second image within r_max adds no pair, no link and
 * no surface mark of its own: surface_sites counts sites.
 * A vertex near its own image links to nothing: pairs inside one vertex are never links, through a face or not.
 * Everything else is the contract above, unchanged: terminals, stones, homes, vertex cells; a pair counts iff
 * d2 <= r_max*r_max; the link key (d2, min(a,b), max(a,b)); the chain as the L - R path of the minimum spanning forest;
 * statuses, records, the orientation of the hops, length as the host's sum of sqrt(d2) in chain order; the stats; r_max is
 * at most the index's cutoff radius; two calls on the same input return the same bytes.
 * direct2 is bit-equal to gap2 of kmcf_site_set_gap_pbc on the same sides and index.
 * kmcf_filament_chain_pbc derives sides and nodes from the list it is given: pass the list of kmcf_neighbor_list_pbc
 * (pbc == 1, the same periods) so that a floating body that passes through a face is ONE node, and a stump of the filament
 * beyond a face belongs to its electrode.  This is not checked (as with kmcf_filament_gap_pbc): an open list under a
 * periodic distance gives open clusters -- bodies cut in two at the faces -- measured across the wrap.
 * Cost on the periodic 5 nm cell: DESIGN 3.12, "Periodic search". */
int kmcf_site_set_chain_pbc(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                            const int *d_site_side /* N */, const int *d_site_node /* N */, double r_max,
                            const int *d_site_cell /* N, or NULL */, int n_cells,
                            kmcf_chain_t *h_chains /* n_cells */, kmcf_hop_t *h_hops /* n_cells*max_hops, or NULL */,
                            int max_hops, kmcf_chain_stats_t *stats /* or NULL */);
int kmcf_filament_chain_pbc(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                            const int *d_site_charge, const int *d_metals, int num_metals,
                            const double *d_x, const double *d_y, const double *d_z,
                            int N_left_tot, int N_right_tot, double r_max,
                            const int *d_site_cell, int n_cells, kmcf_chain_t *h_chains,
                            kmcf_hop_t *h_hops /* n_cells*max_hops, or NULL */, int max_hops,
                            int *d_site_side /* N out, or NULL */, int *d_site_node /* N out, or NULL */,
                            kmcf_chain_stats_t *stats);

/* ---------------------------------------------------------------------- */
/* Site gradient map: the local gradient of a site field (the potential the events read, the band edge, the site
 * temperature) and the largest bond drop per site, with their maxima per cell and for the device.  The reference has no
 * counterpart.
 * IN: site i is in when d_site_mask is NULL or d_site_mask[i] != 0.
 * COUNTED PAIRS of an in site i: the slots s = 0 ... nn-1 of row i of d_neigh_idx, in slot order, whose entry j meets all
 * of: 0 <= j < N (anything else is padding, as for kmcf_conductive_clusters); j != i; j is in; |d_ij| > 0 (coincident
 * sites -- the 5 nm example holds one such pair -- contribute nothing).  ONLY ROW i IS READ: a truncated, one-sided list
 * gives one-sided pairs; an entry that occurs twice in the row counts twice.
 * Displacement d_ij from i to j: open (pbc == 0) the plain difference (x_j - x_i, y_j - y_i, z_j - z_i); pbc == 1: x the
 * plain difference, y and z the library's one minimum image, f = (y_j - y_i) / Ly, f -= round(f), dy = f * Ly (the C round;
 * Ly = h_lattice[1], Lz = h_lattice[2]).  |d| = sqrt((dx dx + dy dy) + dz dz); u = d / |d| per component;
 * q_ij = (value[j] - value[i]) / |d|.  Every operation is rounded on its own (no contraction).
 * Gradient: M = sum u u^T (3 x 3 symmetric), b = sum u q, n_i = number of counted pairs.  The site is FULL iff n_i >= 3
 * and det(M) >= 1e-9 * (n_i / 3)^3 (the trace of M is n_i, so det(M) / (n_i / 3)^3 lies in [0, 1]; a plane or a line of
 * neighbours gives 0 up to rounding).  A full site gets g = M^-1 b -- the least-squares gradient of the pairs with weights
 * 1 / |d|^2 -- as the closed-form symmetric inverse: the cofactors c00 = m11 m22 - m12 m12, c01 = m02 m12 - m01 m22,
 * c02 = m01 m12 - m02 m11, c11 = m00 m22 - m02 m02, c12 = m01 m02 - m00 m12, c22 = m00 m11 - m01 m01,
 * det = (m00 c00 + m01 c01) + m02 c02, g_x = ((c00 b0 + c01 b1) + c02 b2) / det and g_y, g_z alike.  A site that is not
 * full gets g = 0 and full = 0.  |g| = sqrt((gx gx + gy gy) + gz gz).
 * Drop: drop[i] = max over the counted pairs of |q_ij|, drop_to[i] = the j of the FIRST slot that attains it (a |q| that
 * is not a number attains nothing); a site without such a pair gets 0 and -1.
 * Sites that are not in get 0 / 0 / 0 / 0 / -1 / 0 in whichever of gx, gy, gz, drop, drop_to, full are given.
 * Order of addition (fixed by the input): 16 lanes work on a site; lane l adds the terms of its slots l, l + 16, l + 32, ...
 * in ascending order, starting from zero, and keeps its largest |q| (first slot among equals); then four butterfly steps
 * t = 8, 4, 2, 1 in which every lane replaces each of its sums s by s + (the sum lane l xor t holds), and its largest |q|
 * by the other lane's if that is larger, or equal with the lower slot.  Lane 0 solves.
 * Cells: d_site_cell == NULL requires n_cells == 1 and puts every site in cell 0 (kmcf_site_set_gap's convention).  A site
 * whose cell is outside [0, n_cells) gets its outputs and enters the whole-device statistics, but no cell record.
 * Maxima (per cell in h_cells, over all in sites in stats): a value that is not finite enters no maximum; a site without
 * a counted pair is no candidate for the largest drop; g_max / drop_max are the bits of a per-site output (a selection,
 * not a sum); among equal |g| the smallest site id is g_site, among equal drops the smallest drop_from wins (drop_to is
 * that site's drop_to); without a candidate the value is 0 and the ids are -1.
 * n_degenerate: the in sites with n_i >= 3 that fail the determinant test; pairs: sum of n_i over the in sites.
 * Two calls on the same input return the same bytes: no atomics on doubles, every sum in the order above; maxima, ties and
 * counts are integer atomics.  pbc == 0: h_lattice is ignored, the bytes are the same whether it is NULL or set.
 * Scope: a local operation on the whole-device list, like kmcf_conductive_clusters: no collectives; in a rank group every
 * rank that wants the result calls it.  Scratch lives on the communicator.  The call synchronises once, at its end; ms
 * is the device time of everything it enqueued (HIP events).
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL c, d_neigh_idx, d_x, d_y, d_z or
 * d_value; N <= 0 or nn <= 0; pbc outside 0 / 1; with pbc == 1 a NULL h_lattice or a y or z period that is not finite or
 * <= 0; n_cells outside 1 ... 1024; NULL d_site_cell with n_cells != 1; only some of d_gx / d_gy / d_gz set; no output
 * requested at all.  KMCF_ERR_STATE: host-only communicator. */
/* ---------------------------------------------------------------------- */
typedef struct {            /* one per cell, 40 bytes */
    int n_sites, n_full;    /* in sites of the cell; those with a full-rank gradient */
    double g_max;  int g_site;               /* largest |g|; smallest site id among equals; -1 if none */
    double drop_max; int drop_from, drop_to; /* largest drop; smallest drop_from among equals; -1/-1 if none */
} kmcf_gradient_cell_t;
typedef struct {
    int n_sites, n_full, n_degenerate;  int64_t pairs;   /* counted pairs, all in sites */
    double g_max; int g_site; double drop_max; int drop_from, drop_to;   /* over all in sites */
    float ms;
} kmcf_gradient_stats_t;

int kmcf_site_gradient(kmcf_comm *c, int N, int nn, const int *d_neigh_idx /* N*nn */,
                       const double *d_x, const double *d_y, const double *d_z,
                       const double *h_lattice /* 3, host; may be NULL with pbc == 0 */, int pbc,
                       const double *d_value /* N */, const int *d_site_mask /* N or NULL */,
                       const int *d_site_cell /* N or NULL */, int n_cells,
                       double *d_gx, double *d_gy, double *d_gz /* N each; all three or none */,
                       double *d_site_drop /* N or NULL */, int *d_site_drop_to /* N or NULL */,
                       int *d_site_full /* N or NULL */,
                       kmcf_gradient_cell_t *h_cells /* n_cells, or NULL */,
                       kmcf_gradient_stats_t *stats /* or NULL */);

/* ---------------------------------------------------------------------- */
/* Pair correlation: pair-distance histograms per class pair and cell, and    */
/* counts of class members around every site (no reference counterpart)       */
/* ---------------------------------------------------------------------- */
/* How the defects are arranged: the vacancy-vacancy pair distribution (clustering, against a random arrangement), the
 * ion-vacancy separation (recombination), the number of defects within a radius of every site (a density map).
 * Classes: d_site_class[i] in [0, n_classes): site i is a MEMBER of that class.  d_site_class[i] == n_classes
 * (KMCF_PC_PROBE relative to the call): site i is a PROBE -- a centre of the site counts only, never a partner, never in
 * the histogram.  Any other value: the site takes no part.  1 <= n_classes <= KMCF_PC_MAX_CLASSES.
 * Distance: the index's own.  On a non-periodic index (kmcf_compute_cutoff_list, or kmcf_compute_cutoff_list_pbc with
 * pbc == 0), for the sites i and j
 *     dx = x[i] - x[j], likewise dy, dz;  d2 = (dx*dx + dy*dy) + dz*dz
 * and on an index of kmcf_compute_cutoff_list_pbc with pbc == 1 the library's minimum image, Ly and Lz the index's periods:
 *     dx = x[i] - x[j]
 *     fy = (y[i] - y[j]) / Ly;  fy -= round(fy);  dy = fy * Ly        (z likewise; round = C round, half away from zero)
 *     d2 = (dx*dx + dy*dy) + dz*dz
 * every operation rounded to double (no fused multiply-add, an IEEE division), as above kmcf_site_set_gap_pbc.  Both are
 * even in the difference: d2 of (i, j) and of (j, i) are the same bits.  A pair has ONE distance, whatever number of its
 * images lie within reach.  One call serves both kinds of index.
 * Pair: an unordered {i, j}, i != j, both members, d2 <= r_max*r_max, that product formed in double.  It is counted once.
 * Two different sites with equal coordinates are a pair with d2 = 0.
 * Bins: e[k] = r_max * (double)k / (double)n_bins for k = 0 .. n_bins (multiply, then divide, each rounded to double),
 * edge2[k] = e[k] * e[k], and edge2[n_bins] = r_max * r_max; formed on the host and returned in h_edge2.  A pair falls
 * into bin k, the largest k < n_bins with edge2[k] <= d2: the TABLE defines the bin, not an expression in sqrt(d2).
 * 1 <= n_bins <= KMCF_PC_MAX_BINS.
 * Class pair of the classes p <= q: index p * n_classes - p * (p - 1) / 2 + (q - p); n_pairs = n_classes * (n_classes + 1) / 2.
 * Bucket: from d_site_cell as in kmcf_site_set_gap (a value outside [0, n_cells): no valid cell; NULL requires
 * n_cells == 1 and puts every site in cell 0).  Both sites in the same cell c: bucket c.  Both in valid, different
 * cells: the rest bucket n_cells.  Either site without a valid cell: the pair enters no bucket.
 * Outputs:
 *   h_hist[(bucket * n_pairs + pair) * n_bins + k]   counts, n_cells + 1 buckets
 *   h_members[bucket * n_classes + p]                members of class p per cell; bucket n_cells: those without a valid cell
 *   d_site_count[i * n_classes + q]                  device, N * n_classes ints, or NULL: for every centre i (member or
 *       probe) the members j != i of class q with d2 <= r_count*r_count, whatever their cells; the row of every other
 *       site is written as zeros.  0 < r_count <= r_max.
 *   stats    n_pairs_total: the sum of h_hist; n_members, n_probes; max_count: the largest sum of a centre's count row,
 *       max_count_site: the smallest site id that attains it (-1 and 0 without a centre) -- formed with or without
 *       d_site_count; ms: device time of everything the call enqueued (HIP events).
 * Every output is a pure function of the input (integer accumulation only): two calls return the same bytes.
 * Both calls are LOCAL operations on WHOLE-device arrays of the index's N sites, like kmcf_site_set_gap: no collectives,
 * scratch on the index (freed by kmcf_pairwise_destroy), kmcf_poisson_gridless's lists and the gap and chain scratch
 * untouched, one synchronisation per call.
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL coordinates, classes, h_hist,
 * h_members or p; n_classes or n_bins out of range; r_max not finite, <= 0 or above the index's cutoff radius; r_count not
 * finite, <= 0 or > r_max; n_cells < 1, or NULL d_site_cell with n_cells != 1; (n_cells + 1) * n_pairs * n_bins > 2^24. */
#define KMCF_PC_MAX_CLASSES 4
#define KMCF_PC_MAX_BINS 256
typedef struct {
    unsigned long long n_pairs_total;
    int n_members, n_probes;
    int max_count, max_count_site;
    float ms;
} kmcf_pair_stats_t;

int kmcf_pair_correlation(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                          const int *d_site_class /* N */, int n_classes, double r_max, int n_bins, double r_count,
                          const int *d_site_cell /* N, or NULL */, int n_cells,
                          unsigned long long *h_hist /* (n_cells + 1) * n_pairs * n_bins */,
                          int *h_members /* (n_cells + 1) * n_classes */, double *h_edge2 /* n_bins + 1, or NULL */,
                          int *d_site_count /* N * n_classes, or NULL */, kmcf_pair_stats_t *stats /* or NULL */);

/* kmcf_pair_correlation with n_classes = 3 and the classes taken from the device state: class 0 VACANCY (element 2)
 * with charge 0, class 1 VACANCY with charge != 0, class 2 OXYGEN_DEFECT (element 1); every other site a probe when
 * probe_all != 0, otherwise no part.  d_site_class: N ints out (the classes as formed), or NULL.
 * KMCF_ERR_ARG as above, and NULL d_site_element or d_site_charge. */
int kmcf_defect_correlation(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                            const int *d_site_element, const int *d_site_charge, int probe_all,
                            double r_max, int n_bins, double r_count, const int *d_site_cell /* N, or NULL */, int n_cells,
                            unsigned long long *h_hist, int *h_members, double *h_edge2 /* n_bins + 1, or NULL */,
                            int *d_site_count /* N * 3, or NULL */, int *d_site_class /* N out, or NULL */,
                            kmcf_pair_stats_t *stats /* or NULL */);

/* ---------------------------------------------------------------------- */
/* Field sampling: site fields on sample points and regular grids             */
/* (no reference counterpart)                                                  */
/* ---------------------------------------------------------------------- */
/* The value of site quantities at points that are not sites: a potential cut, a temperature map, a vacancy density per
 * voxel, the material of a voxel.  Every point s gathers the MEMBERS within `radius` through the index's cell walk.
 * Members: site j is a member when d_site_mask is NULL or d_site_mask[j] != 0.
 * Distance: the index's own, the arithmetic stated above kmcf_pair_correlation with the point in the place of site i --
 * the plain difference on an open index, the minimum image in y and z on an index of kmcf_compute_cutoff_list_pbc with
 * pbc == 1 -- formed from the point's coordinates AS GIVEN.  Member j is within reach when d2 <= r2 = radius * radius,
 * that product formed in double.
 * Weight: u = d2 / r2;  t = 1.0 - u;  w = t * t  (an IEEE division, no fused multiply-add, no sqrt, no table): 1 on the
 * member, 0 on the rim.
 * Per point s:
 *   d_count[s]       members within reach.
 *   d_nearest[s]     the member within reach with the smallest (bits of d2, site id), -1 with none; d2 >= 0, so the bit
 *                    order is the value order, and a tie in d2 goes to the smaller id.
 *   d_nearest_d2[s]  its d2, +infinity with none.
 *   d_wsum[s]        the sum of w.
 *   d_out[f * n_points + s]   acc_f = the sum of w * v_f[j], v_f = d_values + f * N  (normalize == 0), or acc_f / wsum,
 *                    and `fill` where wsum == 0.0 -- no member within reach, or members on the rim only (normalize == 1: the
 *                    mean of an intensive field).  A number density is the raw sum of a 0 / 1 field times
 *                    105 / (32 pi radius^3), the inverse of the weight's volume integral.
 * Values are not checked: a NaN or an infinity in v_f[j] enters, by the IEEE rules (0 * NaN = NaN on the rim), the
 * points member j is within reach of, in field f, and nothing else.  `fill` may be anything, a NaN included.
 * Order of addition (wsum and every acc_f; fixed by the input alone, no atomics on doubles).  The members are laid out in
 * the order of the index's cells, ascending site id inside a cell.  A point walks the index cell columns (ax, ay) around
 * its own cell -- ax ascending, then ay in the walk's order: ascending on an open index, (cy - 1, cy, cy + 1) mod ncy on a
 * periodic one -- and in a column the one or two contiguous runs of members in ascending cell order; the candidates of a
 * point are numbered 0, 1, ... along that walk.  Sixteen partial sums start at 0.0; candidate number q of a RUN (q counted
 * from the run's start) that is within reach is added to partial q % 16, in walk order; candidates out of reach add
 * nothing.  The partials are then combined by a butterfly: for off = 8, 4, 2, 1 every partial l becomes
 * partial[l] + partial[l ^ off]; the result is partial 0.  Two calls return the same bytes; a NULL mask and a mask of all
 * ones return the same bytes.
 * A point need not lie inside the sites' bounding box: the cell rule clamps it into a boundary cell, which only widens
 * the candidate set.  On a periodic index the sites all lie inside one period [y0, y0 + Ly) by construction of the index;
 * a point is wrapped into that period -- y - floor((y - y0) / Ly) * Ly -- ONLY to find its cell and the walk's bounds, and a
 * wrapped value that rounds onto or past a face is clamped like a site there.  The wrap never enters d2.
 * kmcf_field_grid samples the points (ox + i*hx, oy + j*hy, oz + k*hz), each coordinate one multiplication and one
 * addition rounded to double, point index (i*ny + j)*nz + k (z fastest), and returns the bytes of kmcf_field_sample on
 * those points.
 * stats: n_points; n_empty: points with count 0; n_visits: the sum of count; n_members: sites that passed the mask;
 * max_count, max_count_point: the largest count and the smallest point index that attains it (0 and -1 with no point);
 * ms: device time of everything the call enqueued (HIP events).
 * 0 < radius <= the index's cutoff radius (the reach of the 27-cell walk).  n_points == 0: KMCF_OK, nothing is written,
 * the stats are zero.  Both calls are LOCAL operations on WHOLE-device arrays of the index's N sites, like
 * kmcf_site_set_gap: no collectives, scratch on the index (freed by kmcf_pairwise_destroy; it holds nothing a later call
 * reads), the scratch of the other analyses untouched, one synchronisation per call.
 * KMCF_ERR_ARG before anything needs a device (kmcf_last_error names the argument and the call; p is checked last): NULL
 * d_x, d_y or d_z; n_fields outside 0 .. KMCF_FS_MAX_FIELDS; d_values or d_out NULL with n_fields > 0 (an array of no
 * element, d_out with n_points == 0, may be NULL) or non-NULL with n_fields == 0; n_points < 0; NULL d_px, d_py or d_pz
 * with n_points > 0; for the grid a NULL h_origin, h_spacing or h_dims, a spacing that is not finite or <= 0, a dim < 1, a
 * product of the dims >= 2^31, an origin that is not finite; radius not finite, <= 0 or above the index's cutoff radius;
 * normalize neither 0 nor 1; every output and stats NULL; p NULL.
 * KMCF_ERR_ARG at the call's synchronisation, the message naming the first such point: a point coordinate that is not
 * finite; on a periodic index a point further than 1000 periods from the index's origin in y or z (the factor keeps the
 * rounding of the wrap near 2e-13 of a period, far inside the margin of the walk's bounds).  The outputs are then
 * unspecified. */
#define KMCF_FS_MAX_FIELDS 8
typedef struct {
    long long n_points, n_empty, n_visits;
    int n_members;
    int max_count, max_count_point;
    float ms;
} kmcf_sample_stats_t;

int kmcf_field_sample(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                      const int *d_site_mask /* N or NULL */,
                      int n_fields, const double *d_values /* n_fields * N, field-major; NULL iff n_fields == 0 */,
                      int n_points, const double *d_px, const double *d_py, const double *d_pz,
                      double radius, int normalize, double fill,
                      double *d_out /* n_fields * n_points, field-major; NULL iff n_fields == 0 */,
                      double *d_wsum /* n_points or NULL */, int *d_count /* n_points or NULL */,
                      int *d_nearest /* n_points or NULL */, double *d_nearest_d2 /* n_points or NULL */,
                      kmcf_sample_stats_t *stats /* or NULL */);

int kmcf_field_grid(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                    const int *d_site_mask /* N or NULL */, int n_fields, const double *d_values,
                    const double *h_origin /* 3 */, const double *h_spacing /* 3, > 0 */, const int *h_dims /* 3, >= 1 */,
                    double radius, int normalize, double fill,
                    double *d_out /* n_fields * nx*ny*nz */, double *d_wsum, int *d_count, int *d_nearest,
                    double *d_nearest_d2, kmcf_sample_stats_t *stats /* or NULL */);

/* ---------------------------------------------------------------------- */
/* T path: current solve (Kirchhoff matrix with two virtual nodes + WKB       */
/* tunnelling sub-block), SURVEY 8 rows a14 / f3.  PARITY UNPINNED: no         */
/* reference fixture exercises it (src/KMC_comm.h:243 disables it from main).  */
/* ---------------------------------------------------------------------- */
typedef struct kmcf_tstate kmcf_tstate; /* gpubuf.T_distributed + T_p_distributed + the atom_* arrays */

/* initialize_sparsity_T (src/initialize_sparsity_T.cu:948-1154), called once per bias point
 * (src/kmc_main.cpp:273): filters the sites into atoms (element != DEFECT, OXYGEN_DEFECT;
 * update_atom_arrays, src/current_solver_gpu.cu:1341-1365 -- the set is invariant under KMC
 * events, which only turn O <-> V and d <-> Od) and builds the pattern of the neighbour matrix
 * over Nsub = N_atom + 1 nodes (0 = extraction, 1 = injection, 2.. = atoms, the last atom --
 * the ground node -- cut) for the rows [displs[rank], +counts[rank]) of counts_T / displs_T
 * (kmc_comm.counts_T).  Cell list instead of the O(n_loc * Nsub) scans; the distance of THIS call is
 * the non-periodic one the reference's T kernels use whatever pbc says (src/gpu_solvers.h:280-285);
 * kmcf_initialize_sparsity_T_pbc (below) builds the state under periodic y-z boundaries. */
int kmcf_initialize_sparsity_T(kmcf_comm *c, const double *d_site_x, const double *d_site_y,
                               const double *d_site_z, const int *d_site_element, int N, double nn_dist,
                               int num_source_inj, int num_ground_ext, int num_layers_contact,
                               const int *h_counts_T, const int *h_displs_T, kmcf_tstate **out);

/* The same state under periodic boundaries in y and z.  pbc == 0 (h_lattice may be NULL): kmcf_initialize_sparsity_T --
 * the same launches, and a state whose every later output is the same bytes.  pbc == 1: the periods Ly = h_lattice[1],
 * Lz = h_lattice[2] are copied into the state, and every distance the state forms from then on is the library's ONE
 * minimum image (the text above kmcf_compute_cutoff_list_pbc: x never periodic, the C round, only the nearest image --
 * where a period is shorter than 2 nn_dist a second image adds nothing):
 *   - the neighbour pattern (d < nn_dist): bonds through the y and z faces.  The wrapped cell grid of
 *     kmcf_initialize_sparsity_K where at least 3 cells of nn_dist fit each period and the atoms do not span one; else
 *     every pair is tested;
 *   - the ground flag: the atoms within nn_dist of the last atom THROUGH a face carry +high_G on their diagonal too;
 *   - the tunnel block of every later kmcf_t_assemble / kmcf_update_power_sparse: the pair rule d > nn_dist and the
 *     distance inside the WKB value, in all three storage forms; and the fresh evaluation of kmcf_current_map.
 * d(i, j) and d(j, i) are the same bits (division, round, subtraction and product are odd in the difference, the squares
 * remove the sign), so the block stays exactly symmetric and its storage forms hold the same values.  Everything that
 * reads stored values -- the split SpMV, I_macro, the dissipated power -- is periodic through what was stored; the
 * exports below report the periodic system.  A rank group deals and gathers as before.  The tunnel diagonal of a
 * periodic state is one sum per row of the pair bitmap in every storage form: diagonal and preconditioner are the same
 * bytes as bitmap, tiles or jagged tiles, on one rank or dealt over a group (the open state's tile sums depend on the deal).
 * KMCF_ERR_ARG, kmcf_last_error naming the axis, before anything needs a device: pbc outside 0 / 1; with pbc == 1 a NULL
 * h_lattice or a period that is not finite or <= 0.  Otherwise the errors of kmcf_initialize_sparsity_T. */
int kmcf_initialize_sparsity_T_pbc(kmcf_comm *c, const double *d_site_x, const double *d_site_y, const double *d_site_z,
                                   const int *d_site_element, int N, const double *h_lattice /* 3, host */, int pbc,
                                   double nn_dist, int num_source_inj, int num_ground_ext, int num_layers_contact,
                                   const int *h_counts_T, const int *h_displs_T, kmcf_tstate **out);
/* Inspection: *pbc and (h_lattice may be NULL) the three lattice values the state was built with (zeros if none). */
int kmcf_tstate_periodic(const kmcf_tstate *t, int *pbc, double *h_lattice /* 3, may be NULL */);
int kmcf_tstate_destroy(kmcf_tstate *t);
kmcf_matrix *kmcf_tstate_matrix(kmcf_tstate *t);   /* gpubuf.T_distributed (neighbour part) */

typedef struct {
    int N_atom;             /* gpubuf.N_atom_                                        */
    int Nsub;               /* matrix size = N_atom + 1                              */
    int rows_this_rank;
    int64_t nnz_neighbour;  /* this rank                                             */
    int tunnel_points;      /* all ranks (num_tunnel_points_global)                  */
    int tunnel_points_rank; /* counts_subblock[rank]                                 */
    int tunnel_first;       /* displ_subblock[rank]                                  */
    int64_t nnz_tunnel;     /* this rank's rows of the tunnel sub-block              */
    int tunnel_dense;       /* 1: stored as dense symmetric 64 x 64 tiles (one rank, block more than a quarter full), 0: bitmap + packed values */
    int64_t tunnel_bytes;   /* bytes one application of the sub-block streams in that storage */
} kmcf_tstate_info_t;
int kmcf_tstate_info(const kmcf_tstate *t, kmcf_tstate_info_t *info);
/* Exports for tests / inspection.  Pattern: rows of this rank, GLOBAL columns ascending (pass
 * h_col = NULL to query *nnz).  atom_site: site index of every atom (N_atom ints). */
int kmcf_tstate_pattern(const kmcf_tstate *t, int *h_row_ptr, int *h_col, int64_t *nnz);
int kmcf_tstate_atom_sites(const kmcf_tstate *t, int *h_atom_site);
/* After kmcf_t_assemble: per-row vectors of this rank (caller row order; NULL to skip):
 * diagonal of the neighbour part, 1/diagonal of the whole operator (the preconditioner), rhs. */
int kmcf_tstate_get_vectors(const kmcf_tstate *t, double *h_diag_neighbour, double *h_dinv, double *h_rhs);
/* After kmcf_t_assemble: the tunnel sub-block of this rank as CSR (columns = global tunnel
 * point ids, ascending; sizes from kmcf_tstate_info): h_tunnel_idx (all tunnel_points atom
 * indices), h_row_ptr (tunnel_points_rank + 1), h_col / h_val (nnz_tunnel), h_diag
 * (tunnel_points_rank).  Any pointer may be NULL. */
int kmcf_tstate_get_tunnel(const kmcf_tstate *t, int *h_tunnel_idx, int *h_row_ptr, int *h_col, double *h_val,
                           double *h_diag);

typedef struct {
    double Vd;
    double high_G, low_G, loop_G;  /* src/kmc_main.cpp:294-296: 1e5*p.high_G, p.low_G, 1e7*p.high_G */
    double G0;                     /* :298                                                        */
    double tol;                    /* [J] barrier-slope tolerance, p.q * 0.01 (:299)              */
    double m_e, V0;                /* effective mass [kg], defect state energy [eV]               */
    double alpha_disp;             /* fraction of the power dissipated as heat (:302)            */
    double contact_x_lo, contact_x_hi;  /* Ti / N atoms with x in this window are tunnel points; the
                                      reference hard-codes -4.2 and 52.65 (initialize_sparsity_T.cu:645) */
    double cg_tolerance;           /* the reference passes 1e-30 * N_atom (current_solver_gpu.cu:1455),
                                      i.e. "run max_iterations"; its commented value is 1e-15 * N_atom */
    int cg_max_iterations;         /* 100 there (:1456)                                           */
    int solve_heating;             /* solve_heating_local || solve_heating_global                */
} kmcf_current_params_t;

/* Assembly half of update_power_gpu_sparse_dist (src/current_solver_gpu.cu:1496-1632): atom
 * arrays, neighbour values + diagonal (populate_T_dist :1051-1247, calc_diagonal_T /
 * insert_diag_T :1279-1321), tunnel sub-block pattern + WKB values + diagonal
 * (assemble_sparse_T_submatrix, src/initialize_sparsity_T.cu:707-946), preconditioner
 * (:1323-1338) and right-hand side (:1627-1632).  d_site_CB_edge: update_CB_edge's output [J]. */
int kmcf_t_assemble(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge,
                    const double *d_site_CB_edge, const int *d_metals, int num_metals,
                    const kmcf_current_params_t *p);

/* update_power_gpu_sparse_dist (src/current_solver_gpu.cu:1430-1855; gpu_solvers.h:212):
 * assembly, conjugate_gradient_jacobi_split_sparse (dist_iterative/
 * dist_conjugate_gradient_split_sparse.cpp:18-182) started from d_atom_virtual_potentials
 * (N_atom + 2 doubles, gpubuf.atom_virtual_potentials) and solved in place, then -- what the
 * reference has behind its benchmark exit(1), restated from update_power_gpu_sparse
 * (:2035-2160) -- the potentials are gathered on every rank and scaled by G0 in place,
 * *imacro = injected current (get_imacro_sparse :501-542), and with solve_heating the
 * potentials are shifted by |min| in place and d_site_power (N doubles) receives
 * -alpha * P of every non-metal atom (semantics of the dense kernels set_ineg / copy_pdisp,
 * :2353-2379, :462-474; DESIGN.md records why set_ineg_sparse is not followed). */
int kmcf_update_power_sparse(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge,
                             const double *d_site_CB_edge, const int *d_metals, int num_metals,
                             double *d_atom_virtual_potentials, double *d_site_power,
                             const kmcf_current_params_t *p, double *imacro, kmcf_solve_stats_t *stats);

/* Site-resolved current map: where the current of a solved potential field flows.
 * Nodes are those of the T matrix (0 extraction, 1 injection, a + 2 for atom a); m =
 * d_atom_virtual_potentials (N_atom + 2 doubles, as kmcf_update_power_sparse leaves them; only
 * differences of m enter, so the |min| shift made with solve_heating drops out).  A PAIR is a
 * stored off-diagonal of this rank's rows: an entry (r, c), c != r, of the neighbour matrix, or
 * a set bit (i, j), j != i, of the tunnel pair bitmap; the virtual-virtual pair (0,1)/(1,0) is
 * the loop_G driver term, no device current, and is left out.  With g = -A_rc >= 0 the current
 * from r to c is I_rc = g (m[r] - m[c]), and per node r
 *     through[r] = 1/2 sum_c |I_rc|        what flows through the node
 *     tunnel[r]  = the same over tunnel pairs only
 *     net[r]     = sum_c I_rc              Kirchhoff residual; positive: the node emits.
 * The diagonal start values are no pairs: +high_G in row 0 and in the rows of atoms within
 * nn_dist of the last atom (the cut ground node).  net is therefore EXPECTED to be non-zero at
 * nodes 0 and 1 and at those atoms; everywhere else it measures how far the solve is from
 * conserving current (100 CG iterations need not get there).
 * Site outputs: N doubles each, zero-filled, then out[atom_site[a]] = value[a + 2] for every
 * atom with a row, metal atoms included; the last atom has no row and keeps 0.
 * The tunnel conductances are evaluated afresh from the pair bitmap every assembly builds,
 * whatever storage the solve chose for the block (bitmap, dense, jagged or spread tiles): the
 * call reads the state as the last kmcf_t_assemble / kmcf_update_power_sparse left it, changes
 * scratch buffers only and never touches site_power, the matrix or a tunnel storage.  Two calls
 * on the same input return the same bytes (no atomics; every sum is added in an order the
 * input fixes).  On a rank group every rank calls it: each forms the sums of its own rows, the
 * per-node sums are all-gathered by the row partition, every rank returns the complete site
 * arrays and the same statistics except the two marked "this rank".
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL t,
 * potentials or d_site_current.  KMCF_ERR_STATE: nothing assembled yet.  KMCF_ERR_COMM:
 * communicator not connected. */
typedef struct {
    double i_injection;    /* net[1]: equals I_macro as get_imacro_sparse forms it            */
    double i_extraction;   /* -net[0]: current arriving at the extraction node from atoms      */
    double sum_through;    /* sum over atoms of through[]                                      */
    double sum_tunnel;     /* sum over atoms of tunnel[]                                       */
    double max_through;    /* largest through[] of an atom, and the site that holds it:        */
    int    max_site;       /* the smallest site id among equals; -1 if there is no atom row   */
    int    tunnel_pairs_walked; /* set off-diagonal bits of this rank's rows (saturating)      */
    float  ms;             /* device time of everything the call enqueued (HIP events); this rank */
} kmcf_current_map_stats_t;

int kmcf_current_map(kmcf_tstate *t, const double *d_atom_virtual_potentials,
                     double *d_site_current /* N, required */, double *d_site_tunnel /* N or NULL */,
                     double *d_site_net /* N or NULL */, kmcf_current_map_stats_t *stats /* or NULL */);

/* Current profile: which cell carries the current, where along x it tunnels, which way it flows.
 * Nodes, potentials m, PAIR and I_rc = g (m[r] - m[c]) are exactly kmcf_current_map's.  A COUNTED
 * pair is a PAIR whose two ends are both atoms (nodes >= 2): pairs with a virtual end have no
 * position and are left out.  x_a, y_a, z_a are the coordinates of atom a the state holds.
 * Planes: h_plane_x[0 .. n_planes) strictly ascending and finite; q(a) = number of planes with
 * X_k <= x_a (an atom on a plane lies to its right).  A directed counted pair r -> s CROSSES
 * PLANE k FORWARD iff q(r) <= k < q(s); every pair is stored from both ends, only its left end
 * counts it, once, with its sign.  x is never periodic, so this holds under periodic y-z too.
 * Cells: cell(a) = d_site_cell[atom_site[a]]; the pair (r, s) belongs to cell c when
 * cell(r) == cell(s) == c and 0 <= c < n_cells, every other counted pair to the REST, stored as
 * cell index n_cells.  d_site_cell == NULL requires n_cells == 1 and puts every site in cell 0
 * (kmcf_site_set_gap's convention).
 * Profile: F[c][k][t] = sum of I_rs over the counted pairs of cell c and kind t (0 neighbour
 * pairs, 1 tunnel pairs) that cross plane k forward; h_profile[((c * n_planes) + k) * 2 + t],
 * c in [0, n_cells]; positive = flow towards +x.  It is formed per node: with S_a the sum of I_as
 * over a's counted pairs (of one kind and bucket) that end in another slab, q(s) != q(a),
 * F[c][k][t] = sum of S_a over the atoms of cell c with q(a) <= k (the rest over all atoms): pairs
 * with both ends left of the plane cancel, pairs inside one slab are never added.
 * Current vector: J_a = 1/2 sum_s I_as * d_as over the counted pairs of atom a, both kinds; d_as
 * is the displacement from a to s: dx = x_s - x_a, and dy, dz likewise on an open state; on a
 * periodic state f = (y_s - y_a) / Ly, f -= round(f), dy = f * Ly and z likewise (the library's
 * one minimum image).  Each term is (g * (m_r - m_s)) * d, every operation rounded.  Three
 * optional site arrays, N doubles each, zero-filled, then written at atom_site[a] for the atoms
 * with a row; pass all three or none.  Units: A * Angstrom.
 * Statistics: TOTAL[k] = sum over c = 0 .. n_cells, in that order, of (F[c][k][0] + F[c][k][1]).
 * Contract as for kmcf_current_map: reads the state as the last assembly left it, changes scratch
 * only, never touches site_power, the matrix or a tunnel storage; walks the pair bitmap, so it
 * does not depend on the storage the solve chose; two calls on the same input return the same
 * bytes (no atomics on doubles, every sum in an order the input fixes).  A periodic state uses
 * its distance functor for the WKB value and the minimum image for d_as.  On a rank group every
 * rank calls it: each forms the sums of its own rows, the per-node values are all-gathered by the
 * row partition, every rank returns the complete profile and site arrays.
 * KMCF_ERR_ARG (before anything needs a device; kmcf_last_error names the argument): NULL t,
 * potentials, h_plane_x or h_profile; n_planes or n_cells outside 1 ... 1024; NULL d_site_cell
 * with n_cells != 1; planes not finite or not strictly ascending; only some of the three vector
 * arrays set.  KMCF_ERR_STATE: nothing assembled yet.  KMCF_ERR_COMM: communicator not connected. */
typedef struct {
    double i_injection, i_extraction;   /* as kmcf_current_map_stats_t */
    double flux_min, flux_max;          /* smallest / largest TOTAL forward current over the planes
                                           (all cells + rest, both kinds) */
    double sum_jx;                      /* sum over atoms of jx; 0 when no vector was asked for */
    int    plane_min, plane_max;        /* the planes that hold them, lowest index among equals */
    float  ms_pairs, ms_planes;         /* device time: pair walk + gather / everything behind; this rank */
} kmcf_current_profile_stats_t;

int kmcf_current_profile(kmcf_tstate *t, const double *d_atom_virtual_potentials,
                         const int *d_site_cell /* N, or NULL */, int n_cells,
                         const double *h_plane_x /* n_planes, host */, int n_planes,
                         double *h_profile /* (n_cells + 1) * n_planes * 2, host, required */,
                         double *d_site_jx, double *d_site_jy, double *d_site_jz /* N each, or all NULL */,
                         kmcf_current_profile_stats_t *stats /* or NULL */);

/* update_temperatureglobal_gpu (src/heat_solver_gpu.cu:53-70). */
int kmcf_update_temperature_global(kmcf_comm *c, const double *d_site_power, double *d_T_bg, int N,
                                   double a_coeff, double b_coeff, double number_steps,
                                   double C_thermal, double small_step);

/* Local thermal model: the "Local thermal model" block of the reference's parameters.txt
 * plus the solver's stopping rule. */
typedef struct {
    double background_temp;        /* [K] temperature of the contact sites                         */
    double k_th_metal;             /* [W/mK] pair of metal sites                                   */
    double k_th_vacancies;         /* [W/mK] pair of uncharged vacancies (class 2 of K's rule)     */
    double k_th_non_vacancy;       /* [W/mK] every other pair                                      */
    double L_char;                 /* [m] pair conductance g = k_th * L_char [W/K]                 */
    double c_p;                    /* [J/Kcm^3] heat capacity = c_p * 1e6 * A * t_ox, shared       */
    double A;                      /* [m^2]     equally by the interface sites                     */
    double t_ox;                   /* [m]                                                          */
    double delta_t;                /* [s] step_time > 1e3 * delta_t selects the steady state       */
    double cg_tolerance;           /* sqrt(r.D^-1 r / b.b) <= cg_tolerance, conductances in units  */
                                   /* of the largest pair conductance (local heat)      */
    int cg_max_iterations;
} kmcf_heat_params_t;

/* Local heat solve (the solve_heating_local branch of Device::updateTemperature,
 * src/heat_solver.cpp:76-98, with a sparse operator: DESIGN.md, "Local heat solve").
 * Graph Laplacian of pair conductances on K's pattern, contact sites held at
 * background_temp, source d_site_power [W] (N doubles); one backward-Euler step of
 * step_time, or the steady state when step_time > 1e3 * delta_t (*h_steady = 1).
 * d_site_temperature: N doubles in/out.  Its interface slice is T_old and the start guess;
 * on return every rank holds the whole field (interface solved, contacts = background_temp).
 * The contact slots are written, never read: whatever the caller left there is replaced.
 * step_time == 0 assembles and solves nothing: the interface slice comes back as it was, the
 * contacts are set to background_temp all the same, *h_steady = 0, stats are zero with
 * converged = 1, and the state keeps the system it held.
 * *h_T_bg = mean over the interface sites.  h_T_bg, h_steady and stats may be NULL.
 * Runs on one rank and on rank groups; overwrites the K values of the state (the next
 * kmcf_k_assemble refills them) and never uses K's resident solve plan. */
int kmcf_update_temperature_local(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                                  const int *d_metals, int num_metals, const double *d_site_power,
                                  double *d_site_temperature, int N, int N_left_tot, int N_right_tot,
                                  double step_time, const kmcf_heat_params_t *p,
                                  double *h_T_bg, int *h_steady, kmcf_solve_stats_t *stats);

/* Site neighbour index list (compute_neighbor_list, src/neighbor_lists_gpu.cu:
 * 55-77, 252-292): nn slots per site, -1 padded, ascending j.  Cell list
 * instead of the O(N^2) scan.  d_neigh_idx: count*nn ints. */
int kmcf_neighbor_list(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                       double nn_dist, int nn, int count, int displ, int *d_neigh_idx);

/* The same list under periodic boundaries in y and z: pbc == 1 takes the minimum-image distance (see
 * kmcf_compute_cutoff_list_pbc) with the periods h_lattice[1], h_lattice[2]; same output contract (ascending j, -1
 * padded, rows truncated at nn, the error for a site with too many neighbours).  The wrapped cell grid of
 * kmcf_initialize_sparsity_K; where fewer than 3 cells of nn_dist fit a period, or the sites span one, every pair is
 * tested.  pbc == 0: the bytes of kmcf_neighbor_list (h_lattice may be NULL).  Everything that reads the list --
 * kmcf_update_charge, the event step, kmcf_conductive_clusters, the heat pattern -- is periodic through it.
 * KMCF_ERR_ARG: as kmcf_neighbor_list, and pbc outside 0 / 1, NULL h_lattice or a period not finite or <= 0 with pbc == 1. */
int kmcf_neighbor_list_pbc(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                           const double *h_lattice /* 3, host */, int pbc, double nn_dist, int nn, int count, int displ,
                           int *d_neigh_idx);

#ifdef __cplusplus
}
#endif
#endif /* KMCFIELD_H */
