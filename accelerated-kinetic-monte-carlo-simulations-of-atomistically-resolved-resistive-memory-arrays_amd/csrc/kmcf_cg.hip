// Jacobi-preconditioned CG for gfx950, replacing
// iterative_solver::conjugate_gradient_jacobi / conjugate_gradient
// (dist_iterative/dist_conjugate_gradient.cpp:17-121, 149-276).
//
// Same recurrence, same operation order and same stopping rule as the reference
// (r.z/(b.b) > tol^2 && k <= max_it, :217), but:
//  * the reference's 6 hipBLAS calls + 1 Hadamard kernel + 2 host-returning dots
//    per iteration become 3 kernels (p update | SpMV + p.Ap | x,r,z update + r.z);
//  * alpha, beta, r.z, p.Ap and the convergence flag live in device memory; the
//    host enqueues growing chunks of 2 .. KMCF_CHUNK_ITERS iterations and reads the flag back
//    once per chunk.  Kernels launched after convergence return at once, so x is
//    exactly the iterate the reference would have stopped at;
//  * dot products: one partial per block, summed in a fixed order by every block of
//    the consuming kernel (bitwise reproducible, no fp64 atomics).  With several
//    ranks a 1-block finalize + ncclAllReduce on the compute stream sits in between.
//
// Vector traffic per iteration besides the SpMV: p update 3R+1W, r update 3R+1W, and the x update (1R+1W and one more
// read of p) once in KMCF_CG_XBATCH = B iterations: 80 - 8 (B-1)/B bytes per row (the reference's op sequence: 144 B/row,
// SURVEY 8d).
#include <chrono>
#include <cmath>
#include <cstring>

#include "kmcf_p2p_dev.hpp"

namespace {

// Up to four partial arrays (an SpMV writes one per pass: interior rows, boundary rows, long rows, sub-block).
struct part_ref {
    const double *p[4];
    int n[4];
};

part_ref pr1(const double *a, int na) { return part_ref{{a, nullptr, nullptr, nullptr}, {na, 0, 0, 0}}; }
part_ref pr_none() { return pr1(nullptr, 0); }
part_ref pr_spmv(const kmcf_matrix *m)
{
    const kmcf_part4 q = kmcf_spmv_partials(m);
    return part_ref{{q.p[0], q.p[1], q.p[2], q.p[3]}, {q.n[0], q.n[1], q.n[2], q.n[3]}};
}

// Sum of the partial arrays in a fixed order; every thread of the block gets the result.
__device__ __forceinline__ double reduce_partials(const part_ref &r, double *lds4)
{
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int i = threadIdx.x; i < r.n[q]; i += KMCF_BLOCK) v += r.p[q][i];
    return kmcf_block_sum(v, lds4);
}

// r = b - A x0 ; z = r .* dinv ; partial r.z and b.b   (dist_conjugate_gradient.cpp:187, 201-212)
template <bool PRECOND>
__global__ __launch_bounds__(KMCF_BLOCK) void cg_init_kernel(int n, double *__restrict__ r, const double *__restrict__ Ap,
                                                             const double *__restrict__ dinv,
                                                             double *__restrict__ part_rz, double *__restrict__ part_bb)
{
    __shared__ double lds4[4];
    double rz = 0.0, bb = 0.0;
    for (int i = blockIdx.x * KMCF_BLOCK + threadIdx.x; i < n; i += gridDim.x * KMCF_BLOCK) {
        double b = r[i];
        bb += b * b;
        double ri = b + (-1.0) * Ap[i];
        r[i] = ri;
        double z = PRECOND ? ri * dinv[i] : ri;
        rz += ri * z;
    }
    double t = kmcf_block_sum(rz, lds4);
    double u = kmcf_block_sum(bb, lds4);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = t; part_bb[blockIdx.x] = u; }
}

// One block: S->red[slot] = sum of partials (input of the all-reduce).
__global__ __launch_bounds__(KMCF_BLOCK) void cg_finalize_kernel(part_ref p0, int slot0, part_ref p1, int slot1,
                                                                 kmcf_scalars *__restrict__ S, int check_done)
{
    __shared__ double lds4[4];
    if (check_done && S->done) return;
    double t0 = reduce_partials(p0, lds4);
    if (threadIdx.x == 0) S->red[slot0] = t0;
    if (slot1 >= 0) {
        double t1 = reduce_partials(p1, lds4);
        if (threadIdx.x == 0) S->red[slot1] = t1;
    }
}

// The x += alpha p still pending, oldest first: x = ((x + a_0 p_0) + a_1 p_1) + ...  -- the operations and operands of
// applying them one by one as they arose.  Runtime count; the cold paths (a loop that stops or ends on its limit).
__device__ __forceinline__ void xring_apply2(double2 &xv, const kmcf_xring &h, const double (&a)[4], int pending, int i)
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= h.nb - pending && j < h.nb) {
            const double2 pv = reinterpret_cast<const double2 *>(h.p[j])[i];
            xv.x = xv.x + a[j] * pv.x;
            xv.y = xv.y + a[j] * pv.y;
        }
}
__device__ __forceinline__ void xring_apply1(double &xv, const kmcf_xring &h, const double (&a)[4], int pending, int i)
{
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j >= h.nb - pending && j < h.nb) xv = xv + a[j] * h.p[j][i];
}
__device__ __forceinline__ void xring_steps(const kmcf_xring &h, const kmcf_scalars *S, double (&a)[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = j < h.nb ? S->xa_ring[h.slot[j]] : 0.0;
}

// Loop head of iteration k: stopping rule, beta, p = z + beta p   (:217-227) -- and the x += alpha p of the iterations
// before (:243), which are applied HERE, where the old p is read anyway: the residual kernel does not touch x and p
// (80 instead of 88 bytes per row and iteration; the same operation on the same operands, one kernel later).
// Nothing in an iteration reads x, so with KMCF_CG_XBATCH = B > 1 the direction is not overwritten in place: p_k goes to
// slot k % B of a ring of B buffers (h: the ring from the slot written longest ago -- this launch's target -- to p_(k-1)),
// up to B updates stay pending, and one launch in B applies them in order (NF = B: the flush instance; NF = 0 does not
// touch x).  B = 1: every launch behind the first is the flush instance on one buffer, i.e. the kernel as it was.
// The target of a flush launch IS the buffer of the oldest pending p -- every thread reads its element of it before it
// writes it -- so the ring's pointers are not __restrict__.
// Updates still pending when the loop ends are applied by cg_x_kernel or by the caller's output kernel.
template <bool PRECOND, int NF>
__global__ __launch_bounds__(KMCF_BLOCK) void cg_p_kernel(int n, kmcf_xring h, const double *p_prev, double *p_out,
                                                          const double *__restrict__ r, const double *__restrict__ dinv,
                                                          part_ref prz, part_ref pbb, kmcf_scalars *__restrict__ S, int k,
                                                          int first, double tol2, int check_tol, double *__restrict__ x,
                                                          int pending)
{
    __shared__ double lds4[4];
    const int parity = k & 1;
    // Everything this block needs is requested before anything is waited for (scalars, the partial sums of the
    // previous kernel, the block's first elements -- of every pending p in the flush instance): a block lives for one
    // or two elements per lane, so a chain of dependent loads in front of its stream would be most of its life.
    const int n2 = n >> 1;
    const double2 *r2 = reinterpret_cast<const double2 *>(r), *d2 = reinterpret_cast<const double2 *>(dinv);
    const double2 *q2 = reinterpret_cast<const double2 *>(p_prev);
    double2 *p2 = reinterpret_cast<double2 *>(p_out);
    const int i0 = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    // stopped by an EARLIER launch?  (S->done itself is written by block 0 of this very launch when the stopping rule
    // fires: a block scheduled late would see it, return here and skip its share of the pending x updates below)
    const int stop_k = S->stop_k;
    const bool done = stop_k != 0 && stop_k != k;
    const double rz_prev = S->rz[parity ^ 1], bb_saved = S->bb;
    double2 *x2 = reinterpret_cast<double2 *>(x);
    double xa[NF > 0 ? NF : 1];
#pragma unroll
    for (int j = 0; j < NF; ++j) xa[j] = S->xa_ring[h.slot[j]];
    double2 z0 = make_double2(0.0, 0.0), dv0 = make_double2(1.0, 1.0), pv0 = make_double2(0.0, 0.0), xv0 = pv0;
    double2 hv0[NF > 1 ? NF - 1 : 1];                  // the pending p older than p_(k-1), oldest first
    if (!first && i0 < n2) {
        z0 = r2[i0];
        if (PRECOND) dv0 = d2[i0];
#pragma unroll
        for (int j = 0; j < NF - 1; ++j) hv0[j] = reinterpret_cast<const double2 *>(h.p[j])[i0];
        pv0 = q2[i0];
        if (NF > 0) xv0 = x2[i0];
    }
    const double rz_new = reduce_partials(prz, lds4);
    if (done) return;
    double bb;
    if (first) bb = reduce_partials(pbb, lds4);
    else bb = bb_saved;
    // check_tol: 0 fixed iteration count; 1 relative rule r.z/b.b > tol^2 (:217);
    // 2 absolute rule of solve_sparse_CG_Jacobi (src/iterative_solvers_gpu.cu:838-840, 858):
    //   first test on ||r|| (hipblasDnrm2), later ones on ||r||^2 (hipblasDdot)
    bool go = true;
    if (check_tol == 1) go = rz_new / bb > tol2;
    else if (check_tol == 2) go = (first ? sqrt(rz_new) : rz_new) > tol2;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        S->rz_last = rz_new;
        if (first) S->bb = bb;
        if (go) { S->rz[parity] = rz_new; S->iters += 1; }
        else { S->stop_k = k; S->done = 1; }
    }
    if (!go) {
        // the x += alpha p of the last iterations -- however many are pending, in order -- then nothing more (later
        // kernels see S->done).  Cold: read from the ring, whatever this instance has requested above.
        if (pending) {
            double a[4];
            xring_steps(h, S, a);
            for (int i = i0; i < n2; i += gridDim.x * KMCF_BLOCK) {
                double2 xv = x2[i];
                xring_apply2(xv, h, a, pending, i);
                x2[i] = xv;
            }
            if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
                double xv = x[n - 1];
                xring_apply1(xv, h, a, pending, n - 1);
                x[n - 1] = xv;
            }
        }
        return;
    }
    // two elements per lane and step (16-byte loads and stores; the workspace vectors are 256-byte aligned)
    if (first) {
        for (int i = blockIdx.x * KMCF_BLOCK + threadIdx.x; i < n2; i += gridDim.x * KMCF_BLOCK) {
            double2 rv = r2[i];
            if (PRECOND) { const double2 dv = d2[i]; rv.x *= dv.x; rv.y *= dv.y; }
            p2[i] = rv;                                                    // :226 dcopy(z -> p)
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) p_out[n - 1] = PRECOND ? r[n - 1] * dinv[n - 1] : r[n - 1];
    } else {
        const double beta = rz_new / rz_prev;                              // :220
        if (i0 < n2) {                                                     // (the prefetched element)
            if (NF > 0) {                                                  // :243 of k-NF .. k-1
#pragma unroll
                for (int j = 0; j < NF - 1; ++j) { xv0.x = xv0.x + xa[j] * hv0[j].x; xv0.y = xv0.y + xa[j] * hv0[j].y; }
                xv0.x = xv0.x + xa[NF > 0 ? NF - 1 : 0] * pv0.x;
                xv0.y = xv0.y + xa[NF > 0 ? NF - 1 : 0] * pv0.y;
                x2[i0] = xv0;
            }
            if (PRECOND) { z0.x *= dv0.x; z0.y *= dv0.y; }
            pv0.x = beta * pv0.x + z0.x;                                   // :221 dscal, :222 daxpy
            pv0.y = beta * pv0.y + z0.y;
            p2[i0] = pv0;
        }
        for (int i = i0 + gridDim.x * KMCF_BLOCK; i < n2; i += gridDim.x * KMCF_BLOCK) {
            double2 z = r2[i];
            if (PRECOND) { const double2 dv = d2[i]; z.x *= dv.x; z.y *= dv.y; }
            double2 hv[NF > 1 ? NF - 1 : 1];
#pragma unroll
            for (int j = 0; j < NF - 1; ++j) hv[j] = reinterpret_cast<const double2 *>(h.p[j])[i];
            double2 pv = q2[i];
            if (NF > 0) {
                double2 xv = x2[i];
#pragma unroll
                for (int j = 0; j < NF - 1; ++j) { xv.x = xv.x + xa[j] * hv[j].x; xv.y = xv.y + xa[j] * hv[j].y; }
                xv.x = xv.x + xa[NF > 0 ? NF - 1 : 0] * pv.x;
                xv.y = xv.y + xa[NF > 0 ? NF - 1 : 0] * pv.y;
                x2[i] = xv;
            }
            pv.x = beta * pv.x + z.x;
            pv.y = beta * pv.y + z.y;
            p2[i] = pv;
        }
        if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            const double z = PRECOND ? r[n - 1] * dinv[n - 1] : r[n - 1];
            const double pl = p_prev[n - 1];
            if (NF > 0) {
                double xv = x[n - 1];
#pragma unroll
                for (int j = 0; j < NF - 1; ++j) xv = xv + xa[j] * h.p[j][n - 1];
                xv = xv + xa[NF > 0 ? NF - 1 : 0] * pl;
                x[n - 1] = xv;
            }
            p_out[n - 1] = beta * pl + z;
        }
    }
}

// alpha = rz/pAp ; r -= alpha Ap ; z = r .* dinv ; partial r.z   (:243-264); x += alpha p is left pending (cg_p_kernel)
template <bool PRECOND>
__global__ __launch_bounds__(KMCF_BLOCK) void cg_xr_kernel(int n, double *__restrict__ r, const double *__restrict__ Ap,
                                                           const double *__restrict__ dinv, part_ref ppap,
                                                           kmcf_scalars *__restrict__ S, int parity,
                                                           double *__restrict__ part_rz, int xa_slot, int pending_after)
{
    __shared__ double lds4[4];
    // two elements per lane and step (16-byte loads and stores; the workspace vectors are 256-byte aligned);
    // scalars, partial sums and the block's first elements are all requested before the first wait (cg_p_kernel)
    const int n2 = n >> 1;
    double2 *r2 = reinterpret_cast<double2 *>(r);
    const double2 *A2 = reinterpret_cast<const double2 *>(Ap), *d2 = reinterpret_cast<const double2 *>(dinv);
    const int i0 = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    const int done = S->done;
    const double rz_cur = S->rz[parity];
    double2 av0 = make_double2(0.0, 0.0), rv0 = av0, dv0 = make_double2(1.0, 1.0);
    if (i0 < n2) {
        av0 = A2[i0]; rv0 = r2[i0];
        if (PRECOND) dv0 = d2[i0];
    }
    const double pAp = reduce_partials(ppap, lds4);
    if (done) return;
    const double a = rz_cur / pAp;
    const double na = -a;
    double rz = 0.0;
    if (i0 < n2) {                                  // (the prefetched element; same operations as the loop's)
        rv0.x = rv0.x + na * av0.x;
        rv0.y = rv0.y + na * av0.y;
        r2[i0] = rv0;
        double2 z = rv0;
        if (PRECOND) { z.x *= dv0.x; z.y *= dv0.y; }
        rz += rv0.x * z.x;
        rz += rv0.y * z.y;
    }
    for (int i = i0 + gridDim.x * KMCF_BLOCK; i < n2; i += gridDim.x * KMCF_BLOCK) {
        const double2 av = A2[i];
        double2 rv = r2[i];
        rv.x = rv.x + na * av.x;
        rv.y = rv.y + na * av.y;
        r2[i] = rv;
        double2 z = rv;
        if (PRECOND) { const double2 dv = d2[i]; z.x *= dv.x; z.y *= dv.y; }
        rz += rv.x * z.x;
        rz += rv.y * z.y;
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
        const int i = n - 1;
        const double ri = r[i] + na * Ap[i];
        r[i] = ri;
        const double z = PRECOND ? ri * dinv[i] : ri;
        rz += ri * z;
    }
    double t = kmcf_block_sum(rz, lds4);
    if (threadIdx.x == 0) {
        part_rz[blockIdx.x] = t;
        // (the step length goes into the ring slot of this iteration's p; pending_after: the host's count, one more
        //  than the loop head of this iteration left)
        if (blockIdx.x == 0) { S->pAp = pAp; S->xa = a; S->xa_ring[xa_slot] = a; S->x_pending = pending_after; }
    }
}

// The x += alpha p still pending when the loop ended on its iteration limit, oldest first.
__global__ __launch_bounds__(KMCF_BLOCK) void cg_x_kernel(int n, double *__restrict__ x, kmcf_xring h,
                                                          const kmcf_scalars *__restrict__ S)
{
    const int pending = S->x_pending;
    if (S->done || !pending) return;
    double a[4];
    xring_steps(h, S, a);
    for (int i = blockIdx.x * KMCF_BLOCK + threadIdx.x; i < n; i += gridDim.x * KMCF_BLOCK) {
        double xv = x[i];
        xring_apply1(xv, h, a, pending, i);
        x[i] = xv;
    }
}

// After the loop: the r.z the reference prints (:273) if the loop did not end on the stopping rule.
__global__ __launch_bounds__(KMCF_BLOCK) void cg_tail_kernel(part_ref prz, kmcf_scalars *__restrict__ S)
{
    __shared__ double lds4[4];
    if (S->done) return;
    double t = reduce_partials(prz, lds4);
    if (threadIdx.x == 0) S->rz_last = t;
}

// End of a chunk of iterations: has the loop stopped?  The device says so in pinned host memory (one thread, behind the
// chunk's last kernel): {done, iterations, this check's number} -- and the host polls the number instead of sleeping in
// hipStreamSynchronize, whose wake-up costs more than the ten iterations a small system runs meanwhile (5 nm device:
// 13 checks per cold solve).  After 3 ms without an answer it sleeps in
// hipStreamSynchronize after all.
__global__ void cg_mark_kernel(const kmcf_scalars *__restrict__ S, int *__restrict__ host3, int number)
{
    if (threadIdx.x != 0) return;
    host3[0] = S->done;
    host3[1] = S->iters;
    __threadfence_system();
    __hip_atomic_store(&host3[2], number, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
int cg_chunk_check(kmcf_comm *c, const kmcf_scalars *S, hipStream_t st, bool *done)
{
    if (c->mark_seq == 0x7fffffff) c->mark_seq = 0;
    const int number = ++c->mark_seq;
    // the word the host polls must differ from the number waited for BEFORE the kernel that writes it is enqueued
    // (pinned blocks are recycled by the runtime; nothing else writes this word between checks)
    __atomic_store_n(c->h_pinned + 2, 0, __ATOMIC_RELEASE);
    cg_mark_kernel<<<1, 64, 0, st>>>(S, c->h_pinned, number);
    KMCF_HIP(hipGetLastError());
    const auto t0 = std::chrono::steady_clock::now();
    volatile int *flag = c->h_pinned + 2;
    int spins = 0;
    while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != number) {
        if ((++spins & 255) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 3e-3) {
            KMCF_HIP(hipStreamSynchronize(st));            // (then the mark has been written)
            break;
        }
    }
    *done = c->h_pinned[0] != 0;
    return KMCF_OK;
}

// Reads back the scalars of the solve enqueued last (after ONE stream synchronisation) and fills `stats`.
int pcg_collect(kmcf_matrix *m, double tol2, int absolute, kmcf_solve_stats_t *stats, bool loop_time = true)
{
    kmcf_comm *c = m->comm;
    KMCF_HIP(hipStreamSynchronize(c->stream));
    if (c->nranks > 1 || c->force_collectives) KMCF_HIP(hipStreamSynchronize(c->comm_stream));
    KMCF_TRY(kmcf_p2p_check(c));
    KMCF_TRY(kmcf_cgr_check(m));
    const kmcf_scalars &hS = *c->h_scal;
    if (stats) {
        stats->iterations = hS.iters;
        stats->bb = hS.bb;
        stats->rz = hS.rz_last;
        // (b = 0 from x0 = 0: the system is solved as it stands, and 0 / 0 is no residual)
        stats->relres = hS.bb == 0.0 && hS.rz_last == 0.0 ? 0.0 : std::sqrt(hS.rz_last / hS.bb);
        stats->converged = (hS.done != 0) || !((absolute ? hS.rz_last : hS.rz_last / hS.bb) > tol2);
        if (loop_time) {                                   // (kmcf_pcg_jacobi times the whole call instead: the first
            float ms = 0.f;                                //  hipEventElapsedTime after a synchronisation costs ~13 us)
            KMCF_HIP(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
            stats->ms_solve = ms;
        }
    }
    return KMCF_OK;
}

// The ring as the loop head of iteration k sees it: slots k % B (written B iterations ago: the target) ... (k - 1) % B.
kmcf_xring xring_at(double *const (&ring)[4], int B, int k)
{
    kmcf_xring h = {};
    h.nb = B;
    for (int i = 0; i < B; ++i) { h.p[i] = ring[(k + i) % B]; h.slot[i] = (k + i) % B; }
    return h;
}

template <bool PRECOND>
void cg_p_launch(int nf, int grid, hipStream_t st, int n, const kmcf_xring &h, const double *p_prev, double *p_out, const double *r,
                 const double *dinv, const part_ref &prz, const part_ref &pbb, kmcf_scalars *S, int k, int first, double tol2,
                 int check_tol, double *x, int pending)
{
#define KMCF_CG_P(NF) cg_p_kernel<PRECOND, NF><<<grid, KMCF_BLOCK, 0, st>>>(n, h, p_prev, p_out, r, dinv, prz, pbb, S, k, first, tol2, check_tol, x, pending)
    switch (nf) {
    case 0: KMCF_CG_P(0); break;
    case 1: KMCF_CG_P(1); break;
    case 2: KMCF_CG_P(2); break;
    case 3: KMCF_CG_P(3); break;
    default: KMCF_CG_P(4); break;
    }
#undef KMCF_CG_P
}

// ------------------------------------------------------------------------------------------------
// A solve as a loop of kernels.  cg_run_loop (behind the kernels of both recurrences) is the driver: prologue (scalars,
// p <- x0, A x0), growing chunks of iterations with a look at the stop flag behind each, epilogue.  A recurrence --
// pcg_loop, pcg1_loop -- supplies its set-up (setup: before anything is enqueued; residual0: behind A x0), "enqueue
// iteration k" and "after the loop" (sequence numbers of kmcf_cgplan.hpp, tail kernels), on top of what both share:
struct cg_loop_state {
    kmcf_matrix *const m;
    const kmcf_cg_request &q;
    kmcf_comm *const c = m->comm;
    const hipStream_t st = c->stream;
    kmcf_scalars *const S = m->d_S;
    const int n = m->n_loc, vg = kmcf_vec_grid(n);
    const bool multi = c->nranks > 1 || c->force_collectives;
    const double tol2 = q.tol * q.tol;
    const int check_tol = q.fixed_iters > 0 ? 0 : (q.call == KMCF_CG_CALL_ABSOLUTE ? 2 : 1);   // 0 fixed count, 1 relative, 2 absolute rule
    // what the kernels read for a sum: the local partial array, or -- a group -- the all-reduced scalar in S->red[slot]
    part_ref reduced(const part_ref &loc, int slot) const { return multi ? pr1(&S->red[slot], 1) : loc; }
};

template <bool PRECOND>
struct pcg_loop : cg_loop_state {
    const part_ref prz_loc = pr1(m->d_part_b, vg), pbb_loc = pr1(m->d_part_c, vg), ppap_loc = pr_spmv(m);
    const part_ref prz = reduced(prz_loc, 0), pbb = reduced(pbb_loc, 1), ppap = reduced(ppap_loc, 2);
    // "direct" peer-to-peer protocol: the SpMV counts halo sequence numbers per launch; set back to per executed SpMV
    // after the loop
    bool direct = false;
    u64 halo0 = 0;
    // The p ring (KMCF_CG_XBATCH = B; cg_p_kernel): slot 0 is d_p itself -- it holds x0 for the A x0 of the prologue --
    // and p_k lives in slot k % B.  One rank only: a group's halo lands behind d_p.  m->d_p follows the ring through the
    // loop and is the original buffer again on every way out of it.
    int B = 1;
    double *ring[4] = {m->d_p, nullptr, nullptr, nullptr};
    int pending = 0;                               // x += alpha p not applied yet (the device's S->x_pending while it runs)

    pcg_loop(kmcf_matrix *m_, const kmcf_cg_request &q_) : cg_loop_state{m_, q_} {}
    ~pcg_loop() { m->d_p = ring[0]; }
    int setup() { return KMCF_OK; }

    // r = b - Ap ; z ; r.z ; b.b    (:187-213)
    int residual0()
    {
        cg_init_kernel<PRECOND><<<vg, KMCF_BLOCK, 0, st>>>(n, m->d_r, m->d_Ap, m->d_dinv, m->d_part_b, m->d_part_c);
        KMCF_HIP(hipGetLastError());
        if (multi) {
            cg_finalize_kernel<<<1, KMCF_BLOCK, 0, st>>>(prz_loc, 0, pbb_loc, 1, S, 0);
            KMCF_HIP(hipGetLastError());
            KMCF_TRY(kmcf_comm_allreduce_sum(c, &S->red[0], 2));
        }
        direct = multi && c->nranks > 1 && kmcf_p2p_direct(m);
        halo0 = direct ? *kmcf_p2p_halo_seq(m, 0) : 0;
        B = multi ? 1 : std::min(std::max(kmcf_opt_int(c, KNOB_CG_XBATCH, KMCF_CG_XBATCH_DEFAULT), 1), 4);
        for (int j = 1; j < B; ++j) {
            if (!m->d_p_ring[j - 1]) {
                const size_t len = (size_t)n + m->n_halo + 2;
                KMCF_TRY(kmcf_dev_alloc(&m->d_p_ring[j - 1], len, false));
                KMCF_HIP(hipMemsetAsync(m->d_p_ring[j - 1], 0, len * sizeof(double), st));
            }
            ring[j] = m->d_p_ring[j - 1];
        }
        return KMCF_OK;
    }

    // iteration k (the reference's k): loop head | SpMV + p.Ap | r, z update + r.z
    int iteration(int k)
    {
        // loop head: all `pending` updates of x if the ring is full, none otherwise; p_k into slot k % B
        const int nf = pending == B ? B : 0;
        cg_p_launch<PRECOND>(nf, vg, st, n, xring_at(ring, B, k), ring[(k - 1) % B], ring[k % B], m->d_r, m->d_dinv, prz, pbb, S, k,
                             k == 1 ? 1 : 0, tol2, check_tol, m->d_x, pending);
        KMCF_HIP(hipGetLastError());
        if (nf) pending = 0;
        m->d_p = ring[k % B];                      // (every SpMV path reads m->d_p when it launches)
        KMCF_TRY(kmcf_spmv_device(m, true, true));
        if (multi) {
            cg_finalize_kernel<<<1, KMCF_BLOCK, 0, st>>>(ppap_loc, 2, pr_none(), -1, S, 1);
            KMCF_HIP(hipGetLastError());
            KMCF_TRY(kmcf_comm_allreduce_sum(c, &S->red[2], 1));
        }
        ++pending;
        cg_xr_kernel<PRECOND><<<vg, KMCF_BLOCK, 0, st>>>(n, m->d_r, m->d_Ap, m->d_dinv, ppap, S, k & 1, m->d_part_b, k % B, pending);
        KMCF_HIP(hipGetLastError());
        if (multi) {
            cg_finalize_kernel<<<1, KMCF_BLOCK, 0, st>>>(prz_loc, 0, pr_none(), -1, S, 1);
            KMCF_HIP(hipGetLastError());
            KMCF_TRY(kmcf_comm_allreduce_sum(c, &S->red[0], 1));
        }
        return KMCF_OK;
    }

    int after(const kmcf_cg_loop_end &e, kmcf_cg_result *res)
    {
        const kmcf_xring xring = xring_at(ring, B, e.launched + 1);    // the ring as the next loop head would see it: pending updates last
        if (res) res->xring = xring;
        if (direct) *kmcf_p2p_halo_seq(m, 0) = *kmcf_p2p_halo_seq(m, 1) = kmcf_cg_classic_halo_seq(halo0, e);
        // the loop condition is evaluated once more after the last iteration (:217): it decides `converged` and provides
        // the printed residual (:273)
        if (!e.done && (!q.caller_collects || multi)) {    // (one rank: the caller's output kernel forms this last r.z itself ...
            cg_tail_kernel<<<1, KMCF_BLOCK, 0, st>>>(prz, S);
            KMCF_HIP(hipGetLastError());
        }
        if (!e.done && !q.caller_collects) {               //  ... and applies the pending x updates on its way)
            cg_x_kernel<<<vg, KMCF_BLOCK, 0, st>>>(n, m->d_x, xring, S);
            KMCF_HIP(hipGetLastError());
        }
        return KMCF_OK;
    }
};

// ------------------------------------------------------------------------------------------------
// Single-reduction PCG (Chronopoulos & Gear): the same Krylov iterates in exact arithmetic, but both
// inner products of an iteration -- gamma = (r,z) and delta = (Az,z) -- are available at the same
// point, so a multi-rank group pays ONE all-reduce (of 3 doubles) per iteration instead of two, and an
// iteration is 2 kernels (SpMV with fused delta | fused vector update) instead of 3.  The matrix is
// applied to z = M^-1 r; s = A p is carried by recurrence.  Same stopping rules on gamma: relative to b.b, or the
// absolute one of solve_sparse_CG_Jacobi (the band-edge solve of a group).
// Default for groups of more than one rank (latency-bound there); KMCF_CG_VARIANT=classic|cg1r overrides.
//
//   init : r = b - A x0 ; z = r.*dinv ; gamma = (r,z)
//   loop : w = A z ; delta = (w,z) ; [all-reduce gamma, delta]
//          stop if !(gamma/bb > tol^2)
//          beta = gamma/gamma_old (0 first) ; alpha = gamma / (delta - beta*gamma/alpha_old)
//          p = z + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; z = r.*dinv ; gamma' = (r,z)
template <bool PRECOND>
__global__ __launch_bounds__(KMCF_BLOCK) void cg1_init_kernel(int n, double *__restrict__ r, const double *__restrict__ Ap,
                                                              const double *__restrict__ dinv, double *__restrict__ z_out,
                                                              double *__restrict__ part_rz, double *__restrict__ part_bb)
{
    __shared__ double lds4[4];
    double rz = 0.0, bb = 0.0;
    for (int i = blockIdx.x * KMCF_BLOCK + threadIdx.x; i < n; i += gridDim.x * KMCF_BLOCK) {
        double b = r[i];
        bb += b * b;
        double ri = b + (-1.0) * Ap[i];
        r[i] = ri;
        double z = PRECOND ? ri * dinv[i] : ri;
        z_out[i] = z;
        rz += ri * z;
    }
    double t = kmcf_block_sum(rz, lds4);
    double u = kmcf_block_sum(bb, lds4);
    if (threadIdx.x == 0) { part_rz[blockIdx.x] = t; part_bb[blockIdx.x] = u; }
}

// Three sums of partial arrays in one pass (the loads of all three in flight together, one barrier instead of six); each
// sum is formed exactly as reduce_partials forms it (same per-thread sequence, same butterfly, same (w0 + w1) + (w2 + w3)).
__device__ __forceinline__ void reduce_partials3(const part_ref &a, const part_ref &b, const part_ref &c, bool with_c,
                                                 double (*lds)[4], double &ra, double &rb, double &rc)
{
    double va = 0.0, vb = 0.0, vc = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int i = threadIdx.x; i < a.n[q]; i += KMCF_BLOCK) va += a.p[q][i];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        for (int i = threadIdx.x; i < b.n[q]; i += KMCF_BLOCK) vb += b.p[q][i];
    if (with_c) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            for (int i = threadIdx.x; i < c.n[q]; i += KMCF_BLOCK) vc += c.p[q][i];
    }
    va = kmcf_wave_sum64(va); vb = kmcf_wave_sum64(vb); vc = kmcf_wave_sum64(vc);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { lds[0][w] = va; lds[1][w] = vb; lds[2][w] = vc; }
    __syncthreads();
    ra = (lds[0][0] + lds[0][1]) + (lds[0][2] + lds[0][3]);
    rb = (lds[1][0] + lds[1][1]) + (lds[1][2] + lds[1][3]);
    rc = (lds[2][0] + lds[2][1]) + (lds[2][2] + lds[2][3]);
    __syncthreads();                     // (lds is written again by the caller's kmcf_block_sum, with no barrier of the caller's in between)
}

// The update of the single-reduction loop, for one rank or a host-synchronous group (P2P = false: gamma, delta, b.b are
// the sums of the partial arrays, i.e. of the ONE all-reduced value each when a group's transport reduced them), or with
// the group's exchanges folded in (P2P = true, the "direct" peer-to-peer protocol, kmcf_p2p_dev.hpp): ONE kernel per
// iteration besides the SpMV's two.
//   * all-reduce: every block forms this rank's sums of gamma, delta (and b.b) from the partial arrays; block 0 stores
//     them into slot [parity][rank] of every peer's window and raises its flag there; every block waits (bounded)
//     for the P flags of its OWN window and adds the P slots in rank order -- the same numbers in the same order on
//     every rank and in every block;
//   * acknowledgement of the halo the SpMV in front of this kernel has consumed (block 0);
//   * put: the thread that computes the new z of a row a neighbour needs stores it into buffer (seq_put & 1) of that
//     neighbour's landing zone (after the acknowledgements of seq_put - 2 are in: every block checks); the last block
//     to finish raises the neighbours' flags -- the halo of the NEXT SpMV is on its way while this kernel still runs.
// Both variants: same arithmetic, same summation order (two rows per lane and step, like cg_xr_kernel), so a group's
// iterates do not depend on its transport.  A block lives for one or two steps: scalars, partial sums and the block's
// first elements are all requested before the first wait (a kernel of this size is a chain of memory round trips;
// measured on a rank's eighth of the 40 nm matrix: 9.8 us with the chain done -> reduce -> reduce -> reduce -> loop).
template <bool PRECOND, bool P2P>
__global__ __launch_bounds__(KMCF_BLOCK) void cg1_update_kernel(
    int n, double *__restrict__ x, double *__restrict__ r, double *__restrict__ p, double *__restrict__ s,
    double *__restrict__ z /* in: z, out: next z (SpMV input) */, const double *__restrict__ w,
    const double *__restrict__ dinv, part_ref pgamma, part_ref pdelta, part_ref pbb, kmcf_scalars *__restrict__ S,
    int parity, int first, double tol2, int check_tol, double *__restrict__ part_rz, kmcf_p2p_dev pd, u64 seq_red,
    u64 seq_ack, u64 seq_put, int ar_inside)
{
    __shared__ double lds[3][4];
    __shared__ double red[4];
    __shared__ int s_last;
    const int t = threadIdx.x;
    const int n2 = n >> 1;
    const int i0 = blockIdx.x * KMCF_BLOCK + t;
    double2 *x2 = reinterpret_cast<double2 *>(x), *r2 = reinterpret_cast<double2 *>(r), *p2 = reinterpret_cast<double2 *>(p),
            *s2 = reinterpret_cast<double2 *>(s), *z2 = reinterpret_cast<double2 *>(z);
    const double2 *w2 = reinterpret_cast<const double2 *>(w), *d2 = reinterpret_cast<const double2 *>(dinv);
    // ---- everything this block needs, requested at once
    const int done = S->done;
    const double bb_saved = S->bb, rz_prev = S->rz[parity ^ 1], alpha_prev = S->alpha[parity ^ 1];
    const double2 zero = make_double2(0.0, 0.0);
    double2 zv0 = zero, wv0 = zero, pv0 = zero, sv0 = zero, xv0 = zero, rv0 = zero, dv0 = make_double2(1.0, 1.0);
    int2 pr0 = make_int2(-1, -1);
    if (i0 < n2) {
        zv0 = z2[i0]; wv0 = w2[i0]; xv0 = x2[i0]; rv0 = r2[i0];
        if (!first) { pv0 = p2[i0]; sv0 = s2[i0]; }
        if (PRECOND) dv0 = d2[i0];
        if (P2P) pr0 = reinterpret_cast<const int2 *>(pd.put_row)[i0];
    }
    double gamma, delta, bsum;
    reduce_partials3(pgamma, pdelta, pbb, first != 0, lds, gamma, delta, bsum);
    if (done) return;
    if (P2P && !ar_inside) {
        // the all-reduce ran in a kernel of its own (pgamma ... hold the reduced values): acknowledgement and the wait
        // for the landing buffers only
        if (blockIdx.x == 0 && t >= 64 && t < 64 + pd.n_nb) store_release_system(pd.ack_ptr[t - 64], seq_ack);
        if (t >= 64 && t < 64 + pd.n_nb && seq_put > 2) wait_ge(&pd.acks[(t - 64) * P2P_FS], seq_put - 2, pd.timeout, pd.d_err, pd.h_err, 5);
        __syncthreads();
        if (__hip_atomic_load(pd.d_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    }
    if (P2P && ar_inside) {
        const int rpar = (int)(seq_red & 1);
        if (blockIdx.x == 0) {
            if (t < pd.P) {
                double *slot = reinterpret_cast<double *>(pd.peer[t] + P2P_OFF_RED_SLOT) + ((size_t)rpar * P2P_MAXR + pd.rank) * P2P_FS;
                store_system(&slot[0], gamma);
                store_system(&slot[1], delta);
                store_system(&slot[2], first ? bsum : 0.0);
                store_release_system(reinterpret_cast<u64 *>(pd.peer[t] + P2P_OFF_RED_FLAG) + ((size_t)rpar * P2P_MAXR + pd.rank) * P2P_FS, seq_red);
            } else if (t >= 64 && t < 64 + pd.n_nb) {
                store_release_system(pd.ack_ptr[t - 64], seq_ack);
            }
        }
        if (t < pd.P)
            wait_ge(reinterpret_cast<const u64 *>(pd.peer[pd.rank] + P2P_OFF_RED_FLAG) + ((size_t)rpar * P2P_MAXR + t) * P2P_FS, seq_red, pd.timeout,
                    pd.d_err, pd.h_err, 1);
        else if (t >= 64 && t < 64 + pd.n_nb && seq_put > 2)
            wait_ge(&pd.acks[(t - 64) * P2P_FS], seq_put - 2, pd.timeout, pd.d_err, pd.h_err, 5);
        __syncthreads();
        if (__hip_atomic_load(pd.d_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
        if (t < 3) {
            const double *slots = reinterpret_cast<const double *>(pd.peer[pd.rank] + P2P_OFF_RED_SLOT) + (size_t)rpar * P2P_MAXR * P2P_FS;
            double v = 0.0;
            for (int q = 0; q < pd.P; ++q) v += load_system(&slots[(size_t)q * P2P_FS + t]);      // rank order on every rank
            red[t] = v;
        }
        __syncthreads();
        gamma = red[0]; delta = red[1]; bsum = red[2];
    }
    const double bb = first ? bsum : bb_saved;
    // check_tol as in cg_p_kernel: 0 fixed iteration count; 1 relative rule gamma / b.b > tol^2; 2 absolute rule of
    // solve_sparse_CG_Jacobi (first test on sqrt(r.z), later ones on r.z).  gamma is the group's sum here -- reduced by
    // the transport (P2P = false), by the exchange above or by the kernel in front (P2P = true) -- the same bits on every
    // rank and in every block: all of them stop at the same iteration.
    bool go = true;
    if (check_tol == 1) go = gamma / bb > tol2;
    else if (check_tol == 2) go = (first ? sqrt(gamma) : gamma) > tol2;
    double beta = 0.0, alpha;
    if (first) {
        alpha = gamma / delta;
    } else {
        beta = gamma / rz_prev;
        alpha = gamma / (delta - beta * gamma / alpha_prev);
    }
    if (blockIdx.x == 0 && t == 0) {
        S->rz_last = gamma;
        if (first) S->bb = bb;
        if (go) { S->rz[parity] = gamma; S->alpha[parity] = alpha; S->pAp = delta; S->iters += 1; }
        else S->done = 1;
    }
    if (!go) return;
    const double na = -alpha;
    const long long ppar = (long long)(seq_put & 1);
    double rz = 0.0;
    // one element of one row: p = z + beta p ; s = w + beta s ; x += alpha p ; r -= alpha s ; z = r .* dinv ; r.z
    auto upd = [&](double zi, double wi, double &pi, double &si, double &xi, double &ri, double di, double &zn, int prow) {
        pi = first ? zi : zi + beta * pi;
        si = first ? wi : wi + beta * si;
        xi = xi + alpha * pi;
        ri = ri + na * si;
        zn = PRECOND ? ri * di : ri;
        rz += ri * zn;
        if (P2P && prow >= 0)
            for (int e = pd.putr_ptr[prow]; e < pd.putr_ptr[prow + 1]; ++e) store_system(pd.putr_addr[e] + ppar * pd.putr_stride[e], zn);
    };
    if (i0 < n2) {                                              // (the prefetched step)
        double2 zn;
        upd(zv0.x, wv0.x, pv0.x, sv0.x, xv0.x, rv0.x, dv0.x, zn.x, pr0.x);
        upd(zv0.y, wv0.y, pv0.y, sv0.y, xv0.y, rv0.y, dv0.y, zn.y, pr0.y);
        p2[i0] = pv0; s2[i0] = sv0; x2[i0] = xv0; r2[i0] = rv0; z2[i0] = zn;
    }
    for (int i = i0 + gridDim.x * KMCF_BLOCK; i < n2; i += gridDim.x * KMCF_BLOCK) {
        const double2 zv = z2[i], wv = w2[i];
        double2 pv = first ? zero : p2[i], sv = first ? zero : s2[i], xv = x2[i], rv = r2[i];
        const double2 dv = PRECOND ? d2[i] : make_double2(1.0, 1.0);
        const int2 pr = P2P ? reinterpret_cast<const int2 *>(pd.put_row)[i] : make_int2(-1, -1);
        double2 zn;
        upd(zv.x, wv.x, pv.x, sv.x, xv.x, rv.x, dv.x, zn.x, pr.x);
        upd(zv.y, wv.y, pv.y, sv.y, xv.y, rv.y, dv.y, zn.y, pr.y);
        p2[i] = pv; s2[i] = sv; x2[i] = xv; r2[i] = rv; z2[i] = zn;
    }
    if ((n & 1) && blockIdx.x == 0 && t == 0) {
        const int i = n - 1;
        double pi = first ? 0.0 : p[i], si = first ? 0.0 : s[i], xi = x[i], ri = r[i], zn;
        upd(z[i], w[i], pi, si, xi, ri, PRECOND ? dinv[i] : 1.0, zn, P2P ? pd.put_row[i] : -1);
        p[i] = pi; s[i] = si; x[i] = xi; r[i] = ri; z[i] = zn;
    }
    const double tsum = kmcf_block_sum(rz, &lds[0][0]);
    if (t == 0) part_rz[blockIdx.x] = tsum;
    if (P2P) {
        // the last block to finish raises the neighbours' flags
        __threadfence_system();
        __syncthreads();
        if (t == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_last = __hip_atomic_fetch_add(pd.ctr, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        }
        __syncthreads();
        if (!s_last) return;
        if (t < pd.n_nb) store_release_system(pd.put_flag[t], seq_put);
        if (t == 0) __hip_atomic_store(pd.ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// 1-block finalize for the multi-rank case: red[0] = gamma, red[1] = delta, red[2] = bb partial (first only)
__global__ __launch_bounds__(KMCF_BLOCK) void cg1_finalize_kernel(part_ref pg, part_ref pd, part_ref pb, int first,
                                                                  kmcf_scalars *__restrict__ S)
{
    __shared__ double lds4[4];
    if (S->done) return;
    double g = reduce_partials(pg, lds4);
    double d = reduce_partials(pd, lds4);
    double b = first ? reduce_partials(pb, lds4) : 0.0;
    if (threadIdx.x == 0) { S->red[0] = g; S->red[1] = d; S->red[2] = b; }
}

kmcf_part4 part4_of(const part_ref &r) { return kmcf_part4{{r.p[0], r.p[1], r.p[2], r.p[3]}, {r.n[0], r.n[1], r.n[2], r.n[3]}}; }

template <bool PRECOND>
struct pcg1_loop : cg_loop_state {
    const part_ref pg_loc = pr1(m->d_part_b, vg), pb_loc = pr1(m->d_part_c, vg), pd_loc = pr_spmv(m);   // gamma, b.b, delta
    const part_ref pg = reduced(pg_loc, 0), pd = reduced(pd_loc, 1), pb = reduced(pb_loc, 2);
    const kmcf_part4 parts[3] = {part4_of(pg_loc), part4_of(pd_loc), part4_of(pb_loc)};   // as kmcf_p2p_allreduce_parts takes them
    // "direct" peer-to-peer protocol: the exchanges ride in the update kernel (fused).  Sequence numbers are counted per
    // LAUNCH in the loop and set back to per EXECUTED exchange after it (kmcf_cgplan.hpp).
    bool fused = false;
    // where the all-reduce of a fused iteration runs: inside the update kernel (every block waits for the P flags: one
    // kernel fewer; right when every rank has a GPU of its own) or in a 1-block kernel in front of it (KMCF_P2P_AR=split:
    // ranks SHARING a GPU -- rehearsals -- otherwise fill it with waiting blocks); bench.py times both and keeps the faster
    bool ar_inside = true;
    bool p2p_red = false;                          // the group's reductions run over the peer-to-peer transport
    u64 red0 = 0, halo0 = 0;

    pcg1_loop(kmcf_matrix *m_, const kmcf_cg_request &q_) : cg_loop_state{m_, q_} {}

    int setup()
    {
        if (m->d_pd) return KMCF_OK;
        KMCF_TRY(kmcf_dev_alloc(&m->d_pd, (size_t)n + 2, false));
        return kmcf_dev_alloc(&m->d_s, (size_t)n + 2, false);
    }

    // r = b - A x0 ; z = r .* dinv (into d_p: the SpMV's input) ; gamma ; b.b
    int residual0()
    {
        cg1_init_kernel<PRECOND><<<vg, KMCF_BLOCK, 0, st>>>(n, m->d_r, m->d_Ap, m->d_dinv, m->d_p, m->d_part_b, m->d_part_c);
        KMCF_HIP(hipGetLastError());
        fused = multi && c->nranks > 1 && kmcf_p2p_direct(m);
        const char *ar = kmcf_opt(c, KNOB_P2P_AR);
        ar_inside = !(ar && strcmp(ar, "split") == 0);
        p2p_red = multi && c->nranks > 1 && c->p2p_active;
        red0 = p2p_red ? kmcf_p2p_red_seq(c) : 0;
        halo0 = fused ? *kmcf_p2p_halo_seq(m, 0) : 0;
        return KMCF_OK;
    }

    template <bool P2P>
    int update(int k, const part_ref &g, const part_ref &d, const part_ref &b, const kmcf_p2p_dev &dev, u64 seq_red, u64 seq_ack, u64 seq_put,
               int ar_in)
    {
        cg1_update_kernel<PRECOND, P2P><<<vg, KMCF_BLOCK, 0, st>>>(n, m->d_x, m->d_r, m->d_pd, m->d_s, m->d_p, m->d_Ap, m->d_dinv, g, d, b, S, k & 1,
                                                                   k == 1 ? 1 : 0, tol2, check_tol, m->d_part_b, dev, seq_red, seq_ack, seq_put, ar_in);
        KMCF_HIP(hipGetLastError());
        if (P2P) *kmcf_p2p_halo_seq(m, 1) = seq_put;                   // the halo of the next SpMV is put
        return KMCF_OK;
    }

    // fused, the all-reduce inside the update kernel, which reads the local partials
    int update_fused(int k)
    {
        const u64 sh = *kmcf_p2p_halo_seq(m, 0), sr = kmcf_p2p_next_red_seq(c);
        return update<true>(k, pg_loc, pd_loc, pb_loc, kmcf_p2p_dev_of(m), sr, sh, sh + 1, 1);
    }

    // fused with KMCF_P2P_AR=split: finalize + exchange in a 1-block kernel of its own, the update kernel reads the sums
    int update_fused_split(int k)
    {
        const u64 sh = *kmcf_p2p_halo_seq(m, 0);
        KMCF_TRY(kmcf_p2p_allreduce_parts(c, parts, 3, S, 1));
        return update<true>(k, pg, pd, pb, kmcf_p2p_dev_of(m), 0, sh, sh + 1, 0);
    }

    // the reduction apart from the update: over peer-to-peer, finalize + exchange in one 1-block kernel (the b.b partials
    // only count in the first iteration: later ones re-send stale ones, which nobody reads); over collectives, a 1-block
    // finalize and the transport's all-reduce; one rank: none, the update kernel sums the partial arrays
    int update_separate(int k)
    {
        if (p2p_red) {
            KMCF_TRY(kmcf_p2p_allreduce_parts(c, parts, 3, S, 1));
        } else if (multi) {
            cg1_finalize_kernel<<<1, KMCF_BLOCK, 0, st>>>(pg_loc, pd_loc, pb_loc, k == 1 ? 1 : 0, S);
            KMCF_HIP(hipGetLastError());
            KMCF_TRY(kmcf_comm_allreduce_sum(c, &S->red[0], 3));
        }
        return update<false>(k, pg, pd, pb, kmcf_p2p_dev{}, 0, 0, 0, 0);
    }

    int iteration(int k)
    {
        KMCF_TRY(kmcf_spmv_device(m, true, true, fused ? 1 : 0));      // w = A z, delta partials
        // (the fused transports named first: cg1_update_kernel<*, true> stays ahead of <*, false> in the code object)
        if (fused) return ar_inside ? update_fused(k) : update_fused_split(k);
        return update_separate(k);
    }

    int after(const kmcf_cg_loop_end &e, kmcf_cg_result *)
    {
        if (p2p_red && !fused) kmcf_p2p_set_red_seq(c, kmcf_cg1_red_seq(red0, e));
        if (fused) {
            const kmcf_cg1_fused_seq s = kmcf_cg1_fused_seq_after(red0, halo0, e);
            kmcf_p2p_set_red_seq(c, s.red);
            *kmcf_p2p_halo_seq(m, 0) = s.halo_consumed;
            *kmcf_p2p_halo_seq(m, 1) = s.halo_put;
            if (s.ack_owed) KMCF_TRY(kmcf_p2p_direct_ack(m, s.halo_consumed, false));
        }
        if (e.done) return KMCF_OK;
        // r.z after the last iteration, for the printed residual
        if (multi) {
            cg_finalize_kernel<<<1, KMCF_BLOCK, 0, st>>>(pg_loc, 0, pr_none(), -1, S, 1);
            KMCF_HIP(hipGetLastError());
            KMCF_TRY(kmcf_comm_allreduce_sum(c, &S->red[0], 1));
        }
        cg_tail_kernel<<<1, KMCF_BLOCK, 0, st>>>(pg, S);
        KMCF_HIP(hipGetLastError());
        return KMCF_OK;
    }
};

static_assert(KMCF_CG_CHUNK_MAX == KMCF_CHUNK_ITERS, "kmcf_cgplan.hpp carries its own copy of the largest chunk");

// The driver.  m->d_r holds b, m->d_x the start guess, m->d_dinv 1/diag; q.x0_in_p: d_p already holds x0 and the
// scalars are zero (the fused input kernel of kmcf_pcg_jacobi wrote both).
template <class REC>
int cg_run_loop(kmcf_matrix *m, const kmcf_cg_request &q, kmcf_solve_stats_t *stats, kmcf_cg_result *res)
{
    REC rec(m, q);
    kmcf_comm *c = rec.c;
    hipStream_t st = rec.st;
    const int limit = q.fixed_iters > 0 ? q.fixed_iters : q.max_it;
    KMCF_TRY(rec.setup());
    if (!q.x0_in_p || rec.n == 0) KMCF_HIP(hipMemsetAsync(rec.S, 0, sizeof(kmcf_scalars), st));
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    // p <- x0 ; Ap = A x0    (:178-186)
    if (!q.x0_in_p) KMCF_HIP(hipMemcpyAsync(m->d_p, m->d_x, (size_t)rec.n * sizeof(double), hipMemcpyDeviceToDevice, st));
    KMCF_TRY(kmcf_spmv_device(m, false, false));
    KMCF_TRY(rec.residual0());
    int launched = 0, cap = kmcf_cg_first_chunk_cap(rec.check_tol != 0);
    bool done = false;
    while (launched < limit && !done) {
        const int chunk = kmcf_cg_next_chunk(cap, limit - launched);
        for (int i = 0; i < chunk; ++i) KMCF_TRY(rec.iteration(launched + i + 1));
        launched += chunk;
        if (rec.check_tol) KMCF_TRY(cg_chunk_check(c, rec.S, st, &done));
    }
    KMCF_TRY(rec.after(kmcf_cg_loop_end{done, done ? c->h_pinned[1] : 0, launched}, res));
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    if (q.caller_collects) return KMCF_OK;         // the caller's output kernel writes the scalars to the host
    KMCF_HIP(hipMemcpyAsync(c->h_scal, rec.S, sizeof(kmcf_scalars), hipMemcpyDeviceToHost, st));
    return pcg_collect(m, rec.tol2, q.call == KMCF_CG_CALL_ABSOLUTE, stats);
}

}  // namespace

// A recurrence as ONE register-resident launch (kmcf_cgr.hip), for matrices whose tiles are all resident at once.
// Workspace in, workspace out (or q.b_src / q.x_user in their place), scalars in d_S -- like the loops.
static int pcg_resident(kmcf_matrix *m, const kmcf_cg_request &q, kmcf_solve_stats_t *stats, bool classic)
{
    kmcf_comm *c = m->comm;
    hipStream_t st = c->stream;
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    KMCF_TRY(kmcf_cgr_solve(m, q.precond, q.tol, q.max_it, q.fixed_iters, classic, q.b_src, q.x_user));
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    if (q.caller_collects) return KMCF_OK;         // the caller's output kernel writes the scalars to the host
    KMCF_HIP(hipMemcpyAsync(c->h_scal, m->d_S, sizeof(kmcf_scalars), hipMemcpyDeviceToHost, st));
    return pcg_collect(m, q.tol * q.tol, 0, stats);
}

static kmcf_cg_path cg_path(kmcf_matrix *m, kmcf_cg_call call, bool has_limit)
{
    const kmcf_comm *c = m->comm;
    return kmcf_cg_choose_path(call, c->nranks > 1 || c->force_collectives, kmcf_cg_single_reduction(m), kmcf_cgr_classic_applies(m),
                               has_limit, [m] { return kmcf_cgr_usable(m); });
}

bool kmcf_pcg_resident_applies(kmcf_matrix *m)
{
    const kmcf_comm *c = m->comm;
    return kmcf_cg_resident_applies(c->nranks > 1 || c->force_collectives, kmcf_cg_single_reduction(m), kmcf_cgr_classic_applies(m),
                                    [m] { return kmcf_cgr_usable(m); });
}

// The one entry of every solve on the matrix workspace; the path is decided here and nowhere else (the table:
// kmcf_cgplan.hpp).
int kmcf_cg_solve(kmcf_matrix *m, const kmcf_cg_request &q, kmcf_solve_stats_t *stats, kmcf_cg_result *res)
{
    kmcf_comm *c = m->comm;
    KMCF_TRY(kmcf_group_rendezvous(c));                   // (in-process test groups: see kmcf_internal.hpp)
    c->in_solve = true;
    struct leave_t { kmcf_comm *c; ~leave_t() { c->in_solve = false; } } leave{c};
    const kmcf_cg_path path = cg_path(m, q.call, q.fixed_iters > 0 || q.max_it > 0);
    // (a group's resident plan compares the ranks' group options: a difference found there is reported by every solve)
    if (q.call == KMCF_CG_CALL_RESIDENT_OK && (path == KMCF_CG_RESIDENT_CG1R || path == KMCF_CG_LOOP_CG1R)) KMCF_TRY(kmcf_cgr_agreed(m));
    if (res) *res = kmcf_cg_result{path, {}};
    if (kmcf_cg_is_resident(path)) return pcg_resident(m, q, stats, path == KMCF_CG_RESIDENT_CLASSIC);
    KMCF_CHECK(!q.x_user && !q.b_src, KMCF_ERR_STATE, "solve set up for a resident launch that does not apply");
    int rc = KMCF_OK;
    // (cg1r ahead of classic, a with_bools each: the kernels' template instances come out in the code object in the
    //  order of their first use here, and this order keeps the object what it was)
    if (path == KMCF_CG_LOOP_CG1R)
        with_bools([&](auto precond) { rc = cg_run_loop<pcg1_loop<decltype(precond)::value>>(m, q, stats, res); }, q.precond);
    else
        with_bools([&](auto precond) { rc = cg_run_loop<pcg_loop<decltype(precond)::value>>(m, q, stats, res); }, q.precond);
    return rc;
}

int kmcf_pcg_workspace(kmcf_matrix *m, bool precond, double tol, int max_it, int fixed_iters, kmcf_solve_stats_t *stats,
                       const double *b_src, double *x_user)
{
    return kmcf_cg_solve(m, kmcf_cg_request{KMCF_CG_CALL_RESIDENT_OK, precond, tol, max_it, fixed_iters, false, false, b_src, x_user}, stats);
}

namespace {

// computeDiagonalInvSqrt, src/iterative_solvers_gpu.cu:630-652
__global__ __launch_bounds__(KMCF_BLOCK) void diag_inv_sqrt_kernel(int n, const int *__restrict__ row_ptr,
                                                                   const int *__restrict__ col, const double *__restrict__ val,
                                                                   double *__restrict__ dis)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        double d = 0.0;
        for (int j = row_ptr[i]; j < row_ptr[i + 1]; ++j)
            if (col[j] == i) { d = val[j]; break; }
        dis[i] = 1.0 / sqrt(d);
    }
}

// jacobi_precondition_matrix, :666-680 (16 lanes per row here)
__global__ __launch_bounds__(KMCF_BLOCK) void scale_matrix_kernel(int n, const int *__restrict__ row_ptr,
                                                                  const int *__restrict__ col, double *__restrict__ val,
                                                                  const double *__restrict__ dis)
{
    constexpr int LPR = 16, RPB = KMCF_BLOCK / LPR;
    const int lane = threadIdx.x % LPR;
    for (int r = blockIdx.x * RPB + threadIdx.x / LPR; r < n; r += gridDim.x * RPB)
        for (int j = row_ptr[r] + lane; j < row_ptr[r + 1]; j += LPR) val[j] = val[j] * dis[r] * dis[col[j]];
}

// The same scaling for the rows of one rank of a group: a_ij * s_i * s_j with s_j the rank's own 1/sqrt(diag) for an own
// column and the neighbour's -- landed in the halo slot by the matrix's halo exchange -- for a halo column.  16 lanes per
// row like the other row walks; every entry is written by exactly one lane.
__global__ __launch_bounds__(KMCF_BLOCK) void scale_matrix_halo_kernel(int n, const int *__restrict__ row_ptr,
                                                                       const int *__restrict__ col, double *__restrict__ val,
                                                                       const double *__restrict__ dis,
                                                                       const double *__restrict__ dis_halo)
{
    constexpr int LPR = 16, RPB = KMCF_BLOCK / LPR;
    const int lane = threadIdx.x % LPR;
    for (int r = blockIdx.x * RPB + threadIdx.x / LPR; r < n; r += gridDim.x * RPB) {
        const double si = dis[r];
        for (int j = row_ptr[r] + lane; j < row_ptr[r + 1]; j += LPR) {
            const int cj = col[j];
            val[j] = val[j] * si * (cj < n ? dis[cj] : dis_halo[cj - n]);
        }
    }
}

// jacobi_precondition_array :654-664 (mode 0) / jacobi_unprecondition_array :682-692 (mode 1)
__global__ __launch_bounds__(KMCF_BLOCK) void scale_vector_kernel(int n, double *__restrict__ a, const double *__restrict__ dis, int mode)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        a[i] = mode ? a[i] * 1 / dis[i] : a[i] * dis[i];
}

}  // namespace

// solve_sparse_CG_Jacobi on the workspace: m->d_r = rhs, m->d_x = start guess (internal order).
// Scales A (in place), rhs and the guess, solves, un-scales the solution into m->d_x.  If d_rhs_user is
// given, the scaled rhs is written back to it (the reference scales the caller's rhs in place, :740).
// A rank group: every rank scales its own rows; the column scale of a halo entry is the neighbour's 1/sqrt(diag), fetched
// by ONE halo exchange of that vector (through d_p, like the halo of an SpMV) before the values are touched.
int kmcf_scaled_cg_workspace(kmcf_matrix *m, double tol, int max_iterations, double *d_rhs_user, kmcf_solve_stats_t *stats)
{
    kmcf_comm *c = m->comm;
    const int n = m->n_loc;
    const int g = kmcf_vec_grid(n);
    double *dis = m->d_dinv;  // workspace: 1/sqrt(diag)
    diag_inv_sqrt_kernel<<<g, KMCF_BLOCK, 0, c->stream>>>(n, m->d_row_ptr, m->d_col, m->d_val, dis);
    scale_vector_kernel<<<g, KMCF_BLOCK, 0, c->stream>>>(n, m->d_r, dis, 0);      // rhs scaled (:740)
    if (c->nranks > 1 || c->force_collectives) {
        KMCF_HIP(hipGetLastError());
        KMCF_HIP(hipMemcpyAsync(m->d_p, dis, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        KMCF_TRY(kmcf_group_rendezvous(c));
        KMCF_TRY(kmcf_halo_exchange_begin(m));
        if (m->n_halo > 0 || m->n_send > 0) KMCF_TRY(kmcf_halo_exchange_end(m));
        scale_matrix_halo_kernel<<<g * 4, KMCF_BLOCK, 0, c->stream>>>(n, m->d_row_ptr, m->d_col, m->d_val, dis, m->d_p + n);
    } else
        scale_matrix_kernel<<<g * 4, KMCF_BLOCK, 0, c->stream>>>(n, m->d_row_ptr, m->d_col, m->d_val, dis);  // :745
    scale_vector_kernel<<<g, KMCF_BLOCK, 0, c->stream>>>(n, m->d_x, dis, 1);      // start guess (:751)
    KMCF_HIP(hipGetLastError());
    kmcf_values_changed(m);       // the SpMV reads d_val from here on (or the f64 row-per-lane stream refreshed from it)
    if (d_rhs_user) KMCF_TRY(kmcf_vec_out(m, d_rhs_user, m->d_r));
    // plain CG on the scaled system; the reference carries r = A y - b and p = -r (:826-836),
    // the same iterates as r = b - A y, p = r used here.  The unpreconditioned loop never
    // touches d_dinv, so `dis` stays intact.  (The absolute rule as a loop of kernels, never the resident launch: the
    // system in the matrix is not the one a resident plan of m was made for, and that plan and its buffers are not touched.)
    KMCF_TRY(kmcf_cg_solve(m, kmcf_cg_request{KMCF_CG_CALL_ABSOLUTE, false, std::sqrt(tol * tol), max_iterations, 0}, stats));
    scale_vector_kernel<<<g, KMCF_BLOCK, 0, c->stream>>>(n, m->d_x, dis, 0);      // y = D^-1/2 y' (:864)
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// The same solve with the matrix left as it is.  CG on A' = D^-1/2 A D^-1/2, b' = D^-1/2 b is Jacobi-PCG on A, b term by
// term: with y' = D^1/2 y one has r' = D^-1/2 r, hence r'.r' = r.(D^-1 r) = r.z, p' = D^1/2 p, p'.A'p' = p.Ap -- the same
// alpha, beta and stopping quantity (the absolute rule of :838-858 read on r.z), and D^-1/2 y' = y is what the loop
// already holds.  What this buys: A keeps its value codes, so every iteration runs the coded row-per-lane SpMV (2 B per
// entry) instead of the f64 one (10 B), and the four scaling passes go away.  Differences to the scaled form are
// rounding only (a_ij (s_j p'_j) s_i against a_ij p_j); callers whose A is visible to the user keep the scaled form.
// m->d_dinv = 1/diag on entry.
int kmcf_jacobi_cg_workspace_absolute(kmcf_matrix *m, double tol, int max_iterations, kmcf_solve_stats_t *stats)
{
    return kmcf_cg_solve(m, kmcf_cg_request{KMCF_CG_CALL_ABSOLUTE, true, tol, max_iterations, 0}, stats);
}

int kmcf_pcg_workspace_loop(kmcf_matrix *m, double tol, int max_it, kmcf_solve_stats_t *stats)
{
    return kmcf_cg_solve(m, kmcf_cg_request{KMCF_CG_CALL_LOOP_ONLY, true, tol, max_it, 0}, stats);
}

extern "C" int kmcf_solve_sparse_CG_Jacobi(kmcf_matrix *m, double *d_rhs, double *d_x, double tol, int max_iterations,
                                           kmcf_solve_stats_t *stats)
{
    KMCF_CHECK(m && d_rhs && d_x, KMCF_ERR_ARG, "kmcf_solve_sparse_CG_Jacobi: null argument");
    KMCF_CHECK(m->d_val, KMCF_ERR_STATE, "kmcf_solve_sparse_CG_Jacobi: host-only matrix");
    kmcf_comm *c = m->comm;
    KMCF_CHECK(c->nranks == 1 || c->connected, KMCF_ERR_COMM, "kmcf_solve_sparse_CG_Jacobi: communicator not connected");
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(kmcf_vec_in(m, m->d_r, d_rhs));
    KMCF_TRY(kmcf_vec_in(m, m->d_x, d_x));
    KMCF_TRY(kmcf_scaled_cg_workspace(m, tol, max_iterations, d_rhs, stats));
    KMCF_TRY(kmcf_vec_out(m, d_x, m->d_x));
    KMCF_HIP(hipStreamSynchronize(c->stream));
    return kmcf_p2p_check(c);
}

namespace {
// The caller's r, x and 1/diag into the (internally ordered, aligned) workspace in ONE pass; p <- x0 on the way.
// The permutation between the caller's row order and the internal one is local at the scale of a slab of bricks
// (tens of thousands of rows), not of a cache line: consecutive internal rows sit 8 bytes apart in lines whose
// other 56 bytes belong to other bricks of the same slab.  Each XCD therefore takes one contiguous eighth of the
// internal rows (blockIdx & 7 = XCD, as in the SpMV kernels): the lines of a slab are fetched into ONE L2 and reused
// there, instead of into all eight (measured 44 -> 34.5 us in, 32 -> 22.4 us out at 40 nm).
__device__ __forceinline__ void xcd_range(int n, int &first, int &end, int &stride)
{
    const int xcd = blockIdx.x & 7, bi = blockIdx.x >> 3, nb8 = gridDim.x >> 3;
    const int per = (n + 7) >> 3;
    first = min(n, xcd * per) + bi * KMCF_BLOCK + threadIdx.x;
    end = min(n, (xcd + 1) * per);
    stride = nb8 * KMCF_BLOCK;
}

__global__ __launch_bounds__(KMCF_BLOCK) void cg_in_kernel(int n, const int *__restrict__ perm, const double *__restrict__ r_u,
                                                           const double *__restrict__ x_u, const double *__restrict__ dinv_u,
                                                           double *__restrict__ r, double *__restrict__ x, double *__restrict__ p,
                                                           double *__restrict__ dinv, kmcf_scalars *__restrict__ S)
{
    // the solve's scalars start at zero (a memset of its own between this kernel and the first SpMV cost ~10 us of stream time)
    if (blockIdx.x == 0 && threadIdx.x < sizeof(kmcf_scalars) / sizeof(int)) reinterpret_cast<int *>(S)[threadIdx.x] = 0;
    int first, end, stride;
    xcd_range(n, first, end, stride);
    for (int i = first; i < end; i += stride) {
        const int s = perm ? perm[i] : i;
        const double xv = x_u[s];
        r[i] = r_u[s];
        x[i] = xv;
        p[i] = xv;
        if (dinv_u) dinv[i] = dinv_u[s];
    }
}
__global__ __launch_bounds__(KMCF_BLOCK) void cg_out_kernel(int n, const int *__restrict__ perm, const double *__restrict__ r,
                                                            const double *__restrict__ x, kmcf_xring ring,
                                                            double *__restrict__ r_u, double *__restrict__ x_u,
                                                            const kmcf_scalars *__restrict__ S, kmcf_scalars *__restrict__ host_S,
                                                            part_ref tail_rz)
{
    __shared__ double lds4[4];
    // the solve's scalars straight into pinned host memory: a 120-byte hipMemcpyAsync costs tens of microseconds.
    // tail_rz (classic loop of one rank that ended on its iteration limit): the loop condition's last r.z (:217, :273) is
    // the sum of these partials -- formed here by block 0 exactly as cg_tail_kernel forms it, instead of in a launch of its own
    if (host_S && blockIdx.x == 0) {
        const bool tail = tail_rz.n[0] > 0 && !S->done;
        const double t = tail ? reduce_partials(tail_rz, lds4) : 0.0;       // (block-uniform branch)
        if (threadIdx.x == 0) {
            kmcf_scalars h = *S;
            if (tail) h.rz_last = t;
            *host_S = h;
        }
    }
    // a loop that ended on its iteration limit has left its last x += alpha p to this kernel (cg_p_kernel): up to
    // KMCF_CG_XBATCH of them, applied oldest first from the p ring
    const int pending = S->done ? 0 : S->x_pending;
    double a[4];
    xring_steps(ring, S, a);
    int first, end, stride;
    xcd_range(n, first, end, stride);
    for (int i = first; i < end; i += stride) {
        const int s = perm ? perm[i] : i;
        r_u[s] = r[i];
        double xv = x[i];
        if (pending) xring_apply1(xv, ring, a, pending, i);
        x_u[s] = xv;
    }
}
inline int perm_grid(int n) { return (kmcf_vec_grid(n) + 7) / 8 * 8; }
}  // namespace

extern "C" int kmcf_pcg_jacobi(kmcf_matrix *m, double *d_r, double *d_x, const double *d_diag_inv,
                               double relative_tolerance, int max_iterations, int fixed_iters,
                               kmcf_solve_stats_t *stats)
{
    KMCF_CHECK(m && ((d_r && d_x) || m->n_loc == 0), KMCF_ERR_ARG, "kmcf_pcg_jacobi: null argument");
    KMCF_CHECK(m->d_val, KMCF_ERR_STATE, "kmcf_pcg_jacobi: host-only matrix");
    KMCF_CHECK(max_iterations >= 0 && fixed_iters >= 0, KMCF_ERR_ARG, "kmcf_pcg_jacobi: negative iteration count");
    kmcf_comm *c = m->comm;
    KMCF_CHECK(c->connected, KMCF_ERR_COMM, "kmcf_pcg_jacobi: communicator not connected");
    const bool trace = kmcf_trace(c);
    auto now = [] { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_0 = trace ? now() : 0.0;
    KMCF_TRY(kmcf_enter(c));
    // the caller's vectors may be unaligned slices (x is gpubuf.site_potential_boundary +
    // N_left + disp, src/potential_solver_gpu.cu:861) and are in the caller's row order: work on
    // the aligned, internally ordered workspace
    // one pass in, one pass out, ONE host synchronisation at the end of the whole call (a fixed-iteration solve
    // -- the benchmark's step -- otherwise pays three input kernels, a copy, two output kernels and two syncs)
    const int n = m->n_loc;
    const double t_a = trace ? now() : 0.0;
    KMCF_HIP(hipEventRecord(c->ev_call0, c->stream));
    if (n > 0) {
        cg_in_kernel<<<perm_grid(n), KMCF_BLOCK, 0, c->stream>>>(n, m->d_perm, d_r, d_x, d_diag_inv, m->d_r, m->d_x, m->d_p, m->d_dinv, m->d_S);
        KMCF_HIP(hipGetLastError());
    }
    kmcf_cg_request q{KMCF_CG_CALL_RESIDENT_OK, d_diag_inv != nullptr, relative_tolerance, max_iterations, fixed_iters};
    q.x0_in_p = q.caller_collects = true;
    kmcf_cg_result solved{};
    KMCF_TRY(kmcf_cg_solve(m, q, stats, &solved));
    const double t_b = trace ? now() : 0.0;
    const bool tail_here = kmcf_cg_tail_in_output(solved.path, c->nranks > 1 || c->force_collectives, n);
    cg_out_kernel<<<perm_grid(std::max(n, 1)), KMCF_BLOCK, 0, c->stream>>>(n, m->d_perm, m->d_r, m->d_x, solved.xring, d_r, d_x, m->d_S, c->h_scal,
                                                                           tail_here ? pr1(m->d_part_b, kmcf_vec_grid(n)) : pr_none());
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipEventRecord(c->ev_call1, c->stream));
    // results visible on return (:271 hipDeviceSynchronize)
    const int rc = pcg_collect(m, relative_tolerance * relative_tolerance, 0, stats, false);
    if (rc == KMCF_OK && stats) {
        // device time of everything this call enqueued: vectors in, r = b - A x0, the iterations, vectors out
        float ms = 0.f;
        KMCF_HIP(hipEventSynchronize(c->ev_call1));
        KMCF_HIP(hipEventElapsedTime(&ms, c->ev_call0, c->ev_call1));
        stats->ms_solve = ms;
    }
    if (trace) {
        const double t_c = now();
        fprintf(stderr, "kmcf_pcg_jacobi trace: enter %.1f us, enqueue %.1f us, wait %.1f us, total %.1f us, device %.1f us\n", t_a - t_0,
                t_b - t_a, t_c - t_b, t_c - t_0, stats ? stats->ms_solve * 1e3 : 0.0);
    }
    return rc;
}

namespace {
__global__ __launch_bounds__(KMCF_BLOCK) void perm_in_kernel(int n, double *__restrict__ dst, const double *__restrict__ src,
                                                             const int *__restrict__ perm)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = src[perm[i]];
}
__global__ __launch_bounds__(KMCF_BLOCK) void perm_out_kernel(int n, double *__restrict__ dst, const double *__restrict__ src,
                                                              const int *__restrict__ perm)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[perm[i]] = src[i];
}
}  // namespace

int kmcf_vec_in(kmcf_matrix *m, double *d_internal, const double *d_user)
{
    const int n = m->n_loc;
    if (n == 0) return KMCF_OK;
    if (!m->d_perm) {
        KMCF_HIP(hipMemcpyAsync(d_internal, d_user, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, m->comm->stream));
    } else {
        perm_in_kernel<<<kmcf_vec_grid(n), KMCF_BLOCK, 0, m->comm->stream>>>(n, d_internal, d_user, m->d_perm);
        KMCF_HIP(hipGetLastError());
    }
    return KMCF_OK;
}

int kmcf_vec_out(kmcf_matrix *m, double *d_user, const double *d_internal)
{
    const int n = m->n_loc;
    if (n == 0) return KMCF_OK;
    if (!m->d_perm) {
        KMCF_HIP(hipMemcpyAsync(d_user, d_internal, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, m->comm->stream));
    } else {
        perm_out_kernel<<<kmcf_vec_grid(n), KMCF_BLOCK, 0, m->comm->stream>>>(n, d_user, d_internal, m->d_perm);
        KMCF_HIP(hipGetLastError());
    }
    return KMCF_OK;
}
