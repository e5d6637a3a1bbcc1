// Local heat solve: site temperatures from the dissipated power (the solve_heating_local branch of
// Device::updateTemperature, src/heat_solver.cpp:76-98).
//
// The reference multiplies a dense N_interface x N_interface operator that nothing builds (constructLaplacian,
// src/Device.h:195, has no definition; 10.7 GB at 5 nm).  Here the operator is the graph Laplacian of pair
// conductances on K's pattern, contacts held at background_temp ("Local heat solve"):
//   (C/dt + sum_j g_ij + gL_i + gR_i) T_i - sum_j g_ij T_j = (C/dt) T_old_i + Q_i + (gL_i + gR_i) T0
// g = k_th * L_char with k_th by pair class (metal-metal, vacancy-vacancy, other); without the C/dt terms in the
// steady state.  The system is assembled into K's storage (values, value codes, diag, 1/diag, rhs) in one pass over the
// local rows, exactly as the K assembly writes K, and solved by the kernel-loop Jacobi-PCG; the next K assembly refills
// everything the heat assembly wrote.
#include <cmath>

#include "kmcf_internal.hpp"

namespace {

// pair class: 0 both metal, 1 both uncharged vacancies, 2 any other pair (site classes of site_class_kernel:
// bit 0 metal, bit 1 uncharged vacancy)
__device__ __forceinline__ int heat_class(unsigned char ci, unsigned char cj)
{
    const unsigned char b = ci & cj;
    return (b & 1) ? 0 : ((b & 2) ? 1 : 2);
}

// per-class entry counts, three 21-bit fields in one word (row lengths are far below 2^21)
constexpr int HC_BITS = 21;
__device__ __forceinline__ unsigned long long hc_one(int cls) { return 1ull << (HC_BITS * cls); }
__device__ __forceinline__ double hc_sum(unsigned long long n, const double g[3])
{
    constexpr unsigned long long M = (1ull << HC_BITS) - 1;
    return (double)(n & M) * g[0] + (double)((n >> HC_BITS) & M) * g[1] + (double)((n >> (2 * HC_BITS)) & M) * g[2];
}

// v[k] for a runtime k without indexing the (kernel-argument) array dynamically
template <class T>
__device__ __forceinline__ T sel3(const T (&v)[3], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }

struct heat_args {
    int n_loc, row_site0 /* N_left + displ */, n_left, n_interface;
    const int *row_ptr, *col, *diag_pos, *perm /* internal -> caller local row, or nullptr */;
    const int *left_row_ptr, *left_col, *right_row_ptr, *right_col;
    const unsigned char *cls, *cls_col;
    double g[3];             // pair conductance by class [W/K]
    double dv[3];            // matrix value of each class's entries (-g)
    int code[3];             // dictionary code of each class
    double vc[3];            // value of each dictionary code (0.0 beyond the dictionary)
    double cdt, T0;          // C/dt (0: steady state), contact temperature
    const double *T_old, *Q; // caller's site arrays (N)
    double *val, *diag_out, *left_out, *right_out, *dinv_out, *rhs_out;
    unsigned short *idx16;   // window SpMV: value codes above the slot bits, or nullptr
    double *diagv;           // window SpMV: diagonal per row, or nullptr
};

// diag, 1/diag and rhs of one row from its class counts: sums of integer counts times g, independent of the lane order
// and of the rank count (as the K assembly's)
__device__ __forceinline__ double heat_row_finish(const heat_args &a, int r, int ru, int dpos, unsigned long long cn,
                                                  unsigned long long cl, unsigned long long cr)
{
    const double d = hc_sum(cn, a.g), gl = hc_sum(cl, a.g), gr = hc_sum(cr, a.g);
    const double tot = a.cdt + d + gl + gr;
    const int site = a.row_site0 + ru;
    const double told = a.cdt != 0.0 ? a.cdt * a.T_old[site] : 0.0;
    if (a.diagv) a.diagv[r] = dpos >= 0 ? tot : 0.0;
    a.diag_out[r] = tot;
    a.left_out[r] = gl;
    a.right_out[r] = gr;
    a.dinv_out[r] = 1.0 / tot;
    a.rhs_out[r] = told + a.Q[site] + (gl + gr) * a.T0;
    return tot;
}

// One pass per row (LPR lanes), the layout-agnostic form (k_assemble_kernel's walk).
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void heat_assemble_kernel(const heat_args a)
{
    constexpr int SLOT_MASK = (1 << KMCF_SLOT_BITS) - 1;
    constexpr int RPB = KMCF_BLOCK / LPR;
    const int lane = threadIdx.x % LPR;
    const int groups = (a.n_loc + RPB - 1) / RPB;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int r = grp * RPB + threadIdx.x / LPR;
        const bool valid = r < a.n_loc;
        unsigned long long cn = 0, cl = 0, cr = 0;
        int dpos = -1, ru = 0;
        if (valid) {
            ru = a.perm ? a.perm[r] : r;
            const unsigned char ci = a.cls_col[r];
            dpos = a.diag_pos[r];
            for (int j = a.row_ptr[r] + lane; j < a.row_ptr[r + 1]; j += LPR) {
                if (j == dpos) continue;
                const int k = heat_class(ci, a.cls_col[a.col[j]]);
                a.val[j] = sel3(a.dv, k);
                if (a.idx16) a.idx16[j] = (unsigned short)((a.idx16[j] & SLOT_MASK) | (sel3(a.code, k) << KMCF_SLOT_BITS));
                cn += hc_one(k);
            }
            for (int j = a.left_row_ptr[ru] + lane; j < a.left_row_ptr[ru + 1]; j += LPR)
                cl += hc_one(heat_class(ci, a.cls[a.left_col[j]]));
            for (int j = a.right_row_ptr[ru] + lane; j < a.right_row_ptr[ru + 1]; j += LPR)
                cr += hc_one(heat_class(ci, a.cls[a.n_left + a.n_interface + a.right_col[j]]));
        }
#pragma unroll
        for (int off = LPR / 2; off >= 1; off >>= 1) {
            cn += __shfl_xor(cn, off, 64);
            cl += __shfl_xor(cl, off, 64);
            cr += __shfl_xor(cr, off, 64);
        }
        if (valid && lane == 0) {
            const double tot = heat_row_finish(a, r, ru, dpos, cn, cl, cr);
            if (dpos >= 0) {
                a.val[dpos] = tot;
                if (a.idx16) a.idx16[dpos] = (unsigned short)((a.idx16[dpos] & SLOT_MASK) | (KMCF_CODE_DIAG << KMCF_SLOT_BITS));
            }
        }
    }
}

// The same over the tiles of the window SpMV, for matrices planned for the coded kernel (k_assemble_tile_kernel's walk:
// a tile's slot stream in as one 16-byte load per lane, the classes of its window columns in LDS, codes and values out
// as 16- and 64-byte pieces per lane).
__global__ __launch_bounds__(KMCF_BLOCK) void heat_assemble_tile_kernel(const heat_args a, int n_tiles, const int2 *__restrict__ tile,
                                                                       const int *__restrict__ wcol)
{
    constexpr int U = 8, LPR = 4, SLOT_MASK = (1 << KMCF_SLOT_BITS) - 1;   // KMCF_BLOCK / LPR = 64 rows per pass
    typedef unsigned int pack_t __attribute__((ext_vector_type(U / 2)));
    __shared__ unsigned char wcls[1 << KMCF_SLOT_BITS];
    __shared__ pack_t sidx_pk[KMCF_BLOCK];
    const int tid = threadIdx.x, lane = tid % LPR;
    unsigned short *sib = reinterpret_cast<unsigned short *>(sidx_pk);
    unsigned short *idx16 = a.idx16;
    for (int c = blockIdx.x; c < n_tiles; c += gridDim.x) {
        const int2 t0 = tile[c], t1 = tile[c + 1];
        const int r0 = t0.x, r1 = t1.x, w0 = t0.y, W = t1.y - w0;
        const int base = a.row_ptr[r0], cnt = a.row_ptr[r1] - base;
        const int abase = base & ~(U - 1);                 // aligned start of the block-wide slot load
        for (int w = tid; w < W; w += KMCF_BLOCK) wcls[w] = a.cls_col[wcol[w0 + w]];
        sidx_pk[tid] = *reinterpret_cast<const pack_t *>(idx16 + abase + U * tid);
        __syncthreads();
        double tot = 0.0;
        int dpos = -1;
        {                                                  // tiles of this plan hold at most RPP rows: one pass
            const int r = r0 + tid / LPR;
            const bool valid = r < r1;
            unsigned long long cn = 0, cl = 0, cr = 0;
            int ru = 0;
            if (valid) {
                ru = a.perm ? a.perm[r] : r;
                const unsigned char ci = a.cls_col[r];
                dpos = a.diag_pos[r];
                for (int j = a.row_ptr[r] + lane; j < a.row_ptr[r + 1]; j += LPR) {
                    const int q = j - abase;
                    const int slot = sib[q] & SLOT_MASK;
                    if (j == dpos) { sib[q] = (unsigned short)(slot | (KMCF_CODE_DIAG << KMCF_SLOT_BITS)); continue; }
                    const int k = heat_class(ci, wcls[slot]);
                    sib[q] = (unsigned short)(slot | (sel3(a.code, k) << KMCF_SLOT_BITS));
                    cn += hc_one(k);
                }
                for (int j = a.left_row_ptr[ru] + lane; j < a.left_row_ptr[ru + 1]; j += LPR)
                    cl += hc_one(heat_class(ci, a.cls[a.left_col[j]]));
                for (int j = a.right_row_ptr[ru] + lane; j < a.right_row_ptr[ru + 1]; j += LPR)
                    cr += hc_one(heat_class(ci, a.cls[a.n_left + a.n_interface + a.right_col[j]]));
            }
#pragma unroll
            for (int off = LPR / 2; off >= 1; off >>= 1) {
                cn += __shfl_xor(cn, off, 64);
                cl += __shfl_xor(cl, off, 64);
                cr += __shfl_xor(cr, off, 64);
            }
            if (valid && lane == 0) tot = heat_row_finish(a, r, ru, dpos, cn, cl, cr);
            else dpos = -1;
        }
        __syncthreads();
        // codes and values back to global memory: lane t owns entries abase + 8 t .. + 7; the first and last lanes of a
        // tile share that range with the neighbouring tiles and write entry-wise.  Diagonal entries get a placeholder
        // here and their value after the barrier.  Codes below KMCF_CODE_DIAG index the dictionary (a.dv by code).
        {
            const int q0 = U * tid, lo = base - abase, hi = lo + cnt;
            if (q0 + U > lo && q0 < hi) {
                const pack_t pk = sidx_pk[tid];
                const unsigned short *e = reinterpret_cast<const unsigned short *>(&pk);
                auto value = [&](unsigned short s) { return sel3(a.vc, s >> KMCF_SLOT_BITS); };
                if (q0 >= lo && q0 + U <= hi) {
                    *reinterpret_cast<pack_t *>(idx16 + abase + q0) = pk;
                    double v[U];
#pragma unroll
                    for (int k = 0; k < U; ++k) v[k] = value(e[k]);
                    double4 *vp = reinterpret_cast<double4 *>(a.val + abase + q0);
                    vp[0] = make_double4(v[0], v[1], v[2], v[3]);
                    vp[1] = make_double4(v[4], v[5], v[6], v[7]);
                } else {
                    for (int k = 0; k < U; ++k) {
                        const int q = q0 + k;
                        if (q < lo || q >= hi) continue;
                        idx16[abase + q] = e[k];
                        a.val[abase + q] = value(e[k]);
                    }
                }
            }
        }
        __syncthreads();                                   // orders the placeholder before the value; frees LDS
        if (lane == 0 && dpos >= 0) a.val[dpos] = tot;
    }
}

// contact sites at T0 (the interface rows are the solve's)
__global__ __launch_bounds__(KMCF_BLOCK) void heat_contacts_kernel(double *__restrict__ T, int N, int n_left, int n_interface, double T0)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        if (i < n_left || i >= n_left + n_interface) T[i] = T0;
}

// sum of T over [first, first + n): per-block partials, then one block adds them into part[0]
__global__ __launch_bounds__(KMCF_BLOCK) void tsum_partial_kernel(const double *__restrict__ T, int first, int n, double *__restrict__ part)
{
    __shared__ double lds4[4];
    double s = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += T[first + i];
    const double t = kmcf_block_sum(s, lds4);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ __launch_bounds__(KMCF_BLOCK) void tsum_final_kernel(double *__restrict__ part, int npart)
{
    __shared__ double lds4[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < npart; i += KMCF_BLOCK) s += part[i];
    const double t = kmcf_block_sum(s, lds4);        // (every lane has read its partials before the block's first barrier)
    if (threadIdx.x == 0) part[0] = t;
}

bool positive(double v) { return v > 0.0 && std::isfinite(v); }

}  // namespace

extern "C" int kmcf_update_temperature_local(kmcf_kstate *k, const int *d_site_element, const int *d_site_charge,
                                             const int *d_metals, int num_metals, const double *d_site_power,
                                             double *d_site_temperature, int N, int N_left_tot, int N_right_tot,
                                             double step_time, const kmcf_heat_params_t *p, double *h_T_bg,
                                             int *h_steady, kmcf_solve_stats_t *stats)
{
    KMCF_CHECK(k && d_site_element && d_site_charge && d_metals && d_site_power && d_site_temperature && p, KMCF_ERR_ARG,
               "kmcf_update_temperature_local: null argument");
    KMCF_CHECK(N == k->N && N_left_tot == k->N_left && N_right_tot == k->N_right, KMCF_ERR_ARG,
               "kmcf_update_temperature_local: N/N_left/N_right (%d,%d,%d) differ from the pattern's (%d,%d,%d)",
               N, N_left_tot, N_right_tot, k->N, k->N_left, k->N_right);
    KMCF_CHECK(num_metals >= 0, KMCF_ERR_ARG, "kmcf_update_temperature_local: num_metals = %d", num_metals);
    const struct { const char *name; double v; } pos[] = {
        {"k_th_metal", p->k_th_metal}, {"k_th_vacancies", p->k_th_vacancies}, {"k_th_non_vacancy", p->k_th_non_vacancy},
        {"L_char", p->L_char}, {"c_p", p->c_p}, {"A", p->A}, {"t_ox", p->t_ox}, {"delta_t", p->delta_t}};
    for (const auto &q : pos)
        KMCF_CHECK(positive(q.v), KMCF_ERR_ARG, "kmcf_update_temperature_local: %s = %g must be positive", q.name, q.v);
    KMCF_CHECK(step_time >= 0.0 && std::isfinite(step_time), KMCF_ERR_ARG,
               "kmcf_update_temperature_local: step_time = %g must be >= 0", step_time);
    KMCF_CHECK(std::isfinite(p->background_temp), KMCF_ERR_ARG, "kmcf_update_temperature_local: background_temp = %g", p->background_temp);
    KMCF_CHECK(p->cg_tolerance >= 0.0 && std::isfinite(p->cg_tolerance), KMCF_ERR_ARG,
               "kmcf_update_temperature_local: cg_tolerance = %g must be >= 0", p->cg_tolerance);
    KMCF_CHECK(p->cg_max_iterations > 0, KMCF_ERR_ARG, "kmcf_update_temperature_local: cg_max_iterations = %d must be positive",
               p->cg_max_iterations);
    kmcf_comm *c = k->comm;
    kmcf_matrix *m = k->K;
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "kmcf_update_temperature_local: host-only communicator");
    KMCF_CHECK(c->connected, KMCF_ERR_COMM, "kmcf_update_temperature_local: communicator not connected");
    KMCF_TRY(kmcf_enter(c));

    // Device::updateTemperature: the steady state beyond 1e3 delta_t, else ONE backward-Euler step of step_time (the
    // reference applies its explicit operator int(step_time / delta_t) + 1 times); a step of length 0 leaves T_old
    const bool steady = step_time > 1e3 * p->delta_t;
    const bool solve = steady || step_time > 0.0;
    const double T0 = p->background_temp;
    heat_args a{};
    a.g[0] = p->k_th_metal * p->L_char;
    a.g[1] = p->k_th_vacancies * p->L_char;
    a.g[2] = p->k_th_non_vacancy * p->L_char;
    const double g_max = std::max(a.g[0], std::max(a.g[1], a.g[2]));
    const double C_site = p->c_p * 1e6 * p->A * p->t_ox / k->N_interface;     // C_thermal of the global model, per site
    a.cdt = steady ? 0.0 : C_site / step_time;
    a.T0 = T0;
    // dictionary of the coded SpMV: the distinct off-diagonal values (equal conductivities share one code)
    double dict[3];
    int nd = 0;
    for (int q = 0; q < 3; ++q) {
        a.dv[q] = -a.g[q];
        int code = -1;
        for (int e = 0; e < nd; ++e)
            if (dict[e] == a.dv[q]) code = e;
        if (code < 0) { code = nd; dict[nd++] = a.dv[q]; }
        a.code[q] = code;
    }
    for (int e = 0; e < 3; ++e) a.vc[e] = e < nd ? dict[e] : 0.0;
    double *T_rows = d_site_temperature + N_left_tot + m->row0;     // this rank's interface rows, caller's order
    hipEvent_t a0 = c->ev_a0, a1 = c->ev_a1;
    if (solve) {
        KMCF_HIP(hipEventRecord(a0, c->stream));
        KMCF_TRY(kmcf_k_classes_async(k, d_site_element, d_site_charge, d_metals, num_metals));
        if (m->n_loc > 0) {
            KMCF_TRY(kmcf_matrix_set_dictionary(m, dict, nd));
            a.n_loc = m->n_loc; a.row_site0 = k->N_left + m->row0; a.n_left = k->N_left; a.n_interface = k->N_interface;
            a.row_ptr = m->d_row_ptr; a.col = m->d_col; a.diag_pos = k->d_diag_pos; a.perm = m->d_perm;
            a.left_row_ptr = k->d_left_row_ptr; a.left_col = k->d_left_col;
            a.right_row_ptr = k->d_right_row_ptr; a.right_col = k->d_right_col;
            a.cls = k->d_cls; a.cls_col = k->d_cls_col;
            a.T_old = d_site_temperature; a.Q = d_site_power;
            a.val = m->d_val; a.diag_out = k->d_diag; a.left_out = k->d_left; a.right_out = k->d_right;
            a.dinv_out = m->d_dinv; a.rhs_out = k->d_rhs;
            a.idx16 = m->coded ? m->d_idx16 : nullptr;
            a.diagv = m->coded ? m->d_diagv : nullptr;
            // (the tiles cover the short rows only: a matrix with long rows is assembled row-wise, as K is)
            if (m->coded && m->spmv_kind == 2 && m->tiles_for_coded && m->n_short == m->n_loc)
                heat_assemble_tile_kernel<<<std::min(m->n_tiles, 8 * 256 * 4), KMCF_BLOCK, 0, c->stream>>>(a, m->n_tiles, m->d_tile, m->d_wcol);
            else
                heat_assemble_kernel<16><<<kmcf_grid1d((int64_t)m->n_loc * 16), KMCF_BLOCK, 0, c->stream>>>(a);
            KMCF_HIP(hipGetLastError());
        }
        KMCF_HIP(hipEventRecord(a1, c->stream));
        k->assembled = true;
        // (the matrix and kmcf_k_get_vectors now hold the heat system; the next kmcf_k_assemble refills K)
        KMCF_HIP(hipMemcpyAsync(m->d_r, k->d_rhs, (size_t)m->n_loc * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        KMCF_TRY(kmcf_vec_in(m, m->d_x, T_rows));
        // stopping rule on the system in units of the largest pair conductance: the preconditioned residual of A / g_max
        // is sqrt(g_max) times the one of A, so the loop's sqrt(r.z / b.b) is held to cg_tolerance / sqrt(g_max)
        const double scale = std::sqrt(g_max);
        KMCF_TRY(kmcf_pcg_workspace_loop(m, p->cg_tolerance / scale, p->cg_max_iterations, stats));
        if (stats) stats->relres *= scale;
        KMCF_TRY(kmcf_vec_out(m, T_rows, m->d_x));
    } else if (stats) {
        *stats = kmcf_solve_stats_t{};
        stats->converged = 1;
    }
    heat_contacts_kernel<<<kmcf_grid1d(N), KMCF_BLOCK, 0, c->stream>>>(d_site_temperature, N, N_left_tot, k->N_interface, T0);
    KMCF_HIP(hipGetLastError());
    // replicated on every rank (as kmcf_sum_and_gather_potential replicates the potential), then the mean of the
    // interface sites, added in the same order on every rank
    KMCF_TRY(kmcf_comm_allgatherv_double(c, d_site_temperature + N_left_tot, m->counts.data(), m->displs.data()));
    double *d_part = c->d_scratch;            // 1024 doubles of persistent scratch
    const int g = kmcf_grid1d(k->N_interface, 1024);
    tsum_partial_kernel<<<g, KMCF_BLOCK, 0, c->stream>>>(d_site_temperature, N_left_tot, k->N_interface, d_part);
    KMCF_HIP(hipGetLastError());
    tsum_final_kernel<<<1, KMCF_BLOCK, 0, c->stream>>>(d_part, g);
    KMCF_HIP(hipGetLastError());
    double T_sum = 0.0;
    KMCF_HIP(hipMemcpyAsync(&T_sum, d_part, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    KMCF_HIP(hipStreamSynchronize(c->stream));
    KMCF_TRY(kmcf_p2p_check(c));
    if (h_T_bg) *h_T_bg = T_sum / k->N_interface;          // heat_solver.cpp:219-226
    if (h_steady) *h_steady = steady ? 1 : 0;
    if (stats && solve) {
        float ms = 0.f;
        KMCF_HIP(hipEventElapsedTime(&ms, a0, a1));
        stats->ms_assembly = ms;
    }
    return KMCF_OK;
}
