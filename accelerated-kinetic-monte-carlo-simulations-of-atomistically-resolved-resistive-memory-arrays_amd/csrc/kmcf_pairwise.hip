// Short-range pairwise ("gridless") Poisson term: potential of the charged sites within a cutoff
// (SURVEY.md 8f-1).  Replaces compute_cutoff_list (src/neighbor_lists_gpu.cu:293-372) and
// poisson_gridless_gpu / calculate_pairwise_interaction_indexed (src/potential_solver_gpu.cu:1525-1564,
// 1620-1655).
//
// The reference stores, per site, the indices of ALL possibly-charged sites within 20 A (N x N_cutoff
// ints: ~0.6 GB at 5 nm) and walks the whole list every step, skipping the uncharged ones.  Only a few
// percent of those sites carry a charge, so here the structure is inverted:
//   init:      sites sorted by 20 A cell (positions never change)            -> kmcf_pairwise
//   each step: the charged sites compacted in cell order (the shared compaction of kmcf_cellmembers.hpp:
//              deterministic, all on the device), then 16 lanes per site sum the charged sites of the 27
//              surrounding cells.
// Result per site = sum over charged j != i with dist < cutoff of  q_j erfc(r/(sigma sqrt 2)) k q / r
// (v_solve_gpu, src/gpu_solvers.h:321-329), the same set the reference's list yields as long as charged
// sites are V / Od (update_charge only ever charges those, potential_solver_gpu.cu:27-60).
// kmcf_compute_cutoff_list_pbc builds the same index over one period in y and z; pairwise_pbc_kernel then takes the
// minimum image.  Both kernels are one sum (pairwise_sum) over the walk of kmcf_cellwalk.hpp, which the
// analysis passes share.
#include <algorithm>
#include <cmath>
#include <vector>

#include "kmcf_cellwalk.hpp"      // the walk and, through kmcf_cellmembers.hpp, its list; kmcf_internal.hpp: struct kmcf_pairwise

namespace {

// the members of the per-step compaction (kmcf_cellmembers.hpp): the charged sites, by site id
struct pw_rule {
    const int *charge;
    __device__ __forceinline__ int operator()(int i) const { return charge[i] != 0; }
};
struct pw_emit {
    int *clist;
    __device__ __forceinline__ void operator()(int, int q, int i, int) const { clist[q] = i; }
};

// the reference's distance from site i to site j, operation for operation: open, and on a periodic index the minimum
// image in y and z.  A pair has ONE distance: where a period is shorter than two cutoffs no second image is added.
__device__ __forceinline__ double pairwise_dist(const kmcf_cell_grid &, double xi, double yi, double zi, double xj, double yj,
                                                double zj)
{
    const double dx = xj - xi, dy = yj - yi, dz = zj - zi;
    return sqrt(dx * dx + dy * dy + dz * dz);
}
__device__ __forceinline__ double pairwise_dist(const kmcf_cell_grid_pbc &g, double xi, double yi, double zi, double xj,
                                                double yj, double zj)
{
    return kmcf_min_image_dist(xi, yi, zi, xj, yj, zj, g.ly, g.lz);
}

// calculate_pairwise_interaction_indexed (potential_solver_gpu.cu:1525-1564): potential[i] = sum, written not added, over
// the charged j != i below the cutoff.  16 lanes per site take the runs of kmcf_walk_columns (kmcf_cellwalk.hpp: every
// cell once, no column skipped) in its order; a lane adds its terms in the order it meets them.
template <class GRID>
__device__ __forceinline__ void pairwise_sum(const GRID &g, const int *__restrict__ cell_start, const int *__restrict__ flag_pos,
                                             const int *__restrict__ clist, const double *__restrict__ x,
                                             const double *__restrict__ y, const double *__restrict__ z,
                                             const int *__restrict__ charge, double sigma, double k, double cutoff, int count,
                                             int displ, double *__restrict__ potential)
{
    constexpr int LPS = 16, SPB = KMCF_BLOCK / LPS;
    const double q = 1.60217663e-19;            // gpu_solvers.h:323
    const int lane = threadIdx.x % LPS;
    const int groups = (count + SPB - 1) / SPB;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int idx = grp * SPB + threadIdx.x / LPS;
        const bool valid = idx < count;
        const int i = displ + idx;
        double acc = 0.0;
        if (valid) {
            const double xi = x[i], yi = y[i], zi = z[i];
            kmcf_walk_columns(
                g, xi, yi, zi, cell_start, flag_pos, [](double) { return true; },
                [&](int b, int e) {
                    for (int t = b + lane; t < e; t += LPS) {
                        const int j = clist[t];
                        if (j == i) continue;
                        const double dist = pairwise_dist(g, xi, yi, zi, x[j], y[j], z[j]);
                        if (dist < cutoff) {
                            const double r = 1e-10 * dist;                                    // :1554
                            acc += (double)charge[j] * erfc(r / (sigma * sqrt(2.0))) * k * q / r;  // gpu_solvers.h:325
                        }
                    }
                },
                []() {});
        }
#pragma unroll
        for (int off = LPS / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (valid && lane == 0) potential[i] = acc;
    }
}

__global__ __launch_bounds__(KMCF_BLOCK) void pairwise_kernel(
    kmcf_cell_grid g, const int *__restrict__ cell_start, const int *__restrict__ flag_pos, const int *__restrict__ clist,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
    const int *__restrict__ charge, double sigma, double k, double cutoff, int count, int displ,
    double *__restrict__ potential)
{
    pairwise_sum(g, cell_start, flag_pos, clist, x, y, z, charge, sigma, k, cutoff, count, displ, potential);
}

// the same sum on a periodic index
__global__ __launch_bounds__(KMCF_BLOCK) void pairwise_pbc_kernel(
    kmcf_cell_grid_pbc g, const int *__restrict__ cell_start, const int *__restrict__ flag_pos, const int *__restrict__ clist,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
    const int *__restrict__ charge, double sigma, double k, double cutoff, int count, int displ,
    double *__restrict__ potential)
{
    pairwise_sum(g, cell_start, flag_pos, clist, x, y, z, charge, sigma, k, cutoff, count, displ, potential);
}

inline auto pairwise_kernel_of(const kmcf_cell_grid &) { return pairwise_kernel; }
inline auto pairwise_kernel_of(const kmcf_cell_grid_pbc &) { return pairwise_pbc_kernel; }

// the sites in cell order and the buffers of the per-step compaction, from the host copy of the coordinates; coord(s)
// is the cell id of site s
template <class F>
int index_cells(kmcf_pairwise *p, F cell_of_site)
{
    const int N = p->N;
    std::vector<int> start((size_t)p->ncell + 1, 0), cid((size_t)N), order((size_t)N);
    for (int s = 0; s < N; ++s) {
        cid[s] = cell_of_site(s);
        start[cid[s] + 1]++;
    }
    for (int cc = 0; cc < p->ncell; ++cc) start[cc + 1] += start[cc];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int s = 0; s < N; ++s) order[fill[cid[s]]++] = s;
    KMCF_TRY(kmcf_dev_alloc(&p->d_cell_order, (size_t)N, false));
    KMCF_TRY(kmcf_dev_alloc(&p->d_cell_start, (size_t)p->ncell + 1, false));
    KMCF_TRY(kmcf_members_alloc(&p->charged, N, 1, false));
    KMCF_HIP(hipMemcpy(p->d_cell_order, order.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice));
    KMCF_HIP(hipMemcpy(p->d_cell_start, start.data(), start.size() * sizeof(int), hipMemcpyHostToDevice));
    return KMCF_OK;
}

void pairwise_release(kmcf_pairwise *p)
{
    kmcf_dev_free_all({p->d_cell_order, p->d_cell_start});
    kmcf_members_free(&p->charged);
    delete p;
}

}  // namespace

extern "C" int kmcf_compute_cutoff_list_pbc(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                                            double cutoff_radius, const double *h_lattice, int pbc, kmcf_pairwise **out)
{
    const char *what = "kmcf_compute_cutoff_list_pbc";
    KMCF_CHECK(pbc == 0 || pbc == 1, KMCF_ERR_ARG, "%s: pbc = %d is neither 0 nor 1", what, pbc);
    if (pbc == 0) {                                 // today's index, whatever the lattice says
        KMCF_TRY(kmcf_compute_cutoff_list(c, d_x, d_y, d_z, N, cutoff_radius, out));
        if (h_lattice) std::copy(h_lattice, h_lattice + 3, (*out)->lattice);
        return KMCF_OK;
    }
    KMCF_CHECK(c && d_x && d_y && d_z && out && N > 0 && cutoff_radius > 0, KMCF_ERR_ARG, "%s: bad argument", what);
    KMCF_CHECK(h_lattice, KMCF_ERR_ARG, "%s: h_lattice is NULL with pbc = 1", what);
    const double Ly = h_lattice[1], Lz = h_lattice[2];
    KMCF_CHECK(std::isfinite(Ly) && Ly > 0, KMCF_ERR_ARG, "%s: the period in y, h_lattice[1] = %g, is not finite and > 0", what, Ly);
    KMCF_CHECK(std::isfinite(Lz) && Lz > 0, KMCF_ERR_ARG, "%s: the period in z, h_lattice[2] = %g, is not finite and > 0", what, Lz);
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "%s: host-only communicator", what);
    KMCF_TRY(kmcf_enter_setup(c));
    std::vector<double> x(N), y(N), z(N);
    KMCF_HIP(hipMemcpy(x.data(), d_x, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    KMCF_HIP(hipMemcpy(y.data(), d_y, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    KMCF_HIP(hipMemcpy(z.data(), d_z, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int s = 0; s < N; ++s) {
        lo[0] = std::min(lo[0], x[s]); hi[0] = std::max(hi[0], x[s]);
        lo[1] = std::min(lo[1], y[s]); hi[1] = std::max(hi[1], y[s]);
        lo[2] = std::min(lo[2], z[s]); hi[2] = std::max(hi[2], z[s]);
    }
    // the cells tile [min, min + L): a site at min + L or beyond has no cell of its own
    KMCF_CHECK(hi[1] - lo[1] < Ly, KMCF_ERR_ARG, "%s: the sites span %.17g in y, a whole period (%.17g) or more: wrap them into one cell first",
               what, hi[1] - lo[1], Ly);
    KMCF_CHECK(hi[2] - lo[2] < Lz, KMCF_ERR_ARG, "%s: the sites span %.17g in z, a whole period (%.17g) or more: wrap them into one cell first",
               what, hi[2] - lo[2], Lz);
    kmcf_pairwise *p = new kmcf_pairwise();
    p->comm = c; p->N = N; p->cutoff = cutoff_radius; p->pbc = 1;
    std::copy(h_lattice, h_lattice + 3, p->lattice);
    p->x0 = lo[0]; p->y0 = lo[1]; p->z0 = lo[2]; p->inv = 1.0 / cutoff_radius;
    p->ncx = (int)std::floor((hi[0] - lo[0]) * p->inv) + 1;
    const double ny = std::floor(Ly / cutoff_radius), nz = std::floor(Lz / cutoff_radius);
    const double ncell = (double)p->ncx * std::max(ny, 1.0) * std::max(nz, 1.0);
    if (!(ncell < (double)(1 << 30))) {
        delete p;
        kmcf_set_error("%s: cell grid too large (%g cells)", what, ncell);
        return KMCF_ERR_ARG;
    }
    p->ncy = std::max(1, (int)ny); p->ncz = std::max(1, (int)nz);
    p->inv_y = p->ncy / Ly; p->inv_z = p->ncz / Lz;
    p->ncell = p->ncx * p->ncy * p->ncz;
    const int rc = index_cells(p, [&](int s) {
        return (kmcf_cell_coord(x[s], p->x0, p->inv, p->ncx) * p->ncy + kmcf_cell_coord(y[s], p->y0, p->inv_y, p->ncy)) * p->ncz +
               kmcf_cell_coord(z[s], p->z0, p->inv_z, p->ncz);
    });
    if (rc != KMCF_OK) { pairwise_release(p); return rc; }
    *out = p;
    return KMCF_OK;
}

extern "C" int kmcf_pairwise_periodic(const kmcf_pairwise *p, int *pbc, double *h_lattice)
{
    KMCF_CHECK(p, KMCF_ERR_ARG, "kmcf_pairwise_periodic: p is NULL");
    KMCF_CHECK(pbc, KMCF_ERR_ARG, "kmcf_pairwise_periodic: pbc is NULL");
    *pbc = p->pbc;
    if (h_lattice) std::copy(p->lattice, p->lattice + 3, h_lattice);
    return KMCF_OK;
}

extern "C" int kmcf_compute_cutoff_list(kmcf_comm *c, const double *d_x, const double *d_y, const double *d_z, int N,
                                        double cutoff_radius, kmcf_pairwise **out)
{
    KMCF_CHECK(c && d_x && d_y && d_z && out && N > 0 && cutoff_radius > 0, KMCF_ERR_ARG, "kmcf_compute_cutoff_list: bad argument");
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "kmcf_compute_cutoff_list: host-only communicator");
    KMCF_TRY(kmcf_enter_setup(c));
    std::vector<double> x(N), y(N), z(N);
    KMCF_HIP(hipMemcpy(x.data(), d_x, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    KMCF_HIP(hipMemcpy(y.data(), d_y, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    KMCF_HIP(hipMemcpy(z.data(), d_z, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    kmcf_pairwise *p = new kmcf_pairwise();
    p->comm = c; p->N = N; p->cutoff = cutoff_radius;
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int s = 0; s < N; ++s) {
        lo[0] = std::min(lo[0], x[s]); hi[0] = std::max(hi[0], x[s]);
        lo[1] = std::min(lo[1], y[s]); hi[1] = std::max(hi[1], y[s]);
        lo[2] = std::min(lo[2], z[s]); hi[2] = std::max(hi[2], z[s]);
    }
    p->x0 = lo[0]; p->y0 = lo[1]; p->z0 = lo[2]; p->inv = 1.0 / cutoff_radius;
    p->ncx = (int)std::floor((hi[0] - lo[0]) * p->inv) + 1;
    p->ncy = (int)std::floor((hi[1] - lo[1]) * p->inv) + 1;
    p->ncz = (int)std::floor((hi[2] - lo[2]) * p->inv) + 1;
    p->ncell = p->ncx * p->ncy * p->ncz;
    const int rc = index_cells(p, [&](int s) {
        return (kmcf_cell_coord(x[s], p->x0, p->inv, p->ncx) * p->ncy + kmcf_cell_coord(y[s], p->y0, p->inv, p->ncy)) * p->ncz +
               kmcf_cell_coord(z[s], p->z0, p->inv, p->ncz);
    });
    if (rc != KMCF_OK) { pairwise_release(p); return rc; }
    *out = p;
    return KMCF_OK;
}

extern "C" int kmcf_pairwise_destroy(kmcf_pairwise *p)
{
    if (!p) return KMCF_OK;
    hipSetDevice(p->comm->device);
    hipStreamSynchronize(p->comm->stream);
    kmcf_gap_ws_free(p);
    kmcf_chain_ws_free(p);
    kmcf_pc_ws_free(p);
    kmcf_fs_ws_free(p);
    kmcf_dev_free_all({p->d_cell_order, p->d_cell_start});
    kmcf_members_free(&p->charged);
    delete p;
    return KMCF_OK;
}

extern "C" int kmcf_poisson_gridless(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                     const int *d_site_charge, double sigma, double k, int count, int displ,
                                     double *d_site_potential_charge)
{
    KMCF_CHECK(p && d_x && d_y && d_z && d_site_charge && d_site_potential_charge, KMCF_ERR_ARG, "kmcf_poisson_gridless: null argument");
    KMCF_CHECK(count >= 0 && displ >= 0 && displ + count <= p->N, KMCF_ERR_ARG, "kmcf_poisson_gridless: rows [%d,%d) outside N=%d",
               displ, displ + count, p->N);
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    hipStream_t st = c->stream;
    kmcf_members_enqueue<1>(p, p->charged, pw_rule{d_site_charge}, pw_emit{p->charged.d_site});
    KMCF_HIP(hipGetLastError());
    if (count > 0) {
        int64_t grid = ((int64_t)count * 16 + KMCF_BLOCK - 1) / KMCF_BLOCK;
        if (grid > 8192) grid = 8192;
        p->with_grid([&](auto g) {
            pairwise_kernel_of(g)<<<(int)grid, KMCF_BLOCK, 0, st>>>(g, p->d_cell_start, p->charged.d_pos, p->charged.d_site, d_x, d_y,
                                                                   d_z, d_site_charge, sigma, k, p->cutoff, count, displ,
                                                                   d_site_potential_charge);
        });
        KMCF_HIP(hipGetLastError());
    }
    KMCF_HIP(hipStreamSynchronize(st));
    return KMCF_OK;
}
