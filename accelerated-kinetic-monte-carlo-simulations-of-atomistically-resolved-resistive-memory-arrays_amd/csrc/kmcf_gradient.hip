// Site gradient map (kmcf_site_gradient): per site the weighted least-squares gradient of a site field over the counted
// pairs of its neighbour row, the largest bond drop |q_ij| with the pair that holds it, and the maxima of both per cell
// and for the device.
//
// The reference has no counterpart.  Definitions (counted pairs, displacement, fullness, maxima, ties): include/kmcfield.h
// and DESIGN.md 3.14.
//
// Launches, all on the compute stream:
//   1  clear the rows (one per cell + one for the device)
//   2  the walk: 16 lanes per site, 4 sites per wavefront, a block owns a contiguous range of sites.  Lane l takes the
//      slots l, l + 16, l + 32, ... of the row in ascending order and adds its terms of M (6), b (3) and the pair count
//      from zero; it keeps its largest |q| with the slot (first slot among equals: strict >).  Then the xor butterfly over
//      the 16 lanes, steps 8, 4, 2, 1: every lane replaces its sum s by s + (the sum of lane l ^ step); the maximum takes
//      the other lane's (|q|, slot, j) if its |q| is larger, or equal with the lower slot.  Lane 0 solves and writes.
//      The group's first lane keeps the maxima and counts of its sites (device, and the run of equal cells it is in); a
//      block adds them up in LDS and raises the rows with 64-bit integer atomicMax on (bits of the value) + 1 -- finite
//      non-negative doubles order as their bits; 0 stands for "no candidate" -- and integer adds
//   3  among the sites that attain a row's maximum the smallest site id wins (atomicMin; for the drop on from << 32 | to)
//   4  the cell records
//
// Determinism: no atomics on doubles; every floating-point sum is added in the order above, which the input fixes; maxima,
// minima and counts are integer atomics, independent of the execution order.  No thread waits for another; all 64 lanes
// of every wavefront reach the shuffles (the site index is clamped, the stores are predicated).
#include <cmath>
#include <cstring>

#include "kmcf_internal.hpp"

static_assert(sizeof(kmcf_gradient_cell_t) == 40, "kmcf_gradient_cell_t is 40 bytes");
static_assert(sizeof(kmcf_gradient_stats_t) == 64, "kmcf_gradient_stats_t is 64 bytes");

typedef unsigned long long kmcf_gr_u64;

// a row of maxima and counts: one per cell, the last for the whole device
struct kmcf_gr_row {
    kmcf_gr_u64 gkey, dkey;      // (bits of the largest finite |g| / drop) + 1; 0: no candidate
    kmcf_gr_u64 dpair;           // drop_from << 32 | drop_to of the smallest drop_from that attains dkey; ~0: none
    kmcf_gr_u64 pairs;           // counted pairs (device row only)
    int gsite;                   // smallest site that attains gkey; INT_MAX: none
    int n_sites, n_full, n_deg;  // n_deg: device row only
};
static_assert(sizeof(kmcf_gr_row) == 48, "the device row travels through the 64 pinned bytes");

struct kmcf_gradient_ws {
    size_t cap_N = 0;
    double *d_gm = nullptr;      // |g| per site
    double *d_drop = nullptr;    // drop per site (where the caller gives no d_site_drop)
    int *d_dto = nullptr;        // drop_to per site (where the caller gives no d_site_drop_to)
    size_t cap_rows = 0;
    kmcf_gr_row *d_rows = nullptr;
    kmcf_gradient_cell_t *d_cells = nullptr;
};

void kmcf_gradient_ws_free(kmcf_comm *c)
{
    if (!c || !c->gr_ws) return;
    kmcf_gradient_ws *w = c->gr_ws;
    kmcf_dev_free_all({w->d_gm, w->d_drop, w->d_dto, w->d_rows, w->d_cells});
    delete w;
    c->gr_ws = nullptr;
}

namespace {

typedef kmcf_gr_u64 u64;
constexpr int GR_LPS = 16, GR_SPB = KMCF_BLOCK / GR_LPS;    // lanes per site, sites per block and pass
constexpr int GR_NO_SITE = 0x7fffffff;
constexpr u64 GR_NO_PAIR = ~0ull;
constexpr int GR_MAX_CELLS = 1024;
constexpr double GR_FULL_RATIO = 1e-9;

// displacement from site i to site j: the plain difference, or x plain and the library's one minimum image in y and z
struct disp_open {
    __device__ __forceinline__ void operator()(double xi, double yi, double zi, double xj, double yj, double zj, double &dx,
                                               double &dy, double &dz) const
    {
        dx = xj - xi;
        dy = yj - yi;
        dz = zj - zi;
    }
};
struct disp_min_image {
    double ly, lz;
    __device__ __forceinline__ void operator()(double xi, double yi, double zi, double xj, double yj, double zj, double &dx,
                                               double &dy, double &dz) const
    {
        dx = xj - xi;
        dy = kmcf_min_image(yj - yi, ly);
        dz = kmcf_min_image(zj - zi, lz);
    }
};

// key of a candidate for a maximum: bits + 1 of a finite value >= 0, else 0
__device__ __forceinline__ u64 gr_key(double v)
{
    return (v >= 0.0 && v < __longlong_as_double(0x7ff0000000000000ll)) ? (u64)__double_as_longlong(v) + 1 : 0;
}

__device__ __forceinline__ void gr_raise(kmcf_gr_row *r, u64 gk, u64 dk, int ns, int nf)
{
    if (gk) atomicMax(&r->gkey, gk);
    if (dk) atomicMax(&r->dkey, dk);
    if (ns) atomicAdd(&r->n_sites, ns);
    if (nf) atomicAdd(&r->n_full, nf);
}

// 1
__global__ __launch_bounds__(KMCF_BLOCK) void gr_clear_kernel(int n_rows, kmcf_gr_row *__restrict__ rows)
{
    const int r = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (r < n_rows) rows[r] = kmcf_gr_row{0, 0, GR_NO_PAIR, 0, GR_NO_SITE, 0, 0, 0};
}

// 2: block b owns the sites [b * iters * GR_SPB, (b + 1) * iters * GR_SPB)
template <typename DISP>
__global__ __launch_bounds__(KMCF_BLOCK) void gr_walk_kernel(
    int N, int nn, int iters, const int *__restrict__ neigh, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ z, const double *__restrict__ value, const int *__restrict__ mask,
    const int *__restrict__ site_cell, int n_cells, double *__restrict__ gx, double *__restrict__ gy, double *__restrict__ gz,
    double *__restrict__ drop_out, int *__restrict__ dto_out, int *__restrict__ full_out, double *__restrict__ gm_out,
    kmcf_gr_row *rows, DISP disp)
{
    __shared__ u64 s_gk[2][GR_SPB], s_dk[2][GR_SPB], s_pairs[GR_SPB];
    __shared__ int s_cell[GR_SPB], s_ns[2][GR_SPB], s_nf[2][GR_SPB], s_nd[GR_SPB];
    const int lane = threadIdx.x % GR_LPS, grp = threadIdx.x / GR_LPS;
    const long long first = (long long)blockIdx.x * iters * GR_SPB;
    // what the group's first lane has seen: [0] the device, [1] the run of sites of one cell it is in
    u64 a_gk[2] = {0, 0}, a_dk[2] = {0, 0}, a_pairs = 0;
    int a_ns[2] = {0, 0}, a_nf[2] = {0, 0}, a_nd = 0, a_cell = -1;

    for (int it = 0; it < iters; ++it) {
        const long long site = first + (long long)it * GR_SPB + grp;
        const bool valid = site < N;
        const int i = valid ? (int)site : N - 1;
        const bool in = valid && (!mask || mask[i] != 0);
        double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
        int cnt = 0;
        double bq = -1.0;                    // this lane's largest |q|, its slot and its j
        int bs = GR_NO_SITE, bj = -1;
        if (in) {
            const double xi = x[i], yi = y[i], zi = z[i], vi = value[i];
            const int *__restrict__ row = neigh + (size_t)i * nn;
            for (int s0 = lane; s0 < nn; s0 += 4 * GR_LPS) {
                int j[4];
                bool ok[4];
                double xj[4], yj[4], zj[4], vj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int s = s0 + u * GR_LPS;
                    j[u] = s < nn ? row[s] : -1;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    ok[u] = (unsigned)j[u] < (unsigned)N && j[u] != i && (!mask || mask[j[u]] != 0);
                    const int jj = ok[u] ? j[u] : i;
                    xj[u] = x[jj]; yj[u] = y[jj]; zj[u] = z[jj]; vj[u] = value[jj];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (!ok[u]) continue;
                    double dx, dy, dz;
                    disp(xi, yi, zi, xj[u], yj[u], zj[u], dx, dy, dz);
                    const double d = sqrt((dx * dx + dy * dy) + dz * dz);
                    if (!(d > 0.0)) continue;
                    const double ux = dx / d, uy = dy / d, uz = dz / d, q = (vj[u] - vi) / d;
                    m00 += ux * ux; m01 += ux * uy; m02 += ux * uz;
                    m11 += uy * uy; m12 += uy * uz; m22 += uz * uz;
                    b0 += ux * q; b1 += uy * q; b2 += uz * q;
                    ++cnt;
                    const double aq = fabs(q);
                    if (aq > bq) { bq = aq; bs = s0 + u * GR_LPS; bj = j[u]; }
                }
            }
        }
#pragma unroll
        for (int off = GR_LPS / 2; off >= 1; off >>= 1) {
            m00 += __shfl_xor(m00, off, GR_LPS); m01 += __shfl_xor(m01, off, GR_LPS); m02 += __shfl_xor(m02, off, GR_LPS);
            m11 += __shfl_xor(m11, off, GR_LPS); m12 += __shfl_xor(m12, off, GR_LPS); m22 += __shfl_xor(m22, off, GR_LPS);
            b0 += __shfl_xor(b0, off, GR_LPS); b1 += __shfl_xor(b1, off, GR_LPS); b2 += __shfl_xor(b2, off, GR_LPS);
            cnt += __shfl_xor(cnt, off, GR_LPS);
            const double oq = __shfl_xor(bq, off, GR_LPS);
            const int os = __shfl_xor(bs, off, GR_LPS), oj = __shfl_xor(bj, off, GR_LPS);
            if (oq > bq || (oq == bq && os < bs)) { bq = oq; bs = os; bj = oj; }
        }
        if (lane == 0 && valid) {
            double g0 = 0.0, g1 = 0.0, g2 = 0.0;
            int full = 0;
            if (cnt >= 3) {
                // closed-form symmetric inverse: cofactors, determinant along the first row
                const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
                const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
                const double det = (m00 * c00 + m01 * c01) + m02 * c02;
                const double r = (double)cnt / 3.0;
                if (det >= GR_FULL_RATIO * ((r * r) * r)) {
                    full = 1;
                    g0 = ((c00 * b0 + c01 * b1) + c02 * b2) / det;
                    g1 = ((c01 * b0 + c11 * b1) + c12 * b2) / det;
                    g2 = ((c02 * b0 + c12 * b1) + c22 * b2) / det;
                }
            }
            const double drop = bj >= 0 ? bq : 0.0;
            const double gm = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
            if (gx) { gx[i] = g0; gy[i] = g1; gz[i] = g2; }
            drop_out[i] = drop;
            dto_out[i] = bj;
            if (full_out) full_out[i] = full;
            gm_out[i] = gm;
            if (in) {
                const u64 gk = gr_key(gm), dk = bj >= 0 ? gr_key(drop) : 0;
                a_gk[0] = max(a_gk[0], gk); a_dk[0] = max(a_dk[0], dk);
                ++a_ns[0]; a_nf[0] += full; a_nd += (cnt >= 3 && !full); a_pairs += (u64)cnt;
                const int c = kmcf_site_cell(site_cell, n_cells, i);
                if (c >= 0) {
                    if (c != a_cell) {
                        if (a_cell >= 0) gr_raise(rows + a_cell, a_gk[1], a_dk[1], a_ns[1], a_nf[1]);
                        a_cell = c;
                        a_gk[1] = a_dk[1] = 0;
                        a_ns[1] = a_nf[1] = 0;
                    }
                    a_gk[1] = max(a_gk[1], gk); a_dk[1] = max(a_dk[1], dk);
                    ++a_ns[1]; a_nf[1] += full;
                }
            }
        }
    }
    // the block's groups together: one set of atomics per cell they ended in, one for the device
    if (lane == 0) {
        s_cell[grp] = a_cell;
        s_pairs[grp] = a_pairs;
        s_nd[grp] = a_nd;
#pragma unroll
        for (int k = 0; k < 2; ++k) { s_gk[k][grp] = a_gk[k]; s_dk[k][grp] = a_dk[k]; s_ns[k][grp] = a_ns[k]; s_nf[k][grp] = a_nf[k]; }
    }
    __syncthreads();
    if (threadIdx.x < GR_SPB) {
        const int t = threadIdx.x, c = s_cell[t];
        bool lead = c >= 0;
        for (int k = 0; k < t; ++k) lead = lead && s_cell[k] != c;
        if (lead) {
            u64 gk = 0, dk = 0;
            int ns = 0, nf = 0;
            for (int k = t; k < GR_SPB; ++k)
                if (s_cell[k] == c) { gk = max(gk, s_gk[1][k]); dk = max(dk, s_dk[1][k]); ns += s_ns[1][k]; nf += s_nf[1][k]; }
            gr_raise(rows + c, gk, dk, ns, nf);
        }
    } else if (threadIdx.x == 64) {
        u64 gk = 0, dk = 0, pairs = 0;
        int ns = 0, nf = 0, nd = 0;
        for (int k = 0; k < GR_SPB; ++k) {
            gk = max(gk, s_gk[0][k]); dk = max(dk, s_dk[0][k]); ns += s_ns[0][k]; nf += s_nf[0][k];
            nd += s_nd[k]; pairs += s_pairs[k];
        }
        kmcf_gr_row *r = rows + n_cells;
        gr_raise(r, gk, dk, ns, nf);
        if (nd) atomicAdd(&r->n_deg, nd);
        if (pairs) atomicAdd(&r->pairs, pairs);
    }
}

__device__ __forceinline__ void gr_pick_row(kmcf_gr_row *r, int i, u64 gk, u64 dk, int to)
{
    if (gk && gk == r->gkey && i < kmcf_load_relaxed(&r->gsite)) atomicMin(&r->gsite, i);
    if (dk && dk == r->dkey) {
        const u64 pr = ((u64)(unsigned)i << 32) | (unsigned)to;
        if (pr < kmcf_load_relaxed(&r->dpair)) atomicMin(&r->dpair, pr);
    }
}

// 3: the keys are final (earlier launch)
__global__ __launch_bounds__(KMCF_BLOCK) void gr_pick_kernel(int N, const int *__restrict__ mask, const int *__restrict__ site_cell,
                                                             int n_cells, const double *__restrict__ gm,
                                                             const double *__restrict__ drop, const int *__restrict__ dto,
                                                             kmcf_gr_row *rows)
{
    for (int i = blockIdx.x * KMCF_BLOCK + threadIdx.x; i < N; i += gridDim.x * KMCF_BLOCK) {
        if (mask && mask[i] == 0) continue;
        const int to = dto[i];
        const u64 gk = gr_key(gm[i]), dk = to >= 0 ? gr_key(drop[i]) : 0;
        gr_pick_row(rows + n_cells, i, gk, dk, to);
        const int c = kmcf_site_cell(site_cell, n_cells, i);
        if (c >= 0) gr_pick_row(rows + c, i, gk, dk, to);
    }
}

// what a row says, in the ABI's terms
template <typename T>
__host__ __device__ inline void gr_unpack(const kmcf_gr_row &r, T *out)
{
    union { kmcf_gr_u64 u; double d; } g, d;
    g.u = r.gkey ? r.gkey - 1 : 0;
    d.u = r.dkey ? r.dkey - 1 : 0;
    out->n_sites = r.n_sites;
    out->n_full = r.n_full;
    out->g_max = g.d;
    out->g_site = r.gkey ? r.gsite : -1;
    out->drop_max = d.d;
    out->drop_from = r.dkey ? (int)(r.dpair >> 32) : -1;
    out->drop_to = r.dkey ? (int)(r.dpair & 0xffffffffull) : -1;
}

// 4
__global__ __launch_bounds__(KMCF_BLOCK) void gr_record_kernel(int n_cells, const kmcf_gr_row *__restrict__ rows,
                                                               kmcf_gradient_cell_t *__restrict__ cells)
{
    const int c = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (c < n_cells) {
        kmcf_gradient_cell_t e;
        gr_unpack(rows[c], &e);
        cells[c] = e;
    }
}

// scratch on the communicator, grown on demand and freed by kmcf_comm_destroy; it holds nothing a later call reads
int gr_workspace(kmcf_comm *c, int N, int n_cells)
{
    if (!c->gr_ws) c->gr_ws = new kmcf_gradient_ws();
    kmcf_gradient_ws *w = c->gr_ws;
    if (w->cap_N < (size_t)N) {                          // three buffers of one capacity
        w->cap_N = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_gm, nullptr, (size_t)N, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_drop, nullptr, (size_t)N, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_dto, nullptr, (size_t)N, 0));
        w->cap_N = (size_t)N;
    }
    if (w->cap_rows < (size_t)n_cells + 1) {
        w->cap_rows = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_rows, nullptr, (size_t)n_cells + 1, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_cells, nullptr, (size_t)n_cells, 0));
        w->cap_rows = (size_t)n_cells + 1;
    }
    return KMCF_OK;
}

}  // namespace

extern "C" int kmcf_site_gradient(kmcf_comm *c, int N, int nn, const int *d_neigh_idx, const double *d_x, const double *d_y,
                                  const double *d_z, const double *h_lattice, int pbc, const double *d_value,
                                  const int *d_site_mask, const int *d_site_cell, int n_cells, double *d_gx, double *d_gy,
                                  double *d_gz, double *d_site_drop, int *d_site_drop_to, int *d_site_full,
                                  kmcf_gradient_cell_t *h_cells, kmcf_gradient_stats_t *stats)
{
    const char *what = "kmcf_site_gradient";
    KMCF_CHECK(c, KMCF_ERR_ARG, "%s: c is NULL", what);
    KMCF_CHECK(d_neigh_idx, KMCF_ERR_ARG, "%s: d_neigh_idx is NULL", what);
    KMCF_CHECK(d_x, KMCF_ERR_ARG, "%s: d_x is NULL", what);
    KMCF_CHECK(d_y, KMCF_ERR_ARG, "%s: d_y is NULL", what);
    KMCF_CHECK(d_z, KMCF_ERR_ARG, "%s: d_z is NULL", what);
    KMCF_CHECK(d_value, KMCF_ERR_ARG, "%s: d_value is NULL", what);
    KMCF_CHECK(N > 0, KMCF_ERR_ARG, "%s: N = %d is not > 0", what, N);
    KMCF_CHECK(nn > 0, KMCF_ERR_ARG, "%s: nn = %d is not > 0", what, nn);
    KMCF_CHECK(pbc == 0 || pbc == 1, KMCF_ERR_ARG, "%s: pbc = %d is neither 0 nor 1", what, pbc);
    if (pbc == 1) {
        KMCF_CHECK(h_lattice, KMCF_ERR_ARG, "%s: h_lattice is NULL with pbc = 1", what);
        KMCF_CHECK(std::isfinite(h_lattice[1]) && h_lattice[1] > 0.0, KMCF_ERR_ARG,
                   "%s: the y period h_lattice[1] = %g is not a finite length > 0", what, h_lattice[1]);
        KMCF_CHECK(std::isfinite(h_lattice[2]) && h_lattice[2] > 0.0, KMCF_ERR_ARG,
                   "%s: the z period h_lattice[2] = %g is not a finite length > 0", what, h_lattice[2]);
    }
    KMCF_CHECK(n_cells >= 1 && n_cells <= GR_MAX_CELLS, KMCF_ERR_ARG, "%s: n_cells = %d is outside 1 ... %d", what, n_cells,
               GR_MAX_CELLS);
    KMCF_CHECK(d_site_cell || n_cells == 1, KMCF_ERR_ARG, "%s: d_site_cell is NULL with n_cells = %d", what, n_cells);
    const int n_g = (d_gx != nullptr) + (d_gy != nullptr) + (d_gz != nullptr);
    KMCF_CHECK(n_g == 0 || n_g == 3, KMCF_ERR_ARG, "%s: only %d of d_gx / d_gy / d_gz are set: pass all three or none", what, n_g);
    KMCF_CHECK(n_g || d_site_drop || d_site_drop_to || d_site_full || h_cells || stats, KMCF_ERR_ARG,
               "%s: no output is requested (d_gx / d_gy / d_gz, d_site_drop, d_site_drop_to, d_site_full, h_cells, stats)", what);
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "%s: host-only communicator", what);
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(gr_workspace(c, N, n_cells));
    kmcf_gradient_ws *w = c->gr_ws;
    hipStream_t st = c->stream;
    double *drop = d_site_drop ? d_site_drop : w->d_drop;
    int *dto = d_site_drop_to ? d_site_drop_to : w->d_dto;
    // a block owns iters * GR_SPB consecutive sites; at most 2048 blocks (8 per CU)
    const int64_t groups = ((int64_t)N + GR_SPB - 1) / GR_SPB;
    const int iters = (int)((groups + 2047) / 2048);
    const int walk_grid = (int)((groups + iters - 1) / iters);

    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    gr_clear_kernel<<<kmcf_grid1d(n_cells + 1), KMCF_BLOCK, 0, st>>>(n_cells + 1, w->d_rows);
    if (pbc)
        gr_walk_kernel<<<walk_grid, KMCF_BLOCK, 0, st>>>(N, nn, iters, d_neigh_idx, d_x, d_y, d_z, d_value, d_site_mask, d_site_cell,
                                                        n_cells, d_gx, d_gy, d_gz, drop, dto, d_site_full, w->d_gm, w->d_rows,
                                                        disp_min_image{h_lattice[1], h_lattice[2]});
    else
        gr_walk_kernel<<<walk_grid, KMCF_BLOCK, 0, st>>>(N, nn, iters, d_neigh_idx, d_x, d_y, d_z, d_value, d_site_mask, d_site_cell,
                                                        n_cells, d_gx, d_gy, d_gz, drop, dto, d_site_full, w->d_gm, w->d_rows,
                                                        disp_open{});
    if (h_cells || stats) {
        gr_pick_kernel<<<kmcf_grid1d(N), KMCF_BLOCK, 0, st>>>(N, d_site_mask, d_site_cell, n_cells, w->d_gm, drop, dto, w->d_rows);
        if (h_cells) gr_record_kernel<<<kmcf_grid1d(n_cells), KMCF_BLOCK, 0, st>>>(n_cells, w->d_rows, w->d_cells);
    }
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    if (h_cells)
        KMCF_HIP(hipMemcpyAsync(h_cells, w->d_cells, (size_t)n_cells * sizeof(kmcf_gradient_cell_t), hipMemcpyDeviceToHost, st));
    if (stats) KMCF_HIP(hipMemcpyAsync(c->h_pinned, w->d_rows + n_cells, sizeof(kmcf_gr_row), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipStreamSynchronize(st));
    if (stats) {
        kmcf_gr_row r;
        std::memcpy(&r, c->h_pinned, sizeof r);
        gr_unpack(r, stats);
        stats->n_degenerate = r.n_deg;
        stats->pairs = (int64_t)r.pairs;
        KMCF_HIP(hipEventElapsedTime(&stats->ms, c->ev_t0, c->ev_t1));
    }
    return KMCF_OK;
}
