// Filament gap analysis: nearest approach of two site sets per gap cell (kmcf_site_set_gap), and the same with the sets
// derived from the device state -- the conductive matter attached to the left / right electrode (kmcf_filament_gap).
//
// The reference has no counterpart.  Definitions (sets, cells, pairs, tie-break, profile): include/kmcfield.h and
// DESIGN.md, "Filament gap".  The side of a site is the touch word of its conductive cluster (kmcf_clusters.hip).
//
// Launches, all on the compute stream (kmcf_filament_gap: behind the cluster pass and one kernel that forms the sides):
//   1    clear the per-cell words
//   2    counts of the sides per gap cell and for the device                       [integer atomics, one set per wave and cell]
//   3-5  compact, per INDEX cell (the cells of kmcf_compute_cutoff_list), the B members with their coordinates and gap
//        cell, and the A members: the shared compaction of kmcf_cellmembers.hpp (two sets in one pass; gp_rule, gp_emit),
//        on scratch of this file's own (kmcf_poisson_gridless keeps its lists)
//   6    search: 16 lanes per A site walk the contiguous runs of the 27 surrounding index cells (r_max <= cell edge;
//        kmcf_walk_columns of kmcf_cellwalk.hpp), every lane keeps its lexicographic minimum (d2, b); the group's minimum is
//        stored per A site and lowers the gap cell's best d2 with a 64-bit integer atomicMin on the bit pattern
//        (non-negative doubles order as integers)
//   7    among the A sites that attain their cell's d2, the smallest packed (a << 32 | b) wins (atomicMin again)
//   8    the records; 9 (kmcf_filament_gap with a profile) the histogram
//
// Pruning: before a run of index cells is walked, its distance from the A site (a lower bound, shortened by a margin that
// covers the rounding of the cell assignment) is compared with the smallest d2 known so far -- r_max^2, the gap cell's
// current best (read once per A site; whatever value it has is >= the final one) and what the group has found in the runs
// before.  A run is skipped only if its bound is GREATER: every b at the final minimum of the cell, ties included, lies
// in a run that is walked, so the A sites that attain the minimum hold their exact (d2, smallest b), and the others --
// whose stored minimum may be too large or missing -- never enter step 7.  The result does not depend on what was read.
//
// Periodic index (kmcf_site_set_gap_pbc / kmcf_filament_gap_pbc on an index of kmcf_compute_cutoff_list_pbc with pbc = 1):
// step 6 is gp_search_kernel on the periodic geometry (kmcf_cell_grid_pbc) -- the minimum image in y and z, the wrapped
// cells each once, the bound in y taken to the face through which the neighbour cell is adjacent ("Periodic
// search"); every other step, and everything in step 6 but the walk and the distance, is shared.
//
// Determinism: counts are integer adds, the minimum d2 and the packed pair are integer minima: every output is
// independent of the execution order.  No thread waits for another.
#include <cmath>
#include <limits>

#include "kmcf_cellwalk.hpp"

static_assert(sizeof(kmcf_gap_t) == 56, "kmcf_gap_t is 56 bytes");

struct kmcf_gap_ws {
    int N = 0;                                   // the index's N: the per-site arrays hold that many
    int *d_side = nullptr;                       // side per site (kmcf_filament_gap without d_site_side)
    kmcf_members b;                              // B members with coordinates; d_sum: the A and the B flags
    int *d_bcell = nullptr;                      // ... and their gap cells
    int *d_alist = nullptr, *d_acell = nullptr;  // A members (index-cell order) and their gap cells
    unsigned long long *d_ad2 = nullptr;         // per A member: bits of its smallest d2 (+inf: none seen)
    int *d_ab = nullptr;                         // ... and the b that gives it (-1: none)
    int *d_stats = nullptr;                      // GP_STAT_* words
    size_t cap_cells = 0;
    unsigned long long *d_best = nullptr, *d_pair = nullptr;    // per gap cell: bits of the smallest d2, packed pair
    int *d_cnt = nullptr;                        // per gap cell: n_left, n_right, n_both
    kmcf_gap_t *d_gaps = nullptr;
    size_t cap_prof = 0;
    int *d_prof = nullptr;
};

void kmcf_gap_ws_free(kmcf_pairwise *p)
{
    if (!p || !p->gap_ws) return;
    kmcf_gap_ws *w = p->gap_ws;
    kmcf_members_free(&w->b);
    kmcf_dev_free_all({w->d_side, w->d_alist, w->d_acell, w->d_bcell, w->d_ad2, w->d_ab, w->d_stats, w->d_best, w->d_pair, w->d_cnt,
                       w->d_gaps, w->d_prof});
    delete w;
    p->gap_ws = nullptr;
}

namespace {

typedef unsigned long long u64;
constexpr int GP_LPS = 16, GP_SPB = KMCF_BLOCK / GP_LPS;          // lanes per A site, A sites per block
constexpr int GP_KIND_VACANCY = KMCF_CLUSTER_VACANCY;
enum { GP_STAT_LEFT, GP_STAT_RIGHT, GP_STAT_BOTH, GP_STAT_BRIDGED, GP_STAT_OPEN, GP_STAT_NONE, GP_STAT_WORDS = 8 };

// the sides: touch word of the site's cluster, 0 for non-members
__global__ __launch_bounds__(KMCF_BLOCK) void gp_side_kernel(int N, const unsigned char *__restrict__ cls,
                                                             const int *__restrict__ label, const int *__restrict__ touch,
                                                             int *__restrict__ side)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i < N) side[i] = cls[i] ? (touch[label[i]] & 3) : 0;
}

// 1
__global__ __launch_bounds__(KMCF_BLOCK) void gp_clear_kernel(size_t n_cells, u64 *__restrict__ best, u64 *__restrict__ pair,
                                                              int *__restrict__ cnt, int *__restrict__ stats)
{
    const size_t c = (size_t)blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (c < n_cells) {
        best[c] = KMCF_D2_INF;
        pair[c] = KMCF_NO_PAIR;
        cnt[3 * c] = cnt[3 * c + 1] = cnt[3 * c + 2] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x < GP_STAT_WORDS) stats[threadIdx.x] = 0;
}

// 2: a wave adds once per gap cell it meets (the sites of one cell lie together in most orders), once for the device
__global__ __launch_bounds__(KMCF_BLOCK) void gp_count_kernel(int N, const int *__restrict__ side,
                                                              const int *__restrict__ site_cell, int n_cells, int *cnt, int *stats)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int s = i < N ? (side[i] & 3) : 0;
    const int c = s ? kmcf_site_cell(site_cell, n_cells, i) : -1;
    const u64 d1 = __ballot(s & 1), d2 = __ballot(s & 2), d3 = __ballot(s == 3);
    if (lane == 0) {
        if (d1) atomicAdd(stats + GP_STAT_LEFT, __popcll(d1));
        if (d2) atomicAdd(stats + GP_STAT_RIGHT, __popcll(d2));
        if (d3) atomicAdd(stats + GP_STAT_BOTH, __popcll(d3));
    }
    bool todo = c >= 0;
    for (u64 act = __ballot(todo); act; act = __ballot(todo)) {
        const int leader = __ffsll((long long)act) - 1;
        const int lc = __shfl(c, leader, 64);
        const bool mine = todo && c == lc;
        const u64 a1 = __ballot(mine && (s & 1)), a2 = __ballot(mine && (s & 2)), a3 = __ballot(mine && s == 3);
        if (lane == leader) {
            int *q = cnt + 3 * (size_t)lc;
            if (a1) atomicAdd(q, __popcll(a1));
            if (a2) atomicAdd(q + 1, __popcll(a2));
            if (a3) atomicAdd(q + 2, __popcll(a3));
        }
        if (mine) todo = false;
    }
}

// 3-5, the members of the search: side bits (set 0: A, set 1: B, the walked one) of a site that lies in a gap cell; the
// B members with coordinates and gap cell, the A members with gap cell
struct gp_rule {
    const int *side, *site_cell;
    int n_cells;
    __device__ __forceinline__ int operator()(int i) const
    {
        const int s = side[i] & 3;
        return (s && kmcf_site_cell(site_cell, n_cells, i) >= 0) ? s : 0;
    }
};
struct gp_emit {
    const int *site_cell;
    int n_cells;
    const double *x, *y, *z;
    kmcf_members b;
    int *bcell, *alist, *acell;
    __device__ __forceinline__ void operator()(int set, int q, int i, int) const
    {
        const int c = kmcf_site_cell(site_cell, n_cells, i);
        if (set == 0) {
            alist[q] = i;
            acell[q] = c;
        } else {
            kmcf_member_put(b, q, i, x, y, z);
            bcell[q] = c;
        }
    }
};

// 6: the search, on the open (GRID = kmcf_cell_grid) or the periodic index (kmcf_cell_grid_pbc: the minimum image in y and
// z).  A group of GP_LPS lanes per A member; the loop runs over whole blocks of groups, so every lane of a wave reaches the
// shuffles behind it.  The threshold is uniform over a group, as the walk requires (kmcf_cellwalk.hpp).
template <class GRID>
__global__ __launch_bounds__(KMCF_BLOCK) void gp_search_kernel(GRID g, const int *__restrict__ cell_start,
                                                               const int *__restrict__ bpos, const int *__restrict__ n_a,
                                                               const int *__restrict__ alist, const int *__restrict__ acell,
                                                               const int *__restrict__ bsite, const int *__restrict__ bcell,
                                                               const double *__restrict__ bx, const double *__restrict__ by,
                                                               const double *__restrict__ bz, const double *__restrict__ x,
                                                               const double *__restrict__ y, const double *__restrict__ z,
                                                               double rmax2, u64 *best, u64 *__restrict__ ad2,
                                                               int *__restrict__ ab)
{
    const int nA = *n_a;
    const int lane = threadIdx.x % GP_LPS;
    const int rows = (nA + GP_SPB - 1) / GP_SPB * GP_SPB;
    const double inf = __longlong_as_double((long long)KMCF_D2_INF);
    for (int k = blockIdx.x * GP_SPB + threadIdx.x / GP_LPS; k < rows; k += gridDim.x * GP_SPB) {
        const bool valid = k < nA;
        double bd = inf;                    // this lane's minimum (d2, b)
        int bb = 0x7fffffff;
        int ca = -1;
        if (valid) {
            const int a = alist[k];
            ca = acell[k];
            const double xa = x[a], ya = y[a], za = z[a];
            double thr = rmax2;             // no pair with a larger d2 can be the result (uniform over the group)
            // (the group's first lane's read for all of them: the walk must not part the group's lanes)
            const double seen = __shfl(__longlong_as_double((long long)kmcf_load_relaxed(best + ca)), 0, GP_LPS);
            if (seen < thr) thr = seen;
            kmcf_walk_columns(
                g, xa, ya, za, cell_start, bpos, [&](double bound) { return !(bound > thr); },
                [&](int b, int e) {
                    for (int t = b + lane; t < e; t += GP_LPS) {
                        if (bcell[t] != ca) continue;
                        const double d2 = kmcf_walk_d2(g, xa, ya, za, bx[t], by[t], bz[t]);
                        if (d2 <= rmax2) {
                            const int j = bsite[t];                  // (j == a is a pair like any other)
                            if (d2 < bd || (d2 == bd && j < bb)) { bd = d2; bb = j; }
                        }
                    }
                },
                [&]() {
                    double m = bd;
#pragma unroll
                    for (int off = GP_LPS / 2; off >= 1; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
                    if (m < thr) thr = m;
                });
        }
#pragma unroll
        for (int off = GP_LPS / 2; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int ob = __shfl_xor(bb, off, 64);
            if (od < bd || (od == bd && ob < bb)) { bd = od; bb = ob; }
        }
        if (valid && lane == 0) {
            const bool found = bb != 0x7fffffff;
            const u64 bits = (u64)__double_as_longlong(bd);
            ad2[k] = bits;
            ab[k] = found ? bb : -1;
            if (found) atomicMin(best + ca, bits);
        }
    }
}

// 7: best[] is final (earlier launch); few A members attain it
__global__ __launch_bounds__(KMCF_BLOCK) void gp_pair_kernel(const int *__restrict__ n_a, const int *__restrict__ alist,
                                                             const int *__restrict__ acell, const u64 *__restrict__ ad2,
                                                             const int *__restrict__ ab, const u64 *__restrict__ best, u64 *pair)
{
    const int nA = *n_a;
    for (int k = blockIdx.x * KMCF_BLOCK + threadIdx.x; k < nA; k += gridDim.x * KMCF_BLOCK) {
        const int b = ab[k];
        if (b < 0) continue;
        const int c = acell[k];
        if (ad2[k] == best[c]) atomicMin(pair + c, ((u64)(unsigned)alist[k] << 32) | (unsigned)b);
    }
}

// 8: the records (gap is filled in on the host: sqrt of gap2) and the cell counts
__global__ __launch_bounds__(KMCF_BLOCK) void gp_record_kernel(size_t n_cells, const u64 *__restrict__ best,
                                                               const u64 *__restrict__ pair, const int *__restrict__ cnt,
                                                               const double *__restrict__ x, kmcf_gap_t *__restrict__ gaps,
                                                               int *stats)
{
    const size_t c = (size_t)blockIdx.x * KMCF_BLOCK + threadIdx.x;
    int state = -1;                          // 0 bridged, 1 open, 2 none
    if (c < n_cells) {
        kmcf_gap_t r;
        const u64 pr = pair[c];
        r.n_left = cnt[3 * c]; r.n_right = cnt[3 * c + 1]; r.n_both = cnt[3 * c + 2];
        r.bridged = r.n_both > 0;
        if (pr == KMCF_NO_PAIR) {
            r.gap = r.gap2 = __longlong_as_double((long long)KMCF_D2_INF);
            r.x_left = r.x_right = 0.0;
            r.site_left = r.site_right = -1;
        } else {
            r.gap2 = __longlong_as_double((long long)best[c]);
            r.gap = r.gap2;
            r.site_left = (int)(pr >> 32);
            r.site_right = (int)(pr & 0xffffffffull);
            r.x_left = x[r.site_left];
            r.x_right = x[r.site_right];
        }
        gaps[c] = r;
        state = r.bridged ? 0 : (pr == KMCF_NO_PAIR ? 2 : 1);
    }
    const u64 m0 = __ballot(state == 0), m1 = __ballot(state == 1), m2 = __ballot(state == 2);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(stats + GP_STAT_BRIDGED, __popcll(m0));
        if (m1) atomicAdd(stats + GP_STAT_OPEN, __popcll(m1));
        if (m2) atomicAdd(stats + GP_STAT_NONE, __popcll(m2));
    }
}

// 9: conductive vacancies per gap cell, x bin and side (integer atomics)
__global__ __launch_bounds__(KMCF_BLOCK) void gp_profile_kernel(int N, const unsigned char *__restrict__ cls,
                                                                const int *__restrict__ side, const int *__restrict__ site_cell,
                                                                int n_cells, const double *__restrict__ x, int n_bins, double x_lo,
                                                                double inv_w, int *prof)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i >= N || cls[i] != GP_KIND_VACANCY) return;
    const int s = side[i] & 3;
    if (!s) return;
    const int c = kmcf_site_cell(site_cell, n_cells, i);
    if (c < 0) return;
    const double t = (x[i] - x_lo) * inv_w;
    if (t >= 0.0 && t < (double)n_bins) atomicAdd(prof + ((size_t)c * n_bins + (int)t) * 3 + (s - 1), 1);
}

// scratch on the index, grown on demand and freed by kmcf_pairwise_destroy; it holds nothing a later call reads
int gp_workspace(kmcf_pairwise *p, size_t n_cells, size_t prof_words)
{
    if (!p->gap_ws) {
        kmcf_gap_ws *w = p->gap_ws = new kmcf_gap_ws();
        const size_t n = (size_t)p->N;
        w->N = p->N;
        KMCF_TRY(kmcf_members_alloc(&w->b, p->N, 2, true));
        KMCF_TRY(kmcf_dev_alloc(&w->d_side, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_alist, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_acell, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_bcell, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_ad2, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_ab, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_stats, (size_t)GP_STAT_WORDS, false));
    }
    kmcf_gap_ws *w = p->gap_ws;
    if (w->cap_cells < n_cells) {                      // four buffers of one capacity, exact size
        w->cap_cells = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_best, nullptr, n_cells, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_pair, nullptr, n_cells, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_cnt, nullptr, 3 * n_cells, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_gaps, nullptr, n_cells, 0));
        w->cap_cells = n_cells;
    }
    if (w->cap_prof < prof_words) KMCF_TRY(kmcf_dev_grow(&w->d_prof, &w->cap_prof, prof_words, 0));
    return KMCF_OK;
}

// the argument checks both entry points share; p comes last: everything before it is checked without an index
int gp_check_common(const char *what, const kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                    double r_max, const int *d_site_cell, int n_cells, const kmcf_gap_t *h_gaps, bool periodic_ok)
{
    KMCF_TRY(kmcf_check_coords(what, d_x, d_y, d_z));
    KMCF_CHECK(h_gaps, KMCF_ERR_ARG, "%s: h_gaps is NULL", what);
    KMCF_TRY(kmcf_check_radius(what, "r_max", r_max));
    KMCF_TRY(kmcf_check_cells(what, d_site_cell, n_cells));
    return kmcf_check_index(what, p, "r_max", r_max, periodic_ok ? nullptr : "gap");
}

// steps 1-8 (and 9 with cls and a profile) enqueued behind whatever produced d_side
int gp_enqueue(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z, const int *d_side, double r_max,
               const int *d_site_cell, int n_cells, const unsigned char *d_cls, int n_bins, double x_lo, double x_hi,
               bool profile)
{
    kmcf_gap_ws *w = p->gap_ws;
    hipStream_t st = p->comm->stream;
    const int N = p->N;
    const int site_grid = (N + KMCF_BLOCK - 1) / KMCF_BLOCK;
    const size_t nc = (size_t)n_cells;
    const int cell_grid = (int)((nc + KMCF_BLOCK - 1) / KMCF_BLOCK);
    const int *n_a = w->b.d_sum + kmcf_member_tiles(N);
    int64_t search_grid = ((int64_t)N + GP_SPB - 1) / GP_SPB;      // an upper bound: the kernel strides over the A members
    if (search_grid > 8192) search_grid = 8192;
    int64_t pair_grid = site_grid;
    if (pair_grid > 2048) pair_grid = 2048;

    gp_clear_kernel<<<cell_grid, KMCF_BLOCK, 0, st>>>(nc, w->d_best, w->d_pair, w->d_cnt, w->d_stats);
    gp_count_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, d_side, d_site_cell, n_cells, w->d_cnt, w->d_stats);
    kmcf_members_enqueue<2>(p, w->b, gp_rule{d_side, d_site_cell, n_cells},
                            gp_emit{d_site_cell, n_cells, d_x, d_y, d_z, w->b, w->d_bcell, w->d_alist, w->d_acell});
    p->with_grid([&](auto grid) {
        gp_search_kernel<<<(int)search_grid, KMCF_BLOCK, 0, st>>>(grid, p->d_cell_start, w->b.d_pos, n_a, w->d_alist, w->d_acell,
                                                                 w->b.d_site, w->d_bcell, w->b.d_x, w->b.d_y, w->b.d_z, d_x, d_y,
                                                                 d_z, r_max * r_max, w->d_best, w->d_ad2, w->d_ab);
    });
    gp_pair_kernel<<<(int)pair_grid, KMCF_BLOCK, 0, st>>>(n_a, w->d_alist, w->d_acell, w->d_ad2, w->d_ab, w->d_best, w->d_pair);
    gp_record_kernel<<<cell_grid, KMCF_BLOCK, 0, st>>>(nc, w->d_best, w->d_pair, w->d_cnt, d_x, w->d_gaps, w->d_stats);
    if (profile) {
        const size_t words = nc * (size_t)n_bins * 3;
        KMCF_HIP(hipMemsetAsync(w->d_prof, 0, words * sizeof(int), st));
        gp_profile_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, d_cls, d_side, d_site_cell, n_cells, d_x, n_bins, x_lo,
                                                           (double)n_bins / (x_hi - x_lo), w->d_prof);
    }
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// the copies, the call's one synchronisation, and what the host adds
int gp_finish(kmcf_pairwise *p, int n_cells, kmcf_gap_t *h_gaps, size_t prof_words, int *h_profile, hipEvent_t ev_mid,
              kmcf_gap_stats_t *stats)
{
    kmcf_comm *c = p->comm;
    kmcf_gap_ws *w = p->gap_ws;
    hipStream_t st = c->stream;
    int *h = c->h_pinned;
    KMCF_HIP(hipMemcpyAsync(h_gaps, w->d_gaps, (size_t)n_cells * sizeof(kmcf_gap_t), hipMemcpyDeviceToHost, st));
    if (prof_words) KMCF_HIP(hipMemcpyAsync(h_profile, w->d_prof, prof_words * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h, w->d_stats, GP_STAT_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(c->ev_call1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < n_cells; ++k) h_gaps[k].gap = std::sqrt(h_gaps[k].gap2);
    if (stats) {
        stats->n_left = h[GP_STAT_LEFT];
        stats->n_right = h[GP_STAT_RIGHT];
        stats->n_both = h[GP_STAT_BOTH];
        stats->cells_bridged = h[GP_STAT_BRIDGED];
        stats->cells_open = h[GP_STAT_OPEN];
        stats->cells_none = h[GP_STAT_NONE];
        stats->ms_clusters = 0.f;
        if (ev_mid) KMCF_HIP(hipEventElapsedTime(&stats->ms_clusters, c->ev_t0, ev_mid));
        KMCF_HIP(hipEventElapsedTime(&stats->ms_search, ev_mid ? ev_mid : c->ev_t0, c->ev_call1));
    }
    return KMCF_OK;
}

// the body of kmcf_site_set_gap and kmcf_site_set_gap_pbc: they differ in the name and in whether a periodic index passes
int gp_site_set_gap(const char *what, bool periodic_ok, kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                    const int *d_site_side, double r_max, const int *d_site_cell, int n_cells, kmcf_gap_t *h_gaps,
                    kmcf_gap_stats_t *stats)
{
    KMCF_CHECK(d_site_side, KMCF_ERR_ARG, "%s: d_site_side is NULL", what);
    KMCF_TRY(gp_check_common(what, p, d_x, d_y, d_z, r_max, d_site_cell, n_cells, h_gaps, periodic_ok));
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(gp_workspace(p, (size_t)n_cells, 0));
    KMCF_HIP(hipEventRecord(c->ev_t0, c->stream));
    KMCF_TRY(gp_enqueue(p, d_x, d_y, d_z, d_site_side, r_max, d_site_cell, n_cells, nullptr, 0, 0.0, 0.0, false));
    return gp_finish(p, n_cells, h_gaps, 0, nullptr, nullptr, stats);
}

// the body of kmcf_filament_gap and kmcf_filament_gap_pbc
int gp_filament_gap(const char *what, bool periodic_ok, kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                    const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x, const double *d_y,
                    const double *d_z, int N_left_tot, int N_right_tot, double r_max, const int *d_site_cell, int n_cells,
                    kmcf_gap_t *h_gaps, int n_bins, double x_lo, double x_hi, int *h_profile, int *d_site_side,
                    kmcf_gap_stats_t *stats)
{
    KMCF_CHECK(d_neigh_idx, KMCF_ERR_ARG, "%s: d_neigh_idx is NULL", what);
    KMCF_CHECK(d_site_element, KMCF_ERR_ARG, "%s: d_site_element is NULL", what);
    KMCF_CHECK(d_site_charge, KMCF_ERR_ARG, "%s: d_site_charge is NULL", what);
    KMCF_CHECK(nn > 0, KMCF_ERR_ARG, "%s: nn = %d is not > 0", what, nn);
    KMCF_CHECK(num_metals >= 0, KMCF_ERR_ARG, "%s: num_metals = %d is negative", what, num_metals);
    KMCF_CHECK(num_metals == 0 || d_metals, KMCF_ERR_ARG, "%s: d_metals is NULL with num_metals = %d", what, num_metals);
    KMCF_CHECK(N_left_tot >= 0, KMCF_ERR_ARG, "%s: N_left_tot = %d is negative", what, N_left_tot);
    KMCF_CHECK(N_right_tot >= 0, KMCF_ERR_ARG, "%s: N_right_tot = %d is negative", what, N_right_tot);
    KMCF_CHECK(n_bins >= 0, KMCF_ERR_ARG, "%s: n_bins = %d is negative", what, n_bins);
    KMCF_CHECK(!h_profile || n_bins > 0, KMCF_ERR_ARG, "%s: h_profile is set with n_bins = 0", what);
    KMCF_CHECK(!h_profile || x_hi > x_lo, KMCF_ERR_ARG, "%s: h_profile is set with x_hi = %g not above x_lo = %g", what, x_hi, x_lo);
    KMCF_TRY(gp_check_common(what, p, d_x, d_y, d_z, r_max, d_site_cell, n_cells, h_gaps, periodic_ok));
    const int N = p->N;
    KMCF_CHECK((int64_t)N_left_tot + N_right_tot <= N, KMCF_ERR_ARG, "%s: N_left_tot + N_right_tot = %lld exceeds N = %d", what,
               (long long)N_left_tot + N_right_tot, N);
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    const size_t prof_words = h_profile ? (size_t)n_cells * (size_t)n_bins * 3 : 0;
    KMCF_TRY(gp_workspace(p, (size_t)n_cells, prof_words));
    kmcf_gap_ws *w = p->gap_ws;
    hipStream_t st = c->stream;
    int *side = d_site_side ? d_site_side : w->d_side;
    kmcf_cluster_dev cl;
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    KMCF_TRY(kmcf_clusters_enqueue(c, N, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals, d_x, N_left_tot,
                                   N_right_tot, nullptr, false, 0, &cl));
    gp_side_kernel<<<(N + KMCF_BLOCK - 1) / KMCF_BLOCK, KMCF_BLOCK, 0, st>>>(N, cl.cls, cl.label, cl.touch, side);
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    KMCF_TRY(gp_enqueue(p, d_x, d_y, d_z, side, r_max, d_site_cell, n_cells, cl.cls, n_bins, x_lo, x_hi, h_profile != nullptr));
    return gp_finish(p, n_cells, h_gaps, prof_words, h_profile, c->ev_t1, stats);
}

}  // namespace

extern "C" int kmcf_site_set_gap(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                 const int *d_site_side, double r_max, const int *d_site_cell, int n_cells,
                                 kmcf_gap_t *h_gaps, kmcf_gap_stats_t *stats)
{
    return gp_site_set_gap("kmcf_site_set_gap", false, p, d_x, d_y, d_z, d_site_side, r_max, d_site_cell, n_cells, h_gaps, stats);
}

extern "C" int kmcf_site_set_gap_pbc(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                     const int *d_site_side, double r_max, const int *d_site_cell, int n_cells,
                                     kmcf_gap_t *h_gaps, kmcf_gap_stats_t *stats)
{
    return gp_site_set_gap("kmcf_site_set_gap_pbc", true, p, d_x, d_y, d_z, d_site_side, r_max, d_site_cell, n_cells, h_gaps, stats);
}

extern "C" int kmcf_filament_gap(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                                 const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                                 const double *d_y, const double *d_z, int N_left_tot, int N_right_tot, double r_max,
                                 const int *d_site_cell, int n_cells, kmcf_gap_t *h_gaps, int n_bins, double x_lo, double x_hi,
                                 int *h_profile, int *d_site_side, kmcf_gap_stats_t *stats)
{
    return gp_filament_gap("kmcf_filament_gap", false, p, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals, d_x,
                           d_y, d_z, N_left_tot, N_right_tot, r_max, d_site_cell, n_cells, h_gaps, n_bins, x_lo, x_hi, h_profile,
                           d_site_side, stats);
}

extern "C" int kmcf_filament_gap_pbc(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                                     const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                                     const double *d_y, const double *d_z, int N_left_tot, int N_right_tot, double r_max,
                                     const int *d_site_cell, int n_cells, kmcf_gap_t *h_gaps, int n_bins, double x_lo,
                                     double x_hi, int *h_profile, int *d_site_side, kmcf_gap_stats_t *stats)
{
    return gp_filament_gap("kmcf_filament_gap_pbc", true, p, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals,
                           d_x, d_y, d_z, N_left_tot, N_right_tot, r_max, d_site_cell, n_cells, h_gaps, n_bins, x_lo, x_hi,
                           h_profile, d_site_side, stats);
}
