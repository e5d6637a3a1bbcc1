// The list that a walk over the spatial index reads (kmcf_cellwalk.hpp), built once for every pass that walks: the
// flagged sites ("members") compacted in index-cell order with the payload the pass wants, and pos[N + 1], the list
// position of every slot of the cell order, so that a run of index cells is a contiguous [b, e) of the list.  Used by
// kmcf_pairwise.hip, kmcf_gap.hip, kmcf_chain.hip, kmcf_paircorr.hip and kmcf_fieldsample.hip; each hands in
//   RULE   rule(i): the flag word of site i; bit s: "in set s" (s < SETS); the bits from SETS up are the rule's own and
//          reach the emitter untouched (the pair correlation keeps the site's class there: read once per item)
//   EMIT   emit(set, q, i, word): site i is member q of the set; called in item order, per item lowest set first
// both small structs passed by value.  The walked set -- the one pos[] describes -- is the last.  Three launches:
//   kmcf_member_count_kernel     per tile and set the number of members          -> sum[set * (nb + 1) + tile]
//   kmcf_scan_counts_kernel      one block per set, in place                     -> offsets; a set's total in sum[set * (nb + 1) + nb]
//   kmcf_member_scatter_kernel   the rule again, the positions, pos[], emit
// Output order = cell order, whatever the execution order: the lists are the same bits in every run.  A thread evaluates
// the rule over its KMCF_SCAN_ITEMS items in ascending order.  As kmcf_block.hpp: templates in an anonymous namespace, no
// relocatable device code.  New passes that walk the index use this; they do not copy it.
//
// Also here, for the same passes: the scratch of the list (kmcf_members, kmcf_internal.hpp) and the argument checks
// they share.
#pragma once
#include "kmcf_internal.hpp"

namespace {

template <int SETS, class RULE>
__global__ __launch_bounds__(KMCF_BLOCK) void kmcf_member_count_kernel(int N, int nb, const int *__restrict__ cell_order, RULE rule,
                                                                       int *__restrict__ sum)
{
    __shared__ int lds[4];
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(N, f, [&](int t) { return rule(cell_order[t]); });
#pragma unroll
    for (int s = 0; s < SETS; ++s) {
        const int total = kmcf_tile_count(f, lds, 1 << s);
        if (threadIdx.x == 0) sum[s * (nb + 1) + blockIdx.x] = total;
    }
}

template <int SETS, class RULE, class EMIT>
__global__ __launch_bounds__(KMCF_BLOCK) void kmcf_member_scatter_kernel(int N, int nb, const int *__restrict__ cell_order, RULE rule,
                                                                         const int *__restrict__ sum, int *__restrict__ pos,
                                                                         EMIT emit)
{
    __shared__ int lds[4];
    const int t0 = kmcf_tile_item0();
    int f[KMCF_SCAN_ITEMS], site[KMCF_SCAN_ITEMS], q[SETS];
    kmcf_tile_flags(N, f, [&](int t) { return rule(site[t - t0] = cell_order[t]); });
#pragma unroll
    for (int s = 0; s < SETS; ++s) q[s] = kmcf_tile_pos(f, sum[s * (nb + 1) + blockIdx.x], lds, 1 << s);
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k) {
        const int t = t0 + k;
        if (t >= N) break;
        pos[t] = q[SETS - 1];           // every slot: the runs of the walk start at cell boundaries
#pragma unroll
        for (int s = 0; s < SETS; ++s)
            if (f[k] >> s & 1) emit(s, q[s]++, site[k], f[k]);
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == KMCF_BLOCK - 1) pos[N] = sum[SETS * (nb + 1) - 1];
}

// what most emitters do with a member of the walked set: its site and coordinates
__device__ __forceinline__ void kmcf_member_put(const kmcf_members &m, int q, int i, const double *__restrict__ x,
                                                const double *__restrict__ y, const double *__restrict__ z)
{
    m.d_site[q] = i;
    m.d_x[q] = x[i];
    m.d_y[q] = y[i];
    m.d_z[q] = z[i];
}

inline int kmcf_member_tiles(int N) { return (N + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE; }

// the three launches on the compute stream; m.d_sum + set * (tiles + 1) + tiles then holds the set's number of members
template <int SETS, class RULE, class EMIT>
void kmcf_members_enqueue(const kmcf_pairwise *p, const kmcf_members &m, RULE rule, EMIT emit)
{
    hipStream_t st = p->comm->stream;
    const int N = p->N, nb = kmcf_member_tiles(N);
    kmcf_member_count_kernel<SETS><<<nb, KMCF_BLOCK, 0, st>>>(N, nb, p->d_cell_order, rule, m.d_sum);
    kmcf_scan_counts_kernel<int><<<SETS, KMCF_BLOCK, 0, st>>>(nb, m.d_sum, m.d_sum, nb + 1);
    kmcf_member_scatter_kernel<SETS><<<nb, KMCF_BLOCK, 0, st>>>(N, nb, p->d_cell_order, rule, m.d_sum, m.d_pos, emit);
}

// the list's scratch for an index of N sites
inline int kmcf_members_alloc(kmcf_members *m, int N, int sets, bool coords)
{
    const size_t n = (size_t)N;
    KMCF_TRY(kmcf_dev_alloc(&m->d_pos, n + 1, false));
    KMCF_TRY(kmcf_dev_alloc(&m->d_sum, (size_t)sets * ((size_t)kmcf_member_tiles(N) + 1), false));
    KMCF_TRY(kmcf_dev_alloc(&m->d_site, n, false));
    if (coords)
        for (double **d : {&m->d_x, &m->d_y, &m->d_z}) KMCF_TRY(kmcf_dev_alloc(d, n, false));
    return KMCF_OK;
}

inline void kmcf_members_free(kmcf_members *m)
{
    kmcf_dev_free_all({m->d_pos, m->d_sum, m->d_site, m->d_x, m->d_y, m->d_z});
    *m = kmcf_members();
}

// ---------------------------------------------------------------- argument checks of the analysis passes
inline int kmcf_check_coords(const char *what, const double *d_x, const double *d_y, const double *d_z)
{
    KMCF_CHECK(d_x, KMCF_ERR_ARG, "%s: d_x is NULL", what);
    KMCF_CHECK(d_y, KMCF_ERR_ARG, "%s: d_y is NULL", what);
    KMCF_CHECK(d_z, KMCF_ERR_ARG, "%s: d_z is NULL", what);
    return KMCF_OK;
}

inline int kmcf_check_radius(const char *what, const char *name, double r)
{
    KMCF_CHECK(std::isfinite(r), KMCF_ERR_ARG, "%s: %s is not finite", what, name);
    KMCF_CHECK(r > 0.0, KMCF_ERR_ARG, "%s: %s = %g is not > 0", what, name, r);
    return KMCF_OK;
}

inline int kmcf_check_cells(const char *what, const int *d_site_cell, int n_cells)
{
    KMCF_CHECK(n_cells >= 1, KMCF_ERR_ARG, "%s: n_cells = %d is not >= 1", what, n_cells);
    KMCF_CHECK(d_site_cell || n_cells == 1, KMCF_ERR_ARG, "%s: d_site_cell is NULL with n_cells = %d", what, n_cells);
    return KMCF_OK;
}

// p comes last in every pass: everything before it is checked without an index.  open_search ("gap", "chain"): the call
// is the non-periodic search of that name, which a periodic index does not pass; nullptr: either index passes.
inline int kmcf_check_index(const char *what, const kmcf_pairwise *p, const char *name, double r, const char *open_search)
{
    KMCF_CHECK(p, KMCF_ERR_ARG, "%s: p is NULL", what);
    KMCF_CHECK(!open_search || !p->pbc, KMCF_ERR_ARG, "%s: the index is periodic (kmcf_compute_cutoff_list_pbc with pbc = 1) and "
               "this %s search is non-periodic: call %s_pbc for the minimum image, or build a non-periodic index", what,
               open_search, what);
    KMCF_CHECK(r <= p->cutoff, KMCF_ERR_ARG, "%s: %s = %g exceeds the index's cutoff radius %g", what, name, r, p->cutoff);
    return KMCF_OK;
}

}  // namespace
