// Pair correlation: pair-distance histograms per class pair and cell, and counts of class members around every centre
// (kmcf_pair_correlation), and the same with the classes derived from the device state (kmcf_defect_correlation).
//
// The reference has no counterpart.  Definitions (classes, distance, pair, bins, class pair, bucket, outputs):
// include/kmcfield.h and DESIGN.md 3.16.
//
// Launches, all on the compute stream (kmcf_defect_correlation: behind one kernel that forms the classes):
//   0    hipMemsetAsync of the histogram, the member counts, the packed maximum and (if asked for) the count rows
//   1    members per bucket and class                                  [integer atomics, one per wave and (bucket, class)]
//   2-4  compact, per INDEX cell (the cells of kmcf_compute_cutoff_list), the centres (members and probes) with class and
//        bucket cell, and the members with site id, class, bucket cell and coordinates: the shared compaction of
//        kmcf_cellmembers.hpp (pc_rule, pc_emit), two sets in one pass, on scratch of this file's own
//   5    walk: 16 lanes per centre stride over the contiguous runs of the 27 surrounding index cells (r_max <= cell edge;
//        kmcf_walk_columns of kmcf_cellwalk.hpp); the counts of a centre's row in registers, reduced over the group by
//        shuffles; the histogram in LDS for the bucket of the block's first centre, in global memory for the others
//
// Each pair once: a member centre a adds a partner b to the histogram only when b > a by site id.  The walk visits every
// wrapped index cell once, so a meets b once and b meets a once; both compute the same bits of d2 (kmcf_walk_d2 is even in
// the difference), so both decide d2 <= r_max^2 alike, and exactly the end with the smaller id counts the pair.
//
// The bin is defined by the table edge2[] (formed on the host, the contract's expression): the kernel guesses with
// sqrt(d2) * (n_bins / r_max) and then steps the guess down while edge2[k] > d2 and up while edge2[k + 1] <= d2.
//
// Determinism: every accumulation is an integer add or an integer maximum: every output is independent of the execution
// order.  No atomics on doubles.  No thread waits for another.
#include <cmath>

#include "kmcf_cellwalk.hpp"

static_assert(sizeof(kmcf_pair_stats_t) == 32, "kmcf_pair_stats_t is 32 bytes");

struct kmcf_pc_ws {
    int *d_class = nullptr;                      // class per site (kmcf_defect_correlation without d_site_class)
    kmcf_members m;                              // members (index-cell order) with coordinates; d_sum: the centre and the member flags
    int *d_mcls = nullptr, *d_mcell = nullptr;   // ... their class and bucket cell
    int *d_csite = nullptr, *d_ccls = nullptr, *d_ccell = nullptr;    // centres (index-cell order): site, class, bucket cell
    unsigned long long *d_max = nullptr;         // packed (largest row sum << 32 | ~site); 0: no centre
    size_t cap_hist = 0, cap_members = 0;
    unsigned long long *d_hist = nullptr;
    int *d_members = nullptr;
};

void kmcf_pc_ws_free(kmcf_pairwise *p)
{
    if (!p || !p->pc_ws) return;
    kmcf_pc_ws *w = p->pc_ws;
    kmcf_members_free(&w->m);
    kmcf_dev_free_all({w->d_class, w->d_csite, w->d_ccls, w->d_ccell, w->d_mcls, w->d_mcell, w->d_max, w->d_hist, w->d_members});
    delete w;
    p->pc_ws = nullptr;
}

namespace {

typedef unsigned long long u64;
constexpr int PC_LPS = 16, PC_SPB = KMCF_BLOCK / PC_LPS;          // lanes per centre, centres per block and pass
constexpr int PC_MAX_PASSES = 4;                                  // passes of PC_SPB consecutive centres per block
constexpr int PC_MAX_CLS = KMCF_PC_MAX_CLASSES, PC_MAX_BINS = KMCF_PC_MAX_BINS;
constexpr int PC_MAX_PAIRS = PC_MAX_CLS * (PC_MAX_CLS + 1) / 2;
constexpr int PC_LDS_WORDS = PC_MAX_PAIRS * PC_MAX_BINS;          // 2560 32-bit counters: 10 KB
constexpr int64_t PC_MAX_HIST = (int64_t)1 << 24;
constexpr int EL_OXYGEN_DEFECT = 1, EL_VACANCY = 2;               // src/utils.h:37-44

struct pc_edges { double e2[PC_MAX_BINS + 1]; };                  // the table, handed to the walk as a kernel argument

// the classes of kmcf_defect_correlation
__global__ __launch_bounds__(KMCF_BLOCK) void pc_class_kernel(int N, const int *__restrict__ element, const int *__restrict__ charge,
                                                              int probe_all, int *__restrict__ cls)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int e = element[i];
    int c = probe_all ? 3 : -1;
    if (e == EL_VACANCY) c = charge[i] == 0 ? 0 : 1;
    else if (e == EL_OXYGEN_DEFECT) c = 2;
    cls[i] = c;
}

// 2-4, the lists: set 0 the centres (members and probes) with class and bucket cell, set 1 (the walked one) the members
// with class, bucket cell and coordinates.  A centre's class rides in the flag word above the two set bits
struct pc_rule {
    const int *site_class;
    int n_classes;
    __device__ __forceinline__ int operator()(int i) const
    {
        const int cl = site_class[i];
        return (unsigned)cl < (unsigned)n_classes ? (cl << 2 | 3) : (cl == n_classes ? (cl << 2 | 1) : 0);
    }
};
struct pc_emit {
    const int *site_cell;
    int n_cells;
    const double *x, *y, *z;
    kmcf_members m;
    int *mcls, *mcell, *csite, *ccls, *ccell;
    __device__ __forceinline__ void operator()(int set, int q, int i, int word) const
    {
        const int c = kmcf_site_cell(site_cell, n_cells, i);
        if (set == 0) {
            csite[q] = i;
            ccls[q] = word >> 2;
            ccell[q] = c;
        } else {
            kmcf_member_put(m, q, i, x, y, z);
            mcls[q] = word >> 2;
            mcell[q] = c;
        }
    }
};

// 1: a wave adds once per (bucket, class) it meets
__global__ __launch_bounds__(KMCF_BLOCK) void pc_members_kernel(int N, const int *__restrict__ site_class, int n_classes,
                                                                const int *__restrict__ site_cell, int n_cells, int *members)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int key = -1;
    if (i < N) {
        const int cl = site_class[i];
        if ((unsigned)cl < (unsigned)n_classes) {
            const int c = kmcf_site_cell(site_cell, n_cells, i);
            key = (c < 0 ? n_cells : c) * n_classes + cl;
        }
    }
    bool todo = key >= 0;
    for (u64 act = __ballot(todo); act; act = __ballot(todo)) {
        const int leader = __ffsll((long long)act) - 1;
        const int lk = __shfl(key, leader, 64);
        const bool mine = todo && key == lk;
        const u64 m = __ballot(mine);
        if (lane == leader) atomicAdd(members + lk, __popcll(m));
        if (mine) todo = false;
    }
}

// 5: the walk, on the open (GRID = kmcf_cell_grid) or the periodic index (kmcf_cell_grid_pbc: the minimum image in y and
// z).  Block b serves the centres [b * passes * PC_SPB, (b + 1) * passes * PC_SPB), PC_SPB per pass, a group of PC_LPS lanes
// each; every pass runs over the whole block, so every lane of a wave reaches the shuffles behind the walk.  The
// threshold r_max^2 is uniform, as the walk requires (kmcf_cellwalk.hpp).
//
// LDS counters: 32 bits, for the pairs of the bucket of the block's first centre (index-cell order keeps a crossbar cell's
// sites together); the others go to global memory.  A centre meets every other site at most once, so one counter receives
// at most one add per (centre of the block, other site): at most passes * PC_SPB * (N - 1) adds.  The host chooses
// passes <= PC_MAX_PASSES with passes * PC_SPB * (N - 1) < 2^32 and, where even one pass does not fit (N > 2^28), lds = 0:
// every pair then goes to global memory.  A counter cannot pass 2^32.
template <class GRID>
__global__ __launch_bounds__(KMCF_BLOCK) void pc_walk_kernel(GRID g, const int *__restrict__ cell_start, const int *__restrict__ mpos,
                                                             const int *__restrict__ n_c, const int *__restrict__ csite,
                                                             const int *__restrict__ ccls, const int *__restrict__ ccell,
                                                             const int *__restrict__ msite, const int *__restrict__ mcls,
                                                             const int *__restrict__ mcell, const double *__restrict__ mx,
                                                             const double *__restrict__ my, const double *__restrict__ mz,
                                                             const double *__restrict__ x, const double *__restrict__ y,
                                                             const double *__restrict__ z, int n_classes, int n_bins,
                                                             int n_cells, double rmax2, double rcount2, double inv_w,
                                                             const pc_edges edges, int passes, int lds, u64 *hist,
                                                             int *__restrict__ site_count, u64 *max_pack)
{
    __shared__ unsigned s_hist[PC_LDS_WORDS];
    __shared__ double s_edge[PC_MAX_BINS + 1];
    const int nC = *n_c;
    const int k0 = blockIdx.x * passes * PC_SPB;
    if (k0 >= nC) return;                                            // (the whole block: nothing was touched)
    const int n_pairs = n_classes * (n_classes + 1) / 2;
    const int words = n_pairs * n_bins;
    for (int w = threadIdx.x; w < words; w += KMCF_BLOCK) s_hist[w] = 0;
    for (int w = threadIdx.x; w <= n_bins; w += KMCF_BLOCK) s_edge[w] = edges.e2[w];
    // the bucket kept in LDS: the first centre's cell, the rest bucket if it has none; -2: none (lds == 0)
    const int c0 = ccell[k0];
    const int lds_bucket = lds ? (c0 < 0 ? n_cells : c0) : -2;
    __syncthreads();
    const int lane = threadIdx.x % PC_LPS;
    for (int pass = 0; pass < passes; ++pass) {
        const int k = k0 + pass * PC_SPB + threadIdx.x / PC_LPS;
        const bool valid = k < nC;
        int cnt[PC_MAX_CLS] = {0, 0, 0, 0};
        int a = 0;
        if (valid) {
            a = csite[k];
            const int cla = ccls[k], ca = ccell[k];
            const bool member = cla < n_classes;
            const double xa = x[a], ya = y[a], za = z[a];
            kmcf_walk_columns(
                g, xa, ya, za, cell_start, mpos, [&](double bound) { return !(bound > rmax2); },
                [&](int b, int e) {
                    for (int t = b + lane; t < e; t += PC_LPS) {
                        const int j = msite[t];
                        if (j == a) continue;
                        const double d2 = kmcf_walk_d2(g, xa, ya, za, mx[t], my[t], mz[t]);
                        if (!(d2 <= rmax2)) continue;
                        const int q = mcls[t];
                        if (d2 <= rcount2) {
#pragma unroll
                            for (int s = 0; s < PC_MAX_CLS; ++s) cnt[s] += (q == s);
                        }
                        if (!member || j < a) continue;              // each pair once: the end with the smaller id counts it
                        const int cb = mcell[t];
                        if (ca < 0 || cb < 0) continue;              // no bucket
                        const int bucket = ca == cb ? ca : n_cells;
                        // the guess, then the table decides
                        int kb = (int)(sqrt(d2) * inv_w);
                        kb = kb < 0 ? 0 : (kb > n_bins - 1 ? n_bins - 1 : kb);
                        while (kb > 0 && s_edge[kb] > d2) --kb;
                        while (kb < n_bins - 1 && s_edge[kb + 1] <= d2) ++kb;
                        const int lo = min(cla, q), hi = max(cla, q);
                        const int w = (lo * n_classes - lo * (lo - 1) / 2 + (hi - lo)) * n_bins + kb;
                        if (bucket == lds_bucket) atomicAdd(s_hist + w, 1u);
                        else atomicAdd(hist + (size_t)bucket * words + w, 1ull);
                    }
                },
                [&]() {});
        }
        int total = 0;
#pragma unroll
        for (int s = 0; s < PC_MAX_CLS; ++s) {
#pragma unroll
            for (int off = PC_LPS / 2; off >= 1; off >>= 1) cnt[s] += __shfl_xor(cnt[s], off, 64);
            total += cnt[s];
        }
        if (valid && lane == 0) {
            if (site_count) {
#pragma unroll
                for (int s = 0; s < PC_MAX_CLS; ++s)
                    if (s < n_classes) site_count[(size_t)a * n_classes + s] = cnt[s];
            }
            atomicMax(max_pack, ((u64)(unsigned)total << 32) | (0xffffffffu - (unsigned)a));
        }
    }
    __syncthreads();
    if (lds_bucket >= 0)
        for (int w = threadIdx.x; w < words; w += KMCF_BLOCK) {
            const unsigned v = s_hist[w];
            if (v) atomicAdd(hist + (size_t)lds_bucket * words + w, (u64)v);
        }
}

// scratch on the index, grown on demand and freed by kmcf_pairwise_destroy; it holds nothing a later call reads
int pc_workspace(kmcf_pairwise *p, size_t hist_words, size_t member_words)
{
    if (!p->pc_ws) {
        kmcf_pc_ws *w = p->pc_ws = new kmcf_pc_ws();
        const size_t n = (size_t)p->N;
        KMCF_TRY(kmcf_members_alloc(&w->m, p->N, 2, true));
        for (int **q : {&w->d_class, &w->d_csite, &w->d_ccls, &w->d_ccell, &w->d_mcls, &w->d_mcell}) KMCF_TRY(kmcf_dev_alloc(q, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_max, (size_t)1, false));
    }
    kmcf_pc_ws *w = p->pc_ws;
    KMCF_TRY(kmcf_dev_grow(&w->d_hist, &w->cap_hist, hist_words, 0));
    KMCF_TRY(kmcf_dev_grow(&w->d_members, &w->cap_members, member_words, 0));
    return KMCF_OK;
}

// the argument checks both entry points share; p comes last: everything before it is checked without an index
int pc_check_common(const char *what, const kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                    int n_classes, double r_max, int n_bins, double r_count, const int *d_site_cell, int n_cells,
                    const u64 *h_hist, const int *h_members)
{
    KMCF_TRY(kmcf_check_coords(what, d_x, d_y, d_z));
    KMCF_CHECK(h_hist, KMCF_ERR_ARG, "%s: h_hist is NULL", what);
    KMCF_CHECK(h_members, KMCF_ERR_ARG, "%s: h_members is NULL", what);
    KMCF_CHECK(n_classes >= 1 && n_classes <= PC_MAX_CLS, KMCF_ERR_ARG, "%s: n_classes = %d is outside 1 ... %d", what, n_classes,
               PC_MAX_CLS);
    KMCF_CHECK(n_bins >= 1 && n_bins <= PC_MAX_BINS, KMCF_ERR_ARG, "%s: n_bins = %d is outside 1 ... %d", what, n_bins, PC_MAX_BINS);
    KMCF_TRY(kmcf_check_radius(what, "r_max", r_max));
    KMCF_TRY(kmcf_check_radius(what, "r_count", r_count));
    KMCF_CHECK(r_count <= r_max, KMCF_ERR_ARG, "%s: r_count = %g exceeds r_max = %g", what, r_count, r_max);
    KMCF_TRY(kmcf_check_cells(what, d_site_cell, n_cells));
    const int64_t words = ((int64_t)n_cells + 1) * (n_classes * (n_classes + 1) / 2) * n_bins;
    KMCF_CHECK(words <= PC_MAX_HIST, KMCF_ERR_ARG, "%s: (n_cells + 1) * n_pairs * n_bins = %lld exceeds 2^24: fewer cells or n_bins",
               what, (long long)words);
    return kmcf_check_index(what, p, "r_max", r_max, nullptr);
}

struct pc_call {
    const double *d_x, *d_y, *d_z;
    int n_classes;
    double r_max;
    int n_bins;
    double r_count;
    const int *d_site_cell;
    int n_cells;
    u64 *h_hist;
    int *h_members;
    double *h_edge2;
    int *d_site_count;
    kmcf_pair_stats_t *stats;
};

// launches 0-5 enqueued behind whatever produced d_site_class
int pc_enqueue(kmcf_pairwise *p, const pc_call &a, const int *d_site_class, const pc_edges &edges)
{
    kmcf_pc_ws *w = p->pc_ws;
    hipStream_t st = p->comm->stream;
    const int N = p->N;
    const int site_grid = (N + KMCF_BLOCK - 1) / KMCF_BLOCK;
    const size_t hist_words = ((size_t)a.n_cells + 1) * (size_t)(a.n_classes * (a.n_classes + 1) / 2) * (size_t)a.n_bins;
    const size_t member_words = ((size_t)a.n_cells + 1) * (size_t)a.n_classes;
    // passes * PC_SPB * (N - 1) < 2^32 (pc_walk_kernel: the LDS counters)
    const uint64_t per_pass = (uint64_t)PC_SPB * (uint64_t)std::max(N - 1, 1);
    const int lds = per_pass < ((uint64_t)1 << 32);
    const int passes = lds ? (int)std::min<uint64_t>(PC_MAX_PASSES, (((uint64_t)1 << 32) - 1) / per_pass) : 1;
    const int walk_grid = (int)(((int64_t)N + passes * PC_SPB - 1) / (passes * PC_SPB));   // an upper bound: N centres

    KMCF_HIP(hipMemsetAsync(w->d_hist, 0, hist_words * sizeof(u64), st));
    KMCF_HIP(hipMemsetAsync(w->d_members, 0, member_words * sizeof(int), st));
    KMCF_HIP(hipMemsetAsync(w->d_max, 0, sizeof(u64), st));
    if (a.d_site_count) KMCF_HIP(hipMemsetAsync(a.d_site_count, 0, (size_t)N * a.n_classes * sizeof(int), st));
    pc_members_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, d_site_class, a.n_classes, a.d_site_cell, a.n_cells, w->d_members);
    kmcf_members_enqueue<2>(p, w->m, pc_rule{d_site_class, a.n_classes},
                            pc_emit{a.d_site_cell, a.n_cells, a.d_x, a.d_y, a.d_z, w->m, w->d_mcls, w->d_mcell, w->d_csite, w->d_ccls,
                                    w->d_ccell});
    p->with_grid([&](auto grid) {
        pc_walk_kernel<<<walk_grid, KMCF_BLOCK, 0, st>>>(grid, p->d_cell_start, w->m.d_pos, w->m.d_sum + kmcf_member_tiles(N),
                                                        w->d_csite, w->d_ccls, w->d_ccell, w->m.d_site, w->d_mcls, w->d_mcell,
                                                        w->m.d_x, w->m.d_y, w->m.d_z, a.d_x, a.d_y, a.d_z, a.n_classes, a.n_bins,
                                                        a.n_cells, a.r_max * a.r_max, a.r_count * a.r_count,
                                                        (double)a.n_bins / a.r_max, edges, passes, lds, w->d_hist, a.d_site_count,
                                                        w->d_max);
    });
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// the copies, the call's one synchronisation, and what the host adds
int pc_finish(kmcf_pairwise *p, const pc_call &a, const pc_edges &edges)
{
    kmcf_comm *c = p->comm;
    kmcf_pc_ws *w = p->pc_ws;
    hipStream_t st = c->stream;
    int *h = c->h_pinned;
    const int nb = kmcf_member_tiles(p->N);
    const size_t hist_words = ((size_t)a.n_cells + 1) * (size_t)(a.n_classes * (a.n_classes + 1) / 2) * (size_t)a.n_bins;
    const size_t member_words = ((size_t)a.n_cells + 1) * (size_t)a.n_classes;
    KMCF_HIP(hipMemcpyAsync(a.h_hist, w->d_hist, hist_words * sizeof(u64), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(a.h_members, w->d_members, member_words * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h, w->d_max, sizeof(u64), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h + 2, w->m.d_sum + nb, sizeof(int), hipMemcpyDeviceToHost, st));           // centres
    KMCF_HIP(hipMemcpyAsync(h + 3, w->m.d_sum + 2 * nb + 1, sizeof(int), hipMemcpyDeviceToHost, st));   // members
    KMCF_HIP(hipEventRecord(c->ev_call1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    if (a.h_edge2)
        for (int k = 0; k <= a.n_bins; ++k) a.h_edge2[k] = edges.e2[k];
    if (a.stats) {
        kmcf_pair_stats_t *s = a.stats;
        u64 total = 0;
        for (size_t k = 0; k < hist_words; ++k) total += a.h_hist[k];
        const u64 pack = ((u64)(unsigned)h[1] << 32) | (unsigned)h[0];
        s->n_pairs_total = total;
        s->n_members = h[3];
        s->n_probes = h[2] - h[3];
        s->max_count = pack ? (int)(pack >> 32) : 0;
        s->max_count_site = pack ? (int)(0xffffffffu - (unsigned)(pack & 0xffffffffull)) : -1;
        KMCF_HIP(hipEventElapsedTime(&s->ms, c->ev_t0, c->ev_call1));
    }
    return KMCF_OK;
}

// the table of the contract: multiply, then divide, each rounded to double (the library is built without contraction)
void pc_table(double r_max, int n_bins, pc_edges *t)
{
    for (int k = 0; k <= n_bins; ++k) {
        const double e = r_max * (double)k / (double)n_bins;
        t->e2[k] = e * e;
    }
    t->e2[n_bins] = r_max * r_max;
}

// the body of both calls; element == nullptr: the classes as given
int pc_run(const char *what, kmcf_pairwise *p, const pc_call &a, const int *d_site_class, const int *d_site_element,
           const int *d_site_charge, int probe_all, int *d_class_out)
{
    KMCF_TRY(pc_check_common(what, p, a.d_x, a.d_y, a.d_z, a.n_classes, a.r_max, a.n_bins, a.r_count, a.d_site_cell, a.n_cells,
                             a.h_hist, a.h_members));
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    const size_t hist_words = ((size_t)a.n_cells + 1) * (size_t)(a.n_classes * (a.n_classes + 1) / 2) * (size_t)a.n_bins;
    KMCF_TRY(pc_workspace(p, hist_words, ((size_t)a.n_cells + 1) * (size_t)a.n_classes));
    pc_edges edges;
    pc_table(a.r_max, a.n_bins, &edges);
    KMCF_HIP(hipEventRecord(c->ev_t0, c->stream));
    if (d_site_element) {
        int *cls = d_class_out ? d_class_out : p->pc_ws->d_class;
        pc_class_kernel<<<(p->N + KMCF_BLOCK - 1) / KMCF_BLOCK, KMCF_BLOCK, 0, c->stream>>>(p->N, d_site_element, d_site_charge,
                                                                                        probe_all, cls);
        d_site_class = cls;
    }
    KMCF_TRY(pc_enqueue(p, a, d_site_class, edges));
    return pc_finish(p, a, edges);
}

}  // namespace

extern "C" int kmcf_pair_correlation(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                     const int *d_site_class, int n_classes, double r_max, int n_bins, double r_count,
                                     const int *d_site_cell, int n_cells, unsigned long long *h_hist, int *h_members,
                                     double *h_edge2, int *d_site_count, kmcf_pair_stats_t *stats)
{
    const char *what = "kmcf_pair_correlation";
    KMCF_CHECK(d_site_class, KMCF_ERR_ARG, "%s: d_site_class is NULL", what);
    const pc_call a{d_x, d_y, d_z, n_classes, r_max, n_bins, r_count, d_site_cell, n_cells, h_hist, h_members, h_edge2, d_site_count,
                    stats};
    return pc_run(what, p, a, d_site_class, nullptr, nullptr, 0, nullptr);
}

extern "C" int kmcf_defect_correlation(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                       const int *d_site_element, const int *d_site_charge, int probe_all, double r_max,
                                       int n_bins, double r_count, const int *d_site_cell, int n_cells,
                                       unsigned long long *h_hist, int *h_members, double *h_edge2, int *d_site_count,
                                       int *d_site_class, kmcf_pair_stats_t *stats)
{
    const char *what = "kmcf_defect_correlation";
    KMCF_CHECK(d_site_element, KMCF_ERR_ARG, "%s: d_site_element is NULL", what);
    KMCF_CHECK(d_site_charge, KMCF_ERR_ARG, "%s: d_site_charge is NULL", what);
    const pc_call a{d_x, d_y, d_z, 3, r_max, n_bins, r_count, d_site_cell, n_cells, h_hist, h_members, h_edge2, d_site_count, stats};
    return pc_run(what, p, a, nullptr, d_site_element, d_site_charge, probe_all, d_site_class);
}
