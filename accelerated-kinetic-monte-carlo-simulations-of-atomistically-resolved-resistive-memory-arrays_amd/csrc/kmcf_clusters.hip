// Conductive cluster analysis: connected components of the high-G site graph (kmcf_conductive_clusters).
//
// The reference has no counterpart.  The rule for which pairs conduct is its own: the high_G branch of populate_T_dist
// (src/current_solver_gpu.cu:1227-1241) -- both sites metal, or both uncharged vacancies -- which is also class 1 /
// class 2 of the K rule (kmcf_kstate.hip).  Definitions (members, conductive edges, labels, touch bits, extents):
// include/kmcfield.h and DESIGN.md, "Conductive clusters".
//
// Algorithm: union-find with atomic hooking and path compression (ECL-CC / Afforest style), NOT label propagation: the
// electrode lines are clusters of 1e5-1e6 sites with diameters of hundreds of hops.  Launches, all on the compute stream:
//   1-3  classify the sites, compact the member list (the tile compaction of kmcf_block.hpp)
//   4    hook: LPR lanes per member row; every same-class neighbour is united with the row's site      [walks rows]
//   5    flatten: label[i] = root of i (the smallest id of its component), -1 for non-members
//   6    sizes, extents, the metal clusters' contact bits: summed per block in an LDS hash table, then atomics
//   7    touch bits of the vacancy clusters from the metal clusters next to them (either direction)     [walks rows]
//   8-10 compact the roots into the table (ascending root = scan order) and count the summaries
// Two launches walk neighbour rows whatever the input: stats->passes = 2.
// kmcf_clusters_enqueue is the pass without the read-back: kmcf_conductive_clusters calls it with the summaries, the
// filament gap analysis (kmcf_gap.hip) without launches 8-10, and reads class, label and touch where they lie.
//
// Hooking always puts the LARGER root under the SMALLER: parent[v] <= v at all times, every value ever stored in
// parent[v] is a site of v's component, every walk strictly decreases, and the final root is the minimum id.
//
// Memory model inside the hook kernel: other CUs and other XCDs rewrite parent[] while a wave reads it.  Every update is
// a device-scope atomicCAS / atomicMin; every read of the find loop is a relaxed agent-scope atomic load (served by L2,
// never by a CU's L1 and never kept in a register).  A value that is stale all the same is, by the invariant, an older
// ancestor: a longer walk, never a wrong union.  A failed CAS continues from the value the CAS itself returned.  The
// flatten pass and everything behind it are later launches and read plainly.
//
// NO THREAD WAITS FOR ANOTHER THREAD.  Every loop here advances by its own CAS result (the larger of the two roots
// strictly decreases per retry) or along a strictly decreasing walk: the design is lock-free.  There are no spin-waits,
// no flags and no grid-wide barriers, so there is nothing that could wait forever and nothing to bound.
//
// Determinism: sizes are integer atomic adds, touch bits atomic ORs, extents atomic min / max on a monotone 64-bit key
// of the double; labels are the component's minimum id.  Every output is independent of the execution order.
#include "kmcf_internal.hpp"

static_assert(sizeof(kmcf_cluster_t) == 32, "kmcf_cluster_t is 32 bytes");

struct kmcf_cluster_ws {
    int cap_N = 0;                       // sites the per-site arrays hold
    unsigned char *d_cls = nullptr;      // 0 no member, 1 metal, 2 conductive vacancy
    int *d_parent = nullptr, *d_members = nullptr, *d_label = nullptr, *d_size = nullptr, *d_touch = nullptr;
    unsigned long long *d_xmin = nullptr, *d_xmax = nullptr;
    int *d_msum = nullptr, *d_rsum = nullptr;   // scan scratch of the member and of the root compaction (tiles + 1)
    int *d_stats = nullptr;              // CL_STAT_* words
    kmcf_cluster_t *d_table = nullptr;
    size_t cap_table = 0;
};

void kmcf_cluster_ws_free(kmcf_comm *c)
{
    if (!c || !c->cl_ws) return;
    kmcf_cluster_ws *w = c->cl_ws;
    kmcf_dev_free_all({w->d_cls, w->d_parent, w->d_members, w->d_label, w->d_size, w->d_touch, w->d_xmin, w->d_xmax, w->d_msum,
                       w->d_rsum, w->d_stats, w->d_table});
    delete w;
    c->cl_ws = nullptr;
}

namespace {

constexpr int EL_VACANCY = 2;                          // src/utils.h:37-44
constexpr int CL_NONE = 0, CL_METAL = KMCF_CLUSTER_METAL, CL_VACANCY = KMCF_CLUSTER_VACANCY;
constexpr int CL_PASSES = 2;                           // launches that walk neighbour rows: cl_hook_kernel, cl_touch_kernel
enum { CL_STAT_METAL, CL_STAT_VACANCY, CL_STAT_BRIDGING, CL_STAT_LARGEST_VAC, CL_STAT_LARGEST_BRIDGING, CL_STAT_MEMBERS,
       CL_STAT_CLUSTERS, CL_STAT_WORDS = 8 };

__device__ __forceinline__ int cl_class_of(int el, int q, const int *__restrict__ metals, int num_metals)
{
    for (int m = 0; m < num_metals; ++m)
        if (el == metals[m]) return CL_METAL;
    return (el == EL_VACANCY && q == 0) ? CL_VACANCY : CL_NONE;
}

// 1: classes, parent[i] = i, member counts per tile; block 0 also clears the summary words
__global__ __launch_bounds__(KMCF_BLOCK) void cl_classify_kernel(int N, const int *__restrict__ element,
                                                                 const int *__restrict__ charge, const int *__restrict__ metals,
                                                                 int num_metals, unsigned char *__restrict__ cls,
                                                                 int *__restrict__ parent, int *__restrict__ msum,
                                                                 int *__restrict__ stats)
{
    __shared__ int lds[4];
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(N, f, [&](int i) {
        const int cl = cl_class_of(element[i], charge[i], metals, num_metals);
        cls[i] = (unsigned char)cl;
        parent[i] = i;
        return cl != CL_NONE;
    });
    const int total = kmcf_tile_count(f, lds);
    if (threadIdx.x == 0) msum[blockIdx.x] = total;
    if (blockIdx.x == 0 && threadIdx.x < CL_STAT_WORDS) stats[threadIdx.x] = 0;
}

// 3: member list, ascending site id
__global__ __launch_bounds__(KMCF_BLOCK) void cl_member_scatter_kernel(int N, const unsigned char *__restrict__ cls,
                                                                       const int *__restrict__ msum, int *__restrict__ members)
{
    __shared__ int lds[4];
    const int t0 = kmcf_tile_item0();
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(N, f, [&](int i) { return cls[i] != CL_NONE; });
    int pos = kmcf_tile_pos(f, msum[blockIdx.x], lds);
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k)
        if (f[k]) members[pos++] = t0 + k;
}

__device__ __forceinline__ int cl_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Root of v as far as this thread can see, halving the path on the way.  parent[] only ever decreases (atomicMin here,
// the CAS of cl_unite), so the walk strictly decreases and ends at a site that was a root when it was read.
__device__ __forceinline__ int cl_find(int *parent, int v)
{
    int p = cl_load(parent + v);
    while (p != v) {
        const int gp = cl_load(parent + p);
        if (gp != p) atomicMin(parent + v, gp);
        v = p;
        p = gp;
    }
    return v;
}

// Joins the components of u and v: the larger root goes under the smaller.  A CAS that fails has found `hi` hooked by
// another thread meanwhile; the walk goes on from the value the CAS returned (< hi), so max(ru, rv) strictly decreases.
// `lo` may have stopped being a root: hooking under a non-root keeps parent[hi] < hi inside the component.
// Returns an ancestor of both (the next find of either may start there).
__device__ __forceinline__ int cl_unite(int *parent, int u, int v)
{
    int ru = cl_find(parent, u), rv = cl_find(parent, v);
    while (ru != rv) {
        const int hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;
        ru = cl_find(parent, old);
        rv = lo;
    }
    return ru;
}

// 4: hook.  LPR lanes share one member's row.  An entry outside [0, N) is padding and is never used as an index.
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void cl_hook_kernel(int N, int nn, const int *__restrict__ neigh,
                                                             const unsigned char *__restrict__ cls,
                                                             const int *__restrict__ members, const int *__restrict__ n_members,
                                                             int *parent)
{
    const int M = *n_members;
    const int lane = threadIdx.x % LPR;
    const int groups = gridDim.x * (KMCF_BLOCK / LPR);
    for (int m = blockIdx.x * (KMCF_BLOCK / LPR) + threadIdx.x / LPR; m < M; m += groups) {
        const int i = members[m];
        const int ci = cls[i];
        const int *row = neigh + (size_t)i * nn;
        int a = i;                                       // an ancestor of i: this lane's finds of i start there
        for (int s = lane; s < nn; s += LPR) {
            const int j = row[s];
            if ((unsigned)j >= (unsigned)N || j == i) continue;
            if (cls[j] == ci) a = cl_unite(parent, a, j);
        }
    }
}

__device__ __forceinline__ unsigned long long cl_key(double x)
{
    // monotone in x (negative values included): min / max of the keys are the keys of min / max
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double cl_unkey(unsigned long long k)
{
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

// 5: labels (a later launch than the hooks: plain reads), and the empty summaries of the roots
__global__ __launch_bounds__(KMCF_BLOCK) void cl_flatten_kernel(int N, const unsigned char *__restrict__ cls,
                                                                const int *__restrict__ parent, int *__restrict__ label,
                                                                int *__restrict__ size, int *__restrict__ touch,
                                                                unsigned long long *__restrict__ xmin,
                                                                unsigned long long *__restrict__ xmax)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i >= N) return;
    if (cls[i] == CL_NONE) { label[i] = -1; return; }
    int v = i, p = parent[v];
    while (p != v) { v = p; p = parent[v]; }
    label[i] = v;
    if (v == i) { size[i] = 0; touch[i] = 0; xmin[i] = ~0ull; xmax[i] = 0ull; }
}

// 6: sizes, extents, contact bits of the metal clusters.  An electrode line is ONE label for 1e5-1e6 members: every
// block first sums what it meets in a small hash table in LDS (integer adds, min, max, OR: any order gives the same
// bits) and issues one set of global atomics per label it holds; a label that finds its two probed slots taken by
// others goes to memory directly.
constexpr int CL_HASH = 1024;
__device__ __forceinline__ void cl_summary_atomics(int r, int cnt, int bits, unsigned long long kmin, unsigned long long kmax,
                                                   int *size, int *touch, unsigned long long *xmin, unsigned long long *xmax)
{
    atomicAdd(size + r, cnt);
    atomicMin(xmin + r, kmin);
    atomicMax(xmax + r, kmax);
    if (bits) atomicOr(touch + r, bits);
}

__global__ __launch_bounds__(KMCF_BLOCK) void cl_reduce_kernel(int N, int N_left, int N_right,
                                                               const unsigned char *__restrict__ cls,
                                                               const int *__restrict__ members, const int *__restrict__ n_members,
                                                               const int *__restrict__ label, const double *__restrict__ x,
                                                               int *size, int *touch, unsigned long long *xmin,
                                                               unsigned long long *xmax)
{
    __shared__ int h_key[CL_HASH], h_cnt[CL_HASH], h_bits[CL_HASH];
    __shared__ unsigned long long h_min[CL_HASH], h_max[CL_HASH];
    for (int s = threadIdx.x; s < CL_HASH; s += KMCF_BLOCK) {
        h_key[s] = -1; h_cnt[s] = 0; h_bits[s] = 0; h_min[s] = ~0ull; h_max[s] = 0ull;
    }
    __syncthreads();
    const int M = *n_members;
    for (int m = blockIdx.x * KMCF_BLOCK + threadIdx.x; m < M; m += gridDim.x * KMCF_BLOCK) {
        const int i = members[m];
        const int r = label[i];
        const unsigned long long key = cl_key(x[i]);
        const int bits = cls[i] == CL_METAL ? ((i < N_left ? 1 : 0) | (i >= N - N_right ? 2 : 0)) : 0;
        int slot = (int)(((unsigned)r * 2654435761u) >> 22);            // 10 bits
        bool done = false;
        for (int probe = 0; probe < 2 && !done; ++probe, slot = (slot + 1) & (CL_HASH - 1)) {
            const int old = atomicCAS(&h_key[slot], -1, r);
            if (old == -1 || old == r) {
                atomicAdd(&h_cnt[slot], 1);
                atomicMin(&h_min[slot], key);
                atomicMax(&h_max[slot], key);
                if (bits) atomicOr(&h_bits[slot], bits);
                done = true;
            }
        }
        if (!done) cl_summary_atomics(r, 1, bits, key, key, size, touch, xmin, xmax);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < CL_HASH; s += KMCF_BLOCK)
        if (h_key[s] >= 0) cl_summary_atomics(h_key[s], h_cnt[s], h_bits[s], h_min[s], h_max[s], size, touch, xmin, xmax);
}

// 7: a vacancy cluster takes the contact bits of every metal cluster one of its sites shares a list entry with: read
// from the vacancy's own row, pushed from the metal's row (an entry listed in one row only counts).  The metal
// clusters' bits are complete (earlier launch) and are not written here.
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void cl_touch_kernel(int N, int nn, const int *__restrict__ neigh,
                                                              const unsigned char *__restrict__ cls,
                                                              const int *__restrict__ members, const int *__restrict__ n_members,
                                                              const int *__restrict__ label, int *touch)
{
    const int M = *n_members;
    const int lane = threadIdx.x % LPR;
    const int groups = gridDim.x * (KMCF_BLOCK / LPR);
    const int rows = (M + KMCF_BLOCK / LPR - 1) / (KMCF_BLOCK / LPR) * (KMCF_BLOCK / LPR);   // whole groups shuffle together
    for (int m = blockIdx.x * (KMCF_BLOCK / LPR) + threadIdx.x / LPR; m < rows; m += groups) {
        const bool valid = m < M;
        const int i = valid ? members[m] : 0;
        const int ci = valid ? cls[i] : CL_NONE;
        const int own = ci == CL_METAL ? touch[label[i]] : 0;
        int bits = 0;
        if (ci == CL_VACANCY || own) {
            const int *row = neigh + (size_t)i * nn;
            for (int s = lane; s < nn; s += LPR) {
                const int j = row[s];
                if ((unsigned)j >= (unsigned)N) continue;
                const int cj = cls[j];
                if (ci == CL_VACANCY && cj == CL_METAL) bits |= touch[label[j]];
                if (ci == CL_METAL && cj == CL_VACANCY) {
                    int *t = touch + label[j];
                    // bits are only ever added: a value read early lacks some at worst, and then the OR is issued
                    if ((__hip_atomic_load(t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & own) != own) atomicOr(t, own);
                }
            }
        }
#pragma unroll
        for (int off = LPR / 2; off >= 1; off >>= 1) bits |= __shfl_xor(bits, off, 64);
        if (ci == CL_VACANCY && lane == 0 && bits) atomicOr(touch + label[i], bits);
    }
}

// 8: roots per tile and the summaries (integer adds and maxima: order-independent)
__global__ __launch_bounds__(KMCF_BLOCK) void cl_root_count_kernel(int N, const unsigned char *__restrict__ cls,
                                                                   const int *__restrict__ label, const int *__restrict__ size,
                                                                   const int *__restrict__ touch, int *__restrict__ rsum,
                                                                   int *stats)
{
    __shared__ int lds[4];
    int f[KMCF_SCAN_ITEMS], v[5] = {0, 0, 0, 0, 0};
    kmcf_tile_flags(N, f, [&](int i) {
        if (label[i] != i) return false;
        if (cls[i] == CL_METAL) {
            ++v[CL_STAT_METAL];
        } else {
            const int sz = size[i];
            ++v[CL_STAT_VACANCY];
            v[CL_STAT_LARGEST_VAC] = max(v[CL_STAT_LARGEST_VAC], sz);
            if (touch[i] == 3) {
                ++v[CL_STAT_BRIDGING];
                v[CL_STAT_LARGEST_BRIDGING] = max(v[CL_STAT_LARGEST_BRIDGING], sz);
            }
        }
        return true;
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int q = 0; q < 3; ++q) v[q] += __shfl_xor(v[q], off, 64);
#pragma unroll
        for (int q = 3; q < 5; ++q) v[q] = max(v[q], __shfl_xor(v[q], off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        for (int q = 0; q < 3; ++q)
            if (v[q]) atomicAdd(stats + q, v[q]);
        for (int q = 3; q < 5; ++q)
            if (v[q]) atomicMax(stats + q, v[q]);
    }
    const int total = kmcf_tile_count(f, lds);
    if (threadIdx.x == 0) rsum[blockIdx.x] = total;
}

// 10: the table, ascending root; entries from `cap` on are dropped.  Block 0 completes the summary words.
__global__ __launch_bounds__(KMCF_BLOCK) void cl_root_scatter_kernel(int N, int nb, const unsigned char *__restrict__ cls,
                                                                     const int *__restrict__ label, const int *__restrict__ size,
                                                                     const int *__restrict__ touch,
                                                                     const unsigned long long *__restrict__ xmin,
                                                                     const unsigned long long *__restrict__ xmax,
                                                                     const int *__restrict__ rsum, const int *__restrict__ n_members,
                                                                     kmcf_cluster_t *__restrict__ table, int cap, int *stats)
{
    __shared__ int lds[4];
    const int t0 = kmcf_tile_item0();
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(N, f, [&](int i) { return label[i] == i; });
    int pos = kmcf_tile_pos(f, rsum[blockIdx.x], lds);
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k) {
        if (!f[k]) continue;
        const int i = t0 + k;
        if (pos < cap) {
            kmcf_cluster_t e;
            e.root = i; e.kind = cls[i]; e.size = size[i]; e.touch = touch[i];
            e.x_min = cl_unkey(xmin[i]); e.x_max = cl_unkey(xmax[i]);
            table[pos] = e;
        }
        ++pos;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        stats[CL_STAT_MEMBERS] = *n_members;
        stats[CL_STAT_CLUSTERS] = rsum[nb];
    }
}

// workspace on the communicator, grown on demand and freed by kmcf_comm_destroy; it holds nothing a later call reads
int cl_workspace(kmcf_comm *c, int N, int table_entries)
{
    if (c->cl_ws && c->cl_ws->cap_N < N) kmcf_cluster_ws_free(c);
    if (!c->cl_ws) {
        kmcf_cluster_ws *w = c->cl_ws = new kmcf_cluster_ws();
        const size_t n = (size_t)N, nb = (n + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE + 1;
        KMCF_TRY(kmcf_dev_alloc(&w->d_cls, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_parent, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_members, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_label, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_size, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_touch, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_xmin, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_xmax, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_msum, nb, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_rsum, nb, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_stats, (size_t)CL_STAT_WORDS, false));
        w->cap_N = N;
    }
    kmcf_cluster_ws *w = c->cl_ws;
    if (w->cap_table < (size_t)table_entries) KMCF_TRY(kmcf_dev_grow(&w->d_table, &w->cap_table, (size_t)table_entries, 0));
    return KMCF_OK;
}

}  // namespace

int kmcf_clusters_enqueue(kmcf_comm *c, int N, int nn, const int *d_neigh_idx, const int *d_site_element,
                          const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x, int N_left_tot,
                          int N_right_tot, int *d_site_label, bool summaries, int table_cap, kmcf_cluster_dev *out)
{
    const int cap = table_cap;
    KMCF_TRY(cl_workspace(c, N, cap));
    kmcf_cluster_ws *w = c->cl_ws;
    hipStream_t st = c->stream;
    int *label = d_site_label ? d_site_label : w->d_label;
    const int nb = (N + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE;     // tiles of the scans
    const int *n_members = w->d_msum + nb;
    const bool wide = nn > 8;                                     // 16 lanes per row, 4 for short rows
    const int per_block = KMCF_BLOCK / (wide ? 16 : 4);
    int64_t row_grid = ((int64_t)N + per_block - 1) / per_block;  // an upper bound: the kernels stride over the members
    if (row_grid > 16384) row_grid = 16384;
    int64_t red_grid = ((int64_t)N + KMCF_BLOCK - 1) / KMCF_BLOCK;
    const int site_grid = (int)red_grid;
    if (red_grid > 512) red_grid = 512;                           // two blocks per CU: few sets of atomics per hot label

    cl_classify_kernel<<<nb, KMCF_BLOCK, 0, st>>>(N, d_site_element, d_site_charge, d_metals, num_metals, w->d_cls, w->d_parent,
                                                 w->d_msum, w->d_stats);
    kmcf_scan_counts_kernel<int><<<1, KMCF_BLOCK, 0, st>>>(nb, w->d_msum, w->d_msum, 0);
    cl_member_scatter_kernel<<<nb, KMCF_BLOCK, 0, st>>>(N, w->d_cls, w->d_msum, w->d_members);
    if (wide)
        cl_hook_kernel<16><<<(int)row_grid, KMCF_BLOCK, 0, st>>>(N, nn, d_neigh_idx, w->d_cls, w->d_members, n_members, w->d_parent);
    else
        cl_hook_kernel<4><<<(int)row_grid, KMCF_BLOCK, 0, st>>>(N, nn, d_neigh_idx, w->d_cls, w->d_members, n_members, w->d_parent);
    cl_flatten_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, w->d_cls, w->d_parent, label, w->d_size, w->d_touch, w->d_xmin, w->d_xmax);
    cl_reduce_kernel<<<(int)red_grid, KMCF_BLOCK, 0, st>>>(N, N_left_tot, N_right_tot, w->d_cls, w->d_members, n_members, label, d_x,
                                                          w->d_size, w->d_touch, w->d_xmin, w->d_xmax);
    if (wide)
        cl_touch_kernel<16><<<(int)row_grid, KMCF_BLOCK, 0, st>>>(N, nn, d_neigh_idx, w->d_cls, w->d_members, n_members, label, w->d_touch);
    else
        cl_touch_kernel<4><<<(int)row_grid, KMCF_BLOCK, 0, st>>>(N, nn, d_neigh_idx, w->d_cls, w->d_members, n_members, label, w->d_touch);
    if (summaries) {
        cl_root_count_kernel<<<nb, KMCF_BLOCK, 0, st>>>(N, w->d_cls, label, w->d_size, w->d_touch, w->d_rsum, w->d_stats);
        kmcf_scan_counts_kernel<int><<<1, KMCF_BLOCK, 0, st>>>(nb, w->d_rsum, w->d_rsum, 0);
        cl_root_scatter_kernel<<<nb, KMCF_BLOCK, 0, st>>>(N, nb, w->d_cls, label, w->d_size, w->d_touch, w->d_xmin, w->d_xmax, w->d_rsum,
                                                         n_members, w->d_table, cap, w->d_stats);
    }
    KMCF_HIP(hipGetLastError());
    if (out) { out->cls = w->d_cls; out->label = label; out->touch = w->d_touch; }
    return KMCF_OK;
}

extern "C" int kmcf_conductive_clusters(kmcf_comm *c, int N, int nn, const int *d_neigh_idx, const int *d_site_element,
                                        const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                                        int N_left_tot, int N_right_tot, int *d_site_label, kmcf_cluster_t *h_clusters,
                                        int max_clusters, kmcf_cluster_stats_t *stats)
{
    const char *what = "kmcf_conductive_clusters";
    KMCF_CHECK(c, KMCF_ERR_ARG, "%s: c is NULL", what);
    KMCF_CHECK(d_neigh_idx, KMCF_ERR_ARG, "%s: d_neigh_idx is NULL", what);
    KMCF_CHECK(d_site_element, KMCF_ERR_ARG, "%s: d_site_element is NULL", what);
    KMCF_CHECK(d_site_charge, KMCF_ERR_ARG, "%s: d_site_charge is NULL", what);
    KMCF_CHECK(d_x, KMCF_ERR_ARG, "%s: d_x is NULL", what);
    KMCF_CHECK(N > 0, KMCF_ERR_ARG, "%s: N = %d is not > 0", what, N);
    KMCF_CHECK(nn > 0, KMCF_ERR_ARG, "%s: nn = %d is not > 0", what, nn);
    KMCF_CHECK(num_metals >= 0, KMCF_ERR_ARG, "%s: num_metals = %d is negative", what, num_metals);
    KMCF_CHECK(num_metals == 0 || d_metals, KMCF_ERR_ARG, "%s: d_metals is NULL with num_metals = %d", what, num_metals);
    KMCF_CHECK(N_left_tot >= 0, KMCF_ERR_ARG, "%s: N_left_tot = %d is negative", what, N_left_tot);
    KMCF_CHECK(N_right_tot >= 0, KMCF_ERR_ARG, "%s: N_right_tot = %d is negative", what, N_right_tot);
    KMCF_CHECK((int64_t)N_left_tot + N_right_tot <= N, KMCF_ERR_ARG, "%s: N_left_tot + N_right_tot = %lld exceeds N = %d", what,
               (long long)N_left_tot + N_right_tot, N);
    KMCF_CHECK(max_clusters >= 0, KMCF_ERR_ARG, "%s: max_clusters = %d is negative", what, max_clusters);
    KMCF_CHECK(!h_clusters || max_clusters > 0, KMCF_ERR_ARG, "%s: h_clusters is set with max_clusters = 0", what);
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "%s: host-only communicator", what);
    KMCF_TRY(kmcf_enter(c));
    const int cap = h_clusters ? (max_clusters < N ? max_clusters : N) : 0;
    hipStream_t st = c->stream;
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    KMCF_TRY(kmcf_clusters_enqueue(c, N, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals, d_x, N_left_tot,
                                   N_right_tot, d_site_label, true, cap, nullptr));
    kmcf_cluster_ws *w = c->cl_ws;
    int *h = c->h_pinned;
    KMCF_HIP(hipMemcpyAsync(h, w->d_stats, CL_STAT_WORDS * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    const int n_clusters = h[CL_STAT_CLUSTERS];
    float ms = 0.f, ms_table = 0.f;
    if (h_clusters && n_clusters > 0) {                           // (the count had to reach the host first)
        KMCF_HIP(hipEventRecord(c->ev_call0, st));
        KMCF_HIP(hipMemcpyAsync(h_clusters, w->d_table, (size_t)(n_clusters < cap ? n_clusters : cap) * sizeof(kmcf_cluster_t),
                                hipMemcpyDeviceToHost, st));
        KMCF_HIP(hipEventRecord(c->ev_call1, st));
        KMCF_HIP(hipStreamSynchronize(st));
        KMCF_HIP(hipEventElapsedTime(&ms_table, c->ev_call0, c->ev_call1));
    }
    KMCF_HIP(hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    if (stats) {
        stats->members = h[CL_STAT_MEMBERS];
        stats->n_clusters = n_clusters;
        stats->n_metal_clusters = h[CL_STAT_METAL];
        stats->n_vacancy_clusters = h[CL_STAT_VACANCY];
        stats->n_bridging = h[CL_STAT_BRIDGING];
        stats->largest_vacancy = h[CL_STAT_LARGEST_VAC];
        stats->largest_bridging = h[CL_STAT_LARGEST_BRIDGING];
        stats->passes = CL_PASSES;
        stats->ms = ms + ms_table;
    }
    return KMCF_OK;
}
