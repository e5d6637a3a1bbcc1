// Tunnelling-chain analysis: per gap cell the bottleneck-optimal chain of hops from the left side to the right side
// through floating bodies (kmcf_site_set_chain), and the same with sides and bodies derived from the device state
// (kmcf_filament_chain).
//
// The reference has no counterpart.  Definitions (terminals, stones, homes, links, keys, chain): include/kmcfield.h and
// DESIGN.md 3.12.  A VERTEX is named by one of its sites: a stone by its home, L_c / R_c by their smallest site id; the
// per-vertex arrays below are indexed by that site.
//
// Launches, all on the compute stream (kmcf_filament_chain: behind the cluster pass and one kernel for sides and nodes):
//   1    clear: per-cell words, homes, per-vertex words
//   2    counts of the sides per gap cell, smallest L / R site per cell, home per node        [integer atomicAdd / atomicMin]
//   3    vertex and vertex cell per site; stones and stone sites per cell; members = sites of the vertices of cells with
//        both terminals and no site on both sides (NONE and BRIDGED cells drop out)
//   4-6  compact the members per INDEX cell with coordinates, vertex cell, vertex and component: the shared compaction of
//        kmcf_cellmembers.hpp (ch_rule, ch_emit)
//   round r = 1, 2, ... (Boruvka):
//     a  search: 16 lanes per member walk the runs of the 27 surrounding index cells over the candidates of the same vertex
//        cell and another component; the group's minimum (d2, smallest partner) is stored per member and lowers the
//        component's best d2 (64-bit integer atomicMin on the bits: non-negative doubles order as integers)
//     b  among the members that attain their component's d2, the smallest packed (min << 32 | max) wins (atomicMin)
//     c  hook: every component root with a link appends it to the edge list and points at the other component's root; of
//        a mutual choice (the only cycles: keys are unique) the smaller root stays and appends, the larger only hooks
//     d  jump: every vertex follows the hooks to its new root; the per-component words are reset
//     e  cells whose L and R are still in different components are counted into the round's flag word
//     the host reads the flag words (one synchronisation) and stops when the round chose no link or no such cell is left:
//     Boruvka's edges are edges of the minimum spanning forest, so the forest path between L and R is then final.
//     f  before round 2: the members that found a partner in round 1 (the SURFACE members) are compacted over the member
//        list (4-6 again); the others -- electrode and filament bulk -- have no site of another vertex within r_max and
//        never gain one, as components only merge.  Before round 3 on: the components of the list are refreshed.
//   the records and hop lists are put together on the host from the edge list (at most vertices - 1 edges).
//
// Round 1 also takes, per L member, the smallest d2 to an R member of its cell (direct2).  Pruning (as in kmcf_gap.hip: a
// run of index cells is skipped only if its face-distance bound is GREATER than every threshold that still matters):
// round 1 -- r_max^2, what the member itself has found (anything more would hide a member's partner and with it the
// surface mark), and for L members the cell's direct2 so far; later rounds -- r_max^2, the component's best so far
// (whatever value is read is >= the final one) and what the member has found.  Members that attain the final minimum hold
// their exact (d2, smallest partner); the others never enter b.
//
// Periodic index (kmcf_site_set_chain_pbc / kmcf_filament_chain_pbc on an index of kmcf_compute_cutoff_list_pbc with pbc = 1):
// step a is ch_search_kernel on the periodic geometry (kmcf_cell_grid_pbc; the walk and the distance are those of
// kmcf_cellwalk.hpp) -- the minimum image in y and z, the wrapped cells each once, the bound in y taken to the face through
// which the neighbour cell is adjacent ("Periodic search"); a candidate is met once and has one distance,
// however many of its images lie within r_max; z is not pruned.  Every other launch is shared: the cell id and the order
// inside a cell are those of the open index (one index_cells for both, kmcf_pairwise.hip), which is all the compaction
// reads.  d2 is the same bits from both ends of a pair, so a mutual choice is seen as one by b and c.
//
// Determinism: every device result is an integer sum or minimum; the order of the edge list is not, and the host sorts it
// by key before use.  No thread waits for another; the search stops after CH_MAX_ROUNDS rounds (KMCF_ERR_STATE).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

#include "kmcf_cellwalk.hpp"

static_assert(sizeof(kmcf_chain_t) == 64, "kmcf_chain_t is 64 bytes");
static_assert(sizeof(kmcf_hop_t) == 16, "kmcf_hop_t is 16 bytes");

namespace {
typedef unsigned long long u64;
struct ch_edge {            // a chosen link: the pair (a < b), their vertices
    u64 d2;
    int a, b, va, vb;
};
static_assert(sizeof(ch_edge) == 24, "ch_edge is 24 bytes");
}  // namespace

struct kmcf_chain_ws {
    int N = 0;
    int *d_side = nullptr, *d_node = nullptr;    // kmcf_filament_chain without the caller's arrays
    int *d_home = nullptr;                       // per node: smallest stone site
    int *d_svert = nullptr, *d_svcell = nullptr; // per site: vertex (-1: no member) and vertex cell
    int *d_surf = nullptr;                       // per site: found a partner in round 1
    int *d_root = nullptr, *d_next = nullptr;    // per vertex: component root; the hook of this round
    u64 *d_cbest = nullptr, *d_cpair = nullptr;  // per component root: bits of the smallest d2, packed pair
    kmcf_members l;                              // the list (index-cell order) with coordinates; its length in d_sum[tiles]
    int *d_lvcell = nullptr, *d_lvert = nullptr, *d_lcomp = nullptr;   // ... vertex cell, vertex and component
    u64 *d_ld2 = nullptr;                        // per list member: bits of its smallest d2
    int *d_lj = nullptr;                         // ... and the partner (-1: none)
    ch_edge *d_edges = nullptr;                  // N
    int *d_flags = nullptr;                      // CH_F_*
    size_t cap_cells = 0;
    int *d_words = nullptr;                      // per gap cell: CH_W_*
    u64 *d_direct = nullptr;                     // per gap cell: bits of direct2
};

void kmcf_chain_ws_free(kmcf_pairwise *p)
{
    if (!p || !p->chain_ws) return;
    kmcf_chain_ws *w = p->chain_ws;
    kmcf_members_free(&w->l);
    kmcf_dev_free_all({w->d_side, w->d_node, w->d_home, w->d_svert, w->d_svcell, w->d_surf, w->d_root, w->d_next, w->d_cbest,
                       w->d_cpair, w->d_lvcell, w->d_lvert, w->d_lcomp, w->d_ld2, w->d_lj, w->d_edges, w->d_flags, w->d_words,
                       w->d_direct});
    delete w;
    p->chain_ws = nullptr;
}

namespace {

constexpr int CH_LPS = 16, CH_SPB = KMCF_BLOCK / CH_LPS;          // lanes per member, members per block
constexpr int CH_NO_SITE = 0x7fffffff;
constexpr int CH_MAX_ROUNDS = 40;
enum { CH_W_LEFT, CH_W_RIGHT, CH_W_BOTH, CH_W_STONES, CH_W_STONE_SITES, CH_W_LREP, CH_W_RREP, CH_W_WORDS = 8 };
enum { CH_F_EDGES, CH_F_ERROR, CH_F_SURFACE, CH_F_OPEN0, CH_F_WORDS = CH_F_OPEN0 + CH_MAX_ROUNDS };

// both terminals and no site on both sides: the cell's vertices enter the search
__device__ __forceinline__ bool ch_active(const int *__restrict__ words, int c)
{
    const int *q = words + (size_t)CH_W_WORDS * c;
    return q[CH_W_LEFT] > 0 && q[CH_W_RIGHT] > 0 && q[CH_W_BOTH] == 0;
}

// sides and nodes from the cluster pass: touch of the site's cluster; the label where that cluster floats
__global__ __launch_bounds__(KMCF_BLOCK) void ch_side_node_kernel(int N, const unsigned char *__restrict__ cls,
                                                                  const int *__restrict__ label, const int *__restrict__ touch,
                                                                  int *__restrict__ side, int *__restrict__ node)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int t = cls[i] ? (touch[label[i]] & 3) : 0;
    side[i] = t;
    node[i] = (cls[i] && t == 0) ? label[i] : -1;
}

// 1
__global__ __launch_bounds__(KMCF_BLOCK) void ch_clear_kernel(int N, size_t n_cells, int *__restrict__ home, int *__restrict__ root,
                                                              int *__restrict__ next, u64 *__restrict__ cbest,
                                                              u64 *__restrict__ cpair, int *__restrict__ words,
                                                              u64 *__restrict__ direct, int *__restrict__ flags)
{
    const size_t i = (size_t)blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i < (size_t)N) {
        home[i] = CH_NO_SITE;
        root[i] = next[i] = (int)i;
        cbest[i] = KMCF_D2_INF;
        cpair[i] = KMCF_NO_PAIR;
    }
    if (i < n_cells) {
        int *q = words + CH_W_WORDS * i;
#pragma unroll
        for (int k = 0; k < CH_W_WORDS; ++k) q[k] = 0;
        q[CH_W_LREP] = q[CH_W_RREP] = CH_NO_SITE;
        direct[i] = KMCF_D2_INF;
    }
    if (blockIdx.x == 0 && threadIdx.x < CH_F_WORDS) flags[threadIdx.x] = 0;
}

// 2: a wave adds once per gap cell it meets; the smallest L / R site of a wave's share is its first lane that holds one
__global__ __launch_bounds__(KMCF_BLOCK) void ch_count_kernel(int N, const int *__restrict__ side, const int *__restrict__ node,
                                                              const int *__restrict__ site_cell, int n_cells, int *words, int *home)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int s = i < N ? (side[i] & 3) : 0;
    const int c = i < N ? kmcf_site_cell(site_cell, n_cells, i) : -1;
    if (i < N && s == 0 && c >= 0) {
        const int n = node[i];
        if ((unsigned)n < (unsigned)N) atomicMin(home + n, i);
    }
    bool todo = s != 0 && c >= 0;
    for (u64 act = __ballot(todo); act; act = __ballot(todo)) {
        const int leader = __ffsll((long long)act) - 1;
        const int lc = __shfl(c, leader, 64);
        const bool mine = todo && c == lc;
        const u64 a1 = __ballot(mine && (s & 1)), a2 = __ballot(mine && (s & 2)), a3 = __ballot(mine && s == 3);
        const u64 l1 = __ballot(mine && s == 1), r1 = __ballot(mine && s == 2);
        if (lane == leader) {
            int *q = words + (size_t)CH_W_WORDS * lc;
            const int i0 = i - lane;
            if (a1) atomicAdd(q + CH_W_LEFT, __popcll(a1));
            if (a2) atomicAdd(q + CH_W_RIGHT, __popcll(a2));
            if (a3) atomicAdd(q + CH_W_BOTH, __popcll(a3));
            if (l1) atomicMin(q + CH_W_LREP, i0 + __ffsll((long long)l1) - 1);
            if (r1) atomicMin(q + CH_W_RREP, i0 + __ffsll((long long)r1) - 1);
        }
        if (mine) todo = false;
    }
}

// 3
__global__ __launch_bounds__(KMCF_BLOCK) void ch_vertex_kernel(int N, const int *__restrict__ side, const int *__restrict__ node,
                                                               const int *__restrict__ site_cell, int n_cells,
                                                               const int *__restrict__ home, int *words,
                                                               int *__restrict__ svert, int *__restrict__ svcell)
{
    const int i = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (i >= N) return;
    const int s = side[i] & 3;
    const int c = kmcf_site_cell(site_cell, n_cells, i);
    int vert = -1, vc = -1;
    if (c >= 0 && s == 0) {
        const int n = node[i];
        if ((unsigned)n < (unsigned)N) {
            vert = home[n];
            vc = kmcf_site_cell(site_cell, n_cells, vert);              // (the home is a stone site: it has a cell)
            int *q = words + (size_t)CH_W_WORDS * vc;
            atomicAdd(q + CH_W_STONE_SITES, 1);
            if (vert == i) atomicAdd(q + CH_W_STONES, 1);
        }
    } else if (c >= 0 && s != 3) {
        vc = c;
        vert = words[(size_t)CH_W_WORDS * c + (s == 1 ? CH_W_LREP : CH_W_RREP)];   // (final: written by an earlier launch)
    }
    // the counts of the sides are final; the stone counts this kernel adds are not read here
    const bool member = vert >= 0 && ch_active(words, vc);
    svert[i] = member ? vert : -1;
    svcell[i] = vc;
}

// 4-6, the list.  surf == nullptr: the members; else: the surface members.  With coordinates, vertex cell, vertex, component
struct ch_rule {
    const int *svert, *surf;
    __device__ __forceinline__ int operator()(int i) const { return svert[i] >= 0 && (!surf || surf[i]); }
};
struct ch_emit {
    const int *svert, *svcell, *root;
    const double *x, *y, *z;
    kmcf_members l;
    int *lvcell, *lvert, *lcomp;
    __device__ __forceinline__ void operator()(int, int q, int i, int) const
    {
        const int v = svert[i];
        kmcf_member_put(l, q, i, x, y, z);
        lvcell[q] = svcell[i];
        lvert[q] = v;
        lcomp[q] = root[v];
    }
};

// a: the search of one round over the list, on the open (GRID = kmcf_cell_grid) or the periodic index (kmcf_cell_grid_pbc).
// A group of CH_LPS lanes per member; the loop runs over whole blocks of groups, and both thresholds are uniform over a
// group, as the walk requires (kmcf_cellwalk.hpp), so its lanes reach the shuffles together.
// FIRST: round 1 -- components are vertices, the surface marks, direct2.
template <bool FIRST, class GRID>
__global__ __launch_bounds__(KMCF_BLOCK) void ch_search_kernel(GRID g, const int *__restrict__ cell_start,
                                                               const int *__restrict__ lpos, const int *__restrict__ n_list,
                                                               const int *__restrict__ lsite, const int *__restrict__ lvcell,
                                                               const int *__restrict__ lcomp, const double *__restrict__ lx,
                                                               const double *__restrict__ ly, const double *__restrict__ lz,
                                                               double rmax2, const int *__restrict__ words, u64 *cbest,
                                                               u64 *direct, u64 *__restrict__ ld2, int *__restrict__ lj,
                                                               int *__restrict__ surf, int *flags)
{
    const int n = *n_list;
    const int lane = threadIdx.x % CH_LPS;
    const int rows = (n + CH_SPB - 1) / CH_SPB * CH_SPB;
    const double inf = __longlong_as_double((long long)KMCF_D2_INF);
    for (int k = blockIdx.x * CH_SPB + threadIdx.x / CH_LPS; k < rows; k += gridDim.x * CH_SPB) {
        const bool valid = k < n;
        double bd = inf;                    // this lane's minimum (d2, partner)
        int bb = CH_NO_SITE;
        double dd = inf;                    // FIRST, L members: this lane's smallest d2 to an R member of the cell
        int vc = -1, comp = -1, a = -1;
        bool is_left = false;
        if (valid) {
            a = lsite[k];
            vc = lvcell[k];
            comp = lcomp[k];
            const double xa = lx[k], ya = ly[k], za = lz[k];
            double thr = rmax2;             // no pair with a larger d2 can be this member's or its component's result
            double thr_dir = -1.0;          // ... or the cell's direct2 (L members of round 1 only)
            int rrep = -1;
            if (FIRST) {
                const int *q = words + (size_t)CH_W_WORDS * vc;
                is_left = comp == q[CH_W_LREP];
                rrep = q[CH_W_RREP];
                if (is_left) thr_dir = fmin(rmax2, __shfl(__longlong_as_double((long long)kmcf_load_relaxed(direct + vc)), 0, CH_LPS));
            } else {
                // (the group's first lane's read for all of them: the walk must not part the group's lanes)
                const double seen = __shfl(__longlong_as_double((long long)kmcf_load_relaxed(cbest + comp)), 0, CH_LPS);
                if (seen < thr) thr = seen;
            }
            kmcf_walk_columns(
                g, xa, ya, za, cell_start, lpos, [&](double bound) { return !(bound > thr && bound > thr_dir); },
                [&](int b, int e) {
                    for (int t = b + lane; t < e; t += CH_LPS) {
                        if (lvcell[t] != vc) continue;
                        const int ct = lcomp[t];
                        if (ct == comp) continue;
                        const double d2 = kmcf_walk_d2(g, xa, ya, za, lx[t], ly[t], lz[t]);
                        if (d2 <= rmax2) {
                            const int j = lsite[t];
                            if (d2 < bd || (d2 == bd && j < bb)) { bd = d2; bb = j; }
                            if (FIRST && is_left && ct == rrep && d2 < dd) dd = d2;
                        }
                    }
                },
                [&]() {
                    double m = bd;
#pragma unroll
                    for (int off = CH_LPS / 2; off >= 1; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
                    if (m < thr) thr = m;
                    if (FIRST && is_left) {
                        double md = dd;
#pragma unroll
                        for (int off = CH_LPS / 2; off >= 1; off >>= 1) md = fmin(md, __shfl_xor(md, off, 64));
                        if (md < thr_dir) thr_dir = md;
                    }
                });
        }
#pragma unroll
        for (int off = CH_LPS / 2; off >= 1; off >>= 1) {
            const double od = __shfl_xor(bd, off, 64);
            const int ob = __shfl_xor(bb, off, 64);
            if (od < bd || (od == bd && ob < bb)) { bd = od; bb = ob; }
            if (FIRST) dd = fmin(dd, __shfl_xor(dd, off, 64));
        }
        const bool found = valid && lane == 0 && bb != CH_NO_SITE;
        if (valid && lane == 0) {
            ld2[k] = (u64)__double_as_longlong(bd);
            lj[k] = found ? bb : -1;
            if (found) atomicMin(cbest + comp, (u64)__double_as_longlong(bd));
            if (FIRST) {
                surf[a] = found;
                if (is_left && dd < inf) atomicMin(direct + vc, (u64)__double_as_longlong(dd));
            }
        }
        if (FIRST) {
            const u64 fm = __ballot(found);
            if ((threadIdx.x & 63) == 0 && fm) atomicAdd(flags + CH_F_SURFACE, __popcll(fm));
        }
    }
}

// b: cbest[] is final (earlier launch); few members attain it
__global__ __launch_bounds__(KMCF_BLOCK) void ch_pair_kernel(const int *__restrict__ n_list, const int *__restrict__ lsite,
                                                             const int *__restrict__ lcomp, const u64 *__restrict__ ld2,
                                                             const int *__restrict__ lj, const u64 *__restrict__ cbest, u64 *cpair)
{
    const int n = *n_list;
    for (int k = blockIdx.x * KMCF_BLOCK + threadIdx.x; k < n; k += gridDim.x * KMCF_BLOCK) {
        const int j = lj[k];
        if (j < 0) continue;
        const int comp = lcomp[k], a = lsite[k];
        if (ld2[k] == cbest[comp]) atomicMin(cpair + comp, ((u64)(unsigned)min(a, j) << 32) | (unsigned)max(a, j));
    }
}

// c: root[] and cpair[] are read, next[] and the edge list are written
__global__ __launch_bounds__(KMCF_BLOCK) void ch_hook_kernel(int N, const int *__restrict__ svert, const int *__restrict__ root,
                                                             const u64 *__restrict__ cbest, const u64 *__restrict__ cpair,
                                                             int *__restrict__ next, ch_edge *__restrict__ edges, int *flags)
{
    const int v = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (v >= N) return;
    int to = v;
    const u64 pr = root[v] == v ? cpair[v] : KMCF_NO_PAIR;          // (a site that is no vertex has no pair)
    if (pr != KMCF_NO_PAIR) {
        ch_edge e;
        e.d2 = cbest[v];
        e.a = (int)(pr >> 32);
        e.b = (int)(pr & 0xffffffffull);
        e.va = svert[e.a];
        e.vb = svert[e.b];
        const int ra = root[e.va], rb = root[e.vb];
        const int other = ra == v ? rb : ra;
        const bool mutual = cpair[other] == pr;
        if (!(mutual && v < other)) to = other;
        if (!(mutual && v > other)) {
            const int slot = atomicAdd(flags + CH_F_EDGES, 1);
            if (slot < N) edges[slot] = e;
            else atomicOr(flags + CH_F_ERROR, 1);
        }
    }
    next[v] = to;
}

// d: the hooks form a forest (next[] is not written here); its depth is below N
__global__ __launch_bounds__(KMCF_BLOCK) void ch_jump_kernel(int N, const int *__restrict__ next, int *__restrict__ root,
                                                             u64 *__restrict__ cbest, u64 *__restrict__ cpair, int *flags)
{
    const int v = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (v >= N) return;
    int r = root[v];
    for (int s = 0; s < N; ++s) {
        const int t = next[r];
        if (t == r) break;
        r = t;
    }
    if (next[r] != r) atomicOr(flags + CH_F_ERROR, 2);
    root[v] = r;
    cbest[v] = KMCF_D2_INF;
    cpair[v] = KMCF_NO_PAIR;
}

// e
__global__ __launch_bounds__(KMCF_BLOCK) void ch_open_kernel(size_t n_cells, const int *__restrict__ words,
                                                             const int *__restrict__ root, int *flag)
{
    const size_t c = (size_t)blockIdx.x * KMCF_BLOCK + threadIdx.x;
    bool open = false;
    if (c < n_cells && ch_active(words, (int)c)) {
        const int *q = words + CH_W_WORDS * c;
        open = root[q[CH_W_LREP]] != root[q[CH_W_RREP]];
    }
    const u64 m = __ballot(open);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(flag, __popcll(m));
}

// f (round 3 on): the components of the list
__global__ __launch_bounds__(KMCF_BLOCK) void ch_comp_kernel(const int *__restrict__ n_list, const int *__restrict__ lvert,
                                                             const int *__restrict__ root, int *__restrict__ lcomp)
{
    const int n = *n_list;
    for (int k = blockIdx.x * KMCF_BLOCK + threadIdx.x; k < n; k += gridDim.x * KMCF_BLOCK) lcomp[k] = root[lvert[k]];
}

// scratch on the index, grown on demand and freed by kmcf_pairwise_destroy; it holds nothing a later call reads
int ch_workspace(kmcf_pairwise *p, size_t n_cells)
{
    if (!p->chain_ws) {
        kmcf_chain_ws *w = p->chain_ws = new kmcf_chain_ws();
        const size_t n = (size_t)p->N;
        w->N = p->N;
        KMCF_TRY(kmcf_members_alloc(&w->l, p->N, 1, true));
        for (int **q : {&w->d_side, &w->d_node, &w->d_home, &w->d_svert, &w->d_svcell, &w->d_surf, &w->d_root, &w->d_next,
                        &w->d_lvcell, &w->d_lvert, &w->d_lcomp, &w->d_lj})
            KMCF_TRY(kmcf_dev_alloc(q, n, false));
        for (u64 **q : {&w->d_cbest, &w->d_cpair, &w->d_ld2}) KMCF_TRY(kmcf_dev_alloc(q, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_edges, n, false));
        KMCF_TRY(kmcf_dev_alloc(&w->d_flags, (size_t)CH_F_WORDS, false));
    }
    kmcf_chain_ws *w = p->chain_ws;
    if (w->cap_cells < n_cells) {                      // two buffers of one capacity, exact size
        w->cap_cells = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_words, nullptr, (size_t)CH_W_WORDS * n_cells, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_direct, nullptr, n_cells, 0));
        w->cap_cells = n_cells;
    }
    return KMCF_OK;
}

// the argument checks both entry points share; p comes last: everything before it is checked without an index
int ch_check_common(const char *what, const kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                    double r_max, const int *d_site_cell, int n_cells, const kmcf_chain_t *h_chains, const kmcf_hop_t *h_hops,
                    int max_hops, bool periodic_ok)
{
    KMCF_TRY(kmcf_check_coords(what, d_x, d_y, d_z));
    KMCF_CHECK(h_chains, KMCF_ERR_ARG, "%s: h_chains is NULL", what);
    KMCF_TRY(kmcf_check_radius(what, "r_max", r_max));
    KMCF_TRY(kmcf_check_cells(what, d_site_cell, n_cells));
    KMCF_CHECK(max_hops >= 0, KMCF_ERR_ARG, "%s: max_hops = %d is negative", what, max_hops);
    KMCF_CHECK(!h_hops || max_hops > 0, KMCF_ERR_ARG, "%s: h_hops is set with max_hops = 0", what);
    KMCF_CHECK(h_hops || max_hops == 0, KMCF_ERR_ARG, "%s: h_hops is NULL with max_hops = %d", what, max_hops);
    return kmcf_check_index(what, p, "r_max", r_max, periodic_ok ? nullptr : "chain");
}

// steps 4-6 (kmcf_cellmembers.hpp): the list of the members (surf == nullptr) or of the surface members
void ch_compact(kmcf_pairwise *p, const int *surf, const double *d_x, const double *d_y, const double *d_z)
{
    kmcf_chain_ws *w = p->chain_ws;
    kmcf_members_enqueue<1>(p, w->l, ch_rule{w->d_svert, surf},
                            ch_emit{w->d_svert, w->d_svcell, w->d_root, d_x, d_y, d_z, w->l, w->d_lvcell, w->d_lvert, w->d_lcomp});
}

struct ch_result {
    int rounds = 0, edges = 0, surface = 0;
};

// steps 1-6 and the rounds, behind whatever produced the sides and nodes; one synchronisation per round
int ch_search(const char *what, kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z, const int *d_side,
              const int *d_node, double r_max, const int *d_site_cell, int n_cells, ch_result *res)
{
    kmcf_chain_ws *w = p->chain_ws;
    hipStream_t st = p->comm->stream;
    const int N = p->N;
    const int site_grid = (N + KMCF_BLOCK - 1) / KMCF_BLOCK;
    const size_t nc = (size_t)n_cells;
    const int cell_grid = (int)((nc + KMCF_BLOCK - 1) / KMCF_BLOCK);
    const int *n_list = w->l.d_sum + kmcf_member_tiles(N);
    const int search_grid = (int)std::min<int64_t>(8192, ((int64_t)N + CH_SPB - 1) / CH_SPB);   // the kernel strides
    const int list_grid = std::min(site_grid, 2048);
    const double rmax2 = r_max * r_max;

    ch_clear_kernel<<<std::max(site_grid, cell_grid), KMCF_BLOCK, 0, st>>>(N, nc, w->d_home, w->d_root, w->d_next, w->d_cbest,
                                                                         w->d_cpair, w->d_words, w->d_direct, w->d_flags);
    ch_count_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, d_side, d_node, d_site_cell, n_cells, w->d_words, w->d_home);
    ch_vertex_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, d_side, d_node, d_site_cell, n_cells, w->d_home, w->d_words, w->d_svert,
                                                      w->d_svcell);
    ch_compact(p, nullptr, d_x, d_y, d_z);
    const auto search = [&](auto grid, bool first) {     // step a: the instantiation for the index and the round
        const auto kernel = first ? ch_search_kernel<true, decltype(grid)> : ch_search_kernel<false, decltype(grid)>;
        kernel<<<search_grid, KMCF_BLOCK, 0, st>>>(grid, p->d_cell_start, w->l.d_pos, n_list, w->l.d_site, w->d_lvcell, w->d_lcomp,
                                                  w->l.d_x, w->l.d_y, w->l.d_z, rmax2, w->d_words, w->d_cbest, w->d_direct,
                                                  w->d_ld2, w->d_lj, w->d_surf, w->d_flags);
    };
    int h[CH_F_WORDS];
    int edges_before = 0;
    for (int round = 1; round <= CH_MAX_ROUNDS; ++round) {
        p->with_grid([&](auto grid) { search(grid, round == 1); });
        ch_pair_kernel<<<list_grid, KMCF_BLOCK, 0, st>>>(n_list, w->l.d_site, w->d_lcomp, w->d_ld2, w->d_lj, w->d_cbest, w->d_cpair);
        ch_hook_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, w->d_svert, w->d_root, w->d_cbest, w->d_cpair, w->d_next, w->d_edges,
                                                        w->d_flags);
        ch_jump_kernel<<<site_grid, KMCF_BLOCK, 0, st>>>(N, w->d_next, w->d_root, w->d_cbest, w->d_cpair, w->d_flags);
        ch_open_kernel<<<cell_grid, KMCF_BLOCK, 0, st>>>(nc, w->d_words, w->d_root, w->d_flags + CH_F_OPEN0 + round - 1);
        KMCF_HIP(hipGetLastError());
        KMCF_HIP(hipMemcpyAsync(h, w->d_flags, sizeof(h), hipMemcpyDeviceToHost, st));
        KMCF_HIP(hipStreamSynchronize(st));
        KMCF_CHECK(h[CH_F_ERROR] == 0, KMCF_ERR_STATE, "%s: the component forest is inconsistent (flag %d)", what, h[CH_F_ERROR]);
        res->rounds = round;
        res->edges = h[CH_F_EDGES];
        res->surface = h[CH_F_SURFACE];
        if (h[CH_F_EDGES] == edges_before || h[CH_F_OPEN0 + round - 1] == 0) return KMCF_OK;
        edges_before = h[CH_F_EDGES];
        if (round == 1) ch_compact(p, w->d_surf, d_x, d_y, d_z);
        else ch_comp_kernel<<<list_grid, KMCF_BLOCK, 0, st>>>(n_list, w->d_lvert, w->d_root, w->d_lcomp);
    }
    KMCF_CHECK(false, KMCF_ERR_STATE, "%s: the search did not stop within %d rounds", what, CH_MAX_ROUNDS);
    return KMCF_OK;
}

bool ch_key_less(const ch_edge &p, const ch_edge &q)
{
    return p.d2 != q.d2 ? p.d2 < q.d2 : (p.a != q.a ? p.a < q.a : p.b < q.b);
}

// the copies, the last synchronisation, and the host's part: the tree walk per cell, the records, the hop lists
int ch_finish(kmcf_pairwise *p, int n_cells, const ch_result &res, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops,
              hipEvent_t ev_mid, kmcf_chain_stats_t *stats)
{
    kmcf_comm *c = p->comm;
    kmcf_chain_ws *w = p->chain_ws;
    hipStream_t st = c->stream;
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<int> words((size_t)CH_W_WORDS * n_cells);
    std::vector<u64> direct((size_t)n_cells);
    std::vector<ch_edge> edges((size_t)res.edges);
    KMCF_HIP(hipMemcpyAsync(words.data(), w->d_words, words.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(direct.data(), w->d_direct, direct.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    if (res.edges) KMCF_HIP(hipMemcpyAsync(edges.data(), w->d_edges, edges.size() * sizeof(ch_edge), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(c->ev_call1, st));
    KMCF_HIP(hipStreamSynchronize(st));

    std::sort(edges.begin(), edges.end(), ch_key_less);
    std::unordered_map<int, std::vector<int>> adj;             // vertex -> its forest edges, ascending key
    for (int e = 0; e < (int)edges.size(); ++e) {
        adj[edges[e].va].push_back(e);
        adj[edges[e].vb].push_back(e);
    }
    kmcf_chain_stats_t s = {};
    const kmcf_hop_t no_hop = {-1, -1, inf};
    if (h_hops) std::fill(h_hops, h_hops + (size_t)n_cells * max_hops, no_hop);
    std::unordered_map<int, int> via;                          // vertex -> the edge it was reached through
    std::vector<int> stack;
    std::vector<kmcf_hop_t> hops;
    for (int k = 0; k < n_cells; ++k) {
        const int *q = words.data() + (size_t)CH_W_WORDS * k;
        kmcf_chain_t r;
        r.hop_max = r.hop_max2 = r.direct2 = inf;
        r.length = 0.0;
        r.n_hops = 0;
        r.neck_from = r.neck_to = -1;
        r.n_stones = q[CH_W_STONES];
        r.n_stone_sites = q[CH_W_STONE_SITES];
        r.n_left = q[CH_W_LEFT];
        r.n_right = q[CH_W_RIGHT];
        s.n_stones += r.n_stones;
        s.n_stone_sites += r.n_stone_sites;
        if (q[CH_W_BOTH] > 0) {
            r.status = KMCF_CHAIN_BRIDGED;
            r.hop_max = r.hop_max2 = r.direct2 = 0.0;
            ++s.cells_bridged;
        } else if (r.n_left == 0 || r.n_right == 0) {
            r.status = KMCF_CHAIN_NONE;
            ++s.cells_none;
        } else {
            std::memcpy(&r.direct2, &direct[k], sizeof(double));
            const int src = q[CH_W_LREP], dst = q[CH_W_RREP];
            via.clear();
            via[src] = -1;
            stack.assign(1, src);
            while (!stack.empty() && !via.count(dst)) {
                const int v = stack.back();
                stack.pop_back();
                auto it = adj.find(v);
                if (it == adj.end()) continue;
                for (int e : it->second) {
                    const int u = edges[e].va == v ? edges[e].vb : edges[e].va;
                    if (via.emplace(u, e).second) stack.push_back(u);
                }
            }
            if (!via.count(dst)) {
                r.status = KMCF_CHAIN_OPEN;
                ++s.cells_open;
            } else {
                r.status = KMCF_CHAIN_CHAINED;
                ++s.cells_chained;
                hops.clear();
                for (int v = dst; v != src;) {                 // back from R: (from, to) with `to` on v's side
                    const ch_edge &e = edges[via[v]];
                    const bool to_b = e.vb == v;
                    kmcf_hop_t hop;
                    hop.from = to_b ? e.a : e.b;
                    hop.to = to_b ? e.b : e.a;
                    std::memcpy(&hop.d2, &e.d2, sizeof(double));
                    hops.push_back(hop);
                    v = to_b ? e.va : e.vb;
                }
                std::reverse(hops.begin(), hops.end());
                r.n_hops = (int)hops.size();
                size_t neck = 0;
                for (size_t t = 0; t < hops.size(); ++t) {
                    const kmcf_hop_t &a = hops[t], &b = hops[neck];
                    const int alo = std::min(a.from, a.to), ahi = std::max(a.from, a.to);
                    const int blo = std::min(b.from, b.to), bhi = std::max(b.from, b.to);
                    if (a.d2 > b.d2 || (a.d2 == b.d2 && (alo > blo || (alo == blo && ahi > bhi)))) neck = t;
                    r.length += std::sqrt(a.d2);
                    if (h_hops && t < (size_t)max_hops) h_hops[(size_t)k * max_hops + t] = a;
                }
                r.hop_max2 = hops[neck].d2;
                r.hop_max = std::sqrt(r.hop_max2);
                r.neck_from = hops[neck].from;
                r.neck_to = hops[neck].to;
            }
        }
        h_chains[k] = r;
    }
    if (stats) {
        s.surface_sites = res.surface;
        s.rounds = res.rounds;
        s.forest_edges = res.edges;
        s.ms_clusters = 0.f;
        if (ev_mid) KMCF_HIP(hipEventElapsedTime(&s.ms_clusters, c->ev_t0, ev_mid));
        KMCF_HIP(hipEventElapsedTime(&s.ms_search, ev_mid ? ev_mid : c->ev_t0, c->ev_call1));
        *stats = s;
    }
    return KMCF_OK;
}

// the body of kmcf_site_set_chain and kmcf_site_set_chain_pbc: they differ in the name and in whether a periodic index passes
int ch_site_set_chain(const char *what, bool periodic_ok, kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                      const int *d_site_side, const int *d_site_node, double r_max, const int *d_site_cell, int n_cells,
                      kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops, kmcf_chain_stats_t *stats)
{
    KMCF_CHECK(d_site_side, KMCF_ERR_ARG, "%s: d_site_side is NULL", what);
    KMCF_CHECK(d_site_node, KMCF_ERR_ARG, "%s: d_site_node is NULL", what);
    KMCF_TRY(ch_check_common(what, p, d_x, d_y, d_z, r_max, d_site_cell, n_cells, h_chains, h_hops, max_hops, periodic_ok));
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(ch_workspace(p, (size_t)n_cells));
    KMCF_HIP(hipEventRecord(c->ev_t0, c->stream));
    ch_result res;
    KMCF_TRY(ch_search(what, p, d_x, d_y, d_z, d_site_side, d_site_node, r_max, d_site_cell, n_cells, &res));
    return ch_finish(p, n_cells, res, h_chains, h_hops, max_hops, nullptr, stats);
}

// the body of kmcf_filament_chain and kmcf_filament_chain_pbc
int ch_filament_chain(const char *what, bool periodic_ok, kmcf_pairwise *p, int nn, const int *d_neigh_idx,
                      const int *d_site_element, const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                      const double *d_y, const double *d_z, int N_left_tot, int N_right_tot, double r_max, const int *d_site_cell,
                      int n_cells, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops, int *d_site_side, int *d_site_node,
                      kmcf_chain_stats_t *stats)
{
    KMCF_CHECK(d_neigh_idx, KMCF_ERR_ARG, "%s: d_neigh_idx is NULL", what);
    KMCF_CHECK(d_site_element, KMCF_ERR_ARG, "%s: d_site_element is NULL", what);
    KMCF_CHECK(d_site_charge, KMCF_ERR_ARG, "%s: d_site_charge is NULL", what);
    KMCF_CHECK(nn > 0, KMCF_ERR_ARG, "%s: nn = %d is not > 0", what, nn);
    KMCF_CHECK(num_metals >= 0, KMCF_ERR_ARG, "%s: num_metals = %d is negative", what, num_metals);
    KMCF_CHECK(num_metals == 0 || d_metals, KMCF_ERR_ARG, "%s: d_metals is NULL with num_metals = %d", what, num_metals);
    KMCF_CHECK(N_left_tot >= 0, KMCF_ERR_ARG, "%s: N_left_tot = %d is negative", what, N_left_tot);
    KMCF_CHECK(N_right_tot >= 0, KMCF_ERR_ARG, "%s: N_right_tot = %d is negative", what, N_right_tot);
    KMCF_TRY(ch_check_common(what, p, d_x, d_y, d_z, r_max, d_site_cell, n_cells, h_chains, h_hops, max_hops, periodic_ok));
    const int N = p->N;
    KMCF_CHECK((int64_t)N_left_tot + N_right_tot <= N, KMCF_ERR_ARG, "%s: N_left_tot + N_right_tot = %lld exceeds N = %d", what,
               (long long)N_left_tot + N_right_tot, N);
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(ch_workspace(p, (size_t)n_cells));
    kmcf_chain_ws *w = p->chain_ws;
    hipStream_t st = c->stream;
    int *side = d_site_side ? d_site_side : w->d_side;
    int *node = d_site_node ? d_site_node : w->d_node;
    kmcf_cluster_dev cl;
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    KMCF_TRY(kmcf_clusters_enqueue(c, N, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals, d_x, N_left_tot,
                                   N_right_tot, nullptr, false, 0, &cl));
    ch_side_node_kernel<<<(N + KMCF_BLOCK - 1) / KMCF_BLOCK, KMCF_BLOCK, 0, st>>>(N, cl.cls, cl.label, cl.touch, side, node);
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    ch_result res;
    KMCF_TRY(ch_search(what, p, d_x, d_y, d_z, side, node, r_max, d_site_cell, n_cells, &res));
    return ch_finish(p, n_cells, res, h_chains, h_hops, max_hops, c->ev_t1, stats);
}

}  // namespace

extern "C" int kmcf_site_set_chain(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                   const int *d_site_side, const int *d_site_node, double r_max, const int *d_site_cell,
                                   int n_cells, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops,
                                   kmcf_chain_stats_t *stats)
{
    return ch_site_set_chain("kmcf_site_set_chain", false, p, d_x, d_y, d_z, d_site_side, d_site_node, r_max, d_site_cell, n_cells,
                             h_chains, h_hops, max_hops, stats);
}

extern "C" int kmcf_site_set_chain_pbc(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z,
                                       const int *d_site_side, const int *d_site_node, double r_max, const int *d_site_cell,
                                       int n_cells, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops,
                                       kmcf_chain_stats_t *stats)
{
    return ch_site_set_chain("kmcf_site_set_chain_pbc", true, p, d_x, d_y, d_z, d_site_side, d_site_node, r_max, d_site_cell,
                             n_cells, h_chains, h_hops, max_hops, stats);
}

extern "C" int kmcf_filament_chain(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                                   const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                                   const double *d_y, const double *d_z, int N_left_tot, int N_right_tot, double r_max,
                                   const int *d_site_cell, int n_cells, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops, int max_hops,
                                   int *d_site_side, int *d_site_node, kmcf_chain_stats_t *stats)
{
    return ch_filament_chain("kmcf_filament_chain", false, p, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals, num_metals,
                             d_x, d_y, d_z, N_left_tot, N_right_tot, r_max, d_site_cell, n_cells, h_chains, h_hops, max_hops,
                             d_site_side, d_site_node, stats);
}

extern "C" int kmcf_filament_chain_pbc(kmcf_pairwise *p, int nn, const int *d_neigh_idx, const int *d_site_element,
                                       const int *d_site_charge, const int *d_metals, int num_metals, const double *d_x,
                                       const double *d_y, const double *d_z, int N_left_tot, int N_right_tot, double r_max,
                                       const int *d_site_cell, int n_cells, kmcf_chain_t *h_chains, kmcf_hop_t *h_hops,
                                       int max_hops, int *d_site_side, int *d_site_node, kmcf_chain_stats_t *stats)
{
    return ch_filament_chain("kmcf_filament_chain_pbc", true, p, nn, d_neigh_idx, d_site_element, d_site_charge, d_metals,
                             num_metals, d_x, d_y, d_z, N_left_tot, N_right_tot, r_max, d_site_cell, n_cells, h_chains, h_hops,
                             max_hops, d_site_side, d_site_node, stats);
}
