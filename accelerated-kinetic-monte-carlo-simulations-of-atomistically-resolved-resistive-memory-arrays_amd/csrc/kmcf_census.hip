// Event rate census (kmcf_event_census; no reference counterpart): the event list of a step reduced on the device to
// rates per cell, layer and event type, a spectrum of the rates' binary exponents and, on request, a sum and a best slot
// per row.  The entry point, its checks and the build kernel live in kmcf_events.hip; this file gets the build as a
// callback (kmcf_census_args::build) that fills the census's OWN copy of the list, and reads nothing of the event step.
//
// The list is sparse (40 nm crossbar: 1e4 - 1e5 live of 85 M slots), so everything behind the build works on the live
// slots only:
//   census_count_kernel / kmcf_scan_counts_kernel / census_scatter_kernel   the live slots in ascending slot id (the
//                         flag / scan / scatter compaction of kmcf_block.hpp; one read of the type bytes each)
//   census_key_kernel     per live slot p: its bucket as a 16-bit key; spectrum, n_nan and rows_live by integer atomics
//                         (exact whatever the order); the slot that opens a row also walks the row for the row outputs
//   census_reduce_kernel  the live list cut into pieces (census_pieces: from count * nn, 1 .. 64); block (bucket, piece)
//                         walks the keys of its piece: thread t takes the events p = first + t, + 256, ... and keeps count,
//                         zero count, sum and the maximum with its slot of those that carry the block's key; then
//                         kmcf_block_sum and an LDS tree for the maximum
//   census_combine_kernel one thread per bucket adds its pieces in ascending order and writes the bucket
//                         No atomics on doubles: the order of addition follows from p, that is from the input alone.
// Scratch per slot: 1 B type + 8 B rate + 4 B live slot + 2 B key (the live list is sized for a full list: its length
// is known on the device only, and the call synchronises once, at its end).
#include <climits>
#include <cstring>
#include <limits>
#include <vector>

#include "kmcf_internal.hpp"

static_assert(sizeof(kmcf_census_bucket_t) == 40, "kmcf_census_bucket_t: 40 bytes, written by the device as it stands");

typedef unsigned long long kmcf_cs_u64;

// what one piece of the live list holds of one bucket (census_reduce_kernel -> census_combine_kernel)
struct census_part { double sum, best; int cnt, nz, bslot, pad; };

struct kmcf_census_ws {
    size_t cap_M = 0;                   // slots the four per-slot buffers hold
    unsigned char *d_type = nullptr;
    double *d_prob = nullptr;
    int *d_live = nullptr;              // live slots, ascending
    unsigned short *d_key = nullptr;    // ... and their buckets (CS_NO_KEY: none)
    size_t cap_tiles = 0;
    int *d_offs = nullptr;              // tiles + 1: live slots per tile, scanned in place; the total behind them
    size_t cap_keys = 0;
    kmcf_census_bucket_t *d_table = nullptr;
    int *d_maxslot = nullptr;           // slot of a bucket's maximum (-1: none): what the overall maximum is decided by
    census_part *d_part = nullptr;         // buckets x pieces: what each piece of the live list holds of each bucket
    kmcf_cs_u64 *d_cnt = nullptr;       // CS_WORDS: the spectrum, n_nan, rows_live
    int *d_bad = nullptr;               // the build kernel's word of the thermal modes
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

void kmcf_census_ws_free(kmcf_comm *c)
{
    if (!c || !c->cs_ws) return;
    kmcf_census_ws *w = c->cs_ws;
    kmcf_dev_free_all({w->d_type, w->d_prob, w->d_live, w->d_key, w->d_offs, w->d_table, w->d_maxslot, w->d_part, w->d_cnt, w->d_bad});
    for (hipEvent_t e : w->ev)
        if (e) hipEventDestroy(e);
    delete w;
    c->cs_ws = nullptr;
}

namespace {

constexpr int CS_NULL = 4;                                  // EVENTTYPE NULL_EVENT (kmcf_events.hip: EV_NULL)
constexpr int CS_MAX_BINS = 256, CS_SPEC = 4 * CS_MAX_BINS;
constexpr int CS_W_NAN = CS_SPEC, CS_W_ROWS = CS_SPEC + 1, CS_WORDS = CS_SPEC + 2;
constexpr int CS_UNROLL = 8;                                // keys a thread of census_reduce_kernel requests before it looks at one
constexpr unsigned short CS_NO_KEY = 0xffff;                // (keys < (1024 + 1) * 8 * 4 = 32800)

// the live flags of this thread's KMCF_SCAN_ITEMS slots: one 8-byte read where the tile is whole
__device__ __forceinline__ void census_flags(int M, const unsigned char *__restrict__ type, int (&f)[KMCF_SCAN_ITEMS])
{
    static_assert(KMCF_SCAN_ITEMS == 8, "one 64-bit word of type bytes per thread");
    const int t0 = kmcf_tile_item0();
    kmcf_cs_u64 w = 0;
    const bool whole = t0 >= 0 && t0 <= M - KMCF_SCAN_ITEMS;
    if (whole) w = *reinterpret_cast<const kmcf_cs_u64 *>(type + t0);
    kmcf_tile_flags(M, f, [&](int id) {
        const int ty = whole ? (int)((w >> (8 * (id - t0))) & 0xff) : (int)type[id];
        return ty != CS_NULL;
    });
}

__global__ __launch_bounds__(KMCF_BLOCK) void census_count_kernel(int M, const unsigned char *__restrict__ type, int *__restrict__ counts)
{
    __shared__ int lds4[4];
    int f[KMCF_SCAN_ITEMS];
    census_flags(M, type, f);
    const int n = kmcf_tile_count(f, lds4);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

__global__ __launch_bounds__(KMCF_BLOCK) void census_scatter_kernel(int M, const unsigned char *__restrict__ type, const int *__restrict__ offs,
                                                                    int *__restrict__ live)
{
    __shared__ int lds4[4];
    int f[KMCF_SCAN_ITEMS];
    census_flags(M, type, f);
    int pos = kmcf_tile_pos(f, offs[blockIdx.x], lds4);
    const int t0 = kmcf_tile_item0();
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k)
        if (f[k]) live[pos++] = t0 + k;         // (pos < offs[tiles] <= M: as many flagged items as the count kernel saw)
}

struct census_key_args {
    int displ, nn, num_layers, n_cells, n_bins, e_lo, e_step;
    const int *neigh, *layer, *cell;
    const unsigned char *type;
    const double *prob;
    const int *live, *n_live;
    unsigned short *key;
    kmcf_cs_u64 *cnt;
    double *row_rate;
    int *row_best;
};

// bin of a rate that is not NaN (header: the rule of the spectrum)
__device__ __forceinline__ int census_bin(double P, int n_bins, int e_lo, int e_step)
{
    const kmcf_cs_u64 bits = (kmcf_cs_u64)__double_as_longlong(P);
    const int be = (int)((bits >> 52) & 0x7ff);
    if (be == 0) return 0;                                  // 0.0 and subnormals
    if (be == 0x7ff) return n_bins - 1;                     // infinity
    const long long d = (long long)be - 1023 - e_lo;        // (64 bits: any int e_lo)
    const long long b = d >= 0 ? d / e_step : -((-d + e_step - 1) / e_step);      // floor
    return (int)min(max(b, 0ll), (long long)n_bins - 1);
}

__global__ __launch_bounds__(KMCF_BLOCK) void census_key_kernel(census_key_args a)
{
    __shared__ unsigned int hist[CS_SPEC];
    const int n = *a.n_live, nh = 4 * a.n_bins;
    for (int q = threadIdx.x; q < nh; q += KMCF_BLOCK) hist[q] = 0;
    __syncthreads();
    for (long long p = (long long)blockIdx.x * KMCF_BLOCK + threadIdx.x; p < n; p += (long long)gridDim.x * KMCF_BLOCK) {
        const int slot = a.live[p], r = slot / a.nn, i = a.displ + r;
        const int j = a.neigh[slot], ty = a.type[slot];     // (a live slot: 0 <= j < N, ty in 0..3, by the build kernel)
        const int l = a.layer[j];
        int cell = a.cell ? a.cell[i] : 0;
        if (cell < 0 || cell >= a.n_cells) cell = a.n_cells;
        const bool in_table = l >= 0 && l < a.num_layers && ty >= 0 && ty < 4;
        a.key[p] = in_table ? (unsigned short)((cell * a.num_layers + l) * 4 + ty) : CS_NO_KEY;
        const double P = a.prob[slot];
        if (in_table) {
            if (P != P) atomicAdd(&a.cnt[CS_W_NAN], 1ull);
            else if (a.n_bins > 0) atomicAdd(&hist[ty * a.n_bins + census_bin(P, a.n_bins, a.e_lo, a.e_step)], 1u);
        }
        if (p == 0 || a.live[p - 1] / a.nn != r) {          // the slot that opens its row
            atomicAdd(&a.cnt[CS_W_ROWS], 1ull);
            if (a.row_rate || a.row_best) {
                double acc = 0.0, best = 0.0;
                int bs = -1;
                for (int s = 0; s < a.nn; ++s) {
                    const int sl = r * a.nn + s;
                    if (a.type[sl] == CS_NULL) continue;
                    const double Q = a.prob[sl];
                    if (Q != Q) continue;
                    acc += Q;
                    if (bs < 0 || Q > best) { best = Q; bs = s; }
                }
                if (a.row_rate) a.row_rate[r] = acc;
                if (a.row_best) a.row_best[r] = bs;
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nh; q += KMCF_BLOCK)
        if (hist[q]) atomicAdd(&a.cnt[q], (kmcf_cs_u64)hist[q]);
}

// the better of two candidates (rate, slot): the larger rate, among equal rates the smaller slot; slot INT_MAX: none
__device__ __forceinline__ bool census_better(double ra, int sa, double rb, int sb)
{
    if (sa == INT_MAX) return false;
    if (sb == INT_MAX) return true;
    return ra > rb || (ra == rb && sa < sb);
}

// Block (bucket, piece): the live list is cut into gridDim.y pieces of ceil(n / pieces) consecutive events; thread t takes
// the events p = first + t, first + t + 256, ... of its piece and keeps count, zero count, sum and the maximum with its
// slot of those that carry the block's key; then kmcf_block_sum and an LDS tree for the maximum.
__global__ __launch_bounds__(KMCF_BLOCK) void census_reduce_kernel(const double *__restrict__ prob, const int *__restrict__ live,
                                                                   const int *__restrict__ n_live, const unsigned short *__restrict__ key,
                                                                   census_part *__restrict__ part)
{
    __shared__ double lds4[4];
    __shared__ int ilds4[4];
    __shared__ double s_rate[KMCF_BLOCK];
    __shared__ int s_slot[KMCF_BLOCK];
    const long long n = *n_live, chunk = (n + gridDim.y - 1) / gridDim.y;      // (64 bits: n may lie just below 2^31)
    const long long first = chunk * blockIdx.y, end = min(first + chunk, n);
    const unsigned short mine = (unsigned short)blockIdx.x;
    int cnt = 0, nz = 0, bslot = INT_MAX;
    double sum = 0.0, best = 0.0;
    // CS_UNROLL keys per thread in flight (the walk is bound by the latency of a 2-byte load, not by bytes); they are taken
    // in ascending p, so the order of addition is the one of the plain loop
    for (long long p0 = first + threadIdx.x; p0 < end; p0 += KMCF_BLOCK * CS_UNROLL) {
        unsigned short k[CS_UNROLL];
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u) {
            const long long p = p0 + u * KMCF_BLOCK;
            k[u] = p < end ? key[p] : CS_NO_KEY;
        }
#pragma unroll
        for (int u = 0; u < CS_UNROLL; ++u) {
            if (k[u] != mine) continue;
            const int slot = live[p0 + u * KMCF_BLOCK];
            const double P = prob[slot];
            ++cnt;
            if (P != P) continue;
            nz += (P == 0.0);
            sum += P;
            if (bslot == INT_MAX || P > best) { best = P; bslot = slot; }      // (ascending slots: the first among equals stays)
        }
    }
    const double total = kmcf_block_sum(sum, lds4);
    int n_ev, n_zero;
    kmcf_block_excl_scan(cnt, ilds4, &n_ev);
    kmcf_block_excl_scan(nz, ilds4, &n_zero);
    s_rate[threadIdx.x] = best; s_slot[threadIdx.x] = bslot;
    __syncthreads();
    for (int h = KMCF_BLOCK / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h && census_better(s_rate[threadIdx.x + h], s_slot[threadIdx.x + h], s_rate[threadIdx.x], s_slot[threadIdx.x])) {
            s_rate[threadIdx.x] = s_rate[threadIdx.x + h]; s_slot[threadIdx.x] = s_slot[threadIdx.x + h];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = census_part{total, s_rate[0], n_ev, n_zero, s_slot[0], 0};
}

// One thread per bucket: its pieces in ascending order -- integers add, the sums are added one after the other from 0.0,
// the maximum goes to the larger rate (pieces ascend in slot id: the first among equals stays).
__global__ __launch_bounds__(KMCF_BLOCK) void census_combine_kernel(int n_keys, int pieces, int displ, int nn, const int *__restrict__ neigh,
                                                                    const census_part *__restrict__ part,
                                                                    kmcf_census_bucket_t *__restrict__ table, int *__restrict__ maxslot)
{
    const int key = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    if (key >= n_keys) return;
    long long n_ev = 0;
    int n_zero = 0, bslot = INT_MAX;
    double sum = 0.0, best = 0.0;
    for (int q = 0; q < pieces; ++q) {
        const census_part a = part[(size_t)key * pieces + q];
        n_ev += a.cnt; n_zero += a.nz; sum += a.sum;
        if (census_better(a.best, a.bslot, best, bslot)) { best = a.best; bslot = a.bslot; }
    }
    const bool any = bslot != INT_MAX;
    kmcf_census_bucket_t b;
    b.n_events = n_ev; b.rate_sum = sum; b.rate_max = any ? best : 0.0;
    b.max_i = any ? displ + bslot / nn : -1; b.max_j = any ? neigh[bslot] : -1;
    b.n_zero = n_zero; b.reserved = 0;
    table[key] = b;
    maxslot[key] = any ? bslot : -1;
}

// pieces the live list is cut into: from the list's size (the number of live slots is known on the device only), so that
// a block has a few keys per thread on a sparse list, and at most 65536 blocks in all
int census_pieces(size_t M, size_t n_keys)
{
    const size_t by_size = std::max<size_t>(M / 32768, 1), by_grid = std::max<size_t>(65536 / n_keys, 1);
    return (int)std::min<size_t>(std::min(by_size, by_grid), 64);
}

// the scratch for M slots and n_keys buckets; contents are not kept
int census_workspace(kmcf_comm *c, size_t M, size_t tiles, size_t n_keys)
{
    if (!c->cs_ws) c->cs_ws = new kmcf_census_ws();
    kmcf_census_ws *w = c->cs_ws;
    if (M > w->cap_M) {
        w->cap_M = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_type, nullptr, M, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_prob, nullptr, M, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_live, nullptr, M, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_key, nullptr, M, 0));
        w->cap_M = M;
    }
    KMCF_TRY(kmcf_dev_grow(&w->d_offs, &w->cap_tiles, tiles + 1, 0));
    if (n_keys > w->cap_keys) {
        w->cap_keys = 0;
        KMCF_TRY(kmcf_dev_grow(&w->d_table, nullptr, n_keys, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_maxslot, nullptr, n_keys, 0));
        KMCF_TRY(kmcf_dev_grow(&w->d_part, nullptr, n_keys * 64, 0));
        w->cap_keys = n_keys;
    }
    if (!w->d_cnt) KMCF_TRY(kmcf_dev_alloc(&w->d_cnt, (size_t)CS_WORDS, false));
    if (!w->d_bad) KMCF_TRY(kmcf_dev_alloc(&w->d_bad, (size_t)1, false));
    for (hipEvent_t &e : w->ev)
        if (!e) KMCF_HIP(hipEventCreate(&e));
    return KMCF_OK;
}

// The statistics, from the table (and the slots of its maxima) alone.
void census_stats(const kmcf_census_args &a, const kmcf_census_bucket_t *t, const int *maxslot, kmcf_census_stats_t *s)
{
    const int L = a.num_layers;
    int best_slot = -1;
    s->rate_max = 0.0; s->max_i = s->max_j = s->max_type = -1;
    for (int ty = 0; ty < 4; ++ty) {
        double r = 0.0;
        for (int cell = 0; cell <= a.n_cells; ++cell)
            for (int l = 0; l < L; ++l) {
                const int key = (cell * L + l) * 4 + ty;
                const kmcf_census_bucket_t &b = t[key];
                r += b.rate_sum;
                s->n_type[ty] += b.n_events; s->n_events += b.n_events; s->n_zero += b.n_zero;
                const int ms = maxslot ? maxslot[key] : -1;
                if (ms >= 0 && (best_slot < 0 || b.rate_max > s->rate_max || (b.rate_max == s->rate_max && ms < best_slot))) {
                    best_slot = ms; s->rate_max = b.rate_max; s->max_i = b.max_i; s->max_j = b.max_j; s->max_type = ty;
                }
            }
        s->rate_type[ty] = r;
    }
    s->rate_total = ((s->rate_type[0] + s->rate_type[1]) + s->rate_type[2]) + s->rate_type[3];
    s->dt_mean = s->rate_total == 0 ? std::numeric_limits<double>::infinity() : 1 / s->rate_total;
}

}  // namespace

int kmcf_census_run(kmcf_comm *c, const kmcf_census_args &a)
{
    hipStream_t st = c->stream;
    const size_t M = (size_t)a.count * a.nn, n_keys = (size_t)(a.n_cells + 1) * a.num_layers * 4;
    kmcf_census_stats_t stats;
    memset(&stats, 0, sizeof(stats));
    stats.slots = (int64_t)M;
    if (a.n_bins > 0) memset(a.h_spectrum, 0, (size_t)4 * a.n_bins * sizeof(int64_t));
    if (M == 0) {                                           // no rows: the table of a list without events
        for (size_t q = 0; q < n_keys; ++q) a.h_table[q] = kmcf_census_bucket_t{0, 0.0, 0.0, -1, -1, 0, 0};
        census_stats(a, a.h_table, nullptr, &stats);
        if (a.stats) *a.stats = stats;
        return KMCF_OK;
    }
    const int Mi = (int)M, tiles = (Mi + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE;
    KMCF_TRY(census_workspace(c, M, (size_t)tiles, n_keys));
    kmcf_census_ws *w = c->cs_ws;
    std::vector<int> h_maxslot(n_keys);
    std::vector<kmcf_cs_u64> h_cnt(CS_WORDS);
    int bad_site = KMCF_NO_BAD_SITE;
    const int *d_n_live = w->d_offs + tiles;
    KMCF_HIP(hipMemsetAsync(w->d_bad, 0x7f, sizeof(int), st));
    KMCF_HIP(hipMemsetAsync(w->d_cnt, 0, CS_WORDS * sizeof(kmcf_cs_u64), st));
    if (a.d_row_rate) KMCF_HIP(hipMemsetAsync(a.d_row_rate, 0, (size_t)a.count * sizeof(double), st));
    if (a.d_row_best) KMCF_HIP(hipMemsetAsync(a.d_row_best, 0xff, (size_t)a.count * sizeof(int), st));
    KMCF_HIP(hipEventRecord(w->ev[0], st));
    a.build(a.ctx, w->d_type, w->d_prob, w->d_bad);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipEventRecord(w->ev[1], st));
    census_count_kernel<<<tiles, KMCF_BLOCK, 0, st>>>(Mi, w->d_type, w->d_offs);
    kmcf_scan_counts_kernel<int><<<1, KMCF_BLOCK, 0, st>>>(tiles, w->d_offs, w->d_offs, 0);
    census_scatter_kernel<<<tiles, KMCF_BLOCK, 0, st>>>(Mi, w->d_type, w->d_offs, w->d_live);
    const census_key_args ka = {a.displ, a.nn, a.num_layers, a.n_cells, a.n_bins, a.e_lo, a.e_step, a.d_neigh_idx, a.d_site_layer,
                                a.d_site_cell, w->d_type, w->d_prob, w->d_live, d_n_live, w->d_key, w->d_cnt, a.d_row_rate, a.d_row_best};
    census_key_kernel<<<kmcf_grid1d((int64_t)M, 1024), KMCF_BLOCK, 0, st>>>(ka);
    const int pieces = census_pieces(M, n_keys);
    census_reduce_kernel<<<dim3((unsigned)n_keys, (unsigned)pieces), KMCF_BLOCK, 0, st>>>(w->d_prob, w->d_live, d_n_live, w->d_key, w->d_part);
    census_combine_kernel<<<kmcf_grid1d((int64_t)n_keys), KMCF_BLOCK, 0, st>>>((int)n_keys, pieces, a.displ, a.nn, a.d_neigh_idx, w->d_part,
                                                                            w->d_table, w->d_maxslot);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(a.h_table, w->d_table, n_keys * sizeof(kmcf_census_bucket_t), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h_maxslot.data(), w->d_maxslot, n_keys * sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h_cnt.data(), w->d_cnt, CS_WORDS * sizeof(kmcf_cs_u64), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(&bad_site, w->d_bad, sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(w->ev[2], st));
    KMCF_HIP(hipStreamSynchronize(st));
    KMCF_CHECK(bad_site == KMCF_NO_BAD_SITE, KMCF_ERR_ARG, "%s: the temperature of site %d is not finite or not > 0 (it owns an event)",
               a.what, bad_site);
    for (int q = 0; q < 4 * a.n_bins; ++q) a.h_spectrum[q] = (int64_t)h_cnt[q];
    census_stats(a, a.h_table, h_maxslot.data(), &stats);
    stats.n_nan = (int64_t)h_cnt[CS_W_NAN];
    stats.rows_live = (int)h_cnt[CS_W_ROWS];
    KMCF_HIP(hipEventElapsedTime(&stats.ms_build, w->ev[0], w->ev[1]));
    KMCF_HIP(hipEventElapsedTime(&stats.ms_census, w->ev[1], w->ev[2]));
    if (a.stats) *a.stats = stats;
    return KMCF_OK;
}
