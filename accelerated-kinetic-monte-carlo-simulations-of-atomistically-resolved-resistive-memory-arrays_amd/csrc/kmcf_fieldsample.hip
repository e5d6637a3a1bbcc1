// Field sampling: site fields on sample points (kmcf_field_sample) and on regular grids (kmcf_field_grid).
//
// The reference has no counterpart.  Definitions (members, distance, weight, outputs, order of addition, errors):
// include/kmcfield.h and DESIGN.md 3.17.
//
// Launches, all on the compute stream:
//   0    hipMemsetAsync of the stat words (empty points, visits, packed maximum) and of the two bad-point words
//   1-3  compact the members (mask) in INDEX cell order with site id, coordinates and the n_fields value rows: the shared
//        compaction of kmcf_cellmembers.hpp (fs_rule, fs_emit) on scratch of this file's own; a run of the walk is then a
//        contiguous stream
//   4    walk: 16 lanes per point stride over the contiguous runs of the 27 surrounding index cells (radius <= cell edge;
//        kmcf_walk_columns of kmcf_cellwalk.hpp); count, nearest, wsum and the accumulators of the fields in registers,
//        reduced over the group by shuffles; lane 0 writes
// Both entry points run the same walk kernel; they differ in where a point's coordinates come from (POINTS).
//
// Determinism: the doubles are added in the order the header states (per lane along the walk, then the xor butterfly
// 8, 4, 2, 1); the stats are integer adds and an integer maximum.  No atomics on doubles.  No thread waits for another.
#include <cmath>

#include "kmcf_cellwalk.hpp"

static_assert(sizeof(kmcf_sample_stats_t) == 40, "kmcf_sample_stats_t is 40 bytes");

struct kmcf_fs_ws {
    kmcf_members m;                              // members (index-cell order) with coordinates ...
    double *d_mval = nullptr;                    // ... and value rows, field-major with stride N
    size_t cap_mval = 0;
    unsigned long long *d_stat = nullptr;        // FS_STAT_WORDS words: empty points, visits, packed maximum, bad points
};

void kmcf_fs_ws_free(kmcf_pairwise *p)
{
    if (!p || !p->fs_ws) return;
    kmcf_fs_ws *w = p->fs_ws;
    kmcf_members_free(&w->m);
    kmcf_dev_free_all({w->d_mval, w->d_stat});
    delete w;
    p->fs_ws = nullptr;
}

namespace {

typedef unsigned long long u64;
constexpr int FS_LPS = 16, FS_SPB = KMCF_BLOCK / FS_LPS;          // lanes per point, points per block and pass
constexpr int FS_PASSES = 4;                                      // passes of FS_SPB consecutive points per block
constexpr int FS_MAX_FIELDS = KMCF_FS_MAX_FIELDS;
constexpr int FS_EMPTY = 0, FS_VISITS = 1, FS_MAX = 2, FS_BAD = 3, FS_STAT_WORDS = 4;   // FS_BAD: two ints
constexpr int FS_NO_POINT = 0x7f7f7f7f;                           // a bad-point word at rest (a byte pattern)
constexpr double FS_FAR_PERIODS = 1000.0;

// where a point's coordinates come from: three arrays, or the grid rule (a multiplication and an addition per coordinate)
struct fs_points_arrays {
    const double *px, *py, *pz;
    __device__ __forceinline__ void get(int s, double &x, double &y, double &z) const { x = px[s]; y = py[s]; z = pz[s]; }
};
struct fs_points_grid {
    double ox, oy, oz, hx, hy, hz;
    int ny, nz;
    __device__ __forceinline__ void get(int s, double &x, double &y, double &z) const
    {
        const int k = s % nz, ij = s / nz, j = ij % ny, i = ij / ny;
        x = ox + (double)i * hx;
        y = oy + (double)j * hy;
        z = oz + (double)k * hz;
    }
};

// the position the walk starts from: the point itself on the open index, wrapped into the period in y and z on the
// periodic one; false: the point lies too far out (bad-point word `far`)
__device__ __forceinline__ bool fs_walk_pos(const kmcf_cell_grid &, double, double, double &, double &) { return true; }
__device__ __forceinline__ bool fs_walk_pos(const kmcf_cell_grid_pbc &g, double y, double z, double &yw, double &zw)
{
    if (fabs(y - g.y0) > FS_FAR_PERIODS * g.ly || fabs(z - g.z0) > FS_FAR_PERIODS * g.lz) return false;
    yw = y - floor((y - g.y0) / g.ly) * g.ly;
    zw = z - floor((z - g.z0) / g.lz) * g.lz;
    return true;
}

// 1-3, the list: the members (mask; none: every site) with site id, coordinates and value rows
struct fs_rule {
    const int *mask;
    __device__ __forceinline__ int operator()(int i) const { return mask ? mask[i] != 0 : 1; }
};
struct fs_emit {
    const double *x, *y, *z;
    int N, n_fields;
    const double *values;
    kmcf_members m;
    double *mval;
    __device__ __forceinline__ void operator()(int, int q, int i, int) const
    {
        kmcf_member_put(m, q, i, x, y, z);
        for (int k = 0; k < n_fields; ++k) mval[(size_t)k * N + q] = values[(size_t)k * N + i];
    }
};

// 4: the walk, on the open (GRID = kmcf_cell_grid) or the periodic index (kmcf_cell_grid_pbc: the minimum image in y and
// z).  Block b serves the points [b * FS_PASSES * FS_SPB, (b + 1) * FS_PASSES * FS_SPB), FS_SPB per pass, a group of FS_LPS
// lanes each; every pass runs over the whole block, so every lane of a wave reaches the shuffles behind the walk.  The
// threshold r2 is uniform, as the walk requires (kmcf_cellwalk.hpp).  NF: the bucket of n_fields (0, 1, 2, 4, 8): the
// accumulators are registers; those at and above n_fields stay 0 and are not written.
template <class GRID, int NF, class POINTS>
__global__ __launch_bounds__(KMCF_BLOCK) void fs_walk_kernel(GRID g, POINTS pts, int n_points, const int *__restrict__ cell_start,
                                                             const int *__restrict__ mpos, const int *__restrict__ msite,
                                                             const double *__restrict__ mx, const double *__restrict__ my,
                                                             const double *__restrict__ mz, const double *__restrict__ mval,
                                                             int N, int n_fields, double r2, int normalize, double fill,
                                                             double *__restrict__ out, double *__restrict__ wsum_out,
                                                             int *__restrict__ count_out, int *__restrict__ nearest_out,
                                                             double *__restrict__ nearest_d2_out, u64 *stat)
{
    constexpr int NA = NF ? NF : 1;
    const int lane = threadIdx.x % FS_LPS;
    const int64_t k0 = (int64_t)blockIdx.x * (FS_PASSES * FS_SPB);
    u64 n_empty = 0, n_visits = 0, best = 0;                        // of this thread's points (lane 0 of a group)
    for (int pass = 0; pass < FS_PASSES; ++pass) {
        const int64_t k = k0 + pass * FS_SPB + threadIdx.x / FS_LPS;
        const bool in_range = k < n_points;
        const int s = in_range ? (int)k : 0;
        bool valid = in_range;
        int cnt = 0, near_id = -1;
        u64 near_bits = KMCF_D2_INF;
        double wsum = 0.0, acc[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[q] = 0.0;
        if (in_range) {
            double xa, ya, za;
            pts.get(s, xa, ya, za);
            double yw = ya, zw = za;
            int *bad = reinterpret_cast<int *>(stat + FS_BAD);
            if (!(isfinite(xa) && isfinite(ya) && isfinite(za))) {
                valid = false;
                if (lane == 0) atomicMin(bad, s);
            } else if (!fs_walk_pos(g, ya, za, yw, zw)) {
                valid = false;
                if (lane == 0) atomicMin(bad + 1, s);
            }
            if (valid)
                kmcf_walk_columns(
                    g, xa, yw, zw, cell_start, mpos, [&](double bound) { return !(bound > r2); },
                    [&](int b, int e) {
                        for (int t = b + lane; t < e; t += FS_LPS) {
                            const double d2 = kmcf_walk_d2(g, xa, ya, za, mx[t], my[t], mz[t]);
                            if (!(d2 <= r2)) continue;
                            const double u = d2 / r2, tt = 1.0 - u, w = tt * tt;
                            ++cnt;
                            wsum += w;
#pragma unroll
                            for (int q = 0; q < NF; ++q)
                                if (q < n_fields) acc[q] += w * mval[(size_t)q * N + t];
                            const u64 bits = (u64)__double_as_longlong(d2);
                            const int j = msite[t];
                            if (bits < near_bits || (bits == near_bits && j < near_id)) {
                                near_bits = bits;
                                near_id = j;
                            }
                        }
                    },
                    [&]() {});
        }
#pragma unroll
        for (int off = FS_LPS / 2; off >= 1; off >>= 1) {
            cnt += __shfl_xor(cnt, off, 64);
            wsum += __shfl_xor(wsum, off, 64);
#pragma unroll
            for (int q = 0; q < NF; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
            const u64 ob = __shfl_xor(near_bits, off, 64);
            const int oj = __shfl_xor(near_id, off, 64);
            // (the smaller d2; at equal d2 the smaller id -- -1, no member, only ever meets the bits of +infinity)
            if (ob < near_bits || (ob == near_bits && (unsigned)oj < (unsigned)near_id)) {
                near_bits = ob;
                near_id = oj;
            }
        }
        if (valid && lane == 0) {
            if (count_out) count_out[s] = cnt;
            if (nearest_out) nearest_out[s] = near_id;
            if (nearest_d2_out) nearest_d2_out[s] = __longlong_as_double((long long)near_bits);
            if (wsum_out) wsum_out[s] = wsum;
#pragma unroll
            for (int q = 0; q < NF; ++q)
                if (q < n_fields) out[(size_t)q * n_points + s] = normalize ? (wsum == 0.0 ? fill : acc[q] / wsum) : acc[q];
            n_empty += cnt == 0;
            n_visits += (u64)cnt;
            const u64 pack = ((u64)(unsigned)cnt << 32) | (0xffffffffu - (unsigned)s);
            best = pack > best ? pack : best;
        }
    }
    // the stats: once per wave
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        n_empty += __shfl_xor(n_empty, off, 64);
        n_visits += __shfl_xor(n_visits, off, 64);
        const u64 o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_empty) atomicAdd(stat + FS_EMPTY, n_empty);
        if (n_visits) atomicAdd(stat + FS_VISITS, n_visits);
        if (best) atomicMax(stat + FS_MAX, best);
    }
}

// scratch on the index, grown on demand and freed by kmcf_pairwise_destroy; it holds nothing a later call reads
int fs_workspace(kmcf_pairwise *p, int n_fields)
{
    if (!p->fs_ws) {
        kmcf_fs_ws *w = p->fs_ws = new kmcf_fs_ws();
        KMCF_TRY(kmcf_members_alloc(&w->m, p->N, 1, true));
        KMCF_TRY(kmcf_dev_alloc(&w->d_stat, (size_t)FS_STAT_WORDS, false));
    }
    kmcf_fs_ws *w = p->fs_ws;
    KMCF_TRY(kmcf_dev_grow(&w->d_mval, &w->cap_mval, (size_t)std::max(n_fields, 1) * (size_t)p->N, 0));
    return KMCF_OK;
}

struct fs_call {
    const char *what;
    const double *d_x, *d_y, *d_z;
    const int *d_site_mask;
    int n_fields;
    const double *d_values;
    int n_points;
    double radius;
    int normalize;
    double fill;
    double *d_out, *d_wsum;
    int *d_count, *d_nearest;
    double *d_nearest_d2;
    kmcf_sample_stats_t *stats;
};

// the argument checks both entry points share, in two halves around the checks of the points; p comes last: everything
// before it is checked without an index.  need_out: false with no point at all -- an array of no element may be NULL
int fs_check_sites(const fs_call &a, bool need_out)
{
    const char *what = a.what;
    KMCF_TRY(kmcf_check_coords(what, a.d_x, a.d_y, a.d_z));
    KMCF_CHECK(a.n_fields >= 0 && a.n_fields <= FS_MAX_FIELDS, KMCF_ERR_ARG, "%s: n_fields = %d is outside 0 ... %d", what, a.n_fields,
               FS_MAX_FIELDS);
    KMCF_CHECK(a.n_fields == 0 || a.d_values, KMCF_ERR_ARG, "%s: d_values is NULL with n_fields = %d", what, a.n_fields);
    KMCF_CHECK(a.n_fields == 0 || a.d_out || !need_out, KMCF_ERR_ARG, "%s: d_out is NULL with n_fields = %d", what, a.n_fields);
    KMCF_CHECK(a.n_fields > 0 || !a.d_values, KMCF_ERR_ARG, "%s: d_values is given with n_fields = 0", what);
    KMCF_CHECK(a.n_fields > 0 || !a.d_out, KMCF_ERR_ARG, "%s: d_out is given with n_fields = 0", what);
    return KMCF_OK;
}

int fs_check_rest(const fs_call &a, const kmcf_pairwise *p)
{
    const char *what = a.what;
    KMCF_TRY(kmcf_check_radius(what, "radius", a.radius));
    KMCF_CHECK(a.normalize == 0 || a.normalize == 1, KMCF_ERR_ARG, "%s: normalize = %d is neither 0 nor 1", what, a.normalize);
    KMCF_CHECK(a.d_out || a.d_wsum || a.d_count || a.d_nearest || a.d_nearest_d2 || a.stats, KMCF_ERR_ARG,
               "%s: every output is NULL and stats is NULL: nothing to compute", what);
    return kmcf_check_index(what, p, "radius", a.radius, nullptr);
}

template <class GRID, class POINTS>
void fs_launch_walk(const GRID &g, const POINTS &pts, kmcf_pairwise *p, const fs_call &a)
{
    kmcf_fs_ws *w = p->fs_ws;
    const int per_block = FS_PASSES * FS_SPB;
    const int grid = (int)(((int64_t)a.n_points + per_block - 1) / per_block);
    const double r2 = a.radius * a.radius;
    const auto go = [&](auto nf) {
        fs_walk_kernel<GRID, decltype(nf)::value, POINTS><<<grid, KMCF_BLOCK, 0, p->comm->stream>>>(
            g, pts, a.n_points, p->d_cell_start, w->m.d_pos, w->m.d_site, w->m.d_x, w->m.d_y, w->m.d_z, w->d_mval, p->N, a.n_fields,
            r2, a.normalize, a.fill, a.d_out, a.d_wsum, a.d_count, a.d_nearest, a.d_nearest_d2, w->d_stat);
    };
    if (a.n_fields == 0) go(std::integral_constant<int, 0>());
    else if (a.n_fields == 1) go(std::integral_constant<int, 1>());
    else if (a.n_fields == 2) go(std::integral_constant<int, 2>());
    else if (a.n_fields <= 4) go(std::integral_constant<int, 4>());
    else go(std::integral_constant<int, 8>());
}

// the body of both calls behind the checks of the points
template <class POINTS>
int fs_run(kmcf_pairwise *p, const fs_call &a, const POINTS &pts)
{
    KMCF_TRY(fs_check_rest(a, p));
    if (a.stats) *a.stats = kmcf_sample_stats_t{0, 0, 0, 0, 0, -1, 0.0f};
    if (a.n_points == 0) return KMCF_OK;
    kmcf_comm *c = p->comm;
    KMCF_TRY(kmcf_enter(c));
    KMCF_TRY(fs_workspace(p, a.n_fields));
    kmcf_fs_ws *w = p->fs_ws;
    hipStream_t st = c->stream;
    KMCF_HIP(hipEventRecord(c->ev_t0, st));
    KMCF_HIP(hipMemsetAsync(w->d_stat, 0, FS_BAD * sizeof(u64), st));
    KMCF_HIP(hipMemsetAsync(w->d_stat + FS_BAD, FS_NO_POINT & 0xff, sizeof(u64), st));
    kmcf_members_enqueue<1>(p, w->m, fs_rule{a.d_site_mask}, fs_emit{a.d_x, a.d_y, a.d_z, p->N, a.n_fields, a.d_values, w->m, w->d_mval});
    p->with_grid([&](auto g) { fs_launch_walk(g, pts, p, a); });
    KMCF_HIP(hipGetLastError());
    // the copies, the call's one synchronisation, and what the host forms
    int *h = c->h_pinned;
    KMCF_HIP(hipMemcpyAsync(h, w->d_stat, FS_STAT_WORDS * sizeof(u64), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipMemcpyAsync(h + 2 * FS_STAT_WORDS, w->m.d_sum + kmcf_member_tiles(p->N), sizeof(int), hipMemcpyDeviceToHost, st));   // members
    KMCF_HIP(hipEventRecord(c->ev_call1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    const auto word = [&](int k) { return ((u64)(unsigned)h[2 * k + 1] << 32) | (unsigned)h[2 * k]; };
    const int bad_nf = h[2 * FS_BAD], bad_far = h[2 * FS_BAD + 1];
    KMCF_CHECK(bad_nf == FS_NO_POINT, KMCF_ERR_ARG, "%s: point %d has a coordinate that is not finite", a.what, bad_nf);
    KMCF_CHECK(bad_far == FS_NO_POINT, KMCF_ERR_ARG,
               "%s: point %d lies further than %g periods from the periodic index's origin in y or z: wrap the points first", a.what,
               bad_far, FS_FAR_PERIODS);
    if (a.stats) {
        kmcf_sample_stats_t *s = a.stats;
        const u64 pack = word(FS_MAX);
        s->n_points = a.n_points;
        s->n_empty = (long long)word(FS_EMPTY);
        s->n_visits = (long long)word(FS_VISITS);
        s->n_members = h[2 * FS_STAT_WORDS];
        s->max_count = (int)(pack >> 32);
        s->max_count_point = (int)(0xffffffffu - (unsigned)(pack & 0xffffffffull));
        KMCF_HIP(hipEventElapsedTime(&s->ms, c->ev_t0, c->ev_call1));
    }
    return KMCF_OK;
}

}  // namespace

extern "C" int kmcf_field_sample(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z, const int *d_site_mask,
                                 int n_fields, const double *d_values, int n_points, const double *d_px, const double *d_py,
                                 const double *d_pz, double radius, int normalize, double fill, double *d_out, double *d_wsum,
                                 int *d_count, int *d_nearest, double *d_nearest_d2, kmcf_sample_stats_t *stats)
{
    const char *what = "kmcf_field_sample";
    const fs_call a{what, d_x, d_y, d_z, d_site_mask, n_fields, d_values, n_points, radius, normalize, fill, d_out, d_wsum, d_count,
                    d_nearest, d_nearest_d2, stats};
    KMCF_TRY(fs_check_sites(a, n_points != 0));
    KMCF_CHECK(n_points >= 0, KMCF_ERR_ARG, "%s: n_points = %d is negative", what, n_points);
    KMCF_CHECK(n_points == 0 || d_px, KMCF_ERR_ARG, "%s: d_px is NULL", what);
    KMCF_CHECK(n_points == 0 || d_py, KMCF_ERR_ARG, "%s: d_py is NULL", what);
    KMCF_CHECK(n_points == 0 || d_pz, KMCF_ERR_ARG, "%s: d_pz is NULL", what);
    return fs_run(p, a, fs_points_arrays{d_px, d_py, d_pz});
}

extern "C" int kmcf_field_grid(kmcf_pairwise *p, const double *d_x, const double *d_y, const double *d_z, const int *d_site_mask,
                               int n_fields, const double *d_values, const double *h_origin, const double *h_spacing,
                               const int *h_dims, double radius, int normalize, double fill, double *d_out, double *d_wsum,
                               int *d_count, int *d_nearest, double *d_nearest_d2, kmcf_sample_stats_t *stats)
{
    const char *what = "kmcf_field_grid";
    fs_call a{what, d_x, d_y, d_z, d_site_mask, n_fields, d_values, 0, radius, normalize, fill, d_out, d_wsum, d_count, d_nearest,
              d_nearest_d2, stats};
    KMCF_TRY(fs_check_sites(a, true));
    KMCF_CHECK(h_origin, KMCF_ERR_ARG, "%s: h_origin is NULL", what);
    KMCF_CHECK(h_spacing, KMCF_ERR_ARG, "%s: h_spacing is NULL", what);
    KMCF_CHECK(h_dims, KMCF_ERR_ARG, "%s: h_dims is NULL", what);
    int64_t n = 1;
    for (int k = 0; k < 3; ++k) {
        KMCF_CHECK(std::isfinite(h_origin[k]), KMCF_ERR_ARG, "%s: h_origin[%d] is not finite", what, k);
        KMCF_CHECK(std::isfinite(h_spacing[k]) && h_spacing[k] > 0.0, KMCF_ERR_ARG, "%s: h_spacing[%d] = %g is not finite and > 0", what,
                   k, h_spacing[k]);
        KMCF_CHECK(h_dims[k] >= 1, KMCF_ERR_ARG, "%s: h_dims[%d] = %d is not >= 1", what, k, h_dims[k]);
        n *= h_dims[k];                                       // (below 2^31 before the step: below 2^62 after it)
        KMCF_CHECK(n < ((int64_t)1 << 31), KMCF_ERR_ARG, "%s: the product of h_dims is 2^31 or more", what);
    }
    a.n_points = (int)n;
    return fs_run(p, a, fs_points_grid{h_origin[0], h_origin[1], h_origin[2], h_spacing[0], h_spacing[1], h_spacing[2], h_dims[1],
                                       h_dims[2]});
}
