// Block-wide primitives of the 256-thread (4 wavefront) kernels: the deterministic sum and maximum of a double, the
// exclusive scan of an int, and the flag / scan / scatter compaction built on it.  Included by kmcf_internal.hpp for
// device code.  The library is built without relocatable device code: everything here is forceinline, a template or in
// an anonymous namespace, so each translation unit gets its own instance.  New passes use these; they do not copy them.
#pragma once

// Sum of one double per thread; every thread gets it.  Fixed order: the xor butterfly inside each wavefront
// (kmcf_wave_sum64), then (w0 + w1) + (w2 + w3) -- what the device-order restatements of the tests add.
__device__ __forceinline__ double kmcf_block_sum(double v, double *lds4)
{
    v = kmcf_wave_sum64(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
    __syncthreads();
    return t;
}

__device__ __forceinline__ double kmcf_block_max(double v, double *lds4)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = fmax(fmax(lds4[0], lds4[1]), fmax(lds4[2], lds4[3]));
    __syncthreads();
    return t;
}

// Exclusive scan of one int per thread; *total (if given) receives the block's sum in every thread.
__device__ __forceinline__ int kmcf_block_excl_scan(int v, int *lds4, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int s = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        int t = __shfl_up(s, off, 64);
        if (lane >= off) s += t;
    }
    if (lane == 63) lds4[w] = s;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < w; ++i) base += lds4[i];
    if (total) *total = lds4[0] + lds4[1] + lds4[2] + lds4[3];
    __syncthreads();
    return base + s - v;
}

// ---------------------------------------------------------------- compaction: flag count / scan / scatter
// The input is cut into tiles of KMCF_SCAN_TILE items, one block per tile, KMCF_SCAN_ITEMS consecutive items per thread.
//   count kernel:    kmcf_tile_flags, kmcf_tile_count           -> counts[tile]
//   scan:            kmcf_scan_counts_kernel                    -> offsets[tile], total in offsets[tiles]
//   scatter kernel:  kmcf_tile_flags again, kmcf_tile_pos       -> where the thread's first flagged item goes; the kernel
//                    walks its items in order and advances the position by one per flagged item
// Output order = input order.  A flag word may carry several sets as bits (the gap pass: A and B); count and position
// take the set's mask, one call per set.
constexpr int KMCF_SCAN_ITEMS = 8, KMCF_SCAN_TILE = KMCF_BLOCK * KMCF_SCAN_ITEMS;

// first item of this thread in tile blockIdx.x
__device__ __forceinline__ int kmcf_tile_item0() { return blockIdx.x * KMCF_SCAN_TILE + threadIdx.x * KMCF_SCAN_ITEMS; }

// f[k] = rule(item) for the thread's items below n (ascending; rule may have side effects), 0 for the others
template <class F>
__device__ __forceinline__ void kmcf_tile_flags(int n, int (&f)[KMCF_SCAN_ITEMS], F rule)
{
    const int t0 = kmcf_tile_item0();
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k) f[k] = t0 + k < n ? (int)rule(t0 + k) : 0;
}

__device__ __forceinline__ int kmcf_flagged(const int (&f)[KMCF_SCAN_ITEMS], int mask)
{
    int c = 0;
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k) c += (f[k] & mask) != 0;
    return c;
}

// the tile's number of flagged items (every thread gets it)
__device__ __forceinline__ int kmcf_tile_count(const int (&f)[KMCF_SCAN_ITEMS], int *lds4, int mask = ~0)
{
    int total;
    kmcf_block_excl_scan(kmcf_flagged(f, mask), lds4, &total);
    return total;
}

// output position of this thread's first flagged item; tile_off: the scanned count of its tile
__device__ __forceinline__ int kmcf_tile_pos(const int (&f)[KMCF_SCAN_ITEMS], int tile_off, int *lds4, int mask = ~0)
{
    return tile_off + kmcf_block_excl_scan(kmcf_flagged(f, mask), lds4, nullptr);
}

namespace {

// Exclusive scan of n counts, total into out[n] (n + 1 entries).  One block per independent array: block b works on
// in + b * stride and out + b * stride.  Passes of 256 counts with a carry; the counts of one pass must add up inside an
// int, the carry is a T.  out == in (in place) is allowed when T is int.
template <typename T>
__global__ __launch_bounds__(KMCF_BLOCK) void kmcf_scan_counts_kernel(int n, const int *in, T *out, int stride)
{
    __shared__ int lds4[4];
    __shared__ T carry;
    in += (size_t)blockIdx.x * stride;
    out += (size_t)blockIdx.x * stride;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int b0 = 0; b0 < n; b0 += KMCF_BLOCK) {
        const int b = b0 + threadIdx.x;
        const int v = b < n ? in[b] : 0;
        int total;
        const int ex = kmcf_block_excl_scan(v, lds4, &total);
        if (b < n) out[b] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) out[n] = carry;
}

}  // namespace
