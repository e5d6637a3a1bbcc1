// Host decisions of the T path's tunnel block (kmcf_tstate.hip): which storage form an assembly takes, and how the
// strips of the tiled forms are dealt to the ranks.  Pure functions: plain C++, no HIP header, nothing allocated beyond
// std::vector -- tests/subplan_check.cpp calls them with a synthetic amount of free memory.
//
// THE STORAGE RULE.  The block of n_t tunnel points is held as
//   bitmap  one 64-bit mask per 64 columns and row + the packed f64 values of the set positions (8 B/nnz + 1 bit per
//           position), rows sliced over the ranks;
//   dense   the upper block triangle as 64 x 64 tiles of f64 (kmcf_subop::dense), when the block has 2048 points or more
//           and is more than a QUARTER full.  In bytes the tiles (4 n^2) win from half full on (8 d n^2 + n^2 / 8 for the
//           bitmap form); in time from a quarter on: the tile kernel streams at 5.3 TB/s, the bitmap kernel -- a load of
//           64 x d values per mask word -- at 2.7 (the reference's contact window at 40 nm, 44 % full: 3.8 against 6.3 ms
//           per application).  Not when the tiles would take more than 60 % of the free device memory;
//   jagged  (round 4, one rank) the same tiles holding only their ENTRIES: 4 B per entry of the full block + 1 bit per
//           position, the same sums bit for bit, 2.2 x less memory at 44 % -- but bound by its instruction count, not its
//           bytes (the reference's window on the 4 x 4-cell device, 17 722 points, 44 % full: dense tiles 0.28, jagged
//           tiles 0.41, bitmap 0.49 ms per iteration): taken where the dense tiles do not fit the device's memory and
//           the jagged ones do.
// A rank GROUP (round 4) deals the dense tiles' strips to its ranks (kmcf_subop::spread) under the same rule, weighed
// on the whole block: the ranks agree through one small all-gather (entries of their rows, and whether their share of
// the tiles fits) so that all of them take the same branch.
// KMCF_SUB_DENSE = 0 bitmap / 1 dense tiles / 2 jagged tiles (one rank; a group: dense tiles) overrides the rule, not
// the limit of one p.Ap partial per block row (one rank) or per 256 own points (group).
//
// Free device memory comes from a callable `bool free_bytes(size_t *bytes)` (false: could not be read).  It is called
// at most once, and only where the answer can change the outcome: not when the capacity held already suffices, not when
// the rule says bitmap.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMCF_SUBPLAN_HD __host__ __device__ inline
#else
#define KMCF_SUBPLAN_HD inline
#endif

constexpr int KMCF_SUB_AUTO = INT_MIN;           // `override`: KMCF_SUB_DENSE is not set
constexpr int KMCF_SUB_MAX_PARTIALS = 2048;      // = KMCF_MAX_PARTIALS (kmcf_internal.hpp; asserted in kmcf_tstate.hip)
constexpr int KMCF_SUB_BLOCK = 256;              // = KMCF_BLOCK

// Tile (I, J), J >= I, of the upper block triangle: 64 x 64 f64, row-major, at tile index I nb - I (I - 1) / 2 + (J - I).
KMCF_SUBPLAN_HD long long symm_tile_index(int nb, int I, int J) { return (long long)I * nb - (long long)I * (I - 1) / 2 + (J - I); }

// ---------------------------------------------------------------- the strip deal
struct kmcf_strip { int I, J0, len, first; };    // block row, first block column, tiles, first tile index (uploaded as int4)

struct kmcf_strip_deal {
    std::vector<kmcf_strip> strips;              // this rank's, block rows ascending, then columns
    std::vector<int> first;                      // nb + 1: first of this rank's strips of every block row
    std::vector<int> tile_local;                 // spread: global tile index -> this rank's tile, -1: another rank's
    long long n_tiles = 0;                       // this rank's
};

// Strip after strip (block rows ascending, then columns; strip_len tiles, the last of a block row what is left) to the
// rank that holds the fewest tiles so far, the lowest such rank -- within a strip's length of even, whatever the mix of
// full and ragged strips.  A strip's tiles start at `first`: the global tile index (one rank: P = 1, not spread), or
// this rank's own running count (spread).
inline kmcf_strip_deal kmcf_deal_strips(int nb, int strip_len, int P, int rank, bool spread)
{
    kmcf_strip_deal d;
    d.first.assign((size_t)nb + 1, 0);
    if (spread) d.tile_local.assign((size_t)((long long)nb * (nb + 1) / 2), -1);
    std::vector<long long> held((size_t)P, 0);
    for (int I = 0; I < nb; ++I) {
        d.first[I] = (int)d.strips.size();
        for (int J = I; J < nb; J += strip_len) {
            const int len = std::min(strip_len, nb - J);
            const int owner = (int)(std::min_element(held.begin(), held.end()) - held.begin());
            held[owner] += len;
            if (owner != rank) continue;
            d.strips.push_back({I, J, len, (int)(spread ? d.n_tiles : symm_tile_index(nb, I, J))});
            if (spread)
                for (int q = 0; q < len; ++q) d.tile_local[(size_t)symm_tile_index(nb, I, J + q)] = (int)(d.n_tiles + q);
            d.n_tiles += len;
        }
    }
    d.first[nb] = (int)d.strips.size();
    return d;
}

// ---------------------------------------------------------------- the storage rule
struct kmcf_sub_form { bool dense, jagged; };    // neither: bitmap; jagged comes with dense set

// One rank: nnz entries among n_t points, cap_tiles doubles / cap_jval doubles already held for the two tile forms.
template <class Free>
kmcf_sub_form kmcf_sub_form_one_rank(int n_t, long long nnz, size_t cap_tiles, size_t cap_jval, int override, Free &&free_bytes)
{
    const long long nbl = (n_t + 63) / 64, all_tiles = nbl * (nbl + 1) / 2;
    const double nn2 = (double)n_t * (double)n_t, nbt = nn2 / 8192;
    kmcf_sub_form f{n_t >= 2048 && 4.0 * (double)nnz > nn2, false};
    if (f.dense && cap_tiles < (size_t)all_tiles * 4096) {
        size_t fr = 0;
        if (free_bytes(&fr) && 4.0 * nn2 + 1024.0 * nbt > 0.6 * (double)fr) {
            f.jagged = 4.0 * (double)nnz + 1544.0 * nbt <= 0.6 * (double)fr + 8.0 * (double)cap_jval;
            f.dense = f.jagged;
        }
    }
    if (override != KMCF_SUB_AUTO) { f.dense = override != 0; f.jagged = f.dense && override == 2; }
    if (nbl > KMCF_SUB_MAX_PARTIALS) f.dense = f.jagged = false;       // (one p.Ap partial per block row)
    return f;
}

// A group of P ranks, before the vote: does this rank's share of the dealt tiles fit (what it would hold: every P-th
// strip; 32 KB a tile + its parts)?  No vote is taken when the knob says bitmap.
enum kmcf_sub_vote { KMCF_SUB_NO_VOTE, KMCF_SUB_NO_FIT, KMCF_SUB_FITS };

template <class Free>
kmcf_sub_vote kmcf_sub_group_vote(int n_t, int P, size_t cap_tiles, int override, Free &&free_bytes)
{
    if (override == 0) return KMCF_SUB_NO_VOTE;
    const long long nbl = (n_t + 63) / 64, all_tiles = nbl * (nbl + 1) / 2;
    const double share = ((double)all_tiles / P + nbl) * (32768.0 + 1024.0);
    size_t fr = 0;
    const bool fits = cap_tiles * sizeof(double) >= share || (free_bytes(&fr) && share <= 0.6 * (double)fr);
    return fits ? KMCF_SUB_FITS : KMCF_SUB_NO_FIT;
}

// ... after it: nnz_all entries on all ranks, fit_all: every rank's share fits.  True: dense tiles, spread.  ns, the
// rank's OWN points (one p.Ap partial per 256 of them), is the one input on which the ranks of a group could in
// principle differ: 2048 x 256 points on one rank are beyond every block this path is built for, and the test stays.
inline bool kmcf_sub_group_spread(int n_t, int ns, double nnz_all, bool fit_all, int override)
{
    const double nn2 = (double)n_t * (double)n_t;
    return fit_all && (ns + KMCF_SUB_BLOCK - 1) / KMCF_SUB_BLOCK <= KMCF_SUB_MAX_PARTIALS &&
           (override != KMCF_SUB_AUTO ? override != 0 : n_t >= 2048 && 4.0 * nnz_all > nn2);
}
