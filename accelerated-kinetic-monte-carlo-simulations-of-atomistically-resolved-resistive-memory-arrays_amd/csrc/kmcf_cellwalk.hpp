// The walk over the spatial index of kmcf_compute_cutoff_list(_pbc) that the pairwise term (kmcf_pairwise.hip), the gap
// search (kmcf_gap.hip), the chain search (kmcf_chain.hip), the pair correlation (kmcf_paircorr.hip) and the field
// sampling (kmcf_fieldsample.hip) share.  Device only.  The list it walks is built by kmcf_cellmembers.hpp.
//
// A group of 16 lanes serves one member (a site) or sample point.  kmcf_walk_columns enumerates the columns (ax, ay) of
// the 27 index cells around it; the cells of a column that it reaches are one or two contiguous runs [b, e) of a list
// compacted in cell order (pos[] holds, per slot of the cell order, the list position).  Per column, in this order:
//   keep(bound)  bound = lx*lx + ly*ly, a lower bound of the squared (x, y) distance to every site of the column;
//                false: the column is skipped (z is not pruned)
//   run(b, e)    once per run, in ascending cell order; the caller strides its lanes over [b, e)
//   end()        the column is finished: the searches reduce over the group and lower their thresholds here
// The geometry is picked by the grid's type: kmcf_cell_grid (open) or kmcf_cell_grid_pbc (periodic in y and z).
//
// Invariant.  Column ranges, run bounds and bounds depend on the member alone, and whatever keep() compares them with must
// depend on the member alone too or be read by the group's first lane and broadcast: the 16 lanes of a group then take
// every branch of the walk together and reach every __shfl_xor in end() together.  Only the stride over a run is per lane.
#pragma once
#include "kmcf_cellmembers.hpp"

constexpr unsigned long long KMCF_D2_INF = 0x7ff0000000000000ull;      // bits of +infinity: no d2 seen
constexpr unsigned long long KMCF_NO_PAIR = ~0ull;                     // a packed pair: none

// Lower bound of |v_b - v| over the sites b of index cell column `a` next to the column `c` of v (a = c - 1 or c + 1):
// the distance to the face between them, shortened by far more than the cell rule can misplace a site (relative 1e-9).
__device__ __forceinline__ double kmcf_face_dist(double v, double v0, double edge, int c, int a)
{
    const double f = v0 + (double)(a > c ? c + 1 : c) * edge;
    const double d = (a > c ? f - v : v - f) - 1e-9 * (fabs(f) + fabs(v) + edge);
    return d > 0.0 ? d : 0.0;
}

// Lower bound of the minimum-image |v_b - v| over the sites b of a periodic index's cell next to the cell of v, through
// the face at f (lower: the face below v): the distance to that face, shortened by the relative 1e-9 of kmcf_face_dist,
// the period included in the scale -- the margin also covers the roundings of the cell rule and of fy * Ly in the distance.
__device__ __forceinline__ double kmcf_face_dist_pbc(double v, double f, bool lower, double edge, double period)
{
    const double d = (lower ? v - f : f - v) - 1e-9 * (fabs(f) + fabs(v) + edge + period);
    return d > 0.0 ? d : 0.0;
}

// Open index: x and y clipped to the grid; the cells (ax, ay, cz-1..cz+1) are contiguous in the cell order: one run.  A
// column whose run is empty ends without end(): nothing was found in it, so no threshold moves.
template <class KEEP, class RUN, class END>
__device__ __forceinline__ void kmcf_walk_columns(const kmcf_cell_grid &g, double xa, double ya, double za,
                                                  const int *__restrict__ cell_start, const int *__restrict__ pos, KEEP keep,
                                                  RUN run, END end)
{
    const int cx = kmcf_cell_coord(xa, g.x0, g.inv, g.ncx), cy = kmcf_cell_coord(ya, g.y0, g.inv, g.ncy),
              cz = kmcf_cell_coord(za, g.z0, g.inv, g.ncz);
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, g.ncx - 1); ++ax) {
        const double lx = ax == cx ? 0.0 : kmcf_face_dist(xa, g.x0, g.edge, cx, ax);
        for (int ay = max(cy - 1, 0); ay <= min(cy + 1, g.ncy - 1); ++ay) {
            const double ly = ay == cy ? 0.0 : kmcf_face_dist(ya, g.y0, g.edge, cy, ay);
            if (!keep(lx * lx + ly * ly)) continue;
            const int c_lo = (ax * g.ncy + ay) * g.ncz + max(cz - 1, 0);
            const int c_hi = (ax * g.ncy + ay) * g.ncz + min(cz + 1, g.ncz - 1);
            const int b = pos[cell_start[c_lo]], e = pos[cell_start[c_hi + 1]];
            if (b == e) continue;
            run(b, e);
            end();
        }
    }
}

// Periodic index: x as above; every wrapped cell once.  In y the distinct cells of {cy-1, cy, cy+1} mod ncy (one for
// ncy == 1, two for ncy == 2, else three); in z the cells {cz-1, cz, cz+1} mod ncz as runs of the compacted order -- the
// whole column when ncz <= 3, [cz-1, cz+1] inside, and [0, hi] + [lo, ncz-1] when cz sits on a face.
// Bound in y of a neighbour cell: ncy >= 3 -- the cell below (cy-1 mod ncy) is adjacent through the lower face of cy, the
// cell above through the upper face, and the way round the period is at least one cell edge longer than either; ncy == 2
// -- the other cell is adjacent through both faces: the smaller of the two; own cell (all there is for ncy == 1): 0.
template <class KEEP, class RUN, class END>
__device__ __forceinline__ void kmcf_walk_columns(const kmcf_cell_grid_pbc &g, double xa, double ya, double za,
                                                  const int *__restrict__ cell_start, const int *__restrict__ pos, KEEP keep,
                                                  RUN run, END end)
{
    const int ny = min(g.ncy, 3);               // y cells a member visits
    const double edge_y = g.ly / (double)g.ncy;
    const int cx = kmcf_cell_coord(xa, g.x0, g.inv_x, g.ncx), cy = kmcf_cell_coord(ya, g.y0, g.inv_y, g.ncy),
              cz = kmcf_cell_coord(za, g.z0, g.inv_z, g.ncz);
    // z runs [lo0, hi0] and, if n_runs == 2, [lo1, hi1]
    int n_runs = 1, lo0 = cz - 1, hi0 = cz + 1, lo1 = 0, hi1 = -1;
    if (g.ncz <= 3) { lo0 = 0; hi0 = g.ncz - 1; }
    else if (cz == 0) { lo0 = 0; hi0 = 1; lo1 = hi1 = g.ncz - 1; n_runs = 2; }
    else if (cz == g.ncz - 1) { lo0 = 0; hi0 = 0; lo1 = g.ncz - 2; hi1 = g.ncz - 1; n_runs = 2; }
    const int ay0 = g.ncy == 1 ? cy : cy - 1 + g.ncy;
    // the faces of the member's cell in y
    const double below = kmcf_face_dist_pbc(ya, g.y0 + (double)cy * edge_y, true, edge_y, g.ly);
    const double above = kmcf_face_dist_pbc(ya, g.y0 + (double)(cy + 1) * edge_y, false, edge_y, g.ly);
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, g.ncx - 1); ++ax) {
        const double lx = ax == cx ? 0.0 : kmcf_face_dist(xa, g.x0, g.edge_x, cx, ax);
        for (int sy = 0; sy < ny; ++sy) {
            const int ay = (ay0 + sy) % g.ncy;
            const double ly = ay == cy ? 0.0 : (g.ncy == 2 ? fmin(below, above) : (sy == 0 ? below : above));
            if (!keep(lx * lx + ly * ly)) continue;
            const int col = (ax * g.ncy + ay) * g.ncz;
            for (int r = 0; r < n_runs; ++r)
                run(pos[cell_start[col + (r ? lo1 : lo0)]], pos[cell_start[col + (r ? hi1 : hi0) + 1]]);
            end();
        }
    }
}

// The squared distance of the gap and chain searches from the member a to a candidate b.  Open: the plain difference.
// Periodic: the minimum image in y and z (kmcf_min_image_dist's arithmetic, squared); a pair has ONE distance, however
// many of its images lie within reach.  Both are odd in the difference up to the squares, so both ends of a pair compute
// the same bits: the chain search relies on that to see a mutual choice as one.
__device__ __forceinline__ double kmcf_walk_d2(const kmcf_cell_grid &, double xa, double ya, double za, double xb, double yb,
                                               double zb)
{
    const double dx = xa - xb, dy = ya - yb, dz = za - zb;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ double kmcf_walk_d2(const kmcf_cell_grid_pbc &g, double xa, double ya, double za, double xb,
                                               double yb, double zb)
{
    const double dx = xa - xb, dy = kmcf_min_image(ya - yb, g.ly), dz = kmcf_min_image(za - zb, g.lz);
    return (dx * dx + dy * dy) + dz * dz;
}
