// T path: the current solve of DeviceKMC (Kirchhoff matrix over the atoms + two virtual nodes, WKB
// tunnelling sub-block), SURVEY.md 8 rows a14 / f3.  PARITY UNPINNED by any reference fixture.
//
// Reference -> here:
//   initialize_sparsity_T: O(n_loc * Nsub) distance scans per column block
//   (src/initialize_sparsity_T.cu:10-209, 948-1154)            -> cell list, once per bias point.
//   update_atom_arrays: 7 thrust::copy_if per step (src/current_solver_gpu.cu:1341-1365)
//                                                             -> the atom set is invariant under KMC events
//       (O <-> V, d <-> Od): site indices kept from init, one gather kernel per step, invariance checked.
//   populate_T_dist per block + calc_diagonal_T per block + insert_diag_T (:1051-1321)
//                                                             -> ONE kernel, 16 lanes per row, integer row sums;
//       the off-diagonals are -high_G / -low_G / -loop_G, so the coded window SpMV applies (2 B/nnz); the two
//       virtual-node rows (one entry per contact atom of a layer) are "long rows" (kmcf_internal.hpp).
//   assemble_sparse_T_submatrix: pattern by a thread per row scanning all columns twice, csr2coo, values by a
//   thread per entry with four-fold indirection, rebuilt and re-allocated every step (:707-946)
//                                                             -> the block is dense-ish (36 % at 5 nm, 43 % in the
//       authors' test set), so it is kept as a BITMAP (one 64-bit mask per 64 columns and row, found by a wave
//       per row with one ballot per 64 pairs) + packed f64 values: 8 B/nnz + 1 bit per position instead of the
//       12 B/nnz of CSR; buffers grow only.
//   spmm_split_sparse1: pack, size-1 Isend/Irecv ring of the sub-vector, neighbour SpMV, rocsparse_spmv of the
//   sub-block, unpack_add (dist_iterative/dist_spmv_split_sparse.cpp:5-78)
//                                                             -> pack, all-gather, neighbour SpMV, one bitmap kernel
//       (wave per row, coalesced value stream, x_sub from L2) adding into Ap and into the p.Ap partials.
//
// Shared device pieces (every kernel outside the solve's own -- sub_spmv, sub_symm, sub_symj and their helpers -- is built
// from them):
//   t_points, t_wkb, pair_value   the tunnel points and WKB parameters by value; THE value of one tunnel pair
//   neighbour_walk<LPR>           LPR lanes per internal row of T over the row's off-diagonal entries, butterfly, lane-0 finish
//   bitmap_rows, bitmap_row       a wave per local row of the pair bitmap; (column, packed offset) of every set position
//   profile_add_pair              one counted pair into the sums of the current profile, neighbour and tunnel part alike
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "kmcf_cells.hpp"
#include "kmcf_internal.hpp"
#include "kmcf_subplan.hpp"

static_assert(KMCF_SUB_MAX_PARTIALS == KMCF_MAX_PARTIALS && KMCF_SUB_BLOCK == KMCF_BLOCK, "kmcf_subplan.hpp restates the two constants");
static_assert(sizeof(kmcf_strip) == sizeof(int4), "a strip is uploaded as is to kmcf_subop::d_strips");

// the read-backs of an assembly and of the power pass, in pinned memory
struct t_pinned {
    int n_t, err;          // tunnel points of all ranks; the atom set differs from the one at init
    long long nnz;         // entries of this rank's rows of the tunnel block
    double imacro;
    long long jnnz;        // entries stored by the jagged tiles
};

struct kmcf_tstate {
    kmcf_comm *comm = nullptr;
    kmcf_matrix *T = nullptr;
    int N = 0, N_atom = 0, Nsub = 0, n_inj = 0, n_ext = 0, n_layers = 0;
    double nn_dist = 0.0;
    int pbc = 0;                                   // 1: every distance of the state is the minimum image in y and z
    double lattice[3] = {0.0, 0.0, 0.0};           // the caller's h_lattice (kmcf_initialize_sparsity_T_pbc, pbc == 1), else zeros
    std::vector<int> h_atom_site;
    std::vector<int> h_row_ptr, h_col;             // pattern of this rank, global columns, caller row order
    std::vector<int> h_inv_perm;                   // caller local row -> internal row
    // per atom (device)
    int *d_atom_site = nullptr;
    unsigned char *d_site_is_atom = nullptr;       // N: the atom set at init (invariance check)
    double *d_ax = nullptr, *d_ay = nullptr, *d_az = nullptr, *d_acb = nullptr;
    int *d_ael = nullptr, *d_ach = nullptr;
    unsigned char *d_acls = nullptr;               // bit0 metal, bit1 uncharged vacancy
    // per internal row / column of T
    unsigned char *d_cls_col = nullptr;            // 0x80 | node for the virtual nodes, else the atom's class
    int *d_col_node = nullptr;                     // global node of every internal column (own rows | halo slots)
    int *d_diag_pos = nullptr;
    unsigned char *d_ground = nullptr;             // row's atom neighbours the last atom (the cut ground node)
    int *d_inv_perm = nullptr;
    double *d_diag = nullptr, *d_diag_tot = nullptr, *d_rhs = nullptr;
    // tunnel points (all ranks' points on every rank: site arrays are replicated)
    int *d_blk = nullptr, *d_tidx = nullptr, *d_tinfo = nullptr;
    double *d_tx = nullptr, *d_ty = nullptr, *d_tz = nullptr, *d_tcb = nullptr;
    int *d_rowcnt = nullptr;
    double *d_tdiag = nullptr;
    size_t cap_rowcnt = 0, cap_tdiag = 0;
    std::vector<int> h_tidx;
    kmcf_subop sub;
    // post-processing
    double *d_pdisp = nullptr;                     // Nsub
    double *d_scal = nullptr;                      // [0] imacro, [1] min
    int *d_err = nullptr;
    t_pinned *h_pin = nullptr;
    double *d_agree = nullptr, *h_agree = nullptr; // storage vote of a rank group: 2 P on the device; pinned 2 + 2 P
    bool assembled = false;
    kmcf_current_params_t par{};
    // kmcf_current_map: scratch only (allocated with the state; nothing in it outlives a call)
    double *d_cmap = nullptr;                      // 3 (Nsub + 2): per node sum |I|, tunnel sum |I|, sum I, interleaved
    double *d_cmstat = nullptr, *h_cmstat = nullptr;   // 8 doubles on the device / pinned: the statistics
    std::vector<int> cm_counts, cm_displs;         // 3 x the matrix's row partition (the all-gather of d_cmap)
    // kmcf_current_profile: scratch only, like the current map's
    double *d_cprof = nullptr;                     // CP_STRIDE (Nsub + 2): the per-node sums (nullptr: too many atoms for int32 counts)
    int *d_cpq = nullptr, *d_cpcell = nullptr;     // N_atom each: slab and cell of every atom
    double *d_cpplanes = nullptr, *h_cpplanes = nullptr;   // 1024 planes on the device / pinned (staging of h_plane_x)
    double *d_cpout = nullptr, *h_cpout = nullptr; // the profile + 8 statistics on the device / pinned; grown at the start of a call
    size_t cap_cpout = 0;
    double *d_cppart = nullptr;                    // the segments' slab sums of the binning; grown like d_cpout
    size_t cap_cppart = 0;
    std::vector<void *> cp_retired_dev, cp_retired_host;   // outgrown d_cpout / h_cpout: freed with the state, never inside a call
    std::vector<int> cp_counts, cp_displs;         // CP_STRIDE x the row partition
};

namespace {

constexpr int EL_DEFECT = 0, EL_OXYGEN_DEFECT = 1, EL_VACANCY = 2, EL_TI = 6, EL_N = 8;   // src/utils.h:37-44
constexpr double H_BAR = 1.054571817e-34;        // src/initialize_sparsity_T.cu:6
constexpr double EV_TO_J = 1.60217663e-19;       // :5
constexpr int CODE_HIGH = 0, CODE_LOW = 1, CODE_LOOP = 2;

__device__ __forceinline__ bool in_metals(const int *__restrict__ metals, int nm, int e)
{
    for (int k = 0; k < nm; ++k)
        if (metals[k] == e) return true;
    return false;
}

__device__ __forceinline__ double dist3(double x1, double y1, double z1, double x2, double y2, double z2)
{   // site_dist_gpu, 6-argument overload (src/gpu_solvers.h:280-285)
    const double dx = x2 - x1, dy = y2 - y1, dz = z2 - z1;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// The distance of a pair of tunnel points, chosen at compile time: a kernel that measures a pair is instantiated once per
// geometry and takes the functor by value.  dist_open is empty and calls dist3: the open instantiation is the code it was.
// dist_min_image carries the periods of kmcf_initialize_sparsity_T_pbc and calls the library's one minimum image
// (kmcf_internal.hpp).  (Why d(i, j) and d(j, i) must be the same bits: at pair_value, the one place that measures a pair.)
struct dist_open {
    __device__ __forceinline__ double operator()(double x1, double y1, double z1, double x2, double y2, double z2) const
    {
        return dist3(x1, y1, z1, x2, y2, z2);
    }
};
struct dist_min_image {
    double ly, lz;
    __device__ __forceinline__ double operator()(double x1, double y1, double z1, double x2, double y2, double z2) const
    {
        return kmcf_min_image_dist(x1, y1, z1, x2, y2, z2, ly, lz);
    }
};

// ---------------------------------------------------------------- atoms
__global__ __launch_bounds__(KMCF_BLOCK) void gather_coords_kernel(int n, const int *__restrict__ site, const double *__restrict__ sx,
                                                                   const double *__restrict__ sy, const double *__restrict__ sz,
                                                                   double *__restrict__ ax, double *__restrict__ ay, double *__restrict__ az)
{
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n; a += gridDim.x * blockDim.x) {
        const int s = site[a];
        ax[a] = sx[s]; ay[a] = sy[s]; az[a] = sz[s];
    }
}

// is_defect filter (src/gpu_solvers.h:331-337) against the set found at init
__global__ __launch_bounds__(KMCF_BLOCK) void check_atom_set_kernel(int N, const int *__restrict__ element,
                                                                    const unsigned char *__restrict__ is_atom, int *__restrict__ err)
{
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) {
        const int e = element[s];
        const bool atom = (e != EL_DEFECT) && (e != EL_OXYGEN_DEFECT);
        if (atom != (is_atom[s] != 0)) *err = 1;
    }
}

__global__ __launch_bounds__(KMCF_BLOCK) void gather_atoms_kernel(int n, const int *__restrict__ site, const int *__restrict__ element,
                                                                  const int *__restrict__ charge, const double *__restrict__ cb,
                                                                  const int *__restrict__ metals, int nm, int *__restrict__ ael,
                                                                  int *__restrict__ ach, double *__restrict__ acb,
                                                                  unsigned char *__restrict__ acls)
{
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n; a += gridDim.x * blockDim.x) {
        const int s = site[a];
        const int e = element[s], q = charge[s];
        ael[a] = e; ach[a] = q; acb[a] = cb[s];
        unsigned char c = in_metals(metals, nm, e) ? 1 : 0;
        if (e == EL_VACANCY && q == 0) c |= 2;                 // conductive vacancy (:1231-1232)
        acls[a] = c;
    }
}

__global__ __launch_bounds__(KMCF_BLOCK) void t_cls_col_kernel(int n_cols, const int *__restrict__ col_node,
                                                               const unsigned char *__restrict__ acls, unsigned char *__restrict__ cls_col)
{
    for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += gridDim.x * blockDim.x) {
        const int node = col_node[c];
        cls_col[c] = node < 2 ? (unsigned char)(0x80 | node) : acls[node - 2];
    }
}

// ---------------------------------------------------------------- the walk of the neighbour rows of T
// LPR lanes per internal row r, a block taking whole groups of KMCF_BLOCK / LPR rows (grid: kmcf_grid1d(n_loc * LPR)).  Per
// row: start(r) loads what the row needs and says whether its entries are walked at all; entry(j, acc) for the positions j
// of row_ptr[r] .. row_ptr[r + 1] but the diagonal's, lane l taking l, l + LPR, ... in ascending order and adding into its
// NACC accumulators; an xor butterfly over the row's lanes; finish(r, dpos, acc) on the row's lane 0.  The kernels keep
// what start found for entry and finish in locals of their own.
template <int LPR, typename ACC, int NACC, typename START, typename ENTRY, typename FINISH>
__device__ __forceinline__ void neighbour_walk(int n_loc, const int *__restrict__ row_ptr, const int *__restrict__ diag_pos, START start,
                                               ENTRY entry, FINISH finish)
{
    constexpr int RPB = KMCF_BLOCK / LPR;
    const int lane = threadIdx.x % LPR;
    const int groups = (n_loc + RPB - 1) / RPB;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
        const int r = grp * RPB + threadIdx.x / LPR;
        const bool valid = r < n_loc;
        ACC acc[NACC] = {};
        int dpos = -1;
        if (valid && start(r)) {
            dpos = diag_pos[r];
            for (int j = row_ptr[r] + lane; j < row_ptr[r + 1]; j += LPR)
                if (j != dpos) entry(j, acc);
        }
#pragma unroll
        for (int off = LPR / 2; off >= 1; off >>= 1) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) acc[k] += __shfl_xor(acc[k], off, 64);
        }
        if (valid && lane == 0) finish(r, dpos, acc);
    }
}

// ---------------------------------------------------------------- neighbour values
// populate_T_dist (src/current_solver_gpu.cu:1051-1247) + calc_diagonal_T + insert_diag_T (:1279-1321), one
// pass, LPR lanes per row.  Entry rule by the classes of row and column node:
//   virtual row, virtual column (0,1)/(1,0): -loop_G;  virtual row, atom column: -high_G (:1082-1090, :1097-1106)
//   atom row, virtual column: -high_G (:1126-1136);  atom-atom neighbours: -high_G if both metal or both
//   uncharged vacancies, else -low_G (:1224-1241).
// Diagonal = start value + sum of the row's conductances: the start value is what populate_T_dist leaves in the
// diagonal slot -- +high_G in row 0 (:1077-1080) and in rows of atoms that neighbour the cut ground atom
// (:1113-1123), 0 in row 1 and elsewhere.  Row sums from integer counts (order independent).
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void t_assemble_kernel(
    int n_loc, const int *__restrict__ row_ptr, const int *__restrict__ col, double *__restrict__ val,
    const int *__restrict__ diag_pos, const unsigned char *__restrict__ ground, const unsigned char *__restrict__ cls_col,
    double high_G, double low_G, double loop_G, double *__restrict__ diag_out,
    unsigned short *__restrict__ idx16 /* value codes above the slot bits (rows < n_coded), or nullptr */,
    double *__restrict__ diagv, int n_coded)
{
    constexpr int SLOT_MASK = (1 << KMCF_SLOT_BITS) - 1;
    unsigned char ci = 0;
    bool coded = false;
    neighbour_walk<LPR, int, 3>(
        n_loc, row_ptr, diag_pos,
        [&](int r) { ci = cls_col[r]; coded = idx16 && r < n_coded; return true; },
        [&](int j, int *n /* entries of value code CODE_HIGH, CODE_LOW, CODE_LOOP */) {
            // (read here, not where they are chosen: a choice among three captured references becomes ONE load at an index
            // into the closure, which then cannot leave memory -- 32 bytes of scratch a lane)
            const double g_high = -high_G, g_low = -low_G, g_loop = -loop_G;
            const unsigned char cj = cls_col[col[j]];
            int code;
            if (ci & 0x80) code = (cj & 0x80) ? CODE_LOOP : CODE_HIGH;
            else if (cj & 0x80) code = CODE_HIGH;
            else code = (ci & cj & 3) ? CODE_HIGH : CODE_LOW;
            val[j] = code == CODE_HIGH ? g_high : (code == CODE_LOW ? g_low : g_loop);
            if (coded) idx16[j] = (unsigned short)((idx16[j] & SLOT_MASK) | (code << KMCF_SLOT_BITS));
            n[CODE_HIGH] += code == CODE_HIGH; n[CODE_LOW] += code == CODE_LOW; n[CODE_LOOP] += code == CODE_LOOP;
        },
        [&](int r, int dpos, const int *n) {
            double d0 = 0.0;
            if (ci == 0x80) d0 = high_G;
            else if (!(ci & 0x80) && ground[r]) d0 = high_G;
            const double off = (double)n[CODE_HIGH] * high_G + (double)n[CODE_LOW] * low_G + (double)n[CODE_LOOP] * loop_G;
            const double d = d0 + off;
            if (dpos >= 0) {
                val[dpos] = d;
                if (coded) idx16[dpos] = (unsigned short)((idx16[dpos] & SLOT_MASK) | (KMCF_CODE_DIAG << KMCF_SLOT_BITS));
            }
            if (diagv && r < n_coded) diagv[r] = dpos >= 0 ? d : 0.0;
            diag_out[r] = d;
        });
}

// ---------------------------------------------------------------- tunnel points
// get_is_tunnel_mpi (src/initialize_sparsity_T.cu:618-654) over the atoms 0 .. N_atom - 2 of all ranks; the
// reference's yes * idx / copy_if(is_not_zero) drops atom 0, restated as "atom 0 is never a tunnel point".
// The list is compacted with the tiles of kmcf_block.hpp (2048 atoms per block): count, scan, scatter.
__device__ __forceinline__ int tunnel_flag(int a, int n_scan, const int *__restrict__ ael, const double *__restrict__ ax,
                                           double x_lo, double x_hi)
{
    if (a < 1 || a >= n_scan) return 0;
    const int e = ael[a];
    return (e == EL_VACANCY || ((e == EL_TI || e == EL_N) && (ax[a] > x_lo && ax[a] < x_hi))) ? 1 : 0;
}

__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_count_kernel(int n_scan, const int *__restrict__ ael, const double *__restrict__ ax,
                                                                  double x_lo, double x_hi, int *__restrict__ blk)
{
    __shared__ int lds4[4];
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(n_scan, f, [&](int a) { return tunnel_flag(a, n_scan, ael, ax, x_lo, x_hi); });
    const int total = kmcf_tile_count(f, lds4);
    if (threadIdx.x == 0) blk[blockIdx.x] = total;
}

// scatter: tunnel point list (ascending atom index) + compact per-point data
// info: bit0 vacancy, bit1 "metal_p" (a metal outside the outer contact layers,
// src/initialize_sparsity_T.cu:267-273; num_metals hard-coded to 2 at :800 -- the caller's list is used)
__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_scatter_kernel(
    int n_scan, int N_atom, const int *__restrict__ ael, const double *__restrict__ ax, const double *__restrict__ ay,
    const double *__restrict__ az, const double *__restrict__ acb, const int *__restrict__ metals, int nm,
    double x_lo, double x_hi, int n_layers, int n_inj, int n_ext, const int *__restrict__ blk_off,
    int *__restrict__ tidx, int *__restrict__ tinfo, double *__restrict__ tx, double *__restrict__ ty,
    double *__restrict__ tz, double *__restrict__ tcb)
{
    __shared__ int lds4[4];
    const int base = kmcf_tile_item0();
    int f[KMCF_SCAN_ITEMS];
    kmcf_tile_flags(n_scan, f, [&](int a) { return tunnel_flag(a, n_scan, ael, ax, x_lo, x_hi); });
    int pos = kmcf_tile_pos(f, blk_off[blockIdx.x], lds4);
#pragma unroll
    for (int k = 0; k < KMCF_SCAN_ITEMS; ++k) {
        if (!f[k]) continue;
        const int a = base + k;
        const int e = ael[a];
        int info = (e == EL_VACANCY) ? 1 : 0;
        if (in_metals(metals, nm, e) && (a > (n_layers - 1) * n_inj) && (a < (N_atom - (n_layers - 1) * n_ext))) info |= 2;
        tidx[pos] = a; tinfo[pos] = info;
        tx[pos] = ax[a]; ty[pos] = ay[a]; tz[pos] = az[a]; tcb[pos] = acb[a];
        ++pos;
    }
}

// pair rule of the tunnel pattern (src/initialize_sparsity_T.cu:261-284)
__device__ __forceinline__ bool tunnel_pair(int info_i, int info_j, double cb_i, double cb_j, double tol, bool *c2t)
{
    const bool v1 = info_i & 1, v2 = info_j & 1, m1 = info_i & 2, m2 = info_j & 2;
    const bool t2t = v1 && v2, ct = (v1 && m2) || (v2 && m1), cc = m1 && m2;
    *c2t = ct;
    return (t2t || ct || cc) && (fabs(cb_i - cb_j) > tol);
}

// The tunnel points and the WKB parameters of a state as the kernels take them: by value (points_of / wkb_of fill them;
// a kernel reads the members it needs).  t_point: one point's five values in registers.
struct t_points { const int *info; const double *x, *y, *z, *cb; };
struct t_wkb { double nn_dist, tol, m_e, V0; };
struct t_point { int info; double x, y, z, cb; };

__device__ __forceinline__ t_point load_point(const t_points &P, int i) { return {P.info[i], P.x[i], P.y[i], P.z[i], P.cb[i]}; }

// One wave per local sub row: masks of its row (one ballot per 64 columns) and its entry count
// (calc_nnz_per_row_tunnel + assemble_tunnel_col_indices, :212-372).
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_mask_kernel(int n_loc, int s0, int n_glob, int n_groups, t_points P, t_wkb w,
                                                                 unsigned long long *__restrict__ mask, int *__restrict__ rowcnt, DIST dist)
{
    const int lane = threadIdx.x & 63;
    const int wpb = KMCF_BLOCK / 64;
    for (int s = blockIdx.x * wpb + (threadIdx.x >> 6); s < n_loc; s += gridDim.x * wpb) {
        const int sg = s0 + s;
        const double xi = P.x[sg], yi = P.y[sg], zi = P.z[sg], cbi = P.cb[sg];
        const int fi = P.info[sg];
        int cnt = 0;
        for (int g = 0; g < n_groups; ++g) {
            const int j = g * 64 + lane;
            bool take = false;
            if (j < n_glob) {
                if (j == sg) take = true;                                           // :255-258 diagonal
                else {
                    bool c2t;
                    const double d = dist(xi, yi, zi, P.x[j], P.y[j], P.z[j]);
                    take = d > w.nn_dist && tunnel_pair(fi, P.info[j], cbi, P.cb[j], w.tol, &c2t);   // :261-284
                }
            }
            const unsigned long long mk = __ballot(take);
            if (lane == 0) mask[(size_t)s * n_groups + g] = mk;
            cnt += __popcll(mk);
        }
        if (lane == 0) rowcnt[s] = cnt;
    }
}

// WKB value of an entry (populate_T_tunnel_dist2, src/initialize_sparsity_T.cu:539-611)
__device__ __forceinline__ double wkb_value(double dist_angstrom, double cb_i, double cb_j, bool c2t, double m_e, double V0)
{
    const double local_E_drop = cb_i - cb_j;
    const double prefac = -(sqrt(2 * m_e) / H_BAR) * (2.0 / 3.0);
    const double dist = (1e-10) * dist_angstrom;
    if (c2t) {
        const double energy_window = fabs(local_E_drop);
        const double dV = 0.01;
        const double dE = EV_TO_J * dV * 10000000000;      // :572: the loop below runs once for any physical window
        double T = 0.0;
        for (double iv = 0; iv < energy_window; iv += dE) {
            const double E1 = EV_TO_J * V0 + iv;
            const double E2 = E1 - fabs(local_E_drop);
            if (E2 > 0) T += exp(prefac * (dist / fabs(local_E_drop)) * (pow(E1, 1.5) - pow(E2, 1.5)));
            if (E2 < 0) T += exp(prefac * (dist / fabs(local_E_drop)) * (pow(E1, 1.5)));
        }
        return -T;
    }
    const double E1 = EV_TO_J * V0;
    const double E2 = E1 - fabs(local_E_drop);
    if (E2 > 0) return -exp(prefac * (dist / fabs(E1 - E2)) * (pow(E1, 1.5) - pow(E2, 1.5)));
    if (E2 < 0) return -exp(prefac * (dist / fabs(E1 - E2)) * (pow(E1, 1.5)));
    return 0.0;      // E2 == 0: written by neither branch there (uninitialised memory, :881)
}

// THE value of the tunnel pair (a, b), a the row's point: every kernel that needs one calls this, so the storage forms,
// the current map and the current profile hold the same bits because they run the same expression.  The mirrored tiles,
// and the bitmap where each row measures the pair itself, also need v(a, b) == v(b, a): DIST's expression (dist3, the
// library's minimum image) is odd in every difference up to the squares, so d(a, b) and d(b, a) are the same bits.
// IN_PATTERN: for a fill that finds the pattern itself -- 0.0 unless the pair is an entry (the rule of tunnel_mask_kernel).
template <bool IN_PATTERN, typename DIST>
__device__ __forceinline__ double pair_value(const t_point &a, const t_point &b, const t_wkb &w, const DIST &dist)
{
    bool c2t;
    const bool rule = tunnel_pair(a.info, b.info, a.cb, b.cb, w.tol, &c2t);
    const double d = dist(a.x, a.y, a.z, b.x, b.y, b.z);
    if (IN_PATTERN && !(d > w.nn_dist && rule)) return 0.0;
    return wkb_value(d, a.cb, b.cb, c2t, w.m_e, w.V0);
}

// ---------------------------------------------------------------- the walk of the rows of the pair bitmap
// One wave per local row s (grid: wave_row_grid(n_loc)): row(s).  Inside it bitmap_row(the row's mask words, n_groups,
// off, body) calls body(j, pos) on the lane of every set column j = 64 g + lane, mask words in ascending order, all-zero
// words skipped wave-uniformly; pos = off + the set positions before j: with off = voff[s] the entry's place in the packed
// value stream (a body that ignores pos passes 0, and the offset arithmetic folds away).  A kernel is then: load the row's
// data, walk with a lambda, kmcf_wave_sum64 per accumulator, write on lane 0.  (sub_spmv_kernel keeps its own unrolled walk.)
template <typename ROW>
__device__ __forceinline__ void bitmap_rows(int n_loc, ROW row)
{
    constexpr int wpb = KMCF_BLOCK / 64;
    for (int s = blockIdx.x * wpb + (threadIdx.x >> 6); s < n_loc; s += gridDim.x * wpb) row(s);
}

template <typename BODY>
__device__ __forceinline__ void bitmap_row(const unsigned long long *__restrict__ mrow, int n_groups, long long off, BODY body)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int g = 0; g < n_groups; ++g) {
        const unsigned long long mk = mrow[g];
        if (mk == 0ull) continue;                                          // wave-uniform
        if ((mk >> lane) & 1ull) body(g * 64 + lane, off + __popcll(mk & lt));
        off += __popcll(mk);
    }
}

// Values of the set positions + the row's diagonal = -(sum of the others)
// (populate_T_tunnel_dist2 + calc_diagonal_T_tunnel, :497-614, :669-689).
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_value_kernel(int n_loc, int s0, int n_groups, t_points P, t_wkb w,
                                                                  const unsigned long long *__restrict__ mask, const long long *__restrict__ voff,
                                                                  double *__restrict__ val, double *__restrict__ tdiag, DIST dist)
{
    bitmap_rows(n_loc, [&](int s) {
        const int sg = s0 + s;
        const t_point pi = load_point(P, sg);
        long long dpos = -1;
        double rowsum = 0.0;
        bitmap_row(mask + (size_t)s * n_groups, n_groups, voff[s], [&](int j, long long pos) {
            if (j == sg) { dpos = pos; return; }
            const double v = pair_value<false>(pi, load_point(P, j), w, dist);
            val[pos] = v;
            rowsum += v;
        });
        rowsum = kmcf_wave_sum64(rowsum);
        if (dpos >= 0) val[dpos] = -rowsum;                                // :685
        if ((threadIdx.x & 63) == 0) tdiag[s] = -rowsum;                   // :680
    });
}

// The row sums alone, in tunnel_value_kernel's order of addition, nothing stored but rowsum[s0 + s]: the tunnel diagonal
// of a PERIODIC state held as tiles.  A row's sum then depends on the row alone -- not on the storage form, nor on how a
// group deals the tiles -- so every form and every group size give the diagonal and the preconditioner of the one-rank
// bitmap, bit for bit.
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_rowsum_kernel(int n_loc, int s0, int n_groups, t_points P, t_wkb w,
                                                                   const unsigned long long *__restrict__ mask, double *__restrict__ rowsum_out, DIST dist)
{
    bitmap_rows(n_loc, [&](int s) {
        const int sg = s0 + s;
        const t_point pi = load_point(P, sg);
        double rowsum = 0.0;
        bitmap_row(mask + (size_t)s * n_groups, n_groups, 0, [&](int j, long long) {
            if (j != sg) rowsum += pair_value<false>(pi, load_point(P, j), w, dist);
        });
        rowsum = kmcf_wave_sum64(rowsum);
        if ((threadIdx.x & 63) == 0) rowsum_out[sg] = rowsum;
    });
}

// assemble_preconditioner + invert_diag (src/current_solver_gpu.cu:1323-1338), rhs (:1627-1632)
__global__ __launch_bounds__(KMCF_BLOCK) void copy_diag_rhs_kernel(int n, const double *__restrict__ diag, double *__restrict__ tot,
                                                                   const int *__restrict__ col_node, double loop_G_Vd,
                                                                   double *__restrict__ rhs)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        tot[i] = diag[i];
        const int node = col_node[i];
        rhs[i] = node == 0 ? -loop_G_Vd : (node == 1 ? loop_G_Vd : 0.0);
    }
}

__global__ __launch_bounds__(KMCF_BLOCK) void add_tunnel_diag_kernel(int n_sub, const int *__restrict__ rows,
                                                                     const double *__restrict__ tdiag, double *__restrict__ tot)
{
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sub; s += gridDim.x * blockDim.x) tot[rows[s]] += tdiag[s];
}

__global__ __launch_bounds__(KMCF_BLOCK) void invert_kernel(int n, const double *__restrict__ tot, double *__restrict__ dinv)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dinv[i] = 1 / tot[i];
}

__global__ __launch_bounds__(KMCF_BLOCK) void sub_rows_kernel(int n_sub, int s0, const int *__restrict__ tidx, int row0,
                                                              const int *__restrict__ inv_perm, int *__restrict__ rows)
{
    // shift_vector_by_constant (src/initialize_sparsity_T.cu:904): local row = atom index + 2 - displacement
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sub; s += gridDim.x * blockDim.x)
        rows[s] = inv_perm[tidx[s0 + s] + 2 - row0];
}

// ---------------------------------------------------------------- sub-block operator
__global__ __launch_bounds__(KMCF_BLOCK) void sub_pack_kernel(int n_sub, const int *__restrict__ rows, const double *__restrict__ p,
                                                              double *__restrict__ xsub_loc, const kmcf_scalars *__restrict__ S, int check_done)
{
    if (check_done && S->done) return;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sub; s += gridDim.x * blockDim.x) xsub_loc[s] = p[rows[s]];
}

// y[rows[s]] += S[s, :] x_sub: a wave per row walks the row's masks; the lanes of set positions read their
// value from the packed stream (consecutive lanes -> consecutive values) and x_sub[64 g + lane] (coalesced,
// L2 resident: n_glob doubles).  Four mask words are fetched per step so that four value loads are in flight.
template <bool DOT>
__global__ __launch_bounds__(KMCF_BLOCK) void sub_spmv_kernel(
    int n_loc, int n_glob, int n_groups, const unsigned long long *__restrict__ mask, const long long *__restrict__ voff,
    const double *__restrict__ val, const double *__restrict__ xsub, const int *__restrict__ rows,
    const double *__restrict__ p, double *__restrict__ y, double *__restrict__ part, const kmcf_scalars *__restrict__ S,
    int check_done)
{
    __shared__ double lds4[4];
    if (check_done && S->done) return;
    const int lane = threadIdx.x & 63;
    const int wpb = KMCF_BLOCK / 64;
    const unsigned long long lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    double dot = 0.0;
    for (int s = blockIdx.x * wpb + (threadIdx.x >> 6); s < n_loc; s += gridDim.x * wpb) {
        const unsigned long long *mrow = mask + (size_t)s * n_groups;
        long long off = voff[s];
        double acc = 0.0;
        int g = 0;
        for (; g + 4 <= n_groups; g += 4) {
            const unsigned long long m0 = mrow[g], m1 = mrow[g + 1], m2 = mrow[g + 2], m3 = mrow[g + 3];
            const long long o1 = off + __popcll(m0), o2 = o1 + __popcll(m1), o3 = o2 + __popcll(m2);
            const bool b0 = (m0 >> lane) & 1ull, b1 = (m1 >> lane) & 1ull, b2 = (m2 >> lane) & 1ull, b3 = (m3 >> lane) & 1ull;
            const double v0 = b0 ? __builtin_nontemporal_load(val + off + __popcll(m0 & lt)) : 0.0;
            const double v1 = b1 ? __builtin_nontemporal_load(val + o1 + __popcll(m1 & lt)) : 0.0;
            const double v2 = b2 ? __builtin_nontemporal_load(val + o2 + __popcll(m2 & lt)) : 0.0;
            const double v3 = b3 ? __builtin_nontemporal_load(val + o3 + __popcll(m3 & lt)) : 0.0;
            const int j = g * 64 + lane;
            const double x0 = b0 ? xsub[j] : 0.0, x1 = b1 ? xsub[j + 64] : 0.0, x2 = b2 ? xsub[j + 128] : 0.0,
                         x3 = b3 ? xsub[j + 192] : 0.0;
            acc += v0 * x0; acc += v1 * x1; acc += v2 * x2; acc += v3 * x3;
            off = o3 + __popcll(m3);
        }
        for (; g < n_groups; ++g) {
            const unsigned long long mk = mrow[g];
            if ((mk >> lane) & 1ull) acc += val[off + __popcll(mk & lt)] * xsub[g * 64 + lane];
            off += __popcll(mk);
        }
        acc = kmcf_wave_sum64(acc);
        if (lane == 0) {
            const int r = rows[s];
            y[r] += acc;                                       // unpack_add, dist_spmv_split_sparse.cpp:70-76
            if (DOT) dot += p[r] * acc;
        }
    }
    if (DOT) {
        const double t = kmcf_block_sum(dot, lds4);
        if (threadIdx.x == 0) part[blockIdx.x] = t;
    }
}

// ---------------------------------------------------------------- current and power
__global__ __launch_bounds__(KMCF_BLOCK) void scale_kernel(int n, double *__restrict__ m, double g0)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m[i] = m[i] * g0;
}

// get_imacro_sparse (src/current_solver_gpu.cu:501-542), one block on the rank that owns matrix row 1:
// over that row's entries with column node >= 2: sum of X[1][c] (m[c] - m[1]).
__global__ __launch_bounds__(KMCF_BLOCK) void imacro_kernel(int row, const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                            const double *__restrict__ val, const int *__restrict__ col_node,
                                                            const double *__restrict__ m, double *__restrict__ out)
{
    __shared__ double lds4[4];
    double s = 0.0;
    if (row >= 0) {
        const double m1 = m[1];
        for (int j = row_ptr[row] + threadIdx.x; j < row_ptr[row + 1]; j += KMCF_BLOCK) {
            const int node = col_node[col[j]];
            if (node >= 2) s += val[j] * (m[node] - m1);
        }
    }
    const double t = kmcf_block_sum(s, lds4);
    if (threadIdx.x == 0) *out = t;
}

// min over m[2 .. n) (thrust::min_element, :2068), one block
__global__ __launch_bounds__(KMCF_BLOCK) void min_kernel(int n, const double *__restrict__ m, double *__restrict__ out)
{
    __shared__ double sh[KMCF_BLOCK];
    double v = m[2];
    for (int i = 2 + threadIdx.x; i < n; i += KMCF_BLOCK) v = fmin(v, m[i]);
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = KMCF_BLOCK / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] = fmin(sh[threadIdx.x], sh[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// update_m (:449-459) with the minimum read once (there every thread re-reads m[minidx] while it is being updated)
__global__ __launch_bounds__(KMCF_BLOCK) void shift_kernel(int n, double *__restrict__ m, const double *__restrict__ mn)
{
    const double sh = fabs(*mn);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) m[i] += sh;
}

__device__ __forceinline__ double ineg_of(double x, double mr, double mc, double Vd)
{   // set_ineg, :2367-2377
    const double ical = x * (mr - mc);
    if ((ical < 0 && Vd > 0) || (ical > 0 && Vd < 0)) return -ical;
    return 0.0;
}

// neighbour part of P[r] = sum_c ineg[r][c] m[c] - (sum_c ineg[r][c]) m[r], rows and columns of atoms only
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void power_neighbour_kernel(int n_loc, const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                                     const double *__restrict__ val, const int *__restrict__ diag_pos,
                                                                     const int *__restrict__ col_node, const double *__restrict__ m,
                                                                     double Vd, double *__restrict__ psum, double *__restrict__ isum)
{
    double mr = 0.0;
    neighbour_walk<LPR, double, 2>(
        n_loc, row_ptr, diag_pos,
        [&](int r) {
            const int nr = col_node[r];
            if (nr >= 2) mr = m[nr];
            return nr >= 2;
        },
        [&](int j, double *ab) {
            const int nc = col_node[col[j]];
            if (nc < 2) return;
            const double mc = m[nc];
            const double ig = ineg_of(val[j], mr, mc, Vd);
            ab[0] += ig * mc;
            ab[1] += ig;
        },
        [&](int r, int, const double *ab) { psum[r] = ab[0]; isum[r] = ab[1]; });
}

// tunnel part, added into the same per-row sums: the stored values of the bitmap's rows
__global__ __launch_bounds__(KMCF_BLOCK) void power_tunnel_kernel(
    int n_loc, int s0, int n_groups, const unsigned long long *__restrict__ mask, const long long *__restrict__ voff,
    const double *__restrict__ val, const int *__restrict__ tidx, const int *__restrict__ rows, const double *__restrict__ m,
    double Vd, double *__restrict__ psum, double *__restrict__ isum)
{
    bitmap_rows(n_loc, [&](int s) {
        const int sg = s0 + s;
        const double mr = m[tidx[sg] + 2];
        double a = 0.0, b = 0.0;
        bitmap_row(mask + (size_t)s * n_groups, n_groups, voff[s], [&](int j, long long pos) {
            if (j == sg) return;
            const double mc = m[tidx[j] + 2];
            const double ig = ineg_of(val[pos], mr, mc, Vd);
            a += ig * mc;
            b += ig;
        });
        a = kmcf_wave_sum64(a); b = kmcf_wave_sum64(b);
        if ((threadIdx.x & 63) == 0) { psum[rows[s]] += a; isum[rows[s]] += b; }
    });
}

// P[r] into the row-partitioned pdisp (global row order)
__global__ __launch_bounds__(KMCF_BLOCK) void power_finish_kernel(int n_loc, const int *__restrict__ col_node, const double *__restrict__ m,
                                                                  const double *__restrict__ psum, const double *__restrict__ isum,
                                                                  double *__restrict__ pdisp)
{
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_loc; r += gridDim.x * blockDim.x) {
        const int node = col_node[r];
        pdisp[node] = node >= 2 ? psum[r] + (-isum[r]) * m[node] : 0.0;
    }
}

// copy_pdisp (:462-474): site_power[site of atom a] = -alpha P for non-metal atoms
__global__ __launch_bounds__(KMCF_BLOCK) void copy_pdisp_kernel(int n_atoms_in_matrix, const int *__restrict__ atom_site,
                                                                const unsigned char *__restrict__ acls, const double *__restrict__ pdisp,
                                                                double alpha, double *__restrict__ site_power)
{
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n_atoms_in_matrix; a += gridDim.x * blockDim.x)
        if (!(acls[a] & 1)) site_power[atom_site[a]] = -1 * alpha * pdisp[a + 2];
}


// ---------------------------------------------------------------- dense symmetric sub-block (kmcf_subop::dense)
// (tile (I, J), J >= I, of the upper block triangle: at symm_tile_index(nb, I, J), kmcf_subplan.hpp)
constexpr int SYM_LD = 65;                                   // LDS row stride (doubles): row- AND column-wise reads conflict-free
constexpr int SYM_WAVE_DOUBLES = 64 * SYM_LD + 256;          // tile + four 64-vectors per wave

// Values of the upper tiles (populate_T_tunnel_dist2 on the pairs of the tile; 0 where the pattern has no entry, on
// the diagonal -- set afterwards -- and past the last point).  A wave per strip, lane = column, rows one by one.
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void tunnel_dense_fill_kernel(int n_strips, const int4 *__restrict__ strips, int n_glob, t_points P,
                                                                       t_wkb w, double *__restrict__ tiles, DIST dist)
{
    const int lane = threadIdx.x & 63;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n_strips; s += gridDim.x * 4) {
        const int4 st = strips[s];
        for (int q = 0; q < st.z; ++q) {
            const int J = st.y + q, j = 64 * J + lane;
            const bool jin = j < n_glob;
            const t_point pj = jin ? load_point(P, j) : t_point{};
            double *tile = tiles + ((size_t)st.w + q) * 4096;
            for (int r = 0; r < 64; ++r) {
                const int i = 64 * st.x + r;
                double v = 0.0;
                if (i < n_glob && jin && i != j) v = pair_value<true>(load_point(P, i), pj, w, dist);
                tile[r * 64 + lane] = v;
            }
        }
    }
}

// One pass over the upper tiles.  MODE 0: parts of y = S x (x: the gathered sub-vector).  MODE 1: parts of the
// dissipated-power sums a_i = sum_j ineg(v_ij, m_i, m_j) m_j, b_i = sum_j ineg(v_ij, m_i, m_j) (x: the potentials of the
// tunnel points; the diagonal is skipped).  A wave per strip of tiles of one block row: the tile goes global ->
// registers -> LDS (the NEXT tile's loads are in flight while this one is used); lane r adds row r's products
// column by column (its row sum runs on through the strip's tiles), lane c adds column c's products row by row
// (the tile's contribution to block row J by symmetry; not for diagonal tiles, which are stored complete).
template <int MODE>
__global__ __launch_bounds__(KMCF_BLOCK) void sub_symm_kernel(int n_strips, const int4 *__restrict__ strips, const double *__restrict__ tiles,
                                                              const double *__restrict__ x, double Vd, double *__restrict__ rowpart,
                                                              double *__restrict__ colpart, const kmcf_scalars *__restrict__ S, int check_done)
{
    extern __shared__ double sym_lds[];
    if (check_done && S->done) return;                  // (iterations enqueued behind the stop: nothing to stream)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *T = sym_lds + (size_t)wv * SYM_WAVE_DOUBLES;
    double *xI = T + 64 * SYM_LD, *xJ = xI + 64;
    typedef double dvec2 __attribute__((ext_vector_type(2)));
    dvec2 reg[32];
    const int s0 = blockIdx.x * 4 + wv, ds = gridDim.x * 4;
    int4 st_next = s0 < n_strips ? strips[s0] : make_int4(0, 0, 0, 0);
    if (s0 < n_strips) {
        const dvec2 *src = reinterpret_cast<const dvec2 *>(tiles + (size_t)st_next.w * 4096);
#pragma unroll
        for (int k = 0; k < 32; ++k) reg[k] = __builtin_nontemporal_load(src + k * 64 + lane);
    }
    for (int s = s0; s < n_strips; s += ds) {
        const int4 st = st_next;
        if (s + ds < n_strips) st_next = strips[s + ds];
        const int I = st.x;
        xI[lane] = x[64 * I + lane];
        double ra = 0.0, rb = 0.0;
        for (int q = 0; q < st.z; ++q) {
            const int J = st.y + q;
            // The tile in the registers goes to LDS pair by pair, and each register, as soon as it is free, requests its
            // share of the NEXT tile (of this strip, or the first of the wave's next strip): a wave always has a whole tile
            // (32 KB) in flight.  (Requesting the next tile only after the last pair of this one had arrived left every
            // wave without a single load in flight for one memory latency per tile: 337 us per application at 40 nm.)
            const bool more = q + 1 < st.z, next_strip = !more && s + ds < n_strips;
            const dvec2 *src = reinterpret_cast<const dvec2 *>(tiles + (more ? (size_t)st.w + q + 1 : (size_t)st_next.w) * 4096);
#pragma unroll
            for (int k = 0; k < 32; ++k) {                   // element pair k 64 + lane = row 2 k + (lane >> 5), columns 2 (lane & 31), + 1
                const int r = 2 * k + (lane >> 5), c = 2 * (lane & 31);
                T[r * SYM_LD + c] = reg[k].x;
                T[r * SYM_LD + c + 1] = reg[k].y;
                if (more || next_strip) reg[k] = __builtin_nontemporal_load(src + k * 64 + lane);
            }
            xJ[lane] = x[64 * J + lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool diag = J == I;
            if (MODE == 0) {
                // (x_J / x_I through v_readlane instead of LDS broadcasts: 0.296 against 0.280 ms per iteration -- the kernel is bound by its stream)
#pragma unroll 8
                for (int c = 0; c < 64; ++c) ra += T[lane * SYM_LD + c] * xJ[c];
                if (!diag) {
                    double ca = 0.0;
#pragma unroll 8
                    for (int r = 0; r < 64; ++r) ca += T[r * SYM_LD + lane] * xI[r];
                    colpart[((size_t)st.w + q) * 64 + lane] = ca;
                }
            } else {
                const double mr = xI[lane];
                for (int c = 0; c < 64; ++c) {
                    if (diag && c == lane) continue;
                    const double mc = xJ[c];
                    const double ig = ineg_of(T[lane * SYM_LD + c], mr, mc, Vd);
                    ra += ig * mc;
                    rb += ig;
                }
                if (!diag) {
                    const double mj = xJ[lane];
                    double ca = 0.0, cb = 0.0;
                    for (int r = 0; r < 64; ++r) {
                        const double mi = xI[r];
                        const double ig = ineg_of(T[r * SYM_LD + lane], mj, mi, Vd);
                        ca += ig * mi;
                        cb += ig;
                    }
                    colpart[((size_t)st.w + q) * 128 + lane] = ca;
                    colpart[((size_t)st.w + q) * 128 + 64 + lane] = cb;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (MODE == 0) rowpart[(size_t)s * 64 + lane] = ra;
        else { rowpart[(size_t)s * 128 + lane] = ra; rowpart[(size_t)s * 128 + 64 + lane] = rb; }
    }
}

// ---------------------------------------------------------------- jagged symmetric tiles (kmcf_subop::jagged)
// The upper block triangle again (tile index, strips, row / column parts and their reduction exactly as above), but a
// tile stores only its ENTRIES: the 64 row masks of the pattern (tile-major copy of the bitmap's words) and the values
// in "layers" -- layer k holds the k-th entry of every row that has more than k entries, rows ascending, without gaps
// (a jagged-diagonal layout inside the tile): 4 B per entry of the full block + 1 bit per position, against 4 B per
// POSITION for the dense tiles -- the reference's contact window (44 % full) moves 2.1 x fewer bytes, and the sums are
// the SAME sums: lane r adds row r's products in ascending column order (an absent entry added 0.0 before), lane c
// the tile's column c top-down out of a dense copy of the tile in LDS.  One load instruction per layer, lane r
// reading base_k + (number of rows below r in the layer): consecutive lanes, consecutive addresses.
typedef unsigned long long symj_u64;

// largest of the lanes' values (0 ... 64), through ballots: scalar work only (a shuffle butterfly is six trips through
// the LDS crossbar, ~0.4 us -- per tile)
__device__ __forceinline__ int symj_wave_max(int v)
{
    symj_u64 live = ~0ull;
    int r = 0;
#pragma unroll
    for (int bit = 6; bit >= 0; --bit) {
        const symj_u64 b = __ballot((v >> bit) & 1) & live;
        if (b) { live = b; r |= 1 << bit; }
    }
    return r;
}

// element `l` (a compile-time constant in the unrolled loops) of a 64-vector held one element per lane
__device__ __forceinline__ double symj_lane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// tile-major masks + entries per tile
__global__ __launch_bounds__(KMCF_BLOCK) void symj_mask_kernel(int n_strips, const int4 *__restrict__ strips, int n_glob, int n_groups,
                                                               const symj_u64 *__restrict__ mask, symj_u64 *__restrict__ jmask, int *__restrict__ tcnt)
{
    const int lane = threadIdx.x & 63;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n_strips; s += gridDim.x * 4) {
        const int4 st = strips[s];
        const int i = 64 * st.x + lane;
        for (int q = 0; q < st.z; ++q) {
            const symj_u64 w = i < n_glob ? mask[(size_t)i * n_groups + st.y + q] : 0ull;
            jmask[((size_t)st.w + q) * 64 + lane] = w;
            int c = __popcll(w);
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
            if (lane == 0) tcnt[st.w + q] = c;
        }
    }
}

// values in layer order (populate_T_tunnel_dist2 on the tile's entries; the diagonal entry 0 until symj_set_diag_kernel)
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void symj_fill_kernel(int n_strips, const int4 *__restrict__ strips, int n_glob, t_points P, t_wkb w,
                                                               const symj_u64 *__restrict__ jmask, const long long *__restrict__ jvoff,
                                                               double *__restrict__ jval, DIST dist)
{
    const int lane = threadIdx.x & 63;
    const symj_u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int s = blockIdx.x * 4 + (threadIdx.x >> 6); s < n_strips; s += gridDim.x * 4) {
        const int4 st = strips[s];
        const int i = 64 * st.x + lane;
        const t_point pi = i < n_glob ? load_point(P, i) : t_point{};
        for (int q = 0; q < st.z; ++q) {
            const size_t t = (size_t)st.w + q;
            symj_u64 m = jmask[t * 64 + lane];
            long long base = jvoff[t];
            while (true) {
                const symj_u64 b = __ballot(m != 0);
                if (!b) break;
                if (m) {
                    const int j = 64 * (st.y + q) + __builtin_ctzll(m);
                    m &= m - 1;
                    jval[base + __popcll(b & lt)] = j != i ? pair_value<false>(pi, load_point(P, j), w, dist) : 0.0;
                }
                base += __popcll(b);
            }
        }
    }
}

// tdiag = -(row sums) into the diagonal tiles' diagonal entries (calc_diagonal_T_tunnel, :669-689); a wave per block row
__global__ __launch_bounds__(KMCF_BLOCK) void symj_set_diag_kernel(int n_glob, int nb, const double *__restrict__ rowsum, double *__restrict__ tdiag,
                                                                   const symj_u64 *__restrict__ jmask, const long long *__restrict__ jvoff,
                                                                   double *__restrict__ jval)
{
    const int lane = threadIdx.x & 63;
    const symj_u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    for (int B = blockIdx.x * 4 + (threadIdx.x >> 6); B < nb; B += gridDim.x * 4) {
        const size_t t = (size_t)symm_tile_index(nb, B, B);
        const symj_u64 m = jmask[t * 64 + lane];
        const int cnt = __popcll(m), kl = __popcll(m & lt), i = 64 * B + lane;
        long long pos = jvoff[t];
        for (int k = 0; k < 64; ++k) {
            const symj_u64 b = __ballot(cnt > k);
            if (!b) break;
            if (k < kl) pos += __popcll(b);
            else if (k == kl) pos += __popcll(b & lt);
        }
        if (i < n_glob && ((m >> lane) & 1ull)) {
            const double d = -rowsum[i];
            tdiag[i] = d;
            jval[pos] = d;
        }
    }
}

// One pass over the stored tiles: the jagged twin of sub_symm_kernel (same parts into rowpart / colpart, MODE as there).
// Per tile ONE wait for memory, at the top, for loads that were all requested a tile earlier, before the passes over
// the dense copy: this tile's layers (a lane past its row's end re-reads the layer's first word: no divergent loads),
// the next tile's masks and x_J.  Control flow is scalar (the strip walk is per wavefront), the scatter into the dense
// copy and its removal are branch-free (idle lanes write a dump word).
template <int MODE>
__global__ __launch_bounds__(KMCF_BLOCK) void sub_symj_kernel(int n_strips, const int4 *__restrict__ strips, const symj_u64 *__restrict__ jmask,
                                                              const long long *__restrict__ jvoff, const double *__restrict__ jval,
                                                              const double *__restrict__ x, double Vd, double *__restrict__ rowpart,
                                                              double *__restrict__ colpart, const kmcf_scalars *__restrict__ S, int check_done)
{
    extern __shared__ double sym_lds[];
    if (check_done && S->done) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const symj_u64 lt = lane ? (~0ull >> (64 - lane)) : 0ull;
    double *T = sym_lds + (size_t)wv * SYM_WAVE_DOUBLES;
    double *xI = T + 64 * SYM_LD, *xJ = xI + 64, *dump = xJ + 64;      // (dump: 64 words of the wave's four spare 64-vectors)
#pragma unroll 8
    for (int c = 0; c < 64; ++c) T[lane * SYM_LD + c] = 0.0;           // the dense copy: entries in, entries out again per tile
    const int ds = gridDim.x * 4;
    int s = blockIdx.x * 4 + wv;                                       // (scalar)
    if (s >= n_strips) return;
    int4 st = strips[s];
    st.x = __builtin_amdgcn_readfirstlane(st.x); st.y = __builtin_amdgcn_readfirstlane(st.y);
    st.z = __builtin_amdgcn_readfirstlane(st.z); st.w = __builtin_amdgcn_readfirstlane(st.w);
    int q = 0;
    double v[64];
    auto request = [&](symj_u64 m, long long base) {                   // the layers of a tile (in eights, up to its deepest)
        const int cnt_ = __popcll(m), kmax_ = symj_wave_max(cnt_);
        const double *src = jval + base;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            if ((k & 7) == 0 && k >= kmax_) break;
            const symj_u64 b = __ballot(cnt_ > k);
            v[k] = __builtin_nontemporal_load(src + (cnt_ > k ? __popcll(b & lt) : 0));
            src += __popcll(b);
        }
    };
    // the tile after (s, q) of this wave's walk (scalar): the next of the strip, or the first of the wave's next strip
    auto step = [&](const int4 &a, int sa, int qa, int4 &b, int &sb_, int &qb) -> bool {
        b = a; sb_ = sa; qb = qa + 1;
        if (qb < a.z) return true;
        if (sa + ds >= n_strips) return false;
        sb_ = sa + ds;
        b = strips[sb_];
        b.x = __builtin_amdgcn_readfirstlane(b.x); b.y = __builtin_amdgcn_readfirstlane(b.y);
        b.z = __builtin_amdgcn_readfirstlane(b.z); b.w = __builtin_amdgcn_readfirstlane(b.w);
        qb = 0;
        return true;
    };
    symj_u64 m0 = jmask[(size_t)st.w * 64 + lane];
    int4 st1; int s1, q1;
    bool have1 = step(st, s, q, st1, s1, q1);
    symj_u64 m1 = have1 ? jmask[((size_t)st1.w + q1) * 64 + lane] : 0ull;      // masks run one tile ahead of the values
    request(m0, jvoff[st.w]);
    double xjn = x[64 * st.y + lane];
    xI[lane] = x[64 * st.x + lane];
    double ra = 0.0, rb = 0.0;
    while (true) {
        const int I = st.x, J = st.y + q;
        const size_t t = (size_t)st.w + q;
        const bool diag = J == I;
        const bool more = q + 1 < st.z;
        // ---- this tile's layers are in v (the one wait); entries into the dense copy
        xJ[lane] = xjn;
        const double xi_l = xI[lane], xj_l = xjn;                      // x_I / x_J, one element per lane (columns: readlane)
        const int cnt = __popcll(m0), kmax = symj_wave_max(cnt);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        {
            // entries into the dense copy
            symj_u64 m = m0;
#pragma unroll
            for (int k = 0; k < 64; ++k) {
                if ((k & 7) == 0 && k >= kmax) break;                  // (scalar; k is a compile-time constant in the unrolled body)
                const bool on = m != 0;
                const int c = on ? __builtin_ctzll(m) : 0;
                m &= m - 1;
                double *dst = on ? T + lane * SYM_LD + c : dump + lane;
                *dst = v[k];
            }
        }
        // ---- the next tile's masks arrived with them: its layers, its x_J and the masks of the tile after it go out now
        // and are in flight during the passes over the dense copy
        int4 st2 = st1; int s2 = s1, q2 = q1;
        const bool have2 = have1 && step(st1, s1, q1, st2, s2, q2);
        const symj_u64 m2 = have2 ? jmask[((size_t)st2.w + q2) * 64 + lane] : 0ull;
        double xj1 = 0.0, xi1 = 0.0;
        if (have1) {
            request(m1, jvoff[(size_t)st1.w + q1]);
            xj1 = x[64 * (st1.y + q1) + lane];
            if (s1 != s) xi1 = x[64 * st1.x + lane];
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (kmax > 0) {                                                // the row, as the dense tiles add it (x_J by readlane: no LDS broadcasts)
            if (MODE == 0) {
#pragma unroll
                for (int c = 0; c < 64; ++c) ra += T[lane * SYM_LD + c] * symj_lane(xj_l, c);
            } else {
#pragma unroll
                for (int c = 0; c < 64; ++c) {
                    const double mc = symj_lane(xj_l, c);
                    const double ig = ineg_of(T[lane * SYM_LD + c], xi_l, mc, Vd);
                    if (!(diag && c == lane)) { ra += ig * mc; rb += ig; }
                }
            }
        }
        if (!diag) {
            double ca = 0.0, cb = 0.0;
            if (kmax > 0) {
                if (MODE == 0) {
#pragma unroll
                    for (int r = 0; r < 64; ++r) ca += T[r * SYM_LD + lane] * symj_lane(xi_l, r);
                } else {
#pragma unroll
                    for (int r = 0; r < 64; ++r) {
                        const double mi = symj_lane(xi_l, r);
                        const double ig = ineg_of(T[r * SYM_LD + lane], xj_l, mi, Vd);
                        ca += ig * mi;
                        cb += ig;
                    }
                }
            }
            if (MODE == 0) colpart[t * 64 + lane] = ca;
            else { colpart[t * 128 + lane] = ca; colpart[t * 128 + 64 + lane] = cb; }
        }
        __builtin_amdgcn_wave_barrier();
        if (kmax > 0) {   // entries out again: the lane's row (64 plain stores; walking the mask again costs ten instructions per entry)
#pragma unroll
            for (int c = 0; c < 64; ++c) T[lane * SYM_LD + c] = 0.0;
        }
        if (!more) {                                   // the strip's row parts
            if (MODE == 0) rowpart[(size_t)s * 64 + lane] = ra;
            else { rowpart[(size_t)s * 128 + lane] = ra; rowpart[(size_t)s * 128 + 64 + lane] = rb; }
            ra = rb = 0.0;
        }
        if (!have1) break;
        xjn = xj1;
        if (s1 != s) {
            __builtin_amdgcn_wave_barrier();
            xI[lane] = xi1;
        }
        st = st1; s = s1; q = q1; m0 = m1;
        st1 = st2; s1 = s2; q1 = q2; m1 = m2; have1 = have2;
    }
}

// Adds the parts of one block row B (one block, four waves) in a fixed order: wave w takes the column sums of tiles
// (K, B) for K = w, w + 4, ... < B, then the strips first + w, first + w + 4, ... of its block row, each list in
// ascending order; the four waves' sums are joined as ((c0 + c1) + (c2 + c3)) + ((r0 + r1) + (r2 + r3)).  Into
// y[rows[i]] (MODE 0; rows == nullptr: y[i]) or psum / isum (MODE 1); fused p.Ap partial, one per block (MODE 0).
// (A single lane walking all ~300 parts of its row one dependent load after the other took 83 us at 40 nm.)
template <int MODE, bool DOT>
__global__ __launch_bounds__(KMCF_BLOCK) void sub_symm_reduce_kernel(int n_glob, int nb, const int *__restrict__ strip_first,
                                                                     const double *__restrict__ rowpart, const double *__restrict__ colpart,
                                                                     const int *__restrict__ rows, const double *__restrict__ p,
                                                                     double *__restrict__ y, double *__restrict__ y2, double *__restrict__ part,
                                                                     const kmcf_scalars *__restrict__ S, int check_done,
                                                                     const int *__restrict__ tile_local = nullptr, double *__restrict__ ypart = nullptr)
{
    // Spread over a rank group (tile_local, ypart != nullptr): the same walk over THIS rank's tiles and strips (another
    // rank's tile (K, B) is skipped in place: wave w keeps K = w, w + 4, ...; the strips are this rank's list), the sums
    // of all 64 nb points go to ypart (and ypart + 64 nb, MODE 1) for sub_combine_kernel instead of y.
    __shared__ double sh[2][2][4][64];                  // [a / b][column / row parts][wave][lane]
    __shared__ double lds4[4];
    if (check_done && S->done) return;
    constexpr int W = MODE == 0 ? 64 : 128;
    const int B = blockIdx.x, l = threadIdx.x & 63, w = threadIdx.x >> 6;
    double ca = 0.0, cb = 0.0, ra = 0.0, rb = 0.0;
#pragma unroll 4
    for (int K = w; K < B; K += 4) {
        size_t t = (size_t)symm_tile_index(nb, K, B);
        if (tile_local) {
            const int tl = tile_local[t];
            if (tl < 0) continue;
            t = (size_t)tl;
        }
        ca += colpart[t * W + l];
        if (MODE == 1) cb += colpart[t * W + 64 + l];
    }
    for (int s = strip_first[B] + w; s < strip_first[B + 1]; s += 4) {
        ra += rowpart[(size_t)s * W + l];
        if (MODE == 1) rb += rowpart[(size_t)s * W + 64 + l];
    }
    sh[0][0][w][l] = ca; sh[0][1][w][l] = ra;
    if (MODE == 1) { sh[1][0][w][l] = cb; sh[1][1][w][l] = rb; }
    __syncthreads();
    double dot = 0.0;
    const int i = 64 * B + l;
    if (ypart) {
        if (w == 0) {
            ypart[i] = ((sh[0][0][0][l] + sh[0][0][1][l]) + (sh[0][0][2][l] + sh[0][0][3][l])) +
                       ((sh[0][1][0][l] + sh[0][1][1][l]) + (sh[0][1][2][l] + sh[0][1][3][l]));
            if (MODE == 1)
                ypart[64 * nb + i] = ((sh[1][0][0][l] + sh[1][0][1][l]) + (sh[1][0][2][l] + sh[1][0][3][l])) +
                                     ((sh[1][1][0][l] + sh[1][1][1][l]) + (sh[1][1][2][l] + sh[1][1][3][l]));
        }
        return;
    }
    if (w == 0 && i < n_glob) {
        const double a = ((sh[0][0][0][l] + sh[0][0][1][l]) + (sh[0][0][2][l] + sh[0][0][3][l])) +
                         ((sh[0][1][0][l] + sh[0][1][1][l]) + (sh[0][1][2][l] + sh[0][1][3][l]));
        const int r = rows ? rows[i] : i;
        y[r] += a;
        if (MODE == 0) {
            if (DOT) dot = p[r] * a;
        } else {
            const double b = ((sh[1][0][0][l] + sh[1][0][1][l]) + (sh[1][0][2][l] + sh[1][0][3][l])) +
                             ((sh[1][1][0][l] + sh[1][1][1][l]) + (sh[1][1][2][l] + sh[1][1][3][l]));
            y2[r] += b;
        }
    }
    if (DOT) {
        const double t = kmcf_block_sum(dot, lds4);
        if (threadIdx.x == 0) part[blockIdx.x] = t;
    }
}

// The sums of a rank group's partials (spread storage): point row0 + s = the partials of ranks 0, 1, ... in that order;
// into y[rows[s]] (rows == nullptr: y[s]) and y2 (MODE 1); fused p.Ap partial, one per block of 256 points (MODE 0).
template <int MODE, bool DOT>
__global__ __launch_bounds__(KMCF_BLOCK) void sub_combine_kernel(int ns, int row0, int P, int npad, const double *__restrict__ ypart_all,
                                                                 const int *__restrict__ rows, const double *__restrict__ p,
                                                                 double *__restrict__ y, double *__restrict__ y2, double *__restrict__ part,
                                                                 const kmcf_scalars *__restrict__ S, int check_done)
{
    __shared__ double lds4[4];
    if (check_done && S->done) return;
    constexpr int W = MODE == 0 ? 1 : 2;
    const int s = blockIdx.x * KMCF_BLOCK + threadIdx.x;
    double dot = 0.0;
    if (s < ns) {
        const size_t i = (size_t)row0 + s;
        double a = 0.0, b = 0.0;
        for (int q = 0; q < P; ++q) {
            a += ypart_all[(size_t)q * W * npad + i];
            if (MODE == 1) b += ypart_all[(size_t)q * W * npad + npad + i];
        }
        const int r = rows ? rows[s] : s;
        y[r] += a;
        if (MODE == 1) y2[r] += b;
        else if (DOT) dot = p[r] * a;
    }
    if (DOT) {
        const double t = kmcf_block_sum(dot, lds4);
        if (threadIdx.x == 0) part[blockIdx.x] = t;
    }
}

// tdiag = -(row sums), the diagonal entries of the diagonal tiles (calc_diagonal_T_tunnel, :669-689); tile_local: the
// spread storage's map (only this rank's diagonal tiles exist here)
__global__ __launch_bounds__(KMCF_BLOCK) void symm_set_diag_kernel(int n_glob, int nb, const double *__restrict__ rowsum, double *__restrict__ tdiag,
                                                                   double *__restrict__ tiles, const int *__restrict__ tile_local)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_glob; i += gridDim.x * blockDim.x) {
        const double d = -rowsum[i];
        tdiag[i] = d;
        const int B = i >> 6, l = i & 63;
        long long tl = symm_tile_index(nb, B, B);
        if (tile_local) tl = tile_local[tl];
        if (tl >= 0) tiles[(size_t)tl * 4096 + l * 64 + l] = d;
    }
}

__global__ __launch_bounds__(KMCF_BLOCK) void fill_kernel(int n, double *__restrict__ a, double v)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) a[i] = v;
}

__global__ __launch_bounds__(KMCF_BLOCK) void gather_tunnel_pot_kernel(int n_glob, const int *__restrict__ tidx, const double *__restrict__ m,
                                                                       double *__restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_glob; i += gridDim.x * blockDim.x) out[i] = m[tidx[i] + 2];
}

// ---------------------------------------------------------------- current map (kmcf_current_map)
// Per node r of the T matrix three sums over the stored off-diagonals (r, c) of its row, I_rc = g (m_r - m_c) with
// g = -A_rc: sum |I_rc|, the same over tunnel pairs only, and sum I_rc; kept interleaved in cm[3 node + 0 / 1 / 2] so that
// one all-gather moves them.  The virtual-virtual entry (0, 1) / (1, 0) -- the loop_G driver -- is no pair.
// Neighbour part (neighbour_walk, virtual rows included): sets all three.
template <int LPR>
__global__ __launch_bounds__(KMCF_BLOCK) void current_neighbour_kernel(int n_loc, const int *__restrict__ row_ptr, const int *__restrict__ col,
                                                                       const double *__restrict__ val, const int *__restrict__ diag_pos,
                                                                       const int *__restrict__ col_node, const double *__restrict__ m,
                                                                       double *__restrict__ cm)
{
    int nr = 0;
    double mr = 0.0;
    neighbour_walk<LPR, double, 2>(
        n_loc, row_ptr, diag_pos,
        [&](int r) { nr = col_node[r]; mr = m[nr]; return true; },
        [&](int j, double *ab) {
            const int nc = col_node[col[j]];
            if (nr < 2 && nc < 2) return;                              // (0, 1) / (1, 0)
            const double g = -val[j];
            const double i_rc = g * (mr - m[nc]);
            ab[0] += fabs(i_rc);
            ab[1] += i_rc;
        },
        [&](int, int, const double *ab) { cm[3 * (size_t)nr] = ab[0]; cm[3 * (size_t)nr + 1] = 0.0; cm[3 * (size_t)nr + 2] = ab[1]; });
}

// Tunnel part (the bitmap's rows): the conductance of every set pair is evaluated afresh -- pair_value: the same value
// whatever storage the solve uses --, the row's sums go into the slots of its node (after the neighbour part, same stream).
template <typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void current_tunnel_kernel(int n_loc, int s0, int n_groups, t_points P, t_wkb w,
                                                                    const unsigned long long *__restrict__ mask, const int *__restrict__ tidx,
                                                                    const double *__restrict__ m, double *__restrict__ cm, DIST dist)
{
    bitmap_rows(n_loc, [&](int s) {
        const int sg = s0 + s;
        const t_point pi = load_point(P, sg);
        const int node = tidx[sg] + 2;
        const double mr = m[node];
        double a = 0.0, b = 0.0;
        bitmap_row(mask + (size_t)s * n_groups, n_groups, 0, [&](int j, long long) {
            if (j == sg) return;
            const double gc = -pair_value<false>(pi, load_point(P, j), w, dist);
            const double i_rc = gc * (mr - m[tidx[j] + 2]);
            a += fabs(i_rc);
            b += i_rc;
        });
        a = kmcf_wave_sum64(a); b = kmcf_wave_sum64(b);
        if ((threadIdx.x & 63) == 0) { cm[3 * (size_t)node] += a; cm[3 * (size_t)node + 1] = a; cm[3 * (size_t)node + 2] += b; }
    });
}

// site arrays (zero-filled before): through = half of sum |I|, tunnel likewise, net; atoms with a row only
__global__ __launch_bounds__(KMCF_BLOCK) void current_scatter_kernel(int n_rows_atoms, const int *__restrict__ atom_site,
                                                                     const double *__restrict__ cm, double *__restrict__ site_current,
                                                                     double *__restrict__ site_tunnel, double *__restrict__ site_net)
{
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n_rows_atoms; a += gridDim.x * blockDim.x) {
        const int s = atom_site[a];
        const double *v = cm + 3 * ((size_t)a + 2);
        site_current[s] = 0.5 * v[0];
        if (site_tunnel) site_tunnel[s] = 0.5 * v[1];
        if (site_net) site_net[s] = v[2];
    }
}

// One block: thread t adds atoms t, t + 256, ... in ascending order, then the block sum -- an order the input fixes.
// out: [0] net[1], [1] -net[0], [2] sum through, [3] sum tunnel, [4] max through, [5] its site (lowest among equals; -1)
__global__ __launch_bounds__(KMCF_BLOCK) void current_stats_kernel(int n_rows_atoms, const int *__restrict__ atom_site,
                                                                   const double *__restrict__ cm, double *__restrict__ out)
{
    __shared__ double lds4[4];
    double st = 0.0, su = 0.0, mx = -1.0;
    for (int a = threadIdx.x; a < n_rows_atoms; a += KMCF_BLOCK) {
        const double th = 0.5 * cm[3 * ((size_t)a + 2)];
        st += th;
        su += 0.5 * cm[3 * ((size_t)a + 2) + 1];
        mx = fmax(mx, th);
    }
    st = kmcf_block_sum(st, lds4);
    su = kmcf_block_sum(su, lds4);
    mx = kmcf_block_max(mx, lds4);
    double site = -2147483648.0;                                           // (minus the site: a maximum again)
    for (int a = threadIdx.x; a < n_rows_atoms; a += KMCF_BLOCK)
        if (0.5 * cm[3 * ((size_t)a + 2)] == mx) site = fmax(site, -(double)atom_site[a]);
    site = kmcf_block_max(site, lds4);
    if (threadIdx.x == 0) {
        const bool found = site > -2147483648.0;
        out[0] = cm[3 * 1 + 2];
        out[1] = -cm[2];
        out[2] = st;
        out[3] = su;
        out[4] = found ? mx : 0.0;
        out[5] = found ? -site : -1.0;
    }
}

// ---------------------------------------------------------------- current profile (kmcf_current_profile)
// Per node CP_STRIDE doubles, interleaved so that one all-gather moves them:
//   [0] / [1]  sum of I_as over the node's counted NEIGHBOUR pairs that leave its slab (q(s) != q(a)): those of its own
//              cell / the rest        [2] / [3]  the same over its TUNNEL pairs
//   [4 .. 6]   sum of I_as * d_as (twice J; zeros when no vector is asked for)        [7]  sum of I_as over ALL its pairs
// The two virtual nodes have no position: only [7] is formed for them (the injected / extracted current).
constexpr int CP_STRIDE = 8, CP_MAX = 1024;

// d_as in y and z: plain differences on an open state, the library's minimum image (kmcf_min_image_dist's expression, of
// s against a) on a periodic one; picked by the state's distance functor like the WKB distance itself
__device__ __forceinline__ void pair_disp(const dist_open &, double ya, double za, double ys, double zs, double *dy, double *dz)
{
    *dy = ys - ya; *dz = zs - za;
}
__device__ __forceinline__ void pair_disp(const dist_min_image &d, double ya, double za, double ys, double zs, double *dy, double *dz)
{
    double fy = (ys - ya) / d.ly;
    fy -= round(fy);
    double fz = (zs - za) / d.lz;
    fz -= round(fz);
    *dy = fy * d.ly; *dz = fz * d.lz;
}

// q(a) = number of planes X_k <= x_a (binary search in LDS) and the cell of every atom: n_cells stands for "none"
__global__ __launch_bounds__(KMCF_BLOCK) void profile_key_kernel(int n_atoms, const double *__restrict__ ax, const int *__restrict__ atom_site,
                                                                 const int *__restrict__ site_cell, int n_cells,
                                                                 const double *__restrict__ planes, int n_planes, int *__restrict__ q,
                                                                 int *__restrict__ cell)
{
    __shared__ double X[CP_MAX];
    for (int k = threadIdx.x; k < n_planes; k += KMCF_BLOCK) X[k] = planes[k];
    __syncthreads();
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n_atoms; a += gridDim.x * blockDim.x) {
        const double x = ax[a];
        int lo = 0, hi = n_planes;                                        // planes [0, lo) are <= x, planes [hi, n) are > x
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (X[mid] <= x) lo = mid + 1; else hi = mid;
        }
        q[a] = lo;
        int c = 0;
        if (site_cell) {
            c = site_cell[atom_site[a]];
            if (c < 0 || c >= n_cells) c = n_cells;
        }
        cell[a] = c;
    }
}

// The slab and cell of every atom, as the pair kernels take them
struct cp_keys { const int *q, *cell; int n_cells; };

// The sums of one row while its pairs are walked: CP_SAME / CP_REST / CP_NET, and with VEC the three of the vector behind
// them -- without it they do not exist, so nothing shuffles or adds them.
constexpr int CP_SAME = 0, CP_REST = 1, CP_NET = 2, CP_JX = 3;

// One counted pair a -> s carrying i_as into the sums of a.  s is the other ATOM; its coordinates are cx / cy / cz[cs]: the
// atoms' arrays at s (neighbour part) or the tunnel points' at the point's index (tunnel part; tx[j] == ax[tidx[j]]).
template <bool VEC, typename DIST>
__device__ __forceinline__ void profile_add_pair(double i_as, int s, int cs, int qa, int ca, const cp_keys &K, const double *__restrict__ cx,
                                                 const double *__restrict__ cy, const double *__restrict__ cz, double xa, double ya, double za,
                                                 const DIST &dist, double *sums)
{
    if (K.q[s] != qa) {
        if (ca < K.n_cells && K.cell[s] == ca) sums[CP_SAME] += i_as; else sums[CP_REST] += i_as;
    }
    if constexpr (VEC) {
        double dy, dz;
        pair_disp(dist, ya, za, cy[cs], cz[cs], &dy, &dz);
        sums[CP_JX] += i_as * (cx[cs] - xa); sums[CP_JX + 1] += i_as * dy; sums[CP_JX + 2] += i_as * dz;
    }
}

// Neighbour part (neighbour_walk, virtual rows included); sets all CP_STRIDE values of the row's node.
template <int LPR, bool VEC, typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void profile_neighbour_kernel(
    int n_loc, const int *__restrict__ row_ptr, const int *__restrict__ col, const double *__restrict__ val, const int *__restrict__ diag_pos,
    const int *__restrict__ col_node, const double *__restrict__ m, cp_keys K, const double *__restrict__ ax, const double *__restrict__ ay,
    const double *__restrict__ az, double *__restrict__ pv, DIST dist)
{
    int nr = 0, qa = 0, ca = 0;
    double mr = 0.0, xa = 0.0, ya = 0.0, za = 0.0;
    neighbour_walk<LPR, double, VEC ? 6 : 3>(
        n_loc, row_ptr, diag_pos,
        [&](int r) {
            nr = col_node[r];
            mr = m[nr];
            const int a = nr - 2;
            if (a >= 0) {
                qa = K.q[a]; ca = K.cell[a];
                if (VEC) { xa = ax[a]; ya = ay[a]; za = az[a]; }
            }
            return true;
        },
        [&](int j, double *sums) {
            const int nc = col_node[col[j]];
            if (nr < 2 && nc < 2) return;                              // (0, 1) / (1, 0)
            const double g = -val[j];
            const double i_rc = g * (mr - m[nc]);
            sums[CP_NET] += i_rc;
            if (nr >= 2 && nc >= 2) profile_add_pair<VEC>(i_rc, nc - 2, nc - 2, qa, ca, K, ax, ay, az, xa, ya, za, dist, sums);
        },
        [&](int, int, const double *sums) {
            double *v = pv + CP_STRIDE * (size_t)nr;
            v[0] = sums[CP_SAME]; v[1] = sums[CP_REST]; v[2] = 0.0; v[3] = 0.0; v[7] = sums[CP_NET];
            if constexpr (VEC) { v[4] = sums[CP_JX]; v[5] = sums[CP_JX + 1]; v[6] = sums[CP_JX + 2]; }
            else v[4] = v[5] = v[6] = 0.0;
        });
}

// Tunnel part (the bitmap's rows, every set pair's conductance by pair_value); sets [2] / [3] and adds onto [4 .. 7] of the
// row's node (after the neighbour part, same stream).
template <bool VEC, typename DIST>
__global__ __launch_bounds__(KMCF_BLOCK) void profile_tunnel_kernel(int n_loc, int s0, int n_groups, t_points P, t_wkb w,
                                                                    const unsigned long long *__restrict__ mask, const int *__restrict__ tidx,
                                                                    const double *__restrict__ m, cp_keys K, double *__restrict__ pv, DIST dist)
{
    bitmap_rows(n_loc, [&](int s) {
        const int sg = s0 + s;
        const t_point pi = load_point(P, sg);
        const int a = tidx[sg];
        const double mr = m[a + 2];
        const int qa = K.q[a], ca = K.cell[a];
        constexpr int NS = VEC ? 6 : 3;
        double sums[NS] = {};
        bitmap_row(mask + (size_t)s * n_groups, n_groups, 0, [&](int j, long long) {
            if (j == sg) return;
            const double gc = -pair_value<false>(pi, load_point(P, j), w, dist);
            const int b = tidx[j];
            const double i_rc = gc * (mr - m[b + 2]);
            sums[CP_NET] += i_rc;
            profile_add_pair<VEC>(i_rc, b, j, qa, ca, K, P.x, P.y, P.z, pi.x, pi.y, pi.z, dist, sums);
        });
#pragma unroll
        for (int k = 0; k < NS; ++k) sums[k] = kmcf_wave_sum64(sums[k]);
        if ((threadIdx.x & 63) == 0) {
            double *v = pv + CP_STRIDE * ((size_t)a + 2);
            v[2] = sums[CP_SAME]; v[3] = sums[CP_REST]; v[7] += sums[CP_NET];
            if constexpr (VEC) { v[4] += sums[CP_JX]; v[5] += sums[CP_JX + 1]; v[6] += sums[CP_JX + 2]; }
        }
    });
}

// Binning, in two steps without atomics.  The atoms with a row are cut into n_seg segments of seg_len atoms (a multiple of
// KMCF_BLOCK; both follow from the atom count and n_cells alone, so the order of every addition is fixed by the input).
// profile_bin_kernel, block (g, c): the values of cell c (c == n_cells: the rest values of every atom) of segment g, summed
// by slab into part[c][g][slab][t].  The atoms pass through LDS in chunks of KMCF_BLOCK; thread q % 256 owns slab q and adds
// the chunk's atoms of its slabs in ascending atom order.  (An atom whose two values are zero is skipped: adding a zero
// changes no bit of a sum that starts at +0.)
__global__ __launch_bounds__(KMCF_BLOCK) void profile_bin_kernel(int n_rows_atoms, int seg_len, int n_planes, int n_cells,
                                                                 const int *__restrict__ q, const int *__restrict__ cell,
                                                                 const double *__restrict__ pv, double *__restrict__ part)
{
    __shared__ double bins[2 * (CP_MAX + 1)];
    __shared__ double s0[KMCF_BLOCK], s1[KMCF_BLOCK];
    __shared__ int sq[KMCF_BLOCK];
    const int g = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const bool is_rest = c == n_cells;
    const int n_bins = 2 * (n_planes + 1);
    for (int i = tid; i < n_bins; i += KMCF_BLOCK) bins[i] = 0.0;
    const int a_end = min(n_rows_atoms, (g + 1) * seg_len);
    for (int a0 = g * seg_len; a0 < a_end; a0 += KMCF_BLOCK) {
        const int a = a0 + tid;
        int myq = -1;
        double v0 = 0.0, v1 = 0.0;
        if (a < a_end && (is_rest || cell[a] == c)) {
            const double *v = pv + CP_STRIDE * ((size_t)a + 2);
            v0 = v[is_rest ? 1 : 0]; v1 = v[is_rest ? 3 : 2];
            if (v0 != 0.0 || v1 != 0.0) myq = q[a];
        }
        if (!__syncthreads_or(myq >= 0)) continue;                        // (block-uniform; also the barrier before sq is rewritten)
        sq[tid] = myq; s0[tid] = v0; s1[tid] = v1;
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < KMCF_BLOCK; ++j) {
            const int qq = sq[j];
            if (qq >= 0 && (qq & (KMCF_BLOCK - 1)) == tid) { bins[2 * qq] += s0[j]; bins[2 * qq + 1] += s1[j]; }
        }
    }
    __syncthreads();
    double *out = part + ((size_t)c * gridDim.x + g) * n_bins;
    for (int i = tid; i < n_bins; i += KMCF_BLOCK) out[i] = bins[i];
}

// profile_prefix_kernel, block c: the segments' sums of every slab added in ascending segment order, then
// F[c][k][t] = sum over the slabs q <= k, one thread per kind.
__global__ __launch_bounds__(KMCF_BLOCK) void profile_prefix_kernel(int n_seg, int n_planes, const double *__restrict__ part,
                                                                    double *__restrict__ prof)
{
    __shared__ double bins[2 * (CP_MAX + 1)];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n_bins = 2 * (n_planes + 1);
    for (int i = tid; i < n_bins; i += KMCF_BLOCK) {
        double acc = 0.0;
        for (int g = 0; g < n_seg; ++g) acc += part[((size_t)c * n_seg + g) * n_bins + i];
        bins[i] = acc;
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const int t = tid >> 6;
        double acc = 0.0;
        for (int k = 0; k < n_planes; ++k) {
            acc += bins[2 * k + t];
            prof[((size_t)c * n_planes + k) * 2 + t] = acc;
        }
    }
}

// J to the site arrays (zero-filled before): half of the sums, atoms with a row only
__global__ __launch_bounds__(KMCF_BLOCK) void profile_scatter_kernel(int n_rows_atoms, const int *__restrict__ atom_site,
                                                                     const double *__restrict__ pv, double *__restrict__ site_jx,
                                                                     double *__restrict__ site_jy, double *__restrict__ site_jz)
{
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < n_rows_atoms; a += gridDim.x * blockDim.x) {
        const int s = atom_site[a];
        const double *v = pv + CP_STRIDE * ((size_t)a + 2);
        site_jx[s] = 0.5 * v[4]; site_jy[s] = 0.5 * v[5]; site_jz[s] = 0.5 * v[6];
    }
}

// One block.  total[k] = sum over c = 0 .. n_cells (ascending) of (F[c][k][0] + F[c][k][1]), thread k % 256; its smallest and
// largest value with the lowest plane among equals; sum of jx like current_stats_kernel's sums.
// out: [0] net[1], [1] -net[0], [2] flux_min, [3] flux_max, [4] sum_jx, [5] plane_min, [6] plane_max
__global__ __launch_bounds__(KMCF_BLOCK) void profile_stats_kernel(int n_rows_atoms, int n_planes, int n_cells, const double *__restrict__ prof,
                                                                   const double *__restrict__ pv, int vec, double *__restrict__ out)
{
    __shared__ double lds4[4];
    __shared__ double tot[CP_MAX];
    const double inf = __builtin_huge_val();
    double mx = -inf, mn_neg = -inf;                                       // (minus the minimum: a maximum again)
    for (int k = threadIdx.x; k < n_planes; k += KMCF_BLOCK) {
        double s = 0.0;
        for (int c = 0; c <= n_cells; ++c) {
            const double *f = prof + ((size_t)c * n_planes + k) * 2;
            s += f[0] + f[1];
        }
        tot[k] = s;
        mx = fmax(mx, s); mn_neg = fmax(mn_neg, -s);
    }
    mx = kmcf_block_max(mx, lds4);                                         // (its barriers also publish tot)
    mn_neg = kmcf_block_max(mn_neg, lds4);
    double kmx = -2147483648.0, kmn = -2147483648.0;                       // (minus the plane)
    for (int k = threadIdx.x; k < n_planes; k += KMCF_BLOCK) {
        if (tot[k] == mx) kmx = fmax(kmx, -(double)k);
        if (-tot[k] == mn_neg) kmn = fmax(kmn, -(double)k);
    }
    kmx = kmcf_block_max(kmx, lds4);
    kmn = kmcf_block_max(kmn, lds4);
    double sj = 0.0;
    if (vec)
        for (int a = threadIdx.x; a < n_rows_atoms; a += KMCF_BLOCK) sj += 0.5 * pv[CP_STRIDE * ((size_t)a + 2) + 4];
    sj = kmcf_block_sum(sj, lds4);
    if (threadIdx.x == 0) {
        out[0] = pv[CP_STRIDE * 1 + 7];
        out[1] = -pv[7];
        out[2] = -mn_neg; out[3] = mx; out[4] = sj;
        out[5] = kmn > -2147483648.0 ? -kmn : -1.0;                       // (-1: every total is a NaN)
        out[6] = kmx > -2147483648.0 ? -kmx : -1.0;
    }
}

// growth rule of the per-assembly buffers: a quarter more than needed, 64 elements at least
template <typename T>
int ensure(T **d, size_t *cap, size_t need)
{
    return kmcf_dev_grow(d, cap, need, std::max<size_t>(need + need / 4, 64) - need);
}

// blocks of a kernel that gives a wave to each of ns rows (KMCF_BLOCK / 64 = 4 waves a block: (ns + 3) / 4), at most
// one per p.Ap partial
int wave_row_grid(int ns)
{
    constexpr int wpb = KMCF_BLOCK / 64;
    return std::max(1, std::min((ns + wpb - 1) / wpb, KMCF_MAX_PARTIALS));
}

// blocks of a kernel that gives a wave to each strip of tiles
int strip_grid(int n_strips) { return std::max(1, std::min((n_strips + 3) / 4, 8192)); }

// f(the state's distance functor): where the geometry of a state picks the instantiation of a kernel that BOTH geometries
// run.  (One kernel only a periodic state runs, tunnel_rowsum_kernel<dist_min_image>, is launched by symm_diagonal itself.)
t_points points_of(const kmcf_tstate *t) { return {t->d_tinfo, t->d_tx, t->d_ty, t->d_tz, t->d_tcb}; }
t_wkb wkb_of(const kmcf_tstate *t) { return {t->nn_dist, t->par.tol, t->par.m_e, t->par.V0}; }

template <typename F>
void with_dist(const kmcf_tstate *t, F f)
{
    if (t->pbc) f(dist_min_image{t->lattice[1], t->lattice[2]});
    else f(dist_open{});
}

}  // namespace

extern "C" int kmcf_tstate_destroy(kmcf_tstate *t)
{
    if (!t) return KMCF_OK;
    if (t->comm && t->comm->device >= 0) {
        hipSetDevice(t->comm->device);
        hipStreamSynchronize(t->comm->stream);
        kmcf_dev_free_all({t->d_atom_site, t->d_site_is_atom, t->d_ax, t->d_ay, t->d_az, t->d_acb, t->d_ael, t->d_ach, t->d_acls,
                           t->d_cls_col, t->d_col_node, t->d_diag_pos, t->d_ground, t->d_inv_perm, t->d_diag, t->d_diag_tot, t->d_rhs,
                           t->d_blk, t->d_tidx, t->d_tinfo, t->d_tx, t->d_ty, t->d_tz, t->d_tcb, t->d_rowcnt, t->d_tdiag,
                           t->sub.d_rows, t->sub.d_mask, t->sub.d_voff, t->sub.d_val, t->sub.d_xsub, t->d_pdisp, t->d_scal, t->d_err,
                           t->sub.d_tiles, t->sub.d_strips, t->sub.d_strip_first, t->sub.d_rowpart, t->sub.d_colpart,
                           t->sub.d_jmask, t->sub.d_jvoff, t->sub.d_jval, t->sub.d_jcnt, t->sub.d_tile_local, t->sub.d_ypart, t->d_agree,
                           t->d_cmap, t->d_cmstat, t->d_cprof, t->d_cpq, t->d_cpcell, t->d_cpplanes, t->d_cpout, t->d_cppart});
        for (void *p : t->cp_retired_dev) hipFree(p);
        for (void *p : t->cp_retired_host) hipHostFree(p);
        if (t->h_cpplanes) hipHostFree(t->h_cpplanes);
        if (t->h_cpout) hipHostFree(t->h_cpout);
        if (t->h_pin) hipHostFree(t->h_pin);
        if (t->h_agree) hipHostFree(t->h_agree);
        if (t->h_cmstat) hipHostFree(t->h_cmstat);
    }
    if (t->T) { t->T->sub = nullptr; kmcf_matrix_destroy(t->T); }
    delete t;
    return KMCF_OK;
}

extern "C" kmcf_matrix *kmcf_tstate_matrix(kmcf_tstate *t) { return t ? t->T : nullptr; }

// ---------------------------------------------------------------- kmcf_initialize_sparsity_T, step by step
struct t_host_coords { std::vector<double> x, y, z; };      // the atoms' coordinates as the gather kernel wrote them

static int init_check_args(const kmcf_comm *c, const double *d_site_x, const double *d_site_y, const double *d_site_z,
                           const int *d_site_element, int N, double nn_dist, int num_source_inj, int num_ground_ext,
                           int num_layers_contact, const int *h_counts_T, const int *h_displs_T, kmcf_tstate **out)
{
    KMCF_CHECK(c && d_site_x && d_site_y && d_site_z && d_site_element && h_counts_T && h_displs_T && out, KMCF_ERR_ARG,
               "kmcf_initialize_sparsity_T: null argument");
    KMCF_CHECK(c->device >= 0, KMCF_ERR_STATE, "kmcf_initialize_sparsity_T: host-only communicator");
    KMCF_CHECK(N > 0 && num_source_inj > 0 && num_ground_ext > 0 && num_layers_contact > 0 && nn_dist > 0, KMCF_ERR_ARG,
               "kmcf_initialize_sparsity_T: bad sizes");
    return KMCF_OK;
}

// atoms = sites that are not interstitials (is_defect, src/gpu_solvers.h:331-337), in site order; the per-atom arrays
static int init_atom_set(kmcf_tstate *t, const int *d_site_element, const int *h_counts_T)
{
    const int N = t->N;
    std::vector<int> el((size_t)N);
    KMCF_HIP(hipMemcpy(el.data(), d_site_element, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<unsigned char> is_atom((size_t)N, 0);
    for (int s = 0; s < N; ++s)
        if (el[s] != EL_DEFECT && el[s] != EL_OXYGEN_DEFECT) { t->h_atom_site.push_back(s); is_atom[s] = 1; }
    const int Na = t->N_atom = (int)t->h_atom_site.size();
    const int Nsub = t->Nsub = Na + 1;
    KMCF_CHECK(Na >= 4 && t->n_inj + 2 < Nsub && t->n_ext < Na, KMCF_ERR_ARG,
               "kmcf_initialize_sparsity_T: %d atoms for %d injection / %d extraction atoms", Na, t->n_inj, t->n_ext);
    int64_t tot = 0;
    for (int q = 0; q < t->comm->nranks; ++q) tot += h_counts_T[q];
    KMCF_CHECK(tot == Nsub, KMCF_ERR_ARG, "kmcf_initialize_sparsity_T: counts_T sum to %lld, the matrix has N_atom + 1 = %d rows",
               (long long)tot, Nsub);
    KMCF_TRY(upload(&t->d_atom_site, t->h_atom_site));
    KMCF_TRY(upload(&t->d_site_is_atom, is_atom));
    const size_t na = (size_t)Na;      // (>= 4: no buffer below is empty; all of them start zeroed)
    KMCF_TRY(kmcf_dev_alloc(&t->d_ax, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_ay, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_az, na, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_acb, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_ael, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_ach, na, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_acls, na, true, t->comm->stream));
    KMCF_HIP(hipStreamSynchronize(t->comm->stream));      // (the fills: the gather kernel, on the caller's stream, writes d_ax .. d_az next)
    return KMCF_OK;
}

// the atoms' coordinates out of the caller's site arrays, on the device and (read back and checked) on the host
static int init_gather_coords(kmcf_tstate *t, const double *d_site_x, const double *d_site_y, const double *d_site_z, t_host_coords *xyz)
{
    kmcf_comm *c = t->comm;
    const int N = t->N, Na = t->N_atom;
    // On the CALLER's stream (kmcf_setup_stream, kmcf_internal.hpp): the first kernel that reads the caller's arrays.
    gather_coords_kernel<<<kmcf_grid1d(Na), KMCF_BLOCK, 0, kmcf_setup_stream(c)>>>(Na, t->d_atom_site, d_site_x, d_site_y, d_site_z, t->d_ax, t->d_ay, t->d_az);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipStreamSynchronize(kmcf_setup_stream(c)));
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipStreamSynchronize(c->stream));
    std::vector<double> *got[3] = {&xyz->x, &xyz->y, &xyz->z};
    const double *dev[3] = {t->d_ax, t->d_ay, t->d_az};
    for (int q = 0; q < 3; ++q) {
        got[q]->resize((size_t)Na);
        KMCF_HIP(hipMemcpy(got[q]->data(), dev[q], (size_t)Na * sizeof(double), hipMemcpyDeviceToHost));
    }
    // what the gather kernel read must be what a synchronous copy of the caller's arrays reads (the failure this
    // guards against built a pattern from coordinates whose y and z were still zero: silently)
    std::vector<double> sx((size_t)N);
    const double *src[3] = {d_site_x, d_site_y, d_site_z};
    for (int q = 0; q < 3; ++q) {
        KMCF_HIP(hipMemcpy(sx.data(), src[q], (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
        for (int a = 0; a < Na; ++a)
            KMCF_CHECK(memcmp(&(*got[q])[(size_t)a], &sx[(size_t)t->h_atom_site[(size_t)a]], sizeof(double)) == 0, KMCF_ERR_STATE,
                       "kmcf_initialize_sparsity_T: the gather kernel does not see the site coordinates the host copy sees (atom %d, "
                       "coordinate %d: %.17g against %.17g): an upload of the caller's arrays has not completed for this stream -- "
                       "upload from pinned memory, or synchronise the upload's stream, before the call", a, q, (*got[q])[(size_t)a],
                       sx[(size_t)t->h_atom_site[(size_t)a]]);
    }
    return KMCF_OK;
}

// atom-atom pattern of the atom rows [a0, a1) (calc_nnz_per_row_T / assemble_T_col_indices, "direct terms",
// src/initialize_sparsity_T.cu:62-72, 166-177; the diagonal comes with it: dist 0 < nn_dist)
static int init_atom_pattern(kmcf_tstate *t, int a0, int a1, std::vector<int> *arp, std::vector<int> *acol)
{
    // Open: no lattice (the periods are never read).  Periodic: the wrapped grid where at least 3 cells of nn_dist fit
    // each period and the atoms do not span one, else every pair is tested (host_cells::usable, kmcf_cells.hpp).
    host_cells hc;
    const double open_lattice[3] = {1, 1, 1};
    const double *lattice = t->pbc ? t->lattice : open_lattice;
    KMCF_TRY(build_cells(t->d_ax, t->d_ay, t->d_az, t->N_atom, lattice, t->pbc, t->nn_dist, &hc));
    const int rc = build_pattern(hc, t->d_ax, t->d_ay, t->d_az, lattice, t->pbc, t->nn_dist, a0, a1 - a0, 0, t->N_atom - 1, arp, acol, t->comm->stream);
    hc.release();
    return rc;
}

// rows [row0, row0 + n_loc) with GLOBAL columns (src/initialize_sparsity_T.cu:27-60, 126-164): the two virtual nodes'
// rows, and the atom rows out of the atom-atom pattern (atom a is row a + 2; arp / acol start at atom a0)
static int init_rows(kmcf_tstate *t, int row0, int n_loc, int a0, const std::vector<int> &arp, const std::vector<int> &acol)
{
    const int Nsub = t->Nsub, num_source_inj = t->n_inj, num_ground_ext = t->n_ext;
    std::vector<int> &rp = t->h_row_ptr, &col = t->h_col;
    rp.assign((size_t)n_loc + 1, 0);
    col.clear();
    for (int r = 0; r < n_loc; ++r) {
        const int i = row0 + r;
        if (i == 0) {
            col.push_back(0); col.push_back(1);
            for (int j = std::max(2, (Nsub + 1) - num_ground_ext + 1); j < Nsub; ++j) col.push_back(j);      // :37
        } else if (i == 1) {
            col.push_back(0); col.push_back(1);
            for (int j = 2; j < std::min(num_source_inj + 2, Nsub); ++j) col.push_back(j);                  // :42
        } else {
            if (i > (Nsub + 1) - num_ground_ext) col.push_back(0);                                           // :51
            if (i < num_source_inj + 2) col.push_back(1);                                                    // :56
            const int ar = i - 2 - a0;
            for (int q = arp[ar]; q < arp[ar + 1]; ++q) col.push_back(acol[q] + 2);
        }
        KMCF_CHECK(col.size() < (size_t)INT32_MAX, KMCF_ERR_ARG, "kmcf_initialize_sparsity_T: pattern exceeds int32 indexing");
        rp[r + 1] = (int)col.size();
    }
    return KMCF_OK;
}

// internal row order: virtual nodes first, atoms in bricks like K (kmcf_kstate.hip); long rows are moved behind by the
// matrix builder.  Empty: the caller's order.
static std::vector<int> init_brick_order(const kmcf_comm *c, int row0, int n_loc, const t_host_coords &xyz)
{
    std::vector<int> perm;
    const double edge = kmcf_brick_edge(c);
    if (!(edge > 0 && n_loc > 1)) return perm;
    std::vector<int64_t> key((size_t)n_loc);
    for (int r = 0; r < n_loc; ++r) {
        const int i = row0 + r;
        if (i < 2) { key[r] = -1; continue; }
        const int a = i - 2;
        const int64_t bx = (int64_t)std::floor(xyz.x[a] / edge) + (1 << 19), by = (int64_t)std::floor(xyz.y[a] / edge) + (1 << 19),
                      bz = (int64_t)std::floor(xyz.z[a] / edge) + (1 << 19);
        key[r] = (by << 42) | (bz << 21) | bx;
    }
    perm.resize((size_t)n_loc);
    for (int r = 0; r < n_loc; ++r) perm[r] = r;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return key[a] < key[b]; });
    return perm;
}

// per internal row: caller row, diagonal position, ground flag; per internal column: global node
static int init_row_tables(kmcf_tstate *t, const t_host_coords &xyz)
{
    kmcf_matrix *m = t->T;
    const int n_loc = m->n_loc, row0 = m->row0, Na = t->N_atom;
    const std::vector<int> &rp = t->h_row_ptr, &col = t->h_col;
    std::vector<int> iperm((size_t)n_loc);                      // internal -> caller local row
    for (int i = 0; i < n_loc; ++i) iperm[i] = m->h_perm.empty() ? i : m->h_perm[i];
    t->h_inv_perm.assign((size_t)n_loc, 0);
    for (int i = 0; i < n_loc; ++i) t->h_inv_perm[iperm[i]] = i;
    std::vector<int> diag_pos((size_t)n_loc, -1), col_node((size_t)n_loc + m->n_halo);
    std::vector<unsigned char> ground((size_t)n_loc, 0);
    std::vector<int> halo_gid((size_t)m->n_halo);
    if (m->n_halo > 0) KMCF_HIP(hipMemcpy(halo_gid.data(), m->d_halo_gid, (size_t)m->n_halo * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_loc; ++i) {
        const int r = iperm[i], node = row0 + r;
        col_node[i] = node;
        for (int j = rp[r]; j < rp[r + 1]; ++j)
            if (col[j] == node) { diag_pos[i] = m->h_row_ptr[i] + (j - rp[r]); break; }
        if (node >= 2) {
            const int a = node - 2, g = Na - 1;
            double dx = xyz.x[g] - xyz.x[a], dy = xyz.y[g] - xyz.y[a], dz = xyz.z[g] - xyz.z[a];
            if (t->pbc) {      // kmcf_min_image_dist restated on the host, operation for operation (the squares remove dx's sign)
                double fy = (xyz.y[g] - xyz.y[a]) / t->lattice[1], fz = (xyz.z[g] - xyz.z[a]) / t->lattice[2];
                fy -= std::round(fy); fz -= std::round(fz);
                dy = fy * t->lattice[1]; dz = fz * t->lattice[2];
            }
            ground[i] = std::sqrt(dx * dx + dy * dy + dz * dz) < t->nn_dist ? 1 : 0;      // current_solver_gpu.cu:1115-1117
        }
    }
    for (int h = 0; h < m->n_halo; ++h) col_node[(size_t)n_loc + h] = halo_gid[h];
    KMCF_TRY(upload(&t->d_diag_pos, diag_pos));
    KMCF_TRY(upload(&t->d_ground, ground));
    KMCF_TRY(upload(&t->d_col_node, col_node));
    KMCF_TRY(upload(&t->d_inv_perm, t->h_inv_perm));
    return KMCF_OK;
}

template <typename T>
static int pinned_zeroed(T **h, size_t n)
{
    KMCF_HIP(hipHostMalloc(reinterpret_cast<void **>(h), n * sizeof(T), hipHostMallocDefault));
    memset(*h, 0, n * sizeof(T));
    return KMCF_OK;
}

// what an assembly, the power pass and kmcf_current_map write besides the matrix (the block's own buffers grow per assembly)
static int init_workspace(kmcf_tstate *t, const int *h_counts_T, const int *h_displs_T)
{
    const kmcf_matrix *m = t->T;
    const int n_loc = m->n_loc, Na = t->N_atom, Nsub = t->Nsub, P = t->comm->nranks;
    const size_t na = (size_t)Na, nl1 = (size_t)std::max(n_loc, 1);     // (a rank may hold no row)
    KMCF_TRY(kmcf_dev_alloc(&t->d_cls_col, std::max<size_t>((size_t)n_loc + m->n_halo, 1), true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_diag, nl1, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_diag_tot, nl1, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_rhs, (size_t)n_loc + 2, true, t->comm->stream));
    // tunnel workspace sized by the atom count
    const int nblk = (Na + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE;
    KMCF_TRY(kmcf_dev_alloc(&t->d_blk, (size_t)2 * nblk + 2, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_tidx, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_tinfo, na, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_tx, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_ty, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_tz, na, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_tcb, na, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_pdisp, (size_t)Nsub + 2, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_scal, 4, true, t->comm->stream));
    KMCF_TRY(kmcf_dev_alloc(&t->d_err, 1, true, t->comm->stream));
    KMCF_TRY(pinned_zeroed(&t->h_pin, 1));
    KMCF_TRY(kmcf_dev_alloc(&t->d_agree, (size_t)2 * P, true, t->comm->stream));
    KMCF_TRY(pinned_zeroed(&t->h_agree, (size_t)(2 + 2 * P)));
    t->sub.counts.assign(P, 0);
    t->sub.displs.assign(P, 0);
    // scratch of kmcf_current_map (here, not at its first call: no allocation between the exchanges of a group)
    KMCF_CHECK((int64_t)3 * (Nsub + 2) < (int64_t)INT32_MAX, KMCF_ERR_ARG, "kmcf_initialize_sparsity_T: %d atoms exceed int32 indexing", Na);
    KMCF_TRY(kmcf_dev_alloc(&t->d_cmap, (size_t)3 * (Nsub + 2), true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_cmstat, 8, true, t->comm->stream));
    KMCF_TRY(pinned_zeroed(&t->h_cmstat, 8));
    t->cm_counts.resize((size_t)P); t->cm_displs.resize((size_t)P);
    for (int q = 0; q < P; ++q) { t->cm_counts[q] = 3 * h_counts_T[q]; t->cm_displs[q] = 3 * h_displs_T[q]; }
    // scratch of kmcf_current_profile (the profile itself is sized by the call: grown at its very start)
    if ((int64_t)CP_STRIDE * (Nsub + 2) < (int64_t)INT32_MAX) {
        KMCF_TRY(kmcf_dev_alloc(&t->d_cprof, (size_t)CP_STRIDE * (Nsub + 2), true, t->comm->stream));
        KMCF_TRY(kmcf_dev_alloc(&t->d_cpq, na, true, t->comm->stream)); KMCF_TRY(kmcf_dev_alloc(&t->d_cpcell, na, true, t->comm->stream));
        KMCF_TRY(kmcf_dev_alloc(&t->d_cpplanes, (size_t)CP_MAX, true, t->comm->stream));
        KMCF_TRY(pinned_zeroed(&t->h_cpplanes, (size_t)CP_MAX));
        t->cp_counts.resize((size_t)P); t->cp_displs.resize((size_t)P);
        for (int q = 0; q < P; ++q) { t->cp_counts[q] = CP_STRIDE * h_counts_T[q]; t->cp_displs[q] = CP_STRIDE * h_displs_T[q]; }
    }
    KMCF_HIP(hipStreamSynchronize(t->comm->stream));      // (the fills on the compute stream: done before any stream uses the workspace)
    return KMCF_OK;
}

// both entry points: h_lattice is read with pbc == 1 only (checked by the caller)
static int initialize_sparsity_T(kmcf_comm *c, const double *d_site_x, const double *d_site_y, const double *d_site_z,
                                 const int *d_site_element, int N, const double *h_lattice, int pbc, double nn_dist, int num_source_inj,
                                 int num_ground_ext, int num_layers_contact, const int *h_counts_T,
                                 const int *h_displs_T, kmcf_tstate **out)
{
    KMCF_TRY(init_check_args(c, d_site_x, d_site_y, d_site_z, d_site_element, N, nn_dist, num_source_inj, num_ground_ext,
                             num_layers_contact, h_counts_T, h_displs_T, out));
    KMCF_TRY(kmcf_enter(c));
    KMCF_HIP(hipStreamSynchronize(c->stream));
    kmcf_tstate *t = new kmcf_tstate();
    struct guard_t { kmcf_tstate *t; ~guard_t() { if (t) kmcf_tstate_destroy(t); } } guard{t};      // (a half-built state)
    t->comm = c; t->N = N; t->n_inj = num_source_inj; t->n_ext = num_ground_ext; t->n_layers = num_layers_contact;
    t->nn_dist = nn_dist;
    t->pbc = pbc;
    if (pbc) memcpy(t->lattice, h_lattice, sizeof(t->lattice));
    KMCF_TRY(init_atom_set(t, d_site_element, h_counts_T));
    t_host_coords xyz;
    KMCF_TRY(init_gather_coords(t, d_site_x, d_site_y, d_site_z, &xyz));
    const int n_loc = h_counts_T[c->rank], row0 = h_displs_T[c->rank];
    const int a0 = std::max(row0, 2) - 2, a1 = std::max(row0 + n_loc, 2) - 2;      // atoms [a0, a1) = rows [a0 + 2, a1 + 2)
    std::vector<int> arp, acol;
    KMCF_TRY(init_atom_pattern(t, a0, a1, &arp, &acol));
    KMCF_TRY(init_rows(t, row0, n_loc, a0, arp, acol));
    const std::vector<int> perm = init_brick_order(c, row0, n_loc, xyz);
    KMCF_TRY(kmcf_matrix_build(c, t->Nsub, h_counts_T, h_displs_T, t->h_row_ptr.data(), t->h_col.data(), nullptr,
                               perm.empty() ? nullptr : perm.data(), &t->T));
    KMCF_TRY(init_row_tables(t, xyz));
    KMCF_TRY(init_workspace(t, h_counts_T, h_displs_T));
    guard.t = nullptr;
    *out = t;
    return KMCF_OK;
}

extern "C" int kmcf_initialize_sparsity_T(kmcf_comm *c, const double *d_site_x, const double *d_site_y, const double *d_site_z,
                                          const int *d_site_element, int N, double nn_dist, int num_source_inj,
                                          int num_ground_ext, int num_layers_contact, const int *h_counts_T,
                                          const int *h_displs_T, kmcf_tstate **out)
{
    return initialize_sparsity_T(c, d_site_x, d_site_y, d_site_z, d_site_element, N, nullptr, 0, nn_dist, num_source_inj, num_ground_ext,
                                 num_layers_contact, h_counts_T, h_displs_T, out);
}

extern "C" int kmcf_initialize_sparsity_T_pbc(kmcf_comm *c, const double *d_site_x, const double *d_site_y, const double *d_site_z,
                                              const int *d_site_element, int N, const double *h_lattice, int pbc, double nn_dist,
                                              int num_source_inj, int num_ground_ext, int num_layers_contact, const int *h_counts_T,
                                              const int *h_displs_T, kmcf_tstate **out)
{
    const char *what = "kmcf_initialize_sparsity_T_pbc";
    KMCF_CHECK(pbc == 0 || pbc == 1, KMCF_ERR_ARG, "%s: pbc = %d is neither 0 nor 1", what, pbc);
    if (pbc) {
        KMCF_CHECK(h_lattice, KMCF_ERR_ARG, "%s: h_lattice is NULL with pbc = 1", what);
        KMCF_CHECK(std::isfinite(h_lattice[1]) && h_lattice[1] > 0, KMCF_ERR_ARG, "%s: the period in y, h_lattice[1] = %g, is not finite and > 0",
                   what, h_lattice[1]);
        KMCF_CHECK(std::isfinite(h_lattice[2]) && h_lattice[2] > 0, KMCF_ERR_ARG, "%s: the period in z, h_lattice[2] = %g, is not finite and > 0",
                   what, h_lattice[2]);
    }
    return initialize_sparsity_T(c, d_site_x, d_site_y, d_site_z, d_site_element, N, h_lattice, pbc, nn_dist, num_source_inj, num_ground_ext,
                                 num_layers_contact, h_counts_T, h_displs_T, out);
}

extern "C" int kmcf_tstate_periodic(const kmcf_tstate *t, int *pbc, double *h_lattice)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_tstate_periodic: t is NULL");
    KMCF_CHECK(pbc, KMCF_ERR_ARG, "kmcf_tstate_periodic: pbc is NULL");
    *pbc = t->pbc;
    if (h_lattice) memcpy(h_lattice, t->lattice, sizeof(t->lattice));
    return KMCF_OK;
}

// bytes this rank holds of the block's matrix, per storage form
static int64_t tunnel_bytes(const kmcf_subop &sb)
{
    if (sb.jagged) return (int64_t)sb.jnnz * 8 + (int64_t)sb.n_tiles * 520;          // values + 64 masks and an offset per tile
    if (sb.dense) return (int64_t)sb.n_tiles * 4096 * 8;                             // (spread: this rank's tiles)
    return (int64_t)sb.nnz * 8 + (int64_t)sb.n_loc * ((sb.n_glob + 63) / 64) * 8;    // packed values + bitmap
}

extern "C" int kmcf_tstate_info(const kmcf_tstate *t, kmcf_tstate_info_t *info)
{
    KMCF_CHECK(t && info, KMCF_ERR_ARG, "kmcf_tstate_info: null argument");
    info->N_atom = t->N_atom;
    info->Nsub = t->Nsub;
    info->rows_this_rank = t->T->n_loc;
    info->nnz_neighbour = t->T->nnz;
    info->tunnel_points = t->assembled ? t->sub.n_glob : 0;
    info->tunnel_points_rank = t->assembled ? t->sub.n_loc : 0;
    info->tunnel_first = t->assembled ? t->sub.row0 : 0;
    info->nnz_tunnel = t->assembled ? t->sub.nnz : 0;
    info->tunnel_dense = t->assembled && t->sub.dense ? (t->sub.jagged ? 2 : 1) : 0;
    info->tunnel_bytes = t->assembled ? tunnel_bytes(t->sub) : 0;
    return KMCF_OK;
}

extern "C" int kmcf_tstate_pattern(const kmcf_tstate *t, int *h_row_ptr, int *h_col, int64_t *nnz)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_tstate_pattern: null state");
    if (nnz) *nnz = (int64_t)t->h_col.size();
    if (h_row_ptr) memcpy(h_row_ptr, t->h_row_ptr.data(), t->h_row_ptr.size() * sizeof(int));
    if (h_col && !t->h_col.empty()) memcpy(h_col, t->h_col.data(), t->h_col.size() * sizeof(int));
    return KMCF_OK;
}

extern "C" int kmcf_tstate_atom_sites(const kmcf_tstate *t, int *h_atom_site)
{
    KMCF_CHECK(t && h_atom_site, KMCF_ERR_ARG, "kmcf_tstate_atom_sites: null argument");
    memcpy(h_atom_site, t->h_atom_site.data(), t->h_atom_site.size() * sizeof(int));
    return KMCF_OK;
}

// ---------------------------------------------------------------- the tile forms: one application
// launches of the dense symmetric operator (dynamic LDS beyond 64 KB needs the attribute once per kernel)
template <int MODE>
static int symm_launch(kmcf_subop &sb, const double *x, double Vd, hipStream_t st, const kmcf_scalars *S = nullptr, int check_done = 0)
{
    // (the attribute is set per launch: it is per device, and in-process groups launch from several host threads)
    const size_t lds = (size_t)4 * SYM_WAVE_DOUBLES * sizeof(double);
    const int grid = strip_grid(sb.n_strips);
    if (sb.jagged) {
        KMCF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sub_symj_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        sub_symj_kernel<MODE><<<grid, KMCF_BLOCK, lds, st>>>(sb.n_strips, sb.d_strips, sb.d_jmask, sb.d_jvoff, sb.d_jval, x, Vd, sb.d_rowpart, sb.d_colpart,
                                                             S, check_done);
        KMCF_HIP(hipGetLastError());
        return KMCF_OK;
    }
    KMCF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sub_symm_kernel<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    sub_symm_kernel<MODE><<<grid, KMCF_BLOCK, lds, st>>>(sb.n_strips, sb.d_strips, sb.d_tiles, x, Vd, sb.d_rowpart, sb.d_colpart, S, check_done);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// Spread storage: this rank's partial sums -> every rank's partials (one all-gather on the compute stream) -> the sums
// of the ns points from row0 on, added in rank order (MODE / DOT / rows / y / y2 / part as in sub_symm_reduce_kernel).
// Every rank of the group calls it, also one without points of its own (ns == 0): it holds strips like the others.
template <int MODE, bool DOT>
static int symm_spread_finish(kmcf_comm *c, kmcf_subop &sb, int ns, int row0, const int *rows, const double *p, double *y, double *y2,
                              double *part, const kmcf_scalars *S, int chk)
{
    hipStream_t st = c->stream;
    constexpr int W = MODE == 0 ? 1 : 2;
    const int P = c->nranks, npad = 64 * sb.nb;
    sub_symm_reduce_kernel<MODE, false><<<sb.nb, KMCF_BLOCK, 0, st>>>(sb.n_glob, sb.nb, sb.d_strip_first, sb.d_rowpart, sb.d_colpart, nullptr, nullptr,
                                                                      nullptr, nullptr, nullptr, S, chk, sb.d_tile_local,
                                                                      sb.d_ypart + (size_t)c->rank * W * npad);
    KMCF_HIP(hipGetLastError());
    KMCF_TRY(kmcf_comm_allgatherv_double(c, sb.d_ypart, sb.y_counts[W - 1].data(), sb.y_displs[W - 1].data()));
    if (ns > 0) {
        sub_combine_kernel<MODE, DOT><<<(ns + KMCF_BLOCK - 1) / KMCF_BLOCK, KMCF_BLOCK, 0, st>>>(ns, row0, P, npad, sb.d_ypart, rows, p, y, y2, part, S, chk);
        KMCF_HIP(hipGetLastError());
    }
    return KMCF_OK;
}

// Who applies the tiles: every rank of a group that deals them (also one without points of its own), one rank only
// with points of its own.
static bool symm_applies(const kmcf_subop &sb) { return sb.dense && (sb.spread || sb.n_loc > 0); }

// One application of the tiles to sb.d_xsub: the tile kernel, then the parts added per block row (one rank) or per
// rank, gathered and combined (group).  MODE 0: y[rows[i]] += the sums of points row0 ... row0 + ns (rows == nullptr:
// y[i]), DOT: with the p.Ap partials into part; MODE 1 (the power pass, bias Vd): into y and y2.
template <int MODE, bool DOT>
static int symm_apply(kmcf_comm *c, kmcf_subop &sb, int ns, int row0, const int *rows, const double *p, double *y, double *y2,
                      double *part, const kmcf_scalars *S, int chk, double Vd = 0.0)
{
    KMCF_TRY(symm_launch<MODE>(sb, sb.d_xsub, Vd, c->stream, S, chk));
    if (sb.spread) return symm_spread_finish<MODE, DOT>(c, sb, ns, row0, rows, p, y, y2, part, S, chk);
    sub_symm_reduce_kernel<MODE, DOT><<<sb.nb, KMCF_BLOCK, 0, c->stream>>>(sb.n_glob, sb.nb, sb.d_strip_first, sb.d_rowpart, sb.d_colpart, rows, p,
                                                                           y, y2, part, S, chk);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// ---------------------------------------------------------------- the tile forms: setup (after the tunnel points are known)
// strips of one rank, or (sb.spread) this rank's share of a group's: dealt, uploaded, their buffers sized
static int symm_deal_upload(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    kmcf_comm *c = t->comm;
    hipStream_t st = c->stream;
    const int nb = sb.nb = (sb.n_glob + 63) / 64;
    const int P = sb.spread ? c->nranks : 1, rank = sb.spread ? c->rank : 0;
    sb.n_tiles_glob = (long long)nb * (nb + 1) / 2;
    KMCF_CHECK(sb.n_tiles_glob < (long long)INT32_MAX, KMCF_ERR_ARG, "tunnel block of %d points: tile index exceeds int32", sb.n_glob);
    const kmcf_strip_deal deal = kmcf_deal_strips(nb, std::max(1, kmcf_opt_int(c, KNOB_SUB_STRIP, 16)), P, rank, sb.spread);
    sb.n_tiles = deal.n_tiles;
    sb.n_strips = (int)deal.strips.size();
    if (!sb.jagged) KMCF_TRY(ensure(&sb.d_tiles, &sb.cap_tiles, (size_t)std::max<long long>(sb.n_tiles, 1) * 4096));
    KMCF_TRY(ensure(&sb.d_strips, &sb.cap_strips, deal.strips.size() + 1));
    KMCF_TRY(ensure(&sb.d_strip_first, &sb.cap_sf, deal.first.size()));
    KMCF_TRY(ensure(&sb.d_rowpart, &sb.cap_rowpart, (size_t)(sb.n_strips + 1) * 128));
    KMCF_TRY(ensure(&sb.d_colpart, &sb.cap_colpart, (size_t)std::max<long long>(sb.n_tiles, 1) * 128));
    if (!deal.strips.empty())
        KMCF_HIP(hipMemcpyAsync(sb.d_strips, deal.strips.data(), deal.strips.size() * sizeof(kmcf_strip), hipMemcpyHostToDevice, st));
    KMCF_HIP(hipMemcpyAsync(sb.d_strip_first, deal.first.data(), deal.first.size() * sizeof(int), hipMemcpyHostToDevice, st));
    if (sb.spread) {
        KMCF_TRY(ensure(&sb.d_tile_local, &sb.cap_tile_local, deal.tile_local.size() + 1));
        KMCF_TRY(ensure(&sb.d_ypart, &sb.cap_ypart, (size_t)2 * P * 64 * nb));
        KMCF_HIP(hipMemcpyAsync(sb.d_tile_local, deal.tile_local.data(), deal.tile_local.size() * sizeof(int), hipMemcpyHostToDevice, st));
        for (int w = 1; w <= 2; ++w) {                              // slices of the partials' all-gather: one / two sums per point
            sb.y_counts[w - 1].assign((size_t)P, w * 64 * nb);
            sb.y_displs[w - 1].resize((size_t)P);
            for (int q = 0; q < P; ++q) sb.y_displs[w - 1][q] = q * w * 64 * nb;
        }
    }
    KMCF_HIP(hipStreamSynchronize(st));                            // (the deal goes out of scope)
    return KMCF_OK;
}

// jagged tiles: masks tile-major, entries per tile -> first value of every tile -> values in layer order
static int symm_fill_jagged(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    hipStream_t st = t->comm->stream;
    const int grid = strip_grid(sb.n_strips);
    KMCF_TRY(ensure(&sb.d_jmask, &sb.cap_jmask, (size_t)sb.n_tiles * 64));
    KMCF_TRY(ensure(&sb.d_jcnt, &sb.cap_jcnt, (size_t)sb.n_tiles + 1));
    KMCF_TRY(ensure(&sb.d_jvoff, &sb.cap_jvoff, (size_t)sb.n_tiles + 2));
    symj_mask_kernel<<<grid, KMCF_BLOCK, 0, st>>>(sb.n_strips, sb.d_strips, sb.n_glob, sb.n_groups, sb.d_mask, sb.d_jmask, sb.d_jcnt);
    // (a tile holds at most 4096 entries: the 256 counts of one pass of the scan add up to 2^20 at most)
    kmcf_scan_counts_kernel<long long><<<1, KMCF_BLOCK, 0, st>>>((int)sb.n_tiles, sb.d_jcnt, sb.d_jvoff, 0);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(&t->h_pin->jnnz, sb.d_jvoff + sb.n_tiles, sizeof(long long), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipStreamSynchronize(st));
    sb.jnnz = t->h_pin->jnnz;
    KMCF_TRY(ensure(&sb.d_jval, &sb.cap_jval, (size_t)sb.jnnz + 64));
    with_dist(t, [&](auto dist) {
        symj_fill_kernel<decltype(dist)><<<grid, KMCF_BLOCK, 0, st>>>(sb.n_strips, sb.d_strips, sb.n_glob, points_of(t), wkb_of(t), sb.d_jmask, sb.d_jvoff,
                                                                      sb.d_jval, dist);
    });
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

static int symm_fill_dense(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    with_dist(t, [&](auto dist) {
        tunnel_dense_fill_kernel<decltype(dist)><<<strip_grid(sb.n_strips), KMCF_BLOCK, 0, t->comm->stream>>>(sb.n_strips, sb.d_strips, sb.n_glob, points_of(t),
                                                                                                             wkb_of(t), sb.d_tiles, dist);
    });
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// diagonal = -(row sums) of the tile forms, of ALL points on every rank when the tiles are spread (a rank sets the diagonal
// of the diagonal tiles it holds).  TWO algorithms, by the state's geometry:
//   open state:     one application of the tiles to the vector of ones (the diagonal entries are still 0); a group adds the
//                   ranks' partial sums in rank order, so the last bit of a sum depends on the deal.  The bytes
//                   of this library's open path before periodic states existed: kept.
//   periodic state: tunnel_rowsum_kernel over this rank's rows of the pair bitmap, a group all-gathering the rows' sums:
//                   a second evaluation of every pair's WKB value (5 nm: 34 us), for a diagonal that is the one-rank
//                   bitmap's in every form and under every deal.
static int symm_diagonal(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    hipStream_t st = t->comm->stream;
    const int n_t = sb.n_glob, nb = sb.nb;
    if (t->pbc) {
        if (sb.n_loc > 0)
            tunnel_rowsum_kernel<dist_min_image><<<wave_row_grid(sb.n_loc), KMCF_BLOCK, 0, st>>>(
                sb.n_loc, sb.row0, sb.n_groups, points_of(t), wkb_of(t), sb.d_mask, t->d_tdiag, dist_min_image{t->lattice[1], t->lattice[2]});
        KMCF_HIP(hipGetLastError());
        if (sb.spread) KMCF_TRY(kmcf_comm_allgatherv_double(t->comm, t->d_tdiag, sb.counts.data(), sb.displs.data()));
    } else {
        fill_kernel<<<kmcf_grid1d(64 * nb), KMCF_BLOCK, 0, st>>>(64 * nb, sb.d_xsub, 1.0);
        KMCF_HIP(hipMemsetAsync(t->d_tdiag, 0, (size_t)n_t * sizeof(double), st));
        KMCF_TRY((symm_apply<0, false>(t->comm, sb, n_t, 0, nullptr, nullptr, t->d_tdiag, nullptr, nullptr, nullptr, 0)));
    }
    if (sb.jagged) symj_set_diag_kernel<<<std::max(1, (nb + 3) / 4), KMCF_BLOCK, 0, st>>>(n_t, nb, t->d_tdiag, t->d_tdiag, sb.d_jmask, sb.d_jvoff, sb.d_jval);
    else symm_set_diag_kernel<<<kmcf_grid1d(n_t), KMCF_BLOCK, 0, st>>>(n_t, nb, t->d_tdiag, t->d_tdiag, sb.d_tiles, sb.spread ? sb.d_tile_local : nullptr);
    KMCF_HIP(hipMemsetAsync(sb.d_xsub, 0, (size_t)64 * nb * sizeof(double), st));      // the pad behind the last point stays 0
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

static int symm_setup(kmcf_tstate *t)
{
    KMCF_TRY(symm_deal_upload(t));
    KMCF_TRY(t->sub.jagged ? symm_fill_jagged(t) : symm_fill_dense(t));
    return symm_diagonal(t);
}

// ---------------------------------------------------------------- one assembly, stage by stage (t->par holds the parameters)
// 1. atom arrays (update_atom_arrays, :1341-1365) + invariance of the atom set (the verdict is read in stage 3)
static int asm_atoms(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge, const double *d_site_CB_edge,
                     const int *d_metals, int num_metals)
{
    hipStream_t st = t->comm->stream;
    const int Na = t->N_atom;
    KMCF_HIP(hipMemsetAsync(t->d_err, 0, sizeof(int), st));
    check_atom_set_kernel<<<kmcf_grid1d(t->N), KMCF_BLOCK, 0, st>>>(t->N, d_site_element, t->d_site_is_atom, t->d_err);
    gather_atoms_kernel<<<kmcf_grid1d(Na), KMCF_BLOCK, 0, st>>>(Na, t->d_atom_site, d_site_element, d_site_charge, d_site_CB_edge, d_metals,
                                                           num_metals, t->d_ael, t->d_ach, t->d_acb, t->d_acls);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// 2. neighbour values + their diagonal (one pass), the dictionary of the coded SpMV
static int asm_neighbour_values(kmcf_tstate *t)
{
    kmcf_matrix *m = t->T;
    hipStream_t st = t->comm->stream;
    const kmcf_current_params_t *p = &t->par;
    const int n_loc = m->n_loc, n_cols = n_loc + m->n_halo;
    if (n_loc == 0) return KMCF_OK;
    t_cls_col_kernel<<<kmcf_grid1d(n_cols), KMCF_BLOCK, 0, st>>>(n_cols, t->d_col_node, t->d_acls, t->d_cls_col);
    const double dict[3] = {-p->high_G, -p->low_G, -p->loop_G};
    KMCF_TRY(kmcf_matrix_set_dictionary(m, dict, 3));
    constexpr int LPR = 16;
    t_assemble_kernel<LPR><<<kmcf_grid1d((int64_t)n_loc * LPR), KMCF_BLOCK, 0, st>>>(
        n_loc, m->d_row_ptr, m->d_col, m->d_val, t->d_diag_pos, t->d_ground, t->d_cls_col, p->high_G, p->low_G, p->loop_G,
        t->d_diag, m->coded ? m->d_idx16 : nullptr, m->coded ? m->d_diagv : nullptr, m->n_short);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// 3. tunnel points of all ranks (get_is_tunnel_mpi + copy_if + MPI_Allgatherv, initialize_sparsity_T.cu:739-787): count,
// scan, scatter; the one synchronising read-back (their number, the atom-set verdict); their atom indices on the host
static int asm_tunnel_points(kmcf_tstate *t, const int *d_metals, int num_metals)
{
    hipStream_t st = t->comm->stream;
    const kmcf_current_params_t *p = &t->par;
    const int Na = t->N_atom;
    const int n_scan = Na - 1;                                        // atoms 0 .. N_atom - 2 are matrix rows
    const int nblk = (Na + KMCF_SCAN_TILE - 1) / KMCF_SCAN_TILE;
    tunnel_count_kernel<<<nblk, KMCF_BLOCK, 0, st>>>(n_scan, t->d_ael, t->d_ax, p->contact_x_lo, p->contact_x_hi, t->d_blk);
    kmcf_scan_counts_kernel<int><<<1, KMCF_BLOCK, 0, st>>>(nblk, t->d_blk, t->d_blk + nblk, 0);
    tunnel_scatter_kernel<<<nblk, KMCF_BLOCK, 0, st>>>(n_scan, Na, t->d_ael, t->d_ax, t->d_ay, t->d_az, t->d_acb, d_metals, num_metals,
                                                       p->contact_x_lo, p->contact_x_hi, t->n_layers, t->n_inj, t->n_ext, t->d_blk + nblk,
                                                       t->d_tidx, t->d_tinfo, t->d_tx, t->d_ty, t->d_tz, t->d_tcb);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(&t->h_pin->n_t, t->d_blk + 2 * nblk, sizeof(int), hipMemcpyDeviceToHost, st));   // total = n_t
    KMCF_HIP(hipMemcpyAsync(&t->h_pin->err, t->d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipStreamSynchronize(st));
    KMCF_CHECK(t->h_pin->err == 0, KMCF_ERR_STATE,
               "kmcf_t_assemble: the set of atom sites differs from the one at kmcf_initialize_sparsity_T (call it again)");
    const int n_t = t->h_pin->n_t;
    t->h_tidx.resize((size_t)n_t);
    if (n_t > 0) KMCF_HIP(hipMemcpy(t->h_tidx.data(), t->d_tidx, (size_t)n_t * sizeof(int), hipMemcpyDeviceToHost));
    return KMCF_OK;
}

// 4. counts_subblock / displ_subblock (:752-758): tunnel points by owner of their matrix row (atom index + 2); the
// buffers sized by this rank's share; the storage form reset to the bitmap
static int asm_partition(kmcf_tstate *t)
{
    const kmcf_matrix *m = t->T;
    kmcf_subop &sb = t->sub;
    hipStream_t st = t->comm->stream;
    const int n_t = (int)t->h_tidx.size(), rank = t->comm->rank;
    for (int q = 0; q < t->comm->nranks; ++q) {
        const int lo = m->displs[q], hi = m->displs[q] + m->counts[q];
        const int b = (int)(std::lower_bound(t->h_tidx.begin(), t->h_tidx.end(), lo - 2) - t->h_tidx.begin());
        const int e = (int)(std::lower_bound(t->h_tidx.begin(), t->h_tidx.end(), hi - 2) - t->h_tidx.begin());
        sb.displs[q] = b;
        sb.counts[q] = e - b;
    }
    sb.n_glob = n_t;
    sb.n_loc = sb.counts[rank];
    sb.row0 = sb.displs[rank];
    sb.n_groups = (n_t + 63) / 64;
    sb.nnz = 0;
    const int ns = sb.n_loc, ng = sb.n_groups;
    KMCF_TRY(ensure(&sb.d_rows, &sb.cap_rows, (size_t)ns + 1));
    KMCF_TRY(ensure(&sb.d_voff, &sb.cap_voff, (size_t)ns + 2));
    KMCF_HIP(hipMemsetAsync(sb.d_voff, 0, ((size_t)ns + 2) * sizeof(long long), st));
    KMCF_TRY(ensure(&sb.d_mask, &sb.cap_mask, (size_t)ns * ng + 1));
    KMCF_TRY(ensure(&sb.d_xsub, &sb.cap_x, (size_t)n_t + 320));          // + 256: the 4-group unroll reads x_sub[j + 192] only when set
    KMCF_TRY(ensure(&t->d_rowcnt, &t->cap_rowcnt, (size_t)ns + 1));
    KMCF_TRY(ensure(&t->d_tdiag, &t->cap_tdiag, (size_t)n_t + 1));       // (per LOCAL point; the spread tiles: per point of all ranks)
    sb.dense = sb.jagged = sb.spread = false;
    return KMCF_OK;
}

// 5. the bitmap of this rank's rows (every form keeps it: the tiles are filled from it, kmcf_current_map walks it) and
// the scan of its row counts; the second synchronising read-back: the rows' entries
static int asm_bitmap_pattern(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    hipStream_t st = t->comm->stream;
    const int ns = sb.n_loc, n_t = sb.n_glob;
    if (ns == 0) return KMCF_OK;
    // a row holds at most n_t entries, and the scan adds the 256 counts of one pass in an int
    KMCF_CHECK((int64_t)n_t * KMCF_BLOCK <= (int64_t)INT32_MAX, KMCF_ERR_ARG,
               "tunnel block: %d tunnel points exceed the row-offset scan's range (256 rows of that many entries in an int)", n_t);
    sub_rows_kernel<<<kmcf_grid1d(ns), KMCF_BLOCK, 0, st>>>(ns, sb.row0, t->d_tidx, t->T->row0, t->d_inv_perm, sb.d_rows);
    with_dist(t, [&](auto dist) {
        tunnel_mask_kernel<decltype(dist)><<<wave_row_grid(ns), KMCF_BLOCK, 0, st>>>(ns, sb.row0, n_t, sb.n_groups, points_of(t), wkb_of(t), sb.d_mask,
                                                                                     t->d_rowcnt, dist);
    });
    kmcf_scan_counts_kernel<long long><<<1, KMCF_BLOCK, 0, st>>>(ns, t->d_rowcnt, sb.d_voff, 0);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(&t->h_pin->nnz, sb.d_voff + ns, sizeof(long long), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipStreamSynchronize(st));
    sb.nnz = t->h_pin->nnz;
    return KMCF_OK;
}

// 6. the storage form (the rule: kmcf_subplan.hpp).  A group votes: one all-gather of (entries of my rows, my share of
// the tiles fits), after which every rank decides alike.
static int asm_choose_storage(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    kmcf_comm *c = t->comm;
    hipStream_t st = c->stream;
    const int n_t = sb.n_glob, P = c->nranks;
    if (n_t == 0) return KMCF_OK;
    const char *env = kmcf_opt(c, KNOB_SUB_DENSE);
    const int override = env ? atoi(env) : KMCF_SUB_AUTO;
    auto free_bytes = [](size_t *fr) { size_t tot = 0; return hipMemGetInfo(fr, &tot) == hipSuccess; };
    if (P == 1) {
        const kmcf_sub_form f = kmcf_sub_form_one_rank(n_t, sb.nnz, sb.cap_tiles, sb.cap_jval, override, free_bytes);
        sb.dense = f.dense;
        sb.jagged = f.jagged;
        return KMCF_OK;
    }
    const kmcf_sub_vote vote = kmcf_sub_group_vote(n_t, P, sb.cap_tiles, override, free_bytes);
    if (vote == KMCF_SUB_NO_VOTE) return KMCF_OK;
    double *h_ag = t->h_agree;
    h_ag[0] = (double)sb.nnz; h_ag[1] = vote == KMCF_SUB_FITS ? 1.0 : 0.0;
    KMCF_HIP(hipMemcpyAsync(t->d_agree + 2 * c->rank, h_ag, 2 * sizeof(double), hipMemcpyHostToDevice, st));
    std::vector<int> cnt((size_t)P, 2), dsp((size_t)P);
    for (int q = 0; q < P; ++q) dsp[q] = 2 * q;
    KMCF_TRY(kmcf_comm_allgatherv_double(c, t->d_agree, cnt.data(), dsp.data()));
    KMCF_HIP(hipMemcpyAsync(h_ag + 2, t->d_agree, (size_t)2 * P * sizeof(double), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipStreamSynchronize(st));
    double nnz_all = 0.0;
    bool fit_all = true;
    for (int q = 0; q < P; ++q) { nnz_all += h_ag[2 + 2 * q]; fit_all = fit_all && h_ag[3 + 2 * q] != 0.0; }
    sb.dense = sb.spread = kmcf_sub_group_spread(n_t, sb.n_loc, nnz_all, fit_all, override);
    return KMCF_OK;
}

// 7. the values in the form chosen, the tunnel diagonal with them; the p.Ap partials of one application (sb.grid)
static int asm_values(kmcf_tstate *t)
{
    kmcf_subop &sb = t->sub;
    const int ns = sb.n_loc;
    if (sb.dense) {
        KMCF_TRY(symm_setup(t));
    } else if (ns > 0) {
        KMCF_TRY(ensure(&sb.d_val, &sb.cap_val, (size_t)sb.nnz + 64));
        with_dist(t, [&](auto dist) {
            tunnel_value_kernel<decltype(dist)><<<wave_row_grid(ns), KMCF_BLOCK, 0, t->comm->stream>>>(ns, sb.row0, sb.n_groups, points_of(t), wkb_of(t),
                                                                                                       sb.d_mask, sb.d_voff, sb.d_val, t->d_tdiag, dist);
        });
        KMCF_HIP(hipGetLastError());
    }
    sb.grid = sb.spread ? (ns + KMCF_BLOCK - 1) / KMCF_BLOCK : sb.dense ? sb.nb : ns > 0 ? wave_row_grid(ns) : 0;
    return KMCF_OK;
}

// 8. preconditioner and right-hand side
static int asm_precond_rhs(kmcf_tstate *t)
{
    kmcf_matrix *m = t->T;
    const kmcf_subop &sb = t->sub;
    hipStream_t st = t->comm->stream;
    const int n_loc = m->n_loc, ns = sb.n_loc;
    if (n_loc == 0) return KMCF_OK;
    copy_diag_rhs_kernel<<<kmcf_grid1d(n_loc), KMCF_BLOCK, 0, st>>>(n_loc, t->d_diag, t->d_diag_tot, t->d_col_node, t->par.loop_G * t->par.Vd, t->d_rhs);
    if (ns > 0) add_tunnel_diag_kernel<<<kmcf_grid1d(ns), KMCF_BLOCK, 0, st>>>(ns, sb.d_rows, t->d_tdiag + (sb.spread ? sb.row0 : 0), t->d_diag_tot);
    invert_kernel<<<kmcf_grid1d(n_loc), KMCF_BLOCK, 0, st>>>(n_loc, t->d_diag_tot, m->d_dinv);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

// (an error return from any stage leaves assembled == false)
static int t_assemble_async(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge, const double *d_site_CB_edge,
                            const int *d_metals, int num_metals, const kmcf_current_params_t *p)
{
    t->par = *p;
    t->assembled = false;
    KMCF_TRY(asm_atoms(t, d_site_element, d_site_charge, d_site_CB_edge, d_metals, num_metals));
    KMCF_TRY(asm_neighbour_values(t));
    KMCF_TRY(asm_tunnel_points(t, d_metals, num_metals));
    KMCF_TRY(asm_partition(t));
    KMCF_TRY(asm_bitmap_pattern(t));
    KMCF_TRY(asm_choose_storage(t));
    KMCF_TRY(asm_values(t));
    KMCF_TRY(asm_precond_rhs(t));
    t->T->sub = &t->sub;
    t->assembled = true;
    return KMCF_OK;
}

// Sub-block part of a split SpMV.  begin (called by kmcf_spmv_device BEFORE the CSR part): pack the local part of the
// sub-vector (pack_gpu, dist_spmv_split_sparse.cpp:29-33) and start gathering the rest (:36-48) -- for a group on RCCL
// or the peer-to-peer transport on the COMM stream, so that the exchange runs underneath the neighbour part
// (spmm_split_sparse2 / 3, :123-192, :246-337); finish (after the CSR part): wait for it, y[sub rows] += S x_sub.
int kmcf_subop_begin(kmcf_matrix *m, bool skip_if_done)
{
    kmcf_subop *sb = m->sub;
    kmcf_comm *c = m->comm;
    hipStream_t st = c->stream;
    sb->gather_pending = false;
    if (sb->n_glob == 0) return KMCF_OK;
    const int chk = skip_if_done ? 1 : 0;
    if (sb->n_loc > 0) {
        sub_pack_kernel<<<kmcf_grid1d(sb->n_loc), KMCF_BLOCK, 0, st>>>(sb->n_loc, sb->d_rows, m->d_p, sb->d_xsub + sb->row0, m->d_S, chk);
        KMCF_HIP(hipGetLastError());
    }
    if (c->nranks == 1 && !c->force_collectives) return KMCF_OK;
    if (c->p2p_active || (!c->group && c->nccl)) {
        KMCF_HIP(hipEventRecord(c->ev_subpack, st));
        KMCF_HIP(hipStreamWaitEvent(c->comm_stream, c->ev_subpack, 0));
        const int rc = kmcf_comm_allgatherv_double_comm_stream(c, sb->d_xsub, sb->counts.data(), sb->displs.data());
        if (rc == KMCF_OK) {
            KMCF_HIP(hipEventRecord(c->ev_sub, c->comm_stream));
            sb->gather_pending = true;
            return KMCF_OK;
        }
        if (rc != KMCF_ERR_STATE) return rc;
    }
    return kmcf_comm_allgatherv_double(c, sb->d_xsub, sb->counts.data(), sb->displs.data());     // in order, on the compute stream
}

int kmcf_subop_finish(kmcf_matrix *m, bool with_dot, bool skip_if_done)
{
    kmcf_subop *sb = m->sub;
    kmcf_comm *c = m->comm;
    hipStream_t st = c->stream;
    if (sb->n_glob == 0) return KMCF_OK;
    const int chk = skip_if_done ? 1 : 0;
    if (sb->gather_pending) {
        KMCF_HIP(hipStreamWaitEvent(st, c->ev_sub, 0));
        sb->gather_pending = false;
    }
    double *part = m->d_part_a + 3 * KMCF_MAX_PARTIALS;
    int rc = KMCF_OK;
    if (symm_applies(*sb)) {                                                   // (behind the stop: neither pass runs)
        with_bools([&](auto dot) {
            rc = symm_apply<0, decltype(dot)::value>(c, *sb, sb->n_loc, sb->row0, sb->d_rows, m->d_p, m->d_Ap, nullptr, part, m->d_S, chk);
        }, with_dot);
    } else if (!sb->dense && sb->n_loc > 0) {
        with_bools([&](auto dot) {
            sub_spmv_kernel<decltype(dot)::value><<<sb->grid, KMCF_BLOCK, 0, st>>>(sb->n_loc, sb->n_glob, sb->n_groups, sb->d_mask, sb->d_voff, sb->d_val,
                                                                                   sb->d_xsub, sb->d_rows, m->d_p, m->d_Ap, part, m->d_S, chk);
        }, with_dot);
        KMCF_HIP(hipGetLastError());
    }
    return rc;
}

static int check_params(const kmcf_current_params_t *p)
{
    KMCF_CHECK(p, KMCF_ERR_ARG, "null parameter block");
    KMCF_CHECK(p->high_G > 0 && p->low_G > 0 && p->loop_G > 0 && p->m_e > 0 && p->tol >= 0, KMCF_ERR_ARG, "non-positive conductance / mass");
    KMCF_CHECK(p->cg_max_iterations >= 0, KMCF_ERR_ARG, "negative iteration limit");
    return KMCF_OK;
}

extern "C" int kmcf_t_assemble(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge, const double *d_site_CB_edge,
                               const int *d_metals, int num_metals, const kmcf_current_params_t *p)
{
    KMCF_CHECK(t && d_site_element && d_site_charge && d_site_CB_edge && d_metals, KMCF_ERR_ARG, "kmcf_t_assemble: null argument");
    KMCF_TRY(check_params(p));
    KMCF_TRY(kmcf_enter(t->comm));
    KMCF_TRY(t_assemble_async(t, d_site_element, d_site_charge, d_site_CB_edge, d_metals, num_metals, p));
    KMCF_HIP(hipStreamSynchronize(t->comm->stream));
    return KMCF_OK;
}

extern "C" int kmcf_tstate_get_vectors(const kmcf_tstate *t, double *h_diag_neighbour, double *h_dinv, double *h_rhs)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_tstate_get_vectors: null state");
    KMCF_CHECK(t->assembled, KMCF_ERR_STATE, "kmcf_tstate_get_vectors: call kmcf_t_assemble first");
    KMCF_TRY(kmcf_enter(t->comm));
    KMCF_HIP(hipStreamSynchronize(t->comm->stream));
    const int n = t->T->n_loc;
    std::vector<double> tmp((size_t)std::max(n, 1));
    const double *src[3] = {t->d_diag, t->T->d_dinv, t->d_rhs};
    double *dst[3] = {h_diag_neighbour, h_dinv, h_rhs};
    for (int v = 0; v < 3; ++v) {
        if (!dst[v] || n == 0) continue;
        KMCF_HIP(hipMemcpy(tmp.data(), src[v], (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; ++i) dst[v][t->T->h_perm.empty() ? i : t->T->h_perm[i]] = tmp[i];
    }
    return KMCF_OK;
}

// ---------------------------------------------------------------- kmcf_tstate_get_tunnel (the tests' accessor): the values per form
// jagged: this rank's tiles (64 x 64, zeros where no entry) out of the layers
static int tunnel_tiles_from_layers(const kmcf_subop &sb, std::vector<double> *tiles)
{
    tiles->assign((size_t)sb.n_tiles * 4096, 0.0);
    std::vector<unsigned long long> jm((size_t)sb.n_tiles * 64);
    std::vector<long long> jo((size_t)sb.n_tiles + 1);
    std::vector<double> jv((size_t)sb.jnnz + 1);
    KMCF_HIP(hipMemcpy(jm.data(), sb.d_jmask, jm.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    KMCF_HIP(hipMemcpy(jo.data(), sb.d_jvoff, jo.size() * sizeof(long long), hipMemcpyDeviceToHost));
    if (sb.jnnz) KMCF_HIP(hipMemcpy(jv.data(), sb.d_jval, (size_t)sb.jnnz * sizeof(double), hipMemcpyDeviceToHost));
    for (long long tl = 0; tl < sb.n_tiles; ++tl) {
        unsigned long long m[64];
        for (int r = 0; r < 64; ++r) m[r] = jm[(size_t)tl * 64 + r];
        long long pos = jo[(size_t)tl];
        for (bool any = true; any;) {                    // layer by layer, rows ascending
            any = false;
            for (int r = 0; r < 64; ++r)
                if (m[r]) {
                    (*tiles)[(size_t)tl * 4096 + (size_t)r * 64 + __builtin_ctzll(m[r])] = jv[(size_t)pos++];
                    m[r] &= m[r] - 1;
                    any = true;
                }
        }
    }
    return KMCF_OK;
}

// spread: the tiles of this rank's rows lie on all ranks: the rows' entries are computed afresh as the bitmap storage
// would (the same values: one symmetric expression per pair); the walk puts the diagonal entries in use in their place
static int tunnel_rows_recomputed(const kmcf_tstate *t, double *h_val)
{
    const kmcf_subop &sb = t->sub;
    const int ns = sb.n_loc;
    double *d_v = nullptr, *d_dg = nullptr;
    KMCF_HIP(hipMalloc(reinterpret_cast<void **>(&d_v), ((size_t)sb.nnz + 64) * sizeof(double)));
    if (hipMalloc(reinterpret_cast<void **>(&d_dg), ((size_t)ns + 1) * sizeof(double)) != hipSuccess) { hipFree(d_v); KMCF_HIP(hipErrorOutOfMemory); }
    with_dist(t, [&](auto dist) {
        tunnel_value_kernel<decltype(dist)><<<wave_row_grid(ns), KMCF_BLOCK, 0, t->comm->stream>>>(ns, sb.row0, sb.n_groups, points_of(t), wkb_of(t),
                                                                                                   sb.d_mask, sb.d_voff, d_v, d_dg, dist);
    });
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(t->comm->stream);
    if (e1 == hipSuccess) e1 = hipMemcpy(h_val, d_v, (size_t)sb.nnz * sizeof(double), hipMemcpyDeviceToHost);
    hipFree(d_v); hipFree(d_dg);
    KMCF_HIP(e1);
    return KMCF_OK;
}

// The one walk of this rank's bitmap rows: row offsets and columns; values out of `tiles` when given (the tile forms of
// one rank), the diagonal entries out of d_tdiag (spread), else h_val stays as it is (packed = CSR order already).
static int tunnel_walk_bitmap(const kmcf_tstate *t, const std::vector<double> &tiles, int *h_row_ptr, int *h_col, double *h_val)
{
    const kmcf_subop &sb = t->sub;
    const int ns = sb.n_loc, ng = sb.n_groups;
    std::vector<double> tdiag_now;
    if (sb.spread && h_val && ns) {
        tdiag_now.resize((size_t)ns);
        KMCF_HIP(hipMemcpy(tdiag_now.data(), t->d_tdiag + sb.row0, (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    }
    std::vector<unsigned long long> mk((size_t)ns * ng + 1);
    if (ns) KMCF_HIP(hipMemcpy(mk.data(), sb.d_mask, (size_t)ns * ng * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    int64_t pos = 0;
    if (h_row_ptr) h_row_ptr[0] = 0;
    for (int s = 0; s < ns; ++s) {
        for (int g = 0; g < ng; ++g) {
            unsigned long long w = mk[(size_t)s * ng + g];
            while (w) {
                const int b = __builtin_ctzll(w);
                if (h_col) h_col[pos] = g * 64 + b;
                if (sb.spread && h_val && g * 64 + b == sb.row0 + s) h_val[pos] = tdiag_now[(size_t)s];
                if (!tiles.empty()) {
                    const int i = sb.row0 + s, j = g * 64 + b, lo = std::min(i, j), hi = std::max(i, j);
                    h_val[pos] = tiles[(size_t)symm_tile_index(sb.nb, lo >> 6, hi >> 6) * 4096 + (size_t)(lo & 63) * 64 + (hi & 63)];
                }
                ++pos;
                w &= w - 1;
            }
        }
        if (h_row_ptr) h_row_ptr[s + 1] = (int)pos;
    }
    return KMCF_OK;
}

extern "C" int kmcf_tstate_get_tunnel(const kmcf_tstate *t, int *h_tunnel_idx, int *h_row_ptr, int *h_col, double *h_val, double *h_diag)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_tstate_get_tunnel: null state");
    KMCF_CHECK(t->assembled, KMCF_ERR_STATE, "kmcf_tstate_get_tunnel: call kmcf_t_assemble first");
    KMCF_TRY(kmcf_enter(t->comm));
    KMCF_HIP(hipStreamSynchronize(t->comm->stream));
    const kmcf_subop &sb = t->sub;
    if (h_tunnel_idx && sb.n_glob) memcpy(h_tunnel_idx, t->h_tidx.data(), (size_t)sb.n_glob * sizeof(int));
    const int ns = sb.n_loc;
    if (h_diag && ns) KMCF_HIP(hipMemcpy(h_diag, t->d_tdiag + (sb.spread ? sb.row0 : 0), (size_t)ns * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<double> tiles;
    if (h_val && sb.nnz) {
        if (sb.jagged) {
            KMCF_TRY(tunnel_tiles_from_layers(sb, &tiles));
        } else if (sb.spread) {
            KMCF_TRY(tunnel_rows_recomputed(t, h_val));
        } else if (sb.dense) {                               // values out of the upper tiles (test-sized blocks)
            tiles.resize((size_t)sb.n_tiles * 4096);
            KMCF_HIP(hipMemcpy(tiles.data(), sb.d_tiles, tiles.size() * sizeof(double), hipMemcpyDeviceToHost));
        } else {
            KMCF_HIP(hipMemcpy(h_val, sb.d_val, (size_t)sb.nnz * sizeof(double), hipMemcpyDeviceToHost));   // packed = CSR order
        }
    }
    if (h_row_ptr || h_col || !tiles.empty() || (sb.spread && h_val)) KMCF_TRY(tunnel_walk_bitmap(t, tiles, h_row_ptr, h_col, h_val));
    return KMCF_OK;
}

// The power pass on the scaled potentials: shift (:2068-2071), forward currents and their row sums (:2086-2098) of the
// neighbour part and of the tunnel block in its form, P = I_neg m (:2100-2131), copy_pdisp (:2137)
static int power_pass(kmcf_tstate *t, double *pot, double *d_site_power)
{
    kmcf_comm *c = t->comm;
    kmcf_matrix *m = t->T;
    kmcf_subop &sb = t->sub;
    hipStream_t st = c->stream;
    const kmcf_current_params_t *p = &t->par;
    const int n_loc = m->n_loc, Na = t->N_atom;
    min_kernel<<<1, KMCF_BLOCK, 0, st>>>(Na + 2, pot, t->d_scal + 1);
    shift_kernel<<<kmcf_grid1d(Na + 2), KMCF_BLOCK, 0, st>>>(Na + 2, pot, t->d_scal + 1);
    double *psum = m->d_r, *isum = m->d_Ap;                          // workspace vectors, free after the solve
    if (n_loc > 0) {
        power_neighbour_kernel<16><<<kmcf_grid1d((int64_t)n_loc * 16), KMCF_BLOCK, 0, st>>>(
            n_loc, m->d_row_ptr, m->d_col, m->d_val, t->d_diag_pos, t->d_col_node, pot, p->Vd, psum, isum);
        KMCF_HIP(hipGetLastError());
    }
    if (symm_applies(sb)) {
        gather_tunnel_pot_kernel<<<kmcf_grid1d(sb.n_glob), KMCF_BLOCK, 0, st>>>(sb.n_glob, t->d_tidx, pot, sb.d_xsub);
        KMCF_TRY((symm_apply<1, false>(c, sb, sb.n_loc, sb.row0, sb.d_rows, nullptr, psum, isum, nullptr, nullptr, 0, p->Vd)));
        KMCF_HIP(hipMemsetAsync(sb.d_xsub + sb.n_glob, 0, (size_t)(64 * sb.nb - sb.n_glob) * sizeof(double), st));    // the pad stays 0
    } else if (!sb.dense && sb.n_loc > 0) {
        power_tunnel_kernel<<<sb.grid, KMCF_BLOCK, 0, st>>>(sb.n_loc, sb.row0, sb.n_groups, sb.d_mask, sb.d_voff, sb.d_val, t->d_tidx, sb.d_rows, pot,
                                                            p->Vd, psum, isum);
    }
    if (n_loc > 0) power_finish_kernel<<<kmcf_grid1d(n_loc), KMCF_BLOCK, 0, st>>>(n_loc, t->d_col_node, pot, psum, isum, t->d_pdisp);
    KMCF_HIP(hipGetLastError());
    KMCF_TRY(kmcf_comm_allgatherv_double(c, t->d_pdisp, m->counts.data(), m->displs.data()));
    copy_pdisp_kernel<<<kmcf_grid1d(Na - 1), KMCF_BLOCK, 0, st>>>(Na - 1, t->d_atom_site, t->d_acls, t->d_pdisp, p->alpha_disp, d_site_power);
    KMCF_HIP(hipGetLastError());
    return KMCF_OK;
}

extern "C" int kmcf_update_power_sparse(kmcf_tstate *t, const int *d_site_element, const int *d_site_charge,
                                        const double *d_site_CB_edge, const int *d_metals, int num_metals,
                                        double *d_atom_virtual_potentials, double *d_site_power,
                                        const kmcf_current_params_t *p, double *imacro, kmcf_solve_stats_t *stats)
{
    KMCF_CHECK(t && d_site_element && d_site_charge && d_site_CB_edge && d_metals && d_atom_virtual_potentials, KMCF_ERR_ARG,
               "kmcf_update_power_sparse: null argument");
    KMCF_TRY(check_params(p));
    KMCF_CHECK(!p->solve_heating || d_site_power, KMCF_ERR_ARG, "kmcf_update_power_sparse: solve_heating needs d_site_power");
    kmcf_comm *c = t->comm;
    kmcf_matrix *m = t->T;
    KMCF_CHECK(c->connected, KMCF_ERR_COMM, "kmcf_update_power_sparse: communicator not connected");
    KMCF_TRY(kmcf_enter(c));
    hipStream_t st = c->stream;
    const int n_loc = m->n_loc, Na = t->N_atom;
    KMCF_HIP(hipEventRecord(c->ev_a0, st));
    KMCF_TRY(t_assemble_async(t, d_site_element, d_site_charge, d_site_CB_edge, d_metals, num_metals, p));
    KMCF_HIP(hipEventRecord(c->ev_a1, st));
    // the initial guess is the current content of atom_virtual_potentials, solved in place (:1463)
    double *x_user = d_atom_virtual_potentials + m->row0;
    if (n_loc > 0) KMCF_HIP(hipMemcpyAsync(m->d_r, t->d_rhs, (size_t)n_loc * sizeof(double), hipMemcpyDeviceToDevice, st));
    KMCF_TRY(kmcf_vec_in(m, m->d_x, x_user));
    KMCF_TRY(kmcf_pcg_workspace(m, true, p->cg_tolerance, p->cg_max_iterations, 0, stats));     // :1674
    KMCF_TRY(kmcf_vec_out(m, x_user, m->d_x));
    // every rank gets all Nsub potentials (the reference gathers them on rank 0 only, :1782)
    KMCF_TRY(kmcf_comm_allgatherv_double(c, d_atom_virtual_potentials, m->counts.data(), m->displs.data()));
    // scaled by G0 in place, all N_atom + 2 entries (:2038-2040)
    scale_kernel<<<kmcf_grid1d(Na + 2), KMCF_BLOCK, 0, st>>>(Na + 2, d_atom_virtual_potentials, p->G0);
    // I_macro on the owner of row 1, then shared
    const bool own1 = m->row0 <= 1 && 1 < m->row0 + n_loc;
    imacro_kernel<<<1, KMCF_BLOCK, 0, st>>>(own1 ? t->h_inv_perm[1 - m->row0] : -1, m->d_row_ptr, m->d_col, m->d_val, t->d_col_node,
                                            d_atom_virtual_potentials, t->d_scal);
    KMCF_HIP(hipGetLastError());
    KMCF_TRY(kmcf_comm_allreduce_sum(c, t->d_scal, 1));
    // (into pinned memory that outlives this frame: the error returns below leave before the synchronisation)
    KMCF_HIP(hipMemcpyAsync(&t->h_pin->imacro, t->d_scal, sizeof(double), hipMemcpyDeviceToHost, st));
    if (p->solve_heating) KMCF_TRY(power_pass(t, d_atom_virtual_potentials, d_site_power));
    KMCF_HIP(hipStreamSynchronize(st));
    KMCF_TRY(kmcf_p2p_check(c));
    if (imacro) *imacro = t->h_pin->imacro;
    if (stats) {
        float ms = 0.f;
        KMCF_HIP(hipEventElapsedTime(&ms, c->ev_a0, c->ev_a1));
        stats->ms_assembly = ms;
    }
    return KMCF_OK;
}

extern "C" int kmcf_current_map(kmcf_tstate *t, const double *d_atom_virtual_potentials, double *d_site_current, double *d_site_tunnel,
                                double *d_site_net, kmcf_current_map_stats_t *stats)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_current_map: null state (t)");
    KMCF_CHECK(d_atom_virtual_potentials, KMCF_ERR_ARG, "kmcf_current_map: null d_atom_virtual_potentials");
    KMCF_CHECK(d_site_current, KMCF_ERR_ARG, "kmcf_current_map: null d_site_current");
    KMCF_CHECK(t->assembled, KMCF_ERR_STATE, "kmcf_current_map: call kmcf_t_assemble or kmcf_update_power_sparse first");
    kmcf_comm *c = t->comm;
    kmcf_matrix *m = t->T;
    KMCF_CHECK(c->connected, KMCF_ERR_COMM, "kmcf_current_map: communicator not connected");
    KMCF_TRY(kmcf_enter(c));
    hipStream_t st = c->stream;
    const kmcf_subop &sb = t->sub;
    const int n_loc = m->n_loc, Na = t->N_atom, N = t->N;
    const double *pot = d_atom_virtual_potentials;
    KMCF_HIP(hipEventRecord(c->ev_a0, st));
    KMCF_HIP(hipMemsetAsync(d_site_current, 0, (size_t)N * sizeof(double), st));
    if (d_site_tunnel) KMCF_HIP(hipMemsetAsync(d_site_tunnel, 0, (size_t)N * sizeof(double), st));
    if (d_site_net) KMCF_HIP(hipMemsetAsync(d_site_net, 0, (size_t)N * sizeof(double), st));
    // this rank's rows: the neighbour part sets the three sums of a node, the tunnel part adds the row's pairs of the bitmap
    if (n_loc > 0) {
        current_neighbour_kernel<16><<<kmcf_grid1d((int64_t)n_loc * 16), KMCF_BLOCK, 0, st>>>(n_loc, m->d_row_ptr, m->d_col, m->d_val, t->d_diag_pos,
                                                                                         t->d_col_node, pot, t->d_cmap);
        KMCF_HIP(hipGetLastError());
    }
    if (sb.n_loc > 0) {
        with_dist(t, [&](auto dist) {
            current_tunnel_kernel<decltype(dist)><<<wave_row_grid(sb.n_loc), KMCF_BLOCK, 0, st>>>(sb.n_loc, sb.row0, sb.n_groups, points_of(t), wkb_of(t),
                                                                                                  sb.d_mask, t->d_tidx, pot, t->d_cmap, dist);
        });
        KMCF_HIP(hipGetLastError());
    }
    // every rank gets all nodes (as d_pdisp is gathered: the row partition, three doubles a row)
    KMCF_TRY(kmcf_comm_allgatherv_double(c, t->d_cmap, t->cm_counts.data(), t->cm_displs.data()));
    current_scatter_kernel<<<kmcf_grid1d(Na - 1), KMCF_BLOCK, 0, st>>>(Na - 1, t->d_atom_site, t->d_cmap, d_site_current, d_site_tunnel, d_site_net);
    current_stats_kernel<<<1, KMCF_BLOCK, 0, st>>>(Na - 1, t->d_atom_site, t->d_cmap, t->d_cmstat);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(t->h_cmstat, t->d_cmstat, 6 * sizeof(double), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(c->ev_a1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    KMCF_TRY(kmcf_p2p_check(c));
    if (stats) {
        const double *h = t->h_cmstat;
        stats->i_injection = h[0];
        stats->i_extraction = h[1];
        stats->sum_through = h[2];
        stats->sum_tunnel = h[3];
        stats->max_through = h[4];
        stats->max_site = (int)h[5];
        const long long walked = (long long)sb.nnz - sb.n_loc;               // every row of the bitmap holds its diagonal bit
        stats->tunnel_pairs_walked = (int)std::min<long long>(std::max<long long>(walked, 0), INT32_MAX);
        float ms = 0.f;
        KMCF_HIP(hipEventElapsedTime(&ms, c->ev_a0, c->ev_a1));
        stats->ms = ms;
    }
    return KMCF_OK;
}

// the device and pinned copies of the profile + statistics hold n doubles afterwards; an outgrown pair is kept until the
// state goes (a free would wait for the device, where another rank of the group may already stand in its all-gather)
static int profile_out_grow(kmcf_tstate *t, size_t n, size_t n_part)
{
    if (!t->d_cppart || n_part > t->cap_cppart) {
        if (t->d_cppart) { t->cp_retired_dev.push_back(t->d_cppart); t->d_cppart = nullptr; }
        t->cap_cppart = 0;
        KMCF_TRY(kmcf_dev_alloc(&t->d_cppart, n_part, true, t->comm->stream));
        t->cap_cppart = n_part;
    }
    if (t->d_cpout && n <= t->cap_cpout) return KMCF_OK;
    if (t->d_cpout) { t->cp_retired_dev.push_back(t->d_cpout); t->d_cpout = nullptr; }
    if (t->h_cpout) { t->cp_retired_host.push_back(t->h_cpout); t->h_cpout = nullptr; }
    t->cap_cpout = 0;
    KMCF_TRY(kmcf_dev_alloc(&t->d_cpout, n, true, t->comm->stream));
    KMCF_TRY(pinned_zeroed(&t->h_cpout, n));
    t->cap_cpout = n;
    return KMCF_OK;
}

extern "C" int kmcf_current_profile(kmcf_tstate *t, const double *d_atom_virtual_potentials, const int *d_site_cell, int n_cells,
                                    const double *h_plane_x, int n_planes, double *h_profile, double *d_site_jx, double *d_site_jy,
                                    double *d_site_jz, kmcf_current_profile_stats_t *stats)
{
    KMCF_CHECK(t, KMCF_ERR_ARG, "kmcf_current_profile: null state (t)");
    KMCF_CHECK(d_atom_virtual_potentials, KMCF_ERR_ARG, "kmcf_current_profile: null d_atom_virtual_potentials");
    KMCF_CHECK(h_plane_x, KMCF_ERR_ARG, "kmcf_current_profile: null h_plane_x");
    KMCF_CHECK(h_profile, KMCF_ERR_ARG, "kmcf_current_profile: null h_profile");
    KMCF_CHECK(n_planes >= 1 && n_planes <= CP_MAX, KMCF_ERR_ARG, "kmcf_current_profile: n_planes = %d outside 1 ... %d", n_planes, CP_MAX);
    KMCF_CHECK(n_cells >= 1 && n_cells <= CP_MAX, KMCF_ERR_ARG, "kmcf_current_profile: n_cells = %d outside 1 ... %d", n_cells, CP_MAX);
    KMCF_CHECK(d_site_cell || n_cells == 1, KMCF_ERR_ARG, "kmcf_current_profile: d_site_cell is NULL with n_cells = %d", n_cells);
    for (int k = 0; k < n_planes; ++k) {
        KMCF_CHECK(std::isfinite(h_plane_x[k]), KMCF_ERR_ARG, "kmcf_current_profile: h_plane_x[%d] is not finite", k);
        KMCF_CHECK(k == 0 || h_plane_x[k - 1] < h_plane_x[k], KMCF_ERR_ARG, "kmcf_current_profile: h_plane_x is not strictly ascending at [%d]", k);
    }
    const bool vec = d_site_jx && d_site_jy && d_site_jz;
    KMCF_CHECK(vec || (!d_site_jx && !d_site_jy && !d_site_jz), KMCF_ERR_ARG,
               "kmcf_current_profile: d_site_jx, d_site_jy, d_site_jz: pass all three or none");
    KMCF_CHECK(t->assembled, KMCF_ERR_STATE, "kmcf_current_profile: call kmcf_t_assemble or kmcf_update_power_sparse first");
    KMCF_CHECK(t->d_cprof, KMCF_ERR_STATE, "kmcf_current_profile: %d atoms exceed the int32 counts of the gather", t->N_atom);
    kmcf_comm *c = t->comm;
    kmcf_matrix *m = t->T;
    KMCF_CHECK(c->connected, KMCF_ERR_COMM, "kmcf_current_profile: communicator not connected");
    KMCF_TRY(kmcf_enter(c));
    hipStream_t st = c->stream;
    const kmcf_subop &sb = t->sub;
    const int n_loc = m->n_loc, Na = t->N_atom, N = t->N;
    const double *pot = d_atom_virtual_potentials;
    const size_t n_prof = (size_t)(n_cells + 1) * n_planes * 2;
    // the binning's segments: about 1024 blocks over the cells, a segment a multiple of KMCF_BLOCK atoms
    const int n_rows_atoms = Na - 1;
    const int seg_want = std::max(1, (1024 + n_cells) / (n_cells + 1));
    const int seg_len = std::max(1, ((n_rows_atoms + seg_want - 1) / seg_want + KMCF_BLOCK - 1) / KMCF_BLOCK) * KMCF_BLOCK;
    const int n_seg = std::max(1, (n_rows_atoms + seg_len - 1) / seg_len);
    KMCF_TRY(profile_out_grow(t, n_prof + 8, (size_t)(n_cells + 1) * n_seg * 2 * (n_planes + 1)));      // (the only allocations, before the first kernel)
    memcpy(t->h_cpplanes, h_plane_x, (size_t)n_planes * sizeof(double));
    KMCF_HIP(hipEventRecord(c->ev_a0, st));
    KMCF_HIP(hipMemcpyAsync(t->d_cpplanes, t->h_cpplanes, (size_t)n_planes * sizeof(double), hipMemcpyHostToDevice, st));
    if (vec) {
        KMCF_HIP(hipMemsetAsync(d_site_jx, 0, (size_t)N * sizeof(double), st));
        KMCF_HIP(hipMemsetAsync(d_site_jy, 0, (size_t)N * sizeof(double), st));
        KMCF_HIP(hipMemsetAsync(d_site_jz, 0, (size_t)N * sizeof(double), st));
    }
    profile_key_kernel<<<kmcf_grid1d(Na), KMCF_BLOCK, 0, st>>>(Na, t->d_ax, t->d_atom_site, d_site_cell, n_cells, t->d_cpplanes, n_planes, t->d_cpq,
                                                              t->d_cpcell);
    KMCF_HIP(hipGetLastError());
    // this rank's rows: the neighbour part sets the values of a node, the tunnel part adds the row's pairs of the bitmap
    const cp_keys keys{t->d_cpq, t->d_cpcell, n_cells};
    auto walk = [&](auto dist, auto with_vec) {
        constexpr bool VEC = decltype(with_vec)::value;
        if (n_loc > 0)
            profile_neighbour_kernel<16, VEC, decltype(dist)><<<kmcf_grid1d((int64_t)n_loc * 16), KMCF_BLOCK, 0, st>>>(
                n_loc, m->d_row_ptr, m->d_col, m->d_val, t->d_diag_pos, t->d_col_node, pot, keys, t->d_ax, t->d_ay, t->d_az, t->d_cprof, dist);
        if (sb.n_loc > 0)
            profile_tunnel_kernel<VEC, decltype(dist)><<<wave_row_grid(sb.n_loc), KMCF_BLOCK, 0, st>>>(
                sb.n_loc, sb.row0, sb.n_groups, points_of(t), wkb_of(t), sb.d_mask, t->d_tidx, pot, keys, t->d_cprof, dist);
    };
    with_dist(t, [&](auto dist) {
        if (vec) walk(dist, std::true_type{}); else walk(dist, std::false_type{});
    });
    KMCF_HIP(hipGetLastError());
    KMCF_TRY(kmcf_comm_allgatherv_double(c, t->d_cprof, t->cp_counts.data(), t->cp_displs.data()));
    KMCF_HIP(hipEventRecord(c->ev_a1, st));
    profile_bin_kernel<<<dim3(n_seg, n_cells + 1), KMCF_BLOCK, 0, st>>>(n_rows_atoms, seg_len, n_planes, n_cells, t->d_cpq, t->d_cpcell, t->d_cprof,
                                                                         t->d_cppart);
    profile_prefix_kernel<<<n_cells + 1, KMCF_BLOCK, 0, st>>>(n_seg, n_planes, t->d_cppart, t->d_cpout);
    if (vec) profile_scatter_kernel<<<kmcf_grid1d(Na - 1), KMCF_BLOCK, 0, st>>>(Na - 1, t->d_atom_site, t->d_cprof, d_site_jx, d_site_jy, d_site_jz);
    profile_stats_kernel<<<1, KMCF_BLOCK, 0, st>>>(Na - 1, n_planes, n_cells, t->d_cpout, t->d_cprof, vec ? 1 : 0, t->d_cpout + n_prof);
    KMCF_HIP(hipGetLastError());
    KMCF_HIP(hipMemcpyAsync(t->h_cpout, t->d_cpout, (n_prof + 8) * sizeof(double), hipMemcpyDeviceToHost, st));
    KMCF_HIP(hipEventRecord(c->ev_t1, st));
    KMCF_HIP(hipStreamSynchronize(st));
    KMCF_TRY(kmcf_p2p_check(c));
    memcpy(h_profile, t->h_cpout, n_prof * sizeof(double));
    if (stats) {
        const double *h = t->h_cpout + n_prof;
        stats->i_injection = h[0];
        stats->i_extraction = h[1];
        stats->flux_min = h[2];
        stats->flux_max = h[3];
        stats->sum_jx = h[4];
        stats->plane_min = (int)h[5];
        stats->plane_max = (int)h[6];
        float ms = 0.f;
        KMCF_HIP(hipEventElapsedTime(&ms, c->ev_a0, c->ev_a1));
        stats->ms_pairs = ms;
        KMCF_HIP(hipEventElapsedTime(&ms, c->ev_a1, c->ev_t1));
        stats->ms_planes = ms;
    }
    return KMCF_OK;
}
