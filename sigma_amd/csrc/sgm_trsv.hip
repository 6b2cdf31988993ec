// The triangular sweeps of the ILDU(0) apply, the hot part of a preconditioned solve:
//     x = b ; (I+L)^-1 ; x / D ; (I+U)^-1
// each triangular solve a row recurrence (ldu_solvers.f90:227-236, :254-263).  Everything here runs on the DEVICE; the
// host only picks kernels and launches.  The structures the kernels read are built by sgm_ildu.hip.  Three paths (the
// slab pipeline for 3-D grids is a fourth, in sgm_trsv3.hip):
//   level walkers (apply_levels)   rows are grouped into dependency LEVELS; rows of one level are independent, each lane does
//       its row's z = z - val(k)*x(node(k)) left to right, so the result is bit-identical to the sequential sweep.  The solve
//       runs in "position space": vectors are permuted into level order (xp[pos]), every row is a 64-byte record {count,
//       first 4 (dependency position, value)} so that ONE independent load brings a row and can be issued a level ahead.
//       Wide levels get one launch each; runs of narrow levels (<= 4096 rows) are walked by ONE 1024-thread workgroup that
//       keeps the last 8192 results in an LDS ring: a level then costs LDS reads + a barrier instead of four dependent
//       global round trips.
//   strip pipeline (apply_grid)    grid-like factors (deps r-1, r-w): one launch per sweep, see k_trsv_strip.
//   row-space sweeps (apply_rows)  factors of a few levels (colour orderings): one launch per level on the vectors
//       themselves, no position space at all; rows_cg_fused folds PCG's r update and r.z into them.  Four kernel families
//       (one or two rows per lane, plain or fused into PCG) around ONE row recurrence: row_minus_entries and its
//       two-row form pair_load / pair_minus_entries.  A kernel adds how a row picks up its right-hand side, what a
//       dependency reads and what is stored.
// Also here: the elementwise Jacobi apply (scale_by).  The launchers at the end turn run-time values into template arguments
// through generic lambdas (with_upto2, with_row_slots, with_soa_slots, with_flag); there are no launch macros.  What the
// strip pipeline shares with the slab pipeline (abort, empty marker, DPP shift, the scatter out of position space) is in
// sgm_trsv_device.hpp.
#include "sgm_pc_internal.hpp"
#include "sgm_trsv_device.hpp"

#include <algorithm>
#include <type_traits>

using namespace sgm;

namespace {

// ------------------------------------------------------------------------------ kernels
// z = d * r (vectors are 16-byte aligned: 16-byte accesses for the pairs, the odd tail element alone)
__global__ void k_scale_by(int64_t n, const double *__restrict__ d, const double *__restrict__ r,
                           double *__restrict__ z, const int *flag)
{
    if (flag && *flag) return;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n2 = n >> 1;
    const double2 *d2 = reinterpret_cast<const double2 *>(d), *r2 = reinterpret_cast<const double2 *>(r);
    double2 *z2 = reinterpret_cast<double2 *>(z);
    for (int64_t i = gtid; i < n2; i += stride) {            // x = idiag * b
        const double2 a = d2[i], b = r2[i];
        z2[i] = make_double2(a.x * b.x, a.y * b.y);
    }
    if ((n & 1) && gtid == 0) z[n - 1] = d[n - 1] * r[n - 1];
}

__global__ void k_perm_gather(int64_t n, double *__restrict__ xp, const double *__restrict__ src,
                              const int32_t *__restrict__ order, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < n; p += stride) xp[p] = src[order[p]];            // x = b, in level order
}
__global__ void k_lu_transition(int64_t n, double *__restrict__ xpU, const double *__restrict__ xpL,
                                const int32_t *__restrict__ mapLU, const double *__restrict__ Dp, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < n; p += stride) xpU[p] = xpL[mapLU[p]] / Dp[p];   // x = x / D, re-ordered for the U sweep
}
__global__ void k_perm_scatter(int64_t n, double *__restrict__ dst, const double *__restrict__ xp,
                               const int32_t *__restrict__ order, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < n; p += stride) dst[order[p]] = xp[p];
}

// one wide level: one lane per row, dependencies read from global memory
__global__ void k_trsv_wide(const TrsvRec *__restrict__ recs, const int32_t *__restrict__ pq,
                            const double *__restrict__ pv, int32_t begin, int32_t end, double *xp, const int *flag)
{
    if (flag && *flag) return;
    const int32_t p = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    const TrsvRec r = recs[p];
    double z = xp[p];
#pragma unroll
    for (int j = 0; j < kInline; ++j)
        if (j < r.cnt) z = z - r.v[j] * xp[r.q[j]];
    for (int32_t k = r.k0 + kInline; k < r.k0 + r.cnt; ++k) z = z - pv[k] * xp[pq[k]];
    xp[p] = z;
}

// the same on the structure-of-arrays copy (all rows of the level have <= kInline dependencies):
// positions and values slot-major, every load coalesced (the 64-byte records cost one cache line per
// lane and load instruction)
template <int C>
__global__ void k_trsv_wide_soa(const int32_t *__restrict__ wq, const double *__restrict__ dv, uint32_t nstride,
                                int32_t begin, int32_t end, double *xp, const int *flag)
{
    if (flag && *flag) return;
    const int32_t p = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    double z = xp[p];
    int32_t q[C];
    double v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { q[c] = wq[(size_t)c * nstride + p]; v[c] = dv[(size_t)c * nstride + p]; }
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (q[c] >= 0) z = z - v[c] * xp[q[c]];
    xp[p] = z;
}

// ---- row-space sweeps -----------------------------------------------------------------------------------------------
// THE row recurrence, written once for the four kernels below: a row's right-hand side minus its entries in stored order,
//     t = t - val * dep(row of the entry),
// every product rounded on its own (the build has -ffp-contract=off) -- bit for bit the oracle's sequential sweep.  p = the
// row's position in the level order, which is where its slots lie in rq / rv (rs_at).  C >= 0: C slots, unrolled, every slot
// requested before the first is used, nontemporal (read once per sweep: past the caches the gathers live in); C = -1: `rc`
// slots in a loop (a row's entries fill its first slots).  What dep reads is the caller's business.
template <int C, class Dep>
__device__ inline double row_minus_entries(double t, const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc, int32_t p,
                                           Dep dep)
{
    if constexpr (C >= 0) {
        int32_t q[C > 0 ? C : 1];
        double v[C > 0 ? C : 1];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            q[c] = __builtin_nontemporal_load(rq + rs_at(c, p, rc));
            v[c] = __builtin_nontemporal_load(rv + rs_at(c, p, rc));
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (q[c] >= 0) t = t - v[c] * dep(q[c]);
    } else {
        for (int c = 0; c < rc; ++c) {
            const int32_t q = rq[rs_at(c, p, rc)];
            if (q < 0) break;
            t = t - rv[rs_at(c, p, rc)] * dep(q);
        }
    }
    return t;
}

// The same for TWO consecutive rows per lane -- positions p, p + 1 (p even) holding rows i, i + 1 -- with 16-byte accesses (8-byte
// for the row numbers) on every stream: half the memory instructions per byte; the one-row form streams at 4.3-4.8 TB/s where
// the vector kernels reach 5.6-6.6.  In two steps, because the kernels form the right-hand sides in between: pair_load requests
// the slots of both rows, pair_minus_entries gathers every operand before either row uses one and runs the two subtraction
// chains side by side.  Per row the statements of row_minus_entries in their order: same bits.
// CODED: the dependency rows come from the 4-bit codes (rcode; dl = the factor's rdict in LDS, 15 = no entry) instead of
// rq: 4 bytes per row instead of 4 * C.
typedef double f64x2p __attribute__((ext_vector_type(2)));
typedef int32_t i32x2p __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2p __attribute__((ext_vector_type(2)));
template <int C> struct RowPair { i32x2p jj[C]; f64x2p vv[C]; };
template <int C, bool CODED>
__device__ inline void pair_load(RowPair<C> &e, const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc,
                                 const uint32_t *__restrict__ rcode, const int32_t *dl, int32_t p, int32_t i)
{
    u32x2p cw;
    if (CODED) cw = __builtin_nontemporal_load(reinterpret_cast<const u32x2p *>(rcode + p));
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (CODED) {
            const uint32_t na = (cw.x >> (4 * c)) & 15u, nb = (cw.y >> (4 * c)) & 15u;
            e.jj[c].x = na == 15u ? -1 : i + dl[na];
            e.jj[c].y = nb == 15u ? -1 : i + 1 + dl[nb];
        } else
            e.jj[c] = __builtin_nontemporal_load(reinterpret_cast<const i32x2p *>(rq + rs_at(c, p, rc)));
        e.vv[c] = __builtin_nontemporal_load(reinterpret_cast<const f64x2p *>(rv + rs_at(c, p, rc)));
    }
}
template <int C, class Dep>
__device__ inline void pair_minus_entries(const RowPair<C> &e, double &ta, double &tb, Dep dep)
{
    double da[C], db[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        da[c] = e.jj[c].x >= 0 ? dep(e.jj[c].x) : 0.0;
        db[c] = e.jj[c].y >= 0 ? dep(e.jj[c].y) : 0.0;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if (e.jj[c].x >= 0) ta = ta - e.vv[c].x * da[c];
        if (e.jj[c].y >= 0) tb = tb - e.vv[c].y * db[c];
    }
}

// One level in ROW space (factors of a few levels -- what the reference's greedy colouring makes of a matrix: one level per
// colour): out[i] = src[i] (/ D[i]) - sum over the row's entries, stored order, of val * out[row of the entry];
// i = the level's rows, through `order` or -- a level that is a run of consecutive rows -- counted from row0.  No gather
// into level order before the sweeps, no re-ordering between them, no scatter after: the L sweep reads r and writes the
// work vector, the U sweep divides by D as it picks its right-hand side up and writes z.  C = slots read (the most
// entries of a row of the level; -1: `rc` of them in a loop).  Same operations in the same order as k_trsv_wide_soa
// after k_perm_gather / k_lu_transition, so the same bits.
// MODE 0: a level of the L sweep, y_i = r_i - sum val * y(node); MODE 1: the same for a level whose rows have no U entries
// at all (U's level 0 -- with a colour ordering: the last colour), finished on the spot: z_i = y_i / D_i, y_i is never
// stored; MODE 2: a level of the U sweep, z_i = y_i / D_i - sum val * z(node).  Rows below n0 are L's level 0 when that is
// the run of rows 0 .. n0-1 (the first colour): their y IS r, so nobody copies it -- whoever wants y(q), q < n0, reads r(q).
template <int C, int MODE>
__global__ void k_trsv_rows(const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc, const int32_t *__restrict__ order,
                            int32_t row0, int32_t begin, int32_t end, const double *r, double *y, const double *__restrict__ D,
                            double *z, int32_t n0, const int *flag)
{
    if (flag && *flag) return;
    // tile -> workgroup: the dispatcher deals workgroups b, b + 8, ... to one XCD; they take CONSECUTIVE tiles of 256 positions
    // (XCD k: the k-th eighth of the level), so that a row and its neighbours a grid line away -- other tiles, the same
    // vector entries -- meet in one L2 instead of being fetched once per XCD (the grid is 8 * ceil(tiles / 8) workgroups)
    const int32_t tiles_per_xcd = gridDim.x >> 3;
    const int32_t tile = (blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    const int32_t p = begin + tile * (int32_t)blockDim.x + threadIdx.x;
    if (p >= end) return;
    const int32_t i = row0 >= 0 ? row0 + (p - begin) : order[p];
    double t;
    if (MODE == 2) t = (i < n0 ? r[i] : y[i]) / D[i];
    else t = r[i];
    t = row_minus_entries<C>(t, rq, rv, rc, p, [&](int32_t q) -> double { return MODE == 2 ? z[q] : (q < n0 ? r[q] : y[q]); });
    if (MODE == 0) y[i] = t;
    else if (MODE == 1) z[i] = t / D[i];
    else z[i] = t;
}

// PCG's  r = r - alpha q ; z = M^-1 r ; partial r.z  inside the two launches of a TWO-level factorisation (what the greedy
// colouring makes of a 5- / 7-point matrix: L = the rows of colour 2 reading colour 1, U = the rows of colour 1 reading
// colour 2) -- the r update (k_elem<FCgR<2>>: read r, q, write r) and the dot (k_elem<FDot2>: read r, z) cost 43 + 24 us of a
// 403 us iteration at n = 1e7 as launches of their own.  alpha = res2 / dpr from the partial sums like FCgR's prepare.
//   (before them the caller has updated the entry-less rows 0 .. n0-1 -- a streaming launch over a third of the bytes: with
//    r_j - alpha q_j formed on the fly in MODE 1 its gathers doubled and the launch ran at 4.3 TB/s, 120 us)
//   MODE 1 (rows n0 .. n-1): r_i -= alpha q_i ; z_i = (r_i - sum val * r_j) / D_i      [j < n0]
//   MODE 2 (rows 0 .. n0-1): z_i = r_i / D_i - sum val * z_j                            [j >= n0]
// Same statements and operand order per row as FCgR<2> + k_trsv_rows<C, 1 / 2>: r and z bit-identical; the dot is summed per
// block of this grid instead of k_elem's (tree order either way).
template <int C, int MODE>
__global__ __launch_bounds__(kBlock) void k_trsv_rows_cg(const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc,
                                                         const int32_t *__restrict__ order, int32_t row0, int32_t begin, int32_t end, double *r,
                                                         const double *__restrict__ q, ScalarRef res2, ScalarRef dpr, const double *__restrict__ D,
                                                         double *z, double *part, const int *flag, int gen)
{
    __shared__ double red[2 * (kBlock / 64)];
    const int st = flag ? *flag : 0;
    const ScalarRef rs[2] = {res2, dpr};
    double sc[2];
    load_scalars<kBlock, 2>(rs, sc, red);
    if (st && gen >= st) return;
    const double alpha = sc[0] / sc[1];
    double s = 0.0;
    // (tiles of 256 positions; XCD k = workgroups k, k + 8, ... walks the k-th eighth of them in order: k_trsv_rows' map)
    const int32_t tiles = (end - begin + kBlock - 1) / kBlock, tiles_per_xcd = (tiles + 7) >> 3, wg_per_xcd = gridDim.x >> 3;
    const int32_t t_end = min(tiles, ((int32_t)(blockIdx.x & 7) + 1) * tiles_per_xcd);
    for (int32_t tile = (blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3); tile < t_end; tile += wg_per_xcd) {
        const int32_t p = begin + tile * kBlock + threadIdx.x;
        if (p >= end) continue;
        const int32_t i = row0 >= 0 ? row0 + (p - begin) : order[p];
        const double ri = MODE == 1 ? r[i] - alpha * q[i] : r[i];
        if (MODE == 1) r[i] = ri;
        const double t = row_minus_entries<C>(MODE == 2 ? ri / D[i] : ri, rq, rv, rc, p,
                                              [&](int32_t j) -> double { return MODE == 2 ? z[j] : r[j]; });
        const double zi = MODE == 1 ? t / D[i] : t;
        z[i] = zi;
        s += ri * zi;
    }
    const double tot = block_sum<kBlock>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// The same with two rows per lane (pair_load / pair_minus_entries) -- the level is a run of consecutive rows (row0 >= 0) whose
// first position and first row have one parity, slot stride even; an odd first and an odd last row go alone.
template <int C, int MODE, bool CODED>
__global__ __launch_bounds__(kBlock) void k_trsv_rows_cg2(const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc,
                                                          const uint32_t *__restrict__ rcode, const int32_t *__restrict__ rdict,
                                                          int32_t row0, int32_t begin, int32_t end, double *r, const double *__restrict__ q,
                                                          ScalarRef res2, ScalarRef dpr, const double *__restrict__ D, double *z, double *part,
                                                          const int *flag, int gen)
{
    __shared__ double red[2 * (kBlock / 64)];
    __shared__ int32_t dl[16];
    if (CODED) {
        if (threadIdx.x < 16) dl[threadIdx.x] = rdict[threadIdx.x];
        __syncthreads();
    }
    const int st = flag ? *flag : 0;
    const ScalarRef rs[2] = {res2, dpr};
    double sc[2];
    load_scalars<kBlock, 2>(rs, sc, red);
    if (st && gen >= st) return;
    const double alpha = sc[0] / sc[1];
    double s = 0.0;
    constexpr int TILE = 2 * kBlock;
    auto dep = [&](int32_t j) -> double { return MODE == 2 ? z[j] : r[j]; };
    auto one_row = [&](int32_t p, int32_t i) {               // (k_trsv_rows_cg's row)
        const double ri = MODE == 1 ? r[i] - alpha * q[i] : r[i];
        if (MODE == 1) r[i] = ri;
        const double t = row_minus_entries<C>(MODE == 2 ? ri / D[i] : ri, rq, rv, rc, p, dep);
        const double zi = MODE == 1 ? t / D[i] : t;
        z[i] = zi;
        s += ri * zi;
    };
    // a level that starts at an odd position / row (both odd: the caller checks): its first row alone, the pairs from the next
    const int32_t peel = begin & 1;
    if (peel && blockIdx.x == 0 && threadIdx.x == 0 && begin < end) one_row(begin, row0);
    begin += peel;
    row0 += peel;
    const int32_t tiles = (end - begin + TILE - 1) / TILE, tiles_per_xcd = (tiles + 7) >> 3, wg_per_xcd = gridDim.x >> 3;
    const int32_t t_end = min(tiles, ((int32_t)(blockIdx.x & 7) + 1) * tiles_per_xcd);
    for (int32_t tile = (blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3); tile < t_end; tile += wg_per_xcd) {
        const int32_t p = begin + tile * TILE + 2 * (int32_t)threadIdx.x;
        if (p >= end) continue;
        const int32_t i = row0 + (p - begin);
        if (p + 1 >= end) { one_row(p, i); continue; }
        const f64x2p rr = *reinterpret_cast<const f64x2p *>(r + i), dd = *reinterpret_cast<const f64x2p *>(D + i);
        f64x2p qo;
        qo.x = 0.0; qo.y = 0.0;
        if (MODE == 1) qo = *reinterpret_cast<const f64x2p *>(q + i);
        RowPair<C> e;
        pair_load<C, CODED>(e, rq, rv, rc, rcode, dl, p, i);
        const double ra = MODE == 1 ? rr.x - alpha * qo.x : rr.x, rb = MODE == 1 ? rr.y - alpha * qo.y : rr.y;
        if (MODE == 1) {
            f64x2p rn; rn.x = ra; rn.y = rb;
            *reinterpret_cast<f64x2p *>(r + i) = rn;
        }
        double ta = MODE == 2 ? ra / dd.x : ra, tb = MODE == 2 ? rb / dd.y : rb;
        pair_minus_entries<C>(e, ta, tb, dep);
        f64x2p zn;
        zn.x = MODE == 1 ? ta / dd.x : ta;
        zn.y = MODE == 1 ? tb / dd.y : tb;
        *reinterpret_cast<f64x2p *>(z + i) = zn;
        s += ra * zn.x;
        s += rb * zn.y;
    }
    const double tot = block_sum<kBlock>(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// k_trsv_rows for a level that is a run of consecutive rows: two rows per lane, the dependency rows from the 4-bit codes where
// the factor has them (CODED) -- the forms k_trsv_rows_cg2 measured (83 / 69 us against 98 / 79 with one row per lane and
// 4-byte row numbers, n = 1e7).
template <int C, int MODE, bool CODED>
__global__ __launch_bounds__(kBlock) void k_trsv_rows2(const int32_t *__restrict__ rq, const double *__restrict__ rv, int rc,
                                                       const uint32_t *__restrict__ rcode, const int32_t *__restrict__ rdict, int32_t row0,
                                                       int32_t begin, int32_t end, const double *r, double *y, const double *__restrict__ D,
                                                       double *z, int32_t n0, const int *flag)
{
    __shared__ int32_t dl[16];
    if (flag && *flag) return;
    if (CODED) {
        if (threadIdx.x < 16) dl[threadIdx.x] = rdict[threadIdx.x];
        __syncthreads();
    }
    auto dep = [&](int32_t j) -> double { return MODE == 2 ? z[j] : (j < n0 ? r[j] : y[j]); };
    auto one_row = [&](int32_t p, int32_t i) {               // (k_trsv_rows' row)
        double t;
        if (MODE == 2) t = (i < n0 ? r[i] : y[i]) / D[i];
        else t = r[i];
        t = row_minus_entries<C>(t, rq, rv, rc, p, dep);
        if (MODE == 0) y[i] = t;
        else if (MODE == 1) z[i] = t / D[i];
        else z[i] = t;
    };
    // a level that starts at an odd position / row (both odd, its rows on one side of n0: the caller checks): the first row alone
    const int32_t peel = begin & 1;
    if (peel && blockIdx.x == 0 && threadIdx.x == 0 && begin < end) one_row(begin, row0);
    begin += peel;
    row0 += peel;
    const int32_t tiles_per_xcd = gridDim.x >> 3;
    const int32_t tile = (blockIdx.x & 7) * tiles_per_xcd + (blockIdx.x >> 3);
    const int32_t p = begin + tile * 2 * kBlock + 2 * (int32_t)threadIdx.x;
    if (p >= end) return;
    const int32_t i = row0 + (p - begin);
    if (p + 1 >= end) { one_row(p, i); return; }
    // (i even: rows i, i + 1 lie on one side of the even n0 or straddle nothing -- n0 odd is the caller's scalar case)
    const double *src = MODE == 2 ? (i < n0 ? r : y) : r;
    const f64x2p rr = *reinterpret_cast<const f64x2p *>(src + i);
    f64x2p dd;
    dd.x = 1.0; dd.y = 1.0;
    if (MODE != 0) dd = *reinterpret_cast<const f64x2p *>(D + i);
    RowPair<C> e;
    pair_load<C, CODED>(e, rq, rv, rc, rcode, dl, p, i);
    double ta = MODE == 2 ? rr.x / dd.x : rr.x, tb = MODE == 2 ? rr.y / dd.y : rr.y;
    pair_minus_entries<C>(e, ta, tb, dep);
    f64x2p out;
    out.x = MODE == 1 ? ta / dd.x : ta;
    out.y = MODE == 1 ? tb / dd.y : tb;
    *reinterpret_cast<f64x2p *>((MODE == 0 ? y : z) + i) = out;
}


// a run of narrow levels [l0, l1) walked by ONE workgroup.  The row records and right-hand
// sides are independent of the solve, so they are requested D levels ahead (registers; one
// HBM round trip is ~2 us, one level's arithmetic a fraction of that); results of the current
// run live in an LDS ring indexed by position, so the dependencies of the next level are LDS
// reads; anything older than the ring (or produced before this run) is read from xp, which
// the workgroup fence + barrier before a ring wrap keeps valid.  RPT = rows per lane and
// level (levels of up to RPT*1024 rows); RPT*D records are in flight per lane.
template <int RPT, int D>
__global__ __launch_bounds__(kTrsvBlock) void k_trsv_walk(const TrsvRec *__restrict__ recs,
                                                          const int32_t *__restrict__ pq,
                                                          const double *__restrict__ pv,
                                                          const int32_t *__restrict__ level_ptr, int32_t l0,
                                                          int32_t l1, int32_t n, double *xp, const int *flag)
{
    // Every prefetch load and every result store is issued by ALL lanes on EVERY level (lanes
    // without a row use a clamped record and the scratch slots xp[n + lane]): the compiler can
    // then count the younger requests exactly and waits for a prefetched record with
    // s_waitcnt vmcnt(k > 0); a conditional load or store in the loop would turn every wait
    // into vmcnt(0), i.e. one HBM round trip per level.
    __shared__ double ring[kRing];
    if (flag && *flag) return;
    const int tid = threadIdx.x;
    TrsvRec pre[D][RPT];
    double z0pre[D][RPT];
    int32_t lb[D], le[D];
    // a level's bounds are a scalar load: requested at the top of a step (overlaps the LDS
    // reads), consumed by the row requests at its end
    auto bounds = [&](int32_t l, int32_t &b, int32_t &e) {
        const int32_t lc = min(l, l1 - 1);           // past the run: an empty level (requests are clamped)
        b = level_ptr[lc];
        e = level_ptr[lc + 1];
        if (l >= l1) b = e;
    };
    auto fetch = [&](int slot, int32_t b, int32_t e) {
        lb[slot] = b;
        le[slot] = e;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            const int32_t p = b + tid + r * kTrsvBlock;
            const bool ok = p < e;
            pre[slot][r] = recs[ok ? p : n - 1];
            z0pre[slot][r] = xp[ok ? p : n + tid + r * kTrsvBlock];   // right-hand side: only this row ever writes it
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) {
        int32_t b, e;
        bounds(l0 + j, b, e);
        fetch(j, b, e);
    }
    int32_t fpos = level_ptr[l0];   // every position < fpos is visible in xp (written before a workgroup fence)
    for (int32_t l = l0; l < l1; l += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {                // levels past l1 are empty: same instruction stream
            const int32_t b = lb[j], e = le[j];
            int32_t nb, ne;
            bounds(l + j + D, nb, ne);
            if (e - fpos > kRing) {
                // the ring is about to lose positions that were never fenced: make all stores of
                // this run visible in xp first (rare: once per ~2 widest levels at most)
                __threadfence_block();
                __syncthreads();
                fpos = b;
            }
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const int32_t p = b + tid + r * kTrsvBlock;
                const bool ok = p < e;
                const int32_t cnt = ok ? pre[j][r].cnt : 0;
                double z = z0pre[j][r];
                bool fast = cnt <= kInline;
#pragma unroll
                for (int i = 0; i < kInline; ++i) fast = fast & ((i >= cnt) | (pre[j][r].q[i] >= fpos));
                if (fast) {                          // every dependency is in the LDS ring: no memory wait
#pragma unroll
                    for (int i = 0; i < kInline; ++i) {
                        const double t = z - pre[j][r].v[i] * ring[pre[j][r].q[i] & (kRing - 1)];
                        z = i < cnt ? t : z;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < kInline; ++i)      // (static indices: the records stay in registers)
                        if (i < cnt) {
                            const int32_t q = pre[j][r].q[i];
                            const double xv = q >= fpos ? ring[q & (kRing - 1)] : xp[q];
                            z = z - pre[j][r].v[i] * xv;
                        }
                    for (int32_t k = pre[j][r].k0 + kInline; k < pre[j][r].k0 + cnt; ++k) {
                        const int32_t q = pq[k];
                        const double xv = q >= fpos ? ring[q & (kRing - 1)] : xp[q];
                        z = z - pv[k] * xv;
                    }
                }
                if (ok) ring[p & (kRing - 1)] = z;
                xp[ok ? p : n + tid + r * kTrsvBlock] = z;     // drains in the background; readers use the ring
            }
            // slot j is free again: request level l+j+D into the same registers (issued after the
            // last use, so the compiler needs no second register set and no copies at the back-edge)
            fetch(j, nb, ne);
            // level barrier on the LDS ring only: the global stores above stay in flight
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    }
}

// The same walk for runs whose rows all have <= kInline dependencies, every one of them within
// kRing positions below the end of the row's own level (checked on the host at setup; true for
// grid-like factors).  The ring is pre-loaded with the kRing results that precede the run, so
// EVERY dependency is an LDS read: no fence, no branch, and no memory request inside the loop
// other than the D-level-ahead prefetch and the result store -- the loop is one straight
// instruction stream, which lets the compiler wait for a prefetched row with an exact
// s_waitcnt vmcnt(k).  One workgroup on one CU is bound by the CU's memory pipeline (measured:
// 64-byte records, one per lane = 64 cache lines per load instruction, ~0.9 us per 1000-row
// level), so these runs read a structure-of-arrays copy instead: per row ONE 8-byte word of
// four 16-bit ring slots (position & (kRing-1); kRing = "no entry", a slot that holds 0.0 and
// is paired with the value 0.0) and C values, slot-major -- every load is a coalesced 8 bytes
// per lane, C + 3 memory instructions and ~3 ALU instructions per dependency.
// A = adjacent rows per lane (1 or 2): with A = 2 a lane owns rows 2t and 2t+1 of the level and
// every load moves 16 bytes per lane -- half the memory instructions for the same bytes.
template <class T, int A> struct alignas(sizeof(T)) RowPack { T v[A]; };
template <int TB, int RPT, int D, int C, int A>
__global__ __launch_bounds__(TB) void k_trsv_walk_ring(const uint64_t *__restrict__ dq,
                                                       const uint32_t *__restrict__ dq32,
                                                       const double *__restrict__ dv, uint32_t nstride,
                                                       const int32_t *__restrict__ level_ptr, int32_t l0,
                                                       int32_t l1, int32_t n, double *xp, const int *flag)
{
    // ring[kRing] is a constant 0.0 (the slot absent dependencies point at, with value 0.0:
    // z - 0.0*0.0 == z for every z, so they need no branch); ring[kRing+1+..]: parking
    __shared__ double ring[kRing + 1 + 2 * kTrsvBlock];
    if (flag && *flag) return;
    const uint32_t tid = threadIdx.x;
    {
        const int32_t base = level_ptr[l0];
        for (int32_t q = base - 1 - (int32_t)tid; q >= 0 && q >= base - kRing; q -= TB) ring[q & (kRing - 1)] = xp[q];
        if (tid == 0) ring[kRing] = 0.0;
    }
    // byte offsets fit 32 bits (checked on the host): scalar base + 32-bit lane offset addressing
    // (C <= 2 reads the 32-bit copy of the slot words: of a 64-bit word only the low half would
    //  be used, the register allocator would re-use the idle half, and a write to a register
    //  with a load in flight has to wait for that load)
    using WQ = typename std::conditional<(C <= 2), uint32_t, uint64_t>::type;
    const char *dqb = C <= 2 ? reinterpret_cast<const char *>(dq32) : reinterpret_cast<const char *>(dq);
    const char *dvb[C];
#pragma unroll
    for (int i = 0; i < C; ++i) dvb[i] = reinterpret_cast<const char *>(dv + (size_t)i * nstride);
    char *xpb = reinterpret_cast<char *>(xp);
    RowPack<WQ, A> wq[D][RPT];
    RowPack<double, A> wv[D][RPT][C], z0pre[D][RPT];
    int32_t lb[D], le[D];
    auto bounds = [&](int32_t l, int32_t &b, int32_t &e) {
        const int32_t lc = min(l, l1 - 1);           // past the run: an empty level
        b = level_ptr[lc];
        e = level_ptr[lc + 1];
        if (l >= l1) b = e;
    };
    auto fetch = [&](int slot, int32_t b, int32_t e) {
        lb[slot] = b;
        le[slot] = e;
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            // lanes past the level's end read the rows that follow (the arrays are padded by
            // kNarrow entries); what they compute lands in the parking slots
            const uint32_t off = ((uint32_t)b + A * (tid + r * TB)) * 8u;
            wq[slot][r] = *reinterpret_cast<const RowPack<WQ, A> *>(dqb + (C <= 2 ? off / 2 : off));
#pragma unroll
            for (int i = 0; i < C; ++i) wv[slot][r][i] = *reinterpret_cast<const RowPack<double, A> *>(dvb[i] + off);
            z0pre[slot][r] = *reinterpret_cast<const RowPack<double, A> *>(xpb + off);
        }
    };
#pragma unroll
    for (int j = 0; j < D; ++j) {
        int32_t b, e;
        bounds(l0 + j, b, e);
        fetch(j, b, e);
    }
    __syncthreads();
    const char *ringb = reinterpret_cast<const char *>(ring);
    for (int32_t l = l0; l < l1; l += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {                // levels past l1 are empty: same instruction stream
            const int32_t b = lb[j], e = le[j];
            int32_t nb, ne;
            bounds(l + j + D, nb, ne);
#pragma unroll
            for (int r = 0; r < RPT; ++r)
#pragma unroll
                for (int a = 0; a < A; ++a) {
                    const uint32_t lane_row = A * (tid + r * TB) + a;      // < A * RPT * TB <= 2 * kTrsvBlock ... kNarrow
                    const uint32_t p = (uint32_t)b + lane_row;
                    const bool ok = p < (uint32_t)e;
                    double z = z0pre[j][r].v[a];
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const uint32_t slot = (uint32_t)(wq[j][r].v[a] >> (16 * i)) & 0xffffu;     // ring slot of the dependency
                        z = z - wv[j][r][i].v[a] * *reinterpret_cast<const double *>(ringb + slot * 8u);
                    }
                    // rows past the level's end: results go to parking slots nobody reads
                    const uint32_t park = A * tid + a;
                    *reinterpret_cast<double *>(const_cast<char *>(ringb) + (ok ? (p & (kRing - 1)) : kRing + 1 + park) * 8u) = z;
                    *reinterpret_cast<double *>(xpb + (ok ? p : (uint32_t)n + lane_row) * 8u) = z;
                }
            // slot j is free again: request level l+j+D into the same registers (issued after the
            // last use, so the compiler needs no second register set and no copies at the back-edge)
            fetch(j, nb, ne);
            // level barrier on the LDS ring only: the global stores above stay in flight
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            // keep the next level's address arithmetic below this point: hoisted above, it would
            // pull the wait for that level's (still in flight) row up here
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ---- strip-pipelined triangular solve (GridTri) ------------------------------------------------
// ONE launch per triangular solve, one workgroup of two waves per 64-column strip, all strips running at once:
//   chain wave   walks its strip top to bottom.  A step = shift the previous results one lane up (DPP wave_shr,
//                no LDS on the chain), two products, two subtractions in the row's STORED order (an absent
//                dependency contributes an exact 0.0 whatever its operand holds).  Its only vector-memory traffic is
//                the 32-byte records DEPTH steps ahead (static register slots: exact vmcnt waits) and the result
//                store; lane 0's left neighbours come out of an LDS ring, lane 63's results go into another.
//   helper waves talk to the neighbours: one forwards this strip's edge values to memory, one loads the left strip's
//                into the LDS ring -- sc1 (agent-scope relaxed) accesses, valid across XCDs.  The edge values are their
//                own flags (kEdgeEmpty until written): a hand-off costs one memory round trip.
// Strip ib only ever waits for strip ib-1 -- a workgroup with a smaller index, dispatched no later -- so the launch
// cannot deadlock; every wait loop is bounded all the same and raises the abort word instead of hanging.
// register slots = records in flight per lane (16: 0.91 / 1.81 ms per PCG iteration at 1000^2 / 2000^2, 32: 0.85 / 1.66).  With
// all 32 in flight -- 3 memory operations per step, vmcnt counts to 63 -- the compiler drains the queue once per trip of the
// unrolled loop; the kernel's LA parameter (fewer steps in flight than slots) is there for that experiment.  The launcher
// instantiates this one depth with LA = DEPTH.
constexpr int kStripDepth = 32;
constexpr int kStripChunk = 8;           // steps between LDS hand-offs
constexpr int kStripRing = 512;          // edge values the LDS rings hold (steps)
// ORDER: 0 = every row subtracts its r-w term first, 1 = every row its r-1 term first, 2 = per-row flag (bit 2)
template <int DEPTH, int CH, int ORDER, int LA = DEPTH>
__global__ __launch_bounds__(192) void k_trsv_strip(int32_t NI, int32_t S, const StripRec *__restrict__ rec, double *__restrict__ xp,
                                                    double *edge, int32_t *progress, const int *flag, int spin_limit, int32_t *sticky)
{
    __shared__ double in_ring[kStripRing], out_ring[kStripRing], out_scratch[64 + CH];
    __shared__ int in_avail, out_count, out_sent, lds_abort; // steps of left-edge values available / produced by the chain / forwarded
    if (flag && *flag) return;
    // (tried: a grid of 8 x NI in which only every eighth workgroup works, so that all strips sit on ONE XCD and one L2 serves
    // the hand-offs -- 0.83 vs 0.87 ms at 1000^2, 2.06 vs 1.85 at 2000^2: within noise, gone)
    const int lane = threadIdx.x & 63;
    const bool chain = threadIdx.x < 64;
    const int32_t ib = blockIdx.x;
    int32_t *abort_word = progress + NI;
    if (threadIdx.x == 0) { in_avail = ib == 0 ? S + kStripRing : 0; out_count = 0; out_sent = 0; lds_abort = 0; }
    for (int q = threadIdx.x; q < kStripRing; q += 192) { in_ring[q] = 0.0; out_ring[q] = 0.0; }
    __syncthreads();
    if (chain) {
        const int64_t base = (int64_t)ib * S * 64;
        const f64x2s *R = reinterpret_cast<const f64x2s *>(rec + base + lane);     // 2 x 16 bytes per record
        double *X = xp + base + lane;
        f64x2s ra[DEPTH], rb[DEPTH];
        auto fetch = [&](int slot, int32_t t) {
            const int32_t tc = min(t, S - 1);
            ra[slot] = R[(int64_t)tc * 128];          // (plain loads: the records are re-read by every apply)
            rb[slot] = R[(int64_t)tc * 128 + 1];
        };
#pragma unroll
        // look-ahead LA steps of the DEPTH register slots: two loads and a store per step, and vmcnt counts to 63
        for (int j = 0; j < LA; ++j) fetch(j, j);
        const long long clk0 = wall_clock64();
        double prev = 0.0;
        double eE[CH];                       // lane 0's left neighbours of the current chunk (read out of the ring at its start)
        double *ow = &out_scratch[lane];     // where this lane's results of the current chunk go in LDS
        for (int32_t t0 = 0; t0 < S; t0 += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                const int32_t t = t0 + j;
                if (j % CH == 0) {
                    // lane 0's left neighbours of this chunk must be in the ring
                    int spins = 0;
                    // ... and the helper must have forwarded what the out ring is about to overwrite
                    while (__hip_atomic_load(&in_avail, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < t + CH ||
                           t + CH - __hip_atomic_load(&out_sent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) > kStripRing - CH) {
                        __builtin_amdgcn_s_sleep(1);
                        if (++spins > spin_limit || __hip_atomic_load(&lds_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                            if (lane == 0) raise_abort(abort_word, sticky);
                            return;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < CH; ++u) eE[u] = in_ring[(t + u) & (kStripRing - 1)];
                    ow = lane == 63 ? &out_ring[t & (kStripRing - 1)] : &out_scratch[lane];
                }
                const double left = dpp_shift_up(prev, eE[j % CH]);
                double z = rb[j].x;
                if (ORDER == 2) {                       // per-row order: flag word (bit0 has r-w, bit1 has r-1, bit2 r-1 first)
                    const uint32_t cc = (uint32_t)__double_as_longlong(rb[j].y);
                    const double pS = (cc & 1u) ? ra[j].x * prev : 0.0;
                    const double pW = (cc & 2u) ? ra[j].y * left : 0.0;
                    const bool wfirst = (cc & 4u) != 0;
                    z = z - (wfirst ? pW : pS);
                    z = z - (wfirst ? pS : pW);
                } else {                                // uniform order: the code word holds two 32-bit AND masks (all ones = present)
                    const uint64_t mk = (uint64_t)__double_as_longlong(rb[j].y);
                    const uint32_t mS = (uint32_t)mk, mW = (uint32_t)(mk >> 32);
                    const double rS = ra[j].x * prev, rW = ra[j].y * left;
                    const double pS = __hiloint2double(__double2hiint(rS) & (int)mS, __double2loint(rS) & (int)mS);
                    const double pW = __hiloint2double(__double2hiint(rW) & (int)mW, __double2loint(rW) & (int)mW);
                    z = z - (ORDER == 1 ? pW : pS);
                    z = z - (ORDER == 1 ? pS : pW);
                }
                __builtin_nontemporal_store(z, X + (int64_t)t * 64);
                ow[j % CH] = z;                         // lane 63: the out ring; the other lanes: scratch
                prev = z;
                fetch((j + LA) % DEPTH, t + LA);
                if (j % CH == CH - 1 && lane == 0)
                    __hip_atomic_store(&out_count, t + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        // diagnostics (sgm_pc_get "strip_clocks"): start / end of this strip's chain in the two unused tail slots of its edge row
        if (lane == 0) {
            long long *tail = reinterpret_cast<long long *>(edge + (int64_t)ib * (S + kEdgePad) + S + 64);
            tail[0] = clk0;
            tail[1] = wall_clock64();
        }
        return;
    }
    // ---- helper waves: wave 1 forwards this strip's edge values, wave 2 fetches the left strip's
    const bool forwarder = threadIdx.x < 128;
    double *my_edge = edge + (int64_t)ib * (S + kEdgePad);
    const double *left_edge = edge + (int64_t)(ib > 0 ? ib - 1 : 0) * (S + kEdgePad);
    int spins = 0;
    if (forwarder) {
        // edge values are their own flags (kEdgeEmpty until written, reset before every sweep): no progress word, no wait
        // for the stores to be acknowledged
        int32_t sent = 0;            // steps of this strip's edge values stored
        while (sent < S) {
            const int32_t made = min(__hip_atomic_load(&out_count, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP), S);
            if (made > sent) {
                for (int32_t q = sent + lane; q < made; q += 64)
                    __hip_atomic_store(my_edge + q, out_ring[q & (kStripRing - 1)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane == 0) {
                    __hip_atomic_store(progress + ib, made, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);         // (diagnostics only)
                    __hip_atomic_store(&out_sent, made, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                sent = made;
                spins = 0;
                continue;
            }
            __builtin_amdgcn_s_sleep(4);            // (the helpers share the CU's LDS and memory pipeline with the chain wave: poll gently)
            if (++spins > spin_limit || __hip_atomic_load(&lds_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
                if (lane == 0) raise_abort(abort_word, sticky);
                return;
            }
        }
        // the right strip reads 63 entries past the last step (padding rows there: any value that is not kEdgeEmpty)
        __hip_atomic_store(my_edge + S + lane, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    if (ib == 0) return;
    int32_t got = 0;                 // steps of left-edge values copied into the ring; lane 0 at step t needs the left strip's step t + 63
    while (got < S) {
        // never more than a ring ahead of what the chain has consumed (it has produced out_count steps)
        const int32_t done = __hip_atomic_load(&out_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int32_t room = done + kStripRing - 2 * CH;
        if (got - done > 128) { __builtin_amdgcn_s_sleep(32); continue; }       // comfortably ahead of the chain: stay out of its way
        const int32_t cnt = min(64, min(S, room) - got);
        if (cnt > 0) {
            // ONE memory round trip per look: load the next entries and keep the leading ones that have been written
            double v = 0.0;
            if (lane < cnt) v = __hip_atomic_load(left_edge + got + 63 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool ok = lane >= cnt || (unsigned long long)__double_as_longlong(v) != kEdgeEmpty;
            const unsigned long long miss = ~__ballot(ok);
            const int32_t nvalid = miss ? min(cnt, (int32_t)__builtin_ctzll(miss)) : cnt;
            if (nvalid > 0) {
                if (lane < nvalid) in_ring[(got + lane) & (kStripRing - 1)] = v;
                got += nvalid;
                if (lane == 0) __hip_atomic_store(&in_avail, got >= S ? S + kStripRing : got, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                spins = 0;
                continue;
            }
        }
        __builtin_amdgcn_s_sleep(1);
        if (++spins > spin_limit || __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
            __hip_atomic_load(&lds_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
            if (lane == 0) {
                raise_abort(abort_word, sticky);
                __hip_atomic_store(&lds_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            return;
        }
    }
}
// position-space gather / hand-over of the strip path (padding positions hold 0; the scatter back is k_pos_scatter, sgm_trsv_device.hpp)
// (gather and transition also clear the progress words of the sweep that follows)
__global__ void k_grid_gather(int64_t np, StripRec *__restrict__ rec, const double *__restrict__ src,
                              const int32_t *__restrict__ row, int32_t *__restrict__ progress, int32_t nprog,
                              unsigned long long *__restrict__ edge, int64_t nedge, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = p; q < nprog; q += stride) progress[q] = 0;
    for (int64_t q = p; q < nedge; q += stride) edge[q] = kEdgeEmpty;
    for (; p < np; p += stride) { const int32_t r = row[p]; rec[p].rhs = r >= 0 ? src[r] : 0.0; }
}
__global__ void k_grid_transition(int64_t np, StripRec *__restrict__ recU, const double *__restrict__ xpL,
                                  const int32_t *__restrict__ mapLU, const double *__restrict__ Dp, int32_t *__restrict__ progress,
                                  int32_t nprog, unsigned long long *__restrict__ edge, int64_t nedge, const int *flag)
{
    if (flag && *flag) return;
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = p; q < nprog; q += stride) progress[q] = 0;
    for (int64_t q = p; q < nedge; q += stride) edge[q] = kEdgeEmpty;
    for (; p < np; p += stride) { const int32_t q = mapLU[p]; recU[p].rhs = q >= 0 ? xpL[q] / Dp[p] : 0.0; }   // x = x / D
}

// ------------------------------------------------------------------------------ launchers
// Run-time values as template arguments (Int<>, Flag<>, with_flag: sgm_internal.hpp): f is called once.
// v = LO .. 2: the MODE of a row-space sweep (the fused CG kernels have no MODE 0), the ORDER of a strip factor
template <int LO, class F> void with_upto2(int v, F &&f)
{
    if constexpr (LO == 0) { if (v == 0) return f(Int<0>{}); }
    if (v == 1) return f(Int<1>{});
    f(Int<2>{});
}
// most entries of a row of a row-space level -> the C of its kernel: unrolled for 0 .. 4, 6 and 8 slots -- 5 and 7 read one
// padding slot, which rows_commit (sgm_ildu.hip) sizes the slot arrays for -- and the slot loop (-1) beyond
template <class F> void with_row_slots(int c, F &&f)
{
    switch (c) {
    case 0: return f(Int<0>{});
    case 1: return f(Int<1>{});
    case 2: return f(Int<2>{});
    case 3: return f(Int<3>{});
    case 4: return f(Int<4>{});
    case 5: case 6: return f(Int<6>{});
    case 7: case 8: return f(Int<8>{});
    default: return f(Int<-1>{});
    }
}
constexpr bool pair_slots(int C) { return C >= 1 && C <= 4; }          // the two-rows-per-lane kernels exist for these
// most dependencies of a row of a walkers' level (<= kInline) -> the slots its structure-of-arrays kernel reads
template <class F> void with_soa_slots(int c, F &&f)
{
    if (c <= 2) return f(Int<2>{});
    if (c == 3) return f(Int<3>{});
    f(Int<4>{});
}
// the structure-of-arrays kernels address a slot with 32-bit byte offsets: 8 bytes * nstride must fit
bool offsets32(const TriFactor &T) { return T.nstride < (size_t)500000000; }

// one strip-pipelined sweep: G's records hold the right-hand side on entry, xp the solution on exit
void trsv_grid(const GridTri &G, double *xp, const int *flag, int spin_limit, int32_t *sticky)
{
    // 96 KiB of (unused) dynamic LDS per workgroup: at most ONE strip per CU, so that no two chain waves share a SIMD
    constexpr size_t lds_pad = (size_t)96 * 1024;
    with_upto2<0>(G.order, [&](auto O) {
        const auto kernel = k_trsv_strip<kStripDepth, kStripChunk, decltype(O)::value, kStripDepth>;
        static bool attr = false;            // (one per ORDER: a static of this instantiation of the lambda)
        if (!attr) { (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_pad); attr = true; }
        hipLaunchKernelGGL(kernel, dim3(G.NI), dim3(192), lds_pad, g_rt.stream, G.NI, G.S, (const StripRec *)G.rec, xp, G.edge, G.progress,
                           flag, spin_limit, sticky);
    });
}

// one level of a row-space sweep (mode: k_trsv_rows' MODE)
void launch_rows(const TriFactor &T, const TriFactor::RowLevel &L, int mode, const double *r, double *y, const double *D, double *z,
                 int32_t n0, const int *flag)
{
    hipStream_t st = g_rt.stream;
    const int32_t b = L.b, e = L.e;
    // two rows per lane: row and position of the level of one parity (an odd start is peeled), and no pair astride n0 -- n0 even, or
    // the level's rows all on one side of it with the pairs aligned to the level's own start
    const bool pairs_ok = L.row0 >= 0 && ((L.row0 ^ b) & 1) == 0 &&
                          (((n0 & 1) == 0 && (L.row0 & 1) == 0) || L.row0 >= n0 || L.row0 + (e - b) <= n0);
    const bool pairs = pairs_ok && pair_slots(L.c);
    const int per_block = pairs ? 2 * kBlock : kBlock;
    const dim3 g(8 * (((e - b + per_block - 1) / per_block + 7) / 8));      // (a multiple of 8: see the tile map in the kernels)
    with_row_slots(L.c, [&](auto Cc) { with_upto2<0>(mode, [&](auto Mm) {
        constexpr int C = decltype(Cc)::value, M = decltype(Mm)::value;
        if (!pairs)
            hipLaunchKernelGGL((k_trsv_rows<C, M>), g, dim3(kBlock), 0, st, (const int32_t *)T.rq, (const double *)T.rv, T.rc,
                               (const int32_t *)T.order, L.row0, b, e, r, y, D, z, n0, flag);
        else if constexpr (pair_slots(C))
            with_flag(T.rcode != nullptr, [&](auto CODED) {
                hipLaunchKernelGGL((k_trsv_rows2<C, M, decltype(CODED)::value>), g, dim3(kBlock), 0, st, (const int32_t *)T.rq, (const double *)T.rv, T.rc,
                                   (const uint32_t *)T.rcode, (const int32_t *)T.rdict, L.row0, b, e, r, y, D, z, n0, flag);
            });
    }); });
}

constexpr int kRowsCgGrid = 2048;            // blocks per launch (grid-stride): 2 x 2048 partial sums <= kMaxGrid
void launch_rows_cg(const TriFactor &T, const TriFactor::RowLevel &L, int mode, double *r, const double *q, ScalarRef res2, ScalarRef dpr,
                    const double *D, double *z, double *part, int grid, const int *flag, int gen)
{
    hipStream_t st = g_rt.stream;
    const bool pairs = L.row0 >= 0 && ((L.row0 ^ L.b) & 1) == 0 && pair_slots(L.c);      // (both even, or both odd: the kernel peels the first row)
    with_row_slots(L.c, [&](auto Cc) { with_upto2<1>(mode, [&](auto Mm) {
        constexpr int C = decltype(Cc)::value, M = decltype(Mm)::value;
        if (!pairs)
            hipLaunchKernelGGL((k_trsv_rows_cg<C, M>), dim3(grid), dim3(kBlock), 0, st, (const int32_t *)T.rq, (const double *)T.rv, T.rc,
                               (const int32_t *)T.order, L.row0, L.b, L.e, r, q, res2, dpr, D, z, part, flag, gen);
        else if constexpr (pair_slots(C))
            with_flag(T.rcode != nullptr, [&](auto CODED) {
                hipLaunchKernelGGL((k_trsv_rows_cg2<C, M, decltype(CODED)::value>), dim3(grid), dim3(kBlock), 0, st, (const int32_t *)T.rq, (const double *)T.rv,
                                   T.rc, (const uint32_t *)T.rcode, (const int32_t *)T.rdict, L.row0, L.b, L.e, r, q, res2, dpr, D, z, part,
                                   flag, gen);
            });
    }); });
}

// triangular solve in position space: xp holds the right-hand side on entry, the solution on exit
void trsv(const TriFactor &T, double *xp, const int *flag)
{
    const int32_t n = (int32_t)T.h_order.size();
    hipStream_t st = g_rt.stream;
    for (const auto &L : T.schedule) {
        if (L.narrow) {
            auto walk = [&](auto R, auto DD) {            // rows per lane, levels requested ahead
                hipLaunchKernelGGL((k_trsv_walk<decltype(R)::value, decltype(DD)::value>), dim3(1), dim3(kTrsvBlock), 0, st,
                                   (const TrsvRec *)T.recs, (const int32_t *)T.pq, (const double *)T.pv, (const int32_t *)T.level_ptr_dev,
                                   L.l0, L.l1, n, xp, flag);
            };
            auto ring = [&](auto TB, auto R, auto DD, auto A) { with_soa_slots(L.c, [&](auto C) {      // threads, the two, adjacent rows per lane
                constexpr int tb = decltype(TB)::value;
                const auto kernel = k_trsv_walk_ring<tb, decltype(R)::value, decltype(DD)::value, decltype(C)::value, decltype(A)::value>;
                hipLaunchKernelGGL(kernel, dim3(1), dim3(tb), 0, st, (const uint64_t *)T.dq, (const uint32_t *)T.dq32, (const double *)T.dv,
                                   (uint32_t)T.nstride, (const int32_t *)T.level_ptr_dev, L.l0, L.l1, n, xp, flag);
            }); };
            if (L.ring && offsets32(T)) {
                // class = widest level of the run: <= 256, 512, 1024, 2048, 4096 rows (two rows per lane pair from 512 on)
                // (-1: levels of at most 64 rows -- chains: ONE wave, whose level barrier costs nothing)
                if (L.cls < 0) ring(Int<64>{}, Int<1>{}, Int<4>{}, Int<1>{});
                else if (L.cls == 0) ring(Int<256>{}, Int<1>{}, Int<4>{}, Int<1>{});
                else if (L.cls == 1) ring(Int<256>{}, Int<1>{}, Int<4>{}, Int<2>{});
                else if (L.cls == 2) ring(Int<512>{}, Int<1>{}, Int<4>{}, Int<2>{});
                else if (L.cls == 3) ring(Int<1024>{}, Int<1>{}, Int<2>{}, Int<2>{});
                else ring(Int<1024>{}, Int<2>{}, Int<1>{}, Int<2>{});
            } else if (L.cls <= 2) walk(Int<1>{}, Int<2>{});
            else if (L.cls == 3) walk(Int<2>{}, Int<1>{});
            else walk(Int<4>{}, Int<1>{});
        } else {
            const int32_t b = T.level_ptr[L.l0], e = T.level_ptr[L.l1];
            const dim3 g((e - b + kBlock - 1) / kBlock);
            if (L.c <= kInline && offsets32(T))
                with_soa_slots(L.c, [&](auto C) {
                    hipLaunchKernelGGL((k_trsv_wide_soa<decltype(C)::value>), g, dim3(kBlock), 0, st, (const int32_t *)T.wq, (const double *)T.dv,
                                       (uint32_t)T.nstride, b, e, xp, flag);
                });
            else
                hipLaunchKernelGGL(k_trsv_wide, g, dim3(kBlock), 0, st, (const TrsvRec *)T.recs, (const int32_t *)T.pq,
                                   (const double *)T.pv, b, e, xp, flag);
        }
    }
}

}  // namespace

namespace sgm {

// z = (I+U)^-1 D^-1 (I+L)^-1 r through the strip path
void apply_grid(const IlduState *S, const double *r, double *z, const int *flag, int spin_limit, int32_t *sticky)
{
    hipStream_t st = g_rt.stream;
    const int gl = vec_grid(S->gL.NP), gu = vec_grid(S->gU.NP);
    hipLaunchKernelGGL(k_grid_gather, dim3(gl), dim3(kBlock), 0, st, S->gL.NP, S->gL.rec, r, (const int32_t *)S->gL.row, S->gL.progress,
                       S->gL.NI + 1, reinterpret_cast<unsigned long long *>(S->gL.edge), (int64_t)S->gL.NI * (S->gL.S + kEdgePad), flag);
    trsv_grid(S->gL, S->gxL, flag, spin_limit, sticky);                                       // (I+L) x = b
    hipLaunchKernelGGL(k_grid_transition, dim3(gu), dim3(kBlock), 0, st, S->gU.NP, S->gU.rec, (const double *)S->gxL,
                       (const int32_t *)S->gmapLU, (const double *)S->gDp, S->gU.progress, S->gU.NI + 1,
                       reinterpret_cast<unsigned long long *>(S->gU.edge), (int64_t)S->gU.NI * (S->gU.S + kEdgePad), flag);       // x = x / D
    trsv_grid(S->gU, S->gxU, flag, spin_limit, sticky);                                       // (I+U) x = x
    hipLaunchKernelGGL(k_pos_scatter, dim3(gu), dim3(kBlock), 0, st, S->gU.NP, z, (const double *)S->gxU,
                       (const int32_t *)S->gU.row, flag);
}

// the lower sweep's result of the last apply_grid, out of position space (the setup self-check; slab3_lower_result's twin)
void grid_lower_result(const IlduState *S, double *dst)
{
    hipLaunchKernelGGL(k_pos_scatter, dim3(vec_grid(S->gL.NP)), dim3(kBlock), 0, g_rt.stream, S->gL.NP, dst, (const double *)S->gxL,
                       (const int32_t *)S->gL.row, (const int *)nullptr);
}

// z = (I+U)^-1 D^-1 (I+L)^-1 r through the level-scheduled walkers
void apply_levels(const IlduState *S, const double *r, double *z, const int *flag)
{
    hipStream_t st = g_rt.stream;
    const int64_t n = S->n;
    const int g = vec_grid(n);
    hipLaunchKernelGGL(k_perm_gather, dim3(g), dim3(kBlock), 0, st, n, S->xpL, r, (const int32_t *)S->L.order, flag);
    trsv(S->L, S->xpL, flag);                                             // (I+L) x = b
    hipLaunchKernelGGL(k_lu_transition, dim3(g), dim3(kBlock), 0, st, n, S->xpU, (const double *)S->xpL,
                       (const int32_t *)S->mapLU, (const double *)S->Dp, flag);                     // x = x / D
    trsv(S->U, S->xpU, flag);                                             // (I+U) x = x
    hipLaunchKernelGGL(k_perm_scatter, dim3(g), dim3(kBlock), 0, st, n, z, (const double *)S->xpU,
                       (const int32_t *)S->U.order, flag);
}

// the same through the row-space levels (both factors a few wide levels): one launch per level, nothing else
// (fused: ildu_rows = 1 -- L's first level, when it is rows 0 .. n0-1 without entries, is not copied; the L level that is
// also U's level 0 is finished in the L sweep.  ildu_rows = 2 launches every level of both sweeps.)
void apply_rows(const IlduState *S, const double *r, double *z, const int *flag)
{
    const auto &Ls = S->L.row_levels, &Us = S->U.row_levels;
    const bool fused = S->opt.ildu_rows == 1;
    const int32_t n0 = fused ? S->rows_n0 : 0;
    const bool fin = fused && S->rows_fin;
    for (size_t k = n0 > 0 ? 1 : 0; k < Ls.size(); ++k)                    // (I+L) y = r
        launch_rows(S->L, Ls[k], fin && k + 1 == Ls.size() ? 1 : 0, r, S->xpL, S->D, z, n0, flag);
    for (size_t k = fin ? 1 : 0; k < Us.size(); ++k)                       // (I+U) z = y / D
        launch_rows(S->U, Us[k], 2, r, S->xpL, S->D, z, n0, flag);
}

// *count = partial sums left in `part` (the caller has updated the entry-less rows 0 .. rows_n0-1 of r: pc_cg_fused_rows)
void rows_cg_fused(const IlduState *S, ScalarRef res2, ScalarRef dpr, const double *q, double *r, double *z, double *part, int *count,
                   const int *flag, int gen)
{
    const auto &L1 = S->L.row_levels[1], &U1 = S->U.row_levels[1];
    auto grid_for = [](int32_t rows) { return 8 * std::max(1, std::min(kRowsCgGrid / 8, ((rows + kBlock - 1) / kBlock + 7) / 8)); };
    const int g1 = grid_for(L1.e - L1.b), g2 = grid_for(U1.e - U1.b);
    launch_rows_cg(S->L, L1, 1, r, q, res2, dpr, S->D, z, part, g1, flag, gen);
    launch_rows_cg(S->U, U1, 2, r, q, res2, dpr, S->D, z, part + g1, g2, flag, gen);
    *count = g1 + g2;
}

void scale_by(int64_t n, const double *d, const double *r, double *z, const int *flag)
{
    hipLaunchKernelGGL(k_scale_by, dim3(vec_grid(n)), dim3(kBlock), 0, g_rt.stream, n, d, r, z, flag);
}

}  // namespace sgm
