// ILDU(0) setup (ldu_solvers.f90:95-176, :275-440) of one diagonal block: pattern, factorisation, and every structure the
// sweeps of sgm_trsv.hip / sgm_trsv3.hip read.
//
// On the DEVICE: the pattern pass (k_ildu_count / _split) and the factorisation (k_ildu_init, k_ildu_factor_level*).  The
// reference's algorithm is a sequential IKJ sweep built on get/set/add_value row scans; row i only reads rows k < i of its L
// pattern, so the rows of one dependency level of L run side by side, each lane executing its row's statements in the
// reference's order -- L-I, D, U-I are bit-identical.  Also on the device: the dependency levels of a factor of a few levels
// (tri_levels_device), the grid / slab detection (grid_width_device, slab_dims_device), the anti-diagonal order, the strip
// layout (build_grid), the row-space copies, and the values of every structure at every setup.
// On the HOST: the dependency levels of a factor of MANY levels (tri_levels, from a host copy of the pattern), the level
// walkers' index work (tri_walkers), the factorisation of a factor that is a chain (ildu_factor_row row after row), the grid
// detection as a fall-back (grid_width), and lazy copies for sgm_pc_get.
// A pipelined path is trusted with a pattern only after it has reproduced the row-by-row sweeps on a test vector
// (pipeline_self_check).
#include <hipcub/hipcub.hpp>
#include "sgm_pc_internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstdlib>

using namespace sgm;

namespace {

// ---- ILDU(0) on the device ----------------------------------------------------------------------------------------
// get_value / set_value / add_value of the reference's csr_matrix on one row of a factor (cs_matrices.f90: a scan of the
// row; the LAST matching entry answers a get, EVERY matching entry takes a set / add)
__host__ __device__ inline double row_get(const int32_t *node, const double *val, int32_t b, int32_t e, int32_t j)
{
    double z = 0.0;
    for (int32_t k = b; k < e; ++k)
        if (node[k] == j) z = val[k];
    return z;
}
__host__ __device__ inline void row_set(const int32_t *node, double *val, int32_t b, int32_t e, int32_t j, double z)
{
    for (int32_t k = b; k < e; ++k)
        if (node[k] == j) val[k] = z;
}
__host__ __device__ inline void row_add(const int32_t *node, double *val, int32_t b, int32_t e, int32_t j, double z)
{
    for (int32_t k = b; k < e; ++k)
        if (node[k] == j) val[k] = val[k] + z;
}

// incomplete_ldu_sparsity_pattern, level 0 (ldu_solvers.f90:397-440): entries of A in stored order, i > j -> L,
// j > i -> U.  Two passes over the rows of the part's diagonal block (columns >= ncol_own are halo slots: dropped):
// counts (an exclusive scan between the launches makes the row pointers), fill.
__global__ void k_ildu_count(int32_t n, int32_t ncol_own, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                             int32_t *__restrict__ lcnt, int32_t *__restrict__ ucnt, int32_t *longest)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    int32_t l = 0, u = 0;
    if (i < n)
        for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
            const int32_t j = col[k];
            if (j >= ncol_own) continue;
            l += j < i;
            u += j > i;
        }
    lcnt[i] = l;                 // (slot n: 0 -- the scan's total lands there)
    ucnt[i] = u;
    if (l) atomicMax(longest, l);
    if (u) atomicMax(longest + 1, u);
}
__global__ void k_ildu_split(int32_t n, int32_t ncol_own, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                             const int32_t *__restrict__ Lptr, int32_t *__restrict__ Lnode,
                             const int32_t *__restrict__ Uptr, int32_t *__restrict__ Unode)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t l = Lptr[i], u = Uptr[i];
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j >= ncol_own) continue;
        if (j < i) Lnode[l++] = j;
        else if (j > i) Unode[u++] = j;
    }
}

// Dependency levels of a strictly triangular pattern on the device, for factors of a FEW levels (colour orderings):
// level(i) = 1 + max level(node) over the row's entries, relaxed in place until nothing moves (<= levels sweeps; values
// only grow and never pass the true level).  flags[0]: something moved; flags[1]: a level reached `cap` -- too many
// levels for this path, the host computes them.
__global__ void k_level_relax(int32_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ node, int32_t *level,
                              int32_t cap, int32_t *flags)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t lv = 0;
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) lv = max(lv, level[node[k]] + 1);
    if (lv != level[i]) {
        level[i] = lv;
        flags[0] = 1;
        if (lv >= cap) flags[1] = 1;
    }
}
// (a handful of levels: the counts are gathered per workgroup in LDS first -- millions of atomics on two addresses crawl)
__global__ void k_level_hist(int32_t n, const int32_t *__restrict__ level, int32_t *__restrict__ count, int32_t *__restrict__ rows)
{
    __shared__ int32_t h[kRowLevels + 2];
    for (int q = threadIdx.x; q < kRowLevels + 2; q += blockDim.x) h[q] = 0;
    __syncthreads();
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        atomicAdd(&h[level[i]], 1);
        rows[i] = i;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kRowLevels + 2; q += blockDim.x)
        if (h[q]) atomicAdd(count + q, h[q]);
}
// per level (positions [begin[l], begin[l+1]) of the level order): most entries of a row, whether its rows are consecutive,
// its first row
__global__ void k_level_info(int32_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ level,
                             const int32_t *__restrict__ ptr, const int32_t *__restrict__ begin, int32_t *cmax, int32_t *notrun,
                             int32_t *first)
{
    __shared__ int32_t m[kRowLevels + 2], nr[kRowLevels + 2];
    for (int q = threadIdx.x; q < kRowLevels + 2; q += blockDim.x) { m[q] = 0; nr[q] = 0; }
    __syncthreads();
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) {
        const int32_t i = order[p], l = level[i];
        atomicMax(&m[l], ptr[i + 1] - ptr[i]);
        if (p == begin[l]) first[l] = i;
        else if (order[p - 1] + 1 != i) nr[l] = 1;
    }
    __syncthreads();
    for (int q = threadIdx.x; q < kRowLevels + 2; q += blockDim.x) {
        if (m[q]) atomicMax(cmax + q, m[q]);
        if (nr[q]) notrun[q] = 1;
    }
}

// grid_width on the device (the host version below reads a host copy of the pattern; this one keeps it where it is).
// Pass 1: info[0] / info[1] = smallest / largest dependency distance > 1, info[2] = some row breaks the shape (a
// dependency on the wrong side, more than two entries, the same column twice).  Pass 2, with the width w those agree on:
// info[3] = an r-1 / r+1 dependency across a grid line, or a distance that is neither 1 nor w.
__global__ void k_grid_detect1(int32_t n, int lower, const int32_t *__restrict__ ptr, const int32_t *__restrict__ node, int32_t *info)
{
    __shared__ int32_t lo, hi, bad;
    if (threadIdx.x == 0) { lo = INT32_MAX; hi = 0; bad = 0; }
    __syncthreads();
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) {
        const int32_t b = ptr[r], cnt = ptr[r + 1] - b;
        if (cnt > 2 || (cnt == 2 && node[b] == node[b + 1])) bad = 1;
        for (int32_t k = b; k < b + cnt; ++k) {
            const int32_t dlt = lower ? r - node[k] : node[k] - r;
            if (dlt <= 0) bad = 1;
            else if (dlt > 1) { atomicMin(&lo, dlt); atomicMax(&hi, dlt); }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (lo != INT32_MAX) { atomicMin(info, lo); atomicMax(info + 1, hi); }
        if (bad) info[2] = 1;
    }
}
__global__ void k_grid_detect2(int32_t n, int lower, int32_t w, const int32_t *__restrict__ ptr, const int32_t *__restrict__ node, int32_t *info)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    for (int32_t k = ptr[r]; k < ptr[r + 1]; ++k) {
        const int32_t dlt = lower ? r - node[k] : node[k] - r;
        if (dlt == 1) { if (lower ? r % w == 0 : (r + 1) % w == 0) info[3] = 1; }
        else if (dlt != w) info[3] = 1;
    }
}
// rows of a w-wide grid keyed by their anti-diagonal i + j: a valid levelling of a factor whose rows depend on r-1 and
// r-w only (each of them one anti-diagonal back) -- the order its rows are factorised in
// (h > 0: a w x h x nk grid, rows depend on r-1, r-w, r-w*h: keyed by i + j + k)
__global__ void k_grid_keys(int32_t n, int32_t w, int32_t h, int32_t *__restrict__ key, int32_t *__restrict__ rows, int32_t *__restrict__ count)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int32_t k = h > 0 ? r % w + (r / w) % h + r / (w * h) : r % w + r / w;
    key[r] = k;
    rows[r] = r;
    atomicAdd(count + k, 1);
}

// sparse_static_pattern_ldu_factorization, first loop (ldu_solvers.f90:300-318): A's entries into L, D, U through
// set_value, row by row in stored order
__global__ void k_ildu_init(int32_t n, int32_t ncol_own, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                            const double *__restrict__ val, const int32_t *__restrict__ Lptr, const int32_t *__restrict__ Lnode,
                            double *Lval, const int32_t *__restrict__ Uptr, const int32_t *__restrict__ Unode, double *Uval,
                            double *D)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t lb = Lptr[i], le = Lptr[i + 1], ub = Uptr[i], ue = Uptr[i + 1];
    for (int32_t k = lb; k < le; ++k) Lval[k] = 0.0;
    for (int32_t k = ub; k < ue; ++k) Uval[k] = 0.0;
    double d = 0.0;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k) {
        const int32_t j = col[k];
        if (j >= ncol_own) continue;
        const double v = val[k];
        if (i > j) row_set(Lnode, Lval, lb, le, j, v);
        else if (j > i) row_set(Unode, Uval, ub, ue, j, v);
        else d = v;
    }
    D[i] = d;
}

// its main loop (ldu_solvers.f90:334-382), the statements of one row in the reference's order; the rows of one
// dependency level of L side by side (row i reads rows k < i of its L pattern only -- final since an earlier level --
// and writes its own).  One lane per row.
__host__ __device__ inline void ildu_factor_row(int32_t i, const int32_t *Lptr, const int32_t *Lnode, double *Lval, const int32_t *Uptr,
                                                const int32_t *Unode, double *Uval, double *D);
__global__ void k_ildu_factor_level(const int32_t *__restrict__ order, int32_t begin, int32_t end,
                                    const int32_t *__restrict__ Lptr, const int32_t *__restrict__ Lnode, double *Lval,
                                    const int32_t *__restrict__ Uptr, const int32_t *__restrict__ Unode, double *Uval, double *D)
{
    const int32_t p = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    ildu_factor_row(order[p], Lptr, Lnode, Lval, Uptr, Unode, Uval, D);
}
// (also run row after row on the HOST for factors that are chains: see factor_chain_on_host -- the same statements compiled with the
// same -ffp-contract=off, the same bits)
__host__ __device__ inline void ildu_factor_row(int32_t i, const int32_t *Lptr, const int32_t *Lnode, double *Lval, const int32_t *Uptr,
                                                const int32_t *Unode, double *Uval, double *D)
{
    const int32_t lb = Lptr[i], le = Lptr[i + 1], ub = Uptr[i], ue = Uptr[i + 1];
    double Di = D[i];
    for (int32_t a = lb; a < le; ++a) {
        const int32_t k = Lnode[a];
        const int32_t kb = Uptr[k], ke = Uptr[k + 1];
        double Lik = row_get(Lnode, Lval, lb, le, k);
        const double Uki = row_get(Unode, Uval, kb, ke, i);
        const double Dk = D[k];
        row_set(Lnode, Lval, lb, le, k, Lik / Dk);
        Lik = Lik / Dk;
        for (int32_t c = lb; c < le; ++c) {
            const int32_t j = Lnode[c];
            if (j > k) {
                const double Ukj = row_get(Unode, Uval, kb, ke, j);
                row_add(Lnode, Lval, lb, le, j, -Lik * Dk * Ukj);
            }
        }
        Di = Di - Lik * Dk * Uki;
        for (int32_t c = ub; c < ue; ++c) {
            const int32_t j = Unode[c];
            const double Ukj = row_get(Unode, Uval, kb, ke, j);
            row_add(Unode, Uval, ub, ue, j, -Lik * Dk * Ukj);
        }
    }
    for (int32_t c = ub; c < ue; ++c) {
        const int32_t k = Unode[c];
        const double Uik = row_get(Unode, Uval, ub, ue, k);
        row_set(Unode, Uval, ub, ue, k, Uik / Di);
    }
    D[i] = Di;
}

// index work of the strips' skewed layout, one lane per row: position of the row, its entries' places in the factor's val
// array (r-w term / r-1 term) and the presence / order bits; flags[0] / [1]: some two-term row has its r-w / r-1 term first.
// The upper factor is the lower one of the reversed numbering: i' = w-1-i, j' = nj-1-j.
__global__ void k_grid_build(int32_t n, int32_t w, int32_t nj, int32_t S, int lower, const int32_t *__restrict__ ptr,
                             const int32_t *__restrict__ node, int32_t *__restrict__ row, int32_t *__restrict__ srcS,
                             int32_t *__restrict__ srcW, uint8_t *__restrict__ code, int32_t *__restrict__ pos, int32_t *flags)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    int32_t i = r % w, j = r / w;
    if (!lower) { i = w - 1 - i; j = nj - 1 - j; }
    const int32_t ib = i / 64, l = i % 64;
    const int64_t p = (int64_t)ib * S * 64 + (int64_t)(j + l) * 64 + l;
    pos[r] = (int32_t)p;
    row[p] = r;
    uint8_t c = 0;
    int seen = 0;
    for (int32_t k = ptr[r]; k < ptr[r + 1]; ++k, ++seen) {
        const int32_t dlt = lower ? r - node[k] : node[k] - r;
        if (dlt == 1) { c |= 2; srcW[p] = k; if (seen == 0) c |= 4; }
        else { c |= 1; srcS[p] = k; }
    }
    code[p] = c;
    if ((c & 3) == 3) flags[(c & 4) ? 1 : 0] = 1;                  // (single-term rows fit either order)
}
__global__ void k_grid_map(int32_t n, const int32_t *__restrict__ posU, const int32_t *__restrict__ posL, int32_t *__restrict__ map)
{
    const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) map[posU[r]] = posL[r];
}

__global__ void k_check_vector(int64_t n, double *__restrict__ r)       // the self-check's right-hand side
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) r[i] = 1.0 + 0.25 * (double)(i % 7) - 0.125 * (double)(i % 3);
}

// One sweep of ldu_solve checked row by row (setup self-check of the pipelined sweeps): row i of the result must be what
// the reference's recurrence (ldu_solvers.f90:227-236, :254-263) makes of the right-hand side and of the RESULT's own
// earlier rows -- t = rhs_i (/ D_i); t = t - val * x(node) over the row's entries in stored order -- bit for bit.  If
// that holds for every row the result IS the sequential sweep's (induction along the dependencies), and every row can
// be checked independently.
__global__ void k_sweep_check(int32_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ node, const double *__restrict__ val,
                              const double *__restrict__ rhs, const double *__restrict__ D, const double *__restrict__ x, int32_t *bad)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double t = rhs[i];
    if (D) t = t / D[i];
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) t = t - val[k] * x[node[k]];
    if (__double_as_longlong(t) != __double_as_longlong(x[i])) atomicAdd(bad, 1);
}

// The same for factors whose rows are short (every row of L at most ML entries, of U at most MU: 5-, 7-, 9-point
// matrices): the row's own entries and the rows k it reads are fetched into registers up front -- five dependent memory
// round trips (order, row pointers, own entries, pointers / D of the rows k, their entries) instead of the eleven or so
// the scans above make one after the other; a launch of a narrow level is nothing but that chain.  Then the same
// statements in the same order on the registers, and one store of the row.
template <int M>
__device__ inline double reg_get(const int32_t (&nd)[M], const double (&vl)[M], int cnt, int32_t j)
{
    double z = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (m < cnt && nd[m] == j) z = vl[m];
    return z;
}
template <int M>
__device__ inline void reg_set(const int32_t (&nd)[M], double (&vl)[M], int cnt, int32_t j, double z)
{
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (m < cnt && nd[m] == j) vl[m] = z;
}
template <int M>
__device__ inline void reg_add(const int32_t (&nd)[M], double (&vl)[M], int cnt, int32_t j, double z)
{
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (m < cnt && nd[m] == j) vl[m] = vl[m] + z;
}
template <int ML, int MU>
__global__ void k_ildu_factor_level_short(const int32_t *__restrict__ order, int32_t begin, int32_t end,
                                          const int32_t *__restrict__ Lptr, const int32_t *__restrict__ Lnode, double *Lval,
                                          const int32_t *__restrict__ Uptr, const int32_t *__restrict__ Unode, double *Uval, double *D)
{
    const int32_t p = begin + blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= end) return;
    const int32_t i = order[p];
    const int32_t lb = Lptr[i], ub = Uptr[i];
    const int dl = Lptr[i + 1] - lb, du = Uptr[i + 1] - ub;
    int32_t ln[ML], un[MU];
    double lv[ML], uv[MU];
#pragma unroll
    for (int m = 0; m < ML; ++m) { ln[m] = m < dl ? Lnode[lb + m] : -1; lv[m] = m < dl ? Lval[lb + m] : 0.0; }
#pragma unroll
    for (int m = 0; m < MU; ++m) { un[m] = m < du ? Unode[ub + m] : -1; uv[m] = m < du ? Uval[ub + m] : 0.0; }
    double Di = D[i];
    int32_t kb[ML];
    int kc[ML];
    double dk[ML];
#pragma unroll
    for (int a = 0; a < ML; ++a) {
        const int32_t k = a < dl ? ln[a] : 0;
        kb[a] = a < dl ? Uptr[k] : 0;
        kc[a] = a < dl ? Uptr[k + 1] - kb[a] : 0;
        dk[a] = a < dl ? D[k] : 1.0;
    }
    int32_t kn[ML][MU];
    double kv[ML][MU];
#pragma unroll
    for (int a = 0; a < ML; ++a)
#pragma unroll
        for (int m = 0; m < MU; ++m) {
            kn[a][m] = m < kc[a] ? Unode[kb[a] + m] : -1;
            kv[a][m] = m < kc[a] ? Uval[kb[a] + m] : 0.0;
        }
#pragma unroll
    for (int a = 0; a < ML; ++a) {
        if (a < dl) {
            const int32_t k = ln[a];
            double Lik = reg_get<ML>(ln, lv, dl, k);
            const double Uki = reg_get<MU>(kn[a], kv[a], kc[a], i);
            const double Dk = dk[a];
            reg_set<ML>(ln, lv, dl, k, Lik / Dk);
            Lik = Lik / Dk;
#pragma unroll
            for (int c = 0; c < ML; ++c) {
                if (c < dl && ln[c] > k) {
                    const double Ukj = reg_get<MU>(kn[a], kv[a], kc[a], ln[c]);
                    reg_add<ML>(ln, lv, dl, ln[c], -Lik * Dk * Ukj);
                }
            }
            Di = Di - Lik * Dk * Uki;
#pragma unroll
            for (int c = 0; c < MU; ++c) {
                if (c < du) {
                    const double Ukj = reg_get<MU>(kn[a], kv[a], kc[a], un[c]);
                    reg_add<MU>(un, uv, du, un[c], -Lik * Dk * Ukj);
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < MU; ++c) {
        if (c < du) {
            const double Uik = reg_get<MU>(un, uv, du, un[c]);
            reg_set<MU>(un, uv, du, un[c], Uik / Di);
        }
    }
#pragma unroll
    for (int m = 0; m < ML; ++m)
        if (m < dl) Lval[lb + m] = lv[m];
#pragma unroll
    for (int m = 0; m < MU; ++m)
        if (m < du) Uval[ub + m] = uv[m];
    D[i] = Di;
}

// values into the structures the applies read
__global__ void k_grid_records(int64_t np, const int32_t *__restrict__ srcS, const int32_t *__restrict__ srcW,
                               const uint8_t *__restrict__ code, int order, const double *__restrict__ val, StripRec *__restrict__ rec)
{
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < np; p += stride) {
        StripRec r;
        r.cS = srcS[p] >= 0 ? val[srcS[p]] : 0.0;
        r.cW = srcW[p] >= 0 ? val[srcW[p]] : 0.0;
        r.rhs = 0.0;
        const uint8_t c = code[p];
        if (order == 2) r.code = c;                                // flag word
        else r.code = ((c & 1) ? 0xffffffffull : 0ull) | ((c & 2) ? 0xffffffff00000000ull : 0ull);   // AND masks
        rec[p] = r;
    }
}
__global__ void k_pos_diag(int64_t np, const int32_t *__restrict__ row, const double *__restrict__ D, double *__restrict__ Dp)
{
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; p < np; p += stride) Dp[p] = row[p] >= 0 ? D[row[p]] : 1.0;
}
__global__ void k_tri_entries(int64_t nnz, const int32_t *__restrict__ src, const double *__restrict__ val, double *__restrict__ pv)
{
    int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; k < nnz; k += stride) pv[k] = val[src[k]];
}
// row-space copy of a factor (k_trsv_rows): slot j of position p = entry j of row order[p] -- its column, its value
__global__ void k_rows_index(int32_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ ptr, const int32_t *__restrict__ node,
                             uint32_t nstride, int rc, int32_t *__restrict__ rq)
{
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t i = order[p], b = ptr[i], cnt = ptr[i + 1] - b;
    for (int j = 0; j < rc; ++j) rq[rs_at(j, p, rc)] = j < cnt ? node[b + j] : -1;
}
__global__ void k_rows_values(int32_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ ptr, const double *__restrict__ val,
                              uint32_t nstride, int rc, double *__restrict__ rv)
{
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t i = order[p], b = ptr[i], cnt = ptr[i + 1] - b;
    for (int j = 0; j < rc; ++j) rv[rs_at(j, p, rc)] = j < cnt ? val[b + j] : 0.0;
}

// distinct offsets (dependency row - own row) of the row-space copy into a 64-slot table (INT32_MIN = free); *overflow: more
__global__ void k_rows_offsets(int32_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ rq, int rc, int32_t *table, int *overflow)
{
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t i = order[p];
    for (int c = 0; c < rc; ++c) {
        const int32_t j = rq[rs_at(c, p, rc)];
        if (j < 0) continue;
        const int32_t d = j - i;
        uint32_t h = ((uint32_t)d * 2654435761u) >> 26;
        int probe = 0;
        for (; probe < 64; ++probe, h = (h + 1) & 63u) {
            int32_t cur = __hip_atomic_load(table + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (almost always: already there)
            if (cur == d) break;
            if (cur == INT32_MIN) {
                cur = atomicCAS(table + h, INT32_MIN, d);
                if (cur == INT32_MIN || cur == d) break;
            }
        }
        if (probe == 64) *overflow = 1;
    }
}
__global__ void k_rows_encode(int32_t n, const int32_t *__restrict__ order, const int32_t *__restrict__ rq, int rc, const int32_t *__restrict__ dict,
                              int ndict, uint32_t *__restrict__ rcode)
{
    __shared__ int32_t dl[16];
    if (threadIdx.x < 16) dl[threadIdx.x] = (int)threadIdx.x < ndict ? dict[threadIdx.x] : INT32_MIN;
    __syncthreads();
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t i = order[p];
    uint32_t code = 0;
    for (int c = 0; c < 8; ++c) {
        uint32_t nib = 15u;
        const int32_t j = c < rc ? rq[rs_at(c, p, rc)] : -1;
        if (j >= 0)
            for (int k = 0; k < ndict; ++k)
                if (dl[k] == j - i) { nib = (uint32_t)k; break; }
        code |= nib << (4 * c);
    }
    rcode[p] = code;
}
// after k_rows_index: the codes, where the factor allows them (see TriFactor::rcode)
int rows_encode(TriFactor &T, int32_t n)
{
    dfree(T.rcode); dfree(T.rdict);
    T.rcode = nullptr; T.rdict = nullptr; T.nrdict = 0;
    if (!T.rows_on || T.rc > 8 || n < 1) return SGM_OK;
    hipStream_t st = g_rt.stream;
    int32_t *table = nullptr;
    struct Guard { int32_t *&t; ~Guard() { dfree(t); } } guard{table};
    SGM_TRY(dalloc(&table, 64 + 1));
    std::vector<int32_t> h(65, INT32_MIN);
    h[64] = 0;
    SGM_HIP(hipMemcpyAsync(table, h.data(), 65 * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rows_offsets, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (const int32_t *)T.order, (const int32_t *)T.rq, T.rc,
                       table, reinterpret_cast<int *>(table + 64));
    SGM_HIP(hipMemcpyAsync(h.data(), table, 65 * 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    std::vector<int32_t> dict;
    for (int k = 0; k < 64; ++k)
        if (h[k] != INT32_MIN) dict.push_back(h[k]);
    if (h[64] != 0 || dict.size() > 15) return SGM_OK;
    std::sort(dict.begin(), dict.end());
    dict.resize(16, 0);
    T.nrdict = 0;
    for (int k = 0; k < 64; ++k) T.nrdict += h[k] != INT32_MIN;
    SGM_TRY(dalloc(&T.rdict, 16));
    SGM_TRY(dalloc(&T.rcode, (size_t)n + 2));
    SGM_HIP(hipMemcpyAsync(T.rdict, dict.data(), 16 * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rows_encode, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (const int32_t *)T.order, (const int32_t *)T.rq, T.rc,
                       (const int32_t *)T.rdict, T.nrdict, T.rcode);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipStreamSynchronize(st));                   // (dict is a local)
    return SGM_OK;
}
// The row-space copy of a factor whose level order is on the device (T.order, T.nstride set) and whose widest row has cm <= 64
// entries: slots per row, the dependency rows and their codes (the values: k_rows_values at every setup).  The one place the
// slot rounding lives -- the device and the host level pass lay the same factor out alike.
int rows_commit(TriFactor &T, int32_t n, int cm, const int32_t *dptr, const int32_t *dnode)
{
    hipStream_t st = g_rt.stream;
    T.rows_on = true;
    T.rc = cm <= 4 ? std::max(cm, 1) : cm <= 6 ? 6 : cm <= 8 ? 8 : cm;      // (the unrolled kernels read 6 / 8 slots)
    SGM_TRY(dalloc(&T.rq, T.nstride * (size_t)T.rc));
    SGM_TRY(dalloc(&T.rv, T.nstride * (size_t)T.rc));
    SGM_HIP(hipMemsetAsync(T.rq, 0xff, T.nstride * (size_t)T.rc * 4, st));
    SGM_HIP(hipMemsetAsync(T.rv, 0, T.nstride * (size_t)T.rc * 8, st));
    if (n) hipLaunchKernelGGL(k_rows_index, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (const int32_t *)T.order, dptr, dnode,
                              (uint32_t)T.nstride, T.rc, T.rq);
    SGM_HIP(hipGetLastError());
    return rows_encode(T, n);
}

// the inline values of the row records and their slot-major copy (dv: kInline slots)
__global__ void k_tri_slots(int32_t n, TrsvRec *recs, const double *__restrict__ pv, uint32_t nstride, double *__restrict__ dv)
{
    const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int32_t cnt = recs[p].cnt, k0 = recs[p].k0;
#pragma unroll
    for (int j = 0; j < kInline; ++j) {
        const double v = j < cnt ? pv[k0 + j] : 0.0;
        recs[p].v[j] = v;
        dv[(size_t)j * nstride + p] = v;
    }
}

// dependency levels of a strictly triangular pattern (1-based): level_ptr / order (position -> row, rows of a level in
// ascending order) / pos (row -> position)
void tri_levels(int32_t n, const std::vector<int32_t> &ptr1, const std::vector<int32_t> &node1, bool lower,
                std::vector<int32_t> &level_ptr, std::vector<int32_t> &order, std::vector<int32_t> *pos)
{
    std::vector<int32_t> level(std::max(n, 1), 0);
    int32_t nlev = 0;
    auto visit = [&](int32_t i) {
        int32_t lv = 0;
        for (int32_t k = ptr1[i] - 1; k < ptr1[i + 1] - 1; ++k) lv = std::max(lv, level[node1[k] - 1] + 1);
        level[i] = lv;
        nlev = std::max(nlev, lv + 1);
    };
    if (lower) for (int32_t i = 0; i < n; ++i) visit(i);
    else for (int32_t i = n - 1; i >= 0; --i) visit(i);
    level_ptr.assign(nlev + 1, 0);
    for (int32_t i = 0; i < n; ++i) level_ptr[level[i] + 1]++;
    for (int32_t l = 0; l < nlev; ++l) level_ptr[l + 1] += level_ptr[l];
    order.assign(std::max(n, 1), 0);
    if (pos) pos->assign(std::max(n, 1), 0);
    std::vector<int32_t> cursor(level_ptr.begin(), level_ptr.end() - 1);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t p = cursor[level[i]]++;
        order[p] = i;
        if (pos) (*pos)[i] = p;
    }
}

void free_tri(TriFactor &T)
{
    dfree(T.order); dfree(T.recs); dfree(T.pq); dfree(T.pv); dfree(T.level_ptr_dev); dfree(T.dq); dfree(T.dq32); dfree(T.dv); dfree(T.wq);
    dfree(T.rq); dfree(T.rv); dfree(T.src); dfree(T.rcode); dfree(T.rdict);
    T = TriFactor();
}

// The same index work entirely on the device, for a factor of at most kRowLevels levels (what a colour ordering leaves):
// levels by relaxation, the level order by a stable radix sort of the row numbers on their levels, per-level facts by
// one more pass.  *served = false (and T untouched) when the factor has more levels than that or rows too long for the
// row-space copy: the host pass (tri_levels_dev) then does it from the pattern's host copy.  No host copy of the pattern
// is needed here; T.h_order / T.h_pos stay empty until the level walkers want them (tri_host_order).
int tri_levels_device(TriFactor &T, int32_t n, const int32_t *dptr, const int32_t *dnode, bool *served)
{
    *served = false;
    if (T.have_levels) { *served = T.rows_on; return SGM_OK; }
    if (n < 1 || (size_t)n + kNarrow >= (size_t)500000000) return SGM_OK;
    hipStream_t st = g_rt.stream;
    int32_t *level = nullptr, *small = nullptr, *rows = nullptr, *order = nullptr, *keys = nullptr;
    void *tmp = nullptr;
    struct Tmp { int32_t *&a, *&b, *&c, *&d, *&e; void *&t; ~Tmp() { dfree(a); dfree(b); dfree(c); dfree(d); dfree(e); if (t) (void)hipFree(t); } }
        guard{level, small, rows, order, keys, tmp};
    SGM_TRY(dalloc(&level, (size_t)n));
    SGM_TRY(dalloc(&small, (size_t)2 + 5 * (kRowLevels + 2)));      // flags[2] | count | begin | cmax | notrun | first
    SGM_HIP(hipMemsetAsync(level, 0, (size_t)n * 4, st));
    int32_t *flags = small;                              // [2]
    const int grid = (n + kBlock - 1) / kBlock;
    bool done = false;
    for (int it = 0; it <= kRowLevels + 1 && !done; ++it) {
        int32_t hf[2] = {0, 0};
        SGM_HIP(hipMemsetAsync(flags, 0, 8, st));
        hipLaunchKernelGGL(k_level_relax, dim3(grid), dim3(kBlock), 0, st, n, dptr, dnode, level, (int32_t)kRowLevels, flags);
        SGM_HIP(hipMemcpyAsync(hf, flags, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
        if (hf[1]) return SGM_OK;                        // too many levels for this path
        done = !hf[0];
    }
    if (!done) return SGM_OK;
    // histogram -> level_ptr; stable sort of 0 .. n-1 on the levels -> level order (rows of a level ascending)
    int32_t *count = small + 2, *begin = count + kRowLevels + 2, *cmax = begin + kRowLevels + 2, *notrun = cmax + kRowLevels + 2,
            *first = notrun + kRowLevels + 2;
    SGM_HIP(hipMemsetAsync(count, 0, (size_t)5 * (kRowLevels + 2) * 4, st));
    SGM_TRY(dalloc(&rows, (size_t)n));
    SGM_TRY(dalloc(&order, (size_t)n));
    SGM_TRY(dalloc(&keys, (size_t)n));
    hipLaunchKernelGGL(k_level_hist, dim3(grid), dim3(kBlock), 0, st, n, (const int32_t *)level, count, rows);
    int32_t hcount[kRowLevels + 2];
    SGM_HIP(hipMemcpyAsync(hcount, count, sizeof hcount, hipMemcpyDeviceToHost, st));
    size_t tb = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const int32_t *)level, keys, (const int32_t *)rows, order, n, 0, 6, st);
    SGM_HIP(hipMalloc(&tmp, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const int32_t *)level, keys, (const int32_t *)rows, order, n, 0, 6, st));
    SGM_HIP(hipStreamSynchronize(st));
    int32_t nlev = 0;
    for (int l = 0; l < kRowLevels + 2; ++l) if (hcount[l]) nlev = l + 1;
    if (nlev < 1 || nlev > kRowLevels) return SGM_OK;
    std::vector<int32_t> lp((size_t)nlev + 1, 0);
    for (int l = 0; l < nlev; ++l) lp[l + 1] = lp[l] + hcount[l];
    SGM_HIP(hipMemcpyAsync(begin, lp.data(), (size_t)(nlev + 1) * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_level_info, dim3(grid), dim3(kBlock), 0, st, n, (const int32_t *)order, (const int32_t *)level, dptr,
                       (const int32_t *)begin, cmax, notrun, first);
    int32_t hinfo[3 * (kRowLevels + 2)];
    SGM_HIP(hipMemcpyAsync(hinfo, cmax, sizeof hinfo, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    const int32_t *hc = hinfo, *hn = hinfo + kRowLevels + 2, *hfst = hinfo + 2 * (kRowLevels + 2);
    int cm = 0;
    for (int l = 0; l < nlev; ++l) cm = std::max(cm, hc[l]);
    if (cm > 64) return SGM_OK;
    // commit
    free_tri(T);
    T.level_ptr = lp;
    T.nstride = (size_t)n + kNarrow;
    T.order = order; order = nullptr;                    // (the sorted row numbers ARE the level order)
    SGM_TRY(dalloc(&T.level_ptr_dev, T.level_ptr.size()));
    SGM_HIP(hipMemcpy(T.level_ptr_dev, T.level_ptr.data(), T.level_ptr.size() * 4, hipMemcpyHostToDevice));
    for (int l = 0; l < nlev; ++l) T.row_levels.push_back({lp[l], lp[l + 1], hc[l], hn[l] ? -1 : hfst[l]});
    SGM_TRY(rows_commit(T, n, cm, dptr, dnode));
    T.have_levels = true;
    *served = true;
    return SGM_OK;
}
// host copies of the level order for what still reads them (the level walkers' index work)
int tri_host_order(TriFactor &T, int32_t n)
{
    if (!T.h_order.empty() || n < 1) return SGM_OK;
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    T.h_order.resize((size_t)n);
    T.h_pos.resize((size_t)n);
    SGM_TRY(copy_big(T.h_order.data(), T.order, (size_t)n * 4, hipMemcpyDeviceToHost));
    for (int32_t p2 = 0; p2 < n; ++p2) T.h_pos[T.h_order[p2]] = p2;
    return SGM_OK;
}

// Dependency levels of a strictly triangular factor and, for one of at most kRowLevels levels, its row-space copy.
// lower: rows depend on smaller rows (forward sweep 1..n); upper: on larger rows (backward sweep n..1).  ptr1 / node1:
// the pattern on the host (1-based); dptr / dnode / dval: the factor on the device (0-based, values in pattern order;
// dval null: index work only).
// (ptr1 / node1 may be EMPTY when the device pass is known to have served this factor: tri_levels_device below)
int tri_levels_dev(TriFactor &T, int32_t n, const std::vector<int32_t> &ptr1, const std::vector<int32_t> &node1,
                   const int32_t *dptr, const int32_t *dnode, const double *dval, bool lower)
{
    hipStream_t st = g_rt.stream;
    if (!T.have_levels) {
        free_tri(T);
        tri_levels(n, ptr1, node1, lower, T.level_ptr, T.h_order, &T.h_pos);
        const int32_t nlev = (int32_t)T.level_ptr.size() - 1;
        T.nstride = (size_t)n + kNarrow;          // (padded by kNarrow rows: lanes of the walkers past a level's end read valid memory)
        SGM_TRY(dalloc(&T.order, (size_t)std::max(n, 1)));
        SGM_TRY(dalloc(&T.level_ptr_dev, T.level_ptr.size()));
        if (n) SGM_TRY(copy_big(T.order, T.h_order.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        SGM_HIP(hipMemcpy(T.level_ptr_dev, T.level_ptr.data(), T.level_ptr.size() * 4, hipMemcpyHostToDevice));
        // a few levels (whatever their widths): the row-space copy (dependency rows, slot-major over the level order)
        T.rows_on = false;
        T.rc = 0;
        T.row_levels.clear();
        if (nlev >= 1 && nlev <= kRowLevels && (size_t)n + kNarrow < (size_t)500000000) {
            int cm = 0;
            for (int32_t l = 0; l < nlev; ++l) {
                const int32_t b = T.level_ptr[l], e = T.level_ptr[l + 1];
                int c = 0;
                bool run = true;
                for (int32_t p2 = b; p2 < e; ++p2) {
                    const int32_t i = T.h_order[p2];
                    c = std::max(c, ptr1[i + 1] - ptr1[i]);
                    if (p2 > b) run = run && i == T.h_order[p2 - 1] + 1;
                }
                T.row_levels.push_back({b, e, c, run ? T.h_order[b] : -1});
                cm = std::max(cm, c);
            }
            if (cm <= 64) SGM_TRY(rows_commit(T, n, cm, dptr, dnode));
        }
        T.have_levels = true;
    }
    if (T.rows_on && n && dval)
        hipLaunchKernelGGL(k_rows_values, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (const int32_t *)T.order, dptr, dval,
                           (uint32_t)T.nstride, T.rc, T.rv);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// The level walkers' structures of a factor (tri_levels_dev has run): records in level order, schedule, ring copies --
// index work when the pattern is new, values (from the device factor) every time.
int tri_walkers(TriFactor &T, int32_t n, const std::vector<int32_t> &ptr1, const std::vector<int32_t> &node1, const double *val)
{
    const size_t nnz = node1.size();
    if (!T.have_walkers) {
        SGM_TRY(tri_host_order(T, n));
        dfree(T.recs); dfree(T.pq); dfree(T.pv); dfree(T.dq); dfree(T.dq32); dfree(T.dv); dfree(T.wq); dfree(T.src);
        T.recs = nullptr; T.pq = nullptr; T.pv = nullptr; T.dq = nullptr; T.dq32 = nullptr; T.dv = nullptr; T.wq = nullptr; T.src = nullptr;
        T.schedule.clear();
        std::vector<int32_t> h_src(std::max<size_t>(nnz, 1), 0);      // level-order entry -> factor entry
        const int32_t nlev = (int32_t)T.level_ptr.size() - 1;
        // rows in level order: dependency POSITIONS in stored order
        T.h_recs.assign(std::max(n, 1), TrsvRec());
        T.h_pq.assign(std::max<size_t>(nnz, 1), 0);
        int32_t kk = 0;
        for (int32_t p = 0; p < n; ++p) {
            const int32_t i = T.h_order[p];
            TrsvRec &r = T.h_recs[p];
            r.cnt = ptr1[i + 1] - ptr1[i];
            r.k0 = kk;
            for (int32_t k = ptr1[i] - 1; k < ptr1[i + 1] - 1; ++k, ++kk) {
                T.h_pq[kk] = T.h_pos[node1[k] - 1];
                h_src[kk] = k;
                if (kk - r.k0 < kInline) r.q[kk - r.k0] = T.h_pq[kk];
            }
        }
        // schedule: wide levels alone, runs of narrow levels together
        constexpr int narrow = kNarrow;
        std::vector<int8_t> lev_cls(nlev, 0);
        {
            std::vector<int8_t> raw(nlev, 0);
            for (int32_t l = 0; l < nlev; ++l) {
                const int32_t w = T.level_ptr[l + 1] - T.level_ptr[l];
                raw[l] = w <= 64 ? -1 : w <= 256 ? 0 : w <= 512 ? 1 : w <= kTrsvBlock ? 2 : w <= 2 * kTrsvBlock ? 3 : w <= narrow ? 4 : 5;      // (-1: one wave)
            }
            for (int32_t l = 0; l < nlev; ++l) {          // window maximum over narrow neighbours
                int8_t m = raw[l];
                if (m < 5) {
                    for (int32_t k = l - 1; k >= std::max(0, l - 8) && raw[k] < 5; --k) m = std::max(m, raw[k]);
                    for (int32_t k = l + 1; k <= std::min(nlev - 1, l + 8) && raw[k] < 5; ++k) m = std::max(m, raw[k]);
                }
                lev_cls[l] = m;
            }
        }
        for (int32_t l = 0; l < nlev;) {
            const int32_t sz = T.level_ptr[l + 1] - T.level_ptr[l];
            if (sz > narrow) {
                int cm = 0;
                for (int32_t p = T.level_ptr[l]; p < T.level_ptr[l + 1]; ++p) cm = std::max(cm, T.h_recs[p].cnt);
                T.schedule.push_back({l, l + 1, false, 0, false, cm});      // c: most dependencies of a row of the level
                ++l;
                continue;
            }
            // runs are cut by width class: 256 / 512 / 1024 threads with one row per lane, then 2 and
            // 4 rows per lane (classes 0..4, smoothed so that a run is at least ~16 levels long)
            const int c = lev_cls[l];
            int32_t e = l;
            while (e < nlev && T.level_ptr[e + 1] - T.level_ptr[e] <= narrow && lev_cls[e] == c) ++e;
            // all dependencies inline and within the ring's reach?  (see k_trsv_walk_ring)
            bool ring_ok = true;
            int cmax = 0;
            for (int32_t lev = l; lev < e && ring_ok; ++lev)
                for (int32_t p = T.level_ptr[lev]; p < T.level_ptr[lev + 1] && ring_ok; ++p) {
                    const TrsvRec &r = T.h_recs[p];
                    ring_ok = r.cnt <= kInline;
                    cmax = std::max(cmax, r.cnt);
                    for (int32_t k = r.k0; k < r.k0 + r.cnt && ring_ok; ++k)
                        ring_ok = T.h_pq[k] >= T.level_ptr[lev + 1] - kRing && T.h_pq[k] < p;
                }
            T.schedule.push_back({l, e, true, c, ring_ok, cmax});
            l = e;
        }
        // ring-walker copy of the structure: 16-bit ring slots (only read in ring runs), padded
        // by kNarrow rows so that lanes past a level's end read valid memory
        T.h_dq.assign(T.nstride, 0);
        for (int32_t p = 0; p < n; ++p) {
            const TrsvRec &r = T.h_recs[p];
            uint64_t w = 0;
            for (int j = 0; j < kInline; ++j)
                w |= (uint64_t)(j < r.cnt ? (r.q[j] & (kRing - 1)) : kRing) << (16 * j);
            T.h_dq[p] = w;
        }
        SGM_TRY(dalloc(&T.dq, T.nstride));
        SGM_TRY(dalloc(&T.dv, T.nstride * kInline));
        SGM_HIP(hipMemcpy(T.dq, T.h_dq.data(), T.h_dq.size() * 8, hipMemcpyHostToDevice));
        {
            std::vector<uint32_t> lo(T.nstride);
            for (size_t p = 0; p < T.nstride; ++p) lo[p] = (uint32_t)T.h_dq[p];
            SGM_TRY(dalloc(&T.dq32, T.nstride));
            SGM_HIP(hipMemcpy(T.dq32, lo.data(), lo.size() * 4, hipMemcpyHostToDevice));
        }
        {
            std::vector<int32_t> wq(T.nstride * kInline, -1);
            for (int32_t p = 0; p < n; ++p)
                for (int j = 0; j < kInline && j < T.h_recs[p].cnt; ++j) wq[(size_t)j * T.nstride + p] = T.h_recs[p].q[j];
            SGM_TRY(dalloc(&T.wq, wq.size()));
            SGM_HIP(hipMemcpy(T.wq, wq.data(), wq.size() * 4, hipMemcpyHostToDevice));
        }
        SGM_TRY(dalloc(&T.recs, (size_t)std::max(n, 1)));
        SGM_TRY(dalloc(&T.pq, nnz));
        SGM_TRY(dalloc(&T.pv, nnz));
        SGM_TRY(dalloc(&T.src, nnz));
        if (nnz) SGM_TRY(copy_big(T.pq, T.h_pq.data(), nnz * 4, hipMemcpyHostToDevice));
        if (nnz) SGM_TRY(copy_big(T.src, h_src.data(), nnz * 4, hipMemcpyHostToDevice));
        if (n) SGM_TRY(copy_big(T.recs, T.h_recs.data(), (size_t)n * sizeof(TrsvRec), hipMemcpyHostToDevice));     // (values: k_tri_slots)
        SGM_HIP(hipMemsetAsync(T.dv, 0, T.nstride * kInline * 8, g_rt.stream));          // (the padding slots stay zero)
        T.have_walkers = true;
    }
    // values (every setup), on the device: level-order copy, the inline part of the records, the slot-major copy
    hipStream_t st = g_rt.stream;
    if (nnz) hipLaunchKernelGGL(k_tri_entries, dim3(vec_grid((int64_t)nnz)), dim3(kBlock), 0, st, (int64_t)nnz, (const int32_t *)T.src, val, T.pv);
    if (n) hipLaunchKernelGGL(k_tri_slots, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, T.recs, (const double *)T.pv,
                              (uint32_t)T.nstride, T.dv);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// ---- strip path: host side ---------------------------------------------------------------------
void free_grid(GridTri &G)
{
    dfree(G.rec); dfree(G.row); dfree(G.edge); dfree(G.progress); dfree(G.srcS); dfree(G.srcW); dfree(G.code); dfree(G.pos);
    G = GridTri();
}

// Is the factor grid-like?  lower: deps of row r within {r-1, r-w}, the r-1 one never across a grid
// line (r % w != 0); upper: {r+1, r+w}, (r+1) % w != 0.  Returns w (0 = no).
int32_t grid_width(int32_t n, const std::vector<int32_t> &ptr1, const std::vector<int32_t> &node1, bool lower)
{
    int32_t w = 0;
    for (int32_t r = 0; r < n; ++r)
        for (int32_t k = ptr1[r] - 1; k < ptr1[r + 1] - 1; ++k) {
            const int32_t dlt = lower ? r - (node1[k] - 1) : (node1[k] - 1) - r;
            if (dlt <= 0) return 0;
            if (dlt == 1) continue;
            if (!w) w = dlt;
            if (dlt != w) return 0;
        }
    if (w < 2) return 0;
    for (int32_t r = 0; r < n; ++r) {
        if (ptr1[r + 1] - ptr1[r] > 2) return 0;
        for (int32_t k = ptr1[r] - 1; k < ptr1[r + 1] - 1; ++k) {
            const int32_t c = node1[k] - 1;
            if (lower && c == r - 1 && r % w == 0) return 0;
            if (!lower && c == r + 1 && (r + 1) % w == 0) return 0;
        }
        if (ptr1[r + 1] - ptr1[r] == 2 && node1[ptr1[r] - 1] == node1[ptr1[r]]) return 0;
    }
    return w;
}

// index work of the skewed layout (once per pattern), on the device from the factor's pattern there (0-based)
int build_grid(GridTri &G, int32_t n, int32_t w, const int32_t *dptr, const int32_t *dnode, bool lower)
{
    free_grid(G);
    G.w = w;
    G.nj = (n + w - 1) / w;
    G.NI = (w + 63) / 64;
    G.S = (G.nj + 63 + 31) / 32 * 32;                         // a multiple of every look-ahead depth
    G.NP = (int64_t)G.NI * G.S * 64;
    if (G.NP >= INT32_MAX) return SGM_OK;                     // (positions are int32)
    hipStream_t st = g_rt.stream;
    int32_t *flags = nullptr;
    SGM_TRY(dalloc(&G.rec, (size_t)G.NP));
    SGM_TRY(dalloc(&G.row, (size_t)G.NP));
    SGM_TRY(dalloc(&G.edge, (size_t)G.NI * (G.S + kEdgePad)));
    SGM_TRY(dalloc(&G.progress, (size_t)G.NI + 1));
    SGM_TRY(dalloc(&G.srcS, (size_t)G.NP));
    SGM_TRY(dalloc(&G.srcW, (size_t)G.NP));
    SGM_TRY(dalloc(&G.code, (size_t)G.NP));
    SGM_TRY(dalloc(&G.pos, (size_t)std::max(n, 1)));
    SGM_TRY(dalloc(&flags, 2));
    SGM_HIP(hipMemsetAsync(G.row, 0xff, (size_t)G.NP * 4, st));       // -1 = padding / no such term
    SGM_HIP(hipMemsetAsync(G.srcS, 0xff, (size_t)G.NP * 4, st));
    SGM_HIP(hipMemsetAsync(G.srcW, 0xff, (size_t)G.NP * 4, st));
    SGM_HIP(hipMemsetAsync(G.code, 0, (size_t)G.NP, st));
    SGM_HIP(hipMemsetAsync(flags, 0, 8, st));
    SGM_HIP(hipMemsetAsync(G.edge, 0, (size_t)G.NI * (G.S + kEdgePad) * 8, st));
    if (n) hipLaunchKernelGGL(k_grid_build, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, w, G.nj, G.S, lower ? 1 : 0, dptr, dnode,
                              G.row, G.srcS, G.srcW, G.code, G.pos, flags);
    int32_t hf[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(hf, flags, 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    dfree(flags);
    SGM_HIP(e);
    G.order = hf[0] && hf[1] ? 2 : hf[1] ? 1 : 0;
    G.on = true;
    return SGM_OK;
}

// records in the skewed layout (every setup), from the factor's values on the device
int refresh_grid_values(GridTri &G, const double *val)
{
    if (!G.on) return SGM_OK;
    hipLaunchKernelGGL(k_grid_records, dim3(vec_grid(G.NP)), dim3(kBlock), 0, g_rt.stream, G.NP, (const int32_t *)G.srcS,
                       (const int32_t *)G.srcW, (const uint8_t *)G.code, G.order, val, G.rec);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// grid_width without a host copy of the pattern: 0 = not grid-like
int grid_width_device(int32_t n, const int32_t *dptr, const int32_t *dnode, bool lower, int32_t *w_out)
{
    *w_out = 0;
    if (n < 1) return SGM_OK;
    hipStream_t st = g_rt.stream;
    int32_t *info = nullptr;
    SGM_TRY(dalloc(&info, 4));
    struct Tmp { int32_t *&a; ~Tmp() { dfree(a); } } guard{info};
    const int32_t init[4] = {INT32_MAX, 0, 0, 0};
    int32_t h[4];
    SGM_HIP(hipMemcpyAsync(info, init, 16, hipMemcpyHostToDevice, st));
    const int grid = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_grid_detect1, dim3(grid), dim3(kBlock), 0, st, n, lower ? 1 : 0, dptr, dnode, info);
    SGM_HIP(hipMemcpyAsync(h, info, 16, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (h[2] || h[0] == INT32_MAX || h[0] != h[1] || h[0] < 2) return SGM_OK;
    hipLaunchKernelGGL(k_grid_detect2, dim3(grid), dim3(kBlock), 0, st, n, lower ? 1 : 0, h[0], dptr, dnode, info);
    SGM_HIP(hipMemcpyAsync(h, info, 16, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (!h[3]) *w_out = h[0];
    return SGM_OK;
}
// the factorisation order of a grid-like factor pair: rows sorted (stably) on their anti-diagonal
int grid_factor_order(IlduState *S, int32_t n, int32_t w, int32_t h)
{
    hipStream_t st = g_rt.stream;
    const int32_t nj = (n + w - 1) / w;
    const int32_t nkeys = h > 0 ? w + h + (int32_t)((n + (int64_t)w * h - 1) / ((int64_t)w * h)) : w + nj;   // keys 0 .. w-1 + nj-1
    int bits = 1;
    while ((1 << bits) < nkeys) ++bits;
    int32_t *key = nullptr, *key2 = nullptr, *rows = nullptr, *count = nullptr;
    void *tmp = nullptr;
    struct Tmp { int32_t *&a, *&b, *&c, *&d; void *&t; ~Tmp() { dfree(a); dfree(b); dfree(c); dfree(d); if (t) (void)hipFree(t); } }
        guard{key, key2, rows, count, tmp};
    SGM_TRY(dalloc(&key, (size_t)n));
    SGM_TRY(dalloc(&key2, (size_t)n));
    SGM_TRY(dalloc(&rows, (size_t)n));
    SGM_TRY(dalloc(&count, (size_t)nkeys));
    dfree(S->forder);
    S->forder = nullptr;
    SGM_TRY(dalloc(&S->forder, (size_t)n));
    SGM_HIP(hipMemsetAsync(count, 0, (size_t)nkeys * 4, st));
    hipLaunchKernelGGL(k_grid_keys, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, w, h, key, rows, count);
    size_t tb = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const int32_t *)key, key2, (const int32_t *)rows, S->forder, n, 0, bits, st);
    SGM_HIP(hipMalloc(&tmp, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, (const int32_t *)key, key2, (const int32_t *)rows, S->forder, n, 0, bits, st));
    std::vector<int32_t> hc((size_t)nkeys);
    SGM_HIP(hipMemcpyAsync(hc.data(), count, (size_t)nkeys * 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    S->flevel_ptr.assign(1, 0);
    for (int32_t k = 0; k < nkeys; ++k)
        if (hc[k]) S->flevel_ptr.push_back(S->flevel_ptr.back() + hc[k]);
    return SGM_OK;
}

// The factors' patterns on the device (0-based) from the part's CSR-order arrays ...
// The real entries of an ELLPACK part -- the first degrees(i) slots of every row, in slot order: what the reference's cursor
// hands out (ellpack_graphs.f90:310-369) -- as 0-based CSR arrays.  Padding slots (the last neighbour repeated, value 0) and
// empty rows' node = 0 never appear.  ELL = false: the rows are fixed-length CSR rows (an ELLPACK matrix over ranks,
// sgm_ell_create_dist, whose padding slots are stored entries for the product's sake) and the same first degrees(i) are taken.
template <bool ELL>
__global__ void k_real_entries(int32_t n, const int32_t *__restrict__ src_ptr, const int32_t *__restrict__ scol, const double *__restrict__ sval,
                               const int32_t *__restrict__ rowptr, int32_t *__restrict__ col, double *__restrict__ val)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t b = rowptr[i], d = rowptr[i + 1] - b;
    const int64_t s0 = ELL ? i : src_ptr[i];
    for (int32_t k = 0; k < d; ++k) {
        const int64_t s = ELL ? (int64_t)k * n + s0 : s0 + k;
        col[b + k] = scol[s];
        val[b + k] = sval[s];
    }
}
int real_entries_as_csr(const Part &p, bool ell, Part &v)
{
    hipStream_t st = g_rt.stream;
    const int32_t n = p.n;
    if (ell) SGM_TRY(ell_need_degrees("ILDU(0) setup", p));
    else if (!p.edeg && n) return fail(SGM_ERR_UNSUPPORTED, "ILDU(0) on ELLPACK rows over ranks needs their degrees (this handle has none: sgm_ell_create_dist takes them)");
    v.n = n;
    v.ncol_own = p.ncol_own;
    v.n_halo = p.n_halo;
    v.lean = false;
    SGM_TRY(dalloc(&v.rowptr, (size_t)n + 1));
    SGM_HIP(hipMemsetAsync(v.rowptr, 0, ((size_t)n + 1) * 4, st));
    if (n && p.edeg) SGM_HIP(hipMemcpyAsync(v.rowptr, p.edeg, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
    size_t tb = 0;
    void *tmp = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, v.rowptr, v.rowptr, n + 1, st);
    SGM_HIP(hipMalloc(&tmp, std::max<size_t>(tb, 16)));
    struct Tmp { void *t; ~Tmp() { (void)hipFree(t); } } guard{tmp};
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, v.rowptr, v.rowptr, n + 1, st));
    int32_t total = 0;
    SGM_HIP(hipMemcpyAsync(&total, v.rowptr + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    v.nnz = total;
    SGM_TRY(dalloc(&v.col, (size_t)total + 4));
    SGM_TRY(dalloc(&v.val, (size_t)total + 2));
    SGM_HIP(hipMemsetAsync(v.col + total, 0, 4 * sizeof(int32_t), st));
    SGM_HIP(hipMemsetAsync(v.val + total, 0, 2 * sizeof(double), st));
    const dim3 grid((n + kBlock - 1) / kBlock);
    if (n && ell)
        hipLaunchKernelGGL(k_real_entries<true>, grid, dim3(kBlock), 0, st, n, (const int32_t *)nullptr, (const int32_t *)p.ecol,
                           (const double *)p.eval, (const int32_t *)v.rowptr, v.col, v.val);
    else if (n)
        hipLaunchKernelGGL(k_real_entries<false>, grid, dim3(kBlock), 0, st, n, (const int32_t *)p.rowptr, (const int32_t *)p.col,
                           (const double *)p.val, (const int32_t *)v.rowptr, v.col, v.val);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

int ildu_pattern(IlduState *S, const Part &P, int32_t own)
{
    const int32_t n = P.n;
    hipStream_t st = g_rt.stream;
    int32_t *longest = nullptr;
    SGM_TRY(dalloc(&S->dLptr, (size_t)n + 1));
    SGM_TRY(dalloc(&S->dUptr, (size_t)n + 1));
    SGM_TRY(dalloc(&longest, 2));
    struct Tmp { int32_t *&a; void *t = nullptr; ~Tmp() { dfree(a); if (t) (void)hipFree(t); } } guard{longest};
    SGM_HIP(hipMemsetAsync(longest, 0, 8, st));
    const int grid = (n + 1 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_ildu_count, dim3(grid), dim3(kBlock), 0, st, n, own, (const int32_t *)P.rowptr, (const int32_t *)P.col,
                       S->dLptr, S->dUptr, longest);
    size_t tb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, S->dLptr, S->dLptr, n + 1, st);
    SGM_HIP(hipMalloc(&guard.t, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(guard.t, tb, S->dLptr, S->dLptr, n + 1, st));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(guard.t, tb, S->dUptr, S->dUptr, n + 1, st));
    int32_t tot[2] = {0, 0}, lg[2] = {0, 0};
    SGM_HIP(hipMemcpyAsync(&tot[0], S->dLptr + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipMemcpyAsync(&tot[1], S->dUptr + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipMemcpyAsync(lg, longest, 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    S->nnzL = tot[0]; S->nnzU = tot[1];
    S->maxL = lg[0]; S->maxU = lg[1];
    SGM_TRY(dalloc(&S->dLnode, (size_t)std::max(tot[0], 1)));
    SGM_TRY(dalloc(&S->dUnode, (size_t)std::max(tot[1], 1)));
    if (n) hipLaunchKernelGGL(k_ildu_split, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, own, (const int32_t *)P.rowptr,
                              (const int32_t *)P.col, (const int32_t *)S->dLptr, S->dLnode, (const int32_t *)S->dUptr, S->dUnode);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

}  // namespace

// ------------------------------------------------------------------------------ what sgm_pc.hip and the applies call
namespace sgm {

void free_ildu(IlduState &S)
{
    free_tri(S.L);
    free_tri(S.U);
    dfree(S.D); dfree(S.xpL); dfree(S.xpU); dfree(S.Dp); dfree(S.mapLU);
    dfree(S.dLptr); dfree(S.dLnode); dfree(S.dUptr); dfree(S.dUnode); dfree(S.dLval); dfree(S.dUval); dfree(S.forder);
    free_grid(S.gL); free_grid(S.gU);
    dfree(S.gxL); dfree(S.gxU); dfree(S.gDp); dfree(S.gmapLU);
    slab3_free(S.slab);
    const PcOptions keep = S.opt;          // (the owning preconditioner's options outlive a rebuild of its factors)
    S = IlduState();
    S.opt = keep;
}

// the factors' patterns as 1-based host copies, when something asks: sgm_pc_get, the host's level pass (factors of many levels), the
// grid / slab detection, the level walkers' index work
int ensure_host_pattern(IlduState *S)
{
    if (!S->hLptr.empty() || !S->dLptr) return SGM_OK;
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    auto down = [](std::vector<int32_t> &h, const int32_t *d, size_t cnt) -> int {
        h.resize(cnt);
        if (cnt) SGM_TRY(copy_big(h.data(), d, cnt * 4, hipMemcpyDeviceToHost));
        for (auto &v : h) v += 1;
        return SGM_OK;
    };
    SGM_TRY(down(S->hLptr, S->dLptr, (size_t)S->n + 1));
    SGM_TRY(down(S->hUptr, S->dUptr, (size_t)S->n + 1));
    SGM_TRY(down(S->hLnode, S->dLnode, (size_t)S->nnzL));
    SGM_TRY(down(S->hUnode, S->dUnode, (size_t)S->nnzU));
    return SGM_OK;
}

// Dependency levels of both factors, their row-space copies when they have few levels (index work when the pattern is
// new, values always) and the work vector of the row-space sweeps.  At setup when no pipelined path serves the pattern,
// otherwise on first need.
int ensure_levels(IlduState *S)
{
    if (S->levels_ready) return SGM_OK;
    const int32_t n = S->n;
    const bool fresh = !S->levels_pattern;
    // factors of a few levels: all index work on the device; otherwise from the pattern's host copy
    bool ls = false, us = false;
    SGM_TRY(tri_levels_device(S->L, n, S->dLptr, S->dLnode, &ls));
    SGM_TRY(tri_levels_device(S->U, n, S->dUptr, S->dUnode, &us));
    if (!S->L.have_levels || !S->U.have_levels) SGM_TRY(ensure_host_pattern(S));
    SGM_TRY(tri_levels_dev(S->L, n, S->hLptr, S->hLnode, S->dLptr, S->dLnode, S->dLval, true));
    SGM_TRY(tri_levels_dev(S->U, n, S->hUptr, S->hUnode, S->dUptr, S->dUnode, S->dUval, false));
    if (fresh) {
        dfree(S->xpL);
        S->xpL = nullptr;
        SGM_TRY(dalloc(&S->xpL, (size_t)n + kNarrow));     // + scratch slots of the level walker
    }
    S->rows_n0 = 0;
    S->rows_fin = false;
    if (S->L.rows_on && S->U.rows_on && !S->L.row_levels.empty() && !S->U.row_levels.empty()) {
        const auto &l0 = S->L.row_levels.front(), &ll = S->L.row_levels.back(), &u0 = S->U.row_levels.front();
        if (l0.c == 0 && l0.row0 == 0) S->rows_n0 = l0.e - l0.b;
        S->rows_fin = S->L.row_levels.size() >= 2 && u0.c == 0 && u0.row0 >= 0 && u0.row0 == ll.row0 && u0.e - u0.b == ll.e - ll.b;
    }
    S->levels_pattern = true;
    S->levels_ready = true;
    return SGM_OK;
}

// The level walkers' structures (records, schedules, ring copies, the L -> U hand-over in position space): built when
// neither a pipelined path nor the row-space sweeps serve the pattern, otherwise on first need (an option switched
// off, a retired pipeline).
int ensure_walkers(IlduState *S)
{
    SGM_TRY(ensure_levels(S));
    if (S->walk_ready) return SGM_OK;
    SGM_TRY(ensure_host_pattern(S));
    const int32_t n = S->n;
    const bool fresh = !S->walk_pattern;
    SGM_TRY(tri_walkers(S->L, n, S->hLptr, S->hLnode, S->dLval));
    SGM_TRY(tri_walkers(S->U, n, S->hUptr, S->hUnode, S->dUval));
    if (fresh) {
        dfree(S->xpU); dfree(S->Dp); dfree(S->mapLU);
        S->xpU = S->Dp = nullptr; S->mapLU = nullptr;
        SGM_TRY(dalloc(&S->xpU, (size_t)n + kNarrow));
        SGM_TRY(dalloc(&S->Dp, (size_t)std::max(n, 1)));
        SGM_TRY(dalloc(&S->mapLU, (size_t)std::max(n, 1)));
        std::vector<int32_t> map((size_t)std::max(n, 1));
        for (int32_t p = 0; p < n; ++p) map[p] = S->L.h_pos[S->U.h_order[p]];
        if (n) SGM_TRY(copy_big(S->mapLU, map.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    }
    if (n) hipLaunchKernelGGL(k_pos_diag, dim3(vec_grid(n)), dim3(kBlock), 0, g_rt.stream, (int64_t)n, (const int32_t *)S->U.order,
                              (const double *)S->D, S->Dp);                  // D in U's level order
    S->walk_pattern = true;
    S->walk_ready = true;
    return SGM_OK;
}

// the factor values on the host (sgm_pc_get only)
int ensure_host_values(IlduState *S)
{
    if (S->host_vals) return SGM_OK;
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    S->hLval.resize((size_t)S->nnzL);
    S->hUval.resize((size_t)S->nnzU);
    S->hD.resize((size_t)S->n);
    if (!S->hLval.empty()) SGM_TRY(copy_big(S->hLval.data(), S->dLval, S->hLval.size() * 8, hipMemcpyDeviceToHost));
    if (!S->hUval.empty()) SGM_TRY(copy_big(S->hUval.data(), S->dUval, S->hUval.size() * 8, hipMemcpyDeviceToHost));
    if (S->n) SGM_TRY(copy_big(S->hD.data(), S->D, (size_t)S->n * 8, hipMemcpyDeviceToHost));
    S->host_vals = true;
    return SGM_OK;
}

}  // namespace sgm

namespace {

// ------------------------------------------------------------------------------ the steps of a block's setup
// SGM_PC_TIMING: the time since the last lap on stderr (a tuning aid; a lap synchronises the stream, so only when it is on)
struct LapTimer {
    bool on;
    std::chrono::steady_clock::time_point prev = std::chrono::steady_clock::now();
    void operator()(const char *what)
    {
        if (!on) return;
        (void)hipStreamSynchronize(g_rt.stream);
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "[sigma_hip] ildu setup: %-28s %8.1f ms\n", what, std::chrono::duration<double, std::milli>(t - prev).count());
        prev = t;
    }
};

// An ELLPACK operand: sparse_ldu_setup takes any sparse_matrix_interface (ldu_solvers.f90:95-130); the pattern pass reads A
// through its get_edges cursor (:397-440) and the fill through get_entries (:306-321), and the ELLPACK cursor yields row
// after row the first degrees(i) slots of node(:, i) / val(:, i) (ellpack_graphs.f90:310-369) -- never the padding.  That
// edge stream is a CSR matrix's: the rows' real entries in slot order are laid out as one for the length of the setup, and
// everything else runs on it statement for statement.
int ell_view(const Part &src, int32_t fmt, Part &view)
{
    if (fmt == SGM_FMT_CSR) SGM_TRY(csr_need_arrays(src));
    const int rc = real_entries_as_csr(src, fmt == SGM_FMT_ELL, view);
    if (fmt == SGM_FMT_CSR) csr_release_arrays(src);
    return rc;
}

// The order the rows are factorised in (and, for L's levels, what its sweeps use later): L's dependency levels found on the
// device when they are few (*few); else the anti-diagonals of a grid-like pair; else L's levels from the pattern's host copy
int factor_order(IlduState *S, bool *few, LapTimer &lap)
{
    const int32_t n = S->n;
    SGM_TRY(tri_levels_device(S->L, n, S->dLptr, S->dLnode, few));
    if (!S->L.have_levels && S->opt.ildu_strips) {
        // many levels: a grid-like pair (what the strip pipeline serves)?  Then the anti-diagonals are the order
        SGM_TRY(grid_width_device(n, S->dLptr, S->dLnode, true, &S->dev_wl));
        if (S->dev_wl >= 64) SGM_TRY(grid_width_device(n, S->dUptr, S->dUnode, false, &S->dev_wu));
        if (S->dev_wl >= 64 && S->dev_wl == S->dev_wu && (n + S->dev_wl - 1) / S->dev_wl >= 64)
            SGM_TRY(grid_factor_order(S, n, S->dev_wl, 0));
        else {
            S->dev_wl = S->dev_wu = 0;
            // ... or a 3-D grid's (what the slab pipeline serves: the same bounds as slab3_build)?
            int32_t wl3, hl3, wu3 = 0, hu3 = 0;
            SGM_TRY(slab_dims_device(n, S->dLptr, S->dLnode, true, &wl3, &hl3));
            if (wl3) SGM_TRY(slab_dims_device(n, S->dUptr, S->dUnode, false, &wu3, &hu3));
            const int64_t wh3 = (int64_t)wl3 * hl3;
            if (wl3 && wl3 == wu3 && hl3 == hu3 && wl3 >= 32 && wl3 <= 256 && hl3 >= 8 && (n + wh3 - 1) / wh3 >= 8) {
                SGM_TRY(grid_factor_order(S, n, wl3, hl3));
                S->dev_slab = true;
            }
        }
        lap("grid detection, anti-diagonal order");
    }
    if (!S->L.have_levels && !S->forder) {
        SGM_TRY(ensure_host_pattern(S));
        lap("host copy of the pattern");
        SGM_TRY(tri_levels_dev(S->L, n, S->hLptr, S->hLnode, S->dLptr, S->dLnode, nullptr, true));
    }
    return SGM_OK;
}

// A factor that is (nearly) a chain -- thousands of levels of a few rows each: bands with their first off-diagonal,
// 1-D problems -- would be one launch per row (n = 4e5: 1.9 s of launches; tools/probes/chain_setup.py).  Its rows are
// factored on the HOST instead, one after the other in natural order (row i reads rows k < i only: the reference's own
// loop order), by the very statements of k_ildu_factor_level, and the values go back: two copies and ~0.1 us per row.
int factor_chain_on_host(IlduState *S)
{
    const int32_t n = S->n;
    hipStream_t st = g_rt.stream;
    std::vector<int32_t> hLp((size_t)n + 1), hUp((size_t)n + 1), hLn((size_t)std::max(S->nnzL, 1)), hUn((size_t)std::max(S->nnzU, 1));
    std::vector<double> hLv((size_t)std::max(S->nnzL, 1)), hUv((size_t)std::max(S->nnzU, 1)), hD((size_t)n);
    SGM_HIP(hipMemcpyAsync(hLp.data(), S->dLptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipMemcpyAsync(hUp.data(), S->dUptr, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, st));
    if (S->nnzL) SGM_HIP(hipMemcpyAsync(hLn.data(), S->dLnode, (size_t)S->nnzL * 4, hipMemcpyDeviceToHost, st));
    if (S->nnzU) SGM_HIP(hipMemcpyAsync(hUn.data(), S->dUnode, (size_t)S->nnzU * 4, hipMemcpyDeviceToHost, st));
    if (S->nnzL) SGM_HIP(hipMemcpyAsync(hLv.data(), S->dLval, (size_t)S->nnzL * 8, hipMemcpyDeviceToHost, st));
    if (S->nnzU) SGM_HIP(hipMemcpyAsync(hUv.data(), S->dUval, (size_t)S->nnzU * 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipMemcpyAsync(hD.data(), S->D, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    for (int32_t i = 0; i < n; ++i) ildu_factor_row(i, hLp.data(), hLn.data(), hLv.data(), hUp.data(), hUn.data(), hUv.data(), hD.data());
    if (S->nnzL) SGM_HIP(hipMemcpyAsync(S->dLval, hLv.data(), (size_t)S->nnzL * 8, hipMemcpyHostToDevice, st));
    if (S->nnzU) SGM_HIP(hipMemcpyAsync(S->dUval, hUv.data(), (size_t)S->nnzU * 8, hipMemcpyHostToDevice, st));
    SGM_HIP(hipMemcpyAsync(S->D, hD.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    SGM_HIP(hipStreamSynchronize(st));          // (the host vectors go out of scope)
    return SGM_OK;
}

// sparse_static_pattern_ldu_factorization (ldu_solvers.f90:275-387): the fill on the device, then one launch per level of
// the factorisation order -- or the host loop, *host_factor, for a chain
int factorise(IlduState *S, const Part &P, int32_t own, bool *host_factor)
{
    const int32_t n = S->n;
    hipStream_t st = g_rt.stream;
    hipLaunchKernelGGL(k_ildu_init, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, own, (const int32_t *)P.rowptr,
                       (const int32_t *)P.col, (const double *)P.val, (const int32_t *)S->dLptr, (const int32_t *)S->dLnode,
                       S->dLval, (const int32_t *)S->dUptr, (const int32_t *)S->dUnode, S->dUval, S->D);
    // (rows in the order of L's dependency levels, or -- grid-like factors -- of the grid's anti-diagonals)
    const std::vector<int32_t> &flp = S->forder ? S->flevel_ptr : S->L.level_ptr;
    const int32_t *ford = S->forder ? S->forder : S->L.order;
    const size_t nlev = flp.size() - 1;
    // (a chain of short rows only -- the host loop is O(len^3) per row and single-threaded: a chain of WIDE rows stays on the device)
    *host_factor = nlev > 4096 && (int64_t)nlev * 8 > (int64_t)n && S->maxL + S->maxU <= 16;
    if (*host_factor) SGM_TRY(factor_chain_on_host(S));
    for (size_t l = 0; !*host_factor && l + 1 < flp.size(); ++l) {
        const int32_t b = flp[l], e = flp[l + 1];
        if (S->maxL <= 4 && S->maxU <= 4) {
            hipLaunchKernelGGL((k_ildu_factor_level_short<4, 4>), dim3((e - b + 63) / 64), dim3(64), 0, st,
                               ford, b, e, (const int32_t *)S->dLptr, (const int32_t *)S->dLnode, S->dLval,
                               (const int32_t *)S->dUptr, (const int32_t *)S->dUnode, S->dUval, S->D);
            continue;
        }
        hipLaunchKernelGGL(k_ildu_factor_level, dim3((e - b + kBlock - 1) / kBlock), dim3(kBlock), 0, st,
                           ford, b, e, (const int32_t *)S->dLptr, (const int32_t *)S->dLnode, S->dLval,
                           (const int32_t *)S->dUptr, (const int32_t *)S->dUnode, S->dUval, S->D);
    }
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// Index work of the pipelines, once per pattern: grid-like factors (deps r-1, r-w) get the strip layout, a 3-D grid's the
// slab layout.  few: L has a few levels only -- neither applies and nobody needs the pattern on the host.
int strip_slab_index(IlduState *S, bool few)
{
    const int32_t n = S->n;
    hipStream_t st = g_rt.stream;
    free_grid(S->gL); free_grid(S->gU);
    dfree(S->gxL); dfree(S->gxU); dfree(S->gDp); dfree(S->gmapLU);
    S->gxL = S->gxU = S->gDp = nullptr; S->gmapLU = nullptr;
    S->grid_ok = false;
    int32_t wl = S->dev_wl, wu = S->dev_wu;          // (found on the device already when the pair is grid-like)
    if (!few && !wl && !S->dev_slab) {
        SGM_TRY(ensure_host_pattern(S));
        wl = grid_width(n, S->hLptr, S->hLnode, true);
        wu = grid_width(n, S->hUptr, S->hUnode, false);
    }
    if (S->opt.ildu_strips && wl >= 64 && wl == wu && (n + wl - 1) / wl >= 64) {
        SGM_TRY(build_grid(S->gL, n, wl, S->dLptr, S->dLnode, true));
        SGM_TRY(build_grid(S->gU, n, wl, S->dUptr, S->dUnode, false));
        if (S->gL.on && S->gU.on) {
            SGM_TRY(dalloc(&S->gxL, (size_t)S->gL.NP));
            SGM_TRY(dalloc(&S->gxU, (size_t)S->gU.NP));
            SGM_TRY(dalloc(&S->gDp, (size_t)S->gU.NP));
            SGM_TRY(dalloc(&S->gmapLU, (size_t)S->gU.NP));
            SGM_HIP(hipMemsetAsync(S->gmapLU, 0xff, (size_t)S->gU.NP * 4, st));
            hipLaunchKernelGGL(k_grid_map, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, n, (const int32_t *)S->gU.pos,
                               (const int32_t *)S->gL.pos, S->gmapLU);
            SGM_HIP(hipStreamSynchronize(st));
            dfree(S->gL.pos); dfree(S->gU.pos);
            S->gL.pos = S->gU.pos = nullptr;
        } else { free_grid(S->gL); free_grid(S->gU); }
    }
    slab3_free(S->slab);
    S->slab = nullptr;
    S->slab_ok = false;
    if (S->opt.ildu_strips && !few && !(S->gL.on && S->gU.on) && !S->dev_slab) SGM_TRY(ensure_host_pattern(S));
    if (S->opt.ildu_strips && !few && !(S->gL.on && S->gU.on))
        SGM_TRY(slab3_build(&S->slab, n, S->hLptr, S->hLnode, S->hUptr, S->hUnode, S->dLptr, S->dLnode, S->dUptr, S->dUnode));
    return SGM_OK;
}

// The new values into what the applies read (every setup): the pipeline's records -- or, where no pipelined path serves the
// pattern, the row-space copies or the level walkers' structures, built here when the pattern is new
int refresh_values(IlduState *S, LapTimer &lap)
{
    hipStream_t st = g_rt.stream;
    if (S->slab) SGM_TRY(slab3_refresh(S->slab, S->dLval, S->dUval, S->D));
    const bool have_grid = S->gL.on && S->gU.on;
    if (have_grid) {
        SGM_TRY(refresh_grid_values(S->gL, S->dLval));
        SGM_TRY(refresh_grid_values(S->gU, S->dUval));
        hipLaunchKernelGGL(k_pos_diag, dim3(vec_grid(S->gU.NP)), dim3(kBlock), 0, st, S->gU.NP, (const int32_t *)S->gU.row,
                           (const double *)S->D, S->gDp);
    }
    if (!have_grid && !S->slab) {         // no pipelined path for this pattern: the row-space sweeps or the level walkers serve it
        SGM_TRY(ensure_levels(S));
        lap("levels, row-space copy");
        if (!rows_serve(S)) {
            SGM_TRY(ensure_walkers(S));
            lap("level walkers' structures");
        }
    }
    lap("strip / slab records");
    return SGM_OK;
}

// The pipelines hand data between workgroups inside one launch: before one is trusted with a pattern it must reproduce the
// row-by-row sweeps of ldu_solve (ldu_solvers.f90:160-176, :208-265) bit for bit on a test vector, and raise no abort.
// Checked on the device, every row against the recurrence (k_sweep_check).  A pipeline that fails is switched off for this
// matrix, loudly, and the level-scheduled structures are built in its place.
int pipeline_self_check(IlduState *S, LapTimer &lap)
{
    const int32_t n = S->n;
    const bool have_grid = S->gL.on && S->gU.on;
    double *dr = nullptr, *dz = nullptr, *dy = nullptr;
    int32_t *dbad = nullptr;
    struct Tmp { double *&a, *&b, *&c; int32_t *&d; ~Tmp() { dfree(a); dfree(b); dfree(c); dfree(d); } } tmp{dr, dz, dy, dbad};
    SGM_TRY(dalloc(&dr, (size_t)n));
    SGM_TRY(dalloc(&dz, (size_t)n));
    SGM_TRY(dalloc(&dy, (size_t)n));
    SGM_TRY(dalloc(&dbad, 1));
    hipStream_t st2 = g_rt.stream;
    hipLaunchKernelGGL(k_check_vector, dim3(vec_grid(n)), dim3(kBlock), 0, st2, (int64_t)n, dr);
    (void)hipMemsetAsync(dz, 0, (size_t)n * 8, st2);
    (void)hipMemsetAsync(dy, 0, (size_t)n * 8, st2);
    (void)hipMemsetAsync(dbad, 0, 4, st2);
    if (have_grid) {
        apply_grid(S, dr, dz, nullptr, kStripSpinLimit, nullptr);
        grid_lower_result(S, dy);
    } else {
        slab3_apply(S->slab, dr, dz, nullptr, kStripSpinLimit, nullptr);
        slab3_lower_result(S->slab, dy);
    }
    const int cg = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_sweep_check, dim3(cg), dim3(kBlock), 0, st2, n, (const int32_t *)S->dLptr, (const int32_t *)S->dLnode,
                       (const double *)S->dLval, (const double *)dr, (const double *)nullptr, (const double *)dy, dbad);
    hipLaunchKernelGGL(k_sweep_check, dim3(cg), dim3(kBlock), 0, st2, n, (const int32_t *)S->dUptr, (const int32_t *)S->dUnode,
                       (const double *)S->dUval, (const double *)dy, (const double *)S->D, (const double *)dz, dbad);
    int32_t abL = 0, abU = 0, bad = 0;
    (void)hipMemcpyAsync(&bad, dbad, 4, hipMemcpyDeviceToHost, st2);
    if (have_grid) {
        (void)hipMemcpyAsync(&abL, S->gL.progress + S->gL.NI, 4, hipMemcpyDeviceToHost, st2);
        (void)hipMemcpyAsync(&abU, S->gU.progress + S->gU.NI, 4, hipMemcpyDeviceToHost, st2);
    }
    const hipError_t e = hipStreamSynchronize(st2);
    if (!have_grid && e == hipSuccess) (void)slab3_aborted(S->slab, &abL, &abU);
    const bool same = e == hipSuccess && !abL && !abU && bad == 0;
    if (have_grid) S->grid_ok = same; else S->slab_ok = same;
    if (!same)
        fprintf(stderr, "[sigma_hip] ILDU %s pipeline disabled for this matrix (self-check: abort %d/%d, %d rows differ)\n",
                have_grid ? "strip" : "slab", abL, abU, bad);
    lap("self-check");
    if (!same) {
        SGM_TRY(ensure_levels(S));
        if (!rows_serve(S)) SGM_TRY(ensure_walkers(S));
        lap("levels, walkers' structures");
    }
    return SGM_OK;
}

}  // namespace

// ILDU(0) of part P's diagonal block into S: the pattern and every index structure once per pattern (ldu_solvers.f90:117-125),
// the factorisation and the values of what the applies read at every setup.  The order of the launches, copies and
// synchronisations below is what the setup time is made of.
int sgm::ildu_setup_part(IlduState &state, const Part &src, int32_t fmt)
{
    IlduState *S = &state;
    Part ellview;
    struct EllView { Part &v; ~EllView() { dfree(v.rowptr); dfree(v.col); dfree(v.val); v.rowptr = nullptr; v.col = nullptr; v.val = nullptr; } } ellguard{ellview};
    const bool trim = fmt == SGM_FMT_ELL || src.edeg;     // (edeg on a CSR part: ELLPACK rows over ranks, sgm_ell_create_dist)
    if (trim) SGM_TRY(ell_view(src, fmt, ellview));
    const Part &P = trim ? ellview : src;
    static const bool timing = getenv("SGM_PC_TIMING") != nullptr;
    LapTimer lap{timing};
    const int32_t n = P.n;
    const bool fresh = S->n != n || !S->dLptr;             // ldu_solvers.f90:117-125: pattern once
    SGM_TRY(csr_need_arrays(P));          // (a part that kept only its sliced form rebuilds col / val for the setup)
    struct Release { const Part &p; ~Release() { csr_release_arrays(p); } } rel{P};
    const int32_t own = P.n_halo == 0 ? INT32_MAX : P.ncol_own;
    bool few = false;                     // L has at most kRowLevels levels (found on the device): no pipeline applies, no host pattern needed
    if (fresh) {
        free_ildu(*S);
        S->n = n;
        SGM_TRY(ildu_pattern(S, P, own));
        lap("pattern (device)");
        SGM_TRY(factor_order(S, &few, lap));
        SGM_TRY(dalloc(&S->dLval, (size_t)std::max(S->nnzL, 1)));
        SGM_TRY(dalloc(&S->dUval, (size_t)std::max(S->nnzU, 1)));
        SGM_TRY(dalloc(&S->D, (size_t)std::max(n, 1)));
        lap("levels of L");
    }
    S->n = n;
    S->host_vals = false;
    bool host_factor = false;
    if (n) SGM_TRY(factorise(S, P, own, &host_factor));
    lap(host_factor ? "factorisation (host: a chain)" : "factorisation (device)");
    // (the level-scheduled structures: ensure_levels, in refresh_values or on first need)
    S->levels_ready = false;
    S->walk_ready = false;
    if (fresh) S->levels_pattern = S->walk_pattern = false;
    if (fresh) SGM_TRY(strip_slab_index(S, few));
    lap("strip / slab index work");
    SGM_TRY(refresh_values(S, lap));
    if (((S->gL.on && S->gU.on) || S->slab) && fresh) SGM_TRY(pipeline_self_check(S, lap));
    return SGM_OK;
}
