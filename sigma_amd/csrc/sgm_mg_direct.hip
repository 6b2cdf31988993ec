// Multigrid, direct coarse solve: the coarsest level inverted once at setup, x = Ainv b in every V-cycle.
//
// Setup: D(i,j) = +0.0 plus the stored copies of (i,j) in stored order; W = [D | I]; for k = 0 .. n-1: p = the smallest
// i >= k that maximises |W(i,k)| (a NaN counts as the largest), piv(k) = p + 1, rows k and p swapped, row k divided by
// W(k,k), every other row i: W(i,j) = W(i,j) - (f * W(k,j)) with f = W(i,k) read before the update.  Ainv = the right block.
// Apply: columns in chunks of 256, s_c(i) = +0.0 plus the individually rounded products Ainv(i,j) * b(j) in ascending j,
// x(i) = +0.0 plus s_0(i), s_1(i), ... in ascending c.  Every operation is rounded on its own (-ffp-contract=off).
//
// W is held column-major (leading dimension lda = n rounded up to 64, the padding rows +0.0 and never touched), so a lane's
// neighbour in a column is its neighbour in memory, and the right block IS the layout the apply wants.
//
// The elimination is blocked: a panel of kGjPanel = 32 columns is factored by one workgroup, then its 32 steps are applied
// to every other column that can still change, each element read and written once.  Four launches per panel:
//   k_gj_panel   one workgroup of 1024: per step the arg-max of column k (the smallest index among equals), the refusal
//                test, the swap, the scaled pivot row and the rank-1 update INSIDE the panel; it leaves the multipliers
//                F(i, kk) = W(i,k) of every row at the position the row ends the panel in, and the divisors d(kk)
//   k_gj_swap    one lane per trailing column: the panel's row swaps, in order
//   k_gj_rows    half a wave per trailing column: the 32 panel rows of the column through the 32 steps (lane ii holds row
//                k0 + ii; at step kk lane kk divides, its value is broadcast as U(kk, j), the other lanes update) -- this is
//                both the forward and the Gauss-Jordan backward elimination among the pivot rows
//   k_gj_trail   every other row of the trailing columns: W(i,j) = W(i,j) - (F(i,kk) * U(kk,j)) for kk ascending, the 32
//                multipliers of the row in registers, a tile of columns per workgroup
// Bit-compatible with the step-by-step form: every element sees its updates in ascending k with the same f and the same
// scaled pivot row; a row swap moves whole rows, multipliers included, so swapping first and eliminating afterwards feeds every
// operation the same operands.  Columns j <= k of the left block are skipped: they are never read again (column j is read
// as f at step j only), so they cannot change Ainv or piv.  The right block is updated in full: a skipped
// W(i,j) - (f * +-0.0) would keep a -0.0 that the contract turns into +0.0, and would miss the NaN of an infinite f.
#include "sgm_pc_internal.hpp"

#include <chrono>
#include <climits>

namespace sgm {

constexpr int kGjPanel = 32;                      // columns per panel: the multipliers of a row fit 64 VGPRs in k_gj_trail
constexpr int kGjPanelBlock = 1024;
constexpr int kGjTile = 16;                       // trailing columns per workgroup of k_gj_trail
constexpr int kDirectChunk = 256;                 // columns per chunk of the apply: part of the contract
constexpr int kDirectRows = 64;                   // rows per workgroup of the apply
constexpr int kDirectBlock = 512;                 // 8 waves, two chunks each: the 16 chunks of 4096 columns in one pass
static_assert(SGM_MG_DIRECT_MAX_ROWS <= kDirectChunk * (kDirectBlock / 32), "one pass over the chunks");

typedef double f64x2d __attribute__((ext_vector_type(2)));

struct GjInfo { int32_t bad; int32_t badk; };      // a refused pivot: the flag, and the smallest 1-based step

struct MgDirect {
    int32_t n = 0, lda = 0;
    double *ainv = nullptr;        // device: lda x n, column-major (Ainv(i,j) at j * lda + i), rows n .. lda-1 = +0.0
    int32_t *piv = nullptr;        // device: n, 1-based
    double invert_ms = 0.0;
    std::vector<double> hinv;      // sgm_pc_get staging (row-major)
    std::vector<int32_t> hpiv;
};

// ------------------------------------------------------------------ setup kernels
// one lane per row: the stored entries into the zeroed dense array in stored order, and the row's 1.0 of the right block
__global__ void k_gj_densify(int32_t n, int32_t lda, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                             const double *__restrict__ val, double *__restrict__ W)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
        const int32_t j = col[e];
        if (j < 0 || j >= n) continue;                 // (a square level has none)
        double *w = W + (size_t)j * lda + i;
        *w = *w + val[e];
    }
    W[(size_t)(n + i) * lda + i] = 1.0;
}

// is (a, i) a better pivot candidate than (b, j)?  larger |.|, a NaN above everything, the smaller index among equals
__device__ inline bool gj_better(double a, int32_t i, double b, int32_t j)
{
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return i < j;
}

// trailing column number jt of the panel [k0, k0 + bw): the left block's columns behind the panel, then the right block
__device__ inline int32_t gj_trailing_column(int32_t n, int32_t k0, int32_t bw, int32_t jt)
{
    const int32_t nleft = n - k0 - bw;
    return jt < nleft ? k0 + bw + jt : n + (jt - nleft);
}

__global__ __launch_bounds__(kGjPanelBlock) void k_gj_panel(int32_t n, int32_t lda, int32_t k0, int32_t bw, double *__restrict__ W,
                                                            double *__restrict__ F, double *__restrict__ dpiv,
                                                            int32_t *__restrict__ piv, GjInfo *info)
{
    __shared__ double sa[kGjPanelBlock];
    __shared__ int32_t si[kGjPanelBlock];
    __shared__ int32_t sbad;
    __shared__ double srow[kGjPanel];
    if (info->bad) return;                             // a refused pivot in an earlier panel: nothing more is computed
    const int tid = threadIdx.x;
    for (int32_t kk = 0; kk < bw; ++kk) {
        const int32_t k = k0 + kk;
        double *c = W + (size_t)k * lda;
        double a = -1.0;                               // below every |.|
        int32_t ia = INT_MAX;
        for (int32_t i = k + tid; i < n; i += kGjPanelBlock) {
            const double v = fabs(c[i]);
            if (gj_better(v, i, a, ia)) { a = v; ia = i; }
        }
        sa[tid] = a; si[tid] = ia;
        __syncthreads();
        for (int s = kGjPanelBlock / 2; s > 0; s >>= 1) {
            if (tid < s && gj_better(sa[tid + s], si[tid + s], sa[tid], si[tid])) { sa[tid] = sa[tid + s]; si[tid] = si[tid + s]; }
            __syncthreads();
        }
        const int32_t p = si[0];
        const double d = c[p];
        if (tid == 0) {
            const int bad = d == 0.0 || d != d || fabs(d) == INFINITY;
            sbad = bad;
            if (bad) {
                info->bad = 1;
                atomicMin(&info->badk, k + 1);
            }
            piv[k] = p + 1;
            dpiv[kk] = d;
        }
        __syncthreads();                               // (also: every read of si[0] and c[p] is done)
        if (sbad) return;
        // rows k and p swapped: the panel's live columns k .. k0+bw-1 and the multipliers of the steps before
        if (p != k) {
            if (tid < bw - kk) {
                double *cj = W + (size_t)(k + tid) * lda;
                const double t = cj[k]; cj[k] = cj[p]; cj[p] = t;
            } else if (tid >= 64 && tid < 64 + kk) {
                double *fj = F + (size_t)(tid - 64) * lda;
                const double t = fj[k]; fj[k] = fj[p]; fj[p] = t;
            }
        }
        __syncthreads();
        // the pivot row scaled (column k itself becomes 1 and is never read again); its live part also goes to LDS
        const int nb = bw - kk - 1;                    // panel columns behind k
        if (tid < nb) {
            double *cj = W + (size_t)(k + 1 + tid) * lda;
            const double v = cj[k] / d;
            cj[k] = v;
            srow[tid] = v;
        }
        __syncthreads();
        // f = column k, kept as F(., kk); the panel's columns behind k updated, row k left as it is.  A row's elements are
        // requested eight at a time, then updated, then stored: a load waits for no store of its group
        double *fk = F + (size_t)kk * lda;
        for (int32_t i = tid; i < n; i += kGjPanelBlock) {
            const double f = c[i];
            fk[i] = f;
            if (i == k) continue;
            double *wi = W + (size_t)(k + 1) * lda + i;
            for (int t0 = 0; t0 < nb; t0 += 8) {
                double w[8];
#pragma unroll
                for (int t = 0; t < 8; ++t) w[t] = t0 + t < nb ? wi[(size_t)(t0 + t) * lda] : 0.0;
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    if (t0 + t < nb) wi[(size_t)(t0 + t) * lda] = w[t] - (f * srow[t0 + t]);
            }
        }
        __syncthreads();
    }
}

// the panel's row swaps on the trailing columns, one lane per column, in the order the panel made them
__global__ void k_gj_swap(int32_t n, int32_t lda, int32_t k0, int32_t bw, int32_t ntrail, double *__restrict__ W,
                          const int32_t *__restrict__ piv, const GjInfo *__restrict__ info)
{
    if (info->bad) return;
    const int32_t jt = blockIdx.x * blockDim.x + threadIdx.x;
    if (jt >= ntrail) return;
    double *c = W + (size_t)gj_trailing_column(n, k0, bw, jt) * lda;
    for (int32_t kk = 0; kk < bw; ++kk) {
        const int32_t k = k0 + kk, p = piv[k] - 1;
        if (p != k) { const double t = c[k]; c[k] = c[p]; c[p] = t; }
    }
}

// the bw panel rows of a trailing column through the panel's steps: half a wave per column, lane ii = row k0 + ii
__global__ __launch_bounds__(256) void k_gj_rows(int32_t n, int32_t lda, int32_t k0, int32_t bw, int32_t ntrail, double *__restrict__ W,
                                                 const double *__restrict__ F, const double *__restrict__ dpiv,
                                                 double *__restrict__ U, const GjInfo *__restrict__ info)
{
    if (info->bad) return;
    const int32_t jt = blockIdx.x * (256 / kGjPanel) + (threadIdx.x / kGjPanel);
    const int ii = threadIdx.x % kGjPanel;
    const bool col_ok = jt < ntrail, mine = col_ok && ii < bw;
    double *c = W + (size_t)(col_ok ? gj_trailing_column(n, k0, bw, jt) : 0) * lda;
    double v = mine ? c[k0 + ii] : 0.0;
    const double dv = ii < bw ? dpiv[ii] : 1.0;
    double f[kGjPanel];
#pragma unroll
    for (int kk = 0; kk < kGjPanel; ++kk) f[kk] = mine && kk < bw ? F[(size_t)kk * lda + k0 + ii] : 0.0;
#pragma unroll
    for (int kk = 0; kk < kGjPanel; ++kk) {
        if (kk < bw) {                                 // (uniform: the shuffle is reached by every lane of the wave)
            if (ii == kk) v = v / dv;
            const double u = __shfl(v, kk, kGjPanel);
            if (mine && ii == kk) U[(size_t)jt * kGjPanel + kk] = u;
            if (mine && ii != kk) v = v - (f[kk] * u);
        }
    }
    if (mine) c[k0 + ii] = v;
}

// every row outside the panel, a tile of trailing columns per workgroup: the row's multipliers in registers, each element
// read once, taken through the panel's steps in ascending k, written once
__global__ __launch_bounds__(256) void k_gj_trail(int32_t n, int32_t lda, int32_t k0, int32_t bw, int32_t ntrail, double *__restrict__ W,
                                                  const double *__restrict__ F, const double *__restrict__ U,
                                                  const GjInfo *__restrict__ info)
{
    __shared__ double su[kGjTile][kGjPanel];
    if (info->bad) return;
    const int32_t jt0 = blockIdx.y * kGjTile;
    const int32_t nj = min(kGjTile, ntrail - jt0);
    for (int t = threadIdx.x; t < nj * kGjPanel; t += 256) su[t / kGjPanel][t % kGjPanel] = U[(size_t)jt0 * kGjPanel + t];
    __syncthreads();
    const int32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || (i >= k0 && i < k0 + bw)) return;
    double f[kGjPanel];
#pragma unroll
    for (int kk = 0; kk < kGjPanel; ++kk) f[kk] = kk < bw ? F[(size_t)kk * lda + i] : 0.0;
    for (int32_t t = 0; t < nj; ++t) {
        double *c = W + (size_t)gj_trailing_column(n, k0, bw, jt0 + t) * lda + i;
        double w = *c;
#pragma unroll
        for (int kk = 0; kk < kGjPanel; ++kk)
            if (kk < bw) w = w - (f[kk] * su[t][kk]);
        *c = w;
    }
}

// ------------------------------------------------------------------ apply
// One workgroup per 64 rows.  A half-wave owns one chunk of 256 columns: lane h of it holds rows 2h, 2h + 1 of the block and
// walks the chunk's columns in ascending order with one 16-byte load per column (the 32 lanes read 512 contiguous bytes),
// eight columns requested at a time and the next eight requested before the current eight are summed.  The chunk sums meet in
// LDS and the lane that owns a row adds them in ascending chunk order.
__global__ __launch_bounds__(kDirectBlock) void k_mg_direct_apply(int32_t n, int32_t lda, const double *__restrict__ ainv,
                                                                  const double *__restrict__ b, double *__restrict__ x,
                                                                  const int *__restrict__ flag)
{
    constexpr int U = 8;
    constexpr int SLOTS = kDirectBlock / 32;           // chunks in flight
    __shared__ double sb[SGM_MG_DIRECT_MAX_ROWS];
    __shared__ double ss[SLOTS][kDirectRows];
    const int st = flag ? *flag : 0;
    const int tid = threadIdx.x;
    const int32_t row0 = blockIdx.x * kDirectRows;
    const int32_t nch = (n + kDirectChunk - 1) / kDirectChunk;
    if (st) return;
    for (int32_t j = tid; j < n; j += kDirectBlock) sb[j] = b[j];
    __syncthreads();
    const int ch = tid >> 5, h = tid & 31;
    if (ch < nch) {
        const int32_t j0 = ch * kDirectChunk, j1 = min(j0 + kDirectChunk, n);
        const f64x2d *a = reinterpret_cast<const f64x2d *>(ainv + (size_t)j0 * lda + row0) + h;
        const size_t ld2 = (size_t)lda / 2;
        f64x2d s = {0.0, 0.0};
        f64x2d cur[U] = {}, nxt[U] = {};
        const int32_t cols = j1 - j0, full = cols / U;
        if (full > 0) {
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = __builtin_nontemporal_load(a + (size_t)u * ld2);
        }
        for (int32_t t = 0; t < full; ++t) {
            const f64x2d *an = a + (size_t)(t + 1) * U * ld2;
            if (t + 1 < full) {
#pragma unroll
                for (int u = 0; u < U; ++u) nxt[u] = __builtin_nontemporal_load(an + (size_t)u * ld2);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const double bj = sb[j0 + t * U + u];
                s.x = s.x + cur[u].x * bj;
                s.y = s.y + cur[u].y * bj;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
        for (int32_t jj = full * U; jj < cols; ++jj) {
            const f64x2d v = a[(size_t)jj * ld2];
            const double bj = sb[j0 + jj];
            s.x = s.x + v.x * bj;
            s.y = s.y + v.y * bj;
        }
        ss[ch][2 * h] = s.x;
        ss[ch][2 * h + 1] = s.y;
    }
    __syncthreads();
    if (tid < kDirectRows && row0 + tid < n) {
        double z = 0.0;
        for (int32_t c = 0; c < nch; ++c) z = z + ss[c][tid];
        x[row0 + tid] = z;
    }
}

// ------------------------------------------------------------------ host
void mg_direct_free(MgDirect *D)
{
    if (!D) return;
    dfree(D->ainv); dfree(D->piv);
    delete D;
}

int mg_direct_rows(const MgDirect *D) { return D ? D->n : 0; }
double mg_direct_invert_ms(const MgDirect *D) { return D ? D->invert_ms : 0.0; }

// *out = the inverse of the single-GPU CSR matrix A (a new object; the caller frees the one it held).  Refusals leave *out null.
int mg_direct_setup(MgDirect **out, sgm_mat A)
{
    *out = nullptr;
    const int32_t n = A->nrow;
    if (n > SGM_MG_DIRECT_MAX_ROWS)
        return fail(SGM_ERR_UNSUPPORTED, "multigrid: the coarsest level has %d rows, the direct coarse solve takes at most %d "
                    "(SGM_MG_DIRECT_MAX_ROWS): coarsen further or use the coarse sweeps", n, SGM_MG_DIRECT_MAX_ROWS);
    const auto t0 = std::chrono::steady_clock::now();
    MgDirect *D = new MgDirect;
    struct Guard { MgDirect *D; double *W = nullptr, *F = nullptr, *U = nullptr, *dpiv = nullptr; GjInfo *info = nullptr; bool keep = false;
                   ~Guard() { dfree(W); dfree(F); dfree(U); dfree(dpiv); dfree(info); if (!keep) mg_direct_free(D); } } g{D};
    D->n = n;
    D->lda = (n + 63) / 64 * 64;
    const size_t lda = (size_t)D->lda;
    SGM_TRY(dalloc(&D->ainv, lda * (size_t)n));
    SGM_TRY(dalloc(&D->piv, (size_t)n));
    if (n == 0) { *out = D; g.keep = true; return SGM_OK; }
    SGM_TRY(dalloc(&g.W, lda * 2 * (size_t)n));
    SGM_TRY(dalloc(&g.F, lda * kGjPanel));                       // the multipliers of one panel, column-major
    SGM_TRY(dalloc(&g.U, (size_t)2 * n * kGjPanel));             // the scaled pivot-row values of its trailing columns
    SGM_TRY(dalloc(&g.dpiv, (size_t)kGjPanel));
    SGM_TRY(dalloc(&g.info, 1));
    hipStream_t st = g_rt.stream;
    SGM_HIP(hipMemsetAsync(g.W, 0, lda * 2 * (size_t)n * sizeof(double), st));
    const GjInfo start = {0, INT_MAX};
    SGM_HIP(hipMemcpyAsync(g.info, &start, sizeof start, hipMemcpyHostToDevice, st));
    SGM_HIP(hipStreamSynchronize(st));                 // (`start` is on this frame)
    {
        const Part &p = A->parts[0];
        SGM_TRY(csr_need_arrays(p));
        hipLaunchKernelGGL(k_gj_densify, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n, D->lda,
                           (const int32_t *)p.rowptr, (const int32_t *)p.col, (const double *)p.val, g.W);
        const hipError_t e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(st);       // the arrays may go away below
        csr_release_arrays(p);
        if (e != hipSuccess || e2 != hipSuccess)
            return fail(SGM_ERR_HIP, "multigrid: dense copy of the coarsest level: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    for (int32_t k0 = 0; k0 < n; k0 += kGjPanel) {
        const int32_t bw = std::min(kGjPanel, n - k0), ntrail = 2 * n - k0 - bw;
        hipLaunchKernelGGL(k_gj_panel, dim3(1), dim3(kGjPanelBlock), 0, st, n, D->lda, k0, bw, g.W, g.F, g.dpiv, D->piv, g.info);
        hipLaunchKernelGGL(k_gj_swap, dim3((unsigned)((ntrail + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, n, D->lda, k0, bw, ntrail, g.W,
                           (const int32_t *)D->piv, (const GjInfo *)g.info);
        hipLaunchKernelGGL(k_gj_rows, dim3((unsigned)((ntrail + 256 / kGjPanel - 1) / (256 / kGjPanel))), dim3(256), 0, st, n, D->lda, k0, bw,
                           ntrail, g.W, (const double *)g.F, (const double *)g.dpiv, g.U, (const GjInfo *)g.info);
        hipLaunchKernelGGL(k_gj_trail, dim3((unsigned)((n + 255) / 256), (unsigned)((ntrail + kGjTile - 1) / kGjTile)), dim3(256), 0, st,
                           n, D->lda, k0, bw, ntrail, g.W, (const double *)g.F, (const double *)g.U, (const GjInfo *)g.info);
    }
    SGM_HIP(hipGetLastError());
    GjInfo end;
    SGM_HIP(hipMemcpyAsync(&end, g.info, sizeof end, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipMemcpyAsync(D->ainv, g.W + lda * (size_t)n, lda * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (end.bad)
        return fail(SGM_ERR_UNSUPPORTED, "multigrid: direct coarse solve: singular or non-finite coarse level (%d rows) at "
                    "elimination step %d", n, end.badk);
    D->invert_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = D;
    g.keep = true;
    return SGM_OK;
}

// x = Ainv b on device vectors (b != x), stream-ordered
int mg_direct_apply(const MgDirect *D, const double *b, double *x, const int *flag)
{
    if (D->n == 0) return SGM_OK;
    hipLaunchKernelGGL(k_mg_direct_apply, dim3((unsigned)(D->lda / kDirectRows)), dim3(kDirectBlock), 0, g_rt.stream, D->n, D->lda,
                       (const double *)D->ainv, b, x, flag);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// "mg_coarse_inverse": n * n doubles, row-major; "mg_coarse_pivots": n int32, 1-based
int mg_direct_get(MgDirect *D, const char *name, const void **src, size_t *sz)
{
    const std::string nm(name);
    const size_t n = (size_t)D->n, lda = (size_t)D->lda;
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    if (nm == "mg_coarse_pivots") {
        D->hpiv.assign(n, 0);
        if (n) SGM_HIP(hipMemcpy(D->hpiv.data(), D->piv, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        *src = D->hpiv.data(); *sz = n * sizeof(int32_t);
        return SGM_OK;
    }
    std::vector<double> cm(lda * n);
    if (n) SGM_TRY(copy_big(cm.data(), D->ainv, lda * n * sizeof(double), hipMemcpyDeviceToHost));
    D->hinv.resize(n * n);
    for (size_t j = 0; j < n; ++j)
        for (size_t i = 0; i < n; ++i) D->hinv[i * n + j] = cm[j * lda + i];
    *src = D->hinv.data(); *sz = n * n * sizeof(double);
    return SGM_OK;
}

}  // namespace sgm
