// Multi-vector products Y = [Y +] op(A) X (sgm_mat_matmat, include/sigma_hip.h).
//
// Contract: column j of Y holds exactly the bits the single-vector product (sgm_mat_matvec / _add / _t / _t_add) leaves for
// x = X(:, j): per row +0.0 (or y0, or -- transpose with add -- the chained sum) plus the individually rounded products in
// stored order.  X and Y are column-major with leading dimensions ldx / ldy.
//
// Native kernels serve the three sliced forms in their resident layouts (no new copy of the matrix): the slice's code words
// and values are loaded ONCE and used for KB columns, so a block of KB columns moves the matrix once instead of KB times.
//   k_mm_sl    the 4-bit form (k_csr_sl's, also sliced ELLPACK): row sums by sl_row_sums<W>, the single-vector kernel's own
//   k_mm_slb   the 1-byte form (k_csr_slb's): chunks of 8 slots; a chunk's values and codes once, then per column its 16
//              gathers and its additions in slot order
//   k_mm_sl32  the int32-column form (k_csr_sl32's): the same with the columns beside the values
// Slice map (first_slice), the `sl += gridDim.x` loop, ADD and the chain bit are the single-vector kernels'; no fused dots,
// no stop flag.  Every other layout -- and a matrix whose slice_sched option is on -- runs the column loop: one existing
// product per column.
//
// A call with k columns is cut left to right into blocks of the largest selected width that fits; what is left over
// (a last single column) goes through the existing product.  The selected widths per form are the SGM_MM_*_KBS lists below:
// a (form, KB) pair stays in the list -- and in the build -- only if it measured faster than KB single products
// (profiles/matmat/README.md).
#include "sgm_spmv_device.hpp"

namespace sgm {

// block widths per form, descending (instantiated = selected).  KB = 8 of the 1-byte and int32 forms is not built: the
// compiler's report showed one wave per SIMD (256 VGPRs + accumulation registers; W = 15 with scratch) -- a chunk's 16 gathers
// for 8 columns are 128 loads in flight per lane (profiles/matmat/resource_usage.txt lists what is built)
#define SGM_MM_SL_KBS(X) X(8) X(4) X(2)
#define SGM_MM_SLB_KBS(X) X(4) X(2)
#define SGM_MM_SL32_KBS(X) X(4) X(2)

// ------------------------------------------------------------------ kernels
template <int W, int KB, bool ADD>
__global__ __launch_bounds__(256) void k_mm_sl(
    int32_t n, const uint32_t *__restrict__ scode, const int32_t *__restrict__ dict, const double *__restrict__ sval,
    const double *__restrict__ x, int64_t ldx, double *__restrict__ y, int64_t ldy, int remap)
{
    constexpr int BLOCK = 256;
    __shared__ int32_t dl[16];
    const int tid = threadIdx.x;
    const bool chain = (remap & kChainBit) != 0;
    const int32_t dv = tid < 16 ? dict[tid] : 0;
    const int64_t nsl = ((int64_t)n + kSlRows - 1) / kSlRows;
    double dwy = 0.0, dyy = 0.0;        // (pair_finish's fused-dot operands: not used here)

    int64_t sl = first_slice(remap & kSliceMapBits);
    u32x2 cw = {0xffffffffu, 0xffffffffu};
    f64x2 v[W];
    auto load_slice = [&](int64_t s_) {      // as k_csr_sl: the code words and the W value pairs of the lane's two rows
        const int32_t row_ = (int32_t)(s_ * kSlRows) + 2 * tid;
        cw = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(scode + row_));
        const f64x2 *vb = reinterpret_cast<const f64x2 *>(sval + s_ * (int64_t)(W * kSlRows)) + tid;
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = __builtin_nontemporal_load(vb + u * BLOCK);
    };
    bool have = sl < nsl;
    if (have) load_slice(sl);
    if (tid < 16) dl[tid] = dv;
    __syncthreads();
    while (have) {
        const int32_t row = (int32_t)(sl * kSlRows) + 2 * tid;
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const double *xj = x + j * ldx;
            double *yj = y + j * ldy;
            const f64x2 y0 = pair_load_y0<ADD>(yj, row, n);
            const f64x2 z = sl_row_sums<W>(pair_start<ADD>(y0, chain), cw, v, xj, row, dl);
            pair_finish<ADD, false, false>(yj, nullptr, row, n, y0, z, chain, dwy, dyy);
        }
        sl += gridDim.x;
        have = sl < nsl;
        if (have) load_slice(sl);
    }
}

// one column's share of a chunk of CNT slots, 1-byte codes: its 2 CNT gathers first, then the additions in slot order
template <int CNT>
__device__ __forceinline__ f64x2 mm_slb_chunk(f64x2 z, u32x4s cw, const f64x2 (&v)[8], const double *__restrict__ x, int32_t row,
                                              const int32_t *dl)
{
    double xa[CNT], xb[CNT];
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
        const uint32_t ca = ((u < 4 ? cw.x : cw.y) >> (8 * (u & 3))) & 255u;
        const uint32_t cbv = ((u < 4 ? cw.z : cw.w) >> (8 * (u & 3))) & 255u;
        xa[u] = ca != 255u ? x[row + dl[ca]] : 0.0;
        xb[u] = cbv != 255u ? x[row + 1 + dl[cbv]] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
        const uint32_t ca = ((u < 4 ? cw.x : cw.y) >> (8 * (u & 3))) & 255u;
        const uint32_t cbv = ((u < 4 ? cw.z : cw.w) >> (8 * (u & 3))) & 255u;
        if (ca != 255u) z.x = z.x + v[u].x * xa[u];
        if (cbv != 255u) z.y = z.y + v[u].y * xb[u];
    }
    return z;
}

template <int W, int KB, bool ADD>
__global__ __launch_bounds__(256) void k_mm_slb(
    int32_t n, const uint8_t *__restrict__ sbcode, const int32_t *__restrict__ dict, const double *__restrict__ sval,
    const double *__restrict__ x, int64_t ldx, double *__restrict__ y, int64_t ldy, int remap)
{
    constexpr int BLOCK = 256;
    constexpr int NCH = (W + 7) / 8;
    static_assert(W >= 9 && W <= 32, "rows of 9..32 entries");
    __shared__ int32_t dl[256];
    const int tid = threadIdx.x;
    dl[tid] = dict[tid];
    __syncthreads();
    const bool chain = (remap & kChainBit) != 0;
    const int64_t nsl = ((int64_t)n + kSlRows - 1) / kSlRows;
    double dwy = 0.0, dyy = 0.0;

    for (int64_t sl = first_slice(remap & kSliceMapBits); sl < nsl; sl += gridDim.x) {
        const int32_t row = (int32_t)(sl * kSlRows) + 2 * tid;
        const f64x2 *vb = reinterpret_cast<const f64x2 *>(sval + sl * (int64_t)W * kSlRows) + tid;
        const u32x4s *cb = reinterpret_cast<const u32x4s *>(sbcode + sl * (int64_t)(NCH * 8 * kSlRows)) + tid;
        f64x2 y0[KB], z[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            y0[j] = pair_load_y0<ADD>(y + j * ldy, row, n);
            z[j] = pair_start<ADD>(y0[j], chain);
        }
        // one chunk's registers live at a time (a rolled loop over the full chunks, then the tail)
        auto chunk = [&](int c, auto cnt_tag) {
            constexpr int CNT = decltype(cnt_tag)::value;
            f64x2 v[8];
            const u32x4s cw = __builtin_nontemporal_load(cb + c * BLOCK);
#pragma unroll
            for (int u = 0; u < CNT; ++u) v[u] = __builtin_nontemporal_load(vb + (c * 8 + u) * BLOCK);
#pragma unroll
            for (int j = 0; j < KB; ++j) z[j] = mm_slb_chunk<CNT>(z[j], cw, v, x + j * ldx, row, dl);
        };
#pragma unroll 1
        for (int c = 0; c < W / 8; ++c) chunk(c, std::integral_constant<int, 8>{});
        if (W % 8) chunk(W / 8, std::integral_constant<int, (W % 8 ? W % 8 : 8)>{});
#pragma unroll
        for (int j = 0; j < KB; ++j) pair_finish<ADD, false, false>(y + j * ldy, nullptr, row, n, y0[j], z[j], chain, dwy, dyy);
    }
}

// the same for int32 columns (-1 = no entry)
template <int CNT>
__device__ __forceinline__ f64x2 mm_sl32_chunk(f64x2 z, const i32x2 (&cc)[8], const f64x2 (&v)[8], const double *__restrict__ x)
{
    double xa[CNT], xb[CNT];
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
        xa[u] = cc[u].x >= 0 ? x[cc[u].x] : 0.0;
        xb[u] = cc[u].y >= 0 ? x[cc[u].y] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < CNT; ++u) {
        if (cc[u].x >= 0) z.x = z.x + v[u].x * xa[u];
        if (cc[u].y >= 0) z.y = z.y + v[u].y * xb[u];
    }
    return z;
}

template <int W, int KB, bool ADD>
__global__ __launch_bounds__(256) void k_mm_sl32(
    int32_t n, const int32_t *__restrict__ scol, const double *__restrict__ sval,
    const double *__restrict__ x, int64_t ldx, double *__restrict__ y, int64_t ldy, int remap)
{
    constexpr int BLOCK = 256;
    const int tid = threadIdx.x;
    const bool chain = (remap & kChainBit) != 0;
    const int64_t nsl = ((int64_t)n + kSlRows - 1) / kSlRows;
    double dwy = 0.0, dyy = 0.0;

    for (int64_t sl = first_slice(remap & kSliceMapBits); sl < nsl; sl += gridDim.x) {
        const int32_t row = (int32_t)(sl * kSlRows) + 2 * tid;
        const f64x2 *vb = reinterpret_cast<const f64x2 *>(sval + sl * (int64_t)(W * kSlRows)) + tid;
        const i32x2 *cb = reinterpret_cast<const i32x2 *>(scol + sl * (int64_t)(W * kSlRows)) + tid;
        f64x2 y0[KB], z[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            y0[j] = pair_load_y0<ADD>(y + j * ldy, row, n);
            z[j] = pair_start<ADD>(y0[j], chain);
        }
        auto chunk = [&](int c0, auto cnt_tag) {
            constexpr int CNT = decltype(cnt_tag)::value;
            f64x2 v[8];
            i32x2 cc[8];
#pragma unroll
            for (int u = 0; u < CNT; ++u) {
                v[u] = __builtin_nontemporal_load(vb + (c0 + u) * BLOCK);
                cc[u] = __builtin_nontemporal_load(cb + (c0 + u) * BLOCK);
            }
#pragma unroll
            for (int j = 0; j < KB; ++j) z[j] = mm_sl32_chunk<CNT>(z[j], cc, v, x + j * ldx);
        };
#pragma unroll 1
        for (int c = 0; c < W / 8; ++c) chunk(c * 8, std::integral_constant<int, 8>{});
        if (W % 8) chunk(W / 8 * 8, std::integral_constant<int, (W % 8 ? W % 8 : 8)>{});
#pragma unroll
        for (int j = 0; j < KB; ++j) pair_finish<ADD, false, false>(y + j * ldy, nullptr, row, n, y0[j], z[j], chain, dwy, dyy);
    }
}

// ------------------------------------------------------------------ selection
enum { MM_COLUMNS = 0, MM_SL = 1, MM_SLB = 2, MM_SL32 = 3 };
static const char *const kMmName[] = {"columns", "k_mm_sl", "k_mm_slb", "k_mm_sl32"};

#define MM_LIST(KK) KK,
static const int kMmSlKbs[] = {SGM_MM_SL_KBS(MM_LIST) 0};
static const int kMmSlbKbs[] = {SGM_MM_SLB_KBS(MM_LIST) 0};
static const int kMmSl32Kbs[] = {SGM_MM_SL32_KBS(MM_LIST) 0};
#undef MM_LIST
static const int *mm_widths(int form) { return form == MM_SL ? kMmSlKbs : form == MM_SLB ? kMmSlbKbs : kMmSl32Kbs; }

static bool mm_has_slot_width(int form, int sw)
{
#define LV(WW) if (sw == WW) return true;
    if (form == MM_SL) { SGM_SL_WIDTHS(LV) }
    if (form == MM_SLB) { SGM_SLB_WIDTHS(LV) }
    if (form == MM_SL32) { SGM_SL32_WIDTHS(LV) }
#undef LV
    return false;
}

// the native form of a matrix (M = the matrix a product runs on: A, or the cached A^T), or MM_COLUMNS.  The order of the tests
// is spmv_parts' / launch_range's: the form named here is the one the single-vector product runs.
static int mm_form(const sgm_mat_s *M)
{
    if (M->fmt != SGM_FMT_CSR && M->fmt != SGM_FMT_ELL) return MM_COLUMNS;
    if (M->distributed()) return MM_COLUMNS;
    const Part &p = M->parts[0];
    if (p.n_halo || p.opt.slice_sched || use_ell_colblock(p)) return MM_COLUMNS;
    int form = MM_COLUMNS;
    if (M->fmt == SGM_FMT_ELL) form = use_sliced_ell(p) ? MM_SL : MM_COLUMNS;
    else if (use_sliced(p)) form = MM_SL;
    else if (use_slicedb(p)) form = MM_SLB;
    else if (use_sliced32(p)) form = MM_SL32;
    if (form != MM_COLUMNS && (!mm_has_slot_width(form, p.sw) || !mm_widths(form)[0])) form = MM_COLUMNS;
    return form;
}

// the widths a call with k columns is cut into, left to right: the largest selected width that fits (and is <= cap), 1 for
// what no width fits
static void mm_blocks(int form, int k, int cap, std::vector<int> &out)
{
    out.clear();
    for (int rem = k; rem > 0;) {
        int w = 1;
        if (form != MM_COLUMNS)
            for (const int *kb = mm_widths(form); *kb; ++kb)
                if (*kb <= rem && (cap <= 0 || *kb <= cap)) { w = *kb; break; }
        out.push_back(w);
        rem -= w;
    }
}

// ------------------------------------------------------------------ launches
template <int KB, bool ADD>
static bool mm_launch_sl(const Part &p, int grid, int remap, const double *x, int64_t ldx, double *y, int64_t ldy)
{
#define LV(WW)                                                                                                              \
    if (p.sw == WW) {                                                                                                       \
        hipLaunchKernelGGL((k_mm_sl<WW, KB, ADD>), dim3(grid), dim3(256), 0, g_rt.stream, p.n, (const uint32_t *)p.scode,   \
                           (const int32_t *)p.dict, (const double *)p.sval, x, ldx, y, ldy, remap);                        \
        return true;                                                                                                        \
    }
    SGM_SL_WIDTHS(LV)
#undef LV
    return false;
}
template <int KB, bool ADD>
static bool mm_launch_slb(const Part &p, int grid, int remap, const double *x, int64_t ldx, double *y, int64_t ldy)
{
#define LV(WW)                                                                                                              \
    if (p.sw == WW) {                                                                                                       \
        hipLaunchKernelGGL((k_mm_slb<WW, KB, ADD>), dim3(grid), dim3(256), 0, g_rt.stream, p.n, (const uint8_t *)p.sbcode,  \
                           (const int32_t *)p.dict, (const double *)p.sval, x, ldx, y, ldy, remap);                        \
        return true;                                                                                                        \
    }
    SGM_SLB_WIDTHS(LV)
#undef LV
    return false;
}
template <int KB, bool ADD>
static bool mm_launch_sl32(const Part &p, int grid, int remap, const double *x, int64_t ldx, double *y, int64_t ldy)
{
#define LV(WW)                                                                                                              \
    if (p.sw == WW) {                                                                                                       \
        hipLaunchKernelGGL((k_mm_sl32<WW, KB, ADD>), dim3(grid), dim3(256), 0, g_rt.stream, p.n, (const int32_t *)p.scol,   \
                           (const double *)p.sval, x, ldx, y, ldy, remap);                                                 \
        return true;                                                                                                        \
    }
    SGM_SL32_WIDTHS(LV)
#undef LV
    return false;
}

static bool mm_launch(int form, int kb, bool add, const Part &p, int grid, int remap, const double *x, int64_t ldx, double *y,
                      int64_t ldy)
{
#define LK_SL(KK) if (form == MM_SL && kb == KK) return add ? mm_launch_sl<KK, true>(p, grid, remap, x, ldx, y, ldy) : mm_launch_sl<KK, false>(p, grid, remap, x, ldx, y, ldy);
#define LK_SLB(KK) if (form == MM_SLB && kb == KK) return add ? mm_launch_slb<KK, true>(p, grid, remap, x, ldx, y, ldy) : mm_launch_slb<KK, false>(p, grid, remap, x, ldx, y, ldy);
#define LK_SL32(KK) if (form == MM_SL32 && kb == KK) return add ? mm_launch_sl32<KK, true>(p, grid, remap, x, ldx, y, ldy) : mm_launch_sl32<KK, false>(p, grid, remap, x, ldx, y, ldy);
    SGM_MM_SL_KBS(LK_SL)
    SGM_MM_SLB_KBS(LK_SLB)
    SGM_MM_SL32_KBS(LK_SL32)
#undef LK_SL
#undef LK_SLB
#undef LK_SL32
    return false;
}

// the grid of the single-vector product without fused dots (spmv_ranges / ell_grid), capped for the probe
static int mm_grid(const sgm_mat_s *M, int grid_cap)
{
    const Part &p = M->parts[0];
    int grid = M->fmt == SGM_FMT_ELL ? ell_grid(p) : grid_for_rows(p, p.n > 0 ? p.n : 1, kMaxGrid, false);
    if (grid_cap > 0) grid = std::min(grid, std::max(8, grid_cap / 8 * 8));
    return grid;
}

// ------------------------------------------------------------------ operands
// A caller block staged on the device if it lives on the host or if not every column is 16-byte aligned (stage_in's rule for a
// vector, per column): k columns of `len` entries, leading dimension ld (the staged copy: len rounded up to even)
struct StagedBlock {
    double *dev = nullptr;
    int64_t ld = 0;
    bool owned = false;
    ~StagedBlock() { if (owned) dfree(dev); }
};
static int stage_block_in(StagedBlock &s, const double *v, int64_t ld, int64_t len, int k, int where, bool copy)
{
    if (where == SGM_DEVICE && (reinterpret_cast<uintptr_t>(v) & 15) == 0 && (ld & 1) == 0) {
        s.dev = const_cast<double *>(v);
        s.ld = ld;
        return SGM_OK;
    }
    s.ld = (len + 1) & ~(int64_t)1;
    SGM_TRY(dalloc(&s.dev, (size_t)std::max<int64_t>(s.ld, 2) * k));
    s.owned = true;
    if (copy && len)
        for (int j = 0; j < k; ++j)
            SGM_HIP(hipMemcpyAsync(s.dev + j * s.ld, v + j * ld, (size_t)len * 8,
                                   where == SGM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, g_rt.stream));
    return SGM_OK;
}
// back to the caller: the `len` rows of every column only (what lies between a column's last row and ld is never written)
static int stage_block_out(const StagedBlock &s, double *v, int64_t ld, int64_t len, int k, int where)
{
    if (!s.owned) return SGM_OK;
    if (len)
        for (int j = 0; j < k; ++j)
            SGM_HIP(hipMemcpyAsync(v + j * ld, s.dev + j * s.ld, (size_t)len * 8,
                                   where == SGM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, g_rt.stream));
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    return SGM_OK;
}

// one existing product on device vectors, stream-ordered
static int mm_single(sgm_mat A, bool add, bool trans, const double *x, double *y, int where = SGM_DEVICE, bool async = true)
{
    const bool was_async = g_rt.async;
    if (async) g_rt.async = true;
    const int rc = trans ? (add ? sgm_mat_matvec_t_add(A, x, y, where) : sgm_mat_matvec_t(A, x, y, where))
                         : (add ? sgm_mat_matvec_add(A, x, y, where) : sgm_mat_matvec(A, x, y, where));
    g_rt.async = was_async;
    return rc;
}

static int mm_check(const char *fn, sgm_mat A, int32_t op, int32_t k)
{
    SGM_TRY(require_init());
    if (!A) return fail(SGM_ERR_BAD_ARG, "%s: null matrix", fn);
    if (k < 0) return fail(SGM_ERR_BAD_ARG, "%s: k = %d is negative", fn, k);
    if (op & ~(SGM_OP_ADD | SGM_OP_TRANS)) return fail(SGM_ERR_BAD_ARG, "%s: op = %d holds bits other than SGM_OP_ADD | SGM_OP_TRANS", fn, op);
    if (A->comm) return fail(SGM_ERR_UNSUPPORTED, "%s: not available on a matrix distributed over a communicator", fn);
    if (A->parts.size() > 1) return fail(SGM_ERR_UNSUPPORTED, "%s: not available on an in-process row partition", fn);
    if (A->fmt != SGM_FMT_CSR && A->fmt != SGM_FMT_ELL && A->fmt != SGM_FMT_COMPOSITE) return fail(SGM_ERR_UNSUPPORTED, "%s: unknown matrix format", fn);
    if (A->fmt == SGM_FMT_COMPOSITE)
        for (const sgm_mat_s *C : A->blocks)
            if (C && C->comm) return fail(SGM_ERR_UNSUPPORTED, "%s: not available on a composite of distributed leaves", fn);
    return SGM_OK;
}

static int matmat_impl(const char *fn, sgm_mat A, int32_t op, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                       int32_t block_cap, int32_t grid_cap, int where)
{
    SGM_TRY(mm_check(fn, A, op, k));
    if (k == 0) return SGM_OK;
    const bool add = (op & SGM_OP_ADD) != 0, trans = (op & SGM_OP_TRANS) != 0;
    const int64_t xlen = trans ? A->nrow : A->ncol, ylen = trans ? A->ncol : A->nrow;
    if (!X || !Y) return fail(SGM_ERR_BAD_ARG, "%s: null block", fn);
    if (ldx < xlen) return fail(SGM_ERR_BAD_ARG, "%s: ldx = %lld is shorter than a column of X (%lld entries)", fn, (long long)ldx, (long long)xlen);
    if (ldy < ylen) return fail(SGM_ERR_BAD_ARG, "%s: ldy = %lld is shorter than a column of Y (%lld entries)", fn, (long long)ldy, (long long)ylen);
    {
        const uintptr_t x0 = reinterpret_cast<uintptr_t>(X), x1 = x0 + (size_t)((int64_t)(k - 1) * ldx + xlen) * 8;
        const uintptr_t y0 = reinterpret_cast<uintptr_t>(Y), y1 = y0 + (size_t)((int64_t)(k - 1) * ldy + ylen) * 8;
        if (x0 < y1 && y0 < x1) return fail(SGM_ERR_BAD_ARG, "%s: the address ranges of X and Y overlap", fn);
    }
    if (k == 1) return mm_single(A, add, trans, X, Y, where, false);      // the existing single-vector call, as it is

    sgm_mat_s *M = A;
    if (trans && A->fmt != SGM_FMT_COMPOSITE) {
        SGM_TRY(ensure_transpose(A));
        M = A->T;
    }
    const int form = (block_cap == 1 || A->fmt == SGM_FMT_COMPOSITE) ? MM_COLUMNS : mm_form(M);
    StagedBlock sx, sy;
    SGM_TRY(stage_block_in(sx, X, ldx, xlen, k, where, true));
    SGM_TRY(stage_block_in(sy, Y, ldy, ylen, k, where, add));
    std::vector<int> blocks;
    mm_blocks(form, k, block_cap, blocks);
    const Part &p = M->parts[0];
    const int grid = form != MM_COLUMNS ? mm_grid(M, grid_cap) : 0;
    const int remap = form != MM_COLUMNS ? (slice_map_mode(grid, p.n) | (trans && add ? kChainBit : 0)) : 0;
    int j = 0;
    for (int w : blocks) {
        const double *xj = sx.dev + (int64_t)j * sx.ld;
        double *yj = sy.dev + (int64_t)j * sy.ld;
        if (w == 1) SGM_TRY(mm_single(A, add, trans, xj, yj));
        else if (p.n > 0 && !mm_launch(form, w, add, p, grid, remap, xj, sx.ld, yj, sy.ld))
            return fail(SGM_ERR_UNSUPPORTED, "%s: no %s kernel for W = %d, KB = %d", fn, kMmName[form], p.sw, w);    // (a missing kernel is an error)
        j += w;
    }
    SGM_HIP(hipGetLastError());
    SGM_TRY(stage_block_out(sy, Y, ldy, ylen, k, where));
    return finish();
}

}  // namespace sgm

using namespace sgm;

extern "C" {

int sgm_mat_matmat(sgm_mat A, int32_t op, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy, int where)
{
    return matmat_impl("sgm_mat_matmat", A, op, k, X, ldx, Y, ldy, 0, 0, where);
}

int sgm_mat_matmat_probe(sgm_mat A, int32_t op, int32_t k, const double *X, int64_t ldx, double *Y, int64_t ldy,
                         int32_t block_cap, int32_t grid_cap, int where)
{
    if (block_cap < 0 || grid_cap < 0) return fail(SGM_ERR_BAD_ARG, "sgm_mat_matmat_probe: negative cap");
    return matmat_impl("sgm_mat_matmat_probe", A, op, k, X, ldx, Y, ldy, block_cap, grid_cap, where);
}

int sgm_mat_matmat_kernel(sgm_mat A, int32_t op, int32_t k, char *buf, int len)
{
    const char *fn = "sgm_mat_matmat_kernel";
    SGM_TRY(mm_check(fn, A, op, k));
    if (!buf || len < 1) return fail(SGM_ERR_BAD_ARG, "%s: bad buffer", fn);
    const bool trans = (op & SGM_OP_TRANS) != 0;
    sgm_mat_s *M = A;
    if (trans && A->fmt != SGM_FMT_COMPOSITE) {
        SGM_TRY(ensure_transpose(A));
        M = A->T;
    }
    char one[64];
    if (A->fmt == SGM_FMT_COMPOSITE) snprintf(one, sizeof one, "composite");
    else part_kernel_name(M->parts[0], M->fmt, one, sizeof one);
    const int form = A->fmt == SGM_FMT_COMPOSITE ? MM_COLUMNS : mm_form(M);
    std::string s;
    if (form == MM_COLUMNS) s = std::string("columns: ") + one;
    else {
        std::vector<int> blocks;
        mm_blocks(form, k, 0, blocks);
        for (size_t i = 0; i < blocks.size();) {
            size_t e = i;
            while (e < blocks.size() && blocks[e] == blocks[i]) ++e;
            char item[128];
            if (blocks[i] == 1) snprintf(item, sizeof item, "%s x%d", one, (int)(e - i));
            else snprintf(item, sizeof item, "%s<W=%d,KB=%d> x%d", kMmName[form], M->parts[0].sw, blocks[i], (int)(e - i));
            if (!s.empty()) s += " + ";
            s += item;
            i = e;
        }
    }
    snprintf(buf, (size_t)len, "%s", s.c_str());
    return SGM_OK;
}

}  // extern "C"
