// Multigrid preconditioner: one V-cycle on Galerkin levels, damped Jacobi sweeps.
//
// Levels l = 0 .. L, A_0 = the caller's A, A_{l+1} = P_l^T A_l P_l built by sgm_mat_ptap (owned here, refilled by
// sgm_mat_algebra_refill when only values changed), idiag_l(i) = 1.0 / a_ii by the Jacobi setup's rule (the last stored
// copy of the diagonal, 0.0 when absent).  z = M^-1 r is vcycle(0, r):
//   first sweep (from the zero start)   x(i) = omega * (idiag(i) * b(i))
//   every further sweep, out of place   q = A_l x ; t(i) = b(i) - q(i) ; x'(i) = x(i) + omega * (idiag(i) * t(i))
//   l == L                              coarse_sweeps sweeps -- or, with option "mg_coarse_direct", x = Ainv b with the dense
//                                       inverse of A_L made at setup (sgm_mg_direct.hip)
//   otherwise                           nu_pre sweeps ; r = b - A_l x ; b_c = P_l^T r (the transposed product's order) ;
//                                       x_c = vcycle(l + 1, b_c) ; x = x + (0.0 + P_l x_c) ; nu_post sweeps
// Every operation is rounded on its own (-ffp-contract=off); a row sum is the library's matvec sum: +0.0 plus the
// individually rounded products in stored order.
//
// Hot path: a level whose matrix holds the 4-bit sliced form (k_csr_sl's: sval / scode / dict) or the 1-byte sliced form
// (k_csr_slb's: sval / sbcode / dict; widths 9 and 27) runs a sweep -- or the residual -- as ONE kernel: the row sum formed by the functions
// k_csr_sl / k_csr_slb form it with (sl_row_sums / slb_row_sums, sgm_spmv_device.hpp; two adjacent rows per lane), then the epilogue on the
// lane's own rows.  Against product + elementwise pass that saves q's write and read (16 bytes per row) and a launch.  Any
// other layout runs the composition: spmv_parts into a scratch q, then one k_elem functor.  Same operations on the same
// operands in the same order: the same bits.
#include "sgm_spmv_device.hpp"
#include "sgm_krylov.hpp"
#include "sgm_pc_internal.hpp"

#include <chrono>

namespace sgm {

struct MgLevel {
    sgm_mat A = nullptr;           // level 0: the caller's (borrowed); l > 0: P^T A P of the level above (owned)
    int32_t n = 0;
    double *idiag = nullptr;
    double *x0 = nullptr, *x1 = nullptr;     // the two x buffers of the out-of-place sweeps
    double *b = nullptr, *r = nullptr;       // right-hand side and residual of the level
    double *q = nullptr;                     // A x of the unfused composition
};

struct MgState {
    std::vector<sgm_mat> P;        // P_0 .. P_{L-1}, borrowed
    double omega = 2.0 / 3.0;
    int32_t nu_pre = 1, nu_post = 1, coarse = 8;
    std::vector<MgLevel> lev;
    bool ready = false;
    uint64_t a_serial = 0, a_pattern = 0;    // the matrix the levels were built for
    std::vector<uint64_t> p_pattern;
    double setup_ms = 0.0;
    bool refilled = false;
    std::vector<int32_t> hpaths;   // sgm_pc_get staging
    std::vector<double> hidiag;
    int direct_opt = 0;            // option "mg_coarse_direct": read at setup
    MgDirect *direct = nullptr;    // the inverse of the coarsest level when the last setup ran with the option (else null)
};

// ------------------------------------------------------------------ kernels
// the Jacobi setup's rule (k_jacobi_setup_csr): the LAST stored copy of the diagonal, 0.0 when absent
__global__ void k_mg_idiag(int32_t n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                           const double *__restrict__ val, double *__restrict__ idiag)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double z = 0.0;
    for (int32_t k = rowptr[i]; k < rowptr[i + 1]; ++k)
        if (col[k] == i) z = val[k];
    idiag[i] = 1.0 / z;
}

// x = omega * (idiag * b): the sweep from the zero start
struct FMgFirst {
    static constexpr bool kDot = false;
    const double *b, *idiag; double *x; double omega;
    __device__ bool prepare(double *) { return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 bb = ld2<NT>(b, i), dd = ld2<NT>(idiag, i);
        double2 xx; xx.x = omega * (dd.x * bb.x); xx.y = omega * (dd.y * bb.y);
        st2<NT>(x, i, xx);
    }
    __device__ void single(int64_t i) { x[i] = omega * (idiag[i] * b[i]); }
    __device__ void finish(double *) {}
};
// t = b - q ; x' = x + omega * (idiag * t)   (q = A x from the product before it)
struct FMgSmooth {
    static constexpr bool kDot = false;
    const double *b, *q, *idiag, *xo; double *xn; double omega;
    __device__ bool prepare(double *) { return true; }
    __device__ static double one(double bv, double qv, double dv, double xv, double om)
    {
        const double t = bv - qv;
        return xv + om * (dv * t);
    }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 bb = ld2<NT>(b, i), qq = ld2<NT>(q, i), dd = ld2<NT>(idiag, i), xx = ld2<NT>(xo, i);
        double2 o; o.x = one(bb.x, qq.x, dd.x, xx.x, omega); o.y = one(bb.y, qq.y, dd.y, xx.y, omega);
        st2<NT>(xn, i, o);
    }
    __device__ void single(int64_t i) { xn[i] = one(b[i], q[i], idiag[i], xo[i], omega); }
    __device__ void finish(double *) {}
};
// r = b - q
struct FMgResid {
    static constexpr bool kDot = false;
    const double *b, *q; double *r;
    __device__ bool prepare(double *) { return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 bb = ld2<NT>(b, i), qq = ld2<NT>(q, i);
        double2 o; o.x = bb.x - qq.x; o.y = bb.y - qq.y;
        st2<NT>(r, i, o);
    }
    __device__ void single(int64_t i) { r[i] = b[i] - q[i]; }
    __device__ void finish(double *) {}
};

enum { MG_SMOOTH = 0, MG_RESID = 1 };

// the own-row operands of a lane (rows row, row + 1 of b, idiag, x) and the epilogue on them
struct MgOwn { f64x2 b, d, x; };
template <int MODE>
__device__ inline MgOwn mg_load_own(int32_t row, int32_t n, const double *__restrict__ b, const double *__restrict__ idiag,
                                    const double *__restrict__ x)
{
    MgOwn o;
    o.b = f64x2{0.0, 0.0}; o.d = f64x2{0.0, 0.0}; o.x = f64x2{0.0, 0.0};
    if (row + 1 < n) {
        o.b = *reinterpret_cast<const f64x2 *>(b + row);
        if (MODE == MG_SMOOTH) { o.d = *reinterpret_cast<const f64x2 *>(idiag + row); o.x = *reinterpret_cast<const f64x2 *>(x + row); }
    } else if (row < n) {
        o.b.x = b[row];
        if (MODE == MG_SMOOTH) { o.d.x = idiag[row]; o.x.x = x[row]; }
    }
    return o;
}
template <int MODE>
__device__ inline void mg_store_own(int32_t row, int32_t n, const MgOwn &o, f64x2 z, double omega, double *__restrict__ out)
{
    f64x2 q, t, res;
    q.x = 0.0 + z.x; q.y = 0.0 + z.y;                 // the product's y = 0.0 + sum
    t.x = o.b.x - q.x; t.y = o.b.y - q.y;
    if (MODE == MG_SMOOTH) { res.x = o.x.x + omega * (o.d.x * t.x); res.y = o.x.y + omega * (o.d.y * t.y); }
    else res = t;
    if (row + 1 < n) *reinterpret_cast<f64x2 *>(out + row) = res;
    else if (row < n) out[row] = res.x;
}

// 4-bit sliced form (k_csr_sl's layout and row sum), W = 3, 5, 7, 8
template <int W, int MODE>
__global__ __launch_bounds__(256) void k_mg_sl(int32_t n, const uint32_t *__restrict__ scode, const int32_t *__restrict__ dict,
                                               const double *__restrict__ sval, const double *__restrict__ x,
                                               const double *__restrict__ b, const double *__restrict__ idiag, double omega,
                                               double *__restrict__ out, const int *__restrict__ flag, int remap)
{
    constexpr int BLOCK = 256;
    __shared__ int32_t dl[16];
    // flag, dictionary, the first slice's codes / values and the lane's own rows are all requested before any is waited for
    const int st = stop_flag(flag);
    const int tid = threadIdx.x;
    const int32_t dv = tid < 16 ? dict[tid] : 0;
    const int64_t nsl = ((int64_t)n + kSlRows - 1) / kSlRows;
    int64_t sl = first_slice(remap);
    u32x2 cw = {0xffffffffu, 0xffffffffu};
    f64x2 v[W];
    MgOwn own;
    auto load_slice = [&](int64_t s_) {
        const int32_t row_ = (int32_t)(s_ * kSlRows) + 2 * tid;
        cw = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(scode + row_));
        const f64x2 *vb = reinterpret_cast<const f64x2 *>(sval + s_ * (int64_t)(W * kSlRows)) + tid;
#pragma unroll
        for (int u = 0; u < W; ++u) v[u] = __builtin_nontemporal_load(vb + u * BLOCK);
        own = mg_load_own<MODE>(row_, n, b, idiag, x);
    };
    bool have = sl < nsl;
    if (have) load_slice(sl);
    if (st) return;                                   // (generation INT_MAX: any nonzero flag stops the apply)
    if (tid < 16) dl[tid] = dv;
    __syncthreads();
    while (have) {
        const int64_t nxt = sl + gridDim.x;
        const int32_t row = (int32_t)(sl * kSlRows) + 2 * tid;
        const f64x2 z = sl_row_sums<W>(f64x2{0.0, 0.0}, cw, v, x, row, dl);
        mg_store_own<MODE>(row, n, own, z, omega, out);
        sl = nxt;
        have = sl < nsl;
        if (have) load_slice(sl);
    }
}

// 1-byte sliced form (k_csr_slb's layout and row sum).  Instantiated for the widths the Galerkin levels of 5- / 7-point
// stencils take (9- and 27-point rows); a level with another width of SGM_SLB_WIDTHS -- rows of general matrices, as uneven
// as the padding rule lets them be -- runs the composition
#define SGM_MG_SLB_WIDTHS(X) X(9) X(27)
template <int W, int MODE>
__global__ __launch_bounds__(256) void k_mg_slb(int32_t n, const uint8_t *__restrict__ sbcode, const int32_t *__restrict__ dict,
                                                const double *__restrict__ sval, const double *__restrict__ x,
                                                const double *__restrict__ b, const double *__restrict__ idiag, double omega,
                                                double *__restrict__ out, const int *__restrict__ flag, int remap)
{
    static_assert(W >= 9 && W <= 32, "rows of 9..32 entries");
    __shared__ int32_t dl[256];
    const int st = stop_flag(flag);
    const int tid = threadIdx.x;
    const int32_t dv = dict[tid];
    const int64_t nsl = ((int64_t)n + kSlRows - 1) / kSlRows;
    int64_t sl = first_slice(remap);
    // the first slice's own rows travel with the flag and the dictionary
    MgOwn own;
    if (sl < nsl) own = mg_load_own<MODE>((int32_t)(sl * kSlRows) + 2 * tid, n, b, idiag, x);
    if (st) return;
    dl[tid] = dv;
    __syncthreads();
    while (sl < nsl) {
        const int64_t nxt = sl + gridDim.x;
        const int32_t row = (int32_t)(sl * kSlRows) + 2 * tid;
        const f64x2 z = slb_row_sums<W>(f64x2{0.0, 0.0}, sval, sbcode, sl, tid, x, row, dl);
        mg_store_own<MODE>(row, n, own, z, omega, out);
        sl = nxt;
        if (sl < nsl) own = mg_load_own<MODE>((int32_t)(sl * kSlRows) + 2 * tid, n, b, idiag, x);
    }
}

// ------------------------------------------------------------------ launchers
// 1 = the 4-bit sliced form serves this part, 2 = the 1-byte sliced form, 0 = the unfused composition (what spmv_parts
// would launch decides: the column-blocked form goes first there, then k_csr_sl, then k_csr_slb)
static int mg_path(const Part &p)
{
#ifdef SGM_MG_UNFUSED
    return 0;                                          // measurement builds: the composition everywhere (tools/mg_bench.py)
#endif
    if (p.n_halo != 0 || use_ell_colblock(p) || !p.sval || !p.dict) return 0;
    if (use_sliced(p)) {
#define LV(WW) if (p.sw == WW) return 1;
        SGM_SL_WIDTHS(LV)
#undef LV
        return 0;
    }
    if (use_slicedb(p)) {
#define LV(WW) if (p.sw == WW) return 2;
        SGM_MG_SLB_WIDTHS(LV)
#undef LV
    }
    return 0;
}

template <int MODE>
static void launch_fused(const Part &p, int path, const double *x, const double *b, const double *idiag, double omega,
                         double *out, const int *flag)
{
    const int grid = grid_for_rows(p, p.n > 0 ? p.n : 1, kMaxGrid, false);
    const int remap = slice_map_mode(grid, p.n);
    hipStream_t st = g_rt.stream;
    if (path == 1) {
#define LV(WW)                                                                                                          \
    if (p.sw == WW) {                                                                                                   \
        hipLaunchKernelGGL((k_mg_sl<WW, MODE>), dim3(grid), dim3(256), 0, st, p.n, (const uint32_t *)p.scode,           \
                           (const int32_t *)p.dict, (const double *)p.sval, x, b, idiag, omega, out, flag, remap);      \
        return;                                                                                                         \
    }
        SGM_SL_WIDTHS(LV)
#undef LV
    } else {
#define LV(WW)                                                                                                          \
    if (p.sw == WW) {                                                                                                   \
        hipLaunchKernelGGL((k_mg_slb<WW, MODE>), dim3(grid), dim3(256), 0, st, p.n, (const uint8_t *)p.sbcode,          \
                           (const int32_t *)p.dict, (const double *)p.sval, x, b, idiag, omega, out, flag, remap);      \
        return;                                                                                                         \
    }
        SGM_MG_SLB_WIDTHS(LV)
#undef LV
    }
}

// x' = sweep(x) (MG_SMOOTH) or out = b - A x (MG_RESID) on level Lv
template <int MODE>
static int level_pass(const MgLevel &Lv, const double *b, const double *x, double *out, double omega, const int *flag)
{
    if (Lv.n == 0) return SGM_OK;
    const Part &p = Lv.A->parts[0];
    if (const int path = mg_path(p)) {
        launch_fused<MODE>(p, path, x, b, Lv.idiag, omega, out, flag);
        SGM_HIP(hipGetLastError());
        return SGM_OK;
    }
    const double *xs[1] = {x};
    double *qs[1] = {Lv.q};
    SGM_TRY(spmv_parts(Lv.A, xs, qs, false, nullptr, flag, nullptr));
    if (MODE == MG_SMOOTH) launch_elem(Lv.n, FMgSmooth{b, Lv.q, Lv.idiag, x, out, omega}, flag);
    else launch_elem(Lv.n, FMgResid{b, Lv.q, out}, flag);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

// vcycle(l, b): the sweeps alternate between `first` and `second`; *res = the buffer that holds x at the end
static int vcycle(MgState *S, int l, const double *b, double *first, double *second, const int *flag, double **res)
{
    const int L = (int)S->lev.size() - 1;
    const MgLevel &Lv = S->lev[(size_t)l];
    double *cur = first, *other = second;
    if (l == L && S->direct) {                          // x = Ainv b in place of the coarse sweeps
        SGM_TRY(mg_direct_apply(S->direct, b, first, flag));
        *res = first;
        return SGM_OK;
    }
    if (Lv.n) launch_elem(Lv.n, FMgFirst{b, Lv.idiag, cur, S->omega}, flag);
    const int sweeps = l == L ? S->coarse : S->nu_pre;
    for (int s = 1; s < sweeps; ++s) {
        SGM_TRY(level_pass<MG_SMOOTH>(Lv, b, cur, other, S->omega, flag));
        std::swap(cur, other);
    }
    if (l < L) {
        MgLevel &Lc = S->lev[(size_t)l + 1];
        sgm_mat P = S->P[(size_t)l];
        SGM_TRY(level_pass<MG_RESID>(Lv, b, cur, Lv.r, S->omega, flag));
        {   // b_c = P^T r: a row sum over P^T in the scatter's order (ensure_transpose at setup)
            const double *xs[1] = {Lv.r};
            double *ys[1] = {Lc.b};
            SGM_TRY(spmv_parts(P->T, xs, ys, false, nullptr, flag, nullptr));
        }
        double *xc = nullptr;
        SGM_TRY(vcycle(S, l + 1, Lc.b, Lc.x0, Lc.x1, flag, &xc));
        {   // x = x + (0.0 + P x_c)
            const double *xs[1] = {xc};
            double *ys[1] = {cur};
            SGM_TRY(spmv_parts(P, xs, ys, true, nullptr, flag, nullptr));
        }
        for (int s = 0; s < S->nu_post; ++s) {
            SGM_TRY(level_pass<MG_SMOOTH>(Lv, b, cur, other, S->omega, flag));
            std::swap(cur, other);
        }
    }
    SGM_HIP(hipGetLastError());
    *res = cur;
    return SGM_OK;
}

// ------------------------------------------------------------------ hooks of the pc functions (sgm_internal.hpp)
static void free_level_buffers(MgLevel &Lv)
{
    dfree(Lv.idiag); dfree(Lv.x0); dfree(Lv.x1); dfree(Lv.b); dfree(Lv.r); dfree(Lv.q);
    Lv.idiag = Lv.x0 = Lv.x1 = Lv.b = Lv.r = Lv.q = nullptr;
}
static void free_levels(MgState *S)
{
    for (size_t l = 0; l < S->lev.size(); ++l) {
        free_level_buffers(S->lev[l]);
        if (l > 0 && S->lev[l].A) sgm_mat_destroy(S->lev[l].A);
    }
    S->lev.clear();
    mg_direct_free(S->direct);
    S->direct = nullptr;
    S->ready = false;
}
void mg_free(MgState *S)
{
    if (!S) return;
    free_levels(S);
    delete S;
}

static int check_leaf(sgm_mat M, const char *what, int level)
{
    if (!M) return fail(SGM_ERR_BAD_ARG, "multigrid: null %s at level %d", what, level);
    if (M->fmt == SGM_FMT_COMPOSITE)
        return fail(SGM_ERR_UNSUPPORTED, "multigrid: %s at level %d is a composite matrix (single-GPU CSR leaves only)", what, level);
    if (M->distributed())
        return fail(SGM_ERR_UNSUPPORTED, "multigrid: %s at level %d is distributed / partitioned (single-GPU CSR leaves only)", what, level);
    if (M->fmt != SGM_FMT_CSR)
        return fail(SGM_ERR_UNSUPPORTED, "multigrid: %s at level %d is not CSR (ELLPACK operands are not supported)", what, level);
    return SGM_OK;
}

static int level_idiag(MgLevel &Lv)
{
    if (Lv.n == 0) return SGM_OK;
    const Part &p = Lv.A->parts[0];
    SGM_TRY(csr_need_arrays(p));
    hipLaunchKernelGGL(k_mg_idiag, dim3((unsigned)((Lv.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, g_rt.stream, Lv.n,
                       (const int32_t *)p.rowptr, (const int32_t *)p.col, (const double *)p.val, Lv.idiag);
    const hipError_t e = hipGetLastError();
    csr_release_arrays(p);
    if (e != hipSuccess) return fail(SGM_ERR_HIP, "multigrid: inverse diagonal: %s", hipGetErrorString(e));
    return SGM_OK;
}

int mg_setup(MgState *S, sgm_mat A)
{
    const auto t0 = std::chrono::steady_clock::now();
    const size_t L = S->P.size();
    S->refilled = false;
    // a failed setup leaves nothing to apply
    struct Fail { MgState *S; bool armed = true; ~Fail() { if (armed) free_levels(S); } } guard{S};
    SGM_TRY(check_leaf(A, "A", 0));
    for (size_t l = 0; l < L; ++l) SGM_TRY(check_leaf(S->P[l], "P", (int)l));
    if (A->nrow != A->ncol) return fail(SGM_ERR_DIMS, "multigrid: A is not square (%d x %d)", A->nrow, A->ncol);
    for (size_t l = 0; l < L; ++l) {
        const int32_t want = l == 0 ? A->nrow : S->P[l - 1]->ncol;
        if (S->P[l]->nrow != want)
            return fail(SGM_ERR_DIMS, "multigrid: P at level %zu has %d rows, level %zu has %d", l, S->P[l]->nrow, l, want);
    }
    bool same = S->lev.size() == L + 1 && S->a_serial == A->serial && S->a_pattern == A->pattern_version;
    for (size_t l = 0; same && l < L; ++l) same = S->p_pattern[l] == S->P[l]->pattern_version;
    if (same) {
        // values only: the owned levels are refilled through their symbolic plans, top down
        for (size_t l = 0; l < L; ++l) {
            SGM_TRY(ensure_transpose(S->P[l]));
            SGM_TRY(sgm_mat_algebra_refill(S->lev[l + 1].A, S->lev[l].A, S->P[l]));
        }
        S->refilled = true;
    } else {
        free_levels(S);
        S->lev.resize(L + 1);
        S->lev[0].A = A;
        for (size_t l = 0; l < L; ++l) {
            SGM_TRY(sgm_mat_ptap(&S->lev[l + 1].A, S->lev[l].A, S->P[l]));
            SGM_TRY(ensure_transpose(S->P[l]));
        }
        for (auto &Lv : S->lev) {
            Lv.n = Lv.A->nrow;
            const size_t m = (size_t)Lv.n + 2;
            SGM_TRY(dalloc(&Lv.idiag, m)); SGM_TRY(dalloc(&Lv.x0, m)); SGM_TRY(dalloc(&Lv.x1, m));
            SGM_TRY(dalloc(&Lv.b, m)); SGM_TRY(dalloc(&Lv.r, m)); SGM_TRY(dalloc(&Lv.q, m));
        }
        S->a_serial = A->serial;
        S->a_pattern = A->pattern_version;
        S->p_pattern.resize(L);
        for (size_t l = 0; l < L; ++l) S->p_pattern[l] = S->P[l]->pattern_version;
    }
    for (auto &Lv : S->lev) SGM_TRY(level_idiag(Lv));
    mg_direct_free(S->direct);
    S->direct = nullptr;
    if (S->direct_opt) SGM_TRY(mg_direct_setup(&S->direct, S->lev[L].A));
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    S->setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    S->ready = true;
    guard.armed = false;
    if (trace_on()) {
        int32_t o[4]; double us = 0.0; char nm[160];
        mg_info(S, o, &us, nm, sizeof nm);
        fprintf(stderr, "[sigma_hip] multigrid setup (%s, %.2f ms): %s, about %.0f us per apply\n", S->refilled ? "refill" : "build",
                S->setup_ms, nm, us);
        if (S->direct) fprintf(stderr, "[sigma_hip] multigrid coarse inversion: %d rows, %.2f ms\n", mg_direct_rows(S->direct), mg_direct_invert_ms(S->direct));
    }
    return SGM_OK;
}

// z = M^-1 r on device vectors, stream-ordered.  Level 0 sweeps between z and its second x buffer, started so that the last
// sweep lands in z; r is read until the last sweep, so an in-place apply (r == z) works on a copy of r.
int mg_apply(MgState *S, const double *r, double *z, const int *flag)
{
    if (!S || !S->ready) return fail(SGM_ERR_BAD_ARG, "multigrid: the preconditioner has not been set up (or its last setup failed)");
    MgLevel &L0 = S->lev[0];
    if (L0.n == 0) return SGM_OK;
    const bool coarse_only = S->lev.size() == 1;
    const int swaps = coarse_only ? (S->direct ? 0 : S->coarse - 1) : S->nu_pre - 1 + S->nu_post;
    const double *b = r;
    if (r == z) {
        SGM_HIP(hipMemcpyAsync(L0.b, r, (size_t)L0.n * 8, hipMemcpyDeviceToDevice, g_rt.stream));
        b = L0.b;
    }
    double *first = swaps % 2 == 0 ? z : L0.x1, *second = swaps % 2 == 0 ? L0.x1 : z;
    double *res = nullptr;
    SGM_TRY(vcycle(S, 0, b, first, second, flag, &res));
    if (res != z) return fail(SGM_ERR_HIP, "multigrid: the level-0 sweeps did not end in z");
    return SGM_OK;
}

int mg_apply_vectors(MgState *S, const double *r, double *z, int where)
{
    if (!S || !S->ready) return fail(SGM_ERR_BAD_ARG, "multigrid: the preconditioner has not been set up (or its last setup failed)");
    const int64_t n = S->lev[0].n;
    Staged sr, sz;
    SGM_TRY(stage_in(sr, r, n, where, true));
    SGM_TRY(stage_in(sz, z, n, where, false));
    SGM_TRY(mg_apply(S, sr.dev, sz.dev, nullptr));
    SGM_TRY(stage_out(sz, z, n, where));
    return finish();
}

int mg_get(MgState *S, const char *name, const void **src, size_t *sz)
{
    const std::string nm(name);
    if (!S->ready) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: the multigrid preconditioner has not been set up");
    if (nm == "mg_paths") {
        S->hpaths.resize(S->lev.size());
        for (size_t l = 0; l < S->lev.size(); ++l) S->hpaths[l] = S->lev[l].n ? mg_path(S->lev[l].A->parts[0]) : 0;
        *src = S->hpaths.data(); *sz = S->hpaths.size() * 4;
        return SGM_OK;
    }
    if (nm == "mg_coarse_invert_ms") {                  // host clock around the last inversion, its final synchronisation included
        if (!S->direct) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: '%s' needs option mg_coarse_direct at the last setup", name);
        S->hidiag.assign(1, mg_direct_invert_ms(S->direct));
        *src = S->hidiag.data(); *sz = 8;
        return SGM_OK;
    }
    if (nm == "mg_coarse_inverse" || nm == "mg_coarse_pivots") {
        if (!S->direct) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: '%s' needs option mg_coarse_direct at the last setup", name);
        return mg_direct_get(S->direct, name, src, sz);
    }
    if (nm.rfind("mg_idiag_", 0) == 0 && nm.size() > 9 && nm.find_first_not_of("0123456789", 9) == std::string::npos && nm.size() < 19) {
        const long l = atol(nm.c_str() + 9);
        if (l >= (long)S->lev.size()) return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: '%s': the hierarchy has %zu levels", name, S->lev.size());
        const MgLevel &Lv = S->lev[(size_t)l];
        S->hidiag.assign((size_t)Lv.n, 0.0);
        SGM_HIP(hipStreamSynchronize(g_rt.stream));
        if (Lv.n) SGM_HIP(hipMemcpy(S->hidiag.data(), Lv.idiag, (size_t)Lv.n * 8, hipMemcpyDeviceToHost));
        *src = S->hidiag.data(); *sz = S->hidiag.size() * 8;
        return SGM_OK;
    }
    return fail(SGM_ERR_BAD_ARG, "sgm_pc_get: unknown array '%s'", name);
}

// out4 = {levels, levels, 5 (V-cycle), 0}; est_us from the bytes an apply moves (a fused pass: the product's bytes + the
// own-row operands; the composition 16 bytes per row more) at the streaming rate the other kinds use, plus its launches
int mg_info(MgState *S, int32_t out4[4], double *est_us, char *nm, size_t len)
{
    if (!S->ready) return fail(SGM_ERR_BAD_ARG, "sgm_pc_info: set the preconditioner up first");
    const int nl = (int)S->lev.size();
    double bytes = 0.0, launches = 0.0;
    for (int l = 0; l < nl; ++l) {
        const MgLevel &Lv = S->lev[(size_t)l];
        int64_t mv = 0;
        (void)sgm_mat_footprint(Lv.A, nullptr, &mv);
        const bool fused = Lv.n && mg_path(Lv.A->parts[0]);
        if (l == nl - 1 && S->direct) {                                            // one dense product
            bytes += 8.0 * Lv.n * Lv.n + 16.0 * Lv.n;
            launches += 1;
            continue;
        }
        const int passes = l == nl - 1 ? S->coarse - 1 : S->nu_pre - 1 + S->nu_post;
        bytes += 24.0 * Lv.n;                                                      // the sweep from the zero start
        bytes += passes * ((double)mv + (fused ? 16.0 : 40.0) * Lv.n);             // b, idiag (+ q written and read, x read again)
        launches += 1 + passes * (fused ? 1 : 2);
        if (l < nl - 1) {
            int64_t mp = 0, mt = 0;
            (void)sgm_mat_footprint(S->P[(size_t)l], nullptr, &mp);
            if (S->P[(size_t)l]->T) (void)sgm_mat_footprint(S->P[(size_t)l]->T, nullptr, &mt); else mt = mp;
            bytes += (double)mv + (fused ? 0.0 : 24.0) * Lv.n + (double)mp + 8.0 * Lv.n + (double)mt;
            launches += (fused ? 1 : 2) + 2;
        }
    }
    if (out4) { out4[0] = nl; out4[1] = nl; out4[2] = 5; out4[3] = 0; }
    if (est_us) *est_us = bytes / 5.5e6 + 4.5 * launches;
    if (nm && len && S->direct)
        snprintf(nm, len, "V(%d,%d) omega %g, %d level%s, direct coarse solve (%d rows)", S->nu_pre, S->nu_post, S->omega, nl,
                 nl == 1 ? "" : "s", mg_direct_rows(S->direct));
    else if (nm && len) snprintf(nm, len, "V(%d,%d) omega %g, %d level%s, %d coarse sweep%s", S->nu_pre, S->nu_post, S->omega, nl,
                            nl == 1 ? "" : "s", S->coarse, S->coarse == 1 ? "" : "s");
    return SGM_OK;
}

int mg_set_option(MgState *S, const char *name, int value)
{
    if (!S || strcmp(name, "mg_coarse_direct")) return fail(SGM_ERR_BAD_ARG, "sgm_pc_set_option: '%s' is not a multigrid option", name);
    S->direct_opt = value != 0;
    return SGM_OK;
}

}  // namespace sgm

using namespace sgm;

extern "C" {

int sgm_mg_create(sgm_pc *out, int32_t ncoarse, const sgm_mat *P, double omega, int32_t nu_pre, int32_t nu_post, int32_t coarse_sweeps)
{
    SGM_TRY(require_init());
    if (!out) return fail(SGM_ERR_BAD_ARG, "sgm_mg_create: null out pointer");
    if (ncoarse < 0 || (ncoarse > 0 && !P)) return fail(SGM_ERR_BAD_ARG, "sgm_mg_create: ncoarse = %d needs that many prolongations", ncoarse);
    if (nu_pre < 1 || nu_post < 0 || coarse_sweeps < 1)
        return fail(SGM_ERR_BAD_ARG, "sgm_mg_create: nu_pre >= 1, nu_post >= 0, coarse_sweeps >= 1 (got %d, %d, %d)", nu_pre, nu_post, coarse_sweeps);
    if (!(omega == omega)) return fail(SGM_ERR_BAD_ARG, "sgm_mg_create: omega is not a number");
    for (int32_t l = 0; l < ncoarse; ++l)
        if (!P[l]) return fail(SGM_ERR_BAD_ARG, "sgm_mg_create: null prolongation at level %d", l);
    MgState *S = new MgState;
    S->P.assign(P, P + ncoarse);
    S->omega = omega;
    S->nu_pre = nu_pre; S->nu_post = nu_post; S->coarse = coarse_sweeps;
    *out = pc_adopt_mg(S);
    return SGM_OK;
}

int sgm_mg_level_matrix(sgm_pc pc, int32_t level, sgm_mat *borrowed)
{
    MgState *S = pc_mg(pc);
    if (!S || !borrowed) return fail(SGM_ERR_BAD_ARG, "sgm_mg_level_matrix: not a multigrid preconditioner / null output");
    if (!S->ready) return fail(SGM_ERR_BAD_ARG, "sgm_mg_level_matrix: set the preconditioner up first");
    if (level < 0 || (size_t)level >= S->lev.size())
        return fail(SGM_ERR_BAD_ARG, "sgm_mg_level_matrix: level %d of %zu", level, S->lev.size());
    *borrowed = S->lev[(size_t)level].A;
    return SGM_OK;
}

}  // extern "C"
