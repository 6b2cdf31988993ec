// Sparse matrix algebra on the device: A = B + C, A = B * C, B = P^T A P, B = R A R^T
// (src/matrix/sparse_matrix_algebra.f90:13; sparse_matrix_sum :25-145, sparse_matrix_product_C :310-420, PtAP :425-538,
// RARt :543-655) and the numeric-only refill of such a result.
//
// What the reference computes, per output row i: a fixed sequence of TERMS (column j, value z), the contribution order of
// its loops.  The row's pattern is an ll_graph fed by add_edge in that order (a repeated edge is ignored,
// ll_graphs.f90:355-370), so its columns appear in the order of their FIRST contribution; every value starts at +0.0 and
// each term is added with `val = val + z` (cs_matrices.f90:868-891) in sequence order.  A term is a product rounded on its
// own (-ffp-contract=off: no FMA).  The term sequences:
//   sum      B's row i in stored order, then C's row i
//   product  for (i,k) in B's row i: for (k,j) in C's row k: B_ik*C_kj
//   PtAP     for k ascending with P_ki stored: for (k,l) in A's row k: for every position of column i in P's row k:
//            for (l,j) in P's row l: (P_ki*A_kl)*P_lj   -- the k / n1 walk is row i of P^T (ensure_transpose: rows
//            sorted by (source row, slot)), and tperm maps it back to P's values
//   RARt     PtAP with P = R^T (R%get_column on CSR = R^T's rows, the same transpose)
//
// Symbolic pass: every output row's term count (exact: the sequence above), an exclusive scan -> term offsets.  Rows of at
// most kShortCap terms: one 64-lane workgroup per row, an LDS hash table keyed by column that keeps each column's smallest
// sequence number (atomicMin: duplicates inside one chunk resolve in lane order); a scan over the "first appearance" flags
// gives every column its rank.  Longer rows take the long-row path: their terms expanded to (row, column) keys, a stable
// radix sort (hipCUB), group heads = first appearances, a second sort of the heads by sequence = the ranks.  Both paths write
// the same plan: the output slot (rank inside the row) of every term.
// Numeric pass: one thread per output row walks the row's terms in sequence order and adds each into its slot -- the
// reference's order, no atomics, no tree.  The refill is this pass alone.
#include "sgm_spmv_select.hpp"

#include <climits>

namespace sgm {

enum { ALG_SUM = 0, ALG_PRODUCT = 1, ALG_PTAP = 2 };
constexpr int kShortCap = 256;          // terms of a row the LDS path takes
constexpr int kHash = 512;              // its table: load <= 1/2

struct CsrView { const int32_t *ptr = nullptr, *col = nullptr; const double *val = nullptr; };
struct AlgOp {
    CsrView X, Y;                        // sum: B, C; product: B, C; PtAP: A, P
    const int32_t *tptr = nullptr, *tcol = nullptr, *tpos = nullptr;     // PtAP: P^T's rows (0-based) and the P entry of each
};

struct AlgPlan {
    int op = 0;                          // SGM algebra operation (0 sum, 1 product, 2 PtAP, 3 RARt)
    uint64_t sx = 0, sy = 0;             // serials of the operands, in order
    uint64_t pvx = 0, pvy = 0, pvout = 0; // their pattern_version at creation, and the output's
    int32_t n = 0;                       // output rows
    int64_t nterms = 0;
    int64_t *toff = nullptr;             // n+1 term offsets
    int32_t *tslot = nullptr;            // rank inside its row of every term's column
    int32_t *optr = nullptr;             // n+1 output row pointers (0-based)
    double *val = nullptr;               // refill scratch (nnz)
    int64_t nnz = 0;
    int32_t rows_short = 0, rows_long = 0;
};
void alg_plan_free(AlgPlan *p)
{
    if (!p) return;
    dfree(p->toff); dfree(p->tslot); dfree(p->optr); dfree(p->val);
    delete p;
}

void alg_plan_rows(const AlgPlan *p, int32_t out[2]) { out[0] = p->rows_short; out[1] = p->rows_long; }

// ------------------------------------------------------------------ the term sequence of one output row
// f(col, val, lo, hi, m): the terms of entries lo..hi-1 of one operand row, in order; term value = val[e] (sum) or m*val[e]
template <int KIND, class F>
__device__ inline void walk_row(const AlgOp &op, int32_t i, F &&f)
{
    if (KIND == ALG_SUM) {
        f(op.X.col, op.X.val, op.X.ptr[i], op.X.ptr[i + 1], 0.0);
        f(op.Y.col, op.Y.val, op.Y.ptr[i], op.Y.ptr[i + 1], 0.0);
    } else if (KIND == ALG_PRODUCT) {
        for (int32_t e = op.X.ptr[i]; e < op.X.ptr[i + 1]; ++e) {
            const int32_t k = op.X.col[e];
            f(op.Y.col, op.Y.val, op.Y.ptr[k], op.Y.ptr[k + 1], op.X.val[e]);
        }
    } else {
        const int32_t end = op.tptr[i + 1];
        for (int32_t e = op.tptr[i]; e < end;) {
            const int32_t k = op.tcol[e];
            int32_t g = e + 1;
            while (g < end && op.tcol[g] == k) ++g;           // the positions of column i in P's row k
            for (int32_t a = op.X.ptr[k]; a < op.X.ptr[k + 1]; ++a) {
                const int32_t l = op.X.col[a];
                for (int32_t e2 = e; e2 < g; ++e2) {           // (the l loop is outside the duplicate loop)
                    const double m = op.Y.val[op.tpos[e2]] * op.X.val[a];
                    f(op.Y.col, op.Y.val, op.Y.ptr[l], op.Y.ptr[l + 1], m);
                }
            }
            e = g;
        }
    }
}

template <int KIND>
__global__ void k_alg_count(AlgOp op, int32_t n, int64_t *__restrict__ cnt)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    int64_t c = 0;
    if (i < n) walk_row<KIND>(op, i, [&](const int32_t *, const double *, int32_t lo, int32_t hi, double) { c += hi - lo; });
    cnt[i] = c;                          // cnt[n] = 0: the exclusive scan's total lands there
}

__device__ inline uint32_t alg_hash(int32_t c) { return ((uint32_t)c * 2654435761u) >> (32 - 9); }

// LDS path: one row per 64-lane workgroup (rows of <= kShortCap terms)
template <int KIND>
__global__ __launch_bounds__(64) void k_alg_sym_short(AlgOp op, int32_t n, const int64_t *__restrict__ toff,
                                                      int32_t *__restrict__ tslot, int32_t *__restrict__ ntmp,
                                                      int32_t *__restrict__ count)
{
    __shared__ int32_t hkey[kHash];
    __shared__ int32_t hval[kHash];      // smallest sequence number, then the column's rank
    __shared__ int32_t rank[kShortCap];  // first-appearance flags, then their exclusive prefix sum
    const int lane = threadIdx.x;
    for (int32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int64_t t0 = toff[i];
        const int32_t cnt = (int32_t)(toff[i + 1] - t0);
        if (cnt > kShortCap) continue;                  // the long-row path's
        for (int h = lane; h < kHash; h += 64) { hkey[h] = -1; hval[h] = INT_MAX; }
        for (int s = lane; s < kShortCap; s += 64) rank[s] = 0;
        __syncthreads();
        int32_t base = 0;
        walk_row<KIND>(op, i, [&](const int32_t *col, const double *, int32_t lo, int32_t hi, double) {
            for (int32_t e = lo + lane; e < hi; e += 64) {
                const int32_t c = col[e], s = base + (e - lo);
                uint32_t h = alg_hash(c);
                for (;;) {
                    const int32_t prev = atomicCAS(&hkey[h], -1, c);
                    if (prev == -1 || prev == c) { atomicMin(&hval[h], s); break; }
                    h = (h + 1) & (kHash - 1);
                }
            }
            base += hi - lo;
        });
        __syncthreads();
        for (int h = lane; h < kHash; h += 64)
            if (hkey[h] >= 0) rank[hval[h]] = 1;
        __syncthreads();
        int32_t f[4], loc = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { f[q] = rank[4 * lane + q]; loc += f[q]; }
        int32_t inc = loc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        const int32_t total = __shfl(inc, 63, 64);
        __syncthreads();
        int32_t run = inc - loc;
#pragma unroll
        for (int q = 0; q < 4; ++q) { rank[4 * lane + q] = run; run += f[q]; }
        __syncthreads();
        for (int h = lane; h < kHash; h += 64)
            if (hkey[h] >= 0) {
                const int32_t r = rank[hval[h]];
                hval[h] = r;
                ntmp[t0 + r] = hkey[h];
            }
        __syncthreads();
        base = 0;
        walk_row<KIND>(op, i, [&](const int32_t *col, const double *, int32_t lo, int32_t hi, double) {
            for (int32_t e = lo + lane; e < hi; e += 64) {
                const int32_t c = col[e];
                uint32_t h = alg_hash(c);
                while (hkey[h] != c) h = (h + 1) & (kHash - 1);
                tslot[t0 + base + (e - lo)] = hval[h];
            }
            base += hi - lo;
        });
        if (lane == 0) count[i] = total;
        __syncthreads();
    }
}

// ------------------------------------------------------------------ long-row path (global memory, hipCUB sorts)
__global__ void k_alg_long_flag(int32_t n, const int64_t *__restrict__ toff, int32_t *__restrict__ flag)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = toff[i + 1] - toff[i] > kShortCap ? 1 : 0;
}
__global__ void k_alg_long_count(int32_t nL, const int32_t *__restrict__ L, const int64_t *__restrict__ toff, int64_t *__restrict__ lc)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nL) lc[j] = toff[L[j] + 1] - toff[L[j]];
    if (j == nL) lc[j] = 0;
}
template <int KIND>
__global__ void k_alg_long_expand(AlgOp op, int32_t nL, const int32_t *__restrict__ L, const int64_t *__restrict__ loff,
                                  uint64_t *__restrict__ key, uint32_t *__restrict__ idx)
{
    for (int32_t j = blockIdx.x; j < nL; j += gridDim.x) {
        int64_t base = loff[j];
        walk_row<KIND>(op, L[j], [&](const int32_t *col, const double *, int32_t lo, int32_t hi, double) {
            for (int32_t e = lo + (int32_t)threadIdx.x; e < hi; e += blockDim.x) {
                const int64_t p = base + (e - lo);
                key[p] = ((uint64_t)(uint32_t)j << 32) | (uint32_t)col[e];
                idx[p] = (uint32_t)p;
            }
            base += hi - lo;
        });
    }
}
__global__ void k_alg_heads(int64_t m, const uint64_t *__restrict__ key, int32_t *__restrict__ head)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < m) head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}
// gid = inclusive scan of head: group g = gid-1 starts at p; its first term (stable sort) is the column's first appearance
__global__ void k_alg_groups(int64_t m, const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx,
                             const int32_t *__restrict__ head, const int32_t *__restrict__ gid, uint32_t *__restrict__ gfirst,
                             int32_t *__restrict__ gnum, int32_t *__restrict__ gcount)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || !head[p]) return;
    const int32_t g = gid[p] - 1;
    gfirst[g] = idx[p];
    gnum[g] = g;
    atomicAdd(&gcount[(int32_t)(key[p] >> 32)], 1);     // (integer counts: order-free)
}
// q-th group by first appearance (rows are contiguous in the sequence numbers): its rank = q - first group of its row
__global__ void k_alg_ranks(int32_t G, const int32_t *__restrict__ gorder, const int32_t *__restrict__ gstart,
                            const int32_t *__restrict__ gstart_of, int32_t *__restrict__ grank)
{
    const int32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < G) grank[gorder[q]] = q - gstart[gstart_of[gorder[q]]];
}
__global__ void k_alg_grow(int64_t m, const uint64_t *__restrict__ key, const int32_t *__restrict__ head,
                           const int32_t *__restrict__ gid, int32_t *__restrict__ grow, int32_t *__restrict__ gcol)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m || !head[p]) return;
    const int32_t g = gid[p] - 1;
    grow[g] = (int32_t)(key[p] >> 32);
    gcol[g] = (int32_t)(uint32_t)key[p];
}
__global__ void k_alg_long_write(int64_t m, int32_t G, const uint64_t *__restrict__ key, const uint32_t *__restrict__ idx,
                                 const int32_t *__restrict__ gid, const int32_t *__restrict__ grank, const int32_t *__restrict__ grow,
                                 const int32_t *__restrict__ gcol, const int32_t *__restrict__ L, const int64_t *__restrict__ loff,
                                 const int64_t *__restrict__ toff, int32_t *__restrict__ tslot, int32_t *__restrict__ ntmp)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < m) {
        const int32_t j = (int32_t)(key[p] >> 32);
        tslot[toff[L[j]] + ((int64_t)idx[p] - loff[j])] = grank[gid[p] - 1];
    }
    if (p < G) ntmp[toff[L[grow[p]]] + grank[p]] = gcol[p];
}
__global__ void k_alg_long_counts(int32_t nL, const int32_t *__restrict__ L, const int32_t *__restrict__ gcount, int32_t *__restrict__ count)
{
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < nL) count[L[j]] = gcount[j];
}

// ------------------------------------------------------------------ output arrays, numeric pass
__global__ void k_alg_compact(int32_t n, const int64_t *__restrict__ toff, const int32_t *__restrict__ optr,
                              const int32_t *__restrict__ ntmp, int32_t *__restrict__ ptr1, int32_t *__restrict__ node1)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    ptr1[i] = optr[i] + 1;
    if (i == n) return;
    const int64_t t0 = toff[i];
    for (int32_t r = 0; r < optr[i + 1] - optr[i]; ++r) node1[optr[i] + r] = ntmp[t0 + r] + 1;
}
template <int KIND>
__global__ void k_alg_numeric(AlgOp op, int32_t n, const int64_t *__restrict__ toff, const int32_t *__restrict__ tslot,
                              const int32_t *__restrict__ optr, double *__restrict__ val)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double *row = val + optr[i];
    for (int32_t r = 0; r < optr[i + 1] - optr[i]; ++r) row[r] = 0.0;     // +0.0 (cs_matrix_copy_graph / B%zero())
    const int32_t *slot = tslot + toff[i];
    walk_row<KIND>(op, i, [&](const int32_t *, const double *v, int32_t lo, int32_t hi, double m) {
        for (int32_t e = lo; e < hi; ++e) {
            const double z = KIND == ALG_SUM ? v[e] : m * v[e];
            row[*slot] = row[*slot] + z;                  // val = val + z, in sequence order
            ++slot;
        }
    });
}

// ------------------------------------------------------------------ host side
static const char *kOpName[4] = {"sgm_mat_sum", "sgm_mat_product", "sgm_mat_ptap", "sgm_mat_rart"};

static int check_operand(int op, sgm_mat M, const char *which)
{
    if (!M) return fail(SGM_ERR_BAD_ARG, "%s: null operand %s", kOpName[op], which);
    if (M->fmt == SGM_FMT_COMPOSITE)
        return fail(SGM_ERR_UNSUPPORTED, "%s: operand %s is a composite matrix (single-GPU CSR leaves only)", kOpName[op], which);
    if (M->distributed())
        return fail(SGM_ERR_UNSUPPORTED, "%s: operand %s is distributed / partitioned (single-GPU CSR leaves only)", kOpName[op], which);
    if (M->fmt != SGM_FMT_CSR)
        return fail(SGM_ERR_UNSUPPORTED, "%s: operand %s is not CSR (ELLPACK operands are not supported)", kOpName[op], which);
    return SGM_OK;
}
static int check_dims(int op, sgm_mat X, sgm_mat Y)
{
    switch (op) {
    case 0:
        if (X->nrow != Y->nrow || X->ncol != Y->ncol)
            return fail(SGM_ERR_DIMS, "sgm_mat_sum: shapes differ (%d x %d vs %d x %d)", X->nrow, X->ncol, Y->nrow, Y->ncol);
        break;
    case 1:
        if (X->ncol != Y->nrow) return fail(SGM_ERR_DIMS, "sgm_mat_product: B.ncol = %d != C.nrow = %d", X->ncol, Y->nrow);
        break;
    default:
        if (X->nrow != X->ncol) return fail(SGM_ERR_DIMS, "%s: A is not square (%d x %d)", kOpName[op], X->nrow, X->ncol);
        if (op == 2 && X->ncol != Y->nrow) return fail(SGM_ERR_DIMS, "sgm_mat_ptap: A.ncol = %d != P.nrow = %d", X->ncol, Y->nrow);
        if (op == 3 && Y->ncol != X->nrow) return fail(SGM_ERR_DIMS, "sgm_mat_rart: R.ncol = %d != A.nrow = %d", Y->ncol, X->nrow);
    }
    return SGM_OK;
}

// the operands' device views (lean parts unpacked; Hold releases them again), and the engine's kind
struct Hold {
    std::vector<const Part *> parts;
    ~Hold() { for (const Part *p : parts) csr_release_arrays(*p); }
    int need(const Part &p) { SGM_TRY(csr_need_arrays(p)); parts.push_back(&p); return SGM_OK; }
};
static CsrView view(const Part &p) { CsrView v; v.ptr = p.rowptr; v.col = p.col; v.val = p.val; return v; }
static int bind_operands(int op, sgm_mat X, sgm_mat Y, AlgOp &o, int &kind, Hold &hold)
{
    if (op == 0 || op == 1) {
        SGM_TRY(hold.need(X->parts[0]));
        SGM_TRY(hold.need(Y->parts[0]));
        o.X = view(X->parts[0]);
        o.Y = view(Y->parts[0]);
        kind = op == 0 ? ALG_SUM : ALG_PRODUCT;
        return SGM_OK;
    }
    sgm_mat P = Y;
    if (op == 3) {                        // P = R^T: R's columns by row ascending, duplicates in stored order
        SGM_TRY(ensure_transpose(Y));
        P = Y->T;
    }
    SGM_TRY(ensure_transpose(P));         // P^T's rows = for column i of P, (k ascending, slot) and tperm -> P's entry
    SGM_TRY(hold.need(X->parts[0]));
    SGM_TRY(hold.need(P->parts[0]));
    SGM_TRY(hold.need(P->T->parts[0]));   // (only its row pointers and columns are read)
    o.X = view(X->parts[0]);
    o.Y = view(P->parts[0]);
    o.tptr = P->T->parts[0].rowptr;
    o.tcol = P->T->parts[0].col;
    o.tpos = P->tperm;
    kind = ALG_PTAP;
    return SGM_OK;
}

static int launch_numeric(int kind, const AlgOp &o, const AlgPlan &pl, double *val)
{
    if (pl.n == 0) return SGM_OK;
    const dim3 g((unsigned)((pl.n + 127) / 128)), b(128);
    hipStream_t st = g_rt.stream;
    if (kind == ALG_SUM) hipLaunchKernelGGL(k_alg_numeric<ALG_SUM>, g, b, 0, st, o, pl.n, (const int64_t *)pl.toff, (const int32_t *)pl.tslot, (const int32_t *)pl.optr, val);
    else if (kind == ALG_PRODUCT) hipLaunchKernelGGL(k_alg_numeric<ALG_PRODUCT>, g, b, 0, st, o, pl.n, (const int64_t *)pl.toff, (const int32_t *)pl.tslot, (const int32_t *)pl.optr, val);
    else hipLaunchKernelGGL(k_alg_numeric<ALG_PTAP>, g, b, 0, st, o, pl.n, (const int64_t *)pl.toff, (const int32_t *)pl.tslot, (const int32_t *)pl.optr, val);
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

template <int KIND>
static void launch_symbolic_kernels(const AlgOp &o, int32_t n, int64_t *cnt, const int64_t *toff, int32_t *tslot, int32_t *ntmp,
                                    int32_t *count, int stage)
{
    hipStream_t st = g_rt.stream;
    if (stage == 0)
        hipLaunchKernelGGL(k_alg_count<KIND>, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, o, n, cnt);
    else if (n > 0)
        hipLaunchKernelGGL(k_alg_sym_short<KIND>, dim3((unsigned)std::min<int32_t>(n, 1 << 20)), dim3(64), 0, st, o, n, toff, tslot, ntmp, count);
}
static void symbolic_stage(int kind, const AlgOp &o, int32_t n, int64_t *cnt, const int64_t *toff, int32_t *tslot, int32_t *ntmp,
                           int32_t *count, int stage)
{
    if (kind == ALG_SUM) launch_symbolic_kernels<ALG_SUM>(o, n, cnt, toff, tslot, ntmp, count, stage);
    else if (kind == ALG_PRODUCT) launch_symbolic_kernels<ALG_PRODUCT>(o, n, cnt, toff, tslot, ntmp, count, stage);
    else launch_symbolic_kernels<ALG_PTAP>(o, n, cnt, toff, tslot, ntmp, count, stage);
}

// device scratch freed on every exit
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() { for (void *p : ptrs) if (p) (void)hipFree(p); }
    template <class T> int get(T **p, size_t count) { SGM_TRY(dalloc(p, count)); ptrs.push_back(*p); return SGM_OK; }
};

static int bits_for(int64_t v) { int b = 1; while (b < 62 && (1ll << b) <= v) ++b; return b; }

// the long-row path over the rows L (ascending): tslot / ntmp / count of those rows
static int symbolic_long(int kind, const AlgOp &o, int32_t nL, const int32_t *L, const int64_t *toff, int32_t *tslot, int32_t *ntmp,
                         int32_t *count)
{
    hipStream_t st = g_rt.stream;
    Scratch s;
    int64_t *loff = nullptr;
    SGM_TRY(s.get(&loff, (size_t)nL + 1));
    hipLaunchKernelGGL(k_alg_long_count, dim3((unsigned)((nL + 1 + 255) / 256)), dim3(256), 0, st, nL, L, toff, loff);
    size_t tb = 0;
    void *tmp = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, loff, loff, nL + 1, st);
    SGM_TRY(s.get((char **)&tmp, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, loff, loff, nL + 1, st));
    int64_t m = 0;
    SGM_HIP(hipMemcpyAsync(&m, loff + nL, 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (m > INT32_MAX - 1) return fail(SGM_ERR_UNSUPPORTED, "matrix algebra: %lld terms on long rows exceed the int32 sort", (long long)m);
    uint64_t *key = nullptr, *key2 = nullptr;
    uint32_t *idx = nullptr, *idx2 = nullptr;
    int32_t *head = nullptr, *gid = nullptr;
    SGM_TRY(s.get(&key, (size_t)m)); SGM_TRY(s.get(&key2, (size_t)m));
    SGM_TRY(s.get(&idx, (size_t)m)); SGM_TRY(s.get(&idx2, (size_t)m));
    SGM_TRY(s.get(&head, (size_t)m)); SGM_TRY(s.get(&gid, (size_t)m));
    const unsigned eg = (unsigned)std::min<int32_t>(nL, 4096);
    if (kind == ALG_SUM) hipLaunchKernelGGL(k_alg_long_expand<ALG_SUM>, dim3(eg), dim3(256), 0, st, o, nL, L, (const int64_t *)loff, key, idx);
    else if (kind == ALG_PRODUCT) hipLaunchKernelGGL(k_alg_long_expand<ALG_PRODUCT>, dim3(eg), dim3(256), 0, st, o, nL, L, (const int64_t *)loff, key, idx);
    else hipLaunchKernelGGL(k_alg_long_expand<ALG_PTAP>, dim3(eg), dim3(256), 0, st, o, nL, L, (const int64_t *)loff, key, idx);
    SGM_HIP(hipGetLastError());
    // (row, column) keys, stable: inside one key the terms stay in sequence order
    const int end_bit = 32 + bits_for(nL);
    size_t tb_sort = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort, key, key2, idx, idx2, (int)m, 0, end_bit, st);
    void *tmp2 = nullptr;
    SGM_TRY(s.get((char **)&tmp2, std::max<size_t>(tb_sort, 16)));
    SGM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp2, tb_sort, key, key2, idx, idx2, (int)m, 0, end_bit, st));
    const unsigned mg = (unsigned)((m + 255) / 256);
    hipLaunchKernelGGL(k_alg_heads, dim3(mg), dim3(256), 0, st, m, (const uint64_t *)key2, head);
    size_t tb_scan = 0;
    (void)hipcub::DeviceScan::InclusiveSum(nullptr, tb_scan, head, gid, (int)m, st);
    void *tmp3 = nullptr;
    SGM_TRY(s.get((char **)&tmp3, std::max<size_t>(tb_scan, 16)));
    SGM_HIP(hipcub::DeviceScan::InclusiveSum(tmp3, tb_scan, head, gid, (int)m, st));
    int32_t G = 0;
    SGM_HIP(hipMemcpyAsync(&G, gid + m - 1, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    uint32_t *gfirst = nullptr, *gfirst2 = nullptr;
    int32_t *gnum = nullptr, *gorder = nullptr, *gcount = nullptr, *gstart = nullptr, *grank = nullptr, *grow = nullptr, *gcol = nullptr;
    SGM_TRY(s.get(&gfirst, (size_t)G)); SGM_TRY(s.get(&gfirst2, (size_t)G));
    SGM_TRY(s.get(&gnum, (size_t)G)); SGM_TRY(s.get(&gorder, (size_t)G));
    SGM_TRY(s.get(&grank, (size_t)G)); SGM_TRY(s.get(&grow, (size_t)G)); SGM_TRY(s.get(&gcol, (size_t)G));
    SGM_TRY(s.get(&gcount, (size_t)nL + 1)); SGM_TRY(s.get(&gstart, (size_t)nL + 1));
    SGM_HIP(hipMemsetAsync(gcount, 0, ((size_t)nL + 1) * 4, st));
    hipLaunchKernelGGL(k_alg_groups, dim3(mg), dim3(256), 0, st, m, (const uint64_t *)key2, (const uint32_t *)idx2, (const int32_t *)head,
                       (const int32_t *)gid, gfirst, gnum, gcount);
    hipLaunchKernelGGL(k_alg_grow, dim3(mg), dim3(256), 0, st, m, (const uint64_t *)key2, (const int32_t *)head, (const int32_t *)gid, grow, gcol);
    // the groups by first appearance: their order inside every row is the reference's column order
    size_t tb_sort2 = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tb_sort2, gfirst, gfirst2, gnum, gorder, G, 0, bits_for(m), st);
    void *tmp4 = nullptr;
    SGM_TRY(s.get((char **)&tmp4, std::max<size_t>(tb_sort2, 16)));
    SGM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp4, tb_sort2, gfirst, gfirst2, gnum, gorder, G, 0, bits_for(m), st));
    size_t tb_scan2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb_scan2, gcount, gstart, nL + 1, st);
    void *tmp5 = nullptr;
    SGM_TRY(s.get((char **)&tmp5, std::max<size_t>(tb_scan2, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp5, tb_scan2, gcount, gstart, nL + 1, st));
    hipLaunchKernelGGL(k_alg_ranks, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, G, (const int32_t *)gorder, (const int32_t *)gstart,
                       (const int32_t *)grow, grank);
    hipLaunchKernelGGL(k_alg_long_write, dim3(mg), dim3(256), 0, st, m, G, (const uint64_t *)key2, (const uint32_t *)idx2, (const int32_t *)gid,
                       (const int32_t *)grank, (const int32_t *)grow, (const int32_t *)gcol, L, (const int64_t *)loff, toff, tslot, ntmp);
    hipLaunchKernelGGL(k_alg_long_counts, dim3((unsigned)((nL + 255) / 256)), dim3(256), 0, st, nL, L, (const int32_t *)gcount, count);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipStreamSynchronize(st));
    return SGM_OK;
}

static int algebra_create(int op, sgm_mat *out, sgm_mat X, sgm_mat Y)
{
    SGM_TRY(require_init());
    if (!out) return fail(SGM_ERR_BAD_ARG, "%s: null output", kOpName[op]);
    const char *nx = op <= 1 ? "B" : "A", *ny = op <= 1 ? "C" : op == 2 ? "P" : "R";
    SGM_TRY(check_operand(op, X, nx));
    SGM_TRY(check_operand(op, Y, ny));
    SGM_TRY(check_dims(op, X, Y));
    hipStream_t st = g_rt.stream;
    const int32_t n = op == 0 || op == 1 ? X->nrow : op == 2 ? Y->ncol : Y->nrow;
    const int32_t ncol = op == 0 ? X->ncol : op == 1 ? Y->ncol : n;
    AlgOp o;
    int kind = 0;
    Hold hold;
    SGM_TRY(bind_operands(op, X, Y, o, kind, hold));

    AlgPlan *pl = new AlgPlan;
    struct Guard { AlgPlan *&p; ~Guard() { alg_plan_free(p); } } guard{pl};
    pl->op = op;
    pl->n = n;
    Scratch s;
    int64_t *cnt = nullptr;
    SGM_TRY(dalloc(&pl->toff, (size_t)n + 1));
    cnt = pl->toff;
    symbolic_stage(kind, o, n, cnt, nullptr, nullptr, nullptr, nullptr, 0);
    size_t tb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, pl->toff, n + 1, st);
    char *tmp = nullptr;
    SGM_TRY(s.get(&tmp, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt, pl->toff, n + 1, st));
    SGM_HIP(hipMemcpyAsync(&pl->nterms, pl->toff + n, 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    int32_t *ntmp = nullptr, *count = nullptr, *flag = nullptr, *L = nullptr, *nL_dev = nullptr;
    SGM_TRY(dalloc(&pl->tslot, (size_t)pl->nterms));
    SGM_TRY(s.get(&ntmp, (size_t)pl->nterms));
    SGM_TRY(s.get(&count, (size_t)n + 1));
    SGM_TRY(dalloc(&pl->optr, (size_t)n + 1));
    SGM_HIP(hipMemsetAsync(count, 0, ((size_t)n + 1) * 4, st));
    symbolic_stage(kind, o, n, nullptr, pl->toff, pl->tslot, ntmp, count, 1);
    SGM_HIP(hipGetLastError());
    // rows past the LDS path's capacity
    SGM_TRY(s.get(&flag, (size_t)n + 1));
    SGM_TRY(s.get(&L, (size_t)n + 1));
    SGM_TRY(s.get(&nL_dev, 1));
    int32_t nL = 0;
    if (n > 0) {
        hipLaunchKernelGGL(k_alg_long_flag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const int64_t *)pl->toff, flag);
        hipcub::CountingInputIterator<int32_t> rows(0);
        size_t tbs = 0;
        (void)hipcub::DeviceSelect::Flagged(nullptr, tbs, rows, flag, L, nL_dev, n, st);
        char *tmps = nullptr;
        SGM_TRY(s.get(&tmps, std::max<size_t>(tbs, 16)));
        SGM_HIP(hipcub::DeviceSelect::Flagged(tmps, tbs, rows, flag, L, nL_dev, n, st));
        SGM_HIP(hipMemcpyAsync(&nL, nL_dev, 4, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
    }
    if (nL > 0) SGM_TRY(symbolic_long(kind, o, nL, L, pl->toff, pl->tslot, ntmp, count));
    pl->rows_long = nL;
    pl->rows_short = n - nL;
    size_t tb2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb2, count, pl->optr, n + 1, st);
    char *tmp2 = nullptr;
    SGM_TRY(s.get(&tmp2, std::max<size_t>(tb2, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp2, tb2, count, pl->optr, n + 1, st));
    int32_t nnz = 0;
    SGM_HIP(hipMemcpyAsync(&nnz, pl->optr + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    pl->nnz = nnz;
    int32_t *ptr1 = nullptr, *node1 = nullptr;
    SGM_TRY(s.get(&ptr1, (size_t)n + 1));
    SGM_TRY(s.get(&node1, (size_t)nnz));
    SGM_TRY(dalloc(&pl->val, (size_t)nnz));
    hipLaunchKernelGGL(k_alg_compact, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, n, (const int64_t *)pl->toff,
                       (const int32_t *)pl->optr, (const int32_t *)ntmp, ptr1, node1);
    SGM_HIP(hipGetLastError());
    SGM_TRY(launch_numeric(kind, o, *pl, pl->val));
    SGM_HIP(hipStreamSynchronize(st));
    sgm_mat M = nullptr;
    SGM_TRY(sgm_csr_create(&M, n, ncol, nnz, ptr1, node1, pl->val, SGM_DEVICE));
    pl->sx = X->serial;
    pl->sy = Y->serial;
    pl->pvx = X->pattern_version;
    pl->pvy = Y->pattern_version;
    pl->pvout = M->pattern_version;
    M->alg = pl;
    pl = nullptr;                         // (owned by M now)
    if (trace_on())
        fprintf(stderr, "[sgm] %s: %d x %d, %lld terms, nnz %d, rows: %d LDS, %d long\n", kOpName[op], n, ncol,
                (long long)M->alg->nterms, nnz, M->alg->rows_short, M->alg->rows_long);
    *out = M;
    return SGM_OK;
}

}  // namespace sgm

using namespace sgm;

extern "C" {

int sgm_mat_sum(sgm_mat *out, sgm_mat B, sgm_mat C) { return algebra_create(0, out, B, C); }
int sgm_mat_product(sgm_mat *out, sgm_mat B, sgm_mat C) { return algebra_create(1, out, B, C); }
int sgm_mat_ptap(sgm_mat *out, sgm_mat A, sgm_mat P) { return algebra_create(2, out, A, P); }
int sgm_mat_rart(sgm_mat *out, sgm_mat A, sgm_mat R) { return algebra_create(3, out, A, R); }

int sgm_mat_algebra_refill(sgm_mat out, sgm_mat X, sgm_mat Y)
{
    SGM_TRY(require_init());
    if (!out || !X || !Y) return fail(SGM_ERR_BAD_ARG, "sgm_mat_algebra_refill: null argument");
    AlgPlan *pl = out->alg;
    if (!pl) return fail(SGM_ERR_BAD_ARG, "sgm_mat_algebra_refill: the matrix is not the result of a matrix algebra call");
    if (X->serial != pl->sx || Y->serial != pl->sy)
        return fail(SGM_ERR_BAD_ARG, "sgm_mat_algebra_refill: the operands are not the ones %s was built from (same handles, same order)",
                    kOpName[pl->op]);
    if (X->pattern_version != pl->pvx || Y->pattern_version != pl->pvy)
        return fail(SGM_ERR_BAD_ARG, "sgm_mat_algebra_refill: an operand's pattern changed since %s (permuted)", kOpName[pl->op]);
    if (out->pattern_version != pl->pvout)
        return fail(SGM_ERR_BAD_ARG, "sgm_mat_algebra_refill: the result's pattern changed since %s (permuted)", kOpName[pl->op]);
    AlgOp o;
    int kind = 0;
    {
        Hold hold;
        SGM_TRY(bind_operands(pl->op, X, Y, o, kind, hold));
        SGM_TRY(launch_numeric(kind, o, *pl, pl->val));
        SGM_HIP(hipStreamSynchronize(g_rt.stream));
    }
    return sgm_csr_set_values(out, pl->val, SGM_DEVICE);     // bumps out->version
}

}  // extern "C"
