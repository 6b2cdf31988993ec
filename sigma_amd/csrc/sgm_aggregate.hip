// Algebraic coarsening on the device: smoothed aggregation on a distance-2 maximal independent set.
// The reference has PtAP "for multigrid setup" and neither a multigrid nor a coarsening: the contract is this library's own,
// stated in include/sigma_hip.h (sgm_mat_aggregate) and restated twice in tests/aggregate_restated.py.
//
// Per level, for a square single-GPU CSR matrix A of n rows:
//   d(i)        the LAST stored copy of a_ii, 0.0 when absent (the Jacobi setup's rule)
//   strength    a stored entry a of row i in column j != i is strong when a*a >= theta^2 * (|d(i)| * |d(j)|), every product
//               rounded on its own; N(i) = the j with a strong stored copy of (i,j) or of (j,i)
//   adjacency   N as int32 lists, built ONCE: the strong entries of A's row i, then those of row i of the transpose the
//               library already builds (through tperm to A's values) -- short rows leave out the second copy of a
//               neighbour the first part already holds; every later step is a max over N(i), so duplicates and order do
//               not matter.  The rounds read 4 bytes per edge and no values.
//   rounds      one 8-byte word per vertex: all ones = root, key(i) = undecided, 0 = removed.  Pass 1: m1(i) = max of the
//               word over {i} + N(i); pass 2: m2(i) = max of m1 over {i} + N(i) = the max over distance <= 2.  An
//               undecided vertex that sees all ones is removed, one that sees its own key becomes a root.  Pass 2 reads
//               only m1 of others, so it updates the words in place; it also counts what is still undecided, one
//               atomicAdd per workgroup, and the host reads that counter back (4 bytes, after the stream has drained).
//               Rows of at most 64 neighbours take one lane per row, longer rows one wave per row and a permlane / DPP max.
//   numbering   roots 1..nagg in ascending row index (a scan over the root flags)
//   phase 1     a non-root with a root in N(i) joins the root of largest key
//   phase 2     the others join the aggregate of the largest-key member of N(i) placed so far (read from phase 1's
//               array, written to another: no vertex sees a phase 2 placement)
// The hierarchy composes this with sgm_mat_product / sgm_mat_sum / sgm_mat_ptap: T(i, agg(i)) = 1.0,
// W = A T, W's row i scaled by -(omega * idiag(i)), P = T + W, A_{l+1} = P^T A_l P.
#include "sgm_spmv_select.hpp"

#include <cmath>

namespace sgm {

constexpr uint64_t kAggRoot = ~0ull;
constexpr int kAggWave = 64;             // neighbours a lane-per-row pass takes; longer rows: one wave per row
constexpr int kAggDedup = 32;            // stored entries of a row up to which the transposed part is checked against it

__device__ __host__ inline uint64_t agg_key(int32_t i)
{
    uint32_t h = (uint32_t)i * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return ((uint64_t)h << 32) | (uint32_t)(i + 1);
}

__device__ inline bool agg_strong(double a, double di, double dj, double t2)
{
    return a * a >= t2 * (fabs(di) * fabs(dj));      // a NaN on either side: not strong
}

struct AggGraph {
    int32_t n = 0;
    const int32_t *ptr = nullptr, *col = nullptr;    // A (0-based)
    const double *val = nullptr;
    const int32_t *tptr = nullptr, *tcol = nullptr;  // A^T's rows: source row of every entry, (row, slot) order
    const int32_t *tperm = nullptr;                  // ... and the entry of A behind it
    const double *d = nullptr;
    double t2 = 0.0;
};

__global__ void k_agg_diag(int32_t n, const int32_t *__restrict__ ptr, const int32_t *__restrict__ col,
                           const double *__restrict__ val, double *__restrict__ d)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double z = 0.0;
    for (int32_t e = ptr[i]; e < ptr[i + 1]; ++e)
        if (col[e] == i) z = val[e];
    d[i] = z;
}

// f(j) for every member of N(i): A's strong entries of row i, then the transpose's
template <class F>
__device__ inline void agg_walk(const AggGraph &g, int32_t i, F &&f)
{
    const double di = g.d[i];
    const int32_t lo = g.ptr[i], hi = g.ptr[i + 1];
    for (int32_t e = lo; e < hi; ++e) {
        const int32_t j = g.col[e];
        if (j != i && agg_strong(g.val[e], di, g.d[j], g.t2)) f(j);
    }
    const bool dedup = hi - lo <= kAggDedup;
    for (int32_t e = g.tptr[i]; e < g.tptr[i + 1]; ++e) {
        const int32_t j = g.tcol[e];
        if (j == i || !agg_strong(g.val[g.tperm[e]], g.d[j], di, g.t2)) continue;
        bool seen = false;
        if (dedup)
            for (int32_t q = lo; q < hi && !seen; ++q) seen = g.col[q] == j && agg_strong(g.val[q], di, g.d[j], g.t2);
        if (!seen) f(j);
    }
}

__global__ void k_agg_count(AggGraph g, int32_t *__restrict__ cnt)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > g.n) return;
    int32_t c = 0;
    if (i < g.n) agg_walk(g, i, [&](int32_t) { ++c; });
    cnt[i] = c;                          // cnt[n] = 0: the exclusive scan's total lands there
}

__global__ void k_agg_fill(AggGraph g, const int32_t *__restrict__ aptr, int32_t *__restrict__ adj, uint64_t *__restrict__ s,
                           int32_t *__restrict__ is_long)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    int32_t at = aptr[i];
    agg_walk(g, i, [&](int32_t j) { adj[at++] = j; });
    s[i] = agg_key(i);
    is_long[i] = aptr[i + 1] - aptr[i] > kAggWave ? 1 : 0;
}

// ------------------------------------------------------------------ the rounds
template <int CTRL>
__device__ inline uint64_t dpp_lane_u64(uint64_t v)
{
    int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ inline uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
// max over the 64 lanes of a wave, the same value in every lane: wave_sum's exchange pattern (sgm_internal.hpp) with max
__device__ inline uint64_t wave_max_u64(uint64_t v)
{
    {
        const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = max_u64(((uint64_t)h[0] << 32) | l[0], ((uint64_t)h[1] << 32) | l[1]);
    }
    {
        const unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
        const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = max_u64(((uint64_t)h[0] << 32) | l[0], ((uint64_t)h[1] << 32) | l[1]);
    }
    v = max_u64(v, dpp_lane_u64<0x128>(v));      // row_ror:8
    v = max_u64(v, dpp_lane_u64<0x124>(v));      // row_ror:4
    v = max_u64(v, dpp_lane_u64<0x122>(v));      // row_ror:2
    v = max_u64(v, dpp_lane_u64<0x121>(v));      // row_ror:1
    return v;
}

// one atomicAdd per workgroup of the threads whose `mine` is set
__device__ inline void block_count_add(bool mine, int32_t *counter)
{
    __shared__ int32_t wcount[kBlock / 64];
    const int c = __popcll(__ballot(mine));
    if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int32_t t = 0;
        for (int w = 0; w < kBlock / 64; ++w) t += wcount[w];
        if (t) atomicAdd(counter, t);
    }
}

// pass 1, one lane per row: m1(i) = max(s(i), s over N(i)); a root's is all ones whatever its neighbours hold
__global__ __launch_bounds__(kBlock) void k_agg_pass1(int32_t n, const int32_t *__restrict__ aptr, const int32_t *__restrict__ adj,
                                                     const uint64_t *__restrict__ s, uint64_t *__restrict__ m1,
                                                     int32_t *__restrict__ counter)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) *counter = 0;            // pass 2 of this round counts into it
    if (i >= n) return;
    const int32_t lo = aptr[i], hi = aptr[i + 1];
    if (hi - lo > kAggWave) return;      // k_agg_pass1_long's
    uint64_t v = s[i];
    if (v != kAggRoot)
        for (int32_t e = lo; e < hi; ++e) v = max_u64(v, s[adj[e]]);
    m1[i] = v;
}

// pass 2 and the decision: only an undecided vertex needs its distance-2 max
__global__ __launch_bounds__(kBlock) void k_agg_pass2(int32_t n, const int32_t *__restrict__ aptr, const int32_t *__restrict__ adj,
                                                     uint64_t *__restrict__ s, const uint64_t *__restrict__ m1,
                                                     int32_t *__restrict__ counter)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    bool left = false;
    if (i < n) {
        const int32_t lo = aptr[i], hi = aptr[i + 1];
        const uint64_t v = s[i];
        if (hi - lo <= kAggWave && v != kAggRoot && v != 0) {
            uint64_t m = m1[i];
            for (int32_t e = lo; e < hi; ++e) m = max_u64(m, m1[adj[e]]);
            if (m == kAggRoot) s[i] = 0;
            else if (m == v) s[i] = kAggRoot;
            else left = true;
        }
    }
    block_count_add(left, counter);
}

// the rows of more than 64 neighbours: one wave per row
__global__ __launch_bounds__(kBlock) void k_agg_pass1_long(int32_t nL, const int32_t *__restrict__ L, const int32_t *__restrict__ aptr,
                                                          const int32_t *__restrict__ adj, const uint64_t *__restrict__ s,
                                                          uint64_t *__restrict__ m1)
{
    const int32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= nL) return;
    const int32_t i = L[w];
    uint64_t v = s[i];
    if (v != kAggRoot) {
        for (int32_t e = aptr[i] + lane; e < aptr[i + 1]; e += 64) v = max_u64(v, s[adj[e]]);
        v = wave_max_u64(v);
    }
    if (lane == 0) m1[i] = v;
}

__global__ __launch_bounds__(kBlock) void k_agg_pass2_long(int32_t nL, const int32_t *__restrict__ L, const int32_t *__restrict__ aptr,
                                                          const int32_t *__restrict__ adj, uint64_t *__restrict__ s,
                                                          const uint64_t *__restrict__ m1, int32_t *__restrict__ counter)
{
    const int32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    bool left = false;
    if (w < nL) {
        const int32_t i = L[w];
        const uint64_t v = s[i];
        if (v != kAggRoot && v != 0) {
            uint64_t m = m1[i];
            for (int32_t e = aptr[i] + lane; e < aptr[i + 1]; e += 64) m = max_u64(m, m1[adj[e]]);
            m = wave_max_u64(m);
            if (lane == 0) {
                if (m == kAggRoot) s[i] = 0;
                else if (m == v) s[i] = kAggRoot;
                else left = true;
            }
        }
    }
    block_count_add(left, counter);
}

// ------------------------------------------------------------------ numbering and membership
__global__ void k_agg_root_flags(int32_t n, const uint64_t *__restrict__ s, int32_t *__restrict__ flag)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) flag[i] = i < n && s[i] == kAggRoot ? 1 : 0;
}

// num: roots before row i.  agg1(i) = a root's number, the number of the largest-key root of N(i), or 0
__global__ void k_agg_phase1(int32_t n, const int32_t *__restrict__ aptr, const int32_t *__restrict__ adj,
                             const uint64_t *__restrict__ s, const int32_t *__restrict__ num, int32_t *__restrict__ agg1)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t at = i;
    if (s[i] != kAggRoot) {
        at = -1;
        uint64_t best = 0;
        for (int32_t e = aptr[i]; e < aptr[i + 1]; ++e) {
            const int32_t j = adj[e];
            if (s[j] != kAggRoot) continue;
            const uint64_t k = agg_key(j);
            if (k > best) { best = k; at = j; }
        }
    }
    agg1[i] = at >= 0 ? num[at] + 1 : 0;
}

__global__ void k_agg_phase2(int32_t n, const int32_t *__restrict__ aptr, const int32_t *__restrict__ adj,
                             const int32_t *__restrict__ agg1, int32_t *__restrict__ agg)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t a = agg1[i];
    if (a == 0) {
        uint64_t best = 0;
        for (int32_t e = aptr[i]; e < aptr[i + 1]; ++e) {
            const int32_t j = adj[e], aj = agg1[j];
            if (aj == 0) continue;
            const uint64_t k = agg_key(j);
            if (k > best) { best = k; a = aj; }
        }
    }
    agg[i] = a;
}

// T: row i holds the one entry (agg(i), 1.0); 1-based arrays for sgm_csr_create
__global__ void k_agg_tentative(int32_t n, int32_t *__restrict__ ptr1, double *__restrict__ val)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) ptr1[i] = i + 1;
    if (i < n) val[i] = 1.0;
}

// out = W's values, row i times -(omega * idiag(i)), idiag(i) = 1.0 / d(i) or 0.0 when d(i) == 0
__global__ void k_agg_row_scale(int32_t n, const int32_t *__restrict__ wptr, const double *__restrict__ wval,
                                const double *__restrict__ d, double omega, double *__restrict__ out)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double di = d[i];
    const double f = -(omega * (di == 0.0 ? 0.0 : 1.0 / di));
    for (int32_t e = wptr[i]; e < wptr[i + 1]; ++e) out[e] = f * wval[e];
}

// ------------------------------------------------------------------ host side
namespace {

struct AggScratch {
    std::vector<void *> ptrs;
    ~AggScratch() { for (void *p : ptrs) if (p) (void)hipFree(p); }
    template <class T> int get(T **p, size_t count) { SGM_TRY(dalloc(p, count)); ptrs.push_back(*p); return SGM_OK; }
};
struct AggHold {
    std::vector<const Part *> parts;
    ~AggHold() { for (const Part *p : parts) csr_release_arrays(*p); }
    int need(const Part &p) { SGM_TRY(csr_need_arrays(p)); parts.push_back(&p); return SGM_OK; }
};

// what one level cost, filled when SGM_TRACE is set (events on the library's stream)
struct AggTimes {
    enum { START = 0, ADJ, ROUNDS, PHASES, SMOOTH, GALERKIN, COUNT };
    hipEvent_t ev[COUNT] = {};
    bool on = false, have[COUNT] = {};
    AggTimes() : on(trace_on()) {}
    ~AggTimes() { for (auto e : ev) if (e) (void)hipEventDestroy(e); }
    void mark(int k)
    {
        if (!on) return;
        if (!ev[k] && hipEventCreate(&ev[k]) != hipSuccess) { ev[k] = nullptr; return; }
        have[k] = hipEventRecord(ev[k], g_rt.stream) == hipSuccess;
    }
    double ms(int a, int b)
    {
        float t = 0.0f;
        if (!on || !have[a] || !have[b]) return 0.0;
        (void)hipEventSynchronize(ev[b]);
        return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0;
    }
};

struct AggInfo { int32_t rounds = 0, nlong = 0; int64_t edges = 0; };

int check_matrix(const char *fn, sgm_mat A)
{
    if (!A) return fail(SGM_ERR_BAD_ARG, "%s: null matrix", fn);
    if (A->fmt == SGM_FMT_COMPOSITE)
        return fail(SGM_ERR_UNSUPPORTED, "%s: A is a composite matrix (single-GPU CSR leaves only)", fn);
    if (A->distributed())
        return fail(SGM_ERR_UNSUPPORTED, "%s: A is distributed / partitioned (single-GPU CSR leaves only)", fn);
    if (A->fmt != SGM_FMT_CSR) return fail(SGM_ERR_UNSUPPORTED, "%s: A is not CSR (ELLPACK operands are not supported)", fn);
    if (A->nrow != A->ncol) return fail(SGM_ERR_DIMS, "%s: A is not square (%d x %d)", fn, A->nrow, A->ncol);
    return SGM_OK;
}

inline unsigned row_grid(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

template <class T>
int scan_exclusive(AggScratch &s, T *data, int32_t count)
{
    size_t tb = 0;
    char *tmp = nullptr;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, data, data, count, g_rt.stream);
    SGM_TRY(s.get(&tmp, std::max<size_t>(tb, 16)));
    SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, data, data, count, g_rt.stream));
    return SGM_OK;
}

// agg (n device entries, 1-based aggregate numbers) and d (n device doubles) of A; both the caller's to free
int aggregate_device(sgm_mat A, double theta, int32_t *agg, double *d, int32_t *nagg, AggInfo *info, AggTimes *tm)
{
    hipStream_t st = g_rt.stream;
    const int32_t n = A->nrow;
    *nagg = 0;
    if (n == 0) return SGM_OK;
    SGM_TRY(ensure_transpose(A));
    AggHold hold;
    const Part &p = A->parts[0], &tp = A->T->parts[0];
    SGM_TRY(hold.need(p));
    SGM_TRY(hold.need(tp));
    AggScratch s;
    AggGraph g;
    g.n = n;
    g.ptr = p.rowptr; g.col = p.col; g.val = p.val;
    g.tptr = tp.rowptr; g.tcol = tp.col; g.tperm = A->tperm;
    g.d = d;
    g.t2 = theta * theta;

    if (tm) tm->mark(AggTimes::START);
    hipLaunchKernelGGL(k_agg_diag, dim3(row_grid(n)), dim3(kBlock), 0, st, n, g.ptr, g.col, g.val, d);
    int32_t *aptr = nullptr, *adj = nullptr, *flag = nullptr, *L = nullptr, *counter = nullptr, *agg1 = nullptr;
    uint64_t *state = nullptr, *m1 = nullptr;
    SGM_TRY(s.get(&aptr, (size_t)n + 1));
    hipLaunchKernelGGL(k_agg_count, dim3(row_grid((int64_t)n + 1)), dim3(kBlock), 0, st, g, aptr);
    SGM_HIP(hipGetLastError());
    // (a row holds fewer than 2^31 entries of A and of A^T each; the total is checked through a 64-bit sum of the two nnz)
    if (2 * A->nnz > INT32_MAX) return fail(SGM_ERR_UNSUPPORTED, "aggregation: %lld stored entries exceed the int32 adjacency", (long long)A->nnz);
    SGM_TRY(scan_exclusive(s, aptr, n + 1));
    int32_t edges = 0;
    SGM_HIP(hipMemcpyAsync(&edges, aptr + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    SGM_TRY(s.get(&adj, (size_t)edges));
    SGM_TRY(s.get(&state, (size_t)n));
    SGM_TRY(s.get(&m1, (size_t)n));
    SGM_TRY(s.get(&flag, (size_t)n + 1));
    SGM_TRY(s.get(&L, (size_t)n));
    SGM_TRY(s.get(&counter, 2));
    SGM_TRY(s.get(&agg1, (size_t)n));
    hipLaunchKernelGGL(k_agg_fill, dim3(row_grid(n)), dim3(kBlock), 0, st, g, (const int32_t *)aptr, adj, state, flag);
    SGM_HIP(hipGetLastError());
    // the rows one lane does not take
    int32_t nL = 0;
    {
        hipcub::CountingInputIterator<int32_t> rows(0);
        size_t tb = 0;
        char *tmp = nullptr;
        (void)hipcub::DeviceSelect::Flagged(nullptr, tb, rows, flag, L, counter + 1, n, st);
        SGM_TRY(s.get(&tmp, std::max<size_t>(tb, 16)));
        SGM_HIP(hipcub::DeviceSelect::Flagged(tmp, tb, rows, flag, L, counter + 1, n, st));
        SGM_HIP(hipMemcpyAsync(&nL, counter + 1, 4, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
    }
    if (tm) tm->mark(AggTimes::ADJ);

    const unsigned gl = (unsigned)(((int64_t)nL + kBlock / 64 - 1) / (kBlock / 64));
    int32_t rounds = 0, left = 1;
    while (left > 0) {
        if (rounds > n) return fail(SGM_ERR_HIP, "aggregation: the rounds did not end after %d rounds on %d rows", rounds, n);
        hipLaunchKernelGGL(k_agg_pass1, dim3(row_grid(n)), dim3(kBlock), 0, st, n, (const int32_t *)aptr, (const int32_t *)adj,
                           (const uint64_t *)state, m1, counter);
        if (nL)
            hipLaunchKernelGGL(k_agg_pass1_long, dim3(gl), dim3(kBlock), 0, st, nL, (const int32_t *)L, (const int32_t *)aptr,
                               (const int32_t *)adj, (const uint64_t *)state, m1);
        hipLaunchKernelGGL(k_agg_pass2, dim3(row_grid(n)), dim3(kBlock), 0, st, n, (const int32_t *)aptr, (const int32_t *)adj, state,
                           (const uint64_t *)m1, counter);
        if (nL)
            hipLaunchKernelGGL(k_agg_pass2_long, dim3(gl), dim3(kBlock), 0, st, nL, (const int32_t *)L, (const int32_t *)aptr,
                               (const int32_t *)adj, state, (const uint64_t *)m1, counter);
        SGM_HIP(hipGetLastError());
        // the one readback of a round: it waits for the stream the passes ran on
        SGM_HIP(hipMemcpyAsync(&left, counter, 4, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
        ++rounds;
    }
    if (tm) tm->mark(AggTimes::ROUNDS);

    hipLaunchKernelGGL(k_agg_root_flags, dim3(row_grid((int64_t)n + 1)), dim3(kBlock), 0, st, n, (const uint64_t *)state, flag);
    SGM_TRY(scan_exclusive(s, flag, n + 1));
    hipLaunchKernelGGL(k_agg_phase1, dim3(row_grid(n)), dim3(kBlock), 0, st, n, (const int32_t *)aptr, (const int32_t *)adj,
                       (const uint64_t *)state, (const int32_t *)flag, agg1);
    hipLaunchKernelGGL(k_agg_phase2, dim3(row_grid(n)), dim3(kBlock), 0, st, n, (const int32_t *)aptr, (const int32_t *)adj,
                       (const int32_t *)agg1, agg);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipMemcpyAsync(nagg, flag + n, 4, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (tm) tm->mark(AggTimes::PHASES);
    if (info) { info->rounds = rounds; info->nlong = nL; info->edges = edges; }
    return SGM_OK;
}

// P of one level from its aggregates: T, or T + (row-scaled A T)
int prolongation(sgm_mat A, const int32_t *agg, const double *d, int32_t nagg, double omega, sgm_mat *out)
{
    hipStream_t st = g_rt.stream;
    const int32_t n = A->nrow;
    AggScratch s;
    int32_t *ptr1 = nullptr;
    double *ones = nullptr;
    SGM_TRY(s.get(&ptr1, (size_t)n + 1));
    SGM_TRY(s.get(&ones, (size_t)n));
    hipLaunchKernelGGL(k_agg_tentative, dim3(row_grid((int64_t)n + 1)), dim3(kBlock), 0, st, n, ptr1, ones);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipStreamSynchronize(st));
    sgm_mat T = nullptr, W = nullptr;
    SGM_TRY(sgm_csr_create(&T, n, nagg, n, ptr1, agg, ones, SGM_DEVICE));
    if (omega == 0.0) { *out = T; return SGM_OK; }
    struct Temps { sgm_mat &T, &W; ~Temps() { if (T) sgm_mat_destroy(T); if (W) sgm_mat_destroy(W); } } temps{T, W};
    SGM_TRY(sgm_mat_product(&W, A, T));
    double *scaled = nullptr;
    SGM_TRY(s.get(&scaled, (size_t)W->nnz));
    {
        AggHold hold;
        const Part &wp = W->parts[0];
        SGM_TRY(hold.need(wp));
        hipLaunchKernelGGL(k_agg_row_scale, dim3(row_grid(n)), dim3(kBlock), 0, st, n, (const int32_t *)wp.rowptr, (const double *)wp.val, d,
                           omega, scaled);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipStreamSynchronize(st));
    }
    SGM_TRY(sgm_csr_set_values(W, scaled, SGM_DEVICE));
    sgm_mat P = nullptr;
    SGM_TRY(sgm_mat_sum(&P, T, W));
    alg_plan_free(P->alg);               // P leaves as a plain matrix: its operands do not outlive this call
    P->alg = nullptr;
    *out = P;
    return SGM_OK;
}

}  // namespace

}  // namespace sgm

using namespace sgm;

extern "C" {

int sgm_mat_aggregate(sgm_mat A, double theta, int32_t *agg_out, int32_t *nagg, int where)
{
    SGM_TRY(require_init());
    SGM_TRY(check_matrix("sgm_mat_aggregate", A));
    if (!(theta >= 0.0)) return fail(SGM_ERR_BAD_ARG, "sgm_mat_aggregate: theta = %g (it must be >= 0)", theta);
    if (!agg_out || !nagg) return fail(SGM_ERR_BAD_ARG, "sgm_mat_aggregate: null output");
    if (where != SGM_HOST && where != SGM_DEVICE) return fail(SGM_ERR_BAD_ARG, "sgm_mat_aggregate: where = %d", where);
    const int32_t n = A->nrow;
    AggScratch s;
    int32_t *agg = nullptr;
    double *d = nullptr;
    SGM_TRY(s.get(&agg, (size_t)n));
    SGM_TRY(s.get(&d, (size_t)n));
    int32_t count = 0;
    AggInfo info;
    SGM_TRY(aggregate_device(A, theta, agg, d, &count, &info, nullptr));
    if (n > 0) {
        if (where == SGM_DEVICE) {
            SGM_HIP(hipMemcpyAsync(agg_out, agg, (size_t)n * 4, hipMemcpyDeviceToDevice, g_rt.stream));
            SGM_HIP(hipStreamSynchronize(g_rt.stream));
        } else {
            SGM_TRY(copy_big(agg_out, agg, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
    }
    *nagg = count;
    if (trace_on())
        fprintf(stderr, "[sgm] aggregate: rows %d, aggregates %d, strong %lld, rounds %d, long rows %d\n", n, count,
                (long long)info.edges, info.rounds, info.nlong);
    return SGM_OK;
}

int sgm_mg_aggregation_hierarchy(sgm_mat A, double theta, double smooth_omega, int32_t max_levels, int32_t min_coarse,
                                 sgm_mat *P_out, int32_t *ncoarse)
{
    SGM_TRY(require_init());
    const char *fn = "sgm_mg_aggregation_hierarchy";
    SGM_TRY(check_matrix(fn, A));
    if (!(theta >= 0.0)) return fail(SGM_ERR_BAD_ARG, "%s: theta = %g (it must be >= 0)", fn, theta);
    if (!(smooth_omega >= 0.0) || std::isinf(smooth_omega))
        return fail(SGM_ERR_BAD_ARG, "%s: smooth_omega = %g (it must be finite and >= 0)", fn, smooth_omega);
    if (max_levels < 1) return fail(SGM_ERR_BAD_ARG, "%s: max_levels = %d (it must be >= 1)", fn, max_levels);
    if (min_coarse < 1) return fail(SGM_ERR_BAD_ARG, "%s: min_coarse = %d (it must be >= 1)", fn, min_coarse);
    if (!ncoarse || (!P_out && max_levels > 1)) return fail(SGM_ERR_BAD_ARG, "%s: null output", fn);
    *ncoarse = 0;
    int32_t made = 0;
    sgm_mat cur = A;
    // whatever a failed call built is destroyed again
    struct Undo {
        sgm_mat A, &cur, *P; int32_t &made; bool armed = true;
        ~Undo()
        {
            if (cur != A) sgm_mat_destroy(cur);
            if (!armed) return;
            for (int32_t l = 0; l < made; ++l) { sgm_mat_destroy(P[l]); P[l] = nullptr; }
        }
    } undo{A, cur, P_out, made};
    for (int32_t levels = 1; levels < max_levels && cur->nrow > min_coarse; ++levels) {
        const int32_t n = cur->nrow;
        AggScratch s;
        AggTimes tm;
        AggInfo info;
        int32_t *agg = nullptr, nagg = 0;
        double *d = nullptr;
        SGM_TRY(s.get(&agg, (size_t)n));
        SGM_TRY(s.get(&d, (size_t)n));
        SGM_TRY(aggregate_device(cur, theta, agg, d, &nagg, &info, &tm));
        if (nagg >= n) break;            // no reduction (a diagonal matrix): no level is added
        SGM_TRY(prolongation(cur, agg, d, nagg, smooth_omega, &P_out[made]));
        ++made;
        tm.mark(AggTimes::SMOOTH);
        if (levels + 1 < max_levels && nagg > min_coarse) {
            sgm_mat next = nullptr;
            SGM_TRY(sgm_mat_ptap(&next, cur, P_out[made - 1]));
            if (cur != A) sgm_mat_destroy(cur);
            cur = next;
            tm.mark(AggTimes::GALERKIN);
        }
        if (tm.on)
            fprintf(stderr, "[sgm] aggregation level %d: rows %d, aggregates %d, strong %lld, rounds %d, long rows %d, "
                            "adjacency %.3f ms, rounds %.3f ms, phases %.3f ms, smoothing %.3f ms, galerkin %.3f ms\n",
                    levels - 1, n, nagg, (long long)info.edges, info.rounds, info.nlong, tm.ms(AggTimes::START, AggTimes::ADJ),
                    tm.ms(AggTimes::ADJ, AggTimes::ROUNDS), tm.ms(AggTimes::ROUNDS, AggTimes::PHASES),
                    tm.ms(AggTimes::PHASES, AggTimes::SMOOTH), tm.ms(AggTimes::SMOOTH, AggTimes::GALERKIN));
        if (cur->nrow != nagg) break;    // the next level was not formed: the loop's own test ends it
    }
    undo.armed = false;
    *ncoarse = made;
    return SGM_OK;
}

}  // extern "C"
