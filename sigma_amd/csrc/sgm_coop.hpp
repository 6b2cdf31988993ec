// Shared by sgm_cg.hip and sgm_bicgstab.hip: what the one-workgroup and the cooperative (one launch, up to 256 workgroups)
// solvers of small and mid-sized systems are made of.  Device: the one-workgroup kernels' row sums out of LDS and block dots in
// both orders; the cooperative kernels' grid-wide hand-off (one or two scalars), workgroup geometry, publishing of boundary
// rows and block dots.  Host: the rules that decide when these kernels apply, the driver that runs a solve as launches of
// bounded length (run_chunked), run-time values as template arguments, and the order of the fast paths.
// NOT here, on purpose: the cooperative kernels' matrix load, row sums, halo index arithmetic and proof of co-location.
// k_cg_coop and k_bicg_coop each write them out, with the same text: both kernels sit at 128 VGPRs, and as shared functions
// the first three moved spills (8 more bytes of scratch in 1 k_cg_coop and up to 18 k_bicg_coop kernels) and the proof changed
// the text of every one-XCD kernel; with them written out every kernel compiles to the text it had before this header
// held any device code of theirs (profiles/krylov_dedupe/README.md).
#pragma once
#include "sgm_krylov.hpp"

#include <cctype>
#include <string>

namespace sgm {

// The RMAX row sums of one thread of a single-workgroup solver (rows tid, tid + 1024, ...), x gathered out of LDS
// (`pl`), side by side: slot e of every row is requested before any of them is used, so a row's entries are still
// added left to right but the thread waits for one round trip per SLOT, not per entry (rows one after the other:
// 16 us per CG iteration at n = 1e4, five entries per row).  SL: sliced form (a0 = code words, a1 = offset
// dictionary, val = sval); otherwise CSR (a0 = rowptr, a1 = col).
template <int RMAX, bool SL>
__device__ inline void small_row_sums(double (&q)[RMAX], const double *pl, int32_t n, int32_t sw,
                                      const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                      const double *__restrict__ val)
{
    constexpr int BLOCK = 1024;
    const int tid = threadIdx.x;
    if (SL) {
        uint32_t cw[RMAX];
#pragma unroll
        for (int u = 0; u < RMAX; ++u) {
            const int32_t i = tid + u * BLOCK;
            q[u] = 0.0;
            cw[u] = i < n ? (uint32_t)rowptr[i] : 0xffffffffu;
        }
        constexpr int H = RMAX > 5 ? (RMAX + 1) / 2 : RMAX;        // rows side by side (all ten: 71-89 registers spilled)
#pragma unroll
        for (int h0 = 0; h0 < RMAX; h0 += H)
            for (int32_t e = 0; e < sw; ++e) {
                double v[H];
#pragma unroll
                for (int u = h0; u < h0 + H && u < RMAX; ++u) {
                    const int32_t i = tid + u * BLOCK;
                    if (((cw[u] >> (4 * e)) & 15u) != 15u) v[u - h0] = val[((i >> 9) * sw + e) * 512 + (i & 511)];
                }
#pragma unroll
                for (int u = h0; u < h0 + H && u < RMAX; ++u) {
                    const int32_t i = tid + u * BLOCK;
                    const uint32_t cd = (cw[u] >> (4 * e)) & 15u;
                    if (cd != 15u) q[u] = q[u] + v[u - h0] * pl[i + col[cd]];
                }
            }
#pragma unroll
        for (int u = 0; u < RMAX; ++u) q[u] = 0.0 + q[u];
        return;
    }
    int32_t k0[RMAX], len[RMAX];
    int32_t longest = 0;
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int32_t i = tid + u * BLOCK;
        k0[u] = 0; len[u] = 0; q[u] = 0.0;
        if (i < n) { k0[u] = rowptr[i]; len[u] = rowptr[i + 1] - k0[u]; }
        longest = max(longest, len[u]);
    }
    for (int32_t e = 0; e < longest; ++e) {
        double v[RMAX]; int32_t c[RMAX];
#pragma unroll
        for (int u = 0; u < RMAX; ++u)
            if (e < len[u]) { v[u] = val[k0[u] + e]; c[u] = col[k0[u] + e]; }
#pragma unroll
        for (int u = 0; u < RMAX; ++u)
            if (e < len[u]) q[u] = q[u] + v[u] * pl[c[u]];
    }
#pragma unroll
    for (int u = 0; u < RMAX; ++u) q[u] = 0.0 + q[u];          // A%matvec: y = 0 ; y(i) = y(i) + z
}

// A dot product inside a single-workgroup solver: thread t holds the products of its rows t, t + BLOCK, ... (0.0 beyond n).
// Tree order (dot_order = 0): the thread's own rows first, then the block sum.  SEQ (dot_order = 1): the products are
// parked in LDS by row and ONE wave adds them row 0 to row n-1 -- the reference's dot_product order.
template <int BLOCK, int RMAX, bool SEQ>
__device__ inline double small_dot(const double (&prod)[RMAX], int32_t n, double *pr, double *red)
{
    if (!SEQ) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < RMAX; ++u)
            if ((int32_t)threadIdx.x + u * BLOCK < n) s += prod[u];
        return block_sum<BLOCK>(s, red);
    }
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int32_t i = threadIdx.x + u * BLOCK;
        if (i < n) pr[i] = prod[u];
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const double s = seq_chain_lds(pr, n, 0.0);
        if (threadIdx.x == 0) red[0] = s;
    }
    __syncthreads();
    return red[0];
}
// two at once (BiCGStab's s.t / t.t and r.r / r0.r): SEQ walks them side by side, waves 0 and 1
template <int BLOCK, int RMAX, bool SEQ>
__device__ inline void small_dot2(const double (&prod0)[RMAX], const double (&prod1)[RMAX], int32_t n, double *pr0, double *pr1,
                                  double *red, double &out0, double &out1)
{
    if (!SEQ) {                                             // (each summed as small_dot sums it; the two share their barriers)
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int u = 0; u < RMAX; ++u)
            if ((int32_t)threadIdx.x + u * BLOCK < n) { a += prod0[u]; b += prod1[u]; }
        block_sum2<BLOCK>(a, b, red, out0, out1);
        return;
    }
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int32_t i = threadIdx.x + u * BLOCK;
        if (i < n) { pr0[i] = prod0[u]; pr1[i] = prod1[u]; }
    }
    __syncthreads();
    if (threadIdx.x < 128) {
        const int w = threadIdx.x >> 6;
        const double s = seq_chain_lds(w ? pr1 : pr0, n, 0.0);
        if ((threadIdx.x & 63) == 0) red[w] = s;
    }
    __syncthreads();
    out0 = red[0];
    out1 = red[1];
}

constexpr int kCgSmallMax = 10240;          // 10 rows per thread (sliced matrices): x, r, q in registers (16 rows: 53-168 spilled)
constexpr int kCgSmallMaxCsr = 4096;        // plain CSR arrays: 4 rows per thread (10 rows, n = 1e4: 19 us per iteration, one CU's address pipe)
constexpr int kCgSmallMaxSeq = 10200;       // dot_order = 1: p AND the parked products live in LDS (2 x 10200 doubles + scratch <= 160 KiB)
constexpr int kBiSmallMax = 4096;           // BiCGStab: seven vectors in registers, 4 rows per thread
// (a structured ELLPACK matrix with max_d <= 8 keeps the same sliced form, every slot an entry: its padding slots'
// 0.0 * x(last neighbour) terms are added like the reference's ellpack_matvec_add does)
static bool cg_small_sliced(const Part &p)
{
    return p.scode && p.sval && p.dict && p.opt.csr_sliced && (p.ecol ? p.opt.ell_offset_dict : p.opt.csr_offset_dict) && p.sw <= 8;
}
static bool small_applies(sgm_solver s, sgm_mat A, sgm_pc pc, bool bicg)
{
    if (!(bicg ? s->opt.bicgstab_small : s->opt.cg_small) || s->multi || A->parts.size() != 1 ||
        (A->fmt != SGM_FMT_CSR && A->fmt != SGM_FMT_ELL))
        return false;
    const Part &p = A->parts[0];
    if (p.n < 1 || p.n_halo != 0) return false;
    if (!cg_small_sliced(p) && (A->fmt != SGM_FMT_CSR || !p.rowptr || !p.col || !p.val)) return false;
    int32_t nmax = cg_small_sliced(p) ? kCgSmallMax : kCgSmallMaxCsr;
    if (s->seq) nmax = std::min(nmax, kCgSmallMaxSeq);
    if (bicg) nmax = std::min(nmax, kBiSmallMax);
    if (p.n > nmax) return false;
    // one CU takes about 2.5 us + 0.22 us per 1000 stored slots per iteration (5-point 80^2: 11.3 us, 100^2: 14.9; tridiagonal
    // n = 1e4: 11.0; 7-point 20^3: 16.2); the launch loop 14.3-14.7 whatever the size: beyond ~49k slots the loop it is
    // (BiCGStab: two products per iteration against five launches -- the same break-even)
    if ((cg_small_sliced(p) ? (int64_t)p.n * p.sw : p.nnz) > 49152) return false;
    const int pk = pc ? pc_kind(pc) : 0;
    return pk == 0 || pk == SGM_PC_JACOBI;
}
// more than 64 KiB of dynamic LDS needs the attribute, once per kernel; false = the runtime refused (the caller takes the
// launch loop instead)
static bool allow_lds(const void *fn, size_t bytes)
{
    static std::vector<std::pair<const void *, size_t>> done;
    for (auto &d : done)
        if (d.first == fn && d.second >= bytes) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    done.emplace_back(fn, bytes);
    return true;
}
// ---- CG on a mid-sized system: the whole solve in ONE launch of up to 256 co-resident workgroups ------------------------
// Between k_cg_small's reach (one workgroup, <= 10240 rows) and n ~ 1e6 (256 workgroups x 4096 rows) an iteration of the launch loop is three dependent
// kernels of ~4.4 us each, whatever the traffic (n = 1e5: 13.3 us for 1.4 us of bytes; n = 1e6: 36 us for 15).  Here the
// k_cg_small scheme is spread over G workgroups, one per CU: workgroup b owns RMAX * 1024 consecutive rows -- x and r in the
// registers of the row's thread, its part of p plus a halo of `H` rows either side in LDS, the matrix re-read from its sliced
// form every iteration (L2 / Infinity Cache hits at these sizes) -- and an iteration needs TWO grid-wide hand-offs:
//   (1) q = A p on the own rows, partial p.q -> slot[b]                     | arrive / wait | every workgroup adds the G partials
//   (2) r -= alpha q, z = M^-1 r, partial r.z -> slot[G + b]; the z of its     | arrive / wait | in the same order: same bits
//       first and last H rows -> a global vector                              |               | everywhere, no broadcast
//   (3) x += alpha p, p = z + beta p on the own rows AND on the halo (the neighbours' z from the global vector: the p halo
//       is kept up to date locally, no third hand-off)
// Hand-offs follow the guide's counter recipe (cdna_hip_programming.md section 6, Guideline 16): published doubles leave as sc1
// (agent-scope, write-through) stores, every wave drains its stores, the workgroup joins, lane 0 adds to ONE monotonic
// counter; waiters poll it with relaxed sc1 loads and read the published data with sc1 loads only.  Every wait is bounded:
// a workgroup that gives up raises `abort` -- nothing has been written to x, r, p by then -- and the host runs the launch
// loop instead (grids of <= 256 single-workgroup-per-CU blocks are co-resident on an otherwise idle GPU, but nothing
// promises it).  Same statements and operands as the launch loop / cg_solve (cg_solvers.f90:129-145); only the dot
// products' summation order differs (per-workgroup block sums, then the G partials in index order).
__device__ inline void st_sc1(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline double ld_sc1(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// a store that stays in the storing XCD's L2 (write-through from the CU's L1 like every store): what the XCD-local variant
// publishes with once every participant has proved to sit on ONE XCD, whose L2 is then the coherence point; readers keep
// their sc1 loads (L1 bypassed, served by that L2)
__device__ inline void st_l2(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void st_pub(double *p, double v, bool l2) { if (l2) st_l2(p, v); else st_sc1(p, v); }
__device__ inline int xcc_id()
{
    int v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(v));
    return v & 15;
}

// One grid-wide hand-off = one all-reduced scalar.  No counter and no atomic: workgroup b publishes its partial sum in
// slot[h % 4][b] (an sc1 store, after every wave has drained the sc1 stores of whatever else it publishes with this hand-off);
// thread t < G of EVERY workgroup polls slot[h % 4][t] with sc1 loads until it no longer holds the "not yet written"
// pattern (a NaN with a payload no arithmetic produces), and the block sum of the G values -- same order everywhere -- is the
// scalar.  A slot set is re-armed two hand-offs ahead of its reuse by its owners (slot[(h + 2) % 4][b] when b has passed
// h): every reader of that set's previous use arrived at hand-off h - 1 before anyone could pass it.  Bounded: a poll that
// gives up raises `abort`, and every poll loop looks at it.
constexpr unsigned long long kCoopPoison = 0x7ff8c0de5a5a0001ull;
// The slot sets exist in kCoopReplicas copies, kCoopRepStride doubles apart (lines -- and memory channels -- of their own): a
// publisher writes all of them with ONE wave instruction (lane k stores copy k), a workgroup polls the copy of its XCD.  With
// one copy, 256 workgroups re-reading the same 16 lines made a poll round a queue at one or two channels (2.3 us per
// all-CU hand-off against 0.4 inside one XCD).  Which copy a workgroup polls is a matter of speed only.
constexpr int kCoopReplicas = 8, kCoopRepStride = 4 * 256 + 32, kCoopSecond = kCoopReplicas * kCoopRepStride;      // (second scalar of a hand-off: a region of its own)
constexpr int kCoopSlotDoubles = 2 * kCoopSecond;
#ifdef SGM_COOP_PROBE
// tuning aid (-DSGM_COOP_PROBE builds only): where an iteration's time goes, in 10 ns ticks summed over the launch, as seen by
// thread 0 of workgroup 0.  [0..7] the phases of the iteration, [8..11] inside a hand-off, [15] iterations
static __device__ long long g_coop_probe[16];
#define PROBE_T(k) do { if (probing) { const long long t_ = wall_clock64(); pacc[k] += t_ - tlast; tlast = t_; } } while (0)
#else
#define PROBE_T(k) do { } while (0)
#endif
// NS scalars per hand-off (1, or 2: BiCGStab's t.s and t.t, r.r and r0.r): the second one travels through a slot region of its
// own, kCoopSecond doubles further on.  A kernel that ever carries two passes both_regions = true to EVERY hand-off it makes,
// so that both regions' sets are re-armed two hand-offs ahead whichever kind those hand-offs are.
template <int NS>
__device__ inline bool coop_handoff(double *slots /* replicas x 4 x 256, twice */, int h, double mine_a, double mine_b, int wg, int G, bool l2, int *abort,
                                    int spin_limit, double *red /* 16 doubles per scalar */, int *lds_ok, double *sum_a, double *sum_b, int reps,
                                    bool both_regions, long long *pacc = nullptr)
{
    static_assert(NS == 1 || NS == 2, "one or two scalars");
    // (reps = 1, the one-XCD variant: copy 0 only, for its proof of co-location too -- at most 32 pollers)
    const int my_rep = reps == 1 ? 0 : (xcc_id() & (kCoopReplicas - 1));
#ifdef SGM_COOP_PROBE
    const bool probing = NS == 1 && pacc != nullptr;
    long long tlast = probing ? wall_clock64() : 0;
#endif
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // this wave's sc1 stores (boundary rows) have left
    __syncthreads();
    PROBE_T(8);
    const int tid = threadIdx.x;
    double *set = slots + (h & 3) * 256;
    if (tid == 0) *lds_ok = 1;
    if (tid < reps) {
        st_pub(set + tid * kCoopRepStride + wg, mine_a, l2);
        if (NS == 2) st_pub(set + kCoopSecond + tid * kCoopRepStride + wg, mine_b, l2);
    }
    double va = 0.0, vb = 0.0;
    int ok = 1;
    if (tid < G) {
        int spins = 0;
        for (;;) {
            va = ld_sc1(set + my_rep * kCoopRepStride + tid);
            if (NS == 2) vb = ld_sc1(set + kCoopSecond + my_rep * kCoopRepStride + tid);
            if (__double_as_longlong(va) != (long long)kCoopPoison && (NS == 1 || __double_as_longlong(vb) != (long long)kCoopPoison)) break;
            if (++spins > spin_limit || ((spins & 31) == 0 && __hip_atomic_load(abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                __hip_atomic_store(abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = 0; va = 0.0; vb = 0.0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
    }
    PROBE_T(9);
    __syncthreads();                                         // (lds_ok = 1 is visible before anyone clears it)
    PROBE_T(10);
    if (!ok) *lds_ok = 0;
    double sa, sb = 0.0;
    if constexpr (NS == 1) sa = block_sum<1024>(va, red);             // (its barriers publish lds_ok)
    else block_sum2<1024>(va, vb, red, sa, sb);
    PROBE_T(11);
    if (tid < reps) {
        st_pub(slots + ((h + 2) & 3) * 256 + tid * kCoopRepStride + wg, __longlong_as_double((long long)kCoopPoison), l2);
        if (NS == 2 || both_regions) st_pub(slots + kCoopSecond + ((h + 2) & 3) * 256 + tid * kCoopRepStride + wg, __longlong_as_double((long long)kCoopPoison), l2);
    }
    *sum_a = sa;
    if (NS == 2) *sum_b = sb;
    return *lds_ok != 0;
}

// ---- what k_cg_coop and k_bicg_coop are made of besides the hand-offs (1024 threads, RMAX rows per thread: tid + u * 1024) ----
// The workgroup's place in the launch.  XL (one XCD): the grid is 8 x G workgroups, of which those with blockIdx % 8 == 0 --
// dealt to ONE XCD by the round-robin dispatch -- take part; the others are idle and leave at once, before anything else.
template <bool XL> __device__ inline bool coop_idle() { return XL && (blockIdx.x & 7) != 0; }
struct CoopGeom {
    int G, wg;                  // participants, this workgroup's number among them
    int32_t r0, r1;             // its rows
};
template <int RPW, bool XL>
__device__ inline CoopGeom coop_geom(int32_t n)
{
    CoopGeom g;
    g.G = XL ? (int)(gridDim.x >> 3) : (int)gridDim.x;
    g.wg = XL ? (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    g.r0 = g.wg * RPW;
    g.r1 = min(n, g.r0 + RPW);
    return g;
}
// the first / last H own rows of an own-row vector to an exchange vector (what the neighbours' halos are formed from)
template <int RMAX>
__device__ inline void coop_publish(double *dst, const double (&w)[RMAX], const CoopGeom &g, int32_t H, bool l2)
{
    const int tid = threadIdx.x;
#pragma unroll
    for (int u = 0; u < RMAX; ++u) {
        const int32_t li = tid + u * 1024, i = g.r0 + li;
        if (i < g.r1 && (li < H || i >= g.r1 - H)) st_pub(dst + i, w[u], l2);
    }
}
// this workgroup's part of a dot product (prod: 0.0 on the rows beyond r1), or of two that share their barriers
template <int RMAX>
__device__ inline double coop_dot(const double (&prod)[RMAX], double *red)
{
    double sacc = 0.0;
#pragma unroll
    for (int u = 0; u < RMAX; ++u) sacc += prod[u];
    return block_sum<1024>(sacc, red);
}
template <int RMAX>
__device__ inline void coop_dot2(const double (&pa)[RMAX], const double (&pb)[RMAX], double *red, double &sa, double &sb)
{
    double a = 0.0, c = 0.0;
#pragma unroll
    for (int u = 0; u < RMAX; ++u) { a += pa[u]; c += pb[u]; }
    block_sum2<1024>(a, c, red, sa, sb);
}
constexpr int kCoopSpinLimit = 1 << 19;       // polls (about a microsecond each) before a hand-off gives up
// sliced stencil matrix on one GPU, plain or Jacobi, tree-order dots, beyond the one-workgroup kernel and up to 256 workgroups
static bool coop_applies(sgm_solver s, sgm_mat A, sgm_pc pc, int *rmax_out, int *halo_out, bool *xl_out, bool bicg = false)
{
    if (!(bicg ? s->opt.bicgstab_small : s->opt.cg_small) || s->multi || s->seq || A->parts.size() != 1 || A->comm ||
        (A->fmt != SGM_FMT_CSR && A->fmt != SGM_FMT_ELL) || prof_on())
        return false;
    const Part &p = A->parts[0];
    // (an ELLPACK matrix in its sliced form is the same arrays: every slot an entry, padding = 0.0 x the last neighbour;
    //  its dictionary's unused entries are 0)
    const int ndict = p.ecol ? 15 : p.ndict;
    if (p.n_halo != 0 || !cg_small_sliced(p) || p.n < 2048 || ndict < 1 || ndict > 15) return false;        // (k_cg_small had its turn already)
    const int pk = pc ? pc_kind(pc) : 0;
    if (pk != 0 && pk != SGM_PC_JACOBI) return false;
    // the stencil's reach in rows (the largest |offset| of THIS matrix's dictionary, kept on the part where the dictionary is
    // built -- never cached on the solver: one handle may serve matrices of the same size and different stencils)
    const int H = (p.dict_reach + 1) & ~1;
    // option cg_coop_variant: low four bits = rows per thread pinned (1, 2, 4, 8; 0 = chosen by size), 16 = never the one-XCD variant
    const int force_rmax = s->opt.cg_coop_variant & 15;
    // XCD-local variant: the whole system on the <= 32 CUs of one XCD, 1, 2 or 3 rows per thread with the matrix in registers
    // (4 rows per thread stream the matrix through one XCD's L2 / fabric port: 8.6-9.8 us per iteration at n = 1e5 .. 1.3e5
    // where the all-CU variant with one row per thread takes ~8.5)
    const bool xl_off = (s->opt.cg_coop_variant & 16) != 0;
    *xl_out = false;
    if (!xl_off && !s->coop_xl_retired && g_rt.num_cu >= 64) {
        for (int rmax : {1, 2, 3, 4}) {
            if (force_rmax ? rmax != force_rmax : rmax == 4) continue;
            // (k_bicg_coop: 1, 2 or 4 rows per thread, and on one XCD only one -- two there take 17.6 us per iteration at
            //  n = 65536 where 64 workgroups of one row per thread on all CUs take 15.0)
            if (bicg && rmax != 1 && !force_rmax) continue;
            if (bicg && rmax == 3) continue;
            const int64_t rpw = (int64_t)rmax * 1024, G = (p.n + rpw - 1) / rpw;
            if (G > std::min(32, g_rt.num_cu / 8) || (rpw + (bicg ? 4 : 2) * H + 48 + (bicg && rmax >= 2 ? 2 * rpw : 0)) * 8 > 160 * 1024) continue;
            *rmax_out = rmax; *halo_out = H; *xl_out = true;
            return true;
        }
    }
    for (int rmax : {1, 2, 4, 8}) {
        if (force_rmax && rmax != force_rmax) continue;
        if (rmax == 8 && bicg) continue;                      // (CG only: r moves into LDS to make room)
        const int64_t rpw = (int64_t)rmax * 1024, G = (p.n + rpw - 1) / rpw;
        // one workgroup per CU (co-residency), LDS: p + halo + scratch <= 160 KiB.  (A halo wider than a workgroup's rows -- the
        // planes of a 3-D grid -- is fine: then every row is published, and the halo is read from several owners' rows.)
        if (G > std::min(256, g_rt.num_cu) || (rpw + (bicg ? 4 : 2) * H + 48 + ((bicg && rmax >= 2) ? 2 * rpw : rmax == 8 ? rpw : 0)) * 8 > 160 * 1024) continue;
        *rmax_out = rmax; *halo_out = H;
        return true;
    }
    return false;
}

// every slot of the cooperative kernels' exchange buffer "not yet written", abort word clear, hand-offs counted from 0
static int coop_arm(sgm_solver s, size_t n /* doubles of exchange vectors in front of the slots */)
{
    std::vector<unsigned long long> pat((size_t)kCoopSlotDoubles, kCoopPoison);
    SGM_HIP(hipMemcpyAsync(s->coop_buf + n, pat.data(), pat.size() * 8, hipMemcpyHostToDevice, g_rt.stream));
    SGM_HIP(hipMemsetAsync(s->coop_buf + n + (size_t)kCoopSlotDoubles, 0, 64, g_rt.stream));
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    s->coop_base = 0;
    return SGM_OK;
}

// ---- host: one driver for the four fast-path runners, kernel selection, the order small / cooperative / loop ---------------
// (Int<>, Flag<>, with_flag: sgm_internal.hpp)
// the slice widths with a matrix-in-registers kernel of their own: 3, 5, 7; everything else up to 8 takes the 8-slot one
template <class F> static bool with_slots(int sw, F &&f) { return sw == 3 ? f(Int<3>{}) : sw == 5 ? f(Int<5>{}) : sw == 7 ? f(Int<7>{}) : f(Int<8>{}); }

// What a cooperative solver tells the driver, and what the driver hands its launches
struct CoopRun {
    const char *name;           // "CG" / "BiCGStab": the two messages, and in lower case the trace line
    int per_iter;               // hand-offs per iteration (+ 1 at the start of a fresh solve, + 1 for the one-XCD form's proof)
    size_t nx;                  // doubles of exchange vectors in front of the slots
    int rmax; bool xl;
};
struct CoopArgs { double *gz = nullptr, *slots = nullptr; int *abort = nullptr; int h0 = 0, spin = 0; };
// A solve as launches of at most small_chunk() iterations: the reference's loop has no iteration cap; a launch has one, after
// which the solve continues in the next launch from the vectors and scalars the kernel parked in the solver's work area -- the
// host stays in control.  launch(it_end, resume, args) -> false: the kernel cannot be launched here (LDS request refused).
// *ran = false: that, or (co) a hand-off gave up -- the caller runs the next path from the caller's x.
template <class Launch>
static int run_chunked(sgm_solver s, sgm_mat A, double *x, const CoopRun *co, Launch &&launch, bool *ran)
{
    const size_t n = (size_t)A->parts[0].n;
    CoopArgs c;
    *ran = false;
    if (co) {
        if (!s->coop_buf) {
            if (dalloc(&s->coop_buf, co->nx + (size_t)kCoopSlotDoubles + 64) != SGM_OK) return SGM_OK;
            SGM_TRY(coop_arm(s, co->nx));
        }
        c.gz = s->coop_buf; c.slots = c.gz + co->nx;
        c.abort = reinterpret_cast<int *>(c.slots + (size_t)kCoopSlotDoubles);
        c.spin = s->opt.coop_spin_limit > 0 ? s->opt.coop_spin_limit : kCoopSpinLimit;
        // the caller's x, kept until the first launch has ended: a hand-off that gives up at the LAST join of a launch can leave
        // workgroups that passed it storing their rows of x while the others leave theirs -- an aborted first launch hands the
        // launch loop the caller's x again, not that mixture
        if (!s->x_backup) SGM_TRY(dalloc(&s->x_backup, n + 2));
        SGM_HIP(hipMemcpyAsync(s->x_backup, x, n * 8, hipMemcpyDeviceToDevice, g_rt.stream));
    }
    int flag = 0; int64_t iters = 0; double res = 0.0;
    for (int resume = 0;; resume = 1) {
        int64_t it_end = iters + s->small_chunk();
        if (s->max_iter > 0) it_end = std::min<int64_t>(it_end, s->max_iter);
        c.h0 = s->coop_base & 3;
        if (!launch(it_end, resume, c)) return SGM_OK;
        SGM_HIP(hipGetLastError());
        int habort = 0;
        if (co) SGM_HIP(hipMemcpyAsync(&habort, c.abort, sizeof(int), hipMemcpyDeviceToHost, g_rt.stream));
        SGM_TRY(read_state(s, &flag, &iters, &res));
        if (habort) {
            // a hand-off gave up (the grid was not co-resident, or the GPU is shared).  A resumed solve has moved x already:
            // restart is only exact from the caller's x, which is put back after a first launch
            SGM_TRY(coop_arm(s, co->nx));
            if (!resume) SGM_HIP(hipMemcpyAsync(x, s->x_backup, n * 8, hipMemcpyDeviceToDevice, g_rt.stream));
            if (co->xl) {
                // (the participants were not dealt to one XCD, or one of them never started: the all-CU variant has its turn)
                s->coop_xl_retired = true;
            } else {
                fprintf(stderr, "[sigma_hip] cooperative %s gave up waiting for a workgroup (grid not co-resident / shared GPU?): "
                                "this solver takes the launch loop from now on\n", co->name);
                s->coop_retired = true;
            }
            if (resume) return fail(SGM_ERR_HIP, "cooperative %s aborted in a continued launch", co->name);
            return SGM_OK;
        }
        if (co) {           // hand-offs this launch made; only their count mod 4 matters
            s->coop_base = (int)((s->coop_base + co->per_iter * (iters - (resume ? s->coop_iters0 : 0)) + (resume ? 0 : 1) + (co->xl ? 1 : 0)) & 3);
            s->coop_iters0 = iters;
        }
        if (flag || (s->max_iter > 0 && iters >= s->max_iter)) break;
    }
    *ran = true;
    store_result(s, flag, iters, res);
    if (co && trace_on()) {
        std::string lower(co->name);
        for (char &ch : lower) ch = (char)std::tolower((unsigned char)ch);
        const int64_t rpw = (int64_t)co->rmax * 1024;
        fprintf(stderr, "[sigma_hip] %s: one cooperative launch per %lld iterations, %s, %d workgroups x %lld rows\n", lower.c_str(),
                (long long)s->small_chunk(), co->xl ? "on one XCD" : "all CUs", (int)((n + rpw - 1) / rpw), (long long)rpw);
    }
    return SGM_OK;
}

// The fast paths in front of a launch loop, in their order.  One workgroup takes ~1.5 us + 0.22 us per 1000 stored slots per
// CG iteration (BiCGStab: 8.2 us at 5k slots, 12.9 at 20k), a few workgroups of one XCD ~5 us (BiCGStab ~10.7) whatever the
// size (round 4: tridiagonal n = 1e4 9.9 vs 5.0 us): the cooperative kernel first where it applies (>= 2048 rows) and the
// system has more than 12288 slots, then one workgroup, then the cooperative kernel if it has not had its turn.
// run_small(s, A, x, b, pc, ran), run_coop(s, A, x, b, pc, rmax, H, xl, ran); *ran = false: the caller runs its launch loop.
template <class Small, class Coop>
static int fast_paths(sgm_solver s, sgm_mat A, double *x, const double *b, sgm_pc pc, bool bicg, Small run_small, Coop run_coop, bool *ran)
{
    auto coop = [&]() -> int {
        int rmax = 0, H = 0;
        bool xl = false;
        *ran = false;
        for (int attempt = 0; attempt < 2 && !*ran && !s->coop_retired && coop_applies(s, A, pc, &rmax, &H, &xl, bicg); ++attempt) {
            SGM_TRY(run_coop(s, A, x, b, pc, rmax, H, xl, ran));
            if (!*ran && xl) s->coop_xl_retired = true;
            if (!xl) break;                                  // (the XCD-local variant stood down: once more with all CUs)
        }
        return SGM_OK;
    };
    bool coop_tried = false;
    *ran = false;
    if (small_applies(s, A, pc, bicg)) {
        const Part &p0 = A->parts[0];
        if ((cg_small_sliced(p0) ? (int64_t)p0.n * p0.sw : p0.nnz) > 12288) {
            coop_tried = true;
            SGM_TRY(coop());
            if (*ran) return SGM_OK;
        }
        SGM_TRY(run_small(s, A, x, b, pc, ran));
        if (*ran) return SGM_OK;
    }
    if (!coop_tried) SGM_TRY(coop());
    return SGM_OK;
}

}  // namespace sgm
