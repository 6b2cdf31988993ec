// Editing the values of a matrix that lives in HBM: ordered set / add batches, get, zero, scalar_multiply, add_sparse_matrix
// (src/matrix/sparse_matrix_interfaces.f90:106-128,378-460; CSR leaves cs_matrices.f90:709-724,840-966; ELLPACK leaves
// ellpack_matrices.f90:220-237,444-596), and the reusable plan that makes re-assembly on a fixed mesh one pass over the values.
//
// The contract: a batch of m triples (i_t, j_t, z_t) is processed as if the reference's scalar call were made for t = 1..m.
// Triple t addresses EVERY stored slot k of row i_t with node(k) == j_t (the reference's loops do not stop at the first match);
// an ELLPACK row is scanned over its first degrees(i) slots only.  set: a slot ends up with the z of the last triple addressing
// it.  add: ((v + z_a) + z_b) + ... over its triples in ascending t, every addition rounded on its own (-ffp-contract=off),
// no re-association, no tree, no atomics on values.  A triple that addresses no slot refuses the whole batch before any value is
// written (the reference would grow the pattern, default_sparse_matrix_kernels.f90:176-229).
//
// locate  one lane per triple scans a short row (edit_scan_row, sgm_plan_host.hpp: the statements the host planner runs); a
//         triple on a row of more than 32 slots is scanned by its whole wave.  Counts, an exclusive scan, then the hits
//         (slot, t) in ascending t; the smallest refused t by atomicMin.
// order   a STABLE radix sort of the hits by slot (hipCUB): every addressed slot's chain of sources in ascending t.
// layout  the addressed slots in ascending order, cut into groups of 64; a group stores the k-th source of each of its slots
//         adjacent in memory (position-major).  Position k holds only the slots whose chain is longer than k, compacted, behind
//         a 64-bit mask that says which lanes they are: a lane finds its source at the count of set bits below it, so a
//         group of mixed chain lengths (a finite-element row: 6 on the diagonal, 2 beside it) stores no padding at all --
//         the first, padded form of this layout (every position 64 wide, -1 for the short chains) stored 2.33 indices per
//         triple on the P1 grid.  A group's record: [W, W masks (lo, hi), the sources of position 0, of position 1, ...].
//         A chain longer than max(8, 4 x the group's mean) is kept out of the group, on the long-chain list.
// apply   one lane per addressed slot: contiguous 4-byte source reads, 8-byte gathers of z, one read-modify-write of val in
//         ascending slot order.  A long chain: its wave reads 64 sources at a time and adds them in order.
// Then the tail of sgm_csr_set_values / sgm_ell_set_values: kernel layouts refreshed, version bumped, transpose stale.
#include "sgm_spmv_select.hpp"
#include "sgm_plan_host.hpp"

#include <climits>

namespace sgm {

constexpr int kEditShortRow = 32;       // slots of a row one lane scans on its own

// the index arrays a batch is located in: CSR (0-based rowptr / col) or ELLPACK (slot-major ecol, degrees)
struct EditSrc {
    const int32_t *rowptr = nullptr, *col = nullptr, *edeg = nullptr;
    int32_t n = 0, ncol = 0, ell = 0;
};
struct EditRow { int64_t first, stride; int32_t steps; };
__device__ inline EditRow edit_row(const EditSrc &s, int32_t i)
{
    if (s.ell) return EditRow{i, s.n, s.edeg ? s.edeg[i] : 0};      // (no edeg: a matrix without slots, check_leaf saw to it)
    const int32_t lo = s.rowptr[i];
    return EditRow{lo, 1, s.rowptr[i + 1] - lo};
}

// FILL = false: cnt[t] = hits of triple t (cnt[m] = 0), flags[0] / [1] = smallest t + 1 out of range / without a slot.
// FILL = true: the hits of triple t at off[t].. : hslot = position in the value array, hsrc = t.
template <bool FILL>
__global__ __launch_bounds__(256) void k_edit_locate(EditSrc s, int64_t m, const int32_t *__restrict__ ti, const int32_t *__restrict__ tj,
                                                     int64_t *__restrict__ cnt, const int64_t *__restrict__ off,
                                                     uint32_t *__restrict__ hslot, uint32_t *__restrict__ hsrc,
                                                     unsigned long long *__restrict__ flags)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool valid = false, wide = false;
    EditRow r{0, 1, 0};
    int32_t key = -1;
    if (t < m) {
        const int32_t i = ti[t], j = tj[t];
        valid = i >= 1 && i <= s.n && j >= 1 && j <= s.ncol;
        if (valid) {
            r = edit_row(s, i - 1);
            key = j - 1;
            wide = r.steps > kEditShortRow;
        } else if (!FILL)
            atomicMin(&flags[0], (unsigned long long)t + 1);
    }
    const int32_t *node = s.col;
    int64_t w = FILL && t < m ? off[t] : 0;
    int32_t c = 0;
    if (valid && !wide)
        c = edit_scan_row(node, r.first, r.stride, r.steps, key, [&](int32_t u) {
            if (FILL) { hslot[w] = (uint32_t)(r.first + (int64_t)u * r.stride); hsrc[w] = (uint32_t)t; ++w; }
        });
    // rows too long for one lane: the wave takes them one after the other
    unsigned long long todo = __ballot(wide);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int64_t first = __shfl(r.first, l, 64), stride = __shfl(r.stride, l, 64), wl = __shfl(w, l, 64);
        const int32_t steps = __shfl(r.steps, l, 64), k = __shfl(key, l, 64);
        const int64_t tl = t - lane + l;
        int32_t run = 0;
        for (int32_t u0 = 0; u0 < steps; u0 += 64) {
            const int32_t u = u0 + lane;
            const bool hit = u < steps && node[first + (int64_t)u * stride] == k;
            const unsigned long long b = __ballot(hit);
            if (FILL && hit) {
                const int64_t pos = wl + run + __popcll(b & ((1ull << lane) - 1ull));
                hslot[pos] = (uint32_t)(first + (int64_t)u * stride);
                hsrc[pos] = (uint32_t)tl;
            }
            run += __popcll(b);
        }
        if (lane == l) c = run;
    }
    if (!FILL && t <= m) {
        cnt[t] = t < m ? c : 0;
        if (valid && c == 0) atomicMin(&flags[1], (unsigned long long)t + 1);
    }
}

// z_t = the value of the LAST stored slot of row i_t holding j_t, +0.0 if there is none (cs_matrices.f90:709-724); an index
// outside the matrix is flagged (flags[0] = smallest t + 1) and refused by the caller
__global__ void k_edit_get(EditSrc s, int64_t m, const int32_t *__restrict__ ti, const int32_t *__restrict__ tj,
                           const double *__restrict__ val, double *__restrict__ z, unsigned long long *__restrict__ flags)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int32_t i = ti[t], j = tj[t];
    if (i < 1 || i > s.n || j < 1 || j > s.ncol) { atomicMin(&flags[0], (unsigned long long)t + 1); z[t] = 0.0; return; }
    const EditRow r = edit_row(s, i - 1);
    double v = 0.0;
    edit_scan_row(s.col, r.first, r.stride, r.steps, j - 1, [&](int32_t u) { v = val[r.first + (int64_t)u * r.stride]; });
    z[t] = v;
}

__global__ void k_edit_heads(int64_t H, const uint32_t *__restrict__ key, int32_t *__restrict__ head)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < H) head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}
__global__ void k_edit_unique(int64_t H, const uint32_t *__restrict__ key, const int32_t *__restrict__ head, const int32_t *__restrict__ gid,
                              int32_t *__restrict__ uslot, int32_t *__restrict__ ustart, int64_t naddr)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) ustart[naddr] = (int32_t)H;
    if (p >= H || !head[p]) return;
    const int32_t g = gid[p] - 1;
    uslot[g] = (int32_t)key[p];
    ustart[g] = (int32_t)p;
}

// the width of a group of 64 addressed slots and which of its chains are long: the same in both passes
__device__ inline int32_t wave_max_i32(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline int32_t wave_sum_i32(int32_t v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int32_t edit_group_width(int32_t len, bool live, bool *is_long)
{
    const int32_t total = wave_sum_i32(live ? len : 0), count = wave_sum_i32(live ? 1 : 0);
    const int32_t mean = (total + count - 1) / max(count, 1);
    const int32_t cap = max(8, 4 * mean);
    *is_long = live && len > cap;
    return wave_max_i32(live && len <= cap ? len : 0);
}
// stats: [0] longest chain, [1] long chains, [2] their sources
__global__ __launch_bounds__(256) void k_edit_widths(int64_t naddr, const int32_t *__restrict__ ustart, int64_t *__restrict__ gw,
                                                     int32_t *__restrict__ lflag, unsigned long long *__restrict__ stats, int64_t ngrp)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < naddr;
    const int32_t len = live ? ustart[g + 1] - ustart[g] : 0;
    bool lg = false;
    const int32_t W = edit_group_width(len, live, &lg);
    const int32_t longest = wave_max_i32(len);
    const int32_t nl = wave_sum_i32(lg ? 1 : 0), sl = wave_sum_i32(lg ? len : 0), tot = wave_sum_i32(len);
    if (live) lflag[g] = lg ? 1 : 0;
    if ((threadIdx.x & 63) == 0) {
        const int64_t grp = g >> 6;
        if (grp < ngrp) gw[grp] = 1 + 2 * (int64_t)W + (tot - sl);       // W, W masks, the sources of the chains kept in the group
        if (grp == ngrp - 1) gw[ngrp] = 0;
        if (grp < ngrp) {
            atomicMax(&stats[0], (unsigned long long)longest);
            if (nl) { atomicAdd(&stats[1], (unsigned long long)nl); atomicAdd(&stats[2], (unsigned long long)sl); }
        }
    }
}
__global__ __launch_bounds__(256) void k_edit_fill_groups(int64_t naddr, const int32_t *__restrict__ ustart, const uint32_t *__restrict__ hsrc,
                                                          const int64_t *__restrict__ goff, int32_t *__restrict__ gsrc,
                                                          int32_t *__restrict__ ulast, int64_t ngrp)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t grp = g >> 6;
    if (grp >= ngrp) return;
    const int lane = threadIdx.x & 63;
    const bool live = g < naddr;
    const int32_t s0 = live ? ustart[g] : 0, len = live ? ustart[g + 1] - s0 : 0;
    bool lg = false;
    const int32_t W = edit_group_width(len, live, &lg);
    int32_t *rec = gsrc + goff[grp];
    int64_t p = 1 + 2 * (int64_t)W;
    if (lane == 0) rec[0] = W;
    for (int32_t k = 0; k < W; ++k) {
        const bool has = !lg && k < len;
        const unsigned long long mask = __ballot(has);
        if (lane == 0) { rec[1 + 2 * k] = (int32_t)(uint32_t)mask; rec[2 + 2 * k] = (int32_t)(uint32_t)(mask >> 32); }
        if (has) rec[p + __popcll(mask & ((1ull << lane) - 1ull))] = (int32_t)hsrc[s0 + k];
        p += __popcll(mask);
    }
    if (live) ulast[g] = (int32_t)hsrc[s0 + len - 1];
}

// ------------------------------------------------------------------ the hot path
// MODE 0 set, 1 add.  from_zero: every slot of the matrix is addressed and the batch starts from A%zero(): no read of val
template <int MODE>
__global__ __launch_bounds__(256) void k_edit_apply(int64_t naddr, const int32_t *__restrict__ uslot, const int64_t *__restrict__ goff,
                                                    const int32_t *__restrict__ gsrc, const int32_t *__restrict__ ulast,
                                                    const double *__restrict__ z, double *__restrict__ val, int from_zero)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= naddr) return;
    const int32_t slot = uslot[g];
    if (MODE == 0) {
        val[slot] = z[ulast[g]];
        return;
    }
    const int32_t *rec = gsrc + goff[g >> 6];
    const int32_t W = rec[0];
    const unsigned long long below = (1ull << (threadIdx.x & 63)) - 1ull, me = 1ull << (threadIdx.x & 63);
    const int32_t *src = rec + 1 + 2 * W;
    double v = from_zero ? 0.0 : val[slot];
    for (int32_t k = 0; k < W; ++k) {
        const unsigned long long mask = (unsigned long long)(uint32_t)rec[1 + 2 * k] | ((unsigned long long)(uint32_t)rec[2 + 2 * k] << 32);
        if (mask & me) v = v + z[src[__popcll(mask & below)]];          // val = val + z, in ascending t
        src += __popcll(mask);
    }
    val[slot] = v;
}
// long chains (add): one wave per chain, 64 sources staged in registers at a time and added in order
__global__ __launch_bounds__(256) void k_edit_apply_long(int32_t nlong, const int32_t *__restrict__ lg, const int32_t *__restrict__ uslot,
                                                         const int32_t *__restrict__ ustart, const int32_t *__restrict__ hsrc,
                                                         const double *__restrict__ z, double *__restrict__ val)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t q = blockIdx.x * 4 + wave;
    if (q >= nlong) return;                              // (whole waves leave together)
    const int32_t g = lg[q], s0 = ustart[g], len = ustart[g + 1] - s0;
    double v = val[uslot[g]];
    for (int32_t c = 0; c < len; c += 64) {
        const int32_t cn = min(64, len - c);
        const double zz = lane < cn ? z[hsrc[s0 + c + lane]] : 0.0;      // 64 sources, coalesced index reads
        for (int32_t k = 0; k < cn; ++k) v = v + __shfl(zz, k, 64);     // in order; every lane carries the same sum
    }
    if (lane == 0) val[uslot[g]] = v;
}

__global__ void k_edit_scale(int64_t n, double *__restrict__ v, double alpha, int zero)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) v[i] = zero ? 0.0 : alpha * v[i];
}

// B's stored entries in cursor order as triples: rows ascending, stored order inside a row, ELLPACK padding skipped
__global__ void k_edit_triples_of(EditSrc b, const int32_t *__restrict__ boff, const double *__restrict__ bval, int has_alpha, double alpha,
                                  int32_t *__restrict__ ti, int32_t *__restrict__ tj, double *__restrict__ tz)
{
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n) return;
    const EditRow r = edit_row(b, i);
    int64_t e = b.ell ? boff[i] : r.first;
    for (int32_t u = 0; u < r.steps; ++u, ++e) {
        const int64_t k = r.first + (int64_t)u * r.stride;
        ti[e] = i + 1;
        tj[e] = b.col[k] + 1;
        tz[e] = has_alpha ? alpha * bval[k] : bval[k];
    }
}

// ------------------------------------------------------------------ host side
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch() { for (void *p : ptrs) if (p) (void)hipFree(p); }
    template <class T> int get(T **p, size_t count) { SGM_TRY(dalloc(p, count)); ptrs.push_back(*p); return SGM_OK; }
};
static int bits_for(int64_t v) { int b = 1; while (b < 32 && (1ll << b) <= v) ++b; return b; }

// degrees: the call goes by an ELLPACK operand's degrees (every one but zero / scalar_multiply, which touch all slots alike)
static int check_leaf(const char *fn, sgm_mat A, const char *which = "A", bool degrees = true)
{
    if (!A) return fail(SGM_ERR_BAD_ARG, "%s: null matrix %s", fn, which);
    if (A->fmt == SGM_FMT_COMPOSITE) return fail(SGM_ERR_UNSUPPORTED, "%s: %s is a composite matrix (single-GPU CSR / ELLPACK leaves only)", fn, which);
    if (A->distributed()) return fail(SGM_ERR_UNSUPPORTED, "%s: %s is distributed / partitioned (single-GPU CSR / ELLPACK leaves only)", fn, which);
    if (A->fmt != SGM_FMT_CSR && A->fmt != SGM_FMT_ELL) return fail(SGM_ERR_UNSUPPORTED, "%s: unknown matrix format", fn);
    if (degrees && A->fmt == SGM_FMT_ELL) SGM_TRY(ell_need_degrees(fn, A->parts[0]));      // (never read as degree 0)
    return SGM_OK;
}
static int64_t slots_of(sgm_mat A) { const Part &p = A->parts[0]; return A->fmt == SGM_FMT_ELL ? (int64_t)p.n * p.max_d : p.nnz; }
static double *values_of(sgm_mat A) { Part &p = A->parts[0]; return A->fmt == SGM_FMT_ELL ? p.eval : p.val; }
static EditSrc src_of(sgm_mat A)
{
    const Part &p = A->parts[0];
    EditSrc s;
    s.n = A->nrow;
    s.ncol = A->ncol;
    if (A->fmt == SGM_FMT_ELL) { s.ell = 1; s.col = p.ecol; s.edeg = p.max_d ? p.edeg : nullptr; }
    else { s.rowptr = p.rowptr; s.col = p.col; }
    return s;
}
// the CSR-order arrays of a lean handle while an edit runs (released by the tail)
static int open_arrays(sgm_mat A, bool values_only)
{
    if (A->fmt != SGM_FMT_CSR) return SGM_OK;
    Part &p = A->parts[0];
    return values_only ? lean_val_buffer(p) : csr_need_arrays(p);
}
// how sgm_csr_set_values / sgm_ell_set_values end
static int edit_tail(sgm_mat A)
{
    Part &p = A->parts[0];
    A->t_stale = true;
    A->version += 1;
    if (slots_of(A) > 0) {
        SGM_TRY(pack_sliced(p));
        if (A->fmt == SGM_FMT_ELL) SGM_TRY(refresh_ell_colblock_values(p));
        else if (p.cb_P) SGM_TRY(refresh_ell_colblock_values(p));
    }
    if (A->fmt == SGM_FMT_CSR) csr_release_arrays(p);
    SGM_HIP(hipStreamSynchronize(g_rt.stream));
    return SGM_OK;
}

// caller arrays of a batch on the device
struct Batch {
    Scratch s;
    const int32_t *i = nullptr, *j = nullptr;
    const double *z = nullptr;
};
template <class T>
static int to_device(Scratch &s, const T *src, int64_t m, int where, const T **out)
{
    if (where == SGM_DEVICE || m == 0) { *out = src; return SGM_OK; }
    T *d = nullptr;
    SGM_TRY(s.get(&d, (size_t)m));
    SGM_HIP(hipMemcpyAsync(d, src, (size_t)m * sizeof(T), hipMemcpyHostToDevice, g_rt.stream));
    *out = d;
    return SGM_OK;
}

static void plan_free(sgm_edit_plan pl)
{
    if (!pl) return;
    dfree(pl->uslot); dfree(pl->ulast); dfree(pl->goff); dfree(pl->gsrc); dfree(pl->lg); dfree(pl->ustart); dfree(pl->hsrc);
    delete pl;
}

static int refuse(const char *fn, int which, unsigned long long t1, const int32_t *di, const int32_t *dj, sgm_mat A)
{
    int32_t ij[2] = {0, 0};
    SGM_HIP(hipMemcpy(&ij[0], di + (t1 - 1), 4, hipMemcpyDeviceToHost));
    SGM_HIP(hipMemcpy(&ij[1], dj + (t1 - 1), 4, hipMemcpyDeviceToHost));
    if (which == 0)
        return fail(SGM_ERR_DIMS, "%s: triple t = %llu addresses (%d, %d) outside the %d x %d matrix; nothing was changed", fn, t1, ij[0], ij[1],
                    A->nrow, A->ncol);
    return fail(SGM_ERR_UNSUPPORTED, "%s: triple t = %llu addresses (%d, %d), which is not a stored entry (the pattern is not grown); nothing was changed",
                fn, t1, ij[0], ij[1]);
}

// locate + order + layout; di / dj device arrays.  The matrix's index arrays must be open (open_arrays).
static int plan_build(const char *fn, sgm_edit_plan *out, sgm_mat A, int64_t m, const int32_t *di, const int32_t *dj)
{
    hipStream_t st = g_rt.stream;
    sgm_edit_plan pl = new sgm_edit_plan_s;
    struct Guard { sgm_edit_plan &p; ~Guard() { plan_free(p); } } guard{pl};
    pl->serial = A->serial;
    pl->pattern_version = A->pattern_version;
    pl->m = m;
    pl->nslots = slots_of(A);
    if (pl->nslots > INT32_MAX - 4) return fail(SGM_ERR_UNSUPPORTED, "%s: %lld value slots exceed int32", fn, (long long)pl->nslots);
    if (m > 0) {
        const EditSrc src = src_of(A);
        Scratch s;
        int64_t *off = nullptr;
        unsigned long long *flags = nullptr, hflags[2] = {~0ull, ~0ull};
        SGM_TRY(s.get(&off, (size_t)m + 1));
        SGM_TRY(s.get(&flags, 5));
        SGM_HIP(hipMemsetAsync(flags, 0xff, 16, st));
        SGM_HIP(hipMemsetAsync(flags + 2, 0, 24, st));
        const dim3 lgrid((unsigned)((m + 1 + 255) / 256)), blk(256);
        hipLaunchKernelGGL(k_edit_locate<false>, lgrid, blk, 0, st, src, m, di, dj, off, (const int64_t *)nullptr, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, flags);
        SGM_HIP(hipGetLastError());
        size_t tb = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, off, off, (int)(m + 1), st);
        char *tmp = nullptr;
        SGM_TRY(s.get(&tmp, std::max<size_t>(tb, 16)));
        SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, off, off, (int)(m + 1), st));
        int64_t H = 0;
        SGM_HIP(hipMemcpyAsync(&H, off + m, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(hflags, flags, 16, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
        if (hflags[0] != ~0ull) return refuse(fn, 0, hflags[0], di, dj, A);
        if (hflags[1] != ~0ull) return refuse(fn, 1, hflags[1], di, dj, A);
        if (H > INT32_MAX - 4) return fail(SGM_ERR_UNSUPPORTED, "%s: %lld (triple, slot) pairs exceed the int32 sort", fn, (long long)H);
        pl->hits = H;
        uint32_t *hslot = nullptr, *hslot2 = nullptr, *hsrc = nullptr, *hsrc2 = nullptr;
        int32_t *head = nullptr, *gid = nullptr;
        SGM_TRY(s.get(&hslot, (size_t)H)); SGM_TRY(s.get(&hslot2, (size_t)H));
        SGM_TRY(s.get(&hsrc, (size_t)H));
        SGM_TRY(dalloc(&hsrc2, (size_t)H));
        pl->hsrc = (int32_t *)hsrc2;
        hipLaunchKernelGGL(k_edit_locate<true>, lgrid, blk, 0, st, src, m, di, dj, (int64_t *)nullptr, (const int64_t *)off, hslot, hsrc,
                           (unsigned long long *)nullptr);
        SGM_HIP(hipGetLastError());
        size_t tbs = 0;
        const int end_bit = bits_for(std::max<int64_t>(pl->nslots, 1));
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tbs, hslot, hslot2, hsrc, hsrc2, (int)H, 0, end_bit, st);
        char *tmp2 = nullptr;
        SGM_TRY(s.get(&tmp2, std::max<size_t>(tbs, 16)));
        SGM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp2, tbs, hslot, hslot2, hsrc, hsrc2, (int)H, 0, end_bit, st));
        SGM_TRY(s.get(&head, (size_t)H)); SGM_TRY(s.get(&gid, (size_t)H));
        const dim3 hgrid((unsigned)((H + 255) / 256));
        hipLaunchKernelGGL(k_edit_heads, hgrid, blk, 0, st, H, (const uint32_t *)hslot2, head);
        size_t tb3 = 0;
        (void)hipcub::DeviceScan::InclusiveSum(nullptr, tb3, head, gid, (int)H, st);
        char *tmp3 = nullptr;
        SGM_TRY(s.get(&tmp3, std::max<size_t>(tb3, 16)));
        SGM_HIP(hipcub::DeviceScan::InclusiveSum(tmp3, tb3, head, gid, (int)H, st));
        int32_t naddr = 0;
        SGM_HIP(hipMemcpyAsync(&naddr, gid + H - 1, 4, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
        pl->naddr = naddr;
        const int64_t ngrp = ((int64_t)naddr + 63) / 64;
        int32_t *lflag = nullptr;
        SGM_TRY(dalloc(&pl->uslot, (size_t)naddr));
        SGM_TRY(dalloc(&pl->ulast, (size_t)naddr));
        SGM_TRY(dalloc(&pl->ustart, (size_t)naddr + 1));
        SGM_TRY(dalloc(&pl->goff, (size_t)ngrp + 1));
        SGM_TRY(s.get(&lflag, (size_t)naddr));
        hipLaunchKernelGGL(k_edit_unique, hgrid, blk, 0, st, H, (const uint32_t *)hslot2, (const int32_t *)head, (const int32_t *)gid, pl->uslot,
                           pl->ustart, (int64_t)naddr);
        const dim3 ggrid((unsigned)((ngrp * 64 + 255) / 256));
        hipLaunchKernelGGL(k_edit_widths, ggrid, blk, 0, st, (int64_t)naddr, (const int32_t *)pl->ustart, pl->goff, lflag, flags + 2, ngrp);
        SGM_HIP(hipGetLastError());
        size_t tb4 = 0;
        (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb4, pl->goff, pl->goff, (int)(ngrp + 1), st);
        char *tmp4 = nullptr;
        SGM_TRY(s.get(&tmp4, std::max<size_t>(tb4, 16)));
        SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp4, tb4, pl->goff, pl->goff, (int)(ngrp + 1), st));
        unsigned long long stats[3] = {0, 0, 0};
        SGM_HIP(hipMemcpyAsync(&pl->padded, pl->goff + ngrp, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(stats, flags + 2, 24, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));
        pl->longest = (int64_t)stats[0];
        pl->nlong = (int32_t)stats[1];
        pl->long_entries = (int64_t)stats[2];
        SGM_TRY(dalloc(&pl->gsrc, (size_t)pl->padded));
        hipLaunchKernelGGL(k_edit_fill_groups, ggrid, blk, 0, st, (int64_t)naddr, (const int32_t *)pl->ustart, (const uint32_t *)hsrc2,
                           (const int64_t *)pl->goff, pl->gsrc, pl->ulast, ngrp);
        SGM_HIP(hipGetLastError());
        if (pl->nlong > 0) {
            int32_t *nsel = nullptr;
            SGM_TRY(s.get(&nsel, 1));
            SGM_TRY(dalloc(&pl->lg, (size_t)pl->nlong));
            hipcub::CountingInputIterator<int32_t> ids(0);
            size_t tb5 = 0;
            (void)hipcub::DeviceSelect::Flagged(nullptr, tb5, ids, lflag, pl->lg, nsel, naddr, st);
            char *tmp5 = nullptr;
            SGM_TRY(s.get(&tmp5, std::max<size_t>(tb5, 16)));
            SGM_HIP(hipcub::DeviceSelect::Flagged(tmp5, tb5, ids, lflag, pl->lg, nsel, naddr, st));
        }
        SGM_HIP(hipStreamSynchronize(st));
        if (pl->nlong == 0) {                   // the sorted sources and chain starts serve the long list only
            dfree(pl->hsrc); pl->hsrc = nullptr;
            dfree(pl->ustart); pl->ustart = nullptr;
        }
    }
    if (trace_on())
        fprintf(stderr, "[sgm] %s: plan of %lld triples, %lld hits on %lld of %lld slots, longest chain %lld, %lld stored sources, %d long chains\n",
                fn, (long long)m, (long long)pl->hits, (long long)pl->naddr, (long long)pl->nslots, (long long)pl->longest,
                (long long)pl->padded, pl->nlong);
    *out = pl;
    pl = nullptr;
    return SGM_OK;
}

// the numeric pass on open arrays; dz on the device
static int plan_run(sgm_edit_plan pl, sgm_mat A, const double *dz, int mode, int zero_first)
{
    hipStream_t st = g_rt.stream;
    double *val = values_of(A);
    const bool all = pl->naddr == pl->nslots;
    const bool from_zero = zero_first && mode == SGM_EDIT_ADD && all && pl->nlong == 0;
    if (zero_first && !from_zero && !(mode == SGM_EDIT_SET && all) && pl->nslots > 0)
        hipLaunchKernelGGL(k_edit_scale, dim3(vec_grid(pl->nslots)), dim3(kBlock), 0, st, pl->nslots, val, 0.0, 1);
    if (pl->naddr > 0) {
        const dim3 g((unsigned)((pl->naddr + 255) / 256)), b(256);
        if (mode == SGM_EDIT_SET)
            hipLaunchKernelGGL(k_edit_apply<0>, g, b, 0, st, pl->naddr, (const int32_t *)pl->uslot, (const int64_t *)pl->goff,
                               (const int32_t *)pl->gsrc, (const int32_t *)pl->ulast, dz, val, 0);
        else
            hipLaunchKernelGGL(k_edit_apply<1>, g, b, 0, st, pl->naddr, (const int32_t *)pl->uslot, (const int64_t *)pl->goff,
                               (const int32_t *)pl->gsrc, (const int32_t *)pl->ulast, dz, val, from_zero ? 1 : 0);
        if (mode == SGM_EDIT_ADD && pl->nlong > 0)
            hipLaunchKernelGGL(k_edit_apply_long, dim3((unsigned)((pl->nlong + 3) / 4)), b, 0, st, pl->nlong, (const int32_t *)pl->lg,
                               (const int32_t *)pl->uslot, (const int32_t *)pl->ustart, (const int32_t *)pl->hsrc, dz, val);
    }
    SGM_HIP(hipGetLastError());
    return SGM_OK;
}

static int check_batch(const char *fn, int64_t m, const void *i, const void *j, const void *z, int where)
{
    if (m < 0 || (m && (!i || !j || !z)) || (where != SGM_HOST && where != SGM_DEVICE)) return fail(SGM_ERR_BAD_ARG, "%s: bad argument", fn);
    if (m > INT32_MAX - 4) return fail(SGM_ERR_UNSUPPORTED, "%s: m = %lld exceeds INT32_MAX - 4", fn, (long long)m);
    return SGM_OK;
}

// create + apply + destroy on device arrays
static int one_shot(const char *fn, sgm_mat A, int64_t m, const int32_t *di, const int32_t *dj, const double *dz, int mode)
{
    SGM_TRY(open_arrays(A, false));
    sgm_edit_plan pl = nullptr;
    int rc = plan_build(fn, &pl, A, m, di, dj);
    if (rc != SGM_OK) {                       // refused: nothing written, the handle as it was
        if (A->fmt == SGM_FMT_CSR) csr_release_arrays(A->parts[0]);
        return rc;
    }
    rc = plan_run(pl, A, dz, mode, 0);
    plan_free(pl);
    if (rc != SGM_OK) return rc;
    return edit_tail(A);
}
static int edit_entries(const char *fn, sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, const double *z, int where, int mode)
{
    SGM_TRY(require_init());
    SGM_TRY(check_leaf(fn, A));
    SGM_TRY(check_batch(fn, m, i, j, z, where));
    Batch b;
    SGM_TRY(to_device(b.s, i, m, where, &b.i));
    SGM_TRY(to_device(b.s, j, m, where, &b.j));
    SGM_TRY(to_device(b.s, z, m, where, &b.z));
    return one_shot(fn, A, m, b.i, b.j, b.z, mode);
}

}  // namespace sgm

using namespace sgm;

extern "C" {

int sgm_mat_set_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, const double *z, int where)
{
    return edit_entries("sgm_mat_set_entries", A, m, i, j, z, where, SGM_EDIT_SET);
}
int sgm_mat_add_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, const double *z, int where)
{
    return edit_entries("sgm_mat_add_entries", A, m, i, j, z, where, SGM_EDIT_ADD);
}

int sgm_mat_get_entries(sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, double *z_out, int where)
{
    const char *fn = "sgm_mat_get_entries";
    SGM_TRY(require_init());
    SGM_TRY(check_leaf(fn, A));
    SGM_TRY(check_batch(fn, m, i, j, z_out, where));
    if (m == 0) return SGM_OK;
    hipStream_t st = g_rt.stream;
    Batch b;
    SGM_TRY(to_device(b.s, i, m, where, &b.i));
    SGM_TRY(to_device(b.s, j, m, where, &b.j));
    double *dz = z_out;
    unsigned long long *flags = nullptr, hflag = ~0ull;
    if (where == SGM_HOST) SGM_TRY(b.s.get(&dz, (size_t)m));
    SGM_TRY(b.s.get(&flags, 1));
    SGM_HIP(hipMemsetAsync(flags, 0xff, 8, st));
    SGM_TRY(open_arrays(A, false));
    hipLaunchKernelGGL(k_edit_get, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, src_of(A), m, b.i, b.j, (const double *)values_of(A), dz, flags);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipMemcpyAsync(&hflag, flags, 8, hipMemcpyDeviceToHost, st));
    if (where == SGM_HOST) SGM_HIP(hipMemcpyAsync(z_out, dz, (size_t)m * 8, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));
    if (A->fmt == SGM_FMT_CSR) csr_release_arrays(A->parts[0]);
    if (hflag != ~0ull) return refuse(fn, 0, hflag, b.i, b.j, A);
    return SGM_OK;
}

static int scale_all(const char *fn, sgm_mat A, double alpha, int zero)
{
    SGM_TRY(require_init());
    SGM_TRY(check_leaf(fn, A, "A", false));
    SGM_TRY(open_arrays(A, zero != 0));
    const int64_t n = slots_of(A);
    if (n > 0) hipLaunchKernelGGL(k_edit_scale, dim3(vec_grid(n)), dim3(kBlock), 0, g_rt.stream, n, values_of(A), alpha, zero);
    SGM_HIP(hipGetLastError());
    return edit_tail(A);
}
int sgm_mat_zero(sgm_mat A) { return scale_all("sgm_mat_zero", A, 0.0, 1); }
int sgm_mat_scalar_multiply(sgm_mat A, double alpha) { return scale_all("sgm_mat_scalar_multiply", A, alpha, 0); }

int sgm_mat_add_matrix(sgm_mat A, sgm_mat B, const double *alpha_or_null)
{
    const char *fn = "sgm_mat_add_matrix";
    SGM_TRY(require_init());
    SGM_TRY(check_leaf(fn, A));
    SGM_TRY(check_leaf(fn, B, "B"));
    if (A->nrow != B->nrow || A->ncol != B->ncol)
        return fail(SGM_ERR_DIMS, "%s: shapes differ (%d x %d vs %d x %d)", fn, A->nrow, A->ncol, B->nrow, B->ncol);
    hipStream_t st = g_rt.stream;
    Scratch s;
    const Part &pb = B->parts[0];
    const bool ell = B->fmt == SGM_FMT_ELL;
    int32_t *boff = nullptr;
    int64_t m = pb.nnz;
    SGM_TRY(open_arrays(B, false));
    struct Release { sgm_mat B; ~Release() { if (B->fmt == SGM_FMT_CSR) csr_release_arrays(B->parts[0]); } } rel{B};
    if (ell) {
        m = 0;
        if (pb.n > 0 && pb.max_d > 0 && pb.edeg) {
            SGM_TRY(s.get(&boff, (size_t)pb.n + 1));
            size_t tb = 0;
            (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, pb.edeg, boff, pb.n, st);
            char *tmp = nullptr;
            SGM_TRY(s.get(&tmp, std::max<size_t>(tb, 16)));
            SGM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, tb, pb.edeg, boff, pb.n, st));
            int32_t last[2] = {0, 0};
            SGM_HIP(hipMemcpyAsync(&last[0], boff + pb.n - 1, 4, hipMemcpyDeviceToHost, st));
            SGM_HIP(hipMemcpyAsync(&last[1], pb.edeg + pb.n - 1, 4, hipMemcpyDeviceToHost, st));
            SGM_HIP(hipStreamSynchronize(st));
            m = (int64_t)last[0] + last[1];
        }
    }
    int32_t *ti = nullptr, *tj = nullptr;
    double *tz = nullptr;
    SGM_TRY(s.get(&ti, (size_t)m)); SGM_TRY(s.get(&tj, (size_t)m)); SGM_TRY(s.get(&tz, (size_t)m));
    if (m > 0)
        hipLaunchKernelGGL(k_edit_triples_of, dim3((unsigned)((B->nrow + 255) / 256)), dim3(256), 0, st, src_of(B), (const int32_t *)boff,
                           (const double *)values_of(B), alpha_or_null ? 1 : 0, alpha_or_null ? *alpha_or_null : 1.0, ti, tj, tz);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipStreamSynchronize(st));
    return one_shot(fn, A, m, ti, tj, tz, SGM_EDIT_ADD);
}

int sgm_edit_plan_create(sgm_edit_plan *out, sgm_mat A, int64_t m, const int32_t *i, const int32_t *j, int where)
{
    const char *fn = "sgm_edit_plan_create";
    SGM_TRY(require_init());
    if (!out) return fail(SGM_ERR_BAD_ARG, "%s: null output", fn);
    SGM_TRY(check_leaf(fn, A));
    SGM_TRY(check_batch(fn, m, i, j, i, where));
    Batch b;
    SGM_TRY(to_device(b.s, i, m, where, &b.i));
    SGM_TRY(to_device(b.s, j, m, where, &b.j));
    SGM_TRY(open_arrays(A, false));
    const int rc = plan_build(fn, out, A, m, b.i, b.j);
    if (A->fmt == SGM_FMT_CSR) csr_release_arrays(A->parts[0]);
    return rc;
}

int sgm_edit_plan_apply(sgm_edit_plan plan, sgm_mat A, const double *z, int mode, int zero_first, int where)
{
    const char *fn = "sgm_edit_plan_apply";
    SGM_TRY(require_init());
    if (!plan) return fail(SGM_ERR_BAD_ARG, "%s: null plan", fn);
    SGM_TRY(check_leaf(fn, A));
    if (mode != SGM_EDIT_SET && mode != SGM_EDIT_ADD) return fail(SGM_ERR_BAD_ARG, "%s: mode %d is neither SGM_EDIT_SET nor SGM_EDIT_ADD", fn, mode);
    SGM_TRY(check_batch(fn, plan->m, z, z, z, where));
    if (A->serial != plan->serial) return fail(SGM_ERR_BAD_ARG, "%s: the matrix is not the one the plan was created for", fn);
    if (A->pattern_version != plan->pattern_version)
        return fail(SGM_ERR_BAD_ARG, "%s: the matrix's pattern changed since the plan was created (permuted, or its ELLPACK degrees set)", fn);
    Batch b;
    SGM_TRY(to_device(b.s, z, plan->m, where, &b.z));
    // every slot rewritten from +0.0 or from z: the old values are not read, a lean handle needs only a buffer
    const bool fresh = zero_first || (mode == SGM_EDIT_SET && plan->naddr == plan->nslots);
    SGM_TRY(open_arrays(A, fresh));
    SGM_TRY(plan_run(plan, A, b.z, mode, zero_first));
    return edit_tail(A);
}

int sgm_edit_plan_info(sgm_edit_plan plan, int64_t *out4)
{
    if (!plan || !out4) return fail(SGM_ERR_BAD_ARG, "sgm_edit_plan_info: null argument");
    out4[0] = plan->m;
    out4[1] = plan->naddr;
    out4[2] = plan->longest;
    out4[3] = plan->padded + plan->long_entries;
    return SGM_OK;
}

int sgm_edit_plan_destroy(sgm_edit_plan plan)
{
    if (!plan) return fail(SGM_ERR_BAD_ARG, "sgm_edit_plan_destroy: null plan");
    plan_free(plan);
    return SGM_OK;
}

int sgm_edit_locate_host(int32_t nrow, int32_t ncol, const int32_t *ptr, const int32_t *node, int64_t m, const int32_t *i, const int32_t *j,
                         int64_t *hit_off, int32_t *hit_slot, int64_t capacity, int64_t *needed, int64_t *first_missing)
{
    return host_edit_locate_host(nrow, ncol, ptr, node, m, i, j, hit_off, hit_slot, capacity, needed, first_missing);
}

}  // extern "C"
