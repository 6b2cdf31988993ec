// Shared by the eigensolver translation units (sgm_eigsh.hip: thick-restart Lanczos, sgm_basis_rotate; sgm_davidson.hip:
// generalized Davidson for A x = lambda x and A x = lambda B x): the passes over a basis resident in HBM -- classical
// Gram-Schmidt with its dots, the re-reduction of their partial sums, the in-place rotation by a small matrix -- with_width,
// the one place where a column count picks a kernel's width, the two functors the loops end with, eig_hand_back, the end of
// every call (Ritz vectors, true residuals, the copies out), and what a Davidson step leaves for the host.  One definition, a
// copy per file (the library is built without relocatable device code): the non-template kernels are `static`.
#pragma once
#include "sgm_krylov.hpp"

namespace sgm {

constexpr int kEigMaxNcv = 64;
constexpr double kEigTiny = 9.094947017729282e-13;        // 2^-40: the invariant-subspace trigger and the smallest tol accepted

// The Gram-Schmidt passes over the columns 0 .. kk-1 (kk <= KB) of Q, 16-byte accesses, one accumulator per column and thread.
//   MODE 0:  partial sums of Q^T w                                            -> part_out[c * kMaxGrid + workgroup], c < kk
//   MODE 1:  w(i) = (..(w(i) - coef_0 q_0(i)) - ..) - coef_{kk-1} q_{kk-1}(i), columns ascending ; then as MODE 0 with the new w
//   MODE 2:  the same correction ; partial sums of w.w                       -> part_out[workgroup]
// Thread t of the grid adds the products of elements 2i, 2i+1 for i = t, t + threads, ... (thread 0 then the last element of an
// odd n): the order of every sum depends on n alone, the grid being dot_grid(n).
// HOLD: the columns stay in registers between the correction and the dots (kk <= 32); above that they are read again, by the
// thread that has just read them.
template <int KB, int MODE>
__global__ __launch_bounds__(kBlock) void k_egs(int64_t n, int kk, double *__restrict__ w, const double *__restrict__ Q, int64_t ldq,
                                                const double *__restrict__ coef, double *__restrict__ part_out, const int *flag)
{
    constexpr bool HOLD = KB <= 32;
    __shared__ double red[kBlock / 64];
    __shared__ double cl[KB];
    if (*flag) return;
    if (MODE != 0) {
        if (threadIdx.x < KB) cl[threadIdx.x] = (int)threadIdx.x < kk ? coef[threadIdx.x] : 0.0;
        __syncthreads();
    }
    constexpr int NACC = MODE == 2 ? 1 : KB;
    double acc[NACC];
#pragma unroll
    for (int c = 0; c < NACC; ++c) acc[c] = 0.0;
    const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t n2 = n >> 1;
    for (int64_t i = gtid; i < n2; i += stride) {
        double2 wv = ld2<false>(w, i);
        if constexpr (MODE == 1 && HOLD) {
            double2 vv[KB];
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < kk) vv[c] = ld2<true>(Q + (size_t)c * ldq, i);
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < kk) { wv.x = wv.x - cl[c] * vv[c].x; wv.y = wv.y - cl[c] * vv[c].y; }
            st2<false>(w, i, wv);
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < kk) { acc[c] += vv[c].x * wv.x; acc[c] += vv[c].y * wv.y; }
        } else {
            if constexpr (MODE != 0) {
#pragma unroll 8
                for (int c = 0; c < kk; ++c) {
                    const double2 v = ld2<MODE == 2>(Q + (size_t)c * ldq, i);
                    wv.x = wv.x - cl[c] * v.x; wv.y = wv.y - cl[c] * v.y;
                }
                st2<false>(w, i, wv);
            }
            if constexpr (MODE == 2) { acc[0] += wv.x * wv.x; acc[0] += wv.y * wv.y; }
            else {
#pragma unroll
                for (int c = 0; c < KB; ++c)
                    if (c < kk) {
                        const double2 v = ld2<true>(Q + (size_t)c * ldq, i);
                        acc[c] += v.x * wv.x; acc[c] += v.y * wv.y;
                    }
            }
        }
    }
    if ((n & 1) && gtid == 0) {
        const int64_t i = n - 1;
        double wv = w[i];
        if constexpr (MODE != 0) {
            for (int c = 0; c < kk; ++c) wv = wv - cl[c] * Q[(size_t)c * ldq + i];
            w[i] = wv;
        }
        if constexpr (MODE == 2) acc[0] += wv * wv;
        else {
#pragma unroll
            for (int c = 0; c < KB; ++c)
                if (c < kk) acc[c] += Q[(size_t)c * ldq + i] * wv;
        }
    }
    if constexpr (MODE == 2) {
        const double t = block_sum<kBlock>(acc[0], red);
        if (threadIdx.x == 0) part_out[blockIdx.x] = t;
    } else {
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c < kk) {                        // kk is uniform: every thread takes the same branches
                const double t = block_sum<kBlock>(acc[c], red);
                if (threadIdx.x == 0) part_out[(size_t)c * kMaxGrid + blockIdx.x] = t;
            }
    }
}

// workgroup c: slots[c] = the sum of partial array c (load_scalar's order: one array of `count` == 1 is the value itself)
static __global__ __launch_bounds__(kBlock) void k_eig_reduce(const double *parts, int count, double *slots, const int *flag)
{
    __shared__ double red[kBlock / 64];
    if (flag && *flag) return;
    const double d = load_scalar<kBlock>(ScalarRef{parts + (size_t)blockIdx.x * kMaxGrid, count}, red);
    if (threadIdx.x == 0) slots[blockIdx.x] = d;
}

// dst(i) = src(i) * s, s = *inv read on the device (the 1.0 / norm the step's own kernel left there)
struct FEigScale {
    static constexpr bool kDot = false;
    double *dst; const double *src; const double *inv; double s = 0.0;
    __device__ bool prepare(double *) { s = *inv; return true; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        double2 a = ld2<NT>(src, i); a.x = a.x * s; a.y = a.y * s; st2<NT>(dst, i, a);
    }
    __device__ void single(int64_t i) { dst[i] = src[i] * s; }
    __device__ void finish(double *) {}
};

// r(i) = y(i) - lambda * v(i) ; partial sums of r.r       (the true residual of one Ritz pair; r itself is not stored)
struct FEigResid {
    const double *y, *v; double lambda; double *part; double s = 0.0;
    __device__ bool prepare(double *) { return true; }
    __device__ void one(double yv, double vv) { const double r = yv - lambda * vv; s += r * r; }
    template <bool NT> __device__ void pair(int64_t i)
    {
        const double2 a = ld2<NT>(y, i), b = ld2<NT>(v, i);
        one(a.x, b.x); one(a.y, b.y);
    }
    __device__ void single(int64_t i) { one(y[i], v[i]); }
    __device__ void finish(double *red) { put_partial(s, part, red); }
};

// What a Davidson step leaves for the host (sgm_davidson.hip); lives in device memory and is read with H's new column
struct DavDev {
    double tau;                    // sqrt(t.t) before the orthogonalisation
    double beta;                   // sqrt(t.t) after it
    double inv;                    // 1.0 / beta (at the start: 1.0 / sqrt(q1.q1))
    int32_t flag;                  // nonzero: not (beta > 2^-40 tau) -- the step ends here
    int32_t pad;
};

// inv = 1.0 / sqrt(ww) ; with_tau: tau = sqrt(tt), beta = sqrt(ww) and the test of the step
static __global__ __launch_bounds__(kBlock) void k_dav_norm(ScalarRef ww, ScalarRef tt, int with_tau, DavDev *S)
{
    __shared__ double red[kBlock / 64];
    if (S->flag) return;
    const double d = load_scalar<kBlock>(ww, red);
    const double e = with_tau ? load_scalar<kBlock>(tt, red) : 0.0;
    if (threadIdx.x != 0) return;
    const double beta = sqrt(d);
    S->beta = beta;
    S->inv = 1.0 / beta;
    if (!with_tau) return;
    const double tau = sqrt(e);
    S->tau = tau;
    if (!(beta > kEigTiny * tau)) S->flag = 1;          // (a beta or tau that is not a number compares false too)
}

// Q[:, 0:kk] <- Q[:, 0:m] Z in place: one row per lane, the row's m entries in registers (every column is contiguous, so a wave
// reads 512 contiguous bytes per column), Z (m x kk, column-major) in LDS, read as broadcasts.  Output c of a row is
// ((0.0 + q_0 z_0c) + q_1 z_1c) + ..., ascending, and is written over input c only after the whole row has been read: the
// operation is row-local, so in place is safe.  Compulsory traffic 8 n (m + kk) bytes.
template <int MB>
__global__ __launch_bounds__(kBlock) void k_basis_rotate(int64_t n, int m, int kk, double *Q, int64_t ldq, const double *__restrict__ Z)
{
    __shared__ double Zl[kEigMaxNcv * kEigMaxNcv];
    for (int e = threadIdx.x; e < m * kk; e += kBlock) Zl[e] = Z[e];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += stride) {
        double q[MB];
#pragma unroll
        for (int r = 0; r < MB; ++r) q[r] = r < m ? Q[(size_t)r * ldq + row] : 0.0;
        for (int c = 0; c < kk; ++c) {
            const double *zc = Zl + c * m;
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < MB; ++r)
                if (r < m) s = s + q[r] * zc[r];
            Q[(size_t)c * ldq + row] = s;
        }
    }
}

// The width ladder: f is called once with Int<8 | 16 | 32 | 64>, the narrowest kernel width that holds m columns (m <= kEigMaxNcv;
// Int<>: sgm_internal.hpp)
template <class F> static void with_width(int m, F &&f)
{
    if (m <= 8) f(Int<8>{});
    else if (m <= 16) f(Int<16>{});
    else if (m <= 32) f(Int<32>{});
    else f(Int<64>{});
}

static void launch_rotate(int64_t n, int m, int kk, double *Q, int64_t ldq, const double *Zdev)
{
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + kBlock - 1) / kBlock, 8192));
    with_width(m, [&](auto MB) {
        hipLaunchKernelGGL(k_basis_rotate<decltype(MB)::value>, dim3(grid), dim3(kBlock), 0, g_rt.stream, n, m, kk, Q, ldq, Zdev);
    });
}

template <int MODE>
static void launch_egs(int64_t n, int kk, double *w, const double *Q, int64_t ldq, const double *coef, double *part, const int *flag)
{
    with_width(kk, [&](auto KB) {
        hipLaunchKernelGGL((k_egs<decltype(KB)::value, MODE>), dim3(dot_grid(n)), dim3(kBlock), 0, g_rt.stream, n, kk, w, Q, ldq, coef,
                           part, flag);
    });
}

// The end of a call.  lambda_out and resid_out (k each) are filled with NaN; with found > 0 then
//     Q[:, 0:found] <- Q[:, 0:m] Zsel (m x found, the caller's selection) ; lambda_i = theta[order[i]]
//     resid_i = sqrt(r.r), r = y - lambda_i x, where images(v_i, y, x) has launched what forms the pair's images and counted it
//     (y = A v_i ; x = v_i, or B v_i)
// -- one reduction of the `found` partial arrays in parts (re-reduced into rs), one synchronisation, the n x found block of Q
// copied to V_out when there is one.
template <class Images>
static int eig_hand_back(int64_t n, int64_t ld, int m, int k, int found, double *Q, const double *Zsel, double *Zdev, const double *theta,
                         const int *order, double *parts, double *rs, double *lambda_out, double *V_out, double *resid_out, int where,
                         Images &&images)
{
    hipStream_t st = g_rt.stream;
    const double qnan = std::nan("");
    for (int i = 0; i < k; ++i) lambda_out[i] = resid_out[i] = qnan;
    if (found <= 0) return SGM_OK;
    SGM_HIP(hipMemcpyAsync(Zdev, Zsel, (size_t)m * found * 8, hipMemcpyHostToDevice, st));
    launch_rotate(n, m, found, Q, ld, Zdev);
    for (int i = 0; i < found; ++i) {
        const double *y = nullptr, *x = nullptr;
        lambda_out[i] = theta[order[i]];
        SGM_TRY(images(Q + (size_t)i * ld, y, x));
        launch_elem(n, FEigResid{y, x, lambda_out[i], parts + (size_t)i * kMaxGrid}, nullptr);
    }
    hipLaunchKernelGGL(k_eig_reduce, dim3(found), dim3(kBlock), 0, st, (const double *)parts, dot_grid(n), rs, (const int *)nullptr);
    SGM_HIP(hipGetLastError());
    SGM_HIP(hipMemcpyAsync(resid_out, rs, (size_t)found * 8, hipMemcpyDeviceToHost, st));
    if (V_out)
        SGM_HIP(hipMemcpy2DAsync(V_out, (size_t)n * 8, Q, (size_t)ld * 8, (size_t)n * 8, found,
                                 where == SGM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    SGM_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < found; ++i) resid_out[i] = sqrt(resid_out[i]);
    return SGM_OK;
}

}  // namespace sgm
