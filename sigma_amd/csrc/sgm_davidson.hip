// sgm_davidson, sgm_davidson_gen: the k smallest eigenpairs of A x = lambda x, or of A x = lambda B x (A symmetric, B symmetric
// positive definite), by the generalized Davidson method with thick restart and a caller's preconditioner.  One loop,
// sgm::davidson, serves both; B == nullptr is the standard problem and every place where the two differ is an `if (B)` there.
// The search space V and its image W = A V are resident in HBM; with B also U = B V: the space is orthogonalised in the B-inner
// product and no system with B is solved.  No reference counterpart: the contract is the two loops in include/sigma_hip.h,
// DESIGN.md sections 9h and 9i point to them, tests/davidson_restated.py and tests/davidson_gen_restated.py restate them.
// Compiled with -ffp-contract=off, no MFMA: every operation is rounded on its own.
//
// A step expands the space by the preconditioned residual of the first Ritz pair that has not converged (what B changes is
// marked *, and given after the bar):
//     t = M^-1 r                                                   pc_apply_parts (FCopy without a preconditioner)
//     partial sums of t.t (tau)                                    FDot2
//   * partial sums of h = V[:, 0..m-1]^T t ; h                     k_egs<KB, 0> ; k_eig_reduce            | U^T t
//   * t -= V h ; partial sums of g = V^T t ; g                     k_egs<KB, 1> ; k_eig_reduce            | k_egs2<KB>: g = U^T t
//     t -= V g ; partial sums of t.t (beta)                        k_egs<KB, 2>
//     tau, beta, 1.0 / beta ; the test beta > 2^-40 tau            k_dav_norm      (one workgroup)
//   *                                                                                                     | p = B t ; t.p (d) ; 1.0 / sqrt(d), the
//   *                                                                                                     | test d > 0: spmv_parts, FDot2, k_gdav_bnorm
//   * V_m = t * (1.0 / beta)                                       FEigScale                              | V_m = t / sqrt(d), U_m = p / sqrt(d)
//     W_m = A V_m                                                  spmv_parts
//     partial sums of H(0..m, m) = V[:, 0..m]^T W_m ; the column   k_egs<KB, 0> ; k_eig_reduce
//  -> the host: H's new column, tau, beta, the flag                synchronisation 1
//     symeig of the (m + 1) x (m + 1) matrix                       rayleigh_ritz (host)
//   * z -> the device ; r = W z - theta V z ; partial sums of r.r  k_dav_ritz                             | k_gdav_ritz: r = W z - theta U z ; r.r and p.p,
//     r.r                                                          k_eig_reduce                           | p = U z
//  -> the host: r.r                                                synchronisation 2 (once more per pair that converges in this step,
//                                                                  and per pair looked at again before "converged")
// Of the three Gram-Schmidt passes only the middle one reads two bases with B: the first takes dots alone (against U), the last
// corrects alone (with V), and both are k_egs itself.  k_dav_norm raises a device flag (1) when the new direction lies in the
// space or is not a number, k_gdav_bnorm (2) when not d > 0; the step's remaining kernels then return at once and the host
// leaves the loop at synchronisation 1.
#include "sgm_eigsh_device.hpp"
#include "sgm_symeig_host.hpp"

namespace sgm {

bool pc_serves(sgm_pc pc, sgm_mat A);       // sgm_pc.hip

// inv = 1.0 / sqrt(d), d the sum of the partial array dd ; not (d > 0): the flag becomes 2 (a NaN compares false too)
__global__ __launch_bounds__(kBlock) void k_gdav_bnorm(ScalarRef dd, DavDev *S)
{
    __shared__ double red[kBlock / 64];
    if (S->flag) return;
    const double d = load_scalar<kBlock>(dd, red);
    if (threadIdx.x != 0) return;
    S->inv = 1.0 / sqrt(d);
    if (!(d > 0.0)) S->flag = 2;
}

// k_egs<KB, 1> with two bases: w(i) = (..(w(i) - coef_0 q_0(i)) - ..) - coef_{kk-1} q_{kk-1}(i) over the columns of Q, then the
// partial sums of P^T w with the new w -> part_out[c * kMaxGrid + workgroup].  The same 16-byte accesses and the same thread to
// element map as k_egs, so every sum has its order.  The columns corrected with are not the columns dotted with: nothing is
// held between the two halves, each reads its basis in groups of 8 loads in flight (8 double2 live, not 2 KB of them), and one
// pass moves 8 n (2 kk + 2) bytes where k_egs with its columns held moves 8 n (kk + 2).
template <int KB>
__global__ __launch_bounds__(kBlock) void k_egs2(int64_t n, int kk, double *__restrict__ w, const double *__restrict__ Q,
                                                 const double *__restrict__ P, int64_t ld, const double *__restrict__ coef,
                                                 double *__restrict__ part_out, const int *flag)
{
    __shared__ double red[kBlock / 64];
    __shared__ double cl[KB];
    if (*flag) return;
    if (threadIdx.x < KB) cl[threadIdx.x] = (int)threadIdx.x < kk ? coef[threadIdx.x] : 0.0;
    __syncthreads();
    double acc[KB];
#pragma unroll
    for (int c = 0; c < KB; ++c) acc[c] = 0.0;
    const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t n2 = n >> 1;
    for (int64_t i = gtid; i < n2; i += stride) {
        double2 wv = ld2<false>(w, i);
#pragma unroll
        for (int c0 = 0; c0 < KB; c0 += 8) {
            if (c0 < kk) {                             // kk is uniform: every thread takes the same branches
                double2 qv[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < kk) qv[c] = ld2<true>(Q + (size_t)(c0 + c) * ld, i);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < kk) { wv.x = wv.x - cl[c0 + c] * qv[c].x; wv.y = wv.y - cl[c0 + c] * qv[c].y; }
            }
        }
        st2<false>(w, i, wv);
#pragma unroll
        for (int c0 = 0; c0 < KB; c0 += 8) {
            if (c0 < kk) {
                double2 pv[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < kk) pv[c] = ld2<true>(P + (size_t)(c0 + c) * ld, i);
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < kk) { acc[c0 + c] += pv[c].x * wv.x; acc[c0 + c] += pv[c].y * wv.y; }
            }
        }
    }
    if ((n & 1) && gtid == 0) {
        const int64_t i = n - 1;
        double wv = w[i];
        for (int c = 0; c < kk; ++c) wv = wv - cl[c] * Q[(size_t)c * ld + i];
        w[i] = wv;
#pragma unroll
        for (int c = 0; c < KB; ++c)
            if (c < kk) acc[c] += P[(size_t)c * ld + i] * wv;
    }
#pragma unroll
    for (int c = 0; c < KB; ++c)
        if (c < kk) {
            const double t = block_sum<kBlock>(acc[c], red);
            if (threadIdx.x == 0) part_out[(size_t)c * kMaxGrid + blockIdx.x] = t;
        }
}

static void launch_egs2(int64_t n, int kk, double *w, const double *Q, const double *P, int64_t ld, const double *coef, double *part,
                        const int *flag)
{
    with_width(kk, [&](auto KB) {
        hipLaunchKernelGGL(k_egs2<decltype(KB)::value>, dim3(dot_grid(n)), dim3(kBlock), 0, g_rt.stream, n, kk, w, Q, P, ld, coef, part,
                           flag);
    });
}

// The Ritz pass, one pass over the rows of two bases Y and X (n x m each, leading dimension ld, even): for row i
//     y = ((0.0 + Y(i,0) z_0) + Y(i,1) z_1) + ... ; x the same over X ; r(i) = y - theta * x
// r is stored, y and x are not; the partial sums of r.r go to part_rr and, with PP, those of x.x to part_pp, both in the order of
// k_egs (thread t of the grid dot_grid(n) takes the rows 2i, 2i+1 for i = t, t + threads, ..., thread 0 then the last row of an
// odd n).  z sits in LDS and is read as broadcasts; every column is read with 16-byte accesses, MB / 8 groups of 8 + 8 loads in
// flight per lane.  Compulsory traffic 8 n (2m + 1) bytes.
template <int MB, bool PP>
__device__ __forceinline__ void dav_ritz_body(int64_t n, int m, const double *__restrict__ Y, const double *__restrict__ X, int64_t ld,
                                              const double *__restrict__ z, double theta, double *__restrict__ r,
                                              double *__restrict__ part_rr, double *__restrict__ part_pp)
{
    __shared__ double red[(PP ? 2 : 1) * (kBlock / 64)];
    __shared__ double zl[MB];
    if (threadIdx.x < MB) zl[threadIdx.x] = (int)threadIdx.x < m ? z[threadIdx.x] : 0.0;
    __syncthreads();
    double acc_r = 0.0, acc_p = 0.0;
    const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t n2 = n >> 1;
    for (int64_t i = gtid; i < n2; i += stride) {
        double2 y = make_double2(0.0, 0.0), x = make_double2(0.0, 0.0);
#pragma unroll
        for (int c0 = 0; c0 < MB; c0 += 8) {
            if (c0 < m) {                              // m is uniform: every thread takes the same branches
                double2 yy[8], xx[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        yy[c] = ld2<true>(Y + (size_t)(c0 + c) * ld, i);
                        xx[c] = ld2<true>(X + (size_t)(c0 + c) * ld, i);
                    }
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        const double zc = zl[c0 + c];
                        y.x = y.x + yy[c].x * zc; y.y = y.y + yy[c].y * zc;
                        x.x = x.x + xx[c].x * zc; x.y = x.y + xx[c].y * zc;
                    }
            }
        }
        double2 rr;
        rr.x = y.x - theta * x.x; rr.y = y.y - theta * x.y;
        st2<false>(r, i, rr);
        acc_r += rr.x * rr.x; acc_r += rr.y * rr.y;
        if constexpr (PP) { acc_p += x.x * x.x; acc_p += x.y * x.y; }
    }
    if ((n & 1) && gtid == 0) {
        const int64_t i = n - 1;
        double y = 0.0, x = 0.0;
        for (int c = 0; c < m; ++c) {
            y = y + Y[(size_t)c * ld + i] * zl[c];
            x = x + X[(size_t)c * ld + i] * zl[c];
        }
        const double rv = y - theta * x;
        r[i] = rv;
        acc_r += rv * rv;
        if constexpr (PP) acc_p += x * x;
    }
    if constexpr (PP) {
        double sr, sp;
        block_sum2<kBlock>(acc_r, acc_p, red, sr, sp);
        if (threadIdx.x == 0) { part_rr[blockIdx.x] = sr; part_pp[blockIdx.x] = sp; }
    } else {
        const double t = block_sum<kBlock>(acc_r, red);
        if (threadIdx.x == 0) part_rr[blockIdx.x] = t;
    }
}

// the standard problem: r = W z - theta V z ; partial sums of r.r
template <int MB>
__global__ __launch_bounds__(kBlock) void k_dav_ritz(int64_t n, int m, const double *__restrict__ V, const double *__restrict__ W, int64_t ld,
                                                     const double *__restrict__ z, double theta, double *__restrict__ r,
                                                     double *__restrict__ part_out)
{
    dav_ritz_body<MB, false>(n, m, W, V, ld, z, theta, r, part_out, nullptr);
}

// with B: r = W z - theta U z ; partial sums of r.r and of p.p, p = U z
template <int MB>
__global__ __launch_bounds__(kBlock) void k_gdav_ritz(int64_t n, int m, const double *__restrict__ W, const double *__restrict__ U, int64_t ld,
                                                      const double *__restrict__ z, double theta, double *__restrict__ r,
                                                      double *__restrict__ part_rr, double *__restrict__ part_pp)
{
    dav_ritz_body<MB, true>(n, m, W, U, ld, z, theta, r, part_rr, part_pp);
}

// The counts of a call, as both info layouts take them
struct DavCounts {
    int64_t steps = 0, products = 0, products_b = 0, applies = 0, restarts = 0;
    int found = 0, converged = 0;
};

// The loop of both entry points, which have checked the arguments: B == nullptr is A x = lambda x.
static int davidson(sgm_mat A, sgm_mat B, sgm_pc pc, int32_t k, int32_t ncv, double tol, int32_t max_steps, const double *q1,
                    double *lambda_out, double *V_out, double *resid_out, int where, DavCounts &cnt)
{
    const int64_t n = A->nrow;
    const int64_t ld = (n + 1) & ~(int64_t)1;                     // even leading dimension: 16-byte aligned columns
    const int gd = dot_grid(n);
    struct Bufs {
        double *V = nullptr, *W = nullptr, *U = nullptr, *t = nullptr, *r = nullptr, *p = nullptr, *parts = nullptr, *slots = nullptr,
               *Z = nullptr;
        DavDev *S = nullptr;
        ~Bufs() { dfree(V); dfree(W); dfree(U); dfree(t); dfree(r); dfree(p); dfree(parts); dfree(slots); dfree(Z); dfree(S); }
    } b;
    SGM_TRY(dalloc(&b.V, (size_t)ld * ncv + 2));
    SGM_TRY(dalloc(&b.W, (size_t)ld * ncv + 2));
    SGM_TRY(dalloc(&b.t, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.r, (size_t)ld + 2));
    if (B) {                                                      // the third basis, p = B t and the partial sums of t.p: with B only
        SGM_TRY(dalloc(&b.U, (size_t)ld * ncv + 2));
        SGM_TRY(dalloc(&b.p, (size_t)ld + 2));
    }
    SGM_TRY(dalloc(&b.parts, (size_t)(kEigMaxNcv + (B ? 3 : 2)) * kMaxGrid));
    SGM_TRY(dalloc(&b.slots, (size_t)3 * kEigMaxNcv));
    SGM_TRY(dalloc(&b.Z, (size_t)kEigMaxNcv * kEigMaxNcv));
    SGM_TRY(dalloc(&b.S, 1));
    hipStream_t st = g_rt.stream;
    double *const bases[3] = {b.V, b.W, b.U}, *const vecs[3] = {b.t, b.r, b.p};
    const int nb = B ? 3 : 2;
    // every column of a basis is written (rows 0 .. n-1) before it is read, and no kernel reads past row n-1 (an odd n: its
    // last row alone, by one thread): only the pad row of an odd n is cleared, not 8 ld ncv bytes per basis
    if (ld > n)
        for (int i = 0; i < nb; ++i) SGM_HIP(hipMemset2DAsync(bases[i] + n, (size_t)ld * 8, 0, (size_t)(ld - n) * 8, ncv, st));
    for (int i = 0; i < nb; ++i) SGM_HIP(hipMemsetAsync(vecs[i], 0, ((size_t)ld + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.S, 0, sizeof(DavDev), st));
    double *hs = b.slots, *gs = b.slots + kEigMaxNcv, *rs = b.slots + 2 * kEigMaxNcv;
    double *P_WW = b.parts + (size_t)kEigMaxNcv * kMaxGrid, *P_TT = P_WW + kMaxGrid, *P_D = P_TT + kMaxGrid;      // (P_D: with B only)
    auto v = [&](int c) { return b.V + (size_t)c * ld; };
    auto w = [&](int c) { return b.W + (size_t)c * ld; };
    auto u = [&](int c) { return b.U + (size_t)c * ld; };
    const int *flag = &b.S->flag;
    const double *cx[1]; double *yy[1];
    auto product = [&](sgm_mat M, int64_t &count, const double *src, double *dst, const int *fl) -> int {
        cx[0] = src; yy[0] = dst;
        ++count;
        return spmv_parts(M, cx, yy, false, nullptr, fl, nullptr);
    };
    auto reduce = [&](int count, double *slots, const int *fl) {
        hipLaunchKernelGGL(k_eig_reduce, dim3(count), dim3(kBlock), 0, st, (const double *)b.parts, gd, slots, fl);
    };
    // Column c of the bases from the direction x and the 1.0 / norm in S->inv; fl: the flag the launches look at (none at the start)
    auto new_column = [&](int c, const double *x, const int *fl) -> int {
        if (B) {   // p = B x ; d = x.p ; 1.0 / sqrt(d) ; the d > 0 test, which raises the flag: whatever follows looks at it, at the start too
            SGM_TRY(product(B, cnt.products_b, x, b.p, fl));
            fl = flag;
            launch_elem(n, FDot2{x, b.p, nullptr, nullptr, P_D, nullptr}, fl);
            hipLaunchKernelGGL(k_gdav_bnorm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_D, gd}, b.S);
        }
        launch_elem(n, FEigScale{v(c), x, &b.S->inv}, fl);                        // V_c = x / |x|_2, with B x / sqrt(d)
        if (B) launch_elem(n, FEigScale{u(c), b.p, &b.S->inv}, fl);               // U_c = p / sqrt(d) = B V_c
        return product(A, cnt.products, v(c), w(c), fl);                          // W_c = A V_c
    };

    const int m_cap = ncv;
    std::vector<double> H((size_t)m_cap * m_cap, 0.0), theta(m_cap), Z((size_t)m_cap * m_cap), Zsel((size_t)m_cap * m_cap);
    std::vector<double> col(m_cap + 1), zc(m_cap);
    std::vector<int> order(m_cap);
    DavDev hd{};
    const int keep = std::min(k + (m_cap - k) / 2, m_cap - 1);
    double anorm = 0.0, rp[2] = {0.0, 0.0};
    int m = 1, locked = 0, found = 0, converged = 0;
    bool nan = false;

    // Zsel = the first `count` columns of Z in the Ritz order.  Without B as Jacobi leaves them.  With B each z divided by
    // sqrt(((0.0 + z_0 z_0) + z_1 z_1) + ...): Jacobi leaves |z|_2 = 1 only to a few tens of eps, and a rotation by such a z would
    // scale the B-norm of a kept column by |z|_2 at every restart
    auto select = [&](int count) {
        for (int i = 0; i < count; ++i) {
            const double *z = Z.data() + (size_t)order[i] * m;
            double *zs = Zsel.data() + (size_t)i * m;
            std::copy(z, z + m, zs);
            if (!B) continue;
            double s = 0.0;
            for (int r = 0; r < m; ++r) s = s + z[r] * z[r];
            const double nz = sqrt(s);
            for (int r = 0; r < m; ++r) zs[r] = z[r] / nz;
        }
    };

    {   // V_0 = q1 * (1.0 / sqrt(q1.q1)), or with B q1 / sqrt(q1.B q1) and U_0 = B V_0 ; W_0 = A V_0 ; H(0,0) = V_0.W_0
        Staged s1;
        SGM_TRY(stage_in(s1, q1, n, where, true));
        if (!B) {
            launch_elem(n, FDot2{s1.dev, s1.dev, nullptr, nullptr, P_WW, nullptr}, nullptr);
            hipLaunchKernelGGL(k_dav_norm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, ScalarRef{P_WW, gd}, 0, b.S);
        }
        SGM_TRY(new_column(0, s1.dev, nullptr));
        launch_egs<0>(n, 1, w(0), b.V, ld, nullptr, b.parts, flag);
        reduce(1, hs, B ? flag : nullptr);
        SGM_HIP(hipGetLastError());
        if (B) SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(DavDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(col.data(), hs, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // (the staged copy of q1 is released here)
        if (B && hd.flag) { --cnt.products; nan = true; }         // not (d > 0): W_0 returned at once
        H[0] = col[0];
    }

    while (!nan) {
        // Rayleigh-Ritz on the leading m x m block, smallest first
        nan = !rayleigh_ritz(m, H.data(), m_cap, theta.data(), Z.data(), order.data(), anorm, [](double a, double c2) { return a < c2; });
        if (nan) break;
        // r = the residual of the j-th Ritz pair in that order ; meets = (sqrt(r.r) <= tol * anorm), with B
        // (sqrt(r.r) <= (tol * anorm) * sqrt(p.p)), p = U z                                          (a NaN compares false)
        auto residual_meets = [&](int j, bool &meets) -> int {
            const int c = order[j];
            for (int i = 0; i < m; ++i) zc[i] = Z[i + (size_t)c * m];
            SGM_HIP(hipMemcpyAsync(b.Z, zc.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
            with_width(m, [&](auto MB) {
                constexpr int W_ = decltype(MB)::value;
                const dim3 grid(gd), block(kBlock);
                if (B)
                    hipLaunchKernelGGL(k_gdav_ritz<W_>, grid, block, 0, st, n, m, (const double *)b.W, (const double *)b.U, ld,
                                       (const double *)b.Z, theta[c], b.r, b.parts, b.parts + kMaxGrid);
                else
                    hipLaunchKernelGGL(k_dav_ritz<W_>, grid, block, 0, st, n, m, (const double *)b.V, (const double *)b.W, ld,
                                       (const double *)b.Z, theta[c], b.r, b.parts);
            });
            reduce(B ? 2 : 1, rs, nullptr);
            SGM_HIP(hipGetLastError());
            SGM_HIP(hipMemcpyAsync(rp, rs, B ? 16 : 8, hipMemcpyDeviceToHost, st));
            SGM_HIP(hipStreamSynchronize(st));                    // synchronisation 2 (zc is next written after it)
            meets = B ? sqrt(rp[0]) <= (tol * anorm) * sqrt(rp[1]) : sqrt(rp[0]) <= tol * anorm;
            return SGM_OK;
        };
        // the residual of the first pair that has not been locked; a pair that meets the test is locked and the next one looked at
        const int locked_before = locked;
        bool meets = false;
        while (locked < std::min<int>(k, m)) {
            SGM_TRY(residual_meets(locked, meets));
            if (meets) ++locked;
            else break;
        }
        if (locked == k) {
            // the pairs locked in earlier steps have been derived again since (a Ritz value that came down between two of
            // them has moved them on by one): they are looked at once more before the call says "converged"
            for (int j = 0; j < locked_before; ++j) {
                SGM_TRY(residual_meets(j, meets));
                if (!meets) { locked = j; break; }
            }
        }
        if (locked == k) { found = k; converged = 1; break; }
        if (locked == m) { found = m; break; }                    // every Ritz pair of a space smaller than k has converged
        if (cnt.steps == max_steps) { found = std::min<int>(k, m); break; }
        if (m == m_cap) {
            // thick restart: the first `keep` Ritz vectors in that order, in V and in W, and in U with B
            select(keep);
            SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * keep * 8, hipMemcpyHostToDevice, st));
            for (int i = 0; i < nb; ++i) launch_rotate(n, m, keep, bases[i], ld, b.Z);
            std::fill(H.begin(), H.end(), 0.0);
            for (int i = 0; i < keep; ++i) col[i] = theta[order[i]];
            std::fill(Z.begin(), Z.end(), 0.0);
            for (int i = 0; i < keep; ++i) {                      // the kept pairs are the space's Ritz pairs: theta_i, Z = I
                H[i + (size_t)i * m_cap] = theta[i] = col[i];
                Z[i + (size_t)i * keep] = 1.0;
                order[i] = i;
            }
            m = keep;
            ++cnt.restarts;                                       // (Zsel is next written after the step's synchronisation)
        }
        // expand: t = M^-1 r, twice orthogonalised against V[:, 0..m-1] -- with B in the B-inner product: the dots are against U
        if (pc) {
            const double *rv[1] = {b.r}; double *tv[1] = {b.t};
            SGM_TRY(pc_apply_parts(pc, A, rv, tv, nullptr));
            ++cnt.applies;
        } else
            launch_elem(n, FCopy{b.t, b.r}, nullptr);
        launch_elem(n, FDot2{b.t, b.t, nullptr, nullptr, P_TT, nullptr}, nullptr);
        launch_egs<0>(n, m, b.t, B ? b.U : b.V, ld, nullptr, b.parts, flag);
        reduce(m, hs, flag);
        // the middle pass stays two kernels: with its columns held, k_egs<KB, 1> moves half the bytes of k_egs2 with P = Q = V
        if (B) launch_egs2(n, m, b.t, b.V, b.U, ld, hs, b.parts, flag);
        else launch_egs<1>(n, m, b.t, b.V, ld, hs, b.parts, flag);
        reduce(m, gs, flag);
        launch_egs<2>(n, m, b.t, b.V, ld, gs, P_WW, flag);
        hipLaunchKernelGGL(k_dav_norm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, ScalarRef{P_TT, gd}, 1, b.S);
        SGM_TRY(new_column(m, b.t, flag));
        launch_egs<0>(n, m + 1, w(m), b.V, ld, nullptr, b.parts, flag);
        reduce(m + 1, hs, flag);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(DavDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(col.data(), hs, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // synchronisation 1
        // a step that ends at one of its tests counts none of its products (after the flag they returned at once); the flag is 2
        // with B alone: d is not positive, or not a number
        const bool notnum = hd.tau != hd.tau || hd.beta != hd.beta || (B && hd.flag == 2);
        if (notnum || hd.flag) {
            --cnt.products;
            if (B) --cnt.products_b;
        }
        if (notnum) { nan = true; break; }
        if (hd.flag) { found = std::min<int>(k, locked); break; }
        for (int i = 0; i <= m; ++i) H[i + (size_t)m * m_cap] = H[m + (size_t)i * m_cap] = col[i];
        ++m;
        ++cnt.steps;
    }

    if (nan) found = 0, converged = 0;
    // Vout = V[:, 0..m-1] Z[:, wanted] ; resid_i = sqrt(r.r), r = A v_i - lambda_i v_i, with B A v_i - lambda_i (B v_i)
    select(found);
    SGM_TRY(eig_hand_back(n, ld, m, k, found, b.V, Zsel.data(), b.Z, theta.data(), order.data(), b.parts, rs, lambda_out, V_out, resid_out,
                          where, [&](const double *vi, const double *&y, const double *&x) -> int {
                              y = b.t; x = vi;
                              SGM_TRY(product(A, cnt.products, vi, b.t, nullptr));
                              if (B) {                            // the B products of the true residuals are counted
                                  x = b.p;
                                  SGM_TRY(product(B, cnt.products_b, vi, b.p, nullptr));
                              }
                              return SGM_OK;
                          }));
    cnt.found = found;
    cnt.converged = converged;
    return SGM_OK;
}

}  // namespace sgm

extern "C" {

int sgm_davidson(sgm_mat A, sgm_pc pc, int32_t k, int32_t ncv, double tol, int32_t max_steps, const double *q1,
                 double *lambda_out, double *V_out, double *resid_out, int64_t *info, int where)
{
    SGM_TRY(require_init());
    if (!A || !q1 || !lambda_out || !resid_out || !info) return fail(SGM_ERR_BAD_ARG, "sgm_davidson: null argument");
    if (A->nrow != A->ncol) return fail(SGM_ERR_DIMS, "sgm_davidson: square matrices only (%d x %d)", A->nrow, A->ncol);
    if (A->distributed()) return fail(SGM_ERR_UNSUPPORTED, "sgm_davidson: row-partitioned and distributed matrices are not supported");
    const int64_t n = A->nrow;
    if (k < 1 || ncv <= k || ncv > kEigMaxNcv || ncv >= n || !(tol >= kEigTiny) || max_steps < 0)
        return fail(SGM_ERR_BAD_ARG, "sgm_davidson: needs 1 <= k < ncv <= 64, ncv < n, tol >= 2^-40, max_steps >= 0 "
                                     "(k %d, ncv %d, n %lld, tol %g, max_steps %d)", k, ncv, (long long)n, tol, max_steps);
    if (pc && !pc_serves(pc, A)) return fail(SGM_ERR_BAD_ARG, "sgm_davidson: the preconditioner has not been set up on this matrix");
    DavCounts c;
    SGM_TRY(davidson(A, nullptr, pc, k, ncv, tol, max_steps, q1, lambda_out, V_out, resid_out, where, c));
    info[0] = c.steps;
    info[1] = c.products;
    info[2] = c.applies;
    info[3] = c.restarts;
    info[4] = c.found;
    info[5] = c.converged;
    return SGM_OK;
}

int sgm_davidson_gen(sgm_mat A, sgm_mat B, sgm_pc pc, int32_t k, int32_t ncv, double tol, int32_t max_steps, const double *q1,
                     double *lambda_out, double *V_out, double *resid_out, int64_t *info, int where)
{
    SGM_TRY(require_init());
    if (!A || !B || !q1 || !lambda_out || !resid_out || !info) return fail(SGM_ERR_BAD_ARG, "sgm_davidson_gen: null argument");
    if (A->nrow != A->ncol || B->nrow != B->ncol || A->nrow != B->nrow)
        return fail(SGM_ERR_DIMS, "sgm_davidson_gen: square matrices of one size only (A %d x %d, B %d x %d)", A->nrow, A->ncol,
                    B->nrow, B->ncol);
    if (A->distributed() || B->distributed())
        return fail(SGM_ERR_UNSUPPORTED, "sgm_davidson_gen: row-partitioned and distributed matrices are not supported");
    const int64_t n = A->nrow;
    if (k < 1 || ncv <= k || ncv > kEigMaxNcv || ncv >= n || !(tol >= kEigTiny) || max_steps < 0)
        return fail(SGM_ERR_BAD_ARG, "sgm_davidson_gen: needs 1 <= k < ncv <= 64, ncv < n, tol >= 2^-40, max_steps >= 0 "
                                     "(k %d, ncv %d, n %lld, tol %g, max_steps %d)", k, ncv, (long long)n, tol, max_steps);
    if (pc && !pc_serves(pc, A)) return fail(SGM_ERR_BAD_ARG, "sgm_davidson_gen: the preconditioner has not been set up on A");
    DavCounts c;
    SGM_TRY(davidson(A, B, pc, k, ncv, tol, max_steps, q1, lambda_out, V_out, resid_out, where, c));
    info[0] = c.steps;
    info[1] = c.products;
    info[2] = c.products_b;
    info[3] = c.applies;
    info[4] = c.restarts;
    info[5] = c.found;
    info[6] = c.converged;
    return SGM_OK;
}

}  // extern "C"
