// sgm_davidson_gen: the k smallest eigenpairs of A x = lambda B x (A symmetric, B symmetric positive definite) by the
// generalized Davidson method with thick restart and a caller's preconditioner, orthogonalised in the B-inner product.  The
// search space V and its images W = A V and U = B V are resident in HBM; no system with B is solved.  No reference counterpart:
// the contract is the loop in include/sigma_hip.h (sgm_davidson_gen), DESIGN.md section 9i points to it,
// tests/davidson_gen_restated.py restates it.  Compiled with -ffp-contract=off, no MFMA: every operation is rounded on its own.
//
// A step, after sgm_davidson.hip's (what differs is marked *):
//     t = M^-1 r                                                   pc_apply_parts (FCopy without a preconditioner)
//     partial sums of t.t (tau)                                    FDot2
//   * partial sums of h = U[:, 0..m-1]^T t ; h                     k_egs<KB, 0> on U ; k_eig_reduce
//   * t -= V h ; partial sums of g = U^T t ; g                     k_egs2<KB>        ; k_eig_reduce    corrects with V, dots with U
//     t -= V g ; partial sums of t.t (nu)                          k_egs<KB, 2> on V
//     tau, nu ; the test nu > 2^-40 tau                            k_dav_norm        (one workgroup)
//   * p = B t ; partial sums of t.p (d)                            spmv_parts ; FDot2
//   * 1.0 / sqrt(d) ; the test d > 0                               k_gdav_bnorm      (one workgroup)
//   * V_m = t * (1.0 / sqrt(d)) ; U_m = p * (1.0 / sqrt(d))        FEigScale, twice
//     W_m = A V_m                                                  spmv_parts
//     partial sums of H(0..m, m) = V[:, 0..m]^T W_m ; the column   k_egs<KB, 0> on V ; k_eig_reduce
//  -> the host: H's new column, tau, nu, the flag                  synchronisation 1
//     symeig of the (m + 1) x (m + 1) matrix                       symeig_jacobi (host)
//   * z -> the device ; r = W z - theta U z ; r.r and p.p          k_gdav_ritz ; k_eig_reduce
//  -> the host: r.r, p.p                                           synchronisation 2 (as sgm_davidson: once more per pair locked)
// Of the three Gram-Schmidt passes only the middle one reads two bases: the first takes dots alone (against U), the last
// corrects alone (with V), and both are k_egs itself.  The flag is 1 when the nu test fails and 2 when the d test fails.
#include "sgm_eigsh_device.hpp"
#include "sgm_symeig_host.hpp"

#include <numeric>

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
    const dim3 grid(dot_grid(n)), block(kBlock);
    if (kk <= 8) hipLaunchKernelGGL(k_egs2<8>, grid, block, 0, g_rt.stream, n, kk, w, Q, P, ld, coef, part, flag);
    else if (kk <= 16) hipLaunchKernelGGL(k_egs2<16>, grid, block, 0, g_rt.stream, n, kk, w, Q, P, ld, coef, part, flag);
    else if (kk <= 32) hipLaunchKernelGGL(k_egs2<32>, grid, block, 0, g_rt.stream, n, kk, w, Q, P, ld, coef, part, flag);
    else hipLaunchKernelGGL(k_egs2<64>, grid, block, 0, g_rt.stream, n, kk, w, Q, P, ld, coef, part, flag);
}

// k_dav_ritz over W and U (n x m each, leading dimension ld, even): for row i
//     y = ((0.0 + W(i,0) z_0) + W(i,1) z_1) + ... ; p the same over U ; r(i) = y - theta * p
// r is stored, y and p are not; the partial sums of r.r go to part_rr and those of p.p to part_pp, both in the order of k_egs.
// z sits in LDS and is read as broadcasts; every column is read with 16-byte accesses, MB / 8 groups of 8 + 8 loads in flight
// per lane.  Compulsory traffic 8 n (2m + 1) bytes, as k_dav_ritz.
template <int MB>
__global__ __launch_bounds__(kBlock) void k_gdav_ritz(int64_t n, int m, const double *__restrict__ W, const double *__restrict__ U, int64_t ld,
                                                      const double *__restrict__ z, double theta, double *__restrict__ r,
                                                      double *__restrict__ part_rr, double *__restrict__ part_pp)
{
    __shared__ double red[2 * (kBlock / 64)];
    __shared__ double zl[MB];
    if (threadIdx.x < MB) zl[threadIdx.x] = (int)threadIdx.x < m ? z[threadIdx.x] : 0.0;
    __syncthreads();
    double acc_r = 0.0, acc_p = 0.0;
    const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t n2 = n >> 1;
    for (int64_t i = gtid; i < n2; i += stride) {
        double2 y = make_double2(0.0, 0.0), p = make_double2(0.0, 0.0);
#pragma unroll
        for (int c0 = 0; c0 < MB; c0 += 8) {
            if (c0 < m) {                              // m is uniform: every thread takes the same branches
                double2 ww[8], uu[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        ww[c] = ld2<true>(W + (size_t)(c0 + c) * ld, i);
                        uu[c] = ld2<true>(U + (size_t)(c0 + c) * ld, i);
                    }
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        const double zc = zl[c0 + c];
                        y.x = y.x + ww[c].x * zc; y.y = y.y + ww[c].y * zc;
                        p.x = p.x + uu[c].x * zc; p.y = p.y + uu[c].y * zc;
                    }
            }
        }
        double2 rr;
        rr.x = y.x - theta * p.x; rr.y = y.y - theta * p.y;
        st2<false>(r, i, rr);
        acc_r += rr.x * rr.x; acc_r += rr.y * rr.y;
        acc_p += p.x * p.x; acc_p += p.y * p.y;
    }
    if ((n & 1) && gtid == 0) {
        const int64_t i = n - 1;
        double y = 0.0, p = 0.0;
        for (int c = 0; c < m; ++c) {
            y = y + W[(size_t)c * ld + i] * zl[c];
            p = p + U[(size_t)c * ld + i] * zl[c];
        }
        const double rv = y - theta * p;
        r[i] = rv;
        acc_r += rv * rv;
        acc_p += p * p;
    }
    double sr, sp;
    block_sum2<kBlock>(acc_r, acc_p, red, sr, sp);
    if (threadIdx.x == 0) { part_rr[blockIdx.x] = sr; part_pp[blockIdx.x] = sp; }
}

static void launch_gritz(int64_t n, int m, const double *W, const double *U, int64_t ld, const double *z, double theta, double *r,
                         double *part_rr, double *part_pp)
{
    const dim3 grid(dot_grid(n)), block(kBlock);
    if (m <= 8) hipLaunchKernelGGL(k_gdav_ritz<8>, grid, block, 0, g_rt.stream, n, m, W, U, ld, z, theta, r, part_rr, part_pp);
    else if (m <= 16) hipLaunchKernelGGL(k_gdav_ritz<16>, grid, block, 0, g_rt.stream, n, m, W, U, ld, z, theta, r, part_rr, part_pp);
    else if (m <= 32) hipLaunchKernelGGL(k_gdav_ritz<32>, grid, block, 0, g_rt.stream, n, m, W, U, ld, z, theta, r, part_rr, part_pp);
    else hipLaunchKernelGGL(k_gdav_ritz<64>, grid, block, 0, g_rt.stream, n, m, W, U, ld, z, theta, r, part_rr, part_pp);
}

}  // namespace sgm

extern "C" {

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
    SGM_TRY(dalloc(&b.U, (size_t)ld * ncv + 2));
    SGM_TRY(dalloc(&b.t, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.r, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.p, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.parts, (size_t)(kEigMaxNcv + 3) * kMaxGrid));
    SGM_TRY(dalloc(&b.slots, (size_t)3 * kEigMaxNcv));
    SGM_TRY(dalloc(&b.Z, (size_t)kEigMaxNcv * kEigMaxNcv));
    SGM_TRY(dalloc(&b.S, 1));
    hipStream_t st = g_rt.stream;
    // as sgm_davidson: every column is written (rows 0 .. n-1) before it is read and no kernel reads past row n-1, so only
    // the pad row of an odd n is cleared
    if (ld > n)
        for (double *Q : {b.V, b.W, b.U}) SGM_HIP(hipMemset2DAsync(Q + n, (size_t)ld * 8, 0, (size_t)(ld - n) * 8, ncv, st));
    for (double *x : {b.t, b.r, b.p}) SGM_HIP(hipMemsetAsync(x, 0, ((size_t)ld + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.S, 0, sizeof(DavDev), st));
    double *hs = b.slots, *gs = b.slots + kEigMaxNcv, *rs = b.slots + 2 * kEigMaxNcv;
    double *P_WW = b.parts + (size_t)kEigMaxNcv * kMaxGrid, *P_TT = P_WW + kMaxGrid, *P_D = P_TT + kMaxGrid;
    auto v = [&](int c) { return b.V + (size_t)c * ld; };
    auto w = [&](int c) { return b.W + (size_t)c * ld; };
    auto u = [&](int c) { return b.U + (size_t)c * ld; };
    const int *flag = &b.S->flag;
    const double *cx[1]; double *yy[1];
    int64_t products = 0, products_b = 0, applies = 0, steps = 0, restarts = 0;
    auto product = [&](sgm_mat M, int64_t &count, const double *src, double *dst, const int *fl) -> int {
        cx[0] = src; yy[0] = dst;
        ++count;
        return spmv_parts(M, cx, yy, false, nullptr, fl, nullptr);
    };
    auto reduce = [&](int count, double *slots, const int *fl) {
        hipLaunchKernelGGL(k_eig_reduce, dim3(count), dim3(kBlock), 0, st, (const double *)b.parts, gd, slots, fl);
    };
    // d = x.y ; 1.0 / sqrt(d) ; the d > 0 test ; V_c = x / sqrt(d) ; U_c = y / sqrt(d) ; W_c = A V_c        (y = B x)
    auto new_column = [&](int c, const double *x, const double *y) -> int {
        launch_elem(n, FDot2{x, y, nullptr, nullptr, P_D, nullptr}, flag);
        hipLaunchKernelGGL(k_gdav_bnorm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_D, gd}, b.S);
        launch_elem(n, FEigScale{v(c), x, &b.S->inv}, flag);
        launch_elem(n, FEigScale{u(c), y, &b.S->inv}, flag);
        return product(A, products, v(c), w(c), flag);
    };

    const int m_cap = ncv;
    std::vector<double> H((size_t)m_cap * m_cap, 0.0), Hb, theta(m_cap), Z((size_t)m_cap * m_cap), Zsel((size_t)m_cap * m_cap);
    std::vector<double> col(m_cap + 1), zc(m_cap);
    std::vector<int> order(m_cap);
    DavDev hd;
    const int keep = std::min(k + (m_cap - k) / 2, m_cap - 1);
    double anorm = 0.0, rp[2] = {0.0, 0.0};
    int m = 1, locked = 0, found = 0, converged = 0;
    bool nan = false;

    // Zsel = the first `count` columns of Z in the Ritz order, each z divided by sqrt(((0.0 + z_0 z_0) + z_1 z_1) + ...): Jacobi
    // leaves |z|_2 = 1 only to a few tens of eps, and a rotation by such a z would scale the B-norm of a kept column by |z|_2
    // at every restart
    auto select = [&](int count) {
        for (int i = 0; i < count; ++i) {
            const double *z = Z.data() + (size_t)order[i] * m;
            double s = 0.0;
            for (int r = 0; r < m; ++r) s = s + z[r] * z[r];
            const double nz = sqrt(s);
            for (int r = 0; r < m; ++r) Zsel[r + (size_t)i * m] = z[r] / nz;
        }
    };

    {   // p = B q1 ; d = q1.p ; V_0 = q1 / sqrt(d) ; U_0 = p / sqrt(d) ; W_0 = A V_0 ; H(0,0) = V_0.W_0
        Staged s1;
        SGM_TRY(stage_in(s1, q1, n, where, true));
        SGM_TRY(product(B, products_b, s1.dev, b.p, nullptr));
        SGM_TRY(new_column(0, s1.dev, b.p));
        launch_egs<0>(n, 1, w(0), b.V, ld, nullptr, b.parts, flag);
        reduce(1, hs, flag);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(DavDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(col.data(), hs, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // (the staged copy of q1 is released here)
        if (hd.flag) { --products; nan = true; }                  // not (d > 0): W_0 returned at once
        H[0] = col[0];
    }

    while (!nan) {
        // Rayleigh-Ritz on the leading m x m block
        Hb.assign((size_t)m * m, 0.0);
        for (int jc = 0; jc < m; ++jc)
            for (int i = 0; i < m; ++i) {
                Hb[i + (size_t)jc * m] = H[i + (size_t)jc * m_cap];
                if (Hb[i + (size_t)jc * m] != Hb[i + (size_t)jc * m]) nan = true;
            }
        if (nan) break;
        symeig_jacobi(m, Hb.data(), theta.data(), Z.data());
        for (int i = 0; i < m; ++i) {
            if (theta[i] != theta[i]) nan = true;
            if (fabs(theta[i]) > anorm) anorm = fabs(theta[i]);
        }
        if (nan) break;
        std::iota(order.begin(), order.begin() + m, 0);
        std::stable_sort(order.begin(), order.begin() + m, [&](int a, int c2) { return theta[a] < theta[c2]; });
        // r = the residual of the j-th Ritz pair in that order ; meets = (sqrt(r.r) <= (tol * anorm) * sqrt(p.p))
        auto residual_meets = [&](int j, bool &meets) -> int {
            const int c = order[j];
            for (int i = 0; i < m; ++i) zc[i] = Z[i + (size_t)c * m];
            SGM_HIP(hipMemcpyAsync(b.Z, zc.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
            launch_gritz(n, m, b.W, b.U, ld, b.Z, theta[c], b.r, b.parts, b.parts + kMaxGrid);
            reduce(2, rs, nullptr);
            SGM_HIP(hipGetLastError());
            SGM_HIP(hipMemcpyAsync(rp, rs, 16, hipMemcpyDeviceToHost, st));
            SGM_HIP(hipStreamSynchronize(st));                    // synchronisation 2 (zc is next written after it)
            meets = sqrt(rp[0]) <= (tol * anorm) * sqrt(rp[1]);   // (a NaN compares false)
            return SGM_OK;
        };
        const int locked_before = locked;
        bool meets = false;
        while (locked < std::min<int>(k, m)) {
            SGM_TRY(residual_meets(locked, meets));
            if (meets) ++locked;
            else break;
        }
        if (locked == k) {                                        // the second look at the pairs locked earlier, as sgm_davidson
            for (int j = 0; j < locked_before; ++j) {
                SGM_TRY(residual_meets(j, meets));
                if (!meets) { locked = j; break; }
            }
        }
        if (locked == k) { found = k; converged = 1; break; }
        if (locked == m) { found = m; break; }
        if (steps == max_steps) { found = std::min<int>(k, m); break; }
        if (m == m_cap) {
            // thick restart: the first `keep` Ritz vectors in that order, in V, in W and in U
            select(keep);
            SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * keep * 8, hipMemcpyHostToDevice, st));
            for (double *Q : {b.V, b.W, b.U}) launch_rotate(n, m, keep, Q, ld, b.Z);
            std::fill(H.begin(), H.end(), 0.0);
            for (int i = 0; i < keep; ++i) col[i] = theta[order[i]];
            std::fill(Z.begin(), Z.end(), 0.0);
            for (int i = 0; i < keep; ++i) {
                H[i + (size_t)i * m_cap] = theta[i] = col[i];
                Z[i + (size_t)i * keep] = 1.0;
                order[i] = i;
            }
            m = keep;
            ++restarts;                                           // (Zsel is next written after the step's synchronisation)
        }
        // expand: t = M^-1 r, twice orthogonalised against the space in the B-inner product
        if (pc) {
            const double *rv[1] = {b.r}; double *tv[1] = {b.t};
            SGM_TRY(pc_apply_parts(pc, A, rv, tv, nullptr));
            ++applies;
        } else
            launch_elem(n, FCopy{b.t, b.r}, nullptr);
        launch_elem(n, FDot2{b.t, b.t, nullptr, nullptr, P_TT, nullptr}, nullptr);
        launch_egs<0>(n, m, b.t, b.U, ld, nullptr, b.parts, flag);
        reduce(m, hs, flag);
        launch_egs2(n, m, b.t, b.V, b.U, ld, hs, b.parts, flag);
        reduce(m, gs, flag);
        launch_egs<2>(n, m, b.t, b.V, ld, gs, P_WW, flag);
        hipLaunchKernelGGL(k_dav_norm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, ScalarRef{P_TT, gd}, 1, b.S);
        SGM_TRY(product(B, products_b, b.t, b.p, flag));
        SGM_TRY(new_column(m, b.t, b.p));
        launch_egs<0>(n, m + 1, w(m), b.V, ld, nullptr, b.parts, flag);
        reduce(m + 1, hs, flag);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(DavDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(col.data(), hs, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // synchronisation 1
        // a step that ends at one of its tests counts none of its products (after the flag they returned at once)
        if (hd.flag || hd.tau != hd.tau || hd.beta != hd.beta) { --products; --products_b; }
        if (hd.tau != hd.tau || hd.beta != hd.beta || hd.flag == 2) { nan = true; break; }
        if (hd.flag) { found = std::min<int>(k, locked); break; }
        for (int i = 0; i <= m; ++i) H[i + (size_t)m * m_cap] = H[m + (size_t)i * m_cap] = col[i];
        ++m;
        ++steps;
    }

    const double qnan = std::nan("");
    for (int i = 0; i < k; ++i) lambda_out[i] = resid_out[i] = qnan;
    if (nan) found = 0, converged = 0;
    if (found > 0) {
        // Vout = V[:, 0..m-1] Z[:, wanted] ; resid_i = sqrt(r.r), r = A v_i - lambda_i (B v_i)
        select(found);
        SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * found * 8, hipMemcpyHostToDevice, st));
        launch_rotate(n, m, found, b.V, ld, b.Z);
        for (int i = 0; i < found; ++i) {
            lambda_out[i] = theta[order[i]];
            SGM_TRY(product(A, products, v(i), b.t, nullptr));
            SGM_TRY(product(B, products_b, v(i), b.p, nullptr));
            launch_elem(n, FEigResid{b.t, b.p, lambda_out[i], b.parts + (size_t)i * kMaxGrid}, nullptr);
        }
        reduce(found, rs, nullptr);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(resid_out, rs, (size_t)found * 8, hipMemcpyDeviceToHost, st));
        if (V_out)
            SGM_HIP(hipMemcpy2DAsync(V_out, (size_t)n * 8, b.V, (size_t)ld * 8, (size_t)n * 8, found,
                                     where == SGM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
        SGM_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < found; ++i) resid_out[i] = sqrt(resid_out[i]);
    }
    info[0] = steps;
    info[1] = products;
    info[2] = products_b;
    info[3] = applies;
    info[4] = restarts;
    info[5] = found;
    info[6] = converged;
    return SGM_OK;
}

}  // extern "C"
