// sgm_davidson: the k smallest eigenpairs of a symmetric matrix by the generalized Davidson method with thick restart and a
// caller's preconditioner, the search space V and its image W = A V resident in HBM.  No reference counterpart: the contract is
// the loop in include/sigma_hip.h (sgm_davidson), DESIGN.md section 9h points to it, tests/davidson_restated.py restates it.
// Compiled with -ffp-contract=off, no MFMA: every operation is rounded on its own.
//
// A step expands the space by the preconditioned residual of the first Ritz pair that has not converged:
//     t = M^-1 r                                                   pc_apply_parts (FCopy without a preconditioner)
//     partial sums of t.t (tau)                                    FDot2
//     partial sums of h = V[:, 0..m-1]^T t ; h                     k_egs<KB, 0> ; k_eig_reduce
//     t -= V h ; partial sums of g = V^T t ; g                     k_egs<KB, 1> ; k_eig_reduce
//     t -= V g ; partial sums of t.t (beta)                        k_egs<KB, 2>
//     tau, beta, 1.0 / beta ; the test beta > 2^-40 tau            k_dav_norm      (one workgroup)
//     V_m = t * (1.0 / beta)                                       FEigScale
//     W_m = A V_m                                                  spmv_parts
//     partial sums of H(0..m, m) = V[:, 0..m]^T W_m ; the column   k_egs<KB, 0> ; k_eig_reduce
//  -> the host: H's new column, tau, beta, the flag                synchronisation 1
//     symeig of the (m + 1) x (m + 1) matrix                       symeig_jacobi (host)
//     z -> the device ; r = W z - theta V z ; partial sums of r.r  k_dav_ritz      the one pass that reads both bases
//     r.r                                                          k_eig_reduce
//  -> the host: r.r                                                synchronisation 2 (once more per pair that converges in this step,
//                                                                  and per pair looked at again before "converged")
// k_dav_norm raises a device flag when the new direction lies in the space (or is not a number); the step's remaining kernels
// then return at once and the host leaves the loop at synchronisation 1.
#include "sgm_eigsh_device.hpp"
#include "sgm_symeig_host.hpp"

#include <numeric>

namespace sgm {

bool pc_serves(sgm_pc pc, sgm_mat A);       // sgm_pc.hip

// One pass over the rows of V and W (n x m each, leading dimension ld, even): for row i
//     u = ((0.0 + V(i,0) z_0) + V(i,1) z_1) + ... ; y the same over W ; r(i) = y - theta * u
// r is stored, u and y are not; the partial sums of r.r are left in the order of k_egs (thread t of the grid dot_grid(n) takes
// the rows 2i, 2i+1 for i = t, t + threads, ..., thread 0 then the last row of an odd n).  z sits in LDS and is read as
// broadcasts; every column is read with 16-byte accesses, MB / 8 groups of 8 + 8 loads in flight per lane.  Compulsory traffic
// 8 n (2m + 1) bytes.
template <int MB>
__global__ __launch_bounds__(kBlock) void k_dav_ritz(int64_t n, int m, const double *__restrict__ V, const double *__restrict__ W, int64_t ld,
                                                     const double *__restrict__ z, double theta, double *__restrict__ r,
                                                     double *__restrict__ part_out)
{
    __shared__ double red[kBlock / 64];
    __shared__ double zl[MB];
    if (threadIdx.x < MB) zl[threadIdx.x] = (int)threadIdx.x < m ? z[threadIdx.x] : 0.0;
    __syncthreads();
    double acc = 0.0;
    const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    const int64_t n2 = n >> 1;
    for (int64_t i = gtid; i < n2; i += stride) {
        double2 u = make_double2(0.0, 0.0), y = make_double2(0.0, 0.0);
#pragma unroll
        for (int c0 = 0; c0 < MB; c0 += 8) {
            if (c0 < m) {                              // m is uniform: every thread takes the same branches
                double2 vv[8], ww[8];
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        vv[c] = ld2<true>(V + (size_t)(c0 + c) * ld, i);
                        ww[c] = ld2<true>(W + (size_t)(c0 + c) * ld, i);
                    }
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    if (c0 + c < m) {
                        const double zc = zl[c0 + c];
                        u.x = u.x + vv[c].x * zc; u.y = u.y + vv[c].y * zc;
                        y.x = y.x + ww[c].x * zc; y.y = y.y + ww[c].y * zc;
                    }
            }
        }
        double2 rr;
        rr.x = y.x - theta * u.x; rr.y = y.y - theta * u.y;
        st2<false>(r, i, rr);
        acc += rr.x * rr.x; acc += rr.y * rr.y;
    }
    if ((n & 1) && gtid == 0) {
        const int64_t i = n - 1;
        double u = 0.0, y = 0.0;
        for (int c = 0; c < m; ++c) {
            u = u + V[(size_t)c * ld + i] * zl[c];
            y = y + W[(size_t)c * ld + i] * zl[c];
        }
        const double rv = y - theta * u;
        r[i] = rv;
        acc += rv * rv;
    }
    const double t = block_sum<kBlock>(acc, red);
    if (threadIdx.x == 0) part_out[blockIdx.x] = t;
}

static void launch_ritz(int64_t n, int m, const double *V, const double *W, int64_t ld, const double *z, double theta, double *r, double *part)
{
    const dim3 grid(dot_grid(n)), block(kBlock);
    if (m <= 8) hipLaunchKernelGGL(k_dav_ritz<8>, grid, block, 0, g_rt.stream, n, m, V, W, ld, z, theta, r, part);
    else if (m <= 16) hipLaunchKernelGGL(k_dav_ritz<16>, grid, block, 0, g_rt.stream, n, m, V, W, ld, z, theta, r, part);
    else if (m <= 32) hipLaunchKernelGGL(k_dav_ritz<32>, grid, block, 0, g_rt.stream, n, m, V, W, ld, z, theta, r, part);
    else hipLaunchKernelGGL(k_dav_ritz<64>, grid, block, 0, g_rt.stream, n, m, V, W, ld, z, theta, r, part);
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
    const int64_t ld = (n + 1) & ~(int64_t)1;                     // even leading dimension: 16-byte aligned columns
    const int gd = dot_grid(n);
    struct Bufs {
        double *V = nullptr, *W = nullptr, *t = nullptr, *r = nullptr, *parts = nullptr, *slots = nullptr, *Z = nullptr;
        DavDev *S = nullptr;
        ~Bufs() { dfree(V); dfree(W); dfree(t); dfree(r); dfree(parts); dfree(slots); dfree(Z); dfree(S); }
    } b;
    SGM_TRY(dalloc(&b.V, (size_t)ld * ncv + 2));
    SGM_TRY(dalloc(&b.W, (size_t)ld * ncv + 2));
    SGM_TRY(dalloc(&b.t, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.r, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.parts, (size_t)(kEigMaxNcv + 2) * kMaxGrid));
    SGM_TRY(dalloc(&b.slots, (size_t)3 * kEigMaxNcv));
    SGM_TRY(dalloc(&b.Z, (size_t)kEigMaxNcv * kEigMaxNcv));
    SGM_TRY(dalloc(&b.S, 1));
    hipStream_t st = g_rt.stream;
    // every column of V and W is written (rows 0 .. n-1) before it is read, and no kernel reads past row n-1 (an odd n: its
    // last row alone, by one thread): only the pad row of an odd n is cleared, not 16 ld ncv bytes
    if (ld > n) {
        SGM_HIP(hipMemset2DAsync(b.V + n, (size_t)ld * 8, 0, (size_t)(ld - n) * 8, ncv, st));
        SGM_HIP(hipMemset2DAsync(b.W + n, (size_t)ld * 8, 0, (size_t)(ld - n) * 8, ncv, st));
    }
    SGM_HIP(hipMemsetAsync(b.t, 0, ((size_t)ld + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.r, 0, ((size_t)ld + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.S, 0, sizeof(DavDev), st));
    double *hs = b.slots, *gs = b.slots + kEigMaxNcv, *rs = b.slots + 2 * kEigMaxNcv;
    double *P_WW = b.parts + (size_t)kEigMaxNcv * kMaxGrid, *P_TT = b.parts + (size_t)(kEigMaxNcv + 1) * kMaxGrid;
    auto v = [&](int c) { return b.V + (size_t)c * ld; };
    auto w = [&](int c) { return b.W + (size_t)c * ld; };
    const int *flag = &b.S->flag;
    const double *cx[1]; double *yy[1];
    int64_t products = 0, applies = 0, steps = 0, restarts = 0;
    auto product = [&](const double *src, double *dst, const int *fl) -> int {
        cx[0] = src; yy[0] = dst;
        ++products;
        return spmv_parts(A, cx, yy, false, nullptr, fl, nullptr);
    };
    auto reduce = [&](int count, double *slots, const int *fl) {
        hipLaunchKernelGGL(k_eig_reduce, dim3(count), dim3(kBlock), 0, st, (const double *)b.parts, gd, slots, fl);
    };

    const int m_cap = ncv;
    std::vector<double> H((size_t)m_cap * m_cap, 0.0), Hb, theta(m_cap), Z((size_t)m_cap * m_cap), Zsel((size_t)m_cap * m_cap);
    std::vector<double> col(m_cap + 1), zc(m_cap);
    std::vector<int> order(m_cap);
    DavDev hd;
    const int keep = std::min(k + (m_cap - k) / 2, m_cap - 1);
    double anorm = 0.0, rr = 0.0;
    int m = 1, locked = 0, found = 0, converged = 0;
    bool nan = false;

    {   // V_0 = q1 * (1.0 / sqrt(q1.q1)) ; W_0 = A V_0 ; H(0,0) = V_0.W_0
        Staged s1;
        SGM_TRY(stage_in(s1, q1, n, where, true));
        launch_elem(n, FDot2{s1.dev, s1.dev, nullptr, nullptr, P_WW, nullptr}, nullptr);
        hipLaunchKernelGGL(k_dav_norm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, ScalarRef{P_WW, gd}, 0, b.S);
        launch_elem(n, FEigScale{v(0), s1.dev, &b.S->inv}, nullptr);
        SGM_TRY(product(v(0), w(0), nullptr));
        launch_egs<0>(n, 1, w(0), b.V, ld, nullptr, b.parts, flag);
        reduce(1, hs, nullptr);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(col.data(), hs, 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // (the staged copy of q1 is released here)
        H[0] = col[0];
    }

    for (;;) {
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
        // r = the residual of the j-th Ritz pair in that order ; meets = (sqrt(r.r) <= tol * anorm)   (a NaN compares false)
        auto residual_meets = [&](int j, bool &meets) -> int {
            const int c = order[j];
            for (int i = 0; i < m; ++i) zc[i] = Z[i + (size_t)c * m];
            SGM_HIP(hipMemcpyAsync(b.Z, zc.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
            launch_ritz(n, m, b.V, b.W, ld, b.Z, theta[c], b.r, b.parts);
            reduce(1, rs, nullptr);
            SGM_HIP(hipGetLastError());
            SGM_HIP(hipMemcpyAsync(&rr, rs, 8, hipMemcpyDeviceToHost, st));
            SGM_HIP(hipStreamSynchronize(st));                    // synchronisation 2 (zc is next written after it)
            meets = sqrt(rr) <= tol * anorm;
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
        if (steps == max_steps) { found = std::min<int>(k, m); break; }
        if (m == m_cap) {
            // thick restart: the first `keep` Ritz vectors in that order, in V and in W
            for (int i = 0; i < keep; ++i)
                for (int r = 0; r < m; ++r) Zsel[r + (size_t)i * m] = Z[r + (size_t)order[i] * m];
            SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * keep * 8, hipMemcpyHostToDevice, st));
            launch_rotate(n, m, keep, b.V, ld, b.Z);
            launch_rotate(n, m, keep, b.W, ld, b.Z);
            std::fill(H.begin(), H.end(), 0.0);
            for (int i = 0; i < keep; ++i) col[i] = theta[order[i]];
            std::fill(Z.begin(), Z.end(), 0.0);
            for (int i = 0; i < keep; ++i) {                      // the kept pairs are the space's Ritz pairs: theta_i, Z = I
                H[i + (size_t)i * m_cap] = theta[i] = col[i];
                Z[i + (size_t)i * keep] = 1.0;
                order[i] = i;
            }
            m = keep;
            ++restarts;                                           // (Zsel is next written after the step's synchronisation)
        }
        // expand: t = M^-1 r, twice orthogonalised against V[:, 0..m-1]
        if (pc) {
            const double *rp[1] = {b.r}; double *tp[1] = {b.t};
            SGM_TRY(pc_apply_parts(pc, A, rp, tp, nullptr));
            ++applies;
        } else
            launch_elem(n, FCopy{b.t, b.r}, nullptr);
        launch_elem(n, FDot2{b.t, b.t, nullptr, nullptr, P_TT, nullptr}, nullptr);
        launch_egs<0>(n, m, b.t, b.V, ld, nullptr, b.parts, flag);
        reduce(m, hs, flag);
        launch_egs<1>(n, m, b.t, b.V, ld, hs, b.parts, flag);
        reduce(m, gs, flag);
        launch_egs<2>(n, m, b.t, b.V, ld, gs, P_WW, flag);
        hipLaunchKernelGGL(k_dav_norm, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, ScalarRef{P_TT, gd}, 1, b.S);
        launch_elem(n, FEigScale{v(m), b.t, &b.S->inv}, flag);
        SGM_TRY(product(v(m), w(m), flag));
        launch_egs<0>(n, m + 1, w(m), b.V, ld, nullptr, b.parts, flag);
        reduce(m + 1, hs, flag);
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(DavDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipMemcpyAsync(col.data(), hs, (size_t)(m + 1) * 8, hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // synchronisation 1
        if (hd.tau != hd.tau || hd.beta != hd.beta) { --products; nan = true; break; }
        if (hd.flag) { --products; found = std::min<int>(k, locked); break; }      // (that product returned at once)
        for (int i = 0; i <= m; ++i) H[i + (size_t)m * m_cap] = H[m + (size_t)i * m_cap] = col[i];
        ++m;
        ++steps;
    }

    const double qnan = std::nan("");
    for (int i = 0; i < k; ++i) lambda_out[i] = resid_out[i] = qnan;
    if (nan) found = 0, converged = 0;
    if (found > 0) {
        // Vout = V[:, 0..m-1] Z[:, wanted] ; resid_i = sqrt(r.r), r = A v_i - lambda_i v_i
        for (int i = 0; i < found; ++i)
            for (int r = 0; r < m; ++r) Zsel[r + (size_t)i * m] = Z[r + (size_t)order[i] * m];
        SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * found * 8, hipMemcpyHostToDevice, st));
        launch_rotate(n, m, found, b.V, ld, b.Z);
        for (int i = 0; i < found; ++i) {
            lambda_out[i] = theta[order[i]];
            SGM_TRY(product(v(i), b.t, nullptr));
            launch_elem(n, FEigResid{b.t, v(i), lambda_out[i], b.parts + (size_t)i * kMaxGrid}, nullptr);
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
    info[2] = applies;
    info[3] = restarts;
    info[4] = found;
    info[5] = converged;
    return SGM_OK;
}

}  // extern "C"
