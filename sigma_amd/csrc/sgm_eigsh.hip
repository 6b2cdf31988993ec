// sgm_eigsh: the k smallest or largest eigenpairs of a symmetric matrix by thick-restart Lanczos (Wu-Simon), the basis resident in
// HBM; sgm_basis_rotate, the in-place product Q[:, 0:kk] <- Q[:, 0:m] Z that forms Ritz vectors; sgm_symeig_host, the small dense
// eigensolver of the projected matrix.  No reference counterpart: the contract is the loop in include/sigma_hip.h (sgm_eigsh),
// DESIGN.md section 9g points to it, tests/eigsh_restated.py restates it.  Compiled with -ffp-contract=off, no MFMA: every
// operation is rounded on its own.
//
// A Lanczos step is 8 launches with three dependent reductions (h, g, w.w):
//     w = A q_j                                                  spmv_parts
//     partial sums of h = Q[:, 0..j]^T w                          k_egs<KB, 0>     basis read once
//     h                                                           k_eig_reduce     (j + 1 workgroups re-reduce the partial sums)
//     w -= Q h ; partial sums of g = Q^T w                        k_egs<KB, 1>     basis read once (columns held in registers)
//     g                                                           k_eig_reduce
//     w -= Q g ; partial sums of w.w                              k_egs<KB, 2>     basis read once
//     H(j,j) = h_j + g_j ; beta_j = sqrt(w.w) ; invariant test    k_eig_step       (one workgroup)
//     q_{j+1} = w * (1.0 / beta_j)                                FEigScale
// -- three reads of the j + 1 columns and five passes over w, whatever j is.  Nothing in a cycle waits for the host: the step
// kernel raises a device flag at an invariant subspace (or a NaN) and every later kernel of the cycle returns at once.
// (k_egs, k_eig_reduce, k_basis_rotate, FEigScale, FEigResid and the end of the call, eig_hand_back, are in
// sgm_eigsh_device.hpp, the Rayleigh-Ritz block of a cycle, rayleigh_ritz, in sgm_symeig_host.hpp: sgm_davidson.hip uses them too.)
#include "sgm_eigsh_device.hpp"
#include "sgm_symeig_host.hpp"

namespace sgm {

// lives in device memory; copied to the host once per cycle (the cycle's one synchronisation)
struct EigDev {
    double alpha[kEigMaxNcv];      // H(j,j) of the steps taken
    double beta[kEigMaxNcv];       // beta_j
    double scale;                  // max(anorm, |H(i,i)|, beta_i) over the steps of this cycle so far
    double inv;                    // 1.0 / beta_j of the last step
    int32_t ncols;                 // columns of the basis that are orthonormal: j + 1 after step j
    int32_t flag;                  // nonzero: the cycle has ended early (beta_j <= 2^-40 scale, or not a number)
};

// the end of step j: H(j,j), beta_j, the invariant-subspace test.  first: j is the first step of its cycle (scale starts at anorm)
__global__ __launch_bounds__(kBlock) void k_eig_step(ScalarRef ww, const double *hs, const double *gs, int j, int first, double anorm,
                                                     EigDev *S)
{
    __shared__ double red[kBlock / 64];
    if (S->flag) return;
    const double d = load_scalar<kBlock>(ww, red);
    if (threadIdx.x != 0) return;
    const double alpha = hs[j] + gs[j], beta = sqrt(d);
    double s = first ? anorm : S->scale;
    if (fabs(alpha) > s) s = fabs(alpha);
    if (beta > s) s = beta;
    S->alpha[j] = alpha;
    S->beta[j] = beta;
    S->scale = s;
    S->inv = 1.0 / beta;
    S->ncols = j + 1;
    if (!(beta > kEigTiny * s)) S->flag = 1;          // (a beta that is not a number compares false too)
}

}  // namespace sgm

extern "C" {

int sgm_symeig_host(int32_t m, const double *H, double *theta, double *Z, int32_t *sweeps)
{
    if (m < 1 || !H || !theta || !Z) return fail(SGM_ERR_BAD_ARG, "sgm_symeig_host: bad argument");
    const int32_t sw = symeig_jacobi(m, H, theta, Z);
    if (sweeps) *sweeps = sw;
    return SGM_OK;
}

int sgm_basis_rotate(int64_t n, int32_t m, int32_t kk, double *Q, int64_t ldq, const double *Z, int where)
{
    SGM_TRY(require_init());
    if (n < 1 || m < 1 || m > kEigMaxNcv || kk < 1 || kk > m || !Q || !Z || ldq < n)
        return fail(SGM_ERR_BAD_ARG, "sgm_basis_rotate: needs n >= 1, 1 <= kk <= m <= 64, ldq >= n");
    struct Bufs {
        double *Z = nullptr, *Q = nullptr;
        ~Bufs() { dfree(Z); dfree(Q); }
    } b;
    SGM_TRY(dalloc(&b.Z, (size_t)m * kk));
    hipStream_t st = g_rt.stream;
    SGM_HIP(hipMemcpyAsync(b.Z, Z, (size_t)m * kk * 8, hipMemcpyHostToDevice, st));
    double *Qd = Q;
    const size_t span = (size_t)ldq * (m - 1) + n;               // the entries between Q(0,0) and Q(n-1,m-1)
    if (where == SGM_HOST) {
        SGM_TRY(dalloc(&b.Q, span));
        SGM_HIP(hipMemcpyAsync(b.Q, Q, span * 8, hipMemcpyHostToDevice, st));
        Qd = b.Q;
    }
    launch_rotate(n, m, kk, Qd, ldq, b.Z);
    SGM_HIP(hipGetLastError());
    if (where == SGM_HOST)
        SGM_HIP(hipMemcpy2DAsync(Q, (size_t)ldq * 8, Qd, (size_t)ldq * 8, (size_t)n * 8, kk, hipMemcpyDeviceToHost, st));
    SGM_HIP(hipStreamSynchronize(st));        // (Z's device copy is released on return)
    return SGM_OK;
}

int sgm_eigsh(sgm_mat A, int32_t k, int32_t ncv, int32_t which, double tol, int32_t max_restarts, const double *q1,
              double *lambda_out, double *V_out, double *resid_out, int64_t *info, int where)
{
    SGM_TRY(require_init());
    if (!A || !q1 || !lambda_out || !resid_out || !info) return fail(SGM_ERR_BAD_ARG, "sgm_eigsh: null argument");
    if (A->nrow != A->ncol) return fail(SGM_ERR_DIMS, "sgm_eigsh: square matrices only (%d x %d)", A->nrow, A->ncol);
    if (A->distributed()) return fail(SGM_ERR_UNSUPPORTED, "sgm_eigsh: row-partitioned and distributed matrices are not supported");
    const int64_t n = A->nrow;
    const int m = ncv;
    if (k < 1 || ncv <= k || ncv > kEigMaxNcv || ncv >= n || !(tol >= kEigTiny) || max_restarts < 0 || (which != 0 && which != 1))
        return fail(SGM_ERR_BAD_ARG, "sgm_eigsh: needs 1 <= k < ncv <= 64, ncv < n, tol >= 2^-40, max_restarts >= 0, which 0 or 1 "
                                     "(k %d, ncv %d, n %lld, tol %g, max_restarts %d, which %d)", k, ncv, (long long)n, tol, max_restarts, which);
    const int64_t ld = (n + 1) & ~(int64_t)1;                     // even leading dimension: 16-byte aligned columns
    const int gd = dot_grid(n);
    struct Bufs {
        double *Q = nullptr, *w = nullptr, *parts = nullptr, *slots = nullptr, *Z = nullptr;
        EigDev *S = nullptr;
        ~Bufs() { dfree(Q); dfree(w); dfree(parts); dfree(slots); dfree(Z); dfree(S); }
    } b;
    SGM_TRY(dalloc(&b.Q, (size_t)ld * (m + 1) + 2));
    SGM_TRY(dalloc(&b.w, (size_t)ld + 2));
    SGM_TRY(dalloc(&b.parts, (size_t)(kEigMaxNcv + 1) * kMaxGrid));
    SGM_TRY(dalloc(&b.slots, (size_t)3 * kEigMaxNcv));
    SGM_TRY(dalloc(&b.Z, (size_t)kEigMaxNcv * kEigMaxNcv));
    SGM_TRY(dalloc(&b.S, 1));
    hipStream_t st = g_rt.stream;
    SGM_HIP(hipMemsetAsync(b.Q, 0, ((size_t)ld * (m + 1) + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.w, 0, ((size_t)ld + 2) * 8, st));
    SGM_HIP(hipMemsetAsync(b.S, 0, sizeof(EigDev), st));
    double *hs = b.slots, *gs = b.slots + kEigMaxNcv, *rs = b.slots + 2 * kEigMaxNcv;
    double *P_WW = b.parts + (size_t)kEigMaxNcv * kMaxGrid;
    auto q = [&](int c) { return b.Q + (size_t)c * ld; };
    const int *flag = &b.S->flag;
    const double *cx[1]; double *yy[1];
    int64_t products = 0;
    auto product = [&](const double *src, double *dst, const int *fl) -> int {
        cx[0] = src; yy[0] = dst;
        return spmv_parts(A, cx, yy, false, nullptr, fl, nullptr);
    };
    {   // q_0 = q1 / sqrt(q1.q1)
        Staged s1;
        SGM_TRY(stage_in(s1, q1, n, where, true));
        launch_elem(n, FDot2{s1.dev, s1.dev, nullptr, nullptr, P_WW, nullptr}, nullptr);
        launch_elem(n, FScaleInv{q(0), s1.dev, ScalarRef{P_WW, gd}}, nullptr);
        SGM_HIP(hipStreamSynchronize(st));                        // (the staged copy of q1 is released here)
    }

    std::vector<double> H((size_t)m * m, 0.0), theta(m), Z((size_t)m * m), Zsel((size_t)m * m);
    std::vector<int> order(m);
    EigDev hd;
    const int keep = std::min(k + (m - k) / 2, m - 1);
    double anorm = 0.0;
    int l = 0, nc = 0, found = 0, converged = 0;
    int64_t restarts = 0;
    bool nan = false;
    for (int64_t c = 0;; ++c) {
        for (int j = l; j < m; ++j) {
            SGM_TRY(product(q(j), b.w, flag));
            launch_egs<0>(n, j + 1, b.w, b.Q, ld, nullptr, b.parts, flag);
            hipLaunchKernelGGL(k_eig_reduce, dim3(j + 1), dim3(kBlock), 0, st, (const double *)b.parts, gd, hs, flag);
            launch_egs<1>(n, j + 1, b.w, b.Q, ld, hs, b.parts, flag);
            hipLaunchKernelGGL(k_eig_reduce, dim3(j + 1), dim3(kBlock), 0, st, (const double *)b.parts, gd, gs, flag);
            launch_egs<2>(n, j + 1, b.w, b.Q, ld, gs, P_WW, flag);
            hipLaunchKernelGGL(k_eig_step, dim3(1), dim3(kBlock), 0, st, ScalarRef{P_WW, gd}, (const double *)hs, (const double *)gs, j,
                               j == l ? 1 : 0, anorm, b.S);
            launch_elem(n, FEigScale{q(j + 1), b.w, &b.S->inv}, flag);
        }
        SGM_HIP(hipGetLastError());
        SGM_HIP(hipMemcpyAsync(&hd, b.S, sizeof(EigDev), hipMemcpyDeviceToHost, st));
        SGM_HIP(hipStreamSynchronize(st));                        // the cycle's one synchronisation
        nc = hd.ncols;
        const bool closed = hd.flag != 0;
        products += nc - l;                                       // (the products of a closed cycle's remaining steps returned at once)
        for (int j = l; j < nc; ++j) {
            if (hd.alpha[j] != hd.alpha[j] || hd.beta[j] != hd.beta[j]) nan = true;
            H[j + (size_t)j * m] = hd.alpha[j];
            if (j + 1 < nc) H[(j + 1) + (size_t)j * m] = H[j + (size_t)(j + 1) * m] = hd.beta[j];
        }
        if (nan) break;
        // the leading nc x nc block (nc < m only when the space has closed), wanted end first
        nan = !rayleigh_ritz(nc, H.data(), m, theta.data(), Z.data(), order.data(), anorm,
                             [&](double a, double c2) { return which == 0 ? a < c2 : a > c2; });
        if (nan) break;
        if (closed) {                                             // an invariant subspace: every Ritz pair in it is exact, rho = 0
            found = std::min<int>(k, nc);
            converged = nc >= k;
            break;
        }
        const double bm = hd.beta[m - 1];
        bool all = true;
        for (int i = 0; i < k; ++i)
            if (!(fabs(bm * Z[(m - 1) + (size_t)order[i] * m]) <= tol * anorm)) all = false;
        found = k;
        if (all) { converged = 1; break; }
        if (c == max_restarts) break;
        // thick restart: the first `keep` Ritz vectors in that order, then q_m
        for (int i = 0; i < keep; ++i)
            for (int r = 0; r < m; ++r) Zsel[r + (size_t)i * m] = Z[r + (size_t)order[i] * m];
        SGM_HIP(hipMemcpyAsync(b.Z, Zsel.data(), (size_t)m * keep * 8, hipMemcpyHostToDevice, st));
        launch_rotate(n, m, keep, b.Q, ld, b.Z);
        launch_elem(n, FCopy{q(keep), q(m)}, nullptr);
        std::fill(H.begin(), H.end(), 0.0);
        for (int i = 0; i < keep; ++i) {
            H[i + (size_t)i * m] = theta[order[i]];
            H[keep + (size_t)i * m] = H[i + (size_t)keep * m] = bm * Z[(m - 1) + (size_t)order[i] * m];
        }
        l = keep;
        ++restarts;                                               // (Zsel is next written after the next cycle's synchronisation)
    }

    if (nan) found = 0, converged = 0;
    // V = Q[:, 0..nc-1] Z[:, wanted] ; resid_i = sqrt(r.r), r = A v_i - lambda_i v_i
    for (int i = 0; i < found; ++i)
        for (int r = 0; r < nc; ++r) Zsel[r + (size_t)i * nc] = Z[r + (size_t)order[i] * nc];
    if (found > 0) SGM_HIP(hipMemsetAsync(&b.S->flag, 0, sizeof(int32_t), st));
    SGM_TRY(eig_hand_back(n, ld, nc, k, found, b.Q, Zsel.data(), b.Z, theta.data(), order.data(), b.parts, rs, lambda_out, V_out,
                          resid_out, where, [&](const double *v, const double *&y, const double *&x) {
                              ++products;
                              y = b.w; x = v;
                              return product(v, b.w, nullptr);
                          }));
    info[0] = restarts;
    info[1] = products;
    info[2] = found;
    info[3] = converged;
    return SGM_OK;
}

}  // extern "C"
