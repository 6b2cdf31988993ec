// Cyclic Jacobi for a small dense symmetric matrix, on the host: the eigensolver of sgm_eigsh's projected matrix H (after a
// thick restart H is arrowhead plus tridiagonal, not tridiagonal) and the body of sgm_symeig_host; and rayleigh_ritz, what
// sgm_eigsh and the Davidson loop (sgm_davidson.hip) do with the leading block of their H.  Plain C++ without a HIP
// call, so that a stand-alone program can run it under a host sanitizer (tools/symeig_host_check.cpp).  Must be compiled
// with -ffp-contract=off: every operation below is rounded on its own, and tests/eigsh_restated.py restates it in numpy.
//
// The contract (include/sigma_hip.h, sgm_symeig_host):
//     A = H ; Z = I ; sweeps = 0
//     repeat at most kSymeigMaxSweeps times:
//         every A(p,q), p < q, is exactly 0 (+0 or -0): stop
//         sweeps += 1
//         for p = 0 .. m-2, for q = p+1 .. m-1 (row-major over p < q), with apq = A(p,q) != 0:
//             tau = (A(q,q) - A(p,p)) / (2.0*apq)
//             r = sqrt(1.0 + tau*tau)
//             t = tau >= 0 ? 1.0/(tau + r) : -1.0/(r - tau)
//             c = 1.0/sqrt(1.0 + t*t) ; s = t*c
//             A(p,p) = A(p,p) - t*apq ; A(q,q) = A(q,q) + t*apq ; A(p,q) = A(q,p) = 0
//             for i != p, q:  x = A(i,p) ; y = A(i,q) ; A(i,p) = A(p,i) = c*x - s*y ; A(i,q) = A(q,i) = s*x + c*y
//             for every i:    x = Z(i,p) ; y = Z(i,q) ; Z(i,p) = c*x - s*y ; Z(i,q) = s*x + c*y
//     theta(i) = A(i,i)          (in the order Jacobi leaves them: NOT sorted)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

namespace sgm {

constexpr int kSymeigMaxSweeps = 64;

// H: m x m column-major (both triangles are read); theta: m; Z: m x m column-major, H Z = Z diag(theta); returns the sweeps
inline int32_t symeig_jacobi(int32_t m, const double *H, double *theta, double *Z)
{
    std::vector<double> Av((size_t)m * m);
    double *A = Av.data();
    for (size_t e = 0; e < (size_t)m * m; ++e) { A[e] = H[e]; Z[e] = 0.0; }
    for (int32_t i = 0; i < m; ++i) Z[i + (size_t)i * m] = 1.0;
    auto a = [&](int32_t i, int32_t j) -> double & { return A[i + (size_t)j * m]; };
    auto z = [&](int32_t i, int32_t j) -> double & { return Z[i + (size_t)j * m]; };
    int32_t sweeps = 0;
    for (int sweep = 0; sweep < kSymeigMaxSweeps; ++sweep) {
        bool diagonal = true;
        for (int32_t p = 0; p < m && diagonal; ++p)
            for (int32_t q = p + 1; q < m; ++q)
                if (a(p, q) != 0.0) { diagonal = false; break; }
        if (diagonal) break;
        ++sweeps;
        for (int32_t p = 0; p + 1 < m; ++p)
            for (int32_t q = p + 1; q < m; ++q) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double tau = (a(q, q) - a(p, p)) / (2.0 * apq);
                const double r = std::sqrt(1.0 + tau * tau);
                const double t = tau >= 0.0 ? 1.0 / (tau + r) : -1.0 / (r - tau);
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                a(p, p) = a(p, p) - t * apq;
                a(q, q) = a(q, q) + t * apq;
                a(p, q) = 0.0;
                a(q, p) = 0.0;
                for (int32_t i = 0; i < m; ++i) {
                    if (i == p || i == q) continue;
                    const double x = a(i, p), y = a(i, q);
                    const double xp = c * x - s * y, yq = s * x + c * y;
                    a(i, p) = xp; a(p, i) = xp;
                    a(i, q) = yq; a(q, i) = yq;
                }
                for (int32_t i = 0; i < m; ++i) {
                    const double x = z(i, p), y = z(i, q);
                    z(i, p) = c * x - s * y;
                    z(i, q) = s * x + c * y;
                }
            }
    }
    for (int32_t i = 0; i < m; ++i) theta[i] = a(i, i);
    return sweeps;
}

// Rayleigh-Ritz on the leading m x m block of H (column-major, leading dimension ldh), as sgm_eigsh and the Davidson loop take
// it: theta and Z (m x m) from symeig_jacobi ; anorm = max(anorm, |theta_i|) ; order = 0 .. m-1 sorted by `before` on theta, equal
// values in Jacobi's order.  false when an entry of the block or a theta is not a number: order is not written then.
template <class Before>
inline bool rayleigh_ritz(int32_t m, const double *H, int32_t ldh, double *theta, double *Z, int *order, double &anorm, Before before)
{
    std::vector<double> Hb((size_t)m * m);
    for (int32_t jc = 0; jc < m; ++jc)
        for (int32_t i = 0; i < m; ++i) {
            const double h = H[i + (size_t)jc * ldh];
            if (h != h) return false;
            Hb[i + (size_t)jc * m] = h;
        }
    symeig_jacobi(m, Hb.data(), theta, Z);
    for (int32_t i = 0; i < m; ++i) {
        if (theta[i] != theta[i]) return false;
        if (std::fabs(theta[i]) > anorm) anorm = std::fabs(theta[i]);
    }
    std::iota(order, order + m, 0);
    std::stable_sort(order, order + m, [&](int a, int c) { return before(theta[a], theta[c]); });
    return true;
}

}  // namespace sgm
