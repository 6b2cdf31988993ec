// Stand-alone check of the host code behind sgm_symeig_host (sigma_amd/csrc/sgm_symeig_host.hpp) for a host sanitizer:
//     g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I sigma_amd/csrc
//         tools/symeig_host_check.cpp -o symeig_host_check && ./symeig_host_check
// It runs the Jacobi sweeps on the shapes sgm_eigsh produces (tridiagonal; arrowhead plus tridiagonal after a thick restart;
// diagonal; m = 1, 2, 64) and checks H Z = Z diag(theta) and Z^T Z = I loosely -- the bits are pinned by tests/test_eigsh_cpu.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sgm_symeig_host.hpp"

static double lcg(unsigned long long &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0 - 0.5;
}

static int check(int m, int keep, unsigned long long seed)
{
    std::vector<double> H((size_t)m * m, 0.0), theta(m), Z((size_t)m * m);
    auto h = [&](int i, int j) -> double & { return H[i + (size_t)j * m]; };
    for (int i = 0; i < m; ++i) h(i, i) = 4.0 * lcg(seed);
    for (int i = 0; i < keep && keep < m; ++i) h(keep, i) = h(i, keep) = 1e-3 * lcg(seed);
    for (int i = keep; i + 1 < m; ++i) h(i + 1, i) = h(i, i + 1) = lcg(seed);
    const int sweeps = sgm::symeig_jacobi(m, H.data(), theta.data(), Z.data());
    double worst = 0.0;
    for (int c = 0; c < m; ++c)
        for (int i = 0; i < m; ++i) {
            double hz = 0.0, zz = 0.0;
            for (int l = 0; l < m; ++l) { hz += h(i, l) * Z[l + (size_t)c * m]; zz += Z[l + (size_t)i * m] * Z[l + (size_t)c * m]; }
            worst = std::fmax(worst, std::fabs(hz - theta[c] * Z[i + (size_t)c * m]));
            worst = std::fmax(worst, std::fabs(zz - (i == c ? 1.0 : 0.0)));
        }
    std::printf("m %2d keep %2d: %2d sweeps, worst defect %.2e\n", m, keep, sweeps, worst);
    return worst <= 1e-12 && sweeps < sgm::kSymeigMaxSweeps ? 0 : 1;
}

int main()
{
    int bad = 0;
    const int shapes[][2] = {{1, 0}, {2, 0}, {2, 1}, {8, 0}, {20, 12}, {32, 19}, {64, 0}, {64, 34}, {9, 9}};
    for (const auto &s : shapes) bad += check(s[0], s[1], 12345u + (unsigned)s[0]);
    std::printf(bad ? "symeig_host_check: FAILED\n" : "symeig_host_check: ok\n");
    return bad ? 1 : 0;
}
