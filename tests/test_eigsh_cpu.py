"""The restatement of sgm_eigsh (tests/eigsh_restated.py) held to mathematics, and sgm_symeig_host -- host code, no GPU needed --
held to the restatement bit for bit.

  1  every case: the restatement converges within 200 restarts, its eigenvalues lie within its own TRUE residual (longdouble)
     of the k extreme exact eigenvalues, one to one -- that makes it a yardstick for tests/test_gpu_eigsh.py;
  2  sg.symeig_host equals the restated Jacobi in theta, Z and the sweep count, bit for bit;
  3  Z is orthogonal and Z diag(theta) Z^T gives H back within a bound derived here, not measured;
  4  the restart and product counts of every case are printed (profiles/eigsh/README.md quotes them)."""
import numpy as np
import pytest

import eigsh_restated as ER
import sigma_amd as sg

RUNS = [(name, k, ncv, which) for name in ER.CASES for (k, ncv) in ER.case_grid(name) for which in ("SA", "LA")]
RUNS += [("diag3", 2, 8, "SA"), ("diag3", 2, 8, "LA"), ("outliers", 4, 20, "LA")]


@pytest.mark.parametrize("name,k,ncv,which", RUNS, ids=[f"{n}-k{k}-ncv{m}-{w}" for n, k, m, w in RUNS])
def test_restatement_finds_the_extreme_eigenvalues_within_its_own_residual(name, k, ncv, which):
    c = ER.case(name)
    r = ER.restated(name, k, ncv, which, "numpy" if name == "outliers" else "device")
    R, vn, _ = ER.true_residuals(c, r.lam, r.V)
    dist = ER.spectrum_distances(c, r.lam, which)
    print(f"{name} k={k} ncv={ncv} {which}: restarts {r.restarts}, products {r.products}, max rho {np.max(r.rho):.3e}, "
          f"max true residual {R.max():.3e}, max |R - rho| {np.max(np.abs(R - r.rho)):.3e}, max distance to the spectrum {dist.max():.3e}")
    assert r.converged and r.found == k and r.restarts <= 200
    assert np.all(np.abs(vn - 1.0) <= 1e-10)
    # the residual theorem for symmetric matrices: an eigenvalue within R_i / |v_i| of lam_i; here it must be the i-th extreme one
    assert np.all(dist <= R / vn * (1 + 1e-6) + ER.spectrum_slack(c)), (dist, R / vn)
    order = np.argsort(r.lam if which == "SA" else -r.lam, kind="stable")
    assert np.array_equal(order, np.arange(k))


def _tridiagonal(m, seed):
    rs = np.random.RandomState(seed)
    d, e = rs.standard_normal(m), rs.standard_normal(max(m - 1, 0))
    return np.diag(d) + np.diag(e, 1) + np.diag(e, -1)


def _arrowhead(m, keep, seed):
    """what a thick restart leaves: diag(theta) on the first `keep`, row / column `keep` coupling them, a tridiagonal tail"""
    rs = np.random.RandomState(seed)
    H = np.zeros((m, m))
    H[np.arange(keep), np.arange(keep)] = np.sort(rs.standard_normal(keep))
    H[keep, :keep] = H[:keep, keep] = 1e-3 * rs.standard_normal(keep)
    T = _tridiagonal(m - keep, seed + 1)
    H[keep:, keep:] = T
    return H


SYMEIG = {
    "tridiagonal20": _tridiagonal(20, 1),
    "arrowhead20_keep12": _arrowhead(20, 12, 2),
    "arrowhead32_keep19": _arrowhead(32, 19, 3),
    "diagonal9": np.diag(np.arange(9.0) - 4.0),
    "m1": np.array([[-2.5]]),
    "m2": np.array([[1.0, 2.0], [2.0, -1.0]]),
    "m64": _tridiagonal(64, 4),
    "equal_diagonal": np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 1.0], [0.0, 1.0, 2.0]]),
}


@pytest.mark.parametrize("name", sorted(SYMEIG))
def test_symeig_host_is_the_restated_jacobi_bit_for_bit(name):
    H = SYMEIG[name]
    theta, Z, sweeps = sg.symeig_host(H)
    rt, rZ, rs = ER.symeig(H)
    print(f"{name}: {sweeps} sweeps")
    assert sweeps == rs and sweeps < ER.MAX_SWEEPS
    assert np.array_equal(theta.view(np.uint64), rt.view(np.uint64))
    assert np.array_equal(np.ascontiguousarray(Z).view(np.uint64), np.ascontiguousarray(rZ).view(np.uint64))
    if name.startswith("diagonal") or name == "m1":
        assert sweeps == 0 and np.array_equal(theta, np.diag(H)) and np.array_equal(Z, np.eye(len(H)))


@pytest.mark.parametrize("name", sorted(SYMEIG))
def test_symeig_host_is_orthogonal_and_reproduces_h_within_the_jacobi_bound(name):
    """A computed rotation (c, s) has c^2 + s^2 = 1 + d with |d| <= 8 u (sqrt, two divisions, a product and a sum, each within
    u), and applying it to a pair of columns adds at most gamma_3 of the pair's norm (two products and a sum per entry): one
    rotation moves a pair of columns at most 8 u (relative) away from an exactly orthogonal image.  A column takes part in
    m - 1 rotations per sweep, so after S sweeps every column of Z is within S (m - 1) 8 u (first order) of a column of an
    exactly orthogonal matrix, and |Z^T Z - I| <= 2 S (m - 1) 8 u (1 + that) entrywise.  The same count bounds the backward
    error of the two-sided update of A in the Frobenius norm: |Z diag(theta) Z^T - H|_F <= 2 S (m - 1) 8 u sqrt(m) |H|_F (the
    off-diagonal entries dropped at the end are exact zeros).  Both are evaluated in longdouble."""
    H = SYMEIG[name]
    m = len(H)
    theta, Z, sweeps = sg.symeig_host(H)
    e = 2 * max(sweeps, 1) * max(m - 1, 1) * 8 * ER.U
    Zl, tl = Z.astype(np.longdouble), theta.astype(np.longdouble)
    orth = float(np.max(np.abs(Zl.T @ Zl - np.eye(m))))
    back = float(np.linalg.norm(((Zl * tl) @ Zl.T - H).astype(np.float64)))
    print(f"{name}: |Z^T Z - I|_max {orth:.2e} (bound {e * (1 + e):.2e}), |Z theta Z^T - H|_F {back:.2e} "
          f"(bound {e * np.sqrt(m) * np.linalg.norm(H):.2e})")
    assert orth <= e * (1 + e)
    assert back <= e * np.sqrt(m) * np.linalg.norm(H)
    assert np.abs(np.sort(theta) - np.linalg.eigvalsh(H)).max() <= e * np.sqrt(m) * np.linalg.norm(H) + m * ER.EPS * np.linalg.norm(H)


def test_device_order_of_summation_extends_the_minres_tree_order():
    """For n <= 1024 the order defined in the header is minres_restated.tree_dot; above it there are several workgroups whose
    sums are re-reduced -- and the result depends on n alone"""
    import minres_restated as MN
    rs = np.random.RandomState(7)
    for n in (1, 2, 127, 768, 1024):
        a, b = rs.standard_normal(n), rs.standard_normal(n)
        assert ER.device_sums(a * b) == MN.tree_dot(a, b)
    assert [ER.dot_grid(n) for n in (1, 1024, 1025, 1845, 101440, 10 ** 7)] == [1, 1, 2, 2, 100, 1024]
    a = rs.standard_normal(1845)
    assert abs(ER.device_sums(a * a) - np.dot(a, a)) <= 1845 * ER.EPS * np.dot(a, a)


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    with pytest.raises(sg.SigmaError):
        sg.symeig_host(np.zeros((2, 3)))
    q = sg.eigsh_start_vector(5)
    assert np.array_equal(q, ER.start_vector(5)) and np.all((q >= 1) & (q < 2)) and np.array_equal(q * 1024, np.round(q * 1024))
