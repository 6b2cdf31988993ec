"""The restatement of sgm_davidson_gen (tests/davidson_gen_restated.py) held to mathematics -- host code, no GPU needed --
which makes it a yardstick for tests/test_gpu_davidson_gen.py, and the parts of sg.davidson(.., B=) that refuse before the
library is called.

  1  every case the GPU file pins or holds to the analytic spectrum: the float64 restatement with the device's order of
     summation converges with found == k, and every lam_i lies within |r_i|_{B^-1} / |v_i|_B of the i-th smallest exact
     eigenvalue of the pencil (r_i recomputed in longdouble from the returned pair, B^-1 by a dense solve); V^T B V = I to
     n eps; the reported residual is the true one; a second run in np.longdouble agrees within the two bounds;
  2  the ends that are not convergence;
  3  sg.davidson refuses a B it can refuse without a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import davidson_gen_restated as GR
import davidson_restated as DR
import eigsh_restated as ER
import sigma_amd as sg

# (pair, preconditioner, k, ncv, a caller's q1, a longdouble run too): what tests/test_gpu_davidson_gen.py pins bit for bit,
# then what it holds to the analytic spectrum.  No longdouble run where it would take a minute (ncv = 40), where there is no
# longdouble statement of the operator (the oracle's ILDU, the composite's product) and where a caller's q1 only repeats a case.
RUNS = [("fem33x29", "mg", 4, 20, False, True), ("fem33x29", "mg22direct", 4, 8, False, True), ("fem33x29", "none", 1, 8, False, True),
        ("fem33x29", "none", 4, 40, False, False), ("fem45x41", "mg", 4, 20, True, False), ("mesh19x17", "jacobi", 4, 20, False, True),
        ("mesh19x17", "ildu", 4, 20, False, False), ("comp32x24", "none", 1, 8, False, False),
        ("fem60x50", "mg", 4, 20, False, False), ("fem45x41", "mg", 4, 20, False, True)]


def restated(name, pc, k, ncv, own):
    if pc == "ildu":             # ILDU(0) has no restatement in numpy: the oracle's factors and sweeps, as the GPU file takes them
        import oracle as orc
        c = GR.case(name)
        M = orc.Ildu(orc.CsrMatrix(c.n, c.n, c.A[2], c.A[3], c.A[4]))
        return GR.davidson_gen(c.rowsA, c.rowsB, k, ncv, c.q1, M.solve)
    return GR.restated(name, pc, k, ncv, own)


@pytest.mark.parametrize("name,pc,k,ncv,own,ld", RUNS, ids=[f"{n}-{p}-k{k}-ncv{m}{'-q1' if q else ''}" for n, p, k, m, q, _ in RUNS])
def test_restatement_finds_the_smallest_eigenvalues_within_the_residual_bound_of_the_pencil(name, pc, k, ncv, own, ld):
    """For symmetric A and symmetric positive definite B, an eigenvalue of A x = lam B x lies within |r|_{B^-1} / |v|_B of any
    lam, r = A v - lam B v (the residual theorem of B^-1/2 A B^-1/2 at B^1/2 v); here it must be the i-th smallest, one to
    one.  The slack: the analytic values are evaluated in longdouble; a dense generalized solve (Cholesky of B, eigvalsh) is
    backward stable, |error| <= p(n) eps |B^-1 A| with p(n) taken as n, as test_davidson_cpu.py takes n eps |A| for eigvalsh;
    the same n eps |B^-1 A| covers the roundings of the float64 solve with B inside the bound.  Both runs' lam_i lie within
    their own bound of the same eigenvalue, hence within the sum of the two bounds of each other."""
    c = GR.case(name)
    r = restated(name, pc, k, ncv, own)
    exact = c.spectrum[:k]
    slack = c.n * ER.EPS * GR.pencil_norm(c)
    bound, G = GR.eigenvalue_bounds(c, r.lam, r.V)
    dist = np.abs(r.lam.astype(np.longdouble) - exact).astype(np.float64)
    orth = float(np.max(np.abs(G - np.eye(k))))
    R, fwd = GR.true_residuals(c, r.lam, r.V)
    print(f"{name} {pc} k={k} ncv={ncv}: steps {r.steps}, products {r.products} / {r.products_B}, applies {r.applies}, restarts {r.restarts}; "
          f"max |lam - exact| {dist.max():.3e}, bounds {bound.min():.3e} .. {bound.max():.3e} (slack {slack:.3e}), "
          f"|V^T B V - I| {orth:.3e} (n eps {c.n * ER.EPS:.3e}), max |resid - R| {np.max(np.abs(r.residuals - R)):.3e} (bound {fwd.min():.3e})")
    assert r.converged and r.found == k
    assert r.products == 1 + r.steps + k and r.products_B == 1 + r.steps + k and r.applies == (0 if pc == "none" else r.steps)
    if ncv == 8 and k == 4:
        assert r.restarts >= 2
    if ncv == 40:
        assert r.steps > 32 and r.restarts >= 1       # the space passes 32 columns
    assert np.all(dist <= bound + slack), (dist, bound)
    assert orth <= c.n * ER.EPS
    assert np.all(np.abs(r.residuals - R) <= fwd), (r.residuals, R, fwd)
    assert np.array_equal(np.argsort(r.lam, kind="stable"), np.arange(k))
    if name == "mesh19x17":
        assert abs(r.lam[0] - 1.0) <= bound[0] + slack
    if ld:
        rl = GR.restated_ld(name, pc, k, ncv)
        bl, _ = GR.eigenvalue_bounds(c, rl.lam, rl.V)
        between = np.abs(r.lam.astype(np.longdouble) - rl.lam).astype(np.float64)
        print(f"    longdouble: steps {rl.steps}, max |lam - lam_ld| {between.max():.3e}, its bounds up to {bl.max():.3e}")
        assert rl.converged and rl.found == k
        assert np.all(np.abs(rl.lam - exact).astype(np.float64) <= bl + slack)
        assert np.all(between <= bound + bl + 2 * slack), (between, bound, bl)


def test_restatement_ends_that_are_not_convergence():
    """max_steps = 0: one Ritz pair, as it is; B = -M: d = q1.(B q1) < 0 at the start -- found = 0, the one product with B
    counted, none with A; a NaN in B; q1 an exact eigenvector with k = 2: the space cannot grow past dimension 1."""
    c = GR.case("fem33x29")
    r = GR.davidson_gen(c.rowsA, c.rowsB, 4, 20, c.q1, None, max_steps=0)
    assert (r.steps, r.products, r.products_B, r.found, r.converged) == (0, 2, 2, 1, False)
    assert np.isfinite(r.lam[0]) and np.isnan(r.lam[1:]).all() and np.isnan(r.residuals[1:]).all()
    n, _, ptr, node, val = c.B
    for bad in (-val, np.where(np.arange(len(val)) == 7, np.nan, val)):
        r = GR.davidson_gen(c.rowsA, DR.MR._Rows((n, n, ptr, node, bad)), 4, 20, c.q1, None)
        assert (r.found, r.converged, r.steps, r.products, r.products_B) == (0, False, 0, 0, 1)
        assert np.isnan(r.lam).all() and np.isnan(r.residuals).all()
    # ... a B that stops being positive on the first new direction: diag(1, .., 1, -1e6) is indefinite, q1.(B q1) > 0
    d = DR.case("diag40")
    bd = np.ones(d.n)
    bd[-1] = -1e6
    q = np.ones(d.n)
    q[-1] = 1e-4
    r = GR.davidson_gen(d.rows, DR.MR._Rows(GR._diag_csr(bd)), 2, 8, q, None)
    assert (r.found, r.converged) == (0, False) and r.products == 1 + r.steps and r.products_B == 1 + r.steps
    # diag(1..40) x = lam diag(1 + (i mod 7)/8) x from q1 = 2 e_3: lam = 3 / 1.25, nothing to expand from
    e3 = np.zeros(d.n)
    e3[2] = 2.0
    r = GR.davidson_gen(d.rows, DR.MR._Rows(GR._diag_csr(1.0 + (np.arange(d.n) % 7) / 8.0)), 2, 8, e3, None)
    assert (r.steps, r.found, r.converged) == (0, 1, False) and abs(r.lam[0] - 2.4) <= 4 * ER.EPS and r.residuals[0] <= 16 * ER.EPS


def test_python_surface_refuses_a_bad_mass_matrix_without_a_gpu():
    A = SimpleNamespace(nrow=10)
    B = sg._Matrix()
    B.nrow = B.ncol = 10
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, B=np.eye(10))                          # no matrix of the library's
    assert e.value.code == 1 and "B must be a matrix" in str(e.value)
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, B=B, q1=np.ones(9))                    # a short q1 would be read out of bounds
    assert e.value.code == 2
    B.nrow = B.ncol = 9
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, B=B)
    assert e.value.code == 2 and "9 x 9" in str(e.value)
    r = sg.DavidsonResult(np.zeros(1), None, np.zeros(1), 3, 5, 3, 0, 1, True)
    assert r.products_B == 0
    r = sg.DavidsonResult(np.zeros(1), None, np.zeros(1), 3, 5, 3, 0, 1, True, products_B=5)
    assert r.products_B == 5 and "products_B=5" in repr(r) and "steps=3" in repr(r)
