"""The restatement of sgm_davidson (tests/davidson_restated.py) held to mathematics -- host code, no GPU needed -- which makes
it a yardstick for tests/test_gpu_davidson.py, and the parts of sg.davidson that refuse before the library is called.

  1  every case: the float64 restatement with the device's order of summation converges, and every lam_i lies within the
     restatement's own resid_i of the i-th smallest eigenvalue of the dense matrix (numpy.linalg.eigvalsh; its own error,
     n eps |A|, is added); a second run in np.longdouble agrees with it;
  2  the step counts of the grids the GPU tests compare (63 x 63 and 255 x 255) with the restated V-cycle;
  3  the ends that are not convergence, and a pair that the space meets late: found before "converged" is said;
  4  sg.davidson refuses what it can without a GPU."""
from types import SimpleNamespace

import numpy as np
import pytest

import davidson_restated as DR
import eigsh_restated as ER
import sigma_amd as sg

# (matrix, preconditioner): the non-square grids have simple low eigenvalues
RUNS = [("poisson33x29", "mg"), ("poisson60x50", "mg"), ("spd300", "jacobi"), ("spd300", "none"), ("lap3d", "none")]
K, NCV = 4, 20


@pytest.mark.parametrize("name,pc", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_restatement_finds_the_smallest_eigenvalues_within_its_own_residual(name, pc):
    """The residual theorem for symmetric matrices puts an eigenvalue within |A v - lam v| / |v| of lam; here it must be the
    i-th smallest, one to one.  eigsh_restated's tests hold no longdouble run of their loop to take a bound from, so the bound
    of the longdouble comparison is derived here: both runs' lam_i lie within their own residual of the same exact eigenvalue,
    hence within resid_i + resid_ld_i of each other."""
    c = DR.case(name)
    r = DR.restated(name, pc, K, NCV)
    rl = DR.restated_ld(name, pc, K, NCV)
    exact = np.linalg.eigvalsh(c.dense)[:K]
    slack = c.n * ER.EPS * c.norm2
    dist = np.abs(r.lam - exact)
    vn = np.sqrt(np.sum(r.V.astype(np.longdouble) ** 2, axis=0)).astype(np.float64)
    between = np.abs(r.lam.astype(np.longdouble) - rl.lam).astype(np.float64)
    print(f"{name} {pc}: steps {r.steps} (longdouble {rl.steps}), products {r.products}, applies {r.applies}, restarts {r.restarts}; "
          f"max resid {np.max(r.residuals):.3e}, max |lam - exact| {dist.max():.3e}, max |lam - lam_ld| {between.max():.3e}")
    assert r.converged and r.found == K and rl.converged and rl.found == K
    assert r.products == 1 + r.steps + K and r.applies == (0 if pc == "none" else r.steps)
    assert np.all(np.abs(vn - 1.0) <= 1e-10)
    assert np.all(dist <= r.residuals + slack), (dist, r.residuals)
    assert np.all(np.abs(rl.lam.astype(np.float64) - exact) <= rl.residuals.astype(np.float64) + slack)
    assert np.all(between <= r.residuals + rl.residuals.astype(np.float64)), (between, r.residuals)
    assert np.array_equal(np.argsort(r.lam, kind="stable"), np.arange(K))
    # the reported residual is the true one: recomputed in longdouble within the forward bound of its float64 evaluation
    R, _, fwd = DR.true_residuals(c, r.lam, r.V)
    assert np.all(np.abs(r.residuals - R) <= fwd), (r.residuals, R, fwd)


def test_restated_vcycle_makes_the_step_count_grid_independent():
    """k = 4, ncv = 20, tol 1e-8, V(1,1), omega 0.8, 8 coarse sweeps, the device's order of summation: what
    test_the_vcycle_makes_the_step_count_grid_independent asks of the device, asked of the restatement first."""
    small = DR.restated("poisson63x63", "mg", K, NCV)
    large = DR.restated("poisson255x255", "mg", K, NCV)
    print(f"63 x 63: {small.steps} steps; 255 x 255: {large.steps} steps")
    assert small.converged and large.converged
    assert large.steps <= small.steps + 3
    ex = DR.cos_spectrum(255, 255)[:K]
    assert np.all(np.abs(large.lam - ex).astype(np.float64) <= large.residuals + 16 * ER.EPS * 8.0)


def test_restatement_ends_that_are_not_convergence():
    """max_steps = 0: one Ritz pair, as it is; q1 an exact eigenvector with k = 2: the space cannot grow past dimension 1 --
    found = 1, not converged; a NaN in the matrix: found = 0."""
    c = DR.case("poisson33x29")
    r = DR.davidson(c.rows, 4, 20, c.q1, None, max_steps=0)
    assert (r.steps, r.products, r.found, r.converged) == (0, 2, 1, False)
    assert np.isfinite(r.lam[0]) and np.isnan(r.lam[1:]).all() and np.isnan(r.residuals[1:]).all()
    d = DR.case("diag40")
    e3 = np.zeros(d.n)
    e3[2] = 2.0
    r = DR.davidson(d.rows, 2, 8, e3, None)
    assert (r.steps, r.found, r.converged) == (0, 1, False) and r.lam[0] == 3.0 and r.residuals[0] == 0.0
    bad = DR.MR._Rows((c.n, c.n, c.ptr, c.node, np.where(np.arange(len(c.val)) == 7, np.nan, c.val)))
    r = DR.davidson(bad, 4, 20, c.q1, None)
    assert r.found == 0 and not r.converged and np.isnan(r.lam).all()


def test_a_pair_that_the_space_meets_late_is_found_before_convergence_is_declared():
    """late40: the pairs of 1 and 2 are locked before the Ritz value of 1.001 comes down between them and takes the second
    place untested; the look at the earlier pairs before "converged" finds it (relocks >= 1) and the loop goes on with it.
    Without that look the call would return it as it is, `converged` set, with a residual far above tol |A|."""
    c = DR.case("late40")
    r = DR.restated("late40", "none", 4, 20)
    print(f"late40: steps {r.steps}, restarts {r.restarts}, relocks {r.relocks}, lam {r.lam}, residuals {r.residuals}")
    assert r.converged and r.found == 4 and r.relocks >= 1
    assert np.all(np.abs(r.lam - [1.0, 1.001, 2.0, 3.0]) <= r.residuals + c.n * ER.EPS * c.norm2)
    assert np.all(r.residuals <= 2 * DR.TOL * c.norm2)


def test_python_surface_refuses_bad_arguments_without_a_gpu():
    A = SimpleNamespace(nrow=10)
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, q1=np.ones(9))                         # a short q1 would be read out of bounds
    assert e.value.code == 2
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, pc="jacobi")
    assert e.value.code == 1
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 2, pc=sg.jacobi())                        # a factory's object that has seen no matrix
    assert e.value.code == 1 and "set up" in str(e.value)
    r = sg.DavidsonResult(np.zeros(1), None, np.zeros(1), 3, 5, 3, 0, 1, True)
    assert isinstance(r, sg.EigshResult) and (r.steps, r.products, r.applies, r.restarts, r.found, r.converged) == (3, 5, 3, 0, 1, True)
    assert "steps=3" in repr(r) and "applies=3" in repr(r)
