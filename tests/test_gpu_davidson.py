"""sg.davidson / sgm_davidson on the device (the contract: include/sigma_hip.h, sgm_davidson).

  1  bit for bit: lam, V, residuals, steps, products, applies, restarts, found and converged equal the float64 restatement
     (tests/davidson_restated.py) run with the device's defined order of summation -- CSR, ELLPACK and composite matrices,
     every preconditioner kind, k in {1, 4}, ncv in {8, 20, 40}, host vectors and device tensors, a caller's q1;
  2  independent of the restatement: the analytic spectrum of the grid Laplacians (double eigenvalues included), the reported
     residual against one recomputed in longdouble, orthonormality;
  3  the V-cycle makes the step count grid-independent; 4 fewer products than sg.eigsh "SA" by a factor of 5 or more;
  5  ends (max_steps = 0, an exact eigenvector, NaN), refusals, sg.eigsh untouched; 6 the Fortran host layer."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import davidson_restated as DR
import eigsh_restated as ER
import minres_restated as MN
import sigma_amd as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (matrix, storage, preconditioner, k, ncv, device tensors, a caller's q1).  n = 957 (33 x 29: two 512-row slices, an odd
# tail, one workgroup of partial sums), 300, 768 (the composite), 1845 (45 x 41: odd, two workgroups of partial sums);
# ncv = 8 restarts 13 to 60 times, ncv = 20 two to seven times.  late40 (n = 40): a pair the space meets after two others have
# been locked.  ncv = 40: m passes 32, so k_dav_ritz<64>, k_egs<64, *> (columns not held) and k_basis_rotate<64> run -- spd300
# restarts there twice (64 steps), odd reaches m = 33 without a restart (32 steps, the output rotation included).
PINNED = [
    ("poisson33x29", "csr", "mg", 4, 20, False, False),
    ("poisson33x29", "csr", "mg", 4, 20, True, False),
    ("poisson33x29", "csr", "mg22direct", 4, 8, False, False),
    ("poisson33x29", "ell", "jacobi", 1, 8, True, False),
    ("spd300", "csr", "mg", 4, 20, False, False),
    ("spd300", "csr", "ildu", 4, 20, False, False),
    ("spd300", "csr", "none", 4, 8, True, False),
    ("comp32x24", "composite", "none", 1, 8, False, False),
    ("odd", "csr", "mg", 4, 20, False, True),
    ("late40", "csr", "none", 4, 20, False, False),
    ("spd300", "csr", "none", 4, 40, False, False),
    ("odd", "csr", "mg", 4, 40, False, False),
]
PINNED_IDS = [f"{n}-{f}-{p}-k{k}-ncv{m}{'-tensor' if t else ''}{'-q1' if q else ''}" for n, f, p, k, m, t, q in PINNED]


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _csr(M):
    return sg.csr_matrix(M[0], M[1], np.asarray(M[2], np.int32), np.asarray(M[3], np.int32), np.asarray(M[4], np.float64))


@functools.lru_cache(maxsize=None)
def _matrix(name, fmt):
    """(device matrix, what must stay alive with it)"""
    c = DR.case(name)
    if fmt == "ell":
        en, ev = MN.ell_arrays(c.n, c.ptr, c.node, c.val)
        return sg.ellpack_matrix(c.n, c.n, en, ev), ()
    if fmt == "composite":
        rp, cp, blocks = DR.composite_fixture()
        S = sg.sparse_matrix(rp, cp)
        leaves = []
        for (i, j), B in sorted(blocks.items()):
            leaves.append(_csr(B))
            S.set_submatrix(i + 1, j + 1, leaves[-1])
        return S, leaves
    return sg.csr_matrix(c.n, c.n, c.ptr, c.node, c.val), ()


@functools.lru_cache(maxsize=None)
def _pc(name, fmt, pc):
    """(device preconditioner set up on _matrix(name, fmt), what must stay alive with it)"""
    A, _ = _matrix(name, fmt)
    if pc == "none":
        return None, ()
    keep = ()
    if pc == "jacobi":
        p = sg.jacobi()
    elif pc == "ildu":
        p = sg.ldu()
    else:
        keep = [_csr(P) for P in DR.case(name).Ps]
        if pc == "mg":
            p = sg.multigrid(keep, omega=0.8, nu_pre=1, nu_post=1, coarse_sweeps=8)
        else:
            p = sg.multigrid(keep, omega=0.8, nu_pre=2, nu_post=2, coarse="direct")
    p.setup(A)
    return p, keep


def _own_q1(n):
    return 1.5 + np.cos(0.37 * np.arange(n))


@functools.lru_cache(maxsize=None)
def _restated(name, pc, k, ncv, own_q1=False, max_steps=1000):
    c = DR.case(name)
    if pc == "ildu":            # ILDU(0) in natural order: the oracle's factors and sweeps are the device's bit for bit
        import oracle as orc
        M = orc.Ildu(orc.CsrMatrix(c.n, c.n, c.ptr, c.node, c.val))
        return DR.davidson(c.rows, k, ncv, c.q1, M.solve, DR.TOL, max_steps)
    if own_q1:
        return DR.davidson(c.rows, k, ncv, _own_q1(c.n), DR.preconditioner(name, pc), DR.TOL, max_steps)
    return DR.restated(name, pc, k, ncv, "device", DR.TOL, max_steps)


@functools.lru_cache(maxsize=None)
def _device(name, fmt, pc, k, ncv, tensor=False, own_q1=False, max_steps=1000):
    c = DR.case(name)
    A, _ = _matrix(name, fmt)
    p, _ = _pc(name, fmt, pc)
    q1 = _own_q1(c.n) if own_q1 else c.q1
    if tensor:
        import torch
        q1 = torch.tensor(np.array(q1), device="cuda")
    r = sg.davidson(A, k, pc=p, ncv=ncv, tol=DR.TOL, max_steps=max_steps, q1=q1)
    if tensor:
        assert r.V.is_cuda
        r.V = r.V.cpu().numpy()
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _counts(r):
    return (r.steps, r.products, r.applies, r.restarts, r.found, r.converged)


def _same(d, r):
    assert _counts(d) == _counts(r), (_counts(d), _counts(r))
    assert np.array_equal(_bits(d.lam), _bits(r.lam))
    assert np.array_equal(_bits(d.residuals), _bits(r.residuals))
    assert np.array_equal(d.V, r.V)


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name,fmt,pc,k,ncv,tensor,own_q1", PINNED, ids=PINNED_IDS)
def test_device_is_the_restatement_bit_for_bit(name, fmt, pc, k, ncv, tensor, own_q1):
    r = _restated(name, pc, k, ncv, own_q1)
    d = _device(name, fmt, pc, k, ncv, tensor, own_q1)
    print(f"{name} {fmt} {pc} k={k} ncv={ncv}: device {_counts(d)}; restated {_counts(r)}; "
          f"max |lam - restated| {np.max(np.abs(d.lam - r.lam)):.3e}, max |V - restated| {np.max(np.abs(d.V - r.V)):.3e}")
    assert r.converged and r.found == k
    if name == "odd":           # the sums that decide "converged" are left by two workgroups and re-reduced
        assert ER.dot_grid(DR.case(name).n) == 2 and DR.case(name).n % 2 == 1
    if name == "late40":        # the look at the earlier pairs before "converged" finds one that fails
        assert r.relocks >= 1
    if ncv == 8:
        assert r.restarts >= 2
    _same(d, r)


# ------------------------------------------------------------------ 2. independent of the restatement
@pytest.mark.parametrize("nx,ny,k", [(33, 29, 4), (60, 50, 4), (63, 63, 6)], ids=["33x29-k4", "60x50-k4", "63x63-k6"])
def test_eigenpairs_against_mathematics(nx, ny, k):
    """63 x 63 has double eigenvalues (lambda_2 = lambda_3, lambda_5 = lambda_6): the comparison is with multiplicity.  With
    |v_i| = 1 the residual theorem puts an eigenvalue within |A v_i - lam_i v_i|; the reported residual is held to one
    recomputed in longdouble within the forward bound of its float64 evaluation (eigsh_restated.true_residuals); V^T V to
    n eps entrywise."""
    name = f"poisson{nx}x{ny}"
    c = DR.case(name)
    d = _device(name, "csr", "mg", k, 20)
    assert d.converged and d.found == k and np.isfinite(d.lam).all() and np.isfinite(d.V).all()
    exact = DR.cos_spectrum(nx, ny)[:k]
    dist = np.abs(d.lam.astype(np.longdouble) - exact).astype(np.float64)
    R, vn, fwd = DR.true_residuals(c, d.lam, d.V)
    orth = float(np.max(np.abs(d.V.T @ d.V - np.eye(k))))
    print(f"{name} k={k}: steps {d.steps}, products {d.products}, restarts {d.restarts}; max |lam - analytic| {dist.max():.3e}, "
          f"residuals {d.residuals.min():.3e} .. {d.residuals.max():.3e}, max |reported - R| {np.max(np.abs(d.residuals - R)):.3e} "
          f"(bound {fwd.min():.3e}), |V^T V - I| {orth:.3e} (n eps {c.n * ER.EPS:.3e})")
    assert np.all(dist <= d.residuals), (dist, d.residuals)
    assert np.all(np.abs(d.residuals - R) <= fwd), (d.residuals, R, fwd)
    assert orth <= c.n * ER.EPS
    assert np.array_equal(np.argsort(d.lam, kind="stable"), np.arange(k))
    assert d.products == 1 + d.steps + k and d.applies == d.steps


# ------------------------------------------------------------------ 3. grid independence
def test_the_vcycle_makes_the_step_count_grid_independent():
    """k = 4, ncv = 20, tol 1e-8, V(1,1), omega 0.8, 8 coarse sweeps.  A numpy prototype with np.dot sums took 31 steps on
    63 x 63 and 28 on 255 x 255; three steps are the allowance for the contract's order of summation differing from np.dot."""
    small = _device("poisson63x63", "csr", "mg", 4, 20)
    large = _device("poisson255x255", "csr", "mg", 4, 20)
    print(f"63 x 63: {small.steps} steps; 255 x 255: {large.steps} steps")
    assert small.converged and large.converged
    assert large.steps <= small.steps + 3
    exact = DR.cos_spectrum(255, 255)[:4]
    assert np.all(np.abs(large.lam.astype(np.longdouble) - exact).astype(np.float64) <= large.residuals)


# ------------------------------------------------------------------ 4. against Lanczos
def test_fewer_products_than_lanczos_for_the_small_end():
    """100 x 70: the factor of 5 is a floor for "the preconditioner is doing its work", not a performance claim (the
    prototype: 32 against 648)"""
    d = _device("poisson100x70", "csr", "mg", 4, 20)
    A, _ = _matrix("poisson100x70", "csr")
    e = sg.eigsh(A, 4, "SA", ncv=20, tol=1e-8)
    print(f"100 x 70: davidson {d.products} products ({d.steps} steps), eigsh SA {e.products} products ({e.restarts} restarts)")
    assert d.converged and e.converged
    assert 5 * d.products <= e.products


# ------------------------------------------------------------------ 5. ends, refusals, existing routes
def test_max_steps_zero_returns_one_ritz_pair():
    r = _restated("poisson33x29", "mg", 4, 20, max_steps=0)
    d = _device("poisson33x29", "csr", "mg", 4, 20, max_steps=0)
    assert (d.steps, d.products, d.applies, d.restarts, d.found, d.converged) == (0, 2, 0, 0, 1, False)
    assert np.isfinite(d.lam[0]) and np.isnan(d.lam[1:]).all() and np.isnan(d.residuals[1:]).all()
    assert np.array_equal(d.V[:, 1:], np.zeros((DR.case("poisson33x29").n, 3)))
    _same(d, r)


def test_exact_eigenvector_start_ends_with_one_pair_and_no_convergence():
    """diag(1..40) from q1 = 2 e_3 with k = 2: the residual of the only Ritz pair is exactly zero, the space cannot grow"""
    c = DR.case("diag40")
    A, _ = _matrix("diag40", "csr")
    q1 = np.zeros(c.n)
    q1[2] = 2.0
    d = sg.davidson(A, 2, ncv=8, q1=q1)
    r = DR.davidson(c.rows, 2, 8, q1, None)
    assert d.found == 1 and not d.converged and d.steps == 0
    assert d.lam[0] == 3.0 and d.residuals[0] == 0.0 and np.isnan(d.lam[1])
    _same(d, r)


def test_matrix_with_a_nan_never_reports_convergence():
    c = DR.case("poisson33x29")
    val = c.val.copy()
    val[7] = np.nan
    A = sg.csr_matrix(c.n, c.n, c.ptr, c.node, val)
    for pc in (None, sg.jacobi()):
        if pc is not None:
            pc.setup(A)
        d = sg.davidson(A, 4, pc=pc, ncv=20, q1=c.q1)
        assert not d.converged and d.found == 0
        assert np.isnan(d.lam).all() and np.isnan(d.residuals).all()
    # ... and a start vector of zeros (0 * inf) on a sound matrix
    d = sg.davidson(_matrix("poisson33x29", "csr")[0], 4, ncv=20, q1=np.zeros(c.n))
    assert not d.converged and d.found == 0 and d.steps == 0


def test_bad_arguments_and_unsupported_matrices_are_refused_and_the_next_call_works():
    c = DR.case("poisson33x29")
    A, _ = _matrix("poisson33x29", "csr")
    other, _ = _pc("spd300", "csr", "jacobi")                               # set up, but on a matrix of another size
    other_mg, _ = _pc("poisson60x50", "csr", "mg")                          # ... a V-cycle on a larger one
    bad = [dict(k=0), dict(k=4, ncv=4), dict(k=4, ncv=3), dict(k=4, ncv=65), dict(k=4, ncv=c.n), dict(k=4, ncv=2000),
           dict(k=4, tol=2.0 ** -41), dict(k=4, tol=float("nan")), dict(k=4, max_steps=-1), dict(k=4, pc=sg.jacobi()),
           dict(k=4, pc=other), dict(k=4, pc=other_mg)]
    for kw in bad:
        with pytest.raises(sg.SigmaError) as e:
            sg.davidson(A, **kw)
        assert e.value.code == 1, kw
    sg.davidson(A, 4, ncv=64, max_steps=0)                                   # ncv = 64 and tol = 2^-40 are the last accepted values
    sg.davidson(A, 4, tol=2.0 ** -40, max_steps=0)
    Ap = sg.partitioned_csr_matrix(c.n, c.n, c.ptr, c.node, c.val, np.array([0, 480, c.n]))
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(Ap, 4)
    assert e.value.code == 8 and "partitioned" in str(e.value)
    _, _, B, _ = MN.saddle_blocks()
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(_csr(B), 4)
    assert e.value.code == 2
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 4, q1=np.ones(c.n - 1))
    assert e.value.code == 2
    p, _ = _pc("poisson33x29", "csr", "mg")
    _same(sg.davidson(A, 4, pc=p, ncv=20, tol=DR.TOL, q1=c.q1), _restated("poisson33x29", "mg", 4, 20))


def test_default_arguments():
    """ncv = min(n - 1, max(2k + 1, 20)), q1 = the deterministic vector, want_V = False"""
    A, _ = _matrix("poisson33x29", "csr")
    p, _ = _pc("poisson33x29", "csr", "mg")
    d = sg.davidson(A, 4, p, want_V=False)
    r = _restated("poisson33x29", "mg", 4, 20)
    assert d.V is None and _counts(d) == _counts(r)
    assert np.array_equal(_bits(d.lam), _bits(r.lam)) and np.array_equal(_bits(d.residuals), _bits(r.residuals))


def test_eigsh_gives_the_same_bits_before_and_after_davidson():
    c = DR.case("poisson33x29")
    A, _ = _matrix("poisson33x29", "csr")
    p, _ = _pc("poisson33x29", "csr", "mg")
    e0 = sg.eigsh(A, 4, "SA", ncv=20, tol=1e-8, q1=c.q1)
    sg.davidson(A, 4, pc=p, ncv=20, q1=c.q1)
    e1 = sg.eigsh(A, 4, "SA", ncv=20, tol=1e-8, q1=c.q1)
    assert (e0.restarts, e0.products, e0.found, e0.converged) == (e1.restarts, e1.products, e1.found, e1.converged)
    assert np.array_equal(_bits(e0.lam), _bits(e1.lam)) and np.array_equal(_bits(e0.residuals), _bits(e1.residuals))
    assert np.array_equal(_bits(e0.V), _bits(e1.V))


# ------------------------------------------------------------------ 6. the Fortran host layer
def test_fortran_program_reports_the_four_smallest_eigenpairs():
    """davidson_test_hip: the 127 x 127 grid Laplacian (double eigenvalues for i /= j in 4 - 2 cos(i pi / 128) -
    2 cos(j pi / 128)), three runs.  `vcycle` (hip_multigrid, V(1,1)): the four smallest eigenpairs WITH multiplicity -- lam_i
    within the residual the program forms itself of the i-th smallest analytic eigenvalue -- in at most 40 steps.  `jacobi` and
    `none`: the diagonal is constant, so either way the search space is a Krylov space, which holds one vector of every
    eigenspace; of a double eigenvalue one copy is certain, the second arrives through rounding or not at all, as sg.eigsh
    returns them.  There: every lam is an eigenvalue within that residual; they ascend; the first is the smallest; no DISTINCT
    eigenvalue below the largest returned one is missing.  Without the vectors the forward bound is taken in norms, as for
    eigsh_test_hip: reported and own residual differ by at most 2 (gamma_{d+2} (|A|_inf + |lam|) |v| + gamma_n R)."""
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "davidson_test_hip")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("sigma_amd/fortran/davidson_test_hip was not built (no amdflang at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "davidson_test_hip: ok" in p.stdout, p.stdout
    exact = DR.cos_spectrum(127, 127)[:16].astype(np.float64)
    n = 127 * 127
    for label in ("vcycle", "jacobi", "none"):
        counts = re.search(rf"DAVIDSON {label} steps\s+(\d+)\s+products\s+(\d+)\s+applies\s+(\d+)\s+restarts\s+(\d+)", p.stdout)
        assert counts, p.stdout
        steps, products, applies, restarts = (int(g) for g in counts.groups())
        assert products == 1 + steps + 4 and applies == (0 if label == "none" else steps) and restarts >= 2
        pairs = re.findall(rf"DAVIDSON {label} pair\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)", p.stdout)
        assert [int(t[0]) for t in pairs] == [1, 2, 3, 4], p.stdout
        lam, rep, own, vn = (np.array([float(t[i]) for t in pairs]) for i in (1, 2, 3, 4))
        fwd = ER.gamma(5 + 2) * (8.0 + np.abs(lam)) * vn + ER.gamma(n) * np.maximum(rep, own)
        assert np.all(np.abs(rep - own) <= 2 * fwd), (rep, own, fwd)
        dist = np.abs(lam[:, None] - exact[None, :])
        near = np.argmin(dist, axis=1)
        bar = (own + fwd) / vn * (1 + 1e-6) + 16 * ER.EPS * 8.0
        if label == "vcycle":
            assert steps <= 40, steps
            assert np.all(np.abs(lam - exact[:4]) <= bar), (lam, exact[:4], bar)
        assert np.all(dist[np.arange(4), near] <= bar), (lam, exact[near], bar)
        assert near[0] == 0 and np.all(np.diff(lam) >= -2 * bar.max()), lam
        skipped = [e for e in exact[:near.max()] if np.min(np.abs(lam - e)) > bar.max()]
        assert not skipped, (lam, skipped)
        assert np.all(np.abs(vn - 1.0) <= n * ER.EPS)
