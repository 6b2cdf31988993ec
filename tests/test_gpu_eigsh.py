"""sg.eigsh / sgm_eigsh on the device (the contract: include/sigma_hip.h, sgm_eigsh).

  1  bit for bit: lam, V, residuals, restarts, products, found and converged equal the float64 restatement
     (tests/eigsh_restated.py) run with the device's defined order of summation, with a numpy q1 and again with a device
     tensor; sg.basis_rotate pinned on its own;
  2  independent of the restatement, every case including `outliers` (n = 101,440): the reported residual against the one
     recomputed in longdouble within the forward bound of its float64 evaluation; every lam_i within R_i / |v_i| of the i-th
     extreme exact eigenvalue (residual theorem, one to one: completeness); converged with R_i <= tol |A|_2 + bar_i, bar_i =
     8 x the restatement's own |R_i - rho_i|; orthonormality within 8 x the restatement's;
  3  ends (invariant subspace, too few pairs in it, NaN, max_restarts = 0), 4 refusals, 5 sg.lanczos untouched, 6 Fortran."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import eigsh_restated as ER
import minres_restated as MN
import sigma_amd as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = [(name, fmt, k, ncv, which) for name, fmt in ER.SMALL for (k, ncv) in ER.case_grid(name) for which in ("SA", "LA")]
PINNED_IDS = [f"{n}-{f}-k{k}-ncv{m}-{w}" for n, f, k, m, w in PINNED]
EVERY = PINNED + [("outliers", "csr", 4, 20, "LA")]
EVERY_IDS = PINNED_IDS + ["outliers-csr-k4-ncv20-LA"]


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _csr(M):
    return sg.csr_matrix(M[0], M[1], np.asarray(M[2], np.int32), np.asarray(M[3], np.int32), np.asarray(M[4], np.float64))


@functools.lru_cache(maxsize=None)
def _matrix(name, fmt):
    """(device matrix, what must stay alive with it)"""
    c = ER.case(name)
    if fmt == "ell":
        en, ev = MN.ell_arrays(c.n, c.ptr, c.node, c.val)
        return sg.ellpack_matrix(c.n, c.n, en, ev), ()
    if fmt == "composite":
        K, Bt, B, Cm = MN.saddle_blocks()
        edges = np.array([1, K[0] + 1, K[0] + B[0] + 1], np.int32)
        S = sg.sparse_matrix(edges, edges)
        leaves = [_csr(M) for M in (K, Bt, B, Cm)]
        for (i, j), L in zip(((1, 1), (1, 2), (2, 1), (2, 2)), leaves):
            S.set_submatrix(i, j, L)
        return S, leaves
    return sg.csr_matrix(c.n, c.n, c.ptr, c.node, c.val), ()


@functools.lru_cache(maxsize=None)
def _device(name, fmt, k, ncv, which, tensor=False, max_restarts=200):
    c = ER.case(name)
    A, _ = _matrix(name, fmt)
    q1 = c.q1
    if tensor:
        import torch
        q1 = torch.tensor(np.array(q1), device="cuda")
    r = sg.eigsh(A, k, which=which, ncv=ncv, tol=ER.TOL, max_restarts=max_restarts, q1=q1)
    if tensor:
        assert r.V.is_cuda
        r.V = r.V.cpu().numpy()
    return r


def _restated(name, k, ncv, which, max_restarts=200):
    return ER.restated(name, k, ncv, which, "numpy" if name == "outliers" else "device", ER.TOL, max_restarts)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(d, r):
    assert (d.restarts, d.products, d.found, d.converged) == (r.restarts, r.products, r.found, r.converged)
    assert np.array_equal(_bits(d.lam), _bits(r.lam))
    assert np.array_equal(_bits(d.residuals), _bits(r.residuals))
    assert np.array_equal(d.V, r.V)


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name,fmt,k,ncv,which", PINNED, ids=PINNED_IDS)
def test_device_is_the_restatement_bit_for_bit(name, fmt, k, ncv, which):
    r = _restated(name, k, ncv, which)
    d = _device(name, fmt, k, ncv, which)
    print(f"{name} {fmt} k={k} ncv={ncv} {which}: device restarts {d.restarts} products {d.products}; restated {r.restarts} {r.products}; "
          f"max |lam - restated| {np.max(np.abs(d.lam - r.lam)):.3e}, max |V - restated| {np.max(np.abs(d.V - r.V)):.3e}")
    _same(d, r)
    _same(_device(name, fmt, k, ncv, which, tensor=True), r)


@pytest.mark.parametrize("n,m,kk", [(1, 2, 1), (127, 20, 12), (513, 64, 63), (1845, 33, 5)])
def test_basis_rotate_is_pinned(n, m, kk):
    import torch
    rs = np.random.RandomState(n + m)
    Q, Z = rs.standard_normal((n, m)), rs.standard_normal((m, kk))
    want = ER.rotate(Q, Z)
    got = sg.basis_rotate(Q, Z)
    assert got.shape == (n, kk) and np.array_equal(_bits(got), _bits(want))
    Qt = torch.tensor(np.ascontiguousarray(Q.T), device="cuda")             # the columns as contiguous rows
    out = sg.basis_rotate(Qt, Z)
    assert out.data_ptr() == Qt.data_ptr()                                   # in place
    assert np.array_equal(_bits(out.cpu().numpy().T), _bits(want))
    assert np.array_equal(Qt[kk:].cpu().numpy(), Q.T[kk:])                  # the columns past kk are untouched


# ------------------------------------------------------------------ 2. independent of the restatement
@pytest.mark.parametrize("name,fmt,k,ncv,which", EVERY, ids=EVERY_IDS)
def test_eigenpairs_against_mathematics(name, fmt, k, ncv, which):
    c = ER.case(name)
    d = _device(name, fmt, k, ncv, which)
    r = _restated(name, k, ncv, which)
    assert d.converged and d.found == k and np.isfinite(d.lam).all() and np.isfinite(d.V).all()
    R, vn, fwd = ER.true_residuals(c, d.lam, d.V)
    Rr, _, fwd_r = ER.true_residuals(c, r.lam, r.V)
    bar = 8 * np.abs(Rr - r.rho)
    bar = np.where(bar > 0, bar, fwd_r)
    dist = ER.spectrum_distances(c, d.lam, which)
    orth = float(np.max(np.abs(d.V.T @ d.V - np.eye(k))))
    orth_r = float(np.max(np.abs(r.V.T @ r.V - np.eye(k))))
    print(f"{name} {fmt} k={k} ncv={ncv} {which}: restarts {d.restarts}, products {d.products}; max |reported - R| {np.max(np.abs(d.residuals - R)):.3e} "
          f"(bound {fwd.min():.3e}); max R {R.max():.3e} (tol |A|_2 {ER.TOL * ER.norm2(c):.3e}, bars {bar.min():.3e} .. {bar.max():.3e}); "
          f"max distance to the spectrum {dist.max():.3e}; |V^T V - I| {orth:.3e} (restated {orth_r:.3e})")
    # the reported residual is the true one, within the forward bound of its float64 evaluation
    assert np.all(np.abs(d.residuals - R) <= fwd), (d.residuals, R, fwd)
    # residual theorem, and one to one with the k extreme eigenvalues: completeness
    assert np.all(dist <= R / vn * (1 + 1e-6) + ER.spectrum_slack(c)), (dist, R / vn)
    assert np.array_equal(np.argsort(d.lam if which == "SA" else -d.lam, kind="stable"), np.arange(k))
    # convergence bar
    assert np.all(R <= ER.TOL * ER.norm2(c) + bar), (R, bar)
    assert orth <= 8 * orth_r


# ------------------------------------------------------------------ 3. ends
@pytest.mark.parametrize("which", ["SA", "LA"])
def test_invariant_subspace_with_enough_pairs_is_convergence(which):
    """diag(1..40) from q1 = e1 + e2 + e3: the Krylov space closes at dimension 3"""
    c = ER.case("diag3")
    r = _restated("diag3", 2, 8, which)
    d = _device("diag3", "csr", 2, 8, which)
    assert r.converged and r.found == 2 and np.all(r.rho == 0) and r.restarts == 0 and r.products == 3 + 2
    _same(d, r)
    R, vn, _ = ER.true_residuals(c, d.lam, d.V)
    want = [1.0, 2.0] if which == "SA" else [3.0, 2.0]
    assert np.all(np.abs(d.lam - want) <= R / vn * (1 + 1e-6) + ER.spectrum_slack(c))


def test_invariant_subspace_with_too_few_pairs_is_not_convergence():
    r = _restated("diag3", 5, 8, "SA")
    d = _device("diag3", "csr", 5, 8, "SA")
    assert not d.converged and d.found == 3 and d.restarts == 0
    assert np.isfinite(d.lam[:3]).all() and np.isnan(d.lam[3:]).all() and np.isnan(d.residuals[3:]).all()
    assert np.array_equal(d.V[:, 3:], np.zeros((40, 2)))
    assert np.max(np.abs(d.lam[:3] - [1.0, 2.0, 3.0])) <= 1e-14
    _same(d, r)


def test_matrix_with_a_nan_never_reports_convergence():
    c = ER.case("p32x24")
    val = c.val.copy()
    val[7] = np.nan
    A = sg.csr_matrix(c.n, c.n, c.ptr, c.node, val)
    for which in ("SA", "LA"):
        d = sg.eigsh(A, 4, which=which, ncv=20, tol=ER.TOL, q1=c.q1)
        assert not d.converged and d.found == 0 and d.restarts == 0
        assert np.isnan(d.lam).all() and np.isnan(d.residuals).all()
    # ... and a start vector of zeros (0 / 0) on a sound matrix
    d = sg.eigsh(_matrix("p32x24", "csr")[0], 4, ncv=20, q1=np.zeros(c.n))
    assert not d.converged and d.found == 0


def test_max_restarts_zero_is_one_cycle():
    r = _restated("lap127", 4, 20, "SA", max_restarts=0)
    d = _device("lap127", "csr", 4, 20, "SA", max_restarts=0)
    assert d.restarts == 0 and d.products == 20 + 4 and not d.converged and d.found == 4
    _same(d, r)
    assert np.all(d.residuals > ER.TOL * ER.norm2(ER.case("lap127")))      # one cycle is not enough here: the pairs are returned as they are


def test_default_arguments():
    """ncv = min(n - 1, max(2k + 1, 20)), q1 = the deterministic vector, want_V = False"""
    c = ER.case("lap127")
    A, _ = _matrix("lap127", "csr")
    d = sg.eigsh(A, 4, tol=ER.TOL, want_V=False)
    r = _restated("lap127", 4, 20, "SA")
    assert d.V is None and (d.restarts, d.products) == (r.restarts, r.products)
    assert np.array_equal(_bits(d.lam), _bits(r.lam)) and np.array_equal(_bits(d.residuals), _bits(r.residuals))


# ------------------------------------------------------------------ 4. refusals
def test_bad_arguments_and_unsupported_matrices_are_refused_and_the_next_call_works():
    c = ER.case("lap127")
    A, _ = _matrix("lap127", "csr")
    bad = [dict(k=0), dict(k=4, ncv=4), dict(k=4, ncv=3), dict(k=4, ncv=65), dict(k=4, ncv=127), dict(k=4, ncv=200),
           dict(k=4, tol=2.0 ** -41), dict(k=4, tol=float("nan")), dict(k=4, max_restarts=-1)]
    for kw in bad:
        with pytest.raises(sg.SigmaError) as e:
            sg.eigsh(A, **kw)
        assert e.value.code == 1, kw
    with pytest.raises(sg.SigmaError) as e:
        sg.eigsh(A, 4, which="LM")
    assert e.value.code == 1
    sg.eigsh(A, 4, ncv=64, max_restarts=0)                                   # ncv = 64 and tol = 2^-40 are the last accepted values
    sg.eigsh(A, 4, tol=2.0 ** -40, max_restarts=0)
    Ap = sg.partitioned_csr_matrix(c.n, c.n, c.ptr, c.node, c.val, np.array([0, 64, 127]))
    with pytest.raises(sg.SigmaError) as e:
        sg.eigsh(Ap, 4)
    assert e.value.code == 8 and "partitioned" in str(e.value)
    comm = sg.Comm(0, 1, sg.Comm.unique_id())
    try:
        Ad = sg.dist_csr_matrix(comm, np.array([0, c.n]), c.ptr, c.node, c.val)
        with pytest.raises(sg.SigmaError) as e:
            sg.eigsh(Ad, 4)
        assert e.value.code == 8
        Ad.destroy()
    finally:
        comm.destroy()
    _, _, B, _ = MN.saddle_blocks()
    with pytest.raises(sg.SigmaError) as e:
        sg.eigsh(_csr(B), 4)
    assert e.value.code == 2
    for call in (lambda: sg.basis_rotate(np.zeros((5, 65)), np.zeros((65, 2))), lambda: sg.basis_rotate(np.zeros((5, 3)), np.zeros((3, 0)))):
        with pytest.raises(sg.SigmaError) as e:
            call()
        assert e.value.code == 1
    _same(sg.eigsh(A, 4, ncv=20, tol=ER.TOL, q1=c.q1), _restated("lap127", 4, 20, "SA"))


# ------------------------------------------------------------------ 5. existing routes untouched
def test_lanczos_gives_the_same_t_before_and_after_eigsh():
    c = ER.case("lap127")
    A, _ = _matrix("lap127", "csr")
    T0, Q0 = sg.lanczos(A, 20, c.q1)
    sg.eigsh(A, 4, ncv=20, tol=ER.TOL, q1=c.q1)
    T1, Q1 = sg.lanczos(A, 20, c.q1)
    assert np.array_equal(_bits(T0), _bits(T1)) and np.array_equal(_bits(Q0), _bits(Q1))


# ------------------------------------------------------------------ 6. the Fortran host layer
def test_fortran_program_reports_the_four_smallest_eigenpairs_of_lap127():
    """eigsh_test_hip prints lam_i, the reported residual, the residual it forms itself with A%matvec and |v_i|; without the
    vectors the bounds of group 2 are taken in norms: the 2-norm of |A||v| + |lam||v| is at most (|A|_inf + |lam|) |v|_2 for
    this symmetric matrix, so reported and own residual differ by at most 2 (gamma_{d+2} (|A|_inf + |lam|) |v| + gamma_n R)."""
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "eigsh_test_hip")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("sigma_amd/fortran/eigsh_test_hip was not built (no amdflang at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "eigsh_test_hip: ok" in p.stdout, p.stdout
    c = ER.case("lap127")
    r = _restated("lap127", 4, 20, "SA")
    counts = re.search(r"EIGSH restarts\s+(\d+)\s+products\s+(\d+)", p.stdout)
    assert counts and (int(counts.group(1)), int(counts.group(2))) == (r.restarts, r.products), p.stdout
    pairs = re.findall(r"EIGSH pair\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)", p.stdout)
    assert [int(t[0]) for t in pairs] == [1, 2, 3, 4], p.stdout
    lam, rep, own, vn = (np.array([float(t[i]) for t in pairs]) for i in (1, 2, 3, 4))
    assert np.array_equal(_bits(lam), _bits(r.lam)) and np.array_equal(_bits(rep), _bits(r.residuals))
    ainf = float(np.abs(c.dense).sum(axis=1).max())
    fwd = ER.gamma(c.maxrow + 2) * (ainf + np.abs(lam)) * vn + ER.gamma(c.n) * np.maximum(rep, own)
    assert np.all(np.abs(rep - own) <= 2 * fwd), (rep, own, fwd)
    dist = ER.spectrum_distances(c, lam, "SA")
    assert np.all(dist <= (own + fwd) / vn * (1 + 1e-6) + ER.spectrum_slack(c))
    Rr, _, fwd_r = ER.true_residuals(c, r.lam, r.V)
    bar = np.where(np.abs(Rr - r.rho) > 0, 8 * np.abs(Rr - r.rho), fwd_r)
    assert np.all(own <= ER.TOL * ER.norm2(c) + bar + fwd)
