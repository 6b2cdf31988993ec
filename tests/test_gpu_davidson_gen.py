"""sg.davidson(A, k, .., B=B) / sgm_davidson_gen on the device (the contract: include/sigma_hip.h, sgm_davidson_gen; DESIGN.md
section 9i).

  1  bit for bit: lam, V, residuals and every count equal the float64 restatement (tests/davidson_gen_restated.py) run with the
     device's defined order of summation -- the shapes are the smallest that reach every code path (the table below);
  2  independent of the restatement: the analytic spectrum of the tensor pairs within the residual bound of the pencil, the
     reported residual against one recomputed in longdouble, V^T B V = I, the counts;
  3  B = I held as a matrix against sg.davidson without B;
  4  ends (max_steps = 0, B = -M, NaN), refusals, sg.davidson without B and sg.eigsh untouched; 5 the Fortran host layer."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import davidson_gen_restated as GR
import davidson_restated as DR
import eigsh_restated as ER
import minres_restated as MN
import sigma_amd as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (pair, storage of A, of B, preconditioner, k, ncv, device tensors, a caller's q1)
#   fem33x29 (n = 957): an odd tail, one workgroup of partial sums; ncv = 8: >= 2 restarts, three bases rotated; ell / ell: the
#   ELLPACK products on both sides; ncv = 40: m passes 32, the <64> instantiations of k_egs2 and k_gdav_ritz
#   fem45x41 (n = 1845): odd, two workgroups of partial sums re-reduced
#   mesh19x17 (n = 323): A and B in different formats; comp32x24 (n = 768): a composite A, a diagonal B
PINNED = [
    ("fem33x29", "csr", "csr", "mg", 4, 20, False, False),
    ("fem33x29", "csr", "csr", "mg", 4, 20, True, False),
    ("fem33x29", "csr", "csr", "mg22direct", 4, 8, False, False),
    ("fem33x29", "ell", "ell", "none", 1, 8, False, False),
    ("fem33x29", "csr", "csr", "none", 4, 40, False, False),
    ("fem45x41", "csr", "csr", "mg", 4, 20, False, True),
    ("mesh19x17", "csr", "ell", "jacobi", 4, 20, False, False),
    ("mesh19x17", "csr", "ell", "ildu", 4, 20, False, False),
    ("comp32x24", "composite", "csr", "none", 1, 8, False, False),
]
PINNED_IDS = [f"{n}-{fa}-{fb}-{p}-k{k}-ncv{m}{'-tensor' if t else ''}{'-q1' if q else ''}" for n, fa, fb, p, k, m, t, q in PINNED]


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _csr(M):
    return sg.csr_matrix(M[0], M[1], np.asarray(M[2], np.int32), np.asarray(M[3], np.int32), np.asarray(M[4], np.float64))


@functools.lru_cache(maxsize=None)
def _matrix(name, which, fmt):
    """(device matrix A or B of the pair, what must stay alive with it)"""
    c = GR.case(name)
    M = c.A if which == "A" else c.B
    if fmt == "ell":
        en, ev = MN.ell_arrays(c.n, M[2], M[3], M[4])
        return sg.ellpack_matrix(c.n, c.n, en, ev), ()
    if fmt == "composite":
        rp, cp, blocks = DR.composite_fixture()
        S = sg.sparse_matrix(rp, cp)
        leaves = []
        for (i, j), Bl in sorted(blocks.items()):
            leaves.append(_csr(Bl))
            S.set_submatrix(i + 1, j + 1, leaves[-1])
        return S, leaves
    return _csr(M), ()


@functools.lru_cache(maxsize=None)
def _pc(name, fmt, pc):
    """(device preconditioner set up on A = _matrix(name, "A", fmt), what must stay alive with it)"""
    A, _ = _matrix(name, "A", fmt)
    if pc == "none":
        return None, ()
    keep = ()
    if pc == "jacobi":
        p = sg.jacobi()
    elif pc == "ildu":
        p = sg.ldu()
    else:
        keep = [_csr(P) for P in GR.case(name).Ps]
        if pc == "mg":
            p = sg.multigrid(keep, omega=0.8, nu_pre=1, nu_post=1, coarse_sweeps=8)
        else:
            p = sg.multigrid(keep, omega=0.8, nu_pre=2, nu_post=2, coarse="direct")
    p.setup(A)
    return p, keep


@functools.lru_cache(maxsize=None)
def _restated(name, pc, k, ncv, own_q1=False, max_steps=1000):
    c = GR.case(name)
    if pc == "ildu":            # ILDU(0) in natural order: the oracle's factors and sweeps are the device's bit for bit
        import oracle as orc
        M = orc.Ildu(orc.CsrMatrix(c.n, c.n, c.A[2], c.A[3], c.A[4]))
        return GR.davidson_gen(c.rowsA, c.rowsB, k, ncv, c.q1, M.solve, GR.TOL, max_steps)
    return GR.restated(name, pc, k, ncv, own_q1, max_steps)


@functools.lru_cache(maxsize=None)
def _device(name, fa, fb, pc, k, ncv, tensor=False, own_q1=False, max_steps=1000):
    c = GR.case(name)
    A, _ = _matrix(name, "A", fa)
    B, _ = _matrix(name, "B", fb)
    p, _ = _pc(name, fa, pc)
    q1 = GR.own_q1(c.n) if own_q1 else c.q1
    if tensor:
        import torch
        q1 = torch.tensor(np.array(q1), device="cuda")
    r = sg.davidson(A, k, pc=p, ncv=ncv, tol=GR.TOL, max_steps=max_steps, q1=q1, B=B)
    if tensor:
        assert r.V.is_cuda
        r.V = r.V.cpu().numpy()
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _counts(r):
    return (r.steps, r.products, r.products_B, r.applies, r.restarts, r.found, r.converged)


def _same(d, r):
    assert _counts(d) == _counts(r), (_counts(d), _counts(r))
    assert np.array_equal(_bits(d.lam), _bits(r.lam))
    assert np.array_equal(_bits(d.residuals), _bits(r.residuals))
    assert np.array_equal(d.V, r.V)


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name,fa,fb,pc,k,ncv,tensor,own_q1", PINNED, ids=PINNED_IDS)
def test_device_is_the_restatement_bit_for_bit(name, fa, fb, pc, k, ncv, tensor, own_q1):
    r = _restated(name, pc, k, ncv, own_q1)
    d = _device(name, fa, fb, pc, k, ncv, tensor, own_q1)
    print(f"{name} {fa}/{fb} {pc} k={k} ncv={ncv}: device {_counts(d)}; restated {_counts(r)}; "
          f"max |lam - restated| {np.max(np.abs(d.lam - r.lam)):.3e}, max |V - restated| {np.max(np.abs(d.V - r.V)):.3e}")
    assert r.converged and r.found == k          # (asserted of every case in tests/test_davidson_gen_cpu.py too)
    n = GR.case(name).n
    if name == "fem45x41":      # the sums that decide "converged" are left by two workgroups and re-reduced
        assert ER.dot_grid(n) == 2 and n % 2 == 1
    if name == "fem33x29":
        assert ER.dot_grid(n) == 1 and n % 2 == 1
    if ncv == 8 and k == 4:
        assert r.restarts >= 2
    if ncv == 40:
        assert r.steps > 32
    _same(d, r)


# ------------------------------------------------------------------ 2. independent of the restatement
@pytest.mark.parametrize("nx,ny", [(33, 29), (60, 50), (45, 41)], ids=["33x29", "60x50", "45x41"])
def test_eigenpairs_against_mathematics(nx, ny):
    """The residual theorem of the pencil puts an eigenvalue within |r_i|_{B^-1} / |v_i|_B of lam_i, r_i = A v_i - lam_i B v_i
    recomputed in longdouble from the returned pair; here it is the i-th analytic one, kappa_a(nx) + kappa_b(ny) ascending.
    The reported residual is held to the longdouble one within the forward bound of its float64 evaluation
    (davidson_gen_restated.true_residuals: two products); V^T B V to n eps entrywise."""
    name, k = f"fem{nx}x{ny}", 4
    c = GR.case(name)
    d = _device(name, "csr", "csr", "mg", k, 20)
    assert d.converged and d.found == k and np.isfinite(d.lam).all() and np.isfinite(d.V).all()
    dist = np.abs(d.lam.astype(np.longdouble) - c.spectrum[:k]).astype(np.float64)
    bound, G = GR.eigenvalue_bounds(c, d.lam, d.V)
    R, fwd = GR.true_residuals(c, d.lam, d.V)
    orth = float(np.max(np.abs(G - np.eye(k))))
    print(f"{name}: steps {d.steps}, products {d.products} / {d.products_B}, restarts {d.restarts}; max |lam - analytic| {dist.max():.3e} "
          f"(bounds {bound.min():.3e} .. {bound.max():.3e}), residuals {d.residuals.min():.3e} .. {d.residuals.max():.3e}, "
          f"max |reported - R| {np.max(np.abs(d.residuals - R)):.3e} (bound {fwd.min():.3e}), |V^T B V - I| {orth:.3e} "
          f"(n eps {c.n * ER.EPS:.3e})")
    assert np.all(dist <= bound), (dist, bound)
    assert np.all(np.abs(d.residuals - R) <= fwd), (d.residuals, R, fwd)
    assert orth <= c.n * ER.EPS
    assert np.array_equal(np.argsort(d.lam, kind="stable"), np.arange(k))
    assert d.products == 1 + d.steps + k and d.products_B == 1 + d.steps + k and d.applies == d.steps


def test_unstructured_pair_finds_the_constant_vector():
    """mesh19x17: A = K + M, B = M with natural boundary conditions, so K 1 = 0 and the smallest eigenvalue is exactly 1"""
    c = GR.case("mesh19x17")
    d = _device("mesh19x17", "csr", "ell", "jacobi", 4, 20)
    bound, _ = GR.eigenvalue_bounds(c, d.lam, d.V)
    print(f"mesh19x17: lam {d.lam}, |lam_0 - 1| {abs(d.lam[0] - 1.0):.3e} (bound {bound[0]:.3e})")
    assert d.converged and abs(d.lam[0] - 1.0) <= bound[0]


# ------------------------------------------------------------------ 3. B = I
def test_identity_mass_matrix_agrees_with_the_standard_call():
    """B = I held as a CSR matrix on poisson33x29: the same eigenvalues as sg.davidson(A, 4, pc) within the sum of the two
    runs' residuals (each lam_i lies within its own residual of the same eigenvalue; |v| = 1 to rounding in both).  Not bit
    for bit: the generalized test divides by |U z|."""
    c = GR.case("poisson33x29")
    A, _ = _matrix("poisson33x29", "A", "csr")
    B, _ = _matrix("poisson33x29", "B", "csr")
    p, _ = _pc("poisson33x29", "csr", "mg")
    s = sg.davidson(A, 4, pc=p, ncv=20, tol=GR.TOL, q1=c.q1)
    g = sg.davidson(A, 4, pc=p, ncv=20, tol=GR.TOL, q1=c.q1, B=B)
    print(f"standard {s.lam} ({s.steps} steps), B = I {g.lam} ({g.steps} steps)")
    assert s.converged and g.converged and s.products_B == 0 and g.products_B == 1 + g.steps + 4
    assert np.all(np.abs(s.lam - g.lam) <= s.residuals + g.residuals), (s.lam, g.lam, s.residuals, g.residuals)


# ------------------------------------------------------------------ 4. ends, refusals, existing routes
def test_max_steps_zero_returns_one_ritz_pair():
    r = _restated("fem33x29", "mg", 4, 20, max_steps=0)
    d = _device("fem33x29", "csr", "csr", "mg", 4, 20, max_steps=0)
    assert _counts(d) == (0, 2, 2, 0, 0, 1, False)
    assert np.isfinite(d.lam[0]) and np.isnan(d.lam[1:]).all() and np.isnan(d.residuals[1:]).all()
    assert np.array_equal(d.V[:, 1:], np.zeros((GR.case("fem33x29").n, 3)))
    _same(d, r)


def test_a_mass_matrix_that_is_not_positive_definite_or_a_nan_never_reports_convergence():
    c = GR.case("fem33x29")
    A, _ = _matrix("fem33x29", "A", "csr")
    B, _ = _matrix("fem33x29", "B", "csr")
    n, _, ptr, node, val = c.B
    nanat = lambda v: np.where(np.arange(len(v)) == 7, np.nan, v)
    for bad in (-val, nanat(val)):                                  # B = -M: d = q1.(B q1) < 0 at the start ; a NaN in B
        d = sg.davidson(A, 4, ncv=20, q1=c.q1, B=sg.csr_matrix(n, n, ptr, node, bad))
        assert _counts(d) == (0, 0, 1, 0, 0, 0, False), _counts(d)
        assert np.isnan(d.lam).all() and np.isnan(d.residuals).all()
    An = sg.csr_matrix(n, n, c.A[2], c.A[3], nanat(c.A[4]))         # a NaN in A
    for pc in (None, sg.jacobi()):
        if pc is not None:
            pc.setup(An)
        d = sg.davidson(An, 4, pc=pc, ncv=20, q1=c.q1, B=B)
        assert not d.converged and d.found == 0 and np.isnan(d.lam).all() and np.isnan(d.residuals).all()
    d = sg.davidson(A, 4, ncv=20, q1=np.zeros(c.n), B=B)            # a start vector of zeros: d = 0
    assert _counts(d) == (0, 0, 1, 0, 0, 0, False)
    _same(sg.davidson(A, 4, pc=_pc("fem33x29", "csr", "mg")[0], ncv=20, tol=GR.TOL, q1=c.q1, B=B), _restated("fem33x29", "mg", 4, 20))


def test_bad_arguments_and_unsupported_matrices_are_refused_and_the_next_call_works():
    c = GR.case("fem33x29")
    A, _ = _matrix("fem33x29", "A", "csr")
    B, _ = _matrix("fem33x29", "B", "csr")
    p, _ = _pc("fem33x29", "csr", "mg")
    good = lambda: _same(sg.davidson(A, 4, pc=p, ncv=20, tol=GR.TOL, q1=c.q1, B=B), _restated("fem33x29", "mg", 4, 20))
    other, _ = _pc("mesh19x17", "csr", "jacobi")                            # set up, but on a matrix of another size
    other_mg, _ = _pc("fem60x50", "csr", "mg")                              # ... a V-cycle on a larger one
    bad = [dict(k=0), dict(k=4, ncv=4), dict(k=4, ncv=3), dict(k=4, ncv=65), dict(k=4, ncv=c.n), dict(k=4, ncv=2000),
           dict(k=4, tol=2.0 ** -41), dict(k=4, tol=float("nan")), dict(k=4, max_steps=-1), dict(k=4, pc=sg.jacobi()),
           dict(k=4, pc=other), dict(k=4, pc=other_mg)]
    for kw in bad:
        with pytest.raises(sg.SigmaError) as e:
            sg.davidson(A, B=B, **kw)
        assert e.value.code == 1, kw
        good()
    sg.davidson(A, 4, ncv=64, max_steps=0, B=B)                              # ncv = 64 and tol = 2^-40 are the last accepted values
    sg.davidson(A, 4, tol=2.0 ** -40, max_steps=0, B=B)
    # a null pointer, B included: only the C ABI can be handed one
    lam, res, info = np.zeros(4), np.zeros(4), np.zeros(7, np.int64)
    q1 = np.array(c.q1)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    tail = lambda q, l, r, i: (C.c_int32(4), C.c_int32(20), C.c_double(1e-8), C.c_int32(10), q, l, None, r, i, C.c_int(sg.SGM_HOST))
    for a_, b_, t in ((A._h, None, tail(ptr(q1), ptr(lam), ptr(res), ptr(info))), (None, B._h, tail(ptr(q1), ptr(lam), ptr(res), ptr(info))),
                      (A._h, B._h, tail(None, ptr(lam), ptr(res), ptr(info))), (A._h, B._h, tail(ptr(q1), None, ptr(res), ptr(info))),
                      (A._h, B._h, tail(ptr(q1), ptr(lam), None, ptr(info))), (A._h, B._h, tail(ptr(q1), ptr(lam), ptr(res), None))):
        assert sg.lib().sgm_davidson_gen(a_, b_, None, *t) == 1
        good()
    # partitioned A, partitioned B
    Mp = lambda M: sg.partitioned_csr_matrix(c.n, c.n, M[2], M[3], M[4], np.array([0, 480, c.n]))
    for kw in (dict(A=Mp(c.A), B=B), dict(A=A, B=Mp(c.B))):
        with pytest.raises(sg.SigmaError) as e:
            sg.davidson(kw["A"], 4, B=kw["B"])
        assert e.value.code == 8 and "partitioned" in str(e.value)
        good()
    # a non-square A, a non-square B, sizes that differ (the last two are refused by sg.davidson itself: through the C ABI)
    _, _, R, _ = MN.saddle_blocks()
    Rm = _csr(R)
    Sq = _matrix("mesh19x17", "B", "csr")[0]
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(Rm, 4, B=Rm)
    assert e.value.code == 2
    good()
    for a_, b_ in ((A._h, Rm._h), (Rm._h, B._h), (A._h, Sq._h)):
        assert sg.lib().sgm_davidson_gen(a_, b_, None, *tail(ptr(q1), ptr(lam), ptr(res), ptr(info))) == 2
        good()
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 4, B=Sq)
    assert e.value.code == 2
    with pytest.raises(sg.SigmaError) as e:
        sg.davidson(A, 4, B=B, q1=np.ones(c.n - 1))
    assert e.value.code == 2
    good()


def test_default_arguments():
    """ncv = min(n - 1, max(2k + 1, 20)), q1 = the deterministic vector, want_V = False"""
    A, _ = _matrix("fem33x29", "A", "csr")
    B, _ = _matrix("fem33x29", "B", "csr")
    p, _ = _pc("fem33x29", "csr", "mg")
    d = sg.davidson(A, 4, p, want_V=False, B=B)
    r = _restated("fem33x29", "mg", 4, 20)
    assert d.V is None and _counts(d) == _counts(r)
    assert np.array_equal(_bits(d.lam), _bits(r.lam)) and np.array_equal(_bits(d.residuals), _bits(r.residuals))


def test_davidson_and_eigsh_give_the_same_bits_before_and_after_a_generalized_call():
    c = GR.case("fem33x29")
    A, _ = _matrix("fem33x29", "A", "csr")
    B, _ = _matrix("fem33x29", "B", "csr")
    p, _ = _pc("fem33x29", "csr", "mg")
    runs = lambda: (sg.davidson(A, 4, pc=p, ncv=20, q1=c.q1), sg.eigsh(A, 4, "SA", ncv=20, tol=1e-8, q1=c.q1))
    d0, e0 = runs()
    sg.davidson(A, 4, pc=p, ncv=20, q1=c.q1, B=B)
    d1, e1 = runs()
    assert (d0.steps, d0.products, d0.products_B, d0.applies, d0.restarts, d0.found, d0.converged) == \
           (d1.steps, d1.products, 0, d1.applies, d1.restarts, d1.found, d1.converged)
    assert (e0.restarts, e0.products, e0.found, e0.converged) == (e1.restarts, e1.products, e1.found, e1.converged)
    for a, b in ((d0, d1), (e0, e1)):
        assert np.array_equal(_bits(a.lam), _bits(b.lam)) and np.array_equal(_bits(a.residuals), _bits(b.residuals))
        assert np.array_equal(_bits(a.V), _bits(b.V))


# ------------------------------------------------------------------ 5. the Fortran host layer
def test_fortran_program_reports_the_four_smallest_eigenpairs_of_the_pencil():
    """davidson_gen_test_hip: the 1-D P1 pair at n = 127 through hip_davidson_gen with hip_jacobi(), 4 pairs, each checked by
    the program against 6 (1 - c_j) / (h^2 (2 + c_j)) within the residual bound it forms itself"""
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "davidson_gen_test_hip")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("sigma_amd/fortran/davidson_gen_test_hip was not built (no amdflang at build time)")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "davidson_gen_test_hip: ok" in p.stdout, p.stdout
