"""LSQR without a GPU: the restatement the device solve is pinned to (tests/lsqr_restated.py) solves its own cases, and the new
entry points exist in every layer.

The bar on the solution is computed here, never fixed in advance: |x - x*|_2 / |x*|_2 of the float64 restatement is at most 8 x
the same error of the longdouble restatement, with a floor of 64 eps; x* = x0 + pinv(A)(b - A x0) from numpy's SVD (the damped
normal equations' solution with damp)."""
import os
import re

import numpy as np
import pytest

import lsqr_restated as LS
import sigma_amd as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(LS.CASES)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dot", ["seq", "tree", "numpy"])
def test_restatement_stops_as_listed_and_reaches_the_dense_truth(name, dot):
    c, r, rl = LS.case(name), LS.restated(name, dot), LS.restated_ld(name)
    err, bar = LS.x_error(name, r.x), LS.x_bar(name)
    print(f"{name} {dot}: {r.it} iterations (longdouble {rl.it}), stop {r.stop}, rnorm {float(r.rnorm):.3e}, arnorm {float(r.arnorm):.3e}, "
          f"x error {err:.3e}, bar {bar:.3e}")
    assert r.converged and r.stop == c.stop and rl.stop == c.stop
    assert 0 < r.it <= c.max_iter and len(r.history) == r.it
    assert r.res2 == r.rnorm * r.rnorm and r.history[-1] == r.rnorm
    assert (r.rnorm <= c.tol) if r.stop == 1 else (r.arnorm <= c.tol < r.rnorm)
    assert err <= bar


@pytest.mark.parametrize("name", NAMES)
def test_restated_history_never_increases(name):
    h = LS.restated(name).history
    assert np.all(np.diff(h) <= 0) and np.all(h >= 0)


@pytest.mark.parametrize("name", NAMES)
def test_true_norms_of_the_restatement_are_within_their_own_bars(name):
    """the constants the GPU tests give the device 8 x of, printed"""
    x = LS.restated(name).x
    rr, nr = LS.true_norms(name, x)
    rbar, nbar, cr, cn = LS.bars(name, x)
    print(f"{name}: |b - A x| {rr:.3e} (bar {rbar:.3e}, c = {cr:.3g}), |A^T r - damp^2 (x - x0)| {nr:.3e} (bar {nbar:.3e}, c = {cn:.3g})")
    assert nr <= nbar
    if name in LS.CONSISTENT:
        assert rr <= rbar


@pytest.mark.parametrize("name", ["wide", "incidence13x11", "incidence13x11_consistent"])
def test_minimum_norm_solution_is_orthogonal_to_the_null_space(name):
    d, x = LS.dense_solution(name), LS.restated(name).x
    assert d.null.shape[1] == LS.case(name).n - d.rank > 0
    if name.startswith("incidence"):
        assert d.rank == 142 and np.allclose(np.abs(d.null[:, 0]), 1 / np.sqrt(143))       # the constants
    assert np.linalg.norm(d.null.T @ x) <= 64 * LS.EPS * np.linalg.norm(x)


def test_matrices_are_the_ones_the_cases_name():
    c = LS.case("fit23x17")
    assert (c.m, c.n) == (391, 108) and LS.dense_solution("fit23x17").rank == 108
    w = LS.case("wide")
    assert (w.m, w.n) == (108, 391) and np.array_equal(w.dense, c.dense.T)
    i = LS.case("incidence13x11")
    assert (i.m, i.n) == (262, 143) and np.all(i.dense.sum(axis=1) == 0) and np.all(np.abs(i.dense).sum(axis=1) == 2)
    r = LS.case("random2051x1027")
    assert (r.m, r.n) == (2051, 1027) and np.all(np.diag(r.dense) == 4.0) and set(np.diff(r.ptr)) <= {5, 6}
    print("cond:", {n: round(LS.dense_solution(n).cond, 2) for n in ("fit23x17", "incidence13x11", "random2051x1027")})
    assert LS.dense_solution("random2051x1027").cond < 10
    for name in LS.CASES:                       # A^T's rows: source row ascending, then slot
        k = LS.case(name)
        assert np.allclose(k.rows_t.matvec(k.b), k.dense.T @ k.b, rtol=0, atol=1e-12)
        assert np.all(np.diff(k.rows_t.node.reshape(-1)[k.rows_t.ptr[3]:k.rows_t.ptr[4]]) >= 0)


def test_golden_right_hand_side_of_the_fortran_program_is_the_case_s():
    """sigma_amd/fortran/lsqr_test_hip reads b of `fit23x17` from tests/golden/lsqr/fit23x17_b.txt: the same doubles"""
    b = np.loadtxt(os.path.join(ROOT, "tests", "golden", "lsqr", "fit23x17_b.txt"))
    assert np.array_equal(b.view(np.uint64), LS.case("fit23x17").b.view(np.uint64))


def test_tree_dot_above_one_workgroup_is_a_sum_of_the_same_products():
    rs = np.random.RandomState(3)
    for n in (391, 1024, 1027, 2051):
        a = rs.standard_normal(n)
        exact = float(np.dot(a.astype(np.longdouble), a.astype(np.longdouble)))
        assert abs(LS.tree_dot(a, a) - exact) <= 14 * LS.EPS * exact            # (a tree of depth <= 14 over <= 2051 products)
    a = rs.standard_normal(1024)
    assert LS.tree_dot(a, a) == LS.MN.tree_dot(a, a)


@pytest.mark.parametrize("name", NAMES)
def test_agrees_with_scipy_at_a_fixed_iteration_count_and_in_the_count(name):
    """scipy's stopping tests are relative (atol, btol against its running norm estimates), so the iterates are compared at the
    restatement's own count with scipy's tests off; the count itself with scipy's atol / btol chosen so that its tests are the
    restatement's absolute ones at the end: |r| <= btol |b| and |A^T r| <= atol anorm |r|, anorm its running estimate of |A|_F."""
    spl = pytest.importorskip("scipy.sparse.linalg")
    sp = pytest.importorskip("scipy.sparse")
    c, r = LS.case(name), LS.restated(name, "numpy")
    A = sp.csr_matrix((c.val, c.node - 1, c.ptr - 1), shape=(c.m, c.n))
    out = spl.lsqr(A, c.b, damp=c.damp, atol=0.0, btol=0.0, conlim=0.0, iter_lim=r.it, x0=c.x0 if name == "guess" else None)
    x = out[0]
    err = float(np.linalg.norm(x - r.x) / np.linalg.norm(r.x))
    print(f"{name}: scipy at {r.it} iterations: |x - restated| / |restated| {err:.3e}, bar {LS.x_bar(name):.3e}; scipy r1norm {out[3]:.3e}, "
          f"arnorm {out[7]:.3e}, restated {float(r.rnorm):.3e}, {float(r.arnorm):.3e}")
    assert out[2] == r.it and err <= LS.x_bar(name) and LS.x_error(name, x) <= LS.x_bar(name)
    r0 = c.b - c.dense @ c.x0
    if r.stop == 1:
        kw = dict(atol=0.0, btol=c.tol / float(np.linalg.norm(r0)))
    else:                                       # (out[4], out[5]: scipy's own r2norm and its running estimate of |A|_F at that count)
        kw = dict(atol=c.tol / (out[5] * out[4]), btol=0.0)
    out = spl.lsqr(A, c.b, damp=c.damp, conlim=0.0, iter_lim=c.max_iter, x0=c.x0 if name == "guess" else None, **kw)
    print(f"{name}: scipy stops at {out[2]} (istop {out[1]}), restated at {r.it}")
    assert out[1] in (1, 2) and abs(out[2] - r.it) <= 1


def test_ends_of_the_restatement():
    R = lambda m, n, ptr, node, val: (LS.MR._Rows((m, n, np.array(ptr), np.array(node), np.array(val, np.float64))),
                                      LS.MR._Rows(LS.MR.transpose((m, n, np.array(ptr), np.array(node), np.array(val, np.float64)))))
    c = LS.case("fit23x17")
    r = LS.solve(c, b=np.zeros(c.m))
    assert r.stop == 1 and r.it == 0 and np.array_equal(r.x, c.x0) and r.res2 == 0.0
    Z = R(2, 2, [1, 2, 3], [1, 2], [0.0, 0.0])
    r = LS.lsqr(*Z, np.array([1.0, 2.0]), np.zeros(2))
    assert r.stop == 2 and r.it == 0 and r.converged and r.rnorm == np.sqrt(5.0)
    T = R(2, 1, [1, 2, 3], [1, 1], [1.0, 0.0])
    r = LS.lsqr(*T, np.array([0.0, 1.0]), np.zeros(1))
    assert r.stop == 2 and r.it == 0 and np.array_equal(r.x, np.zeros(1))
    I2 = R(2, 2, [1, 2, 3], [1, 2], [1.0, 1.0])
    r = LS.lsqr(*I2, np.array([1.0, 0.0]), np.zeros(2))
    assert r.stop == 1 and r.it == 1 and np.array_equal(r.x, np.array([1.0, 0.0])) and r.rnorm == 0.0
    val = c.val.copy()
    val[7] = np.nan
    M = (c.m, c.n, c.ptr, c.node, val)
    r = LS.solve(c, rows=LS.MR._Rows(M), rows_t=LS.MR._Rows(LS.MR.transpose(M)))
    assert r.stop == 3 and not r.converged and np.isnan(r.res2) and np.isfinite(r.x).all()
    r5 = LS.solve(c, max_iter=5)
    assert r5.stop == 0 and r5.it == 5 and not r5.converged and np.array_equal(r5.history, LS.restated("fit23x17").history[:5])


def test_damped_case_accumulates_psi_and_solves_another_problem():
    """`damped` is there for the Psi accumulation: its rnorm stays above sqrt(Psi) > 0 while arnorm goes to the tolerance"""
    r = LS.restated("damped")
    assert r.stop == 2 and r.rnorm > 1.0 and r.arnorm <= LS.TOL
    assert LS.x_error("damped", LS.restated("fit23x17").x) > 1e-3          # (another problem than the undamped one)


def test_python_layer_has_lsqr_and_the_library_exports_it():
    """(fails without the feature)"""
    assert hasattr(sg, "lsqr")
    s = sg.lsqr()
    assert isinstance(s, sg.lsqr_solver) and s.tolerance == 1e-16 and s.normal_tolerance == 1e-16 and s.damp == 0.0
    s = sg.lsqr(1e-8, damp=0.5)
    assert (s.tolerance, s.normal_tolerance, s.damp) == (1e-8, 1e-8, 0.5)
    assert sg.lsqr(1e-8, 1e-6).normal_tolerance == 1e-6
    sg.build()
    for f in ("sgm_lsqr_create", "sgm_lsqr_set_params", "sgm_lsqr_info"):
        assert hasattr(sg.lib(), f)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigma_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sgm_lsqr_create\s*\(\s*sgm_solver\s*\*\s*out\s*,\s*double\s+tolerance\s*,\s*double\s+normal_tolerance\s*,"
                     r"\s*double\s+damp\s*\)\s*;", txt)
    assert re.search(r"\bSGM_SOLVER_LSQR\s*=\s*5\b", txt)
    f90 = open(os.path.join(ROOT, "sigma_amd", "fortran", "sigma_hip.f90")).read()
    for f in ("sgm_lsqr_create", "sgm_lsqr_set_params", "sgm_lsqr_info"):
        assert f"bind(c, name='{f}')" in f90


def test_bad_creation_parameters_are_refused_and_setup_fails_loudly_without_a_gpu():
    import ctypes as C
    sg.build()
    h = C.c_void_p()
    for ntol, damp in ((-1.0, 0.0), (float("nan"), 0.0), (1e-8, -0.5), (1e-8, float("nan"))):
        assert sg.lib().sgm_lsqr_create(C.byref(h), C.c_double(1e-8), C.c_double(ntol), C.c_double(damp)) == 1
    assert sg.lib().sgm_lsqr_create(C.byref(h), C.c_double(1e-8), C.c_double(1e-8), C.c_double(0.5)) == 0
    assert sg.lib().sgm_lsqr_set_params(h, C.c_double(-1.0), C.c_double(0.0)) == 1
    assert sg.lib().sgm_lsqr_set_params(h, C.c_double(1e-6), C.c_double(0.25)) == 0
    assert sg.lib().sgm_solver_destroy(h) == 0
    try:
        import torch
        if torch.cuda.is_available():
            return
    except ImportError:
        pass
    c = LS.case("fit23x17")
    with pytest.raises(sg.SigmaError) as e:
        A = sg.csr_matrix(c.m, c.n, c.ptr, c.node, c.val)
        sg.lsqr(1e-10).setup(A)
    assert e.value.code == 6
