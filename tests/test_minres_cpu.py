"""MINRES without a GPU: the restatement the device solve is pinned to (tests/minres_restated.py) solves its own cases, and
the new entry point exists in every layer.

The bar on the solution is computed here, never fixed in advance: |x - x_dense|_inf / |x_dense|_inf of the float64 restatement
is at most 8 x the same error of the longdouble restatement, with a floor of 64 eps cond(A); x_dense = numpy.linalg.solve on
the dense matrix."""
import os
import re

import numpy as np
import pytest

import minres_restated as MN
import sigma_amd as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{n}-{p}" for n, p in MN.PAIRS]


@pytest.mark.parametrize("name,pc", MN.PAIRS, ids=IDS)
@pytest.mark.parametrize("dot", ["seq", "tree", "numpy"])
def test_restatement_reaches_the_tolerance_and_the_dense_solution(name, pc, dot):
    c, r = MN.case(name), MN.restated(name, pc, dot)
    assert r.converged and r.failed == ""
    assert r.it <= c.max_iter and len(r.history) == r.it
    assert np.sqrt(r.res2) <= c.tol
    if name == "zero_rhs":
        assert r.it == 0 and r.res2 == 0.0 and np.array_equal(r.x, np.zeros(c.n))
        return
    err, bar = MN.x_error(name, r.x), MN.x_bar(name, pc)
    print(f"{name} {pc}: {r.it} iterations (longdouble {MN.restated_ld(name, pc).it}), x error {err:.3e}, bar {bar:.3e}")
    assert MN.restated_ld(name, pc).converged
    assert err <= bar


@pytest.mark.parametrize("name,pc", MN.PAIRS, ids=IDS)
def test_restated_history_never_increases(name, pc):
    h = MN.restated(name, pc).history
    assert np.all(np.diff(h) <= 0)
    assert np.all(h >= 0)


def test_sequential_dot_is_one_accumulator_first_to_last():
    a = np.array([1e16, 1.0, -1e16, 1.0])
    b = np.ones(4)
    assert MN.seq_dot(a, b) == 1.0                    # ((1e16 + 1) - 1e16) + 1: the first 1 is lost, the last is not
    assert MN.seq_dot(a[:0], b[:0]) == 0.0


def test_tree_dot_is_a_sum_of_the_same_products_in_another_order():
    rs = np.random.RandomState(3)
    for n in (1, 2, 63, 391, 576, 957, 1024):
        a, b = rs.standard_normal(n), rs.standard_normal(n)
        exact = float(np.dot(a.astype(np.longdouble), b.astype(np.longdouble)))
        scale = float(np.dot(np.abs(a), np.abs(b)))
        assert abs(MN.tree_dot(a, b) - exact) <= 12 * MN.EPS * scale          # (a tree of depth <= 12 over <= 1024 products)
    a = np.arange(1.0, 9.0)
    assert MN.tree_dot(a, np.ones(8)) == 36.0


def test_iteration_count_depends_on_the_order_of_the_dot_products():
    """Why the default-order device solve is compared with the restatement run in the device's own order: in float64 the
    count of the cases past 100 iterations moves by about five with the order of summation alone (the Lanczos vectors have
    lost their orthogonality to rounding by then; longdouble needs fewer steps still) -- more than the 2 % the count is held
    to.  The figures are printed, only their existence is asserted."""
    spread = {}
    for name, pc in (("shifted23x17_ell", "none"), ("guess", "none")):
        its = {d: MN.restated(name, pc, d).it for d in MN.DOTS}
        its["longdouble"] = MN.restated_ld(name, pc).it
        print(name, its)
        spread[name] = max(its.values()) - min(its.values())
    assert max(spread.values()) >= 4


def test_ends_that_are_not_convergence():
    """a preconditioner with a negative entry (bb < 0), gamma == 0 (A = 0), a NaN in the matrix: never converged, x is the
    last iterate that was finished"""
    c = MN.case("shifted24")
    idiag = c.rows.idiag().copy()
    idiag[100] = 1.0 / -1.0
    r = MN.minres(c.rows, c.b, c.x0, lambda u: idiag * u, c.tol, c.max_iter, MN.seq_dot)
    assert not r.converged and r.failed == "bb" and np.isnan(r.res2) and np.isfinite(r.x).all() and len(r.history) == r.it
    Z = MN.MR._Rows((2, 2, np.array([1, 2, 3]), np.array([1, 2]), np.zeros(2)))
    r = MN.minres(Z, np.array([1.0, 2.0]), np.zeros(2), None, 1e-10, 8, MN.seq_dot)
    assert not r.converged and r.failed == "gamma" and r.it == 0 and r.res2 == np.sqrt(5.0) * np.sqrt(5.0) and np.array_equal(r.x, np.zeros(2))
    val = c.val.copy()
    val[7] = np.nan
    N = MN.MR._Rows((c.n, c.n, c.ptr, c.node, val))
    r = MN.minres(N, c.b, c.x0, None, c.tol, c.max_iter, MN.seq_dot)
    assert not r.converged and np.isnan(r.res2) and r.it == 0 and np.array_equal(r.x, c.x0)


def test_saddle_matrix_is_symmetric_indefinite_and_the_blocks_assemble_to_it():
    c = MN.case("saddle")
    assert np.array_equal(c.dense, c.dense.T)
    ev = np.linalg.eigvalsh(c.dense)
    assert ev[0] < 0 < ev[-1]
    K, Bt, B, Cm = MN.saddle_blocks()
    def dense(M):
        D = np.zeros((M[0], M[1]))
        D[np.repeat(np.arange(M[0]), np.diff(M[2])), M[3] - 1] = M[4]
        return D
    assert np.array_equal(np.block([[dense(K), dense(Bt)], [dense(B), dense(Cm)]]), c.dense)
    assert np.array_equal(dense(Bt), dense(B).T)
    for name in ("shifted24", "shifted23x17_ell", "n1", "n2"):
        d = MN.case(name).dense
        assert np.array_equal(d, d.T) and np.linalg.eigvalsh(d)[0] < 0


def test_python_layer_has_minres():
    assert hasattr(sg, "minres")
    s = sg.minres()
    assert isinstance(s, sg.minres_solver) and s.tolerance == 1e-16
    assert sg.minres(1e-8).tolerance == 1e-8


def test_library_exports_sgm_minres_create_and_the_header_declares_it():
    sg.build()
    assert hasattr(sg.lib(), "sgm_minres_create")
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigma_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+sgm_minres_create\s*\(\s*sgm_solver\s*\*\s*out\s*,\s*double\s+tolerance\s*\)\s*;", txt)
    assert re.search(r"\bSGM_SOLVER_MINRES\s*=\s*4\b", txt)
    f90 = open(os.path.join(ROOT, "sigma_amd", "fortran", "sigma_hip.f90")).read()
    assert "bind(c, name='sgm_minres_create')" in f90
