"""LSQR on the device against its restatement (tests/lsqr_restated.py; the contract: include/sigma_hip.h, sgm_lsqr_create, and
DESIGN.md section 9j).

  1  dot_order = 1: iteration count, stop, res2, history and every bit of x equal the float64 restatement with the sequential dot.
  2  default (tree) dot order: converged with the same stop; the count within +-2 of the tree-order restatement's; a history that
     never increases; the true |A^T (b - A x) - damp^2 (x - x0)|_2 and, on consistent cases, |b - A x|_2 (longdouble, on the
     host) within tol + c eps (|A|_inf |x|_2 + |b|_2) [|A|_inf], c = 8 x what the float64 restatement's own x needs -- computed
     here and printed; the x error against the dense truth within max(8 x the longdouble restatement's, 64 eps).
  3  ends, 4 values changed after setup, 5 refusals, 6 vector placement, 7 live parameters, 8 the Fortran host layer."""
import os
import re
import subprocess

import numpy as np
import pytest

import lsqr_restated as LS
import minres_restated as MN
import sigma_amd as sg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{n}-{f}" for n, f in LS.PAIRS]


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _matrix(c, fmt="csr", val=None):
    val = c.val if val is None else val
    if fmt == "ell":
        en, ev, deg = LS.ell_arrays(c.m, c.ptr, c.node, val)
        return sg.ellpack_matrix(c.m, c.n, en, ev, degrees=deg)
    return sg.csr_matrix(c.m, c.n, c.ptr, c.node, val)


def _small(m, n, ptr, node, val):
    return sg.csr_matrix(m, n, np.array(ptr, np.int32), np.array(node, np.int32), np.array(val, np.float64))


def _solver(c, seq, damp=None, max_iter=None):
    s = sg.lsqr(c.tol, damp=c.damp if damp is None else damp)
    s.set_option("dot_order", 1 if seq else 0)
    s.set_max_iter(c.max_iter if max_iter is None else max_iter)
    s.set_history(c.max_iter + 8)
    return s


def _solve(name, fmt, seq, on_device=False, max_iter=None, A=None):
    c = LS.case(name)
    if A is None:
        A = _matrix(c, fmt)
    s = _solver(c, seq, max_iter=max_iter)
    s.setup(A)
    x, b = c.x0.copy(), c.b
    if on_device:
        import torch
        x, b = torch.tensor(x, device="cuda"), torch.tensor(b, device="cuda")
    s.solve(A, x, b, check=False)
    if on_device:
        x = x.cpu().numpy()
    return s, x, A


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(s, x, r):
    assert s.last_iterations == r.it
    assert s.stop == r.stop and s.converged == r.converged
    assert _bits([s.res2])[0] == _bits([r.res2])[0]
    assert np.array_equal(s.history, r.history)
    assert np.array_equal(_bits(x), _bits(r.x))
    if r.stop != 3:
        assert s.rnorm == r.rnorm and s.arnorm == r.arnorm


# ------------------------------------------------------------------ 1. bit for bit with dot_order = 1
@pytest.mark.parametrize("name,fmt", LS.PAIRS, ids=IDS)
def test_sequential_dot_order_is_the_restatement_bit_for_bit(name, fmt):
    r = LS.restated(name)
    s, x, _ = _solve(name, fmt, seq=True)
    print(f"{name} {fmt}: device {s.last_iterations} iterations, stop {s.stop}, res2 {s.res2!r}; restated {r.it}, {r.stop}, {float(r.res2)!r}")
    _same(s, x, r)


# ------------------------------------------------------------------ 2. default dot order
@pytest.mark.parametrize("name,fmt", LS.PAIRS, ids=IDS)
def test_tree_dot_order_converges_like_the_restatement(name, fmt):
    c, r = LS.case(name), LS.restated(name, "tree")
    s, x, _ = _solve(name, fmt, seq=False)
    rr, nr = LS.true_norms(name, x)
    rbar, nbar, cr, cn = LS.bars(name, x)
    err, xbar = LS.x_error(name, x), LS.x_bar(name)
    print(f"{name} {fmt}: {s.last_iterations} iterations (restated {r.it} in tree order, {LS.restated(name).it} sequential), stop {s.stop}, "
          f"rnorm {s.rnorm:.3e}, arnorm {s.arnorm:.3e}; true |b - A x| {rr:.3e} (bar {rbar:.3e}, c = {cr:.3g}), "
          f"|A^T r - damp^2 (x - x0)| {nr:.3e} (bar {nbar:.3e}, c = {cn:.3g}); x error {err:.3e}, bar {xbar:.3e}")
    assert s.converged and s.stop == r.stop == c.stop
    assert LS.count_ok(s.last_iterations, r.it)
    assert np.isfinite(x).all()
    h = s.history
    assert len(h) == s.last_iterations and np.all(np.diff(h) <= 0)
    assert nr <= nbar
    if name in LS.CONSISTENT:
        assert rr <= rbar
    assert err <= xbar
    if name in ("wide", "incidence13x11", "incidence13x11_consistent"):
        assert np.linalg.norm(LS.dense_solution(name).null.T @ x) <= 64 * LS.EPS * np.linalg.norm(x)


# ------------------------------------------------------------------ 3. ends
def test_zero_right_hand_side_returns_at_once():
    c = LS.case("guess")
    A = _matrix(c)
    s = _solver(c, False)
    s.setup(A)
    x = np.zeros(c.n)
    s.solve(A, x, np.zeros(c.m))
    assert s.last_iterations == 0 and s.stop == 1 and s.converged and s.res2 == 0.0
    assert np.array_equal(x, np.zeros(c.n)) and len(s.history) == 0


@pytest.mark.parametrize("seq", [True, False], ids=["sequential-dot", "tree-dot"])
def test_tiny_systems_end_where_the_contract_says(seq):
    def run(A, n, b):
        s = sg.lsqr(1e-10)
        s.set_option("dot_order", int(seq))
        s.set_max_iter(8)
        s.setup(A)
        x = np.zeros(n)
        s.solve(A, x, np.array(b))
        return s, x
    # the 2 x 2 zero matrix (stored zeros), b = (1, 2): A^T u = 0, alpha = 0
    s, x = run(_small(2, 2, [1, 2, 3], [1, 2], [0.0, 0.0]), 2, [1.0, 2.0])
    assert s.stop == 2 and s.last_iterations == 0 and s.converged and np.array_equal(x, np.zeros(2)) and s.rnorm == np.sqrt(5.0)
    # A = [[1], [0]], b = (0, 1): b is orthogonal to the range
    s, x = run(_small(2, 1, [1, 2, 3], [1, 1], [1.0, 0.0]), 1, [0.0, 1.0])
    assert s.stop == 2 and s.last_iterations == 0 and np.array_equal(x, np.zeros(1))
    # the identity, b = (1, 0): beta' = 0 in step 1; 1.0/beta' is never formed
    s, x = run(_small(2, 2, [1, 2, 3], [1, 2], [1.0, 1.0]), 2, [1.0, 0.0])
    assert s.stop == 1 and s.last_iterations == 1 and s.converged and s.res2 == 0.0
    assert np.array_equal(_bits(x), _bits(np.array([1.0, 0.0])))


def test_matrix_with_a_nan_never_reports_convergence():
    c = LS.case("fit23x17")
    val = c.val.copy()
    val[7] = np.nan
    A = _matrix(c, val=val)
    for seq in (True, False):
        for x0 in (c.x0, LS.case("guess").x0):
            s = _solver(c, seq)
            s.setup(A)
            x = x0.copy()
            s.solve(A, x, c.b)                              # check=True: this end is not an error
            assert not s.converged and s.stop == 3 and np.isnan(s.res2)
            assert np.isfinite(x).all() or np.array_equal(x, x0)
            assert len(s.history) == s.last_iterations


def test_max_iter_stops_the_solve_and_iterations_accumulate():
    c, r = LS.case("fit23x17"), LS.restated("fit23x17")
    s, x, A = _solve("fit23x17", "csr", seq=True, max_iter=5)
    assert s.last_iterations == 5 and not s.converged and s.stop == 0
    assert np.array_equal(s.history, r.history[:5])
    assert s.res2 == r.history[4] * r.history[4]
    assert np.array_equal(_bits(x), _bits(LS.solve(c, max_iter=5).x))
    with pytest.raises(sg.SigmaError) as e:             # the cap is an error unless check=False, as for cg
        s.solve(A, c.x0.copy(), c.b)
    assert e.value.code == 5
    assert s.iterations == 10 and s.last_iterations == 5
    s.set_max_iter(c.max_iter)
    x = c.x0.copy()
    s.solve(A, x, c.b)
    assert s.converged and s.last_iterations == r.it and s.iterations == 10 + r.it
    assert np.array_equal(_bits(x), _bits(r.x))


# ------------------------------------------------------------------ 4. values changed after setup
@pytest.mark.parametrize("fmt", ["csr", "ell"])
def test_values_changed_after_setup_reach_the_cached_transpose(fmt):
    """A.scalar_multiply(2.0) and then a set_value, each followed by a solve WITHOUT a new setup: the restatement on the new
    matrix, bit for bit"""
    c = LS.case("incidence13x11")
    A = _matrix(c, fmt)
    s = _solver(c, True)
    s.setup(A)
    x = c.x0.copy()
    s.solve(A, x, c.b)
    _same(s, x, LS.restated("incidence13x11"))
    A.scalar_multiply(2.0)
    val = 2.0 * c.val
    for step in range(2):
        M = (c.m, c.n, c.ptr, c.node, val)
        r = LS.solve(c, rows=LS.MR._Rows(M), rows_t=LS.MR._Rows(LS.MR.transpose(M)))
        x = c.x0.copy()
        s.solve(A, x, c.b)
        _same(s, x, r)
        assert r.converged and not np.array_equal(r.x, LS.restated("incidence13x11").x)
        if step == 0:                                   # row 6 holds the columns node[10], node[11]
            A.set_value(6, int(c.node[10]), -3.0)
            val = val.copy()
            val[10] = -3.0


# ------------------------------------------------------------------ 5. refusals
def test_partitioned_and_composite_matrices_a_preconditioner_and_short_vectors_are_refused():
    m = MN.case("shifted24")
    Ap = sg.partitioned_csr_matrix(m.n, m.n, m.ptr, m.node, m.val, np.array([0, 288, 576]))
    with pytest.raises(sg.SigmaError) as e:
        sg.lsqr(1e-10).setup(Ap)
    assert e.value.code == 8 and "LSQR" in str(e.value) and "partitioned" in str(e.value)
    K, Bt, B, Cm = MN.saddle_blocks()
    edges = np.array([1, K[0] + 1, K[0] + B[0] + 1], np.int32)
    S = sg.sparse_matrix(edges, edges)
    leaves = [sg.csr_matrix(M[0], M[1], np.asarray(M[2], np.int32), np.asarray(M[3], np.int32), np.asarray(M[4], np.float64))
              for M in (K, Bt, B, Cm)]
    for (i, j), L in zip(((1, 1), (1, 2), (2, 1), (2, 2)), leaves):
        S.set_submatrix(i, j, L)
    with pytest.raises(sg.SigmaError) as e:
        sg.lsqr(1e-10).setup(S)
    assert e.value.code == 8 and "LSQR" in str(e.value) and "composite" in str(e.value)
    # a preconditioner
    A = sg.csr_matrix(m.n, m.n, m.ptr, m.node, m.val)
    pc = sg.jacobi()
    pc.setup(A)
    s = sg.lsqr(1e-10)
    s.setup(A)
    x = np.zeros(m.n)
    with pytest.raises(sg.SigmaError) as e:
        s.solve(A, x, m.b, pc)
    assert e.value.code == 8 and "LSQR" in str(e.value) and np.array_equal(x, np.zeros(m.n))
    # the existing solvers still refuse a rectangular matrix, with the same code
    c = LS.case("fit23x17")
    R = _matrix(c)
    with pytest.raises(sg.SigmaError) as e:
        sg.cg(1e-10).setup(R)
    assert e.value.code == 2 and "non-square" in str(e.value)
    s = sg.lsqr(1e-10)
    s.setup(R)
    for x, b in ((np.zeros(c.n - 1), c.b), (np.zeros(c.n), c.b[:-1]), (np.zeros(c.n), np.zeros(c.n))):
        with pytest.raises(sg.SigmaError) as e:
            s.solve(R, x, b)
        assert e.value.code == 2


# ------------------------------------------------------------------ 6. vector placement
@pytest.mark.parametrize("seq", [True, False], ids=["sequential-dot", "tree-dot"])
def test_device_tensors_give_the_same_bits_and_a_second_solve_takes_no_iterations(seq):
    s, x, A = _solve("guess", "csr", seq)
    s2, x2, _ = _solve("guess", "csr", seq, on_device=True, A=A)
    assert s2.last_iterations == s.last_iterations and s2.res2 == s.res2 and s2.stop == s.stop
    assert np.array_equal(_bits(x2), _bits(x))
    assert np.array_equal(s2.history, s.history)
    # in place from the least-squares solution: alpha beta = |A^T (b - A x)| is below the tolerance before the first step.
    # (The recurrence's arnorm at the end of the first solve is an estimate of it; the true value, in longdouble, is at most
    #  the bar of test 2, which is the tolerance itself on this case: c = 0 there.)
    import torch
    c = LS.case("guess")
    xt, bt = torch.tensor(x, device="cuda"), torch.tensor(c.b, device="cuda")
    before = s.iterations
    s.solve(A, xt, bt)
    assert s.last_iterations == 0 and s.converged and s.stop == 2 and s.iterations == before
    assert np.array_equal(_bits(xt.cpu().numpy()), _bits(x))


# ------------------------------------------------------------------ 7. live parameters
def test_set_params_is_live_on_one_handle():
    c = LS.case("fit23x17")
    A = _matrix(c)
    s = _solver(c, True, damp=0.0)
    s.setup(A)
    x = c.x0.copy()
    s.solve(A, x, c.b)
    _same(s, x, LS.restated("fit23x17"))
    s.damp = 0.5
    x = c.x0.copy()
    s.solve(A, x, c.b)
    r = LS.solve(c, damp=0.5)
    assert r.stop == 2 and r.it < LS.restated("fit23x17").it
    _same(s, x, r)
    s.set_params(c.tol, 1e-4, 0.0)                       # a looser test on A^T r ends the solve earlier, on the same iterates
    x = c.x0.copy()
    s.solve(A, x, c.b)
    r = LS.lsqr(c.rows, c.rows_t, c.b, c.x0, c.tol, 1e-4, 0.0, c.max_iter, LS.seq_dot)
    assert r.it < LS.restated("fit23x17").it
    _same(s, x, r)


# ------------------------------------------------------------------ 8. the Fortran host layer
def test_fortran_program_reports_the_iteration_count_of_fit23x17():
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "lsqr_test_hip")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("sigma_amd/fortran/lsqr_test_hip was not built (no amdflang at build time)")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "lsqr", "fit23x17_b.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.replace("\n ", "")
    assert "lsqr_test_hip: ok" in out, r.stdout
    found = re.search(r"LSQR iterations\s+(\d+)", out)
    assert found and int(found.group(1)) == LS.restated("fit23x17").it, r.stdout
