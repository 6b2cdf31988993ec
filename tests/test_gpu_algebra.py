"""Sparse matrix algebra on the device (sgm_mat_sum / product / ptap / rart, sgm_mat_algebra_refill): bit for bit against
the reference's results (tests/golden/algebra) and against the restated contract (tests/algebra_restated.py) -- ptr and
node equal, values equal as bits (-0.0 != +0.0; NaN positions, not payloads)."""
import glob
import os

import numpy as np
import pytest

import algebra_restated as R
import sigma_amd as sg
from sigma_amd import problems as PB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "algebra", "*.npz")))
CALL = {"sum": sg.sparse_matrix_sum, "product": sg.sparse_matrix_product, "ptap": sg.PtAP, "rart": sg.RARt}


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _dev(m):
    nrow, ncol, ptr, node, val = m
    return sg.csr_matrix(nrow, ncol, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64))


def _read(M):
    return (M.nrow, M.ncol, M.get("ptr", np.int32), M.get("node", np.int32), M.get("val", np.float64))


def _check(got, want):
    assert (got[0], got[1]) == (want[0], want[1])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[3], want[3])
    assert np.array_equal(R.bits(got[4]), R.bits(want[4]))


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_every_fixture_is_reproduced_bit_for_bit(path):
    op, X, Y, Z = R.fixture_operands(np.load(path))
    Xd, Yd = _dev(X), _dev(Y)
    M = CALL[op](Xd, Yd)
    _check(_read(M), Z)
    assert np.array_equal(M.get("val", np.float64).view(np.int64), np.asarray(Z[4]).view(np.int64))


def _operands(rs, op, m, k, n, density, **kw):
    if op == "sum":
        return R.random_csr(rs, m, k, density, **kw), R.random_csr(rs, m, k, density, **kw)
    if op == "product":
        return R.random_csr(rs, m, k, density, **kw), R.random_csr(rs, k, n, density, **kw)
    if op == "ptap":
        return R.random_csr(rs, m, m, density, **kw), R.random_csr(rs, m, n, density, **kw)
    return R.random_csr(rs, m, m, density, **kw), R.random_csr(rs, n, m, density, **kw)


@pytest.mark.parametrize("op", R.OPS)
def test_random_cases_against_the_restatement(op):
    """rectangular shapes, stored duplicate columns in every operand position, +-0, Inf / NaN, empty rows, n = 1"""
    rs = np.random.RandomState(31 + R.OPS.index(op))
    shapes = [(1, 1, 1), (1, 7, 3), (57, 33, 41), (120, 80, 64), (9, 200, 5)]
    for s, (m, k, n) in enumerate(shapes):
        for dup in (0.0, 0.3):
            X, Y = _operands(rs, op, m, k, n, 0.12 if s < 4 else 0.5, dup=dup, zeros=0.1, specials=0.03, empty_rows=0.2)
            got = _read(CALL[op](_dev(X), _dev(Y)))
            _check(got, R.vectorised(op, X, Y))


def test_an_empty_result():
    X = R.random_csr(np.random.RandomState(1), 10, 6, 0.3)
    Y = (6, 4, np.ones(7, np.int32), np.zeros(0, np.int32), np.zeros(0))        # no entries at all
    M = sg.sparse_matrix_product(_dev(X), _dev(Y))
    assert M.nnz == 0
    _check(_read(M), R.vectorised("product", X, Y))
    S = sg.sparse_matrix_sum(_dev(Y), _dev(Y))
    assert S.nnz == 0 and np.array_equal(S.get("ptr", np.int32), np.ones(7, np.int32))


def test_long_rows_take_the_long_row_path_and_stay_exact():
    rs = np.random.RandomState(5)
    # B: row 0 dense (3000 entries), the rest sparse; C: wide rows (about 60 entries) with duplicates
    m, k, n = 40, 3000, 5000
    B = R.random_csr(rs, m, k, 0.002, dup=0.1)
    ptr, node, val = list(B[2]), list(B[3]), list(B[4])
    dense = rs.permutation(k) + 1
    node = list(dense) + node
    val = list(rs.standard_normal(k)) + val
    ptr = [1] + [p + k for p in ptr[1:]]
    B = (m, k, np.array(ptr, np.int32), np.array(node, np.int32), np.array(val))
    Cm = R.random_csr(rs, k, n, 0.012, dup=0.1, zeros=0.05)
    M = sg.sparse_matrix_product(_dev(B), _dev(Cm))
    short, long_ = M.algebra_rows()
    assert long_ >= 1 and short + long_ == m
    _check(_read(M), R.vectorised("product", B, Cm))
    # a long row of a sum, and of a PtAP (a dense column of P)
    S1 = R.random_csr(rs, 8, 400, 0.9, dup=0.2)
    S = sg.sparse_matrix_sum(_dev(S1), _dev(S1))
    assert S.algebra_rows()[1] >= 1
    _check(_read(S), R.vectorised("sum", S1, S1))
    A = R.random_csr(rs, 300, 300, 0.03, dup=0.1)
    P = R.random_csr(rs, 300, 20, 0.3)
    T = sg.PtAP(_dev(A), _dev(P))
    assert T.algebra_rows()[1] >= 1
    _check(_read(T), R.vectorised("ptap", A, P))


def test_mid_size_ptap_and_product_on_a_512_grid():
    nx = 512
    A = (nx * nx, nx * nx) + tuple(PB.poisson2d_csr(nx, nx))
    p = PB.interp2d_csr(nx, nx)
    P = (nx * nx, p[3]) + tuple(p[:3])
    Ad, Pd = _dev(A), _dev(P)
    _check(_read(sg.PtAP(Ad, Pd)), R.vectorised("ptap", A, P))
    M = sg.sparse_matrix_product(Ad, Ad)
    assert M.algebra_rows() == (nx * nx, 0)
    _check(_read(M), R.vectorised("product", A, A))


@pytest.mark.parametrize("op", R.OPS)
def test_refill_equals_a_fresh_build_and_is_refused_after_a_pattern_change(op):
    rs = np.random.RandomState(77 + R.OPS.index(op))
    X, Y = _operands(rs, op, 50, 40, 30, 0.1, dup=0.2, zeros=0.1)
    Xd, Yd = _dev(X), _dev(Y)
    M = CALL[op](Xd, Yd)
    X2 = X[:4] + (rs.standard_normal(len(X[4])),)
    Y2 = Y[:4] + (rs.standard_normal(len(Y[4])),)
    Xd.set_values(X2[4])
    Yd.set_values(Y2[4])
    M.refill(Xd, Yd)
    fresh = _read(CALL[op](Xd, Yd))
    _check(_read(M), fresh)
    _check(fresh, R.vectorised(op, X2, Y2))
    # refused: other handles, operands swapped, an operand permuted, the result permuted
    with pytest.raises(sg.SigmaError) as e:
        M.refill(_dev(X2), Yd)
    assert e.value.code == 1
    with pytest.raises(sg.SigmaError) as e:
        M.refill(Yd, Xd)
    assert e.value.code == 1
    M2 = CALL[op](Xd, Yd)
    Xd.left_permute(np.arange(X[0], 0, -1, dtype=np.int32))
    with pytest.raises(sg.SigmaError) as e:
        M2.refill(Xd, Yd)
    assert e.value.code == 1 and "pattern" in str(e.value)
    Xe, Ye = _dev(X), _dev(Y)
    M3 = CALL[op](Xe, Ye)
    M3.left_permute(np.arange(M3.nrow, 0, -1, dtype=np.int32))
    with pytest.raises(sg.SigmaError) as e:
        M3.refill(Xe, Ye)
    assert e.value.code == 1


def test_dimension_errors_and_unsupported_operands():
    rs = np.random.RandomState(3)
    a = _dev(R.random_csr(rs, 5, 6, 0.5))
    b = _dev(R.random_csr(rs, 6, 6, 0.5))
    c = _dev(R.random_csr(rs, 5, 5, 0.5))
    cases = [(sg.sparse_matrix_sum, a, b), (sg.sparse_matrix_product, a, c), (sg.PtAP, a, b), (sg.PtAP, b, a),
             (sg.RARt, a, b), (sg.RARt, b, c)]
    for f, x, y in cases:
        with pytest.raises(sg.SigmaError) as e:
            f(x, y)
        assert e.value.code == 2, (f.__name__, str(e.value))
    n = 16
    ptr, node, val = PB.poisson2d_csr(4, 4)
    ell = sg.ellpack_matrix(n, n, *_ell_arrays(n, ptr, node, val))
    part = sg.partitioned_csr_matrix(n, n, ptr, node, val, np.array([0, 8, 16], np.int64))
    comp = sg.sparse_matrix(np.array([1, n + 1], np.int32), np.array([1, n + 1], np.int32))
    leaf = sg.csr_matrix(n, n, ptr, node, val)
    comp.set_submatrix(1, 1, leaf)
    comp._build()
    for bad in (ell, part, comp):
        for f in (sg.sparse_matrix_sum, sg.sparse_matrix_product, sg.PtAP, sg.RARt):
            for x, y in ((bad, leaf), (leaf, bad)):
                with pytest.raises(sg.SigmaError) as e:
                    f(x, y)
                assert e.value.code == 8, (f.__name__, str(e.value))


def _ell_arrays(n, ptr, node, val):
    deg = np.diff(ptr)
    md = int(deg.max())
    en = np.zeros((n, md), np.int32)
    ev = np.zeros((n, md))
    for i in range(n):
        cols = node[ptr[i] - 1:ptr[i + 1] - 1]
        en[i, :len(cols)] = cols
        en[i, len(cols):] = cols[-1]
        ev[i, :len(cols)] = val[ptr[i] - 1:ptr[i + 1] - 1]
    return en.ravel(), ev.ravel()


def test_cg_on_the_coarse_operator_matches_the_oracle():
    import oracle as orc
    nx = 33
    A = (nx * nx, nx * nx) + tuple(PB.poisson2d_csr(nx, nx))
    p = PB.interp2d_csr(nx, nx)
    P = (nx * nx, p[3]) + tuple(p[:3])
    Bc = sg.PtAP(_dev(A), _dev(P))
    want = R.vectorised("ptap", A, P)
    _check(_read(Bc), want)
    n = want[0]
    b = np.full(n, 1.0 / n)
    Bo = orc.CsrMatrix(n, n, want[2], want[3], want[4])
    ur, itr, _, _ = orc.cg(Bo, b, tol=1e-12)
    sg.set_option("dot_order", 1)
    try:
        s = sg.cg(1e-12)
        s.setup(Bc)
        u = np.zeros(n)
        s.solve(Bc, u, b)
    finally:
        sg.set_option("dot_order", 0)
    assert s.iterations == itr
    assert np.array_equal(u, ur)
