"""Sparse matrix algebra without a GPU: the two restatements of the contract (tests/algebra_restated.py) against the
reference's own results (tests/golden/algebra, made by tools/algebra_golden) and against each other, scipy as a sanity
check, and the five C entry points refusing null handles without crashing."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import algebra_restated as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "algebra", "*.npz")))


def test_the_algebra_fixtures_are_there_and_cover_all_four_operations():
    assert len(FIXTURES) >= 7
    ops = {R.fixture_operands(np.load(f))[0] for f in FIXTURES}
    assert ops == set(R.OPS)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_literal_transcription_reproduces_the_reference_fixture_bit_for_bit(path):
    op, X, Y, Z = R.fixture_operands(np.load(path))
    got = R.literal(op, X, Y)
    assert R.same(got, Z)
    assert np.array_equal(got[4].view(np.int64), np.asarray(Z[4]).view(np.int64))    # (no NaN in the fixtures: raw bits)


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_vectorised_restatement_reproduces_the_reference_fixture_bit_for_bit(path):
    op, X, Y, Z = R.fixture_operands(np.load(path))
    assert R.same(R.vectorised(op, X, Y), Z)


def _random_operands(rs, op, dup, zeros, specials):
    m, k, n = (int(v) for v in rs.randint(1, 40, size=3))
    kw = dict(dup=dup, zeros=zeros, specials=specials, empty_rows=0.15)
    if op == "sum":
        return R.random_csr(rs, m, k, 0.2, **kw), R.random_csr(rs, m, k, 0.2, **kw)
    if op == "product":
        return R.random_csr(rs, m, k, 0.15, **kw), R.random_csr(rs, k, n, 0.15, **kw)
    if op == "ptap":
        return R.random_csr(rs, m, m, 0.15, **kw), R.random_csr(rs, m, n, 0.15, **kw)
    return R.random_csr(rs, m, m, 0.15, **kw), R.random_csr(rs, n, m, 0.15, **kw)


@pytest.mark.parametrize("op", R.OPS)
@pytest.mark.parametrize("seed", range(6))
def test_vectorised_restatement_equals_the_literal_one_on_random_inputs(op, seed):
    """stored duplicate columns, explicit +-0, Inf / NaN, empty rows and columns, rectangular shapes"""
    rs = np.random.RandomState(1000 * seed + R.OPS.index(op))
    X, Y = _random_operands(rs, op, dup=0.2 if seed % 2 else 0.0, zeros=0.1, specials=0.05 if seed >= 4 else 0.0)
    assert R.same(R.vectorised(op, X, Y), R.literal(op, X, Y))


def test_restatement_orders_columns_by_first_appearance_and_keeps_duplicate_terms():
    # B = [[1 at col 3, 2 at col 1]], C rows: row 3 -> cols (2, 1), row 1 -> cols (1, 1 again)
    B = (1, 3, np.array([1, 3], np.int32), np.array([3, 1], np.int32), np.array([1.0, 2.0]))
    Cm = (3, 2, np.array([1, 3, 3, 5], np.int32), np.array([1, 1, 2, 1], np.int32), np.array([10.0, 20.0, 30.0, 40.0]))
    for f in (R.literal, R.vectorised):
        _, _, ptr, node, val = f("product", B, Cm)
        assert list(ptr) == [1, 3] and list(node) == [2, 1]
        assert list(val) == [30.0, ((0.0 + 40.0) + 20.0) + 40.0]
    # a single term of -0.0 gives +0.0
    Z = (1, 1, np.array([1, 2], np.int32), np.array([1], np.int32), np.array([-0.0]))
    E = (1, 1, np.array([1, 1], np.int32), np.zeros(0, np.int32), np.zeros(0))
    for f in (R.literal, R.vectorised):
        assert f("sum", Z, E)[4].view(np.int64)[0] == 0


@pytest.mark.parametrize("op", R.OPS)
def test_restatements_agree_with_scipy_to_rounding(op):
    sp = pytest.importorskip("scipy.sparse")
    rs = np.random.RandomState(7 + R.OPS.index(op))
    X, Y = _random_operands(rs, op, dup=0.2, zeros=0.0, specials=0.0)

    def S(m):
        nrow, ncol, ptr, node, val = m
        return sp.csr_matrix((val, np.asarray(node) - 1, np.asarray(ptr) - 1), shape=(nrow, ncol))   # duplicates summed

    want = {"sum": lambda: S(X) + S(Y), "product": lambda: S(X) @ S(Y), "ptap": lambda: S(Y).T @ S(X) @ S(Y),
            "rart": lambda: S(Y) @ S(X) @ S(Y).T}[op]().toarray()
    for f in (R.literal, R.vectorised):
        got = S(f(op, X, Y)).toarray()
        assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(want).max()))


def test_the_five_entry_points_refuse_null_handles_without_crashing():
    import sigma_amd as sg
    L = sg.lib()
    h = C.c_void_p()
    for name in ("sgm_mat_sum", "sgm_mat_product", "sgm_mat_ptap", "sgm_mat_rart"):
        rc = getattr(L, name)(C.byref(h), C.c_void_p(), C.c_void_p())
        assert rc in (6, 1), (name, rc)            # SGM_ERR_NO_DEVICE without a GPU, SGM_ERR_BAD_ARG with one
        assert not h.value
        assert L.sgm_last_error()
        rc = getattr(L, name)(None, C.c_void_p(), C.c_void_p())
        assert rc in (6, 1), (name, rc)
    rc = L.sgm_mat_algebra_refill(C.c_void_p(), C.c_void_p(), C.c_void_p())
    assert rc in (6, 1), rc


def test_the_python_names_are_the_references():
    import sigma_amd as sg
    for name in ("sparse_matrix_sum", "sparse_matrix_product", "PtAP", "RARt"):
        assert callable(getattr(sg, name))
    assert callable(sg.csr_matrix.refill)
