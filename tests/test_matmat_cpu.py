"""Multi-vector products without a GPU: the numpy restatement of the contract (tests/matmat_restated.py) equals the oracle's
single-vector products column by column, the library exports the three entry points in every layer, and the block
decomposition restated in Python gives the widths include/sigma_hip.h states."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fused_dot_cases as F
import matmat_restated as MM
import oracle as orc
import sigma_amd as sg
from sigma_amd import problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPORTS = ("sgm_mat_matmat", "sgm_mat_matmat_kernel", "sgm_mat_matmat_probe")
K = 5


def _csr_case(st, seed):
    rs = np.random.RandomState(seed)
    return orc.CsrMatrix(st["n"], st["m"], st["ptr"], st["node"], rs.standard_normal(st["node"].size))


def _grid5():
    return _csr_case(F.grid5(17, 13), 1)


def _banded():
    return _csr_case(F.banded_short_rows(513, 613, 8), 2)


def _interp():
    ptr, node, val, nc = P.interp2d_csr(9, 7)
    return orc.CsrMatrix(63, nc, ptr, node, val)


def _signed_zero():
    """Every product is -0.0 (values -0.0 times positive x) or +0.0 * -x: row sums that are zeros of either sign on the way."""
    st = F.grid5(6, 5)
    val = np.where(np.arange(st["node"].size) % 3 == 0, 0.0, -0.0)
    return orc.CsrMatrix(st["n"], st["m"], st["ptr"], st["node"], val)


def _ell_grid5():
    ptr, node, _ = P.poisson2d_csr(11, 7)
    ei = np.repeat(np.arange(1, 78, dtype=np.int32), np.diff(ptr))
    rs = np.random.RandomState(3)
    return orc.EllMatrix.from_edges(77, 77, ei, node, rs.standard_normal(node.size))


CASES = {"grid5_17x13": _grid5, "banded_513_w8": _banded, "interp2d_9x7": _interp, "signed_zero": _signed_zero,
         "ell_grid5_11x7": _ell_grid5}


def _blocks(A, name):
    rs = np.random.RandomState(len(name))
    X = np.asfortranarray(rs.standard_normal((A.m, K)))
    Xt = np.asfortranarray(rs.standard_normal((A.n, K)))
    Y0 = np.asfortranarray(rs.standard_normal((A.n, K)))
    Yt0 = np.asfortranarray(rs.standard_normal((A.m, K)))
    if name == "signed_zero":
        X, Xt = np.abs(X) + 1.0, np.abs(Xt) + 1.0
        X[:, 1] *= -1.0
        Y0[:], Yt0[:] = -0.0, -0.0
        Y0[::2, 2], Yt0[::2, 2] = 0.0, 0.0
    return X, Xt, Y0, Yt0


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_oracle_column_by_column(name):
    A = CASES[name]()
    X, Xt, Y0, Yt0 = _blocks(A, name)
    Y = MM.matmat(A, X)
    Ya = MM.matmat(A, X, Y0, MM.OP_ADD)
    Yt = MM.matmat(A, Xt, None, MM.OP_TRANS)
    Yta = MM.matmat(A, Xt, Yt0, MM.OP_TRANS | MM.OP_ADD)
    assert Y.shape == (A.n, K) and Yt.shape == (A.m, K)
    for j in range(K):
        x, xt = np.ascontiguousarray(X[:, j]), np.ascontiguousarray(Xt[:, j])
        # the bits, signed zeros included
        assert np.array_equal(_bits(Y[:, j]), _bits(A.matvec(x))), (name, j, "matvec")
        assert np.array_equal(_bits(Ya[:, j]), _bits(A.matvec_add(x, Y0[:, j].copy()))), (name, j, "matvec_add")
        assert np.array_equal(_bits(Yt[:, j]), _bits(A.matvec_t(xt))), (name, j, "matvec_t")
        assert np.array_equal(_bits(Yta[:, j]), _bits(A.matvec_t_add(xt, Yt0[:, j].copy()))), (name, j, "matvec_t_add")


def test_signed_zero_case_really_meets_both_zeros():
    A = CASES["signed_zero"]()
    X, Xt, Y0, Yt0 = _blocks(A, "signed_zero")
    Y = MM.matmat(A, X)
    assert not np.signbit(Y).any()                      # 0.0 + (-0.0) is +0.0
    Yta = MM.matmat(A, Xt, Yt0, MM.OP_TRANS | MM.OP_ADD)
    assert np.signbit(Yta).any() and not np.signbit(Yta).all()      # the chained sum keeps a -0.0 it started from


def test_library_exports_the_three_entry_points_in_every_layer():
    """(fails without the feature)"""
    sg.build()
    for f in EXPORTS:
        assert hasattr(sg.lib(), f), f
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sigma_hip.h")).read(), flags=re.S)
    assert re.search(r"#define\s+SGM_OP_ADD\s+1\b", txt) and re.search(r"#define\s+SGM_OP_TRANS\s+2\b", txt)
    assert re.search(r"\bint\s+sgm_mat_matmat\s*\(\s*sgm_mat\s+A\s*,\s*int32_t\s+op\s*,\s*int32_t\s+k\s*,\s*const\s+double\s*\*\s*X\s*,"
                     r"\s*int64_t\s+ldx\s*,\s*double\s*\*\s*Y\s*,\s*int64_t\s+ldy\s*,\s*int\s+where\s*\)\s*;", txt)
    assert re.search(r"\bint\s+sgm_mat_matmat_kernel\s*\(\s*sgm_mat\s+A\s*,\s*int32_t\s+op\s*,\s*int32_t\s+k\s*,\s*char\s*\*\s*buf\s*,"
                     r"\s*int\s+len\s*\)\s*;", txt)
    assert re.search(r"\bint\s+sgm_mat_matmat_probe\s*\(", txt)
    f90 = open(os.path.join(ROOT, "sigma_amd", "fortran", "sigma_hip.f90")).read()
    for f in EXPORTS:
        assert f"bind(c, name='{f}')" in f90
    for f in ("hip_matmat", "hip_matmat_add", "hip_matmat_t", "hip_matmat_t_add"):
        assert re.search(rf"procedure\s*::\s*\w+\s*=>\s*{f}\b", f90), f
    for f in ("matmat", "matmat_add", "matmat_t", "matmat_t_add", "matmat_kernel"):
        assert callable(getattr(sg.csr_matrix, f)) and callable(getattr(sg.sparse_matrix, f)), f
    assert callable(sg.matmat_probe) and (sg.OP_ADD, sg.OP_TRANS) == (1, 2)


def test_each_entry_point_fails_loudly_without_a_gpu_or_a_handle():
    sg.build()
    L = sg.lib()
    x = np.zeros((4, 2), order="F")
    y = np.zeros((4, 2), order="F")
    buf = C.create_string_buffer(64)
    px, py = C.c_void_p(x.ctypes.data), C.c_void_p(y.ctypes.data)
    rcs = (L.sgm_mat_matmat(None, C.c_int32(0), C.c_int32(2), px, C.c_int64(4), py, C.c_int64(4), C.c_int(0)),
           L.sgm_mat_matmat_kernel(None, C.c_int32(0), C.c_int32(2), buf, C.c_int(64)),
           L.sgm_mat_matmat_probe(None, C.c_int32(0), C.c_int32(2), px, C.c_int64(4), py, C.c_int64(4), C.c_int32(0), C.c_int32(0), C.c_int(0)))
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        gpu = False
    # no device: SGM_ERR_NO_DEVICE before anything else; with one (and sgm_init done or not) never SGM_OK on a null handle
    assert all(rc != 0 for rc in rcs), rcs
    if not gpu:
        assert all(rc in (1, 6) for rc in rcs), rcs
        assert L.sgm_last_error()
        ptr, node, val = P.poisson2d_csr(4, 3)
        with pytest.raises(sg.SigmaError):
            A = sg.csr_matrix(12, 12, ptr, node, val)
            A.matmat(np.zeros((12, 2), order="F"), np.zeros((12, 2), order="F"))
    assert not y.any()


def _header_examples():
    txt = open(os.path.join(ROOT, "include", "sigma_hip.h")).read()
    m = re.search(r"With the widths 8, 4 and 2 selected:(.*?)\(which widths", txt, flags=re.S)
    assert m, "the header no longer states the decomposition"
    return {int(k): [int(w) for w in ws.split("+")] for k, ws in re.findall(r"(\d+): (\d+(?: \+ \d+)*)", m.group(1))}


def test_block_decomposition_gives_the_widths_the_header_states():
    stated = _header_examples()
    assert {2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 20} <= set(stated)
    for k, ws in stated.items():
        assert MM.blocks(k, (8, 4, 2)) == ws, (k, ws)
    for widths in ((8, 4, 2), (4, 2), (4,), ()):
        for k in range(21):
            b = MM.blocks(k, widths)
            assert sum(b) == k and all(w in widths or w == 1 for w in b), (widths, k, b)
            assert b == sorted(b, reverse=True)                     # left to right, the largest that fits
            if widths and 2 in widths:
                assert b.count(1) == k % 2                          # a ladder down to 2 leaves at most one single column
            # binary digits below the largest width, whole blocks of it above
            if widths == (8, 4, 2):
                assert b == [8] * (k // 8) + [w for w in (4, 2, 1) if k % 8 & w]
    assert MM.blocks(0, (8, 4, 2)) == [] and MM.blocks(1, (8, 4, 2)) == [1]
    assert MM.k_max((8, 4, 2)) == 15 and MM.blocks(15, (8, 4, 2)) == [8, 4, 2, 1]
    assert MM.k_max((4, 2)) == 7 and MM.blocks(7, (4, 2)) == [4, 2, 1]


def test_python_blocks_are_checked_before_the_c_call():
    """Shapes and lengths are refused in Python: the C ABI takes raw pointers."""
    class Shape(sg._Matrix):        # a handle-less matrix of 12 x 12: the checks below never reach the library
        x_len = 12
    A = Shape()
    A.nrow = A.ncol = 12
    with pytest.raises(sg.SigmaError):
        A.matmat(np.zeros((11, 2), order="F"), np.zeros((12, 2), order="F"))      # short X
    with pytest.raises(sg.SigmaError):
        A.matmat(np.zeros((12, 2), order="F"), np.zeros((12, 3), order="F"))      # column counts differ
    with pytest.raises(TypeError):
        A.matmat(np.zeros((12, 2), order="F"), np.zeros((12, 2), order="C"))      # an output that is not column-major
    big = np.zeros((15, 3), order="F")
    ptr, where, k, ld, _keep = sg._block(big[:12], 12, "X")
    assert (where, k, ld) == (sg.SGM_HOST, 3, 15)
