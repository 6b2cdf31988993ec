"""Multi-vector products on the GPU (sgm_mat_matmat, include/sigma_hip.h): column j of Y = [Y +] op(A) X holds exactly the bits
the single-vector product leaves for column j of X -- compared, with np.array_equal, against the oracle's per-column product AND
against H.matvec / H.matvec_add / H.matvec_t / H.matvec_t_add of that column on the device.

The handles are the cases of tests/fused_dot_cases.py (the smallest shapes at which each kernel family can go wrong), created by
tests/test_gpu_fused_dots.py's recipe (restated in make_handle).  Blocks carry odd and even leading dimensions (ldx = n + 3,
ldy = n + 5): X's padding rows are NaN (a read of them would show), Y's hold a sentinel that must survive, Y starts as NaN
without the add bit.

WIDTHS is the selection the library is built with (sgm_matmat.hip's SGM_MM_*_KBS lists; profiles/matmat/README.md says why):
matmat_kernel must name exactly the decomposition tests/matmat_restated.py restates from it.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fused_dot_cases as F
import matmat_restated as MM
import oracle as orc
import sigma_amd as sg
from sigma_amd import problems as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = 1, 8
SENTINEL = -123.25
WIDTHS = {"k_mm_sl": (8, 4, 2), "k_mm_slb": (4, 2), "k_mm_sl32": (4, 2)}
NATIVE_KEYS = {"k_csr_sl": "k_mm_sl", "sliced ellpack": "k_mm_sl", "k_csr_slb": "k_mm_slb", "k_csr_sl32": "k_mm_sl32"}
NATIVE_FAMILIES = ("k_csr_sl", "k_csr_slb", "k_csr_sl32", "sliced ellpack", "lean parts")


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def make_handle(R):
    """The case's matrix on the device: created under the case's defaults (put back afterwards), then its handle options
    (tests/test_gpu_fused_dots.py's recipe)."""
    case, A = R.case, R.A
    for k, v in case.create.items():
        sg.set_option(k, v)
    try:
        if R.fmt == "composite":
            ptr = np.asarray(R.cuts, np.int32) + 1
            H = sg.sparse_matrix(ptr, ptr)
            for (it, jt), L in R.leaves.items():
                H.set_submatrix(it + 1, jt + 1, sg.csr_matrix(L.n, L.m, L.ptr, L.node, L.val))
            H._build()
        elif R.fmt == "ell":
            H = sg.ellpack_matrix(R.n, R.m, A.node, A.val)
        elif case.nparts:
            H = sg.partitioned_csr_matrix(R.n, R.m, A.ptr, A.node, A.val, R.starts)
        else:
            H = sg.csr_matrix(R.n, R.m, A.ptr, A.node, A.val)
    finally:
        for k in case.create:
            sg.set_option(k, F.OPTION_DEFAULTS[k])
    for k, v in case.handle.items():
        H.set_option(k, v)
    return H


def case_handle(name):
    R = F.reference(name, "real")
    H = make_handle(R)
    assert F.kernel_key(H.kernel, R.fmt) == R.case.key, (name, H.kernel)
    return R, H


def native_of(R):
    """The multi-vector kernel family the case's product has, or None: the column loop."""
    return NATIVE_KEYS.get(R.case.key)


def expected_kernel(H, mm, k):
    """sgm_mat_matmat_kernel's text for k columns, from the restated decomposition."""
    one = H.kernel
    if mm is None:
        return "columns: " + one
    W = re.search(r"W=(\d+)", one).group(1)
    b, items, i = MM.blocks(k, WIDTHS[mm]), [], 0
    while i < len(b):
        e = i
        while e < len(b) and b[e] == b[i]:
            e += 1
        items.append(f"{one} x{e - i}" if b[i] == 1 else f"{mm}<W={W},KB={b[i]}> x{e - i}")
        i = e
    return " + ".join(items)


def block_data(R, k, seed=0):
    """X (m x k, column 0 = the case's x) and Y0 (n x k, column 0 = the case's y0)."""
    rs = np.random.RandomState(1000 + seed + k)
    X = np.asfortranarray(rs.standard_normal((R.m, k)))
    Y0 = np.asfortranarray(rs.standard_normal((R.n, k)))
    X[:, 0], Y0[:, 0] = R.x, R.y0
    return X, Y0


def padded(V, extra, fill):
    """V inside a Fortran-ordered array with `extra` more rows holding `fill`: (the whole array, the view of V's rows)."""
    big = np.full((V.shape[0] + extra, V.shape[1]), fill, order="F")
    big[:V.shape[0]] = V
    return big, big[:V.shape[0]]


def run_block(call, X, Y0, n, add):
    """One block product through `call(Xview, Yview)` on padded blocks; the padding is checked, the n x k result returned."""
    k = X.shape[1]
    _xb, xv = padded(X, 3, np.nan)
    yb, yv = padded(Y0 if add else np.full((n, k), np.nan), 5, SENTINEL)
    call(xv, yv)
    assert (yb[n:] == SENTINEL).all(), "the rows of Y between a column's end and ldy were written"
    return np.array(yv, order="F")


def check_columns(R, H, k, add, call=None, seed=0):
    """The contract for one (case, k, add): every column against the oracle and against the device's single-vector product."""
    X, Y0 = block_data(R, k, seed)
    Y = run_block(call or (H.matmat_add if add else H.matmat), X, Y0, R.n, add)
    assert np.array_equal(Y[:, 0], R.y[1 if add else 0]), (R.case.name, k, add, "column 0 against the case's reference")
    for j in range(k):
        x = np.ascontiguousarray(X[:, j])
        assert np.array_equal(Y[:, j], F.oracle_matvec(R, x, Y0[:, j].copy() if add else None)), \
            (R.case.name, k, add, j, "oracle")
        yd = Y0[:, j].copy() if add else np.full(R.n, np.nan)
        (H.matvec_add if add else H.matvec)(x, yd)
        assert np.array_equal(Y[:, j], yd), (R.case.name, k, add, j, "device matvec")
    return Y


# ------------------------------------------------------------------------------------ 1. every native case, k = k_max
@pytest.mark.parametrize("name", [c.name for c in F.CASES if c.family in NATIVE_FAMILIES])
def test_every_native_case_at_k_max(name):
    R, H = case_handle(name)
    mm = native_of(R)
    k = MM.k_max(WIDTHS[mm]) if mm else 3          # (the lean SELL parts run the column loop)
    assert H.matmat_kernel(k) == expected_kernel(H, mm, k), H.matmat_kernel(k)
    if mm:
        assert H.matmat_kernel(k).startswith(mm + "<"), H.matmat_kernel(k)
    for add in (0, 1):
        check_columns(R, H, k, add)


# ------------------------------------------------------------------------------------ 2. one case of every other family
def _smallest(family):
    return min((c for c in F.CASES if c.family == family), key=lambda c: F.structure(c.name)["n"]).name


@pytest.mark.parametrize("family", [f for f in F.FAMILIES if f not in NATIVE_FAMILIES and f != "partition"])
def test_column_loop_on_every_other_family(family):
    R, H = case_handle(_smallest(family))
    assert H.matmat_kernel(3).startswith("columns:"), H.matmat_kernel(3)
    for add in (0, 1):
        check_columns(R, H, 3, add)


# ------------------------------------------------------------------------------------ 3. k sweep
@pytest.mark.parametrize("name", ["sl_banded_513_w8", "slb_27pt_23x17x11", "sl32_513_w16"])
def test_k_sweep(name):
    R, H = case_handle(name)
    mm = native_of(R)
    for k in (1, 2, 3, 4, 5, 7, 8, 9, 17):
        assert H.matmat_kernel(k) == expected_kernel(H, mm, k), (k, H.matmat_kernel(k))
        for add in (0, 1):
            check_columns(R, H, k, add, seed=k)


# ------------------------------------------------------------------------------------ 4. column independence
@pytest.mark.parametrize("name", ["sl_banded_70001_w8", "slb_9pt_70x51"])
def test_a_nan_and_an_inf_stay_in_their_column(name):
    R, H = case_handle(name)
    k = MM.k_max(WIDTHS[native_of(R)])
    X, Y0 = block_data(R, k)
    for add in (0, 1):
        call = H.matmat_add if add else H.matmat
        clean = run_block(call, X, Y0, R.n, add)
        Xn = X.copy(order="F")
        Xn[R.m // 3, 2], Xn[2 * R.m // 3, 2] = np.nan, np.inf
        dirty = run_block(call, Xn, Y0, R.n, add)
        others = [j for j in range(k) if j != 2]
        assert np.array_equal(dirty[:, others], clean[:, others]), (name, add)
        yd = Y0[:, 2].copy() if add else np.full(R.n, np.nan)
        with np.errstate(invalid="ignore"):
            (H.matvec_add if add else H.matvec)(np.ascontiguousarray(Xn[:, 2]), yd)
        assert not np.isfinite(yd).all()
        assert np.array_equal(dirty[:, 2], yd, equal_nan=True), (name, add)


# ------------------------------------------------------------------------------------ 5. slice loop, slice maps, caps
@pytest.mark.parametrize("name,k,grid_cap", [("sl_banded_70001_w8", 15, 8),         # 137 slices, 18 rounds, round-robin
                                             ("sl_banded_1048573_w3", 5, 256),       # the XCD-block-cyclic map, 8 rounds
                                             ("slb_27pt_23x17x11", 7, 8), ("sl32_40001_w12", 7, 8)])
def test_capped_grids_give_the_bits_of_the_uncapped_call(name, k, grid_cap):
    R, H = case_handle(name)
    X, Y0 = block_data(R, k)
    for add in (0, 1):
        op = sg.OP_ADD if add else 0
        ref = run_block(H.matmat_add if add else H.matmat, X, Y0, R.n, add)
        assert np.array_equal(ref[:, 0], R.y[add])
        got = run_block(lambda x, y: sg.matmat_probe(H, x, y, op=op, grid_cap=grid_cap), X, Y0, R.n, add)
        assert np.array_equal(got, ref), (name, add, grid_cap)


@pytest.mark.parametrize("name", ["sl_banded_513_w8", "slb_27pt_23x17x11", "sl32_513_w16"])
def test_capped_block_widths_give_the_bits_of_the_uncapped_call(name):
    R, H = case_handle(name)
    k = MM.k_max(WIDTHS[native_of(R)])
    X, Y0 = block_data(R, k)
    for add in (0, 1):
        op = sg.OP_ADD if add else 0
        ref = run_block(H.matmat_add if add else H.matmat, X, Y0, R.n, add)
        for cap in (1, 2, 4):
            got = run_block(lambda x, y: sg.matmat_probe(H, x, y, op=op, block_cap=cap), X, Y0, R.n, add)
            assert np.array_equal(got, ref), (name, add, cap)


# ------------------------------------------------------------------------------------ 6. transpose
def _grid5_301():
    st = F.grid5(301, 233)
    return st["n"], st["m"], st["ptr"], st["node"], np.random.RandomState(5).standard_normal(st["node"].size)


def _interp_33():
    ptr, node, val, nc = P.interp2d_csr(33, 29)
    return 33 * 29, nc, ptr, node, val


@pytest.mark.parametrize("make", [_grid5_301, _interp_33], ids=["grid5_301x233", "interp2d_33x29"])
def test_transposed_products(make):
    n, m, ptr, node, val = make()
    H = sg.csr_matrix(n, m, ptr, node, val)
    Ao = orc.CsrMatrix(n, m, ptr, node, val)
    k = 7
    rs = np.random.RandomState(n)
    X = np.asfortranarray(rs.standard_normal((n, k)))          # x has nrow entries, y has ncol
    Y0 = np.asfortranarray(rs.standard_normal((m, k)))
    assert H.matmat_kernel(k, sg.OP_TRANS) == H.matmat_kernel(k, sg.OP_TRANS | sg.OP_ADD)
    print("MATMAT_T", H.matmat_kernel(k, sg.OP_TRANS))
    for add in (0, 1):
        Y = run_block(H.matmat_t_add if add else H.matmat_t, X, Y0, m, add)
        for j in range(k):
            x = np.ascontiguousarray(X[:, j])
            yo = Ao.matvec_t_add(x, Y0[:, j].copy()) if add else Ao.matvec_t(x)
            assert np.array_equal(Y[:, j], yo), (add, j, "oracle")
            yd = Y0[:, j].copy() if add else np.full(m, np.nan)
            (H.matvec_t_add if add else H.matvec_t)(x, yd)
            assert np.array_equal(Y[:, j], yd), (add, j, "device matvec_t")


# ------------------------------------------------------------------------------------ 7. other operands
def test_device_tensors_in_place_and_staged():
    """Device blocks of shape (k, n).  The tensors are made on the host and copied over, and read back whole: host <-> device
    copies and views only, none of torch's own kernels."""
    import torch
    R, H = case_handle("sl_banded_512_w5")
    k, n = 7, R.n
    X, Y0 = block_data(R, k)
    ref = check_columns(R, H, k, 0)
    ref_add = check_columns(R, H, k, 1)
    dev = torch.device("cuda:0")

    def to_dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    Xd = to_dev(X.T)                                                    # shape (k, n): the columns as contiguous rows
    assert Xd.data_ptr() % 16 == 0 and n % 2 == 0                       # every column 16-byte aligned: used in place
    Yd = to_dev(np.full((k, n), np.nan))
    H.matmat(Xd, Yd)
    assert np.array_equal(Yd.cpu().numpy().T, ref)
    Yd = to_dev(Y0.T)
    H.matmat_add(Xd, Yd)
    assert np.array_equal(Yd.cpu().numpy().T, ref_add)
    # views at an odd element offset: no column is 16-byte aligned, the staging rule is taken; what lies around the views stays
    xflat = np.concatenate([[np.nan], X.T.reshape(-1), [np.nan]])
    for add, want in ((0, ref), (1, ref_add)):
        yflat = np.concatenate([[SENTINEL], Y0.T.reshape(-1) if add else np.full(k * n, np.nan), [SENTINEL]])
        xbase, ybase = to_dev(xflat), to_dev(yflat)
        Xv, Yv = xbase[1:1 + k * n].view(k, n), ybase[1:1 + k * n].view(k, n)
        assert Xv.data_ptr() % 16 == 8 and Yv.data_ptr() % 16 == 8
        (H.matmat_add if add else H.matmat)(Xv, Yv)
        out = ybase.cpu().numpy()
        assert np.array_equal(out[1:-1].reshape(k, n).T, want), add
        assert out[0] == SENTINEL and out[-1] == SENTINEL
    # an odd leading dimension (n + 1 entries per row, n used): staged as well
    Xo = to_dev(np.hstack([X.T, np.full((k, 1), np.nan)]))
    Yo = to_dev(np.full((k, n + 1), SENTINEL))
    H.matmat(Xo, Yo)
    out = Yo.cpu().numpy()
    assert np.array_equal(out[:, :n].T, ref) and (out[:, n] == SENTINEL).all()


def test_slice_sched_handle_takes_the_column_loop_with_the_same_bits():
    R, H = case_handle("sl_banded_70001_w8")
    k = 7
    X, Y0 = block_data(R, k)
    before = [run_block(H.matmat_add if add else H.matmat, X, Y0, R.n, add) for add in (0, 1)]
    assert H.matmat_kernel(k).startswith("k_mm_sl<")
    H.set_option("slice_sched", 1)
    assert H.matmat_kernel(k) == "columns: " + H.kernel
    for add in (0, 1):
        assert np.array_equal(check_columns(R, H, k, add), before[add])


def test_a_call_after_value_edits_sees_the_new_values():
    R, H = case_handle("sl_grid5_301x233")
    k = 5
    X, Y0 = block_data(R, k)
    before = run_block(H.matmat, X, Y0, R.n, 0)
    A = R.A
    rows = np.array([1, R.n // 2, R.n], np.int32)
    cols = A.node[A.ptr[rows - 1] - 1].astype(np.int32)               # the first stored entry of each of the three rows
    H.set_value(rows, cols, np.array([7.5, -2.25, 1e3]))
    after = run_block(H.matmat, X, Y0, R.n, 0)
    changed = np.zeros(R.n, bool)
    changed[rows - 1] = True
    assert np.array_equal(after[~changed], before[~changed]) and not np.array_equal(after[changed], before[changed])
    for j in range(k):
        yd = np.full(R.n, np.nan)
        H.matvec(np.ascontiguousarray(X[:, j]), yd)
        assert np.array_equal(after[:, j], yd), j


# ------------------------------------------------------------------------------------ 8. refusals
def _raw(H, op, k, X, ldx, Y, ldy):
    return sg.lib().sgm_mat_matmat(H._h, C.c_int32(op), C.c_int32(k), C.c_void_p(X.ctypes.data), C.c_int64(ldx),
                                   C.c_void_p(Y.ctypes.data), C.c_int64(ldy), C.c_int(sg.SGM_HOST))


def test_refusals():
    R = F.reference("part3_grid5_450x450", "real")
    Hp = make_handle(R)
    X = np.zeros((R.m, 3), order="F")
    Y = np.full((R.n, 3), SENTINEL, order="F")
    with pytest.raises(sg.SigmaError) as e:
        Hp.matmat(X, Y)
    assert e.value.code == UNSUPPORTED and "sgm_mat_matmat" in str(e.value)
    with pytest.raises(sg.SigmaError) as e:
        Hp.matmat_kernel(3)
    assert e.value.code == UNSUPPORTED
    assert (Y == SENTINEL).all()

    R, H = case_handle("sl_banded_513_w8")
    n = R.n
    X = np.asfortranarray(np.random.RandomState(0).standard_normal((n, 4)))
    Y = np.full((n, 4), SENTINEL, order="F")
    assert _raw(H, 0, 4, X, n - 1, Y, n) == BAD_ARG                   # short ldx
    assert _raw(H, 0, 4, X, n, Y, n - 1) == BAD_ARG                   # short ldy
    assert _raw(H, 0, -1, X, n, Y, n) == BAD_ARG                      # k < 0
    assert _raw(H, 4, 4, X, n, Y, n) == BAD_ARG                       # an op bit that does not exist
    assert (Y == SENTINEL).all()
    Z = np.asfortranarray(np.random.RandomState(1).standard_normal((n, 6)))
    keep = Z.copy(order="F")
    assert _raw(H, 0, 4, Z, n, Z, n) == BAD_ARG                       # X and Y the same block
    assert _raw(H, 0, 4, Z[:, :4], n, Z[:, 2:], n) == BAD_ARG         # Y starts inside X
    assert _raw(H, 0, 4, Z[:, 2:], n, Z[:, :4], n) == BAD_ARG         # X starts inside Y
    assert np.array_equal(Z, keep)
    assert _raw(H, 0, 2, Z[:, :2], n, Z[:, 2:], n) == 0               # adjacent, not overlapping: fine
    assert np.array_equal(Z[:, :2], keep[:, :2]) and np.array_equal(Z[:, 4:], keep[:, 4:])
    for j in range(2):
        yd = np.full(n, np.nan)
        H.matvec(np.ascontiguousarray(keep[:, j]), yd)
        assert np.array_equal(Z[:, 2 + j], yd)
    assert _raw(H, 0, 0, X, n, Y, n) == 0 and (Y == SENTINEL).all()   # k = 0: OK, nothing written
    assert H.matmat_kernel(0) == ""


# ------------------------------------------------------------------------------------ 9. the Fortran program
def test_fortran_program_compares_every_column_with_matvec():
    exe = os.path.join(ROOT, "sigma_amd", "fortran", "matmat_test_hip")
    if not os.path.exists(exe) and not os.path.exists("/opt/rocm/bin/amdflang"):
        pytest.skip("sigma_amd/fortran/matmat_test_hip was not built (no amdflang at build time)")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "matmat_test_hip: ok" in r.stdout and "FAILED" not in r.stdout, r.stdout
