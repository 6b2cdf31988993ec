"""sgm_lanczos and sgm_generalized_lanczos on the device against their restatement (tests/lanczos_restated.py), bit for bit, at
the smallest shapes at which each mechanism of sgm_lanczos.hip exists, and against a longdouble run within 8 x the oracle's own
deviation (tests/test_lanczos_cpu.py measures the table and ties the restatement to the oracle).

  bits      T and Q `np.array_equal` to the restatement with the device's order of every sum (include/sigma_hip.h, "Dot
            products").  On a leaf matrix alpha_i = q_i . A q_i comes out of the product kernel's epilogue in that kernel's own
            order: the restatement is fed the scalar sgm_mat_matvec_dots reports for the same product (itself pinned by
            tests/test_gpu_fused_dots.py) -- legitimate because a restated q_i that is not the device's already fails the
            comparison of column i.  On composites and in-process partitions alpha is a sum like every other.
  accuracy  on the symmetric cases max |T - T_ld|, max |Q - Q_ld| and max |Q^T Q - I| (the pencil: |Q^T B Q - I|) within 8 x the
            oracle's (the margin tests/test_gpu_gmres.py gives a different but legal order of summation), never above the
            1e-9 / 1e-10 of tests/test_gpu_parity.py.
  C ABI     where = SGM_DEVICE with an aligned and an only 8-byte aligned q1 and Q_out on the device, Q_out = NULL, refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import fused_dot_cases as F
import lanczos_restated as LR
import sigma_amd as sg
from test_gpu_fused_dots import make_handle
from test_lanczos_cpu import MEASURED, OLD_BAR_Q, OLD_BAR_T

pytestmark = pytest.mark.gpu
BAD_ARG, DIMS = 1, 2
TOL = 1e-14


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _csr(n, ptr, node, val):
    return sg.csr_matrix(n, n, ptr, node, val)


def _composite(n, ptr, node, val):
    """(handle, leaves kept alive): the 2 x 2 composite cut at LR.CUT"""
    bp = np.array([1, LR.CUT + 1, n + 1], np.int32)
    S = sg.sparse_matrix(bp, bp)
    keep = []
    for (i, j), L in sorted(LR.composite_leaves(n, ptr, node, val, LR.CUT).items()):
        keep.append(sg.csr_matrix(*L))
        S.set_submatrix(i + 1, j + 1, keep[-1])
    return S, keep


def _epilogue_alpha(H, n):
    """alpha_of for a leaf matrix: the scalar the product kernel's epilogue leaves for q . A q"""
    def alpha_of(i, q, w):
        q = np.ascontiguousarray(q)
        y = np.zeros(n)
        wy, none, _ = H.matvec_dots(q, y, w=q, yy=False)
        assert none is None and _same(y, w), i                    # the product the restatement used is the device's
        return wy[0]
    return alpha_of


def _check_shape_of_t(T):
    assert _same(T[0], T[2]) and T[2, -1] == 0.0 and T[0, -1] == 0.0


def _accuracy(tag, key, T, Q):
    dev = LR.deviations(key, T, Q)
    bars = (min(OLD_BAR_T, 8 * MEASURED[key][0]), min(OLD_BAR_Q, 8 * MEASURED[key][1]), min(OLD_BAR_Q, 8 * MEASURED[key][2]))
    print(f"LANCZOS accuracy {tag}: T {dev[0]:.3e} (bar {bars[0]:.1e}), Q {dev[1]:.3e} (bar {bars[1]:.1e}), "
          f"orthogonality {dev[2]:.3e} (bar {bars[2]:.1e})")
    assert all(d <= b for d, b in zip(dev, bars)), (tag, dev, bars)


# ------------------------------------------------------------------------------------ plain Lanczos, leaf operands
@functools.lru_cache(maxsize=None)
def _plain_run(name):
    """(device T, Q, restated T, Q) of a CSR leaf case, or of the ELLPACK one"""
    c = LR.case(name)
    Ao = LR.oracle_matrix(name)
    H = sg.ellpack_matrix(c.n, c.n, Ao.node, Ao.val) if name.endswith("_ell") else _csr(c.n, c.ptr, c.node, c.val)
    T, Q = sg.lanczos(H, c.steps, c.q1)
    Tr, Qr = LR.lanczos(Ao.matvec, c.q1, c.steps, "device", alpha_of=_epilogue_alpha(H, c.n))
    return T, Q, Tr, Qr


LEAVES = list(LR.PLAIN) + ["grid33x31_ell"]


@pytest.mark.parametrize("name", LEAVES)
def test_lanczos_on_a_leaf_is_the_restatement_bit_for_bit(name):
    """n = 255, 1024, 1025, 2049, 262147 (see lanczos_restated.PLAIN for what each reaches) and the ELLPACK operand"""
    T, Q, Tr, Qr = _plain_run(name)
    print(f"LANCZOS bits {name}: T off by {np.abs(T - Tr).max():.3e}, Q by {np.abs(Q - Qr).max():.3e}")
    assert np.array_equal(T, Tr), np.abs(T - Tr).max()
    assert np.array_equal(Q, Qr), np.abs(Q - Qr).max(axis=0)
    _check_shape_of_t(T)
    assert np.isfinite(T).all() and np.isfinite(Q).all()


@pytest.mark.parametrize("name", LEAVES)
def test_lanczos_on_a_leaf_is_as_accurate_as_the_oracle(name):
    T, Q, _, _ = _plain_run(name)
    _accuracy(name, name, T, Q)


@pytest.mark.parametrize("family", sorted(LR.FAMILY))
def test_lanczos_on_every_kernel_family_is_the_restatement_bit_for_bit(family):
    """one `real` case of tests/fused_dot_cases.py per SpMV kernel family, 6 steps; the composite is the separate dot kernel's
    route (alpha in the device's order, the product the block loop over the leaves)"""
    R = F.reference(LR.FAMILY[family], "real")
    H = make_handle(R)
    assert F.kernel_key(H.kernel, R.fmt) == family, H.kernel
    q1 = LR.start_vector(R.n, 9)
    T, Q = sg.lanczos(H, LR.FAMILY_STEPS, q1)
    alpha_of = None if family == "composite" else _epilogue_alpha(H, R.n)
    Tr, Qr = LR.lanczos(lambda x: F.oracle_matvec(R, x, None), q1, LR.FAMILY_STEPS, "device", alpha_of=alpha_of)
    print(f"LANCZOS bits family {family!r} n={R.n}: T off by {np.abs(T - Tr).max():.3e}, Q by {np.abs(Q - Qr).max():.3e}")
    assert np.array_equal(T, Tr) and np.array_equal(Q, Qr)
    _check_shape_of_t(T)
    assert np.isfinite(T).all()


# ------------------------------------------------------------------------------------ the routes without a fused alpha
@functools.lru_cache(maxsize=None)
def _route_run(route):
    c = LR.case("grid33x31")
    if route == "composite":
        H, keep = _composite(c.n, c.ptr, c.node, c.val)
        matvec = LR.composite_matvec(LR.composite_leaves(c.n, c.ptr, c.node, c.val, LR.CUT), LR.CUT, c.n)
    else:
        H = sg.partitioned_csr_matrix(c.n, c.n, c.ptr, c.node, c.val, LR.part_starts(c.n, int(route[-1])))
        matvec = LR.oracle_matrix("grid33x31").matvec
    T, Q = sg.lanczos(H, c.steps, c.q1)
    Tr, Qr = LR.lanczos(matvec, c.q1, c.steps, "device")
    return T, Q, Tr, Qr


@pytest.mark.parametrize("route", ["composite", "part2", "part3"])
def test_lanczos_without_a_fused_alpha_is_the_restatement_bit_for_bit(route):
    """a 2 x 2 composite of the 33 x 31 grid cut at row 511, and its in-process partitions of 2 and 3 parts: the product by
    matvec_plain, alpha by the dot kernel -- no callback, every scalar is a sum in the device's order"""
    T, Q, Tr, Qr = _route_run(route)
    print(f"LANCZOS bits {route}: T off by {np.abs(T - Tr).max():.3e}, Q by {np.abs(Q - Qr).max():.3e}")
    assert np.array_equal(T, Tr) and np.array_equal(Q, Qr)
    _check_shape_of_t(T)
    _accuracy(route, "grid33x31", T, Q)


@pytest.mark.parametrize("name", sorted(LR.DEGENERATE))
def test_degenerate_runs_are_the_restatement_nan_for_nan(name):
    """n = 1, 3 steps: beta_1 = 0 exactly, q_2 = 0/0 and everything after it NaN, as in eigensolver.f90 (no breakdown test
    there); n = 3, 5 steps: more steps than rows, steps 4 and 5 run on rounding residue"""
    c = LR.case(name)
    H = _csr(c.n, c.ptr, c.node, c.val)
    T, Q = sg.lanczos(H, c.steps, c.q1)
    Ao = LR.oracle_matrix(name)
    Tr, Qr = LR.lanczos(Ao.matvec, c.q1, c.steps, "device", alpha_of=_epilogue_alpha(H, c.n))
    print(f"LANCZOS degenerate {name}: T = {T.tolist()}")
    assert _same(T, Tr) and _same(Q, Qr)
    assert _same(T[0], T[2]) and T[2, -1] == 0.0
    assert np.isnan(T).any() == (name == "n1")
    if name == "n1":
        assert T[1, 0] == 2.0 and T[2, 0] == 0.0 and Q[0, 0] == 1.0 and np.isnan(Q[0, 1:]).all() and np.isnan(T[1, 1:]).all()


# ------------------------------------------------------------------------------------ generalized Lanczos
def _pencil(variant):
    """(A, B, keepalive, restated A, B, solve) of a variant; B's solver is CG(1e-14) in the reference's dot order except for
    `default_order`"""
    import oracle as orc
    c = LR.case("pencil33x31")
    Ao, Bo = LR.oracle_matrix("pencil33x31")
    keep = []
    Amv, Bmv = Ao.matvec, Bo.matvec
    solve = lambda w, v: orc.cg(Bo, v, x0=w, tol=TOL)[0]                        # noqa: E731
    if variant == "composite":
        A, ka = _composite(c.n, c.ptr, c.node, c.val)
        B, kb = _composite(c.n, c.ptr, c.node, c.bval)
        keep = ka + kb
        Amv = LR.composite_matvec(LR.composite_leaves(c.n, c.ptr, c.node, c.val, LR.CUT), LR.CUT, c.n)
        Bmv = LR.composite_matvec(LR.composite_leaves(c.n, c.ptr, c.node, c.bval, LR.CUT), LR.CUT, c.n)
        solve = lambda w, v: LR.cg(Bmv, v, w, TOL)                              # noqa: E731
    elif variant == "part2":
        starts = LR.part_starts(c.n, 2)
        A = sg.partitioned_csr_matrix(c.n, c.n, c.ptr, c.node, c.val, starts)
        B = sg.partitioned_csr_matrix(c.n, c.n, c.ptr, c.node, c.bval, starts)
    else:
        A, B = _csr(c.n, c.ptr, c.node, c.val), _csr(c.n, c.ptr, c.node, c.bval)
    s = sg.cg(TOL)
    if variant != "default_order":
        s.set_option("dot_order", 1)
    B.set_solver(s)
    if variant == "jacobi":
        B.set_preconditioner(sg.jacobi())
        J = orc.Jacobi(Bo)
        solve = lambda w, v: orc.cg(Bo, v, x0=w, pc=J, tol=TOL)[0]              # noqa: E731
    return A, B, keep, Amv, Bmv, solve


@pytest.mark.parametrize("variant", ["leaf", "jacobi", "composite", "part2", "default_order"])
def test_generalized_lanczos_is_the_restatement_bit_for_bit(variant):
    """33 x 31, 12 steps.  With B%solve = CG(1e-14) in the reference's dot order the inner solve is the oracle's bit for bit
    (the composite: the restated CG over the block loop), so T and Q are the restatement's; in the default order only the
    accuracy bars apply."""
    c = LR.case("pencil33x31")
    A, B, _keep, Amv, Bmv, solve = _pencil(variant)
    T, Q = sg.generalized_lanczos(A, B, c.steps, c.q1)
    _check_shape_of_t(T)
    if variant != "default_order":
        Tr, Qr = LR.generalized_lanczos(Amv, Bmv, solve, c.q1, c.steps, "device")
        print(f"LANCZOS bits pencil {variant}: T off by {np.abs(T - Tr).max():.3e}, Q by {np.abs(Q - Qr).max():.3e}")
        assert np.array_equal(T, Tr) and np.array_equal(Q, Qr)
    _accuracy("pencil " + variant, "pencil33x31", T, Q)


# ------------------------------------------------------------------------------------ the C ABI, device vectors
def _call_lanczos(H, steps, q1_ptr, n, where, Q_ptr):
    T = np.zeros((steps, 3))
    rc = sg.lib().sgm_lanczos(H._h, C.c_int32(steps), C.c_void_p(q1_ptr), C.c_void_p(T.ctypes.data),
                              C.c_void_p(Q_ptr) if Q_ptr else None, C.c_int(where))
    return rc, T.T.copy()


def test_lanczos_with_device_vectors_gives_the_host_calls_bits():
    """n = 1025 (odd: the padded leading dimension is stripped on the way out).  q1 on the device at a 16-byte aligned address is
    read in place; at an address that is only 8-byte aligned it is staged (stage_in); Q_out goes device to device."""
    import torch
    T0, Q0, _, _ = _plain_run("grid41x25")
    c = LR.case("grid41x25")
    H = _csr(c.n, c.ptr, c.node, c.val)
    buf = torch.zeros(c.n + 1, dtype=torch.float64, device="cuda")
    for shift in (0, 1):
        q1 = buf[shift:shift + c.n]
        q1.copy_(torch.from_numpy(c.q1.copy()))
        assert q1.data_ptr() % 16 == 8 * shift
        Qd = torch.full((c.steps * c.n + 1,), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc, T = _call_lanczos(H, c.steps, q1.data_ptr(), c.n, sg.SGM_DEVICE, Qd.data_ptr())
        assert rc == 0, sg.lib().sgm_last_error()
        Qh = Qd.cpu().numpy()
        assert np.isnan(Qh[-1])                                     # nothing written past n x steps
        assert np.array_equal(T, T0) and np.array_equal(Qh[:-1].reshape(c.steps, c.n).T, Q0), shift
        assert np.array_equal(q1.cpu().numpy(), c.q1)               # the caller's vector is left alone
    # Q_out = NULL: the same T
    T1, none = sg.lanczos(H, c.steps, c.q1, want_Q=False)
    assert none is None and np.array_equal(T1, T0)


def test_generalized_lanczos_with_device_vectors_gives_the_host_calls_bits():
    import torch
    c = LR.case("grid41x25")
    bval = LR.mass_like(c.n, c.ptr, c.node)
    A, B = _csr(c.n, c.ptr, c.node, c.val), _csr(c.n, c.ptr, c.node, bval)
    s = sg.cg(TOL)
    s.set_option("dot_order", 1)
    B.set_solver(s)
    steps = 6
    T0, Q0 = sg.generalized_lanczos(A, B, steps, c.q1)
    T1, none = sg.generalized_lanczos(A, B, steps, c.q1, want_Q=False)
    assert none is None and np.array_equal(T1, T0)
    q1 = torch.from_numpy(c.q1.copy()).cuda()
    assert q1.data_ptr() % 16 == 0
    Qd = torch.full((steps * c.n + 1,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    T = np.zeros((steps, 3))
    rc = sg.lib().sgm_generalized_lanczos(A._h, B._h, s._h, None, C.c_int32(steps), C.c_void_p(q1.data_ptr()),
                                          C.c_void_p(T.ctypes.data), C.c_void_p(Qd.data_ptr()), C.c_int(sg.SGM_DEVICE))
    assert rc == 0, sg.lib().sgm_last_error()
    Qh = Qd.cpu().numpy()
    assert np.isnan(Qh[-1])
    assert np.array_equal(T.T, T0) and np.array_equal(Qh[:-1].reshape(steps, c.n).T, Q0)


def test_refusals_of_both_entry_points():
    """nsteps = 1: BAD_ARG; a rectangular matrix: DIMS; a pencil of differently sized operands: DIMS"""
    c = LR.case("grid15x17")
    H = _csr(c.n, c.ptr, c.node, c.val)
    rc, _ = _call_lanczos(H, 1, c.q1.ctypes.data, c.n, sg.SGM_HOST, 0)
    assert rc == BAD_ARG
    ptr = np.arange(1, 6, dtype=np.int32)
    R = sg.csr_matrix(4, 5, ptr, np.arange(1, 5, dtype=np.int32), np.ones(4))
    rc, _ = _call_lanczos(R, 3, c.q1.ctypes.data, 4, sg.SGM_HOST, 0)
    assert rc == DIMS
    d = LR.case("n3")
    B = _csr(d.n, d.ptr, d.node, d.val)
    s = sg.cg(TOL)
    B.set_solver(s)
    T = np.zeros((3, 3))
    for nsteps, A, want in ((1, B, BAD_ARG), (3, H, DIMS), (3, R, DIMS)):
        rc = sg.lib().sgm_generalized_lanczos(A._h, B._h, s._h, None, C.c_int32(nsteps), C.c_void_p(c.q1.ctypes.data),
                                              C.c_void_p(T.ctypes.data), None, C.c_int(sg.SGM_HOST))
        assert rc == want, (nsteps, rc, want)
