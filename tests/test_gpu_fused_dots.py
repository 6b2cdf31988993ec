"""The dot products fused into every SpMV kernel, pinned: sgm_mat_matvec_dots (H.matvec_dots) launches a product with the w.y / y.y
epilogues exactly as CG, BiCGStab and Lanczos do in the default dot order and returns the scalars a consumer would see, per part;
tests/fused_dot_cases.py says what they must be -- `==` the exact integers on the `int` data (whatever the summation tree),
within gamma_n * sum |w_i y_i| of the correctly rounded sum on the `real` data -- on the smallest structures at which each
kernel family can go wrong."""
import numpy as np
import pytest

import sigma_amd as sg
import fused_dot_cases as F

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = 1, 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    sg.init(0)


def make_handle(R):
    """The case's matrix on the device: created under the case's defaults (put back afterwards), then its handle options."""
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


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("data", F.DATASETS)
@pytest.mark.parametrize("name", [c.name for c in F.CASES])
def test_fused_dots_of_every_kernel_family(name, data):
    """y and both scalars of every part, y = A x and y += A x, the three epilogue variants, a repeated call and a call after a
    product with another w.  Measured on an MI355X (worst |device - exact| / bar per family over the `real` cases, and the
    counts covered): see the table in DESIGN.md, "Parity of the fused dots"."""
    R = F.reference(name, data)
    H = make_handle(R)
    assert F.kernel_key(H.kernel, R.fmt) == R.case.key, H.kernel
    nparts = len(R.parts)
    for add in (0, 1):
        def fresh():
            return R.y0.copy() if add else np.full(R.n, np.nan)
        yref = R.y[add]
        y = fresh()
        (H.matvec_add if add else H.matvec)(R.x, y)
        assert np.array_equal(y, yref), (name, data, add, "plain product")
        y = fresh()
        wy, yy, cnt = H.matvec_dots(R.x, y, w=R.w, add=add)
        assert np.array_equal(y, yref), (name, data, add, "both dots")
        assert wy.shape == yy.shape == cnt.shape == (nparts,)
        assert list(cnt) == R.count, (name, list(cnt), R.count)
        # the scalars themselves
        for ip in range(nparts):
            ex_wy, ex_yy = R.wy[add][ip], R.yy[add][ip]
            if data == "int":
                print(f"FUSED_DOT int  {name} add={add} part={ip} count={cnt[ip]} wy={wy[ip]:.0f} ({ex_wy:.0f}) yy={yy[ip]:.0f} ({ex_yy:.0f})")
                assert wy[ip] == ex_wy and yy[ip] == ex_yy, (name, add, ip, wy[ip], ex_wy, yy[ip], ex_yy)
            else:
                g = F.gamma(R.parts[ip][1] - R.parts[ip][0])
                bar_wy, bar_yy = g * R.abs_wy[add][ip], g * R.abs_yy[add][ip]
                r_wy = abs(wy[ip] - ex_wy) / bar_wy if bar_wy else 0.0
                r_yy = abs(yy[ip] - ex_yy) / bar_yy if bar_yy else 0.0
                print(f"FUSED_DOT real {name} family={R.case.family!r} add={add} part={ip} count={cnt[ip]} ratio_wy={r_wy:.3e} ratio_yy={r_yy:.3e}")
                assert abs(wy[ip] - ex_wy) <= bar_wy, (name, add, ip, wy[ip], ex_wy, bar_wy)
                assert abs(yy[ip] - ex_yy) <= bar_yy, (name, add, ip, yy[ip], ex_yy, bar_yy)
        # variant invariance: (w only) and (yy only) leave the bits of (w and yy), and the same y
        y = fresh()
        wy1, none, cnt1 = H.matvec_dots(R.x, y, w=R.w, add=add, yy=False)
        assert none is None and np.array_equal(y, yref) and np.array_equal(cnt1, cnt)
        assert np.array_equal(wy1, wy), (name, add, "w only", wy1, wy)
        y = fresh()
        none, yy1, cnt1 = H.matvec_dots(R.x, y, add=add)
        assert none is None and np.array_equal(y, yref) and np.array_equal(cnt1, cnt)
        assert np.array_equal(yy1, yy), (name, add, "yy only", yy1, yy)
        # a product with another w in between (-w: every partial sum negates exactly, in any order), then the first call again
        y = fresh()
        wy2, yy2, _ = H.matvec_dots(R.x, y, w=-R.w, add=add)
        assert np.array_equal(wy2, -wy) and np.array_equal(yy2, yy), (name, add, "-w")
        y = fresh()
        wy3, yy3, cnt3 = H.matvec_dots(R.x, y, w=R.w, add=add)
        assert np.array_equal(y, yref) and np.array_equal(wy3, wy) and np.array_equal(yy3, yy) and np.array_equal(cnt3, cnt), (name, add, "repeat")


def test_kernel_table_every_family_is_reached():
    """Coverage by assertion: the kernels the cases run, read off the handles, are exactly the families of the table."""
    seen = {}
    for c in F.CASES:
        if F.structure(c.name)["n"] > 100000:
            continue                       # (the same kernels at a larger size)
        R = F.reference(c.name, "int")
        H = make_handle(R)
        seen.setdefault(F.kernel_key(H.kernel, R.fmt), []).append(c.name)
        H.destroy()
    assert set(seen) == set(F.KERNEL_KEYS), (sorted(seen), sorted(F.KERNEL_KEYS))


@pytest.mark.parametrize("name", ["sl_banded_70001_w8", "spmv_ragged_3001", "ellcb_ell_3001_d12"])
def test_fused_dots_with_nan_and_inf_in_x(name):
    """One NaN and one Inf in x: wy and yy are NaN or +-Inf exactly where a sum over the oracle's y is -- never a finite number."""
    R = F.reference(name, "real")
    H = make_handle(R)
    xb = R.x.copy()
    xb[R.m // 3] = np.nan
    xb[(2 * R.m) // 3] = np.inf
    yb = F.oracle_matvec(R, xb, None)
    assert np.isnan(yb).any() and np.isinf(yb).any()
    y = np.zeros(R.n)
    wy, yy, _ = H.matvec_dots(xb, y, w=R.w)
    assert _same(y, yb)
    for got, cls in ((wy[0], F.nonfinite_class(R.w, yb)), (yy[0], F.nonfinite_class(yb, yb))):
        assert cls is not None
        assert np.isnan(got) if cls == "nan" else got == float(cls), (name, got, cls)
    # only an Inf: the sums are infinite (or NaN where +Inf meets -Inf), not NaN by default
    xb = R.x.copy()
    xb[(2 * R.m) // 3] = np.inf
    yb = F.oracle_matvec(R, xb, None)
    wy, yy, _ = H.matvec_dots(xb, y, w=R.w)
    assert _same(y, yb)
    for got, cls in ((wy[0], F.nonfinite_class(R.w, yb)), (yy[0], F.nonfinite_class(yb, yb))):
        assert cls is not None
        assert np.isnan(got) if cls == "nan" else got == float(cls), (name, got, cls)


@pytest.mark.parametrize("name", ["sl_banded_70001_w8", "sell_xw_700", "ell_do8_40001_d8"])
def test_lanczos_consumes_the_scalar_the_entry_reports(name):
    """The fused path of sgm_lanczos: alpha_1 = q_1 . A q_1 as the consumer kernel reduced it == what matvec_dots reports for the
    same product, bit for bit."""
    R = F.reference(name, "real")
    H = make_handle(R)
    q1 = np.random.RandomState(9).standard_normal(R.n)
    T, Q = sg.lanczos(H, 2, q1)
    q = np.ascontiguousarray(Q[:, 0])
    y = np.zeros(R.n)
    wy, none, _ = H.matvec_dots(q, y, w=q, yy=False)
    assert none is None and wy[0] == T[1][0], (wy[0], T[1][0])
    assert np.array_equal(y, F.oracle_matvec(R, q, None))
    assert abs(wy[0] - F.exact_dot(q, y)) <= F.gamma(R.n) * np.abs(q * y).sum()


def test_refusals_and_rectangular_operators():
    """Neither dot asked for: BAD_ARG.  w on a rectangular matrix: UNSUPPORTED; y.y alone is fine there and exact."""
    import oracle as orc
    rs = np.random.RandomState(6)
    n, m = 700, 714
    deg = rs.randint(0, 9, size=n)
    ptr = np.concatenate([[1], 1 + np.cumsum(deg)]).astype(np.int32)
    node = (np.repeat(np.arange(n), deg) + rs.randint(0, 15, size=int(deg.sum())) + 1).astype(np.int32)
    val = rs.randint(1, 4, size=node.size).astype(np.float64)
    A = orc.CsrMatrix(n, m, ptr, node, val)
    H = sg.csr_matrix(n, m, ptr, node, val)
    x, w = rs.randint(1, 4, size=m).astype(np.float64), np.ones(n)
    y = np.zeros(n)
    with pytest.raises(sg.SigmaError) as e:
        H.matvec_dots(x, y, yy=False)
    assert e.value.code == BAD_ARG
    with pytest.raises(sg.SigmaError) as e:
        H.matvec_dots(x, y, w=w)
    assert e.value.code == UNSUPPORTED
    none, yy, cnt = H.matvec_dots(x, y)
    yref = A.matvec(x)
    assert none is None and np.array_equal(y, yref) and yy[0] == F.exact_dot(yref, yref) and cnt[0] == 8


def test_slice_schedule_keeps_the_fused_dots_exact():
    """160 x 128 x 210, 7 points, integer values, generated on the device: the sliced kernel with its grid at the cap (8400
    slices on 4096 workgroups, every workgroup a second and third round), slice_sched 0, 1 and 8 -- the schedules change which
    workgroup sums which slice, so on integers all three must leave the closed form sum over rows, computed in int64 on the
    device."""
    import torch
    nx, ny, nz = 160, 128, 210
    n = nx * ny * nz
    dev = torch.device("cuda", 0)
    k = torch.arange(n, device=dev)
    i, j, l = k % nx, (k // nx) % ny, k // (nx * ny)
    offs = ((-nx * ny, l > 0), (-nx, j > 0), (-1, i > 0), (0, torch.ones_like(k, dtype=torch.bool)), (1, i < nx - 1), (nx, j < ny - 1), (nx * ny, l < nz - 1))
    vals = (1, 2, 3, 2, 1, 3, 2)
    xi = (k * 7 + k // 11) % 3 + 1
    wi = ((k * 5 + k // 13) % 3 + 1) * (1 - 2 * ((k // 3) % 2))
    yi = torch.zeros(n, dtype=torch.int64, device=dev)
    for (o, m), v in zip(offs, vals):
        yi += torch.where(m, v * xi[torch.clamp(k + o, 0, n - 1)], torch.zeros_like(k))
    wy_ref, yy_ref = int((wi * yi).sum().item()), int((yi * yi).sum().item())
    assert int((wi.abs() * yi).sum().item()) < 2 ** 53 and yy_ref < 2 ** 53 and int(yi.min().item()) >= 1
    M = torch.stack([m for _o, m in offs], 1)
    Ccol = torch.stack([k + o for o, _m in offs], 1)
    V = torch.tensor(vals, dtype=torch.float64, device=dev).repeat(n, 1)
    ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(M.sum(1), 0)
    ptr1, node1, val = (ptr + 1).to(torch.int32), (Ccol[M] + 1).to(torch.int32), V[M].contiguous()
    x, w, yd = xi.double(), wi.double(), yi.double()
    out = {}
    A = sg.csr_matrix(n, n, ptr1, node1, val)
    assert A.kernel.startswith("k_csr_sl<W=7>")
    for sched in (0, 1, 8):              # (the handle's own option: the schedule is rebuilt for the next product)
        A.set_option("slice_sched", sched)
        y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
        wy, yy, cnt = A.matvec_dots(x, y, w=w)
        sg.synchronize()
        assert torch.equal(y, yd), sched
        out[sched] = (wy[0], yy[0], cnt[0])
    for sched in (0, 1, 8):
        assert out[sched] == (float(wy_ref), float(yy_ref), 4096), (sched, out[sched], wy_ref, yy_ref)


def test_dot_of_integer_vectors_is_exact():
    """sg.dot (FDot2 through launch_elem: the partial-sum machinery every vector kernel's fused dot uses) on +-{1, 2, 3}: the
    exact integer, at sizes around the workgroup edges, beyond one round of the grid, and odd."""
    rs = np.random.RandomState(12)
    for n in (1, 2, 3, 255, 256, 257, 4097, 262145, 1000003):
        a = (rs.randint(1, 4, size=n) * rs.choice([-1, 1], size=n)).astype(np.float64)
        b = (rs.randint(1, 4, size=n) * rs.choice([-1, 1], size=n)).astype(np.float64)
        assert sg.dot(a, b) == float(np.dot(a.astype(np.int64), b.astype(np.int64))), n
        assert sg.dot(a, a) == float(np.dot(a.astype(np.int64), a.astype(np.int64))), n
