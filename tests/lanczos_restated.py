"""The contract of sgm_lanczos and sgm_generalized_lanczos (include/sigma_hip.h), restated in numpy for the tests, statement by
statement, from src/eigensolver.f90:27-155 as oracle/sigma_oracle.c restates it and not from the kernels: once in float64 with
the sum as a parameter, once in np.longdouble.  Host only: nothing here touches a GPU.

Every operation is rounded on its own; m = nsteps; `A u` is a callable (the tests pass the oracle matrix's matvec).

  lanczos                                                      generalized_lanczos (B%solve = `solve`, started from w)
    q_1 = q1 / sqrt(q1.q1)                                       w = B q1 ; q_1 = q1 / sqrt(w.q1) ; z_1 = B q_1 ; z_0 = 0
    i = 1 .. m:                                                  i = 1 .. m-1:
      w = A q_i ; alpha = q_i.w                                    w = A q_i ; v = w - beta z_{i-1}   (skipped at i = 1)
      i == m: T(2,m) = alpha, stop                                 alpha = sum(v * q_i) ; v = v - alpha z_i
      w = w - alpha q_i ; i > 1: w = w - beta q_{i-1}              w = solve(w, v) ; beta = sqrt(w.v)
      k = 1 .. i-2: h = q_k.w ; w = w - h q_k                      q_{i+1} = w / beta ; z_{i+1} = v / beta
      beta = sqrt(w.w) ; q_{i+1} = w / beta                        T(2,i) = alpha ; T(1,i) = T(3,i) = beta
      T(2,i) = alpha ; T(1,i) = T(3,i) = beta                    w = A q_m ; v = w - beta z_m ; T(2,m) = sum(v * q_m)

The order of a sum is the parameter `sum` (eigsh_restated.SUMS): "seq", one accumulator first element to last, is the oracle's;
"device" is the device's defined order, a function of n alone: with G = min(1024, max(1, ceil(n / 1024))) workgroups of 256
threads, thread t of the 256 G adds the products of elements 2i, 2i+1 for i = t, t + 256 G, ... to its own accumulator, which
starts at 0.0 (thread 0 then the last element of an odd n); each wave of 64 threads sums its accumulators by the butterfly
v += v[lane ^ 32], ^ 16, ... ^ 1; a workgroup adds its four wave sums left to right; for G > 1 the G workgroup sums are re-reduced
the same way by one workgroup: thread t adds sums t, t + 256, ... to 0.0, then the butterfly and the four wave sums
(eigsh_restated.device_sums).  Every sum of both routines is taken in that order, with one exception: on a leaf matrix (one
CSR or ELLPACK part) the alpha of plain Lanczos comes out of the product kernel's epilogue, in that kernel's own order (what
sgm_mat_matvec_dots reports; `alpha_of` feeds it in).  On composites and in-process partitions alpha is a sum in the device's
order like every other; over ranks each sum is reduced to a slot and all-reduced, which this restatement does not cover."""
import functools
from types import SimpleNamespace

import numpy as np

import eigsh_restated as ER
import mg_restated as MR
import minres_restated as MN

MUTATIONS = (None, "skip_single", "drop_last_correction")


def _dot_of(sum_):
    sums = ER.SUMS[sum_]
    return lambda a, b: sums((a * b)[:, None])[0]


def lanczos(A, q1, m, sum="device", dtype=np.float64, alpha_of=None, mutate=None):
    """The left loop above.  alpha_of(i, q_i, w) (i from 1) replaces alpha = q_i.w.  Returns T (3 x m) and Q (n x m).
    mutate (the sensitivity check of tests/test_lanczos_cpu.py only): "skip_single" leaves the last element of an odd n out of
    the update w = w - alpha q_i - beta q_{i-1} of step 3; "drop_last_correction" never applies the correction of k = i-2."""
    assert mutate in MUTATIONS
    ft = dtype
    dot = _dot_of(sum)
    q1 = np.asarray(q1, ft)
    n = len(q1)
    T = np.zeros((3, m), ft)
    Q = np.zeros((n, m), ft)
    beta = ft(0.0)
    with np.errstate(all="ignore"):
        Q[:, 0] = q1 / np.sqrt(dot(q1, q1))
        for i in range(1, m + 1):
            qi = Q[:, i - 1]
            w = A(qi)
            alpha = dot(qi, w) if alpha_of is None else ft(alpha_of(i, qi, w))
            if i == m:
                T[1, m - 1] = alpha
                break
            u = w - alpha * qi
            if i > 1:
                u = u - beta * Q[:, i - 2]
            if mutate == "skip_single" and i == 3 and n & 1:
                u[n - 1] = w[n - 1]
            w = u
            for k in range(1, i - 1):
                h = dot(Q[:, k - 1], w)
                if mutate == "drop_last_correction" and k == i - 2:
                    break
                w = w - h * Q[:, k - 1]
            beta = np.sqrt(dot(w, w))
            Q[:, i] = w / beta
            T[1, i - 1] = alpha
            T[0, i - 1] = T[2, i - 1] = beta
    return T, Q


def generalized_lanczos(A, B, solve, q1, m, sum="device", dtype=np.float64):
    """The right loop above; solve(w, v) returns the solution of B x = v that B's solver reaches from the initial guess w."""
    ft = dtype
    dot = _dot_of(sum)
    q1 = np.asarray(q1, ft)
    n = len(q1)
    T = np.zeros((3, m), ft)
    Q = np.zeros((n, m), ft)
    Z = np.zeros((n, m + 1), ft)                     # z_0 .. z_m
    beta = ft(0.0)
    with np.errstate(all="ignore"):
        w = B(q1)
        Q[:, 0] = q1 / np.sqrt(dot(w, q1))
        Z[:, 1] = B(Q[:, 0])
        for i in range(1, m):
            qi = Q[:, i - 1]
            w = A(qi)
            v = w - beta * Z[:, i - 1] if i > 1 else w
            alpha = dot(v, qi)
            v = v - alpha * Z[:, i]
            w = np.asarray(solve(w, v), ft)
            beta = np.sqrt(dot(w, v))
            Q[:, i] = w / beta
            Z[:, i + 1] = v / beta
            T[1, i - 1] = alpha
            T[0, i - 1] = T[2, i - 1] = beta
        w = A(Q[:, m - 1])
        v = w - beta * Z[:, m]
        T[1, m - 1] = dot(v, Q[:, m - 1])
    return T, Q


def cg(A, b, x0, tol, dtype=np.float64):
    """cg_solve (src/solver/cg_solvers.f90:116-150 as orc_cg restates it) from the initial guess x0, sums first element to
    last: the pencil's inner solve where the oracle cannot hold the operand (a composite: A is the block loop), and in
    longdouble.  (mg_restated.pcg starts from zero, on a float64 CSR matrix.)  Returns x."""
    dot = _dot_of("seq")
    x = np.array(x0, dtype)
    b = np.asarray(b, dtype)
    with np.errstate(all="ignore"):
        r = b - A(x)
        p = r.copy()
        res2 = dot(r, r)
        while np.sqrt(res2) > tol:
            q = A(p)
            alpha = res2 / dot(p, q)
            x = x + alpha * p
            r = r - alpha * q
            dpr = dot(r, r)
            p = r + (dpr / res2) * p
            res2 = dpr
    return x


# ------------------------------------------------------------------------------------ the cases
def tridiagonal(n):
    """symmetric, diagonally dominant, not Toeplitz (1-based CSR): diagonal 2 + (i mod 5) / 8, off-diagonal -(1 + (i mod 3) / 16)
    between rows i and i + 1"""
    i = np.arange(n)
    d = 2.0 + (i % 5) / 8.0
    e = -(1.0 + (i[:-1] % 3) / 16.0)
    deg = np.full(n, 3)
    deg[[0, n - 1]] = 2 if n > 1 else 1
    ptr = np.concatenate([[1], 1 + np.cumsum(deg)]).astype(np.int32)
    node = np.zeros(ptr[-1] - 1, np.int32)
    val = np.zeros(ptr[-1] - 1)
    lo = ptr[:-1] - 1
    has_l = i > 0
    node[lo[has_l]] = i[has_l]                       # column i - 1, 1-based
    val[lo[has_l]] = e[i[has_l] - 1]
    dpos = lo + has_l
    node[dpos] = i + 1
    val[dpos] = d
    has_r = i < n - 1
    node[dpos[has_r] + 1] = i[has_r] + 2
    val[dpos[has_r] + 1] = e[i[has_r]]
    return n, ptr, node, val


def grid5(nx, ny):
    from sigma_amd import problems as P
    ptr, node, val = P.poisson2d_csr(nx, ny)
    return nx * ny, ptr, node, val


def mass_like(n, ptr, node):
    """B of the pencil (tests/test_gpu_parity.py): diagonal 1 + (row mod 7) / 16, off-diagonal -1/16 on the pattern of A"""
    rows = np.repeat(np.arange(1, n + 1), np.diff(ptr))
    return np.where(rows == node, 1.0 + (rows % 7) / 16.0, -1.0 / 16.0)


# plain Lanczos on a CSR leaf: name -> (matrix, steps, what the size reaches)
PLAIN = {
    "grid15x17": (functools.partial(grid5, 15, 17), 12, "n = 255: one workgroup, odd tail"),
    "grid32x32": (functools.partial(grid5, 32, 32), 12, "n = 1024: the last n with one partial sum"),
    "grid41x25": (functools.partial(grid5, 41, 25), 12, "n = 1025: the first re-reduction, odd tail"),
    "tri2049": (functools.partial(tridiagonal, 2049), 12, "n = 2049: odd tail on three workgroups"),
    "tri262147": (functools.partial(tridiagonal, 262147), 4, "n = 262147: 257 partial sums, a second re-reduction round, odd"),
}
GRID = (33, 31)                 # the matrix of the ELLPACK, composite, partition and pencil cases: n = 1023
GRID_STEPS = 12
CUT = 511                       # the composite's block boundary: an odd row inside a grid line
DEGENERATE = {"n1": (1, 3), "n3": (3, 5)}          # name -> (n, steps)
# the accuracy table's keys: the symmetric runs, each named by what the ORACLE runs (the composite and the partitions of the
# 33 x 31 grid are the oracle's CSR run)
SYMMETRIC = tuple(PLAIN) + ("grid33x31", "grid33x31_ell", "pencil33x31")


def part_starts(n, nparts):
    """the part boundaries the partition tests of tests/test_gpu_parity.py use: even rows"""
    return np.array([0] + [2 * ((n * k // nparts) // 2) for k in range(1, nparts)] + [n], np.int64)


def start_vector(n, seed):
    return 2 * np.random.RandomState(seed).random_sample(n) - 1


@functools.lru_cache(maxsize=None)
def case(name):
    """n, ptr, node, val (1-based CSR), steps, q1, rows (mg_restated._Rows, for the longdouble products); the pencil also bval
    and brows.  The degenerate cases are tridiagonal(n) with q1 = 0.75, 0.5, ..."""
    if name in PLAIN:
        n, ptr, node, val = PLAIN[name][0]()
        steps = PLAIN[name][1]
    elif name in DEGENERATE:
        n, steps = DEGENERATE[name]
        n, ptr, node, val = tridiagonal(n)
    else:
        n, ptr, node, val = grid5(*GRID)
        steps = GRID_STEPS
    c = SimpleNamespace(name=name, n=n, ptr=ptr, node=node, val=val, steps=steps)
    c.q1 = 0.75 - 0.25 * np.arange(n) if name in DEGENERATE else start_vector(n, 12 + n % 7)
    c.rows = MR._Rows((n, n, ptr, node, val))
    if name == "pencil33x31":
        c.bval = mass_like(n, ptr, node)
        c.brows = MR._Rows((n, n, ptr, node, c.bval))
    for a in (c.val, c.q1):
        a.setflags(write=False)
    return c


def oracle_matrix(name):
    """the oracle's matrix of a case (the pencil: A and B)"""
    import oracle as orc
    from sigma_amd import problems as P
    c = case(name)
    if name == "grid33x31_ell":
        return orc.EllMatrix.from_edges(c.n, c.n, *P.poisson2d_edges(*GRID))
    A = orc.CsrMatrix(c.n, c.n, c.ptr, c.node, c.val)
    if name == "pencil33x31":
        return A, orc.CsrMatrix(c.n, c.n, c.ptr, c.node, c.bval)
    return A


def composite_leaves(n, ptr, node, val, cut):
    """the 2 x 2 blocks of a CSR matrix cut at row and column `cut`: {(i, j): (nrow, ncol, ptr, node, val)}, 1-based, every row's
    entries in their stored order"""
    cuts = [0, cut, n]
    row = np.repeat(np.arange(n), np.diff(ptr))
    col = node - 1
    out = {}
    for i in range(2):
        for j in range(2):
            sel = (row >= cuts[i]) & (row < cuts[i + 1]) & (col >= cuts[j]) & (col < cuts[j + 1])
            nr = cuts[i + 1] - cuts[i]
            deg = np.bincount(row[sel] - cuts[i], minlength=nr)
            p = np.concatenate([[1], 1 + np.cumsum(deg)]).astype(np.int32)
            out[(i, j)] = (nr, cuts[j + 1] - cuts[j], p, (col[sel] - cuts[j] + 1).astype(np.int32), val[sel].copy())
    return out


def composite_matvec(leaves, cut, n):
    """y = 0 ; y_i = y_i + A_ij x_j block by block (composite_matvec_add over the oracle's leaves): a row that crosses the cut
    adds two separately rounded sums, which is not the assembled row's left-to-right sum"""
    import oracle as orc
    cuts = [0, cut, n]
    mats = {k: orc.CsrMatrix(*v) for k, v in leaves.items()}

    def matvec(x):
        x = np.ascontiguousarray(x, np.float64)
        y = np.zeros(n)
        for (i, j), L in sorted(mats.items()):
            L.matvec_add(x[cuts[j]:cuts[j + 1]].copy(), y[cuts[i]:cuts[i + 1]])
        return y
    return matvec


# ------------------------------------------------------------------------------------ the longdouble runs
def _ld_matvec(rows):
    val = rows.val.astype(np.longdouble)
    return lambda u: MN.rows_matvec(rows, u, val)


@functools.lru_cache(maxsize=None)
def longdouble_run(name):
    """(T, Q) of a symmetric case in np.longdouble (sums first element to last; the pencil's inner solve: the CG above in
    longdouble to 1e-17, three decades below the 1e-14 of the float64 runs)"""
    c = case(name)
    ld = np.longdouble
    A = _ld_matvec(c.rows)
    if name == "pencil33x31":
        B = _ld_matvec(c.brows)
        T, Q = generalized_lanczos(A, B, lambda w, v: cg(B, v, w, ld(1e-17), dtype=ld), c.q1, c.steps, "seq", ld)
    else:
        T, Q = lanczos(A, c.q1, c.steps, "seq", ld)
    for a in (T, Q):
        a.setflags(write=False)
    return T, Q


def deviations(name, T, Q):
    """max |T - T_ld|, max |Q - Q_ld| over all columns, and max |Q^T Q - I| (the pencil: |Q^T B Q - I|, its Lanczos vectors are
    B-orthonormal and never re-orthogonalised), the last in longdouble from Q alone"""
    Tl, Ql = longdouble_run(name)
    c = case(name)
    Qx = np.asarray(Q, np.longdouble)
    if name == "pencil33x31":
        B = _ld_matvec(c.brows)
        BQ = np.stack([B(Qx[:, j].copy()) for j in range(Qx.shape[1])], 1)
    else:
        BQ = Qx
    G = Qx.T @ BQ
    return (float(np.max(np.abs(T - Tl))), float(np.max(np.abs(Qx - Ql))), float(np.max(np.abs(G - np.eye(G.shape[0])))))


# ------------------------------------------------------------------------------------ one case per SpMV kernel family
# kernel family (fused_dot_cases.KERNEL_KEYS) -> the case of fused_dot_cases.CASES that stands for it, with its `real` data:
# independent normal values on every stored entry, so none of these matrices is symmetric -- they take part in the bit-for-bit
# comparison only.  Lanczos on an unsymmetric matrix is still the same sequence of statements.
FAMILY_STEPS = 6
FAMILY = {
    "k_csr_sl": "sl_banded_513_w8",
    "k_csr_slb": "slb_27pt_23x17x11",
    "k_csr_sl32": "sl32_513_w16",
    "k_csr_do CW=1": "do1_2049",
    "k_csr_do CW=4": "do4_2049",
    "k_csr_sell xw": "sell_xw_700",
    "k_csr_sell": "sell_700",
    "k_csr_rl": "rl_700",
    "k_csr_spmv": "spmv_ragged_3001",
    "k_ellcb ell": "ellcb_ell_3001_d12",
    "k_ellcb csr": "ellcb_csr_3001",
    "k_ell_spmv": "ell_spmv_4097_d5",
    "k_ell_do<4>": "ell_do4_200_d3",
    "k_ell_do<8>": "ell_do8_200_d8",
    "k_ell_do<16>": "ell_do16_200_d16",
    "sliced ellpack": "ell_sliced_513",
    "composite": "composite_480",
}
