"""The contract of sgm_mat_matmat (include/sigma_hip.h) restated in numpy.  Host only: nothing here touches a GPU.

Column by column, every product and every addition rounded on its own, a row's terms added left to right in stored order:

    op = 0            Y(i, j) = 0.0 + z,   z = ((0.0 + a_i1 x_c1) + a_i2 x_c2) + ...
    ADD               Y(i, j) = Y0(i, j) + z
    TRANS             the terms of column i of A in (row, slot) order -- the order the reference's scatter adds them in --
                      summed from 0.0
    TRANS | ADD       the same sum CHAINED onto Y0(i, j): ((Y0 + t_1) + t_2) + ...

An ELLPACK matrix walks all max_d slots of a row (its padding multiplies 0.0 by x(last neighbour)).

`blocks(k, widths)` restates how a call with k columns is cut: left to right, the largest selected width that fits, single
columns for what no width fits.
"""
import numpy as np

OP_ADD, OP_TRANS = 1, 2


def rows_of(A):
    """(n, m, ptr0, col0, val): the stored slots of an oracle CsrMatrix / EllMatrix, row by row, 0-based."""
    if A.ptr is not None:
        return A.n, A.m, A.ptr.astype(np.int64) - 1, A.node.astype(np.int64) - 1, A.val
    ptr0 = np.arange(A.n + 1, dtype=np.int64) * A.max_d
    return A.n, A.m, ptr0, A.node.reshape(-1).astype(np.int64) - 1, A.val.reshape(-1)


def transposed(n, m, ptr0, col, val):
    """The rows of A^T with every row's terms in (source row, slot) order: a stable sort by column."""
    order = np.argsort(col, kind="stable")
    src_row = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr0))
    tptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=m))]).astype(np.int64)
    return tptr, src_row[order], val[order]


def sum_rows(ptr0, col, val, x, z):
    """z(i) <- (((z(i) + v_1 x_c1) + v_2 x_c2) + ...) over row i's slots in stored order; one rounding per operation."""
    lens = np.diff(ptr0)
    with np.errstate(invalid="ignore", over="ignore"):
        for u in range(int(lens.max()) if lens.size else 0):
            r = np.nonzero(lens > u)[0]
            k = ptr0[r] + u
            p = val[k] * x[col[k]]
            z[r] = z[r] + p
    return z


def matmat(A, X, Y0=None, op=0):
    """The block product of an oracle matrix, per the contract.  X: (x length, k); Y0: (y length, k) with the add bit."""
    n, m, ptr0, col, val = rows_of(A)
    add, trans = bool(op & OP_ADD), bool(op & OP_TRANS)
    X = np.asarray(X, np.float64)
    k = X.shape[1]
    if trans:
        ptr0, col, val = transposed(n, m, ptr0, col, val)
        n, m = m, n
    assert X.shape[0] == m and (not add or Y0.shape == (n, k))
    Y = np.empty((n, k), order="F")
    for j in range(k):
        x = np.ascontiguousarray(X[:, j])
        with np.errstate(invalid="ignore", over="ignore"):
            if trans and add:
                Y[:, j] = sum_rows(ptr0, col, val, x, np.array(Y0[:, j], np.float64))
            else:
                z = sum_rows(ptr0, col, val, x, np.zeros(n))
                Y[:, j] = (Y0[:, j] + z) if add else (0.0 + z)
    return Y


def blocks(k, widths):
    """The widths a call with k columns is cut into, left to right."""
    out, rem = [], k
    while rem > 0:
        w = max([w for w in widths if w <= rem], default=1)
        out.append(w)
        rem -= w
    return out


def k_max(widths):
    """2 KBmax - 1: one block of every width of a power-of-two ladder plus the single-column remainder."""
    return 2 * max(widths) - 1
