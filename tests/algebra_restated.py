"""The contract of sparse matrix algebra (src/matrix/sparse_matrix_algebra.f90), restated twice for the tests.

Matrices are (nrow, ncol, ptr, node, val) with 1-based ptr / node, as stored.  For every output row the reference
produces a sequence of terms (column, value) in contribution order; the row's columns are the distinct columns in the
order of their FIRST term, and each value is +0.0 plus its terms added one after another in sequence order.

* `literal(op, X, Y)` transcribes the reference's loops (sparse_matrix_sum :25-145, sparse_matrix_product_C :310-420,
  PtAP :425-538, RARt :543-655) with Python floats: slow, for fixture sizes.
* `vectorised(op, X, Y)` expands every term as arrays (row, column, value) in sequence order, takes the first appearance
  of each (row, column) and accumulates with np.add.at (unbuffered: in index order) -- for large matrices.

op is one of "sum", "product", "ptap", "rart"."""
import numpy as np

OPS = ("sum", "product", "ptap", "rart")


def _rows(m):
    nrow, ncol, ptr, node, val = m
    ptr = np.asarray(ptr, np.int64) - 1
    node = np.asarray(node, np.int64) - 1
    return [[(int(node[e]), float(val[e])) for e in range(ptr[i], ptr[i + 1])] for i in range(nrow)]


def _columns(m):
    """R%get_column on CSR: the entries of column k by row ascending, duplicates in stored order"""
    nrow, ncol = m[0], m[1]
    cols = [[] for _ in range(ncol)]
    for r, row in enumerate(_rows(m)):
        for c, v in row:
            cols[c].append((r, v))
    return cols


def _assemble(nrow, ncol, seqs):
    ptr, node, val = [1], [], []
    for seq in seqs:
        slot = {}
        vals = []
        for j, z in seq:
            if j not in slot:                        # ll_graph%add_edge: a repeated edge is ignored
                slot[j] = len(vals)
                node.append(j + 1)
                vals.append(0.0)                     # B%zero(): +0.0
            vals[slot[j]] = vals[slot[j]] + z        # add_value: val = val + z
        val += vals
        ptr.append(len(node) + 1)
    return nrow, ncol, np.array(ptr, np.int32), np.array(node, np.int32), np.array(val, np.float64)


def literal(op, X, Y):
    if op == "sum":
        xr, yr = _rows(X), _rows(Y)
        return _assemble(X[0], X[1], [xr[i] + yr[i] for i in range(X[0])])
    if op == "product":
        xr, yr = _rows(X), _rows(Y)
        seqs = []
        for i in range(X[0]):
            seqs.append([(j, b * c) for k, b in xr[i] for j, c in yr[k]])
        return _assemble(X[0], Y[1], seqs)
    # PtAP / RARt: the loop over A's entries (k, l) in cursor order
    A = _rows(X)
    if op == "ptap":
        prow = _rows(Y)
        nout = Y[1]
    else:
        prow = _columns(Y)
        nout = Y[0]
    seqs = [[] for _ in range(nout)]
    for k in range(X[0]):
        for l, a in A[k]:
            for i, p_ki in prow[k]:
                for j, p_lj in prow[l]:
                    seqs[i].append((j, p_ki * a * p_lj))
    return _assemble(nout, nout, seqs)


def _expand(ptr0, deg, sel):
    """for every index e in sel: the entries ptr0[e] .. ptr0[e]+deg[e]-1, in order; returns (owner position, entry)"""
    cnt = deg[sel]
    owner = np.repeat(np.arange(len(sel)), cnt)
    start = np.repeat(ptr0[sel] - (np.cumsum(cnt) - cnt), cnt)
    return owner, start + np.arange(int(cnt.sum()))


def _csr0(m):
    nrow, ncol, ptr, node, val = m
    ptr = np.asarray(ptr, np.int64) - 1
    return ptr, np.asarray(node, np.int64) - 1, np.asarray(val, np.float64), np.diff(ptr)


def _row_ids(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


def terms(op, X, Y):
    """(nrow, ncol, row, col, value) of every term, in sequence order"""
    if op == "sum":
        xp, xn, xv, _ = _csr0(X)
        yp, yn, yv, _ = _csr0(Y)
        row = np.concatenate([_row_ids(xp), _row_ids(yp)])
        order = np.argsort(row, kind="stable")
        return X[0], X[1], row[order], np.concatenate([xn, yn])[order], np.concatenate([xv, yv])[order]
    if op == "product":
        xp, xn, xv, _ = _csr0(X)
        yp, yn, yv, ydeg = _csr0(Y)
        xrow = _row_ids(xp)
        owner, e2 = _expand(yp, ydeg, xn)
        with np.errstate(all="ignore"):
            z = xv[owner] * yv[e2]
        return X[0], Y[1], xrow[owner], yn[e2], z
    ap, an, av, _ = _csr0(X)
    if op == "ptap":
        pp, pn, pv, pdeg = _csr0(Y)
        nout = Y[1]
    else:                                           # P = R^T: column k of R by row ascending, duplicates in stored order
        rp, rn, rv, _ = _csr0(Y)
        rrow = _row_ids(rp)
        order = np.argsort(rn, kind="stable")
        pdeg = np.bincount(rn, minlength=Y[1]).astype(np.int64)
        pp = np.concatenate([[0], np.cumsum(pdeg)])
        pn, pv = rrow[order], rv[order]
        nout = Y[0]
    prow = _row_ids(pp)
    arow = _row_ids(ap)
    # (n1, a): P entry n1 in row k, A entry a in row k
    o1, a = _expand(ap, np.diff(ap), prow)           # for every P entry n1 (row k): A's row k
    n1 = o1
    o2, n2 = _expand(pp, pdeg, an[a])                 # for every (n1, a): P's row l
    n1, a = n1[o2], a[o2]
    i = pn[n1]
    # sequence: i, then k (= row of a) ascending, then a (stored order), then n1 (stored order), then n2
    order = np.lexsort((n2, n1, a, i))
    n1, a, n2, i = n1[order], a[order], n2[order], i[order]
    with np.errstate(all="ignore"):
        z = (pv[n1] * av[a]) * pv[n2]
    del arow
    return nout, nout, i, pn[n2], z


def vectorised(op, X, Y):
    nrow, ncol, row, col, z = terms(op, X, Y)
    key = row.astype(np.int64) * max(ncol, 1) + col
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")          # distinct (row, column) by first appearance: row-major, then first term
    slot = np.empty(len(uk), np.int64)
    slot[order] = np.arange(len(uk))
    val = np.zeros(len(uk))                           # +0.0
    with np.errstate(all="ignore"):
        np.add.at(val, slot[inv.ravel()], z)          # unbuffered: the terms of a slot in sequence order
    orow = (uk[order] // max(ncol, 1))
    node = (uk[order] % max(ncol, 1)) + 1
    ptr = np.ones(nrow + 1, np.int64)
    ptr[1:] += np.cumsum(np.bincount(orow, minlength=nrow))
    return nrow, ncol, ptr.astype(np.int32), node.astype(np.int32), val


def bits(v):
    """value bits with every NaN made one NaN (the payload of a NaN is not part of the contract; its position is)"""
    v = np.asarray(v, np.float64).copy()
    v[np.isnan(v)] = np.nan
    return v.view(np.int64)


def same(a, b):
    return (a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
            and np.array_equal(bits(a[4]), bits(b[4])))


def random_csr(rs, nrow, ncol, density, dup=0.0, zeros=0.0, specials=0.0, empty_rows=0.0):
    """seeded CSR arrays with unsorted columns; dup: fraction of stored duplicate columns; zeros: fraction of stored +-0.0;
    specials: fraction of +-Inf / NaN; empty_rows: fraction of rows left empty"""
    ptr, node, val = [1], [], []
    for i in range(nrow):
        d = 0 if rs.rand() < empty_rows else rs.binomial(ncol, density)
        cols = list(rs.permutation(ncol)[:d])
        if cols and dup:
            cols += list(rs.choice(cols, size=rs.binomial(len(cols), dup)))
            rs.shuffle(cols)
        node += [c + 1 for c in cols]
        ptr.append(len(node) + 1)
    val = rs.standard_normal(len(node))
    if len(val):
        if zeros:
            k = rs.rand(len(val)) < zeros
            val[k] = np.where(rs.rand(k.sum()) < 0.5, -0.0, 0.0)
        if specials:
            k = rs.rand(len(val)) < specials
            val[k] = rs.choice([np.inf, -np.inf, np.nan], size=k.sum())
    return nrow, ncol, np.array(ptr, np.int32), np.array(node, np.int32), val


def fixture_operands(d):
    X = (int(d["x_shape"][0]), int(d["x_shape"][1]), d["x_ptr"], d["x_node"], d["x_val"])
    Y = (int(d["y_shape"][0]), int(d["y_shape"][1]), d["y_ptr"], d["y_node"], d["y_val"])
    Z = (int(d["z_shape"][0]), int(d["z_shape"][1]), d["z_ptr"], d["z_node"], d["z_val"])
    return OPS[int(d["op"])], X, Y, Z
