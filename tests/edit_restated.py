"""The contract of the value edits (include/sigma_hip.h, "editing values on the device"), restated twice in numpy:

  * literally -- a transcription of the reference's loops (cs_matrices.f90:709-724,840-966, ellpack_matrices.f90:220-237,
    444-596, sparse_matrix_interfaces.f90:378-460), one triple after the other, every matching slot of the row;
  * vectorised -- locate by sorted keys, a stable argsort of the hits by slot, ordered segment sums position by position.

A structure S is a dict: {"fmt": "csr", "nrow", "ncol", "ptr", "node"} (1-based arrays as the reference holds them; rows may
be unsorted and may store a column twice) or {"fmt": "ell", "nrow", "ncol", "node" (nrow, max_d) = the reference's
(max_d, nrow) in Fortran order, "degrees"}.  Values: val(nnz), or val (nrow, max_d).  A slot is the 0-based flat position in
that value array.  Also here: the small P1 finite-element generator (after examples/fem.f90's formulas) and random batches.
"""
import numpy as np


def csr(nrow, ncol, ptr, node):
    return {"fmt": "csr", "nrow": int(nrow), "ncol": int(ncol), "ptr": np.asarray(ptr, np.int32), "node": np.asarray(node, np.int32)}


def ell(nrow, ncol, node, degrees):
    node = np.asarray(node, np.int32).reshape(int(nrow), -1)
    return {"fmt": "ell", "nrow": int(nrow), "ncol": int(ncol), "node": node, "degrees": np.asarray(degrees, np.int32)}


def nslots(S):
    return int(len(S["node"])) if S["fmt"] == "csr" else int(S["node"].size)


def row_slots(S, i):
    """(flat slots, their columns) of row i (1-based) in the order the reference scans them"""
    if S["fmt"] == "csr":
        lo, hi = int(S["ptr"][i - 1]) - 1, int(S["ptr"][i]) - 1
        return np.arange(lo, hi), S["node"][lo:hi]
    md = S["node"].shape[1]
    d = int(S["degrees"][i - 1])
    return (i - 1) * md + np.arange(d), S["node"][i - 1, :d]


def check_range(S, i, j):
    bad = np.nonzero((i < 1) | (i > S["nrow"]) | (j < 1) | (j > S["ncol"]))[0]
    return int(bad[0]) + 1 if len(bad) else 0


# ------------------------------------------------------------------ literal transcription
def locate_literal(S, i, j):
    """(hit_off (m+1), hit_slot, first_missing): the slots every triple addresses, ascending, and the smallest 1-based t
    that addresses none (0 = none)"""
    off, slots, miss = [0], [], 0
    for t in range(len(i)):
        sl, cols = row_slots(S, int(i[t]))
        n = 0
        for k in range(len(sl)):
            if cols[k] == j[t]:
                slots.append(int(sl[k]))
                n += 1
        if n == 0 and miss == 0:
            miss = t + 1
        off.append(len(slots))
    return np.array(off, np.int64), np.array(slots, np.int64), miss


def apply_literal(S, val, i, j, z, mode):
    """mode 'set' / 'add' on a copy of val; raises LookupError naming t for a missing entry (nothing is changed)"""
    _, _, miss = locate_literal(S, i, j)
    if miss:
        raise LookupError(miss)
    out = np.array(val, np.float64).copy()
    flat = out.reshape(-1)
    for t in range(len(i)):
        sl, cols = row_slots(S, int(i[t]))
        for k in range(len(sl)):
            if cols[k] == j[t]:
                if mode == "set":
                    flat[sl[k]] = z[t]
                else:
                    flat[sl[k]] = flat[sl[k]] + z[t]
    return out


def get_literal(S, val, i, j):
    flat = np.asarray(val, np.float64).reshape(-1)
    z = np.zeros(len(i))
    for t in range(len(i)):
        sl, cols = row_slots(S, int(i[t]))
        for k in range(len(sl)):
            if cols[k] == j[t]:
                z[t] = flat[sl[k]]
    return z


# ------------------------------------------------------------------ vectorised
def _stored(S):
    """(slots, rows, cols) of every addressable slot, ascending slot"""
    if S["fmt"] == "csr":
        rows = np.repeat(np.arange(1, S["nrow"] + 1, dtype=np.int64), np.diff(S["ptr"].astype(np.int64)))
        return np.arange(len(rows), dtype=np.int64), rows, S["node"].astype(np.int64)
    n, md = S["node"].shape
    live = np.arange(md)[None, :] < S["degrees"][:, None]
    slots = np.nonzero(live.reshape(-1))[0].astype(np.int64)
    return slots, slots // md + 1, S["node"].reshape(-1)[slots].astype(np.int64)


def locate_vectorised(S, i, j):
    slots, rows, cols = _stored(S)
    key = rows * (S["ncol"] + 1) + cols
    order = np.argsort(key, kind="stable")               # inside one key: ascending slot
    skey = key[order]
    tkey = np.asarray(i, np.int64) * (S["ncol"] + 1) + np.asarray(j, np.int64)
    lo, hi = np.searchsorted(skey, tkey, "left"), np.searchsorted(skey, tkey, "right")
    cnt = hi - lo
    off = np.zeros(len(tkey) + 1, np.int64)
    np.cumsum(cnt, out=off[1:])
    src = np.repeat(np.arange(len(tkey), dtype=np.int64), cnt)
    pos = lo[src] + (np.arange(off[-1], dtype=np.int64) - off[src])
    missing = np.nonzero(cnt == 0)[0]
    return off, slots[order[pos]], (int(missing[0]) + 1 if len(missing) else 0)


def apply_vectorised(S, val, i, j, z, mode):
    off, hslot, miss = locate_vectorised(S, i, j)
    if miss:
        raise LookupError(miss)
    out = np.array(val, np.float64).copy()
    flat = out.reshape(-1)
    z = np.asarray(z, np.float64)
    src = np.repeat(np.arange(len(i), dtype=np.int64), np.diff(off))
    order = np.argsort(hslot, kind="stable")             # every slot's chain in ascending t
    s, t = hslot[order], src[order]
    head = np.ones(len(s), bool)
    head[1:] = s[1:] != s[:-1]
    start = np.nonzero(head)[0]
    length = np.diff(np.append(start, len(s)))
    uslot = s[start]
    if mode == "set":
        flat[uslot] = z[t[start + length - 1]]
        return out
    for k in range(int(length.max()) if len(length) else 0):
        live = length > k
        flat[uslot[live]] = flat[uslot[live]] + z[t[start[live] + k]]     # one rounded addition per position
    return out


def get_vectorised(S, val, i, j):
    off, hslot, _ = locate_vectorised(S, i, j)
    flat = np.asarray(val, np.float64).reshape(-1)
    z = np.zeros(len(i))
    has = np.diff(off) > 0
    z[has] = flat[hslot[off[1:][has] - 1]]
    return z


# ------------------------------------------------------------------ the composite calls as batches
def expand_multiple(is_, js, B):
    """set / add_multiple_values(is, js, B): for k in is: for l in js: (is(k), js(l), B(k,l)) -- rows outer"""
    is_, js, B = np.asarray(is_, np.int32), np.asarray(js, np.int32), np.asarray(B, np.float64)
    return np.repeat(is_, len(js)), np.tile(js, len(is_)), B.reshape(-1).copy()


def matrix_triples(SB, valB, alpha=None):
    """add_sparse_matrix(A, B, alpha): B's stored entries in cursor order, z = alpha * B_ij rounded"""
    slots, rows, cols = _stored(SB)
    z = np.asarray(valB, np.float64).reshape(-1)[slots]
    if alpha is not None:
        z = np.float64(alpha) * z
    return rows.astype(np.int32), cols.astype(np.int32), z


def chain_stats(S, i, j):
    off, hslot, _ = locate_vectorised(S, i, j)
    u, c = np.unique(hslot, return_counts=True)
    return len(u), int(c.max()) if len(c) else 0


# ------------------------------------------------------------------ P1 finite elements on a jittered grid
def fem_grid(nx, ny, seed=1, jitter=0.1):
    """nx x ny nodes, two triangles per cell; x (2, nn), ele (3, ne), 1-based node numbers"""
    rs = np.random.RandomState(seed)
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    x = np.stack([gx.reshape(-1), gy.reshape(-1)])
    x = x + rs.uniform(-jitter, jitter, size=x.shape)
    cx, cy = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1))
    a = (cy * nx + cx).reshape(-1) + 1
    b, c, d = a + 1, a + nx, a + nx + 1
    ele = np.empty((3, 2 * len(a)), np.int32)
    ele[:, 0::2] = np.stack([a, b, d])
    ele[:, 1::2] = np.stack([a, d, c])
    return x, ele


def fem_elements(x, ele, kind):
    """element matrices (ne, 3, 3) after examples/fem.f90 (laplacian2d :28-49, mass2d :68-87)"""
    e = ele.astype(np.int64) - 1
    if kind == "stiffness":
        V = np.empty((e.shape[1], 3, 2))
        for i in range(3):
            j, k = e[(i + 1) % 3], e[(i + 2) % 3]
            V[:, i, 0] = x[1, j] - x[1, k]
            V[:, i, 1] = x[0, k] - x[0, j]
        det = V[:, 0, 0] * V[:, 1, 1] - V[:, 0, 1] * V[:, 1, 0]
        area = np.abs(det) / 2.0
        G = V[:, :, None, 0] * V[:, None, :, 0] + V[:, :, None, 1] * V[:, None, :, 1]
        return (0.25 / area)[:, None, None] * G
    T = np.empty((e.shape[1], 2, 2))
    for jj in range(2):
        for ii in range(2):
            T[:, ii, jj] = x[ii, e[jj]] - x[ii, e[2]]
    area = 0.5 * np.abs(T[:, 0, 0] * T[:, 1, 1] - T[:, 0, 1] * T[:, 1, 0])
    BE = np.repeat((area / 12.0)[:, None, None], 3, 1).repeat(3, 2)
    for ii in range(3):
        BE[:, ii, ii] = area / 6.0
    return BE


def fem_indices(ele):
    """the (i, j) of fem.f90's stream: for n: for j: for i: (ele(i,n), ele(j,n))"""
    ti = np.repeat(ele.T[:, None, :], 3, 1).reshape(-1)            # i fastest
    tj = np.repeat(ele.T[:, :, None], 3, 2).reshape(-1)
    return ti.astype(np.int32), tj.astype(np.int32)


def fem_triples(x, ele, kind):
    AE = fem_elements(x, ele, kind)                                  # AE[n, i, j]
    ti, tj = fem_indices(ele)
    return ti, tj, np.ascontiguousarray(AE.transpose(0, 2, 1)).reshape(-1)     # (n, j, i) order


def pattern_csr(nrow, ncol, ei, ej):
    """cs_graph of an edge list in insertion order (ll_graphs.f90:355-370 + cs_graphs.f90:109-197): repeated edges ignored,
    a row's columns in the order of their first insertion"""
    key = ei.astype(np.int64) * (ncol + 1) + ej
    _, first = np.unique(key, return_index=True)
    first.sort()
    r, c = ei[first], ej[first]
    order = np.argsort(r, kind="stable")
    ptr = np.ones(nrow + 1, np.int32)
    np.cumsum(np.bincount(r - 1, minlength=nrow), out=ptr[1:])
    ptr[1:] += 1
    return csr(nrow, ncol, ptr, c[order])


# ------------------------------------------------------------------ random structures and batches
def random_csr(rs, nrow, ncol, mean_deg, dup_frac=0.2, empty_rows=()):
    """unsorted rows, some columns stored twice (what sgm_csr_create accepts and no reference assembly produces)"""
    ptr, node = [1], []
    for r in range(nrow):
        if r in empty_rows:
            ptr.append(ptr[-1])
            continue
        d = 1 + rs.poisson(mean_deg)
        cols = list(rs.permutation(ncol)[:min(d, ncol)] + 1)
        for c in list(cols):
            if rs.rand() < dup_frac:
                cols.insert(rs.randint(len(cols) + 1), c)
        node += cols
        ptr.append(ptr[-1] + len(cols))
    return csr(nrow, ncol, ptr, node)


def random_ell(rs, nrow, ncol, max_d):
    deg = rs.randint(0, max_d + 1, size=nrow)
    deg[rs.randint(nrow)] = max_d
    node = np.zeros((nrow, max_d), np.int32)
    for r in range(nrow):
        cols = rs.permutation(ncol)[:deg[r]] + 1
        node[r, :deg[r]] = cols
        if deg[r]:
            node[r, deg[r]:] = cols[-1]                  # padding repeats the last neighbour (ellpack_graphs.f90:164)
    return ell(nrow, ncol, node, deg)


def special_values(rs, m, nan=True):
    """normal values with +0.0, -0.0 and +Inf among them; nan: also -Inf and NaN (sums then make NaNs, whose payload bits are
    the adder's choice: compare those by position)"""
    z = rs.standard_normal(m)
    pick = rs.rand(m)
    z[pick < 0.05] = 0.0
    z[(pick >= 0.05) & (pick < 0.10)] = -0.0
    z[(pick >= 0.10) & (pick < 0.12)] = np.inf
    if nan:
        z[(pick >= 0.12) & (pick < 0.13)] = -np.inf
        z[(pick >= 0.13) & (pick < 0.14)] = np.nan
    return z


def random_batch(rs, S, m, repeats=0.5, nan=True):
    """m triples on stored entries, a share of them repeating earlier ones"""
    slots, rows, cols = _stored(S)
    pick = rs.randint(len(slots), size=m)
    rep = rs.rand(m) < repeats
    pick[rep] = pick[rs.randint(max(1, m // 8), size=int(rep.sum()))]
    return rows[pick].astype(np.int32), cols[pick].astype(np.int32), special_values(rs, m, nan)
