"""The contract of the algebraic coarsening (sgm_mat_aggregate / sgm_mg_aggregation_hierarchy),
restated twice for the tests.

Matrices are (nrow, ncol, ptr, node, val) with 1-based ptr / node, as stored; every index below is 0-based.

    d(i)      the LAST stored copy of a_ii, 0.0 when absent
    strong    a stored entry a of row i, column j != i, with a*a >= (theta*theta) * (|d(i)| * |d(j)|) (each product rounded
              on its own; a NaN on either side: not strong); N(i) = the j with a strong stored (i,j) or (j,i)
    key(i)    h = uint32(i) * 0x9E3779B1; h ^= h >> 15; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16;
              key = (uint64(h) << 32) | (i + 1)
    roots     i in R <=> no j at distance 1 or 2 with key(j) > key(i) is in R
    numbers   roots 1..nagg by ascending row
    phase 1   a non-root with a root in N(i) joins the root of largest key
    phase 2   every other vertex joins the aggregate of the largest-key member of N(i) that is a root or a phase 1 vertex
    P         T(i, agg(i)) = 1.0; smooth_omega == 0: P = T; else W = A T, row i of W times -(smooth_omega * idiag(i)),
              P = T + W (algebra_restated), idiag(i) = 1.0 / d(i) or 0.0 when d(i) == 0

* `literal` transcribes this: the sequential greedy pass over the squared graph in descending key order, loops for the phases.
* `vectorised` runs the parallel rounds (two neighbour-max passes, np.maximum.at) and the phases as array operations.

`hierarchy` composes either with algebra_restated.vectorised; `cases()` are the matrices both test files walk."""
import os

import numpy as np

import algebra_restated as R
import mg_restated as MG

ROOT_WORD = np.uint64(0xFFFFFFFFFFFFFFFF)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------ shared pieces
def key_of(i):
    """key(i) with Python integers"""
    h = (i * 0x9E3779B1) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return (h << 32) | (i + 1)


def keys(n):
    """key(0 .. n-1) as uint64, with uint32 array arithmetic"""
    i = np.arange(n, dtype=np.uint32)
    h = i * np.uint32(0x9E3779B1)
    h ^= h >> np.uint32(15)
    h = h * np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h = h * np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return (h.astype(np.uint64) << np.uint64(32)) | (i.astype(np.uint64) + np.uint64(1))


def _csr0(M):
    n, m, ptr, node, val = M
    ptr = np.asarray(ptr, np.int64) - 1
    return n, ptr, np.asarray(node, np.int64) - 1, np.asarray(val, np.float64)


def diagonal(M):
    """d: the last stored copy of the diagonal entry, 0.0 when absent"""
    n, ptr, node, val = _csr0(M)
    row = np.repeat(np.arange(n), np.diff(ptr))
    d = np.zeros(n)
    hit = node == row
    d[row[hit]] = val[hit]                       # a repeated index keeps the last value assigned
    return d


def idiag(M):
    """1.0 / d(i) by mg_restated._Rows' rule, 0.0 where d(i) == 0"""
    d = diagonal(M)
    with np.errstate(all="ignore"):
        inv = MG._Rows(M).idiag()
    return np.where(d == 0.0, 0.0, inv)


def strong_entries(M, theta):
    """(row, column) of every strong stored entry, in stored order"""
    n, ptr, node, val = _csr0(M)
    row = np.repeat(np.arange(n), np.diff(ptr))
    d = diagonal(M)
    t2 = float(theta) * float(theta)
    with np.errstate(all="ignore"):
        strong = (node != row) & (val * val >= t2 * (np.abs(d[row]) * np.abs(d[node])))
    return row[strong], node[strong]


# ------------------------------------------------------------------------------------ literal
def literal(M, theta):
    """(agg (1-based, int32), nagg)"""
    n, ptr, node, val = _csr0(M)
    d = [0.0] * n
    for i in range(n):
        for e in range(ptr[i], ptr[i + 1]):
            if node[e] == i:
                d[i] = float(val[e])
    t2 = float(theta) * float(theta)
    N = [set() for _ in range(n)]
    for i in range(n):
        for e in range(ptr[i], ptr[i + 1]):
            j, a = int(node[e]), float(val[e])
            if j != i and a * a >= t2 * (abs(d[i]) * abs(d[j])):     # (a comparison with a NaN is false)
                N[i].add(j)
                N[j].add(i)
    key = [key_of(i) for i in range(n)]
    root = [False] * n
    for i in sorted(range(n), key=lambda v: -key[v]):                 # every vertex of larger key is decided already
        near = any(root[j] for j in N[i]) or any(root[k] for j in N[i] for k in N[j] if k != i)
        root[i] = not near
    agg = [0] * n
    nagg = 0
    for i in range(n):
        if root[i]:
            nagg += 1
            agg[i] = nagg
    phase1 = list(agg)
    for i in range(n):
        if not root[i]:
            best = max((j for j in N[i] if root[j]), key=lambda v: key[v], default=None)
            if best is not None:
                phase1[i] = agg[best]
    out = list(phase1)
    for i in range(n):
        if phase1[i] == 0:
            best = max((j for j in N[i] if phase1[j] != 0), key=lambda v: key[v])
            out[i] = phase1[best]
    return np.array(out, np.int32), nagg


# ------------------------------------------------------------------------------------ vectorised: the rounds
def vectorised(M, theta, stats=None):
    n = M[0]
    r, c = strong_entries(M, theta)
    U, V = np.concatenate([r, c]), np.concatenate([c, r])             # V in N(U), both directions
    key = keys(n)
    s = key.copy()
    rounds = 0
    while True:
        undecided = (s != ROOT_WORD) & (s != 0)
        if not undecided.any():
            break
        m1 = s.copy()
        np.maximum.at(m1, U, s[V])
        m2 = m1.copy()
        np.maximum.at(m2, U, m1[V])
        removed = undecided & (m2 == ROOT_WORD)
        new_root = undecided & ~removed & (m2 == s)
        s[removed] = 0
        s[new_root] = ROOT_WORD
        rounds += 1
    root = s == ROOT_WORD
    num = np.cumsum(root)
    nagg = int(num[-1]) if n else 0
    agg = np.where(root, num, 0)
    low = np.uint64(0xFFFFFFFF)
    best = np.zeros(n, np.uint64)
    m = ~root[U] & root[V]
    np.maximum.at(best, U[m], key[V[m]])
    got = best != 0
    phase1 = agg.copy()
    phase1[got] = agg[(best[got] & low).astype(np.int64) - 1]
    best2 = np.zeros(n, np.uint64)
    m = (phase1[U] == 0) & (phase1[V] != 0)
    np.maximum.at(best2, U[m], key[V[m]])
    rest = phase1 == 0
    out = phase1.copy()
    out[rest] = phase1[(best2[rest] & low).astype(np.int64) - 1]
    if stats is not None:
        stats.append({"rows": n, "aggregates": nagg, "rounds": rounds, "strong": len(r)})
    return out.astype(np.int32), nagg


# ------------------------------------------------------------------------------------ the prolongation and the hierarchy
def tentative(agg, nagg):
    n = len(agg)
    return n, nagg, np.arange(1, n + 2, dtype=np.int32), np.asarray(agg, np.int32), np.ones(n)


def prolongation(A, agg, nagg, smooth_omega):
    T = tentative(agg, nagg)
    if smooth_omega == 0:
        return T
    n, m, ptr, node, val = R.vectorised("product", A, T)
    with np.errstate(all="ignore"):
        f = -(np.float64(smooth_omega) * idiag(A))
        val = np.repeat(f, np.diff(ptr)) * val
    return R.vectorised("sum", T, (n, m, ptr, node, val))


def hierarchy(A, theta=0.08, smooth_omega=2.0 / 3.0, max_levels=25, min_coarse=64, aggregate=vectorised, stats=None):
    """[P_0, P_1, ...] (possibly empty)"""
    Ps = []
    levels = 1
    while levels < max_levels and A[0] > min_coarse:
        agg, nagg = vectorised(A, theta, stats) if aggregate is vectorised else aggregate(A, theta)
        if nagg >= A[0]:
            break
        Ps.append(prolongation(A, agg, nagg, smooth_omega))
        levels += 1
        if levels < max_levels and nagg > min_coarse:
            A = R.vectorised("ptap", A, Ps[-1])
        else:
            break
    return Ps


# ------------------------------------------------------------------------------------ the matrices of the tests
def _golden_csr(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    ptr, node, val = g["ref_ptr"], g["ref_node"], g["ref_val"]
    n = len(ptr) - 1
    return n, n, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64)


def _poisson(nx, ny):
    from sigma_amd import problems as Pr
    ptr, node, val = Pr.poisson2d_csr(nx, ny)
    return nx * ny, nx * ny, ptr, node, val


def _from_rows(rows):
    """rows: list of lists of (column (0-based), value)"""
    ptr = np.cumsum([0] + [len(r) for r in rows]) + 1
    node = np.array([c + 1 for r in rows for c, _ in r], np.int32)
    val = np.array([v for r in rows for _, v in r], np.float64)
    return len(rows), len(rows), ptr.astype(np.int32), node, val


def path(n):
    return _from_rows([[(j, 2.0 if j == i else -1.0) for j in (i - 1, i, i + 1) if 0 <= j < n] for i in range(n)])


def star(leaves):
    rows = [[(0, float(leaves))] + [(j, -1.0) for j in range(1, leaves + 1)]]
    rows += [[(0, -1.0), (j, 1.0)] for j in range(1, leaves + 1)]
    return _from_rows(rows)


def cases():
    """name -> matrix; built on every call (cheap), the same in both test files"""
    from sigma_amd import problems as Pr
    out = {}
    for nx, ny in ((31, 31), (33, 29), (100, 70)):
        out[f"poisson_{nx}x{ny}"] = _poisson(nx, ny)
    ptr, node, val = Pr.laplace3d_csr(8, 7, 6)
    out["laplace3d_8x7x6"] = (336, 336, ptr, node, val)
    out["random_spd_300"] = MG.random_spd_case(300)[0]
    out["stencil27_9x8x8"] = MG.stencil27_case(9, 8, 8)[0]
    out["duplicates_16"] = _golden_csr("duplicates_csr_16")
    out["random_skew_128"] = _golden_csr("random_skew_128")
    rs = np.random.RandomState(20240607)
    n, _, ptr, node, val = R.random_csr(rs, 150, 150, 0.03)
    out["pattern_asymmetric_150"] = (n, n, ptr, node, val)
    out["diagonal_40"] = _from_rows([[(i, 1.0 + i)] for i in range(40)])
    out["n1"] = _from_rows([[(0, 3.0)]])
    out["n2"] = _from_rows([[(0, 2.0), (1, -1.0)], [(0, -1.0), (1, 2.0)]])
    out["path_65"] = path(65)
    out["path_513"] = path(513)
    out["star_200"] = star(200)
    # row 3 stores a zero diagonal, row 5 none: with theta > 0 their couplings are strong whatever their size
    n, _, ptr, node, val = path(12)
    val = val.copy()
    val[(np.asarray(node) == 4) & (np.repeat(np.arange(12), np.diff(ptr)) == 3)] = 0.0
    keep = ~((np.asarray(node) == 6) & (np.repeat(np.arange(12), np.diff(ptr)) == 5))
    ptr2 = np.concatenate([[0], np.cumsum(np.bincount(np.repeat(np.arange(12), np.diff(ptr))[keep], minlength=12))]) + 1
    out["zero_and_missing_diagonal"] = (12, 12, ptr2.astype(np.int32), np.asarray(node)[keep], val[keep])
    n, _, ptr, node, val = _poisson(9, 7)
    val = val.copy()
    val[40] = np.nan
    out["one_nan"] = (n, n, ptr, node, val)
    return out


HIERARCHY_CASES = ("poisson_33x29", "poisson_100x70", "laplace3d_8x7x6", "random_spd_300", "stencil27_9x8x8")
