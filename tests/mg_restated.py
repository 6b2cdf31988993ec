"""The contract of the multigrid preconditioner (sgm_mg_create), restated twice for the tests.

Matrices are (nrow, ncol, ptr, node, val) with 1-based ptr / node, as stored.  Levels l = 0 .. L, A_0 = A,
A_{l+1} = P_l^T A_l P_l exactly as algebra_restated.vectorised("ptap", ...) builds it; idiag_l(i) = 1.0 / a_ii with the Jacobi
setup's rule (the LAST stored copy of the diagonal, 0.0 when absent).  Every operation is rounded on its own; a row sum is
+0.0 plus the individually rounded products in stored order.  vcycle(l, b):

    first sweep (zero start)      x(i) = omega * (idiag(i) * b(i))
    further sweeps, out of place  q = A_l x ; t(i) = b(i) - q(i) ; x'(i) = x(i) + omega * (idiag(i) * t(i))
    l == L                        coarse_sweeps sweeps
    otherwise                     nu_pre sweeps ; r = b - A_l x ; b_c = P_l^T r (the reference's scatter order) ;
                                  x_c = vcycle(l + 1, b_c) ; x(i) = x(i) + (0.0 + sum_k P_l(i,k) x_c(k)) ; nu_post sweeps

* `Literal` transcribes this with Python floats, entry by entry: slow, for small levels.
* `Vectorised` walks the SLOTS of all rows at once (slot s of every row that has one), which keeps every row's order.

Both take the hierarchy from `levels(A, Ps)`; `pcg` is the reference's preconditioned CG (cg_solvers.f90:160-190) on top."""
import numpy as np

import algebra_restated as R


def levels(A, Ps):
    """[A_0, A_1, ..., A_L] with A_{l+1} = P_l^T A_l P_l (algebra_restated.vectorised)"""
    out = [A]
    for P in Ps:
        out.append(R.vectorised("ptap", out[-1], P))
    return out


def _csr0(M):
    nrow, ncol, ptr, node, val = M
    return nrow, ncol, np.asarray(ptr, np.int64) - 1, np.asarray(node, np.int64) - 1, np.asarray(val, np.float64)


# ------------------------------------------------------------------------------------ literal
class Literal:
    def __init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps, lev=None):
        self.lev = lev if lev is not None else levels(A, Ps)
        self.Ps = list(Ps)
        self.omega, self.nu_pre, self.nu_post, self.coarse = float(omega), int(nu_pre), int(nu_post), int(coarse_sweeps)
        self.idiag = [self._idiag(M) for M in self.lev]

    @staticmethod
    def _idiag(M):
        n, _, ptr, node, val = _csr0(M)
        out = np.empty(n)
        for i in range(n):
            z = 0.0
            for e in range(ptr[i], ptr[i + 1]):
                if node[e] == i:
                    z = float(val[e])                  # the last stored copy
            with np.errstate(all="ignore"):
                out[i] = np.float64(1.0) / np.float64(z)
        return out

    @staticmethod
    def _matvec(M, x):
        n, _, ptr, node, val = _csr0(M)
        y = np.empty(n)
        for i in range(n):
            z = 0.0
            for e in range(ptr[i], ptr[i + 1]):
                z = z + float(val[e]) * float(x[node[e]])
            y[i] = 0.0 + z
        return y

    @staticmethod
    def _matvec_t(M, x):
        n, m, ptr, node, val = _csr0(M)
        y = [0.0] * m
        for j in range(n):                             # csc_matvec_add: y(node(k)) += val(k) * x(j), rows then slots
            for k in range(ptr[j], ptr[j + 1]):
                y[node[k]] = y[node[k]] + float(val[k]) * float(x[j])
        return np.array([0.0 + v for v in y])

    def _sweep(self, l, b, x):
        q = self._matvec(self.lev[l], x)
        d = self.idiag[l]
        out = np.empty(len(x))
        with np.errstate(all="ignore"):
            for i in range(len(x)):
                t = np.float64(b[i]) - np.float64(q[i])
                out[i] = np.float64(x[i]) + np.float64(self.omega) * (np.float64(d[i]) * t)
        return out

    def vcycle(self, l, b):
        d = self.idiag[l]
        with np.errstate(all="ignore"):
            x = np.array([np.float64(self.omega) * (np.float64(d[i]) * np.float64(b[i])) for i in range(len(b))])
        last = l == len(self.lev) - 1
        for _ in range((self.coarse if last else self.nu_pre) - 1):
            x = self._sweep(l, b, x)
        if last:
            return x
        q = self._matvec(self.lev[l], x)
        with np.errstate(all="ignore"):
            r = np.array([np.float64(b[i]) - np.float64(q[i]) for i in range(len(b))])
        xc = self.vcycle(l + 1, self._matvec_t(self.Ps[l], r))
        px = self._matvec(self.Ps[l], xc)
        with np.errstate(all="ignore"):
            x = np.array([np.float64(x[i]) + np.float64(px[i]) for i in range(len(x))])
        for _ in range(self.nu_post):
            x = self._sweep(l, b, x)
        return x

    def apply(self, r):
        return self.vcycle(0, np.asarray(r, np.float64))


# ------------------------------------------------------------------------------------ vectorised over slots
class _Rows:
    """a CSR matrix ready for slot-by-slot row sums"""

    def __init__(self, M):
        self.n, self.m, ptr, self.node, self.val = _csr0(M)
        self.ptr = ptr
        self.deg = np.diff(ptr)
        self.maxd = int(self.deg.max()) if self.n else 0
        # rows that own a slot s, for every s (rows sorted: deg > s)
        self.rows = [np.nonzero(self.deg > s)[0] for s in range(self.maxd)]

    def matvec(self, x):
        z = np.zeros(self.n)                           # +0.0
        with np.errstate(all="ignore"):
            for s, rows in enumerate(self.rows):
                e = self.ptr[rows] + s
                z[rows] = z[rows] + self.val[e] * x[self.node[e]]
            return 0.0 + z

    def idiag(self):
        z = np.zeros(self.n)
        for s, rows in enumerate(self.rows):
            e = self.ptr[rows] + s
            hit = self.node[e] == rows
            z[rows[hit]] = self.val[e[hit]]            # later slots overwrite: the last stored copy
        with np.errstate(all="ignore"):
            return 1.0 / z


def transpose(M):
    """M^T with every row's entries in (source row, slot) order: the order the reference's scatter adds them in"""
    n, m, ptr, node, val = _csr0(M)
    row = np.repeat(np.arange(n), np.diff(ptr))
    order = np.argsort(node, kind="stable")
    tptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=m))])
    return m, n, (tptr + 1).astype(np.int32), (row[order] + 1).astype(np.int32), val[order]


class Vectorised:
    def __init__(self, A, Ps, omega, nu_pre, nu_post, coarse_sweeps, lev=None):
        self.lev = lev if lev is not None else levels(A, Ps)
        self.omega, self.nu_pre, self.nu_post, self.coarse = float(omega), int(nu_pre), int(nu_post), int(coarse_sweeps)
        self.A = [_Rows(M) for M in self.lev]
        self.P = [_Rows(P) for P in Ps]
        self.PT = [_Rows(transpose(P)) for P in Ps]
        self.idiag = [a.idiag() for a in self.A]

    def _sweep(self, l, b, x):
        q = self.A[l].matvec(x)
        with np.errstate(all="ignore"):
            t = b - q
            return x + self.omega * (self.idiag[l] * t)

    def vcycle(self, l, b):
        with np.errstate(all="ignore"):
            x = self.omega * (self.idiag[l] * b)
        last = l == len(self.A) - 1
        for _ in range((self.coarse if last else self.nu_pre) - 1):
            x = self._sweep(l, b, x)
        if last:
            return x
        with np.errstate(all="ignore"):
            r = b - self.A[l].matvec(x)
            xc = self.vcycle(l + 1, self.PT[l].matvec(r))
            x = x + self.P[l].matvec(xc)
        for _ in range(self.nu_post):
            x = self._sweep(l, b, x)
        return x

    def apply(self, r):
        return self.vcycle(0, np.asarray(r, np.float64))


# ------------------------------------------------------------------------------------ Krylov on top
def pcg(A, b, apply_pc=None, tol=1e-10, max_iter=100000, dot=np.dot):
    """cg_solve / cg_solve_pc (cg_solvers.f90:124-190) from x = 0; returns (x, iterations, res2).  apply_pc(r) = M^-1 r, or
    None for plain CG.  The stop test is sqrt(r.z) <= tol (sqrt(r.r) without a preconditioner)."""
    A = A if isinstance(A, _Rows) else _Rows(A)
    b = np.asarray(b, np.float64)
    x = np.zeros(len(b))
    r = b - A.matvec(x)
    z = apply_pc(r) if apply_pc else r
    p = z.copy()
    res2 = dot(r, z)
    it = 0
    while np.sqrt(res2) > tol and it < max_iter:
        q = A.matvec(p)
        alpha = res2 / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        z = apply_pc(r) if apply_pc else r
        dpr = dot(r, z)
        p = z + (dpr / res2) * p
        res2 = dpr
        it += 1
    return x, it, res2


# ------------------------------------------------------------------------------------ the test problems
def poisson_case(nx, ny, min_edge=5):
    """(A, [P_0 ...]) of the nx x ny Poisson matrix and its interp2d hierarchy"""
    from sigma_amd import problems as Pr
    ptr, node, val = Pr.poisson2d_csr(nx, ny)
    n = nx * ny
    Ps = [(nf, nc, p, nd, v) for p, nd, v, nf, nc in Pr.interp2d_hierarchy(nx, ny, min_edge)]
    return (n, n, ptr, node, val), Ps


def edges_to_csr(n, ei, ej, ev):
    """CSR arrays of an edge list in insertion order per row (no duplicates in the generators used here)"""
    order = np.argsort(ei, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ei - 1, minlength=n))]) + 1
    return n, n, ptr.astype(np.int32), ej[order].astype(np.int32), np.asarray(ev, np.float64)[order]


def piecewise_constant(n, width=4):
    """P(i, i // width) = 1: n x ceil(n / width)"""
    nc = (n + width - 1) // width
    return n, nc, np.arange(1, n + 2, dtype=np.int32), (np.arange(n) // width + 1).astype(np.int32), np.ones(n)


def random_spd_case(n=300, seed=1):
    """random_spd_edges(n) with the piecewise-constant P taken twice (300 -> 75 -> 19)"""
    from sigma_amd import problems as Pr
    ei, ej, ev = Pr.random_spd_edges(n, seed=seed)
    A = edges_to_csr(n, ei, ej, ev)
    P0 = piecewise_constant(n)
    P1 = piecewise_constant(P0[1])
    return A, [P0, P1]


def stencil27_case(nx, ny, nz):
    """a 27-point matrix (27 on the diagonal, -1 to every neighbour of the 3 x 3 x 3 box, offsets in ascending order) with the
    piecewise-constant P: rows of up to 27 entries on the fine level"""
    n = nx * ny * nz
    k = np.arange(n)
    i, j, l = k % nx, (k // nx) % ny, k // (nx * ny)
    cols, vals, keep = [], [], []
    for dl in (-1, 0, 1):
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                ok = (i + di >= 0) & (i + di < nx) & (j + dj >= 0) & (j + dj < ny) & (l + dl >= 0) & (l + dl < nz)
                cols.append(k + di + dj * nx + dl * nx * ny)
                vals.append(np.full(n, 27.0 if (di, dj, dl) == (0, 0, 0) else -1.0))
                keep.append(ok)
    cols, vals, keep = np.stack(cols, 1), np.stack(vals, 1), np.stack(keep, 1)
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]) + 1
    A = (n, n, ptr.astype(np.int32), (cols[keep] + 1).astype(np.int32), vals[keep])
    return A, [piecewise_constant(n)]
