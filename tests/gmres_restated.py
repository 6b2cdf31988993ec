"""GMRES(m) restated in extended precision, for the tests (numpy only).

In exact arithmetic the residual of GMRES after k steps of a cycle is unique,

    |r_k| = min_y | r_0 - (M^-1 A) K_k y |,     K_k = [r_0, (M^-1 A) r_0, ..., (M^-1 A)^(k-1) r_0],

whatever orthogonalisation builds the basis.  So this file imitates none of the device's: Arnoldi with every new vector
orthogonalised TWICE against all earlier ones, the small least-squares problem by Givens rotations, everything in
np.longdouble (the 80-bit format on x86: eps 1.08e-19, 2^11 below double's).  What it returns is the optimal residual to
about n * 1e-19 -- a reference that is right to many more digits than any double-precision GMRES it is compared with.

Matrices are the stored (ptr, node, val) arrays with 1-based ptr / node.  `csr_op` turns them into the callable `op`;
a row's sum runs over its slots in stored order, slot s of every row that has one at once (the row loop, vectorised)."""
import numpy as np

LD = np.longdouble
EPS_LD = np.finfo(LD).eps
EPS_D = np.finfo(np.float64).eps


def _norm(v):
    return np.sqrt(np.dot(v, v))


def csr_op(ptr, node, val):
    """x -> A x in longdouble"""
    ptr = np.asarray(ptr, np.int64) - 1
    node = np.asarray(node, np.int64) - 1
    val = np.asarray(val, LD)
    n = len(ptr) - 1
    deg = np.diff(ptr)
    rows = [np.nonzero(deg > s)[0] for s in range(int(deg.max()) if n else 0)]

    def op(x):
        x = np.asarray(x, LD)
        y = np.zeros(n, LD)
        for s, rs in enumerate(rows):
            e = ptr[rs] + s
            y[rs] = y[rs] + val[e] * x[node[e]]
        return y
    return op


def inf_norm(ptr, node, val):
    """max row sum of |a_ij|"""
    ptr = np.asarray(ptr, np.int64) - 1
    a = np.abs(np.asarray(val, LD))
    return max([a[ptr[i]:ptr[i + 1]].sum() for i in range(len(ptr) - 1)] + [LD(0)])


def precondition(op, apply_pc):
    """v -> M^-1 (A v)"""
    if apply_pc is None:
        return op
    return lambda v: np.asarray(apply_pc(op(v)), LD)


class _Cycle:
    """one cycle from r0: V (orthonormal rows), the rotated H, g, the residual after every step"""

    def __init__(self, op, r0, m, steps, tol=None):
        r0 = np.asarray(r0, LD)
        n = len(r0)
        self.beta = _norm(r0)
        self.res = []
        self.closed = None              # the step (1-based) at which the Krylov space closed
        self.singular = False           # ... and closed without reaching the right-hand side: (M^-1 A) is singular on it
        self.k = 0                      # columns that enter the update of x
        steps = min(int(m), int(steps))
        if steps <= 0 or not self.beta > 0:
            return
        V = np.zeros((steps + 1, n), LD)
        H = np.zeros((steps + 1, steps), LD)
        cs, sn, g = np.zeros(steps, LD), np.zeros(steps, LD), np.zeros(steps + 1, LD)
        V[0] = r0 / self.beta
        g[0] = self.beta
        for j in range(steps):
            w = op(V[j])
            wn = _norm(w)
            h = np.zeros(j + 1, LD)
            for _ in range(2):
                c = V[:j + 1] @ w
                w = w - c @ V[:j + 1]
                h = h + c
            hn = _norm(w)
            closed = not hn > n * EPS_LD * wn
            if closed:
                hn = LD(0)
                self.closed = j + 1
            else:
                V[j + 1] = w / hn
            H[:j + 1, j] = h
            H[j + 1, j] = hn
            for i in range(j):
                h0, h1 = H[i, j], H[i + 1, j]
                H[i, j] = cs[i] * h0 + sn[i] * h1
                H[i + 1, j] = -sn[i] * h0 + cs[i] * h1
            d = np.sqrt(H[j, j] * H[j, j] + H[j + 1, j] * H[j + 1, j])
            if not d > 0:               # A v_j lies in span(v_0 .. v_{j-1}) with nothing left over: no step to take
                self.singular = True
                self.res.append(abs(g[j]))
                break
            cs[j], sn[j] = H[j, j] / d, H[j + 1, j] / d
            H[j, j], H[j + 1, j] = d, LD(0)
            g[j + 1] = -sn[j] * g[j]
            g[j] = cs[j] * g[j]
            self.k = j + 1
            self.res.append(abs(g[j + 1]))
            if closed or (tol is not None and not self.res[-1] > tol):
                break
        self.V, self.H, self.g = V, H, g

    def update(self, x):
        k = self.k
        if k == 0:
            return x
        y = np.zeros(k, LD)
        for i in range(k - 1, -1, -1):
            y[i] = (self.g[i] - np.dot(self.H[i, i + 1:k], y[i + 1:k])) / self.H[i, i]
        return x + y @ self.V[:k]


def optimal_history(op, r0, m, steps):
    """(residual norms after steps 1, 2, ... of ONE cycle from r0, the step at which the Krylov space closed or None).
    The new vector of a step counts as zero when its norm is <= n * eps_longdouble * |op(v)|; the history ends there."""
    c = _Cycle(op, r0, m, steps)
    return np.array(c.res, LD), c.closed


def restarted(op, apply_pc, b, x0, m, tol, max_iter, full=False):
    """GMRES(m) on M^-1 A x = M^-1 b (left preconditioning; apply_pc None = none) from x0, at most max_iter steps,
    stopping when the residual estimate is not above tol: (x, the residual after every step across restarts, the number of
    steps).  full=True adds the list of (first step, starting norm) of every cycle."""
    b = np.asarray(b, LD)
    x = np.asarray(x0, LD).copy()
    pop = precondition(op, apply_pc)
    res, cycles, it = [], [], 0
    while True:
        r = b - op(x)
        if apply_pc is not None:
            r = np.asarray(apply_pc(r), LD)
        beta = _norm(r)
        if not beta > tol or it >= max_iter:
            break
        c = _Cycle(pop, r, m, max_iter - it, tol)
        cycles.append((it, beta))
        res += c.res
        it += len(c.res)
        x = c.update(x)
        if c.singular or c.closed is not None or not c.res[-1] > tol:
            break
    res = np.array(res, LD)
    return (x, res, it, cycles) if full else (x, res, it)


def true_residual(A, x, b, apply_pc=None):
    """| M^-1 (b - A x) |_2 in longdouble; A = (ptr, node, val) or a callable"""
    op = A if callable(A) else csr_op(*A)
    r = np.asarray(b, LD) - op(np.asarray(x, LD))
    if apply_pc is not None:
        r = np.asarray(apply_pc(r), LD)
    return _norm(r)
