"""The contract of MINRES (sgm_minres_create), restated for the tests: once in float64 with the dot
product as a parameter, once in np.longdouble.

Preconditioned MINRES (Paige-Saunders) for symmetric A and a symmetric positive definite M.  Every operation is rounded on its
own; `A u` is +0.0 plus the individually rounded products of a row in stored order (mg_restated._Rows); `a.b` is `dot`;
`M^-1 u` is `apply_pc(u)`, or u itself without a preconditioner.

    r1 = b - A x ; y = M^-1 r1 ; beta1 = sqrt(r1.y)
    beta1 == 0: return (0 iterations, res2 = 0, converged)
    oldb = 0 ; beta = beta1 ; dbar = 0 ; epsln = 0 ; phibar = beta1 ; cs = -1 ; sn = 0 ; w = w2 = 0 ; r2 = r1
    while fabs(phibar) > tolerance and iterations < max_iter, k = 1, 2, ...:
        s = 1.0/beta ; v = s*y
        y = A v
        k >= 2:  t = beta/oldb ; y = y - t*r1
        alfa = v.y
        t = alfa/beta ; y = y - t*r2
        r1 = r2 ; r2 = y ; y = M^-1 r2
        oldb = beta ; bb = r2.y ; beta = sqrt(bb)
        oldeps = epsln ; delta = cs*dbar + sn*alfa ; gbar = sn*dbar - cs*alfa ; epsln = sn*beta ; dbar = -(cs*beta)
        gamma = sqrt(gbar*gbar + beta*beta) ; gi = 1.0/gamma ; cs = gbar*gi ; sn = beta*gi
        phi = cs*phibar ; phibar = sn*phibar
        w1 = w2 ; w2 = w ; w = ((v - oldeps*w1) - delta*w2) * gi ; x = x + phi*w
        iterations += 1 ; history gets fabs(phibar)
    res2 = phibar*phibar

Ends that are not convergence: bb < 0 or bb not a number (at the start or in a step), gamma == 0, gamma or phibar not a
number.  The solve stops at that step: the step is not counted, x keeps the value it had before it, converged = False; res2 is
NaN, or the last phibar*phibar for gamma == 0."""
import functools
from types import SimpleNamespace

import numpy as np

import mg_restated as MR

EPS = float(np.finfo(np.float64).eps)
TOL = 1e-10


def seq_dot(a, b):
    """ONE accumulator fed first element to last (option dot_order = 1)"""
    return np.cumsum(a * b)[-1] if len(a) else np.float64(0.0)


def tree_dot(a, b):
    """The solver's default ("tree") order for vectors of up to 1024 entries, which one workgroup of 256 threads sums: thread t
    adds the products of elements 2i, 2i+1 for i = t, t + 256, ... to its own accumulator (thread 0 then the last element of
    an odd length); each wave of 64 threads sums its accumulators by the butterfly v += v[lane ^ 32], ^ 16, ... ^ 1; the four
    wave sums are added left to right."""
    n = len(a)
    assert n <= 1024
    p = a * b
    acc = np.zeros(256)
    n2 = n // 2
    for r0 in range(0, n2, 256):
        i = np.arange(r0, min(r0 + 256, n2))
        acc[:len(i)] = acc[:len(i)] + p[2 * i]
        acc[:len(i)] = acc[:len(i)] + p[2 * i + 1]
    if n & 1:
        acc[0] = acc[0] + p[n - 1]
    w = acc.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    s = w[0, 0]
    for k in range(1, 4):
        s = s + w[k, 0]
    return s


DOTS = {"seq": seq_dot, "tree": tree_dot, "numpy": np.dot}


def rows_matvec(R, x, val=None):
    """mg_restated._Rows.matvec in the precision of x (val: R's values in that precision)"""
    if x.dtype == np.float64:
        return R.matvec(x)
    z = np.zeros(R.n, x.dtype)
    with np.errstate(all="ignore"):
        for s, rows in enumerate(R.rows):
            e = R.ptr[rows] + s
            z[rows] = z[rows] + val[e] * x[R.node[e]]
    return z


def minres(R, b, x0, apply_pc=None, tol=TOL, max_iter=0, dot=np.dot, dtype=np.float64):
    """The loop above on the rows R (mg_restated._Rows), in `dtype`.  Returns a namespace: x, it, res2, history (of
    fabs(phibar)), converged, failed ("" / "bb" / "gamma" / "nan")."""
    ft = dtype
    val = R.val.astype(ft)
    A = lambda u: rows_matvec(R, u, val)
    M = (lambda u: apply_pc(u)) if apply_pc is not None else (lambda u: u)
    one, nan = ft(1.0), ft(np.nan)
    x = np.array(x0, ft)
    b = np.asarray(b, ft)
    tol = ft(tol)
    hist = []

    def out(it, res2, conv, failed=""):
        return SimpleNamespace(x=x, it=it, res2=res2, history=np.array(hist, ft), converged=bool(conv), failed=failed)

    with np.errstate(all="ignore"):
        r1 = b - A(x)
        y = M(r1)
        bb = ft(dot(r1, y))
        if bb < 0 or bb != bb:
            return out(0, nan, False, "bb")
        beta1 = np.sqrt(bb)
        if beta1 == 0:
            return out(0, ft(0.0), True)
        oldb, beta, dbar, epsln, phibar, cs, sn = ft(0.0), beta1, ft(0.0), ft(0.0), beta1, ft(-1.0), ft(0.0)
        w = np.zeros(len(b), ft)
        w2 = np.zeros(len(b), ft)
        r2 = r1
        it = 0
        while np.abs(phibar) > tol and (max_iter <= 0 or it < max_iter):
            s = one / beta
            v = s * y
            y = A(v)
            if it >= 1:
                t = beta / oldb
                y = y - t * r1
            alfa = ft(dot(v, y))
            t = alfa / beta
            y = y - t * r2
            r1, r2 = r2, y
            y = M(r2)
            bb = ft(dot(r2, y))
            if bb < 0 or bb != bb:
                return out(it, nan, False, "bb")
            oldb, beta = beta, np.sqrt(bb)
            oldeps = epsln
            delta = cs * dbar + sn * alfa
            gbar = sn * dbar - cs * alfa
            gamma = np.sqrt(gbar * gbar + beta * beta)
            if gamma == 0:
                return out(it, phibar * phibar, False, "gamma")
            gi = one / gamma
            epsln = sn * beta
            dbar = -(cs * beta)
            cs = gbar * gi
            sn = beta * gi
            phi = cs * phibar
            newphibar = sn * phibar
            if gamma != gamma or newphibar != newphibar:
                return out(it, nan, False, "nan")
            phibar = newphibar
            w1, w2 = w2, w
            w = ((v - oldeps * w1) - delta * w2) * gi
            x = x + phi * w
            it += 1
            hist.append(np.abs(phibar))
        return out(it, phibar * phibar, not (np.abs(phibar) > tol))


# ------------------------------------------------------------------------------------ the cases
def _shifted(nx, ny, shift=0.3):
    from sigma_amd import problems as Pr
    ptr, node, val = Pr.poisson2d_csr(nx, ny)
    val = val.copy()
    row = np.repeat(np.arange(1, nx * ny + 1), np.diff(ptr))
    val[node == row] -= shift
    return nx * ny, ptr, node, val


def saddle_blocks():
    """K = poisson2d_csr(16, 16) + I (256 x 256), B (64 x 256) with B(i, 4i+1) = 1 and B(i, 4i+2) = -1 (0-based), its
    transpose, and -0.01 I (64 x 64): each as (nrow, ncol, ptr, node, val), 1-based"""
    n, ptr, node, val = _shifted(16, 16, -1.0)
    K = (n, n, ptr, node, val)
    m = 64
    i = np.arange(m)
    B = (m, n, (1 + 2 * np.arange(m + 1)).astype(np.int32), np.stack([4 * i + 2, 4 * i + 3], 1).ravel().astype(np.int32),
         np.tile([1.0, -1.0], m))
    cnt = np.zeros(n, np.int64)
    cnt[4 * i + 1] = 1
    cnt[4 * i + 2] = 1
    tptr = np.concatenate([[0], np.cumsum(cnt)]) + 1
    tnode = np.empty(2 * m, np.int32)
    tval = np.empty(2 * m)
    tnode[0::2], tnode[1::2] = i + 1, i + 1            # rows 4i+1 and 4i+2 follow each other
    tval[0::2], tval[1::2] = 1.0, -1.0
    Bt = (n, m, tptr.astype(np.int32), tnode, tval)
    Cm = (m, m, np.arange(1, m + 2, dtype=np.int32), np.arange(1, m + 1, dtype=np.int32), np.full(m, -0.01))
    return K, Bt, B, Cm


def _saddle():
    """[K B^T; B -0.01 I] as one CSR matrix: every row holds its left block's entries, then its right block's"""
    K, Bt, B, Cm = saddle_blocks()
    nk, m = K[0], B[0]
    ptr, node, val = [1], [], []
    for top, (L, Rb, off) in enumerate([(K, Bt, nk), (B, Cm, nk)]):
        for i in range(L[0]):
            for blk, shift in ((L, 0), (Rb, off)):
                lo, hi = blk[2][i] - 1, blk[2][i + 1] - 1
                node.extend((blk[3][lo:hi] + shift).tolist())
                val.extend(blk[4][lo:hi].tolist())
            ptr.append(len(node) + 1)
    return nk + m, np.array(ptr, np.int32), np.array(node, np.int32), np.array(val, np.float64)


def ell_arrays(n, ptr, node, val):
    """the ELLPACK arrays (n x max_d) of a CSR matrix: padding = last neighbour / 0.0"""
    deg = np.diff(ptr)
    md = int(deg.max())
    en = np.zeros((n, md), np.int32)
    ev = np.zeros((n, md))
    for i in range(n):
        cols = node[ptr[i] - 1:ptr[i + 1] - 1]
        en[i, :len(cols)] = cols
        en[i, len(cols):] = cols[-1]
        ev[i, :len(cols)] = val[ptr[i] - 1:ptr[i + 1] - 1]
    return en, ev


# name -> (matrix, storage on the device, preconditioners)
CASES = {
    "shifted24": ("shifted24", "csr", ("none", "jacobi")),
    "shifted23x17_ell": ("shifted23x17", "ell", ("none",)),
    "saddle": ("saddle", "csr", ("none",)),
    "saddle_composite": ("saddle", "composite", ("none",)),
    "poisson33x29_mg": ("poisson33x29", "csr", ("mg",)),
    "n1": ("n1", "csr", ("none",)),
    "n2": ("n2", "csr", ("none",)),
    "zero_rhs": ("shifted24", "csr", ("none",)),
    "guess": ("shifted24", "csr", ("none",)),
}
PAIRS = [(name, pc) for name, (_, _, pcs) in CASES.items() for pc in pcs]


@functools.lru_cache(maxsize=None)
def _matrix(key):
    if key == "shifted24":
        return _shifted(24, 24)
    if key == "shifted23x17":
        return _shifted(23, 17)
    if key == "saddle":
        return _saddle()
    if key == "poisson33x29":
        A, _ = MR.poisson_case(33, 29)
        return A[0], A[2], A[3], A[4]
    if key == "n1":
        return 1, np.array([1, 2], np.int32), np.array([1], np.int32), np.array([-2.0])
    if key == "n2":             # [[1, 2], [2, -1]]: eigenvalues +-sqrt(5)
        return 2, np.array([1, 3, 5], np.int32), np.array([1, 2, 1, 2], np.int32), np.array([1.0, 2.0, 2.0, -1.0])
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def case(name):
    """n, ptr, node, val (1-based CSR), fmt, b, x0, tol, max_iter, rows (mg_restated._Rows), dense"""
    key, fmt, pcs = CASES[name]
    n, ptr, node, val = _matrix(key)
    i = np.arange(1, n + 1)
    b = np.zeros(n) if name == "zero_rhs" else np.sin(0.001 * i)
    x0 = np.cos(0.002 * i) if name == "guess" else np.zeros(n)
    rows = MR._Rows((n, n, ptr, node, val))
    dense = np.zeros((n, n))
    r0 = np.repeat(np.arange(n), np.diff(ptr))
    np.add.at(dense, (r0, node - 1), val)
    for a in (b, x0, val, dense):
        a.setflags(write=False)
    return SimpleNamespace(name=name, n=n, ptr=ptr, node=node, val=val, fmt=fmt, pcs=pcs, b=b, x0=x0, tol=TOL, max_iter=4 * n,
                           rows=rows, dense=dense)


@functools.lru_cache(maxsize=None)
def mg_hierarchy():
    """(A, Ps) of the 33 x 29 Poisson matrix and its interp2d hierarchy"""
    return MR.poisson_case(33, 29)


@functools.lru_cache(maxsize=None)
def preconditioner(name, pc):
    """apply_pc of the float64 restatement (None without one)"""
    c = case(name)
    if pc == "none":
        return None
    if pc == "jacobi":
        idiag = c.rows.idiag()
        return lambda u: idiag * u
    A, Ps = mg_hierarchy()
    return MR.Vectorised(A, Ps, 0.8, 1, 1, 8).apply


def preconditioner_ld(name, pc):
    """M^-1 for the longdouble restatement and the true residual: Jacobi in longdouble; the V-cycle is the float64 one (the
    only statement of it there is) on the rounded vector"""
    c = case(name)
    if pc == "none":
        return None
    if pc == "jacobi":
        idiag = c.rows.idiag()
        idl = np.longdouble(1.0) / (np.longdouble(1.0) / idiag.astype(np.longdouble))
        return lambda u: idl * u
    f = preconditioner(name, pc)
    return lambda u: f(np.asarray(u, np.float64)).astype(np.longdouble)


@functools.lru_cache(maxsize=None)
def restated(name, pc, dot="seq"):
    """the float64 restatement of a case with the sequential dot (what dot_order = 1 is held to), the default tree order, or
    numpy's dot"""
    c = case(name)
    r = minres(c.rows, c.b, c.x0, preconditioner(name, pc), c.tol, c.max_iter, DOTS[dot])
    r.x.setflags(write=False)
    r.history.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated_ld(name, pc):
    c = case(name)
    r = minres(c.rows, c.b, c.x0, preconditioner_ld(name, pc), c.tol, c.max_iter, np.dot, np.longdouble)
    r.x.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def dense_solution(name):
    c = case(name)
    x = np.linalg.solve(c.dense, c.b)
    x.setflags(write=False)
    return x, float(np.linalg.cond(c.dense))


def x_error(name, x):
    """|x - x_dense|_inf / |x_dense|_inf (|x|_inf where x_dense = 0)"""
    xd, _ = dense_solution(name)
    d = float(np.max(np.abs(np.asarray(x, np.longdouble) - xd)))
    s = float(np.max(np.abs(xd)))
    return d / s if s > 0 else d


def x_bar(name, pc):
    """8 x the same error of the longdouble restatement, with a floor of 64 eps cond(A)"""
    _, cond = dense_solution(name)
    return max(8 * x_error(name, restated_ld(name, pc).x), 64 * EPS * cond)


def true_residual(name, pc, x):
    """sqrt((b - A x).M^-1 (b - A x)) in longdouble"""
    c = case(name)
    xl = np.asarray(x, np.longdouble)
    r = c.b.astype(np.longdouble) - rows_matvec(c.rows, xl, c.val.astype(np.longdouble))
    M = preconditioner_ld(name, pc)
    return float(np.sqrt(np.dot(r, M(r) if M else r)))


def residual_bar(name, pc, x):
    """tol + c eps (|A|_inf |x|_2 + |b|_2), c = 8 x what the float64 restatement's own x needs (0 where it needs none)"""
    c = case(name)
    scale = EPS * (float(np.abs(c.dense).sum(axis=1).max()) * float(np.linalg.norm(x)) + float(np.linalg.norm(c.b)))
    xr = restated(name, pc).x
    scale_r = EPS * (float(np.abs(c.dense).sum(axis=1).max()) * float(np.linalg.norm(xr)) + float(np.linalg.norm(c.b)))
    need = max(0.0, (true_residual(name, pc, xr) - c.tol) / scale_r) if scale_r > 0 else 0.0
    return c.tol + 8 * need * scale, need


def count_ok(it, ref):
    """within +-2 of the restatement's count, or within 2 % where the count is above 100"""
    return abs(it - ref) <= max(2, 0.02 * ref)
