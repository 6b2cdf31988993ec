"""The contract of LSQR (sgm_lsqr_create), restated for the tests: once in float64 with the dot product as
a parameter, once in np.longdouble.

LSQR (Paige-Saunders) for min |A x - b|_2, A of m x n entries, optionally damped.  Every operation is rounded on its own; every
sqrt(a*a + b*b) is that expression; `A u` is +0.0 plus the individually rounded products of a row in stored order
(mg_restated._Rows); `A^T u` is the same row sum over mg_restated.transpose(A), whose rows hold A's entries by source row
ascending, then slot -- the order sgm_mat_matvec_t documents; `a.a` is `dot`.  Neither bidiagonalisation vector is normalised:

    u = b - A x ; beta = sqrt(u.u)                              beta == 0: return (0 iterations, stop 1)
    z = A^T u ; v = (1.0/beta)*z ; alpha = sqrt(v.v)            alpha == 0: return (0 iterations, stop 2)
    w = (1.0/alpha)*v ; phibar = beta ; rhobar = alpha ; Psi = 0 ; rnorm = beta ; arnorm = alpha*beta ; the two tests
    step k = 1, 2, ... while iterations < max_iter:
        y = A v ; u = (1.0/alpha)*y - (alpha/beta)*u ; beta' = sqrt(u.u)
        beta' != 0: z = A^T u ; v = (1.0/beta')*z - (beta'/alpha)*v ; alpha' = sqrt(v.v)        beta' == 0: alpha' = 0
        damp != 0:  rhobar1 = sqrt(rhobar*rhobar + damp*damp) ; c1 = rhobar/rhobar1 ; s1 = damp/rhobar1
                    psi = s1*phibar ; phibar = c1*phibar ; Psi = Psi + psi*psi                   otherwise rhobar1 = rhobar
        rho = sqrt(rhobar1*rhobar1 + beta'*beta') ; c = rhobar1/rho ; s = beta'/rho ; theta = s*alpha'
        rhobar = -(c*alpha') ; phi = c*phibar ; phibar = s*phibar
        rnorm = sqrt(phibar*phibar + Psi) (fabs(phibar) with damp == 0) ; arnorm = (fabs(phibar)*alpha')*fabs(c)
        x = x + (phi/rho)*w ; beta' != 0 and alpha' != 0: w = (1.0/alpha')*v - (theta/rho)*w
        iterations += 1 ; history gets rnorm
        stop 1 if beta' == 0 ; else stop 2 if alpha' == 0 ; else the two tests
    tests: stop 1 if not rnorm > tolerance ; else stop 2 if not arnorm > normal_tolerance
    res2 = rnorm*rnorm

stop 0 is the cap.  stop 3: u.u or v.v negative or not a number, rho or the new phibar not a number; that step stores nothing (x
keeps the last finished iterate, the step is not counted, res2 is NaN)."""
import functools
from types import SimpleNamespace

import numpy as np

import eigsh_restated as ER
import mg_restated as MR
import minres_restated as MN

EPS = MN.EPS
TOL = 1e-10

seq_dot = MN.seq_dot
count_ok = MN.count_ok


def tree_dot(a, b):
    """The solver's default order: minres_restated.tree_dot up to 1024 entries (one workgroup), and for longer vectors its
    extension to several workgroups whose sums one workgroup adds again (eigsh_restated.device_sums)."""
    return ER.device_sums(a * b) if len(a) > 1024 else MN.tree_dot(a, b)


DOTS = {"seq": seq_dot, "tree": tree_dot, "numpy": np.dot}


def lsqr(R, Rt, b, x0, tol=TOL, ntol=TOL, damp=0.0, max_iter=0, dot=np.dot, dtype=np.float64):
    """The loop above on the rows R of A and Rt of A^T (mg_restated._Rows), in `dtype`.  Returns a namespace: x, it, stop, res2,
    rnorm, arnorm, history (of rnorm), converged."""
    ft = dtype
    val, valt = R.val.astype(ft), Rt.val.astype(ft)
    A = lambda u: MN.rows_matvec(R, u, val)
    At = lambda u: MN.rows_matvec(Rt, u, valt)
    one, nan, zero = ft(1.0), ft(np.nan), ft(0.0)
    x = np.array(x0, ft)
    b = np.asarray(b, ft)
    tol, ntol, damp = ft(tol), ft(ntol), ft(damp)
    hist = []

    def out(it, stop, rnorm, arnorm):
        res2 = nan if stop == 3 else rnorm * rnorm
        return SimpleNamespace(x=x, it=it, stop=stop, res2=res2, rnorm=rnorm, arnorm=arnorm, history=np.array(hist, ft),
                               converged=stop in (1, 2))

    def tests(rnorm, arnorm):
        if not rnorm > tol:
            return 1
        if not arnorm > ntol:
            return 2
        return 0

    with np.errstate(all="ignore"):
        u = b - A(x)
        uu = ft(dot(u, u))
        if uu < 0 or uu != uu:
            return out(0, 3, nan, nan)
        beta = np.sqrt(uu)
        if beta == 0:
            return out(0, 1, beta, zero)
        v = (one / beta) * At(u)
        vv = ft(dot(v, v))
        if vv < 0 or vv != vv:
            return out(0, 3, nan, nan)
        alpha = np.sqrt(vv)
        rnorm, arnorm = beta, alpha * beta
        if alpha == 0:
            return out(0, 2, rnorm, arnorm)
        stop = tests(rnorm, arnorm)
        if stop:
            return out(0, stop, rnorm, arnorm)
        w = (one / alpha) * v
        phibar, rhobar, Psi = beta, alpha, zero
        it = 0
        while max_iter <= 0 or it < max_iter:
            y = A(v)
            u = (one / alpha) * y - (alpha / beta) * u
            uu = ft(dot(u, u))
            if uu < 0 or uu != uu:
                return out(it, 3, rnorm, arnorm)
            betan = np.sqrt(uu)
            alphan = zero
            if betan != 0:
                v = (one / betan) * At(u) - (betan / alpha) * v
                vv = ft(dot(v, v))
                if vv < 0 or vv != vv:
                    return out(it, 3, rnorm, arnorm)
                alphan = np.sqrt(vv)
            pb, ps = phibar, Psi
            rhobar1 = rhobar
            if damp != 0:
                rhobar1 = np.sqrt(rhobar * rhobar + damp * damp)
                c1, s1 = rhobar / rhobar1, damp / rhobar1
                psi = s1 * pb
                pb = c1 * pb
                ps = ps + psi * psi
            rho = np.sqrt(rhobar1 * rhobar1 + betan * betan)
            c, s = rhobar1 / rho, betan / rho
            theta = s * alphan
            phi = c * pb
            pbn = s * pb
            if rho != rho or pbn != pbn:
                return out(it, 3, rnorm, arnorm)
            rhobar, phibar, Psi = -(c * alphan), pbn, ps
            rnorm = np.sqrt(phibar * phibar + Psi) if damp != 0 else np.abs(phibar)
            arnorm = (np.abs(phibar) * alphan) * np.abs(c)
            x = x + (phi / rho) * w
            if betan != 0 and alphan != 0:
                w = (one / alphan) * v - (theta / rho) * w
            alpha, beta = alphan, betan
            it += 1
            hist.append(rnorm)
            stop = 1 if betan == 0 else 2 if alphan == 0 else tests(rnorm, arnorm)
            if stop:
                return out(it, stop, rnorm, arnorm)
        return out(it, 0, rnorm, arnorm)


# ------------------------------------------------------------------------------------ the matrices
def _fit():
    from sigma_amd import problems as Pr
    ptr, node, val, nc = Pr.interp2d_csr(23, 17)
    return 23 * 17, nc, np.asarray(ptr, np.int32), np.asarray(node, np.int32), np.asarray(val, np.float64)


def _incidence(nx, ny):
    """edge-by-node incidence matrix of the nx x ny grid graph: the edges to the right neighbour, row after row of the grid,
    then the edges to the upper neighbour; -1 at the lower-numbered node, +1 at the other"""
    k = np.arange(nx * ny).reshape(ny, nx)
    tail = np.concatenate([k[:, :-1].ravel(), k[:-1, :].ravel()])
    head = np.concatenate([k[:, 1:].ravel(), k[1:, :].ravel()])
    ne = len(tail)
    ptr = (1 + 2 * np.arange(ne + 1)).astype(np.int32)
    node = np.stack([tail + 1, head + 1], 1).ravel().astype(np.int32)
    return ne, nx * ny, ptr, node, np.tile([-1.0, 1.0], ne)


def _random(m, n, per_row=5, seed=11):
    """per_row distinct random columns per row with standard normal values, plus 4.0 on the leading diagonal (rows below n),
    stored first"""
    rs = np.random.RandomState(seed)
    ptr, node, val = [1], [], []
    for i in range(m):
        cols = rs.choice(n, per_row, replace=False)
        vals = rs.standard_normal(per_row)
        if i < n:
            keep = cols != i
            cols, vals = np.concatenate([[i], cols[keep]]), np.concatenate([[4.0], vals[keep]])
        node.extend((cols + 1).tolist())
        val.extend(vals.tolist())
        ptr.append(len(node) + 1)
    return m, n, np.array(ptr, np.int32), np.array(node, np.int32), np.array(val, np.float64)


@functools.lru_cache(maxsize=None)
def _matrix(key):
    """(m, n, ptr, node, val), 1-based"""
    if key == "fit23x17":
        return _fit()
    if key == "wide":
        return MR.transpose(_fit())
    if key == "incidence13x11":
        return _incidence(13, 11)
    if key == "random2051x1027":
        return _random(2051, 1027)
    raise KeyError(key)


# name -> (matrix, storage formats on the device, damp, the stop the solve ends with)
CASES = {
    "fit23x17": ("fit23x17", ("csr",), 0.0, 2),
    "fit23x17_consistent": ("fit23x17", ("csr",), 0.0, 1),
    "wide": ("wide", ("csr",), 0.0, 1),
    "damped": ("fit23x17", ("csr",), 0.5, 2),
    "guess": ("fit23x17", ("csr",), 0.0, 2),
    "incidence13x11": ("incidence13x11", ("csr", "ell"), 0.0, 2),
    "incidence13x11_consistent": ("incidence13x11", ("csr", "ell"), 0.0, 1),
    "random2051x1027": ("random2051x1027", ("csr", "ell"), 0.0, 2),
}
PAIRS = [(name, fmt) for name, (_, fmts, _, _) in CASES.items() for fmt in fmts]
CONSISTENT = ("fit23x17_consistent", "wide", "incidence13x11_consistent")


@functools.lru_cache(maxsize=None)
def _vectors():
    """b (and t with b = A t on the consistent cases, x0 on `guess`) of every case: drawn from RandomState(3) one after the
    other in the order of CASES"""
    rs = np.random.RandomState(3)
    out = {}
    for name, (key, _, _, _) in CASES.items():
        m, n = _matrix(key)[:2]
        if name in CONSISTENT:
            b = MR._Rows(_matrix(key)).matvec(rs.standard_normal(n))
        else:
            b = rs.standard_normal(m)
        x0 = rs.standard_normal(n) if name == "guess" else np.zeros(n)
        out[name] = (b, x0)
    return out


def ell_arrays(m, ptr, node, val):
    """the ELLPACK arrays (m x max_d) of a CSR matrix (padding: the last neighbour, 0.0) and the degrees"""
    en, ev = MN.ell_arrays(m, ptr, node, val)
    return en, ev, np.diff(ptr).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """m, n, ptr, node, val (1-based CSR), fmts, b, x0, tol, damp, stop, max_iter, rows / rows_t (mg_restated._Rows of A and
    A^T), dense.  (The ELLPACK form adds only padding products 0.0 * x(j) to sums that start at +0.0: the same bits.)"""
    key, fmts, damp, stop = CASES[name]
    M = _matrix(key)
    m, n, ptr, node, val = M
    b, x0 = _vectors()[name]
    dense = np.zeros((m, n))
    np.add.at(dense, (np.repeat(np.arange(m), np.diff(ptr)), node - 1), val)
    for a in (b, x0, val, dense):
        a.setflags(write=False)
    return SimpleNamespace(name=name, key=key, m=m, n=n, ptr=ptr, node=node, val=val, fmts=fmts, b=b, x0=x0, tol=TOL, damp=damp,
                           stop=stop, max_iter=4 * n, rows=MR._Rows(M), rows_t=MR._Rows(MR.transpose(M)), dense=dense)


def solve(c, dot="seq", dtype=np.float64, max_iter=None, damp=None, rows=None, rows_t=None, b=None, x0=None):
    return lsqr(rows or c.rows, rows_t or c.rows_t, c.b if b is None else b, c.x0 if x0 is None else x0, c.tol, c.tol,
                c.damp if damp is None else damp, c.max_iter if max_iter is None else max_iter,
                DOTS[dot] if isinstance(dot, str) else dot, dtype)


@functools.lru_cache(maxsize=None)
def restated(name, dot="seq"):
    """the float64 restatement of a case with the sequential dot (what dot_order = 1 is held to), the default tree order, or
    numpy's dot"""
    r = solve(case(name), dot)
    r.x.setflags(write=False)
    r.history.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated_ld(name):
    r = solve(case(name), np.dot, np.longdouble)
    r.x.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------ the truth and the bars
@functools.lru_cache(maxsize=None)
def dense_solution(name):
    """x0 + pinv(A) (b - A x0) from numpy's SVD; damped: x0 + V diag(s / (s^2 + damp^2)) U^T (b - A x0), the solution of the
    damped normal equations.  Also the null space of A (columns, orthonormal) and |A|_inf."""
    c = case(name)
    U, s, Vt = np.linalg.svd(c.dense, full_matrices=True)
    rank = int(np.sum(s > s[0] * max(c.m, c.n) * EPS))
    r0 = c.b - c.dense @ c.x0
    sr = s[:rank]
    x = c.x0 + Vt[:rank].T @ ((sr / (sr * sr + c.damp * c.damp)) * (U[:, :rank].T @ r0))
    null = Vt[rank:].T
    x.setflags(write=False)
    return SimpleNamespace(x=x, rank=rank, null=null, cond=float(s[0] / s[rank - 1]), norm_inf=float(np.abs(c.dense).sum(axis=1).max()))


def x_error(name, x):
    """|x - x*|_2 / |x*|_2"""
    xs = dense_solution(name).x
    return float(np.linalg.norm(np.asarray(x, np.longdouble) - xs) / np.linalg.norm(xs))


def x_bar(name):
    """max(8 x the longdouble restatement's error, 64 eps) (relative to |x*|_2)"""
    return max(8 * x_error(name, restated_ld(name).x), 64 * EPS)


def true_norms(name, x):
    """(|b - A x|_2, |A^T (b - A x) - damp^2 (x - x0)|_2) in longdouble"""
    c = case(name)
    xl = np.asarray(x, np.longdouble)
    r = c.b.astype(np.longdouble) - MN.rows_matvec(c.rows, xl, c.val.astype(np.longdouble))
    g = MN.rows_matvec(c.rows_t, r, c.rows_t.val.astype(np.longdouble)) - np.longdouble(c.damp) ** 2 * (xl - c.x0)
    return float(np.sqrt(np.dot(r, r))), float(np.sqrt(np.dot(g, g)))


def _scales(name, x):
    c, d = case(name), dense_solution(name)
    s = EPS * (d.norm_inf * float(np.linalg.norm(x)) + float(np.linalg.norm(c.b)))
    return s, s * d.norm_inf


def bars(name, x):
    """(residual bar, normal-equations bar, c_r, c_n): tol + c eps (|A|_inf |x|_2 + |b|_2) [|A|_inf], c = 8 x what the float64
    restatement's own x needs (0 where it needs none); the estimates rnorm / arnorm the solve stops on are recurrences, the true
    norms differ from them by rounding of this size"""
    c = case(name)
    xr = restated(name).x
    rr, nr = true_norms(name, xr)
    sr, sn = _scales(name, xr)
    need_r = max(0.0, (rr - c.tol) / sr) if name in CONSISTENT else 0.0
    need_n = max(0.0, (nr - c.tol) / sn)
    s, t = _scales(name, x)
    return c.tol + 8 * need_r * s, c.tol + 8 * need_n * t, need_r, need_n
