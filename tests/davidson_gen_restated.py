"""The contract of sgm_davidson_gen (include/sigma_hip.h), restated in numpy for the tests, statement by
statement, from the header and not from the kernels: in float64 with the dot product as a parameter, and in np.longdouble.

Every operation is rounded on its own; `A u` and `B u` are +0.0 plus the individually rounded products of a row in stored
order (mg_restated._Rows; davidson_restated.CompositeRows for the composite); `a.b` is eigsh_restated's (`device`: the order
the header defines, a function of n alone); rotations are eigsh_restated.rotate; `M^-1 u` is `apply_pc(u)`, a copy without a
preconditioner; keep = min(k + (ncv - k)//2, ncv - 1).

    p = B q1 ; d = q1.p ; not (d > 0): leave, found = 0
    t = 1.0/sqrt(d) ; V_0 = q1 * t ; U_0 = p * t ; W_0 = A V_0 ; H(0,0) = V_0.W_0
    m = 1 ; locked = 0 ; anorm = 0 ; steps = restarts = 0
    loop:
      a NaN in H[:m, :m]: leave, found = 0 ; (theta, Z) = symeig(H[:m, :m]) ; a NaN in theta: leave, found = 0
      anorm = max(anorm, max |theta_i|) ; order ascending, ties by index
      the residual of order[j] = c: y = W[:, :m] Z[:, c], p = U[:, :m] Z[:, c] (`rotate`) ; r = y - theta_c * p
                                    it meets the test when sqrt(r.r) <= (tol * anorm) * sqrt(p.p)
      while locked < min(k, m): the residual of order[locked] ; meets: locked += 1, else leave the while
      locked == k: for j = 0 .. (locked at the start of this pass) - 1: the residual of order[j] ; fails: locked = j, stop
      locked == k: leave, found = k, converged ; locked == m: leave, found = m ; steps == max_steps: leave, found = min(k, m)
      m == ncv: Zk = the first keep columns of Z in that order, each z divided by sqrt(((0.0 + z_0 z_0) + z_1 z_1) + ...) ;
                V[:, :keep] = V[:, :m] Zk ; W and U the same ; H = diag(theta of the kept) ; theta = those,
                Z = I, order = 0, 1, .. ; m = keep ; restarts += 1
      t = M^-1 r ; tau = sqrt(t.t)
      h_i = U_i.t ; t = (..(t - h_0 V_0) - ..) - h_{m-1} V_{m-1} ; g_i = U_i.t ; t = (..(t - g_0 V_0) - ..) ; nu = sqrt(t.t)
      a NaN in tau or nu: leave, found = 0 ; not (nu > 2^-40 * tau): leave, found = min(k, locked)
      p = B t ; d = t.p ; not (d > 0): leave, found = 0
      s = 1.0/sqrt(d) ; V_m = t * s ; U_m = p * s ; W_m = A V_m ; H(i,m) = H(m,i) = V_i.W_m, i = 0..m ; m += 1 ; steps += 1
    Vout = V[:, :m] Zf, Zf = the first found columns of Z, divided the same way ; lambda_i = theta_i
    resid_i = sqrt(r.r), r = A v_i - lambda_i * (B v_i)
    a step that ends at one of its tests counts none of its products ; products with A: W_0, one per step, one per returned
    pair ; with B: the first, one per step, one per returned pair ; applies: one per `t = M^-1 r` with a preconditioner.

Below the loop: the case registry of tests/test_davidson_gen_cpu.py and tests/test_gpu_davidson_gen.py -- the matrices (pure
data), q1, the interp2d_hierarchy prolongations of the tensor grids -- and the yardsticks that do not use the restatement."""
import functools
from types import SimpleNamespace

import numpy as np

import davidson_restated as DR
import edit_restated as ED
import eigsh_restated as ER
import mg_direct_restated as MD
import mg_restated as MR
import minres_restated as MN

EPS = ER.EPS
TINY = ER.TINY
TOL = 1e-8


def unit_columns(Zs):
    """every column z divided by sqrt(((0.0 + z_0 z_0) + z_1 z_1) + ...): the sum ascending, every operation rounded"""
    s = np.zeros(Zs.shape[1], Zs.dtype)
    for i in range(Zs.shape[0]):
        s = s + Zs[i] * Zs[i]
    return Zs / np.sqrt(s)


def davidson_gen(RA, RB, k, ncv, q1, apply_pc=None, tol=TOL, max_steps=1000, dot="device", dtype=np.float64):
    """The loop above on the rows RA, RB.  Returns a namespace: lam, V, residuals (the restatement's own sqrt(r.r) of the
    returned pairs), steps, products, products_B, applies, restarts, found, converged, anorm."""
    ft = dtype
    sums = ER.SUMS[dot]
    dot1 = lambda a, b: sums((a * b)[:, None])[0]
    vala, valb = RA.val.astype(ft), RB.val.astype(ft)
    n = RA.n
    assert RB.n == n and 1 <= k < ncv <= 64 and ncv < n and tol >= TINY and max_steps >= 0
    keep = min(k + (ncv - k) // 2, ncv - 1)
    one, tiny, zero = ft(1.0), ft(TINY), ft(0.0)
    q1 = np.asarray(q1, ft)
    V = np.zeros((n, ncv), ft)
    W = np.zeros((n, ncv), ft)
    U = np.zeros((n, ncv), ft)
    H = np.zeros((ncv, ncv), ft)
    st = SimpleNamespace(steps=0, products=0, products_B=0, applies=0, restarts=0)

    def A(u):
        st.products += 1
        return MN.rows_matvec(RA, u, vala)

    def B(u):
        st.products_B += 1
        return MN.rows_matvec(RB, u, valb)

    def out(found, converged, m, theta, Z, order, anorm):
        lam = np.full(k, np.nan, ft)
        resid = np.full(k, np.nan, ft)
        Vout = np.zeros((n, k), ft)
        if found > 0:
            sel = order[:found]
            Vout[:, :found] = ER.rotate(V[:, :m], unit_columns(Z[:, sel]))
            lam[:found] = theta[sel]
            for i in range(found):
                y = A(Vout[:, i])
                p = B(Vout[:, i])
                r = y - lam[i] * p
                resid[i] = np.sqrt(dot1(r, r))
        return SimpleNamespace(lam=lam, V=Vout, residuals=resid, steps=st.steps, products=st.products, products_B=st.products_B,
                               applies=st.applies, restarts=st.restarts, found=found, converged=bool(converged), anorm=anorm)

    with np.errstate(all="ignore"):
        p = B(q1)
        d = dot1(q1, p)
        if not (d > zero):
            return out(0, False, 0, None, None, None, zero)
        t = one / np.sqrt(d)
        V[:, 0] = q1 * t
        U[:, 0] = p * t
        W[:, 0] = A(V[:, 0])
        H[0, 0] = dot1(V[:, 0], W[:, 0])
        m, locked, anorm = 1, 0, zero
        theta = Z = order = None
        while True:
            if np.isnan(H[:m, :m]).any():
                return out(0, False, m, theta, Z, order, anorm)
            theta, Z, _ = ER.symeig(H[:m, :m], ft)
            if np.isnan(theta).any():
                return out(0, False, m, theta, Z, order, anorm)
            anorm = max(anorm, np.max(np.abs(theta)))
            order = np.argsort(theta, kind="stable")

            def residual(j):
                c = order[j]
                y = ER.rotate(W[:, :m], Z[:, c:c + 1])[:, 0]
                p = ER.rotate(U[:, :m], Z[:, c:c + 1])[:, 0]
                rj = y - theta[c] * p
                return rj, bool(np.sqrt(dot1(rj, rj)) <= (ft(tol) * anorm) * np.sqrt(dot1(p, p)))

            locked_before = locked
            while locked < min(k, m):
                r, meets = residual(locked)
                if meets:
                    locked += 1
                else:
                    break
            if locked == k:
                for j in range(locked_before):
                    r, meets = residual(j)
                    if not meets:
                        locked = j
                        break
            if locked == k:
                return out(k, True, m, theta, Z, order, anorm)
            if locked == m:
                return out(m, False, m, theta, Z, order, anorm)
            if st.steps == max_steps:
                return out(min(k, m), False, m, theta, Z, order, anorm)
            if m == ncv:
                kept = order[:keep]
                Zk = unit_columns(Z[:, kept])
                V[:, :keep] = ER.rotate(V[:, :m], Zk)
                W[:, :keep] = ER.rotate(W[:, :m], Zk)
                U[:, :keep] = ER.rotate(U[:, :m], Zk)
                theta = theta[kept].copy()
                H[:] = 0
                H[np.arange(keep), np.arange(keep)] = theta
                Z = np.eye(keep, dtype=ft)
                order = np.arange(keep)
                m = keep
                st.restarts += 1
            if apply_pc is not None:
                t = np.asarray(apply_pc(r), ft)
                st.applies += 1
            else:
                t = r.copy()
            tau = np.sqrt(dot1(t, t))
            h = sums(U[:, :m] * t[:, None])
            for i in range(m):
                t = t - h[i] * V[:, i]
            g = sums(U[:, :m] * t[:, None])
            for i in range(m):
                t = t - g[i] * V[:, i]
            nu = np.sqrt(dot1(t, t))
            if np.isnan(tau) or np.isnan(nu):
                return out(0, False, m, theta, Z, order, anorm)
            if not (nu > tiny * tau):
                return out(min(k, locked), False, m, theta, Z, order, anorm)
            p = B(t)
            d = dot1(t, p)
            if not (d > zero):
                st.products_B -= 1                      # a step that ends at one of its tests counts none of its products
                return out(0, False, m, theta, Z, order, anorm)
            s = one / np.sqrt(d)
            V[:, m] = t * s
            U[:, m] = p * s
            W[:, m] = A(V[:, m])
            col = sums(V[:, :m + 1] * W[:, m][:, None])
            H[:m + 1, m] = col
            H[m, :m + 1] = col
            m += 1
            st.steps += 1


# ------------------------------------------------------------------------------------ the matrices (pure data)
def kappa(n):
    """6 (1 - c_j) / (h^2 (2 + c_j)), c_j = cos(j pi h), h = 1/(n+1), j = 1 .. n, in longdouble: the eigenvalues of
    K1(n) x = kappa M1(n) x"""
    h = np.longdouble(1) / np.longdouble(n + 1)
    c = np.cos(np.arange(1, n + 1, dtype=np.longdouble) * ER._PI_LD * h)
    return np.longdouble(6) * (np.longdouble(1) - c) / (h * h * (np.longdouble(2) + c))


def fem_spectrum(nx, ny):
    """the generalized eigenvalues of fem<nx>x<ny>, ascending, in longdouble"""
    return np.sort((kappa(nx)[:, None] + kappa(ny)[None, :]).ravel())


def _csr_of_dense(D, mask):
    """1-based CSR (columns ascending) of the entries of D where mask is set"""
    n = D.shape[0]
    r, c = np.nonzero(mask)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]) + 1
    return n, n, ptr.astype(np.int32), (c + 1).astype(np.int32), np.ascontiguousarray(D[r, c])


def _diag_csr(d):
    n = len(d)
    return n, n, np.arange(1, n + 2, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), np.asarray(d, np.float64)


@functools.lru_cache(maxsize=None)
def _pair(key):
    """(A, B, Ps): A, B = (n, n, ptr, node, val), 1-based CSR; Ps: the hierarchy of A, or None"""
    from sigma_amd import problems as Pr
    if key.startswith("fem"):
        nx, ny = (int(s) for s in key[3:].split("x"))
        n = nx * ny
        (pa, na, va), (pb, nb, vb) = Pr.fem2d_pair_csr(nx, ny)
        Ps = [(nf, nc, p, nd, v) for p, nd, v, nf, nc in Pr.interp2d_hierarchy(nx, ny)]
        return (n, n, pa, na, va), (n, n, pb, nb, vb), Ps
    if key == "mesh19x17":
        # P1 elements on a jittered 19 x 17 node mesh (n = 323, odd), natural boundary: A = K + M, B = M, so that the constant
        # vector is the eigenvector of the smallest eigenvalue, exactly 1
        x, ele = ED.fem_grid(19, 17)
        n = x.shape[1]
        D = {}
        for kind in ("stiffness", "mass"):
            ti, tj, tv = ED.fem_triples(x, ele, kind)
            D[kind] = np.zeros((n, n))
            np.add.at(D[kind], (ti - 1, tj - 1), tv)
        mask = np.zeros((n, n), bool)
        mask[ti - 1, tj - 1] = True
        return _csr_of_dense(D["stiffness"] + D["mass"], mask), _csr_of_dense(D["mass"], mask), None
    if key == "comp32x24":            # the composite fixture of davidson_restated with the diagonal B = 1 + (i mod 7)/8
        A, _ = DR._matrix(key)
        return A, _diag_csr(1.0 + (np.arange(A[0]) % 7) / 8.0), None
    if key.startswith("poisson"):     # B = I held as a matrix
        A, Ps = DR._matrix(key)
        return A, _diag_csr(np.ones(A[0])), Ps
    raise KeyError(key)


def own_q1(n):
    return 1.5 + np.cos(0.37 * np.arange(n))


@functools.lru_cache(maxsize=None)
def case(key):
    """n, A, B (1-based CSR tuples), Ps, rowsA, rowsB, denseA (None above 2000 rows), denseB (None above 3000), q1, maxrow (the longest row of A
    or B), spectrum (the exact generalized eigenvalues, ascending, longdouble: analytic for fem, a dense solve otherwise, None
    above 2000 rows without a formula)"""
    A, B, Ps = _pair(key)
    n = A[0]
    rowsA = DR.CompositeRows(*DR.composite_fixture()) if key == "comp32x24" else MR._Rows(A)
    rowsB = MR._Rows(B)
    dA = DR._dense(n, *A[2:]) if n <= 2000 else None
    dB = DR._dense(n, *B[2:]) if n <= 3000 else None
    if key.startswith("fem"):
        spec = fem_spectrum(*(int(s) for s in key[3:].split("x")))
    elif dA is not None:
        L = np.linalg.cholesky(dB)
        Li = np.linalg.inv(L)
        spec = np.linalg.eigvalsh(Li @ dA @ Li.T).astype(np.longdouble)
    else:
        spec = None
    q1 = ER.start_vector(n)
    for a in (A[4], B[4], q1):
        a.setflags(write=False)
    return SimpleNamespace(name=key, n=n, A=A, B=B, Ps=Ps, rowsA=rowsA, rowsB=rowsB, denseA=dA, denseB=dB, q1=q1, spectrum=spec,
                           maxrow=int(max(np.diff(A[2]).max(), np.diff(B[2]).max())))


@functools.lru_cache(maxsize=None)
def preconditioner(key, pc):
    """apply_pc of the float64 restatement, the kinds and parameters of davidson_restated.preconditioner, built on this
    module's A: "none", "jacobi", "mg" (V(1,1), omega 0.8, 8 coarse sweeps), "mg22direct" (V(2,2), the coarsest level solved
    directly).  ILDU(0) has no restatement in numpy: the tests that need it pass the oracle's solve."""
    c = case(key)
    if pc == "none":
        return None
    if pc == "jacobi":
        idiag = c.rowsA.idiag()
        return lambda u: idiag * u
    if pc == "mg":
        return MR.Vectorised(c.A, c.Ps, 0.8, 1, 1, 8).apply
    if pc == "mg22direct":
        return MD.Vectorised(c.A, c.Ps, 0.8, 2, 2).apply
    raise KeyError(pc)


def preconditioner_ld(key, pc):
    """M^-1 for the longdouble restatement, as davidson_restated.preconditioner_ld: a V-cycle is the float64 one on the
    rounded vector"""
    if pc == "none":
        return None
    if pc == "jacobi":
        idl = np.longdouble(1.0) / (np.longdouble(1.0) / case(key).rowsA.idiag().astype(np.longdouble))
        return lambda u: idl * u
    f = preconditioner(key, pc)
    return lambda u: f(np.asarray(u, np.float64)).astype(np.longdouble)


def _freeze(r):
    for a in (r.lam, r.V, r.residuals):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated(key, pc, k, ncv, own=False, max_steps=1000):
    """the float64 run with the device's order of summation (own: from own_q1 instead of the default start vector)"""
    c = case(key)
    q1 = own_q1(c.n) if own else c.q1
    return _freeze(davidson_gen(c.rowsA, c.rowsB, k, ncv, q1, preconditioner(key, pc), TOL, max_steps))


@functools.lru_cache(maxsize=None)
def restated_ld(key, pc, k, ncv):
    c = case(key)
    return _freeze(davidson_gen(c.rowsA, c.rowsB, k, ncv, c.q1, preconditioner_ld(key, pc), TOL, 1000, "numpy", np.longdouble))


# ------------------------------------------------------------------------------------ yardsticks that do not use the restatement
def _ld_products(c, v):
    """A v, B v, |A||v|, |B||v| in longdouble from the case's own CSR arrays (the assembled A of the composite)"""
    RA = MR._Rows(c.A) if c.name == "comp32x24" else c.rowsA
    va, vb = c.A[4].astype(np.longdouble), c.B[4].astype(np.longdouble)
    return (MN.rows_matvec(RA, v, va), MN.rows_matvec(c.rowsB, v, vb), MN.rows_matvec(RA, np.abs(v), np.abs(va)),
            MN.rows_matvec(c.rowsB, np.abs(v), np.abs(vb)))


def true_residuals(c, lam, V):
    """eigsh_restated.true_residuals extended to two products: R_i = |A v_i - lam_i B v_i|_2 in longdouble, and the forward
    bound of the float64 evaluation of sqrt(r.r) -- every entry of A v and of B v carries gamma_d of its absolute row sum (d:
    the longest row), the product with lam and the subtraction two more roundings: the 2-norm of
    gamma_{d+2} (|A||v| + |lam| |B||v|) plus gamma_n R_i."""
    Rs, bounds = [], []
    for i in range(len(lam)):
        v = np.asarray(V[:, i], np.longdouble)
        li = np.longdouble(lam[i])
        av, bv, aa, bb = _ld_products(c, v)
        r = av - li * bv
        R = np.sqrt(np.dot(r, r))
        e = aa + np.abs(li) * bb
        Rs.append(float(R))
        bounds.append(float(ER.gamma(c.maxrow + 2) * np.sqrt(np.dot(e, e)) + ER.gamma(c.n) * R))
    return np.array(Rs), np.array(bounds)


def eigenvalue_bounds(c, lam, V):
    """|r_i|_{B^-1} / |v_i|_B with r_i = A v_i - lam_i B v_i recomputed in longdouble from the pair (B^-1 by a dense solve):
    the residual theorem of the pencil puts an eigenvalue within it of lam_i.  Also V^T B V in longdouble, rounded."""
    assert c.denseB is not None
    Vl = np.asarray(V, np.longdouble)
    BV = np.zeros_like(Vl)
    Rm = np.zeros(Vl.shape)
    for i in range(len(lam)):
        av, bv, _, _ = _ld_products(c, Vl[:, i])
        BV[:, i] = bv
        Rm[:, i] = av - np.longdouble(lam[i]) * bv
    G = Vl.T @ BV
    rb = np.sum(Rm * np.linalg.solve(c.denseB, Rm), axis=0)          # r^T B^-1 r, one factorisation for all pairs
    return np.sqrt(rb / np.diag(G).astype(np.float64)), G.astype(np.float64)


def pencil_norm(c):
    """an upper bound of |B^-1 A|_2 in the B-inner product, the largest generalized eigenvalue in modulus: for the slack
    n eps |B^-1 A| of a dense eigenvalue solve and of the roundings of r"""
    return float(np.max(np.abs(c.spectrum)))
