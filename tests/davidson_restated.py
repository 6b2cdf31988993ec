"""The contract of sgm_davidson (include/sigma_hip.h), restated in numpy for the tests, statement by
statement, from the header and not from the kernels: in float64 with the dot product as a parameter, and in np.longdouble.

Every operation is rounded on its own; `A u` is +0.0 plus the individually rounded products of a row in stored order
(mg_restated._Rows); `a.b` is eigsh_restated's (`device`: the order the header defines, a function of n alone); `M^-1 u` is
`apply_pc(u)`, a copy without a preconditioner; keep = min(k + (ncv - k)//2, ncv - 1).

    t = 1.0/sqrt(q1.q1) ; V_0 = q1 * t ; W_0 = A V_0 ; H(0,0) = V_0.W_0
    m = 1 ; locked = 0 ; anorm = 0 ; steps = restarts = 0
    loop:
      a NaN in H[:m, :m]: leave, found = 0 ; (theta, Z) = symeig(H[:m, :m]) ; a NaN in theta: leave, found = 0
      anorm = max(anorm, max |theta_i|) ; order ascending, ties by index
      while locked < min(k, m):
          c = order[locked] ; u = V[:, :m] Z[:, c], y = W[:, :m] Z[:, c]  (`rotate`: ((0.0 + V(i,0) z_0) + V(i,1) z_1) + ...)
          r = y - theta_c * u ; rn = sqrt(r.r) ; rn <= tol * anorm: locked += 1, else leave the while
      locked == k: for j = 0 .. (locked at the start of this pass) - 1: r, rn of order[j] ; not (rn <= tol * anorm): locked = j, stop
      locked == k: leave, found = k, converged ; locked == m: leave, found = m ; steps == max_steps: leave, found = min(k, m)
      m == ncv: V[:, :keep] = V[:, :m] Z[:, first keep] ; W the same ; H = diag(theta of the kept) ; theta = those, Z = I,
                order = 0, 1, .. ; m = keep ; restarts += 1
      t = M^-1 r ; tau = sqrt(t.t)
      h_i = V_i.t ; t = (..(t - h_0 V_0) - ..) - h_{m-1} V_{m-1} ; g_i = V_i.t ; t = (..(t - g_0 V_0) - ..) ; beta = sqrt(t.t)
      a NaN in tau or beta: leave, found = 0 ; not (beta > 2^-40 * tau): leave, found = min(k, locked)
      s = 1.0/beta ; V_m = t * s ; W_m = A V_m ; H(i,m) = H(m,i) = V_i.W_m, i = 0..m ; m += 1 ; steps += 1
    Vout = V[:, :m] Z[:, first found] ; lambda_i = theta_i ; resid_i = sqrt(r.r), r = A v_i - lambda_i * v_i
    products: W_0, one per step, one per returned pair ; applies: one per `t = M^-1 r` with a preconditioner."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import eigsh_restated as ER
import mg_direct_restated as MD
import mg_restated as MR
import minres_restated as MN

EPS = ER.EPS
TINY = ER.TINY
TOL = 1e-8
ROOT = ER.ROOT


def davidson(R, k, ncv, q1, apply_pc=None, tol=TOL, max_steps=1000, dot="device", dtype=np.float64):
    """The loop above on the rows R (mg_restated._Rows).  Returns a namespace: lam, V, residuals (the restatement's own
    sqrt(r.r) of the returned pairs), steps, products, applies, restarts, found, converged, anorm, relocks (how often the
    look at the earlier pairs before "converged" found one that fails: not a field of the device's result)."""
    ft = dtype
    sums = ER.SUMS[dot]
    dot1 = lambda a, b: sums((a * b)[:, None])[0]
    val = R.val.astype(ft)
    A = lambda u: MN.rows_matvec(R, u, val)
    n = R.n
    assert 1 <= k < ncv <= 64 and ncv < n and tol >= TINY and max_steps >= 0
    keep = min(k + (ncv - k) // 2, ncv - 1)
    one, tiny = ft(1.0), ft(TINY)
    q1 = np.asarray(q1, ft)
    V = np.zeros((n, ncv), ft)
    W = np.zeros((n, ncv), ft)
    H = np.zeros((ncv, ncv), ft)
    st = SimpleNamespace(steps=0, products=0, applies=0, restarts=0, relocks=0)

    def product(u):
        st.products += 1
        return A(u)

    def out(found, converged, m, theta, Z, order, anorm):
        lam = np.full(k, np.nan, ft)
        resid = np.full(k, np.nan, ft)
        Vout = np.zeros((n, k), ft)
        if found > 0:
            sel = order[:found]
            Vout[:, :found] = ER.rotate(V[:, :m], Z[:, sel])
            lam[:found] = theta[sel]
            for i in range(found):
                y = product(Vout[:, i])
                r = y - lam[i] * Vout[:, i]
                resid[i] = np.sqrt(dot1(r, r))
        return SimpleNamespace(lam=lam, V=Vout, residuals=resid, steps=st.steps, products=st.products, applies=st.applies,
                               restarts=st.restarts, found=found, converged=bool(converged), anorm=anorm, relocks=st.relocks)

    with np.errstate(all="ignore"):
        t = one / np.sqrt(dot1(q1, q1))
        V[:, 0] = q1 * t
        W[:, 0] = product(V[:, 0])
        H[0, 0] = dot1(V[:, 0], W[:, 0])
        m, locked, anorm = 1, 0, ft(0.0)
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
                u = ER.rotate(V[:, :m], Z[:, c:c + 1])[:, 0]
                y = ER.rotate(W[:, :m], Z[:, c:c + 1])[:, 0]
                rj = y - theta[c] * u
                return rj, bool(np.sqrt(dot1(rj, rj)) <= ft(tol) * anorm)

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
                        st.relocks += 1
                        break
            if locked == k:
                return out(k, True, m, theta, Z, order, anorm)
            if locked == m:
                return out(m, False, m, theta, Z, order, anorm)
            if st.steps == max_steps:
                return out(min(k, m), False, m, theta, Z, order, anorm)
            if m == ncv:
                kept = order[:keep]
                V[:, :keep] = ER.rotate(V[:, :m], Z[:, kept])
                W[:, :keep] = ER.rotate(W[:, :m], Z[:, kept])
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
            h = sums(V[:, :m] * t[:, None])
            for i in range(m):
                t = t - h[i] * V[:, i]
            g = sums(V[:, :m] * t[:, None])
            for i in range(m):
                t = t - g[i] * V[:, i]
            beta = np.sqrt(dot1(t, t))
            if np.isnan(tau) or np.isnan(beta):
                return out(0, False, m, theta, Z, order, anorm)
            if not (beta > tiny * tau):
                return out(min(k, locked), False, m, theta, Z, order, anorm)
            s = one / beta
            V[:, m] = t * s
            W[:, m] = product(V[:, m])
            col = sums(V[:, :m + 1] * W[:, m][:, None])
            H[:m + 1, m] = col
            H[m, :m + 1] = col
            m += 1
            st.steps += 1


# ------------------------------------------------------------------------------------ the cases
class CompositeRows:
    """The product of a composite matrix, the reference's composite_matvec_add: y = 0, then for every row block its column
    blocks in order, y(i) = y(i) + (the leaf's own row sum, which starts at +0.0).  float64 only.  blocks[(it, jt)] = (nrow,
    ncol, ptr, node, val), 1-based; row_ptr / col_ptr: the 1-based block edges."""

    def __init__(self, row_ptr, col_ptr, blocks):
        self.rp, self.cp = np.asarray(row_ptr) - 1, np.asarray(col_ptr) - 1
        self.n = int(self.rp[-1])
        self.leaves = {ij: MR._Rows(B) for ij, B in sorted(blocks.items())}
        self.val = np.zeros(0)

    def matvec(self, x):
        y = np.zeros(self.n)
        with np.errstate(all="ignore"):
            for (it, jt), L in self.leaves.items():
                r0, r1, c0, c1 = self.rp[it], self.rp[it + 1], self.cp[jt], self.cp[jt + 1]
                y[r0:r1] = y[r0:r1] + L.matvec(np.ascontiguousarray(x[c0:c1]))
        return y


def composite_fixture(name="comp_poisson2d_32x24"):
    """(row_ptr, col_ptr, blocks) of a 2 x 2 composite fixture of tests/golden"""
    g = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    rp, cp = g["ref_comp_row_ptr"].astype(np.int32), g["ref_comp_col_ptr"].astype(np.int32)
    blocks = {}
    for i in range(2):
        for j in range(2):
            t = f"ref_blk{i + 1}{j + 1}_"
            blocks[(i, j)] = (int(rp[i + 1] - rp[i]), int(cp[j + 1] - cp[j]), g[t + "ptr"].astype(np.int32), g[t + "node"].astype(np.int32),
                              g[t + "val"].astype(np.float64))
    return rp, cp, blocks


def _dense(n, ptr, node, val):
    D = np.zeros((n, n))
    np.add.at(D, (np.repeat(np.arange(n), np.diff(ptr)), node - 1), val)
    return D


@functools.lru_cache(maxsize=None)
def _poisson(nx, ny):
    return MR.poisson_case(nx, ny)


@functools.lru_cache(maxsize=None)
def _matrix(key):
    """(A, Ps) with A = (n, n, ptr, node, val), 1-based CSR; Ps: its hierarchy, or None"""
    if key.startswith("poisson"):
        nx, ny = (int(s) for s in key[len("poisson"):].split("x"))
        return _poisson(nx, ny)
    if key == "spd300":
        return MR.random_spd_case(300)
    if key == "lap3d":
        d = np.load(os.path.join(ROOT, "tests", "golden", "laplace3d_8x7x6.npz"))
        n = int(d["n"])
        return (n, n, d["ref_ptr"].astype(np.int32), d["ref_node"].astype(np.int32), d["ref_val"].astype(np.float64)), None
    if key == "comp32x24":           # the assembled matrix of the composite fixture (case() takes its product from the blocks)
        n, ptr, node, val = ER._golden("comp_poisson2d_32x24")
        return (n, n, ptr, node, val), None
    if key == "odd":                 # 45 x 41 = 1845 rows: an odd n above one workgroup's 1024 -- two workgroups of partial sums
        return _poisson(45, 41)
    if key == "diag40":
        n = 40
        return (n, n, np.arange(1, n + 2, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), np.arange(1, n + 1, dtype=np.float64)), None
    if key == "late40":
        # diag(1, 1.001, 2, 3, .., 39) with q1 = (1, 1e-7, 1, 1, ..): the space meets the eigenvector of 1.001 late, after the
        # pairs of 1 and 2 have been locked, and its Ritz value comes down between them
        n = 40
        d = np.concatenate([[1.0, 1.001], np.arange(2, n)]).astype(np.float64)
        return (n, n, np.arange(1, n + 2, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), d), None
    raise KeyError(key)


def cos_spectrum(nx, ny):
    """the spectrum of the nx x ny 5-point Laplacian, ascending, in longdouble"""
    return np.sort((ER._cos_spectrum(nx)[:, None] + ER._cos_spectrum(ny)[None, :]).ravel())


@functools.lru_cache(maxsize=None)
def case(key):
    """n, ptr, node, val (1-based CSR), Ps, rows (mg_restated._Rows), dense (None above 4096 rows), q1, maxrow, norm2 (an
    upper bound of |A|_2: the largest absolute row sum)"""
    A, Ps = _matrix(key)
    n, _, ptr, node, val = A
    rows = CompositeRows(*composite_fixture()) if key == "comp32x24" else MR._Rows(A)
    dense = _dense(n, ptr, node, val) if n <= 4096 else None
    q1 = ER.start_vector(n)
    if key == "late40":
        q1 = np.ones(n)
        q1[1] = 1e-7
    absrow = np.zeros(n)
    np.add.at(absrow, np.repeat(np.arange(n), np.diff(ptr)), np.abs(val))
    for a in (val, q1):
        a.setflags(write=False)
    return SimpleNamespace(name=key, n=n, ptr=ptr, node=node, val=val, A=A, Ps=Ps, rows=rows, dense=dense, q1=q1,
                           maxrow=int(np.diff(ptr).max()), norm2=float(absrow.max()))


@functools.lru_cache(maxsize=None)
def preconditioner(key, pc):
    """apply_pc of the float64 restatement: "none" -> None, "jacobi", "mg" (V(1,1), omega 0.8, 8 coarse sweeps),
    "mg22direct" (V(2,2), omega 0.8, the coarsest level solved directly).  ILDU(0) has no restatement in numpy: the tests that
    need it pass the oracle's solve."""
    c = case(key)
    if pc == "none":
        return None
    if pc == "jacobi":
        idiag = c.rows.idiag()
        return lambda u: idiag * u
    if pc == "mg":
        return MR.Vectorised(c.A, c.Ps, 0.8, 1, 1, 8).apply
    if pc == "mg22direct":
        return MD.Vectorised(c.A, c.Ps, 0.8, 2, 2).apply
    raise KeyError(pc)


def preconditioner_ld(key, pc):
    """M^-1 for the longdouble restatement: Jacobi in longdouble; a V-cycle is the float64 one (the only statement of it there
    is) on the rounded vector"""
    c = case(key)
    if pc == "none":
        return None
    if pc == "jacobi":
        idl = np.longdouble(1.0) / (np.longdouble(1.0) / c.rows.idiag().astype(np.longdouble))
        return lambda u: idl * u
    f = preconditioner(key, pc)
    return lambda u: f(np.asarray(u, np.float64)).astype(np.longdouble)


def _freeze(r):
    for a in (r.lam, r.V, r.residuals):
        a.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated(key, pc, k, ncv, dot="device", tol=TOL, max_steps=1000):
    c = case(key)
    return _freeze(davidson(c.rows, k, ncv, c.q1, preconditioner(key, pc), tol, max_steps, dot))


@functools.lru_cache(maxsize=None)
def restated_ld(key, pc, k, ncv, tol=TOL, max_steps=1000):
    c = case(key)
    return _freeze(davidson(c.rows, k, ncv, c.q1, preconditioner_ld(key, pc), tol, max_steps, "numpy", np.longdouble))


def true_residuals(c, lam, V):
    """eigsh_restated.true_residuals on a case of this module (longdouble residual norms, |v_i|, the forward bound of the
    float64 evaluation of sqrt(r.r))"""
    return ER.true_residuals(c, lam, V)
