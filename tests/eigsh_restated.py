"""The contract of sgm_eigsh, sgm_symeig_host and sgm_basis_rotate (include/sigma_hip.h), restated in numpy
for the tests, statement by statement, from the header and not from the kernels: once in float64 with the dot product as a
parameter, once in np.longdouble.

Every operation is rounded on its own; `A u` is +0.0 plus the individually rounded products of a row in stored order
(mg_restated._Rows); m = ncv; keep = min(k + (m - k)//2, m - 1).

    q_0 = q1 / sqrt(q1.q1) ; l = 0 ; anorm = 0 ; H = 0
    cycle c = 0, 1, ...:
      for j = l .. m-1:
         w = A q_j
         h_i = q_i.w, i = 0..j ; w = (..(w - h_0 q_0) - ..) - h_j q_j
         g_i = q_i.w, i = 0..j ; w = (..(w - g_0 q_0) - ..) - g_j q_j
         H(j,j) = h_j + g_j ; beta_j = sqrt(w.w)
         s = (j == l ? anorm : s) ; |H(j,j)| > s: s = |H(j,j)| ; beta_j > s: s = beta_j
         not (beta_j > 2^-40 * s): the cycle ends with nc = j + 1 columns ("closed")
         j < m-1: H(j+1,j) = H(j,j+1) = beta_j
         t = 1.0/beta_j ; q_{j+1} = w * t
      a NaN among this cycle's H(j,j), beta_j: leave with found = 0, converged = False
      (theta, Z) = symeig(H[:nc, :nc]) ; anorm = max(anorm, max |theta_i|)
      order: ascending for SA, descending for LA, ties by index
      closed: leave with found = min(k, nc), converged = (nc >= k)
      rho_i = |beta_{m-1} * Z(m-1, i)|
      rho_i <= tol * anorm for the first k: leave converged ; c == max_restarts: leave, not converged (found = k either way)
      Q[:, :keep] = Q[:, :m] Z[:, first keep] ; q_keep = q_m
      H = 0 ; H(i,i) = theta_i, H(keep,i) = H(i,keep) = beta_{m-1} * Z(m-1, i) for the kept i ; l = keep ; restarts += 1
    V = Q[:, :nc] Z[:, first found] ; lambda_i = theta_i ; resid_i = sqrt(r.r), r = A v_i - lambda_i * v_i

symeig is cyclic Jacobi (`symeig` below spells it out); `Q Z` adds ((0.0 + q_0 z_0c) + q_1 z_1c) + ... ascending (`rotate`)."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import mg_restated as MR
import minres_restated as MN

EPS = float(np.finfo(np.float64).eps)
U = EPS / 2                       # unit roundoff
TINY = 2.0 ** -40
MAX_SWEEPS = 64
TOL = 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------ dot products
def dot_grid(n):
    """workgroups of the kernels that leave partial sums: a function of n alone"""
    return min(1024, max(1, -(-n // 1024)))


def _block_sums(acc):
    """acc: (..., G, 256) thread accumulators -> (..., G): each wave of 64 sums by the butterfly v += v[lane ^ 32], ^ 16, ..,
    ^ 1; the four wave sums are added left to right"""
    w = acc.reshape(acc.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    s = w[..., 0, 0]
    for k in range(1, 4):
        s = s + w[..., k, 0]
    return s


def device_sums(P):
    """The device's defined order (header: "Dot products") for the columns of P (n x c products): thread t of the 256 G adds
    elements 2i, 2i+1 for i = t, t + 256 G, ... to an accumulator that starts at 0.0 (thread 0 then the last element of an odd
    n); workgroup sums as _block_sums; for G > 1 one workgroup re-reduces them: thread t adds sums t, t + 256, ... to 0.0."""
    P = np.asarray(P)
    if P.ndim == 1:
        return device_sums(P[:, None])[0]
    n, c = P.shape
    G = dot_grid(n)
    T = 256 * G
    n2 = n // 2
    acc = np.zeros((c, T), P.dtype)
    for r0 in range(0, n2, T):
        i = np.arange(r0, min(r0 + T, n2))
        acc[:, :len(i)] = acc[:, :len(i)] + P[2 * i].T
        acc[:, :len(i)] = acc[:, :len(i)] + P[2 * i + 1].T
    if n & 1:
        acc[:, 0] = acc[:, 0] + P[n - 1]
    part = _block_sums(acc.reshape(c, G, 256))             # (c, G)
    if G == 1:
        return part[:, 0]
    v = np.zeros((c, 256), P.dtype)
    for r0 in range(0, G, 256):
        cnt = min(256, G - r0)
        v[:, :cnt] = v[:, :cnt] + part[:, r0:r0 + cnt]
    return _block_sums(v.reshape(c, 1, 256))[:, 0]


def _sums_device(P):
    return device_sums(P)


def _sums_seq(P):
    return np.cumsum(P, axis=0)[-1]


def _sums_numpy(P):
    return np.array([np.dot(P[:, c], np.ones(P.shape[0], P.dtype)) for c in range(P.shape[1])], P.dtype)


# each takes the n x c array of products and returns the c sums
SUMS = {"device": _sums_device, "seq": _sums_seq, "numpy": _sums_numpy}


# ------------------------------------------------------------------------------------ symeig, rotate
def symeig(H, dtype=np.float64):
    """Cyclic Jacobi on the full symmetric H (header, sgm_symeig_host).  Returns theta (unsorted), Z, sweeps."""
    ft = dtype
    A = np.array(H, ft)
    m = A.shape[0]
    Z = np.eye(m, dtype=ft)
    one, two = ft(1.0), ft(2.0)
    sweeps = 0
    iu = np.triu_indices(m, 1)
    with np.errstate(all="ignore"):
        for _ in range(MAX_SWEEPS):
            if not np.any(A[iu] != 0):
                break
            sweeps += 1
            for p in range(m - 1):
                for q in range(p + 1, m):
                    apq = A[p, q]
                    if apq == 0:
                        continue
                    tau = (A[q, q] - A[p, p]) / (two * apq)
                    r = np.sqrt(one + tau * tau)
                    t = one / (tau + r) if tau >= 0 else -one / (r - tau)
                    c = one / np.sqrt(one + t * t)
                    s = t * c
                    app, aqq = A[p, p] - t * apq, A[q, q] + t * apq
                    x, y = A[:, p].copy(), A[:, q].copy()
                    xp, yq = c * x - s * y, s * x + c * y
                    A[:, p] = xp
                    A[p, :] = xp
                    A[:, q] = yq
                    A[q, :] = yq
                    A[p, p], A[q, q] = app, aqq
                    A[p, q] = A[q, p] = 0
                    x, y = Z[:, p].copy(), Z[:, q].copy()
                    Z[:, p] = c * x - s * y
                    Z[:, q] = s * x + c * y
    return np.diag(A).copy(), Z, sweeps


def rotate(Q, Z):
    """Q[:, :m] Z: entry (i, c) = ((0.0 + Q(i,0) Z(0,c)) + Q(i,1) Z(1,c)) + ..., ascending"""
    m, kk = Z.shape
    out = np.zeros((Q.shape[0], kk), Q.dtype)
    for r in range(m):
        out = out + Q[:, r:r + 1] * Z[r:r + 1, :]
    return out


# ------------------------------------------------------------------------------------ the loop
def eigsh(R, k, ncv, which, q1, tol=TOL, max_restarts=200, dot="device", dtype=np.float64):
    """The loop above on the rows R (mg_restated._Rows).  Returns a namespace: lam, V, residuals (the restatement's own
    sqrt(r.r)), rho (the estimates of the returned pairs), restarts, products, found, converged, anorm."""
    ft = dtype
    sums = SUMS[dot]
    val = R.val.astype(ft)
    A = lambda u: MN.rows_matvec(R, u, val)
    n, m = R.n, ncv
    assert 1 <= k < m <= 64 and m < n and tol >= TINY and max_restarts >= 0 and which in ("SA", "LA")
    keep = min(k + (m - k) // 2, m - 1)
    one, tiny = ft(1.0), ft(TINY)
    q1 = np.asarray(q1, ft)
    Q = np.zeros((n, m + 1), ft)
    H = np.zeros((m, m), ft)
    products = restarts = 0
    nanres = SimpleNamespace(lam=np.full(k, np.nan), V=np.zeros((n, k)), residuals=np.full(k, np.nan), rho=np.full(k, np.nan),
                             found=0, converged=False)
    with np.errstate(all="ignore"):
        Q[:, 0] = q1 / np.sqrt(sums((q1 * q1)[:, None])[0])
        l, anorm, c = 0, ft(0.0), 0
        while True:
            nc, closed, s = m, False, anorm
            beta = np.zeros(m, ft)
            for j in range(l, m):
                w = A(Q[:, j])
                products += 1
                h = sums(Q[:, :j + 1] * w[:, None])
                for i in range(j + 1):
                    w = w - h[i] * Q[:, i]
                g = sums(Q[:, :j + 1] * w[:, None])
                for i in range(j + 1):
                    w = w - g[i] * Q[:, i]
                H[j, j] = h[j] + g[j]
                beta[j] = np.sqrt(sums((w * w)[:, None])[0])
                if j == l:
                    s = anorm
                if np.abs(H[j, j]) > s:
                    s = np.abs(H[j, j])
                if beta[j] > s:
                    s = beta[j]
                if not (beta[j] > tiny * s):
                    nc, closed = j + 1, True
                    break
                if j < m - 1:
                    H[j + 1, j] = H[j, j + 1] = beta[j]
                t = one / beta[j]
                Q[:, j + 1] = w * t
            if np.isnan(np.diag(H)[l:nc]).any() or np.isnan(beta[l:nc]).any():
                nanres.restarts, nanres.products, nanres.anorm = restarts, products, anorm
                return nanres
            theta, Z, _ = symeig(H[:nc, :nc], ft)
            anorm = max(anorm, np.max(np.abs(theta)))
            order = np.argsort(theta if which == "SA" else -theta, kind="stable")
            if closed:
                found, converged = min(k, nc), nc >= k
                rho = np.zeros(found, ft)
                break
            rho = np.abs(beta[m - 1] * Z[m - 1, order])
            found = k
            if np.all(rho[:k] <= ft(tol) * anorm):
                converged = True
                break
            if c == max_restarts:
                converged = False
                break
            kept = order[:keep]
            Q[:, :keep] = rotate(Q[:, :m], Z[:, kept])
            Q[:, keep] = Q[:, m]
            H[:] = 0
            for i in range(keep):
                H[i, i] = theta[kept[i]]
                H[keep, i] = H[i, keep] = beta[m - 1] * Z[m - 1, kept[i]]
            l = keep
            restarts += 1
            c += 1
        sel = order[:found]
        V = rotate(Q[:, :nc], Z[:, sel])
        lam = theta[sel]
        resid = np.zeros(found, ft)
        for i in range(found):
            y = A(V[:, i])
            products += 1
            r = y - lam[i] * V[:, i]
            resid[i] = np.sqrt(sums((r * r)[:, None])[0])
    pad = lambda a: np.concatenate([a, np.full(k - found, np.nan, ft)])
    Vp = np.zeros((n, k), ft)
    Vp[:, :found] = V
    return SimpleNamespace(lam=pad(lam), V=Vp, residuals=pad(resid), rho=pad(rho[:found]), restarts=restarts, products=products,
                           found=found, converged=bool(converged), anorm=anorm)


# ------------------------------------------------------------------------------------ the cases
def start_vector(n):
    """sg.eigsh's default q1: 1 + ((i * 2654435761) mod 1024) / 1024, exact in float64"""
    i = np.arange(n, dtype=np.uint64)
    return 1.0 + ((i * np.uint64(2654435761)) % np.uint64(1024)).astype(np.float64) / 1024.0


def grid5(nx, ny, raised=()):
    """the 5-point Laplacian of an nx x ny grid (1-based CSR), diagonal entries of the rows in `raised` lifted by 10, 20, ..."""
    from sigma_amd import problems as Pr
    ptr, node, val = Pr.poisson2d_csr(nx, ny)
    val = val.copy()
    if len(raised):
        row = np.repeat(np.arange(nx * ny), np.diff(ptr))
        for a, r in enumerate(raised):
            val[(row == r) & (node - 1 == r)] += 10.0 * (a + 1)
    return nx * ny, ptr, node, val


def outlier_rows(n):
    """8 rows spread over the grid, away from each other"""
    return [int(n * (2 * a + 1) / 16) for a in range(8)]


def _golden(name):
    d = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    return int(d["n"]), d["ref_ptr"].astype(np.int32), d["ref_node"].astype(np.int32), d["ref_val"].astype(np.float64)


# name -> (matrix key, storage formats on the device)
CASES = {
    "lap127": ("lap127", ("csr", "ell")),
    "p32x24": ("p32x24", ("csr", "ell")),
    "grid45x41": ("grid45x41", ("csr",)),
    "spd128": ("spd128", ("csr",)),
    "saddle": ("saddle", ("composite",)),
}
GRID = [(1, 8), (4, 20), (6, 32)]
SMALL = [(name, fmt) for name, (_, fmts) in CASES.items() for fmt in fmts]


@functools.lru_cache(maxsize=None)
def _matrix(key):
    if key == "lap127":
        return _golden("diffusion1d_csr_127")
    if key == "p32x24":
        return _golden("poisson2d_32x24")
    if key == "grid45x41":
        return grid5(45, 41)
    if key == "spd128":
        return _golden("random_spd_128")
    if key == "saddle":
        return MN._saddle()
    if key == "diag3":
        n = 40
        return n, np.arange(1, n + 2, dtype=np.int32), np.arange(1, n + 1, dtype=np.int32), np.arange(1, n + 1, dtype=np.float64)
    if key == "outliers":
        return grid5(320, 317, outlier_rows(320 * 317))
    raise KeyError(key)


# pi to the precision of np.longdouble (a float64 pi would put an error of 1e-16 * j into every angle)
_PI_LD = np.longdouble(4) * np.arctan(np.longdouble(1))


def _cos_spectrum(nx):
    """2 - 2 cos(j pi / (nx + 1)), j = 1 .. nx, in longdouble: the spectrum of tridiag(-1, 2, -1)"""
    j = np.arange(1, nx + 1, dtype=np.longdouble)
    return np.longdouble(2) - np.longdouble(2) * np.cos(j * _PI_LD / np.longdouble(nx + 1))


@functools.lru_cache(maxsize=None)
def case(name):
    """n, ptr, node, val (1-based CSR), rows (mg_restated._Rows), dense (None above 4096 rows), q1, spectrum (ascending,
    longdouble: analytic where there is a formula, eigvalsh of the dense matrix otherwise; None for `outliers`), maxrow,
    norm2 (|A|_2 or an upper bound of it)"""
    n, ptr, node, val = _matrix(name)
    rows = MR._Rows((n, n, ptr, node, val))
    dense = None
    if n <= 4096:
        dense = np.zeros((n, n))
        r0 = np.repeat(np.arange(n), np.diff(ptr))
        np.add.at(dense, (r0, node - 1), val)
        assert np.array_equal(dense, dense.T)
    if name == "lap127":
        # diffusion_1d: the golden file carries the matrix; its spectrum is that of tridiag(-1, 2, -1) scaled by its diagonal / 2
        scale = np.longdouble(dense[0, 0]) / 2
        assert np.allclose(np.diag(dense, 1), -float(scale)) and np.allclose(np.diag(dense), 2 * float(scale))
        spec = np.sort(scale * _cos_spectrum(127))
    elif name == "p32x24":
        spec = np.sort((_cos_spectrum(32)[:, None] + _cos_spectrum(24)[None, :]).ravel())
    elif name == "grid45x41":
        spec = np.sort((_cos_spectrum(45)[:, None] + _cos_spectrum(41)[None, :]).ravel())
    elif name == "diag3":
        # q1 = e1 + e2 + e3 spans an invariant subspace of dimension 3: all a Krylov method can see of diag(1..40) is {1, 2, 3}
        spec = np.arange(1, 4, dtype=np.longdouble)
    elif dense is not None:
        spec = np.linalg.eigvalsh(dense).astype(np.longdouble)
    else:
        spec = None
    if name == "diag3":
        q1 = np.zeros(n)
        q1[:3] = 1.0
    else:
        q1 = start_vector(n)
    absrow = np.zeros(n)
    np.add.at(absrow, np.repeat(np.arange(n), np.diff(ptr)), np.abs(val))
    for a in (val, q1):
        a.setflags(write=False)
    return SimpleNamespace(name=name, n=n, ptr=ptr, node=node, val=val, rows=rows, dense=dense, q1=q1, spectrum=spec,
                           maxrow=int(np.diff(ptr).max()), norm2=float(absrow.max()))


@functools.lru_cache(maxsize=None)
def restated(name, k, ncv, which, dot="device", tol=TOL, max_restarts=200):
    c = case(name)
    r = eigsh(c.rows, k, ncv, which, c.q1, tol, max_restarts, dot)
    for a in (r.lam, r.V, r.residuals, r.rho):
        a.setflags(write=False)
    return r


# ------------------------------------------------------------------------------------ yardsticks that do not use the restatement
def gamma(p):
    return p * U / (1 - p * U)


def true_residuals(c, lam, V):
    """R_i = |A v_i - lam_i v_i|_2 and |v_i|_2 in longdouble from the case's own CSR arrays, and the forward bound of the float64
    evaluation of sqrt(r.r): the 2-norm of gamma_{d+2} (|A||v| + |lam||v|) plus gamma_n R_i (d: the longest row)"""
    vall = c.val.astype(np.longdouble)
    absval = np.abs(vall)
    Rs, norms, bounds = [], [], []
    for i in range(len(lam)):
        v = np.asarray(V[:, i], np.longdouble)
        li = np.longdouble(lam[i])
        r = MN.rows_matvec(c.rows, v, vall) - li * v
        R = np.sqrt(np.dot(r, r))
        e = MN.rows_matvec(c.rows, np.abs(v), absval) + np.abs(li) * np.abs(v)
        bound = gamma(c.maxrow + 2) * np.sqrt(np.dot(e, e)) + gamma(c.n) * R
        Rs.append(float(R))
        norms.append(float(np.sqrt(np.dot(v, v))))
        bounds.append(float(bound))
    return np.array(Rs), np.array(norms), np.array(bounds)


def extremes(spectrum, k, which):
    """the k extreme exact eigenvalues in the order the solver returns them: ascending for SA, descending for LA"""
    return spectrum[:k] if which == "SA" else spectrum[::-1][:k]


OUTLIER_LIFTS = 10.0 * np.arange(8, 0, -1)         # 80, 70, ..., 10: the lifted diagonal entries of `outliers`, descending


def spectrum_slack(c):
    """what the yardstick itself may be off by: the analytic formulas are evaluated in longdouble (a few of its roundings of
    |A|); eigvalsh of a dense symmetric matrix is backward stable, |error| <= p(n) eps |A|_2 with p(n) taken as n"""
    if c.name in ("lap127", "p32x24", "grid45x41", "diag3"):
        return 16 * float(np.finfo(np.longdouble).eps) * c.norm2
    return c.n * EPS * c.norm2


def spectrum_distances(c, lam, which):
    """distance of every lam_i to the i-th extreme exact eigenvalue (ascending for SA, descending for LA).
    `outliers` has no formula and is too large for eigvalsh: A = L + D with L the 5-point Laplacian (0 < lambda(L) < 8) and D
    the diagonal lift, so by Weyl's inequalities the i-th largest eigenvalue of A lies in [d_i, d_i + 8] with d_i the i-th
    largest lift (80, 70, 60, 50 for the first four): disjoint intervals holding exactly one eigenvalue each.  The distance
    returned is then that of lam_i to its interval (LA only)."""
    lam = np.asarray(lam, np.longdouble)
    if c.spectrum is not None:
        return np.abs(lam - extremes(c.spectrum, len(lam), which)).astype(np.float64)
    assert c.name == "outliers" and which == "LA" and len(lam) <= 8
    lo = OUTLIER_LIFTS[:len(lam)]
    return np.maximum(0.0, np.maximum(lo - lam, lam - (lo + 8.0))).astype(np.float64)


def norm2(c):
    """|A|_2 where the spectrum is known; for `outliers` its largest diagonal entry, a lower bound (the Rayleigh quotient of a
    unit vector): a bar built from it is the stricter one"""
    if c.spectrum is not None:
        return float(np.max(np.abs(c.spectrum)))
    row = np.repeat(np.arange(c.n), np.diff(c.ptr))
    return float(c.val[c.node - 1 == row].max())


def case_grid(name):
    """(k, ncv) per case.  `saddle` with (1, 8) does not converge within 200 restarts in the restatement (the smallest
    eigenvalue of the indefinite matrix, 8 columns): it takes (1, 16) instead, the cap stays"""
    if name == "saddle":
        return [(1, 16), (4, 20), (6, 32)]
    return GRID
