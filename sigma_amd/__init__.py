"""sigma_amd -- MI355X-native SpMV + Krylov path for SiGMA (danshapero/sigma).

This package is the thin host side above the C ABI of ``libsigma_hip.so``
(include/sigma_hip.h): it mirrors the reference's operator / solver interface for the
hot path -- same names, argument meaning and error behaviour --

    A = csr_matrix(n, m, ptr, node, val)       cs_matrices.f90:32-151  (1-based arrays)
    A = ellpack_matrix(n, m, node, val)        ellpack_matrices.f90:28-105
    sparse_matrix_sum(B, C), sparse_matrix_product(B, C), PtAP(A, P), RARt(A, R)
                                               sparse_matrix_algebra.f90:13; result.refill(X, Y)
    A.matvec(x, y); A.matvec_add(x, y)         linear_operator_interface.f90:185-194
    A.set_value(i, j, z); A.add_value(i, j, z); A.get_value(i, j); A.add_multiple_values(is, js, B);
    A.add_sparse_matrix(B, alpha); A.zero(); A.scalar_multiply(alpha)      sparse_matrix_interfaces.f90:106-128,378-460
                                               (scalars or ordered batches, edited in HBM); edit_plan(A, i, j).add(z)
    solver = cg(tolerance)                     cg_solvers.f90:36-47
    solver = bicgstab(tolerance)               bicgstab_solvers.f90:37-48
    solver = gmres(tolerance, restart); solver = minres(tolerance)         extensions: GMRES(m); MINRES for symmetric indefinite A
    solver = lsqr(tolerance, normal_tolerance, damp)                       extension: least squares with a rectangular A
    pc = jacobi(); pc = ldu(incomplete, level) jacobi_solvers.f90:23-31, ldu_solvers.f90:73-86
    pc = multigrid(P, omega, nu_pre, nu_post)  V-cycle on the Galerkin levels of the prolongations P (an extension)
                                               coarse="direct": the last level inverted at setup, applied as a dense product
    agg, nagg = aggregate(A, theta); P = aggregation_hierarchy(A, theta, smooth_omega, max_levels, min_coarse)
                                               smoothed aggregation: the prolongations from A alone (an extension)
    solver.setup(A); pc.setup(A)
    solver.solve(A, x, b[, pc])                generic solve: linear_solve / linear_solve_pc
    solver.iterations, solver.tolerance, solver.nn, solver.initialized
    solver.destroy(); A.destroy()

All arithmetic happens in hand-written HIP kernels for gfx950; there is NO CPU fallback:
importing works anywhere (so the build and symbol checks run on a CPU box), but any
compute call without a GPU raises SigmaError.  Vectors may be numpy arrays (copied over
PCIe inside the call) or CUDA/HIP torch tensors (used in place in HBM).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsigma_hip.so")

SGM_HOST, SGM_DEVICE = 0, 1
FMT_CSR, FMT_ELL = 1, 2

_lib = None


class SigmaError(RuntimeError):
    """Nonzero status from libsigma_hip.so (the reference would print and exit(1))."""

    def __init__(self, code, msg):
        super().__init__(f"[sigma_hip status {code}] {msg}")
        self.code = code


def build(force=False):
    """Compile libsigma_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    import subprocess
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", src, "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def _share_torch_hip_runtime():
    """One HIP/HSA runtime per process.  A torch wheel carries its own libamdhip64.so.7 and a
    libhsa-runtime64.so its other libraries ask for by a name the system copy does not answer to,
    so `import torch` AFTER this library has pulled in /opt/rocm's runtime starts a second HSA
    runtime and torch then finds no GPU.  When torch is installed but not yet imported, load its
    libamdhip64 first; the dynamic linker then hands the same copy to libsigma_hip.so (same
    soname), exactly as when torch was imported first.  SGM_HIP_RUNTIME=system skips this."""
    import sys
    if "torch" in sys.modules or os.environ.get("SGM_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """The loaded C-ABI library.  Fails loudly when the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SigmaError(-1, f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                 "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.sgm_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def _ck(rc):
    if rc != 0:
        raise SigmaError(rc, lib().sgm_last_error().decode(errors="replace"))


def init(device=0):
    _ck(lib().sgm_init(C.c_int(device)))


_adopted_stream = None      # hipStream_t the library launches on when it is not its own


def set_stream(stream_ptr):
    global _adopted_stream
    _ck(lib().sgm_set_stream(C.c_void_p(stream_ptr)))
    _adopted_stream = stream_ptr or None


def set_async(on):
    _ck(lib().sgm_set_async(C.c_int(1 if on else 0)))


def synchronize():
    _ck(lib().sgm_synchronize())


def set_option(name, value):
    """sgm_set_option: the DEFAULT that matrices / solvers / preconditioners created later start with (options are per
    handle: include/sigma_hip.h lists them; A.set_option / solver.set_option / pc.set_option change one handle)."""
    _ck(lib().sgm_set_option(name.encode(), C.c_int(int(value))))


def use_torch_stream():
    """Launch on torch's current HIP stream so torch.cuda.Event brackets our kernels."""
    import torch
    set_stream(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------ #
def _is_torch(a):
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def _arg(a, dtype, writable=False):
    """(pointer, where, keepalive) for a numpy array or a device torch tensor."""
    if _is_torch(a):
        import torch
        want = {np.float64: torch.float64, np.int32: torch.int32, np.int64: torch.int64}[dtype]
        if a.dtype != want or not a.is_contiguous():
            raise TypeError(f"torch tensor must be contiguous {want}")
        if not a.is_cuda:
            return _arg(a.numpy(), dtype, writable)
        # the library launches on its own stream unless it adopted torch's (use_torch_stream): a
        # tensor torch is still producing on another stream must be finished before we read it
        cur = torch.cuda.current_stream(a.device)
        if cur.cuda_stream != _adopted_stream:
            cur.synchronize()
        return C.c_void_p(a.data_ptr()), SGM_DEVICE, a
    arr = np.asarray(a)
    if arr.dtype != dtype or not arr.flags.c_contiguous or (writable and not arr.flags.writeable):
        if writable:
            raise TypeError(f"output array must be a contiguous writable {np.dtype(dtype)} numpy array")
        arr = np.ascontiguousarray(arr, dtype)
    return C.c_void_p(arr.ctypes.data), SGM_HOST, arr


def _len(a):
    return int(a.numel()) if _is_torch(a) else int(np.asarray(a).size)


def _need(a, n, what):
    """The C ABI takes raw pointers: a short vector would be read or written out of bounds."""
    if _len(a) < n:
        raise SigmaError(2, f"{what}: vector has {_len(a)} entries, the operation needs {n}")


OP_ADD, OP_TRANS = 1, 2        # SGM_OP_ADD, SGM_OP_TRANS (sgm_mat_matmat)


def _block(B, n, what, writable=False):
    """(pointer, where, k, ld, keepalive) for a block of k vectors of at least n entries, basis_rotate's convention: a numpy
    array of shape (rows, k) whose columns are contiguous (Fortran order, or a view of the leading rows of such an array:
    ld = the column stride), or a device tensor of shape (k, rows) whose rows are contiguous (ld = the row stride)."""
    if _is_torch(B) and B.is_cuda:
        import torch
        if B.dim() != 2 or B.dtype != torch.float64 or (B.shape[1] > 1 and B.stride(1) != 1):
            raise TypeError(f"{what}: a device block holds its columns as contiguous float64 rows: shape (k, n) expected")
        k, rows = int(B.shape[0]), int(B.shape[1])
        ld = int(B.stride(0)) if k > 1 else rows
        if ld < rows:
            raise TypeError(f"{what}: the rows of a device block must not overlap")
        cur = torch.cuda.current_stream(B.device)
        if cur.cuda_stream != _adopted_stream:
            cur.synchronize()
        ptr, where, keep = C.c_void_p(B.data_ptr()), SGM_DEVICE, B
    else:
        arr = B.numpy() if _is_torch(B) else np.asarray(B)
        if arr.ndim != 2:
            raise SigmaError(2, f"{what}: a block must have shape (n, k)")
        k, rows = int(arr.shape[1]), int(arr.shape[0])
        ok = arr.dtype == np.float64 and (rows <= 1 or arr.strides[0] == 8) and \
            (k <= 1 or (arr.strides[1] % 8 == 0 and arr.strides[1] >= 8 * max(rows, 1)))
        if not ok or (writable and not arr.flags.writeable):
            if writable:
                raise TypeError(f"{what}: the output block must be a writable float64 numpy array of shape (n, k) in Fortran order")
            arr = np.asfortranarray(arr, np.float64)
        ld = arr.strides[1] // 8 if k > 1 else max(rows, 1)
        ptr, where, keep = C.c_void_p(arr.ctypes.data), SGM_HOST, arr
    if rows < n:
        raise SigmaError(2, f"{what}: the block's columns have {rows} entries, the operation needs {n}")
    return ptr, where, k, max(ld, 1), keep


def matmat_probe(A, X, Y, op=0, block_cap=0, grid_cap=0):
    """sgm_mat_matmat_probe (test introspection): A.matmat & co. with the block width capped (block_cap = 1: the column loop,
    0 = no cap) and the native kernels' grid capped at grid_cap workgroups (0 = automatic).  Same bits whatever the caps."""
    return A._matmat(op, X, Y, "matmat_probe", block_cap=block_cap, grid_cap=grid_cap)


def _same_where(*ws):
    if len(set(ws)) != 1:
        raise TypeError("all vectors of one call must live in the same place (host or device)")
    return ws[0]


class _Matrix:
    """linear_operator face (nrow, ncol, matvec, matvec_add, destroy)."""

    def __init__(self):
        self._h = C.c_void_p()
        self.nrow = self.ncol = 0
        self.solver = None       # linear_operator%solver / %pc (linear_operator_interface.f90:29)
        self.pc = None

    # -- linear_operator_interface.f90:185-194 ------------------------------------------
    def _lens(self):
        """(entries matvec reads from x, entries it writes to y): ncol / nrow, or owned+halo /
        owned rows for a matrix distributed over processes."""
        return self.x_len, getattr(self, "n_local", self.nrow)

    def matvec(self, x, y):
        nx, ny = self._lens()
        _need(x, nx, "matvec x"); _need(y, ny, "matvec y")
        px, wx, _k1 = _arg(x, np.float64)
        py, wy, _k2 = _arg(y, np.float64, writable=True)
        _ck(lib().sgm_mat_matvec(self._h, px, py, C.c_int(_same_where(wx, wy))))
        return y

    def matvec_add(self, x, y):
        nx, ny = self._lens()
        _need(x, nx, "matvec_add x"); _need(y, ny, "matvec_add y")
        px, wx, _k1 = _arg(x, np.float64)
        py, wy, _k2 = _arg(y, np.float64, writable=True)
        _ck(lib().sgm_mat_matvec_add(self._h, px, py, C.c_int(_same_where(wx, wy))))
        return y

    def matvec_dots(self, x, y, w=None, add=False, yy=True):
        """sgm_mat_matvec_dots (test introspection): y = A x (add: y += A x) launched with the fused dot epilogues the
        solvers use, and what they leave per part: (wy, yy, count), numpy arrays of length nparts -- sum(w * y), sum(y * y)
        as a consumer kernel would reduce the partial sums, and how many partial sums there are; None where a dot was not
        asked for (w=None: no w.y; yy=False: no y.y)."""
        if hasattr(self, "_build"):
            self._build()
        nx, ny = self._lens()
        _need(x, nx, "matvec_dots x"); _need(y, ny, "matvec_dots y")
        px, wx, _k1 = _arg(x, np.float64)
        py, wy_, _k2 = _arg(y, np.float64, writable=True)
        ws = [wx, wy_]
        pw = None
        if w is not None:
            _need(w, ny, "matvec_dots w")
            pw, ww, _k3 = _arg(w, np.float64)
            ws.append(ww)
        P = getattr(self, "nparts", 1)
        o_wy = np.zeros(P, np.float64) if w is not None else None
        o_yy = np.zeros(P, np.float64) if yy else None
        cnt = np.zeros(P, np.int32)
        _ck(lib().sgm_mat_matvec_dots(self._h, px, py, pw, C.c_int(1 if add else 0),
                                      C.c_void_p(o_wy.ctypes.data) if o_wy is not None else None,
                                      C.c_void_p(o_yy.ctypes.data) if o_yy is not None else None,
                                      C.c_void_p(cnt.ctypes.data), C.c_int(_same_where(*ws))))
        return o_wy, o_yy, cnt

    # -- linear_operator_interface.f90:199-208 ------------------------------------------
    def matvec_t(self, x, y):
        _need(x, getattr(self, "n_local", self.nrow), "matvec_t x"); _need(y, getattr(self, "nc_local", self.ncol), "matvec_t y")
        px, wx, _k1 = _arg(x, np.float64)
        py, wy, _k2 = _arg(y, np.float64, writable=True)
        _ck(lib().sgm_mat_matvec_t(self._h, px, py, C.c_int(_same_where(wx, wy))))
        return y

    def matvec_t_add(self, x, y):
        _need(x, getattr(self, "n_local", self.nrow), "matvec_t_add x"); _need(y, getattr(self, "nc_local", self.ncol), "matvec_t_add y")
        px, wx, _k1 = _arg(x, np.float64)
        py, wy, _k2 = _arg(y, np.float64, writable=True)
        _ck(lib().sgm_mat_matvec_t_add(self._h, px, py, C.c_int(_same_where(wx, wy))))
        return y

    # -- multi-vector products (an extension: sgm_mat_matmat, include/sigma_hip.h) ---------
    def _matmat(self, op, X, Y, what, block_cap=None, grid_cap=0):
        if hasattr(self, "_build"):
            self._build()
        trans = bool(op & OP_TRANS)
        nx = getattr(self, "n_local", self.nrow) if trans else self._lens()[0]
        ny = getattr(self, "nc_local", self.ncol) if trans else self._lens()[1]
        px, wx, kx, ldx, _k1 = _block(X, nx, what + " X")
        py, wy, ky, ldy, _k2 = _block(Y, ny, what + " Y", writable=True)
        if kx != ky:
            raise SigmaError(2, f"{what}: X holds {kx} columns, Y holds {ky}")
        w = C.c_int(_same_where(wx, wy))
        if block_cap is None:
            _ck(lib().sgm_mat_matmat(self._h, C.c_int32(op), C.c_int32(kx), px, C.c_int64(ldx), py, C.c_int64(ldy), w))
        else:
            _ck(lib().sgm_mat_matmat_probe(self._h, C.c_int32(op), C.c_int32(kx), px, C.c_int64(ldx), py, C.c_int64(ldy),
                                           C.c_int32(block_cap), C.c_int32(grid_cap), w))
        return Y

    def matmat(self, X, Y):
        """Y = A X for a block of k vectors: column j of Y holds the bits matvec leaves for column j of X.  Blocks follow
        basis_rotate's convention: a numpy array of shape (n, k) in Fortran order, or a device tensor of shape (k, n) that
        holds the columns as contiguous rows."""
        return self._matmat(0, X, Y, "matmat")

    def matmat_add(self, X, Y):
        return self._matmat(OP_ADD, X, Y, "matmat_add")

    def matmat_t(self, X, Y):
        return self._matmat(OP_TRANS, X, Y, "matmat_t")

    def matmat_t_add(self, X, Y):
        return self._matmat(OP_TRANS | OP_ADD, X, Y, "matmat_t_add")

    def matmat_kernel(self, k, op=0):
        """What matmat would run for k columns, without running it (sgm_mat_matmat_kernel)."""
        if hasattr(self, "_build"):
            self._build()
        buf = C.create_string_buffer(512)
        _ck(lib().sgm_mat_matmat_kernel(self._h, C.c_int32(op), C.c_int32(k), buf, C.c_int(512)))
        return buf.value.decode()

    def halo_nbrs(self, part=0):
        """Exchange plan of local part `part` (parity checks): list of dicts with peer, send_count,
        recv_count, recv_offset and the send list (0-based local indices)."""
        n = C.c_int32(0)
        _ck(lib().sgm_mat_halo_nbr(self._h, C.c_int32(part), C.c_int32(-1), C.byref(n), None, None, None, None, None, C.c_int32(0)))
        out = []
        for k in range(n.value):
            pe, sc, rc, ro = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
            _ck(lib().sgm_mat_halo_nbr(self._h, C.c_int32(part), C.c_int32(k), None, C.byref(pe), C.byref(sc), C.byref(rc),
                                       C.byref(ro), None, C.c_int32(0)))
            idx = np.zeros(sc.value, np.int32)
            if sc.value:
                _ck(lib().sgm_mat_halo_nbr(self._h, C.c_int32(part), C.c_int32(k), None, None, None, None, None,
                                           C.c_void_p(idx.ctypes.data), C.c_int32(sc.value)))
            out.append({"peer": pe.value, "send_count": sc.value, "recv_count": rc.value, "recv_offset": ro.value,
                        "send_idx": idx})
        return out

    @property
    def x_len(self):
        n = C.c_int64(0)
        _ck(lib().sgm_mat_info(self._h, None, None, None, None, C.byref(n)))
        return n.value

    def footprint(self):
        """(resident_bytes, matvec_bytes): what the handle keeps in HBM, and what one y = A x moves by
        construction with the kernel the current options select (sgm_mat_footprint)."""
        if hasattr(self, "_build"):
            self._build()
        r, m = C.c_int64(0), C.c_int64(0)
        _ck(lib().sgm_mat_footprint(self._h, C.byref(r), C.byref(m)))
        return r.value, m.value

    # -- src/graph/permutations.f90 + cs_matrices.f90:471-490 -----------------------------
    def bfs_order(self):
        """breadth_first_search(p, g) on the matrix graph: p(i) = visiting number (1-based), -1 unreached."""
        p = np.zeros(self.nrow, np.int32)
        _ck(lib().sgm_graph_bfs_order(self._h, p.ctypes.data_as(C.c_void_p)))
        return p

    def greedy_coloring(self):
        """greedy_coloring(colors, g): returns (colors, num_colors)."""
        c = np.zeros(self.nrow, np.int32)
        nc = C.c_int32(0)
        _ck(lib().sgm_graph_greedy_coloring(self._h, c.ctypes.data_as(C.c_void_p), C.byref(nc)))
        return c, nc.value

    def greedy_color_ordering(self):
        """greedy_color_ordering(p, ptrs, num_colors, g): returns (p, ptrs[:num_colors+1], num_colors)."""
        p = np.zeros(self.nrow, np.int32)
        ptrs = np.zeros(self.nrow + 2, np.int32)
        nc = C.c_int32(0)
        _ck(lib().sgm_graph_greedy_color_order(self._h, p.ctypes.data_as(C.c_void_p), ptrs.ctypes.data_as(C.c_void_p),
                                               C.c_int32(len(ptrs)), C.byref(nc)))
        return p, ptrs[:nc.value + 1].copy(), nc.value

    def left_permute(self, p):
        pp, w, _k = _arg(p, np.int32)
        _ck(lib().sgm_mat_left_permute(self._h, pp, C.c_int(w)))

    def right_permute(self, p):
        pp, w, _k = _arg(p, np.int32)
        _ck(lib().sgm_mat_right_permute(self._h, pp, C.c_int(w)))

    def set_option(self, name, value):
        """sgm_mat_set_option: this matrix's own kernel-selection option (same bits whichever)."""
        if hasattr(self, "_build"):
            self._build()
        _ck(lib().sgm_mat_set_option(self._h, name.encode(), C.c_int(int(value))))
        return self

    @property
    def kernel(self):
        """Name of the SpMV kernel variant this matrix runs with under its options."""
        buf = C.create_string_buffer(64)
        _ck(lib().sgm_mat_kernel(self._h, buf, C.c_int(64)))
        return buf.value.decode()

    # -- linear_operator_interface.f90:213-280: A%solve facade ---------------------------
    def set_solver(self, solver):
        self.solver = solver
        solver.setup(self)

    def set_preconditioner(self, pc):
        self.pc = pc
        pc.setup(self)

    def solve(self, x, b):
        if self.solver is None:
            raise SigmaError(1, "A%solve: no solver set (linear_operator_interface.f90:213-233)")
        return self.solver.solve(self, x, b, self.pc)

    def get(self, name, dtype):
        """Read a leaf matrix back in the reference's layout (sgm_mat_get)."""
        need = C.c_size_t(0)
        _ck(lib().sgm_mat_get(self._h, name.encode(), None, C.c_size_t(0), C.byref(need)))
        out = np.zeros(need.value // np.dtype(dtype).itemsize, dtype)
        _ck(lib().sgm_mat_get(self._h, name.encode(), C.c_void_p(out.ctypes.data), C.c_size_t(out.nbytes), None))
        return out

    # -- sparse_matrix_interfaces.f90:106-128,378-460: editing the values in HBM (sgm_edit.hip) ------------
    def _triples(self, i, j, z=None):
        """(m, pi, pj, pz, where, keepalive): scalars or equal-length arrays = one ordered batch, all in one place"""
        if not (_is_torch(i) or _is_torch(j) or (z is not None and _is_torch(z))):
            i, j = np.atleast_1d(np.asarray(i, np.int32)), np.atleast_1d(np.asarray(j, np.int32))
            if z is not None:
                z = np.atleast_1d(np.asarray(z, np.float64))
        m = _len(i)
        if _len(j) != m or (z is not None and _len(z) != m):
            raise SigmaError(2, "a batch of entries needs i, j and z of the same length")
        pi, w1, k1 = _arg(i, np.int32)
        pj, w2, k2 = _arg(j, np.int32)
        if z is None:
            return m, pi, pj, None, _same_where(w1, w2), (k1, k2)
        pz, w3, k3 = _arg(z, np.float64)
        return m, pi, pj, pz, _same_where(w1, w2, w3), (k1, k2, k3)

    def set_value(self, i, j, z):
        """A%set_value(i, j, z) (cs_matrices.f90:840-863, ellpack_matrices.f90:444-470) for one entry or, with arrays, for
        t = 1..m in order: every stored slot of row i holding j gets z; the last triple wins (sgm_mat_set_entries)."""
        m, pi, pj, pz, w, _k = self._triples(i, j, z)
        _ck(lib().sgm_mat_set_entries(self._h, C.c_int64(m), pi, pj, pz, C.c_int(w)))

    def add_value(self, i, j, z):
        """A%add_value(i, j, z) (cs_matrices.f90:868-891) for one entry or an ordered batch: val = val + z in ascending t,
        every addition rounded on its own (sgm_mat_add_entries).  An entry outside the pattern is refused, nothing changes."""
        m, pi, pj, pz, w, _k = self._triples(i, j, z)
        _ck(lib().sgm_mat_add_entries(self._h, C.c_int64(m), pi, pj, pz, C.c_int(w)))

    def get_value(self, i, j):
        """A%get_value(i, j) (cs_matrices.f90:709-724): the last stored slot of row i holding j, +0.0 if there is none; a float
        for scalars, else an array (a device tensor when i, j are device tensors)."""
        scalar = np.isscalar(i) and np.isscalar(j)
        m, pi, pj, _z, w, _k = self._triples(i, j)
        if w == SGM_DEVICE:
            import torch
            out = torch.zeros(m, dtype=torch.float64, device=i.device)
        else:
            out = np.zeros(m)
        pz, _w, _k2 = _arg(out, np.float64, writable=True)
        _ck(lib().sgm_mat_get_entries(self._h, C.c_int64(m), pi, pj, pz, C.c_int(w)))
        return float(out[0]) if scalar else out

    def _multiple(self, is_, js, B):
        is_, js = np.asarray(is_, np.int32).reshape(-1), np.asarray(js, np.int32).reshape(-1)
        B = np.asarray(B.cpu() if _is_torch(B) else B, np.float64)
        if B.shape != (len(is_), len(js)):
            raise SigmaError(2, f"multiple values: B is {B.shape}, is / js have {len(is_)} / {len(js)} entries")
        return np.repeat(is_, len(js)), np.tile(js, len(is_)), np.ascontiguousarray(B).reshape(-1)      # rows outer

    def set_multiple_values(self, is_, js, B):
        """A%set_multiple_values(is, js, B): the batch for k in is: for l in js: (is(k), js(l), B(k,l))."""
        self.set_value(*self._multiple(is_, js, B))

    def add_multiple_values(self, is_, js, B):
        """A%add_multiple_values(is, js, B) (cs_matrices.f90:934-966, ellpack_matrices.f90:538-573): rows outer."""
        self.add_value(*self._multiple(is_, js, B))

    def add_sparse_matrix(self, B, alpha=None):
        """A%add_sparse_matrix(B [, alpha]) (sparse_matrix_interfaces.f90:430-460): B's stored entries in cursor order,
        z = alpha * B_ij rounded, added; B's pattern must lie inside A's (sgm_mat_add_matrix)."""
        a = None if alpha is None else C.byref(C.c_double(float(alpha)))
        _ck(lib().sgm_mat_add_matrix(self._h, B._h, a))

    def zero(self):
        """A%zero(): every stored slot 0.0, ELLPACK padding included (sgm_mat_zero)."""
        _ck(lib().sgm_mat_zero(self._h))

    def scalar_multiply(self, alpha):
        """A%scalar_multiply(alpha): val = alpha * val over every stored slot (sgm_mat_scalar_multiply)."""
        _ck(lib().sgm_mat_scalar_multiply(self._h, C.c_double(float(alpha))))

    @classmethod
    def from_edges(cls, nrow, ncol, ei, ej, ev):
        """Assemble on the device from an edge list in insertion order (1-based), like
        g%add_edge ... convert_graph_type ... A%set_value (sgm_csr/ell_from_edges)."""
        self = cls.__new__(cls)
        _Matrix.__init__(self)
        pi, w1, _k1 = _arg(ei, np.int32)
        pj, w2, _k2 = _arg(ej, np.int32)
        pv, w3, _k3 = _arg(ev, np.float64)
        ne = ei.numel() if _is_torch(ei) else len(ei)
        self.nrow, self.ncol = int(nrow), int(ncol)
        fn = lib().sgm_csr_from_edges if cls is csr_matrix else lib().sgm_ell_from_edges
        _ck(fn(C.byref(self._h), C.c_int32(nrow), C.c_int32(ncol), C.c_int64(ne), pi, pj, pv,
               C.c_int(_same_where(w1, w2, w3))))
        return self

    # -- sparse_matrix_to_file (sparse_matrix_interfaces.f90:601-653): text dump -----------
    def to_file(self, filename, trans=False):
        """`nrow ncol nnz`, then one `i j value` line per stored entry in stored order (rows in
        order, a row's entries as they lie in memory); `trans` swaps i/j and the dimensions like the
        reference.  Values are written with 17 significant digits (they read back bit for bit)."""
        if isinstance(self, ellpack_matrix):
            # the reference's edge cursor hands out the first degrees(i) slots of every row (ellpack_graphs.f90:310-369); a matrix
            # without degrees refuses here (get("degrees"))
            deg = self.get("degrees", np.int32)
            keep = np.arange(self.max_d)[None, :] < deg[:, None]
            node = self.get("node", np.int32).reshape(self.nrow, self.max_d)[keep]
            val = self.get("val", np.float64).reshape(self.nrow, self.max_d)[keep]
            ptr = np.concatenate([[0], np.cumsum(deg, dtype=np.int64)])
        elif isinstance(self, csr_matrix):
            ptr, node, val = self.get("ptr", np.int32), self.get("node", np.int32), self.get("val", np.float64)
        else:
            raise SigmaError(7, "to_file: CSR and ELLPACK matrices only")
        rows = np.repeat(np.arange(1, self.nrow + 1, dtype=np.int64), np.diff(ptr))
        a, b = (node, rows) if trans else (rows, node)
        dims = (self.ncol, self.nrow) if trans else (self.nrow, self.ncol)
        with open(filename, "w") as f:
            f.write(f" {dims[0]} {dims[1]} {len(val)}\n")
            f.writelines(f" {int(i)} {int(j)} {float(v)!r}\n" for i, j, v in zip(a, b, val))

    @classmethod
    def from_file(cls, filename):
        """Read a file written by to_file (or by the reference's A%to_file): the entries are
        inserted in file order, so a CSR matrix written and read back has identical arrays."""
        with open(filename) as f:
            nrow, ncol, nnz = (int(t) for t in f.readline().split())
            data = np.loadtxt(f, dtype=np.float64, ndmin=2) if nnz else np.zeros((0, 3))
        if data.shape[0] != nnz:
            raise SigmaError(2, f"from_file: header says {nnz} entries, file holds {data.shape[0]}")
        return cls.from_edges(nrow, ncol, data[:, 0].astype(np.int32), data[:, 1].astype(np.int32),
                              np.ascontiguousarray(data[:, 2]))

    def destroy(self):
        if self._h:
            _ck(lib().sgm_mat_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class csr_matrix(_Matrix):
    """csr_matrix (cs_matrices.f90:112-151): g%ptr(n+1), g%node(nnz), val(nnz), 1-based."""

    def __init__(self, nrow, ncol, ptr, node, val):
        super().__init__()
        pp, w1, _k1 = _arg(ptr, np.int32)
        pn, w2, _k2 = _arg(node, np.int32)
        pv, w3, _k3 = _arg(val, np.float64)
        self.nrow, self.ncol = int(nrow), int(ncol)
        self.nnz = int(len(val))
        _ck(lib().sgm_csr_create(C.byref(self._h), C.c_int32(nrow), C.c_int32(ncol), C.c_int64(self.nnz),
                                 pp, pn, pv, C.c_int(_same_where(w1, w2, w3))))

    def set_values(self, val):
        pv, w, _k = _arg(val, np.float64)
        _ck(lib().sgm_csr_set_values(self._h, pv, C.c_int(w)))


    # -- sparse_matrix_algebra.f90: the result of sparse_matrix_sum / sparse_matrix_product / PtAP / RARt ----
    def refill(self, X, Y):
        """Recompute only the values of this result from the operands' current values (sgm_mat_algebra_refill): X, Y are
        the handles it was built from, in the same order; none of the three may have been permuted since."""
        _ck(lib().sgm_mat_algebra_refill(self._h, X._h, Y._h))
        return self

    def algebra_rows(self):
        """(rows whose symbolic pass ran in LDS, rows that took the long-row path) of a matrix algebra result."""
        r = self.get("algebra_rows", np.int32)
        return int(r[0]), int(r[1])


class edit_plan:
    """sgm_edit_plan: a batch of entries (i, j) of A located and ordered once; .add(z) / .set(z) then take only new values
    (the same m values in the same order) -- re-assembly on a fixed mesh as one pass over A's values.  The plan belongs to A:
    another handle, or A after a permutation, is refused."""

    def __init__(self, A, i, j):
        self._h = C.c_void_p()
        self.A = A
        self.m, pi, pj, _z, w, _k = A._triples(i, j)
        _ck(lib().sgm_edit_plan_create(C.byref(self._h), A._h, C.c_int64(self.m), pi, pj, C.c_int(w)))

    def _apply(self, z, mode, zero_first, A=None):
        _need(z, self.m, "edit_plan values")
        pz, w, _k = _arg(z, np.float64)
        _ck(lib().sgm_edit_plan_apply(self._h, (A or self.A)._h, pz, C.c_int(mode), C.c_int(1 if zero_first else 0), C.c_int(w)))

    def add(self, z, zero_first=False, A=None):
        self._apply(z, 1, zero_first, A)

    def set(self, z, A=None):
        self._apply(z, 0, False, A)

    def info(self):
        """{m, slots addressed, longest chain, stored source indices incl. padding}"""
        out = (C.c_int64 * 4)()
        _ck(lib().sgm_edit_plan_info(self._h, out))
        return {"m": out[0], "slots": out[1], "longest_chain": out[2], "stored_sources": out[3]}

    def destroy(self):
        if self._h:
            _ck(lib().sgm_edit_plan_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def edit_locate_host(nrow, ncol, ptr, node, i, j):
    """sgm_edit_locate_host: the locate step of the edits as host-only index work on 1-based CSR arrays; returns
    (hit_off (m+1), hit_slot (1-based positions), first_missing (t, or 0))."""
    ptr, node = np.ascontiguousarray(ptr, np.int32), np.ascontiguousarray(node, np.int32)
    i, j = np.ascontiguousarray(i, np.int32), np.ascontiguousarray(j, np.int32)
    m = len(i)
    off = np.zeros(m + 1, np.int64)
    needed, miss = C.c_int64(0), C.c_int64(0)
    args = (C.c_int32(nrow), C.c_int32(ncol), C.c_void_p(ptr.ctypes.data), C.c_void_p(node.ctypes.data), C.c_int64(m),
            C.c_void_p(i.ctypes.data), C.c_void_p(j.ctypes.data), C.c_void_p(off.ctypes.data))
    _ck(lib().sgm_edit_locate_host(*args, None, C.c_int64(0), C.byref(needed), C.byref(miss)))
    slot = np.zeros(needed.value, np.int32)
    _ck(lib().sgm_edit_locate_host(*args, C.c_void_p(slot.ctypes.data), C.c_int64(len(slot)), C.byref(needed), C.byref(miss)))
    return off, slot, miss.value


def _algebra(fn, X, Y):
    M = csr_matrix.__new__(csr_matrix)
    _Matrix.__init__(M)
    _ck(fn(C.byref(M._h), X._h, Y._h))
    nr, nc, nnz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    _ck(lib().sgm_mat_info(M._h, C.byref(nr), C.byref(nc), C.byref(nnz), None, None))
    M.nrow, M.ncol, M.nnz = nr.value, nc.value, nnz.value
    return M


def sparse_matrix_sum(B, C_):
    """A = B + C (sparse_matrix_algebra.f90:25-145), bit-identical to the reference; a new csr_matrix."""
    return _algebra(lib().sgm_mat_sum, B, C_)


def sparse_matrix_product(B, C_):
    """A = B * C (sparse_matrix_algebra.f90:154-189 -> sparse_matrix_product_C :310-420); a new csr_matrix."""
    return _algebra(lib().sgm_mat_product, B, C_)


def PtAP(A, P):
    """B = P^T A P (sparse_matrix_algebra.f90:425-538); a new csr_matrix."""
    return _algebra(lib().sgm_mat_ptap, A, P)


def RARt(A, R):
    """B = R A R^T (sparse_matrix_algebra.f90:543-655); a new csr_matrix."""
    return _algebra(lib().sgm_mat_rart, A, R)


class partitioned_csr_matrix(_Matrix):
    """The multi-GPU row partition with all P row blocks on one GPU (test vehicle)."""

    def __init__(self, nrow, ncol, ptr, node, val, row_starts):
        super().__init__()
        ptr = np.ascontiguousarray(ptr, np.int32)
        node = np.ascontiguousarray(node, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        rs = np.ascontiguousarray(row_starts, np.int64)
        self.nrow, self.ncol, self.nnz = int(nrow), int(ncol), int(len(val))
        self.nparts = len(rs) - 1
        _ck(lib().sgm_csr_create_partitioned(C.byref(self._h), C.c_int32(len(rs) - 1), C.c_void_p(rs.ctypes.data),
                                             C.c_int32(nrow), C.c_int32(ncol), C.c_int64(self.nnz),
                                             C.c_void_p(ptr.ctypes.data), C.c_void_p(node.ctypes.data),
                                             C.c_void_p(val.ctypes.data)))


    @classmethod
    def from_parts(cls, row_starts, parts):
        """sgm_csr_create_partitioned_parts: the same in-process partition handed over part by part -- parts[k] =
        (ptr_local, node_global, val) of rows row_starts[k] .. row_starts[k+1]-1, numpy arrays or device tensors (all
        of one kind) -- for matrices too large to assemble whole on the host."""
        self = cls.__new__(cls)
        _Matrix.__init__(self)
        rs = np.ascontiguousarray(row_starts, np.int64)
        P = len(rs) - 1
        assert len(parts) == P
        keep, wheres = [], []
        pp, pn, pv = (C.c_void_p * P)(), (C.c_void_p * P)(), (C.c_void_p * P)()
        nnz = (C.c_int64 * P)()
        for k, (a, b, c) in enumerate(parts):
            p1, w1, k1 = _arg(a, np.int32)
            p2, w2, k2 = _arg(b, np.int32)
            p3, w3, k3 = _arg(c, np.float64)
            keep += [k1, k2, k3]
            wheres += [w1, w2, w3]
            pp[k], pn[k], pv[k] = p1, p2, p3
            nnz[k] = int(len(c))
        self.nrow = self.ncol = int(rs[-1])
        self.nparts = P
        self.nnz = int(sum(nnz))
        _ck(lib().sgm_csr_create_partitioned_parts(C.byref(self._h), C.c_int32(P), C.c_void_p(rs.ctypes.data), nnz, pp, pn, pv,
                                                   C.c_int(_same_where(*wheres))))
        return self


class dist_csr_matrix(_Matrix):
    """This rank's row block of a matrix partitioned over processes (RCCL).  col_starts: the partition of x when it
    is not the rows' (sgm_csr_create_dist_rect: an off-diagonal block of a composite)."""

    def __init__(self, comm, row_starts, ptr_local, node_global, val, col_starts=None):
        super().__init__()
        rs = np.ascontiguousarray(row_starts, np.int64)
        cs = rs if col_starts is None else np.ascontiguousarray(col_starts, np.int64)
        pp, w1, _k1 = _arg(ptr_local, np.int32)
        pn, w2, _k2 = _arg(node_global, np.int32)
        pv, w3, _k3 = _arg(val, np.float64)
        self.nrow, self.ncol = int(rs[-1]), int(cs[-1])
        self.n_local = int(rs[comm.rank + 1] - rs[comm.rank])
        self.nc_local = int(cs[comm.rank + 1] - cs[comm.rank])
        self.nnz = int(len(val))
        _ck(lib().sgm_csr_create_dist_rect(C.byref(self._h), comm._h, C.c_void_p(rs.ctypes.data), C.c_void_p(cs.ctypes.data),
                                           C.c_int64(self.nnz), pp, pn, pv, C.c_int(_same_where(w1, w2, w3))))


class dist_ellpack_matrix(_Matrix):
    """This rank's rows of an ELLPACK matrix partitioned over processes (sgm_ell_create_dist): node / val
    as C arrays of shape (n_local, max_d) = the reference's (max_d, n_local), GLOBAL 1-based columns; degrees: this rank's
    degrees(n_local), where node / val live (None: recovered from the padding, see ellpack_matrix)."""

    def __init__(self, comm, row_starts, node_global, val, degrees=None):
        super().__init__()
        rs = np.ascontiguousarray(row_starts, np.int64)
        max_d = int(node_global.shape[1])
        pn, w1, _k1 = _arg(node_global, np.int32)
        pv, w2, _k2 = _arg(val, np.float64)
        self.nrow = self.ncol = int(rs[-1])
        self.n_local = self.nc_local = int(rs[comm.rank + 1] - rs[comm.rank])
        self.max_d = max_d
        pd, w3, _k3 = (None, w1, None) if degrees is None else _arg(degrees, np.int32)
        _ck(lib().sgm_ell_create_dist(C.byref(self._h), comm._h, C.c_void_p(rs.ctypes.data), C.c_int32(max_d), pn, pv, pd,
                                      C.c_int(_same_where(w1, w2, w3))))


class sparse_matrix(_Matrix):
    """The composite "matrix of matrices" (sparse_matrix_composites.f90:41-162): row_ptr /
    col_ptr are the 1-based block offsets, set_submatrix(it, jt, B) places a leaf (1-based
    block indices); build() freezes the layout.  matvec_add loops over the blocks like
    composite_matvec_add (:1076-1099)."""

    def __init__(self, row_ptr, col_ptr):
        super().__init__()
        self.row_ptr = np.ascontiguousarray(row_ptr, np.int32)
        self.col_ptr = np.ascontiguousarray(col_ptr, np.int32)
        self.num_row_mats, self.num_col_mats = len(self.row_ptr) - 1, len(self.col_ptr) - 1
        self.nrow, self.ncol = int(self.row_ptr[-1] - 1), int(self.col_ptr[-1] - 1)
        self.sub_mats = [[None] * self.num_col_mats for _ in range(self.num_row_mats)]

    def set_submatrix(self, it, jt, B):
        self.sub_mats[it - 1][jt - 1] = B
        if self._h:
            self.destroy()

    def _build(self):
        if self._h:
            return
        arr = (C.c_void_p * (self.num_row_mats * self.num_col_mats))()
        for i, row in enumerate(self.sub_mats):
            for j, B in enumerate(row):
                arr[i * self.num_col_mats + j] = B._h if B is not None else None
        _ck(lib().sgm_composite_create(C.byref(self._h), C.c_int32(self.num_row_mats), C.c_int32(self.num_col_mats),
                                       C.c_void_p(self.row_ptr.ctypes.data), C.c_void_p(self.col_ptr.ctypes.data), arr))
        leaves = [B for row in self.sub_mats for B in row if B is not None]
        if leaves and hasattr(leaves[0], "n_local"):
            # over distributed leaves the vectors are this rank's slices of the block vectors, concatenated
            self.n_local = sum(next(B.n_local for B in row if B is not None) for row in self.sub_mats)
            self.nc_local = sum(next(self.sub_mats[i][j].nc_local for i in range(self.num_row_mats) if self.sub_mats[i][j] is not None)
                                for j in range(self.num_col_mats))

    def matvec(self, x, y):
        self._build()
        return super().matvec(x, y)

    def matvec_add(self, x, y):
        self._build()
        return super().matvec_add(x, y)

    def matvec_t(self, x, y):
        self._build()
        return super().matvec_t(x, y)

    def matvec_t_add(self, x, y):
        self._build()
        return super().matvec_t_add(x, y)


class ellpack_matrix(_Matrix):
    """ellpack_matrix (ellpack_matrices.f90:28-105): node(max_d,n), val(max_d,n) in Fortran
    order, i.e. a C array of shape (n, max_d); padding = last neighbour / 0.0.
    degrees: the graph's degrees(n) -- the first degrees(i) slots of row i are its entries (sgm_ell_set_degrees).  None: recovered
    from the padding for add_edge-shaped, all-zero and zero-padded rows; if any row has another shape the matrix holds no degrees,
    its products work and every reader of degrees raises SigmaError 8.  Arrays a delete_edge has touched need `degrees`
    (include/sigma_hip.h states why)."""

    def __init__(self, nrow, ncol, node, val, degrees=None):
        super().__init__()
        if _is_torch(node):
            max_d = int(node.shape[1])
        else:
            node = np.ascontiguousarray(node, np.int32)
            val = np.ascontiguousarray(val, np.float64)
            max_d = int(node.shape[1]) if node.ndim == 2 else int(node.size // max(nrow, 1))
        pn, w1, _k1 = _arg(node, np.int32)
        pv, w2, _k2 = _arg(val, np.float64)
        self.nrow, self.ncol, self.max_d = int(nrow), int(ncol), max_d
        _ck(lib().sgm_ell_create(C.byref(self._h), C.c_int32(nrow), C.c_int32(ncol), C.c_int32(max_d), pn, pv,
                                 C.c_int(_same_where(w1, w2))))
        if degrees is not None:
            try:
                self.set_degrees(degrees)
            except SigmaError:
                self.destroy()
                raise

    def set_degrees(self, degrees):
        """sgm_ell_set_degrees: degrees(nrow), checked (SigmaError 2 and the previous degrees kept on a violation); plans and
        derived matrices made before are refused or rebuilt afterwards."""
        if not _is_torch(degrees):
            degrees = np.ascontiguousarray(degrees, np.int32)
        if _len(degrees) != self.nrow:
            raise SigmaError(2, f"set_degrees: {_len(degrees)} degrees for {self.nrow} rows")
        pd, w, _k = _arg(degrees, np.int32)
        _ck(lib().sgm_ell_set_degrees(self._h, pd, C.c_int(w)))

    def set_values(self, val):
        pv, w, _k = _arg(val, np.float64)
        _ck(lib().sgm_ell_set_values(self._h, pv, C.c_int(w)))


# ------------------------------------------------------------------------------------ #
class _Preconditioner:
    """linear_solver used as a preconditioner (setup / solve / destroy)."""
    _kind = 0

    def __init__(self):
        self._h = C.c_void_p()
        self.nn = 0
        self.initialized = False
        self._opts = {}

    def setup(self, A):
        if hasattr(A, "_build"):
            A._build()
        if not self._h:
            # the factory (jacobi() / ldu()) has seen no matrix: options set before the first setup decide how it builds
            _ck(lib().sgm_pc_create(C.byref(self._h), C.c_int32(self._kind)))
            for k, v in self._opts.items():
                _ck(lib().sgm_pc_set_option(self._h, k.encode(), C.c_int(int(v))))
        _ck(lib().sgm_pc_setup(self._h, A._h))
        self.nn = getattr(A, "n_local", A.nrow)
        self.initialized = True

    def info(self, part=0):
        """sgm_pc_info: {"levels": (L, U), "path": 0..4, "colours": n, "est_us": per apply, "name": e.g. "strip pipeline,
        6323 levels"} -- whether an apply will be a dependency chain (natural-order ILDU of a grid) or a few bandwidth-bound
        sweeps (ldu(reorder="colour"))."""
        o = (C.c_int32 * 4)()
        us = C.c_double()
        nm = C.create_string_buffer(160)
        _ck(lib().sgm_pc_info(self._h, C.c_int32(part), o, C.byref(us), nm, C.c_int(160)))
        return {"levels": (int(o[0]), int(o[1])), "path": int(o[2]), "colours": int(o[3]), "est_us": float(us.value), "name": nm.value.decode()}

    def set_option(self, name, value):
        """sgm_pc_set_option: this preconditioner's own "ildu_strips" / "ildu_rows" / "pipeline_spin_limit"."""
        self._opts[name] = int(value)
        if self._h:
            _ck(lib().sgm_pc_set_option(self._h, name.encode(), C.c_int(int(value))))
        return self

    def solve(self, A, x, b):
        """pc%solve(A, x, b): x = M^-1 b."""
        _need(b, self.nn, "pc%solve b"); _need(x, self.nn, "pc%solve x")
        pb, wb, _k1 = _arg(b, np.float64)
        px, wx, _k2 = _arg(x, np.float64, writable=True)
        _ck(lib().sgm_pc_apply(self._h, pb, px, C.c_int(_same_where(wb, wx))))
        return x

    def get(self, name, dtype):
        need = C.c_size_t(0)
        _ck(lib().sgm_pc_get(self._h, name.encode(), None, C.c_size_t(0), C.byref(need)))
        out = np.zeros(need.value // np.dtype(dtype).itemsize, dtype)
        _ck(lib().sgm_pc_get(self._h, name.encode(), C.c_void_p(out.ctypes.data), C.c_size_t(out.nbytes), None))
        return out

    def destroy(self):
        if self._h:
            _ck(lib().sgm_pc_destroy(self._h))
            self._h = C.c_void_p()
        self.initialized = False

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class jacobi_solver(_Preconditioner):
    _kind = 1       # SGM_PC_JACOBI

    @property
    def idiag(self):
        return self.get("idiag", np.float64)


class sparse_ldu_solver(_Preconditioner):
    _kind = 2       # SGM_PC_ILDU0


def jacobi():
    """jacobi() factory (jacobi_solvers.f90:23-31)."""
    return jacobi_solver()


class _LevelMatrix(csr_matrix):
    """A level matrix of a multigrid preconditioner: a csr_matrix handle the preconditioner owns (destroy is a no-op)."""

    def destroy(self):
        self._h = C.c_void_p()


class multigrid_solver(_Preconditioner):
    """One V-cycle on Galerkin levels with damped Jacobi sweeps (sgm_mg_create; include/sigma_hip.h states the contract)."""
    _kind = 3       # SGM_PC_MG

    def __init__(self, P, omega, nu_pre, nu_post, coarse_sweeps, coarse="sweeps"):
        if coarse not in ("sweeps", "direct"):
            raise ValueError(f'multigrid: coarse is "sweeps" or "direct", not {coarse!r}')
        super().__init__()
        self.P = list(P)            # borrowed by the library: kept alive here
        hs = (C.c_void_p * max(len(self.P), 1))(*[p._h for p in self.P])
        _ck(lib().sgm_mg_create(C.byref(self._h), C.c_int32(len(self.P)), hs, C.c_double(float(omega)),
                                C.c_int32(int(nu_pre)), C.c_int32(int(nu_post)), C.c_int32(int(coarse_sweeps))))
        if coarse == "direct":
            self.set_option("mg_coarse_direct", 1)

    @property
    def levels(self):
        return len(self.P) + 1

    def level_handle(self, level):
        """A_level as a matrix object (level 0 = the caller's A); it belongs to the preconditioner."""
        M = _LevelMatrix.__new__(_LevelMatrix)
        _Matrix.__init__(M)
        _ck(lib().sgm_mg_level_matrix(self._h, C.c_int32(int(level)), C.byref(M._h)))
        nr, nc, nnz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _ck(lib().sgm_mat_info(M._h, C.byref(nr), C.byref(nc), C.byref(nnz), None, None))
        M.nrow, M.ncol, M.nnz = nr.value, nc.value, nnz.value
        return M

    def level_matrix(self, level):
        """(nrow, ncol, ptr, node, val) of A_level, 1-based like the reference."""
        M = self.level_handle(level)
        return M.nrow, M.ncol, M.get("ptr", np.int32), M.get("node", np.int32), M.get("val", np.float64)

    def paths(self):
        """per level: 1 = sweeps fused on the 4-bit sliced form, 2 = on the 1-byte sliced form, 0 = product + elementwise pass"""
        return self.get("mg_paths", np.int32)

    def idiag(self, level):
        return self.get(f"mg_idiag_{int(level)}", np.float64)

    def coarse_inverse(self):
        """the n x n inverse of the coarsest level (option "mg_coarse_direct" / coarse="direct"), as setup computed it"""
        a = self.get("mg_coarse_inverse", np.float64)
        n = int(round(np.sqrt(a.size)))
        return a.reshape(n, n)

    def coarse_pivots(self):
        """the pivot rows of that elimination, 1-based: piv[k] = the row swapped with row k + 1 at step k + 1"""
        return self.get("mg_coarse_pivots", np.int32)


def multigrid(P, omega=2.0 / 3.0, nu_pre=1, nu_post=1, coarse_sweeps=8, coarse="sweeps"):
    """V(nu_pre, nu_post) multigrid preconditioner on the Galerkin hierarchy of the prolongations P (a list of csr_matrix,
    P[l] of shape n_l x n_{l+1}; an empty list = the coarse sweeps on A alone): damped Jacobi sweeps with weight omega,
    coarse_sweeps of them on the last level.  An extension: the reference has PtAP "for multigrid setup" and no multigrid.
    Symmetric positive definite -- valid inside cg -- when nu_pre == nu_post, A is SPD and 0 < omega * lambda_max(D^-1 A) < 2
    (not checked).  coarse="direct": the last level (at most 4096 rows) is inverted at setup -- dense Gauss-Jordan with
    partial pivoting on the device -- and every V-cycle applies that inverse in place of the coarse sweeps."""
    return multigrid_solver(P, omega, nu_pre, nu_post, coarse_sweeps, coarse)


def aggregate(A, theta=0.08, device=False):
    """(agg, nagg): the aggregates of A's strength graph (sgm_mat_aggregate; include/sigma_hip.h states the contract) --
    agg[i] in 1..nagg for every row, a numpy array, or an int32 device tensor with device=True."""
    if hasattr(A, "_build"):
        A._build()
    n = int(A.nrow)
    if device:
        import torch
        agg = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda")
    else:
        agg = np.zeros(max(n, 1), np.int32)
    pa, w, _k = _arg(agg, np.int32, writable=True)
    nagg = C.c_int32(0)
    _ck(lib().sgm_mat_aggregate(A._h, C.c_double(float(theta)), pa, C.byref(nagg), C.c_int(w)))
    return agg[:n], nagg.value


def aggregation_hierarchy(A, theta=0.08, smooth_omega=2.0 / 3.0, max_levels=25, min_coarse=64):
    """The prolongations of a smoothed-aggregation hierarchy of A (sgm_mg_aggregation_hierarchy): a list of csr_matrix the
    caller owns, possibly empty; multigrid(aggregation_hierarchy(A)).setup(A) is the preconditioner built from A alone."""
    if hasattr(A, "_build"):
        A._build()
    slots = max(int(max_levels) - 1, 1)
    hs = (C.c_void_p * slots)()
    made = C.c_int32(0)
    _ck(lib().sgm_mg_aggregation_hierarchy(A._h, C.c_double(float(theta)), C.c_double(float(smooth_omega)),
                                           C.c_int32(int(max_levels)), C.c_int32(int(min_coarse)), hs, C.byref(made)))
    out = []
    for l in range(made.value):
        M = csr_matrix.__new__(csr_matrix)
        _Matrix.__init__(M)
        M._h = C.c_void_p(hs[l])
        nr, nc, nnz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        _ck(lib().sgm_mat_info(M._h, C.byref(nr), C.byref(nc), C.byref(nnz), None, None))
        M.nrow, M.ncol, M.nnz = nr.value, nc.value, nnz.value
        out.append(M)
    return out


def ldu(incomplete=True, level=0, reorder=None):
    """ldu(incomplete, level) factory (ldu_solvers.f90:73-86).  Like the reference
    (ldu_set_params :143-151) the arguments are accepted and forced to ILDU(0).
    reorder="colour" (an extension, off by default): ILDU(0) of the colour-ordered matrix P A P^T -- P = the reference's
    greedy_color_ordering of A's graph -- applied as z = P^T M^-1 P r; A, b and x stay as the caller holds them."""
    pc = sparse_ldu_solver()
    if reorder in ("colour", "color"):
        pc.set_option("ildu_reorder", 1)
    elif reorder not in (None, "natural"):
        raise SigmaError(1, f"ldu: reorder is None or 'colour', not {reorder!r}")
    return pc


class _Solver:
    """linear_solver (linear_operator_interface.f90:61-73)."""

    def __init__(self, tolerance):
        self._h = C.c_void_p()
        self.tolerance = 1.0e-16 if tolerance is None else float(tolerance)   # cg_solvers.f90:106
        self.nn = 0
        self.initialized = False
        self._max_iter = 0
        self._hist = 0
        self._opts = {}

    def _create(self):
        raise NotImplementedError

    def set_option(self, name, value):
        """sgm_solver_set_option: this solver's own "cg_small" / "bicgstab_small" / "krylov_graph" / "dot_order" (CG, BiCGStab,
        MINRES, LSQR) / "gmres_cgs2" (read at the next solve)."""
        self._opts[name] = int(value)
        if self._h:
            _ck(lib().sgm_solver_set_option(self._h, name.encode(), C.c_int(int(value))))
        return self

    def setup(self, A):
        if hasattr(A, "_build"):
            A._build()
        if not self._h:
            self._create()
            if self._max_iter:
                _ck(lib().sgm_solver_set_max_iter(self._h, C.c_int64(self._max_iter)))
            if self._hist:
                _ck(lib().sgm_solver_set_history(self._h, C.c_int64(self._hist)))
            for k, v in self._opts.items():
                _ck(lib().sgm_solver_set_option(self._h, k.encode(), C.c_int(int(v))))
        _ck(lib().sgm_solver_setup(self._h, A._h))
        self.nn = A.nrow
        self.initialized = True

    def set_params(self, tolerance=None):
        """solver%set_params(tolerance) (cg_solvers.f90:95-111): without an argument the tolerance goes back to 1e-16."""
        self.tolerance = 1.0e-16 if tolerance is None else float(tolerance)
        return self

    def set_max_iter(self, max_iter):
        """Extension: the reference has no iteration cap.  <= 0 = unbounded."""
        self._max_iter = int(max_iter)
        if self._h:
            _ck(lib().sgm_solver_set_max_iter(self._h, C.c_int64(self._max_iter)))

    def set_history(self, capacity):
        self._hist = int(capacity)
        if self._h:
            _ck(lib().sgm_solver_set_history(self._h, C.c_int64(self._hist)))

    def solve(self, A, x, b, pc=None, check=True):
        """solver%solve(A, x, b[, pc]): x holds the initial guess on entry, the solution on
        exit.  With set_max_iter, hitting the cap raises unless check=False."""
        nloc = getattr(A, "n_local", A.nrow)
        _need(x, nloc, "solve x"); _need(b, nloc, "solve b")
        px, wx, _k1 = _arg(x, np.float64, writable=True)
        pb, wb, _k2 = _arg(b, np.float64)
        # solver.tolerance is a live public field, read at every solve like cg_solvers.f90:133
        _ck(lib().sgm_solver_set_tolerance(self._h, C.c_double(float(self.tolerance))))
        rc = lib().sgm_solver_solve(self._h, A._h, px, pb, pc._h if pc is not None else None,
                                    C.c_int(_same_where(wx, wb)))
        if rc == 5 and not check:
            return x
        _ck(rc)
        return x

    def _info(self):
        it, last = C.c_int64(0), C.c_int64(0)
        r, cv = C.c_double(0.0), C.c_int32(0)
        _ck(lib().sgm_solver_info(self._h, C.byref(it), C.byref(r), C.byref(cv), C.byref(last)))
        return it.value, r.value, cv.value, last.value

    @property
    def iterations(self):
        return self._info()[0] if self._h else 0

    @property
    def last_iterations(self):
        return self._info()[3]

    @property
    def res2(self):
        return self._info()[1]

    @property
    def converged(self):
        return bool(self._info()[2])

    @property
    def history(self):
        cnt = C.c_int64(0)
        _ck(lib().sgm_solver_get_history(self._h, None, C.c_int64(0), C.byref(cnt)))
        out = np.zeros(cnt.value, np.float64)
        if cnt.value:
            _ck(lib().sgm_solver_get_history(self._h, C.c_void_p(out.ctypes.data), C.c_int64(cnt.value), None))
        return out

    def destroy(self):
        if self._h:
            _ck(lib().sgm_solver_destroy(self._h))
            self._h = C.c_void_p()
        self.initialized = False

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class cg_solver(_Solver):
    def _create(self):
        _ck(lib().sgm_cg_create(C.byref(self._h), C.c_double(self.tolerance)))


class bicgstab_solver(_Solver):
    def _create(self):
        _ck(lib().sgm_bicgstab_create(C.byref(self._h), C.c_double(self.tolerance)))


class gmres_solver(_Solver):
    def __init__(self, tolerance, restart):
        super().__init__(tolerance)
        self.restart = int(restart)

    def _create(self):
        _ck(lib().sgm_gmres_create(C.byref(self._h), C.c_double(self.tolerance), C.c_int32(self.restart)))


class minres_solver(_Solver):
    def _create(self):
        _ck(lib().sgm_minres_create(C.byref(self._h), C.c_double(self.tolerance)))


class lsqr_solver(_Solver):
    """LSQR (sgm_lsqr_create): x has A.ncol entries, b has A.nrow; tolerance, normal_tolerance and damp are live fields, sent
    before every solve."""

    def __init__(self, tolerance, normal_tolerance, damp):
        super().__init__(tolerance)
        self.normal_tolerance = self.tolerance if normal_tolerance is None else float(normal_tolerance)
        self.damp = float(damp)

    def _create(self):
        _ck(lib().sgm_lsqr_create(C.byref(self._h), C.c_double(self.tolerance), C.c_double(self.normal_tolerance),
                                  C.c_double(self.damp)))

    def set_params(self, tolerance=None, normal_tolerance=None, damp=0.0):
        """Without arguments: tolerance = normal_tolerance = 1e-16, damp = 0."""
        super().set_params(tolerance)
        self.normal_tolerance = self.tolerance if normal_tolerance is None else float(normal_tolerance)
        self.damp = float(damp)
        return self

    def solve(self, A, x, b, pc=None, check=True):
        """min |A x - b|_2 (damped: the correction to the initial guess, see sgm_lsqr_create): x holds the initial guess on
        entry, the solution on exit.  With set_max_iter, hitting the cap raises unless check=False.  `pc` is there for the
        signature of the other solvers only: the library refuses a preconditioner (SigmaError 8)."""
        _need(x, A.ncol, "lsqr solve x"); _need(b, A.nrow, "lsqr solve b")
        px, wx, _k1 = _arg(x, np.float64, writable=True)
        pb, wb, _k2 = _arg(b, np.float64)
        _ck(lib().sgm_solver_set_tolerance(self._h, C.c_double(float(self.tolerance))))
        _ck(lib().sgm_lsqr_set_params(self._h, C.c_double(float(self.normal_tolerance)), C.c_double(float(self.damp))))
        rc = lib().sgm_solver_solve(self._h, A._h, px, pb, pc._h if pc is not None else None, C.c_int(_same_where(wx, wb)))
        if rc == 5 and not check:
            return x
        _ck(rc)
        return x

    def _lsqr_info(self):
        stop, rn, arn = C.c_int32(0), C.c_double(0.0), C.c_double(0.0)
        _ck(lib().sgm_lsqr_info(self._h, C.byref(stop), C.byref(rn), C.byref(arn)))
        return stop.value, rn.value, arn.value

    @property
    def stop(self):
        """why the last solve ended: 1 rnorm <= tolerance, 2 arnorm <= normal_tolerance, 0 the iteration cap, 3 a NaN"""
        return self._lsqr_info()[0]

    @property
    def rnorm(self):
        return self._lsqr_info()[1]

    @property
    def arnorm(self):
        return self._lsqr_info()[2]


def cg(tolerance=None):
    """cg(tolerance) factory (cg_solvers.f90:36-47); default tolerance 1e-16 (:106)."""
    return cg_solver(tolerance)


def bicgstab(tolerance=None):
    """bicgstab(tolerance) factory (bicgstab_solvers.f90:37-48)."""
    return bicgstab_solver(tolerance)


def gmres(tolerance=None, restart=30):
    """GMRES(restart).  Not in the reference; conventions follow cg."""
    return gmres_solver(tolerance, restart)


def minres(tolerance=1e-16):
    """Preconditioned MINRES (Paige-Saunders) for symmetric A, definite or not, and a symmetric positive definite
    preconditioner (sgm_minres_create; include/sigma_hip.h states the contract).  Not in the reference; conventions follow cg,
    except that the history holds |phibar| = sqrt(res2).  Single-GPU csr_matrix, ellpack_matrix and sparse_matrix operands;
    with set_option("dot_order", 1) the whole solve is pinned bit for bit.  A step that cannot be finished (the preconditioner
    is not positive definite, a NaN) ends the solve without raising: `converged` is then False."""
    return minres_solver(tolerance)


def lsqr(tolerance=1e-16, normal_tolerance=None, damp=0.0):
    """LSQR (Paige-Saunders) for min |A x - b|_2 with a rectangular A of any shape and rank, optionally Tikhonov-damped
    (sgm_lsqr_create; include/sigma_hip.h states the contract).  Not in the reference.  Two ABSOLUTE tolerances: `tolerance` on
    the residual norm estimate (stop 1: a compatible system is solved), `normal_tolerance` on the estimate of |A^T r|_2 (stop 2:
    the least-squares solution); None = the value of `tolerance`.  From x = 0 the solution is the minimum-norm one.  Single-GPU
    csr_matrix and ellpack_matrix operands, no preconditioner; the history holds rnorm = sqrt(res2); with
    set_option("dot_order", 1) the whole solve is pinned bit for bit.  A NaN ends the solve without raising (stop 3).
    The cached transpose inherits A's kernel options: on a grid-like operand A.set_option("ell_colblock", 0) before setup keeps
    its product on the row kernels (profiles/lsqr/ measures the difference)."""
    return lsqr_solver(tolerance, normal_tolerance, damp)


# ------------------------------------------------------------------------------------ #
class Comm:
    """RCCL communicator for the row partition (one process per GPU)."""

    def __init__(self, rank, nranks, unique_id, halo_unique_id=None):
        self._h = C.c_void_p()
        self.rank, self.nranks = int(rank), int(nranks)
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        _ck(lib().sgm_comm_init(C.byref(self._h), C.c_int(rank), C.c_int(nranks), buf))
        if halo_unique_id is not None:        # a second communicator for the halo send / recv pairs
            buf2 = (C.c_char * 128).from_buffer_copy(bytes(halo_unique_id))
            _ck(lib().sgm_comm_attach_halo_comm(self._h, buf2))

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        _ck(lib().sgm_comm_unique_id(buf))
        return bytes(buf)

    def group_selftest(self):
        """sgm_comm_group_selftest: one group of send / recv (to itself) + all-reduce on this communicator's transport;
        returns (delivered, allreduced, microseconds) -- delivered must be 42 + rank, allreduced nranks."""
        out = (C.c_double * 3)()
        _ck(lib().sgm_comm_group_selftest(self._h, out))
        return float(out[0]), float(out[1]), float(out[2])

    @property
    def group_ok(self):
        """sgm_comm_group_ok: did this transport take the probe group of sgm_comm_init (pairs + all-reduce in one group)?"""
        return bool(lib().sgm_comm_group_ok(self._h))

    def destroy(self):
        if self._h:
            _ck(lib().sgm_comm_destroy(self._h))
            self._h = C.c_void_p()


DIST_PHASES = ("halo_post_to_done", "interior_rows", "halo_wait_exposed", "boundary_rows", "dot_reduce_kernels", "allreduce")


def dist_profile(on):
    """Switch the phase timers of the row-partitioned path on / off (and clear them)."""
    _ck(lib().sgm_dist_profile(C.c_int(1 if on else 0)))


def dist_profile_read():
    """{phase: {"ms": total, "count": spans}} since the last read (synchronises the library's streams)."""
    ms = (C.c_double * 6)()
    cnt = (C.c_int64 * 6)()
    _ck(lib().sgm_dist_profile_read(ms, cnt))
    return {nm: {"ms": float(ms[k]), "count": int(cnt[k])} for k, nm in enumerate(DIST_PHASES)}


def lanczos(A, nsteps, q1, want_Q=True):
    """lanczos(A, T, Q) (src/eigensolver.f90:27-90) on the device with the start vector q1:
    returns (T[3, nsteps], Q[n, nsteps] or None).  The eigenvalues of the tridiagonal
    (diag T[1], off-diagonal T[2][:-1]) are what eigensolve :160-208 gets from dstev.
    A may be row-partitioned: an in-process partition takes and returns global vectors, a rank of a matrix distributed
    over processes its owned slice of q1 and of Q (T is the same on every rank)."""
    if hasattr(A, "_build"):
        A._build()
    pq, w, _k = _arg(q1, np.float64)
    nloc = getattr(A, "n_local", A.nrow)          # a rank of a distributed matrix works on its owned slice
    _need(q1, nloc, "lanczos q1")
    T = np.zeros((nsteps, 3), np.float64)
    Q = np.zeros((nsteps, nloc), np.float64) if want_Q else None
    if w != SGM_HOST:
        raise TypeError("lanczos: pass the start vector as a numpy array")
    _ck(lib().sgm_lanczos(A._h, C.c_int32(nsteps), pq, C.c_void_p(T.ctypes.data),
                          C.c_void_p(Q.ctypes.data) if want_Q else None, C.c_int(SGM_HOST)))
    return T.T.copy(), (Q.T.copy() if want_Q else None)


def generalized_lanczos(A, B, nsteps, q1, want_Q=True):
    """generalized_lanczos(A, B, T, Q) (src/eigensolver.f90:95-155) on the device: Lanczos for
    A x = lambda B x with the start vector q1.  Like the reference it uses the solver (and
    preconditioner) set on B with B.set_solver / B.set_preconditioner for the per-step solve
    `B%solve(w, v)`.  Returns (T[3, nsteps], Q[n, nsteps] or None)."""
    for M in (A, B):
        if hasattr(M, "_build"):
            M._build()
    if B.solver is None:
        raise SigmaError(1, "generalized_lanczos: B has no solver set (eigensolver.f90:101-103 assumes B%set_solver)")
    pq, w, _k = _arg(q1, np.float64)
    if w != SGM_HOST:
        raise TypeError("generalized_lanczos: pass the start vector as a numpy array")
    nloc = getattr(A, "n_local", A.nrow)
    _need(q1, nloc, "generalized_lanczos q1")
    T = np.zeros((nsteps, 3), np.float64)
    Q = np.zeros((nsteps, nloc), np.float64) if want_Q else None
    _ck(lib().sgm_solver_set_tolerance(B.solver._h, C.c_double(float(B.solver.tolerance))))
    _ck(lib().sgm_generalized_lanczos(A._h, B._h, B.solver._h, B.pc._h if B.pc is not None else None, C.c_int32(nsteps), pq,
                                      C.c_void_p(T.ctypes.data), C.c_void_p(Q.ctypes.data) if want_Q else None,
                                      C.c_int(SGM_HOST)))
    return T.T.copy(), (Q.T.copy() if want_Q else None)


def _ritz(T, Q, normalise_sign):
    """The LAPACK tail of eigensolve (src/eigensolver.f90:174-186): dstev('V') on the tridiagonal, V = Q Z.
    Host side (scipy's LAPACK), like the reference's."""
    from scipy.linalg import eigh_tridiagonal
    lam, Z = eigh_tridiagonal(T[1], T[2][:-1])
    V = Q @ Z
    if normalise_sign:                                   # V(:,i) = V(1,i) / |V(1,i)| * V(:,i)   (:182-184)
        V = V * (V[0] / np.abs(V[0]))
    return lam, V


def eigensolve(A, n, q1):
    """eigensolve(A, lambda, V) (src/eigensolver.f90:160-188): n Lanczos steps on the device, the
    tridiagonal eigenproblem on the host.  Returns (lambda[n] ascending, V[nrow, n])."""
    T, Q = lanczos(A, n, q1)
    return _ritz(T, Q, True)


def generalized_eigensolve(A, B, n, q1):
    """generalized_eigensolve(A, B, lambda, V) (src/eigensolver.f90:193-208); B needs a solver set."""
    T, Q = generalized_lanczos(A, B, n, q1)
    return _ritz(T, Q, False)


class EigshResult:
    """What eigsh returns: lam[k], V[n, k] (or None), residuals[k] (the TRUE |A v - lam v|_2), restarts, products, found,
    converged.  Entries from `found` on are NaN (lam, residuals) / zero columns (V)."""

    def __init__(self, lam, V, residuals, restarts, products, found, converged):
        self.lam, self.V, self.residuals = lam, V, residuals
        self.restarts, self.products, self.found, self.converged = restarts, products, found, converged

    def __repr__(self):
        return (f"EigshResult(lam={self.lam!r}, residuals={self.residuals!r}, restarts={self.restarts}, products={self.products}, "
                f"found={self.found}, converged={self.converged})")


def eigsh_start_vector(n):
    """The start vector eigsh uses when none is given: 1 + ((i * 2654435761) mod 1024) / 1024, i = 0 .. n-1 -- exact in
    float64, the same on every run, not an RNG."""
    i = np.arange(n, dtype=np.uint64)
    return 1.0 + ((i * np.uint64(2654435761)) % np.uint64(1024)).astype(np.float64) / 1024.0


def eigsh(A, k, which="SA", ncv=None, tol=1e-8, max_restarts=200, q1=None, want_V=True):
    """sgm_eigsh: the k smallest ("SA") or largest ("LA") algebraic eigenvalues of the symmetric matrix A and their
    eigenvectors by thick-restart Lanczos on the device (the contract: include/sigma_hip.h).  Convergence is decided by the
    Lanczos estimate rho <= tol * anorm; `residuals` are the true residual norms.  ncv defaults to min(n - 1, max(2k + 1, 20)).
    V is a numpy array when q1 is one (or None), a device tensor when q1 is a device tensor."""
    if hasattr(A, "_build"):
        A._build()
    if which not in ("SA", "LA"):
        raise SigmaError(1, f"eigsh: which must be 'SA' or 'LA', not {which!r}")
    n = A.nrow
    if ncv is None:
        ncv = min(n - 1, max(2 * k + 1, 20))
    if q1 is None:
        q1 = eigsh_start_vector(n)
    pq, w, _k = _arg(q1, np.float64)
    _need(q1, n, "eigsh q1")
    kk = max(int(k), 1)
    lam = np.zeros(kk, np.float64)
    res = np.zeros(kk, np.float64)
    info = np.zeros(4, np.int64)
    V = pv = None
    if want_V:
        if w == SGM_DEVICE:
            import torch
            V = torch.zeros((kk, n), dtype=torch.float64, device=q1.device)
            pv = C.c_void_p(V.data_ptr())
        else:
            V = np.zeros((kk, n), np.float64)
            pv = C.c_void_p(V.ctypes.data)
    _ck(lib().sgm_eigsh(A._h, C.c_int32(int(k)), C.c_int32(int(ncv)), C.c_int32(1 if which == "LA" else 0), C.c_double(float(tol)),
                        C.c_int32(int(max_restarts)), pq, C.c_void_p(lam.ctypes.data), pv, C.c_void_p(res.ctypes.data),
                        C.c_void_p(info.ctypes.data), C.c_int(w)))
    if want_V:
        V = V.T if w == SGM_DEVICE else V.T.copy()
    return EigshResult(lam, V, res, int(info[0]), int(info[1]), int(info[2]), bool(info[3]))


class DavidsonResult(EigshResult):
    """What davidson returns: EigshResult's fields with `steps` (expansions of the search space) and `applies` (of the
    preconditioner; 0 without one) added, and `products_B` (products with the mass matrix; 0 without one)."""

    def __init__(self, lam, V, residuals, steps, products, applies, restarts, found, converged, products_B=0):
        super().__init__(lam, V, residuals, restarts, products, found, converged)
        self.steps, self.applies, self.products_B = steps, applies, products_B

    def __repr__(self):
        return (f"DavidsonResult(lam={self.lam!r}, residuals={self.residuals!r}, steps={self.steps}, products={self.products}, "
                f"applies={self.applies}, restarts={self.restarts}, found={self.found}, converged={self.converged}, "
                f"products_B={self.products_B})")


def davidson(A, k, pc=None, ncv=None, tol=1e-8, max_steps=1000, q1=None, want_V=True, B=None):
    """sgm_davidson: the k smallest algebraic eigenvalues of the symmetric matrix A and their eigenvectors by the generalized
    Davidson method with thick restart on the device (the contract: include/sigma_hip.h).  pc: a preconditioner that has been
    set up on A (jacobi(), ldu(), multigrid(...)), or None; with a V-cycle the step count does not grow with the grid.  A pair
    counts as converged when the residual the two bases give is <= tol * anorm; `residuals` are the true residual norms.
    ncv defaults to min(n - 1, max(2k + 1, 20)).  V is a numpy array when q1 is one (or None), a device tensor when q1 is a
    device tensor.
    B (a symmetric positive definite matrix of A's size, any single-GPU format): sgm_davidson_gen -- the k smallest eigenvalues
    of A x = lam B x with V^T B V = I, one product with B per step and no solve with it; a pair counts as converged when
    |W z - theta U z| <= tol * anorm * |U z| (U = B V), `residuals` are the true |A v - lam B v|_2, `products_B` counts the
    products with B.  pc stays a preconditioner set up on A."""
    if hasattr(A, "_build"):
        A._build()
    if pc is not None and not isinstance(pc, _Preconditioner):
        raise SigmaError(1, f"davidson: pc must be a preconditioner (jacobi(), ldu(), multigrid(..)) or None, not {type(pc).__name__}")
    if pc is not None and not pc._h:
        raise SigmaError(1, "davidson: the preconditioner has not been set up (pc.setup(A))")
    n = A.nrow
    if B is not None:
        if not isinstance(B, _Matrix):
            raise SigmaError(1, f"davidson: B must be a matrix (csr_matrix, ellpack_matrix, sparse_matrix) or None, not {type(B).__name__}")
        if hasattr(B, "_build"):
            B._build()
        if (B.nrow, B.ncol) != (n, n):
            raise SigmaError(2, f"davidson: B is {B.nrow} x {B.ncol}, A has {n} rows")
    if ncv is None:
        ncv = min(n - 1, max(2 * int(k) + 1, 20))
    if q1 is None:
        q1 = eigsh_start_vector(n)
    pq, w, _k = _arg(q1, np.float64)
    _need(q1, n, "davidson q1")
    kk = max(int(k), 1)
    lam = np.zeros(kk, np.float64)
    res = np.zeros(kk, np.float64)
    info = np.zeros(7, np.int64)
    V = pv = None
    if want_V:
        if w == SGM_DEVICE:
            import torch
            V = torch.zeros((kk, n), dtype=torch.float64, device=q1.device)
            pv = C.c_void_p(V.data_ptr())
        else:
            V = np.zeros((kk, n), np.float64)
            pv = C.c_void_p(V.ctypes.data)
    tail = (C.c_int32(int(k)), C.c_int32(int(ncv)), C.c_double(float(tol)), C.c_int32(int(max_steps)), pq, C.c_void_p(lam.ctypes.data),
            pv, C.c_void_p(res.ctypes.data), C.c_void_p(info.ctypes.data), C.c_int(w))
    hp = pc._h if pc is not None else None
    if B is None:
        _ck(lib().sgm_davidson(A._h, hp, *tail))
        steps, products, applies, restarts, found, converged = (int(x) for x in info[:6])
        products_B = 0
    else:
        _ck(lib().sgm_davidson_gen(A._h, B._h, hp, *tail))
        steps, products, products_B, applies, restarts, found, converged = (int(x) for x in info)
    if want_V:
        V = V.T if w == SGM_DEVICE else V.T.copy()
    return DavidsonResult(lam, V, res, steps, products, applies, restarts, found, bool(converged), products_B)


def symeig_host(H):
    """sgm_symeig_host: all eigenpairs of a small dense symmetric matrix by cyclic Jacobi, on the host (no GPU needed).
    Returns (theta[m] in the order Jacobi leaves them, Z[m, m] with H Z = Z diag(theta), sweeps)."""
    H = np.asarray(H, np.float64)
    m = H.shape[0]
    if H.ndim != 2 or H.shape[1] != m:
        raise SigmaError(2, "symeig_host: H must be a square matrix")
    Hf = np.asfortranarray(H)
    theta = np.zeros(m, np.float64)
    Z = np.zeros((m, m), np.float64, order="F")
    sweeps = C.c_int32(0)
    _ck(lib().sgm_symeig_host(C.c_int32(m), C.c_void_p(Hf.ctypes.data), C.c_void_p(theta.ctypes.data), C.c_void_p(Z.ctypes.data),
                              C.byref(sweeps)))
    return theta, Z, int(sweeps.value)


def basis_rotate(Q, Z):
    """sgm_basis_rotate: Q[:, 0:kk] <- Q[:, 0:m] Z on the device, Z (m x kk) a numpy array.  Q: a numpy array of shape (n, m) --
    a rotated copy's first kk columns are returned -- or a device tensor of shape (m, n) holding the columns as contiguous
    rows, rotated in place (its first kk rows are returned)."""
    Z = np.asfortranarray(np.asarray(Z, np.float64))
    m, kk = Z.shape
    if _is_torch(Q) and Q.is_cuda:
        if Q.dim() != 2 or Q.shape[0] != m:
            raise SigmaError(2, f"basis_rotate: a device Q holds its columns as rows: shape ({m}, n) expected")
        pq, w, _k = _arg(Q, np.float64)
        n = int(Q.shape[1])
        _ck(lib().sgm_basis_rotate(C.c_int64(n), C.c_int32(m), C.c_int32(kk), pq, C.c_int64(n), C.c_void_p(Z.ctypes.data), C.c_int(w)))
        return Q[:kk]
    Qf = np.array(Q, np.float64, order="F")
    if Qf.ndim != 2 or Qf.shape[1] != m:
        raise SigmaError(2, f"basis_rotate: Q must have shape (n, {m})")
    n = Qf.shape[0]
    _ck(lib().sgm_basis_rotate(C.c_int64(n), C.c_int32(m), C.c_int32(kk), C.c_void_p(Qf.ctypes.data), C.c_int64(n),
                               C.c_void_p(Z.ctypes.data), C.c_int(SGM_HOST)))
    return Qf[:, :kk].copy()


def halo_plan_host(n_own, col_begin, node_global):
    """Host-only index work of the row partition (no GPU needed): returns
    (node_local 1-based, halo_cols sorted unique global 1-based)."""
    node = np.ascontiguousarray(node_global, np.int32)
    out = np.zeros(len(node), np.int32)
    halo = np.zeros(max(len(node), 1), np.int32)
    nh = C.c_int32(0)
    _ck(lib().sgm_halo_plan_host(C.c_int32(n_own), C.c_int64(col_begin), C.c_int64(len(node)),
                                 C.c_void_p(node.ctypes.data), C.c_void_p(out.ctypes.data),
                                 C.c_void_p(halo.ctypes.data), C.byref(nh)))
    return out, halo[:nh.value].copy()


def dist_plan_host(rank, nranks, row_starts, halo_cols):
    """sgm_dist_plan_host (no GPU needed): (want[nranks], want_off[nranks+1], req[len(halo)])."""
    rs = np.ascontiguousarray(row_starts, np.int64)
    halo = np.ascontiguousarray(halo_cols, np.int32)
    want, off, req = np.zeros(nranks, np.int32), np.zeros(nranks + 1, np.int32), np.zeros(max(len(halo), 1), np.int32)
    _ck(lib().sgm_dist_plan_host(C.c_int32(rank), C.c_int32(nranks), C.c_void_p(rs.ctypes.data), C.c_int32(len(halo)),
                                 C.c_void_p(halo.ctypes.data), C.c_void_p(want.ctypes.data), C.c_void_p(off.ctypes.data),
                                 C.c_void_p(req.ctypes.data)))
    return want, off, req[:len(halo)].copy()


def dist_neighbors_host(rank, nranks, want_all):
    """sgm_dist_neighbors_host: list of (peer, send_count, recv_count, recv_offset) from the
    all-gathered want matrix (row q = rank q's want)."""
    wa = np.ascontiguousarray(want_all, np.int32).reshape(nranks, nranks)
    arr = [np.zeros(max(nranks, 1), np.int32) for _ in range(4)]
    n = C.c_int32(0)
    _ck(lib().sgm_dist_neighbors_host(C.c_int32(rank), C.c_int32(nranks), C.c_void_p(wa.ctypes.data),
                                      *[C.c_void_p(a.ctypes.data) for a in arr], C.byref(n)))
    return [tuple(int(a[i]) for a in arr) for i in range(n.value)]


def partition_links_host(row_starts, ptr, node):
    """sgm_partition_links_host: the (sender, receiver, recv_offset, send list) links that
    sgm_csr_create_partitioned builds for these row blocks (host-only)."""
    rs = np.ascontiguousarray(row_starts, np.int64)
    ptr = np.ascontiguousarray(ptr, np.int32)
    node = np.ascontiguousarray(node, np.int32)
    nparts = len(rs) - 1
    nl, need = C.c_int32(0), C.c_int64(0)
    _ck(lib().sgm_partition_links_host(C.c_int32(nparts), C.c_void_p(rs.ctypes.data), C.c_void_p(ptr.ctypes.data),
                                       C.c_void_p(node.ctypes.data), C.byref(nl), None, None, None, None, None,
                                       C.c_int64(0), C.byref(need)))
    a = [np.zeros(max(nl.value, 1), np.int32) for _ in range(4)]
    idx = np.zeros(max(need.value, 1), np.int32)
    _ck(lib().sgm_partition_links_host(C.c_int32(nparts), C.c_void_p(rs.ctypes.data), C.c_void_p(ptr.ctypes.data),
                                       C.c_void_p(node.ctypes.data), C.byref(nl), *[C.c_void_p(v.ctypes.data) for v in a],
                                       C.c_void_p(idx.ctypes.data), C.c_int64(len(idx)), None))
    out, off = [], 0
    for i in range(nl.value):
        cnt = int(a[3][i])
        out.append({"sender": int(a[0][i]), "receiver": int(a[1][i]), "recv_offset": int(a[2][i]),
                    "send_idx": idx[off:off + cnt].copy()})
        off += cnt
    return out


def partition_rows_by_nnz(ptr, nparts, align=512):
    """sgm_partition_rows_by_nnz: contiguous row blocks balanced by 12 nnz + 20 rows, boundaries at
    multiples of `align` rows; returns row_starts (nparts+1, 0-based, int64)."""
    ptr = np.ascontiguousarray(ptr, np.int32)
    rs = np.zeros(nparts + 1, np.int64)
    _ck(lib().sgm_partition_rows_by_nnz(C.c_int32(len(ptr) - 1), C.c_void_p(ptr.ctypes.data), C.c_int32(nparts),
                                        C.c_int32(align), C.c_void_p(rs.ctypes.data)))
    return rs


def ell_degrees_host(node):
    """sgm_ell_degrees_host: degrees(n) of an ELLPACK graph (node as (n, max_d) = the reference's (max_d, n), 1-based) recovered
    from the padding the reference keeps -- what sgm_ell_create does when no degrees are handed in; -1 for a row the padding
    does not describe (a handle with such a row holds no degrees at all)."""
    node = np.ascontiguousarray(node, np.int32)
    n, md = node.shape
    deg = np.zeros(max(n, 1), np.int32)
    _ck(lib().sgm_ell_degrees_host(C.c_int32(n), C.c_int32(md), C.c_void_p(node.ctypes.data), C.c_void_p(deg.ctypes.data)))
    return deg[:n]


def left_permute_rows_host(p, ptr, node, val, r0, r1):
    """sgm_left_permute_rows_host: rows [r0, r1) (0-based) of A%left_permute(p) cut out of the whole matrix (1-based ptr / node):
    what a rank keeps of a permuted matrix distributed over ranks.  Returns (lptr, lnode, lval)."""
    p = np.ascontiguousarray(p, np.int32)
    ptr = np.ascontiguousarray(ptr, np.int32)
    node = np.ascontiguousarray(node, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    n = len(ptr) - 1
    lptr = np.zeros(r1 - r0 + 1, np.int32)
    need = C.c_int64(0)
    args = (C.c_int32(n), C.c_void_p(p.ctypes.data), C.c_void_p(ptr.ctypes.data), C.c_void_p(node.ctypes.data),
            C.c_void_p(val.ctypes.data), C.c_int64(r0), C.c_int64(r1), C.c_void_p(lptr.ctypes.data))
    _ck(lib().sgm_left_permute_rows_host(*args, None, None, C.c_int64(0), C.byref(need)))
    lnode = np.zeros(max(need.value, 1), np.int32)
    lval = np.zeros(max(need.value, 1), np.float64)
    _ck(lib().sgm_left_permute_rows_host(*args, C.c_void_p(lnode.ctypes.data), C.c_void_p(lval.ctypes.data), C.c_int64(need.value), None))
    return lptr, lnode[:need.value], lval[:need.value]


def slice_sched_host(n_slices, period_rows, grid, band_slices=64):
    """sgm_slice_sched_host: the order in which `grid` workgroups take the 512-row slices of a sliced
    matrix whose rows carry a far offset of `period_rows`; returns the (iters, grid) int32 table
    (slice or -1)."""
    it = C.c_int32(0)
    _ck(lib().sgm_slice_sched_host(C.c_int64(n_slices), C.c_int64(period_rows), C.c_int32(grid), C.c_int32(band_slices),
                                   None, C.c_int64(0), C.byref(it)))
    tab = np.empty(it.value * grid, np.int32)
    _ck(lib().sgm_slice_sched_host(C.c_int64(n_slices), C.c_int64(period_rows), C.c_int32(grid), C.c_int32(band_slices),
                                   C.c_void_p(tab.ctypes.data), C.c_int64(tab.size), C.byref(it)))
    return tab.reshape(it.value, grid)


def heartbeat():
    """sgm_heartbeat: where the thread driving the library is right now; callable from another thread (no HIP call).
    {"phase": words, "phase_code", "beats", "iteration", "halo_posts", "allreduce_posts", "solves"}."""
    out = (C.c_int64 * 6)()
    name = C.create_string_buffer(160)
    lib().sgm_heartbeat(out, name, C.c_int(160))
    return {"phase": name.value.decode(), "phase_code": int(out[0]), "beats": int(out[1]), "iteration": int(out[2]),
            "halo_posts": int(out[3]), "allreduce_posts": int(out[4]), "solves": int(out[5])}


def dot(a, b):
    pa, wa, _k1 = _arg(a, np.float64)
    pb, wb, _k2 = _arg(b, np.float64)
    n = a.numel() if _is_torch(a) else len(a)
    r = C.c_double(0.0)
    _ck(lib().sgm_dot(C.c_int64(n), pa, pb, C.byref(r), C.c_int(_same_where(wa, wb))))
    return r.value


def axpy(alpha, x, y):
    px, wx, _k1 = _arg(x, np.float64)
    py, wy, _k2 = _arg(y, np.float64, writable=True)
    n = x.numel() if _is_torch(x) else len(x)
    _ck(lib().sgm_axpy(C.c_int64(n), C.c_double(alpha), px, py, C.c_int(_same_where(wx, wy))))
    return y
