#!/usr/bin/env python3
"""One JSON line per solve: iteration count, `converged`, SHA-256 of x and of the residual history -- over the cooperative,
one-workgroup and launch-loop paths of CG and BiCGStab, one MINRES and one GMRES(30) solve, and the ILDU(0) apply and
ILDU-preconditioned CG over the triangular sweeps' paths (strips, walkers, slabs, row-space levels).  Run it on two checkouts
(--tree PATH picks whose sigma_amd is imported), each in a process of its own: a change that moves no rounding leaves the two
outputs identical.  Public Python API only."""
import argparse, hashlib, json, os, sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))
import numpy as np
import sigma_amd as sg
from sigma_amd import problems as P

sg.init(0)


def banded(n, entries):
    """CSR arrays (1-based) of the matrix with value v on offset d for (d, v) in `entries`, rows in the order given"""
    rows = np.arange(n)
    keep = np.array([(rows + d >= 0) & (rows + d < n) for d, _ in entries]).T
    cols = np.array([rows + d + 1 for d, _ in entries]).T
    vals = np.tile(np.array([v for _, v in entries], float), (n, 1))
    ptr = np.concatenate([[1], 1 + np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return ptr, cols[keep].astype(np.int32), vals[keep]


def skew(ptr, node, val):
    """BiCGStab's matrices: entries right of the diagonal x 0.8, left of it x 1.2, the diagonal x 1.05"""
    rows = np.repeat(np.arange(1, len(ptr)), np.diff(ptr))
    return val * (1.0 + 0.2 * np.sign(rows - node)) * np.where(rows == node, 1.05, 1.0)


SHAPES = [("tridiagonal 4099", 4099, P.tridiag_csr(4099, 2.5, -1.0, -1.0)),
          ("5-point 64x41", 64 * 41, P.poisson2d_csr(64, 41)),
          ("5-point 64x65", 64 * 65, P.poisson2d_csr(64, 65)),
          ("5-point 96x86", 96 * 86, P.poisson2d_csr(96, 86)),
          ("7-point 13^3", 13 ** 3, P.laplace3d_csr(13, 13, 13)),
          # six stored entries per row (one of them an explicit 0.0): a slice width with no kernel of its own, the 8-slot one
          ("6 slots 4200", 4200, banded(4200, [(-3, -1.0), (-1, -1.0), (0, 4.5), (1, -1.0), (2, 0.0), (3, -1.0)]))]


def solve(label, kind, n, csr, jac=False, opts=(), tol=1e-9, max_iter=0, x0=0.25):
    ptr, node, val = csr
    if kind == "bicgstab":
        val = skew(ptr, node, val)
    A = sg.csr_matrix(n, n, ptr, node, val)
    pc = None
    if jac:
        pc = sg.jacobi(); pc.setup(A)
    s = {"cg": sg.cg, "bicgstab": sg.bicgstab, "minres": sg.minres, "gmres": lambda t: sg.gmres(t, 30)}[kind](tol)
    s.set_history(100000)
    for k, v in opts:
        s.set_option(k, v)
    if max_iter:
        s.set_max_iter(max_iter)
    s.setup(A)
    u = np.full(n, x0)
    b = np.sin(0.01 * np.arange(1, n + 1)) + 0.5
    s.solve(A, u, b, pc, check=False)
    print(json.dumps({"case": label, "solver": kind, "jacobi": jac, "options": dict(opts), "max_iter": max_iter,
                      "iterations": int(s.last_iterations), "converged": bool(s.converged),
                      "x": hashlib.sha256(u.tobytes()).hexdigest(),
                      "history": hashlib.sha256(np.array(s.history, float).tobytes()).hexdigest()}), flush=True)


for kind in ("cg", "bicgstab"):
    small = "cg_small" if kind == "cg" else "bicgstab_small"
    for jac in (False, True):
        for label, n, csr in SHAPES:
            for variant in (0, 1, 2, 4, 8, 16, 20):
                solve(label, kind, n, csr, jac, (("cg_coop_variant", variant),))
        # chunked launches (1, 7), the default, and the launch loop (0): cooperative (tridiagonal 4099) and one workgroup (32 x 32)
        for label, n, csr in (SHAPES[0], ("5-point 32x32", 1024, P.poisson2d_csr(32, 32))):
            for chunk in (1, 7, None, 0):
                solve(label, kind, n, csr, jac, () if chunk is None else ((small, chunk),))
        for graph in (0, 1):
            solve(SHAPES[2][0], kind, SHAPES[2][1], SHAPES[2][2], jac, ((small, 0), ("krylov_graph", graph)), tol=1e-12)
    solve("5-point 32x32", kind, 1024, P.poisson2d_csr(32, 32), False, (("dot_order", 1),))
    solve("5-point 64x65", kind, 64 * 65, P.poisson2d_csr(64, 65), False, (), tol=1e-300, max_iter=37)
    solve("5-point 32x32", kind, 1024, P.poisson2d_csr(32, 32), False, (), tol=1e-300, max_iter=37)
    solve("5-point 64x65", kind, 64 * 65, P.poisson2d_csr(64, 65), False, ((small, 0),), tol=1e-300, max_iter=37)
solve("5-point 64x65", "minres", 64 * 65, P.poisson2d_csr(64, 65))
solve("5-point 64x65", "gmres", 64 * 65, P.poisson2d_csr(64, 65))


def ildu(label, n, csr, colour=False, opts=()):
    """ILDU(0): SHA-256 of z = M^-1 b from pc.solve, and of x and the history of a CG solve preconditioned with it; the
    path that served (strips, slabs, row-space levels) rides along"""
    ptr, node, val = csr
    A = sg.csr_matrix(n, n, ptr, node, val)
    if colour:
        p, _, _ = A.greedy_color_ordering()
        A.left_permute(p); A.right_permute(p)
    pc = sg.ldu()
    for k, v in opts:
        pc.set_option(k, v)
    pc.setup(A)
    b = np.sin(0.01 * np.arange(1, n + 1)) + 0.5
    z = np.zeros(n)
    pc.solve(A, z, b)
    s = sg.cg(1e-9)
    s.set_history(100000)
    # (capped: the six-slot band's ILDU(0) is not symmetric -- the explicit 0.0 at +2 fills, nothing at -2 does -- and CG with
    # it stalls at |r|^2 = 1.04e-17, above the tolerance; a solve has no cap of its own.  The others take 23 .. 181 iterations.)
    s.set_max_iter(400)
    s.setup(A)
    u = np.full(n, 0.25)
    s.solve(A, u, b, pc, check=False)
    print(json.dumps({"case": label, "solver": "ildu + cg", "colour": colour, "options": dict(opts), "max_iter": 400,
                      "path": {k: pc.get(k, np.int32).tolist() for k in ("levels", "strips", "slabs", "row_levels")},
                      "iterations": int(s.last_iterations), "converged": bool(s.converged),
                      "z": hashlib.sha256(z.tobytes()).hexdigest(), "x": hashlib.sha256(u.tobytes()).hexdigest(),
                      "history": hashlib.sha256(np.array(s.history, float).tobytes()).hexdigest()}), flush=True)


# the triangular sweeps: strip pipeline and level walkers (natural order), row-space levels fused / unfused / off (colour order)
for strips in (1, 0):
    ildu(SHAPES[2][0], SHAPES[2][1], SHAPES[2][2], False, (("ildu_strips", strips),))
for label, n, csr in (SHAPES[2], ("5-point 91x93", 91 * 93, P.poisson2d_csr(91, 93))):
    for rows in (1, 2, 0):
        ildu(label, n, csr, True, (("ildu_rows", rows),))
for colour in (False, True):
    ildu(SHAPES[4][0], SHAPES[4][1], SHAPES[4][2], colour)
ildu(SHAPES[5][0], SHAPES[5][1], SHAPES[5][2])
