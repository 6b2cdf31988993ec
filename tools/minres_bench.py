"""MINRES beside the library's other Krylov loops at C2 size: the 5-point Poisson matrix of an nx x nx grid, b(i) = sin(0.001 i),
x = 0, no preconditioner, device vectors.  Timed with HIP events on the stream the library launches on; medians of --reps.
Recorded, not gated.

  per_iteration   MINRES, plain CG and BiCGStab on the Poisson matrix: a solve capped at K2 iterations minus one capped at K1
                  (tolerance 0, so the cap ends both), over K2 - K1 -- the start of a solve (x and b staged, r = b - A x) drops
                  out.  Vector traffic per iteration from the statements: MINRES reads 10 and writes 5 vectors beside the
                  product's (y -= t r1 | v.y: 3 + 1; y -= t r2 | y.y: 2 + 1; w, x, v: 5 + 3), CG reads 6 and writes 3
  to_tolerance    MINRES, BiCGStab and GMRES(30) on that matrix minus 0.3 I (symmetric indefinite) to 1e-8 |b|_2, each capped
                  at --cap iterations; a solve that ends at the cap is reported as a miss, with the residual |b - A x|_2 it
                  reached

    python tools/minres_bench.py [--nx 3162] [--reps 5] [--cap 20000] [--out FILE]     one JSON line
    python tools/minres_bench.py --trace minres|cg|bicgstab [--iters 200]               one capped solve (for a kernel trace:
                                                                                       kernel calls / iterations = launches per iteration)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K1, K2 = 100, 300


def matrix(sg, nx, shift):
    from sigma_amd import problems as P
    n = nx * nx
    ptr, node, val = P.poisson2d_csr(nx, nx)
    if shift:
        row = np.repeat(np.arange(1, n + 1, dtype=np.int64), np.diff(ptr))
        val = val.copy()
        val[node == row] -= shift
    return sg.csr_matrix(n, n, ptr, node, val)


def make(sg, kind, tol):
    return {"minres": sg.minres, "cg": sg.cg, "bicgstab": sg.bicgstab, "gmres": lambda t: sg.gmres(t, 30)}[kind](tol)


def capped_solve_time(sg, torch, A, b, kind, cap, reps):
    s = make(sg, kind, 0.0)
    s.set_max_iter(cap)
    s.setup(A)
    x = torch.zeros_like(b)
    ts = []
    for rep in range(reps + 1):                     # (the first one warms up)
        x.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.solve(A, x, b, None, check=False)
        e1.record()
        e1.synchronize()
        if rep:
            ts.append(e0.elapsed_time(e1) * 1e-3)
        assert s.last_iterations == cap, (kind, s.last_iterations, cap)
    s.destroy()
    return float(np.median(ts))


def trace(a):
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    A = matrix(sg, a.nx, 0.0)
    n = a.nx * a.nx
    b = torch.sin(0.001 * torch.arange(1, n + 1, dtype=torch.float64, device="cuda"))
    s = make(sg, a.trace, 0.0)
    s.set_max_iter(a.iters)
    s.setup(A)
    x = torch.zeros_like(b)
    s.solve(A, x, b, None, check=False)
    torch.cuda.synchronize()
    print(json.dumps({"nx": a.nx, "solver": a.trace, "iterations": s.last_iterations}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=20000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, choices=["minres", "cg", "bicgstab"])
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if a.trace:
        return trace(a)
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    nx, n = a.nx, a.nx * a.nx
    b = torch.sin(0.001 * torch.arange(1, n + 1, dtype=torch.float64, device="cuda"))
    rec = {"nx": nx, "rows": n, "k1": K1, "k2": K2, "cap": a.cap}

    A = matrix(sg, nx, 0.0)
    rec["kernel"] = A.kernel
    per = {}
    for kind in ("minres", "cg", "bicgstab"):
        t1 = capped_solve_time(sg, torch, A, b, kind, K1, a.reps)
        t2 = capped_solve_time(sg, torch, A, b, kind, K2, a.reps)
        per[kind] = {"solve_k1_s": t1, "solve_k2_s": t2, "us_per_iteration": (t2 - t1) / (K2 - K1) * 1e6}
    rec["per_iteration"] = per
    rec["minres_over_cg"] = per["minres"]["us_per_iteration"] / per["cg"]["us_per_iteration"]
    A.destroy()
    del A
    torch.cuda.empty_cache()

    As = matrix(sg, nx, 0.3)
    bnorm = float(torch.linalg.norm(b))
    tol = 1e-8 * bnorm
    rec.update(shift=0.3, b_norm=bnorm, tolerance=tol)
    to_tol = {}
    for kind in ("minres", "bicgstab", "gmres"):
        s = make(sg, kind, tol)
        s.set_max_iter(a.cap)
        s.setup(As)
        x = torch.zeros_like(b)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.solve(As, x, b, None, check=False)
        e1.record()
        e1.synchronize()
        q = torch.zeros_like(b)
        As.matvec(x, q)
        true = float(torch.linalg.norm(b - q))
        to_tol[kind] = {"reached": bool(s.converged), "iterations": int(s.last_iterations), "seconds": e0.elapsed_time(e1) * 1e-3,
                        "sqrt_res2": float(np.sqrt(s.res2)) if s.res2 == s.res2 else "nan", "true_residual": true,
                        "true_residual_over_b": true / bnorm}
        s.destroy()
    rec["to_tolerance"] = to_tol
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
