"""LSQR at C2 size: A = problems.interp2d_csr(nx, nx), the 2:1 interpolation onto an nx x nx grid (nx = 3162: 9,998,244 x
2,499,561, full column rank, cond about 2), b(i) = sin(0.001 i), x = 0, device vectors.  Timed with HIP events on the stream the
library launches on; medians of --reps.  Recorded, not gated.

  per_step        a solve capped at K2 steps minus one capped at K1 (both tolerances 0, so the cap ends both), over K2 - K1 -- the
                  start of a solve (x and b staged, u = b - A x, the first A^T u) drops out.  Vector traffic per step from the
                  statements, beside the two products: FLsqrU reads 2 and writes 1 vector of m entries, FLsqrV the same of n,
                  FLsqrWX reads 3 and writes 2 of n: 24 m + 64 n bytes.
  products        sgm_mat_matvec and sgm_mat_matvec_t alone on the same operand (device vectors)
  no_colblock     per_step and products again on a second handle of the operand with the matrix option "ell_colblock" = 0 (the
                  cached transpose inherits A's options): the transposed copy then runs an ordinary row kernel instead of the
                  column-blocked two-phase form its scattered columns select by default -- the same bits either way
  to_tolerance    LSQR to normal_tolerance = 1e-8 |A^T b|_2 against CG on the explicit A^T A = sg.PtAP(I, A) with the right-hand
                  side A^T b and the same absolute tolerance (CG's sqrt(res2) is the normal equations' residual); the Galerkin
                  build is timed on its own.  Iterations, seconds and the TRUE |A^T (b - A x)|_2 of both; a solve that ends at
                  --cap is reported as a miss with what it reached.

    python tools/lsqr_bench.py [--nx 3162] [--reps 5] [--cap 2000] [--out FILE]     one JSON line
    python tools/lsqr_bench.py --trace [--iters 200] [--colblock 0]
                                                          one capped solve, the two products alone and, for scale, the library's
                                                          own y += a x kernel (FAxpy: 2 reads + 1 write, FLsqrU's and FLsqrV's
                                                          pattern) at the footprints of FLsqrU / FLsqrV / FLsqrWX (for a kernel
                                                          trace: kernel calls / steps = launches per step)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K1, K2 = 100, 300


def operand(sg, nx, colblock=None):
    from sigma_amd import problems as P
    ptr, node, val, nc = P.interp2d_csr(nx, nx)
    A = sg.csr_matrix(nx * nx, nc, ptr, node, val)
    if colblock is not None:
        A.set_option("ell_colblock", colblock)
    return A, nx * nx, nc


def timed(torch, f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def capped_solve_time(sg, torch, A, b, n, cap, reps):
    s = sg.lsqr(0.0, 0.0)
    s.set_max_iter(cap)
    s.setup(A)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    ts = []
    for rep in range(reps + 1):                     # (the first one warms up)
        x.zero_()
        t = timed(torch, lambda: s.solve(A, x, b, check=False))
        if rep:
            ts.append(t)
        assert s.last_iterations == cap and s.stop == 0, (s.last_iterations, s.stop, cap)
    s.destroy()
    return float(np.median(ts))


def normal_residual(torch, A, x, b, m, n):
    q = torch.zeros(m, dtype=torch.float64, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.matvec(x, q)
    A.matvec_t(b - q, g)
    return float(torch.linalg.norm(g))


def trace(a):
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    A, m, n = operand(sg, a.nx, a.colblock)
    b = torch.sin(0.001 * torch.arange(1, m + 1, dtype=torch.float64, device="cuda"))
    s = sg.lsqr(0.0, 0.0)
    s.set_max_iter(a.iters)
    s.setup(A)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    s.solve(A, x, b, check=False)
    q = torch.zeros(m, dtype=torch.float64, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    for _ in range(20):
        A.matvec(x, q)
        A.matvec_t(b, g)
    # y += a x over N doubles moves 24 N bytes: N = m, n and 5 n / 3 entries for the 24 m, 24 n and 40 n bytes of the three
    # passes; 10, 20 and 40 calls, so that the trace tells the three sizes apart by their call counts if it lists them apart,
    # and the event times below do so whatever it lists
    axpy = {}
    for N, calls in ((m, 10), (n, 20), (5 * n // 3, 40)):
        src = torch.ones(N, dtype=torch.float64, device="cuda")
        dst = torch.zeros_like(src)
        sg.axpy(0.5, src, dst)
        t = timed(torch, lambda: [sg.axpy(0.5, src, dst) for _ in range(calls)])
        axpy[str(N)] = {"calls": calls + 1, "bytes": 24 * N, "us_per_call_events": t / calls * 1e6}
    torch.cuda.synchronize()
    print(json.dumps({"nx": a.nx, "rows": m, "cols": n, "colblock": a.colblock, "steps": s.last_iterations, "products_alone": 20,
                      "axpy": axpy}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cap", type=int, default=2000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--colblock", type=int, default=None, help="--trace only: the operand's \"ell_colblock\" option")
    a = ap.parse_args()
    if a.trace:
        return trace(a)
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    A, m, n = operand(sg, a.nx)
    b = torch.sin(0.001 * torch.arange(1, m + 1, dtype=torch.float64, device="cuda"))
    rec = {"nx": a.nx, "rows": m, "cols": n, "nnz": int(A.nnz) if hasattr(A, "nnz") else None, "k1": K1, "k2": K2, "cap": a.cap,
           "kernel": A.kernel, "vector_bytes_per_step": 24 * m + 64 * n}

    t1 = capped_solve_time(sg, torch, A, b, n, K1, a.reps)
    t2 = capped_solve_time(sg, torch, A, b, n, K2, a.reps)
    rec["per_step"] = {"solve_k1_s": t1, "solve_k2_s": t2, "us_per_step": (t2 - t1) / (K2 - K1) * 1e6}

    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    q = torch.zeros(m, dtype=torch.float64, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    A.matvec(x, q); A.matvec_t(b, g)                 # (warm-up)
    rec["products"] = {
        "matvec_us": float(np.median([timed(torch, lambda: A.matvec(x, q)) for _ in range(a.reps)])) * 1e6,
        "matvec_t_us": float(np.median([timed(torch, lambda: A.matvec_t(b, g)) for _ in range(a.reps)])) * 1e6}

    A0, _, _ = operand(sg, a.nx, 0)
    t1 = capped_solve_time(sg, torch, A0, b, n, K1, a.reps)
    t2 = capped_solve_time(sg, torch, A0, b, n, K2, a.reps)
    A0.matvec_t(b, g)
    rec["no_colblock"] = {"solve_k1_s": t1, "solve_k2_s": t2, "us_per_step": (t2 - t1) / (K2 - K1) * 1e6,
                          "matvec_t_us": float(np.median([timed(torch, lambda: A0.matvec_t(b, g)) for _ in range(a.reps)])) * 1e6}
    A0.destroy()
    del A0

    atb = float(torch.linalg.norm(g))
    tol = 1e-8 * atb
    rec.update(atb_norm=atb, tolerance=tol)
    to_tol = {}
    s = sg.lsqr(0.0, tol)
    s.set_max_iter(a.cap)
    s.setup(A)
    x.zero_()
    sec = timed(torch, lambda: s.solve(A, x, b, check=False))
    to_tol["lsqr"] = {"reached": bool(s.converged), "stop": int(s.stop), "iterations": int(s.last_iterations), "seconds": sec,
                      "arnorm": float(s.arnorm), "rnorm": float(s.rnorm), "true_normal_residual": normal_residual(torch, A, x, b, m, n)}
    s.destroy()

    i = np.arange(1, m + 2, dtype=np.int32)
    eye = sg.csr_matrix(m, m, i, i[:-1].copy(), np.ones(m))
    holder = {}
    build = timed(torch, lambda: holder.update(N=sg.PtAP(eye, A)))
    N = holder["N"]
    c = sg.cg(tol)
    c.set_max_iter(a.cap)
    c.setup(N)
    x.zero_()
    sec = timed(torch, lambda: c.solve(N, x, g, None, check=False))
    to_tol["cg_on_AtA"] = {"reached": bool(c.converged), "iterations": int(c.last_iterations), "seconds": sec, "galerkin_build_s": build,
                           "sqrt_res2": float(np.sqrt(c.res2)) if c.res2 == c.res2 else "nan",
                           "true_normal_residual": normal_residual(torch, A, x, b, m, n)}
    c.destroy()
    rec["to_tolerance"] = to_tol
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
