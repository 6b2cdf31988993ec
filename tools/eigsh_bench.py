"""sg.eigsh at C2 size: the 5-point Poisson matrix of an nx x nx grid, k = 4, ncv = 20, the default start vector as a device
tensor.  Timed with a host clock around calls that end in a device synchronisation (every sgm_eigsh call does); medians of
--reps after a warm-up call.  Recorded, not gated.

  cycle      which = "SA" with max_restarts = 0, 1 and 5.  The smallest eigenvalues of this matrix do not converge without
             shift-invert, so this leg measures the COST of a cycle, not a solve: the first cycle is 20 Lanczos steps, a restart
             cycle is the rotation of the basis, a copy and ncv - keep = 8 steps; (t(5) - t(1)) / 4 is one restart cycle.
             Every call also forms 4 Ritz vectors and their 4 true residuals.
  solve      the same matrix with 8 diagonal entries raised by 10, 20, ..., 80 (the largest eigenvalues are then well separated),
             which = "LA", tol = 1e-8: restarts, products, seconds, the true residuals.  (rho, the Lanczos estimate, is compared
             with tol * anorm inside the call and is not returned: converged = True says rho <= tol * anorm for all 4.)
  replaces   sg.eigensolve(A, 20, q1) end to end -- 20 steps of sgm_lanczos, Q to the host, scipy's tridiagonal eigensolver, the
             host product Q Z -- against one cycle of the same ncv here (max_restarts = 0, V returned on the device).

    python tools/eigsh_bench.py [--nx 3162] [--reps 3] [--out FILE]        one JSON line
    python tools/eigsh_bench.py --trace [--restarts 2]                      one call (for a kernel trace: per-kernel times)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, NCV = 4, 20


def matrix(sg, nx, raised):
    from sigma_amd import problems as P
    n = nx * nx
    ptr, node, val = P.poisson2d_csr(nx, nx)
    if raised:
        val = val.copy()
        for a in range(8):
            r = int(n * (2 * a + 1) / 16)                      # 8 rows spread over the grid
            e = np.arange(ptr[r] - 1, ptr[r + 1] - 1)
            val[e[node[e] - 1 == r]] += 10.0 * (a + 1)
    return sg.csr_matrix(n, n, ptr, node, val)


def timed(fn, reps):
    ts, out = [], None
    for rep in range(reps + 1):                                # (the first one warms up)
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--restarts", type=int, default=2)
    a = ap.parse_args()
    import torch
    import sigma_amd as sg
    sg.init(0)
    nx, n = a.nx, a.nx * a.nx
    q1h = sg.eigsh_start_vector(n)
    q1 = torch.tensor(q1h, device="cuda")
    A = matrix(sg, nx, False)
    if a.trace:
        r = sg.eigsh(A, K, which="SA", ncv=NCV, tol=1e-8, max_restarts=a.restarts, q1=q1)
        torch.cuda.synchronize()
        print(json.dumps({"nx": nx, "rows": n, "k": K, "ncv": NCV, "restarts": r.restarts, "products": r.products}), flush=True)
        return
    keep = K + (NCV - K) // 2
    rec = {"nx": nx, "rows": n, "k": K, "ncv": NCV, "keep": keep, "kernel": A.kernel, "reps": a.reps}

    cyc = {}
    for mr in (0, 1, 5):
        t, r = timed(lambda: sg.eigsh(A, K, which="SA", ncv=NCV, tol=1e-8, max_restarts=mr, q1=q1), a.reps)
        assert r.restarts == mr and not r.converged
        cyc[f"max_restarts_{mr}_s"] = t
        cyc[f"max_restarts_{mr}_products"] = r.products
    cyc["first_cycle_and_4_residuals_s"] = cyc["max_restarts_0_s"]
    cyc["restart_cycle_s"] = (cyc["max_restarts_5_s"] - cyc["max_restarts_1_s"]) / 4
    cyc["restart_cycle_steps"] = NCV - keep
    # what a restart cycle must move, from the statements: the rotation 8 n (m + keep); step j reads the j + 1 columns three
    # times (h | w -= Q h, g | w -= Q g, w.w) and passes over w five times (the first pass reads it, the other two read and
    # write it); the scaling reads w and writes q_{j+1}; the product's own traffic is not counted here
    steps = range(keep, NCV)
    rec["restart_cycle_bytes"] = {"rotate": 8 * n * (NCV + keep), "copy": 16 * n,
                                  "gram_schmidt": int(sum(8 * n * (3 * (j + 1) + 5) for j in steps)), "scale": 16 * n * len(steps)}
    rec["cycle"] = cyc

    # what it replaces (host q1: sg.lanczos takes a numpy start vector)
    t_old, (lam_old, V_old) = timed(lambda: sg.eigensolve(A, NCV, q1h), 1)
    del V_old
    rec["replaces"] = {"eigensolve_20_steps_end_to_end_s": t_old, "eigsh_one_cycle_ncv20_s": cyc["max_restarts_0_s"],
                       "ratio": t_old / cyc["max_restarts_0_s"], "Q_host_bytes": 8 * n * NCV}
    A.destroy()
    del A
    torch.cuda.empty_cache()

    Ao = matrix(sg, nx, True)
    t, r = timed(lambda: sg.eigsh(Ao, K, which="LA", ncv=NCV, tol=1e-8, max_restarts=200, q1=q1), a.reps)
    rec["solve"] = {"which": "LA", "tol": 1e-8, "converged": r.converged, "restarts": r.restarts, "products": r.products, "seconds": t,
                    "lam": [float(x) for x in r.lam], "true_residuals": [float(x) for x in r.residuals],
                    "rho": "not returned; converged means rho <= tol * anorm for every pair"}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
