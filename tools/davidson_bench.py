"""sg.davidson at C2 size: the 5-point Poisson matrix of an nx x nx grid, k = 4, ncv = 20, tol = 1e-8, the default start vector
as a device tensor, sg.multigrid(problems.interp2d_hierarchy(nx, nx), omega = 0.8) -- V(1,1), 8 coarse sweeps -- with and
without coarse = "direct".  Recorded, not gated.

  solve      time to solution (a host clock around the call, which ends in a device synchronisation; median of --reps after a
             warm-up call), steps, products, applies, restarts, the eigenvalues, the true residuals and their distance to the
             analytic eigenvalues, for both coarse solvers
  parts      one V-cycle apply and one product, each timed with HIP events on the stream the library launches on (median of 20
             after 3): the two parts of a step that are not new
  lanczos    sg.eigsh(A, 4, "SA", ncv = 20, tol = 1e-8) on the same matrix with max_restarts capped (--lanczos-restarts) so that
             the call stays under a minute: converged or not, products, seconds, the true residuals it reached

    python tools/davidson_bench.py [--nx 3162] [--reps 3] [--out FILE]        one JSON line
    python tools/davidson_bench.py --trace                                     one V(1,1) solve and a two-step call without a
                                                                               preconditioner (its FCopy is the copy kernel the
                                                                               rates are set beside), for a kernel trace
    python tools/davidson_bench.py --digest STATS.csv --steps S                a kernel-stats file of that run, by part of a step
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, NCV, TOL, OMEGA = 4, 20, 1e-8, 0.8

# kernel name fragment -> part of a step (first match; everything else: the V-cycle, the products and the set-up of the
# hierarchy, which the trace cannot tell apart by name -- `parts` times an apply and a product on their own)
GROUPS = [("k_dav_ritz", "k_dav_ritz"), ("k_basis_rotate", "rotation"), ("k_egs", "orthogonalisation"),
          ("k_eig_reduce", "orthogonalisation"), ("k_dav_norm", "orthogonalisation"), ("FEigScale", "orthogonalisation"),
          ("FDot2", "orthogonalisation"), ("FEigResid", "true residuals"), ("FCopy", "copy")]


def digest(path, steps):
    tot, calls = {}, {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            g = next((grp for frag, grp in GROUPS if frag in row["Name"]), "everything else")
            tot[g] = tot.get(g, 0.0) + float(row["TotalDurationNs"])
            calls[g] = calls.get(g, 0) + int(row["Calls"])
    out = {g: {"calls": calls[g], "total_us": tot[g] / 1e3, "us_per_step": tot[g] / 1e3 / steps} for g in sorted(tot)}
    print(json.dumps({"steps": steps, "kernel_time_by_part": out}), flush=True)


def problem(sg, nx):
    from sigma_amd import problems as P
    n = nx * nx
    ptr, node, val = P.poisson2d_csr(nx, nx)
    A = sg.csr_matrix(n, n, ptr, node, val)
    Ps = [sg.csr_matrix(nf, nc, p, nd, v) for p, nd, v, nf, nc in P.interp2d_hierarchy(nx, nx)]
    return A, Ps


def analytic(nx, k):
    j = np.arange(1, 8, dtype=np.longdouble)
    pi = np.longdouble(4) * np.arctan(np.longdouble(1))
    c = np.longdouble(2) - np.longdouble(2) * np.cos(j * pi / np.longdouble(nx + 1))
    return np.sort((c[:, None] + c[None, :]).ravel())[:k]


def timed(fn, reps):
    ts, out = [], None
    for rep in range(reps + 1):                                # (the first one warms up)
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), out


def events(torch, fn, reps=20, warmup=3):
    ts = []
    for rep in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts[warmup:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--digest", default=None)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--lanczos-restarts", type=int, default=1500)
    a = ap.parse_args()
    if a.digest:
        return digest(a.digest, a.steps)
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    nx, n = a.nx, a.nx * a.nx
    q1 = torch.tensor(sg.eigsh_start_vector(n), device="cuda")
    A, Ps = problem(sg, nx)
    if a.trace:
        pc = sg.multigrid(Ps, omega=OMEGA)
        pc.setup(A)
        r = sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1)
        r0 = sg.davidson(A, K, ncv=NCV, tol=TOL, max_steps=2, q1=q1)
        torch.cuda.synchronize()
        print(json.dumps({"nx": nx, "rows": n, "k": K, "ncv": NCV, "steps": r.steps, "products": r.products, "restarts": r.restarts,
                          "converged": r.converged, "unpreconditioned_steps": r0.steps}), flush=True)
        return
    rec = {"nx": nx, "rows": n, "k": K, "ncv": NCV, "tol": TOL, "kernel": A.kernel, "reps": a.reps, "levels": len(Ps) + 1}
    exact = analytic(nx, K)
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros_like(x)
    rec["product_s"] = events(torch, lambda: A.matvec(x, y))
    for coarse in ("sweeps", "direct"):
        pc = sg.multigrid(Ps, omega=OMEGA, coarse=coarse)
        pc.setup(A)
        t, r = timed(lambda: sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1), a.reps)
        apply_s = events(torch, lambda: pc.solve(A, y, x))
        rec[f"davidson_coarse_{coarse}"] = {
            "seconds": t, "steps": r.steps, "products": r.products, "applies": r.applies, "restarts": r.restarts, "converged": r.converged,
            "seconds_per_step": t / max(r.steps, 1), "vcycle_apply_s": apply_s,
            "lam": [float(v) for v in r.lam], "true_residuals": [float(v) for v in r.residuals],
            "distance_to_analytic": [float(abs(np.longdouble(v) - e)) for v, e in zip(r.lam, exact)]}
        del r
        pc.destroy()
    t0 = time.perf_counter()
    e = sg.eigsh(A, K, "SA", ncv=NCV, tol=TOL, max_restarts=a.lanczos_restarts, q1=q1, want_V=False)
    rec["lanczos_SA"] = {"max_restarts": a.lanczos_restarts, "seconds": time.perf_counter() - t0, "converged": e.converged,
                         "restarts": e.restarts, "products": e.products, "lam": [float(v) for v in e.lam],
                         "true_residuals": [float(v) for v in e.residuals],
                         "distance_to_analytic": [float(abs(np.longdouble(v) - x_)) for v, x_ in zip(e.lam, exact)]}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
