"""sg.davidson(A, k, pc, B=B) at C2 size: the tensor P1 pair fem<nx>x<nx> of sigma_amd.problems.fem2d_pair_csr (A = Ky (x) Mx +
My (x) Kx, B = My (x) Mx, both 9-point), k = 4, ncv = 20, tol = 1e-8, the default start vector as a device tensor,
sg.multigrid(problems.interp2d_hierarchy(nx, nx), omega = 0.8) -- V(1,1), 8 coarse sweeps -- set up on A.  Recorded, not gated.

  solve      time to solution (a host clock around the call, which ends in a device synchronisation; median of --reps after a
             warm-up call), steps, products with A and with B, applies, restarts, the eigenvalues, the true residuals and their
             distance to the analytic eigenvalues kappa_i(nx) + kappa_j(nx)
  parts      one V-cycle apply, one product with A and one with B, each timed with HIP events on the stream the library
             launches on (median of 20 after 3)

    python tools/davidson_gen_bench.py [--nx 3162] [--reps 3] [--out FILE]     one JSON line
    python tools/davidson_gen_bench.py --trace                                  for a kernel trace: one V(1,1) solve of the pencil,
                                                                                then five times over [sg.davidson(A) and
                                                                                sg.davidson(A, B=B), both capped at 19 steps] --
                                                                                every call makes the Ritz passes m = 1 .. 20 and
                                                                                the Gram-Schmidt passes m = 1 .. 19 once, with no
                                                                                restart, so the kernels of the two loops meet the
                                                                                same n and m --, then a two-step sg.davidson(A)
                                                                                without a preconditioner, whose FCopy is the
                                                                                copy kernel
    python tools/davidson_gen_bench.py --digest KERNEL_TRACE.csv --steps S      the per-dispatch trace of that run: kernel time of
                                                                                the first solve by part of a step, and for each
                                                                                of the five repetitions the rate of k_dav_ritz,
                                                                                k_gdav_ritz, k_egs<., 1> and k_egs2 on their
                                                                                compulsory bytes as a fraction of the copy
                                                                                kernel's
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
CAP, REPS = 19, 5

# kernel name fragment -> part of a step (first match; everything else: the V-cycle, the products and the set-up of the
# hierarchy, which the trace cannot tell apart by name -- `parts` times an apply and the two products on their own)
GROUPS = [("k_gdav_ritz", "k_gdav_ritz"), ("k_dav_ritz", "k_dav_ritz"), ("k_basis_rotate", "rotation"), ("k_egs", "orthogonalisation"),
          ("k_eig_reduce", "orthogonalisation"), ("k_dav_norm", "orthogonalisation"), ("k_gdav_bnorm", "orthogonalisation"),
          ("FEigScale", "orthogonalisation"), ("FDot2", "orthogonalisation"), ("FEigResid", "true residuals"), ("FCopy", "copy")]


def _dispatches(path):
    """(kernel name, start ns, duration ns) of every dispatch, in time order"""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows]
    return sorted(out, key=lambda t: t[1])


def digest(path, steps, n):
    d = _dispatches(path)
    # the first solve ends at the first k_dav_ritz (the standard loop runs only in the repetitions)
    first_std = next(i for i, t in enumerate(d) if "k_dav_ritz" in t[0])
    tot, calls = {}, {}
    for name, _, dur in d[:first_std]:
        g = next((grp for frag, grp in GROUPS if frag in name), "everything else")
        tot[g] = tot.get(g, 0.0) + dur
        calls[g] = calls.get(g, 0) + 1
    by_part = {g: {"calls": calls[g], "total_us": tot[g] / 1e3, "us_per_step": tot[g] / 1e3 / steps} for g in sorted(tot)}
    # the repetitions: a call of one loop lasts from its first Ritz pass to the first Ritz pass of the other loop.  Within a
    # call every step launches k_dav_norm once, after its Gram-Schmidt passes and before its Ritz pass, so a dispatch meets
    # m = 1 + (the k_dav_norm dispatches of the call so far) columns: its compulsory bytes follow from its name and m.
    nbytes = {"k_dav_ritz": lambda m: 8.0 * n * (2 * m + 1), "k_gdav_ritz": lambda m: 8.0 * n * (2 * m + 1),
              "k_egs_mode1": lambda m: 8.0 * n * (m + 2), "k_egs2": lambda m: 8.0 * n * (2 * m + 2)}

    def family(name):
        if "k_gdav_ritz" in name or "k_dav_ritz" in name or "k_egs2" in name:
            return next(f for f in ("k_gdav_ritz", "k_dav_ritz", "k_egs2") if f in name)
        return "k_egs_mode1" if "k_egs<" in name and ", 1>" in name else None

    calls_of, loop, m = [], None, 1
    copy = []
    for name, _, dur in d[first_std:]:
        f = family(name)
        if f in ("k_dav_ritz", "k_gdav_ritz") and f != loop:
            loop, m = f, 1
            calls_of.append({})
        if "k_dav_norm" in name:
            m += 1
        if "FCopy" in name:
            copy.append(dur)
        if f:
            t, by = calls_of[-1].get(f, (0.0, 0.0))
            calls_of[-1][f] = (t + dur, by + nbytes[f](m))
    copy_rate = 16.0 * n / (np.mean(copy) * 1e-9)
    kernels = {}
    for f in nbytes:
        reps = [c[f] for c in calls_of if f in c][:REPS]
        rates = [by / (t * 1e-9) for t, by in reps]
        kernels[f] = {"us_per_call_of_the_loop": [t / 1e3 for t, _ in reps], "GB_per_call_of_the_loop": [by / 1e9 for _, by in reps],
                      "TBps": [r / 1e12 for r in rates], "of_copy": [r / copy_rate for r in rates],
                      "of_copy_median_min_max": [float(np.median(rates) / copy_rate), min(rates) / copy_rate, max(rates) / copy_rate]}
    print(json.dumps({"steps": steps, "rows": n, "copy_TBps": copy_rate / 1e12, "copy_us": [c / 1e3 for c in copy],
                      "kernel_time_by_part_first_solve": by_part, "kernels": kernels}), flush=True)


def problem(sg, nx):
    from sigma_amd import problems as P
    n = nx * nx
    (pa, na, va), (pb, nb, vb) = P.fem2d_pair_csr(nx, nx)
    A = sg.csr_matrix(n, n, pa, na, va)
    B = sg.csr_matrix(n, n, pb, nb, vb)
    Ps = [sg.csr_matrix(nf, nc, p, nd, v) for p, nd, v, nf, nc in P.interp2d_hierarchy(nx, nx)]
    return A, B, Ps


def analytic(nx, k):
    one, two, six = np.longdouble(1), np.longdouble(2), np.longdouble(6)
    h = one / np.longdouble(nx + 1)
    c = np.cos(np.arange(1, 8, dtype=np.longdouble) * (np.longdouble(4) * np.arctan(one)) * h)
    kap = six * (one - c) / (h * h * (two + c))
    return np.sort((kap[:, None] + kap[None, :]).ravel())[:k]


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
    a = ap.parse_args()
    if a.digest:
        return digest(a.digest, a.steps, a.nx * a.nx)
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    nx, n = a.nx, a.nx * a.nx
    q1 = torch.tensor(sg.eigsh_start_vector(n), device="cuda")
    A, B, Ps = problem(sg, nx)
    pc = sg.multigrid(Ps, omega=OMEGA)
    pc.setup(A)
    if a.trace:
        r = sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1, B=B)
        for rep in range(REPS):
            s = sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1, max_steps=CAP, want_V=False)
            g = sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1, max_steps=CAP, want_V=False, B=B)
        r0 = sg.davidson(A, K, ncv=NCV, tol=TOL, max_steps=2, q1=q1)
        torch.cuda.synchronize()
        print(json.dumps({"nx": nx, "rows": n, "k": K, "ncv": NCV, "steps": r.steps, "products": r.products, "products_B": r.products_B,
                          "restarts": r.restarts, "converged": r.converged, "capped_standard": [s.steps, s.restarts, s.converged],
                          "capped_generalized": [g.steps, g.restarts, g.converged], "unpreconditioned_steps": r0.steps}), flush=True)
        return
    rec = {"nx": nx, "rows": n, "k": K, "ncv": NCV, "tol": TOL, "kernel_A": A.kernel, "kernel_B": B.kernel, "reps": a.reps,
           "levels": len(Ps) + 1}
    exact = analytic(nx, K)
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros_like(x)
    rec["product_A_s"] = events(torch, lambda: A.matvec(x, y))
    rec["product_B_s"] = events(torch, lambda: B.matvec(x, y))
    rec["vcycle_apply_s"] = events(torch, lambda: pc.solve(A, y, x))
    t, r = timed(lambda: sg.davidson(A, K, pc=pc, ncv=NCV, tol=TOL, q1=q1, B=B), a.reps)
    rec["davidson_gen"] = {
        "seconds": t, "steps": r.steps, "products": r.products, "products_B": r.products_B, "applies": r.applies, "restarts": r.restarts,
        "converged": r.converged, "seconds_per_step": t / max(r.steps, 1), "lam": [float(v) for v in r.lam],
        "true_residuals": [float(v) for v in r.residuals],
        "distance_to_analytic": [float(abs(np.longdouble(v) - e)) for v, e in zip(r.lam, exact)]}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
