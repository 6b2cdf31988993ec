"""The multigrid preconditioner at C2 size: the 5-point Poisson matrix of an nx x nx grid, problems.interp2d_hierarchy, V(1,1)
with omega = 0.8 and 8 coarse sweeps, b = A * test_vector.  Timed with HIP events on the stream the library launches on
(setups: a host clock around a call that ends in a synchronisation); medians of --reps after --warmup.

  setup         first sgm_pc_setup (levels built by sgm_mat_ptap) and a second one after the values changed (refill)
  apply         one z = M^-1 r on device vectors; its compulsory bytes from the per-level count below, as a fraction of 8 TB/s
  apply_unfused the same apply with the fused sweep / residual kernels bypassed: a second build of the library whose
                sgm_mg.hip is compiled with -DSGM_MG_UNFUSED (`make -C tools mg_unfused`), run in a child process, and the
                two alternated (--alternations) so that they see the same machine
  solve         plain CG (the parent commit's code path) against V(1,1)-PCG, both to 1e-10, HIP events around the whole solve
                -> the gate: first setup + V(1,1)-PCG < plain CG

Compulsory bytes of one apply, level by level (mv(M) = what one product with M moves: its stored form, x once, y once --
sgm_mat_footprint; the transposed prolongation is counted like the prolongation):
  first sweep 24 n;  every further sweep mv(A_l) + 16 n (b, idiag);  residual mv(A_l) + 8 n (b);
  restriction mv(P_l);  prolongation mv(P_l) + 8 n (x read as well as written)

    python tools/mg_bench.py [--nx 3162] [--warmup 2] [--reps 7] [--out FILE]        one JSON line; exit 1 if the gate is missed
    python tools/mg_bench.py --solve-only                                             one setup + one solve (for a kernel trace)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
UNFUSED_LIB = os.path.join(ROOT, "tools", "mg_unfused", "libsigma_hip.so")
PEAK = 8.0e12
OMEGA, NU, COARSE, TOL = 0.8, 1, 8, 1e-10


def timed(f, warmup, reps):
    import torch
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts)), [round(t * 1e3, 4) for t in ts]


def problem(sg, nx):
    from sigma_amd import problems as P
    n = nx * nx
    ptr, node, val = P.poisson2d_csr(nx, nx)
    A = sg.csr_matrix(n, n, ptr, node, val)
    Ps = [sg.csr_matrix(nf, nc, p, nd, v) for p, nd, v, nf, nc in P.interp2d_hierarchy(nx, nx)]
    return A, Ps, P.test_vector(n)


def apply_bytes(pc, Ps):
    per_level, total = [], 0
    nl = len(Ps) + 1
    for l in range(nl):
        M = pc.level_handle(l)
        n, mv = M.nrow, M.footprint()[1]
        sweeps = COARSE - 1 if l == nl - 1 else 2 * NU - 1
        b = 24 * n + sweeps * (mv + 16 * n)
        if l < nl - 1:
            mp = Ps[l].footprint()[1]
            b += (mv + 8 * n) + mp + (mp + 8 * n)
        per_level.append({"level": l, "rows": n, "kernel": M.kernel, "bytes": int(b)})
        total += b
    return int(total), per_level


def child(a):
    """apply times only, with whatever library --lib names: one JSON line {"apply_s": [...]} per alternation on request"""
    import torch
    import sigma_amd as sg
    if a.lib:
        sg.LIB_PATH = a.lib
    sg.init(0)
    sg.use_torch_stream()
    A, Ps, xs = problem(sg, a.nx)
    pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
    pc.setup(A)
    r = torch.from_numpy(xs).cuda()
    z = torch.zeros_like(r)
    print(json.dumps({"ready": True, "paths": pc.paths().tolist()}), flush=True)
    for line in sys.stdin:                      # one measurement per line received: the parent alternates the two builds
        if line.strip() != "go":
            break
        t, ms = timed(lambda: pc.solve(A, z, r), a.warmup, a.reps)
        print(json.dumps({"apply_s": t, "apply_ms_all": ms}), flush=True)


def solve_only(a):
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    A, Ps, xs = problem(sg, a.nx)
    pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
    pc.setup(A)
    r = torch.from_numpy(xs).cuda()
    b, x = torch.zeros_like(r), torch.zeros_like(r)
    A.matvec(r, b)
    s = sg.cg(TOL)
    s.setup(A)
    s.solve(A, x, b, pc)
    torch.cuda.synchronize()
    print(json.dumps({"nx": a.nx, "pcg_iterations": s.last_iterations, "pcg_max_error": float((x - r).abs().max())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="(child) the library build to load")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--solve-only", action="store_true", help="one setup and one V(1,1)-PCG solve: the run a kernel trace is taken of")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.solve_only:
        return solve_only(a)
    import torch
    import sigma_amd as sg
    sg.init(0)
    sg.use_torch_stream()
    nx, n = a.nx, a.nx * a.nx
    A, Ps, xs = problem(sg, nx)
    rec = {"nx": nx, "rows": n, "levels": len(Ps) + 1, "omega": OMEGA, "nu": NU, "coarse_sweeps": COARSE, "tolerance": TOL}

    def setup_once(pc):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pc.setup(A)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    firsts = []
    for _ in range(3):                          # a fresh preconditioner each time: levels built by sgm_mat_ptap
        pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
        firsts.append(setup_once(pc))
        pc.destroy()
    pc = sg.multigrid(Ps, omega=OMEGA, nu_pre=NU, nu_post=NU, coarse_sweeps=COARSE)
    firsts.append(setup_once(pc))
    refills = []
    for _ in range(4):
        A.scalar_multiply(1.0)                  # the values "changed": version bumped, pattern kept
        refills.append(setup_once(pc))
    rec.update(setup_first_s=float(np.median(firsts[1:])), setup_first_s_all=firsts, setup_refill_s=float(np.median(refills)),
               setup_refill_s_all=refills, paths=pc.paths().tolist(), info=pc.info())

    r = torch.from_numpy(xs).cuda()
    z = torch.zeros_like(r)
    t_apply, apply_ms = timed(lambda: pc.solve(A, z, r), a.warmup, a.reps)
    nbytes, per_level = apply_bytes(pc, Ps)
    rec.update(apply_s=t_apply, apply_ms_all=apply_ms, apply_bytes=nbytes, apply_frac_8TBs=nbytes / t_apply / PEAK,
               apply_bytes_per_level=per_level)

    # time to solution
    b = torch.zeros_like(r)
    A.matvec(r, b)

    def solve(with_pc):
        s = sg.cg(TOL)
        s.setup(A)
        x = torch.zeros_like(b)
        t, ms = timed(lambda: (x.zero_(), s.solve(A, x, b, pc if with_pc else None)), 1, 3)
        err = float((x - r).abs().max())
        return t, ms, s.last_iterations, err       # (s.iterations adds up over the solves of the timing loop)
    t_pcg, pcg_ms, it_pcg, err_pcg = solve(True)
    t_cg, cg_ms, it_cg, err_cg = solve(False)
    rec.update(pcg_solve_s=t_pcg, pcg_ms_all=pcg_ms, pcg_iterations=it_pcg, pcg_max_error=err_pcg,
               cg_solve_s=t_cg, cg_ms_all=cg_ms, cg_iterations=it_cg, cg_max_error=err_cg,
               cg_over_pcg=t_cg / t_pcg, cg_over_pcg_with_first_setup=t_cg / (t_pcg + rec["setup_first_s"]),
               gate_pcg_with_setup_lt_cg=bool(t_pcg + rec["setup_first_s"] < t_cg))
    pc.destroy()
    del pc, A, Ps, r, z, b
    torch.cuda.empty_cache()

    # fused against unfused, alternated, each build in a process of its own
    if os.path.exists(UNFUSED_LIB):
        kids = {}
        for name, lib in (("fused", None), ("unfused", UNFUSED_LIB)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--nx", str(nx), "--warmup", str(a.warmup), "--reps", str(a.reps)]
            if lib:
                cmd += ["--lib", lib]
            k = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            kids[name] = (k, json.loads(k.stdout.readline()))
        runs = {"fused": [], "unfused": []}
        for _ in range(a.alternations):
            for name in ("fused", "unfused"):
                k = kids[name][0]
                k.stdin.write("go\n"); k.stdin.flush()
                runs[name].append(json.loads(k.stdout.readline())["apply_s"])
        for name in kids:
            k = kids[name][0]
            k.stdin.write("end\n"); k.stdin.flush()
            k.wait(timeout=120)
        rec.update(apply_fused_s_alternated=runs["fused"], apply_unfused_s_alternated=runs["unfused"],
                   unfused_paths=kids["unfused"][1]["paths"], apply_fused_s=float(np.median(runs["fused"])),
                   apply_unfused_s=float(np.median(runs["unfused"])),
                   unfused_over_fused=float(np.median(runs["unfused"]) / np.median(runs["fused"])))
    else:
        rec["apply_unfused_s"] = "not measured (tools/mg_unfused/libsigma_hip.so is not built: make -C tools mg_unfused)"
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    sys.exit(0 if rec["gate_pcg_with_setup_lt_cg"] else 1)


if __name__ == "__main__":
    main()
