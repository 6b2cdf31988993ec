"""Re-assembly of a P1 finite-element matrix on a fixed mesh through an edit plan, at C2 size: nx x nx nodes, two triangles per
cell, the 9 (i, j) of every element in fem.f90's order (m = 18 (nx-1)^2 triples, chains of 6 on the diagonal), z resident
on the device.  Timed with HIP events on the stream the library launches on (median of --reps after --warmup):

  apply        plan.add(z, zero_first=True)                        the new route
  old route    device-to-host copy of z (8 m bytes, into pinned and into pageable memory) + sgm_csr_set_values(host values):
               what the parent commit has to MOVE, its host accumulation loop not counted        -> the gate: apply < old route
  set          sgm_csr_set_values(device values): the copy + repack tail an apply shares         -> accumulate = apply - set
  accumulate over its compulsory bytes 12 m + 16 * slots addressed, as a fraction of 8 TB/s (aim 0.25; recorded, not gated)

    python tools/edit_bench.py [--nx 3162] [--warmup 2] [--reps 7] [--out FILE]        one JSON line; exit 1 if the gate is missed
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigma_amd as sg  # noqa: E402

PEAK = 8.0e12


def stream_indices(nx, dev):
    """(i, j) of the element stream on the device: for n: for j: for i: (ele(i,n), ele(j,n)), 1-based int32"""
    c = torch.arange((nx - 1) * (nx - 1), device=dev, dtype=torch.int64)
    a = (c // (nx - 1)) * nx + c % (nx - 1) + 1
    b, cc, d = a + 1, a + nx, a + nx + 1
    ele = torch.stack([torch.stack([a, b, d], 1), torch.stack([a, d, cc], 1)], 1).reshape(-1, 3)      # (ne, 3)
    ti = ele[:, None, :].expand(-1, 3, -1).reshape(-1).to(torch.int32)       # i fastest
    tj = ele[:, :, None].expand(-1, -1, 3).reshape(-1).to(torch.int32)
    return ti.contiguous(), tj.contiguous()


def timed(f, warmup, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nx", type=int, default=3162)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sg.init(0)
    sg.use_torch_stream()
    dev = torch.device("cuda:0")
    nx, nn = a.nx, a.nx * a.nx
    ti, tj = stream_indices(nx, dev)
    m = ti.numel()
    z = torch.rand(m, device=dev, dtype=torch.float64) + 0.5
    t0 = time.perf_counter()
    A = sg.csr_matrix.from_edges(nn, nn, ti, tj, torch.zeros_like(z))
    t_pattern = time.perf_counter() - t0
    t0 = time.perf_counter()
    plan = sg.edit_plan(A, ti, tj)
    t_plan = time.perf_counter() - t0
    info = plan.info()
    nnz = info["slots"]
    t_apply, apply_ms = timed(lambda: plan.add(z, zero_first=True), a.warmup, a.reps)
    t_apply_top, _ = timed(lambda: plan.add(z), 1, a.reps)
    dval = torch.from_numpy(A.get("val", np.float64)).to(dev)
    t_set, set_ms = timed(lambda: A.set_values(dval), a.warmup, a.reps)
    # the parent commit's only route: z to the host, (its accumulation loop, not counted,) the values back up
    pinned = torch.empty(m, dtype=torch.float64, pin_memory=True)
    t_d2h_pinned, _ = timed(lambda: (pinned.copy_(z, non_blocking=False), torch.cuda.synchronize()), 1, 5)
    pageable = torch.empty(m, dtype=torch.float64)
    t_d2h_pageable, _ = timed(lambda: (pageable.copy_(z), torch.cuda.synchronize()), 1, 5)
    hval = dval.cpu().numpy()
    t_set_host, _ = timed(lambda: A.set_values(hval), 1, 5)
    old = min(t_d2h_pinned, t_d2h_pageable) + t_set_host
    acc = t_apply - t_set
    acc_bytes = 12 * m + 16 * nnz
    rec = {"nx": nx, "rows": nn, "kernel": A.kernel, "m": m, "slots_addressed": nnz, "longest_chain": info["longest_chain"],
           "stored_sources": info["stored_sources"], "padding_factor": info["stored_sources"] / m,
           "pattern_from_edges_s": t_pattern, "plan_create_s": t_plan,
           "apply_zero_first_s": t_apply, "apply_zero_first_ms_all": apply_ms, "apply_on_top_s": t_apply_top,
           "set_values_device_s": t_set, "set_values_device_ms_all": set_ms, "repack_share_of_apply_upper": t_set / t_apply,
           "old_d2h_pinned_s": t_d2h_pinned, "old_d2h_pageable_s": t_d2h_pageable, "old_set_values_host_s": t_set_host,
           "old_route_s": old, "gate_apply_lt_old_route": bool(t_apply < old), "old_route_over_apply": old / t_apply,
           "accumulate_s": acc, "accumulate_bytes": acc_bytes, "accumulate_frac_8TBs": acc_bytes / max(acc, 1e-9) / PEAK,
           "apply_bytes_with_tail_frac_8TBs": (acc_bytes + 0) / t_apply / PEAK}
    print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
    plan.destroy()
    sys.exit(0 if rec["gate_apply_lt_old_route"] else 1)


if __name__ == "__main__":
    main()
