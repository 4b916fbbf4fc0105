"""The spring chain as a device system against the same chain as a host callable
(writes profiles/chain_device.jsonl).

  solve    solver.ilqr_timeopt_batch on the chain at n = 24, m = 3, N = 60 (the problem
           data of tests/golden/make_golden_wide.py), B = 256 and B = 4096, with the
           systems.SpringChain itself and with SpringChain.host() (the vectorised NumPy
           callable): wall time, the four stage timers, and T* equal between the two.
           Device solves are warmed and alternated with nothing else on the device;
           the host solve is run once per batch size (it takes seconds).
  kernels  rollout, central linearisation and line search alone at B = 4096: medians of
           HIP-event times over alternated rounds in one process.  The linearisation's
           achieved store rate (A, B and a_res, algorithmic bytes) is set against the
           write ceiling tools/copy_ceiling.py measures (its fill_ of 4 GiB, run here in
           the same process and rounds); the line search is given per lane-step
           (B x n_alpha rows x 16 lanes x N steps).

    python tools/bench_chain.py [--no-host] [out.jsonl]
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from time_opt_ilqr_amd import engine, solver, systems  # noqa: E402
from time_opt_ilqr_amd.utils import as_terminal_weight  # noqa: E402

P, M, N, T_MIN, T_MAX, MAX_ITER = 12, 3, 60, 8, 55, 8


def event_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def problems(Bn):
    mk = [systems.make_spring_chain(P, M, N=N, seed=4024 + b) for b in range(Bn)]
    return mk[0], np.stack([q[1] for q in mk])


def solve(system, mk, x0, stage_timers):
    F, _, xg, ur, Q, R, alpha, w = mk[:8]
    t0 = time.perf_counter()
    res = solver.ilqr_timeopt_batch(system, x0, xg, ur, Q, R, as_terminal_weight(alpha, 2 * P), w,
                                    N, T_MIN, T_MAX, max_iter=MAX_ITER, stage_timers=stage_timers)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def bench_solves(out, host):
    for Bn in (256, 4096):
        mk, x0 = problems(Bn)
        F = mk[0]
        for _ in range(2):
            solve(F, mk, x0, False)
        walls = [solve(F, mk, x0, False)[0] for _ in range(5)]
        _, res = solve(F, mk, x0, True)
        rec = {"what": "solve", "B": Bn, "n": 2 * P, "m": M, "N": N, "max_iter": MAX_ITER,
               "device_wall_s": statistics.median(walls), "device_wall_s_all": walls,
               "device_timers_s": res["timers"], "iterations": res["iterations"],
               "crashed": int(res["crashed"].sum().item())}
        if host:
            wall_h, res_h = solve(F.host(), mk, x0, True)
            rec.update(host_wall_s=wall_h, host_timers_s=res_h["timers"],
                       t_star_equal=bool(torch.equal(res["T_star"], res_h["T_star"])),
                       host_over_device=wall_h / rec["device_wall_s"])
        out(rec)


def bench_kernels(out, dev):
    Bn = 4096
    mk, x0 = problems(Bn)
    F, _, xg, ur, Q, R, alpha, w = mk[:8]
    n, t = 2 * P, lambda a: torch.as_tensor(np.asarray(a, dtype=float), device=dev)  # noqa: E731
    U = 0.1 * torch.randn((Bn, N, M), dtype=torch.float64, device=dev)
    x0 = t(x0)
    X = engine.rollout(F, x0, U, F.dt)
    lin = engine.linearize(F, X, U, F.dt, central=True)
    Qf = as_terminal_weight(alpha, n)
    T = torch.full((Bn,), T_MAX, dtype=torch.int32, device=dev)
    ric = engine.riccati(lin.A, lin.B, X, U, t(xg), t(ur), t(Q), t(R), t(Qf), T, 1e-3, mode=0,
                         reg_max_tries=1)
    K, k = ric.K.clone(), ric.k.clone()
    K[:, T_MAX:], k[:, T_MAX:] = 0.0, 0.0
    cost = engine.CostParams(t(xg), t(ur), t(Q), t(R), t(Qf), float(w))
    fill = torch.empty((4 << 30) // 8, dtype=torch.float64, device=dev)
    fns = {"rollout": lambda: engine.rollout(F, x0, U, F.dt),
           "linearize_central": lambda: engine.linearize(F, X, U, F.dt, central=True),
           "linearize_forward": lambda: engine.linearize(F, X, U, F.dt, central=False),
           "linesearch": lambda: engine.forward_linesearch(F, X, U, T, K, k, cost, F.dt),
           "write_4GiB": lambda: fill.fill_(1.0)}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in fns}
    for _ in range(7):  # alternated rounds
        for name, fn in fns.items():
            ts[name] += event_ms(fn, 5)
    ms = {name: statistics.median(v) for name, v in ts.items()}
    write_gbs = fill.numel() * 8 / (ms["write_4GiB"] * 1e-3) / 1e9
    lin_bytes = Bn * N * (n * n + n * M + n) * 8
    n_alpha = len(engine.ALPHAS)
    rec = {"what": "kernels", "B": Bn, "n": n, "m": M, "N": N, "ms": ms,
           "write_ceiling_GB/s": write_gbs,
           "linearize_central_store_GB/s": lin_bytes / (ms["linearize_central"] * 1e-3) / 1e9,
           "linearize_forward_store_GB/s": lin_bytes / (ms["linearize_forward"] * 1e-3) / 1e9,
           "linesearch_ns_per_lane_step": ms["linesearch"] * 1e6 / (Bn * n_alpha * 16 * N),
           "linesearch_accepted_hist": torch.bincount(
               engine.forward_linesearch(F, X, U, T, K, k, cost, F.dt).accepted.long() + 2,
               minlength=n_alpha + 2).tolist()}
    rec["linearize_central_frac_of_write"] = rec["linearize_central_store_GB/s"] / write_gbs
    out(rec)


def main():
    dev = torch.device("cuda", 0)
    files = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = files[0] if files else os.path.join(REPO, "profiles", "chain_device.jsonl")
    open(path, "w").close()

    def out(rec):  # one line per record, written as it is measured
        print(json.dumps(rec), flush=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    bench_kernels(out, dev)
    bench_solves(out, "--no-host" not in sys.argv)


if __name__ == "__main__":
    main()
