"""The one-pass window method (baseline2) on the device against the propagator and the
brute-force select (writes profiles/onepass_device.jsonl).

  solve    solver.ilqr_timeopt_batch on the quadrotor maker's problem (N = 160, its T_min
           and T_max, max_iter = 15, S_window = 20: ilqr_timeopt's defaults) at
           B = 1, 256 and 4096, x0 drawn as run_suite draws it (sigma 0.4 on the position),
           problem 0 the maker's own start.  Whole solves, warmed, the three methods
           alternated round by round in one process; wall times without stage timers,
           then one solve per method with them.  T* of every method: problem 0's, and how
           many problems agree with the propagator.
  ref      at B = 1 the device one-pass wall time against the reference's own one-pass
           time on this problem, 2.951 s (the onepass row of its plots/summary.csv).

    python tools/bench_onepass.py [--quick] [out.jsonl]
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

from time_opt_ilqr_amd import solver, systems  # noqa: E402
from time_opt_ilqr_amd.utils import as_terminal_weight  # noqa: E402

METHODS = ("propagator", "bruteforce", "onepass")
MAX_ITER, S_WINDOW = 15, 20
REFERENCE_ONEPASS_S = 2.951  # plots/summary.csv of the reference, Quadrotor, onepass


def problems(Bn):
    mk = systems.make_quadrotor()
    x0 = np.tile(np.asarray(mk[1], dtype=float), (Bn, 1))
    rng = np.random.default_rng(0)
    x0[1:, :3] += 0.4 * rng.standard_normal((Bn - 1, 3))
    return mk, x0


def solve(mk, x0, method, stage_timers):
    F, _, xg, ur, Q, R, alpha, w, N, T_min, T_max, wrap_idx, _ = mk
    t0 = time.perf_counter()
    res = solver.ilqr_timeopt_batch(F.system_id, x0, xg, ur, Q, R, as_terminal_weight(alpha, 12),
                                    w, N, T_min, T_max, dt=F.dt, max_iter=MAX_ITER,
                                    wrap_idx=wrap_idx, method=method, S_window=S_WINDOW,
                                    stage_timers=stage_timers)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def main():
    files = [a for a in sys.argv[1:] if not a.startswith("--")]
    path = files[0] if files else os.path.join(REPO, "profiles", "onepass_device.jsonl")
    quick = "--quick" in sys.argv
    open(path, "w").close()

    def out(rec):  # one line per record, written as it is measured
        print(json.dumps(rec), flush=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    for Bn in (1, 256) if quick else (1, 256, 4096):
        mk, x0 = problems(Bn)
        walls = {m: [] for m in METHODS}
        warm = {m: solve(mk, x0, m, False)[0] for m in METHODS}
        # a solve that takes seconds is not repeated five times
        rounds = 5 if max(warm.values()) < 2.0 else 2
        for _ in range(rounds):  # alternated rounds
            for m in METHODS:
                walls[m].append(solve(mk, x0, m, False)[0])
        rec = {"what": "solve", "system": "quadrotor", "B": Bn, "N": int(mk[8]),
               "T_min": int(mk[9]), "T_max": int(mk[10]), "max_iter": MAX_ITER,
               "S_window": S_WINDOW, "rounds": rounds}
        base = None
        for m in METHODS:
            _, res = solve(mk, x0, m, True)
            T = res["T_star"]
            base = T if base is None else base
            rec[m] = {"wall_s": statistics.median(walls[m]), "wall_s_all": walls[m],
                      "first_call_s": warm[m], "timers_s": res["timers"],
                      "iterations": res["iterations"], "T_star_problem0": int(T[0].item()),
                      "T_star_equal_to_propagator": int((T == base).sum().item()),
                      "crashed": int(res["crashed"].sum().item()),
                      "J_final_problem0": float(res["J_hist"][0, max(
                          int(res["n_hist"][0].item()) - 1, 0)].item())}
        if "onepass_failed" in res:
            rec["onepass"]["sweep_failures"] = int((res["onepass_failed"] != 0).sum().item())
        rec["onepass_over_propagator"] = rec["onepass"]["wall_s"] / rec["propagator"]["wall_s"]
        rec["onepass_over_bruteforce"] = rec["onepass"]["wall_s"] / rec["bruteforce"]["wall_s"]
        if Bn == 1:
            rec["reference_onepass_s"] = REFERENCE_ONEPASS_S
            rec["reference_over_device"] = REFERENCE_ONEPASS_S / rec["onepass"]["wall_s"]
        out(rec)


if __name__ == "__main__":
    main()
