"""Fleets as device systems against the same fleets as host callables (writes
profiles/fleet_device.jsonl).

Whole solves (solver.ilqr_timeopt_batch, method="propagator") of quadrotor x 2 (n = 24,
m = 8, N = 80) and double integrator x 15 (n = 30, m = 15, N = 60) -- the problems of
systems.make_fleet, one seed per problem -- at B = 1, 256 and 4096:

  device  the systems.Fleet itself: rollout, FD linearisation, true cost and line search
          in csrc/fleet.hip;
  host    the same fleet wrapped as host_dynamics.HostDynamics (Fleet.host(), the
          vectorised NumPy twin): what a wide system that comes as a callable costs.

Both run on the same tree in one process, alternated (device, host, device, ...): the
device solve is warmed and its wall time is the median over the rounds; the host solve
is run once per round.  max_iter is small (default 2: the warm update and two
iterations) because the host side takes minutes at B = 4096; the ratio is per solve of
that length.  T* of the two is compared.

    python tools/bench_fleet.py [--max-iter K] [--rounds R] [--no-host] [out.jsonl]
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

FLEETS = (("quadrotor", 2, 80, 100.0), ("double_integrator", 15, 60, 100.0))  # base count N w_scale
BATCHES = (1, 256, 4096)


def _opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def problems(base, count, N, w_scale, Bn):
    mk = systems.make_fleet(base, count, N=N, seed=7000, w_scale=w_scale)
    x0 = np.stack([systems.make_fleet(base, count, N=N, seed=7000 + b, w_scale=w_scale)[1]
                   for b in range(Bn)])
    return mk, x0


def solve(system, mk, x0, max_iter, stage_timers):
    _, _, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap, _ = mk
    t0 = time.perf_counter()
    res = solver.ilqr_timeopt_batch(system, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                    max_iter=max_iter, wrap_idx=wrap, stage_timers=stage_timers)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".jsonl")]
    path = files[0] if files else os.path.join(REPO, "profiles", "fleet_device.jsonl")
    max_iter, rounds, host = _opt("--max-iter", 2), _opt("--rounds", 3), "--no-host" not in sys.argv
    open(path, "w").close()

    def out(rec):  # one line per record, written as it is measured
        print(json.dumps(rec), flush=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    for base, count, N, w_scale in FLEETS:
        for Bn in BATCHES:
            mk, x0 = problems(base, count, N, w_scale, Bn)
            F = mk[0]
            H = F.host()
            for _ in range(2):
                solve(F, mk, x0, max_iter, False)
            dev_s, host_s, res, res_h = [], [], None, None
            # the host solve at B = 4096 takes minutes: one round there
            for _ in range(rounds if Bn < 4096 else 1):
                dev_s.append(solve(F, mk, x0, max_iter, False)[0])
                if host:
                    wall, res_h = solve(H, mk, x0, max_iter, True)
                    host_s.append(wall)
            dev_s.append(solve(F, mk, x0, max_iter, False)[0])
            _, res = solve(F, mk, x0, max_iter, True)
            rec = {"what": "solve", "fleet": F.name, "B": Bn, "n": F.n, "m": F.m, "N": N,
                   "max_iter": max_iter, "device_wall_s": statistics.median(dev_s),
                   "device_wall_s_all": dev_s, "device_timers_s": res["timers"],
                   "iterations": res["iterations"], "crashed": int(res["crashed"].sum().item())}
            if host:
                rec.update(host_wall_s=statistics.median(host_s), host_wall_s_all=host_s,
                           host_timers_s=res_h["timers"],
                           t_star_equal=bool(torch.equal(res["T_star"], res_h["T_star"])),
                           host_over_device=statistics.median(host_s) / rec["device_wall_s"])
            out(rec)


if __name__ == "__main__":
    main()
