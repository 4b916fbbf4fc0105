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

With --proximity (writes profiles/fleet_proximity.jsonl) it measures the
fleets' proximity cost instead, on the crossing problems of systems.make_fleet_crossing
(quadrotor x 2 and point mass x 7, N = 80, B = 4096), device events, warmed, one process:
the Taylor kernel's time and bytes against a 2 GiB copy timed in the same process; the cost
and line-search kernels with and without the proximity term, alternated; a whole solve on
the device, and at B = 64 against Fleet.host() with stage_cost() as extra_stage_cost.
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


# ---- the proximity cost (--proximity; profiles/fleet_proximity.jsonl)
PROX_FLEETS = (("quadrotor", 2, 80, 1600.0), ("pointmass", 7, 80, 1600.0))  # base count N w_scale
PROX_B, PROX_HOST_B = 4096, 64


def _events(fn, iters=10, warm=5):
    """median ms of fn() over `iters` launches (HIP events), warmed"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def proximity_rows(out, max_iter, rounds, host):
    """The Taylor kernel against the chip's copy rate measured in this process, the cost and
    line-search kernels with and without the proximity term (alternated), and a whole solve
    on the device against Fleet.host() with stage_cost()."""
    from time_opt_ilqr_amd import engine
    dev = torch.device("cuda", torch.cuda.current_device())
    tt = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    kw = dict(device=dev, dtype=torch.float64, generator=g)
    # tools/copy_ceiling.py's "copy": 2 GiB -> 2 GiB, half reads, half writes
    buf = torch.empty((4 << 30) // 8, dtype=torch.float64, device=dev).normal_()
    src, dst = buf[:buf.numel() // 2], buf[buf.numel() // 2:]
    copy_ms = _events(lambda: dst.copy_(src))
    copy_gbs = 2 * src.numel() * 8 / (copy_ms * 1e-3) / 1e9
    out({"what": "copy", "ms": copy_ms, "GB/s": copy_gbs})
    del buf, src, dst
    Bn = PROX_B
    for base, count, N, w_scale in PROX_FLEETS:
        mk = systems.make_fleet_crossing(base, count, N=N, seed=7000, w_scale=w_scale)
        F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap, _ = mk
        plain = systems.Fleet(F.base_id, F.count)
        n, m = F.n, F.m
        x0b = np.stack([systems.make_fleet_crossing(base, count, N=N, seed=7000 + b,
                                                    w_scale=w_scale)[1] for b in range(Bn)])
        U = tt(ur) + 0.05 * torch.randn((Bn, N, m), **kw)
        X = engine.rollout(F, tt(x0b), U, F.dt)
        rec = {"fleet": F.name, "B": Bn, "n": n, "m": m, "N": N}
        # 1. the Taylor kernel: reads n, writes n^2 + n + 1 doubles per state row
        Xs = X[:, :N].contiguous()
        ms = _events(lambda: engine.fleet_proximity_cost(F, Xs))
        written = Bn * N * (n * n + n + 1) * 8
        gbs = (written + Bn * N * n * 8) / (ms * 1e-3) / 1e9
        out(dict(rec, what="taylor", ms=ms, bytes_written=written, **{"GB/s": gbs},
                 share_of_copy_rate=gbs / copy_gbs))
        # 2. cost and line search, plain and with the term, alternated
        lin = engine.linearize(F, X, U, F.dt, central=True)
        T = torch.full((Bn,), T_max, dtype=torch.int32, device=dev)
        ex = dict(zip(("c_extra", "qx_extra", "qxx_extra"), engine.fleet_proximity_cost(F, Xs)))
        ric = engine.riccati(lin.A, lin.B, X, U, tt(xg), tt(ur), tt(Q), tt(R), tt(Qf), T, 1e-3,
                             mode=0, reg_max_tries=1, wrap_idx=wrap, **ex)
        K, k = ric.K.clone(), ric.k.clone()
        K[:, T_max:], k[:, T_max:] = 0.0, 0.0
        del lin, ric, ex
        cost = engine.CostParams(tt(xg), tt(ur), tt(Q), tt(R), tt(Qf), float(w), None, wrap)
        for name, fn in (("cost_true", lambda S: engine.cost_true(S, X, U, T, cost)),
                         ("linesearch", lambda S: engine.forward_linesearch(S, X, U, T, K, k, cost,
                                                                            F.dt))):
            t = {"plain": [], "proximity": []}
            for r in range(rounds * 2):
                for key, S in ((("plain", plain), ("proximity", F)) if r % 2 == 0 else
                               (("proximity", F), ("plain", plain))):
                    t[key].append(_events(lambda: fn(S)))
            pm, xm = statistics.median(t["plain"]), statistics.median(t["proximity"])
            out(dict(rec, what=name, plain_ms=pm, proximity_ms=xm, ratio=xm / pm,
                     plain_ms_all=t["plain"], proximity_ms_all=t["proximity"]))
        del K, k, X, U, Xs
        # 3. a whole solve on the device against Fleet.host() with stage_cost()
        for _ in range(2):
            solve(F, mk, x0b, max_iter, False)
        dev_s = [solve(F, mk, x0b, max_iter, False)[0] for _ in range(rounds)]
        _, res = solve(F, mk, x0b, max_iter, True)
        r = dict(rec, what="solve", max_iter=max_iter, device_wall_s=statistics.median(dev_s),
                 device_wall_s_all=dev_s, device_timers_s=res["timers"],
                 iterations=res["iterations"], crashed=int(res["crashed"].sum().item()))
        out(r)
        if host:
            # the host evaluates the Python stage cost state by state (minutes at B = 4,096):
            # the comparison runs at PROX_HOST_B problems, the device warmed at that size
            xh = x0b[:PROX_HOST_B]
            for _ in range(2):
                solve(F, mk, xh, max_iter, False)
            dev_s = [solve(F, mk, xh, max_iter, False)[0] for _ in range(rounds)]
            _, res = solve(F, mk, xh, max_iter, True)
            t0 = time.perf_counter()
            res_h = solver.ilqr_timeopt_batch(F.host(), xh, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                              max_iter=max_iter, wrap_idx=wrap,
                                              extra_stage_cost=F.stage_cost())
            torch.cuda.synchronize()
            hw = time.perf_counter() - t0
            out(dict(rec, what="solve_vs_host", B=PROX_HOST_B, max_iter=max_iter,
                     device_wall_s=statistics.median(dev_s), device_wall_s_all=dev_s,
                     host_wall_s=hw, host_timers_s=res_h["timers"],
                     t_star_equal=bool(torch.equal(res["T_star"], res_h["T_star"])),
                     host_over_device=hw / statistics.median(dev_s)))


def main():
    if "--proximity" in sys.argv:
        files = [a for a in sys.argv[1:] if a.endswith(".jsonl")]
        path = files[0] if files else os.path.join(REPO, "profiles", "fleet_proximity.jsonl")
        open(path, "w").close()

        def out(rec):
            print(json.dumps(rec), flush=True)
            with open(path, "a") as f:
                f.write(json.dumps(rec) + "\n")

        proximity_rows(out, _opt("--max-iter", 2), _opt("--rounds", 3), "--no-host" not in sys.argv)
        return
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
