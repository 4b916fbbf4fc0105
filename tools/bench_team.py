"""Teams as device systems (writes profiles/team_device.jsonl).

1. Whole solves (solver.ilqr_timeopt_batch, method="propagator") of the teams quad_pm3
   (quadrotor + 3 point masses, n = 24, m = 10) and quad_di4_pm2 (quadrotor + 4 DI + 2 point
   masses, n = 28, m = 12), N = 80 -- the problems of systems.make_team, one seed per
   problem -- at B = 1, 256 and 4096: the systems.Team itself against the same team wrapped
   as host_dynamics.HostDynamics (Team.host(), the vectorised NumPy twin).  Both run in one
   process, alternated; the device solve is warmed and its wall time is the median over the
   rounds; the host solve runs once per round (one round at B = 4096, where it takes
   minutes).  max_iter is small (default 2) for the same reason; T* of the two is compared.

2. What a mixed row costs: the kernel times (HIP events, warmed, B = 4096, one process) of
   every entry for a team of equal members against the fleet of them, alternated with the
   order flipped each round -- Team([2, 2]) against Fleet(2, 2) at N = 80 and Team([0] * 15)
   against Fleet(0, 15) at N = 60 -- and for the team of all five kinds (n = 26, m = 9,
   dt = 0.02, N = 80), whose rows diverge five ways in every step.

    python tools/bench_team.py [--max-iter K] [--rounds R] [--no-host] [--no-solves] [out.jsonl]

With --proximity (writes profiles/team_proximity.jsonl) it measures the
teams' proximity cost instead, on the crossing problems of systems.make_team_crossing at
B = 4,096: the Taylor kernel's time and bytes against the 2 GiB copy of
tools/copy_ceiling.py timed in the same process; the same for the fleet's Taylor kernel
against the team's on equal-member pairs, alternated with the order flipped each round; the
cost and line-search kernels with and without the term, alternated; and a whole solve on
the device against Team.host() with stage_cost() at B = 64.
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

# tag, members, N, w_scale, T_min: the settings of the whole-solve fixtures
TEAMS = (("quad_pm3", (2, 3, 3, 3), 80, 1600.0, 15),
         ("quad_di4_pm2", (2, 0, 0, 0, 0, 3, 3), 80, 1600.0, 15))
BATCHES = (1, 256, 4096)
KERNEL_B = 4096


def _opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def problems(ids, N, w_scale, T_min, Bn):
    mk = systems.make_team(ids, N=N, seed=7000, w_scale=w_scale, T_min=T_min)
    x0 = np.stack([systems.make_team(ids, N=N, seed=7000 + b, w_scale=w_scale)[1]
                   for b in range(Bn)])
    return mk, x0


def solve(system, mk, x0, max_iter, stage_timers):
    _, _, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap, _ = mk
    t0 = time.perf_counter()
    res = solver.ilqr_timeopt_batch(system, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                    max_iter=max_iter, wrap_idx=wrap, stage_timers=stage_timers)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, res


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


def entries(mk, Bn, dev):
    """name -> fn(system): every entry on one set of inputs (the maker's problem, inputs
    near u_ref, small gains)"""
    F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap, _ = mk
    tt = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)  # noqa: E731
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    kw = dict(device=dev, dtype=torch.float64, generator=g)
    n, m = F.n, F.m
    x0b = tt(x0) + 0.05 * torch.randn((Bn, n), **kw)
    # small enough that no quadrotor meets its pitch guard in N steps
    U = tt(ur) + 0.002 * torch.randn((Bn, N, m), **kw)
    X = engine.rollout(F, x0b, U, F.dt)
    assert bool(torch.isfinite(X).all())
    K = 0.01 * torch.randn((Bn, N, m, n), **kw)
    k = 0.002 * torch.randn((Bn, N, m), **kw)
    T = torch.full((Bn,), T_max, dtype=torch.int32, device=dev)
    cost = engine.CostParams(tt(xg), tt(ur), tt(Q), tt(R), tt(Qf), float(w), None, wrap)
    Xs, Us = X[:, :N].reshape(-1, n).contiguous(), U.reshape(-1, m).contiguous()
    return {
        "dynamics": lambda S: engine.dynamics(S, Xs, Us, F.dt),
        "rollout": lambda S: engine.rollout(S, x0b, U, F.dt),
        "linearize_central": lambda S: engine.linearize(S, X, U, F.dt, central=True),
        "linearize_forward": lambda S: engine.linearize(S, X, U, F.dt, central=False),
        "cost_true": lambda S: engine.cost_true(S, X, U, T, cost),
        "linesearch": lambda S: engine.forward_linesearch(S, X, U, T, K, k, cost, F.dt),
    }


def kernel_rows(out, rounds):
    dev = torch.device("cuda", torch.cuda.current_device())
    Bn = KERNEL_B
    for sid, count, N in ((2, 2, 80), (0, 15, 60)):
        mk = systems.make_fleet(sid, count, N=N, seed=7000, w_scale=100.0)
        Fl, Tm = mk[0], systems.Team([sid] * count)
        for name, fn in entries(mk, Bn, dev).items():
            a, b = fn(Fl), fn(Tm)
            same = all(torch.equal(getattr(a, key), getattr(b, key)) for key in
                       (("A", "B", "a_res") if name.startswith("linearize") else
                        ("X", "U", "J", "J_old", "accepted") if name == "linesearch" else ())) \
                if not torch.is_tensor(a) else bool(torch.equal(a, b))
            del a, b
            t = {"fleet": [], "team": []}
            for r in range(rounds * 2):
                for key, S in ((("fleet", Fl), ("team", Tm)) if r % 2 == 0 else
                               (("team", Tm), ("fleet", Fl))):
                    t[key].append(_events(lambda: fn(S)))
            fm, tm = statistics.median(t["fleet"]), statistics.median(t["team"])
            out({"what": "kernel", "fleet": Fl.name, "team": Tm.name, "entry": name, "B": Bn,
                 "n": Fl.n, "m": Fl.m, "N": N, "fleet_ms": fm, "team_ms": tm,
                 "team_over_fleet": tm / fm, "bitwise_equal": same, "fleet_ms_all": t["fleet"],
                 "team_ms_all": t["team"]})
    mk = systems.make_team((0, 1, 2, 3, 4), N=80, seed=7000, dt=0.02)
    F = mk[0]
    for name, fn in entries(mk, Bn, dev).items():
        ts = [_events(lambda: fn(F)) for _ in range(rounds * 2)]
        out({"what": "kernel", "team": F.name, "entry": name, "B": Bn, "n": F.n, "m": F.m,
             "N": 80, "team_ms": statistics.median(ts), "team_ms_all": ts})


# ---- the proximity cost (--proximity; profiles/team_proximity.jsonl)
PROX_TEAMS = (("quad_pm3", (2, 3, 3, 3), 80, 1600.0, 40), ("pm_quad_di", (3, 2, 0), 80, 1600.0, 15),
              ("di2_pm2", (0, 0, 3, 3), 80, 1600.0, 10))  # tag members N w_scale T_min
PROX_PAIRS = ((3, 7, 80), (2, 2, 80), (0, 15, 60))  # base count N: Fleet against Team of equals
PROX_HOST_B = 64


def proximity_rows(out, max_iter, rounds, host):
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
    Bn = KERNEL_B

    def rate(ms, n, rows):  # reads n, writes n^2 + n + 1 doubles per state row
        written = rows * (n * n + n + 1) * 8
        gbs = (written + rows * n * 8) / (ms * 1e-3) / 1e9
        return {"ms": ms, "bytes_written": written, "GB/s": gbs, "share_of_copy_rate": gbs / copy_gbs}

    # 1. the fleet's Taylor kernel against the team's on equal members, alternated
    for sid, count, N in PROX_PAIRS:
        mk = systems.make_fleet_crossing(sid, count, N=N, seed=7000, w_scale=1600.0)
        Fl = mk[0]
        Tm = systems.Team([sid] * count).with_proximity(Fl.proximity)
        x0b = np.stack([systems.make_fleet_crossing(sid, count, N=N, seed=7000 + b,
                                                    w_scale=1600.0)[1] for b in range(Bn)])
        U = tt(mk[3]) + 0.05 * torch.randn((Bn, N, Fl.m), **kw)
        Xs = engine.rollout(Fl, tt(x0b), U, Fl.dt)[:, :N].contiguous()
        a, b = engine.fleet_proximity_cost(Fl, Xs), engine.team_proximity_cost(Tm, Xs)
        # the bit patterns: a rollout that met the quadrotor's guard holds NaN rows
        same = all(torch.equal(p.view(torch.int64), q.view(torch.int64)) for p, q in zip(a, b))
        nan_rows = int(torch.isnan(Xs).any(-1).sum().item())
        del a, b
        t = {"fleet": [], "team": []}
        for r in range(rounds * 2):
            for key in (("fleet", "team") if r % 2 == 0 else ("team", "fleet")):
                fn = (lambda: engine.fleet_proximity_cost(Fl, Xs)) if key == "fleet" else \
                    (lambda: engine.team_proximity_cost(Tm, Xs))
                t[key].append(_events(fn))
        fm, tm = statistics.median(t["fleet"]), statistics.median(t["team"])
        out({"what": "taylor_pair", "fleet": Fl.name, "team": Tm.name, "B": Bn, "N": N, "n": Fl.n,
             "fleet_taylor": rate(fm, Fl.n, Bn * N), "team_taylor": rate(tm, Fl.n, Bn * N),
             "team_over_fleet": tm / fm, "bitwise_equal": same, "nan_state_rows": nan_rows,
             "fleet_ms_all": t["fleet"],
             "team_ms_all": t["team"]})
        del Xs, U
    for tag, ids, N, w_scale, T_min in PROX_TEAMS:
        mk = systems.make_team_crossing(ids, N=N, seed=7000, w_scale=w_scale, T_min=T_min)
        F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap, _ = mk
        plain = systems.Team(F.member_ids, dt=F.dt)
        n, m = F.n, F.m
        x0b = np.stack([systems.make_team_crossing(ids, N=N, seed=7000 + b, w_scale=w_scale)[1]
                        for b in range(Bn)])
        # small enough that no quadrotor meets its pitch guard in N steps
        U = tt(ur) + 0.002 * torch.randn((Bn, N, m), **kw)
        X = engine.rollout(F, tt(x0b), U, F.dt)
        assert bool(torch.isfinite(X).all())
        rec = {"team": tag, "members": list(ids), "B": Bn, "n": n, "m": m, "N": N}
        # 2. the Taylor kernel
        Xs = X[:, :N].contiguous()
        ms = _events(lambda: engine.team_proximity_cost(F, Xs))
        out(dict(rec, what="taylor", **rate(ms, n, Bn * N)))
        # 3. cost and line search, plain and with the term, alternated
        lin = engine.linearize(F, X, U, F.dt, central=True)
        T = torch.full((Bn,), T_max, dtype=torch.int32, device=dev)
        ex = dict(zip(("c_extra", "qx_extra", "qxx_extra"), engine.team_proximity_cost(F, Xs)))
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
        if not host:
            continue
        # 4. a whole solve at PROX_HOST_B problems against Team.host() with stage_cost(): the
        # host evaluates the Python stage cost state by state
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
                 device_timers_s=res["timers"], host_wall_s=hw, host_timers_s=res_h["timers"],
                 t_star_equal=bool(torch.equal(res["T_star"], res_h["T_star"])),
                 host_over_device=hw / statistics.median(dev_s)))


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".jsonl")]
    if "--proximity" in sys.argv:
        path = files[0] if files else os.path.join(REPO, "profiles", "team_proximity.jsonl")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        open(path, "w").close()

        def out(rec):
            print(json.dumps(rec), flush=True)
            with open(path, "a") as f:
                f.write(json.dumps(rec) + "\n")

        proximity_rows(out, _opt("--max-iter", 2), _opt("--rounds", 3), "--no-host" not in sys.argv)
        return
    path = files[0] if files else os.path.join(REPO, "profiles", "team_device.jsonl")
    max_iter, rounds, host = _opt("--max-iter", 2), _opt("--rounds", 3), "--no-host" not in sys.argv
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    open(path, "w").close()

    def out(rec):  # one line per record, written as it is measured
        print(json.dumps(rec), flush=True)
        with open(path, "a") as f:
            f.write(json.dumps(rec) + "\n")

    kernel_rows(out, rounds)
    if "--no-solves" in sys.argv:
        return
    for tag, ids, N, w_scale, T_min in TEAMS:
        for Bn in BATCHES:
            mk, x0 = problems(ids, N, w_scale, T_min, Bn)
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
            rec = {"what": "solve", "team": tag, "members": list(ids), "B": Bn, "n": F.n,
                   "m": F.m, "N": N, "max_iter": max_iter,
                   "device_wall_s": statistics.median(dev_s), "device_wall_s_all": dev_s,
                   "device_timers_s": res["timers"], "iterations": res["iterations"],
                   "crashed": int(res["crashed"].sum().item())}
            if host:
                rec.update(host_wall_s=statistics.median(host_s), host_wall_s_all=host_s,
                           host_timers_s=res_h["timers"],
                           t_star_equal=bool(torch.equal(res["T_star"], res_h["T_star"])),
                           host_over_device=statistics.median(host_s) / rec["device_wall_s"])
            out(rec)


if __name__ == "__main__":
    main()
