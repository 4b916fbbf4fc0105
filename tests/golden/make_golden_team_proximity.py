"""Generate the team proximity goldens (team_prox_solve_*.npz, team_prox_cases_*.npz) by
running the REFERENCE with the NumPy bump cost of a team as extra_stage_cost.

Run as make_golden_team.py is run, from outside both trees:

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_team_proximity.py
        [REFERENCE_DIR] [--only TAG[,TAG...]] [--cases-only | --solves-only] [--out DIR]

It imports the reference's solver, linearisation and makers from that directory (read only,
no bytecode written).  A team stacks members of different reference systems as in
make_golden_team.py.  Every file holds data only.

The cost (bump_cost() below; time_opt_ilqr_amd.systems.Team.stage_cost is its twin, and
include/hop_mixed_proximity.h states it).  Positions live in a workspace of dimension D, the
largest pd among the members (pd: 1 DI, cart-pole, segway; 2 point mass; 3 quadrotor);
member a's workspace position P_a is its pd_a leading state entries padded with zeros to D.
g(d; r, w) = w exp(-|d|^2 / (2 r^2)), |d|^2 over all D coordinates, between every member and
every obstacle row (o [D], r, w) and between every pair a < b.  Gradient -(c / r^2) d and
second-order term H = c d d^T / r^4, each restricted to the pd_a (and pd_b) coordinates the
members have: +H[:pd_a, :pd_a], +H[:pd_b, :pd_b], -H[:pd_a, :pd_b] and its transpose.

Whole solves (team_prox_solve_<tag>_<i>.npz).  Problem data (problem() below, repeated by
time_opt_ilqr_amd.systems.make_team_crossing): make_golden_fleet_proximity.py's crossing on
mixed members -- every member's maker with the team's dt and N, the starts' position entries
on the circle of radius 2 (member a takes the circle's first pd_a coordinates) at angle
2 pi a / count + 0.15 N(0, 1), the goals turned by 2.2 rad, no Laplacian coupling, q_pos
added to Q on the position entries, one obstacle at (0.3, 0.2, 0)[:D] of radius 0.5,
separation radius 0.4, both bumps of weight 1.5, w = the largest of the makers' times the
scale.  SOLVES lists per shape the scale and the T_min values tried in order (None: the
largest of the makers'); seeds 7000 .. per setting, max_iter = 6 under both methods, and
make_golden_fleet.py's keep rule: every select gap of both methods >= 1e-3 and
len(T_hist) >= 2, KEEP = 3 trials that share w, Q and the cost.  A set whose T* sit on T_min
is kept only if no later T_min yields an interior one.

Kernel-level cases (team_prox_cases_<tag>.npz), N = 12: make_golden_team.py's case_inputs()
(repeated verbatim) with the cost of prox_inputs() (repeated verbatim in
tests/test_gpu_team_proximity.py), which redraws every member's position entries of the
cost trajectories so that pairs and obstacles lie within two radii --
  tay    c, cx, cxx at 67 states (the first state of every cost trajectory)
  cost   B = 67: cost_timeopt_true with the cost
  ls     forward_linesearch_fixedT with the cost in the backward pass and in J, under
         make_golden_fleet.py's filter (every candidate |J' - J_old| >= 1e-6 |J_old|)
The generator asserts max c >= 0.1 x the largest weight over the 67 states.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _args():
    pos, opt = [], {}
    it = iter(sys.argv[1:])
    for a in it:
        if a in ("--only", "--out"):
            opt[a[2:]] = next(it)
        elif a in ("--cases-only", "--solves-only"):
            opt[a[2:]] = True
        else:
            pos.append(a)
    return pos, opt


def _reference_dir(pos):
    """REFERENCE_DIR from the command line, else the REF of make_golden.py beside this file."""
    if pos:
        return pos[0]
    with open(os.path.join(HERE, "make_golden.py")) as f:
        for line in f:
            if line.startswith("REF = "):
                return line.split("=", 1)[1].strip().strip('"\'')
    raise SystemExit("name the reference's directory on the command line")


POS, OPT = _args()
sys.path.insert(0, _reference_dir(POS))
os.environ.setdefault("MPLBACKEND", "Agg")

import linearization as ref_lin  # noqa: E402
import solver as ref_solver  # noqa: E402
import systems as ref_systems  # noqa: E402

# system id -> (maker, N of its fleets' solves, position entries)
MEMBERS = {0: (ref_systems.make_double_integrator, 60, (0,)),
           1: (ref_systems.make_cartpole_swingup, 120, (0,)),
           2: (ref_systems.make_quadrotor, 80, (0, 1, 2)),
           3: (ref_systems.make_pointmass_navigation, 80, (0, 1)),
           4: (ref_systems.make_segway_balance, 80, (0,))}
# tag -> (member ids, the shared dt)
TAGS = {"pm_quad_di": ((3, 2, 0), 0.05), "di2_pm2": ((0, 0, 3, 3), 0.05),
        "quad_pm3": ((2, 3, 3, 3), 0.05), "pm7_di": ((3,) * 7 + (0,), 0.05),
        "all5": ((0, 1, 2, 3, 4), 0.02)}
# per shape: (w scale, the T_min values tried in order; None = the largest of the makers')
SOLVES = {"di2_pm2": (1600.0, (10,)), "pm_quad_di": (1600.0, (15,)),
          "quad_pm3": (1600.0, (None, 15))}
Q_POS, BUMP_WEIGHT = 0.5, 1.5
SEED0, SEEDS = 7000, 8
MIN_GAP, KEEP, MAX_ITER = 1e-3, 3, 6
RADIUS, JITTER, TURN = 2.0, 0.15, 2.2
OBSTACLE, OBS_RADIUS, SEP_RADIUS = (0.3, 0.2, 0.0), 0.5, 0.4
METHODS = {"propagator": "propagator_all_Jt_aug",
           "bruteforce": "bruteforce_all_Jt_backward_expansion"}
N_CASE, B_COST, LS_POOL = 12, 67, 12


def solve_n(ids):
    """N of a team's solves: the largest of its members' fleets'"""
    return max(MEMBERS[s][1] for s in ids)


def stacked(ids, dt, N=None):
    """(F of the team, the members' maker tuples, the state and input offsets)"""
    mks = [MEMBERS[s][0](dt=dt) if N is None else MEMBERS[s][0](dt=dt, N=N) for s in ids]
    ns = [len(mk[1]) for mk in mks]
    ms = [len(np.atleast_1d(mk[3])) for mk in mks]
    xo = [int(v) for v in np.cumsum([0] + ns[:-1])]
    uo = [int(v) for v in np.cumsum([0] + ms[:-1])]

    def F(x, u):
        x = np.asarray(x, dtype=float).reshape(-1)
        u = np.asarray(u, dtype=float).reshape(-1)
        return np.concatenate([np.asarray(mk[0](x[i:i + k], u[j:j + l]), dtype=float).reshape(-1)
                               for mk, i, k, j, l in zip(mks, xo, ns, uo, ms)])

    return F, mks, xo, uo


def blocks(mats):
    mats = [np.atleast_2d(np.asarray(M, dtype=float)) for M in mats]
    out = np.zeros((sum(len(M) for M in mats),) * 2)
    o = 0
    for M in mats:
        out[o:o + len(M), o:o + len(M)] = M
        o += len(M)
    return out


def team_wrap(mks, xo):
    return [o + i for mk, o in zip(mks, xo) for i in (mk[11] or [])]


def pos_dims(ids):
    return [len(MEMBERS[s][2]) for s in ids]


def bump_cost(n, xo, pds, obstacles, sep):
    """the proximity cost (x, u) -> (c, cx, cxx) on the stacked state of a team"""
    D = max(pds)
    rows = np.asarray(obstacles, dtype=float).reshape(-1, D + 2)
    r_s, w_s = sep
    count = len(xo)

    def cost(x, u=None):
        x = np.asarray(x, dtype=float).reshape(-1)
        P = np.zeros((count, D))
        for a in range(count):
            P[a, :pds[a]] = x[xo[a]:xo[a] + pds[a]]
        c, cx, cxx = 0.0, np.zeros(n), np.zeros((n, n))
        for a in range(count):
            pa = pds[a]
            sa = slice(xo[a], xo[a] + pa)
            for row in rows:
                o, r, w = row[:D], row[D], row[D + 1]
                if w == 0.0:
                    continue
                d = P[a] - o
                ci = w * np.exp(-float(d @ d) / (2.0 * r * r))
                c += ci
                cx[sa] += (-(ci / (r * r)) * d)[:pa]
                cxx[sa, sa] += (ci * np.outer(d, d) / r ** 4)[:pa, :pa]
            for b in range(a + 1, count if w_s != 0.0 else 0):
                pb = pds[b]
                sb = slice(xo[b], xo[b] + pb)
                d = P[a] - P[b]
                ci = w_s * np.exp(-float(d @ d) / (2.0 * r_s * r_s))
                g, H = -(ci / (r_s * r_s)) * d, ci * np.outer(d, d) / r_s ** 4
                c += ci
                cx[sa] += g[:pa]
                cx[sb] -= g[:pb]
                cxx[sa, sa] += H[:pa, :pa]
                cxx[sb, sb] += H[:pb, :pb]
                cxx[sa, sb] -= H[:pa, :pb]
                cxx[sb, sa] -= H[:pb, :pa]
        return c, cx, cxx

    return cost


def problem(tag, seed, scale, t_min=None):
    """the crossing problem (time_opt_ilqr_amd.systems.make_team_crossing builds the same)"""
    ids, dt = TAGS[tag]
    N = solve_n(ids)
    F, mks, xo, uo = stacked(ids, dt, N)
    pds, count = pos_dims(ids), len(ids)
    D = max(pds)
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(count) / count + JITTER * rng.standard_normal(count)
    x0 = np.concatenate([np.asarray(mk[1], dtype=float) for mk in mks])
    xg = np.concatenate([np.asarray(mk[2], dtype=float) for mk in mks])
    for a in range(count):
        for ang_a, x in ((ang[a], x0), (ang[a] + TURN, xg)):
            circle = RADIUS * np.array([np.cos(ang_a), np.sin(ang_a), 0.0])
            x[xo[a]:xo[a] + pds[a]] = circle[:pds[a]]
    Q = blocks([mk[4] for mk in mks])
    idx = [o + i for s, o in zip(ids, xo) for i in MEMBERS[s][2]]
    Q[idx, idx] += Q_POS
    Qf = blocks([mk[6] * np.eye(len(mk[1])) if np.ndim(mk[6]) == 0 else mk[6] for mk in mks])
    obstacles = np.array([list(OBSTACLE[:D]) + [OBS_RADIUS, BUMP_WEIGHT]])
    sep = (SEP_RADIUS, BUMP_WEIGHT)
    return dict(F=F, extra=bump_cost(len(x0), xo, pds, obstacles, sep),
                members=np.asarray(ids, dtype=np.int64), dt=dt, seed=seed, N=N, x0=x0, xg=xg,
                u_ref=np.concatenate([np.atleast_1d(np.asarray(mk[3], dtype=float))
                                      for mk in mks]),
                Q=Q, R=blocks([mk[5] for mk in mks]), Qf=Qf,
                w=max(float(mk[7]) for mk in mks) * scale, scale=scale, q_pos=Q_POS,
                bump_weight=BUMP_WEIGHT, prox_obs=obstacles, prox_sep=np.asarray(sep),
                T_min=int(max(int(mk[9]) for mk in mks) if t_min is None else t_min),
                T_max=int(min(min(int(mk[10]) for mk in mks), N - 5)),
                wrap_idx=team_wrap(mks, xo))


def solve(p, method):
    gaps = []
    name = METHODS[method]
    real = getattr(ref_solver, name)

    def spy(*a, **k):
        J = real(*a, **k)
        win = np.sort(np.asarray(J)[p["T_min"] - 1:p["T_max"]])
        gaps.append(float((win[1] - win[0]) / abs(win[0])))
        return J

    setattr(ref_solver, name, spy)
    try:
        sol = ref_solver.ilqr_timeopt(p["F"], p["x0"], p["xg"], p["u_ref"], p["Q"], p["R"],
                                      p["Qf"], p["w"], p["N"], p["T_min"], p["T_max"],
                                      method=method, max_iter=MAX_ITER, wrap_idx=p["wrap_idx"],
                                      extra_stage_cost=p["extra"])
    finally:
        setattr(ref_solver, name, real)
    X = np.asarray(sol["X"])
    T = int(sol["T_hist"][-1])
    extra = sum(p["extra"](X[k])[0] for k in range(T))
    return dict(T_hist=np.asarray(sol["T_hist"], dtype=np.int64),
                J_hist=np.asarray(sol["J_hist"], dtype=np.float64), gaps=np.asarray(gaps),
                extra_share=float(extra / sol["J_hist"][-1]))


def passes(r):
    return len(r["gaps"]) > 0 and r["gaps"].min() >= MIN_GAP and len(r["T_hist"]) >= 2


def search(tag, scale, t_min):
    """(the first KEEP kept trials, the best minimum gap seen)"""
    best, kept = 0.0, []
    for seed in range(SEED0, SEED0 + SEEDS):
        p = problem(tag, seed, scale, t_min)
        res = {}
        for method in METHODS:
            try:
                res[method] = solve(p, method)
            except Exception as e:  # the reference raised: not a usable trial
                print(f"{tag} scale={scale:g} seed={seed} {method}: {type(e).__name__}",
                      flush=True)
                res = None
                break
            g = res[method]["gaps"]
            if len(g):
                best = max(best, float(g.min()))
            if not passes(res[method]):
                break
        ok = res is not None and len(res) == len(METHODS) and all(passes(r) for r in res.values())
        if res:
            print(f"{tag} T_min={p['T_min']} scale={scale:g} seed={seed} " + " ".join(
                f"{m}: min gap {r['gaps'].min() if len(r['gaps']) else float('nan'):.2e} "
                f"T_hist {r['T_hist'].tolist()} extras {r['extra_share']:.1%} of J"
                for m, r in res.items()) + (" kept" if ok else " dropped"), flush=True)
        if ok:
            kept.append((p, res))
            if len(kept) == KEEP:
                break
    return kept, best


def write_solves(tag, out):
    scale, ladder = SOLVES[tag]
    kept, best, boundary = [], 0.0, None
    for t_min in ladder:
        kept, b = search(tag, scale, t_min)
        best = max(best, b)
        if len(kept) < KEEP:
            kept = []
            continue
        interior = all(int(r["T_hist"].min()) > p["T_min"] for p, res in kept for r in res.values())
        if interior:
            break
        boundary = boundary or kept
        print(f"{tag}: T* on T_min = {kept[0][0]['T_min']}")
        kept = []
    kept = kept or boundary or []
    print(f"{tag}: {len(kept)} trials kept, best minimum gap seen {best:.2e}", flush=True)
    for i, (p, res) in enumerate(kept):
        d = {k: v for k, v in p.items() if k not in ("F", "extra")}
        d.update(max_iter=MAX_ITER, n=len(p["x0"]), m=len(p["u_ref"]),
                 wrap_idx=np.asarray(p["wrap_idx"], dtype=np.int64))
        for m, r in res.items():
            for k in ("T_hist", "J_hist", "gaps", "extra_share"):
                d[f"{k}_{m}"] = r[k]
        np.savez_compressed(os.path.join(out, f"team_prox_solve_{tag}_{i}.npz"), **d)


# ---- kernel-level cases -----------------------------------------------------------
# BEGIN case_inputs (repeated verbatim in tests/test_gpu_team.py)
def case_inputs(seed, n, m, n_member, N=12, B=67, pool=12):
    """every input of the kernel-level cases that a seed determines"""
    rng = np.random.default_rng(seed)

    def spd(k, lo):
        G = rng.standard_normal((k, k))
        return G @ G.T / k + lo * np.eye(k)

    c = dict(Q=spd(n, 0.1), Qf=3.0 * spd(n, 0.3), R=spd(m, 0.1), w=0.37,
             xg=rng.uniform(-0.3, 0.3, n), u_ref=rng.uniform(-0.2, 0.2, m))
    c["X"] = rng.uniform(-4.0, 4.0, (B, N + 1, n))  # past +-pi: the wrap matters
    c["U"] = rng.uniform(-1.0, 1.0, (B, N, m))
    c["T"] = rng.integers(1, N + 1, B).astype(np.int32)
    # linearisation with a NaN planted in one member (the second where there is one)
    c["Xn"] = rng.uniform(-1.0, 1.0, (N + 1, n))
    c["Un"] = rng.uniform(-1.0, 1.0, (N, m))
    c["nan_at"] = (5, (n_member if n > n_member else 0) + 1)
    c["Xn"][c["nan_at"]] = np.nan
    # line search pool: starts near the goal, mild controls
    c["x0"] = c["xg"] + rng.uniform(-0.4, 0.4, (pool, n))
    c["U0"] = c["u_ref"] + 0.3 * rng.uniform(-1.0, 1.0, (pool, N, m))
    c["T0"] = np.array([N, 5, 9, 3] * (pool // 4), dtype=np.int32)
    return c
# END case_inputs


# BEGIN prox_inputs (repeated verbatim in tests/test_gpu_team_proximity.py)
def prox_inputs(seed, c, xo, pds):
    """the cost of the kernel-level cases: four obstacle rows in D = max(pds) columns (one of
    weight 0, which must contribute nothing) and a separation pair; every member's position
    entries of the cost trajectories c["X"] are redrawn in place so that pairs and obstacles
    lie within two radii"""
    D = max(pds)
    rng = np.random.default_rng(seed + 50000)
    obs = np.concatenate([rng.uniform(-0.6, 0.6, (4, D)), rng.uniform(0.3, 0.6, (4, 1)),
                          rng.uniform(0.5, 2.0, (4, 1))], axis=1)
    obs[2, D + 1] = 0.0
    sep = (0.45, 1.3)
    for o, pd in zip(xo, pds):
        sl = slice(o, o + pd)
        c["X"][..., sl] = rng.uniform(-0.8, 0.8, c["X"][..., sl].shape)
    return obs, sep
# END prox_inputs


def candidate(F, X, U, T, K, k, c, wrap, alpha, extra):
    """J' of one step size as forward_linesearch_fixedT forms it (NaN: rejected rollout)"""
    N = len(U)
    Xn, Un = np.zeros_like(X), U.copy()
    Xn[0] = X[0]
    with np.errstate(all="ignore"):
        for i in range(N):
            if i < T:
                dx = ref_solver.wrap_error((Xn[i] - X[i]).reshape(-1), wrap)
                Un[i] = (U[i] + (K[i] @ dx + float(alpha) * k[i]).reshape(-1)).reshape(-1)
            Xn[i + 1] = F(Xn[i], Un[i])
            if not np.all(np.isfinite(Xn[i + 1])):
                return np.nan
        return ref_solver.cost_timeopt_true(Xn, Un, c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"],
                                            c["w"], T, wrap, extra)


ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05)
LS_ROLES = (1.0, 8.0, 1.0, 3.0)  # factor on k: plain, overshooting, (inactive), pushed


def write_cases(tag, out):
    ids, dt = TAGS[tag]
    F, mks, xo, uo = stacked(ids, dt)
    pds = pos_dims(ids)
    D = max(pds)
    n = xo[-1] + len(mks[-1][1])
    m = uo[-1] + len(np.atleast_1d(mks[-1][3]))
    wrap = team_wrap(mks, xo)
    seed = 9800 + list(TAGS).index(tag)
    c = case_inputs(seed, n, m, xo[1], N_CASE, B_COST, LS_POOL)
    obs, sep = prox_inputs(seed, c, xo, pds)
    extra = bump_cost(n, xo, pds, obs, sep)
    d = dict(seed=seed, members=np.asarray(ids, dtype=np.int64), dt=dt, n=n, m=m,
             wrap_idx=np.asarray(wrap, dtype=np.int64), prox_obs=obs, prox_sep=np.asarray(sep),
             check=np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum(), obs.sum()]))
    tay = [extra(c["X"][b, 0]) for b in range(B_COST)]
    d["tay_c"] = np.array([t[0] for t in tay])
    d["tay_cx"] = np.stack([t[1] for t in tay])
    d["tay_cxx"] = np.stack([t[2] for t in tay])
    w_bump = max(float(obs[:, D + 1].max()), sep[1])
    assert d["tay_c"].max() >= 0.1 * w_bump, (tag, d["tay_c"].max())
    d["cost_J"] = np.array([ref_solver.cost_timeopt_true(
        c["X"][b], c["U"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], c["w"], int(c["T"][b]),
        wrap, extra) for b in range(B_COST)])
    plain = np.array([ref_solver.cost_timeopt_true(
        c["X"][b], c["U"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], c["w"], int(c["T"][b]),
        wrap) for b in range(B_COST)])
    # line search: one problem per role from the pool
    picks, outs = [], []
    for role, fac in enumerate(LS_ROLES):
        for b in range(role, LS_POOL, len(LS_ROLES)):
            T = int(c["T0"][b])
            X = ref_solver.rollout(F, c["x0"][b], c["U0"][b])
            A, Bm = ref_lin.linearize_central_diff_traj(F, X, c["U0"][b])
            kl, Kl, ok = ref_solver.backward_pass_truncated(
                A, Bm, X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], T,
                lm_lambda=1e-3, wrap_idx=wrap, extra_stage_cost=extra)
            if not ok:
                continue
            K, k = np.zeros((N_CASE, m, n)), np.zeros((N_CASE, m))
            for i in range(T):
                K[i], k[i] = np.asarray(Kl[i]).reshape(m, n), fac * np.asarray(kl[i]).reshape(-1)
            J0 = ref_solver.cost_timeopt_true(X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"],
                                              c["Qf"], c["w"], T, wrap, extra)
            Jc = np.array([candidate(F, X, c["U0"][b], T, K, k, c, wrap, al, extra)
                           for al in ALPHAS])
            if not np.all(~np.isfinite(Jc) | (np.abs(Jc - J0) >= 1e-6 * abs(J0))):
                continue
            Xo, Uo, J, acc = ref_solver.forward_linesearch_fixedT(
                F, X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], c["w"], T,
                [k[i] for i in range(T)], [K[i] for i in range(T)], alphas=ALPHAS, wrap_idx=wrap,
                extra_stage_cost=extra)
            win = int(np.flatnonzero(Jc < J0)[0]) if acc else -1
            assert (not acc) or J == Jc[win]
            picks.append(b)
            extra0 = sum(extra(X[i])[0] for i in range(T))
            outs.append((X, K, k, Xo, Uo, J, J0, win, extra0))
            break
        else:
            raise RuntimeError(f"{tag}: no line-search candidate for role {role} passes the filter")
    d["ls_pick"] = np.asarray(picks, dtype=np.int64)
    for i, key in enumerate(("ls_X", "ls_K", "ls_k", "ls_Xo", "ls_Uo", "ls_J", "ls_J0", "ls_acc",
                             "ls_extra0")):
        d[key] = np.stack([np.asarray(o[i]) for o in outs])
    print(f"{tag}: cases written; max c {d['tay_c'].max():.3f} (w_bump {w_bump:.2f}); the cost is "
          f"{np.median((d['cost_J'] - plain) / d['cost_J']):.1%} of cost_J (median), "
          f"{np.median(d['ls_extra0'] / d['ls_J0']):.1%} of the line search's J_old; accepted "
          f"{d['ls_acc'].tolist()} (role 2 runs inactive in the test)", flush=True)
    np.savez_compressed(os.path.join(out, f"team_prox_cases_{tag}.npz"), **d)


def main():
    out = OPT.get("out", HERE)
    only = OPT["only"].split(",") if "only" in OPT else None
    for tag in TAGS:
        if only and tag not in only:
            continue
        if "solves-only" not in OPT:
            write_cases(tag, out)
        if "cases-only" not in OPT and tag in SOLVES:
            write_solves(tag, out)


if __name__ == "__main__":
    main()
