"""Generate the team goldens (team_solve_*.npz, team_cases_*.npz) by running the REFERENCE.

Run where a checkout of the reference (dmmsjtu-umich/time-opt-ilqr) is at hand, from
outside both trees, naming the reference's directory (tests/golden/make_golden.py's
source of the reference is the default):

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_team.py [REFERENCE_DIR]
        [--only TAG[,TAG...]] [--cases-only | --solves-only] [--out DIR]

It imports the reference's solver, linearisation and makers from that directory (read
only, no bytecode written).  A team stacks members of different reference systems: the
stacked callable F(x, u) = the concatenation of each member's maker F on its slice, every
maker called with the team's dt.  Every file holds data only.

Whole solves (team_solve_<tag>_<i>.npz), the procedure and filter of make_golden_fleet.py.
Problem data (problem() below, repeated by time_opt_ilqr_amd.systems.make_team): every
member's maker with the team's dt and N (SOLVE_N); x0 = the makers' starts plus seeded
noise on the position entries, drawn in member order, then entry order; Q = the block
diagonal of the members' Q plus a path Laplacian over consecutive members' first
coordinates, kappa = 0.5 min(Q_a[0, 0], Q_a+1[0, 0]) (before any coupling is added), or
0.5 max(Q_a[0, 0], Q_a+1[0, 0], 1) where that minimum is 0; R and the terminal weight
block diagonal; w = the largest of the makers' times a scale searched over {100, 400,
1600}, seeds 7000 .. 7039 per scale; T_max = min(the makers', N - 5); T_min the largest of
the makers'.  ilqr_timeopt runs with max_iter = 6 under both methods.  A trial is KEPT only
if every window gap of both methods is >= 1e-3 and both have len(T_hist) >= 2.  The first
scale that yields KEEP = 3 trials is used (the kept trials of a shape share w, so they can
run as one batch).  T_min is lowered (TMIN_LADDER) while the kept trials' T* sit on it; the
boundary set is kept only if no interior one passes.  Shapes for which no trial passes get
no solve fixture; the best gap seen is printed.  The filter is a condition on the
reference alone.

Kernel-level cases (team_cases_<tag>.npz), N = 12, for every shape of TAGS: the fleet
generator's cases with case_inputs() (repeated verbatim in tests/test_gpu_team.py), its
n_member argument being the second member's offset --
  cost   B = 67: cost_timeopt_true with dense coupled Q, Qf, R and the team's wrap_idx
  nan    the NaN pattern of linearize_{forward,central}_diff_traj on the stacked callable
         with a NaN planted in the second member's state at one step
  ls     forward_linesearch_fixedT on the stacked callable with the gains of the
         reference's backward_pass_truncated; only cases where every candidate has
         |J' - J_old| >= 1e-6 |J_old| are kept, so no accept decision rests on rounding
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

# system id -> (maker, N of its fleets' solves, noise on the position entries, position
# entries)
MEMBERS = {0: (ref_systems.make_double_integrator, 60, 0.2, (0,)),
           1: (ref_systems.make_cartpole_swingup, 120, 0.05, (0,)),
           2: (ref_systems.make_quadrotor, 80, 0.4, (0, 1, 2)),
           3: (ref_systems.make_pointmass_navigation, 80, 0.2, (0, 1)),
           4: (ref_systems.make_segway_balance, 80, 0.02, (0,))}
# tag -> (member ids, the shared dt)
TAGS = {"all5": ((0, 1, 2, 3, 4), 0.02), "pm_quad_di": ((3, 2, 0), 0.05),
        "di2_pm2": ((0, 0, 3, 3), 0.05), "quad_pm3": ((2, 3, 3, 3), 0.05),
        "quad_di4_pm2": ((2, 0, 0, 0, 0, 3, 3), 0.05), "pm7_di": ((3,) * 7 + (0,), 0.05),
        "cp2_seg3": ((1, 1, 4, 4, 4), 0.02)}
SOLVE_TAGS = ("di2_pm2", "quad_pm3", "quad_di4_pm2", "cp2_seg3")
SCALES = (100.0, 400.0, 1600.0)
SEED0, SEEDS = 7000, 40
MIN_GAP, KEEP, MAX_ITER, COUPLING = 1e-3, 3, 6, 0.5
# the makers' largest T_min, then lower
TMIN_LADDER = {"di2_pm2": (None, 10), "quad_pm3": (None, 15), "quad_di4_pm2": (None, 15),
               "cp2_seg3": (None, 12)}
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


def problem(tag, seed, scale, t_min=None):
    """the joint problem (time_opt_ilqr_amd.systems.make_team builds the same data)"""
    ids, dt = TAGS[tag]
    N = solve_n(ids)
    F, mks, xo, uo = stacked(ids, dt, N)
    rng = np.random.default_rng(seed)
    x0 = np.concatenate([np.asarray(mk[1], dtype=float) for mk in mks])
    for s, o in zip(ids, xo):
        idx = [o + i for i in MEMBERS[s][3]]
        x0[idx] += MEMBERS[s][2] * rng.standard_normal(len(idx))
    Q = blocks([mk[4] for mk in mks])
    q00 = [float(np.asarray(mk[4], dtype=float)[0, 0]) for mk in mks]
    for a in range(len(mks) - 1):
        lo = min(q00[a], q00[a + 1])
        kappa = COUPLING * (lo if lo != 0.0 else max(q00[a], q00[a + 1], 1.0))
        i, j = xo[a], xo[a + 1]
        Q[i, i] += kappa
        Q[j, j] += kappa
        Q[i, j] -= kappa
        Q[j, i] -= kappa
    Qf = blocks([mk[6] * np.eye(len(mk[1])) if np.ndim(mk[6]) == 0 else mk[6] for mk in mks])
    return dict(F=F, members=np.asarray(ids, dtype=np.int64), dt=dt, seed=seed, N=N, x0=x0,
                xg=np.concatenate([np.asarray(mk[2], dtype=float) for mk in mks]),
                u_ref=np.concatenate([np.atleast_1d(np.asarray(mk[3], dtype=float))
                                      for mk in mks]),
                Q=Q, R=blocks([mk[5] for mk in mks]), Qf=Qf,
                w=max(float(mk[7]) for mk in mks) * scale, scale=scale,
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
                                      method=method, max_iter=MAX_ITER, wrap_idx=p["wrap_idx"])
    finally:
        setattr(ref_solver, name, real)
    return dict(T_hist=np.asarray(sol["T_hist"], dtype=np.int64),
                J_hist=np.asarray(sol["J_hist"], dtype=np.float64), gaps=np.asarray(gaps),
                X=np.asarray(sol["X"]), U=np.asarray(sol["U"]))


def passes(r):
    return len(r["gaps"]) > 0 and r["gaps"].min() >= MIN_GAP and len(r["T_hist"]) >= 2


def search(tag, t_min):
    """(kept trials of the first scale that yields KEEP, the best minimum gap seen)"""
    best, most = 0.0, []
    for scale in SCALES:
        kept = []
        for seed in range(SEED0, SEED0 + SEEDS):
            p = problem(tag, seed, scale, t_min)
            res = {}
            for method in METHODS:
                try:
                    res[method] = solve(p, method)
                except Exception as e:  # the reference raised: not a usable trial
                    print(f"{tag} scale={scale:g} seed={seed} {method}: {type(e).__name__}")
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
                    f"T_hist {r['T_hist'].tolist()}" for m, r in res.items())
                    + (" kept" if ok else " dropped"), flush=True)
            if ok:
                kept.append((p, res))
                if len(kept) == KEEP:
                    return kept, best
        if len(kept) > len(most):
            most = kept
    return most, best


def write_solves(tag, out):
    kept, best, boundary = [], 0.0, None
    for t_min in TMIN_LADDER.get(tag, (None,)):
        kept, b = search(tag, t_min)
        best = max(best, b)
        if not kept:
            continue
        interior = all(int(r["T_hist"].min()) > p["T_min"] for p, res in kept for r in res.values())
        if interior:
            break
        boundary = boundary or kept
        print(f"{tag}: T* on T_min = {kept[0][0]['T_min']}: lowering T_min")
        kept = []
    kept = kept or boundary or []
    print(f"{tag}: {len(kept)} trials kept, best minimum gap seen {best:.2e}", flush=True)
    for i, (p, res) in enumerate(kept):
        d = {k: v for k, v in p.items() if k != "F"}
        d.update(max_iter=MAX_ITER, n=len(p["x0"]), m=len(p["u_ref"]),
                 wrap_idx=np.asarray(p["wrap_idx"], dtype=np.int64))
        for m, r in res.items():
            for k in ("T_hist", "J_hist", "gaps"):
                d[f"{k}_{m}"] = r[k]
        np.savez_compressed(os.path.join(out, f"team_solve_{tag}_{i}.npz"), **d)


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


def candidate(F, X, U, T, K, k, c, wrap, alpha):
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
                                            c["w"], T, wrap)


ALPHAS = (1.0, 0.5, 0.25, 0.1, 0.05)
LS_ROLES = (1.0, 8.0, 1.0, 3.0)  # factor on k: plain, overshooting, (inactive), pushed


def write_cases(tag, out):
    ids, dt = TAGS[tag]
    F, mks, xo, uo = stacked(ids, dt)
    n = xo[-1] + len(mks[-1][1])
    m = uo[-1] + len(np.atleast_1d(mks[-1][3]))
    wrap = team_wrap(mks, xo)
    seed = 9700 + list(TAGS).index(tag)
    c = case_inputs(seed, n, m, xo[1], N_CASE, B_COST, LS_POOL)
    d = dict(seed=seed, members=np.asarray(ids, dtype=np.int64), dt=dt, n=n, m=m,
             wrap_idx=np.asarray(wrap, dtype=np.int64),
             check=np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum()]))
    d["cost_J"] = np.array([ref_solver.cost_timeopt_true(
        c["X"][b], c["U"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], c["w"], int(c["T"][b]),
        wrap) for b in range(B_COST)])
    with np.errstate(all="ignore"):
        for form, fn in (("fwd", ref_lin.linearize_forward_diff_traj),
                         ("cen", ref_lin.linearize_central_diff_traj)):
            A, Bm = fn(F, c["Xn"], c["Un"])
            d[f"nan_A_{form}"] = np.isnan(np.asarray(A))
            d[f"nan_B_{form}"] = np.isnan(np.asarray(Bm))
    # line search: one problem per role from the pool
    picks, outs = [], []
    for role, fac in enumerate(LS_ROLES):
        for b in range(role, LS_POOL, len(LS_ROLES)):
            T = int(c["T0"][b])
            X = ref_solver.rollout(F, c["x0"][b], c["U0"][b])
            A, Bm = ref_lin.linearize_central_diff_traj(F, X, c["U0"][b])
            kl, Kl, ok = ref_solver.backward_pass_truncated(
                A, Bm, X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], T,
                lm_lambda=1e-3, wrap_idx=wrap)
            if not ok:
                continue
            K, k = np.zeros((N_CASE, m, n)), np.zeros((N_CASE, m))
            for i in range(T):
                K[i], k[i] = np.asarray(Kl[i]).reshape(m, n), fac * np.asarray(kl[i]).reshape(-1)
            J0 = ref_solver.cost_timeopt_true(X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"],
                                              c["Qf"], c["w"], T, wrap)
            Jc = np.array([candidate(F, X, c["U0"][b], T, K, k, c, wrap, al) for al in ALPHAS])
            if not np.all(~np.isfinite(Jc) | (np.abs(Jc - J0) >= 1e-6 * abs(J0))):
                continue
            Xo, Uo, J, acc = ref_solver.forward_linesearch_fixedT(
                F, X, c["U0"][b], c["xg"], c["u_ref"], c["Q"], c["R"], c["Qf"], c["w"], T,
                [k[i] for i in range(T)], [K[i] for i in range(T)], alphas=ALPHAS, wrap_idx=wrap)
            win = int(np.flatnonzero(Jc < J0)[0]) if acc else -1
            assert (not acc) or J == Jc[win]
            picks.append(b)
            outs.append((X, K, k, Xo, Uo, J, J0, win))
            break
        else:
            raise RuntimeError(f"{tag}: no line-search candidate for role {role} passes the filter")
    d["ls_pick"] = np.asarray(picks, dtype=np.int64)
    for i, key in enumerate(("ls_X", "ls_K", "ls_k", "ls_Xo", "ls_Uo", "ls_J", "ls_J0", "ls_acc")):
        d[key] = np.stack([np.asarray(o[i]) for o in outs])
    print(f"{tag}: cases written; line search accepted {d['ls_acc'].tolist()} "
          f"(role 2 runs inactive in the test)", flush=True)
    np.savez_compressed(os.path.join(out, f"team_cases_{tag}.npz"), **d)


def main():
    out = OPT.get("out", HERE)
    only = OPT["only"].split(",") if "only" in OPT else None
    for tag in TAGS:
        if only and tag not in only:
            continue
        if "solves-only" not in OPT:
            write_cases(tag, out)
        if "cases-only" not in OPT and tag in SOLVE_TAGS:
            write_solves(tag, out)


if __name__ == "__main__":
    main()
