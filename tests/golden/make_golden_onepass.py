"""Generate the one-pass (baseline2) goldens by running the REFERENCE.

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_onepass.py [REFERENCE_DIR]

Run it from outside both trees.  It imports the reference's solver, linearization,
horizon_selection and systems at generation time and stores data only:

  onepass_pick_cases.npz     synthetic calls of onepass_pick_T_singlepass (n = 2, n = 12)
  onepass_prefix_cases.npz   extend_nominal_backward on all five systems, N = 12, S in {1, 4}
  onepass_curve_cases.npz    nominal_cost_curve on the trajectories of ilqr_<tag>.npz
  onepass_rollout_cases.npz  onepass_rollout with K, k of the reference's sweep
  onepass_solve_<name>.npz   whole solves ilqr_timeopt(method="onepass") with the margin of
                             every decision the reference took

A solve is kept only if every decision has a margin well above the tests' bars: window gap
between the best and second-best finite Jw >= 1e-4 relative, accept / reject margin
|Jcand - J_prev| / |J_prev| >= 1e-6, gap between the two best step sizes >= 1e-6, gate
margin |dn - dx_max| / dx_max >= 1e-6.  The two fallback solves (NaN in U_init) take no
such decision and are stored as they are.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HOP_REFERENCE_DIR", "")
if not REF or not os.path.isdir(REF):
    raise SystemExit("usage: make_golden_onepass.py REFERENCE_DIR")
sys.path.insert(0, REF)

import horizon_selection as hs  # noqa: E402
import linearization as lz  # noqa: E402
import solver as rs  # noqa: E402
import systems as rsys  # noqa: E402
from utils import wrap_error  # noqa: E402

warnings.filterwarnings("ignore")
TAGS = ["di", "cartpole", "quadrotor", "pointmass", "segway"]
MAKERS = dict(di=rsys.make_double_integrator, cartpole=rsys.make_cartpole_swingup,
              quadrotor=rsys.make_quadrotor, pointmass=rsys.make_pointmass_navigation,
              segway=rsys.make_segway_balance)
MIN_WINDOW_GAP, MIN_ACCEPT, MIN_ALPHA_GAP, MIN_GATE = 1e-4, 1e-6, 1e-6, 1e-6
ALPHAS = (1.0, 0.5, 0.25, 0.1)


def fixture(tag):
    return np.load(os.path.join(HERE, f"ilqr_{tag}.npz"))


def problem(tag):
    d = fixture(tag)
    mk = MAKERS[tag](N=int(d["N"]))
    F, x0, xg, u_ref, Q, R, alpha, w, N, _, _, wrap_idx, extra = mk
    esc = extra["extra_stage_cost"] if extra else None
    return dict(F=F, x0=np.asarray(x0, float), xg=xg, u_ref=u_ref, Q=Q, R=R, alpha=alpha, w=w,
                N=int(d["N"]), T_min=int(d["T_min"]), T_max=int(d["T_max"]), wrap_idx=wrap_idx,
                esc=esc, central=bool(d["central"]))


def two_best_gap(vals):
    v = np.sort(np.asarray(vals, float)[np.isfinite(vals)])
    if v.size < 2:
        return np.inf
    return float((v[1] - v[0]) / max(abs(v[0]), 1e-300))


# ---------------------------------------------------------------- pick cases
def pick_cases():
    out, names = {}, []

    def add(name, n, L, T_bar, T_min, T_max, S_left, S_right, wrap_idx, seed, *, edit=None):
        rng = np.random.default_rng(seed)
        X_ext = np.cumsum(rng.normal(0.0, 0.3, (L, n)), axis=0)
        M = rng.normal(0.0, 1.0, (L, n, n))
        Vxx = M @ M.transpose(0, 2, 1) + np.eye(n)
        Vx = rng.normal(0.0, 1.0, (L, n))
        V0 = 5.0 + np.abs(rng.normal(0.0, 2.0, L))
        off = min(S_right, L - 1)
        c = dict(Vxx=Vxx, Vx=Vx, V0=V0, X_ext=X_ext, x0=X_ext[off].copy())
        if edit:
            edit(c)
        T, Jw = hs.onepass_pick_T_singlepass(list(c["Vxx"]), list(c["Vx"]), list(c["V0"]),
                                             c["X_ext"], c["x0"], T_bar, T_min, T_max, S_left,
                                             S_right, wrap_idx)
        i = len(names)
        names.append(name)
        for k, v in c.items():
            out[f"c{i}_{k}"] = v
        out[f"c{i}_par"] = np.array([n, L, T_bar, T_min, T_max, S_left, S_right])
        out[f"c{i}_wrap"] = np.array(wrap_idx or [], dtype=np.int64)
        out[f"c{i}_T"] = np.int64(T)
        out[f"c{i}_Jw"] = Jw
        print(f"pick {name}: T*={T} evaluated={int(np.isfinite(Jw).sum())}")

    def far(c):  # two prefix states far away: the gate removes them
        c["X_ext"][0] += 400.0
        c["X_ext"][1] -= 300.0

    def nan_v0(c):  # no finite J anywhere: the clip fallback (the median gate alone can
        c["V0"][:] = np.nan  # never remove every candidate)

    def fixed_point(c):
        c["X_ext"][:] = c["x0"]

    def const_v0(c):
        c["Vxx"][:] = 0.0
        c["Vx"][:] = 0.0
        c["V0"][:] = 3.25
        c["X_ext"][:] = c["x0"]

    def sym_v0(T_bar, S):
        def f(c):
            c["Vxx"][:] = 0.0
            c["Vx"][:] = 0.0
            c["X_ext"][:] = c["x0"]
            i = np.arange(len(c["V0"]))
            c["V0"][:] = 1.0 + np.abs(np.abs(i - S) - 2.0)  # minima at T_bar -+ 2, equal
        return f

    for n, wrap in ((2, None), (12, [6, 7, 8])):
        s = 100 * n
        add(f"n{n}_plain", n, 24, 20, 5, 30, 6, 6, wrap, s + 1)
        add(f"n{n}_cut_left", n, 24, 7, 5, 30, 6, 6, wrap, s + 2)
        add(f"n{n}_cut_right", n, 24, 28, 5, 30, 6, 6, wrap, s + 3)
        add(f"n{n}_L_gt_R", n, 24, 40, 5, 30, 3, 3, wrap, s + 4)
        add(f"n{n}_asym", n, 24, 18, 5, 30, 2, 7, wrap, s + 5)
        add(f"n{n}_even_count", n, 24, 18, 5, 30, 3, 4, wrap, s + 6)
        add(f"n{n}_odd_count", n, 24, 18, 5, 30, 4, 4, wrap, s + 7)
        add(f"n{n}_gate", n, 24, 20, 5, 30, 6, 6, wrap, s + 8, edit=far)
        add(f"n{n}_nan_v0", n, 24, 20, 5, 30, 6, 6, wrap, s + 9, edit=nan_v0)
        add(f"n{n}_fixed_point", n, 24, 20, 5, 30, 6, 6, wrap, s + 10, edit=fixed_point)
        add(f"n{n}_tie_const", n, 24, 20, 5, 30, 6, 6, wrap, s + 11, edit=const_v0)
        add(f"n{n}_tie_sym", n, 24, 20, 5, 30, 6, 6, wrap, s + 12, edit=sym_v0(20, 6))
        # the shrink loop's call form: S_right below the arrays' offset (x0 = X_ext[6])
        add(f"n{n}_shrink", n, 24, 20, 5, 30, 3, 3, wrap, s + 13,
            edit=lambda c: c.__setitem__("x0", c["X_ext"][6].copy()))
        add(f"n{n}_wide_window", n, 130, 70, 1, 135, 64, 64, wrap, s + 14)
        # arrays shorter than the window reaches: candidates with i >= len(X_ext) are skipped
        add(f"n{n}_short_arrays", n, 10, 20, 5, 30, 6, 6, wrap, s + 16)
        if wrap:  # angles beyond +-pi, so the wrap changes dx0
            add(f"n{n}_wrapped", n, 24, 20, 5, 30, 6, 6, wrap, s + 15,
                edit=lambda c: c["X_ext"].__iadd__(np.linspace(0, 9, 24)[:, None]))
    out["names"] = np.array(names)
    np.savez(os.path.join(HERE, "onepass_pick_cases.npz"), **out)


# ---------------------------------------------------------------- prefix cases
def prefix_cases():
    out = {}
    N = 12
    for tag in TAGS:
        p = problem(tag)
        F, n, m = p["F"], len(p["x0"]), len(np.atleast_1d(p["u_ref"]))
        rng = np.random.default_rng(len(tag) + n)
        ur = np.atleast_1d(np.asarray(p["u_ref"], float))
        starts = {
            "generic": (p["x0"] + rng.normal(0.0, 0.1, n), ur + rng.normal(0.0, 0.2, m)),
            # a fixed point of F(., u_ref): the first iteration's residual is (about) zero
            "fixed": (np.asarray(p["xg"], float) if tag != "cartpole" else np.zeros(n), ur),
            "overflow": (np.full(n, 1.79e308), ur),
        }
        for name, (xs, uf) in starts.items():
            U = np.tile(uf, (N, 1)) + (0.0 if name != "generic" else rng.normal(0.0, 0.1, (N, m)))
            X = rs.rollout(F, xs, U, max_state_norm=np.inf)
            X[0] = xs
            for S in (1, 4):
                Xe, Ue = lz.extend_nominal_backward(F, X, U, U[0], S_back=S, max_iter=4,
                                                    damping=0.5)
                key = f"{tag}_{name}_S{S}"
                out[key + "_X"], out[key + "_U"] = X, U
                out[key + "_Xe"], out[key + "_Ue"] = Xe, Ue
                print(f"prefix {key}: |X_ext[0] - x0| = {np.abs(Xe[0] - xs).max():.3e}")
    np.savez(os.path.join(HERE, "onepass_prefix_cases.npz"), **out)


# ---------------------------------------------------------------- nominal curve
def curve_cases():
    out = {}
    for tag in TAGS:
        p, d = problem(tag), fixture(tag)
        for name in ("normal", "nan_tail"):
            X, U = d["X"].copy(), d["U"].copy()
            if name == "nan_tail":
                X[p["T_max"] - 2:] = np.nan
            J = rs.nominal_cost_curve(X, U, p["xg"], p["u_ref"], p["Q"], p["R"], p["alpha"],
                                      p["w"], p["T_min"], p["T_max"], p["wrap_idx"], p["esc"])
            T_bar = int(np.argmin(J[p["T_min"] - 1:p["T_max"]]) + p["T_min"])
            out[f"{tag}_{name}_J"], out[f"{tag}_{name}_Tbar"] = J, np.int64(T_bar)
            print(f"curve {tag} {name}: T_bar={T_bar}")
    np.savez(os.path.join(HERE, "onepass_curve_cases.npz"), **out)


# ---------------------------------------------------------------- recording a solve
class Recorder:
    """wraps the reference's pick, sweep and rollout inside its solver module"""

    def __init__(self):
        self.picks, self.rolls, self.sweeps = [], [], []
        self._orig = (rs.onepass_pick_T_singlepass, rs.onepass_rollout,
                      rs.value_expansions_and_gains_prefix)

    def __enter__(self):
        pick0, roll0, sweep0 = self._orig

        def pick(Vxx, Vx, V0, X_ext, x0, T_bar, T_min, T_max, S_left, S_right, wrap_idx, **kw):
            T, Jw = pick0(Vxx, Vx, V0, X_ext, x0, T_bar, T_min, T_max, S_left, S_right, wrap_idx,
                          **kw)
            L, R = max(T_min, T_bar - S_left), min(T_max, T_bar + S_right)
            dns = []
            for Tc in range(L, R + 1):
                i = T_bar - Tc + S_right
                if 0 <= i < len(X_ext):
                    dns.append(float(np.linalg.norm(wrap_error((x0 - X_ext[i]).reshape(-1),
                                                               wrap_idx))))
            norms = [v for v in dns if np.isfinite(v) and v > 1e-12]
            gate = np.inf
            if norms:
                dx_max = 5.0 * float(np.median(norms))
                gate = min(abs(v - dx_max) / dx_max for v in dns)
            self.picks.append(dict(T=T, window_gap=two_best_gap(Jw), gate=gate,
                                   S=(S_left, S_right)))
            return T, Jw

        def roll(F, X_ext, U_ext, xg, u_ref, Q, R, alpha, w, K, k, **kw):
            res = roll0(F, X_ext, U_ext, xg, u_ref, Q, R, alpha, w, K, k, **kw)
            kw1 = {a: b for a, b in kw.items() if a != "alphas"}
            Js = [roll0(F, X_ext, U_ext, xg, u_ref, Q, R, alpha, w, K, k, alphas=(a,), **kw1)[2]
                  for a in kw.get("alphas", ALPHAS)]
            self.rolls.append(dict(J=res[2], ok=res[3], alpha_gap=two_best_gap(Js), Js=Js,
                                   args=(X_ext, U_ext, K, k, dict(kw))))
            return res

        def sweep(*a, **kw):
            try:
                r = sweep0(*a, **kw)
            except Exception:
                self.sweeps.append(False)
                raise
            self.sweeps.append(True)
            return r

        rs.onepass_pick_T_singlepass, rs.onepass_rollout = pick, roll
        rs.value_expansions_and_gains_prefix = sweep
        return self

    def __exit__(self, *exc):
        (rs.onepass_pick_T_singlepass, rs.onepass_rollout,
         rs.value_expansions_and_gains_prefix) = self._orig


def accept_margins(J_hist, rolls):
    """the accept / reject margin of every rollout: replay solver.py:719 on the recorded
    candidates, with J_prev starting at the warm start's J (or +inf without one)"""
    for first in ((J_hist[0],) if J_hist else ()) + (np.inf,):
        prev, acc, marg = first, [], []
        for r in rolls:
            if np.isfinite(prev) and np.isfinite(r["J"]):
                marg.append(abs(r["J"] - prev) / abs(prev))
            if r["ok"] and r["J"] < prev:
                prev = r["J"]
                acc.append(prev)
        want = J_hist[1:] if np.isfinite(first) else J_hist
        if acc == list(want):
            return marg
    raise RuntimeError("the recorded rollouts do not replay to J_hist")


def solve(p, S_window, max_iter, x0=None, U_init=None):
    with Recorder() as rec:
        sol = rs.ilqr_timeopt(p["F"], p["x0"] if x0 is None else x0, p["xg"], p["u_ref"], p["Q"],
                              p["R"], p["alpha"], p["w"], p["N"], p["T_min"], p["T_max"],
                              U_init=U_init, method="onepass", max_iter=max_iter,
                              S_window=S_window, wrap_idx=p["wrap_idx"],
                              use_central_diff=p["central"], extra_stage_cost=p["esc"])
    Jc = sol["J_curve"]
    d = dict(x0=p["x0"] if x0 is None else x0, S_window=np.int64(S_window),
             max_iter=np.int64(max_iter), X=sol["X"], U=sol["U"],
             J_hist=np.array(sol["J_hist"], float), T_hist=np.array(sol["T_hist"], np.int64),
             T_star=np.int64(sol["T_star"]), has_curve=np.bool_(Jc is not None),
             J_curve=np.full(p["T_max"], np.nan) if Jc is None else Jc,
             has_error=np.bool_(sol["onepass_error"] is not None),
             n_picks=np.int64(len(rec.picks)), n_rollouts=np.int64(len(rec.rolls)),
             sweeps_ok=np.array(rec.sweeps, bool))
    if U_init is not None:
        d["U_init"] = U_init
    return sol, rec, d


def margins(sol, rec):
    acc = accept_margins(sol["J_hist"], rec.rolls) if all(rec.sweeps) else [0.0]
    return dict(window_gap=np.array([q["window_gap"] for q in rec.picks]),
                gate_margin=np.array([q["gate"] for q in rec.picks]),
                alpha_gap=np.array([r["alpha_gap"] for r in rec.rolls]),
                accept_margin=np.array(acc))


def passes(mg, rec):
    mins = {k: (float(v.min()) if v.size else np.inf) for k, v in mg.items()}
    ok = (all(rec.sweeps) and mins["window_gap"] >= MIN_WINDOW_GAP
          and mins["gate_margin"] >= MIN_GATE and mins["alpha_gap"] >= MIN_ALPHA_GAP
          and mins["accept_margin"] >= MIN_ACCEPT)
    return ok, mins


def solve_cases():
    kept = {}
    for name, tag, S in (("di", "di", 3), ("pointmass", "pointmass", 3),
                         ("cartpole", "cartpole", 3), ("quadrotor", "quadrotor", 3),
                         ("di_s6", "di", 6)):
        p = problem(tag)
        sol, rec, d = solve(p, S, 6)
        mg = margins(sol, rec)
        ok, mins = passes(mg, rec)
        print(f"solve {name}: T_hist={sol['T_hist']} picks={len(rec.picks)} "
              f"rollouts={len(rec.rolls)} mins={ {k: f'{v:.1e}' for k, v in mins.items()} } "
              f"{'kept' if ok else 'DROPPED'}")
        if ok:
            np.savez(os.path.join(HERE, f"onepass_solve_{name}.npz"), **d, **mg)
            kept[name] = (p, rec)
    # four more DI problems for the batched solve: x0 drawn as run_suite does (sigma 0.2)
    p, nb = problem("di"), 0
    for seed in range(40):
        x0 = p["x0"] + 0.2 * np.random.default_rng(1000 + seed).standard_normal(2)
        sol, rec, d = solve(p, 3, 6, x0=x0)
        mg = margins(sol, rec)
        ok, mins = passes(mg, rec)
        print(f"solve di seed={1000 + seed}: T_hist={sol['T_hist']} rollouts={len(rec.rolls)} "
              f"mins={ {k: f'{v:.1e}' for k, v in mins.items()} } {'kept' if ok else 'dropped'}")
        if ok:
            np.savez(os.path.join(HERE, f"onepass_solve_di_b{nb}.npz"), **d, **mg,
                     seed=np.int64(1000 + seed))
            nb += 1
        if nb == 4:
            break
    else:
        raise RuntimeError("too few DI problems pass the margin filter")
    # the segway maker's start sits at its optimum: draw x0 as run_suite does (seeded,
    # sigma 0.02 per state, scaled up until the solve moves), at most 40 seeds
    p = problem("segway")
    for seed in range(40):
        scale = 2.0 ** (seed // 8)
        rng = np.random.default_rng(seed)
        x0 = p["x0"] + scale * 0.02 * rng.standard_normal(4)
        sol, rec, d = solve(p, 3, 6, x0=x0)
        mg = margins(sol, rec)
        ok, mins = passes(mg, rec)
        ok = ok and len(sol["J_hist"]) >= 2
        print(f"solve segway seed={seed} scale={scale}: T_hist={sol['T_hist']} "
              f"mins={ {k: f'{v:.1e}' for k, v in mins.items()} } {'kept' if ok else 'dropped'}")
        if ok:
            np.savez(os.path.join(HERE, "onepass_solve_segway.npz"), **d, **mg,
                     seed=np.int64(seed), scale=np.float64(scale))
            break
    else:
        print("segway: no seed passes the filter; kernel-level tests only")
    # the fallback path: DI, N = 50, S_window = 3, max_iter = 4, U_init = 0 with NaNs
    p = problem("di")
    for name, first_nan in (("fallback_tail", 20), ("fallback_early", 5)):
        U0 = np.zeros((p["N"], 1))
        if name == "fallback_tail":
            U0[first_nan:] = np.nan
        else:
            U0[first_nan] = np.nan
        # max_iter = 4 is the single-problem case, 6 the row of the batched solve
        for max_iter, suffix in ((4, ""), (6, "_it6")):
            sol, rec, d = solve(p, 3, max_iter, U_init=U0)
            print(f"solve {name}{suffix}: T_hist={sol['T_hist']} J_hist={sol['J_hist']} "
                  f"T_star={sol['T_star']} error={sol['onepass_error'] is not None} "
                  f"sweeps={rec.sweeps}")
            np.savez(os.path.join(HERE, f"onepass_solve_{name}{suffix}.npz"), **d)
    return kept


# ---------------------------------------------------------------- rollout cases
def rollout_cases(kept):
    out, names = {}, []
    for tag in ("di", "pointmass", "quadrotor"):
        p, rec = kept[tag]
        X_ext, U_ext, K, k, kw = rec.rolls[0]["args"]
        S, T_bar = int(kw["S_right"]), int(kw["T_bar"])
        K, k = np.stack(K), np.stack(k)
        variants = [("center", T_bar, K, k, ALPHAS), ("right", T_bar + S, K, k, ALPHAS),
                    ("left", max(1, T_bar - S), K, k, ALPHAS),
                    ("nan_alpha", T_bar, K, k, (1.0, np.nan, 0.25, 0.1)),
                    ("k_zero", T_bar, K, 0.0 * k, ALPHAS)]
        kinf = k.copy()
        kinf[T_bar - 1 + S - 2] = np.inf
        variants.append(("all_fail", T_bar, K, kinf, ALPHAS))
        for name, T_star, Kv, kv, al in variants:
            call = lambda a: rs.onepass_rollout(  # noqa: E731
                p["F"], X_ext, U_ext, p["xg"], p["u_ref"], p["Q"], p["R"], p["alpha"], p["w"],
                list(Kv), list(kv), T_bar=T_bar, T_star=T_star, S_right=S,
                wrap_idx=p["wrap_idx"], extra_stage_cost=p["esc"], alphas=a)
            Xn, Un, J, ok = call(tuple(al))
            Js = np.array([call((a,))[2] for a in al])
            key = f"{tag}_{name}"
            names.append(key)
            out[key + "_T"] = np.array([T_bar, T_star, S])
            out[key + "_K"], out[key + "_k"] = Kv, kv
            out[key + "_alphas"] = np.array(al)
            out[key + "_Xn"], out[key + "_Un"] = Xn, Un
            out[key + "_J"], out[key + "_ok"] = np.float64(J), np.bool_(ok)
            out[key + "_Js"], out[key + "_gap"] = Js, np.float64(two_best_gap(Js))
            print(f"rollout {key}: T*={T_star} ok={ok} J={J:.6g} Js={Js} gap={two_best_gap(Js):.1e}")
        out[tag + "_X_ext"], out[tag + "_U_ext"] = X_ext, U_ext
    out["names"] = np.array(names)
    np.savez(os.path.join(HERE, "onepass_rollout_cases.npz"), **out)


def main():
    pick_cases()
    prefix_cases()
    curve_cases()
    rollout_cases(solve_cases())


if __name__ == "__main__":
    main()
