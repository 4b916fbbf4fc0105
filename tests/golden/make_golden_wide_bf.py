"""Generate the wide-shape brute-force solver goldens (wide_bf_solve_*.npz) by running
the REFERENCE.

Run where a checkout of the reference (dmmsjtu-umich/time-opt-ilqr) is at hand, from
outside both trees, naming the reference's directory (tests/golden/make_golden.py's
source of the reference is the default):

    PYTHONDONTWRITEBYTECODE=1 python <repo>/tests/golden/make_golden_wide_bf.py [REFERENCE_DIR]

It imports the reference's solver from that directory (read only, no bytecode
written) and runs ilqr_timeopt(method="bruteforce", max_iter=8) on the mass-spring chain
of make_golden_wide.py (chain_dynamics below, the same expressions, repeated in
tests/test_gpu_wide_jcurve.py): n = 18 (m = 2), n = 24 (m = 3), n = 30 (m = 3),
dt = 0.1, N = 60, T_min = 8, T_max = 55, Q positive definite on every state.

For every horizon selection of a solve (a call of the reference's
bruteforce_all_Jt_backward_expansion) it records the relative gap between the two
smallest J in the window.  A trial is KEPT only if every gap is >= 1e-3: below that a
last-bit difference may move the argmin, and the test asserts T_hist exactly.  The
filter lives here; the test skips nothing.  Each file holds data only: the settings,
x0, T_hist, J_hist, the final J_curve, X and U and the gaps.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _reference_dir():
    """REFERENCE_DIR from the command line, else the REF of make_golden.py beside this file."""
    if len(sys.argv) > 1:
        return sys.argv[1]
    with open(os.path.join(HERE, "make_golden.py")) as f:
        for line in f:
            if line.startswith("REF = "):
                return line.split("=", 1)[1].strip().strip('"\'')
    raise SystemExit("name the reference's directory on the command line")


sys.path.insert(0, _reference_dir())
os.environ.setdefault("MPLBACKEND", "Agg")

import solver as ref_solver  # noqa: E402

DT, N, T_MIN, T_MAX, MAX_ITER = 0.1, 60, 8, 55, 8
SHAPES = ((18, 2), (24, 3), (30, 3))  # (n, m): n / 2 masses, m actuated
MIN_GAP = 1e-3
KEEP = 3


def chain_dynamics(n, m, dt=DT):
    """x = [positions (n/2), velocities (n/2)]; unit masses in a chain fixed at both
    ends, spring force k d + ks sin(d) on the stretch d, damping c; input j pushes
    mass j * (n/2) // m.  Explicit Euler step."""
    p = n // 2
    act = [j * p // m for j in range(m)]
    k, ks, c = 2.0, 0.5, 0.3

    def F(x, u):
        x = np.asarray(x, dtype=float).reshape(-1)
        u = np.asarray(u, dtype=float).reshape(-1)
        q, v = x[:p], x[p:]
        ext = np.concatenate(([0.0], q, [0.0]))
        d = np.diff(ext)                      # stretch of spring i (between i-1 and i)
        f = k * d + ks * np.sin(d)
        acc = f[1:] - f[:-1] - c * v
        for j, i in enumerate(act):
            acc[i] += u[j]
        return np.concatenate((q + dt * v, v + dt * acc))

    return F


def problem(n, m, seed):
    rng = np.random.default_rng(seed)
    p = n // 2
    x0 = np.concatenate((rng.uniform(-1.0, 1.0, p), 0.2 * rng.standard_normal(p)))
    xg = np.zeros(n)
    u_ref = np.zeros(m)
    Q = np.diag(np.concatenate((np.full(p, 1.0), np.full(p, 0.2))))
    R = 0.1 * np.eye(m)
    alpha = 20.0
    w = 0.5
    return x0, xg, u_ref, Q, R, alpha, w


def run(n, m, seed):
    F = chain_dynamics(n, m)
    x0, xg, u_ref, Q, R, alpha, w = problem(n, m, seed)
    gaps = []
    real = ref_solver.bruteforce_all_Jt_backward_expansion

    def spy(*a, **k):
        J = real(*a, **k)
        win = np.sort(np.asarray(J)[T_MIN - 1:T_MAX])
        gaps.append(float((win[1] - win[0]) / abs(win[0])))
        return J

    ref_solver.bruteforce_all_Jt_backward_expansion = spy
    try:
        sol = ref_solver.ilqr_timeopt(F, x0, xg, u_ref, Q, R, alpha, w, N, T_MIN, T_MAX,
                                      method="bruteforce", max_iter=MAX_ITER)
    finally:
        ref_solver.bruteforce_all_Jt_backward_expansion = real
    return dict(n=n, m=m, seed=seed, dt=DT, N=N, T_min=T_MIN, T_max=T_MAX, max_iter=MAX_ITER,
                x0=x0, xg=xg, u_ref=u_ref, Q=Q, R=R, alpha=alpha, w=w,
                T_hist=np.asarray(sol["T_hist"], dtype=np.int64),
                J_hist=np.asarray(sol["J_hist"], dtype=np.float64),
                J_curve=np.asarray(sol["J_curve"], dtype=np.float64),
                X=np.asarray(sol["X"]), U=np.asarray(sol["U"]), gaps=np.asarray(gaps))


def main():
    for n, m in SHAPES:
        kept, seed = 0, 4000 + n
        while kept < KEEP:
            d = run(n, m, seed)
            ok = len(d["gaps"]) > 0 and d["gaps"].min() >= MIN_GAP and len(d["T_hist"]) >= 2
            print(f"n={n} seed={seed} selects={len(d['gaps'])} min gap={d['gaps'].min():.2e} "
                  f"T_hist={d['T_hist'].tolist()} {'kept' if ok else 'dropped'}")
            if ok:
                np.savez(os.path.join(HERE, f"wide_bf_solve_n{n}_{kept}.npz"), **d)
                kept += 1
            seed += 1
            if seed > 4000 + n + 40:
                raise RuntimeError("too few trials pass the gap filter")


if __name__ == "__main__":
    main()
