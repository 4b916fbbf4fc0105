"""GPU: the spring-chain device system (include/hop_chain.h, csrc/chain.hip) against the
NumPy chain and host_dynamics (held bit for bit to the reference's loops by
tests/test_host_dynamics.py), and whole solves against the reference's stored ones.

Bars (derived in tests/test_chain_cpu.py): F 4e-15 absolute with its q' half bitwise;
A, B, a_res 1e-9 absolute, unreachable entries exactly 0.0, q' rows bitwise; a rollout of
N = 12 steps 1e-12 absolute (N steps x 4e-15 x the Euler map's <= 1.04 growth per step);
trajectory-level quantities (J relative, X', U') 1e-9; solves: T_hist equal, J_hist 1e-6
elementwise relative (the existing wide tests' bar).
"""
import functools
import os

import numpy as np
import pytest

from test_chain_cpu import F_TOL, LIN_TOL, chain_F, check_lin

pytestmark = pytest.mark.gpu
TRAJ_TOL, ROLL_TOL, SOLVE_TOL = 1e-9, 1e-12, 1e-6
DBL_MAX = np.finfo(float).max


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _chain(p, m, dt=0.1):
    from time_opt_ilqr_amd import systems
    return systems.SpringChain(p, m, dt)


# ---------------------------------------------------------------- 1. dynamics
@pytest.mark.parametrize("p,m", [(1, 1), (2, 1), (8, 3), (12, 12), (15, 4)])
def test_chain_dynamics(dev, p, m):
    from time_opt_ilqr_amd import engine
    rng = np.random.default_rng(31 * p + m)
    X, U = rng.uniform(-1, 1, (37, 2 * p)), rng.uniform(-1, 1, (37, m))
    F = _chain(p, m)
    out = _np(engine.dynamics(F, _t(X, dev), _t(U, dev), F.dt))
    ref = chain_F(p, m)(X, U)
    err = float(np.abs(out - ref).max())
    print(f"chain F device p={p} m={m}: max abs err {err:.2e}")
    assert err <= F_TOL
    assert np.array_equal(out[:, :p], ref[:, :p])
    assert np.array_equal(F(X[3], U[3]), out[3]) and np.array_equal(_np(F.batch(
        _t(X, dev), _t(U, dev))), out)


# ---------------------------------------------------------------- 2. rollout
@pytest.mark.parametrize("p,m", [(12, 3), (15, 4)])
def test_chain_rollout(dev, p, m):
    from time_opt_ilqr_amd import engine, host_dynamics
    rng = np.random.default_rng(57 + p)
    Bn, N = 5, 12
    x0 = np.concatenate((rng.uniform(-1, 1, (Bn, p)), 0.2 * rng.standard_normal((Bn, p))), 1)
    U = rng.uniform(-1, 1, (Bn, N, m))
    U[1, 4, 0] = 1e9     # one push past max_state_norm = 1e6: x_5 and the tail are NaN
    U[3, 6, m - 1] = np.nan
    F = _chain(p, m)
    X = _np(engine.rollout(F, _t(x0, dev), _t(U, dev), F.dt))
    ref = host_dynamics.rollout_batch(F.host(), x0, U)
    assert np.array_equal(np.isnan(X), np.isnan(ref))
    for b, first in ((1, 5), (3, 7)):  # a NaN tail from the same step as the host
        assert np.isnan(ref[b, first:]).all() and not np.isnan(ref[b, :first]).any()
    assert not np.isnan(ref[[0, 2, 4]]).any()
    ok = ~np.isnan(ref)
    err = float(np.abs(X[ok] - ref[ok]).max())
    print(f"chain rollout p={p} m={m}: max abs err {err:.2e}")
    assert err <= ROLL_TOL
    # one shared x0 [n]
    X1 = _np(engine.rollout(F, _t(x0[0], dev), _t(U[:1], dev), F.dt))
    assert np.array_equal(X1[0], X[0])


# ---------------------------------------------------------------- 3. linearisation
@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("p,m", [(12, 3), (15, 4), (1, 1)])
def test_chain_linearize(dev, p, m, central):
    import torch
    from time_opt_ilqr_amd import engine, host_dynamics, linearization
    rng = np.random.default_rng(91 + p)
    Bn, N, n_use, n = 5, 14, 9, 2 * p
    X = rng.uniform(-1, 1, (Bn, N + 1, n))
    U = rng.uniform(-1, 1, (Bn, N, m))
    X[2, 4, 0] = np.nan
    F = _chain(p, m)
    full = engine.linearize(F, _t(X, dev), _t(U, dev), F.dt, central=central, want_fx=True)
    ref = host_dynamics.linearize_batch(F.host(), X, U, central=central)
    A, B, ar = _np(full.A), _np(full.B), _np(full.a_res)
    for g, r in zip((A, B, ar), ref):
        assert np.array_equal(np.isnan(g), np.isnan(r))
    if not central:  # the forward form marks the whole step
        assert np.isnan(A[2, 4]).all() and np.isnan(B[2, 4]).all()
    fin = np.ones((Bn, N), dtype=bool)
    fin[2, 3:5] = False  # the steps that read the NaN state
    check_lin(p, m, (A[fin], B[fin], ar[fin]), tuple(r[fin] for r in ref),
              "device " + ("central" if central else "forward"))
    Fx = chain_F(p, m)(X[:, :N][fin], U[fin])
    assert float(np.abs(_np(full.Fx)[fin] - Fx).max()) <= F_TOL
    # n_use: the steps beyond it are not written
    part = engine.linearize(F, _t(X, dev), _t(U, dev), F.dt, central=central, n_use=n_use)
    assert part.n_use == n_use
    assert np.array_equal(_np(part.A)[:, :n_use], A[:, :n_use], equal_nan=True)
    sent = -7.0
    from time_opt_ilqr_amd import _lib
    At = torch.full((Bn, N, n, n), sent, dtype=torch.float64, device=dev)
    Bt = torch.full((Bn, N, n, m), sent, dtype=torch.float64, device=dev)
    at = torch.full((Bn, N, n), sent, dtype=torch.float64, device=dev)
    Xt, Ut = _t(X, dev), _t(U, dev)
    _lib.check(_lib.load().hop_chain_linearize_f64(
        _lib.C.byref(engine._chain_params(F)), _lib.ptr(Xt), _lib.ptr(Ut), Bn, N, n_use,
        int(central), 1e-5, 1e-5, 1e-6, 1e-6, _lib.ptr(At), _lib.ptr(Bt), _lib.ptr(at), None,
        _lib.stream_handle(dev)))
    for got, whole in ((At, A), (Bt, B), (at, ar)):
        got = _np(got)
        assert (got[:, n_use:] == sent).all()
        assert np.array_equal(got[:, :n_use], whole[:, :n_use], equal_nan=True)
    if p == 12:  # the reference-named drop-ins, one trajectory
        fn = linearization.linearize_central_diff_traj if central else \
            linearization.linearize_forward_diff_traj
        Al, Bl = fn(F, X[0], U[0])
        assert np.array_equal(np.stack(Al), A[0]) and np.array_equal(np.stack(Bl), B[0])
        al = linearization.compute_affine_residuals(F, X[0], U[0])
        assert np.array_equal(np.stack(al)[:, :, 0], ar[0])


# ---------------------------------------------------------------- 4. true cost
def _dense_cost(p, m, rng):
    n = 2 * p
    G = rng.standard_normal((n, n))
    Q = G @ G.T / n + 0.1 * np.eye(n)
    G = rng.standard_normal((n, n))
    Qf = 3.0 * (G @ G.T / n) + np.eye(n)
    G = rng.standard_normal((m, m))
    R = G @ G.T / m + 0.1 * np.eye(m)
    return rng.uniform(-0.3, 0.3, n), rng.uniform(-0.2, 0.2, m), Q, R, Qf, 0.37


@pytest.mark.parametrize("dense", [True, False])
def test_chain_cost_true(dev, dense):
    from time_opt_ilqr_amd import engine, host_dynamics
    p, m, N = 12, 3, 12
    Bn = N + 3
    rng = np.random.default_rng(123)
    xg, ur, Q, R, Qf, w = _dense_cost(p, m, rng)
    if not dense:
        Q, R, Qf = np.diag(np.diag(Q)), np.diag(np.diag(R)), np.diag(np.diag(Qf))
    X = rng.uniform(-1, 1, (Bn, N + 1, 2 * p))
    U = rng.uniform(-1, 1, (Bn, N, m))
    T = np.array(list(range(1, N + 1)) + [0, 7, N + 1], dtype=np.int32)
    X[N + 1, 5, p + 2] = np.nan  # inside the rows T = 7 reads
    X[3, 9, 1] = np.nan          # beyond T = 4: not read
    F = _chain(p, m)
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), w)
    J = _np(engine.cost_true(F, _t(X, dev), _t(U, dev), T, cost))
    ref = np.array([host_dynamics.cost_true(X[b], U[b], xg, ur, Q, R, Qf, w, int(T[b]))
                    for b in range(Bn - 1)])
    assert J[N] == np.inf and ref[N] == np.inf          # T = 0
    assert J[N + 1] == np.inf and ref[N + 1] == np.inf  # a NaN state
    assert np.isnan(J[N + 2])                           # T > N (hop_cost_true_f64's convention)
    err = _elem_rel(J[:N], ref[:N])
    print(f"chain cost_true dense={dense}: max rel err {err:.2e}")
    assert err <= TRAJ_TOL


# ---------------------------------------------------------------- 5. line search
def _host_candidate(H, X, U, T, K, k, cost_np, alpha):
    """J' of one (problem, alpha) as host_dynamics.linesearch forms it (NaN when the
    rollout is not finite)"""
    from time_opt_ilqr_amd import host_dynamics
    N = len(U)
    Xn, Un = np.zeros_like(X), U.copy()
    Xn[0] = X[0]
    with np.errstate(all="ignore"):
        for i in range(N):
            if i < T:
                Un[i] = U[i] + (K[i] @ (Xn[i] - X[i]) + alpha * k[i])
            Xn[i + 1] = H(Xn[i], Un[i])
            if not np.all(np.isfinite(Xn[i + 1])):
                return np.nan
        return host_dynamics.cost_true(Xn, Un, *cost_np[:6], T)


@functools.lru_cache(maxsize=None)
def _linesearch_case():
    """B = 6, N = 12, (p, m) = (12, 3).  Gains: engine.riccati on the device
    linearisation.  T* = 1, N and values between; problem 2 is inactive; in problem 5 the
    alpha = 1 rollout overflows and a later index wins.  The filter (every (problem,
    alpha) has |J' - J_old| >= 1e-6 |J_old| in the host result, so no accept decision
    hangs on the last bits) runs here, on the CPU, over a pool of candidates.

    The overflow: a control is costed, so a finite winning J' keeps every control and
    hence every state up to T* moderate, and beyond T* the chain is linear plus a bounded
    sine: an overflow that separates alpha = 1 from alpha = 0.5 needs a direction the
    cost does not see.  The line search's R and Qf carry a zero row and column on input
    m - 1 and on the velocity it drives; problem 5 has T* = 1, k_0 on that input makes
    acc_1 = 1.5 x 2^970 at alpha = 1 and 0.75 x 2^970 at alpha = 0.5, and U_1 there is
    DBL_MAX, whose sum with acc_1 overflows exactly when acc_1 >= 2^970 (half an ulp)."""
    import torch
    from time_opt_ilqr_amd import engine, host_dynamics
    from time_opt_ilqr_amd.utils import as_terminal_weight
    dev = torch.device("cuda", 0)
    p, m, N, pool = 12, 3, 12, 24
    n = 2 * p
    F = _chain(p, m)
    H = F.host()
    rng = np.random.default_rng(777)
    x0 = np.concatenate((rng.uniform(-1, 1, (pool, p)), 0.2 * rng.standard_normal((pool, p))), 1)
    U = 0.3 * rng.uniform(-1, 1, (pool, N, m))
    xg, ur = np.zeros(n), np.zeros(m)
    Q = np.diag(np.concatenate((np.full(p, 1.0), np.full(p, 0.2))))
    R, Qf = 0.1 * np.eye(m), as_terminal_weight(20.0, n)
    w = 0.5
    T = np.array([1, N, 5, 9, 3, 1] * (pool // 6), dtype=np.int32)
    X = engine.rollout(F, _t(x0, dev), _t(U, dev), F.dt)
    lin = engine.linearize(F, X, _t(U, dev), F.dt, central=True)
    ric = engine.riccati(lin.A, lin.B, X, _t(U, dev), _t(xg, dev), _t(ur, dev), _t(Q, dev),
                         _t(R, dev), _t(Qf, dev), _t(T, dev, torch.int32), 1e-3, mode=0,
                         reg_max_tries=1)
    assert int(ric.status.abs().sum()) == 0
    X, K, k = _np(X), _np(ric.K), _np(ric.k)
    for b in range(pool):  # the pass writes steps < T* only
        K[b, T[b]:], k[b, T[b]:] = 0.0, 0.0
    # the line search's cost: blind to input m - 1 and to the velocity it drives
    ja, va = m - 1, p + (m - 1) * p // m
    R_ls, Qf_ls = R.copy(), Qf.copy()
    R_ls[ja, ja] = 0.0
    Qf_ls[va, va] = 0.0
    cost_np = (xg, ur, Q, R_ls, Qf_ls, w, None)
    alphas = engine.ALPHAS
    kept = {}
    for role in range(6):
        for b in range(role, pool, 6):
            Xb, Ub, Kb, kb = X[b].copy(), U[b].copy(), K[b].copy(), k[b].copy()
            if role == 5:
                kb[0, ja] = -1.5 * 2.0 ** 970 / (F.c * F.dt)
                Ub[1, ja] = DBL_MAX
            J0 = host_dynamics.cost_true(Xb, Ub, *cost_np[:6], int(T[b]))
            Jc = np.array([_host_candidate(H, Xb, Ub, int(T[b]), Kb, kb, cost_np, al)
                           for al in alphas])
            clear = np.all(~np.isfinite(Jc) | (np.abs(Jc - J0) >= 1e-6 * abs(J0)))
            if role == 5:  # alpha = 1 overflows, a later index wins
                clear = clear and np.isnan(Jc[0]) and bool(np.any(Jc[1:] < J0))
            if clear:
                kept[role] = (Xb, Ub, Kb, kb, int(T[b]))
                break
        assert role in kept, f"no candidate for problem {role} passes the builder's filter"
    Xs, Us, Ks, ks, Ts = (np.stack([kept[r][i] for r in range(6)]) for i in range(5))
    active = np.array([1, 1, 0, 1, 1, 1], dtype=np.int32)
    ref = host_dynamics.linesearch_batch(H, Xs, Us, Ts, Ks, ks, active, cost_np, alphas)
    return dict(F=F, X=Xs, U=Us, K=Ks, k=ks, T=Ts.astype(np.int32), active=active, ref=ref,
                cost=(xg, ur, Q, R_ls, Qf_ls, w))


def test_chain_forward_linesearch(dev):
    from time_opt_ilqr_amd import engine
    c = _linesearch_case()
    F = c["F"]
    xg, ur, Q, R, Qf, w = c["cost"]
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), w)
    r = engine.forward_linesearch(F, _t(c["X"], dev), _t(c["U"], dev), c["T"], _t(c["K"], dev),
                                  _t(c["k"], dev), cost, F.dt, active=c["active"])
    Xo, Uo, J, J0, acc = c["ref"]
    got = _np(r.accepted)
    print("chain line search accepted", got.tolist(), "host", acc.tolist())
    assert got.tolist() == acc.tolist()
    assert got[2] == -2 and got[5] >= 1 and sorted(c["T"].tolist()) == [1, 1, 3, 5, 9, 12]
    on = c["active"] != 0
    eJ, eJ0 = _elem_rel(_np(r.J)[on], J[on]), _elem_rel(_np(r.J_old)[on], J0[on])
    big = np.abs(Xo) > 10.0  # the overflow problem's tail: relative there
    eX = float((np.abs(_np(r.X) - Xo) / np.where(big, np.abs(Xo), 1.0)).max())
    bigu = np.abs(Uo) > 10.0
    eU = float((np.abs(_np(r.U) - Uo) / np.where(bigu, np.abs(Uo), 1.0)).max())
    print(f"chain line search: J {eJ:.2e} J_old {eJ0:.2e} X' {eX:.2e} U' {eU:.2e}")
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL
    # the inactive problem keeps X, U bit for bit
    assert np.array_equal(_np(r.X)[2], c["X"][2]) and np.array_equal(_np(r.U)[2], c["U"][2])


# ---------------------------------------------------------------- 6. zero gains
@pytest.mark.parametrize("dense", [False, True])
def test_chain_linesearch_zero_gains_is_the_rollout(dev, dense):
    import torch
    from time_opt_ilqr_amd import engine
    p, m, Bn, N = 12, 3, 5, 12
    rng = np.random.default_rng(99)
    xg, ur, Q, R, Qf, w = _dense_cost(p, m, rng)
    if not dense:
        Q, R, Qf = np.diag(np.diag(Q)), np.diag(np.diag(R)), np.diag(np.diag(Qf))
    F = _chain(p, m)
    x0 = rng.uniform(-1, 1, (Bn, 2 * p))
    U = _t(rng.uniform(-1, 1, (Bn, N, m)), dev)
    X = engine.rollout(F, _t(x0, dev), U, F.dt)
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), w)
    K = torch.zeros((Bn, N, m, 2 * p), dtype=torch.float64, device=dev)
    k = torch.zeros((Bn, N, m), dtype=torch.float64, device=dev)
    T = np.array([1, 4, 7, N, 9], dtype=np.int32)
    r = engine.forward_linesearch(F, X, U, T, K, k, cost, F.dt)
    assert _np(r.accepted).tolist() == [-1] * Bn
    assert torch.equal(r.J, r.J_old) and torch.equal(r.X, X) and torch.equal(r.U, U)
    assert torch.equal(engine.cost_true(F, X, U, T, cost), r.J_old)
    # the candidates themselves, from a workspace of the test's own: every (problem,
    # alpha) row is the rollout and its J is J_old, bit for bit
    from time_opt_ilqr_amd import _lib
    lib, al = _lib.load(), engine.ALPHAS
    cp = engine._chain_params(F)
    cargs, keep = engine._chain_cost_args(cost, Bn, 2 * p, m, dev)
    nb = int(lib.hop_chain_forward_workspace_bytes(_lib.C.byref(cp), Bn, N, len(al)))
    ws = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    Tt = _t(T, dev, torch.int32)
    out = [torch.empty_like(X), torch.empty_like(U)] + [
        torch.empty((Bn,), dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.empty((Bn,), dtype=torch.int32, device=dev)]
    _lib.check(lib.hop_chain_forward_linesearch_f64(
        _lib.C.byref(cp), _lib.ptr(X), _lib.ptr(U), *cargs, _lib.ptr(Tt), None, _lib.ptr(K),
        _lib.ptr(k), (_lib.C.c_double * len(al))(*al), len(al), Bn, N, _lib.ptr(ws), nb,
        *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
    torch.cuda.synchronize(dev)
    Jc = ws[:Bn * len(al)].reshape(Bn, len(al))
    assert torch.equal(Jc, r.J_old[:, None].expand(Bn, len(al)))
    rows = ws[Bn * len(al):].reshape(Bn, len(al), -1)
    nx = (N + 1) * 2 * p
    assert torch.equal(rows[:, :, :nx], X.reshape(Bn, 1, nx).expand(Bn, len(al), nx))
    assert torch.equal(rows[:, :, nx:], U.reshape(Bn, 1, -1).expand(Bn, len(al), N * m))


# ---------------------------------------------------------------- 7. single solves
def _solve_fixture(dev, golden_dir, name, method):
    from time_opt_ilqr_amd import solver
    d = np.load(os.path.join(golden_dir, name))
    assert float(d["gaps"].min()) >= 1e-3
    n, m = int(d["n"]), int(d["m"])
    F = _chain(n // 2, m, float(d["dt"]))
    sol = solver.ilqr_timeopt(F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], float(d["alpha"]),
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method=method, max_iter=int(d["max_iter"]))
    assert list(sol["T_hist"]) == d["T_hist"].tolist(), (name, sol["T_hist"])
    err = _elem_rel(np.asarray(sol["J_hist"]), d["J_hist"])
    print(name, method, "J_hist relative error", err)
    assert err <= SOLVE_TOL
    return F, d, sol


@pytest.mark.parametrize("trial", range(3))
@pytest.mark.parametrize("n", [16, 24, 30])
def test_chain_solve_propagator_vs_reference(dev, golden_dir, n, trial):
    _solve_fixture(dev, golden_dir, f"wide_solve_n{n}_{trial}.npz", "propagator")


@pytest.mark.parametrize("trial", range(3))
@pytest.mark.parametrize("n", [18, 24, 30])
def test_chain_solve_bruteforce_vs_reference(dev, golden_dir, n, trial):
    _solve_fixture(dev, golden_dir, f"wide_bf_solve_n{n}_{trial}.npz", "bruteforce")


@pytest.mark.parametrize("trial", range(3))
def test_chain_solve_narrow_vs_reference(dev, golden_dir, trial):
    """n = 8, m = 2: the narrow select and Riccati kernels under the same device system"""
    from time_opt_ilqr_amd import solver
    F, d, sol = _solve_fixture(dev, golden_dir, f"chain_solve_n8_{trial}.npz", "propagator")
    if trial == 0:  # the reference-named drop-ins on the solution
        T = int(sol["T_star"])
        args = (d["xg"], d["u_ref"], d["Q"], d["R"], float(d["alpha"]), float(d["w"]))
        X = solver.rollout(F, d["x0"], sol["U"])
        assert np.array_equal(X, sol["X"])
        J = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, system=F)
        assert abs(J - sol["J_hist"][-1]) <= TRAJ_TOL * abs(J)
        sol2 = solver.ilqr_timeopt_ourmethod(F, d["x0"], *args, int(d["N"]), int(d["T_min"]),
                                             int(d["T_max"]), max_iter=int(d["max_iter"]))
        assert sol2["T_hist"] == sol["T_hist"] and sol2["J_hist"] == sol["J_hist"]


# ---------------------------------------------------------------- 8. batched solves
def test_chain_batched_solve(dev, golden_dir):
    from time_opt_ilqr_amd import host_dynamics, solver
    from time_opt_ilqr_amd.utils import as_terminal_weight
    ds = [np.load(os.path.join(golden_dir, f"wide_solve_n24_{t}.npz")) for t in range(3)]
    d = ds[0]
    order = [2, 0, 1, 1, 2, 0, 2]  # B = 7, permuted
    F = _chain(12, int(d["m"]), float(d["dt"]))
    assert not isinstance(F, host_dynamics.HostDynamics)
    res = solver.ilqr_timeopt_batch(
        F, np.stack([ds[i]["x0"] for i in order]), d["xg"], d["u_ref"], d["Q"], d["R"],
        as_terminal_weight(float(d["alpha"]), 24), float(d["w"]), int(d["N"]), int(d["T_min"]),
        int(d["T_max"]), max_iter=int(d["max_iter"]), stage_timers=False)
    assert _np(res["crashed"]).tolist() == [0] * 7
    nh = _np(res["n_hist"])
    worst = 0.0
    for b, i in enumerate(order):
        x = ds[i]
        assert _np(res["T_hist"][b, :nh[b]]).tolist() == x["T_hist"].tolist(), b
        worst = max(worst, _elem_rel(_np(res["J_hist"][b, :nh[b]]), x["J_hist"]))
    print("chain batched solve: J_hist relative error", worst)
    assert worst <= SOLVE_TOL


# ---------------------------------------------------------------- 9. refusals
def test_chain_refusals(dev):
    import torch
    from time_opt_ilqr_amd import engine, solver, systems
    mk = systems.make_spring_chain(12, 3, seed=1)
    F, x0, xg, ur, Q, R = mk[:6]
    N = 12
    U = torch.zeros((2, N, 3), dtype=torch.float64, device=dev)
    X = engine.rollout(F, _t(x0, dev), U, F.dt)
    with pytest.raises(ValueError, match="tile64"):
        engine.linearize(F, X, U, F.dt, tile64=True)
    t = lambda a: _t(a, dev)  # noqa: E731
    K = torch.zeros((2, N, 3, 24), dtype=torch.float64, device=dev)
    k = torch.zeros((2, N, 3), dtype=torch.float64, device=dev)
    for kw in (dict(wrap_idx=[2]), dict(obstacles=np.array([[0.0, 0.0, 1.0, 1.0]]))):
        cost = engine.CostParams(t(xg), t(ur), t(Q), t(R), t(np.eye(24)), 0.5, **kw)
        with pytest.raises(ValueError):
            engine.cost_true(F, X, U, [N, N], cost)
        with pytest.raises(ValueError):
            engine.forward_linesearch(F, X, U, [N, N], K, k, cost, F.dt)
        with pytest.raises(ValueError):
            solver.ilqr_timeopt_batch(F, x0, xg, ur, Q, R, np.eye(24), 0.5, N, 2, N, **kw)
    with pytest.raises(ValueError):
        solver.ilqr_timeopt_batch(F, x0, xg, ur, Q, R, np.eye(24), 0.5, N, 2, N,
                                  extra_stage_cost=lambda x, u: (0.0, np.zeros(24),
                                                                 np.zeros((24, 24))))
