"""GPU: fleets of the built-in systems as device systems (include/hop_fleet.h,
csrc/fleet.hip).

Yardsticks and bars:
* dynamics, rollout and the linearisation's diagonal blocks, a_res and Fx: the existing
  kernels (hop_dynamics_f64, hop_rollout_f64, hop_linearize_f64) run on each member's
  slice -- bitwise, no tolerance; every off-block entry of A and B exactly 0.0;
* the NaN pattern of a step with a NaN in one member, the true cost and the line search:
  fixtures of the reference on the stacked callable (tests/golden/make_golden_fleet.py),
  J, X' and U' to the chain test's TRAJ_TOL = 1e-9, accepted indices exact (the
  generator keeps only cases whose every candidate is 1e-6 clear of J_old);
* whole solves: T_hist equal, J_hist to the chain test's SOLVE_TOL = 1e-6 against
  tests/golden/fleet_solve_*.npz (every select gap >= 1e-3, filtered by the generator).
Batch sizes 1, 5 and 67: none a multiple of 4 (rows per wave), 67 crosses a wave and a
workgroup.
"""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRAJ_TOL, SOLVE_TOL = 1e-9, 1e-6
N = 12
BATCHES = (1, 5, 67)
# base system id, count, n, m
SHAPES = {"di1": (0, 1, 2, 1), "di7": (0, 7, 14, 7), "di8": (0, 8, 16, 8),
          "di15": (0, 15, 30, 15), "pm7": (3, 7, 28, 14), "cp5": (1, 5, 20, 5),
          "seg6": (4, 6, 24, 6), "quad2": (2, 2, 24, 8)}
TAGS = list(SHAPES)
FLEET_LDS = (256, (2 * 31 * 31 + 16 * 16 + 16 * 32) * 8)  # threads, bytes: cost / line search


# BEGIN case_inputs (repeated verbatim in tests/test_gpu_fleet.py)
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


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _fleet(tag):
    from time_opt_ilqr_amd import systems
    sid, count, n, m = SHAPES[tag]
    F = systems.Fleet(sid, count)
    assert (F.n, F.m) == (n, m)
    return F


@functools.lru_cache(maxsize=None)
def _case(tag, golden_dir):
    sid, count, n, m = SHAPES[tag]
    d = np.load(os.path.join(golden_dir, f"fleet_cases_{tag}.npz"))
    c = case_inputs(int(d["seed"]), n, m, n // count)
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum()])
    assert np.array_equal(got, d["check"]), "the inputs are not the generator's"
    return c, d


def _members(F, t):
    """the member slices of a tensor whose last axis is the stacked state or input"""
    k = F.n_member if t.shape[-1] == F.n else F.m_member
    return [t[..., a * k:(a + 1) * k].contiguous() for a in range(F.count)]


def _cost(c, F, dev):
    from time_opt_ilqr_amd import engine
    return engine.CostParams(_t(c["xg"], dev), _t(c["u_ref"], dev), _t(c["Q"], dev),
                             _t(c["R"], dev), _t(c["Qf"], dev), c["w"], None, F.wrap_idx)


# ---------------------------------------------------------------- 1. dynamics, rollout
@pytest.mark.parametrize("tag", TAGS)
def test_fleet_dynamics_is_the_members_kernel_bitwise(dev, tag):
    import torch
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    rng = np.random.default_rng(5 + F.n)
    for Bn in BATCHES:
        X = _t(rng.uniform(-1.0, 1.0, (Bn, F.n)), dev)
        U = _t(rng.uniform(-1.0, 1.0, (Bn, F.m)), dev)
        got = engine.dynamics(F, X, U, F.dt)
        ref = torch.cat([engine.dynamics(F.base_id, x, u, F.dt)
                         for x, u in zip(_members(F, X), _members(F, U))], -1)
        assert torch.equal(got, ref), (tag, Bn)
        assert torch.equal(F.batch(X, U), got)
    # strided rows: only the n (m) leading entries of each row are read and written
    from time_opt_ilqr_amd import _lib
    Xs = _t(rng.uniform(-1.0, 1.0, (5, F.n + 3)), dev)
    Us = _t(rng.uniform(-1.0, 1.0, (5, F.m + 2)), dev)
    out = torch.full((5, F.n + 1), -7.0, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().hop_fleet_dynamics_f64(
        _lib.C.byref(engine._fleet_params(F)), _lib.ptr(Xs), F.n + 3, _lib.ptr(Us), F.m + 2, 5,
        _lib.ptr(out), F.n + 1, _lib.stream_handle(dev)))
    ref = engine.dynamics(F, Xs[:, :F.n].contiguous(), Us[:, :F.m].contiguous(), F.dt)
    assert torch.equal(out[:, :F.n], ref) and bool((out[:, F.n] == -7.0).all())


@pytest.mark.parametrize("tag", TAGS)
def test_fleet_rollout_is_the_members_kernel_bitwise(dev, tag):
    import torch
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    rng = np.random.default_rng(17 + F.n)
    for Bn in BATCHES:
        x0 = _t(rng.uniform(-0.5, 0.5, (Bn, F.n)), dev)
        # the quadrotor: torques small enough that no member meets its pitch guard in N steps
        U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * (0.05 if F.base_id == 2 else 1.0), dev)
        got = engine.rollout(F, x0, U, F.dt)
        ref = torch.cat([engine.rollout(F.base_id, x, u, F.dt)
                         for x, u in zip(_members(F, x0), _members(F, U))], -1)
        assert bool(torch.isfinite(ref).all()) and torch.equal(got, ref), (tag, Bn)
    # a shared x0 (batch stride 0)
    got = engine.rollout(F, x0[0], U, F.dt)
    assert torch.equal(got[:, 0], x0[:1].expand(Bn, F.n))
    assert torch.equal(got[0], engine.rollout(F, x0[:1], U[:1], F.dt)[0])


def test_fleet_rollout_stops_on_the_stacked_norm(dev):
    """DI x 8 (no libm: NumPy gives the same bits).  Member 0 accelerates, the others sit
    at position 3; max_state_norm = 10 is crossed by the stacked norm while every member's
    own norm is below it.  The reference's rule (solver.py:42-62) on the stacked state, in
    NumPy: the first state that is not finite or has norm > max_state_norm and every state
    after it are NaN, for every member."""
    import torch
    from time_opt_ilqr_amd import engine
    F = _fleet("di8")
    dt, M, Bn = F.dt, 10.0, 5
    x0 = np.zeros((Bn, F.n))
    x0[:, 2::2] = 3.0
    U = np.zeros((Bn, N, F.m))
    U[:, :, 0] = 15.0 + 3.0 * np.arange(Bn)[:, None]  # a different step per problem
    U[Bn - 1, :, 0] = 1.0                                # the last problem never trips
    ref = np.zeros((Bn, N + 1, F.n))
    ref[:, 0] = x0
    stop = []
    for b in range(Bn):
        for k in range(N):
            x, u = ref[b, k], U[b, k]
            xn = np.empty(F.n)
            xn[0::2] = x[0::2] + dt * x[1::2]
            xn[1::2] = x[1::2] + dt * u
            nrm = float(np.linalg.norm(xn))
            assert abs(nrm - M) > 1e-6  # the decision does not rest on the order of the sum
            if not np.all(np.isfinite(xn)) or nrm > M:
                ref[b, k + 1:] = np.nan
                # only the stacked norm trips: every member's own norm is below the bound
                assert max(np.hypot(xn[0::2], xn[1::2])) < M
                break
            ref[b, k + 1] = xn
        stop.append(int(np.isnan(ref[b, :, 0]).argmax()) if np.isnan(ref[b]).any() else -1)
    assert stop[-1] == -1 and all(2 <= s <= N for s in stop[:-1]) and len(set(stop)) >= 3, stop
    got = _np(engine.rollout(F, _t(x0, dev), _t(U, dev), dt, max_state_norm=M))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
    # the members' own kernel with the same bound runs on
    mem = engine.rollout(0, _t(x0[:, :2], dev), _t(U[:, :, :1], dev), dt, max_state_norm=M)
    assert bool(torch.isfinite(mem[0, :stop[0] + 1]).all())


# ---------------------------------------------------------------- 2. linearisation
@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("tag", TAGS)
def test_fleet_linearize_blocks_bitwise_and_zeros(dev, tag, central):
    import torch
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    ns, ms = F.n_member, F.m_member
    rng = np.random.default_rng(23 + F.n)
    mA = torch.kron(torch.eye(F.count), torch.ones(ns, ns)).bool().to(dev)
    mB = torch.kron(torch.eye(F.count), torch.ones(ns, ms)).bool().to(dev)
    for Bn in BATCHES:
        X = _t(rng.uniform(-1.0, 1.0, (Bn, N + 1, F.n)), dev)
        U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)), dev)
        r = engine.linearize(F, X, U, F.dt, central=central, want_fx=True)
        for t, mk in ((r.A, mA), (r.B, mB)):
            off = t[..., ~mk]
            assert bool((off == 0.0).all()) and not bool(torch.signbit(off).any()), (tag, Bn)
        for a, (x, u) in enumerate(zip(_members(F, X), _members(F, U))):
            ref = engine.linearize(F.base_id, x, u, F.dt, central=central, want_fx=True)
            sl, su = slice(a * ns, (a + 1) * ns), slice(a * ms, (a + 1) * ms)
            assert torch.equal(r.A[..., sl, sl], ref.A) and torch.equal(r.B[..., sl, su], ref.B)
            assert torch.equal(r.a_res[..., sl], ref.a_res) and torch.equal(r.Fx[..., sl], ref.Fx)


@pytest.mark.parametrize("tag", TAGS)
def test_fleet_linearize_nan_pattern_and_tail(dev, golden_dir, tag):
    """the reference's NaN pattern for a NaN in one member's state at one step (fixture),
    and steps k >= n_use left untouched (a_res and Fx nullable)"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    F = _fleet(tag)
    c, d = _case(tag, golden_dir)
    X, U = _t(c["Xn"][None], dev), _t(c["Un"][None], dev)
    for form, central in (("fwd", False), ("cen", True)):
        r = engine.linearize(F, X, U, F.dt, central=central)
        assert np.array_equal(_np(torch.isnan(r.A[0])), d[f"nan_A_{form}"]), (tag, form)
        assert np.array_equal(_np(torch.isnan(r.B[0])), d[f"nan_B_{form}"]), (tag, form)
    k = c["nan_at"][0]
    assert bool(torch.isnan(r.a_res[0, k - 1]).any()) and bool(torch.isnan(r.a_res[0, k]).any())
    # n_use = 7 of 12: the tail keeps what it held
    Bn, n_use = 5, 7
    rng = np.random.default_rng(31 + F.n)
    X = _t(rng.uniform(-1.0, 1.0, (Bn, N + 1, F.n)), dev)
    U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)), dev)
    full = engine.linearize(F, X, U, F.dt, central=True, want_fx=True)
    A = torch.full((Bn, N, F.n, F.n), -7.0, dtype=torch.float64, device=dev)
    B = torch.full((Bn, N, F.n, F.m), -7.0, dtype=torch.float64, device=dev)
    for ar in (torch.full((Bn, N, F.n), -7.0, dtype=torch.float64, device=dev), None):
        _lib.check(_lib.load().hop_fleet_linearize_f64(
            _lib.C.byref(engine._fleet_params(F)), _lib.ptr(X), _lib.ptr(U), Bn, N, n_use, 1, 1e-5,
            1e-5, 1e-6, 1e-6, _lib.ptr(A), _lib.ptr(B), _lib.ptr(ar), None,
            _lib.stream_handle(dev)))
        assert bool((A[:, n_use:] == -7.0).all()) and bool((B[:, n_use:] == -7.0).all())
        assert torch.equal(A[:, :n_use], full.A[:, :n_use])
        assert torch.equal(B[:, :n_use], full.B[:, :n_use])
        if ar is not None:
            assert bool((ar[:, n_use:] == -7.0).all())
            assert torch.equal(ar[:, :n_use], full.a_res[:, :n_use])


# ---------------------------------------------------------------- 3. true cost
@pytest.mark.parametrize("tag", TAGS)
def test_fleet_cost_true_vs_reference(dev, golden_dir, tag):
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    c, d = _case(tag, golden_dir)
    assert sorted(d["wrap_idx"].tolist()) == sorted(F.wrap_idx)
    cost = _cost(c, F, dev)
    worst = 0.0
    for Bn in BATCHES:
        J = _np(engine.cost_true(F, _t(c["X"][:Bn], dev), _t(c["U"][:Bn], dev), c["T"][:Bn], cost))
        worst = max(worst, _elem_rel(J, d["cost_J"][:Bn]))
    print(f"fleet cost_true {tag}: max rel err {worst:.2e}")
    assert worst <= TRAJ_TOL
    # T = 0 -> +inf, T > N -> NaN, a NaN on the rows read -> +inf, beyond them: not read
    X = c["X"][:5].copy()
    X[2, 3, F.n - 1] = np.nan
    X[3, 9, 0] = np.nan
    T = np.array([0, N + 1, 7, 4, N], dtype=np.int32)
    J = _np(engine.cost_true(F, _t(X, dev), _t(c["U"][:5], dev), T, cost))
    assert J[0] == np.inf and np.isnan(J[1]) and J[2] == np.inf and np.isfinite(J[3:]).all()


# ---------------------------------------------------------------- 4. line search
@pytest.mark.parametrize("tag", TAGS)
def test_fleet_forward_linesearch_vs_reference(dev, golden_dir, tag):
    """the reference's forward_linesearch_fixedT on the stacked callable; problem 2 runs
    inactive and is copied through"""
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    c, d = _case(tag, golden_dir)
    pick = d["ls_pick"]
    U, T = c["U0"][pick], c["T0"][pick]
    active = np.array([1, 1, 0, 1], dtype=np.int32)
    on = active != 0
    r = engine.forward_linesearch(F, _t(d["ls_X"], dev), _t(U, dev), T, _t(d["ls_K"], dev),
                                  _t(d["ls_k"], dev), _cost(c, F, dev), F.dt, active=active)
    got = _np(r.accepted)
    print(f"fleet line search {tag}: accepted {got.tolist()} reference {d['ls_acc'].tolist()}")
    assert got[on].tolist() == d["ls_acc"][on].tolist() and got[2] == -2
    assert (got[on] >= 0).all() and len(set(got[on].tolist())) >= 2
    eJ = _elem_rel(_np(r.J)[on], d["ls_J"][on])
    eJ0 = _elem_rel(_np(r.J_old), d["ls_J0"])
    eX = float(np.abs(_np(r.X)[on] - d["ls_Xo"][on]).max())
    eU = float(np.abs(_np(r.U)[on] - d["ls_Uo"][on]).max())
    print(f"fleet line search {tag}: J {eJ:.2e} J_old {eJ0:.2e} X' {eX:.2e} U' {eU:.2e}")
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL
    assert float(np.abs(d["ls_Xo"]).max()) < 50.0  # absolute and relative bars coincide
    assert np.array_equal(_np(r.X)[2], d["ls_X"][2]) and np.array_equal(_np(r.U)[2], U[2])
    assert _np(r.J)[2] == _np(r.J_old)[2]


@pytest.mark.parametrize("tag", TAGS)
def test_fleet_linesearch_zero_gains_is_the_rollout(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    F = _fleet(tag)
    c, _ = _case(tag, golden_dir)
    Bn = 5
    rng = np.random.default_rng(41 + F.n)
    x0 = _t(rng.uniform(-1.0, 1.0, (Bn, F.n)), dev)
    U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)), dev)
    X = engine.rollout(F, x0, U, F.dt)
    cost = _cost(c, F, dev)
    K = torch.zeros((Bn, N, F.m, F.n), dtype=torch.float64, device=dev)
    k = torch.zeros((Bn, N, F.m), dtype=torch.float64, device=dev)
    T = np.array([1, 4, 7, N, 9], dtype=np.int32)
    r = engine.forward_linesearch(F, X, U, T, K, k, cost, F.dt)
    assert _np(r.accepted).tolist() == [-1] * Bn
    assert torch.equal(r.J, r.J_old) and torch.equal(r.X, X) and torch.equal(r.U, U)
    assert torch.equal(engine.cost_true(F, X, U, T, cost), r.J_old)
    # the candidates themselves, from a workspace of the test's own: every (problem,
    # alpha) row is the rollout and its J is J_old, bit for bit
    lib, al = _lib.load(), engine.ALPHAS
    fp = engine._fleet_params(F)
    cargs, keep = engine._chain_cost_args(cost, Bn, F.n, F.m, dev, F)
    nb = int(lib.hop_fleet_forward_workspace_bytes(_lib.C.byref(fp), Bn, N, len(al)))
    assert nb == Bn * len(al) * (1 + (N + 1) * F.n + N * F.m) * 8
    ws = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    Tt = _t(T, dev, torch.int32)
    out = [torch.empty_like(X), torch.empty_like(U)] + [
        torch.empty((Bn,), dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.empty((Bn,), dtype=torch.int32, device=dev)]
    _lib.check(lib.hop_fleet_forward_linesearch_f64(
        _lib.C.byref(fp), _lib.ptr(X), _lib.ptr(U), *cargs, _lib.ptr(Tt), None, _lib.ptr(K),
        _lib.ptr(k), (_lib.C.c_double * len(al))(*al), len(al), Bn, N, _lib.ptr(ws), nb,
        *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
    torch.cuda.synchronize(dev)
    Jc = ws[:Bn * len(al)].reshape(Bn, len(al))
    assert torch.equal(Jc, r.J_old[:, None].expand(Bn, len(al)))
    rows = ws[Bn * len(al):].reshape(Bn, len(al), -1)
    nx = (N + 1) * F.n
    assert torch.equal(rows[:, :, :nx], X.reshape(Bn, 1, nx).expand(Bn, len(al), nx))
    assert torch.equal(rows[:, :, nx:], U.reshape(Bn, 1, -1).expand(Bn, len(al), N * F.m))


# ---------------------------------------------------------------- 5. LDS
@pytest.mark.parametrize("tag", ["di15", "quad2", "cp5"])
def test_fleet_kernels_on_poisoned_lds(dev, golden_dir, tag):
    """the cost and line-search kernels stage Q, Qf, R and a vector per row in LDS: the
    same bits after each of the three fill patterns"""
    from test_gpu_lds_poison import run_poisoned
    from time_opt_ilqr_amd import engine
    F = _fleet(tag)
    c, d = _case(tag, golden_dir)
    cost = _cost(c, F, dev)
    pick = d["ls_pick"]
    Xc, Uc, Tc = _t(c["X"][:5], dev), _t(c["U"][:5], dev), c["T"][:5]
    Xl, Ul, Kl, kl = (_t(a, dev) for a in (d["ls_X"], c["U0"][pick], d["ls_K"], d["ls_k"]))

    def fn():
        r = engine.forward_linesearch(F, Xl, Ul, c["T0"][pick], Kl, kl, cost, F.dt)
        return dict(Jc=engine.cost_true(F, Xc, Uc, Tc, cost), J=r.J, J_old=r.J_old, X=r.X, U=r.U,
                    accepted=r.accepted)

    base = run_poisoned(dev, fn, FLEET_LDS, 2)
    assert _elem_rel(_np(base["Jc"]), d["cost_J"][:5]) <= TRAJ_TOL
    assert _np(base["accepted"]).tolist() == d["ls_acc"].tolist()


# ---------------------------------------------------------------- 6. whole solves
def _solve_fixture(dev, golden_dir, name, method):
    from time_opt_ilqr_amd import solver, systems
    d = np.load(os.path.join(golden_dir, name))
    assert float(d[f"gaps_{method}"].min()) >= 1e-3
    F = systems.Fleet(int(d["sid"]), int(d["count"]))
    sol = solver.ilqr_timeopt(F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method=method, max_iter=int(d["max_iter"]),
                              wrap_idx=d["wrap_idx"].tolist())
    assert list(sol["T_hist"]) == d[f"T_hist_{method}"].tolist(), (name, sol["T_hist"])
    err = _elem_rel(np.asarray(sol["J_hist"]), d[f"J_hist_{method}"])
    print(name, method, "J_hist relative error", err)
    assert err <= SOLVE_TOL
    return F, d, sol


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
@pytest.mark.parametrize("trial", range(3))
@pytest.mark.parametrize("tag", ["di8", "di15", "seg6", "pm7", "quad2"])
def test_fleet_solve_vs_reference(dev, golden_dir, tag, trial, method):
    from time_opt_ilqr_amd import solver
    F, d, sol = _solve_fixture(dev, golden_dir, f"fleet_solve_{tag}_{trial}.npz", method)
    if tag == "seg6" and trial == 0 and method == "propagator":
        # the reference-named drop-ins on the solution
        T = int(sol["T_star"])
        args = (d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"], float(d["w"]))
        wrap = d["wrap_idx"].tolist()
        assert np.array_equal(solver.rollout(F, d["x0"], sol["U"]), sol["X"])
        J = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, wrap, system=F)
        assert abs(J - sol["J_hist"][-1]) <= TRAJ_TOL * abs(J)
        kw = dict(max_iter=int(d["max_iter"]), wrap_idx=wrap)
        sol2 = solver.ilqr_timeopt_ourmethod(F, d["x0"], *args, int(d["N"]), int(d["T_min"]),
                                             int(d["T_max"]), **kw)
        assert sol2["T_hist"] == sol["T_hist"] and sol2["J_hist"] == sol["J_hist"]
        sol3 = solver.ilqr_timeopt_baseline1(F, d["x0"], *args, int(d["N"]), int(d["T_min"]),
                                             int(d["T_max"]), **kw)
        assert list(sol3["T_hist"]) == d["T_hist_bruteforce"].tolist()


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
def test_fleet_batched_solve_equals_the_single_solves(dev, golden_dir, method):
    """the kept DI x 8 fixtures as one batch (B = 3): row by row the single solves"""
    from time_opt_ilqr_amd import solver, systems
    ds = [np.load(os.path.join(golden_dir, f"fleet_solve_di8_{t}.npz")) for t in range(3)]
    d = ds[0]
    assert len({float(x["w"]) for x in ds}) == 1 and all(np.array_equal(x["Q"], d["Q"]) for x in ds)
    F = systems.Fleet(0, 8)
    kw = dict(max_iter=int(d["max_iter"]), method=method, wrap_idx=[])
    res = solver.ilqr_timeopt_batch(F, np.stack([x["x0"] for x in ds]), d["xg"], d["u_ref"],
                                    d["Q"], d["R"], d["Qf"], float(d["w"]), int(d["N"]),
                                    int(d["T_min"]), int(d["T_max"]), stage_timers=False, **kw)
    assert _np(res["crashed"]).tolist() == [0] * 3
    nh = _np(res["n_hist"])
    worst = 0.0
    for b, x in enumerate(ds):
        one = solver.ilqr_timeopt(F, x["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                                  float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                                  **kw)
        assert _np(res["T_hist"][b, :nh[b]]).tolist() == list(one["T_hist"]), b
        assert list(one["T_hist"]) == x[f"T_hist_{method}"].tolist()
        worst = max(worst, _elem_rel(_np(res["J_hist"][b, :nh[b]]), np.asarray(one["J_hist"])),
                    _elem_rel(_np(res["J_hist"][b, :nh[b]]), x[f"J_hist_{method}"]))
    print(f"fleet batched solve {method}: J_hist relative error", worst)
    assert worst <= SOLVE_TOL


def test_fleet_of_one_is_the_builtin_system(dev):
    """DI x 1 gives the T_hist of the built-in DI on the same problem"""
    from time_opt_ilqr_amd import solver, systems
    F, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, wrap, _ = systems.make_fleet(
        0, 1, N=60, seed=7001, w_scale=100.0)
    assert (F.n, F.m, wrap) == (2, 1, [])
    D = systems.make_double_integrator(N=60)[0]
    for method in ("propagator", "bruteforce"):
        a = solver.ilqr_timeopt(F, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, method=method,
                                max_iter=6)
        b = solver.ilqr_timeopt(D, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, method=method,
                                max_iter=6)
        assert len(a["T_hist"]) >= 2 and list(a["T_hist"]) == list(b["T_hist"])
        assert _elem_rel(np.asarray(a["J_hist"]), np.asarray(b["J_hist"])) <= SOLVE_TOL
