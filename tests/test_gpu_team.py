"""GPU: teams, mixed fleets of the built-in systems as device systems (include/hop_team.h,
csrc/team.hip).

Yardsticks and bars:
* dynamics, rollout and the linearisation's diagonal blocks, a_res and Fx: the existing
  kernels (hop_dynamics_f64, hop_rollout_f64, hop_linearize_f64) run on each member's
  slice at the team's dt -- bitwise, no tolerance; every off-block entry of A and B
  exactly 0.0;
* the NaN pattern of a step with a NaN in the second member, the true cost and the line
  search: fixtures of the reference on the stacked callable
  (tests/golden/make_golden_team.py), J, X' and U' to TRAJ_TOL = 1e-9, accepted indices
  exact (the generator keeps only cases whose every candidate is 1e-6 clear of J_old);
* a team of equal members against the fleet of them: every output of all six entries
  bit for bit (NaNs included);
* member order: a permuted team's rollouts are the permuted rollouts bit for bit, its cost
  equal to 1e-12 relative (sums of at most 31 non-negative terms in another order);
* whole solves: T_hist equal, J_hist to SOLVE_TOL = 1e-6 against
  tests/golden/team_solve_*.npz (every select gap >= 1e-3, filtered by the generator).
Batch sizes 1, 5 and 67: none a multiple of 4 (rows per wave), 67 crosses a wave and a
workgroup.
"""
import functools
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TRAJ_TOL, SOLVE_TOL, ORDER_TOL = 1e-9, 1e-6, 1e-12
N = 12
BATCHES = (1, 5, 67)
# member ids, n, m, dt
SHAPES = {"all5": ((0, 1, 2, 3, 4), 26, 9, 0.02), "pm_quad_di": ((3, 2, 0), 18, 7, 0.05),
          "di2_pm2": ((0, 0, 3, 3), 12, 6, 0.05), "quad_pm3": ((2, 3, 3, 3), 24, 10, 0.05),
          "quad_di4_pm2": ((2, 0, 0, 0, 0, 3, 3), 28, 12, 0.05),
          "pm7_di": ((3,) * 7 + (0,), 30, 15, 0.05), "cp2_seg3": ((1, 1, 4, 4, 4), 20, 5, 0.02)}
TAGS = list(SHAPES)
SIZES = {0: (2, 1), 1: (4, 1), 2: (12, 4), 3: (4, 2), 4: (4, 1)}
# threads, bytes of the team Lds struct (Q, Qf, R and 16 exchange vectors): cost / line search
TEAM_LDS = (256, (2 * 31 * 31 + 16 * 16 + 16 * 32) * 8)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVES = sorted(f for f in os.listdir(GOLDEN) if re.fullmatch(r"team_solve_\w+_\d\.npz", f))


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


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _same_bits(a, b):
    """torch.equal on the bit patterns, so that NaNs compare too"""
    import torch
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


def _team(tag):
    from time_opt_ilqr_amd import systems
    ids, n, m, dt = SHAPES[tag]
    F = systems.Team(ids, dt=dt)
    assert (F.n, F.m) == (n, m)
    return F


@functools.lru_cache(maxsize=None)
def _case(tag, golden_dir):
    ids, n, m, dt = SHAPES[tag]
    d = np.load(os.path.join(golden_dir, f"team_cases_{tag}.npz"))
    c = case_inputs(int(d["seed"]), n, m, SIZES[ids[0]][0])
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum()])
    assert np.array_equal(got, d["check"]), "the inputs are not the generator's"
    return c, d


def _members(F, t):
    """(system id, member slice) of a tensor whose last axis is the stacked state or input"""
    on_x = t.shape[-1] == F.n
    offs = F.x_offsets if on_x else F.u_offsets
    return [(s, t[..., o:o + SIZES[s][0 if on_x else 1]].contiguous())
            for s, o in zip(F.member_ids, offs)]


def _cost(c, F, dev):
    from time_opt_ilqr_amd import engine
    return engine.CostParams(_t(c["xg"], dev), _t(c["u_ref"], dev), _t(c["Q"], dev),
                             _t(c["R"], dev), _t(c["Qf"], dev), c["w"], None, F.wrap_idx)


def _quiet(F):
    """a factor per input: the quadrotors' torques small enough that no member meets its
    pitch guard in N steps"""
    f = np.ones(F.m)
    for s, o in zip(F.member_ids, F.u_offsets):
        if s == 2:
            f[o:o + 4] = 0.05
    return f


# ---------------------------------------------------------------- 1. dynamics, rollout
@pytest.mark.parametrize("tag", TAGS)
def test_team_dynamics_is_the_members_kernel_bitwise(dev, tag):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    F = _team(tag)
    rng = np.random.default_rng(5 + F.n)
    for Bn in BATCHES:
        X = _t(rng.uniform(-1.0, 1.0, (Bn, F.n)), dev)
        U = _t(rng.uniform(-1.0, 1.0, (Bn, F.m)), dev)
        got = engine.dynamics(F, X, U, F.dt)
        ref = torch.cat([engine.dynamics(s, x, u, F.dt)
                         for (s, x), (_, u) in zip(_members(F, X), _members(F, U))], -1)
        assert torch.equal(got, ref), (tag, Bn)
        assert torch.equal(F.batch(X, U), got)
    # strided rows: only the n (m) leading entries of each row are read and written
    Xs = _t(rng.uniform(-1.0, 1.0, (5, F.n + 3)), dev)
    Us = _t(rng.uniform(-1.0, 1.0, (5, F.m + 2)), dev)
    out = torch.full((5, F.n + 1), -7.0, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().hop_team_dynamics_f64(
        _lib.C.byref(engine._team_params(F)), _lib.ptr(Xs), F.n + 3, _lib.ptr(Us), F.m + 2, 5,
        _lib.ptr(out), F.n + 1, _lib.stream_handle(dev)))
    ref = engine.dynamics(F, Xs[:, :F.n].contiguous(), Us[:, :F.m].contiguous(), F.dt)
    assert torch.equal(out[:, :F.n], ref) and bool((out[:, F.n] == -7.0).all())


@pytest.mark.parametrize("tag", TAGS)
def test_team_rollout_is_the_members_kernel_bitwise(dev, tag):
    import torch
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    rng = np.random.default_rng(17 + F.n)
    for Bn in BATCHES:
        x0 = _t(rng.uniform(-0.5, 0.5, (Bn, F.n)), dev)
        U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * _quiet(F), dev)
        got = engine.rollout(F, x0, U, F.dt)
        ref = torch.cat([engine.rollout(s, x, u, F.dt)
                         for (s, x), (_, u) in zip(_members(F, x0), _members(F, U))], -1)
        assert bool(torch.isfinite(ref).all()) and torch.equal(got, ref), (tag, Bn)
    # a shared x0 (batch stride 0)
    got = engine.rollout(F, x0[0], U, F.dt)
    assert torch.equal(got[:, 0], x0[:1].expand(Bn, F.n))
    assert torch.equal(got[0], engine.rollout(F, x0[:1], U[:1], F.dt)[0])
    # a NaN in one member (an input of the second, at step 4 of problem 3) makes every
    # member NaN from there on; the other problems run on
    Un = U.clone()
    Un[3, 4, F.u_offsets[1]] = float("nan")
    got = engine.rollout(F, x0, Un, F.dt)
    assert bool(torch.isnan(got[3, 5:]).all()) and torch.equal(got[3, :5], ref[3, :5])
    keep = [b for b in range(Bn) if b != 3]
    assert torch.equal(got[keep], ref[keep])


def test_team_rollout_stops_on_the_stacked_norm(dev):
    """DI, DI, point mass, point mass (no libm: the NumPy twin gives the same bits).  The
    first DI accelerates, the others sit at position 3; max_state_norm = 10 is crossed by
    the stacked norm while every member's own norm is below it.  The reference's rule
    (solver.py:42-62) on the stacked state, in NumPy: the first state that is not finite or
    has norm > max_state_norm and every state after it are NaN, for every member."""
    import torch
    from time_opt_ilqr_amd import engine
    F = _team("di2_pm2")
    dt, M, Bn = F.dt, 10.0, 5
    x0 = np.zeros((Bn, F.n))
    x0[:, [2, 4, 5, 8, 9]] = 3.0
    U = np.zeros((Bn, N, F.m))
    U[:, :, 0] = 15.0 + 3.0 * np.arange(Bn)[:, None]  # a different step per problem
    U[Bn - 1, :, 0] = 1.0                                # the last problem never trips
    ref = np.zeros((Bn, N + 1, F.n))
    ref[:, 0] = x0
    stop = []
    for b in range(Bn):
        for k in range(N):
            xn = F(ref[b, k], U[b, k])
            nrm = float(np.linalg.norm(xn))
            assert abs(nrm - M) > 1e-6  # the decision does not rest on the order of the sum
            if not np.all(np.isfinite(xn)) or nrm > M:
                ref[b, k + 1:] = np.nan
                # only the stacked norm trips: every member's own norm is below the bound
                assert max(np.linalg.norm(xn[o:o + SIZES[s][0]])
                           for s, o in zip(F.member_ids, F.x_offsets)) < M
                break
            ref[b, k + 1] = xn
        stop.append(int(np.isnan(ref[b, :, 0]).argmax()) if np.isnan(ref[b]).any() else -1)
    assert stop[-1] == -1 and all(2 <= s <= N for s in stop[:-1]) and len(set(stop)) >= 3, stop
    got = _np(engine.rollout(F, _t(x0, dev), _t(U, dev), dt, max_state_norm=M))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])
    # the member's own kernel with the same bound runs on
    mem = engine.rollout(0, _t(x0[:, :2], dev), _t(U[:, :, :1], dev), dt, max_state_norm=M)
    assert bool(torch.isfinite(mem[0, :stop[0] + 1]).all())


# ---------------------------------------------------------------- 2. linearisation
def _block_masks(F, dev):
    import torch
    mA = torch.zeros((F.n, F.n), dtype=torch.bool, device=dev)
    mB = torch.zeros((F.n, F.m), dtype=torch.bool, device=dev)
    for s, i, j in zip(F.member_ids, F.x_offsets, F.u_offsets):
        mA[i:i + SIZES[s][0], i:i + SIZES[s][0]] = True
        mB[i:i + SIZES[s][0], j:j + SIZES[s][1]] = True
    return mA, mB


@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("tag", TAGS)
def test_team_linearize_blocks_bitwise_and_zeros(dev, tag, central):
    import torch
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    rng = np.random.default_rng(23 + F.n)
    mA, mB = _block_masks(F, dev)
    for Bn in BATCHES:
        X = _t(rng.uniform(-1.0, 1.0, (Bn, N + 1, F.n)), dev)
        U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)), dev)
        r = engine.linearize(F, X, U, F.dt, central=central, want_fx=True)
        for t, mk in ((r.A, mA), (r.B, mB)):
            off = t[..., ~mk]
            assert bool((off == 0.0).all()) and not bool(torch.signbit(off).any()), (tag, Bn)
        for (s, x), (_, u), i, j in zip(_members(F, X), _members(F, U), F.x_offsets,
                                        F.u_offsets):
            ref = engine.linearize(s, x, u, F.dt, central=central, want_fx=True)
            sl, su = slice(i, i + SIZES[s][0]), slice(j, j + SIZES[s][1])
            assert torch.equal(r.A[..., sl, sl], ref.A) and torch.equal(r.B[..., sl, su], ref.B)
            assert torch.equal(r.a_res[..., sl], ref.a_res) and torch.equal(r.Fx[..., sl], ref.Fx)


@pytest.mark.parametrize("tag", TAGS)
def test_team_linearize_nan_pattern_and_tail(dev, golden_dir, tag):
    """the reference's NaN pattern for a NaN in the second member's state at one step
    (fixture), and steps k >= n_use left untouched (a_res and Fx nullable)"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    F = _team(tag)
    c, d = _case(tag, golden_dir)
    assert c["nan_at"][1] == F.x_offsets[1] + 1
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
        _lib.check(_lib.load().hop_team_linearize_f64(
            _lib.C.byref(engine._team_params(F)), _lib.ptr(X), _lib.ptr(U), Bn, N, n_use, 1, 1e-5,
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
def test_team_cost_true_vs_reference(dev, golden_dir, tag):
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    c, d = _case(tag, golden_dir)
    assert sorted(d["wrap_idx"].tolist()) == sorted(F.wrap_idx)
    cost = _cost(c, F, dev)
    worst = 0.0
    for Bn in BATCHES:
        J = _np(engine.cost_true(F, _t(c["X"][:Bn], dev), _t(c["U"][:Bn], dev), c["T"][:Bn], cost))
        worst = max(worst, _elem_rel(J, d["cost_J"][:Bn]))
    print(f"team cost_true {tag}: max rel err {worst:.2e}")
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
def test_team_forward_linesearch_vs_reference(dev, golden_dir, tag):
    """the reference's forward_linesearch_fixedT on the stacked callable; problem 2 runs
    inactive and is copied through"""
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    c, d = _case(tag, golden_dir)
    pick = d["ls_pick"]
    U, T = c["U0"][pick], c["T0"][pick]
    active = np.array([1, 1, 0, 1], dtype=np.int32)
    on = active != 0
    r = engine.forward_linesearch(F, _t(d["ls_X"], dev), _t(U, dev), T, _t(d["ls_K"], dev),
                                  _t(d["ls_k"], dev), _cost(c, F, dev), F.dt, active=active)
    got = _np(r.accepted)
    print(f"team line search {tag}: accepted {got.tolist()} reference {d['ls_acc'].tolist()}")
    assert got[on].tolist() == d["ls_acc"][on].tolist() and got[2] == -2
    eJ = _elem_rel(_np(r.J)[on], d["ls_J"][on])
    eJ0 = _elem_rel(_np(r.J_old), d["ls_J0"])
    eX = float(np.abs(_np(r.X)[on] - d["ls_Xo"][on]).max())
    eU = float(np.abs(_np(r.U)[on] - d["ls_Uo"][on]).max())
    print(f"team line search {tag}: J {eJ:.2e} J_old {eJ0:.2e} X' {eX:.2e} U' {eU:.2e}")
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL
    assert float(np.abs(d["ls_Xo"]).max()) < 50.0  # absolute and relative bars coincide
    assert np.array_equal(_np(r.X)[2], d["ls_X"][2]) and np.array_equal(_np(r.U)[2], U[2])
    assert _np(r.J)[2] == _np(r.J_old)[2]


def _linesearch_direct(dev, F, X, U, T, K, k, cost, active=None):
    """the line-search entry of a team or a fleet on a workspace of the caller's own:
    (X', U', J, J_old, accepted, the workspace, its size in bytes)"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, Nn = U.shape[:2]
    al = engine.ALPHAS
    ws_fn, par = engine._object_entry(F, "forward_workspace_bytes")
    fn = engine._object_entry(F, "forward_linesearch_f64")[0]
    cargs, keep = engine._chain_cost_args(cost, Bn, F.n, F.m, dev, F)
    nb = int(ws_fn(_lib.C.byref(par), Bn, Nn, len(al)))
    ws = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    Tt = _t(T, dev, torch.int32)
    act = None if active is None else _t(active, dev, torch.int32)
    out = [torch.empty_like(X), torch.empty_like(U)] + [
        torch.empty((Bn,), dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.empty((Bn,), dtype=torch.int32, device=dev)]
    _lib.check(fn(_lib.C.byref(par), _lib.ptr(X), _lib.ptr(U), *cargs, _lib.ptr(Tt),
                  _lib.ptr(act), _lib.ptr(K), _lib.ptr(k), (_lib.C.c_double * len(al))(*al),
                  len(al), Bn, Nn, _lib.ptr(ws), nb, *[_lib.ptr(o) for o in out],
                  _lib.stream_handle(dev)))
    torch.cuda.synchronize(dev)
    del keep
    return out + [ws, nb]


@pytest.mark.parametrize("tag", TAGS)
def test_team_linesearch_zero_gains_is_the_rollout(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    c, _ = _case(tag, golden_dir)
    Bn = 5
    rng = np.random.default_rng(41 + F.n)
    x0 = _t(rng.uniform(-1.0, 1.0, (Bn, F.n)), dev)
    U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * _quiet(F), dev)
    X = engine.rollout(F, x0, U, F.dt)
    assert bool(torch.isfinite(X).all())
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
    na = len(engine.ALPHAS)
    *_, ws, nb = _linesearch_direct(dev, F, X, U, T, K, k, cost)
    assert nb == Bn * na * (1 + (N + 1) * F.n + N * F.m) * 8
    Jc = ws[:Bn * na].reshape(Bn, na)
    assert torch.equal(Jc, r.J_old[:, None].expand(Bn, na))
    rows = ws[Bn * na:].reshape(Bn, na, -1)
    nx = (N + 1) * F.n
    assert torch.equal(rows[:, :, :nx], X.reshape(Bn, 1, nx).expand(Bn, na, nx))
    assert torch.equal(rows[:, :, nx:], U.reshape(Bn, 1, -1).expand(Bn, na, N * F.m))


# ---------------------------------------------------------------- 5. a team of equals
@pytest.mark.parametrize("ftag,sid,count", [("quad2", 2, 2), ("di15", 0, 15), ("cp5", 1, 5)])
def test_team_of_equal_members_is_the_fleet_bitwise(dev, golden_dir, ftag, sid, count):
    """contract (b): every output of all six entries, B = 67, on the fleet cases' inputs"""
    import torch
    from test_gpu_fleet import case_inputs as fleet_inputs
    from time_opt_ilqr_amd import _lib, engine, systems
    Fl, Tm = systems.Fleet(sid, count), systems.Team([sid] * count)
    assert (Tm.n, Tm.m, Tm.dt, Tm.wrap_idx) == (Fl.n, Fl.m, Fl.dt, Fl.wrap_idx)
    d = np.load(os.path.join(golden_dir, f"fleet_cases_{ftag}.npz"))
    c = fleet_inputs(int(d["seed"]), Fl.n, Fl.m, Fl.n_member)
    Bn = 67
    X, U = _t(c["X"], dev), _t(c["U"], dev)
    assert X.shape[0] == Bn
    both = lambda f: (f(Fl), f(Tm))  # noqa: E731
    a, b = both(lambda F: engine.dynamics(F, X[:, 0].contiguous(), U[:, 0].contiguous(), F.dt))
    assert _same_bits(a, b)
    x0 = (0.25 * X[:, 0]).contiguous()
    a, b = both(lambda F: engine.rollout(F, x0, U, F.dt))
    assert _same_bits(a, b) and bool(torch.isfinite(a[:, 1]).any())
    Xr = a
    # a bound that about half of the problems cross on their way (the stacked norm)
    M = float(torch.nanmedian(torch.linalg.norm(Xr[:, N // 2], dim=-1)))
    a, b = both(lambda F: engine.rollout(F, x0, U, F.dt, max_state_norm=M))
    assert _same_bits(a, b)
    assert len(set(_np(torch.isnan(a[:, :, 0]).sum(1)).tolist())) >= 3  # stops at several steps
    for central in (False, True):
        for Xl in (X, Xr):  # the second may hold NaN rows: the NaN rules
            a, b = both(lambda F: engine.linearize(F, Xl, U, F.dt, central=central, want_fx=True))
            for key in ("A", "B", "a_res", "Fx"):
                assert _same_bits(getattr(a, key), getattr(b, key)), (ftag, central, key)
    cost = both(lambda F: _cost(c, F, dev))
    T = c["T"].copy()
    T[:3] = (0, N + 1, N)
    a, b = (engine.cost_true(F, X, U, T, cs) for F, cs in zip((Fl, Tm), cost))
    assert _same_bits(a, b) and bool(torch.isfinite(a[3:]).all())
    # the line search: small gains on rollouts from near the goal; every output and the
    # whole workspace (the candidates' J, X' and U')
    rng = np.random.default_rng(77 + Fl.n)
    x0 = _t(c["xg"] + rng.uniform(-0.4, 0.4, (Bn, Fl.n)), dev)
    U0 = _t(c["u_ref"] + 0.3 * rng.uniform(-1.0, 1.0, (Bn, N, Fl.m)), dev)
    X0 = engine.rollout(Fl, x0, U0, Fl.dt)
    assert bool(torch.isfinite(X0).all())
    K = _t(0.05 * rng.standard_normal((Bn, N, Fl.m, Fl.n)), dev)
    # k pulls the inputs towards u_ref, by a factor that overshoots in some problems
    fac = np.array([0.5, 4.0, 8.0, 16.0])[np.arange(Bn) % 4]
    k = _t(-fac[:, None, None] * (_np(U0) - c["u_ref"]), dev)
    active = (np.arange(Bn) % 7 != 3).astype(np.int32)
    a, b = (_linesearch_direct(dev, F, X0, U0, c["T"], K, k, cs, active)
            for F, cs in zip((Fl, Tm), cost))
    assert a[-1] == b[-1] > 0
    for i, key in enumerate(("X", "U", "J", "J_old", "accepted", "workspace")):
        assert _same_bits(a[i], b[i]), (ftag, key)
    acc = _np(a[4])
    assert (acc[active == 0] == -2).all() and (acc[active != 0] >= -1).all()
    assert len(set(acc.tolist())) >= 3  # accepted at different step sizes, not one path
    lib = _lib.load()
    for args in ((Bn, N, 5), (1, 0, 1), (4, 10, 8)):
        assert lib.hop_team_forward_workspace_bytes(_lib.C.byref(engine._team_params(Tm)), *args) \
            == lib.hop_fleet_forward_workspace_bytes(_lib.C.byref(engine._fleet_params(Fl)), *args)


# ---------------------------------------------------------------- 6. member order
def test_team_member_order(dev, golden_dir):
    """pm_quad_di and its permutation (DI, point mass, quadrotor) with every datum permuted
    to match: the rollouts are the permuted rollouts bit for bit; the cost sums at most 31
    non-negative terms in another order, so it agrees to 1e-12 relative"""
    import torch
    from time_opt_ilqr_amd import engine, systems
    F = _team("pm_quad_di")
    G = systems.Team([0, 3, 2])
    c, d = _case("pm_quad_di", golden_dir)
    order = [2, 0, 1]  # G's members as members of F
    ix = np.concatenate([np.arange(F.x_offsets[a], F.x_offsets[a] + SIZES[F.member_ids[a]][0])
                         for a in order])
    iu = np.concatenate([np.arange(F.u_offsets[a], F.u_offsets[a] + SIZES[F.member_ids[a]][1])
                         for a in order])
    assert [F.member_ids[a] for a in order] == list(G.member_ids)
    assert sorted(ix.tolist().index(i) for i in F.wrap_idx) == sorted(G.wrap_idx)
    cg = dict(c, xg=c["xg"][ix], u_ref=c["u_ref"][iu], Q=c["Q"][np.ix_(ix, ix)],
              Qf=c["Qf"][np.ix_(ix, ix)], R=c["R"][np.ix_(iu, iu)])
    Bn = 67
    T = c["T"].copy()
    X, U = _t(c["X"], dev), _t(c["U"], dev)
    Jf = _np(engine.cost_true(F, X, U, T, _cost(c, F, dev)))
    Jg = _np(engine.cost_true(G, _t(c["X"][..., ix], dev), _t(c["U"][..., iu], dev), T,
                              _cost(cg, G, dev)))
    err = _elem_rel(Jg, Jf)
    print(f"team member order: cost relative difference {err:.2e}")
    assert np.isfinite(Jf).all() and err <= ORDER_TOL
    rng = np.random.default_rng(91)
    x0 = rng.uniform(-0.5, 0.5, (Bn, F.n))
    Ur = rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * _quiet(F)
    Xf = engine.rollout(F, _t(x0, dev), _t(Ur, dev), F.dt)
    Xg = engine.rollout(G, _t(x0[:, ix], dev), _t(Ur[..., iu], dev), G.dt)
    assert bool(torch.isfinite(Xf).all()) and torch.equal(Xg, Xf[..., _t(ix, dev, torch.int64)])
    # a tight bound: both stop at the same step (the stacked norm is one sum either way
    # only up to rounding, so the bound sits clear of every norm along the way)
    nrm = torch.linalg.norm(Xf, dim=-1)
    M = float(nrm.max()) * 0.8
    assert float((nrm - M).abs().min()) > 1e-9
    Xf = engine.rollout(F, _t(x0, dev), _t(Ur, dev), F.dt, max_state_norm=M)
    Xg = engine.rollout(G, _t(x0[:, ix], dev), _t(Ur[..., iu], dev), G.dt, max_state_norm=M)
    assert bool(torch.isnan(Xf).any()) and _same_bits(Xg, Xf[..., _t(ix, dev, torch.int64)])


# ---------------------------------------------------------------- 7. LDS
@pytest.mark.parametrize("tag", ["all5", "quad_di4_pm2", "pm7_di"])
def test_team_kernels_on_poisoned_lds(dev, golden_dir, tag):
    """the cost and line-search kernels stage Q, Qf, R and a vector per row in LDS: the
    same bits after each of the three fill patterns"""
    from test_gpu_lds_poison import run_poisoned
    from time_opt_ilqr_amd import engine
    F = _team(tag)
    c, d = _case(tag, golden_dir)
    cost = _cost(c, F, dev)
    pick = d["ls_pick"]
    Xc, Uc, Tc = _t(c["X"][:5], dev), _t(c["U"][:5], dev), c["T"][:5]
    Xl, Ul, Kl, kl = (_t(a, dev) for a in (d["ls_X"], c["U0"][pick], d["ls_K"], d["ls_k"]))

    def fn():
        r = engine.forward_linesearch(F, Xl, Ul, c["T0"][pick], Kl, kl, cost, F.dt)
        return dict(Jc=engine.cost_true(F, Xc, Uc, Tc, cost), J=r.J, J_old=r.J_old, X=r.X, U=r.U,
                    accepted=r.accepted)

    base = run_poisoned(dev, fn, TEAM_LDS, 2)
    assert _elem_rel(_np(base["Jc"]), d["cost_J"][:5]) <= TRAJ_TOL
    assert _np(base["accepted"]).tolist() == d["ls_acc"].tolist()
    assert _elem_rel(_np(base["J_old"]), d["ls_J0"]) <= TRAJ_TOL


# ---------------------------------------------------------------- 8. whole solves
def _solve_fixture(dev, golden_dir, name, method):
    from time_opt_ilqr_amd import solver, systems
    d = np.load(os.path.join(golden_dir, name))
    assert float(d[f"gaps_{method}"].min()) >= 1e-3
    F = systems.Team(d["members"].tolist(), dt=float(d["dt"]))
    sol = solver.ilqr_timeopt(F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method=method, max_iter=int(d["max_iter"]),
                              wrap_idx=d["wrap_idx"].tolist())
    assert list(sol["T_hist"]) == d[f"T_hist_{method}"].tolist(), (name, sol["T_hist"])
    err = _elem_rel(np.asarray(sol["J_hist"]), d[f"J_hist_{method}"])
    print(name, method, "J_hist relative error", err)
    assert err <= SOLVE_TOL
    return F, d, sol


def test_team_solve_fixtures_are_there():
    tags = {n[len("team_solve_"):-6] for n in SOLVES}
    assert {"di2_pm2", "quad_pm3", "quad_di4_pm2"} <= tags <= set(SHAPES)


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
@pytest.mark.parametrize("name", SOLVES)
def test_team_solve_vs_reference(dev, golden_dir, name, method):
    from time_opt_ilqr_amd import solver
    F, d, sol = _solve_fixture(dev, golden_dir, name, method)
    if name == "team_solve_quad_pm3_0.npz" and method == "propagator":
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
        from time_opt_ilqr_amd import linearization
        A, B = linearization.linearize_central_diff_traj(F, sol["X"][:4], sol["U"][:3])
        assert np.asarray(A).shape == (3, F.n, F.n) and np.asarray(B).shape == (3, F.n, F.m)
        assert np.asarray(A)[0][0, F.x_offsets[1]] == 0.0


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
def test_team_batched_solve_equals_the_single_solves(dev, golden_dir, method):
    """the kept di2_pm2 fixtures as one batch (B = 3): row by row the single solves"""
    from time_opt_ilqr_amd import solver, systems
    ds = [np.load(os.path.join(golden_dir, f"team_solve_di2_pm2_{t}.npz")) for t in range(3)]
    d = ds[0]
    assert len({float(x["w"]) for x in ds}) == 1 and all(np.array_equal(x["Q"], d["Q"]) for x in ds)
    assert len({int(x["T_min"]) for x in ds}) == 1
    F = systems.Team(d["members"].tolist(), dt=float(d["dt"]))
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
    print(f"team batched solve {method}: J_hist relative error", worst)
    assert worst <= SOLVE_TOL


def test_team_of_one_is_the_builtin_system(dev):
    """a team of one DI gives the T_hist of the built-in DI on the same problem"""
    from time_opt_ilqr_amd import solver, systems
    F, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, wrap, _ = systems.make_team(
        [0], N=60, seed=7001, w_scale=100.0)
    assert (F.n, F.m, wrap) == (2, 1, [])
    D = systems.make_double_integrator(N=60)[0]
    for method in ("propagator", "bruteforce"):
        a = solver.ilqr_timeopt(F, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, method=method,
                                max_iter=6)
        b = solver.ilqr_timeopt(D, x0, xg, ur, Q, R, Qf, w, Nn, T_min, T_max, method=method,
                                max_iter=6)
        assert len(a["T_hist"]) >= 2 and list(a["T_hist"]) == list(b["T_hist"])
        assert _elem_rel(np.asarray(a["J_hist"]), np.asarray(b["J_hist"])) <= SOLVE_TOL
