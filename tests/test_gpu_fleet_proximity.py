"""GPU: the fleets' proximity cost (include/hop_fleet_proximity.h, csrc/fleet_proximity.hpp).

Yardsticks and bars:
* the Taylor kernel, the true cost and the line search: fixtures of the reference with the
  NumPy bump cost as extra_stage_cost (tests/golden/make_golden_fleet_proximity.py), to
  the project's trajectory tolerance TRAJ_TOL = 1e-9, accepted indices exact (the generator
  keeps only cases whose every candidate is 1e-6 clear of J_old); entries off the position
  blocks exactly +0.0 and cxx symmetric bit for bit;
* a cost with no term: c exactly 0, and the proximity entries equal the plain hop_fleet_*
  entries bit for bit;
* plain cost_true + the Taylor kernel's c summed over k < T against the proximity
  cost_true: 1e-12 (two summation orders of at most 13 fp64 terms of one sign);
* whole solves: T_hist equal, J_hist to the fleet test's SOLVE_TOL = 1e-6 against
  tests/golden/fleet_prox_solve_*.npz (every select gap >= 1e-3, filtered by the generator).
Shapes: N = 12, batches 1, 5 and 67 (none a multiple of 4 rows per wave; 67 crosses a wave
and a workgroup).
"""
import functools
import os

import numpy as np
import pytest

from test_gpu_fleet import case_inputs

pytestmark = pytest.mark.gpu
TRAJ_TOL, SOLVE_TOL, SUM_TOL = 1e-9, 1e-6, 1e-12
N = 12
BATCHES = (1, 5, 67)
# base system id, count, n, m, pd
SHAPES = {"pm3": (3, 3, 12, 6, 2), "pm4": (3, 4, 16, 8, 2), "pm7": (3, 7, 28, 14, 2),
          "quad2": (2, 2, 24, 8, 3), "di15": (0, 15, 30, 15, 1)}
TAGS = list(SHAPES)
SOLVE_TAGS = ["pm3", "pm4", "pm7", "quad2", "di15"]
# threads, static LDS bytes: the cost / line-search kernels, the Taylor kernel
PROX_LDS = (256, (2 * 31 * 31 + 16 * 16 + 16 * 32 + 16 * 5) * 8)
TAYLOR_LDS = (256, (16 * 5 + 16 * (48 + 120 + 144)) * 8)


# BEGIN prox_inputs (repeated verbatim in tests/test_gpu_fleet_proximity.py)
def prox_inputs(seed, c, count, n_member, pd):
    """the cost of the kernel-level cases: four obstacle rows (one of weight 0, which must
    contribute nothing) and a separation pair; the position entries of the cost
    trajectories c["X"] are redrawn in place so that pairs and obstacles lie within two
    radii"""
    rng = np.random.default_rng(seed + 50000)
    obs = np.concatenate([rng.uniform(-0.6, 0.6, (4, pd)), rng.uniform(0.3, 0.6, (4, 1)),
                          rng.uniform(0.5, 2.0, (4, 1))], axis=1)
    obs[2, pd + 1] = 0.0
    sep = (0.45, 1.3)
    for a in range(count):
        sl = slice(a * n_member, a * n_member + pd)
        c["X"][..., sl] = rng.uniform(-0.8, 0.8, c["X"][..., sl].shape)
    return obs, sep
# END prox_inputs


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _elem_rel(got, ref):
    """max elementwise relative error; where the reference is 0 the result must be 0"""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    zero = ref == 0.0
    assert np.array_equal(got[zero], ref[zero]), "a nonzero where the reference has an exact 0"
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int64)


@functools.lru_cache(maxsize=None)
def _case(tag, golden_dir):
    """(inputs, fixture, fleet with the cost, the same fleet without): computed once"""
    from time_opt_ilqr_amd import systems
    sid, count, n, m, pd = SHAPES[tag]
    d = np.load(os.path.join(golden_dir, f"fleet_prox_cases_{tag}.npz"))
    c = case_inputs(int(d["seed"]), n, m, n // count)
    obs, sep = prox_inputs(int(d["seed"]), c, count, n // count, pd)
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum(), obs.sum()])
    assert np.array_equal(got, d["check"]), "the inputs are not the generator's"
    F = systems.Fleet(sid, count, proximity=systems.Proximity(obs, sep))
    assert (F.n, F.m, F.pos_dim) == (n, m, pd)
    assert sorted(d["wrap_idx"].tolist()) == sorted(F.wrap_idx)
    return c, d, F, systems.Fleet(sid, count)


def _cost(c, F, dev):
    from time_opt_ilqr_amd import engine
    return engine.CostParams(_t(c["xg"], dev), _t(c["u_ref"], dev), _t(c["Q"], dev),
                             _t(c["R"], dev), _t(c["Qf"], dev), c["w"], None, F.wrap_idx)


def _null(F):
    """F with a cost that has no term"""
    from time_opt_ilqr_amd import systems
    return systems.Fleet(F.base_id, F.count, proximity=systems.Proximity())


# ---------------------------------------------------------------- 1. the Taylor kernel
@pytest.mark.parametrize("tag", TAGS)
def test_taylor_kernel_vs_reference(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    c, d, F, _ = _case(tag, golden_dir)
    n = F.n
    X = _t(c["X"][:, 0], dev)
    pos = torch.zeros(n, dtype=torch.bool, device=dev)
    pos[F.position_idx] = True
    worst = 0.0
    for Bn in BATCHES:
        cc, cx, cxx = engine.fleet_proximity_cost(F, X[:Bn])
        worst = max(worst, _elem_rel(_np(cc), d["tay_c"][:Bn]), _elem_rel(_np(cx), d["tay_cx"][:Bn]),
                    _elem_rel(_np(cxx), d["tay_cxx"][:Bn]))
        # off the position blocks: exactly +0.0
        for off in (cx[:, ~pos], cxx[:, ~pos, :], cxx[:, :, ~pos]):
            assert bool((_bits(off) == 0).all()), (tag, Bn)
        assert torch.equal(_bits(cxx), _bits(cxx.transpose(1, 2))), (tag, Bn)
    print(f"fleet proximity taylor {tag}: max elementwise rel err {worst:.2e}")
    assert worst <= TRAJ_TOL
    assert float(d["tay_c"].max()) >= 0.1 * max(float(d["prox_obs"][:, -1].max()),
                                                float(d["prox_sep"][1]))
    # nullable outputs: each alone is the full call's
    for want in (("c",), ("cx",), ("cxx",), ("c", "cxx")):
        part = engine.fleet_proximity_cost(F, X, want=want)
        for name, g, r in zip(("c", "cx", "cxx"), part, (cc, cx, cxx)):
            assert (g is None) == (name not in want)
            assert g is None or torch.equal(_bits(g), _bits(r))
    # a leading shape, and strided rows: only the n leading entries of a row are read
    lead = engine.fleet_proximity_cost(F, X[:66].reshape(6, 11, n))
    assert lead[2].shape == (6, 11, n, n) and torch.equal(lead[2].reshape(66, n, n), cxx[:66])
    Xs = torch.full((5, n + 3), 1e300, dtype=torch.float64, device=dev)
    Xs[:, :n] = X[:5]
    out = [torch.full(s, -7.0, dtype=torch.float64, device=dev) for s in ((5,), (5, n), (5, n, n))]
    px, tab = engine._proximity_struct(F, dev)
    _lib.check(_lib.load().hop_fleet_proximity_taylor_f64(
        _lib.C.byref(engine._fleet_params(F)), _lib.C.byref(px), _lib.ptr(Xs), n + 3, 5,
        *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
    for g, r in zip(out, (cc, cx, cxx)):
        assert torch.equal(_bits(g), _bits(r[:5]))


# ---------------------------------------------------------------- 2. null costs
def _ls_equal(a, b):
    import torch
    return all(torch.equal(_bits(getattr(a, f)), _bits(getattr(b, f))) if f != "accepted" else
               torch.equal(a.accepted, b.accepted) for f in ("X", "U", "J", "J_old", "accepted"))


@pytest.mark.parametrize("tag", TAGS)
def test_null_cost_is_the_plain_fleet_bitwise(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine
    c, d, F, plain = _case(tag, golden_dir)
    Z = _null(F)
    cc, cx, cxx = engine.fleet_proximity_cost(Z, _t(c["X"][:, 0], dev))
    for t in (cc, cx, cxx):
        assert bool((_bits(t) == 0).all())  # exactly +0.0
    cost = _cost(c, F, dev)
    X, U, T = _t(c["X"], dev), _t(c["U"], dev), c["T"]
    Jp = engine.cost_true(plain, X, U, T, cost)
    assert torch.equal(_bits(engine.cost_true(Z, X, U, T, cost)), _bits(Jp))
    assert not torch.equal(engine.cost_true(F, X, U, T, cost), Jp)  # the cost itself is seen
    pick = d["ls_pick"]
    args = (_t(d["ls_X"], dev), _t(c["U0"][pick], dev), c["T0"][pick], _t(d["ls_K"], dev),
            _t(d["ls_k"], dev), cost)
    assert _ls_equal(engine.forward_linesearch(Z, *args, F.dt),
                     engine.forward_linesearch(plain, *args, F.dt))


def test_fleet_of_one_with_separation_only_is_the_plain_fleet(dev):
    import torch
    from time_opt_ilqr_amd import engine, systems
    plain = systems.Fleet("pointmass", 1)
    one = systems.Fleet("pointmass", 1, proximity=systems.Proximity(separation=(0.4, 2.0)))
    n, m, Bn = 4, 2, 5
    c = case_inputs(77, n, m, n, N, Bn, 12)
    cost = _cost(c, plain, dev)
    cc = engine.fleet_proximity_cost(one, _t(c["X"][:, 0], dev))[0]
    assert bool((_bits(cc) == 0).all())
    x0, U = _t(c["x0"][:Bn], dev), _t(c["U0"][:Bn], dev)
    X = engine.rollout(plain, x0, U, plain.dt)
    T = c["T0"][:Bn]
    assert torch.equal(_bits(engine.cost_true(one, X, U, T, cost)),
                       _bits(engine.cost_true(plain, X, U, T, cost)))
    rng = np.random.default_rng(3)
    K = _t(0.05 * rng.standard_normal((Bn, N, m, n)), dev)
    k = _t(0.05 * rng.standard_normal((Bn, N, m)), dev)
    a = engine.forward_linesearch(one, X, U, T, K, k, cost, plain.dt)
    b = engine.forward_linesearch(plain, X, U, T, K, k, cost, plain.dt)
    assert _ls_equal(a, b)


# ---------------------------------------------------------------- 3, 4. the true cost
@pytest.mark.parametrize("tag", TAGS)
def test_prox_cost_true_vs_reference_and_taylor_sum(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine
    c, d, F, plain = _case(tag, golden_dir)
    cost = _cost(c, F, dev)
    worst = 0.0
    for Bn in BATCHES:
        J = engine.cost_true(F, _t(c["X"][:Bn], dev), _t(c["U"][:Bn], dev), c["T"][:Bn], cost)
        worst = max(worst, _elem_rel(_np(J), d["cost_J"][:Bn]))
    print(f"fleet proximity cost_true {tag}: max rel err {worst:.2e}")
    assert worst <= TRAJ_TOL
    # consistency: plain cost + sum_{k < T} c_k from the Taylor kernel
    X, U = _t(c["X"], dev), _t(c["U"], dev)
    T = _t(c["T"], dev, torch.int32)
    ck = engine.fleet_proximity_cost(F, X[:, :N], want=("c",))[0]
    mask = torch.arange(N, device=dev)[None, :] < T[:, None]
    total = engine.cost_true(plain, X, U, c["T"], cost) + (ck * mask).sum(1)
    err = _elem_rel(_np(J), _np(total))
    print(f"fleet proximity cost_true {tag}: against plain + sum of c_k {err:.2e}; the cost is "
          f"{float(((ck * mask).sum(1) / J).median()):.1%} of J (median)")
    assert err <= SUM_TOL
    # T = 0 -> +inf, T > N -> NaN, a NaN on the rows read -> +inf, beyond them: not read
    Xb = c["X"][:5].copy()
    Xb[2, 3, 0] = np.nan
    Xb[3, 9, 0] = np.nan
    Tb = np.array([0, N + 1, 7, 4, N], dtype=np.int32)
    Jb = _np(engine.cost_true(F, _t(Xb, dev), _t(c["U"][:5], dev), Tb, cost))
    assert Jb[0] == np.inf and np.isnan(Jb[1]) and Jb[2] == np.inf and np.isfinite(Jb[3:]).all()


# ---------------------------------------------------------------- 5. line search
@pytest.mark.parametrize("tag", TAGS)
def test_prox_forward_linesearch_vs_reference(dev, golden_dir, tag):
    """the reference's forward_linesearch_fixedT with the bump cost; problem 2 runs inactive"""
    from time_opt_ilqr_amd import engine
    c, d, F, plain = _case(tag, golden_dir)
    pick = d["ls_pick"]
    U, T = c["U0"][pick], c["T0"][pick]
    active = np.array([1, 1, 0, 1], dtype=np.int32)
    on = active != 0
    r = engine.forward_linesearch(F, _t(d["ls_X"], dev), _t(U, dev), T, _t(d["ls_K"], dev),
                                  _t(d["ls_k"], dev), _cost(c, F, dev), F.dt, active=active)
    got = _np(r.accepted)
    print(f"fleet proximity line search {tag}: accepted {got.tolist()} reference "
          f"{d['ls_acc'].tolist()}; the cost is {np.round(d['ls_extra0'] / d['ls_J0'], 3).tolist()} "
          "of J_old")
    assert got[on].tolist() == d["ls_acc"][on].tolist() and got[2] == -2
    assert (got[on] >= 0).all() and len(set(got[on].tolist())) >= 2
    eJ = _elem_rel(_np(r.J)[on], d["ls_J"][on])
    eJ0 = _elem_rel(_np(r.J_old), d["ls_J0"])
    eX = float(np.abs(_np(r.X)[on] - d["ls_Xo"][on]).max())
    eU = float(np.abs(_np(r.U)[on] - d["ls_Uo"][on]).max())
    print(f"fleet proximity line search {tag}: J {eJ:.2e} J_old {eJ0:.2e} X' {eX:.2e} U' {eU:.2e}")
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL
    assert float(np.abs(d["ls_Xo"]).max()) < 50.0  # absolute and relative bars coincide
    assert np.array_equal(_np(r.X)[2], d["ls_X"][2]) and np.array_equal(_np(r.U)[2], U[2])
    assert _np(r.J)[2] == _np(r.J_old)[2]
    # the cost is in J_old: the plain fleet's differs by the fixture's share
    J0p = _np(engine.forward_linesearch(plain, _t(d["ls_X"], dev), _t(U, dev), T,
                                        _t(d["ls_K"], dev), _t(d["ls_k"], dev),
                                        _cost(c, F, dev), F.dt).J_old)
    assert _elem_rel(d["ls_J0"] - J0p, d["ls_extra0"]) <= 1e-6


@pytest.mark.parametrize("tag", TAGS)
def test_prox_linesearch_zero_gains_is_the_rollout(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    c, _, F, plain = _case(tag, golden_dir)
    Bn = 5
    rng = np.random.default_rng(41 + F.n)
    x0 = _t(rng.uniform(-0.8, 0.8, (Bn, F.n)), dev)
    U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * (0.05 if F.base_id == 2 else 1.0), dev)
    X = engine.rollout(F, x0, U, F.dt)
    assert torch.equal(X, engine.rollout(plain, x0, U, F.dt)) and bool(torch.isfinite(X).all())
    cost = _cost(c, F, dev)
    K = torch.zeros((Bn, N, F.m, F.n), dtype=torch.float64, device=dev)
    k = torch.zeros((Bn, N, F.m), dtype=torch.float64, device=dev)
    T = np.array([1, 4, 7, N, 9], dtype=np.int32)
    r = engine.forward_linesearch(F, X, U, T, K, k, cost, F.dt)
    assert _np(r.accepted).tolist() == [-1] * Bn
    assert torch.equal(r.J, r.J_old) and torch.equal(r.X, X) and torch.equal(r.U, U)
    assert torch.equal(engine.cost_true(F, X, U, T, cost), r.J_old)
    assert not torch.equal(engine.cost_true(plain, X, U, T, cost), r.J_old)
    # the candidates themselves, from a workspace of the test's own: every (problem,
    # alpha) row is the rollout and its J is J_old, bit for bit
    lib, al = _lib.load(), engine.ALPHAS
    fp = engine._fleet_params(F)
    px, tab = engine._proximity_struct(F, dev)
    cargs, keep = engine._chain_cost_args(cost, Bn, F.n, F.m, dev, F)
    nb = int(lib.hop_fleet_forward_workspace_bytes(_lib.C.byref(fp), Bn, N, len(al)))
    ws = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    Tt = _t(T, dev, torch.int32)
    out = [torch.empty_like(X), torch.empty_like(U)] + [
        torch.empty((Bn,), dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.empty((Bn,), dtype=torch.int32, device=dev)]
    _lib.check(lib.hop_fleet_prox_forward_linesearch_f64(
        _lib.C.byref(fp), _lib.ptr(X), _lib.ptr(U), *cargs, _lib.C.byref(px), _lib.ptr(Tt), None,
        _lib.ptr(K), _lib.ptr(k), (_lib.C.c_double * len(al))(*al), len(al), Bn, N, _lib.ptr(ws),
        nb, *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
    torch.cuda.synchronize(dev)
    Jc = ws[:Bn * len(al)].reshape(Bn, len(al))
    assert torch.equal(Jc, r.J_old[:, None].expand(Bn, len(al)))
    rows = ws[Bn * len(al):].reshape(Bn, len(al), -1)
    nx = (N + 1) * F.n
    assert torch.equal(rows[:, :, :nx], X.reshape(Bn, 1, nx).expand(Bn, len(al), nx))
    assert torch.equal(rows[:, :, nx:], U.reshape(Bn, 1, -1).expand(Bn, len(al), N * F.m))


# ---------------------------------------------------------------- 6. LDS
@pytest.mark.parametrize("tag", ["di15", "quad2"])
def test_prox_kernels_on_poisoned_lds(dev, golden_dir, tag):
    """the cost and line-search kernels stage Q, Qf, R, the table and a vector per row in
    LDS, the Taylor kernel the table, positions, pair coefficients and diagonal blocks: the
    same bits after each of the three fill patterns"""
    from test_gpu_lds_poison import run_poisoned
    from time_opt_ilqr_amd import engine
    c, d, F, _ = _case(tag, golden_dir)
    cost = _cost(c, F, dev)
    pick = d["ls_pick"]
    Xc, Uc, Tc = _t(c["X"][:5], dev), _t(c["U"][:5], dev), c["T"][:5]
    Xl, Ul, Kl, kl = (_t(a, dev) for a in (d["ls_X"], c["U0"][pick], d["ls_K"], d["ls_k"]))
    Xt = _t(c["X"][:21, 0], dev)

    def fn():
        r = engine.forward_linesearch(F, Xl, Ul, c["T0"][pick], Kl, kl, cost, F.dt)
        return dict(Jc=engine.cost_true(F, Xc, Uc, Tc, cost), J=r.J, J_old=r.J_old, X=r.X, U=r.U,
                    accepted=r.accepted)

    def taylor():
        cc, cx, cxx = engine.fleet_proximity_cost(F, Xt)
        return dict(c=cc, cx=cx, cxx=cxx)

    base = run_poisoned(dev, fn, PROX_LDS, 2)
    assert _elem_rel(_np(base["Jc"]), d["cost_J"][:5]) <= TRAJ_TOL
    assert _np(base["accepted"]).tolist() == d["ls_acc"].tolist()
    base = run_poisoned(dev, taylor, TAYLOR_LDS, 2)
    assert _elem_rel(_np(base["cxx"]), d["tay_cxx"][:21]) <= TRAJ_TOL


# ---------------------------------------------------------------- 7. whole solves
def _fixture_fleet(d):
    from time_opt_ilqr_amd import systems
    return systems.Fleet(int(d["sid"]), int(d["count"]),
                         proximity=systems.Proximity(d["prox_obs"], tuple(d["prox_sep"])))


def _solve_fixture(golden_dir, name, method):
    from time_opt_ilqr_amd import solver
    d = np.load(os.path.join(golden_dir, name))
    assert float(d[f"gaps_{method}"].min()) >= 1e-3
    F = _fixture_fleet(d)
    sol = solver.ilqr_timeopt(F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method=method, max_iter=int(d["max_iter"]),
                              wrap_idx=d["wrap_idx"].tolist())
    assert list(sol["T_hist"]) == d[f"T_hist_{method}"].tolist(), (name, sol["T_hist"])
    err = _elem_rel(np.asarray(sol["J_hist"]), d[f"J_hist_{method}"])
    print(name, method, "J_hist relative error", err, "the cost's share of J",
          float(d[f"extra_share_{method}"]))
    assert err <= SOLVE_TOL
    return F, d, sol


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
@pytest.mark.parametrize("trial", range(3))
@pytest.mark.parametrize("tag", SOLVE_TAGS)
def test_prox_solve_vs_reference(dev, golden_dir, tag, trial, method):
    from time_opt_ilqr_amd import solver
    F, d, sol = _solve_fixture(golden_dir, f"fleet_prox_solve_{tag}_{trial}.npz", method)
    if tag == "pm3" and trial == 0 and method == "propagator":
        # the reference-named drop-ins on the solution
        T = int(sol["T_star"])
        args = (d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"], float(d["w"]))
        wrap = d["wrap_idx"].tolist()
        J = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, wrap, system=F)
        assert abs(J - sol["J_hist"][-1]) <= TRAJ_TOL * abs(J)
        stage = F.stage_cost()
        extra = sum(stage(sol["X"][k])[0] for k in range(T))
        Jp = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, wrap,
                                      system=type(F)(F.base_id, F.count))
        assert abs((J - Jp) - extra) <= 1e-9 * abs(J) and extra > 0.0
        kw = dict(max_iter=int(d["max_iter"]), wrap_idx=wrap)
        sol2 = solver.ilqr_timeopt_ourmethod(F, d["x0"], *args, int(d["N"]), int(d["T_min"]),
                                             int(d["T_max"]), **kw)
        assert sol2["T_hist"] == sol["T_hist"] and sol2["J_hist"] == sol["J_hist"]
        sol3 = solver.ilqr_timeopt_baseline1(F, d["x0"], *args, int(d["N"]), int(d["T_min"]),
                                             int(d["T_max"]), **kw)
        assert list(sol3["T_hist"]) == d["T_hist_bruteforce"].tolist()
        # forward_linesearch_fixedT with zero gains: nothing accepted, J = J_old with the cost
        Nn, n, m = len(sol["U"]), F.n, F.m
        Xo, Uo, Jl, acc = solver.forward_linesearch_fixedT(
            F, sol["X"], sol["U"], *args, T, [np.zeros(m)] * T, [np.zeros((m, n))] * T,
            wrap_idx=wrap)
        assert not acc and abs(Jl - J) <= TRAJ_TOL * abs(J)


# ---------------------------------------------------------------- 8. the host path
def test_prox_host_path_selects_the_same_horizons(dev, golden_dir):
    """Fleet.host() with extra_stage_cost = stage_cost(): the same T_hist as the device"""
    from time_opt_ilqr_amd import solver
    d = np.load(os.path.join(golden_dir, "fleet_prox_solve_pm4_0.npz"))
    F = _fixture_fleet(d)
    sol = solver.ilqr_timeopt(F.host(), d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method="propagator", max_iter=int(d["max_iter"]),
                              wrap_idx=d["wrap_idx"].tolist(), extra_stage_cost=F.stage_cost())
    assert list(sol["T_hist"]) == d["T_hist_propagator"].tolist()
    assert _elem_rel(np.asarray(sol["J_hist"]), d["J_hist_propagator"]) <= SOLVE_TOL


# ---------------------------------------------------------------- 9. batched
@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
def test_prox_batched_solve_equals_the_single_solves(dev, golden_dir, method):
    """the kept point mass x 4 fixtures as one batch (B = 3): row by row the single solves"""
    from time_opt_ilqr_amd import solver
    ds = [np.load(os.path.join(golden_dir, f"fleet_prox_solve_pm4_{t}.npz")) for t in range(3)]
    d = ds[0]
    assert len({float(x["w"]) for x in ds}) == 1 and all(np.array_equal(x["Q"], d["Q"]) for x in ds)
    assert all(np.array_equal(x["prox_obs"], d["prox_obs"]) for x in ds)
    F = _fixture_fleet(d)  # the starts and the goals differ per seed: xg is per problem
    kw = dict(max_iter=int(d["max_iter"]), method=method, wrap_idx=[])
    res = solver.ilqr_timeopt_batch(F, np.stack([x["x0"] for x in ds]),
                                    np.stack([x["xg"] for x in ds]), d["u_ref"],
                                    d["Q"], d["R"], d["Qf"], float(d["w"]), int(d["N"]),
                                    int(d["T_min"]), int(d["T_max"]), stage_timers=False, **kw)
    assert _np(res["crashed"]).tolist() == [0] * 3
    nh = _np(res["n_hist"])
    worst = 0.0
    for b, x in enumerate(ds):
        one = solver.ilqr_timeopt(F, x["x0"], x["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                                  float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                                  **kw)
        assert _np(res["T_hist"][b, :nh[b]]).tolist() == list(one["T_hist"]), b
        assert list(one["T_hist"]) == x[f"T_hist_{method}"].tolist()
        worst = max(worst, _elem_rel(_np(res["J_hist"][b, :nh[b]]), np.asarray(one["J_hist"])),
                    _elem_rel(_np(res["J_hist"][b, :nh[b]]), x[f"J_hist_{method}"]))
    print(f"fleet proximity batched solve {method}: J_hist relative error", worst)
    assert worst <= SOLVE_TOL
