"""GPU: the teams' proximity cost (include/hop_mixed_proximity.h, csrc/team_proximity.hpp).

Yardsticks and bars (the fleets' own, tests/test_gpu_fleet_proximity.py):
* the Taylor kernel, the true cost and the line search: fixtures of the reference with the
  NumPy bump cost of a team as extra_stage_cost
  (tests/golden/make_golden_team_proximity.py), to TRAJ_TOL = 1e-9, accepted indices exact;
  entries off the position blocks -- a DI's absent y and a point mass's absent z included --
  exactly +0.0 and cxx symmetric bit for bit;
* a cost with no term: c exactly +0.0, and the proximity entries equal the plain team
  entries bit for bit;
* plain cost_true + the Taylor kernel's c summed over k < T against the proximity
  cost_true: SUM_TOL = 1e-12 (two summation orders of at most 13 fp64 terms of one sign);
* contract (b): a team of equal members against its fleet with the same cost, every output
  of the three entries bit for bit, the line-search workspace included;
* member order: c to 1e-12 (one sum of non-negative terms in another order), cx and cxx
  permuted to 1e-9;
* whole solves: T_hist equal, J_hist to SOLVE_TOL = 1e-6 against
  tests/golden/team_prox_solve_*.npz (every select gap >= 1e-3, filtered by the generator).
Shapes: N = 12, batches 1, 5 and 67 (none a multiple of 4 rows per wave; 67 crosses a wave
and a workgroup).
"""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

from test_gpu_team import SIZES, case_inputs

pytestmark = pytest.mark.gpu
TRAJ_TOL, SOLVE_TOL, SUM_TOL = 1e-9, 1e-6, 1e-12
N = 12
BATCHES = (1, 5, 67)
# member ids, n, m, dt, D
SHAPES = {"pm_quad_di": ((3, 2, 0), 18, 7, 0.05, 3), "di2_pm2": ((0, 0, 3, 3), 12, 6, 0.05, 2),
          "quad_pm3": ((2, 3, 3, 3), 24, 10, 0.05, 3), "pm7_di": ((3,) * 7 + (0,), 30, 15, 0.05, 2),
          "all5": ((0, 1, 2, 3, 4), 26, 9, 0.02, 3)}
TAGS = list(SHAPES)
PDS = {0: 1, 1: 1, 2: 3, 3: 2, 4: 1}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVES = sorted(f for f in os.listdir(GOLDEN) if re.fullmatch(r"team_prox_solve_\w+_\d\.npz", f))
# threads, static LDS bytes of the larger instantiation: the cost / line-search kernels (the
# team's blocks and vectors, the table, the position slab), the Taylor kernel (table,
# positions, pair coefficients, diagonal blocks, the index words)
PROX_LDS = (256, (2 * 31 * 31 + 16 * 16 + 16 * 32 + 16 * 5 + 16 * 48) * 8)
TAYLOR_LDS = (256, (16 * 5 + 16 * (48 + 120 + 144)) * 8 + 32 * 4)


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
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous()


def _same(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _offsets(ids):
    return [int(v) for v in np.cumsum([0] + [SIZES[s][0] for s in ids[:-1]])]


@functools.lru_cache(maxsize=None)
def _case(tag, golden_dir):
    """(inputs, fixture, team with the cost, the same team without): computed once"""
    from time_opt_ilqr_amd import systems
    ids, n, m, dt, D = SHAPES[tag]
    d = np.load(os.path.join(golden_dir, f"team_prox_cases_{tag}.npz"))
    xo = _offsets(ids)
    c = case_inputs(int(d["seed"]), n, m, xo[1])
    obs, sep = prox_inputs(int(d["seed"]), c, xo, [PDS[s] for s in ids])
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum(), obs.sum()])
    assert np.array_equal(got, d["check"]), "the inputs are not the generator's"
    plain = systems.Team(ids, dt=dt)
    F = plain.with_proximity(systems.Proximity(obs, sep))
    assert (F.n, F.m, F.pos_dim) == (n, m, D) and F.proximity is not None
    assert sorted(d["wrap_idx"].tolist()) == sorted(F.wrap_idx)
    return c, d, F, plain


def _cost(c, F, dev):
    from time_opt_ilqr_amd import engine
    return engine.CostParams(_t(c["xg"], dev), _t(c["u_ref"], dev), _t(c["Q"], dev),
                             _t(c["R"], dev), _t(c["Qf"], dev), c["w"], None, F.wrap_idx)


def _pos_mask(F, dev):
    import torch
    pos = torch.zeros(F.n, dtype=torch.bool, device=dev)
    pos[F.position_idx] = True
    return pos


def _taylor_direct(dev, F, X, stride, rows, want=(True, True, True)):
    """the Taylor entry of a team or a fleet on rows of the caller's own stride"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    n = F.n
    out = [torch.full(s, -7.0, dtype=torch.float64, device=dev) if w else None
           for s, w in zip(((rows,), (rows, n), (rows, n, n)), want)]
    px, tab = engine._proximity_struct(F, dev)
    tail = (_lib.C.byref(px), _lib.ptr(X), stride, rows, *[_lib.ptr(o) for o in out],
            _lib.stream_handle(dev))
    if engine.is_team(F):
        rc = _lib.load().hop_mixed_proximity_taylor_f64(*engine._team_members(F), *tail)
    else:
        rc = _lib.load().hop_fleet_proximity_taylor_f64(_lib.C.byref(engine._fleet_params(F)),
                                                        *tail)
    _lib.check(rc)
    torch.cuda.synchronize(dev)
    del tab
    return out


def _linesearch_direct(dev, F, X, U, T, K, k, cost, active=None):
    """the proximity line-search entry of a team or a fleet on a workspace of the caller's
    own: [X', U', J, J_old, accepted, the workspace, its size in bytes]"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    lib = _lib.load()
    Bn, Nn = U.shape[:2]
    al = engine.ALPHAS
    ws_fn, par = engine._object_entry(F, "forward_workspace_bytes")
    cargs, keep = engine._chain_cost_args(cost, Bn, F.n, F.m, dev, F)
    px, tab = engine._proximity_struct(F, dev)
    nb = int(ws_fn(_lib.C.byref(par), Bn, Nn, len(al)))
    ws = torch.zeros((nb // 8,), dtype=torch.float64, device=dev)
    Tt = _t(T, dev, torch.int32)
    act = None if active is None else _t(active, dev, torch.int32)
    out = [torch.empty_like(X), torch.empty_like(U)] + [
        torch.empty((Bn,), dtype=torch.float64, device=dev) for _ in range(2)] + [
        torch.empty((Bn,), dtype=torch.int32, device=dev)]
    if engine.is_team(F):
        fn, head = lib.hop_mixed_prox_forward_linesearch_f64, \
            engine._team_members(F) + (float(F.dt),)
    else:
        fn, head = lib.hop_fleet_prox_forward_linesearch_f64, (_lib.C.byref(par),)
    _lib.check(fn(*head, _lib.ptr(X), _lib.ptr(U), *cargs, _lib.C.byref(px), _lib.ptr(Tt),
                  _lib.ptr(act), _lib.ptr(K), _lib.ptr(k), (_lib.C.c_double * len(al))(*al),
                  len(al), Bn, Nn, _lib.ptr(ws), nb, *[_lib.ptr(o) for o in out],
                  _lib.stream_handle(dev)))
    torch.cuda.synchronize(dev)
    del keep, tab
    return out + [ws, nb]


# ---------------------------------------------------------------- 1. the Taylor kernel
@pytest.mark.parametrize("tag", TAGS)
def test_taylor_kernel_vs_reference(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine
    c, d, F, _ = _case(tag, golden_dir)
    n = F.n
    X = _t(c["X"][:, 0], dev)
    pos = _pos_mask(F, dev)
    assert int(pos.sum()) == sum(F.pos_dims) < len(F.pos_dims) * F.pos_dim  # something is padded
    worst = 0.0
    for Bn in BATCHES:
        cc, cx, cxx = engine.team_proximity_cost(F, X[:Bn])
        worst = max(worst, _elem_rel(_np(cc), d["tay_c"][:Bn]), _elem_rel(_np(cx), d["tay_cx"][:Bn]),
                    _elem_rel(_np(cxx), d["tay_cxx"][:Bn]))
        # off the position blocks: exactly +0.0
        for off in (cx[:, ~pos], cxx[:, ~pos, :], cxx[:, :, ~pos]):
            assert bool((_bits(off) == 0).all()), (tag, Bn)
        assert torch.equal(_bits(cxx), _bits(cxx.transpose(1, 2))), (tag, Bn)
    print(f"team proximity taylor {tag}: max elementwise rel err {worst:.2e}")
    assert worst <= TRAJ_TOL
    assert float(d["tay_c"].max()) >= 0.1 * max(float(d["prox_obs"][:, -1].max()),
                                                float(d["prox_sep"][1]))
    # nullable outputs: each alone is the full call's
    for want in (("c",), ("cx",), ("cxx",), ("c", "cxx")):
        part = engine.team_proximity_cost(F, X, want=want)
        for name, g, r in zip(("c", "cx", "cxx"), part, (cc, cx, cxx)):
            assert (g is None) == (name not in want)
            assert g is None or _same(g, r)
    # a leading shape, and strided rows: only the n leading entries of a row are read
    lead = engine.team_proximity_cost(F, X[:66].reshape(6, 11, n))
    assert lead[2].shape == (6, 11, n, n) and _same(lead[2].reshape(66, n, n), cxx[:66])
    Xs = torch.full((5, n + 3), 1e300, dtype=torch.float64, device=dev)
    Xs[:, :n] = X[:5]
    for g, r in zip(_taylor_direct(dev, F, Xs, n + 3, 5), (cc, cx, cxx)):
        assert _same(g, r[:5])


# ---------------------------------------------------------------- 2. degenerate costs
def _ls_equal(a, b):
    return all(_same(getattr(a, f), getattr(b, f)) for f in ("X", "U", "J", "J_old", "accepted"))


@pytest.mark.parametrize("tag", TAGS)
def test_null_cost_is_the_plain_team_bitwise(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine, systems
    c, d, F, plain = _case(tag, golden_dir)
    # no table and no separation; a table of weight-0 rows only contributes +0.0 as well
    Z = plain.with_proximity(systems.Proximity())
    for t in engine.team_proximity_cost(Z, _t(c["X"][:, 0], dev)):
        assert bool((_bits(t) == 0).all())  # exactly +0.0
    rows = d["prox_obs"].copy()
    rows[:, -1] = 0.0
    W0 = plain.with_proximity(systems.Proximity(rows, (0.45, 0.0)))
    for t in engine.team_proximity_cost(W0, _t(c["X"][:, 0], dev)):
        assert bool((_bits(t) == 0).all())
    cost = _cost(c, F, dev)
    X, U, T = _t(c["X"], dev), _t(c["U"], dev), c["T"]
    Jp = engine.cost_true(plain, X, U, T, cost)
    assert _same(engine.cost_true(Z, X, U, T, cost), Jp)
    assert not torch.equal(engine.cost_true(F, X, U, T, cost), Jp)  # the cost itself is seen
    pick = d["ls_pick"]
    args = (_t(d["ls_X"], dev), _t(c["U0"][pick], dev), c["T0"][pick], _t(d["ls_K"], dev),
            _t(d["ls_k"], dev), cost)
    assert _ls_equal(engine.forward_linesearch(Z, *args, F.dt),
                     engine.forward_linesearch(plain, *args, F.dt))


@pytest.mark.parametrize("sid", [3, 2])
def test_team_of_one_with_separation_only_is_the_plain_team(dev, sid):
    from time_opt_ilqr_amd import engine, systems
    plain = systems.Team([sid])
    one = plain.with_proximity(systems.Proximity(separation=(0.4, 2.0)))
    n, m, Bn = plain.n, plain.m, 5
    c = case_inputs(77, n, m, n, N, Bn, 12)
    cost = _cost(c, plain, dev)
    cc = engine.team_proximity_cost(one, _t(c["X"][:, 0], dev))[0]
    assert bool((_bits(cc) == 0).all())
    x0 = _t(c["x0"][:Bn], dev)
    U = _t(c["U0"][:Bn] * (0.05 if sid == 2 else 1.0), dev)
    X = engine.rollout(plain, x0, U, plain.dt)
    T = c["T0"][:Bn]
    assert _same(engine.cost_true(one, X, U, T, cost), engine.cost_true(plain, X, U, T, cost))
    rng = np.random.default_rng(3)
    K = _t(0.05 * rng.standard_normal((Bn, N, m, n)), dev)
    k = _t(0.05 * rng.standard_normal((Bn, N, m)), dev)
    a = engine.forward_linesearch(one, X, U, T, K, k, cost, plain.dt)
    b = engine.forward_linesearch(plain, X, U, T, K, k, cost, plain.dt)
    assert _ls_equal(a, b)


# ---------------------------------------------------------------- 3. the true cost
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
    print(f"team proximity cost_true {tag}: max rel err {worst:.2e}")
    assert worst <= TRAJ_TOL
    # consistency: plain cost + sum_{k < T} c_k from the Taylor kernel
    X, U = _t(c["X"], dev), _t(c["U"], dev)
    T = _t(c["T"], dev, torch.int32)
    ck = engine.team_proximity_cost(F, X[:, :N], want=("c",))[0]
    mask = torch.arange(N, device=dev)[None, :] < T[:, None]
    total = engine.cost_true(plain, X, U, c["T"], cost) + (ck * mask).sum(1)
    err = _elem_rel(_np(J), _np(total))
    print(f"team proximity cost_true {tag}: against plain + sum of c_k {err:.2e}; the cost is "
          f"{float(((ck * mask).sum(1) / J).median()):.1%} of J (median)")
    assert err <= SUM_TOL
    # T = 0 -> +inf, T > N -> NaN, a NaN on the rows read -> +inf, beyond them: not read
    Xb = c["X"][:5].copy()
    Xb[2, 3, 0] = np.nan
    Xb[3, 9, 0] = np.nan
    Tb = np.array([0, N + 1, 7, 4, N], dtype=np.int32)
    Jb = _np(engine.cost_true(F, _t(Xb, dev), _t(c["U"][:5], dev), Tb, cost))
    assert Jb[0] == np.inf and np.isnan(Jb[1]) and Jb[2] == np.inf and np.isfinite(Jb[3:]).all()


# ---------------------------------------------------------------- 4. line search
def test_line_search_fixtures_accept_at_three_step_sizes(golden_dir):
    seen = set()
    for tag in TAGS:
        d = _case(tag, golden_dir)[1]
        seen |= set(d["ls_acc"][[0, 1, 3]].tolist())
    assert len(seen) >= 3, seen


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
    print(f"team proximity line search {tag}: accepted {got.tolist()} reference "
          f"{d['ls_acc'].tolist()}; the cost is {np.round(d['ls_extra0'] / d['ls_J0'], 3).tolist()} "
          "of J_old")
    assert got[on].tolist() == d["ls_acc"][on].tolist() and got[2] == -2
    eJ = _elem_rel(_np(r.J)[on], d["ls_J"][on])
    eJ0 = _elem_rel(_np(r.J_old), d["ls_J0"])
    eX = float(np.abs(_np(r.X)[on] - d["ls_Xo"][on]).max())
    eU = float(np.abs(_np(r.U)[on] - d["ls_Uo"][on]).max())
    print(f"team proximity line search {tag}: J {eJ:.2e} J_old {eJ0:.2e} X' {eX:.2e} U' {eU:.2e}")
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL
    assert float(np.abs(d["ls_Xo"]).max()) < 50.0  # absolute and relative bars coincide
    assert np.array_equal(_np(r.X)[2], d["ls_X"][2]) and np.array_equal(_np(r.U)[2], U[2])
    assert _np(r.J)[2] == _np(r.J_old)[2]
    # the cost is in J_old: the plain team's differs by the fixture's share
    J0p = _np(engine.forward_linesearch(plain, _t(d["ls_X"], dev), _t(U, dev), T,
                                        _t(d["ls_K"], dev), _t(d["ls_k"], dev),
                                        _cost(c, F, dev), F.dt).J_old)
    assert _elem_rel(d["ls_J0"] - J0p, d["ls_extra0"]) <= 1e-6


def _quiet(F):
    f = np.ones(F.m)
    for s, o in zip(F.member_ids, F.u_offsets):
        if s == 2:
            f[o:o + 4] = 0.05
    return f


@pytest.mark.parametrize("tag", TAGS)
def test_prox_linesearch_zero_gains_is_the_rollout(dev, golden_dir, tag):
    import torch
    from time_opt_ilqr_amd import engine
    c, _, F, plain = _case(tag, golden_dir)
    Bn = 5
    rng = np.random.default_rng(41 + F.n)
    x0 = _t(rng.uniform(-0.8, 0.8, (Bn, F.n)), dev)
    U = _t(rng.uniform(-1.0, 1.0, (Bn, N, F.m)) * _quiet(F), dev)
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
    na = len(engine.ALPHAS)
    *_, ws, nb = _linesearch_direct(dev, F, X, U, T, K, k, cost)
    assert nb == Bn * na * (1 + (N + 1) * F.n + N * F.m) * 8
    Jc = ws[:Bn * na].reshape(Bn, na)
    assert torch.equal(Jc, r.J_old[:, None].expand(Bn, na))
    rows = ws[Bn * na:].reshape(Bn, na, -1)
    nx = (N + 1) * F.n
    assert torch.equal(rows[:, :, :nx], X.reshape(Bn, 1, nx).expand(Bn, na, nx))
    assert torch.equal(rows[:, :, nx:], U.reshape(Bn, 1, -1).expand(Bn, na, N * F.m))


# ---------------------------------------------------------------- 5. contract (b)
@pytest.mark.parametrize("sid,count", [(3, 4), (2, 2), (0, 15), (1, 5)])
def test_team_of_equal_members_is_the_fleet_bitwise(dev, sid, count):
    """every output of the three proximity entries, B = 67, the workspace included"""
    import torch
    from test_gpu_fleet import case_inputs as fleet_inputs
    from test_gpu_fleet_proximity import prox_inputs as fleet_prox_inputs
    from time_opt_ilqr_amd import engine, systems
    plain = systems.Fleet(sid, count)
    seed = 9300 + 100 * sid + count
    c = fleet_inputs(seed, plain.n, plain.m, plain.n_member)
    obs, sep = fleet_prox_inputs(seed, c, count, plain.n_member, plain.pos_dim)
    p = systems.Proximity(obs, sep)
    Fl = systems.Fleet(sid, count, proximity=p)
    Tm = systems.Team([sid] * count).with_proximity(p)
    assert (Tm.n, Tm.m, Tm.dt, Tm.wrap_idx, Tm.pos_dim) == (Fl.n, Fl.m, Fl.dt, Fl.wrap_idx,
                                                            Fl.pos_dim)
    Bn = 67
    X, U = _t(c["X"], dev), _t(c["U"], dev)
    assert X.shape[0] == Bn
    x = X[:, 0].contiguous()
    a, b = (_taylor_direct(dev, F, x, F.n, Bn) for F in (Fl, Tm))
    for g, r, key in zip(a, b, ("c", "cx", "cxx")):
        assert _same(g, r), (sid, count, key)
    assert float(a[0].max()) >= 0.1 * sep[1]
    cost = [_cost(c, F, dev) for F in (Fl, Tm)]
    T = c["T"].copy()
    T[:3] = (0, N + 1, N)
    a, b = (engine.cost_true(F, X, U, T, cs) for F, cs in zip((Fl, Tm), cost))
    assert _same(a, b) and bool(torch.isfinite(a[3:]).all())
    assert not torch.equal(a[3:], engine.cost_true(plain, X, U, T, cost[0])[3:])
    rng = np.random.default_rng(77 + Fl.n)
    x0 = _t(c["xg"] + rng.uniform(-0.4, 0.4, (Bn, Fl.n)), dev)
    U0 = _t(c["u_ref"] + 0.3 * rng.uniform(-1.0, 1.0, (Bn, N, Fl.m)), dev)
    X0 = engine.rollout(Fl, x0, U0, Fl.dt)
    assert bool(torch.isfinite(X0).all())
    K = _t(0.05 * rng.standard_normal((Bn, N, Fl.m, Fl.n)), dev)
    fac = np.array([0.5, 4.0, 8.0, 16.0])[np.arange(Bn) % 4]
    k = _t(-fac[:, None, None] * (_np(U0) - c["u_ref"]), dev)
    active = (np.arange(Bn) % 7 != 3).astype(np.int32)
    a, b = (_linesearch_direct(dev, F, X0, U0, c["T"], K, k, cs, active)
            for F, cs in zip((Fl, Tm), cost))
    assert a[-1] == b[-1] > 0
    for i, key in enumerate(("X", "U", "J", "J_old", "accepted", "workspace")):
        assert _same(a[i], b[i]), (sid, count, key)
    acc = _np(a[4])
    assert (acc[active == 0] == -2).all() and (acc[active != 0] >= -1).all()


# ---------------------------------------------------------------- 6. member order
def test_member_order(dev, golden_dir):
    """pm_quad_di and its permutation (DI, point mass, quadrotor) with the states permuted:
    c sums the same non-negative bumps in another order (1e-12); cx and cxx are the
    permuted ones (1e-9)"""
    from time_opt_ilqr_amd import engine, systems
    c, d, F, _ = _case("pm_quad_di", golden_dir)
    G = systems.Team([0, 3, 2]).with_proximity(F.proximity)
    order = [2, 0, 1]  # G's members as members of F
    ix = np.concatenate([np.arange(F.x_offsets[a], F.x_offsets[a] + SIZES[F.member_ids[a]][0])
                         for a in order])
    assert [F.member_ids[a] for a in order] == list(G.member_ids)
    X = c["X"][:, 0]
    cf, cxf, cxxf = (_np(t) for t in engine.team_proximity_cost(F, _t(X, dev)))
    cg, cxg, cxxg = (_np(t) for t in engine.team_proximity_cost(G, _t(X[:, ix], dev)))
    e0 = _elem_rel(cg, cf)
    e1 = _elem_rel(cxg, cxf[:, ix])
    e2 = _elem_rel(cxxg, cxxf[:, ix][:, :, ix])
    print(f"team proximity member order: c {e0:.2e} cx {e1:.2e} cxx {e2:.2e}")
    assert e0 <= SUM_TOL and max(e1, e2) <= TRAJ_TOL


# ---------------------------------------------------------------- 7. LDS
@pytest.mark.parametrize("tag", ["all5", "quad_di4_pm2", "pm7_di"])
def test_prox_kernels_on_poisoned_lds(dev, golden_dir, tag):
    """the cost and line-search kernels stage Q, Qf, R, the table, a vector and a position
    slab per row in LDS, the Taylor kernel the table, positions, pair coefficients, diagonal
    blocks and index words: the same bits after each of the three fill patterns"""
    import test_gpu_team as tt
    from test_gpu_lds_poison import run_poisoned
    from time_opt_ilqr_amd import engine, systems
    if tag in SHAPES:
        c, d, F, _ = _case(tag, golden_dir)
    else:  # no proximity fixture of this shape: the plain team's inputs and a drawn cost
        c, d = tt._case(tag, golden_dir)
        c = dict(c, X=c["X"].copy())
        plain = tt._team(tag)
        obs, sep = prox_inputs(int(d["seed"]), c, list(plain.x_offsets), list(plain.pos_dims))
        F = plain.with_proximity(systems.Proximity(obs, sep))
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
        cc, cx, cxx = engine.team_proximity_cost(F, Xt)
        return dict(c=cc, cx=cx, cxx=cxx)

    base = run_poisoned(dev, fn, PROX_LDS, 2)
    stage = F.stage_cost()
    if tag in SHAPES:
        assert _elem_rel(_np(base["Jc"]), d["cost_J"][:5]) <= TRAJ_TOL
        assert _np(base["accepted"]).tolist() == d["ls_acc"].tolist()
    base = run_poisoned(dev, taylor, TAYLOR_LDS, 2)
    ref = np.stack([stage(x)[2] for x in c["X"][:21, 0]])
    assert float(np.abs(_np(base["cxx"]) - ref).max()) <= TRAJ_TOL * max(1.0, np.abs(ref).max())
    assert np.abs(ref).max() > 0.1


# ---------------------------------------------------------------- 8. global memory
@contextlib.contextmanager
def _table_in(F, dev):
    """call(i) puts the team's obstacle table where the engine caches it, so that the table
    the kernels read is the arena's copy; the cache entry is dropped afterwards"""
    prox = F.proximity
    cache = prox.__dict__.setdefault("_device_tables", {})
    before = cache.pop(str(dev), None)
    rows = prox.table(int(F.pos_dim))
    assert len(rows)

    def use(i):
        cache[str(dev)] = i["table"]
    try:
        yield dict(table=_t(np.asarray(rows.tolist()), dev)), use
    finally:
        cache.pop(str(dev), None)
        if before is not None:
            cache[str(dev)] = before


def test_prox_entries_global_memory(dev, golden_dir):
    """the three entries in tests/arena.py's carved buffer with the three fill patterns:
    results unchanged by a bit, nothing outside the documented extents written, no input
    changed"""
    import torch
    import test_gpu_global_memory as gm
    from time_opt_ilqr_amd import _lib, engine
    c, d, F, _ = _case("pm_quad_di", golden_dir)
    n = F.n
    ALL = gm.ALL
    X = _t(c["X"][:5, 0], dev)
    pick = d["ls_pick"]
    wrap = F.wrap_idx
    with _table_in(F, dev) as (table, use_table):
        def call(i):
            use_table(i)
            return dict(zip(("c", "cx", "cxx"), engine.team_proximity_cost(F, i["X"])))
        base = gm.run_case(dev, "team-prox-taylor", dict(X=X, **table), call,
                           dict(c=ALL, cx=ALL, cxx=ALL))
        for key in ("c", "cx", "cxx"):
            assert _elem_rel(_np(base[key]), d["tay_" + key][:5]) <= TRAJ_TOL, key
        Xs = torch.full((5, n + 3), 1e300, dtype=torch.float64, device=dev)
        Xs[:, :n] = X

        def direct(i):
            use_table(i)
            t_ = engine._torch()
            out = [t_.empty(s, dtype=torch.float64, device=dev) for s in ((5,), (5, n), (5, n, n))]
            px, tab = engine._proximity_struct(F, dev)
            _lib.check(_lib.load().hop_mixed_proximity_taylor_f64(
                *engine._team_members(F), _lib.C.byref(px), _lib.ptr(i["X"]), n + 3, 5,
                *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
            return dict(zip(("c", "cx", "cxx"), out))
        strided = gm.run_case(dev, "team-prox-taylor-strided", dict(X=Xs, **table), direct,
                              dict(c=ALL, cx=ALL, cxx=ALL))
        for key in ("c", "cx", "cxx"):
            assert _same(strided[key], base[key]), key

        inputs = dict(X=_t(c["X"][:5], dev), U=_t(c["U"][:5], dev),
                      T=_t(np.asarray(c["T"][:5]), dev, torch.int32),
                      **gm._row_cost_inputs(c, dev), **table)

        def call(i):
            use_table(i)
            return dict(J=engine.cost_true(F, i["X"], i["U"], i["T"], gm._cost_params(i, wrap)))
        base = gm.run_case(dev, "team-prox-cost_true", inputs, call, dict(J=ALL))
        assert _elem_rel(_np(base["J"]), d["cost_J"][:5]) <= TRAJ_TOL

        active = np.array([1, 1, 0, 1])
        inputs = dict(X=_t(d["ls_X"], dev), U=_t(c["U0"][pick], dev), K=_t(d["ls_K"], dev),
                      k=_t(d["ls_k"], dev), T=_t(c["T0"][pick], dev, torch.int32),
                      active=_t(active, dev, torch.int32), **gm._row_cost_inputs(c, dev), **table)

        def call(i):
            use_table(i)
            r = engine.forward_linesearch(F, i["X"], i["U"], i["T"], i["K"], i["k"],
                                          gm._cost_params(i, wrap), F.dt, active=i["active"])
            return dict(X=r.X, U=r.U, J=r.J, J_old=r.J_old, accepted=r.accepted)
        base = gm.run_case(dev, "team-prox-linesearch", inputs, call,
                           dict(X=ALL, U=ALL, J=ALL, J_old=ALL, accepted=ALL))
    on = active != 0
    got = _np(base["accepted"])
    assert got[on].tolist() == d["ls_acc"][on].tolist() and (got[~on] == -2).all()
    assert _elem_rel(_np(base["J"])[on], d["ls_J"][on]) <= TRAJ_TOL
    assert _elem_rel(_np(base["J_old"]), d["ls_J0"]) <= TRAJ_TOL
    assert float(np.abs(_np(base["X"]) - d["ls_Xo"])[on].max()) <= TRAJ_TOL


# ---------------------------------------------------------------- 9. whole solves
def _fixture_team(d):
    from time_opt_ilqr_amd import systems
    return systems.Team(d["members"].tolist(), dt=float(d["dt"])).with_proximity(
        systems.Proximity(d["prox_obs"], tuple(d["prox_sep"])))


def _solve(F, d, method):
    from time_opt_ilqr_amd import solver
    return solver.ilqr_timeopt(F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                               float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                               method=method, max_iter=int(d["max_iter"]),
                               wrap_idx=d["wrap_idx"].tolist())


def test_team_prox_solve_fixtures_are_there():
    tags = {re.fullmatch(r"team_prox_solve_(\w+)_\d\.npz", f).group(1) for f in SOLVES}
    assert tags == {"di2_pm2", "pm_quad_di", "quad_pm3"} and len(SOLVES) == 9


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
@pytest.mark.parametrize("name", SOLVES)
def test_prox_solve_vs_reference(dev, golden_dir, name, method):
    from time_opt_ilqr_amd import solver
    d = np.load(os.path.join(golden_dir, name))
    assert float(d[f"gaps_{method}"].min()) >= 1e-3
    F = _fixture_team(d)
    sol = _solve(F, d, method)
    assert list(sol["T_hist"]) == d[f"T_hist_{method}"].tolist(), (name, sol["T_hist"])
    err = _elem_rel(np.asarray(sol["J_hist"]), d[f"J_hist_{method}"])
    print(name, method, "J_hist relative error", err, "the cost's share of J",
          float(d[f"extra_share_{method}"]))
    assert err <= SOLVE_TOL
    if name == "team_prox_solve_di2_pm2_0.npz" and method == "propagator":
        # the reference-named drop-ins on the solution
        from time_opt_ilqr_amd import systems
        T = int(sol["T_star"])
        args = (d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"], float(d["w"]))
        wrap = d["wrap_idx"].tolist()
        J = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, wrap, system=F)
        assert abs(J - sol["J_hist"][-1]) <= TRAJ_TOL * abs(J)
        stage = F.stage_cost()
        extra = sum(stage(sol["X"][k])[0] for k in range(T))
        Jp = solver.cost_timeopt_true(sol["X"], sol["U"], *args, T, wrap,
                                      system=systems.Team(F.member_ids, dt=F.dt))
        assert abs((J - Jp) - extra) <= 1e-9 * abs(J) and extra > 0.0
        Xo, Uo, Jl, acc = solver.forward_linesearch_fixedT(
            F, sol["X"], sol["U"], *args, T, [np.zeros(F.m)] * T, [np.zeros((F.m, F.n))] * T,
            wrap_idx=wrap)
        assert not acc and abs(Jl - J) <= TRAJ_TOL * abs(J)


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
@pytest.mark.parametrize("trial", range(3))
def test_di15_team_is_the_fleet_solve_bitwise(dev, golden_dir, trial, method):
    """the solve in which the cost decides the horizon: Team([0] * 15) with the fleet
    fixture's cost gives the fixture's T_hist and the Fleet device solve's T_hist and J_hist
    bit for bit"""
    from time_opt_ilqr_amd import systems
    d = np.load(os.path.join(golden_dir, f"fleet_prox_solve_di15_{trial}.npz"))
    p = systems.Proximity(d["prox_obs"], tuple(d["prox_sep"]))
    Fl = systems.Fleet(0, 15, proximity=p)
    Tm = systems.Team([0] * 15).with_proximity(p)
    a, b = _solve(Fl, d, method), _solve(Tm, d, method)
    assert list(b["T_hist"]) == d[f"T_hist_{method}"].tolist()
    assert list(a["T_hist"]) == list(b["T_hist"])
    assert np.array_equal(np.asarray(a["J_hist"]), np.asarray(b["J_hist"]))


def test_prox_host_path_selects_the_same_horizons(dev, golden_dir):
    """Team.host() with extra_stage_cost = stage_cost(): the same T_hist as the device"""
    from time_opt_ilqr_amd import solver
    d = np.load(os.path.join(golden_dir, "team_prox_solve_di2_pm2_0.npz"))
    F = _fixture_team(d)
    sol = solver.ilqr_timeopt(F.host(), d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], d["Qf"],
                              float(d["w"]), int(d["N"]), int(d["T_min"]), int(d["T_max"]),
                              method="propagator", max_iter=int(d["max_iter"]),
                              wrap_idx=d["wrap_idx"].tolist(), extra_stage_cost=F.stage_cost())
    assert list(sol["T_hist"]) == d["T_hist_propagator"].tolist()
    assert _elem_rel(np.asarray(sol["J_hist"]), d["J_hist_propagator"]) <= SOLVE_TOL


@pytest.mark.parametrize("method", ["propagator", "bruteforce"])
def test_prox_batched_solve_equals_the_single_solves(dev, golden_dir, method):
    """the kept di2_pm2 fixtures as one batch (B = 3): row by row the single solves"""
    from time_opt_ilqr_amd import solver
    ds = [np.load(os.path.join(golden_dir, f"team_prox_solve_di2_pm2_{t}.npz")) for t in range(3)]
    d = ds[0]
    assert len({float(x["w"]) for x in ds}) == 1 and all(np.array_equal(x["Q"], d["Q"]) for x in ds)
    assert all(np.array_equal(x["prox_obs"], d["prox_obs"]) for x in ds)
    F = _fixture_team(d)  # the starts and the goals differ per seed: xg is per problem
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
    print(f"team proximity batched solve {method}: J_hist relative error", worst)
    assert worst <= SOLVE_TOL
