"""The wide brute-force J curve (hop_bruteforce_jcurve_wide_f64, include/hop_wide_jcurve.h)
against the per-horizon wide Riccati pass (bitwise), the NumPy oracle, the narrow kernels
on the shapes both run, and the reference's own method="bruteforce" solves at n > 16."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

SHAPES = [(17, 4), (24, 16), (25, 9), (31, 8)]  # HR = 12, 12, 16, 16; m up to the limit
N, T_MAX, BN = 12, 11, 5   # B * t_max = 55 waves: the last workgroup has one live wave
WRAP, W_STAGE, LM = [1], 0.7, 1e-6


def _t(x, dev, dtype=None):
    import torch
    # np.array: a writable copy (the cached problems are read-only)
    return torch.as_tensor(np.array(x, order="C"), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


@functools.lru_cache(maxsize=None)
def _problems(n, m, N=N, Bn=BN, seed=8100):
    """(A, B, X, U, xg, u_ref, Q, R, Qf, alpha) stacked over the batch; problem 1 has a
    non-symmetric Q.  Read-only: the tests copy what they change."""
    probs = [orc.synth_riccati_problem(seed + 10 * n + i, n, m, N) for i in range(Bn)]
    A, B, X, U, xg, ur, Q, R = (np.stack([p[j] for p in probs]) for j in range(8))
    if Bn > 1:
        Q[1] = Q[1] + 0.1 * np.triu(np.random.default_rng(seed).standard_normal((n, n)), 1)
    alpha = np.array([p[8] for p in probs])
    Qf = np.stack([orc.terminal_weight(a, n) for a in alpha])
    out = (A, B, X, U, xg, ur, Q, R, Qf, alpha)
    for x in out:
        x.setflags(write=False)
    return out


def _oracle_curve(P, b, t_max, extra=None):
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    return orc.bruteforce_J(list(A[b]), list(B[b]), X[b], U[b], xg[b], ur[b], Q[b], R[b],
                            float(alpha[b]), W_STAGE, t_max, lm_lambda=LM, wrap_idx=WRAP,
                            extra=extra)


def _wide(dev, P, t_max, **kw):
    from time_opt_ilqr_amd import engine
    kw = {**dict(lm_lambda=LM, w_stage=W_STAGE, wrap_idx=WRAP), **kw}
    J, st = engine.bruteforce_jcurve_wide(*[_t(x, dev) for x in P[:9]], t_max, **kw)
    return _np(J), _np(st)


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES)
def test_wide_jcurve_equals_per_horizon_wide_riccati(dev, n, m):
    """every horizon of the one-launch curve is the mode-1 pass at that horizon: the same
    status, and V_0 bit for bit (NaN where that pass failed)"""
    from time_opt_ilqr_amd import engine
    P = list(_problems(n, m))
    X = P[2].copy()
    X[3, 7, 0] = np.nan
    P[2] = X
    args = [_t(x, dev) for x in P[:9]]
    J, st = engine.bruteforce_jcurve_wide(*args, T_MAX, lm_lambda=LM, w_stage=W_STAGE,
                                          wrap_idx=WRAP)
    J, st = _np(J), _np(st)
    assert J.shape == (BN, T_MAX) and st.shape == (BN, T_MAX) and st.dtype == np.int32
    for T in range(1, T_MAX + 1):
        r = engine.riccati(*args, T, LM, mode=1, w_stage=W_STAGE, wrap_idx=WRAP, reg_max_tries=1)
        sr = _np(r.status)
        assert st[:, T - 1].tolist() == sr.tolist(), T
        ok = (sr & orc.ST_FAIL) == 0
        assert np.array_equal(J[ok, T - 1], _np(r.V0)[ok, 0]), T
        assert np.isnan(J[~ok, T - 1]).all(), T
    # the NaN state at step 7 is read by the horizons T >= 7 (as x_T, or as a stage) only
    assert ((st[3] & orc.ST_NONFINITE) != 0).tolist() == [T - 1 >= 6 for T in range(1, T_MAX + 1)]
    assert (st[[0, 1, 2, 4]] == 0).all()


# 2 -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,extra", [(n, m, False) for n, m in SHAPES] + [(24, 16, True)])
def test_wide_jcurve_vs_oracle(dev, n, m, extra):
    """J against the oracle's bruteforce_J: 1e-6 elementwise, the bar test_gpu_wide.py
    holds the wide mode-1 V0 to (J is an element of that array)"""
    P = _problems(n, m)
    kw, ex = {}, [None] * BN
    if extra:  # the extra stage cost: PSD cxx, cx and c per (problem, step)
        rng = np.random.default_rng(6)
        M = rng.standard_normal((BN, N, n, n))
        cxx = 0.05 * M @ M.transpose(0, 1, 3, 2) / n
        cx = 0.1 * rng.standard_normal((BN, N, n))
        c0 = rng.uniform(0.0, 0.5, (BN, N))
        kw = dict(qxx_extra=_t(cxx, dev), qx_extra=_t(cx, dev), c_extra=_t(c0, dev))

        def make(b):
            Xb = P[2][b]
            return lambda x, u: (lambda k: (c0[b, k], cx[b, k], cxx[b, k]))(
                int(np.argmin(np.abs(Xb[:N] - x).sum(axis=1))))
        ex = [make(b) for b in range(BN)]
    J, st = _wide(dev, P, T_MAX, **kw)
    Jo = np.stack([_oracle_curve(P, b, T_MAX, ex[b]) for b in range(BN)])
    err = _elem_rel(J, Jo)
    print(f"n={n} m={m} extra={extra}: J max elementwise relative error {err:.3e}")
    assert err <= 1e-6
    assert (st == 0).all()


# 3 -------------------------------------------------------------------------
def test_wide_jcurve_bruteforce_only_rules(dev):
    """what the brute-force curve does differently from value_expansions (solver.py:326-356
    checks nothing itself, only chol_solve raises)"""
    n, m, Nn = 20, 4, 8
    P = list(_problems(n, m, Nn, 3))
    X = P[2].copy()
    X[1, 0, 2] = np.nan   # x_0: only the stage cost and Vx of step 0 see it
    R = P[7].copy()
    R[2] = -50.0 * np.eye(m)  # negative definite: no jitter makes Quu_reg factor
    P[2], P[7] = X, R
    J, st = _wide(dev, P, Nn)
    print("status", st.tolist())
    assert (st[0] == 0).all() and _elem_rel(J[0], _oracle_curve(P, 0, Nn)) <= 1e-6
    assert ((st[1] & orc.ST_FAIL) == 0).all()
    assert not np.isfinite(J[1]).any()
    with np.errstate(all="ignore"):
        assert not np.isfinite(_oracle_curve(P, 1, Nn)).any()  # the oracle does not raise either
    assert ((st[2] & orc.ST_FAIL) != 0).all()
    assert np.isnan(J[2]).all()
    with pytest.raises(np.linalg.LinAlgError):
        _oracle_curve(P, 2, 1)
    # the mode-1 pass does fail on the NaN x_0 (horizon_selection.py:209-210)
    from time_opt_ilqr_amd import engine
    r = engine.riccati(*[_t(x, dev) for x in P[:9]], Nn, LM, mode=1, w_stage=W_STAGE,
                       wrap_idx=WRAP, reg_max_tries=1)
    assert int(_np(r.status)[1]) & orc.ST_FAIL


# 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(12, 3), (16, 2)])
def test_wide_jcurve_kernel_on_narrow_shapes(dev, n, m):
    """the wide entry called directly (Python routes n <= 16 to the narrow kernels)
    against engine.bruteforce_jcurve, the narrow generic kernels, on the same inputs"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    P = list(_problems(n, m))
    X = P[2].copy()
    X[3, 7, 0] = np.nan
    P[2] = X
    args = [_t(x, dev) for x in P[:9]]
    Jn, sn = engine.bruteforce_jcurve(*args, T_MAX, lm_lambda=LM, w_stage=W_STAGE, wrap_idx=WRAP)
    J = torch.empty((BN, T_MAX), dtype=torch.float64, device=dev)
    st = torch.empty((BN, T_MAX), dtype=torch.int32, device=dev)
    strides = [n, m, n * n, m * m, n * n]  # xg, u_ref, Q, R, Qf per problem
    ins = [_lib.ptr(a) for a in args[:4]]
    for a, s in zip(args[4:], strides):
        ins += [_lib.ptr(a), s]
    _lib.check(_lib.load().hop_bruteforce_jcurve_wide_f64(
        *ins, None, None, None, LM, W_STAGE, engine.wrap_mask(WRAP, n), BN, N, n, m, T_MAX,
        _lib.ptr(J), _lib.ptr(st), _lib.stream_handle(dev)))
    torch.cuda.synchronize()
    J, st, Jn, sn = _np(J), _np(st), _np(Jn), _np(sn)
    assert st.tolist() == sn.tolist()
    ok = (sn & orc.ST_FAIL) == 0
    assert ok.sum() == BN * T_MAX - 5 and np.isnan(J[~ok]).all() and np.isnan(Jn[~ok]).all()
    gap = _elem_rel(J[ok], Jn[ok])
    print(f"n={n} m={m}: wide vs narrow J, max elementwise relative gap {gap:.3e}")
    assert gap <= 1e-6


# 5 -------------------------------------------------------------------------
def test_wide_jcurve_edges(dev):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    n, m, Nn = 20, 3, 6
    P = _problems(n, m, Nn, BN)
    full, sf = _wide(dev, P, Nn)  # t_max = n_alloc
    assert (sf == 0).all()
    assert _elem_rel(full, np.stack([_oracle_curve(P, b, Nn) for b in range(BN)])) <= 1e-6
    # the horizons are independent sweeps: a shorter curve is the longer one's prefix
    J1, s1 = _wide(dev, P, 1)
    assert J1.shape == (BN, 1) and np.array_equal(J1, full[:, :1]) and (s1 == 0).all()
    # t_max < n_alloc: the steps past t_max are never read
    t = 4
    Pn = [x.copy() for x in P[:9]]
    Pn[0][:, t:] = np.nan
    Pn[1][:, t:] = np.nan
    Pn[2][:, t + 1:] = np.nan
    Pn[3][:, t:] = np.nan
    Jt, s_t = _wide(dev, Pn, t)
    assert np.array_equal(Jt, full[:, :t]) and (s_t == 0).all()
    # B = 1
    Jb, sb = _wide(dev, [x[2:3] for x in P[:9]], Nn)
    assert np.array_equal(Jb, full[2:3]) and (sb == 0).all()
    # a permutation of the batch permutes the rows
    perm = np.array([3, 0, 4, 2, 1])
    Jp, sp = _wide(dev, [x[perm] for x in P[:9]], Nn)
    assert np.array_equal(Jp, full[perm]) and (sp == 0).all()
    # batch-shared cost blocks (stride 0) against the same blocks repeated per problem
    shared = list(P[:4]) + [x[0] for x in P[4:9]]
    rep = list(P[:4]) + [np.repeat(x[:1], BN, axis=0) for x in P[4:9]]
    Js, ss = _wide(dev, shared, Nn)
    Jr, sr = _wide(dev, rep, Nn)
    assert np.array_equal(Js, Jr) and np.array_equal(ss, sr) and (ss == 0).all()
    assert np.array_equal(Js[0], full[0])
    # t_max = N + 1 is the reference's IndexError
    with pytest.raises(_lib.HopError, match="t_max > n_alloc"):
        _wide(dev, P, Nn + 1)
    # an empty batch
    Je, se = engine.bruteforce_jcurve_wide(*[_t(x, dev)[:0] for x in P[:4]],
                                           *[_t(x[0], dev) for x in P[4:9]], Nn)
    assert tuple(Je.shape) == (0, Nn) and tuple(se.shape) == (0, Nn)
    assert Je.dtype == torch.float64 and se.dtype == torch.int32
    # float64 only
    with pytest.raises(ValueError, match="float64"):
        engine.bruteforce_jcurve_wide(*[_t(x, dev).to(torch.float32) for x in P[:9]], Nn)


# 6 -------------------------------------------------------------------------
def test_wide_jcurve_dropin(dev):
    """horizon_selection.bruteforce_all_Jt_backward_expansion routes n = 20 to the wide
    entry: the curve, an extra_stage_cost callable, and the reference's LinAlgError"""
    from time_opt_ilqr_amd import horizon_selection as hs
    n, m, Nn = 20, 3, 8
    A, B, X, U, xg, ur, Q, R, alpha = orc.synth_riccati_problem(8700, n, m, Nn)
    M = np.random.default_rng(8701).standard_normal((n, n))
    H = 0.05 * (M @ M.T / n)
    g = 0.1 * np.random.default_rng(8702).standard_normal(n)

    def extra(x, u):
        return 0.5 * float(x @ H @ x) + float(g @ x) + 0.2, H @ x + g, H

    for ex in (None, extra):
        J = hs.bruteforce_all_Jt_backward_expansion(list(A), list(B), X, U, xg, ur, Q, R, alpha,
                                                    0.3, Nn, wrap_idx=[1], extra_stage_cost=ex)
        Jo = orc.bruteforce_J(list(A), list(B), X, U, xg, ur, Q, R, alpha, 0.3, Nn, wrap_idx=[1],
                              extra=ex)
        err = _elem_rel(J, Jo)
        print("drop-in", "extra" if ex else "plain", f"{err:.3e}")
        assert J.shape == (Nn,) and err <= 1e-6
    with pytest.raises(np.linalg.LinAlgError):
        hs.bruteforce_all_Jt_backward_expansion(list(A), list(B), X, U, xg, ur, Q,
                                                -50.0 * np.eye(m), alpha, 0.3, Nn)
    with pytest.raises(IndexError):
        hs.bruteforce_all_Jt_backward_expansion(list(A), list(B), X, U, xg, ur, Q, R, alpha, 0.3,
                                                Nn + 1)


# 7 -------------------------------------------------------------------------
def _chain_dynamics(n, m, dt):
    """the mass-spring chain of tests/golden/make_golden_wide_bf.py (same expressions)"""
    p = n // 2
    act = [j * p // m for j in range(m)]
    k, ks, c = 2.0, 0.5, 0.3

    def F(x, u):
        x = np.asarray(x, dtype=float).reshape(-1)
        u = np.asarray(u, dtype=float).reshape(-1)
        q, v = x[:p], x[p:]
        ext = np.concatenate(([0.0], q, [0.0]))
        d = np.diff(ext)
        f = k * d + ks * np.sin(d)
        acc = f[1:] - f[:-1] - c * v
        for j, i in enumerate(act):
            acc[i] += u[j]
        return np.concatenate((q + dt * v, v + dt * acc))

    return F


def _fixture(golden_dir, n, trial):
    d = np.load(os.path.join(golden_dir, f"wide_bf_solve_n{n}_{trial}.npz"))
    assert float(d["gaps"].min()) >= 1e-3
    return d


@pytest.mark.parametrize("n", [18, 24, 30])
def test_wide_bruteforce_solver_vs_reference(dev, golden_dir, n):
    """solver.ilqr_timeopt(F=callable, method="bruteforce") against the reference's own
    solves (wide_bf_solve_*.npz; every select of every stored trial has an argmin gap
    >= 1e-3): T_hist exactly, J_hist to 1e-6 (the bar of test_wide_solver_vs_reference),
    the last J curve over [T_min, T_max] to 1e-8 (the bar of the narrow
    test_ilqr_bruteforce_outer_loop_vs_reference)"""
    from time_opt_ilqr_amd import solver
    for trial in range(3):
        d = _fixture(golden_dir, n, trial)
        m = int(d["m"])
        F = _chain_dynamics(n, m, float(d["dt"]))
        args = (F, d["x0"], d["xg"], d["u_ref"], d["Q"], d["R"], float(d["alpha"]), float(d["w"]),
                int(d["N"]), int(d["T_min"]), int(d["T_max"]))
        sols = [solver.ilqr_timeopt(*args, method="bruteforce", max_iter=int(d["max_iter"]))]
        if trial == 0:
            sols.append(solver.ilqr_timeopt_baseline1(*args, max_iter=int(d["max_iter"])))
        lo, hi = int(d["T_min"]) - 1, int(d["T_max"])
        for sol in sols:
            eh = _elem_rel(np.asarray(sol["J_hist"]), d["J_hist"]) if len(
                sol["J_hist"]) == len(d["J_hist"]) else float("nan")
            ec = _elem_rel(sol["J_curve"][lo:hi], d["J_curve"][lo:hi])
            print(f"n={n} trial={trial}: T_hist {sol['T_hist']}, J_hist relative error {eh:.3e}, "
                  f"J_curve relative error {ec:.3e}")
            assert list(sol["T_hist"]) == d["T_hist"].tolist(), (trial, sol["T_hist"])
            assert eh <= 1e-6
            assert sol["J_curve"].shape == d["J_curve"].shape
            assert ec <= 1e-8


# 8 -------------------------------------------------------------------------
def test_wide_bruteforce_batched_solve(dev, golden_dir):
    """the three n = 24 fixtures as one batch of ilqr_timeopt_batch(HostDynamics)"""
    from time_opt_ilqr_amd import host_dynamics, solver
    from time_opt_ilqr_amd.utils import as_terminal_weight
    n = 24
    ds = [_fixture(golden_dir, n, i) for i in range(3)]
    d = ds[0]
    m = int(d["m"])
    system = host_dynamics.HostDynamics(_chain_dynamics(n, m, float(d["dt"])), n, m)
    res = solver.ilqr_timeopt_batch(
        system, np.stack([x["x0"] for x in ds]), d["xg"], d["u_ref"], d["Q"], d["R"],
        as_terminal_weight(float(d["alpha"]), n), float(d["w"]), int(d["N"]), int(d["T_min"]),
        int(d["T_max"]), max_iter=int(d["max_iter"]), method="bruteforce")
    assert _np(res["crashed"]).tolist() == [0, 0, 0]
    nh = _np(res["n_hist"])
    for b, x in enumerate(ds):
        k = int(nh[b])
        assert _np(res["T_hist"])[b, :k].tolist() == x["T_hist"].tolist(), b
        err = _elem_rel(_np(res["J_hist"])[b, :k], x["J_hist"])
        print(f"batched n=24 problem {b}: J_hist relative error {err:.3e}")
        assert err <= 1e-6


# 9 -------------------------------------------------------------------------
def test_integration_md_wide_jcurve_ctypes_stub_runs(dev):
    """INTEGRATION.md's stub for the new entry runs as written at n = 17 and agrees bit
    for bit with engine.bruteforce_jcurve_wide"""
    from time_opt_ilqr_amd import _lib, engine
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(repo, "INTEGRATION.md")).read()
    blocks = [b for b in re.findall(r"```python\n(.*?)```", text, re.S)
              if "hop_bruteforce_jcurve_wide_f64" in b]
    assert len(blocks) == 1
    for other in ("hop_lft_sweep_wide_f64", "hop_lft_sweep_f64", "hop_bruteforce_jcurve_f64",
                  "hop_bruteforce_jcurve_legacy_f64"):
        assert other not in blocks[0]
    ns = {}
    code = blocks[0].replace("/path/to/time_opt_ilqr_amd/libhop_amd.so", _lib.LIB_PATH)
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    n, m, Nn = 17, 2, 8
    A, B, X, U, xg, ur, Q, R, Qf, alpha = (np.array(x) for x in _problems(n, m, Nn, 2))
    J, st = ns["bruteforce_all_Jt_wide_batched"](A, B, X, U, xg[0], ur[0], Q[0], R[0], Qf[0], Nn,
                                                 0.3)
    Je, se = engine.bruteforce_jcurve_wide(*[_t(x, dev) for x in (A, B, X, U, xg[0], ur[0], Q[0],
                                                                   R[0], Qf[0])], Nn, w_stage=0.3)
    assert np.array_equal(J, _np(Je)) and np.array_equal(st, _np(se))
    assert (st == 0).all() and np.isfinite(J).all()
