"""No kernel may depend on what the kernel before it left in LDS.

LDS keeps its contents from one kernel to the next, and every other GPU test runs on
whatever the previous test left there (finite data, in practice).  Here each kernel runs
after the test hooks of include/hop_testhooks.h have written a known 64-bit pattern over
the LDS of every compute unit:

  0x0000000000000000  the baseline
  0xFFFFFFFFFFFFFFFF  NaN as f64 and as f32, -1 as an integer
  0x7FE0000000000000  a huge finite f64: 0 x it and sums with it stay finite, but wrong

and every case asserts
  * the witness: after a fill, a scan launched with the geometry of the kernel under test
    (for kernels whose LDS size is chosen at launch: a whole compute unit's LDS, which
    covers any allocation) finds the pattern in every word of at least 0.9 of its
    workgroups (expected 1.0; printed) -- a fill that did not land must not let a case
    pass vacuously;
  * bitwise invariance: outputs and status words after the two non-zero patterns equal
    those after the zero pattern bit for bit (the kernels are deterministic);
  * the oracle: the zero-pattern outputs meet the bars the existing tests of that entry
    use, and healthy problems have status 0.
"""
import functools

import numpy as np
import pytest

from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

PATTERNS = (0x0000000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FE0000000000000)
GROUPS_PER_CU = 2
WIDE = (128, 48128)         # threads, LDS bytes of lft_wide_kernel / riccati_wide_kernel
AUG_WIDE = (256, 38912)     # augment_kernel<double, 32>
AUG_NARROW = (256, 20480)   # augment_kernel<double, 16>
WHOLE_CU = (256, 163840)    # covers every allocation (LDS size chosen at launch)
N, BN = 6, 5                # batches of 5: the last wide workgroup has an idle wave
SENTINEL = 7.25             # what the outputs hold before a launch writes them


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.array(x, order="C"), dtype=dtype or torch.float64, device=dev)


def _np(t):
    return t.cpu().numpy()


def _rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _bits(t):
    import torch
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    return t


def run_poisoned(dev, fn, geom, groups, patterns=PATTERNS, reset=None):
    """For each pattern: fill, scan at `geom` = (threads, lds_bytes) with `groups`
    workgroups, fill again, fn().  fn returns a dict of device tensors (None entries are
    dropped); reset(), if given, runs before the first fill (it may launch kernels).
    Asserts the witness and the bitwise invariance; returns the zero-pattern outputs."""
    import torch
    from time_opt_ilqr_amd import _lib
    lib = _lib.load()
    stream = _lib.stream_handle(dev)
    threads, lds_bytes = geom
    flags = torch.empty((groups,), dtype=torch.int32, device=dev)
    runs = []
    for pat in patterns:
        flags.fill_(-1)
        if reset is not None:
            reset()
        torch.cuda.synchronize()
        _lib.check(lib.hop_test_lds_fill(pat, GROUPS_PER_CU, stream))
        _lib.check(lib.hop_test_lds_scan(pat, lds_bytes, threads, groups, _lib.ptr(flags), stream))
        _lib.check(lib.hop_test_lds_fill(pat, GROUPS_PER_CU, stream))
        out = fn()
        torch.cuda.synchronize()
        f = _np(flags)
        assert set(f.tolist()) <= {0, 1}, f  # every scan group reported
        share = float((f == 1).mean())
        print(f"pattern {pat:#018x}: witness share {share:.3f} of {groups} groups "
              f"({threads} threads, {lds_bytes} B)")
        assert share >= 0.9, (hex(pat), share)
        runs.append({k: v.clone() for k, v in out.items() if v is not None})
    torch.cuda.synchronize()
    base = runs[0]
    differ = []
    for pat, r in zip(patterns[1:], runs[1:]):
        assert r.keys() == base.keys()
        for k in base:
            if not torch.equal(_bits(r[k]), _bits(base[k])):
                differ.append((hex(pat), k))
                if k == "status":
                    print(f"pattern {pat:#018x}: status {_np(r[k]).tolist()} "
                          f"unpoisoned {_np(base[k]).tolist()}")
    assert not differ, differ
    return base


# ---------------------------------------------------------------------------
# the wide family: LFT sweep
# ---------------------------------------------------------------------------
def _sweep_fn(dev, A, Bm, Q, Ri, z0, QT, direct):
    """engine.propagate with every output, or (direct) hop_lft_sweep_wide_f64 itself: the
    engine routes s <= 16 to the narrow kernels"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, Nn, s, _ = A.shape
    m = Bm.shape[-1]
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0, QT)]
    if not direct:
        def fn():
            r = engine.propagate(*args, t_min=2, t_max=Nn, return_efg=True, return_prefix=True)
            return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star, efg=r.efg,
                        prefix=r.prefix)
        return fn, None
    lib = _lib.load()
    tA, tB, tQ, tR, tz, tQT = args
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(J=torch.empty((Bn, Nn), **f64), status=torch.empty((Bn,), dtype=torch.int32, device=dev),
               t_star=torch.empty((Bn,), dtype=torch.int32, device=dev),
               j_star=torch.empty((Bn,), **f64), efg=torch.empty((Bn, Nn, 3, s, s), **f64),
               prefix=torch.empty((Bn, Nn, 3, s, s), **f64))

    def reset():
        for v in out.values():
            v.fill_(7)

    def fn():
        _lib.check(lib.hop_lft_sweep_wide_f64(
            _lib.ptr(tA), _lib.ptr(tB), _lib.ptr(tQ), _lib.ptr(tR), m * m, 0, 1, _lib.ptr(tQT),
            _lib.ptr(tz), 0, Bn, Nn, Nn, s, m, 8, 2, Nn, _lib.ptr(out["J"]),
            _lib.ptr(out["status"]), _lib.ptr(out["t_star"]), _lib.ptr(out["j_star"]),
            _lib.ptr(out["efg"]), _lib.ptr(out["prefix"]), _lib.stream_handle(dev)))
        return out
    return fn, reset


@pytest.mark.parametrize("s", [16, 17, 20, 21, 24, 25, 28, 29, 32])  # both ends of every HR
def test_poisoned_wide_sweep(dev, s):
    m = 3
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(9100 + s, BN, s, m, N)
    fn, reset = _sweep_fn(dev, A, Bm, Q, Ri, z0[0], QT, direct=(s == 16))
    base = run_poisoned(dev, fn, WIDE, (BN + 1) // 2, reset=reset)
    assert _np(base["status"]).tolist() == [0] * BN
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
    assert sto.tolist() == [0] * BN
    err = _elem_rel(_np(base["J"]), Jo)
    print(f"s={s}: J elementwise relative error {err:.3e}")
    assert err <= 1e-9
    To, _ = orc.select_horizon(Jo, 2, N)
    assert _np(base["t_star"]).tolist() == To.tolist()
    efg, pre = _np(base["efg"]), _np(base["prefix"])
    for b in range(BN):
        o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b], want_efg=True, want_prefix=True)
        for i, key in enumerate(("E", "F", "G")):
            assert _rel(efg[b, :, i], o[key]) <= 1e-9, (b, key)
        for i, key in enumerate(("Ebar", "Fbar", "Gbar")):
            assert _rel(pre[b, :, i], o[key]) <= 1e-9, (b, key)


@pytest.mark.parametrize("s", [17, 20])
def test_poisoned_wide_sweep_status_paths(dev, s):
    """the recipe of test_wide_status_bits_and_nonfinite: the jitter retries and the LU
    slot re-read the parked image; the NaN horizon must flag exactly what it flags
    unpoisoned (the bitwise comparison of status and J)"""
    m = 3
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(900, BN, s, m, N)
    Q, QT = Q.copy(), QT.copy()
    Q[0, 2] = Q[0, 2] - np.eye(s) * (np.linalg.eigvalsh(Q[0, 2]).min() + 5e-8)  # needs jitter
    Q[1, 3] = -np.eye(s)                                                     # LU slot
    QT[2, 4, 0, 0] = np.nan
    fn, _ = _sweep_fn(dev, A, Bm, Q, Ri, z0[0], QT, direct=False)
    base = run_poisoned(dev, fn, WIDE, (BN + 1) // 2)
    st, J = _np(base["status"]), _np(base["J"])
    o = [orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b]) for b in range(BN)]
    print("status", st.tolist(), "oracle", [x["status"] for x in o])
    assert st[0] & orc.ST_JITTER and not st[0] & orc.ST_LU and o[0]["status"] & orc.ST_JITTER
    assert st[1] & orc.ST_LU and o[1]["status"] & orc.ST_LU
    assert st[2] & orc.ST_NONFINITE
    assert np.isnan(J[2, 4]) and np.isfinite(np.delete(J[2], 4)).all()
    assert st[3:].tolist() == [0, 0]
    assert _elem_rel(J[0, :2], o[0]["J"][:2]) <= 1e-6
    assert np.isfinite(J[1]).all() and _elem_rel(J[1], o[1]["J"]) <= 1e-6
    assert _elem_rel(J[3:], np.stack([o[3]["J"], o[4]["J"]])) <= 1e-9


# ---------------------------------------------------------------------------
# the wide family: Riccati passes and the J curve
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ric_problems(n, m, Nn=N, Bn=BN, seed=9300):
    probs = [orc.synth_riccati_problem(seed + 10 * n + i, n, m, Nn) for i in range(Bn)]
    A, B, X, U, xg, ur, Q, R = (np.stack([p[j] for p in probs]) for j in range(8))
    alpha = np.array([p[8] for p in probs])
    Qf = np.stack([orc.terminal_weight(a, n) for a in alpha])
    out = (A, B, X, U, xg, ur, Q, R, Qf, alpha)
    for x in out:
        x.setflags(write=False)
    return out


def _extra(P, n, Bn=BN, Nn=N):
    """the extra stage cost of test_wide_riccati_vs_oracle: PSD cxx, cx and c per
    (problem, step), and the oracle's callables for it"""
    rng = np.random.default_rng(6)
    M = rng.standard_normal((Bn, Nn, n, n))
    cxx = 0.05 * M @ M.transpose(0, 1, 3, 2) / n
    cx = 0.1 * rng.standard_normal((Bn, Nn, n))
    c0 = rng.uniform(0.0, 0.5, (Bn, Nn))

    def make(b):
        Xb = P[2][b]
        return lambda x, u: (lambda k: (c0[b, k], cx[b, k], cxx[b, k]))(
            int(np.argmin(np.abs(Xb[:Nn] - x).sum(axis=1))))
    return (cxx, cx, c0), [make(b) for b in range(Bn)]


def _riccati_fn(dev, entry, P, T, lm, mode, w_stage, wrap, ex=None, reg_max_tries=12):
    """hop_riccati_wide_f64 / hop_riccati_f64 called directly with every V output, on
    outputs that hold SENTINEL wherever the pass does not write"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    lib = _lib.load()
    A, B, X, U, xg, ur, Q, R, Qf = (_t(x, dev) for x in P[:9])
    Bn, Nn, n, _ = A.shape
    m = B.shape[-1]
    ext = [None] * 3 if ex is None else [_t(x, dev) for x in ex]
    hz = torch.as_tensor(np.asarray(T, dtype=np.int32), device=dev)
    lmt = torch.full((Bn,), lm, dtype=torch.float64, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = dict(K=torch.empty((Bn, Nn, m, n), **f64), k=torch.empty((Bn, Nn, m), **f64),
               Vxx=torch.empty((Bn, Nn + 1, n, n), **f64), Vx=torch.empty((Bn, Nn + 1, n), **f64),
               V0=torch.empty((Bn, Nn + 1), **f64),
               status=torch.empty((Bn,), dtype=torch.int32, device=dev))
    wm = engine.wrap_mask(wrap, n)

    def reset():
        for v in out.values():
            v.fill_(SENTINEL if v.dtype == torch.float64 else -7)

    def fn():
        _lib.check(getattr(lib, entry)(
            _lib.ptr(A), _lib.ptr(B), _lib.ptr(X), _lib.ptr(U), _lib.ptr(xg), n, _lib.ptr(ur), m,
            _lib.ptr(Q), n * n, _lib.ptr(R), m * m, _lib.ptr(Qf), n * n, _lib.ptr(ext[0]),
            _lib.ptr(ext[1]), _lib.ptr(ext[2]), _lib.ptr(hz), _lib.ptr(lmt), float(w_stage), wm,
            mode, reg_max_tries, Bn, Nn, n, m, _lib.ptr(out["K"]), _lib.ptr(out["k"]), _lib.ptr(out["Vxx"]),
            _lib.ptr(out["Vx"]), _lib.ptr(out["V0"]), _lib.ptr(out["status"]),
            _lib.stream_handle(dev)))
        return out
    return fn, reset


def _check_riccati_oracle(base, P, T, lm, mode, w_stage, wrap, exo, healthy):
    from gain_check import assert_per_step
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    for i in healthy:
        Ti = int(T[i])
        if mode == 0:
            ks, Ks, ok, Vxxs, Vxs = orc.riccati_truncated(
                list(A[i]), list(B[i]), X[i], U[i], xg[i], ur[i], Q[i], R[i], alpha[i], Ti,
                lm_lambda=lm, wrap_idx=wrap, want_v=True, extra=exo[i])
            assert ok
            V0 = None
        else:
            Vxxs, Vxs, V0, Ks, ks = orc.riccati_expand(
                list(A[i]), list(B[i]), X[i], U[i], xg[i], ur[i], Q[i], R[i], alpha[i], Ti, 0,
                lm_lambda=lm, w_stage=w_stage, wrap_idx=wrap, extra=exo[i])
        assert_per_step(_np(base["k"][i, :Ti]), np.array(ks), 1e-6, f"{i} k")
        assert_per_step(_np(base["K"][i, :Ti]), np.array(Ks), 1e-6, f"{i} K")
        assert_per_step(_np(base["Vxx"][i, :Ti + 1]), np.array(Vxxs), 1e-6, f"{i} Vxx")
        assert_per_step(_np(base["Vx"][i, :Ti + 1]), np.array(Vxs), 1e-6, f"{i} Vx")
        if V0 is not None:
            assert_per_step(_np(base["V0"][i, :Ti + 1]), np.array(V0), 1e-6, f"{i} V0")
        # nothing is written past the horizon
        assert (_np(base["K"][i, Ti:]) == SENTINEL).all()
        assert (_np(base["Vxx"][i, Ti + 1:]) == SENTINEL).all()


# n = 16: HR = 8 (through the C entry: the engine routes it to the narrow kernels);
# 17 and 24: HR = 12; 25 and 31: HR = 16
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n,m,extra", [(16, 8, False), (17, 1, False), (24, 16, True),
                                       (25, 8, False), (31, 16, False)])
def test_poisoned_wide_riccati(dev, n, m, extra, mode):
    P = list(_ric_problems(n, m))
    R = P[7].copy()
    R[4] = -np.eye(m) * 50.0  # negative definite: a genuine ST_FAIL beside the healthy ones
    P[7] = R
    T = np.array([1, 2, N // 2, N, N], dtype=np.int32)
    wrap, lm, w_stage = [1], 1e-3, (0.3 if mode == 1 else 0.0)
    ex, exo = _extra(P, n) if extra else (None, [None] * BN)
    # mode 1 with one regularisation attempt: the lambda escalation would rescue the
    # negative-definite R (the healthy problems need none: their status is 0)
    fn, reset = _riccati_fn(dev, "hop_riccati_wide_f64", P, T, lm, mode, w_stage, wrap, ex,
                            reg_max_tries=12 if mode == 0 else 1)
    base = run_poisoned(dev, fn, WIDE, (BN + 1) // 2, reset=reset)
    st = _np(base["status"])
    print(f"n={n} m={m} mode={mode}: status {st.tolist()}")
    assert st[:4].tolist() == [0] * 4
    assert st[4] & orc.ST_FAIL and not st[4] & orc.ST_NONFINITE
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    bad = (list(A[4]), list(B[4]), X[4], U[4], xg[4], ur[4], Q[4], R[4], alpha[4], int(T[4]))
    if mode == 0:
        assert orc.riccati_truncated(*bad, lm_lambda=lm, wrap_idx=wrap, extra=exo[4])[2] is False
    else:
        with pytest.raises(np.linalg.LinAlgError):
            orc.riccati_expand(*bad, 0, lm_lambda=lm, w_stage=w_stage, wrap_idx=wrap,
                               extra=exo[4], reg_max_tries=1)
    _check_riccati_oracle(base, P, T, lm, mode, w_stage, wrap, exo, range(4))


@pytest.mark.parametrize("n,m", [(17, 4), (24, 16), (31, 8)])
def test_poisoned_wide_jcurve(dev, n, m):
    from time_opt_ilqr_amd import engine
    P = _ric_problems(n, m)
    args = [_t(x, dev) for x in P[:9]]
    wrap, lm, w_stage = [1], 1e-6, 0.7

    def fn():
        J, st = engine.bruteforce_jcurve_wide(*args, N, lm_lambda=lm, w_stage=w_stage,
                                              wrap_idx=wrap)
        return dict(J=J, status=st)
    base = run_poisoned(dev, fn, WIDE, (BN * N + 1) // 2)
    st = _np(base["status"])
    print(f"n={n} m={m}: per-horizon status {st.tolist()}")
    assert (st == 0).all()
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    Jo = np.stack([orc.bruteforce_J(list(A[b]), list(B[b]), X[b], U[b], xg[b], ur[b], Q[b], R[b],
                                    float(alpha[b]), w_stage, N, lm_lambda=lm, wrap_idx=wrap)
                   for b in range(BN)])
    err = _elem_rel(_np(base["J"]), Jo)
    print(f"n={n} m={m}: J max elementwise relative error {err:.3e}")
    assert err <= 1e-6  # the bar of test_wide_jcurve_vs_oracle


# ---------------------------------------------------------------------------
# the builders (augment.hip), wide and narrow, and the fused trajectory form
# ---------------------------------------------------------------------------
def _traj_batch(seeds, n, m, Nn):
    ps = [orc.synth_traj_problem(int(s), n, m, Nn) for s in seeds]
    st = {k: np.stack([p[k] for p in ps]) for k in ("A", "B", "a_res", "X", "U", "xg", "u_ref",
                                                     "Q", "R", "alpha", "w")}
    st["P"] = np.stack([orc.terminal_weight(p["alpha"], n) for p in ps])
    st["R_inv"] = np.stack([orc.spd_inverse(orc.sym(p["R"]))[0] for p in ps])
    st["wrap_idx"] = ps[0]["wrap_idx"]
    return ps, st


def _traj_blocks(p, rho):
    Aa, Ba, Qa, _, z0, Ri = orc.augment_stage(list(p["A"]), list(p["B"]), p["a_res"], p["X"],
                                              p["U"], p["xg"], p["u_ref"], p["Q"], p["R"],
                                              p["w"], wrap_idx=p["wrap_idx"], rho_reg=rho)
    QT = orc.augment_terminal(p["X"], p["xg"], p["alpha"], wrap_idx=p["wrap_idx"], rho_reg=rho)
    return Aa, Ba, Qa, Ri, z0, QT


@pytest.mark.parametrize("n,m", [(16, 4), (24, 6), (31, 8), (4, 1)])  # (4, 1): the narrow builder
def test_poisoned_augment(dev, n, m):
    from time_opt_ilqr_amd import engine
    ps, st = _traj_batch(range(900, 900 + BN), n, m, N)
    args = [_t(st[k], dev) for k in ("A", "B", "a_res", "X", "U", "xg", "u_ref", "Q")]
    P, w = _t(st["P"], dev), _t(st["w"], dev)

    def fn():
        o = engine.augment(*args, P, w, wrap_idx=st["wrap_idx"])
        return dict(A=o.A, B=o.B, Q=o.Q, QT=o.QT, z0=o.z0)
    base = run_poisoned(dev, fn, AUG_WIDE if n >= 16 else AUG_NARROW, BN)
    for b, p in enumerate(ps):
        Aa, Ba, Qa, Ri, z0, QT = _traj_blocks(p, 1e-12)
        for name, ref in (("A", Aa), ("B", Ba), ("Q", Qa), ("QT", QT)):
            assert _rel(_np(base[name][b]), ref) <= 1e-14, (b, name)
    assert _np(base["z0"]).tolist() == [0.0] * n + [1.0]


def test_poisoned_wide_trajectory_form(dev):
    from time_opt_ilqr_amd import engine
    n, m = 24, 6
    ps, st = _traj_batch(range(900, 900 + BN), n, m, N)
    args = [_t(st[k], dev) for k in ("A", "B", "a_res", "X", "U", "xg", "u_ref", "Q")]
    Ri, P, w = _t(st["R_inv"], dev), _t(st["P"], dev), _t(st["w"], dev)

    def fn():
        r = engine.propagate_traj(*args, Ri, P, w, wrap_idx=st["wrap_idx"], rho_reg=1.0,
                                  t_min=2, t_max=N)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_poisoned(dev, fn, WIDE, (BN + 1) // 2)
    Jref = np.stack([orc.lft_sweep(*_traj_blocks(p, 1.0), N)["J"] for p in ps])
    print("J max-norm relative", _rel(_np(base["J"]), Jref))
    assert _rel(_np(base["J"]), Jref) <= 1e-9
    assert (_np(base["status"]) == 0).all()
    Tref, _ = orc.select_horizon(Jref, 2, N)
    assert _np(base["t_star"]).tolist() == Tref.tolist()


# ---------------------------------------------------------------------------
# breadth: one poisoned case for every other source that declares LDS
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("generic", [False, True])
def test_poisoned_narrow_sweep_s13(dev, generic):
    """lft_sweep_v2.hip (the conditioned default) and lft_sweep.hip (force_generic) at the
    smoke run's shape"""
    from time_opt_ilqr_amd import _lib, engine
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(42, 5, 13, 4, 24)
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]

    def fn():
        with _lib.options(force_generic=generic):
            r = engine.propagate(*args, t_min=5, t_max=24)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_poisoned(dev, fn, WHOLE_CU, 2)
    Jo, _ = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
    assert _elem_rel(_np(base["J"]), Jo) <= 1e-6
    assert _np(base["status"]).tolist() == [0] * 5
    assert _np(base["t_star"]).tolist() == orc.select_horizon(Jo, 5, 24)[0].tolist()


def test_poisoned_small_sweep_tile64(dev):
    """lft_small.hip: s = 5, m = 1 fp32 in the tile64 layout, with a jitter and an LU-slot
    problem; a batch that is no multiple of the 64-lane wave"""
    import torch
    from time_opt_ilqr_amd import engine
    Bn, Nn, s, m = 70, 20, 5, 1
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(905, Bn, s, m, Nn)
    Q = Q.copy()
    Q[7, 3] = Q[7, 3] - np.eye(s) * (np.linalg.eigvalsh(Q[7, 3]).min() + 5e-7)  # jitter
    Q[65, 5] = -np.eye(s)                                                   # LU slot
    tA, tB, tQ, tR, tz, tQT = (_t(x, dev, torch.float32) for x in (A, Bm, Q, Ri, z0[0], QT))
    At, Bt, Qt, QTt = (engine.to_tile64(x) for x in (tA, tB, tQ, tQT))

    def fn():
        r = engine.propagate(At, Bt, Qt, tR, tz, QTt, t_min=3, t_max=Nn)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_poisoned(dev, fn, WHOLE_CU, 2)
    ss = _np(base["status"])
    assert ss[7] & orc.ST_JITTER and ss[65] & orc.ST_LU
    ok = [i for i in range(Bn) if i not in (7, 65)]
    Jo, _ = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
    assert _elem_rel(_np(base["J"]).astype(float)[ok], Jo[ok]) <= 2e-3  # the fp32 bar


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_poisoned_narrow_riccati(dev, mode, generic):
    """riccati_fast.hip (the default at fp64) and riccati.hip (force_generic), n = 12, m = 4"""
    from time_opt_ilqr_amd import _lib
    n, m = 12, 4
    P = _ric_problems(n, m)
    T = np.array([1, 2, N // 2, N, N], dtype=np.int32)
    wrap, lm, w_stage = [1], 1e-3, (0.3 if mode == 1 else 0.0)
    call, reset = _riccati_fn(dev, "hop_riccati_f64", P, T, lm, mode, w_stage, wrap)

    def fn():
        with _lib.options(force_generic=generic):
            return call()
    base = run_poisoned(dev, fn, WHOLE_CU, 2, reset=reset)
    assert _np(base["status"]).tolist() == [0] * BN
    _check_riccati_oracle(base, P, T, lm, mode, w_stage, wrap, [None] * BN, range(BN))


@pytest.mark.parametrize("generic", [False, True])
def test_poisoned_narrow_jcurve(dev, generic):
    from time_opt_ilqr_amd import _lib, engine
    n, m = 12, 4
    P = _ric_problems(n, m)
    args = [_t(x, dev) for x in P[:9]]
    wrap, lm, w_stage = [1], 1e-6, 0.7

    def fn():
        with _lib.options(force_generic=generic):
            J, st = engine.bruteforce_jcurve(*args, N, lm_lambda=lm, w_stage=w_stage,
                                             wrap_idx=wrap)
        return dict(J=J, status=st)
    base = run_poisoned(dev, fn, WHOLE_CU, 4)
    assert (_np(base["status"]) == 0).all()
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    Jo = np.stack([orc.bruteforce_J(list(A[b]), list(B[b]), X[b], U[b], xg[b], ur[b], Q[b], R[b],
                                    float(alpha[b]), w_stage, N, lm_lambda=lm, wrap_idx=wrap)
                   for b in range(BN)])
    assert _elem_rel(_np(base["J"]), Jo) <= 1e-6


def test_poisoned_linearize(dev):
    """linearize.hip: the segway (no libm call: bit-exact against the oracle), a ragged
    batch that is no multiple of the 64-step tile"""
    from oracle import dyn_oracle as dyn
    from time_opt_ilqr_amd import engine
    sid, Bn, Nn = 4, 5, 29
    n, m = dyn.DIMS[sid]
    rng = np.random.default_rng(504)
    X = 1.5 * rng.standard_normal((Bn, Nn + 1, n))
    U = 1.5 * rng.standard_normal((Bn, Nn, m))
    dt = dyn.DEFAULT_DT[sid]
    Xt, Ut = _t(X, dev), _t(U, dev)
    for central in (False, True):
        def fn():
            r = engine.linearize(sid, Xt, Ut, dt, central=central)
            return dict(A=r.A, B=r.B, a_res=r.a_res)
        base = run_poisoned(dev, fn, (256, 5888), (Bn * Nn + 63) // 64)
        ref = dyn.linearize(sid, X, U, dt, central=central)
        for key, r in zip(("A", "B", "a_res"), ref):
            assert np.array_equal(_np(base[key]), r, equal_nan=True), (central, key)


def test_poisoned_forward_linesearch(dev):
    """forward.hip: the smoke run's double-integrator line search"""
    from oracle import ilqr_oracle as io
    from time_opt_ilqr_amd import engine
    rng = np.random.default_rng(7)
    Nn, Bn, dt = 20, 3, 0.05
    U = 0.1 * rng.standard_normal((Bn, Nn, 1))
    X = np.stack([io.rollout(0, dt, np.array([1.0, 0.0]), U[b]) for b in range(Bn)])
    K = -0.5 * np.ones((Bn, Nn, 1, 2))
    k = -0.2 * (X[:, :Nn, :1] - 2.0)
    xg, ur, Q, R, Qf = np.array([2.0, 0.0]), np.zeros(1), np.diag([1.0, 0.1]), np.eye(1) * 1e-2, \
        np.eye(2) * 50.0
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), 0.02)
    Xt, Ut, Kt, kt = (_t(x, dev) for x in (X, U, K, k))

    def fn():
        r = engine.forward_linesearch(0, Xt, Ut, [Nn] * Bn, Kt, kt, cost, dt)
        return dict(X=r.X, U=r.U, J=r.J, J_old=r.J_old, accepted=r.accepted)
    base = run_poisoned(dev, fn, (64, 104), Bn)
    for b in range(Bn):
        _, _, Jo, _, ai = io.forward_linesearch(0, dt, X[b], U[b], xg, ur, Q, R, Qf, 0.02, Nn,
                                                k[b], K[b])
        assert int(base["accepted"][b]) == ai
        assert abs(float(base["J"][b]) - Jo) <= 1e-12 * max(1.0, abs(Jo))


def test_poisoned_chain_cost_and_linesearch(dev):
    """chain.hip: the true cost and the line search on test_gpu_chain's cases"""
    from test_gpu_chain import TRAJ_TOL, _chain, _dense_cost, _linesearch_case
    from time_opt_ilqr_amd import engine, host_dynamics
    p, m, Nn = 12, 3, 12
    rng = np.random.default_rng(123)
    xg, ur, Q, R, Qf, w = _dense_cost(p, m, rng)
    X = rng.uniform(-1, 1, (BN, Nn + 1, 2 * p))
    U = rng.uniform(-1, 1, (BN, Nn, m))
    T = np.array([1, 4, 7, Nn, Nn], dtype=np.int32)
    F = _chain(p, m)
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), w)
    Xt, Ut = _t(X, dev), _t(U, dev)
    base = run_poisoned(dev, lambda: dict(J=engine.cost_true(F, Xt, Ut, T, cost)), (256, 19840), 1)
    ref = np.array([host_dynamics.cost_true(X[b], U[b], xg, ur, Q, R, Qf, w, int(T[b]))
                    for b in range(BN)])
    assert _elem_rel(_np(base["J"]), ref) <= TRAJ_TOL

    c = _linesearch_case()
    F = c["F"]
    xg, ur, Q, R, Qf, w = c["cost"]
    cost = engine.CostParams(_t(xg, dev), _t(ur, dev), _t(Q, dev), _t(R, dev), _t(Qf, dev), w)
    Xt, Ut, Kt, kt = (_t(c[x], dev) for x in ("X", "U", "K", "k"))

    def fn():
        r = engine.forward_linesearch(F, Xt, Ut, c["T"], Kt, kt, cost, F.dt, active=c["active"])
        return dict(X=r.X, U=r.U, J=r.J, J_old=r.J_old, accepted=r.accepted)
    base = run_poisoned(dev, fn, (256, 19840), 6)
    Xo, Uo, J, J0, acc = c["ref"]
    assert _np(base["accepted"]).tolist() == acc.tolist()
    on = c["active"] != 0
    assert _elem_rel(_np(base["J"])[on], J[on]) <= TRAJ_TOL
    assert _elem_rel(_np(base["J_old"])[on], J0[on]) <= TRAJ_TOL


@pytest.mark.parametrize("central", [False, True])
def test_poisoned_chain_linearize(dev, central):
    """chain.hip's linearisation (the kernel that scrubs its LDS before it ends)"""
    from test_chain_cpu import check_lin
    from test_gpu_chain import _chain
    from time_opt_ilqr_amd import engine, host_dynamics
    p, m = 12, 3
    rng = np.random.default_rng(91 + p)
    Nn, n = 14, 2 * p
    X = rng.uniform(-1, 1, (BN, Nn + 1, n))
    U = rng.uniform(-1, 1, (BN, Nn, m))
    F = _chain(p, m)
    Xt, Ut = _t(X, dev), _t(U, dev)

    def fn():
        r = engine.linearize(F, Xt, Ut, F.dt, central=central)
        return dict(A=r.A, B=r.B, a_res=r.a_res)
    base = run_poisoned(dev, fn, (256, 6512), 4)
    ref = host_dynamics.linearize_batch(F.host(), X, U, central=central)
    check_lin(p, m, tuple(_np(base[k]) for k in ("A", "B", "a_res")), ref,
              "poisoned " + ("central" if central else "forward"))


def test_poisoned_onepass_rollout(dev, golden_dir):
    """onepass.hip: the rollout and its pick on the double integrator's stored case"""
    import os
    from test_gpu_onepass import _cost, _problem, _rel as rel
    from time_opt_ilqr_amd import engine
    tag, key = "di", "di_center"
    p = _problem(tag, golden_dir)
    F, Nn = p["F"], p["N"]
    d = np.load(os.path.join(golden_dir, "onepass_rollout_cases.npz"))
    X_ext, U_ext = d[tag + "_X_ext"], d[tag + "_U_ext"]
    n, m = X_ext.shape[1], U_ext.shape[1]
    T_bar, T_star, S = (int(v) for v in d[key + "_T"])
    K, k = np.zeros((S + Nn, m, n)), np.zeros((S + Nn, m))
    K[:T_bar + S], k[:T_bar + S] = d[key + "_K"], d[key + "_k"].reshape(T_bar + S, m)
    al = [float(a) for a in d[key + "_alphas"]]
    Xt, Ut, Kt, kt = (_t(x, dev)[None] for x in (X_ext, U_ext, K, k))
    cost = _cost(p, dev)

    def fn():
        r = engine.onepass_rollout(F.system_id, Xt, Ut, Kt, kt, cost, F.dt, [T_bar], [T_star], S,
                                   alphas=al)
        return dict(X=r.X, U=r.U, J=r.J, accepted=r.accepted)
    base = run_poisoned(dev, fn, (256, 8), 1)
    assert bool(d[key + "_ok"]) and int(base["accepted"][0]) >= 0
    Jr = float(d[key + "_J"])
    assert abs(float(base["J"][0]) - Jr) <= 1e-9 * abs(Jr)
    assert rel(_np(base["X"][0]), d[key + "_Xn"]) <= 1e-9
    assert rel(_np(base["U"][0]), d[key + "_Un"]) <= 1e-9
