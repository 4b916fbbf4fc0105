"""GPU parity: libhop_amd.so (through the C ABI) vs the CPU oracle / golden vectors.

Tolerances (north star: K_k / V_k / J to 1e-6 relative in fp64 on identical,
well-conditioned linearisations):
  * synthetic fp64 ............ max |got - ref| <= 1e-6 * max |ref| per array
                                (elementwise for J, which is > 0)
  * synthetic fp32 ............ 2e-3 relative, same T*
  * real linearisations ....... T* equal, J within 1e-3 (DI) / 5e-2 (Quadrotor):
    their terminal blocks have Schur complement 1e-12 (cond 1e14..1e21) and the
    reference itself moves J by up to 1e-5..1e0 under 1e-14 input perturbations
    (SURVEY.md section 0.2), so 1e-6 is not a meaningful bar there.
"""
import os

import numpy as np
import pytest

from gain_check import assert_per_step
from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

RTOL64 = 1e-6


def _t(x, dev, dtype=None):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float64, device=dev)


def _rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def _elem_rel(got, ref):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


# ---------------------------------------------------------------------------
# LFT sweep
# ---------------------------------------------------------------------------

SYNTH = ["s13_m4_N100", "s5_m1_N200", "s3_m1_N50", "s13_m4_N128", "s16_m6_N40"]


@pytest.mark.parametrize("tag", SYNTH)
def test_lft_synthetic_fp64_vs_reference(dev, golden_dir, tag):
    from time_opt_ilqr_amd import engine
    d = _load(golden_dir, f"lft_synth_{tag}.npz")
    s, m, N, bs, cnt = (int(d[k]) for k in ("s", "m", "N", "base_seed", "count"))
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(bs, cnt, s, m, N)
    res = engine.propagate(_t(A, dev), _t(Bm, dev), _t(Q, dev), _t(Ri, dev), _t(z0, dev),
                           _t(QT, dev), t_min=int(d["T_min"]), t_max=int(d["T_max"]),
                           return_efg=True)
    J = res.J.cpu().numpy()
    assert res.status.cpu().numpy().tolist() == [0] * cnt
    assert _elem_rel(J, d["J"]) <= RTOL64, _elem_rel(J, d["J"])
    assert res.t_star.cpu().numpy().tolist() == d["T_star"].tolist()
    efg = res.efg.cpu().numpy()
    k = d["E"].shape[1]
    for i, key in enumerate(("E", "F", "G")):
        assert _rel(efg[:, :k, i], d[key]) <= RTOL64, key


def test_lft_prefix_outputs_match_oracle(dev):
    from time_opt_ilqr_amd import engine
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_problem(11, 13, 4, 12)
    o = orc.lft_sweep(A, Bm, Q, Ri, z0, QT, want_prefix=True)
    res = engine.propagate(_t(A[None], dev), _t(Bm[None], dev), _t(Q[None], dev), _t(Ri, dev),
                           _t(z0, dev), _t(QT[None], dev), return_prefix=True)
    pre = res.prefix[0].cpu().numpy()
    for i, key in enumerate(("Ebar", "Fbar", "Gbar")):
        assert _rel(pre[:, i], o[key]) <= RTOL64, key


def test_lft_per_step_R_inverted_in_kernel(dev, golden_dir):
    from time_opt_ilqr_amd import engine
    d = _load(golden_dir, "lft_rlist_s7_m3_N30.npz")
    s, m, N = int(d["s"]), int(d["m"]), int(d["N"])
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_problem(int(d["seed"]), s, m, N)
    res = engine.propagate(_t(A[None], dev), _t(Bm[None], dev), _t(Q[None], dev),
                           _t(d["R_list"][None], dev), _t(z0, dev), _t(QT[None], dev),
                           r_is_inverse=False)
    assert _elem_rel(res.J[0].cpu().numpy(), d["J"]) <= RTOL64


@pytest.mark.parametrize("tag,jtol", [("DI_N50", 1e-3), ("Quad_N160", 5e-2)])
def test_lft_real_linearisations(dev, golden_dir, tag, jtol):
    from time_opt_ilqr_amd import engine
    d = _load(golden_dir, f"real_{tag}.npz")
    tmin, tmax = int(d["T_min"]), int(d["T_max"])
    for call in ("first", "last"):
        g = lambda k: d[f"p{call}_{k}"]  # noqa: E731
        res = engine.propagate(_t(g("A")[None], dev), _t(g("B")[None], dev),
                               _t(g("Q")[None], dev), _t(g("R_inv"), dev), _t(g("z0"), dev),
                               _t(g("QT")[None], dev), t_min=tmin, t_max=tmax)
        J = res.J[0].cpu().numpy()
        Jref = g("J")
        Tref, _ = orc.select_horizon(Jref, tmin, tmax)
        assert int(res.t_star[0]) == int(Tref), (call, int(res.t_star[0]), int(Tref))
        assert _elem_rel(J, Jref) <= jtol, (call, _elem_rel(J, Jref))


def test_lft_fp32_synthetic(dev, golden_dir):
    import torch
    from time_opt_ilqr_amd import engine
    d = _load(golden_dir, "lft_synth_s5_m1_N200.npz")
    s, m, N, bs, cnt = (int(d[k]) for k in ("s", "m", "N", "base_seed", "count"))
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(bs, cnt, s, m, N)
    f = lambda x: _t(x, dev, torch.float32)  # noqa: E731
    res = engine.propagate(f(A), f(Bm), f(Q), f(Ri), f(z0), f(QT),
                           t_min=int(d["T_min"]), t_max=int(d["T_max"]))
    assert _elem_rel(res.J.cpu().numpy(), d["J"]) <= 2e-3
    assert res.t_star.cpu().numpy().tolist() == d["T_star"].tolist()


def test_lft_padding_invariance(dev):
    """s=5 problems embedded block-diagonally into s=13, m=4 give the same J."""
    from time_opt_ilqr_amd import engine
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_problem(21, 5, 1, 30)
    N = 30
    P = lambda M, fill: np.stack([_embed(M[k], 13, 13, fill) for k in range(N)])  # noqa: E731
    Ap, Qp, QTp = P(A, 0.0), P(Q, 1.0), P(QT, 1.0)
    Bp = np.zeros((N, 13, 4))
    Bp[:, :4, :1] = Bm[:, :4, :]
    Bp[:, 12, :1] = Bm[:, 4, :]
    Rip = np.eye(4)
    Rip[0, 0] = Ri[0, 0]
    zp = np.zeros(13)
    zp[12] = 1.0
    r1 = engine.propagate(_t(A[None], dev), _t(Bm[None], dev), _t(Q[None], dev), _t(Ri, dev),
                          _t(z0, dev), _t(QT[None], dev))
    r2 = engine.propagate(_t(Ap[None], dev), _t(Bp[None], dev), _t(Qp[None], dev), _t(Rip, dev),
                          _t(zp, dev), _t(QTp[None], dev))
    assert _elem_rel(r2.J.cpu().numpy(), r1.J.cpu().numpy()) <= 1e-12


def _embed(M, s_out, m_out, fill):
    """Block-decoupled padding: real state dims keep indices, homogeneous coordinate last."""
    s = M.shape[0]
    out = np.zeros((s_out, m_out))
    n = s - 1
    out[:n, :n] = M[:n, :n]
    out[:n, -1] = M[:n, -1]
    out[-1, :n] = M[-1, :n]
    out[-1, -1] = M[-1, -1]
    for i in range(n, s_out - 1):
        out[i, i] = fill
    return out


def test_lft_batch_tail_permutation_and_prefix(dev):
    """B not a multiple of 16; permuting the batch permutes results bitwise;
    n_use < N reproduces the prefix of the full curve bitwise."""
    import torch
    from time_opt_ilqr_amd import engine
    Bn, s, m, N = 37, 13, 4, 20
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(500, Bn, s, m, N)
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    r1 = engine.propagate(*args)
    perm = np.random.default_rng(0).permutation(Bn)
    args_p = [_t(x[perm], dev) for x in (A, Bm, Q, Ri)] + [_t(z0[0], dev), _t(QT[perm], dev)]
    r2 = engine.propagate(*args_p)
    assert torch.equal(r2.J, r1.J[torch.as_tensor(perm, device=dev)])
    r3 = engine.propagate(*args, n_use=7)
    assert torch.equal(r3.J, r1.J[:, :7])
    Jo, st = orc.lft_sweep_batch(A[[0, 17, 36]], Bm[[0, 17, 36]], Q[[0, 17, 36]], Ri[[0, 17, 36]],
                                 z0[0], QT[[0, 17, 36]])
    assert _elem_rel(r1.J.cpu().numpy()[[0, 17, 36]], Jo) <= RTOL64


def test_lft_status_bits_and_nonfinite(dev):
    """Indefinite Q blocks trigger jitter escalation / LU fallback like chol_inv;
    NaN input is reported as non-finite (reference: FloatingPointError)."""
    from time_opt_ilqr_amd import engine
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(900, 3, 5, 1, 6)
    Q = Q.copy()
    Q[0, 2] = Q[0, 2] - np.eye(5) * (np.linalg.eigvalsh(Q[0, 2]).min() + 5e-8)  # needs jitter
    Q[1, 3] = -np.eye(5)                                                     # LU fallback
    QT = QT.copy()
    QT[2, 4, 0, 0] = np.nan
    res = engine.propagate(_t(A, dev), _t(Bm, dev), _t(Q, dev), _t(Ri, dev), _t(z0[0], dev),
                           _t(QT, dev))
    st = res.status.cpu().numpy()
    J = res.J.cpu().numpy()
    o0 = orc.lft_sweep(A[0], Bm[0], Q[0], Ri[0], z0[0], QT[0])
    o1 = orc.lft_sweep(A[1], Bm[1], Q[1], Ri[1], z0[1], QT[1])
    assert st[0] & orc.ST_JITTER and not st[0] & orc.ST_LU
    assert o0["status"] & orc.ST_JITTER
    assert st[1] & orc.ST_LU and o1["status"] & orc.ST_LU
    # problem 0: the escalated block leaves E_2 with an eigenvalue ~1/(5e-8); the
    # compose step then cancels terms of size ~2e7, so only the horizons before
    # that block are compared tightly (NumPy's own inv vs Cholesky paths already
    # differ by 3e-3 after it).
    assert _elem_rel(J[0, :2], o0["J"][:2]) <= 1e-6
    assert _elem_rel(J[0], o0["J"]) <= 1e-1
    assert np.isfinite(J[1]).all() and _elem_rel(J[1], o1["J"]) <= 1e-6
    assert st[2] & orc.ST_NONFINITE
    assert np.isnan(J[2, 4]) and np.isfinite(np.delete(J[2], 4)).all()


def test_config2_full_batch_spot_check(dev):
    """Config 2 shape (s=13, m=4, N=100, B=4096): all finite / status 0 and
    8 problems re-checked against the oracle; duplicated problems agree bitwise."""
    import torch
    from time_opt_ilqr_amd import engine
    from time_opt_ilqr_amd import synth
    Bn, s, m, N = 4096, 13, 4, 100
    A, Bm, Q, Ri, z0, QT = synth.device_batch(Bn, s, m, N, seed=7, device=dev)
    A[4095] = A[3]
    Bm[4095] = Bm[3]
    Q[4095] = Q[3]
    QT[4095] = QT[3]
    Ri[4095] = Ri[3]
    res = engine.propagate(A, Bm, Q, Ri, z0, QT, t_min=40, t_max=100)
    torch.cuda.synchronize()
    assert int(res.status.abs().sum()) == 0
    assert bool(torch.isfinite(res.J).all())
    assert torch.equal(res.J[4095], res.J[3])
    idx = [0, 1, 777, 1500, 2049, 3000, 4001, 4094]
    h = lambda t: t[idx].cpu().numpy()  # noqa: E731
    Jo, _ = orc.lft_sweep_batch(h(A), h(Bm), h(Q), h(Ri), z0.cpu().numpy(), h(QT))
    assert _elem_rel(res.J[idx].cpu().numpy(), Jo) <= RTOL64
    Ts, Js = orc.select_horizon(Jo, 40, 100)
    assert res.t_star[idx].cpu().numpy().tolist() == Ts.tolist()


def test_select_horizon_kernel(dev):
    from time_opt_ilqr_amd import engine
    rng = np.random.default_rng(3)
    J = rng.integers(0, 5, size=(300, 60)).astype(np.float64)  # many ties
    J[7, 30] = np.nan
    J[8, 2] = np.nan   # outside the window
    ts, js = engine.select_horizon(_t(J, dev), 5, 50)
    ref_t, ref_j = orc.select_horizon(J, 5, 50)
    assert ts.cpu().numpy().tolist() == ref_t.tolist()
    got = js.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref_j))
    assert np.array_equal(got[~np.isnan(got)], ref_j[~np.isnan(ref_j)])


# ---------------------------------------------------------------------------
# Riccati passes
# ---------------------------------------------------------------------------

def test_riccati_truncated_and_expand_vs_reference(dev, golden_dir):
    """Eight synthetic problems (horizons 1 .. 100) against the reference's own
    backward_pass_truncated / value_expansions_and_gains_prefix output, every step
    on its own (tests/gain_check.py)."""
    from time_opt_ilqr_amd import engine
    d = _load(golden_dir, "riccati_synth_n12_m4_N100.npz")
    n, m, N = int(d["n"]), int(d["m"]), int(d["N"])
    probs = [orc.synth_riccati_problem(int(sd), n, m, N) for sd in d["seeds"]]
    cnt = len(probs)
    assert cnt >= 8
    st = lambda j: np.stack([p[j] for p in probs])  # noqa: E731
    A, B, X, U, xg, ur, Q, R = (st(j) for j in range(8))
    Qf = np.stack([orc.terminal_weight(p[8], n) for p in probs])
    T = d["T_stars"].astype(np.int32)
    args = [_t(x, dev) for x in (A, B, X, U, xg, ur, Q, R, Qf)]
    r0 = engine.riccati(*args, T, float(d["lm"]), mode=0)
    r1 = engine.riccati(*args, T, float(d["lm"]), mode=1, w_stage=float(d["w_stage"]))
    assert r0.status.cpu().numpy().tolist() == [0] * cnt
    assert r1.status.cpu().numpy().tolist() == [0] * cnt
    for i in range(cnt):
        Ti = int(T[i])
        assert_per_step(r0.k[i, :Ti].cpu().numpy(), d[f"p{i}_k"], RTOL64, f"{i} k")
        assert_per_step(r0.K[i, :Ti].cpu().numpy(), d[f"p{i}_K"], RTOL64, f"{i} K")
        assert_per_step(r1.K[i, :Ti].cpu().numpy(), d[f"p{i}_K2"], RTOL64, f"{i} K2")
        assert_per_step(r1.k[i, :Ti].cpu().numpy(), d[f"p{i}_k2"], RTOL64, f"{i} k2")
        assert_per_step(r1.Vxx[i, :Ti + 1].cpu().numpy(), d[f"p{i}_Vxx"], RTOL64, f"{i} Vxx")
        assert_per_step(r1.Vx[i, :Ti + 1].cpu().numpy(), d[f"p{i}_Vx"], RTOL64, f"{i} Vx")
        assert_per_step(r1.V0[i, :Ti + 1].cpu().numpy(), d[f"p{i}_V0"], RTOL64, f"{i} V0")


def test_value_expansions_shift_and_wrap(dev, golden_dir):
    from time_opt_ilqr_amd import horizon_selection as hs
    d = _load(golden_dir, "riccati_shift_n6_m2_N60.npz")
    n, m, N = int(d["n"]), int(d["m"]), int(d["N"])
    A, B, X, U, xg, ur, Q, R, alpha = orc.synth_riccati_problem(int(d["seed"]), n, m, N)
    Vxx, Vx, V0, K, k = hs.value_expansions_and_gains_prefix(
        list(A), list(B), X, U, xg, ur, Q, R, alpha, int(d["T_bar"]), int(d["S_right"]),
        lm_lambda=float(d["lm"]), w_stage=float(d["w_stage"]), wrap_idx=[int(i) for i in d["wrap_idx"]])
    assert _rel(np.array(V0), d["V0"]) <= RTOL64
    assert _rel(np.array(Vx), d["Vx"]) <= RTOL64
    assert _rel(np.array(Vxx), d["Vxx"]) <= RTOL64
    assert _rel(np.array(K), d["K"]) <= RTOL64
    assert _rel(np.array(k), d["k"]) <= RTOL64


def test_backward_pass_truncated_failure(dev, golden_dir):
    from time_opt_ilqr_amd import horizon_selection as hs
    d = _load(golden_dir, "riccati_fail_n4_m2_N20.npz")
    A, B, X, U, xg, ur, Q, R, alpha = orc.synth_riccati_problem(int(d["seed"]), 4, 2, 20)
    k, K, ok = hs.backward_pass_truncated(list(A), list(B), X, U, xg, ur, Q, d["R"], alpha, 20)
    assert ok is False and bool(d["ok"]) is False and k is None and K is None


def test_bruteforce_curve(dev, golden_dir):
    from time_opt_ilqr_amd import horizon_selection as hs
    d = _load(golden_dir, "bruteforce_n4_m2_N40.npz")
    A, B, X, U, xg, ur, Q, R, alpha = orc.synth_riccati_problem(int(d["seed"]), 4, 2, 40)
    J = hs.bruteforce_all_Jt_backward_expansion(list(A), list(B), X, U, xg, ur, Q, R, alpha,
                                                float(d["w"]), int(d["T_max"]))
    assert _rel(J, d["J"]) <= RTOL64


def test_real_DI_dropins(dev, golden_dir):
    """Reference-shaped drop-ins on the captured DoubleIntegrator linearisation."""
    from time_opt_ilqr_amd import horizon_selection as hs
    d = _load(golden_dir, "real_DI_N50.npz")
    J = hs.propagator_all_Jt_aug(list(d["plast_A"]), list(d["plast_B"]), list(d["plast_Q"]),
                                 None, d["plast_z0"], list(d["plast_QT"]),
                                 T_use=int(d["plast_T_use"]), R_inv_cached=d["plast_R_inv"])
    assert hs.select_horizon(J, int(d["T_min"]), int(d["T_max"])) == int(d["T_star_final"])
    k, K, ok = hs.backward_pass_truncated(list(d["bwd_A"]), list(d["bwd_B"]), d["bwd_X"],
                                          d["bwd_U"], d["xg"], d["u_ref"], d["Q"], d["R"],
                                          float(d["alpha"]), int(d["bwd_T_star"]),
                                          lm_lambda=float(d["bwd_lm"]))
    assert ok
    assert_per_step(np.array(k), d["bwd_k"], RTOL64, "k")
    assert_per_step(np.array(K), d["bwd_K"], RTOL64, "K")
    bf = hs.bruteforce_all_Jt_backward_expansion(
        list(d["bwd_A"]), list(d["bwd_B"]), d["bwd_X"], d["bwd_U"], d["xg"], d["u_ref"],
        d["Q"], d["R"], float(d["alpha"]), float(d["w"]), len(d["bf_J"]))
    assert _rel(bf, d["bf_J"]) <= RTOL64


@pytest.mark.parametrize("schedule", [pytest.param(v, marks=pytest.mark.devbuild)
                                      for v in ("2", "8", "10", "12", "14")] + ["30", "40"])
def test_lft_fast_path_matches_generic_kernel(dev, schedule):
    """Every schedule of the exact-size fp64 kernel (LDS-DMA streamed, s=13/m=4)
    and the generic kernel agree, including the jitter / LU retry paths and batch
    tails.  Product builds carry the default (40: conditioned prefix + rerun) and
    the reference association (30, HOP_OPT_REFERENCE_ASSOC); the A/B schedules
    (2 select pivots, 8 offset-form C++ chain, 10/12/14 hand-scheduled asm) exist
    only in developer builds."""
    from time_opt_ilqr_amd import _lib, engine
    if schedule not in ("30", "40") and not _lib.dev_build():
        pytest.skip("A/B schedule: developer builds only (HOP_DEV_BUILD=1)")
    Bn, s, m, N = 37, 13, 4, 30
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(700, Bn, s, m, N)
    Q = Q.copy()
    Q[3, 5] = Q[3, 5] - np.eye(s) * (np.linalg.eigvalsh(Q[3, 5]).min() + 5e-7)  # jitter
    Q[20, 7] = -np.eye(s)                                                    # LU slot
    QT = QT.copy()
    QT[36, 2] = QT[36, 2] - np.eye(s) * (np.linalg.eigvalsh(QT[36, 2]).min() + 5e-6)
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    kw = dict(reference_assoc=True) if schedule == "30" else (
        {} if schedule == "40" else dict(variant=int(schedule)))
    with _lib.options(**kw):
        fast = engine.propagate(*args, t_min=5, t_max=30)
    with _lib.options(force_generic=True):
        gen = engine.propagate(*args, t_min=5, t_max=30)
    st_f, st_g = fast.status.cpu().numpy(), gen.status.cpu().numpy()
    assert st_f.tolist() == st_g.tolist()
    assert st_f[3] & orc.ST_JITTER and st_f[20] & orc.ST_LU and st_f[36] & orc.ST_JITTER
    ok = [i for i in range(Bn) if i not in (3, 20, 36)]
    assert _elem_rel(fast.J.cpu().numpy()[ok], gen.J.cpu().numpy()[ok]) <= 1e-10
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
    assert sto.tolist() == st_f.tolist()
    assert _elem_rel(fast.J.cpu().numpy()[ok], Jo[ok]) <= RTOL64
    assert _elem_rel(fast.J.cpu().numpy()[20], Jo[20]) <= 1e-6
    assert fast.t_star.cpu().numpy()[ok].tolist() == gen.t_star.cpu().numpy()[ok].tolist()


@pytest.mark.parametrize("s,m,dt,tol", [(5, 1, "f32", 2e-3), (3, 1, "f64", 1e-10),
                                        (4, 2, "f64", 1e-10)])
def test_lft_small_path_matches_generic_and_oracle(dev, s, m, dt, tol):
    """The one-problem-per-lane kernel (lft_small.hip, s <= 5) agrees with the
    generic kernel and the oracle, including jitter / LU-slot problems and a
    batch that is not a multiple of the 64-lane wave."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, N = 131, 40
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(900 + s, Bn, s, m, N)
    Q = Q.copy()
    Q[7, 3] = Q[7, 3] - np.eye(s) * (np.linalg.eigvalsh(Q[7, 3]).min() + 5e-7)  # jitter
    Q[70, 5] = -np.eye(s)                                                   # LU slot
    td = torch.float32 if dt == "f32" else torch.float64
    args = [torch.as_tensor(np.ascontiguousarray(x), dtype=td, device=dev)
            for x in (A, Bm, Q, Ri, z0[0], QT)]
    small = engine.propagate(*args, t_min=3, t_max=N)
    with _lib.options(force_generic=True):
        gen = engine.propagate(*args, t_min=3, t_max=N)
    ss = small.status.cpu().numpy()
    assert ss[7] & orc.ST_JITTER and ss[70] & orc.ST_LU
    ok = [i for i in range(Bn) if i not in (7, 70)]
    Js, Jg = small.J.cpu().numpy().astype(float), gen.J.cpu().numpy().astype(float)
    assert _elem_rel(Js[ok], Jg[ok]) <= tol
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
    if dt == "f64":  # fp32 can legitimately need jitter where fp64 does not
        diff = [(i, int(ss[i]), int(sto[i])) for i in range(Bn) if ss[i] != sto[i]]
        assert not diff, diff
    assert _elem_rel(Js[ok], Jo[ok]) <= max(tol, RTOL64)
    if dt == "f64":
        assert small.t_star.cpu().numpy()[ok].tolist() == gen.t_star.cpu().numpy()[ok].tolist()


def test_cond_kernel_alone_matches_lft_kernel(dev):
    """The conditioned-prefix kernel on clean inputs: no problem is handed over
    (status 0, and the result is NOT bitwise the reference-association kernel's,
    so the conditioned kernel produced it), J within 1e-10 of the reference
    association (HOP_OPT_REFERENCE_ASSOC) and of the oracle, same T*/J*, batch
    tail included (B = 53)."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, s, m, N = 53, 13, 4, 100
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(4242, Bn, s, m, N)
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    cnd = engine.propagate(*args, t_min=30, t_max=100)
    with _lib.options(reference_assoc=True):
        ref = engine.propagate(*args, t_min=30, t_max=100)
    assert cnd.status.cpu().numpy().tolist() == [0] * Bn
    assert not torch.equal(cnd.J, ref.J)
    assert _elem_rel(cnd.J.cpu().numpy(), ref.J.cpu().numpy()) <= 1e-10
    Jo, _ = orc.lft_sweep_batch(A[:6], Bm[:6], Q[:6], Ri[:6], z0[0], QT[:6])
    assert _elem_rel(cnd.J.cpu().numpy()[:6], Jo) <= 1e-10
    assert cnd.t_star.cpu().numpy().tolist() == ref.t_star.cpu().numpy().tolist()
    assert _elem_rel(cnd.j_star.cpu().numpy(), ref.j_star.cpu().numpy()) <= 1e-10


def test_cond_forced_handover_is_the_lft_kernel(dev):
    """HOP_OPT_FORCE_HANDOVER flags every problem: the rerun launch then recomputes
    the whole batch with the reference association, bitwise equal to
    HOP_OPT_REFERENCE_ASSOC."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, s, m, N = 21, 13, 4, 40
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(4343, Bn, s, m, N)
    Q = Q.copy()
    Q[4, 7] = -np.eye(s)  # LU slot
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    with _lib.options(force_handover=True):
        f = engine.propagate(*args, t_min=5, t_max=40)
    with _lib.options(reference_assoc=True):
        r = engine.propagate(*args, t_min=5, t_max=40)
    assert torch.equal(f.J, r.J) and torch.equal(f.status, r.status)
    assert torch.equal(f.t_star, r.t_star) and torch.equal(f.j_star, r.j_star)
    assert int(r.status[4]) & orc.ST_LU


def test_cond_packed_layout_handover_large_batch(dev):
    """B = 4101 (more waves than SIMDs): the conditioned kernel runs its packed-image
    layout at two waves per SIMD.  Forced hand-over: the rerun launch (the LFT kernel in
    its own layout) recomputes every problem, bitwise equal to HOP_OPT_REFERENCE_ASSOC;
    default: the problem that needs chol_inv's LU slot is handed over (its status bits
    and J the LFT kernel's, bitwise), the rest within 1e-9 of the reference association."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, s, m, N = 4101, 13, 4, 24
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(5151, Bn, s, m, N)
    Q = Q.copy()
    Q[4099, 7] = -np.eye(s)  # LU slot, in the last workgroup
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    with _lib.options(force_handover=True):
        f = engine.propagate(*args, t_min=3, t_max=N)
    with _lib.options(reference_assoc=True):
        r = engine.propagate(*args, t_min=3, t_max=N)
    d = engine.propagate(*args, t_min=3, t_max=N)
    assert torch.equal(f.J, r.J) and torch.equal(f.status, r.status)
    assert torch.equal(f.t_star, r.t_star)
    assert int(r.status[4099]) & orc.ST_LU
    assert torch.equal(d.status, r.status)
    assert torch.equal(d.J[4099], r.J[4099])
    assert float(((d.J - r.J).abs() / r.J.abs()).max()) <= 1e-9


@pytest.mark.devbuild
@pytest.mark.parametrize("s,m,dt", [(5, 1, "f32"), (3, 1, "f64"), (4, 2, "f64")])
def test_small_cond_kernel(dev, s, m, dt):
    """Small-s COND kernels (developer builds, opt-in): alone (variant 62) no
    problem is handed over and J matches the LFT instantiation (the default); with
    HOP_OPT_FORCE_HANDOVER the rerun launch recomputes every problem bitwise like
    the LFT instantiation; cond + rerun (variant 61) keeps chol_inv's status bits
    on a bad block."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    if not _lib.dev_build():
        pytest.skip("small-s conditioned kernels: developer builds only (HOP_DEV_BUILD=1)")
    tdt = torch.float64 if dt == "f64" else torch.float32
    Bn, N = 131, 40
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(5150 + s, Bn, s, m, N)
    Q = Q.copy()
    Q[7, 11] = -np.eye(s)  # LU slot on the LFT path
    args = [_t(x, dev, tdt) for x in (A, Bm, Q, Ri, z0[0], QT)]
    ref = engine.propagate(*args, t_min=4, t_max=N)
    with _lib.options(variant=62):
        alone = engine.propagate(*args, t_min=4, t_max=N)
    st = alone.status.cpu().numpy()
    assert st[7] == 16 and (np.delete(st, 7) == 0).all()
    ok = [i for i in range(Bn) if i != 7]
    tol = 1e-10 if dt == "f64" else 1e-3
    assert _elem_rel(alone.J.cpu().numpy()[ok], ref.J.cpu().numpy()[ok]) <= tol
    with _lib.options(variant=61):  # cond + rerun (not the default)
        dflt = engine.propagate(*args, t_min=4, t_max=N)
    assert torch.equal(dflt.status, ref.status) and int(dflt.status[7]) & orc.ST_LU
    assert torch.equal(dflt.J[7], ref.J[7])
    with _lib.options(variant=61, force_handover=True):
        forced = engine.propagate(*args, t_min=4, t_max=N)
    assert torch.equal(forced.J, ref.J) and torch.equal(forced.status, ref.status)
    assert torch.equal(forced.t_star, ref.t_star)


def test_cond_fp32_blocks_config5_shape(dev, golden_dir):
    """fp32 blocks at s=13, m=4 (config 5 shape, N=128): the conditioned kernel reads
    fp32 images and computes in fp64, so J is the reference's to fp32 input rounding
    (2e-5 here; the generic fp32 kernel is at its 2e-3 bar) with T* equal;
    HOP_OPT_FORCE_HANDOVER hands every problem to the generic fp32 kernel (bitwise
    equal to HOP_OPT_FORCE_GENERIC); batch tail 5."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    d = _load(golden_dir, "lft_synth_s13_m4_N128.npz")
    s, m, N, bs, cnt = (int(d[k]) for k in ("s", "m", "N", "base_seed", "count"))
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(bs, cnt, s, m, N)
    f = lambda x: _t(x, dev, torch.float32)  # noqa: E731
    args = [f(x) for x in (A, Bm, Q, Ri, z0, QT)]
    kw = dict(t_min=int(d["T_min"]), t_max=int(d["T_max"]))
    res = engine.propagate(*args, **kw)
    assert res.J.dtype == torch.float32
    assert _elem_rel(res.J.cpu().numpy(), d["J"]) <= 2e-5
    assert res.t_star.cpu().numpy().tolist() == d["T_star"].tolist()
    assert int(res.status.abs().sum()) == 0
    with _lib.options(force_handover=True):
        forced = engine.propagate(*args, **kw)
    with _lib.options(force_generic=True):
        gen = engine.propagate(*args, **kw)
    assert torch.equal(forced.J, gen.J) and torch.equal(forced.status, gen.status)
    assert _elem_rel(gen.J.cpu().numpy(), d["J"]) <= 2e-3


def test_cond_fp32_blocks_no_rerun_skips_the_second_launch(dev):
    """fp32 blocks at s = 13, m = 4 under HOP_OPT_NO_RERUN: the conditioned kernel
    alone, no second launch (no triage on this path), so a problem it hands over (Q_3 =
    -I: chol_inv's LU slot in the reference, utils.py:69-93) keeps the hand-over word
    and every other problem the conditioned kernel's J and status 0; with
    HOP_OPT_FORCE_HANDOVER too, every problem keeps HOP_HANDOVER_WORD(0).  Without
    NO_RERUN the handed-over problem is the generic fp32 kernel's, bitwise
    (HOP_OPT_REFERENCE_ASSOC), as is the whole forced batch.  Five problems, six
    steps: one full wave and a tail of one."""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn, s, m, N, b, k = 5, 13, 4, 6, 2, 3
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(4848, Bn, s, m, N)
    Q = Q.copy()
    Q[b, k] = -np.eye(s)
    args = [_t(x, dev, torch.float32) for x in (A, Bm, Q, Ri, z0[0], QT)]
    kw = dict(t_min=2, t_max=N)
    d = engine.propagate(*args, **kw)
    with _lib.options(reference_assoc=True):
        r = engine.propagate(*args, **kw)
    with _lib.options(no_rerun=True):
        nr = engine.propagate(*args, **kw)
    with _lib.options(no_rerun=True, force_handover=True):
        nf = engine.propagate(*args, **kw)
    with _lib.options(force_handover=True):
        f = engine.propagate(*args, **kw)
    torch.cuda.synchronize()
    ok = [i for i in range(Bn) if i != b]
    st = nr.status.cpu().numpy()
    assert st[b] & _lib.ST_HANDOVER and (st[ok] == 0).all(), st
    assert (nf.status.cpu().numpy() == _lib.ST_HANDOVER).all(), nf.status
    assert int(r.status[b]) & orc.ST_LU
    nn = lambda x: x.nan_to_num(7.0)  # noqa: E731  (NaN patterns compare equal)
    assert torch.equal(d.status, r.status) and torch.equal(nn(d.J[b]), nn(r.J[b]))
    assert torch.equal(d.J[ok], nr.J[ok])  # not handed over: the first launch's values
    assert torch.equal(nn(f.J), nn(r.J)) and torch.equal(f.status, r.status)
    assert torch.equal(f.t_star, r.t_star) and torch.equal(nn(f.j_star), nn(r.j_star))


def test_cond_nonfinite_short_horizons_and_tails(dev):
    """Default s=13 path (conditioned kernel + rerun): a NaN block is handed over and
    reported exactly as the reference association reports it (non-finite J at that
    horizon, ST_NONFINITE); N = 1 and t_min = t_max; a batch of 17 (tail of 1)."""
    import torch
    from time_opt_ilqr_amd import engine
    Bn, s, m, N = 17, 13, 4, 12
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(6060, Bn, s, m, N)
    QT = QT.copy()
    QT[16, 5, 2, 3] = np.nan
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    res = engine.propagate(*args, t_min=3, t_max=3)
    st = res.status.cpu().numpy()
    J = res.J.cpu().numpy()
    assert st[16] & orc.ST_NONFINITE and (st[:16] == 0).all()
    assert np.isnan(J[16, 5]) and np.isfinite(np.delete(J[16], 5)).all()
    Jo, _ = orc.lft_sweep_batch(A[:16], Bm[:16], Q[:16], Ri[:16], z0[0], QT[:16])
    assert _elem_rel(J[:16], Jo) <= 1e-10
    assert (res.t_star.cpu().numpy()[:16] == 3).all()
    one = engine.propagate(*args, n_use=1)
    Jo1, _ = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT, N=1)
    assert _elem_rel(one.J.cpu().numpy(), Jo1) <= 1e-10
    assert int(one.status.abs().sum()) == 0
    empty = engine.propagate(*args, n_use=0)
    assert empty.J.shape == (Bn, 0) and int(empty.status.abs().sum()) == 0


@pytest.mark.parametrize("s,m", [(13, 4), (8, 2), (5, 1), (3, 1)])
def test_nonfinite_inputs_status_and_curve_match_oracle(dev, s, m):
    """chol_inv's _assert_finite (utils.py:77): a non-finite block raises in the
    reference; the oracle reports its inverse as NaN with ST_NONFINITE alone (no
    jitter ladder).  Every kernel family (s=13 default + rerun, generic s=8, small
    s=5/3) gives the oracle's exact status word and NaN pattern, the finite
    horizons to 1e-9: NaN in Q_k (every later horizon NaN), in QT_k (one horizon),
    inf in A_k, NaN in z0, and an indefinite block beside them (jitter bits kept);
    since round 5 also +inf on the diagonal of Q_k and of QT_k (an "infinite cost"
    pivot, which an exact reciprocal would turn into a finite zero row: the
    kernels' v_rcp + Newton gives NaN there, and the reference raises)."""
    from time_opt_ilqr_amd import engine
    Bn, N = 8, 14
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(7070 + s, Bn, s, m, N)
    A, Q, QT, z0 = A.copy(), Q.copy(), QT.copy(), z0.copy()
    Q[0, 4, 1, 2] = np.nan
    QT[1, 6, 0, 0] = np.nan
    A[2, 3, 0, 1] = np.inf
    z0[3, 1] = np.nan
    Q[4, 2] = Q[4, 2] - np.eye(s) * (np.linalg.eigvalsh(Q[4, 2]).min() + 5e-8)  # jitter
    Q[5, 9, s - 1, 0] = -np.inf
    Q[6, 3, 1, 1] = np.inf
    QT[7, 5, s - 1, s - 1] = np.inf
    res = engine.propagate(_t(A, dev), _t(Bm, dev), _t(Q, dev), _t(Ri, dev), _t(z0, dev),
                           _t(QT, dev))
    st = res.status.cpu().numpy()
    J = res.J.cpu().numpy()
    for b in range(Bn):
        with np.errstate(invalid="ignore", over="ignore"):  # NaN / inf blocks by design
            o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b])
        assert int(st[b]) == int(o["status"]), (b, int(st[b]), int(o["status"]))
        nan = np.isnan(o["J"])
        assert np.array_equal(np.isnan(J[b]), nan), (b, J[b], o["J"])
        if b != 4 and not nan.all():  # b=4: the escalated block amplifies rounding
            assert _elem_rel(J[b][~nan], o["J"][~nan]) <= 1e-9, b


def test_random_shapes_every_path_vs_oracle(dev):
    """Seeded random shapes (s 2..16, m 1..min(s, 6), N 1..24, B 1..9, fp64/fp32,
    batch-major and tile64 where the small-s path takes them, random t_min/t_max):
    J against the oracle (fp64 1e-9 elementwise, fp32 2e-3), T* equal in fp64, and
    the status word equal on these well-conditioned inputs."""
    import torch
    from time_opt_ilqr_amd import engine
    rng = np.random.default_rng(20261016)
    for case in range(14):
        s = int(rng.integers(2, 17))
        m = int(rng.integers(1, min(s, 6) + 1))
        N = int(rng.integers(1, 25))
        Bn = int(rng.integers(1, 10))
        f32 = bool(rng.integers(0, 2)) and s <= 13
        t_min = int(rng.integers(1, N + 1))
        t_max = int(rng.integers(t_min, N + 1))
        A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(500 + 37 * case, Bn, s, m, N)
        dt = torch.float32 if f32 else torch.float64
        args = [_t(x, dev, dt) for x in (A, Bm, Q, Ri, z0[0], QT)]
        r = engine.propagate(*args, t_min=t_min, t_max=t_max)
        Jo, st = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT)
        tag = (case, s, m, N, Bn, "f32" if f32 else "f64", t_min, t_max)
        J = r.J.double().cpu().numpy()
        assert _elem_rel(J, Jo) <= (2e-3 if f32 else 1e-9), tag
        Ts, _ = orc.select_horizon(Jo, t_min, t_max)
        if not f32:
            assert r.t_star.cpu().numpy().tolist() == Ts.tolist(), tag
            assert r.status.cpu().numpy().tolist() == st.tolist(), tag
        tiled = {(2, 1), (3, 1), (4, 1), (4, 2)} | ({(5, 1), (5, 2)} if f32 else set())
        if (s, m) in tiled:  # the same problems on tile64 blocks (small-s instantiations)
            tl = engine.propagate(*(engine.to_tile64(x) for x in args[:3]), args[3], args[4],
                                  engine.to_tile64(args[5]), t_min=t_min, t_max=t_max)
            assert _elem_rel(tl.J.double().cpu().numpy(), Jo) <= (2e-3 if f32 else 1e-9), tag
