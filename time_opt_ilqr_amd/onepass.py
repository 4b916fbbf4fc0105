"""The one-pass window method (baseline2, ``method="onepass"``) of the device outer loop.

``solve_batch`` runs ``ilqr_timeopt(method="onepass")`` (the reference's
solver.py:534-537, 630-765) for a batch of independent problems of one built-in device
system.  Per outer iteration: the FD linearisation, the negative-time prefix
(hop_onepass_extend_backward_f64) and its forward-difference linearisation, one value
sweep around T_bar over the extended trajectory (hop_riccati_f64 mode 1), the window pick
(hop_onepass_pick_f64), up to three rounds of rollout (hop_onepass_rollout_f64) and
shrink-and-pick-again, and the shared accept / LM / stop step (hop_ilqr_accept_f64).  A
problem whose sweep fails takes the reference's fallback in the same iteration: the
truncated Riccati pass at T_bar and the ordinary line search.  The host only sequences
launches.

Reproduced as the reference does them:
* the shrink loop re-picks with the shrunken S_right while the arrays keep their offset,
  so the candidates' index moves with it (solver.py:726-729);
* it re-picks after the third failed round too, and that curve is the one returned;
* the rollout keeps the smallest J over all step sizes, not the first improving one;
* a failed sweep never stops a problem (no ``crashed`` mark): it is retried every
  iteration with the LM parameter the rejections have raised.
"""
from __future__ import annotations

import time
from typing import Any, Dict

import numpy as np

from . import _lib, engine, host_dynamics

PREIMAGE_ITERS, PREIMAGE_TOL, PREIMAGE_DAMPING = 4, 1e-9, 0.5  # solver.py:636-642


def check_scope(system, S_window, onepass_preimage, extra_stage_cost=None):
    """The inputs method="onepass" takes on the device; everything else raises here,
    before anything touches the GPU."""
    if engine.is_fleet(system):
        raise NotImplementedError("method='onepass' is not implemented for a fleet (the "
                                  "one-pass primitives cover the five built-in systems)")
    if engine.is_team(system):
        raise NotImplementedError("method='onepass' is not implemented for a team (the "
                                  "one-pass primitives cover the five built-in systems)")
    if isinstance(system, host_dynamics.HostDynamics) or (
            callable(system) and not hasattr(system, "system_id") and not engine.is_chain(system)):
        raise NotImplementedError("method='onepass' runs the five built-in device systems "
                                  "(systems.DeviceDynamics); host dynamics and Python "
                                  "callables are out of scope")
    if engine.is_chain(system):
        raise NotImplementedError("method='onepass' is not implemented for the spring chain "
                                  "(n > 16)")
    if extra_stage_cost is not None:
        raise NotImplementedError("method='onepass' takes the point-mass obstacle table; a "
                                  "Python extra_stage_cost is out of scope")
    pre = str(onepass_preimage).lower().strip()
    if pre in ("newton", "copy"):
        raise NotImplementedError(f"onepass_preimage={pre!r}: only 'fixedpoint' runs on the "
                                  "device")
    if pre != "fixedpoint":
        raise ValueError(f"unknown onepass_preimage {onepass_preimage!r}")
    S = int(S_window)
    if S == 0:
        raise ValueError("S_window = 0: the reference's shrink step then reads X_ext[-1]; the "
                         "device loop needs 1 <= S_window <= 64")
    if not 1 <= S <= _lib.ONEPASS_MAX_WINDOW:
        raise ValueError(f"S_window must be in [1, {_lib.ONEPASS_MAX_WINDOW}], got {S}")
    return S


def solve_batch(system, x0, xg, u_ref, Q, R, Qf, w, N, T_min, T_max, *, dt, U_init, max_iter,
                lm_init, wrap_idx, use_central_diff, obstacles, alphas, device, stage_timers,
                S_window, onepass_preimage, extra_stage_cost) -> Dict[str, Any]:
    """ilqr_timeopt_batch(method="onepass"): its arguments, its result keys, plus
    ``onepass_error`` [B] (the last sweep's status), ``onepass_failed`` [B] (the failure
    bits of every sweep so far: where the reference's onepass_error is not None) and
    ``J_curve_valid`` [B] (False where the reference returns no curve)."""
    from .solver import IlqrState
    S = check_scope(system, S_window, onepass_preimage, extra_stage_cost)
    import torch
    sid = engine.system_id(system)
    n, m = engine.system_dims(sid)
    dev = device or torch.device("cuda", torch.cuda.current_device())
    f64, i32 = torch.float64, torch.int32
    tt = lambda a: torch.as_tensor(np.asarray(a, dtype=float) if not isinstance(  # noqa: E731
        a, torch.Tensor) else a, dtype=f64, device=dev).contiguous()
    N, T_min, T_max = int(N), int(T_min), int(T_max)
    if not 1 <= T_min <= T_max <= N:
        raise IndexError("need 1 <= T_min <= T_max <= N (the reference indexes lists of N)")
    x0 = tt(x0)
    Bn = x0.shape[0] if x0.dim() == 2 else 1
    xg_t, ur_t, Q_t, R_t, Qf_t = tt(xg), tt(np.atleast_1d(u_ref) if not isinstance(
        u_ref, torch.Tensor) else u_ref), tt(Q), tt(R), tt(Qf)
    if R_t.dim() != 2 or Qf_t.dim() != 2:
        raise ValueError("R and Qf must be single matrices shared by the batch")
    obs = None if obstacles is None or len(obstacles) == 0 else tt(obstacles)
    w_t = torch.full((1,), float(w), dtype=f64, device=dev)
    w_f = float(w)
    per = [(xg_t, 1), (ur_t, 1), (Q_t, 2)]  # blocks that may be per problem

    def cost_of(idx):
        """the cost blocks of the problems idx (None: all)"""
        xs = [t if idx is None or t.dim() == d or t.shape[0] == 1 else t.index_select(0, idx)
              for t, d in per]
        return xs, engine.CostParams(xs[0], xs[1], xs[2], R_t, Qf_t, w_t, obs, wrap_idx)

    if U_init is None:
        U = ur_t.reshape(-1, m).expand(Bn, m)[:, None, :].expand(Bn, N, m).contiguous()
    else:
        U = tt(U_init)
        if U.dim() == 1:
            U = U.reshape(-1, 1)
        if U.dim() == 2:
            U = U[None]
        if U.dim() != 3 or U.shape[-1] != m or U.shape[0] not in (1, Bn):
            raise ValueError(f"U_init must be [N', {m}] or [B or 1, N', {m}]")
        U = U.expand(Bn, -1, -1)
        if U.shape[1] < N:
            U = torch.cat([U, U[:, -1:].expand(Bn, N - U.shape[1], m)], 1)
        U = U[:, :N].contiguous()
    nan = float("nan")
    timers = {k: (0.0 if stage_timers else nan)
              for k in ("linearize", "select", "backward", "forward")}
    t_rollout = 0.0 if stage_timers else nan

    def clock(key, t0):
        if stage_timers:
            torch.cuda.synchronize(dev)
            timers[key] += time.perf_counter() - t0

    t0 = time.perf_counter()
    X = engine.rollout(sid, x0, U, dt)
    if stage_timers:
        torch.cuda.synchronize(dev)
        t_rollout = time.perf_counter() - t0
    H = int(max_iter) + 1
    zi = lambda *s: torch.zeros(s, dtype=i32, device=dev)  # noqa: E731
    st = IlqrState(X, U, torch.full((Bn,), float(lm_init), dtype=f64, device=dev), zi(Bn),
                   torch.zeros((Bn, H), dtype=f64, device=dev), zi(Bn, H), zi(Bn), zi(Bn), zi(Bn))
    fields = ("X", "U", "lm", "T_bar", "J_hist", "T_hist", "n_hist", "done", "crashed")
    bad = _lib.ST_FAIL | _lib.ST_NONFINITE
    J_curve = torch.full((Bn, T_max), nan, dtype=f64, device=dev)
    curve_valid = torch.zeros((Bn,), dtype=torch.bool, device=dev)
    err_last, err_any = zi(Bn), zi(Bn)
    status_log = []

    def extras(Xs):
        """the obstacle terms of the stage cost at the states Xs [B, K, n]"""
        if obs is None:
            return {}
        c, cx, cxx = engine.obstacle_cost(Xs, obs)
        return dict(qxx_extra=cxx, qx_extra=cx, c_extra=c)

    def truncated_update(s, xs, cost, lin, T, mask, warm):
        """backward_pass_truncated at T and the ordinary line search for the problems in
        mask (solver.py:541-553 warm, 684-701 the fallback)"""
        t0 = time.perf_counter()
        ric = engine.riccati(lin.A, lin.B, s.X, s.U, xs[0], xs[1], xs[2], R_t, Qf_t, T, s.lm,
                             mode=0, wrap_idx=wrap_idx, reg_max_tries=1, **extras(s.X[:, :N]))
        clock("backward", t0)
        t0 = time.perf_counter()
        active = mask & ((ric.status & bad) == 0)
        fw = engine.forward_linesearch(sid, s.X, s.U, T, ric.K, ric.k, cost, dt, alphas=alphas,
                                       active=active)
        clock("forward", t0)
        return fw

    def warm_start(s, idx):
        xs, cost = cost_of(idx)
        # solver.py:534-537: T_bar from the nominal trajectory's cost curve
        _, T_bar = engine.nominal_cost_curve(sid, s.X, s.U, cost, T_min, T_max)
        s.T_bar.copy_(T_bar)
        t0 = time.perf_counter()
        lin = engine.linearize(sid, s.X, s.U, dt, central=use_central_diff)
        clock("linearize", t0)
        every = torch.ones_like(s.done, dtype=torch.bool)
        fw = truncated_update(s, xs, cost, lin, s.T_bar, every, True)
        engine.ilqr_accept(s, fw.J, fw.accepted, s.T_bar, warm=True)
        s.X, s.U = fw.X, fw.U

    def iterate(s, idx):
        """one outer iteration (solver.py:564-748, the onepass branch) of the problems in s;
        returns the sweep's status, the window curve and the rows that have one"""
        xs, cost = cost_of(idx)
        t0 = time.perf_counter()
        lin = engine.linearize(sid, s.X, s.U, dt, central=use_central_diff)
        X_ext, U_ext = engine.extend_nominal_backward(
            sid, s.X, s.U, s.U[:, 0], dt, S, max_iter=PREIMAGE_ITERS, tol=PREIMAGE_TOL,
            damping=PREIMAGE_DAMPING)
        pre = engine.linearize(sid, X_ext[:, :S + 1], U_ext[:, :S], dt, central=False)
        A_ext = torch.cat([pre.A, lin.A], 1)
        B_ext = torch.cat([pre.B, lin.B], 1)
        clock("linearize", t0)
        t0 = time.perf_counter()
        sweep = engine.riccati(A_ext, B_ext, X_ext, U_ext, xs[0], xs[1], xs[2], R_t, Qf_t,
                               s.T_bar + S, s.lm, mode=1, w_stage=w_f, wrap_idx=wrap_idx,
                               reg_max_tries=12, **extras(X_ext[:, :S + N]))
        failed = (sweep.status & bad) != 0
        x_start = X_ext[:, S].contiguous()
        T_star, Jw = engine.onepass_pick(sweep.Vxx, sweep.Vx, sweep.V0, X_ext, x_start, s.T_bar,
                                         T_min, T_max, S, S, wrap_idx=wrap_idx)
        clock("select", t0)
        t0 = time.perf_counter()
        nh = s.n_hist.long()
        J_prev = torch.where(nh > 0, s.J_hist.gather(1, (nh - 1).clamp(min=0)[:, None])[:, 0],
                             torch.full_like(s.lm, float("inf")))
        pending = ~failed
        accepted = torch.full_like(s.n_hist, -1)
        X_out, U_out, J_out, T_out = s.X, s.U, J_prev.clone(), s.T_bar.clone()
        S_L = S_R = S
        for _shrink in range(3):
            if not bool(pending.any().item()):
                break
            ro = engine.onepass_rollout(sid, X_ext, U_ext, sweep.K, sweep.k, cost, dt, s.T_bar,
                                        T_star, S, active=pending)
            acc = pending & ro.ok & (ro.J < J_prev)
            X_out = torch.where(acc[:, None, None], ro.X, X_out)
            U_out = torch.where(acc[:, None, None], ro.U, U_out)
            J_out = torch.where(acc, ro.J, J_out)
            T_out = torch.where(acc, T_star, T_out)
            accepted = torch.where(acc, torch.zeros_like(accepted), accepted)
            pending = pending & ~acc
            # shrink and pick again for the problems still pending (solver.py:723-730)
            S_L, S_R = max(1, S_L // 2), max(1, S_R // 2)
            T2, Jw2 = engine.onepass_pick(sweep.Vxx, sweep.Vx, sweep.V0, X_ext, x_start, s.T_bar,
                                          T_min, T_max, S_L, S_R, wrap_idx=wrap_idx)
            T_star = torch.where(pending, T2, T_star)
            Jw = torch.where(pending[:, None], Jw2, Jw)
        clock("forward", t0)
        if bool(failed.any().item()):
            # the fallback of solver.py:674-701 for the problems whose sweep raised
            fw = truncated_update(s, xs, cost, lin, s.T_bar, failed, False)
            acc = failed & (fw.accepted >= 0)
            X_out = torch.where(acc[:, None, None], fw.X, X_out)
            U_out = torch.where(acc[:, None, None], fw.U, U_out)
            J_out = torch.where(acc, fw.J, J_out)
            accepted = torch.where(acc, torch.zeros_like(accepted), accepted)
            Jw = torch.where(failed[:, None], torch.full_like(Jw, float("nan")), Jw)
        engine.ilqr_accept(s, J_out, accepted, T_out, warm=False)
        s.X, s.U = X_out, U_out
        return sweep.status, Jw, ~failed

    def gather(idx):
        return IlqrState(*[getattr(st, f).index_select(0, idx) for f in fields])

    def scatter(cur, idx):
        for f in fields:
            getattr(st, f).index_copy_(0, idx, getattr(cur, f))

    warm_start(st, None)
    iters = 0
    for _ in range(int(max_iter)):
        idx = (st.done == 0).nonzero()[:, 0]
        n_live = int(idx.numel())
        if n_live == 0:
            break
        whole = n_live == Bn
        cur = st if whole else gather(idx)
        stat, Jw, valid = iterate(cur, None if whole else idx)
        if whole:
            idx = torch.arange(Bn, device=dev)
        else:
            scatter(cur, idx)
        J_curve.index_copy_(0, idx, Jw)
        curve_valid.index_copy_(0, idx, valid)
        err_last.index_copy_(0, idx, stat)
        err_any.index_copy_(0, idx, err_any.index_select(0, idx) | (stat & bad))
        status_log.append(torch.zeros_like(err_last).index_copy_(0, idx, stat))
        iters += 1
    nh = st.n_hist
    last = (nh - 1).clamp(min=0).long()
    T_res = torch.where(nh > 0, st.T_hist.gather(1, last[:, None])[:, 0], st.T_bar)
    sel = torch.stack(status_log, 1) if status_log else zi(Bn, 0)
    return dict(X=st.X, U=st.U, J_hist=st.J_hist, T_hist=st.T_hist, n_hist=nh, T_star=T_res,
                crashed=st.crashed, lm=st.lm, iterations=iters, timers=timers,
                t_rollout=t_rollout, J_curve=J_curve, select_status=sel,
                onepass_error=err_last, onepass_failed=err_any, J_curve_valid=curve_valid)
