"""Drop-ins for the reference's linearization.py on the device.

  linearize_forward_diff_traj(F, X, U, epsx, epsu, relx, relu)   linearization.py:216-262
  linearize_central_diff_traj(F, X, U, epsx, epsu, relx, relu)   linearization.py:177-211
  compute_affine_residuals(F, X, U)                              linearization.py:269-270

Same names, arguments and return shapes (lists of per-step NumPy blocks) for one
trajectory; ``linearize_batch`` is the batched device form (torch tensors in
HBM, the layout engine.propagate_traj / engine.riccati read).  ``F`` must be a
:class:`~time_opt_ilqr_amd.systems.DeviceDynamics` or
:class:`~time_opt_ilqr_amd.systems.SpringChain`, :class:`~time_opt_ilqr_amd.systems.Fleet`
or :class:`~time_opt_ilqr_amd.systems.Team` (a system the kernel knows):
an arbitrary Python callable is refused with TypeError rather than evaluated on
the CPU.
"""
from __future__ import annotations

import numpy as np

from . import engine
from .systems import DeviceDynamics, Fleet, SpringChain, Team


def _check_F(F):
    if not isinstance(F, (DeviceDynamics, SpringChain, Fleet, Team)):
        raise TypeError("F must be a time_opt_ilqr_amd.systems DeviceDynamics (the device "
                        "linearisation has no path for arbitrary Python dynamics)")
    return F


def _sys(F):
    return F if engine.is_object_system(F) else F.system_id


def _run(F, X, U, central, epsx, epsu, relx, relu):
    import torch
    F = _check_F(F)
    X = np.asarray(X, dtype=float)
    U = np.asarray(U, dtype=float)
    if U.ndim == 1:
        U = U.reshape(-1, F.m)
    N = len(U)
    dev = torch.device("cuda", torch.cuda.current_device())
    Xt = torch.as_tensor(np.ascontiguousarray(X[:N + 1]), device=dev)
    if Xt.shape[0] < N + 1:  # the linearisations only read X[:N]
        Xt = torch.cat([Xt, Xt[-1:].expand(N + 1 - Xt.shape[0], -1)], 0)
    Ut = torch.as_tensor(np.ascontiguousarray(U), device=dev)
    return engine.linearize(_sys(F), Xt[None], Ut[None], F.dt, central=central,
                            epsx=epsx, epsu=epsu, relx=relx, relu=relu)


def linearize_forward_diff_traj(F, X, U, epsx: float = 1e-5, epsu: float = 1e-5,
                                relx: float = 1e-6, relu: float = 1e-6):
    """Forward differences with h = max(eps, rel * max(1, |v|)); an all-NaN
    (A_k, B_k) where F(x_k, u_k) is not finite.  Returns (A_list, B_list)."""
    if len(U) == 0:
        return [], []
    r = _run(F, X, U, False, epsx, epsu, relx, relu)
    return list(r.A[0].cpu().numpy()), list(r.B[0].cpu().numpy())


def linearize_central_diff_traj(F, X, U, epsx: float = 1e-5, epsu: float = 1e-5,
                                relx: float = 1e-6, relu: float = 1e-6):
    """Central differences (F(v + h e) - F(v - h e)) / 2h.  Returns (A_list, B_list)."""
    if len(U) == 0:
        return [], []
    r = _run(F, X, U, True, epsx, epsu, relx, relu)
    return list(r.A[0].cpu().numpy()), list(r.B[0].cpu().numpy())


def compute_affine_residuals(F, X, U):
    """[F(x_k, u_k) - x_{k+1}] as (n, 1) columns, k < len(U)."""
    if len(U) == 0:
        return []
    r = _run(F, X, U, False, 1e-5, 1e-5, 1e-6, 1e-6)
    return [a.reshape(-1, 1) for a in r.a_res[0].cpu().numpy()]


def linearize_batch(F, X, U, *, central: bool = False, n_use=None, epsx: float = 1e-5,
                    epsu: float = 1e-5, relx: float = 1e-6, relu: float = 1e-6,
                    want_fx: bool = False) -> "engine.Linearization":
    """Batched form: X [B, N+1, n], U [B, N, m] fp64 device tensors ->
    engine.Linearization(A [B, N, n, n], B [B, N, n, m], a_res [B, N, n])."""
    F = _check_F(F)
    return engine.linearize(_sys(F), X, U, F.dt, central=central, n_use=n_use, epsx=epsx,
                            epsu=epsu, relx=relx, relu=relu, want_fx=want_fx)


def extend_nominal_backward(F, X, U, u_fill, *, S_back: int, preimage_method: str = "fixedpoint",
                            max_iter: int = 6, tol: float = 1e-9, damping: float = 0.5):
    """linearization.py:109-170 with the fixed-point preimage (linearization.py:41-71) on
    the device: (X_ext [S_back + N + 1, n], U_ext [S_back + N, m]).  The Newton and copy
    preimages have no kernel: NotImplementedError.  1 <= S_back <= 64 (S_back <= 0 returns
    copies, as the reference does)."""
    import torch
    F = _check_F(F)
    if engine.is_object_system(F):
        raise NotImplementedError("the negative-time prefix covers the five built-in systems")
    pre = str(preimage_method).lower().strip()
    if pre != "fixedpoint":  # the reference runs its fixed-point step for any other name too
        raise NotImplementedError(f"preimage_method={pre!r}: only 'fixedpoint' runs on the device")
    X = np.asarray(X, dtype=float)
    U = np.asarray(U, dtype=float)
    if U.ndim == 1:
        U = U.reshape(-1, F.m)
    if int(S_back) <= 0:
        return X.copy(), U.copy()
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=float), device=dev)  # noqa: E731
    Xe, Ue = engine.extend_nominal_backward(F.system_id, t(X)[None], t(U)[None],
                                            t(np.asarray(u_fill, dtype=float).reshape(-1)), F.dt,
                                            int(S_back), max_iter=max_iter, tol=tol,
                                            damping=damping)
    return Xe[0].cpu().numpy(), Ue[0].cpu().numpy()
