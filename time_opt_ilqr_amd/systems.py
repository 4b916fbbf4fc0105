"""The reference's benchmark systems (systems.py) with their dynamics on the device.

Each ``make_*`` returns the reference's 13-tuple
``(F, x0, xg, u_ref, Q, R, alpha, w, N, T_min, T_max, wrap_idx, extra)`` with the
same problem data (systems.py:28-349); ``F`` is a :class:`DeviceDynamics`, whose
evaluations run in libhop_amd.so (hop_dynamics_f64 / hop_linearize_f64,
csrc/dynamics.hpp).  ``F(x, u)`` keeps the reference's single-step call
signature; the batched forms are ``F.batch`` and the linearisation drop-ins in
:mod:`time_opt_ilqr_amd.linearization`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from . import engine


@dataclass(frozen=True)
class DeviceDynamics:
    """x_{k+1} = F(x_k, u_k) of system ``system_id`` with step ``dt``."""
    system_id: int
    dt: float
    n: int
    m: int
    name: str = ""

    def __call__(self, x, u):
        """One step for one (x, u) pair, NumPy in / NumPy out (reference call form)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        xt = torch.as_tensor(np.asarray(x, dtype=float).reshape(self.n), device=dev)
        ut = torch.as_tensor(np.asarray(u, dtype=float).reshape(self.m), device=dev)
        return engine.dynamics(self.system_id, xt, ut, self.dt).cpu().numpy()

    def batch(self, X, U):
        """x' for device tensors X [..., n], U [..., m]."""
        return engine.dynamics(self.system_id, X, U, self.dt)


def _F(sid, dt, name):
    n, m = {0: (2, 1), 1: (4, 1), 2: (12, 4), 3: (4, 2), 4: (4, 1)}[sid]
    return DeviceDynamics(sid, float(dt), n, m, name)


def make_double_integrator(dt: float = 0.05, N: int = 120):
    """systems.py:28-50: x = [pos, vel], u = [acc]."""
    F = _F(0, dt, "double_integrator")
    return (F, np.array([1.0, 0.0]), np.array([2.0, 0.0]), np.array([0.0]),
            np.diag([1.0, 0.1]), np.array([[1e-2]]), 50.0, 0.02, N, 10, 80, [], None)


def make_cartpole_swingup(dt: float = 0.02, N: int = 360):
    """systems.py:57-112: x = [cart_pos, cart_vel, theta (0 = down), theta_dot]."""
    F = _F(1, dt, "cartpole")
    return (F, np.zeros(4), np.array([0.0, 0.0, math.pi, 0.0]), np.array([0.0]),
            np.diag([0.01, 0.2, 0.0, 0.2]), np.array([[0.02]]), np.diag([5.0, 5.0, 800.0, 40.0]),
            0.03, N, 40, 320, [2], None)


def make_quadrotor(dt: float = 0.05, N: int = 160):
    """systems.py:119-230: x = [pos, vel, euler (phi, th, psi), omega], u = [thrust, tau];
    F returns all-NaN past its guards (non-finite input, ||x|| > 1e6,
    |cos(pitch)| < 1e-3, |omega| > 1e3)."""
    F = _F(2, dt, "quadrotor")
    x0 = np.zeros(12)
    x0[0:3] = 2.0
    return (F, x0, np.zeros(12), np.array([9.81, 0.0, 0.0, 0.0]),
            np.diag([5, 5, 5, 1, 1, 1, 20, 20, 10, 1, 1, 1]).astype(float),
            np.diag([1e-3, 1e-2, 1e-2, 1e-2]), 300.0, 0.005, N, 40, 160, [6, 7, 8], None)


OBSTACLES = ((np.array([-1.0, -0.5]), 0.65, 6.0), (np.array([0.0, 0.2]), 0.70, 6.0),
             (np.array([1.0, 1.0]), 0.65, 6.0))


def obstacle_stage_cost(x, u=None):
    """The point-mass maker's extra_stage_cost (systems.py:271-293): soft Gaussian
    obstacle penalties -> (c, cx [4], cxx [4, 4]) at one state."""
    p = np.asarray(x[:2], dtype=float)
    c, cx, cxx = 0.0, np.zeros(4), np.zeros((4, 4))
    for o, r, wt in OBSTACLES:
        d = p - o
        ci = wt * math.exp(-float(d @ d) / (2.0 * r * r))
        c += ci
        cx[:2] += -(ci / (r * r)) * d
        cxx[:2, :2] += ci * (np.outer(d, d) / (r ** 4) - np.eye(2) / (r * r))
    return c, cx, cxx


def make_pointmass_navigation(dt: float = 0.05, N: int = 240):
    """systems.py:237-296: 2-D double integrator with obstacle penalties (extra)."""
    F = _F(3, dt, "pointmass")
    extra = dict(obstacles=[dict(center=o, radius=r, weight=wt) for o, r, wt in OBSTACLES],
                 extra_stage_cost=obstacle_stage_cost)
    return (F, np.array([-2.0, -2.0, 0.0, 0.0]), np.array([2.0, 2.0, 0.0, 0.0]), np.zeros(2),
            np.diag([0.0, 0.0, 0.15, 0.15]), np.diag([0.05, 0.05]),
            np.diag([250.0, 250.0, 30.0, 30.0]), 0.06, N, 30, 220, [], extra)


def make_segway_balance(dt: float = 0.02, N: int = 240):
    """systems.py:303-349: linearised wheel-pendulum, x = [x, x_dot, th, th_dot]."""
    F = _F(4, dt, "segway")
    return (F, np.array([0.05, 0.0, 0.08, 0.0]), np.zeros(4), np.array([0.0]),
            np.diag([1.0, 0.1, 25.0, 1.0]), np.array([[0.25]]),
            np.diag([20.0, 2.0, 250.0, 10.0]), 1e-4, N, 40, 200, [2], None)


@dataclass(frozen=True)
class SpringChain:
    """The mass-spring chain as a device system (include/hop_chain.h, csrc/chain.hip):
    x = [q (p positions), v (p velocities)], unit masses between two fixed ends, spring
    force k d + ks sin(d) on the stretch d, damping c, input j on mass j * p // m, one
    explicit Euler step of dt.  Its size is a run-time argument (1 <= m <= p <= 15, so up
    to 30 states): the engine and solver functions take the object itself as ``system`` /
    ``F`` and step with its own dt."""
    p: int
    m: int
    dt: float = 0.1
    k: float = 2.0
    ks: float = 0.5
    c: float = 0.3
    n: int = 0          # 2 p (filled in)
    name: str = "spring_chain"

    def __post_init__(self):
        if not 1 <= int(self.p) <= 15 or not 1 <= int(self.m) <= int(self.p):
            raise ValueError("SpringChain needs 1 <= m <= p <= 15")
        if self.n not in (0, 2 * int(self.p)):
            raise ValueError("SpringChain: n is 2 p")
        if not float(self.dt) > 0.0:
            raise ValueError("SpringChain: dt must be positive")
        object.__setattr__(self, "n", 2 * int(self.p))

    def chain_params(self):
        """(p, m, dt, k, ks, c): what the hop_chain_* entries take."""
        return int(self.p), int(self.m), float(self.dt), float(self.k), float(self.ks), \
            float(self.c)

    def __call__(self, x, u):
        """One step for one (x, u) pair, NumPy in / NumPy out (reference call form)."""
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        xt = torch.as_tensor(np.asarray(x, dtype=float).reshape(self.n), device=dev)
        ut = torch.as_tensor(np.asarray(u, dtype=float).reshape(self.m), device=dev)
        return engine.dynamics(self, xt, ut, self.dt).cpu().numpy()

    def batch(self, X, U):
        """x' for device tensors X [..., n], U [..., m]."""
        return engine.dynamics(self, X, U, self.dt)

    def host(self):
        """The same chain as a host_dynamics.HostDynamics(vectorized=True): the NumPy
        expressions of tests/golden/make_golden_wide.py's chain_dynamics on stacked rows
        (x [K, n], u [K, m] -> [K, n]), evaluated on the host."""
        from .host_dynamics import HostDynamics
        p, m, dt, k, ks, c = self.chain_params()
        act = [j * p // m for j in range(m)]

        def F(x, u):
            x = np.asarray(x, dtype=float)
            u = np.asarray(u, dtype=float)
            one = x.ndim == 1
            x, u = x.reshape(-1, 2 * p), u.reshape(-1, m)
            q, v = x[:, :p], x[:, p:]
            z = np.zeros((x.shape[0], 1))
            d = np.diff(np.concatenate((z, q, z), axis=1), axis=1)
            f = k * d + ks * np.sin(d)
            acc = f[:, 1:] - f[:, :-1] - c * v
            for j, i in enumerate(act):
                acc[:, i] += u[:, j]
            out = np.concatenate((q + dt * v, v + dt * acc), axis=1)
            return out[0] if one else out

        return HostDynamics(F, 2 * p, m, name=self.name + "_host", vectorized=True)


def make_spring_chain(p: int = 12, m: int = 3, dt: float = 0.1, N: int = 60, seed: int = 0,
                      k: float = 2.0, ks: float = 0.5, c: float = 0.3):
    """The chain problem of tests/golden/make_golden_wide.py (problem()): a random start
    (positions uniform in [-1, 1], velocities 0.2 N(0, 1), from ``seed``), the origin as
    goal, Q = diag(1 on positions, 0.2 on velocities), R = 0.1 I, alpha = 20, w = 0.5,
    T in [8, 55]."""
    F = SpringChain(int(p), int(m), float(dt), float(k), float(ks), float(c))
    rng = np.random.default_rng(seed)
    x0 = np.concatenate((rng.uniform(-1.0, 1.0, p), 0.2 * rng.standard_normal(p)))
    Q = np.diag(np.concatenate((np.full(p, 1.0), np.full(p, 0.2))))
    return (F, x0, np.zeros(2 * p), np.zeros(m), Q, 0.1 * np.eye(m), 20.0, 0.5, N, 8,
            min(55, N), [], None)


MAKERS = {"double_integrator": make_double_integrator, "cartpole": make_cartpole_swingup,
          "quadrotor": make_quadrotor, "pointmass": make_pointmass_navigation,
          "segway": make_segway_balance, "spring_chain": make_spring_chain}
