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


# ---- fleets: `count` copies of one built-in system, coupled through the cost -------

def _wrap_pi(a):
    """utils.py:127-128: (a + pi) % (2 pi) - pi"""
    return np.remainder(a + np.pi, 2.0 * np.pi) - np.pi


def _np_di(x, u, dt):
    return np.stack([x[:, 0] + dt * x[:, 1], x[:, 1] + dt * u[:, 0]], -1)


def _np_cartpole(x, u, dt):
    g, m_cart, m_pole, length = 9.81, 1.0, 0.1, 0.5
    total_mass = m_cart + m_pole
    polemass_length = m_pole * length
    th_u = x[:, 2] - math.pi
    costh, sinth = np.cos(th_u), np.sin(th_u)
    temp = (u[:, 0] + polemass_length * x[:, 3] * x[:, 3] * sinth) / total_mass
    denom = length * (4.0 / 3.0 - m_pole * costh * costh / total_mass)
    th_acc = (g * sinth - costh * temp) / denom
    x_acc = temp - polemass_length * th_acc * costh / total_mass
    return np.stack([x[:, 0] + dt * x[:, 1], x[:, 1] + dt * x_acc,
                     _wrap_pi(x[:, 2] + dt * x[:, 3]), x[:, 3] + dt * th_acc], -1)


def _np_quadrotor(x, u, dt):
    m, g, kv, kw = 1.0, 9.81, 0.05, 0.01
    inertia = np.array([0.02, 0.02, 0.04])
    with np.errstate(all="ignore"):
        bad = ~(np.isfinite(x).all(-1) & np.isfinite(u).all(-1))
        bad |= np.sqrt((x * x).sum(-1)) > 1e6
        phi, th, psi, omg = x[:, 6], x[:, 7], x[:, 8], x[:, 9:12]
        bad |= np.abs(np.cos(th)) < 1e-3
        bad |= (np.abs(omg) > 1e3).any(-1)
        s, c = np.sin, np.cos
        # third column of Rb = Rz Ry Rx (the only one the thrust along e3 reaches)
        rb = np.stack([c(psi) * s(th) * c(phi) + s(psi) * s(phi),
                       s(psi) * s(th) * c(phi) - c(psi) * s(phi), c(th) * c(phi)], -1)
        acc = rb * u[:, :1] / m - np.array([0.0, 0.0, g]) - kv * x[:, 3:6]
        t, sec = np.tan(th), 1.0 / np.cos(th)
        eulerdot = np.stack([omg[:, 0] + s(phi) * t * omg[:, 1] + c(phi) * t * omg[:, 2],
                             c(phi) * omg[:, 1] - s(phi) * omg[:, 2],
                             s(phi) * sec * omg[:, 1] + c(phi) * sec * omg[:, 2]], -1)
        omgdot = (u[:, 1:4] - np.cross(omg, omg * inertia)) / inertia - kw * omg
        xn = x + dt * np.concatenate([x[:, 3:6], acc, eulerdot, omgdot], -1)
    return np.where(bad[:, None], np.nan, xn)


def _np_pointmass(x, u, dt):
    return np.stack([x[:, 0] + dt * x[:, 2], x[:, 1] + dt * x[:, 3], x[:, 2] + dt * u[:, 0],
                     x[:, 3] + dt * u[:, 1]], -1)


def _np_segway(x, u, dt):
    g, r, M, m, l = 9.81, 0.15, 1.0, 2.0, 0.5  # noqa: E741
    I = (1.0 / 3.0) * m * l * l  # noqa: E741
    a1, a2, a3 = M + m, m * l, I + m * l * l
    Den = a1 * a3 - a2 * a2
    A_tau, A_th = a3 / (r * Den) - a2 / Den, -(a2 * m * g * l) / Den
    B_tau, B_th = -a2 / (r * Den) + a1 / Den, (a1 * m * g * l) / Den
    xdd = A_tau * u[:, 0] + A_th * x[:, 2]
    thdd = B_tau * u[:, 0] + B_th * x[:, 2]
    return np.stack([x[:, 0] + dt * x[:, 1], x[:, 1] + dt * xdd, _wrap_pi(x[:, 2] + dt * x[:, 3]),
                     x[:, 3] + dt * thdd], -1)


# per system id: (n_s, m_s, name, the maker's wrap_idx, position entries, NumPy F on rows)
_MEMBERS = {0: (2, 1, "double_integrator", (), (0,), _np_di),
            1: (4, 1, "cartpole", (2,), (0,), _np_cartpole),
            2: (12, 4, "quadrotor", (6, 7, 8), (0, 1, 2), _np_quadrotor),
            3: (4, 2, "pointmass", (), (0, 1), _np_pointmass),
            4: (4, 1, "segway", (2,), (0,), _np_segway)}
_MEMBER_MAKERS = {0: make_double_integrator, 1: make_cartpole_swingup, 2: make_quadrotor,
                  3: make_pointmass_navigation, 4: make_segway_balance}
FLEET_MAX_N, FLEET_MAX_M = 31, 16  # include/hop_fleet.h: the wide Riccati pass's limits


PROXIMITY_MAX_OBSTACLES = 16  # include/hop_fleet_proximity.h HOP_FLEET_MAX_OBSTACLES


class Proximity:
    """A fleet's proximity cost (include/hop_fleet_proximity.h): Gaussian bumps
    g(d; r, w) = w exp(-|d|^2 / (2 r^2)) on the members' positions p_a (the leading ``pd``
    entries of a member's state: 1 for DI, cart-pole and segway, 2 for the point mass, 3 for
    the quadrotor).

    ``obstacles`` [K, pd + 2] (centre, radius, weight), K <= 16: g(p_a - o; r, w) for every
    member and row.  ``separation`` (radius, weight) or None: g(p_a - p_b; r_s, w_s) for every
    pair a < b.  Radii must be > 0 and weights finite and >= 0; the column count is checked
    against the fleet's ``pd`` when the object is attached (``Fleet(..., proximity=...)``).

    The second-order term is the positive semidefinite part of a bump's Hessian,
    c d d^T / r^4: the -c I / r^2 term is left out on purpose, so it is not the full Hessian
    of the point-mass obstacle cost (``obstacle_stage_cost``).  With the full Hessian the
    reference's brute-force J curve loses definiteness at useful weights and the
    propagator's J curve flattens until the selected horizon jumps between T_min and T_max.

    The LFT select inverts Q_k + cxx.  A Q that is zero on the position entries, as the
    point-mass maker's is, makes the select degenerate once a rank-one cxx is added: give
    the positions weight.  A fleet's ``obstacles=`` keyword (the point-mass table with the
    full Hessian) stays NotImplementedError."""

    def __init__(self, obstacles=None, separation=None):
        obs = np.zeros((0, 0)) if obstacles is None else np.array(obstacles, dtype=float)
        if obs.size == 0:
            obs = np.zeros((0, 0))
        if obs.ndim != 2:
            raise ValueError("Proximity: obstacles must be [K, pd + 2]")
        if len(obs) > PROXIMITY_MAX_OBSTACLES:
            raise ValueError(f"Proximity: at most {PROXIMITY_MAX_OBSTACLES} obstacles")
        if len(obs):
            if obs.shape[1] < 3:
                raise ValueError("Proximity: obstacles must be [K, pd + 2]")
            if not np.all(np.isfinite(obs[:, :-2])):
                raise ValueError("Proximity: obstacle centres must be finite")
            self._check(obs[:, -2], obs[:, -1], "obstacle")
        obs.setflags(write=False)  # the engine uploads the table once per device
        self.obstacles = obs
        if separation is None:
            self.separation = None
        else:
            r, w = (float(v) for v in separation)
            self._check(np.array([r]), np.array([w]), "separation")
            self.separation = (r, w)

    @staticmethod
    def _check(r, w, what):
        if not (np.all(np.isfinite(r)) and np.all(r > 0.0)):
            raise ValueError(f"Proximity: {what} radii must be finite and > 0")
        if not (np.all(np.isfinite(w)) and np.all(w >= 0.0)):
            raise ValueError(f"Proximity: {what} weights must be finite and >= 0")

    def check_pos_dim(self, pd):
        """the obstacle table's columns against a fleet's position entries"""
        if len(self.obstacles) and self.obstacles.shape[1] != pd + 2:
            raise ValueError(f"Proximity: obstacles have {self.obstacles.shape[1]} columns, "
                             f"a fleet with {pd} position entries needs {pd + 2}")

    def table(self, pd):
        """the obstacle rows [K, pd + 2] (K may be 0)"""
        return self.obstacles.reshape(-1, pd + 2)

    def sep(self):
        """(radius, weight), (1.0, 0.0) for no separation term"""
        return self.separation if self.separation is not None else (1.0, 0.0)


class Fleet:
    """``count`` copies of one built-in system ``base`` (a DeviceDynamics, a system id 0..4
    or a name) as one device system (include/hop_fleet.h, csrc/fleet.hip): x = [x^0 | x^1 |
    ...] and u = [u^0 | u^1 | ...] member-major, F the concatenation of the members' F, the
    members coupled only through dense Q, Qf and R.  n = count n_s <= 31 and m = count m_s
    <= 16.  The engine and solver functions take the object itself as ``system`` / ``F``; it
    steps with the member's own dt unless ``dt`` is given.  ``wrap_idx`` holds the members'
    angle indices, repeated per member.  Calling it evaluates a NumPy twin of F on the host
    (one state, or stacked rows), so ``host()`` wraps the same fleet for comparison.

    ``proximity`` (a :class:`Proximity`) adds obstacle and member-separation bumps on the
    members' ``pos_dim`` position entries as a stage cost evaluated on the device
    (include/hop_fleet_proximity.h): engine.cost_true, engine.forward_linesearch and the
    solver functions then run the proximity entries, and ``stage_cost()`` is its NumPy
    twin."""

    def __init__(self, base, count, dt=None, proximity=None):
        if isinstance(base, DeviceDynamics):
            sid, base_dt = int(base.system_id), float(base.dt)
        else:
            sid = engine.system_id(base)
            base_dt = float(_MEMBER_MAKERS[sid]()[0].dt)
        if sid not in _MEMBERS:
            raise ValueError(f"unknown base system {base!r}")
        ns, ms, name, wrap, pos, f_np = _MEMBERS[sid]
        count = int(count)
        if count < 1:
            raise ValueError("Fleet needs count >= 1")
        if count * ns > FLEET_MAX_N or count * ms > FLEET_MAX_M:
            raise ValueError(f"Fleet: {count} x {name} has n = {count * ns}, m = {count * ms}; "
                             f"the limits are n <= {FLEET_MAX_N} and m <= {FLEET_MAX_M}")
        self.base_id, self.count = sid, count
        self.dt = base_dt if dt is None else float(dt)
        if not self.dt > 0.0:
            raise ValueError("Fleet: dt must be positive")
        self.n_member, self.m_member = ns, ms
        self.n, self.m = count * ns, count * ms
        self.name = f"{name}_x{count}"
        self.wrap_idx = [a * ns + i for a in range(count) for i in wrap]
        self.position_idx = [a * ns + i for a in range(count) for i in pos]
        self._f_np = f_np
        self.pos_dim = len(pos)
        if proximity is not None:
            if not isinstance(proximity, Proximity):
                raise TypeError("Fleet: proximity must be a systems.Proximity")
            proximity.check_pos_dim(self.pos_dim)
        self.proximity = proximity

    def stage_cost(self):
        """The proximity cost as a NumPy callable (x, u) -> (c, cx [n], cxx [n, n]): what
        ``host()`` users pass as ``extra_stage_cost``, and the twin the device kernels are
        tested against.  Zeros for a fleet without a proximity cost."""
        n, ns, pd, count = self.n, self.n_member, self.pos_dim, self.count
        prox = self.proximity
        rows = np.zeros((0, pd + 2)) if prox is None else prox.table(pd)
        r_s, w_s = (1.0, 0.0) if prox is None else prox.sep()

        def cost(x, u=None):
            p = np.asarray(x, dtype=float).reshape(count, ns)[:, :pd]
            c, cx, cxx = 0.0, np.zeros(n), np.zeros((n, n))

            def add(a, b, d, r, w):  # one bump between member a and an obstacle or member b
                nonlocal c
                ci = w * np.exp(-float(d @ d) / (2.0 * r * r))
                g, H = -(ci / (r * r)) * d, ci * np.outer(d, d) / r ** 4
                sa = slice(a * ns, a * ns + pd)
                c += ci
                cx[sa] += g
                cxx[sa, sa] += H
                if b is not None:
                    sb = slice(b * ns, b * ns + pd)
                    cx[sb] -= g
                    cxx[sb, sb] += H
                    cxx[sa, sb] -= H
                    cxx[sb, sa] -= H

            for a in range(count):
                for row in rows:
                    if row[pd + 1] != 0.0:
                        add(a, None, p[a] - row[:pd], row[pd], row[pd + 1])
                if w_s != 0.0:
                    for b in range(a + 1, count):
                        add(a, b, p[a] - p[b], r_s, w_s)
            return c, cx, cxx

        cost.proximity = prox
        return cost

    def fleet_params(self):
        """(system, count, dt): what the hop_fleet_* entries take."""
        return self.base_id, self.count, self.dt

    def __call__(self, x, u):
        """F on the host in NumPy: x [n], u [m] -> [n], or stacked rows [K, n], [K, m]."""
        x = np.asarray(x, dtype=float)
        u = np.asarray(u, dtype=float)
        one = x.ndim == 1
        xr = x.reshape(-1, self.n_member)
        ur = u.reshape(-1, self.m_member)
        out = self._f_np(xr, ur, self.dt).reshape(-1, self.n)
        return out[0] if one else out

    def batch(self, X, U):
        """x' for device tensors X [..., n], U [..., m]."""
        return engine.dynamics(self, X, U, self.dt)

    def host(self):
        """The same fleet as a host_dynamics.HostDynamics(vectorized=True)."""
        from .host_dynamics import HostDynamics
        return HostDynamics(self.__call__, self.n, self.m, name=self.name + "_host",
                            vectorized=True)


def _blockdiag(M, count):
    M = np.atleast_2d(np.asarray(M, dtype=float))
    return np.kron(np.eye(count), M)


FLEET_NOISE = {0: 0.2, 1: 0.05, 2: 0.4, 3: 0.2, 4: 0.02}  # on the position entries of x0


def make_fleet(base, count, N=None, seed=0, coupling=0.5, w_scale=1.0, T_min=None):
    """A joint problem of ``count`` members (tests/golden/make_golden_fleet.py's): the
    member maker's data with its own N unless given and T_max = min(maker's, N - 5); x0 =
    the maker's start plus FLEET_NOISE[system] N(0, 1) from ``seed`` on the position
    entries; Q = blockdiag(Q_member) + coupling Q_member[0, 0] L with L the graph Laplacian
    of a path over the members' first coordinates; R and the terminal weight (returned
    expanded, [n, n]) block-diagonal; w = w_scale times the maker's.  Returns the usual
    13-tuple with F a :class:`Fleet`."""
    F0 = Fleet(base, 1)
    sid = F0.base_id
    mk = _MEMBER_MAKERS[sid]() if N is None else _MEMBER_MAKERS[sid](N=int(N))
    Fm, x0m, xgm, urm, Qm, Rm, alpha, w, Nn, t_min, t_max = mk[:11]
    F = Fleet(Fm, count)
    ns = F.n_member
    rng = np.random.default_rng(seed)
    x0 = np.tile(np.asarray(x0m, dtype=float), F.count)
    x0[F.position_idx] += FLEET_NOISE[sid] * rng.standard_normal(len(F.position_idx))
    Q = _blockdiag(Qm, F.count)
    kappa = float(coupling) * float(np.asarray(Qm)[0, 0])
    first = [a * ns for a in range(F.count)]
    for a, b in zip(first[:-1], first[1:]):
        Q[a, a] += kappa
        Q[b, b] += kappa
        Q[a, b] -= kappa
        Q[b, a] -= kappa
    Qf_m = alpha * np.eye(ns) if np.ndim(alpha) == 0 else np.asarray(alpha, dtype=float)
    return (F, x0, np.tile(np.asarray(xgm, dtype=float), F.count),
            np.tile(np.atleast_1d(np.asarray(urm, dtype=float)), F.count), Q,
            _blockdiag(Rm, F.count), _blockdiag(Qf_m, F.count), float(w) * float(w_scale), int(Nn),
            int(t_min if T_min is None else T_min), int(min(t_max, Nn - 5)), list(F.wrap_idx),
            None)


CROSSING_RADIUS, CROSSING_JITTER, CROSSING_TURN = 2.0, 0.15, 2.2
CROSSING_OBSTACLE, CROSSING_OBS_RADIUS, CROSSING_SEP_RADIUS = (0.3, 0.2, 0.0), 0.5, 0.4


def make_fleet_crossing(base, count, N=None, seed=0, w_scale=1.0, q_pos=0.5, bump_weight=1.5,
                        T_min=None):
    """A crossing problem of ``count`` members with a proximity cost
    (tests/golden/make_golden_fleet_proximity.py's): the member maker's data as in
    :func:`make_fleet`, without the coupling.  The starts' position entries lie on a circle
    of radius 2 (its first ``pd`` coordinates), member a at angle 2 pi a / count + 0.15
    N(0, 1) from ``seed``; the goals are the starts turned by 2.2 rad, so the members cross
    near the centre.  Q gets ``q_pos`` added on the position entries (the select needs
    weight there, see :class:`Proximity`).  One obstacle sits at (0.3, 0.2[, 0]) with radius
    0.5, the separation radius is 0.4, and both bumps weigh ``bump_weight``.  Returns the
    usual 13-tuple with F a :class:`Fleet` that carries the :class:`Proximity`."""
    F0 = Fleet(base, 1)
    sid, pd = F0.base_id, F0.pos_dim
    mk = _MEMBER_MAKERS[sid]() if N is None else _MEMBER_MAKERS[sid](N=int(N))
    Fm, x0m, xgm, urm, Qm, Rm, alpha, w, Nn, t_min, t_max = mk[:11]
    prox = Proximity(
        obstacles=[list(CROSSING_OBSTACLE[:pd]) + [CROSSING_OBS_RADIUS, float(bump_weight)]],
        separation=(CROSSING_SEP_RADIUS, float(bump_weight)))
    F = Fleet(Fm, count, proximity=prox)
    ns = F.n_member
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(F.count) / F.count \
        + CROSSING_JITTER * rng.standard_normal(F.count)
    x0 = np.tile(np.asarray(x0m, dtype=float), F.count)
    xg = np.tile(np.asarray(xgm, dtype=float), F.count)
    for a in range(F.count):
        for ang_a, x in ((ang[a], x0), (ang[a] + CROSSING_TURN, xg)):
            circle = CROSSING_RADIUS * np.array([np.cos(ang_a), np.sin(ang_a), 0.0])
            x[a * ns:a * ns + pd] = circle[:pd]
    Q = _blockdiag(Qm, F.count)
    Q[F.position_idx, F.position_idx] += float(q_pos)
    Qf_m = alpha * np.eye(ns) if np.ndim(alpha) == 0 else np.asarray(alpha, dtype=float)
    return (F, x0, xg, np.tile(np.atleast_1d(np.asarray(urm, dtype=float)), F.count), Q,
            _blockdiag(Rm, F.count), _blockdiag(Qf_m, F.count), float(w) * float(w_scale), int(Nn),
            int(t_min if T_min is None else T_min), int(min(t_max, Nn - 5)), list(F.wrap_idx),
            None)


# ---- teams: members of different built-in systems, coupled through the cost ---------

TEAM_MAX_MEMBERS = 15  # include/hop_team.h HOP_TEAM_MAX_MEMBERS


class Team:
    """Members of different built-in systems as one device system (include/hop_team.h,
    csrc/team.hip).  ``members`` is a sequence of DeviceDynamics, system ids 0..4 or names,
    1 to 15 of them; member a owns states ``[x_offsets[a], x_offsets[a] + n_s(a))`` and
    inputs ``[u_offsets[a], u_offsets[a] + m_s(a))``, the offsets being the running sums in
    member order.  F is the concatenation of the members' F at one shared step ``dt``, the
    members coupled only through dense Q, Qf and R; n = sum n_s <= 31 and m = sum m_s <= 16.
    The shared step is ``dt`` if given, else the members' own, which must then agree
    (cart-pole and segway default to 0.02, the others to 0.05).  The engine and solver
    functions take the object itself as ``system`` / ``F``, wherever they take a
    :class:`Fleet` without a proximity cost; a team of equal members computes that fleet's
    numbers bit for bit.  ``wrap_idx`` and ``position_idx`` hold the members' angle and
    position indices shifted by their offsets.  Calling it evaluates a NumPy twin of F on
    the host (one state, or stacked rows), so ``host()`` wraps the same team for comparison.

    ``with_proximity(prox)`` returns the same team carrying a :class:`Proximity` as a stage
    cost evaluated on the device (include/hop_mixed_proximity.h); ``proximity`` is None
    otherwise.  The members' positions differ in dimension (``pos_dims``), so they live in a
    common workspace of dimension ``pos_dim`` = max(pos_dims): member a's workspace position
    is its leading ``pos_dims[a]`` state entries padded with zeros -- a DI moves on the x
    axis, a point mass in the plane z = 0, a quadrotor in space -- the obstacle table is
    [K, pos_dim + 2], and a bump's gradient and second-order block are restricted to the
    coordinates a member has.  engine.cost_true, engine.forward_linesearch and the solver
    functions then run the proximity entries, and ``stage_cost()`` is the NumPy twin; a team
    of equal members computes the numbers of that :class:`Fleet` with the same cost bit for
    bit."""

    proximity = None

    def __init__(self, members, dt=None):
        try:
            members = list(members)
        except TypeError:
            raise ValueError("Team: members must be a sequence of systems") from None
        if not 1 <= len(members) <= TEAM_MAX_MEMBERS:
            raise ValueError(f"Team needs 1 to {TEAM_MAX_MEMBERS} members, got {len(members)}")
        ids, dts = [], []
        for mem in members:
            if isinstance(mem, DeviceDynamics):
                sid, own = mem.system_id, float(mem.dt)
            else:
                try:
                    sid = engine.system_id(mem)
                except ValueError:
                    raise ValueError(f"Team: unknown member {mem!r}") from None
                own = None
            if not isinstance(sid, (int, np.integer)) or int(sid) not in _MEMBERS:
                raise ValueError(f"Team: unknown member {mem!r}")
            sid = int(sid)
            ids.append(sid)
            dts.append(float(_MEMBER_MAKERS[sid]()[0].dt) if own is None else own)
        self.member_ids = tuple(ids)
        sizes = [_MEMBERS[s][:2] for s in ids]
        self.n, self.m = sum(s[0] for s in sizes), sum(s[1] for s in sizes)
        if self.n > FLEET_MAX_N or self.m > FLEET_MAX_M:
            raise ValueError(f"Team: n = {self.n}, m = {self.m}; the limits are "
                             f"n <= {FLEET_MAX_N} and m <= {FLEET_MAX_M}")
        if dt is None:
            if len(set(dts)) != 1:
                raise ValueError(f"Team: the members' own steps differ ({sorted(set(dts))}): "
                                 "give the shared dt")
            self.dt = dts[0]
        else:
            self.dt = float(dt)
        if not self.dt > 0.0:
            raise ValueError("Team: dt must be positive")
        self.x_offsets = tuple(int(v) for v in np.cumsum([0] + [s[0] for s in sizes[:-1]]))
        self.u_offsets = tuple(int(v) for v in np.cumsum([0] + [s[1] for s in sizes[:-1]]))
        self.wrap_idx = [xo + i for s, xo in zip(ids, self.x_offsets) for i in _MEMBERS[s][3]]
        self.position_idx = [xo + i for s, xo in zip(ids, self.x_offsets)
                             for i in _MEMBERS[s][4]]
        self.name = "team_" + "+".join(_MEMBERS[s][2] for s in ids)
        self.pos_dims = tuple(len(_MEMBERS[s][4]) for s in ids)
        self.pos_dim = max(self.pos_dims)

    def with_proximity(self, prox):
        """A new team, equal otherwise, that carries the :class:`Proximity` ``prox`` (its
        obstacle table in ``pos_dim`` + 2 columns)."""
        if not isinstance(prox, Proximity):
            raise TypeError("Team.with_proximity: prox must be a systems.Proximity")
        prox.check_pos_dim(self.pos_dim)
        out = Team(self.member_ids, dt=self.dt)
        out.proximity = prox
        return out

    def stage_cost(self):
        """The proximity cost as a NumPy callable (x, u) -> (c, cx [n], cxx [n, n]): what
        ``host()`` users pass as ``extra_stage_cost``, and the twin the device kernels are
        tested against.  Zeros for a team without a proximity cost."""
        n, D, count = self.n, self.pos_dim, len(self.member_ids)
        xo, pds = self.x_offsets, self.pos_dims
        prox = self.proximity
        rows = np.zeros((0, D + 2)) if prox is None else prox.table(D)
        r_s, w_s = (1.0, 0.0) if prox is None else prox.sep()

        def cost(x, u=None):
            x = np.asarray(x, dtype=float).reshape(-1)
            p = np.zeros((count, D))
            for a in range(count):
                p[a, :pds[a]] = x[xo[a]:xo[a] + pds[a]]
            c, cx, cxx = 0.0, np.zeros(n), np.zeros((n, n))

            def add(a, b, d, r, w):  # one bump between member a and an obstacle or member b
                nonlocal c
                ci = w * np.exp(-float(d @ d) / (2.0 * r * r))
                g, H = -(ci / (r * r)) * d, ci * np.outer(d, d) / r ** 4
                pa = pds[a]
                sa = slice(xo[a], xo[a] + pa)
                c += ci
                cx[sa] += g[:pa]
                cxx[sa, sa] += H[:pa, :pa]
                if b is not None:
                    pb = pds[b]
                    sb = slice(xo[b], xo[b] + pb)
                    cx[sb] -= g[:pb]
                    cxx[sb, sb] += H[:pb, :pb]
                    cxx[sa, sb] -= H[:pa, :pb]
                    cxx[sb, sa] -= H[:pb, :pa]

            for a in range(count):
                for row in rows:
                    if row[D + 1] != 0.0:
                        add(a, None, p[a] - row[:D], row[D], row[D + 1])
                if w_s != 0.0:
                    for b in range(a + 1, count):
                        add(a, b, p[a] - p[b], r_s, w_s)
            return c, cx, cxx

        cost.proximity = prox
        return cost

    def team_params(self):
        """(member system ids, dt): what the hop_team_* entries take."""
        return self.member_ids, self.dt

    def __call__(self, x, u):
        """F on the host in NumPy: x [n], u [m] -> [n], or stacked rows [K, n], [K, m]."""
        x = np.asarray(x, dtype=float)
        u = np.asarray(u, dtype=float)
        one = x.ndim == 1
        xr, ur = x.reshape(-1, self.n), u.reshape(-1, self.m)
        out = np.empty_like(xr)
        for sid, xo, uo in zip(self.member_ids, self.x_offsets, self.u_offsets):
            ns, ms, f_np = _MEMBERS[sid][0], _MEMBERS[sid][1], _MEMBERS[sid][5]
            out[:, xo:xo + ns] = f_np(xr[:, xo:xo + ns], ur[:, uo:uo + ms], self.dt)
        return out[0] if one else out

    def batch(self, X, U):
        """x' for device tensors X [..., n], U [..., m]."""
        return engine.dynamics(self, X, U, self.dt)

    def host(self):
        """The same team as a host_dynamics.HostDynamics(vectorized=True)."""
        from .host_dynamics import HostDynamics
        return HostDynamics(self.__call__, self.n, self.m, name=self.name + "_host",
                            vectorized=True)


def _blocks(mats):
    mats = [np.atleast_2d(np.asarray(M, dtype=float)) for M in mats]
    out = np.zeros((sum(len(M) for M in mats),) * 2)
    o = 0
    for M in mats:
        out[o:o + len(M), o:o + len(M)] = M
        o += len(M)
    return out


def make_team(members, N=None, seed=0, coupling=0.5, w_scale=1.0, T_min=None, dt=None):
    """A joint problem of mixed members (tests/golden/make_golden_team.py's): every
    member's maker is called with the team's dt and N (N = the smallest of the makers' own
    unless given).  x0 = the makers' starts plus FLEET_NOISE[kind] N(0, 1) from ``seed`` on
    the position entries, drawn in member order, then entry order.  Q = the block diagonal
    of the members' Q plus a path Laplacian over consecutive members' first coordinates
    with, for members a and a + 1, kappa = coupling min(Q_a[0, 0], Q_a+1[0, 0]) (both taken
    before any coupling is added), or coupling max(Q_a[0, 0], Q_a+1[0, 0], 1) where that
    minimum is 0.  R and the terminal weight (returned expanded, [n, n]) are block diagonal,
    w = w_scale times the largest of the makers', T_max = min(the makers', N - 5) and T_min
    the largest of the makers' unless given.  Returns the usual 13-tuple with F a
    :class:`Team`."""
    F = Team(members, dt=dt)
    if N is None:
        N = min(int(_MEMBER_MAKERS[s]()[8]) for s in F.member_ids)
    N = int(N)
    mks = [_MEMBER_MAKERS[s](dt=F.dt, N=N) for s in F.member_ids]
    rng = np.random.default_rng(seed)
    x0 = np.concatenate([np.asarray(mk[1], dtype=float) for mk in mks])
    for sid, xo in zip(F.member_ids, F.x_offsets):
        pos = [xo + i for i in _MEMBERS[sid][4]]
        x0[pos] += FLEET_NOISE[sid] * rng.standard_normal(len(pos))
    Q = _blocks([mk[4] for mk in mks])
    q00 = [float(np.asarray(mk[4], dtype=float)[0, 0]) for mk in mks]
    for a in range(len(mks) - 1):
        lo = min(q00[a], q00[a + 1])
        kappa = float(coupling) * (lo if lo != 0.0 else max(q00[a], q00[a + 1], 1.0))
        i, j = F.x_offsets[a], F.x_offsets[a + 1]
        Q[i, i] += kappa
        Q[j, j] += kappa
        Q[i, j] -= kappa
        Q[j, i] -= kappa
    Qf = _blocks([mk[6] * np.eye(len(mk[1])) if np.ndim(mk[6]) == 0 else mk[6] for mk in mks])
    return (F, x0, np.concatenate([np.asarray(mk[2], dtype=float) for mk in mks]),
            np.concatenate([np.atleast_1d(np.asarray(mk[3], dtype=float)) for mk in mks]), Q,
            _blocks([mk[5] for mk in mks]), Qf, float(w_scale) * max(float(mk[7]) for mk in mks),
            N, int(max(int(mk[9]) for mk in mks) if T_min is None else T_min),
            int(min(min(int(mk[10]) for mk in mks), N - 5)), list(F.wrap_idx), None)


def make_team_crossing(members, N=None, seed=0, w_scale=1.0, q_pos=0.5, bump_weight=1.5,
                       T_min=None, dt=None):
    """A crossing problem of mixed members with a proximity cost
    (tests/golden/make_golden_team_proximity.py's): :func:`make_fleet_crossing`'s recipe on
    the members of a :class:`Team`.  Every member's maker is called with the team's dt and N,
    and N, T_min and T_max follow :func:`make_team`'s rules; there is no Laplacian coupling.
    The starts' position entries lie on the circle of radius 2, member a at angle
    2 pi a / count + 0.15 N(0, 1) from ``seed`` taking the circle's first ``pos_dims[a]``
    coordinates; the goals are the starts turned by 2.2 rad.  Q gets ``q_pos`` added on the
    position entries, one obstacle sits at (0.3, 0.2, 0)[:pos_dim] with radius 0.5, the
    separation radius is 0.4, and both bumps weigh ``bump_weight``.  Returns the usual
    13-tuple with F a :class:`Team` that carries the :class:`Proximity`."""
    F0 = Team(members, dt=dt)
    if N is None:
        N = min(int(_MEMBER_MAKERS[s]()[8]) for s in F0.member_ids)
    N = int(N)
    mks = [_MEMBER_MAKERS[s](dt=F0.dt, N=N) for s in F0.member_ids]
    D, count = F0.pos_dim, len(F0.member_ids)
    prox = Proximity(
        obstacles=[list(CROSSING_OBSTACLE[:D]) + [CROSSING_OBS_RADIUS, float(bump_weight)]],
        separation=(CROSSING_SEP_RADIUS, float(bump_weight)))
    F = F0.with_proximity(prox)
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(count) / count + CROSSING_JITTER * rng.standard_normal(count)
    x0 = np.concatenate([np.asarray(mk[1], dtype=float) for mk in mks])
    xg = np.concatenate([np.asarray(mk[2], dtype=float) for mk in mks])
    for a, (xo, pd) in enumerate(zip(F.x_offsets, F.pos_dims)):
        for ang_a, x in ((ang[a], x0), (ang[a] + CROSSING_TURN, xg)):
            circle = CROSSING_RADIUS * np.array([np.cos(ang_a), np.sin(ang_a), 0.0])
            x[xo:xo + pd] = circle[:pd]
    Q = _blocks([mk[4] for mk in mks])
    Q[F.position_idx, F.position_idx] += float(q_pos)
    Qf = _blocks([mk[6] * np.eye(len(mk[1])) if np.ndim(mk[6]) == 0 else mk[6] for mk in mks])
    return (F, x0, xg,
            np.concatenate([np.atleast_1d(np.asarray(mk[3], dtype=float)) for mk in mks]), Q,
            _blocks([mk[5] for mk in mks]), Qf, float(w_scale) * max(float(mk[7]) for mk in mks),
            N, int(max(int(mk[9]) for mk in mks) if T_min is None else T_min),
            int(min(min(int(mk[10]) for mk in mks), N - 5)), list(F.wrap_idx), None)
