"""CPU: teams, mixed fleets of the built-in systems as device systems (include/hop_team.h).

* the six entries are exported and bound in a table of their own, stay out of the other
  headers and tables, and the header and sources are in the build lists;
* every entry validates its arguments on the host before any launch;
* systems.Team / make_team, the scope refusals and the routing by shape;
* the host build of csrc/team_math.hpp (team_host.cpp: team.hip's per-member arithmetic)
  against the members' host dynamics (dyn_host.cpp), bitwise, with every off-block entry
  an exact 0.0, its NaN pattern against the reference's fixtures, and the same file as a
  stand-alone program under AddressSanitizer and UBSan.
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
CSRC = os.path.join(REPO, "time_opt_ilqr_amd", "csrc")
NAMES = ["hop_team_cost_true_f64", "hop_team_dynamics_f64", "hop_team_forward_linesearch_f64",
         "hop_team_forward_workspace_bytes", "hop_team_linearize_f64", "hop_team_rollout_f64"]
# member ids, n, m, dt (the issue's table)
SHAPES = {"all5": ((0, 1, 2, 3, 4), 26, 9, 0.02), "pm_quad_di": ((3, 2, 0), 18, 7, 0.05),
          "di2_pm2": ((0, 0, 3, 3), 12, 6, 0.05), "quad_pm3": ((2, 3, 3, 3), 24, 10, 0.05),
          "quad_di4_pm2": ((2, 0, 0, 0, 0, 3, 3), 28, 12, 0.05),
          "pm7_di": ((3,) * 7 + (0,), 30, 15, 0.05), "cp2_seg3": ((1, 1, 4, 4, 4), 20, 5, 0.02)}
SIZES = {0: (2, 1), 1: (4, 1), 2: (12, 4), 3: (4, 2), 4: (4, 1)}
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-fno-builtin-sin", "-fno-builtin-cos",
       "-fno-builtin-tan", "-DHOP_HD="]
_P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _gxx(tmp, name):
    so = str(tmp / f"lib{name}.so")
    subprocess.check_call(GXX + ["-O2", "-shared", "-fPIC", os.path.join(CSRC, name + ".cpp"),
                                 "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """g++ builds of csrc/team_math.hpp (team_host.cpp) and of the members' own
    dynamics.hpp (dyn_host.cpp)"""
    d = tmp_path_factory.mktemp("team")
    th, dh = _gxx(d, "team_host"), _gxx(d, "dyn_host")
    lin = [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_double] * 4 + [_P] * 4
    th.team_host_shape.argtypes = [C.c_int, _P, _P, _P]
    th.team_host_dynamics.argtypes = [C.c_int, _P, C.c_double, _P, _P, C.c_int64, _P]
    th.team_host_linearize.argtypes = [C.c_int, _P, C.c_double] + lin
    dh.dyn_host_linearize.argtypes = [C.c_int, C.c_double] + lin
    return th, dh


def _p(a):
    return a.ctypes.data_as(_P)


def _ids(ids):
    return np.ascontiguousarray(ids, dtype=np.int32)


def _offsets(ids):
    xo = np.cumsum([0] + [SIZES[s][0] for s in ids[:-1]]).tolist()
    uo = np.cumsum([0] + [SIZES[s][1] for s in ids[:-1]]).tolist()
    return xo, uo


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


# ---------------------------------------------------------------- the ABI
def test_team_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_team.h") == NAMES
    assert sorted(_lib.TEAM_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    headers = sorted(h for h in os.listdir(os.path.join(REPO, "include")) if h.endswith(".h"))
    assert "hop_team.h" in headers and "hop_fleet.h" in headers
    others = set()
    for h in headers:
        if h != "hop_team.h":
            others |= set(_functions(h))
            assert "hop_team" not in open(os.path.join(REPO, "include", h)).read(), h
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        assert name not in others
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES, _lib.FLEET_SIGNATURES,
                      _lib.FLEET_PROXIMITY_SIGNATURES, _lib.ONEPASS_SIGNATURES,
                      _lib.TESTHOOK_SIGNATURES):
            assert name not in table
        # hop_fleet.h's list with the team's parameters in place of the fleet's
        assert _lib.TEAM_SIGNATURES[name] == _lib.FLEET_SIGNATURES[name.replace("team", "fleet")]
    assert len(_functions("hop.h")) == 40 and lib.hop_abi_version() == 1
    text = open(os.path.join(REPO, "include", "hop_team.h")).read()
    assert f"#define HOP_TEAM_MAX_MEMBERS {_lib.TEAM_MAX_MEMBERS} " in text
    assert C.sizeof(_lib.TeamParams) == 72 and _lib.TeamParams.dt.offset == 64


def test_team_sources_are_in_the_build_lists():
    from time_opt_ilqr_amd import build
    assert "hop_team.h" in inspect.getsource(build._digest)
    assert "team.hip" in build.SOURCES and "team_math.hpp" in build.HEADERS


# ---------------------------------------------------------------- validation
def _params(ids=(3, 2, 0), dt=0.05, count=None):
    from time_opt_ilqr_amd import _lib
    par = _lib.TeamParams()
    par.count, par.dt = len(ids) if count is None else count, dt
    for a, s in enumerate(ids[:15]):
        par.system[a] = s
    return par


D = C.c_void_p(16)  # never dereferenced: every call here ends on the host


def _calls(lib, par, *, batch=4, null=False, n_alloc=10, n_use=10, n_alpha=5, ws=1 << 40,
           wrap=0, stride=64, only=None):
    """every launching entry (or the one named) with the same bad or empty arguments:
    name -> rc.  Every call made here must end on the host."""
    q = None if null else D
    pp = C.byref(par) if par is not None else None
    al = (C.c_double * 8)(*([1.0] * 8))
    cost = (q, 0, q, 0, q, q, q, q, 0, wrap)
    fns = {
        "dynamics": lambda: lib.hop_team_dynamics_f64(pp, q, stride, q, stride, batch, q, stride,
                                                      None),
        "rollout": lambda: lib.hop_team_rollout_f64(pp, q, 0, q, batch, n_alloc, 1e6, q, None),
        "linearize": lambda: lib.hop_team_linearize_f64(pp, q, q, batch, n_alloc, n_use, 1, 1e-5,
                                                        1e-5, 1e-6, 1e-6, q, q, q, q, None),
        "cost": lambda: lib.hop_team_cost_true_f64(pp, q, q, q, *cost, batch, n_alloc, q, None),
        "linesearch": lambda: lib.hop_team_forward_linesearch_f64(
            pp, q, q, *cost, q, q, q, q, al, n_alpha, batch, n_alloc, q, ws, q, q, q, q, q, None),
    }
    return {k: f() for k, f in fns.items() if only in (None, k)}


def test_team_validation_without_gpu(lib):
    err = lib.hop_last_error
    wsb = lambda par: lib.hop_team_forward_workspace_bytes(C.byref(par), 4, 10, 5)  # noqa: E731
    # every shape of the issue's table is accepted; an empty batch launches nothing
    for tag, (ids, n, m, dt) in SHAPES.items():
        ok = _params(ids, dt)
        assert wsb(ok) == 4 * 5 * (1 + 11 * n + 10 * m) * 8, tag
        assert all(rc == 0 for rc in _calls(lib, ok, batch=0).values()), tag
    assert wsb(_params((0,) * 15)) > 0 and wsb(_params((3,) * 7 + (0,))) > 0
    # HOP_E_SIZE: count outside 1..15
    for count in (0, -2, 16, 1 << 20):
        par = _params((0,) * 15, count=count)
        assert all(rc == -2 for rc in _calls(lib, par).values()), count
        assert b"count must be in [1, 15]" in err()
        assert wsb(par) == 0
        assert all(rc == -2 for rc in _calls(lib, par, batch=0).values())  # an empty batch too
    # HOP_E_SIZE: n > 31 or m > 16 -- the first teams that do not fit
    for ids in ((2, 2, 1, 1), (2, 2, 2), (3,) * 8, (3,) * 7 + (0, 0), (1,) * 8, (0, 2, 2, 4, 4)):
        par = _params(ids)
        assert all(rc == -2 for rc in _calls(lib, par).values()), ids
        assert b"n must be <= 31 and m <= 16" in err()
        assert wsb(par) == 0
    # HOP_E_ARG: an unknown member, wherever it stands
    for ids in ((5,), (0, -1), (3, 2, 0, 7), (0,) * 14 + (9,)):
        par = _params(ids)
        assert all(rc == -1 for rc in _calls(lib, par).values()), ids
        assert b"unknown member system" in err()
        assert wsb(par) == 0
    for dt in (0.0, -0.1, float("nan")):
        assert all(rc == -1 for rc in _calls(lib, _params(dt=dt)).values())
        assert b"dt must be positive" in err()
    par = _params()  # point mass, quadrotor, DI: n = 18, m = 7
    assert all(rc == -1 for rc in _calls(lib, par, null=True).values())
    assert b"null" in err()
    assert all(rc == -1 for rc in _calls(lib, None).values())
    assert b"null team parameters" in err()
    one = lambda name, **kw: _calls(lib, par, only=name, **kw)[name]  # noqa: E731
    assert one("linearize", n_use=11) == -1 and b"n_use > n_alloc" in err()
    for na in (0, 9):
        assert one("linesearch", n_alpha=na) == -1 and b"n_alpha" in err()
    need = wsb(par)
    assert need == 4 * 5 * (1 + 11 * 18 + 10 * 7) * 8
    assert one("linesearch", ws=need - 1) == -1 and b"workspace too small" in err()
    assert one("dynamics", stride=17) == -1 and b"stride" in err()
    # wrap bits at or above n = 18
    for name in ("cost", "linesearch"):
        assert one(name, wrap=1 << 18) == -1 and b"wrap bits" in err(), name
        assert one(name, wrap=1 << 31) == -1
        assert one(name, wrap=7 << 10, batch=0) == 0
    # negative sizes
    assert all(rc == -1 for rc in _calls(lib, par, batch=-1).values())
    assert one("rollout", n_alloc=-1) == -1 and one("cost", n_alloc=-1) == -1
    assert one("linesearch", n_alloc=-1) == -1 and one("linearize", n_alloc=-1, n_use=-1) == -1
    assert lib.hop_team_rollout_f64(C.byref(par), D, -1, D, 4, 10, 1e6, D, None) == -1
    # too many rows for one launch
    assert all(rc == -2 for rc in _calls(lib, par, batch=1 << 40).values())
    # an empty batch launches nothing, with or without pointers; so does n_use = 0
    assert all(rc == 0 for rc in _calls(lib, par, batch=0).values())
    assert all(rc == 0 for rc in _calls(lib, par, batch=0, null=True).values())
    assert one("linearize", n_use=0) == 0


# ---------------------------------------------------------------- the object
def test_team_object_and_refusals_without_gpu():
    from time_opt_ilqr_amd import engine, host_dynamics, linearization, onepass, solver, systems
    F = systems.Team(["pointmass", systems.make_quadrotor()[0], 0])
    assert (F.n, F.m, F.dt, F.member_ids) == (18, 7, 0.05, (3, 2, 0))
    assert F.x_offsets == (0, 4, 16) and F.u_offsets == (0, 2, 6)
    assert F.wrap_idx == [10, 11, 12] and F.position_idx == [0, 1, 4, 5, 6, 16]
    assert F.team_params() == ((3, 2, 0), 0.05) and isinstance(F.name, str) and F.name
    assert engine.is_team(F) and not engine.is_fleet(F) and not engine.is_chain(F)
    assert engine.is_object_system(F) and engine.system_dims(F) == (18, 7)
    assert not engine.is_team(2) and not engine.is_team("quadrotor")
    assert not engine.is_team(systems.Fleet(0, 2)) and not engine.is_team(systems.SpringChain(4, 2))
    assert solver._on_device(F) and solver._sys(F) is F and linearization._sys(F) is F
    par = engine._team_params(F)
    assert (par.count, list(par.system)[:3], par.dt) == (3, [3, 2, 0], 0.05)
    for tag, (ids, n, m, dt) in SHAPES.items():
        T = systems.Team(ids, dt=dt)
        assert (T.n, T.m, T.dt) == (n, m, dt), tag
        xo, uo = _offsets(ids)
        assert list(T.x_offsets) == xo and list(T.u_offsets) == uo
    assert systems.Team([1, 4]).dt == 0.02 and systems.Team([0] * 15).n == 30
    assert systems.Team([systems.make_segway_balance(dt=0.05)[0], 0]).dt == 0.05
    # Team's own errors
    for members in ([], (), [0] * 16, [5], ["unicycle"], [0, None], [2, 2, 2], [3] * 8, [1] * 8,
                    [0, 1], ["quadrotor", "segway"], 3):
        with pytest.raises(ValueError):
            systems.Team(members)
    for dt in (0.0, -0.05, float("nan")):
        with pytest.raises(ValueError):
            systems.Team([0, 3], dt=dt)
    with pytest.raises(TypeError):
        systems.Team([0, 3], proximity=systems.Proximity(separation=(0.4, 1.0)))
    # Fleet is unchanged: it takes one base, not a list
    with pytest.raises(ValueError):
        systems.Fleet([0, 3], 2)
    # callable: the NumPy twin, which HostDynamics wraps
    H = F.host()
    assert isinstance(H, host_dynamics.HostDynamics) and (H.n, H.m) == (18, 7) and H.vectorized
    rng = np.random.default_rng(3)
    x, u = rng.uniform(-1, 1, (4, 18)), rng.uniform(-1, 1, (4, 7))
    assert F(x, u).shape == (4, 18) and np.array_equal(F(x[1], u[1]), F(x, u)[1])
    assert np.array_equal(F(x, u)[:, 16:], systems.Fleet(0, 1)(x[:, 16:], u[:, 6:]))
    assert np.array_equal(F(x, u)[:, 4:16], systems.Fleet(2, 1)(x[:, 4:16], u[:, 2:6]))
    mk = systems.make_team([3, 2, 0], N=80, seed=1)
    assert len(mk) == 13 and isinstance(mk[0], systems.Team) and mk[12] is None
    F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap = mk[:12]
    assert (N, T_min, T_max, wrap, w) == (80, 40, 75, [10, 11, 12], 0.06)
    # the point mass has Q[0, 0] = 0: kappa = 0.5 max(0, 5, 1); then 0.5 min(5, 1)
    assert Q[0, 4] == -2.5 and Q[0, 0] == 2.5 and Q[4, 4] == 5.0 + 2.5 + 0.5
    assert Q[4, 16] == -0.5 and Q[16, 16] == 1.5 and Q[0, 16] == 0.0 and Q[1, 5] == 0.0
    assert Qf.shape == (18, 18) and R.shape == (7, 7) and ur.tolist() == [0, 0, 9.81, 0, 0, 0, 0]
    # onepass, a Python stage cost and the obstacle table are out of scope
    stage = lambda x, u: (0.0, np.zeros(18), np.zeros((18, 18)))  # noqa: E731
    for call in (
        lambda: solver.ilqr_timeopt_batch(F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                          method="onepass"),
        lambda: solver.ilqr_timeopt(F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, method="onepass"),
        lambda: solver.ilqr_timeopt_batch(F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                          extra_stage_cost=stage),
        lambda: solver.ilqr_timeopt(F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                    extra_stage_cost=stage),
        lambda: solver.ilqr_timeopt_batch(F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max,
                                          obstacles=np.array([[0.0, 0.0, 1.0, 1.0]])),
        lambda: engine._onepass_system(F),
        lambda: linearization.extend_nominal_backward(F, np.zeros((3, 18)), np.zeros((2, 7)),
                                                      ur, S_back=4),
    ):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(NotImplementedError, match="team"):
        onepass.check_scope(F, 20, "fixedpoint")


def _solve_fixtures():
    return sorted(f for f in os.listdir(GOLDEN) if re.fullmatch(r"team_solve_\w+_\d\.npz", f))


def test_make_team_rebuilds_the_fixture_problems():
    """systems.make_team and tests/golden/make_golden_team.py's problem() are one recipe"""
    from time_opt_ilqr_amd import systems
    names = _solve_fixtures()
    tags = {n[len("team_solve_"):-6] for n in names}
    assert {"di2_pm2", "quad_pm3", "quad_di4_pm2"} <= tags <= set(SHAPES)
    for name in names:
        d = np.load(os.path.join(GOLDEN, name))
        ids, n, m, dt = SHAPES[name[len("team_solve_"):-6]]
        assert tuple(d["members"].tolist()) == ids and float(d["dt"]) == dt
        mk = systems.make_team(ids, N=int(d["N"]), seed=int(d["seed"]), dt=dt,
                               w_scale=float(d["scale"]), T_min=int(d["T_min"]))
        for got, key in zip(mk[1:7], ("x0", "xg", "u_ref", "Q", "R", "Qf")):
            assert np.array_equal(got, d[key]), (name, key)
        assert mk[7] == float(d["w"]) and mk[8:11] == (int(d["N"]), int(d["T_min"]), int(d["T_max"]))
        assert mk[11] == d["wrap_idx"].tolist() == mk[0].wrap_idx
        for method in ("propagator", "bruteforce"):
            assert float(d[f"gaps_{method}"].min()) >= 1e-3 and len(d[f"T_hist_{method}"]) >= 2


def test_sharded_solver_passes_the_team_through(monkeypatch):
    import torch
    from time_opt_ilqr_amd import distributed, solver, systems
    seen = {}

    def fake(system, x0, *a, **k):
        seen["system"], seen["kw"] = system, k
        B = len(x0)
        return dict(n_hist=torch.ones(B, dtype=torch.int32), J_hist=torch.ones(B, 2),
                    T_star=torch.full((B,), 16, dtype=torch.int32),
                    crashed=torch.zeros(B, dtype=torch.int32))

    monkeypatch.setattr(solver, "ilqr_timeopt_batch", fake)
    mk = systems.make_team([0, 0, 3, 3], N=80)
    full, local, (lo, hi) = distributed.ilqr_timeopt_sharded(
        mk[0], np.stack([mk[1]] * 3), *mk[2:7], mk[7], 80, 10, 75, device=torch.device("cpu"),
        wrap_idx=mk[11], method="bruteforce")
    assert seen["system"] is mk[0] and (lo, hi) == (0, 3)
    assert full["T_star"].tolist() == [16, 16, 16]


# ---------------------------------------------------------------- routing by shape
class _Recorder:
    """stands in for the loaded library: records the entries called, launches nothing"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append(name)
            return 0
        return fn


@pytest.mark.parametrize("tag,wide", [("di2_pm2", False), ("pm_quad_di", True),
                                      ("quad_pm3", True), ("pm7_di", True)])
def test_team_routing_by_shape(monkeypatch, tag, wide):
    """the team's own entries step it, and the select and Riccati kernels are chosen by
    shape alone -- n <= 15 the narrow select, n >= 16 the wide one; the Riccati pass is
    wide from n = 17, as for every other system"""
    import torch
    from time_opt_ilqr_amd import _lib, engine, systems
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda path=None: rec)
    monkeypatch.setattr(_lib, "stream_handle", lambda device=None: None)
    monkeypatch.setattr(engine, "_dev", lambda t, name, dtype=None, device=None: t.contiguous())
    ids, n, m, dt = SHAPES[tag]
    F = systems.Team(ids, dt=dt)
    Bn, N = 2, 6
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    U = z(Bn, N, m)
    X = engine.rollout(F, z(n), U, F.dt)
    engine.dynamics(F, X[:, :N], U, F.dt)
    lin = engine.linearize(F, X, U, F.dt, central=True)
    cost = engine.CostParams(z(n), z(m), torch.eye(n, dtype=torch.float64),
                             torch.eye(m, dtype=torch.float64), torch.eye(n, dtype=torch.float64),
                             torch.full((1,), 0.5, dtype=torch.float64), None, F.wrap_idx)
    engine.cost_true(F, X, U, [N, N], cost)
    assert rec.calls == ["hop_team_rollout_f64", "hop_team_dynamics_f64",
                         "hop_team_linearize_f64", "hop_team_cost_true_f64"]
    # the cost arguments end in the wrap mask, as a fleet's do
    cargs, _ = engine._chain_cost_args(cost, Bn, n, m, X.device, F)
    assert len(cargs) == 10 and cargs[-1] == engine.wrap_mask(F.wrap_idx, n)
    rec.calls.clear()
    eye_n, eye_m = torch.eye(n, dtype=torch.float64), torch.eye(m, dtype=torch.float64)
    engine.propagate_traj(lin.A, lin.B, lin.a_res, X, U, z(n), z(m), eye_n, eye_m, eye_n,
                          torch.full((1,), 0.5, dtype=torch.float64), n_use=5, t_min=2, t_max=5)
    sel = [c for c in rec.calls if ("sweep" in c or "augment" in c) and "bytes" not in c]
    if wide:
        assert sel == ["hop_augment_wide_f64", "hop_lft_sweep_wide_f64"], sel
    else:
        assert sel == ["hop_lft_sweep_traj_f64"], sel
    rec.calls.clear()
    T = torch.full((Bn,), 4, dtype=torch.int32)
    engine.riccati(lin.A, lin.B, X, U, z(n), z(m), eye_n, eye_m, eye_n, T,
                   torch.full((Bn,), 1e-3, dtype=torch.float64), mode=0, reg_max_tries=1)
    assert [c for c in rec.calls if "riccati" in c] == [
        "hop_riccati_wide_f64" if n > _lib.MAX_DIM else "hop_riccati_f64"]
    rec.calls.clear()
    for name in ("forward_workspace_bytes", "forward_linesearch_f64"):
        fn, par = engine._object_entry(F, name)
        assert isinstance(par, _lib.TeamParams) and par.count == len(ids)
        assert list(par.system)[:len(ids)] == list(ids)
        fn()
    assert rec.calls == ["hop_team_forward_workspace_bytes", "hop_team_forward_linesearch_f64"]


# ---------------------------------------------------------------- the math
def _member_lin(dh, sid, dt, X, U, central, n_use=None):
    """dyn_host_linearize (the members' own arithmetic) on a member trajectory"""
    Bn, N = U.shape[:2]
    n, m = X.shape[-1], U.shape[-1]
    n_use = N if n_use is None else n_use
    A, B = np.full((Bn, N, n, n), -7.0), np.full((Bn, N, n, m), -7.0)
    ar, Fx = np.full((Bn, N, n), -7.0), np.full((Bn, N, n), -7.0)
    assert dh.dyn_host_linearize(sid, dt, _p(X), _p(U), Bn, N, n_use, int(central), 1e-5, 1e-5,
                                 1e-6, 1e-6, _p(A), _p(B), _p(ar), _p(Fx)) == 0
    return A, B, ar, Fx


def _team_lin(th, tag, X, U, central, n_use=None):
    ids, n, m, dt = SHAPES[tag]
    Bn, N = U.shape[:2]
    n_use = N if n_use is None else n_use
    A, B = np.full((Bn, N, n, n), -7.0), np.full((Bn, N, n, m), -7.0)
    ar, Fx = np.full((Bn, N, n), -7.0), np.full((Bn, N, n), -7.0)
    assert th.team_host_linearize(len(ids), _p(_ids(ids)), dt, _p(X), _p(U), Bn, N, n_use,
                                  int(central), 1e-5, 1e-5, 1e-6, 1e-6, _p(A), _p(B), _p(ar),
                                  _p(Fx)) == 0
    return A, B, ar, Fx


def block_mask(ids):
    """[n, n] and [n, m] masks of the members' diagonal blocks"""
    xo, uo = _offsets(ids)
    n, m = xo[-1] + SIZES[ids[-1]][0], uo[-1] + SIZES[ids[-1]][1]
    mA, mB = np.zeros((n, n), dtype=bool), np.zeros((n, m), dtype=bool)
    for s, i, j in zip(ids, xo, uo):
        mA[i:i + SIZES[s][0], i:i + SIZES[s][0]] = True
        mB[i:i + SIZES[s][0], j:j + SIZES[s][1]] = True
    return mA, mB


def test_team_host_shape_is_the_tables(hosts):
    th, _ = hosts
    n, m = C.c_int(), C.c_int()
    for tag, (ids, nn, mm, dt) in SHAPES.items():
        assert th.team_host_shape(len(ids), _p(_ids(ids)), C.byref(n), C.byref(m)) == 0
        assert (n.value, m.value) == (nn, mm), tag
    for ids, code in (((0,) * 16, 1), ((), 1), ((0, 5), 2), ((2, 2, 2), 3), ((3,) * 8, 3)):
        assert th.team_host_shape(len(ids), _p(_ids(ids + (0,))), C.byref(n), C.byref(m)) == code


@pytest.mark.parametrize("tag", list(SHAPES))
def test_team_math_F_is_the_members_F_bitwise(hosts, tag):
    th, dh = hosts
    ids, n, m, dt = SHAPES[tag]
    xo, uo = _offsets(ids)
    rng = np.random.default_rng(11 + n)
    X, U = rng.uniform(-1.0, 1.0, (23, n)), rng.uniform(-1.0, 1.0, (23, m))
    out = np.full_like(X, -7.0)
    assert th.team_host_dynamics(len(ids), _p(_ids(ids)), dt, _p(X), _p(U), len(X), _p(out)) == 0
    # the members' own F through dyn_host's Fx on one-step trajectories, at the team's dt
    for s, i, j in zip(ids, xo, uo):
        ns, ms = SIZES[s]
        Xm = np.ascontiguousarray(np.repeat(X[:, None, i:i + ns], 2, axis=1))
        Um = np.ascontiguousarray(U[:, None, j:j + ms])
        Fx = _member_lin(dh, s, dt, Xm, Um, False)[3]
        assert np.array_equal(out[:, i:i + ns], Fx[:, 0]), (tag, i)
    # and the NumPy twin of systems.Team agrees with it (libm: to a few ulp)
    from time_opt_ilqr_amd import systems
    tw = systems.Team(ids, dt=dt)(X, U)
    assert float(np.abs(tw - out).max()) <= 1e-14
    if not set(ids) & {1, 2}:  # no libm call: bitwise
        assert np.array_equal(tw, out)


@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_team_math_linearize_blocks_bitwise_and_zeros(hosts, tag, central):
    th, dh = hosts
    ids, n, m, dt = SHAPES[tag]
    xo, uo = _offsets(ids)
    rng = np.random.default_rng(3 * n + m)
    Bn, N = 3, 5
    X = rng.uniform(-1.0, 1.0, (Bn, N + 1, n))
    U = rng.uniform(-1.0, 1.0, (Bn, N, m))
    A, B, ar, Fx = _team_lin(th, tag, X, U, central)
    mA, mB = block_mask(ids)
    assert (A[..., ~mA] == 0.0).all() and (B[..., ~mB] == 0.0).all()
    assert not np.signbit(A[..., ~mA]).any() and not np.signbit(B[..., ~mB]).any()
    for s, i, j in zip(ids, xo, uo):
        ns, ms = SIZES[s]
        Xa, Ua = np.ascontiguousarray(X[..., i:i + ns]), np.ascontiguousarray(U[..., j:j + ms])
        Am, Bm, arm, Fxm = _member_lin(dh, s, dt, Xa, Ua, central)
        sl, su = slice(i, i + ns), slice(j, j + ms)
        assert np.array_equal(A[..., sl, sl], Am) and np.array_equal(B[..., sl, su], Bm), (tag, i)
        assert np.array_equal(ar[..., sl], arm) and np.array_equal(Fx[..., sl], Fxm), (tag, i)
    # the stacked callable through host_dynamics' loops (the reference's): the same numbers
    # up to libm and the order of BLAS sums in the twin -- test_fleet_cpu.py's bar
    from time_opt_ilqr_amd import host_dynamics, systems
    ref = host_dynamics.linearize_batch(systems.Team(ids, dt=dt).host(), X, U, central=central)
    errs = [float(np.abs(g - r).max()) for g, r in zip((A, B, ar), ref)]
    print(f"team lin host {tag} central={central}: max abs err vs the twin {errs}")
    assert max(errs) <= 1e-9
    assert (ref[0][..., ~mA] == 0.0).all() and (ref[1][..., ~mB] == 0.0).all()


@pytest.mark.parametrize("tag", list(SHAPES))
def test_team_math_nan_pattern_is_the_references(hosts, tag):
    """a NaN planted in the second member's state at one step: the NaN pattern of A and B
    equals the reference's (tests/golden/make_golden_team.py ran its linearisations on the
    stacked callable)"""
    th, _ = hosts
    ids, n, m, dt = SHAPES[tag]
    d = np.load(os.path.join(GOLDEN, f"team_cases_{tag}.npz"))
    from test_gpu_team import case_inputs
    c = case_inputs(int(d["seed"]), n, m, _offsets(ids)[0][1])
    assert np.isnan(c["Xn"][c["nan_at"]]) and int(np.isnan(c["Xn"]).sum()) == 1
    assert c["nan_at"][1] == _offsets(ids)[0][1] + 1
    for form, central in (("fwd", False), ("cen", True)):
        A, B, _, _ = _team_lin(th, tag, c["Xn"][None], c["Un"][None], central)
        assert np.array_equal(np.isnan(A[0]), d[f"nan_A_{form}"]), (tag, form)
        assert np.array_equal(np.isnan(B[0]), d[f"nan_B_{form}"]), (tag, form)
        k = c["nan_at"][0]
        assert d[f"nan_A_{form}"][k].any() and not d[f"nan_A_{form}"][k - 1].any()
        if not central:  # the forward form: the whole (A_k, B_k)
            assert d["nan_A_fwd"][k].all() and d["nan_B_fwd"][k].all()


def test_team_math_n_use_leaves_the_tail(hosts):
    th, _ = hosts
    tag = "pm_quad_di"
    ids, n, m, dt = SHAPES[tag]
    rng = np.random.default_rng(6)
    X = rng.uniform(-1.0, 1.0, (2, 8, n))
    U = rng.uniform(-1.0, 1.0, (2, 7, m))
    A, B, ar, Fx = _team_lin(th, tag, X, U, True, n_use=5)
    for t in (A, B, ar, Fx):
        assert (t[:, 5:] == -7.0).all() and (t[:, :5] != -7.0).any()
    A2, B2, ar2, _ = _team_lin(th, tag, X[:, :6].copy(), U[:, :5].copy(), True)
    assert np.array_equal(A[:, :5], A2) and np.array_equal(B[:, :5], B2)
    assert np.array_equal(ar[:, :5], ar2)


def test_team_host_program_under_sanitizers(tmp_path):
    """team_host.cpp as a stand-alone program (its own main) built with AddressSanitizer
    and UBSan: the step and both linearisation forms over all5 and pm7_di in buffers of
    exactly the documented sizes, the blocks' structure checked by the program"""
    exe = str(tmp_path / "team_host_san")
    subprocess.check_call(GXX + ["-O1", "-g", "-DTEAM_HOST_MAIN", "-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=undefined",
                                 os.path.join(CSRC, "team_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stderr == ""
    assert "all5: n = 26, m = 9, 5 members, 0 bad entries" in r.stdout
    assert "pm7_di: n = 30, m = 15, 8 members, 0 bad entries" in r.stdout
    assert r.stdout.strip().endswith("OK")


def test_team_case_inputs_are_one_text():
    """the generator and the GPU test build the kernel-level inputs from one function"""
    def body(path):
        src = open(path).read()
        return src.split("# BEGIN case_inputs")[1].split("# END case_inputs")[0].split("\n", 1)[1]
    a = body(os.path.join(GOLDEN, "make_golden_team.py"))
    b = body(os.path.join(REPO, "tests", "test_gpu_team.py"))
    assert a == b and "def case_inputs(" in a
    from test_gpu_team import case_inputs
    for tag, (ids, n, m, dt) in SHAPES.items():
        d = np.load(os.path.join(GOLDEN, f"team_cases_{tag}.npz"))
        c = case_inputs(int(d["seed"]), n, m, _offsets(ids)[0][1])
        got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum()])
        assert np.array_equal(got, d["check"]), tag
        assert (int(d["n"]), int(d["m"]), tuple(d["members"].tolist())) == (n, m, ids)
        assert float(d["dt"]) == dt
