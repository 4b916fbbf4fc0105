"""CPU: fleets of the built-in systems as device systems (include/hop_fleet.h).

* the six entries are exported and bound in a table of their own, stay out of the other
  headers, and the header and sources are in the build lists;
* every entry validates its arguments on the host before any launch;
* the host build of csrc/fleet_math.hpp (fleet_host.cpp: fleet.hip's per-member
  arithmetic) against the members' host dynamics (dyn_host.cpp), bitwise, with every
  off-block entry an exact 0.0, and its NaN pattern against the reference's fixtures;
* systems.Fleet / make_fleet, the scope refusals and the routing by shape.
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
NAMES = ["hop_fleet_cost_true_f64", "hop_fleet_dynamics_f64",
         "hop_fleet_forward_linesearch_f64", "hop_fleet_forward_workspace_bytes",
         "hop_fleet_linearize_f64", "hop_fleet_rollout_f64"]
# base system id, count, n, m (the issue's table)
SHAPES = {"di1": (0, 1, 2, 1), "di7": (0, 7, 14, 7), "di8": (0, 8, 16, 8),
          "di15": (0, 15, 30, 15), "pm7": (3, 7, 28, 14), "cp5": (1, 5, 20, 5),
          "seg6": (4, 6, 24, 6), "quad2": (2, 2, 24, 8)}
MEMBER_DT = {0: 0.05, 1: 0.02, 2: 0.05, 3: 0.05, 4: 0.02}
_P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _gxx(tmp, name, extra=()):
    so = str(tmp / f"lib{name}.so")
    src = os.path.join(REPO, "time_opt_ilqr_amd", "csrc", name + ".cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin-sin",
                           "-fno-builtin-cos", "-fno-builtin-tan", "-shared", "-fPIC", "-DHOP_HD=",
                           *extra, src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """g++ builds of csrc/fleet_math.hpp (fleet_host.cpp) and of the members' own
    dynamics.hpp (dyn_host.cpp)"""
    d = tmp_path_factory.mktemp("fleet")
    fh, dh = _gxx(d, "fleet_host"), _gxx(d, "dyn_host")
    lin = [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int] + [C.c_double] * 4 + [_P] * 4
    fh.fleet_host_dynamics.argtypes = [C.c_int, C.c_int, C.c_double, _P, _P, C.c_int64, _P]
    fh.fleet_host_linearize.argtypes = [C.c_int, C.c_int, C.c_double] + lin
    dh.dyn_host_linearize.argtypes = [C.c_int, C.c_double] + lin
    return fh, dh


def _p(a):
    return a.ctypes.data_as(_P)


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


# ---------------------------------------------------------------- the ABI
def test_fleet_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_fleet.h") == NAMES
    assert sorted(_lib.FLEET_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    others = set()
    for h in ("hop.h", "hop_wide.h", "hop_wide_jcurve.h", "hop_chain.h", "hop_onepass.h"):
        others |= set(_functions(h))
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        assert name not in others
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES, _lib.ONEPASS_SIGNATURES):
            assert name not in table
    assert len(_functions("hop.h")) == 40 and lib.hop_abi_version() == 1
    text = open(os.path.join(REPO, "include", "hop_fleet.h")).read()
    assert f"#define HOP_FLEET_MAX_N {_lib.FLEET_MAX_N} " in text
    assert f"#define HOP_FLEET_MAX_M {_lib.FLEET_MAX_M} " in text


def test_fleet_sources_are_in_the_build_lists():
    from time_opt_ilqr_amd import build
    assert "hop_fleet.h" in inspect.getsource(build._digest)
    assert "fleet.hip" in build.SOURCES and "fleet_math.hpp" in build.HEADERS


# ---------------------------------------------------------------- validation
def _params(system=2, count=2, dt=0.05):
    from time_opt_ilqr_amd import _lib
    return _lib.FleetParams(system, count, dt)


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
        "dynamics": lambda: lib.hop_fleet_dynamics_f64(pp, q, stride, q, stride, batch, q, stride,
                                                       None),
        "rollout": lambda: lib.hop_fleet_rollout_f64(pp, q, 0, q, batch, n_alloc, 1e6, q, None),
        "linearize": lambda: lib.hop_fleet_linearize_f64(pp, q, q, batch, n_alloc, n_use, 1, 1e-5,
                                                         1e-5, 1e-6, 1e-6, q, q, q, q, None),
        "cost": lambda: lib.hop_fleet_cost_true_f64(pp, q, q, q, *cost, batch, n_alloc, q, None),
        "linesearch": lambda: lib.hop_fleet_forward_linesearch_f64(
            pp, q, q, *cost, q, q, q, q, al, n_alpha, batch, n_alloc, q, ws, q, q, q, q, q, None),
    }
    return {k: f() for k, f in fns.items() if only in (None, k)}


def test_fleet_validation_without_gpu(lib):
    err = lib.hop_last_error
    # HOP_E_SIZE: count < 1, n > 31 or m > 16 -- the last fleet that fits and the first
    # that does not, for every member system
    for system, last in ((0, 15), (1, 7), (2, 2), (3, 7), (4, 7)):
        ok = _params(system, last)
        assert lib.hop_fleet_forward_workspace_bytes(C.byref(ok), 4, 10, 5) > 0
        assert all(rc == 0 for rc in _calls(lib, ok, batch=0).values()), (system, last)
        for count in (last + 1, 0, -3):
            par = _params(system, count)
            for name, rc in _calls(lib, par).items():
                assert rc == -2, (system, count, name)
            assert b"count must be >= 1" in err() or b"n must be <= 31 and m <= 16" in err()
            assert lib.hop_fleet_forward_workspace_bytes(C.byref(par), 4, 10, 5) == 0
            # the shape is checked for an empty batch too
            assert all(rc == -2 for rc in _calls(lib, par, batch=0).values())
    for system in (-1, 5):
        assert all(rc == -1 for rc in _calls(lib, _params(system, 1)).values())
        assert b"unknown system" in err()
        assert lib.hop_fleet_forward_workspace_bytes(C.byref(_params(system, 1)), 4, 10, 5) == 0
    for dt in (0.0, -0.1, float("nan")):
        assert all(rc == -1 for rc in _calls(lib, _params(dt=dt)).values())
        assert b"dt must be positive" in err()
    par = _params()  # quadrotor x 2: n = 24, m = 8
    assert all(rc == -1 for rc in _calls(lib, par, null=True).values())
    assert b"null" in err()
    assert all(rc == -1 for rc in _calls(lib, None).values())
    one = lambda name, **kw: _calls(lib, par, only=name, **kw)[name]  # noqa: E731
    assert one("linearize", n_use=11) == -1 and b"n_use > n_alloc" in err()
    for na in (0, 9):
        assert one("linesearch", n_alpha=na) == -1 and b"n_alpha" in err()
    need = lib.hop_fleet_forward_workspace_bytes(C.byref(par), 4, 10, 5)
    assert need == 4 * 5 * (1 + 11 * 24 + 10 * 8) * 8
    assert one("linesearch", ws=need - 1) == -1 and b"workspace too small" in err()
    assert one("dynamics", stride=23) == -1 and b"stride" in err()
    # wrap bits at or above n = 24
    for name in ("cost", "linesearch"):
        assert one(name, wrap=1 << 24) == -1 and b"wrap bits" in err(), name
        assert one(name, wrap=1 << 31) == -1
        assert one(name, wrap=(7 << 6) | (7 << 18), batch=0) == 0
    # negative sizes
    assert all(rc == -1 for rc in _calls(lib, par, batch=-1).values())
    assert one("rollout", n_alloc=-1) == -1 and one("cost", n_alloc=-1) == -1
    assert one("linesearch", n_alloc=-1) == -1 and one("linearize", n_alloc=-1, n_use=-1) == -1
    assert lib.hop_fleet_rollout_f64(C.byref(par), D, -1, D, 4, 10, 1e6, D, None) == -1
    # too many rows for one launch
    assert all(rc == -2 for rc in _calls(lib, par, batch=1 << 40).values())
    # an empty batch launches nothing, with or without pointers; so does n_use = 0
    assert all(rc == 0 for rc in _calls(lib, par, batch=0).values())
    assert all(rc == 0 for rc in _calls(lib, par, batch=0, null=True).values())
    assert one("linearize", n_use=0) == 0


# ---------------------------------------------------------------- the object
def test_fleet_object_and_refusals_without_gpu():
    from time_opt_ilqr_amd import engine, host_dynamics, linearization, solver, systems
    F = systems.Fleet("quadrotor", 2)
    assert (F.n, F.m, F.dt, F.count, F.base_id) == (24, 8, 0.05, 2, 2)
    assert F.fleet_params() == (2, 2, 0.05) and F.wrap_idx == [6, 7, 8, 18, 19, 20]
    assert engine.is_fleet(F) and not engine.is_chain(F) and engine.system_dims(F) == (24, 8)
    assert engine.wrap_mask(F.wrap_idx, F.n) == (7 << 6) | (7 << 18)
    assert not engine.is_fleet(2) and not engine.is_fleet("quadrotor")
    assert not engine.is_fleet(systems.SpringChain(4, 2))
    assert solver._on_device(F) and solver._sys(F) is F and linearization._sys(F) is F
    assert systems.Fleet(systems.make_segway_balance()[0], 6, dt=0.01).dt == 0.01
    assert systems.Fleet(4, 6).dt == 0.02 and systems.Fleet(0, 15).n == 30
    # the sizes out of range
    for base, count in ((0, 16), ("cartpole", 8), ("segway", 8), ("pointmass", 8),
                        ("quadrotor", 3), (0, 0), (2, -1)):
        with pytest.raises(ValueError):
            systems.Fleet(base, count)
    for base in (5, "unicycle"):
        with pytest.raises(ValueError):
            systems.Fleet(base, 2)
    with pytest.raises(ValueError):
        systems.Fleet(0, 2, dt=0.0)
    # callable: the NumPy twin, which HostDynamics wraps
    H = F.host()
    assert isinstance(H, host_dynamics.HostDynamics) and (H.n, H.m) == (24, 8) and H.vectorized
    mk = systems.make_fleet("quadrotor", 2, N=80, seed=1)
    assert len(mk) == 13 and isinstance(mk[0], systems.Fleet) and mk[12] is None
    F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max, wrap = mk[:12]
    assert (N, T_min, T_max, wrap) == (80, 40, 75, [6, 7, 8, 18, 19, 20])
    assert Q[0, 12] == -2.5 and Q[0, 0] == 7.5 and Q[12, 12] == 7.5 and Q[1, 13] == 0.0
    assert Qf.shape == (24, 24) and R.shape == (8, 8) and np.array_equal(ur[:4], ur[4:])
    # onepass, a Python stage cost and the obstacle table are out of scope
    stage = lambda x, u: (0.0, np.zeros(24), np.zeros((24, 24)))  # noqa: E731
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
        lambda: linearization.extend_nominal_backward(F, np.zeros((3, 24)), np.zeros((2, 8)),
                                                      ur, S_back=4),
    ):
        with pytest.raises(NotImplementedError):
            call()
    from time_opt_ilqr_amd import onepass
    with pytest.raises(NotImplementedError, match="fleet"):
        onepass.check_scope(F, 20, "fixedpoint")


@pytest.mark.parametrize("tag", ["di8", "di15", "seg6", "pm7", "quad2"])
def test_make_fleet_rebuilds_the_fixture_problems(tag):
    """systems.make_fleet and tests/golden/make_golden_fleet.py's problem() are one recipe"""
    from time_opt_ilqr_amd import systems
    sid, count, n, m = SHAPES[tag]
    for trial in range(3):
        d = np.load(os.path.join(GOLDEN, f"fleet_solve_{tag}_{trial}.npz"))
        mk = systems.make_fleet(sid, count, N=int(d["N"]), seed=int(d["seed"]),
                                w_scale=float(d["scale"]), T_min=int(d["T_min"]))
        for got, key in zip(mk[1:7], ("x0", "xg", "u_ref", "Q", "R", "Qf")):
            assert np.array_equal(got, d[key]), (tag, trial, key)
        assert mk[7] == float(d["w"]) and mk[8:11] == (int(d["N"]), int(d["T_min"]), int(d["T_max"]))
        assert mk[11] == d["wrap_idx"].tolist() == mk[0].wrap_idx
        for method in ("propagator", "bruteforce"):
            assert float(d[f"gaps_{method}"].min()) >= 1e-3 and len(d[f"T_hist_{method}"]) >= 2


def test_sharded_solver_passes_the_object_through(monkeypatch):
    from time_opt_ilqr_amd import distributed, systems
    import torch
    from time_opt_ilqr_amd import solver
    F = systems.Fleet(0, 8)
    seen = {}

    def fake(system, x0, *a, **k):
        seen["system"], seen["kw"] = system, k
        B = len(x0)
        return dict(n_hist=torch.ones(B, dtype=torch.int32), J_hist=torch.ones(B, 2),
                    T_star=torch.full((B,), 16, dtype=torch.int32),
                    crashed=torch.zeros(B, dtype=torch.int32))

    monkeypatch.setattr(solver, "ilqr_timeopt_batch", fake)
    mk = systems.make_fleet(0, 8, N=60)
    full, local, (lo, hi) = distributed.ilqr_timeopt_sharded(
        F, np.stack([mk[1]] * 3), *mk[2:7], mk[7], 60, 10, 55, device=torch.device("cpu"),
        wrap_idx=mk[11], method="bruteforce")
    assert seen["system"] is F and (lo, hi) == (0, 3)
    assert seen["kw"]["wrap_idx"] == [] and seen["kw"]["method"] == "bruteforce"
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


@pytest.mark.parametrize("count,wide", [(1, False), (7, False), (8, True), (15, True)])
def test_fleet_routing_by_shape(monkeypatch, count, wide):
    """DI x count: the fleet's own entries step it, and the select and Riccati kernels are
    chosen by shape alone -- n <= 15 the narrow select, n >= 16 the wide one (s = n + 1 > 16);
    the Riccati pass is wide from n = 17, as for every other system"""
    import torch
    from time_opt_ilqr_amd import _lib, engine, systems
    rec = _Recorder()
    monkeypatch.setattr(_lib, "load", lambda path=None: rec)
    monkeypatch.setattr(_lib, "stream_handle", lambda device=None: None)
    monkeypatch.setattr(engine, "_dev", lambda t, name, dtype=None, device=None: t.contiguous())
    F = systems.Fleet(0, count)
    n, m, Bn, N = F.n, F.m, 2, 6
    z = lambda *s: torch.zeros(s, dtype=torch.float64)  # noqa: E731
    U = z(Bn, N, m)
    X = engine.rollout(F, z(n), U, F.dt)
    engine.dynamics(F, X[:, :N], U, F.dt)
    lin = engine.linearize(F, X, U, F.dt, central=True)
    cost = engine.CostParams(z(n), z(m), torch.eye(n, dtype=torch.float64),
                             torch.eye(m, dtype=torch.float64), torch.eye(n, dtype=torch.float64),
                             torch.full((1,), 0.5, dtype=torch.float64), None, F.wrap_idx)
    engine.cost_true(F, X, U, [N, N], cost)
    assert rec.calls == ["hop_fleet_rollout_f64", "hop_fleet_dynamics_f64",
                         "hop_fleet_linearize_f64", "hop_fleet_cost_true_f64"]
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
    ric = engine.riccati(lin.A, lin.B, X, U, z(n), z(m), eye_n, eye_m, eye_n, T,
                         torch.full((Bn,), 1e-3, dtype=torch.float64), mode=0, reg_max_tries=1)
    assert [c for c in rec.calls if "riccati" in c] == [
        "hop_riccati_wide_f64" if n > _lib.MAX_DIM else "hop_riccati_f64"]  # n = 16: narrow
    rec.calls.clear()
    # the line search (it records its workspace on the GPU's stream, so only its lookup
    # runs here; tests/test_gpu_fleet.py runs it)
    for name in ("forward_workspace_bytes", "forward_linesearch_f64"):
        fn, par = engine._object_entry(F, name)
        assert isinstance(par, _lib.FleetParams) and (par.system, par.count) == (0, count)
        fn()
    assert rec.calls == ["hop_fleet_forward_workspace_bytes", "hop_fleet_forward_linesearch_f64"]


# ---------------------------------------------------------------- the math
def _rows(tag, rows, seed):
    sid, count, n, m = SHAPES[tag]
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (rows, n)), rng.uniform(-1.0, 1.0, (rows, m))


def _member_lin(dh, sid, X, U, central, n_use=None):
    """dyn_host_linearize (the members' own arithmetic) on a member trajectory"""
    Bn, N = U.shape[:2]
    n, m = X.shape[-1], U.shape[-1]
    n_use = N if n_use is None else n_use
    A, B = np.full((Bn, N, n, n), -7.0), np.full((Bn, N, n, m), -7.0)
    ar, Fx = np.full((Bn, N, n), -7.0), np.full((Bn, N, n), -7.0)
    assert dh.dyn_host_linearize(sid, MEMBER_DT[sid], _p(X), _p(U), Bn, N, n_use, int(central),
                                 1e-5, 1e-5, 1e-6, 1e-6, _p(A), _p(B), _p(ar), _p(Fx)) == 0
    return A, B, ar, Fx


def _fleet_lin(fh, tag, X, U, central, n_use=None):
    sid, count, n, m = SHAPES[tag]
    Bn, N = U.shape[:2]
    n_use = N if n_use is None else n_use
    A, B = np.full((Bn, N, n, n), -7.0), np.full((Bn, N, n, m), -7.0)
    ar, Fx = np.full((Bn, N, n), -7.0), np.full((Bn, N, n), -7.0)
    assert fh.fleet_host_linearize(sid, count, MEMBER_DT[sid], _p(X), _p(U), Bn, N, n_use,
                                   int(central), 1e-5, 1e-5, 1e-6, 1e-6, _p(A), _p(B), _p(ar),
                                   _p(Fx)) == 0
    return A, B, ar, Fx


def block_mask(count, ns, ms):
    """[n, n] and [n, m] masks of the diagonal blocks"""
    return (np.kron(np.eye(count), np.ones((ns, ns))) > 0,
            np.kron(np.eye(count), np.ones((ns, ms))) > 0)


@pytest.mark.parametrize("tag", list(SHAPES))
def test_kernel_math_F_is_the_members_F_bitwise(hosts, tag):
    fh, dh = hosts
    sid, count, n, m = SHAPES[tag]
    ns, ms = n // count, m // count
    X, U = _rows(tag, 23, 11 + n)
    out = np.full_like(X, -7.0)
    assert fh.fleet_host_dynamics(sid, count, MEMBER_DT[sid], _p(X), _p(U), len(X), _p(out)) == 0
    # the members' own F through dyn_host's Fx on one-step trajectories
    Xm = np.ascontiguousarray(np.repeat(X.reshape(-1, 1, ns), 2, axis=1))
    Um = np.ascontiguousarray(U.reshape(-1, 1, ms))
    Fx = _member_lin(dh, sid, Xm, Um, False)[3]
    assert np.array_equal(out, Fx.reshape(len(X), n))
    # and the NumPy twin of systems.Fleet agrees with it (libm: to a few ulp)
    from time_opt_ilqr_amd import systems
    tw = systems.Fleet(sid, count)(X, U)
    assert float(np.abs(tw - out).max()) <= 1e-14
    if sid in (0, 3, 4):  # no libm call: bitwise
        assert np.array_equal(tw, out)


@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("tag", list(SHAPES))
def test_kernel_math_linearize_blocks_bitwise_and_zeros(hosts, tag, central):
    fh, dh = hosts
    sid, count, n, m = SHAPES[tag]
    ns, ms = n // count, m // count
    rng = np.random.default_rng(3 * n + m)
    Bn, N = 3, 5
    X = rng.uniform(-1.0, 1.0, (Bn, N + 1, n))
    U = rng.uniform(-1.0, 1.0, (Bn, N, m))
    A, B, ar, Fx = _fleet_lin(fh, tag, X, U, central)
    mA, mB = block_mask(count, ns, ms)
    assert (A[..., ~mA] == 0.0).all() and (B[..., ~mB] == 0.0).all()
    assert not np.signbit(A[..., ~mA]).any() and not np.signbit(B[..., ~mB]).any()
    for a in range(count):
        Xa = np.ascontiguousarray(X[..., a * ns:(a + 1) * ns])
        Ua = np.ascontiguousarray(U[..., a * ms:(a + 1) * ms])
        Am, Bm, arm, Fxm = _member_lin(dh, sid, Xa, Ua, central)
        sl, su = slice(a * ns, (a + 1) * ns), slice(a * ms, (a + 1) * ms)
        assert np.array_equal(A[..., sl, sl], Am) and np.array_equal(B[..., sl, su], Bm), (tag, a)
        assert np.array_equal(ar[..., sl], arm) and np.array_equal(Fx[..., sl], Fxm), (tag, a)
    # the stacked callable through host_dynamics' loops (the reference's): the same numbers
    # up to libm and the order of BLAS sums in the twin
    from time_opt_ilqr_amd import host_dynamics, systems
    ref = host_dynamics.linearize_batch(systems.Fleet(sid, count).host(), X, U, central=central)
    errs = [float(np.abs(g - r).max()) for g, r in zip((A, B, ar), ref)]
    print(f"fleet lin host {tag} central={central}: max abs err vs the twin {errs}")
    assert max(errs) <= 1e-9
    assert (ref[0][..., ~mA] == 0.0).all() and (ref[1][..., ~mB] == 0.0).all()


@pytest.mark.parametrize("tag", list(SHAPES))
def test_kernel_math_nan_pattern_is_the_references(hosts, tag):
    """a NaN planted in one member's state at one step: the NaN pattern of A and B equals
    the reference's (tests/golden/make_golden_fleet.py ran its linearisations on the
    stacked callable)"""
    fh, _ = hosts
    sid, count, n, m = SHAPES[tag]
    d = np.load(os.path.join(GOLDEN, f"fleet_cases_{tag}.npz"))
    from test_gpu_fleet import case_inputs
    c = case_inputs(int(d["seed"]), n, m, n // count)
    assert np.isnan(c["Xn"][c["nan_at"]]) and int(np.isnan(c["Xn"]).sum()) == 1
    for form, central in (("fwd", False), ("cen", True)):
        A, B, _, _ = _fleet_lin(fh, tag, c["Xn"][None], c["Un"][None], central)
        assert np.array_equal(np.isnan(A[0]), d[f"nan_A_{form}"]), (tag, form)
        assert np.array_equal(np.isnan(B[0]), d[f"nan_B_{form}"]), (tag, form)
        k = c["nan_at"][0]
        assert d[f"nan_A_{form}"][k].any() and not d[f"nan_A_{form}"][k - 1].any()
        if not central:  # the forward form: the whole (A_k, B_k)
            assert d["nan_A_fwd"][k].all() and d["nan_B_fwd"][k].all()


def test_kernel_math_n_use_leaves_the_tail(hosts):
    fh, _ = hosts
    tag = "quad2"
    sid, count, n, m = SHAPES[tag]
    rng = np.random.default_rng(6)
    X = rng.uniform(-1.0, 1.0, (2, 8, n))
    U = rng.uniform(-1.0, 1.0, (2, 7, m))
    A, B, ar, Fx = _fleet_lin(fh, tag, X, U, True, n_use=5)
    for t in (A, B, ar, Fx):
        assert (t[:, 5:] == -7.0).all() and (t[:, :5] != -7.0).any()
    A2, B2, ar2, _ = _fleet_lin(fh, tag, X[:, :6].copy(), U[:, :5].copy(), True)
    assert np.array_equal(A[:, :5], A2) and np.array_equal(B[:, :5], B2)
    assert np.array_equal(ar[:, :5], ar2)


def test_case_inputs_are_one_text():
    """the generator and the GPU test build the kernel-level inputs from one function"""
    def body(path):
        src = open(path).read()
        return src.split("# BEGIN case_inputs")[1].split("# END case_inputs")[0].split("\n", 1)[1]
    a = body(os.path.join(GOLDEN, "make_golden_fleet.py"))
    b = body(os.path.join(REPO, "tests", "test_gpu_fleet.py"))
    assert a == b and "def case_inputs(" in a
    from test_gpu_fleet import case_inputs
    for tag, (sid, count, n, m) in SHAPES.items():
        d = np.load(os.path.join(GOLDEN, f"fleet_cases_{tag}.npz"))
        c = case_inputs(int(d["seed"]), n, m, n // count)
        got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum()])
        assert np.array_equal(got, d["check"]), tag
        assert (int(d["n"]), int(d["m"]), int(d["count"])) == (n, m, count)
