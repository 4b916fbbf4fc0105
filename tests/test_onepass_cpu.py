"""CPU: the one-pass window method's primitives of include/hop_onepass.h.

* its five entries are exported and bound in a table of their own, stay out of the other
  headers, and the header is in the build digest;
* every entry validates its arguments on the host before any launch;
* the host build of csrc/onepass_pick.hpp (onepass_host.cpp: the pick kernel's
  per-problem arithmetic) against the reference's onepass_pick_T_singlepass on the cases
  of tests/golden/onepass_pick_cases.npz (make_golden_onepass.py): T exactly, Jw to 1e-12
  relative with the same NaN pattern;
* the inputs method="onepass" does not take raise before anything touches the GPU.

The 1e-12 bar: J_T sums n^2 + n + 1 <= 157 products of O(1)..O(100) terms that do not
cancel (Vxx is positive definite, V0 >= 5), so two summation orders differ by at most
~157 * 1.1e-16 relative.
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hop_onepass_extend_backward_f64", "hop_onepass_nominal_curve_f64",
         "hop_onepass_pick_f64", "hop_onepass_rollout_f64",
         "hop_onepass_rollout_workspace_bytes"]
_P = C.c_void_p
D = C.c_void_p(16)  # never dereferenced: every call here ends on the host


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def pick_host(tmp_path_factory):
    """g++ build of csrc/onepass_pick.hpp (the pick kernel's per-problem math)."""
    d = tmp_path_factory.mktemp("onepass")
    so = str(d / "libonepass_host.so")
    src = os.path.join(REPO, "time_opt_ilqr_amd", "csrc", "onepass_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC",
                           "-DHOP_HD=", src, "-o", so])
    h = C.CDLL(so)
    h.onepass_host_pick.argtypes = [_P] * 6 + [C.c_int64] + [C.c_int32] * 6 + \
        [C.c_uint32, C.c_double, _P, _P]
    return h


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


# ---------------------------------------------------------------- the ABI
def test_onepass_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_onepass.h") == NAMES
    assert sorted(_lib.ONEPASS_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    others = set()
    for h in ("hop.h", "hop_wide.h", "hop_wide_jcurve.h", "hop_chain.h"):
        others |= set(_functions(h))
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        assert name not in others
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES):
            assert name not in table
    assert len(_functions("hop.h")) == 40
    assert lib.hop_abi_version() == 1


def test_onepass_header_is_in_the_build_digest():
    from time_opt_ilqr_amd import build
    assert "hop_onepass.h" in inspect.getsource(build._digest)
    assert "onepass.hip" in build.SOURCES
    assert "onepass_pick.hpp" in build.HEADERS and "cost_device.hpp" in build.HEADERS


def _calls(lib, *, system=0, batch=4, null=False, N=10, T_min=2, T_max=8, S=3, n=2, n_ext=14,
           S_left=3, S_right=3, n_alpha=4, ws=1 << 40, wrap=0, n_obs=0, only=None):
    """every launching entry (or the one named) with the same bad or empty arguments:
    name -> rc.  Every call made here must end on the host."""
    q = None if null else D
    al = (C.c_double * 8)(*([1.0] * 8))
    cost = (q, 0, q, 0, q, 0, q, 0, q, 0, q, 0, q if n_obs else None, n_obs, wrap)
    fns = {
        "curve": lambda: lib.hop_onepass_nominal_curve_f64(system, q, q, *cost, T_min, T_max,
                                                           batch, N, q, q, None),
        "extend": lambda: lib.hop_onepass_extend_backward_f64(system, 0.05, q, q, q, batch, N, S,
                                                              4, 1e-9, 0.5, q, q, None),
        "pick": lambda: lib.hop_onepass_pick_f64(q, q, q, q, q, q, batch, n, n_ext, T_min, T_max,
                                                 S_left, S_right, wrap, 5.0, q, q, None),
        "rollout": lambda: lib.hop_onepass_rollout_f64(
            system, 0.05, q, q, *cost, q, q, q, q, q, al, n_alpha, batch, N, S, q, ws, q, q, q, q,
            None),
    }
    return {k: f() for k, f in fns.items() if only in (None, k)}


def test_onepass_validation_without_gpu(lib):
    err = lib.hop_last_error
    one = lambda name, **kw: _calls(lib, only=name, **kw)[name]  # noqa: E731
    for name in ("curve", "extend", "rollout"):
        for system in (-1, 5):
            assert one(name, system=system) == -1 and b"unknown system" in err(), name
    assert all(rc == -1 for rc in _calls(lib, null=True).values())
    assert b"null" in err()
    assert all(rc == -1 for rc in _calls(lib, batch=-1).values())
    assert all(rc == -2 for rc in _calls(lib, batch=1 << 40).values())
    # an empty batch launches nothing, with or without pointers
    assert all(rc == 0 for rc in _calls(lib, batch=0).values())
    assert all(rc == 0 for rc in _calls(lib, batch=0, null=True).values())
    # horizons and windows
    for kw in (dict(T_min=0), dict(T_min=9, T_max=8), dict(T_max=11)):
        assert one("curve", **kw) == -1 and b"T_min <= T_max <= N" in err()
    for kw in (dict(T_min=0), dict(T_min=9, T_max=8)):
        assert one("pick", **kw) == -1 and b"T_min <= T_max" in err()
    assert one("extend", S=0) == -1 and b"S >= 1" in err()
    assert one("extend", S=65) == -2 and b"HOP_ONEPASS_MAX_WINDOW" in err()
    assert one("rollout", S=65) == -2 and one("rollout", S=-1) == -1
    assert one("pick", S_left=-1) == -1 and one("pick", S_right=-1) == -1
    assert one("pick", S_left=65) == -2 and one("pick", S_right=65) == -2
    assert one("pick", S_left=64, S_right=64) != -2
    for n in (0, 3, 13, 16):
        assert one("pick", n=n) == -2 and b"(2, 4, 12)" in err()
    assert one("pick", n_ext=0) == -1
    assert one("pick", wrap=4) == -1 and b"wrap index" in err()  # bit 2 of a 2-state system
    assert one("curve", wrap=4) == -1 and one("rollout", wrap=4) == -1
    assert one("curve", n_obs=65) == -1 and one("rollout", n_obs=-1) == -1
    for na in (0, 9):
        assert one("rollout", n_alpha=na) == -1 and b"n_alpha" in err()
    need = lib.hop_onepass_rollout_workspace_bytes(2, 4, 10, 4)
    assert need == 4 * 4 * (1 + 11 * 12 + 10 * 4) * 8
    assert one("rollout", system=2, ws=need - 1) == -1 and b"workspace too small" in err()
    assert lib.hop_onepass_rollout_workspace_bytes(7, 4, 10, 4) == 0
    assert lib.hop_onepass_rollout_workspace_bytes(2, -1, 10, 4) == 0


def test_onepass_scope_errors_without_gpu():
    """what method="onepass" does not take raises what the scope says, before any GPU use"""
    from time_opt_ilqr_amd import host_dynamics, solver, systems
    mk = systems.make_double_integrator(N=50)
    F, x0, xg, u_ref, Q, R, alpha, w = mk[:8]
    args = (x0, xg, u_ref, Q, R, alpha, w, 50, 10, 50)
    call = lambda G, **kw: solver.ilqr_timeopt(G, *args, method="onepass", **kw)  # noqa: E731
    py_F = lambda x, u: np.array([x[0] + 0.05 * x[1], x[1] + 0.05 * u[0]])  # noqa: E731
    with pytest.raises(NotImplementedError):
        call(py_F)
    with pytest.raises(NotImplementedError):
        call(host_dynamics.HostDynamics(py_F, 2, 1))
    with pytest.raises(NotImplementedError):
        call(F, extra_stage_cost=lambda x, u: (0.0, np.zeros(2), np.zeros((2, 2))))
    with pytest.raises(NotImplementedError):
        call(systems.SpringChain(12, 3))
    for pre in ("newton", "copy"):
        with pytest.raises(NotImplementedError):
            call(F, onepass_preimage=pre)
    with pytest.raises(ValueError):
        call(F, S_window=0)
    with pytest.raises(ValueError):
        call(F, S_window=65)
    Qf = np.eye(2) * alpha
    batch = lambda s, **kw: solver.ilqr_timeopt_batch(  # noqa: E731
        s, x0[None], xg, u_ref, Q, np.atleast_2d(R), Qf, w, 50, 10, 50, method="onepass", **kw)
    with pytest.raises(NotImplementedError):
        batch(host_dynamics.HostDynamics(py_F, 2, 1))
    with pytest.raises(NotImplementedError):
        batch(systems.SpringChain(12, 3))
    with pytest.raises(NotImplementedError):
        batch(0, dt=0.05, onepass_preimage="newton")
    with pytest.raises(ValueError):
        batch(0, dt=0.05, S_window=0)
    assert callable(solver.ilqr_timeopt_baseline2) and callable(solver.nominal_cost_curve)
    assert callable(solver.onepass_rollout)


# ---------------------------------------------------------------- the pick arithmetic
def _pick_cases():
    d = np.load(os.path.join(REPO, "tests", "golden", "onepass_pick_cases.npz"))
    return d, [str(s) for s in d["names"]]


def check_pick(name, T, Jw, T_ref, Jw_ref):
    """the issue's bars: T exactly, Jw to 1e-12 relative with the same NaN pattern"""
    assert T == T_ref, (name, T, T_ref)
    assert np.array_equal(np.isnan(Jw), np.isnan(Jw_ref)), name
    ok = ~np.isnan(Jw_ref)
    err = float(np.max(np.abs(Jw[ok] - Jw_ref[ok]) / np.abs(Jw_ref[ok]))) if ok.any() else 0.0
    print(f"pick {name}: T*={T} evaluated={int(ok.sum())} max rel err {err:.2e}")
    assert err <= 1e-12, (name, err)


def test_pick_host_build_matches_the_reference(pick_host):
    d, names = _pick_cases()
    assert len(names) == 31
    for i, name in enumerate(names):
        n, L, T_bar, T_min, T_max, S_left, S_right = (int(v) for v in d[f"c{i}_par"])
        mask = sum(1 << int(j) for j in d[f"c{i}_wrap"])
        arr = [np.ascontiguousarray(d[f"c{i}_{k}"]) for k in ("Vxx", "Vx", "V0", "X_ext", "x0")]
        Tb = np.array([T_bar], dtype=np.int32)
        T = np.full(1, -7, dtype=np.int32)
        Jw = np.full(T_max, -7.0)
        p = lambda a: a.ctypes.data_as(_P)  # noqa: E731
        rc = pick_host.onepass_host_pick(*[p(a) for a in arr], p(Tb), 1, n, L, T_min, T_max,
                                         S_left, S_right, mask, 5.0, p(T), p(Jw))
        assert rc == 0
        check_pick(name, int(T[0]), Jw, int(d[f"c{i}_T"]), d[f"c{i}_Jw"])


def test_pick_host_build_batches_and_refuses_bad_shapes(pick_host):
    """two problems with different T_bar in one call give each its own row; sizes the
    kernel has no instantiation for are refused"""
    d, names = _pick_cases()
    i, j = names.index("n2_plain"), names.index("n2_gate")
    par = [int(v) for v in d[f"c{i}_par"]]
    assert par == [int(v) for v in d[f"c{j}_par"]]
    n, L, T_bar, T_min, T_max, S_left, S_right = par
    arr = [np.ascontiguousarray(np.stack([d[f"c{i}_{k}"], d[f"c{j}_{k}"]]))
           for k in ("Vxx", "Vx", "V0", "X_ext", "x0")]
    Tb = np.array([T_bar, T_bar], dtype=np.int32)
    T = np.zeros(2, dtype=np.int32)
    Jw = np.zeros((2, T_max))
    p = lambda a: a.ctypes.data_as(_P)  # noqa: E731
    assert pick_host.onepass_host_pick(*[p(a) for a in arr], p(Tb), 2, n, L, T_min, T_max, S_left,
                                       S_right, 0, 5.0, p(T), p(Jw)) == 0
    for r, c in enumerate((i, j)):
        check_pick(names[c], int(T[r]), Jw[r], int(d[f"c{c}_T"]), d[f"c{c}_Jw"])
    assert pick_host.onepass_host_pick(*[p(a) for a in arr], p(Tb), 2, 3, L, T_min, T_max, S_left,
                                       S_right, 0, 5.0, p(T), p(Jw)) == -2
    assert pick_host.onepass_host_pick(*[p(a) for a in arr], p(Tb), 2, n, L, 0, T_max, S_left,
                                       S_right, 0, 5.0, p(T), p(Jw)) == -1
