"""CPU: the spring-chain device system of include/hop_chain.h.

* its six entries are exported and bound in a table of their own, stay out of hop.h,
  hop_wide.h and hop_wide_jcurve.h, and the header is in the build digest;
* every entry validates its arguments on the host before any launch;
* the host build of csrc/chain_dynamics.hpp (chain_host.cpp: the kernels' per-step
  arithmetic, springs first, then every entry of [A | B] from them) against the NumPy
  chain of tests/golden/make_golden_wide.py and host_dynamics.linearize.

Where the bars come from (inputs in [-1, 1]): a sin that is 2 ulp off moves a spring
force f by <= 1.1e-16 plus one rounding of f (|f| <= 4.5), acc by <= ~6e-15 and v' by dt
times that plus one rounding: F to 4e-15 absolute, its q' half bitwise (no sin reaches
it).  A central quotient divides two such errors by 2 h = 2e-5, a forward one by 1e-5:
A, B and a_res to 1e-9 absolute; the entries a column cannot reach are exact zeros and
the q' rows of A and B are bitwise host_dynamics' (the same IEEE operations).
"""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["hop_chain_cost_true_f64", "hop_chain_dynamics_f64",
         "hop_chain_forward_linesearch_f64", "hop_chain_forward_workspace_bytes",
         "hop_chain_linearize_f64", "hop_chain_rollout_f64"]
F_TOL, LIN_TOL = 4e-15, 1e-9
SHAPES = [(1, 1), (2, 2), (8, 3), (15, 4)]
_P = C.c_void_p


def chain_F(p, m, dt=0.1, k=2.0, ks=0.5, c=0.3):
    """the mass-spring chain of tests/golden/make_golden_wide.py (same expressions), on
    one state or on stacked rows"""
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

    return F


def chain_F_reference(p, m, dt=0.1):
    """make_golden_wide.py's chain_dynamics verbatim (one state per call)"""
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


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def chain_host(tmp_path_factory):
    """g++ build of csrc/chain_dynamics.hpp (the chain kernels' per-step math)."""
    d = tmp_path_factory.mktemp("chain")
    so = str(d / "libchain_host.so")
    src = os.path.join(REPO, "time_opt_ilqr_amd", "csrc", "chain_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-builtin-sin",
                           "-shared", "-fPIC", "-DHOP_HD=", src, "-o", so])
    h = C.CDLL(so)
    par = [C.c_int, C.c_int] + [C.c_double] * 4
    h.chain_host_dynamics.argtypes = par + [_P, _P, C.c_int64, _P]
    h.chain_host_linearize.argtypes = par + [_P, _P, C.c_int64, C.c_int, C.c_int, C.c_int] + \
        [C.c_double] * 4 + [_P] * 4
    return h


def _p(a):
    return a.ctypes.data_as(_P)


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


# ---------------------------------------------------------------- the ABI
def test_chain_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_chain.h") == NAMES
    assert sorted(_lib.CHAIN_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    others = set(_functions("hop.h")) | set(_functions("hop_wide.h")) | \
        set(_functions("hop_wide_jcurve.h"))
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        assert name not in others
        assert name not in _lib.SIGNATURES and name not in _lib.WIDE_SIGNATURES
        assert name not in _lib.WIDE_JCURVE_SIGNATURES
    assert len(_functions("hop.h")) == 40
    assert lib.hop_abi_version() == 1


def test_chain_header_is_in_the_build_digest():
    from time_opt_ilqr_amd import build
    assert "hop_chain.h" in inspect.getsource(build._digest)
    assert "chain.hip" in build.SOURCES and "chain_dynamics.hpp" in build.HEADERS


def _params(p=12, m=3, dt=0.1):
    from time_opt_ilqr_amd import _lib
    return _lib.ChainParams(p, m, dt, 2.0, 0.5, 0.3)


D = C.c_void_p(16)  # never dereferenced: every call here ends on the host


def _calls(lib, par, *, batch=4, null=False, n_alloc=10, n_use=10, n_alpha=5, ws=1 << 40,
           only=None):
    """every launching entry (or the one named) with the same bad or empty arguments:
    name -> rc.  Every call made here must end on the host."""
    q = None if null else D
    pp = C.byref(par) if par is not None else None
    al = (C.c_double * 8)(*([1.0] * 8))
    cost = (q, 0, q, 0, q, q, q, q, 0)
    fns = {
        "dynamics": lambda: lib.hop_chain_dynamics_f64(pp, q, 64, q, 64, batch, q, 64, None),
        "rollout": lambda: lib.hop_chain_rollout_f64(pp, q, 0, q, batch, n_alloc, 1e6, q, None),
        "linearize": lambda: lib.hop_chain_linearize_f64(pp, q, q, batch, n_alloc, n_use, 1, 1e-5,
                                                         1e-5, 1e-6, 1e-6, q, q, q, q, None),
        "cost": lambda: lib.hop_chain_cost_true_f64(pp, q, q, q, *cost, batch, n_alloc, q, None),
        "linesearch": lambda: lib.hop_chain_forward_linesearch_f64(
            pp, q, q, *cost, q, q, q, q, al, n_alpha, batch, n_alloc, q, ws, q, q, q, q, q, None),
    }
    return {k: f() for k, f in fns.items() if only in (None, k)}


def test_chain_validation_without_gpu(lib):
    err = lib.hop_last_error
    for p, m, msg in ((0, 1, b"p must be in [1, 15]"), (16, 1, b"p must be in [1, 15]"),
                      (4, 0, b"m must be in [1, p]"), (4, 5, b"m must be in [1, p]")):
        par = _params(p, m)
        for name, rc in _calls(lib, par).items():
            assert rc == -2, (p, m, name)
        lib.hop_chain_rollout_f64(C.byref(par), D, 0, D, 4, 10, 1e6, D, None)
        assert msg in err()
        assert lib.hop_chain_forward_workspace_bytes(C.byref(par), 4, 10, 5) == 0
        # the shape is checked for an empty batch too
        assert all(rc == -2 for rc in _calls(lib, par, batch=0).values())
    for dt in (0.0, -0.1, float("nan")):
        assert all(rc == -1 for rc in _calls(lib, _params(dt=dt)).values())
        assert b"dt must be positive" in err()
    par = _params()
    assert all(rc == -1 for rc in _calls(lib, par, null=True).values())
    assert b"null" in err()
    assert all(rc == -1 for rc in _calls(lib, None).values())
    one = lambda name, **kw: _calls(lib, par, only=name, **kw)[name]  # noqa: E731
    assert one("linearize", n_use=11) == -1 and b"n_use > n_alloc" in err()
    for na in (0, 9):
        assert one("linesearch", n_alpha=na) == -1 and b"n_alpha" in err()
    need = lib.hop_chain_forward_workspace_bytes(C.byref(par), 4, 10, 5)
    assert need == 4 * 5 * (1 + 11 * 24 + 10 * 3) * 8
    assert one("linesearch", ws=need - 1) == -1 and b"workspace too small" in err()
    assert all(rc == -1 for rc in _calls(lib, par, batch=-1).values())
    assert one("linearize", n_alloc=-1, n_use=-1) == -1
    # too many rows for one launch
    assert all(rc == -2 for rc in _calls(lib, par, batch=1 << 40).values())
    # an empty batch launches nothing, with or without pointers; so does n_use = 0
    assert all(rc == 0 for rc in _calls(lib, par, batch=0).values())
    assert all(rc == 0 for rc in _calls(lib, par, batch=0, null=True).values())
    assert one("linearize", n_use=0) == 0


def test_spring_chain_object_and_refusals_without_gpu():
    from time_opt_ilqr_amd import engine, solver, systems
    F = systems.SpringChain(12, 3)
    assert (F.n, F.m, F.dt, F.k, F.ks, F.c) == (24, 3, 0.1, 2.0, 0.5, 0.3)
    assert engine.is_chain(F) and engine.system_dims(F) == (24, 3)
    assert not engine.is_chain(2) and not engine.is_chain("quadrotor")
    for p, m in ((0, 1), (16, 2), (4, 5), (4, 0)):
        with pytest.raises(ValueError):
            systems.SpringChain(p, m)
    mk = systems.MAKERS["spring_chain"](12, 3, seed=4024)
    assert isinstance(mk[0], systems.SpringChain) and len(mk) == 13
    # the problem data of make_golden_wide.py's problem(): the stored fixture's x0
    d = np.load(os.path.join(REPO, "tests", "golden", "wide_solve_n24_0.npz"))
    x0 = systems.make_spring_chain(12, 3, seed=int(d["seed"]))[1]
    assert np.array_equal(x0, d["x0"]) and np.array_equal(mk[4], d["Q"])
    assert np.array_equal(mk[5], d["R"]) and (mk[6], mk[7]) == (float(d["alpha"]), float(d["w"]))
    assert solver._on_device(F)
    with pytest.raises(ValueError):  # a Python stage cost needs host dynamics
        solver.ilqr_timeopt_batch(F, mk[1], mk[2], mk[3], mk[4], mk[5], np.eye(24), 0.5, 60, 8, 55,
                                  extra_stage_cost=lambda x, u: (0.0, np.zeros(24),
                                                                 np.zeros((24, 24))))


# ---------------------------------------------------------------- the math
def _batch(p, m, seed, rows):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (rows, 2 * p)), rng.uniform(-1.0, 1.0, (rows, m))


def test_host_system_is_the_numpy_chain_bit_for_bit():
    from time_opt_ilqr_amd import systems
    for p, m in SHAPES + [(12, 12)]:
        X, U = _batch(p, m, 10 * p + m, 23)
        H = systems.SpringChain(p, m, 0.1).host()
        assert H.vectorized and (H.n, H.m) == (2 * p, m)
        assert np.array_equal(H.F(X, U), chain_F(p, m)(X, U))
        ref = chain_F_reference(p, m)
        rows = np.stack([ref(X[r], U[r]) for r in range(len(X))])
        assert np.array_equal(H.F(X, U), rows)
        assert np.array_equal(H(X[0], U[0]), rows[0])


@pytest.mark.parametrize("p,m", SHAPES)
def test_kernel_math_F(chain_host, p, m):
    X, U = _batch(p, m, 100 + p, 41)
    out = np.full_like(X, -7.0)
    assert chain_host.chain_host_dynamics(p, m, 0.1, 2.0, 0.5, 0.3, _p(X), _p(U), len(X),
                                          _p(out)) == 0
    ref = chain_F(p, m)(X, U)
    err = float(np.abs(out - ref).max())
    print(f"chain F host p={p} m={m}: max abs err {err:.2e}")
    assert err <= F_TOL
    assert np.array_equal(out[:, :p], ref[:, :p])  # q' bitwise: no sin reaches it


def _host_lin(h, p, m, X, U, central, n_use=None, dt=0.1):
    Bn, N = U.shape[:2]
    n = 2 * p
    n_use = N if n_use is None else n_use
    A = np.full((Bn, N, n, n), -7.0)
    B = np.full((Bn, N, n, m), -7.0)
    ar = np.full((Bn, N, n), -7.0)
    Fx = np.full((Bn, N, n), -7.0)
    assert h.chain_host_linearize(p, m, dt, 2.0, 0.5, 0.3, _p(X), _p(U), Bn, N, n_use,
                                  int(central), 1e-5, 1e-5, 1e-6, 1e-6, _p(A), _p(B), _p(ar),
                                  _p(Fx)) == 0
    return A, B, ar, Fx


def stencil(p, m):
    """mask [n, n + m] of the entries a column can reach (the others are exact zeros)"""
    n = 2 * p
    S = np.zeros((n, n + m), dtype=bool)
    for j in range(p):
        S[j, j] = S[j, p + j] = S[p + j, p + j] = True
        for a in (j - 1, j, j + 1):
            if 0 <= a < p:
                S[p + a, j] = True
    for j in range(m):
        S[p + j * p // m, n + j] = True
    return S


def check_lin(p, m, got, ref, tag):
    """the issue's bars: A, B, a_res to 1e-9, the unreachable entries exactly 0.0, the q'
    rows of A and B bitwise"""
    A, B, ar = got
    Ar, Br, arr = ref
    S = stencil(p, m)
    AB, ABr = np.concatenate((A, B), -1), np.concatenate((Ar, Br), -1)
    errs = [float(np.abs(a - b).max()) for a, b in ((A, Ar), (B, Br), (ar, arr))]
    print(f"chain lin {tag} p={p} m={m}: max abs err A {errs[0]:.2e} B {errs[1]:.2e} "
          f"a_res {errs[2]:.2e}")
    assert max(errs) <= LIN_TOL
    assert (AB[..., ~S] == 0.0).all() and (ABr[..., ~S] == 0.0).all()
    assert np.array_equal(AB[..., :p, :], ABr[..., :p, :])


@pytest.mark.parametrize("central", [False, True])
@pytest.mark.parametrize("p,m", SHAPES)
def test_kernel_math_linearize(chain_host, p, m, central):
    from time_opt_ilqr_amd import host_dynamics, systems
    rng = np.random.default_rng(7 * p + m)
    Bn, N = 3, 5
    X = rng.uniform(-1.0, 1.0, (Bn, N + 1, 2 * p))
    U = rng.uniform(-1.0, 1.0, (Bn, N, m))
    A, B, ar, Fx = _host_lin(chain_host, p, m, X, U, central)
    H = systems.SpringChain(p, m, 0.1).host()
    ref = host_dynamics.linearize_batch(H, X, U, central=central)
    check_lin(p, m, (A, B, ar), ref, "host " + ("central" if central else "forward"))
    # the per-call form of the reference's loops gives the same numbers
    one = host_dynamics.linearize(chain_F_reference(p, m), X[0], U[0], central=central)
    assert all(np.array_equal(a, b[0]) for a, b in zip(one, ref))
    assert float(np.abs(Fx - chain_F(p, m)(X[:, :N].reshape(-1, 2 * p), U.reshape(-1, m))
                        .reshape(Bn, N, -1)).max()) <= F_TOL


def test_kernel_math_forward_marks_a_nan_step(chain_host):
    from time_opt_ilqr_amd import host_dynamics, systems
    p, m = 8, 3
    rng = np.random.default_rng(5)
    X = rng.uniform(-1.0, 1.0, (1, 5, 2 * p))
    U = rng.uniform(-1.0, 1.0, (1, 4, m))
    X[0, 2, 3] = np.nan
    H = systems.SpringChain(p, m, 0.1).host()
    for central in (False, True):
        A, B, ar, _ = _host_lin(chain_host, p, m, X, U, central)
        Ar, Br, arr = host_dynamics.linearize_batch(H, X, U, central=central)
        assert np.array_equal(np.isnan(A), np.isnan(Ar))
        assert np.array_equal(np.isnan(B), np.isnan(Br))
        assert np.array_equal(np.isnan(ar), np.isnan(arr))
        ok = ~np.isnan(Ar)
        assert float(np.abs(A[ok] - Ar[ok]).max()) <= LIN_TOL
        if not central:
            assert np.isnan(A[0, 2]).all() and np.isnan(B[0, 2]).all()
            assert not np.isnan(A[0, [0, 1, 3]]).any()


def test_kernel_math_n_use_leaves_the_tail(chain_host):
    p, m = 8, 3
    rng = np.random.default_rng(6)
    X = rng.uniform(-1.0, 1.0, (2, 8, 2 * p))
    U = rng.uniform(-1.0, 1.0, (2, 7, m))
    A, B, ar, Fx = _host_lin(chain_host, p, m, X, U, True, n_use=5)
    for t in (A, B, ar, Fx):
        assert (t[:, 5:] == -7.0).all() and (t[:, :5] != -7.0).any()
    A2, B2, ar2, _ = _host_lin(chain_host, p, m, X[:, :6].copy(), U[:, :5].copy(), True)
    assert np.array_equal(A[:, :5], A2) and np.array_equal(B[:, :5], B2)
    assert np.array_equal(ar[:, :5], ar2)
