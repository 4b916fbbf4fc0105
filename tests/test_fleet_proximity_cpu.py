"""CPU: the fleets' proximity cost (include/hop_fleet_proximity.h).

* the three entries are exported and bound in a table of their own; hop_fleet.h keeps its
  seven functions and hop.h its 40; the header and sources are in the build lists;
* every entry validates the cost on the host before any launch;
* systems.Fleet.stage_cost() (the NumPy twin) against the reference-side fixtures
  (tests/golden/make_golden_fleet_proximity.py), against central differences, and the
  second-order term symmetric and positive semidefinite;
* systems.Proximity / Fleet validation, the scope refusals, and make_fleet_crossing.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NAMES = ["hop_fleet_prox_cost_true_f64", "hop_fleet_prox_forward_linesearch_f64",
         "hop_fleet_proximity_taylor_f64"]
FLEET_NAMES = ["hop_fleet_cost_true_f64", "hop_fleet_dynamics_f64",
               "hop_fleet_forward_linesearch_f64", "hop_fleet_forward_workspace_bytes",
               "hop_fleet_linearize_f64", "hop_fleet_rollout_f64"]
# base system id, count, n, m, pd (the issue's table)
SHAPES = {"pm3": (3, 3, 12, 6, 2), "pm4": (3, 4, 16, 8, 2), "pm7": (3, 7, 28, 14, 2),
          "quad2": (2, 2, 24, 8, 3), "di15": (0, 15, 30, 15, 1)}
SOLVE_TAGS = ["pm3", "pm4", "pm7", "quad2", "di15"]
_P = C.c_void_p


@pytest.fixture(scope="module")
def lib():
    from time_opt_ilqr_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _functions(header):
    src = open(os.path.join(REPO, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"^\s*(?:int|int64_t|size_t|const char\*)\s+(hop_\w+)\s*\(", src,
                                 flags=re.M)))


def _fleet(tag, d=None):
    from time_opt_ilqr_amd import systems
    sid, count, n, m, pd = SHAPES[tag]
    prox = None
    if d is not None:
        prox = systems.Proximity(d["prox_obs"], tuple(d["prox_sep"]))
    F = systems.Fleet(sid, count, proximity=prox)
    assert (F.n, F.m, F.pos_dim) == (n, m, pd)
    return F


# ---------------------------------------------------------------- the ABI
def test_proximity_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_fleet_proximity.h") == NAMES
    assert sorted(_lib.FLEET_PROXIMITY_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES, _lib.FLEET_SIGNATURES, _lib.ONEPASS_SIGNATURES):
            assert name not in table
    # the headers the existing tests pin keep their lists
    assert _functions("hop_fleet.h") == FLEET_NAMES and sorted(_lib.FLEET_SIGNATURES) == FLEET_NAMES
    assert len(_functions("hop.h")) == 40 and lib.hop_abi_version() == 1
    text = open(os.path.join(REPO, "include", "hop_fleet_proximity.h")).read()
    assert f"#define HOP_FLEET_MAX_OBSTACLES {_lib.FLEET_MAX_OBSTACLES} " in text
    # the struct's layout: pointer, int32 (padded), two doubles
    assert C.sizeof(_lib.FleetProximity) == 32
    assert _lib.FleetProximity.sep_radius.offset == 16


def test_proximity_sources_are_in_the_build_lists():
    from time_opt_ilqr_amd import build
    assert "hop_fleet_proximity.h" in inspect.getsource(build._digest)
    assert "fleet_proximity.hpp" in build.HEADERS and "fleet.hip" in build.SOURCES


# ---------------------------------------------------------------- validation
D = C.c_void_p(16)  # never dereferenced: every call here ends on the host


def _calls(lib, prox, *, system=2, count=2, batch=4, stride=64, wrap=0, only=None):
    """the three entries (or those named) with the cost under test: name -> rc.  Every call
    made here must end on the host: each is given an argument that the host refuses, or an
    empty batch."""
    from time_opt_ilqr_amd import _lib
    par = _lib.FleetParams(system, count, 0.05)
    pp = C.byref(par)
    px = C.byref(prox) if prox is not None else None
    al = (C.c_double * 8)(*([1.0] * 8))
    cost = (D, 0, D, 0, D, D, D, D, 0, wrap)
    fns = {
        "taylor": lambda: lib.hop_fleet_proximity_taylor_f64(pp, px, D, stride, batch, D, D, D,
                                                             None),
        "cost": lambda: lib.hop_fleet_prox_cost_true_f64(pp, D, D, D, *cost, px, batch, 10, D,
                                                         None),
        "linesearch": lambda: lib.hop_fleet_prox_forward_linesearch_f64(
            pp, D, D, *cost, px, D, D, D, D, al, 5, batch, 10, D, 1 << 40, D, D, D, D, D, None),
    }
    return {k: f() for k, f in fns.items() if only is None or k in only}


def test_proximity_validation_without_gpu(lib):
    from time_opt_ilqr_amd import _lib
    err = lib.hop_last_error
    P = _lib.FleetProximity
    inf, nan = float("inf"), float("nan")
    # a valid cost and an empty batch: nothing launched, with or without a table
    for ok in (P(D, 16, 0.4, 1.5), P(None, 0, 0.4, 1.5), P(None, 0, 0.0, 0.0), P(D, 3, -1.0, 0.0)):
        assert all(rc == 0 for rc in _calls(lib, ok, batch=0).values())
    bad = [(None, b"null proximity"),
           (P(D, -1, 0.4, 1.0), b"n_obs"), (P(D, 17, 0.4, 1.0), b"n_obs"),
           (P(None, 1, 0.4, 1.0), b"null obstacle table"),
           (P(D, 2, 0.0, 1.0), b"separation radius"), (P(D, 2, -0.4, 1.0), b"separation radius"),
           (P(D, 2, nan, 1.0), b"separation radius"), (P(D, 2, inf, 1.0), b"separation radius"),
           (P(D, 2, 0.4, inf), b"separation weight"), (P(D, 2, 0.4, nan), b"separation weight"),
           (P(D, 2, 0.4, -1.0), b"separation weight")]
    for prox, msg in bad:
        for batch in (4, 0):  # the cost is checked for an empty batch too
            for name, rc in _calls(lib, prox, batch=batch).items():
                assert rc == -1 and msg in err(), (name, msg, err())
    # the fleet's own checks come first and keep their codes
    good = P(D, 2, 0.4, 1.0)
    assert all(rc == -2 for rc in _calls(lib, good, count=3).values())
    assert all(rc == -1 for rc in _calls(lib, good, system=7, count=1).values())
    assert all(rc == -1 for rc in _calls(lib, good, batch=-1).values())
    assert all(rc == -2 for rc in _calls(lib, good, batch=1 << 40).values())
    r = _calls(lib, good, wrap=1 << 24, only=("cost", "linesearch"))
    assert r == {"cost": -1, "linesearch": -1} and b"wrap bits" in err()
    assert _calls(lib, good, stride=23, only=("taylor",)) == {"taylor": -1} and b"stride" in err()
    # null pointers with rows to process
    par = _lib.FleetParams(2, 2, 0.05)
    assert lib.hop_fleet_proximity_taylor_f64(C.byref(par), C.byref(good), None, 24, 4, D, D, D,
                                              None) == -1
    # no output asked for: nothing to do
    assert lib.hop_fleet_proximity_taylor_f64(C.byref(par), C.byref(good), None, 24, 4, None,
                                              None, None, None) == 0


# ---------------------------------------------------------------- the NumPy twin
@pytest.mark.parametrize("tag", list(SHAPES))
def test_stage_cost_matches_the_fixtures(tag):
    from test_gpu_fleet import case_inputs
    from test_gpu_fleet_proximity import prox_inputs
    sid, count, n, m, pd = SHAPES[tag]
    d = np.load(os.path.join(GOLDEN, f"fleet_prox_cases_{tag}.npz"))
    c = case_inputs(int(d["seed"]), n, m, n // count)
    obs, sep = prox_inputs(int(d["seed"]), c, count, n // count, pd)
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum(), obs.sum()])
    assert np.array_equal(got, d["check"]) and np.array_equal(obs, d["prox_obs"])
    assert tuple(d["prox_sep"]) == sep and (obs[:, pd + 1] == 0.0).sum() == 1
    F = _fleet(tag, d)
    cost = F.stage_cost()
    w_bump = max(float(obs[:, pd + 1].max()), sep[1])
    assert d["tay_c"].max() >= 0.1 * w_bump  # the bumps are not all ~0
    worst = 0.0
    pos = np.zeros(n, dtype=bool)
    pos[F.position_idx] = True
    for b in range(len(d["tay_c"])):
        x = c["X"][b, 0]
        cc, cx, cxx = cost(x, None)
        for g, r in ((cc, d["tay_c"][b]), (cx, d["tay_cx"][b]), (cxx, d["tay_cxx"][b])):
            g, r = np.asarray(g), np.asarray(r)
            assert np.array_equal(g == 0.0, r == 0.0)
            nz = r != 0.0
            if nz.any():
                worst = max(worst, float(np.max(np.abs(g[nz] - r[nz]) / np.abs(r[nz]))))
        # off the position entries: exact zeros
        assert not cx[~pos].any() and not cxx[~pos].any() and not cxx[:, ~pos].any()
        # symmetric, and positive semidefinite
        assert np.array_equal(cxx, cxx.T)
        ev = np.linalg.eigvalsh(cxx)
        assert ev[0] >= -1e-12 * ev[-1], (tag, b, ev[0], ev[-1])
        # cx against central differences of c: the truncation error of a step h is
        # h^2 / 6 |c'''| <= h^2 / 6 * 2 c / r^3 with r >= 0.3, c <= sum of the weights
        if b < 8:
            h = 1e-5
            fd = np.zeros(n)
            for i in F.position_idx:
                e = np.zeros(n)
                e[i] = h
                fd[i] = (cost(x + e)[0] - cost(x - e)[0]) / (2 * h)
            assert np.abs(fd - cx).max() <= 1e-6 * max(1.0, np.abs(cx).max()), (tag, b)
    print(f"stage_cost {tag}: max elementwise rel err vs the fixture {worst:.2e}")
    assert worst <= 1e-13


def test_stage_cost_without_a_cost_is_zero():
    from time_opt_ilqr_amd import systems
    F = systems.Fleet(3, 4)
    assert F.proximity is None and F.pos_dim == 2 and F.fleet_params() == (3, 4, 0.05)
    c, cx, cxx = F.stage_cost()(np.ones(16), None)
    assert c == 0.0 and not cx.any() and not cxx.any() and cxx.shape == (16, 16)
    # a fleet of one with separation only: no pair
    F1 = systems.Fleet(3, 1, proximity=systems.Proximity(separation=(0.4, 2.0)))
    assert F1.stage_cost()(np.ones(4), None)[0] == 0.0


# ---------------------------------------------------------------- the objects
def test_proximity_and_fleet_validation():
    from time_opt_ilqr_amd import engine, systems
    P = systems.Proximity
    p = P([[0.3, 0.2, 0.5, 1.5]], (0.4, 1.5))
    assert p.obstacles.shape == (1, 4) and p.separation == (0.4, 1.5)
    assert P().obstacles.size == 0 and P().separation is None and P().sep() == (1.0, 0.0)
    assert P(obstacles=np.zeros((0, 4))).table(2).shape == (0, 4)
    for kw in (dict(obstacles=[[0.0, 0.0, 0.0, 1.0]]), dict(obstacles=[[0.0, 0.0, -1.0, 1.0]]),
               dict(obstacles=[[0.0, 0.0, 1.0, -1.0]]), dict(obstacles=[[0.0, 0.0, 1.0, np.inf]]),
               dict(obstacles=[[0.0, 0.0, 1.0, np.nan]]), dict(obstacles=[[0.0, 0.0, np.nan, 1.0]]),
               dict(obstacles=[[np.nan, 0.0, 1.0, 1.0]]), dict(obstacles=np.zeros((17, 4)) + 1.0),
               dict(obstacles=[0.0, 0.0, 1.0, 1.0]), dict(separation=(0.0, 1.0)),
               dict(separation=(-0.4, 1.0)), dict(separation=(0.4, -1.0)),
               dict(separation=(0.4, np.inf)), dict(separation=(np.nan, 1.0))):
        with pytest.raises(ValueError):
            P(**kw)
    assert len(P(obstacles=np.zeros((16, 4)) + 1.0).obstacles) == 16
    # the column count is checked against the fleet's pd when the cost is attached
    for base, count, pd in (("pointmass", 4, 2), ("quadrotor", 2, 3), (0, 8, 1), ("cartpole", 3, 1),
                            ("segway", 3, 1)):
        ok = P(np.ones((2, pd + 2)), (0.4, 1.0))
        F = systems.Fleet(base, count, proximity=ok)
        assert F.proximity is ok and F.pos_dim == pd and engine.fleet_proximity(F) is ok
        assert len(F.fleet_params()) == 3
        with pytest.raises(ValueError, match="columns"):
            systems.Fleet(base, count, proximity=P(np.ones((2, pd + 3))))
    with pytest.raises(TypeError):
        systems.Fleet(3, 4, proximity=[[0.0, 0.0, 1.0, 1.0]])
    assert engine.fleet_proximity(systems.Fleet(3, 4)) is None
    assert engine.fleet_proximity(3) is None and engine.fleet_proximity("pointmass") is None
    text = P.__doc__
    assert "give" in text and "the positions weight" in text and "NotImplementedError" in text


def test_refusals_stay():
    """onepass, the point-mass obstacle table and a Python stage cost still raise for a
    fleet, with or without a proximity cost"""
    from time_opt_ilqr_amd import solver, systems
    mk = systems.make_fleet_crossing("pointmass", 4, N=80, seed=7000, w_scale=400.0)
    F, x0, xg, ur, Q, R, Qf, w, N, T_min, T_max = mk[:11]
    assert F.proximity is not None
    stage = F.stage_cost()
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
    ):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError, match="proximity"):
        from time_opt_ilqr_amd import engine
        engine.fleet_proximity_cost(systems.Fleet(3, 4), np.zeros((2, 16)))


@pytest.mark.parametrize("tag", SOLVE_TAGS)
def test_make_fleet_crossing_rebuilds_the_fixture_problems(tag):
    """systems.make_fleet_crossing and the generator's problem() are one recipe"""
    from time_opt_ilqr_amd import systems
    sid, count, n, m, pd = SHAPES[tag]
    for trial in range(3):
        d = np.load(os.path.join(GOLDEN, f"fleet_prox_solve_{tag}_{trial}.npz"))
        mk = systems.make_fleet_crossing(sid, count, N=int(d["N"]), seed=int(d["seed"]),
                                         w_scale=float(d["scale"]), q_pos=float(d["q_pos"]),
                                         bump_weight=float(d["bump_weight"]),
                                         T_min=int(d["T_min"]))
        for got, key in zip(mk[1:7], ("x0", "xg", "u_ref", "Q", "R", "Qf")):
            assert np.array_equal(got, d[key]), (tag, trial, key)
        assert mk[7] == float(d["w"]) and mk[8:11] == (int(d["N"]), int(d["T_min"]), int(d["T_max"]))
        assert mk[11] == d["wrap_idx"].tolist() == mk[0].wrap_idx and mk[12] is None
        prox = mk[0].proximity
        assert np.array_equal(prox.table(pd), d["prox_obs"]) and prox.sep() == tuple(d["prox_sep"])
        # positions carry weight in Q (the select needs it)
        assert (np.diag(d["Q"])[mk[0].position_idx] >= float(d["q_pos"])).all()
        for method in ("propagator", "bruteforce"):
            assert float(d[f"gaps_{method}"].min()) >= 1e-3 and len(d[f"T_hist_{method}"]) >= 2


def test_generator_inputs_are_one_text():
    """the generator and the tests build the kernel-level inputs from the same functions"""
    def body(path, name):
        src = open(path).read()
        return src.split(f"# BEGIN {name}")[1].split(f"# END {name}")[0].split("\n", 1)[1]
    gen = os.path.join(GOLDEN, "make_golden_fleet_proximity.py")
    a = body(gen, "case_inputs")
    assert a == body(os.path.join(GOLDEN, "make_golden_fleet.py"), "case_inputs")
    assert a == body(os.path.join(REPO, "tests", "test_gpu_fleet.py"), "case_inputs")
    b = body(gen, "prox_inputs")
    assert b == body(os.path.join(REPO, "tests", "test_gpu_fleet_proximity.py"), "prox_inputs")
    assert "def prox_inputs(" in b
