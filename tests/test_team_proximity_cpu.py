"""CPU: the teams' proximity cost (include/hop_mixed_proximity.h).

* the three entries are exported and bound in a table of their own, absent from every other
  table and header; the new header does not name the teams' header or its entries; the header
  and sources are in the build lists;
* every entry validates the composition and the cost on the host before any launch;
* systems.Team.with_proximity and stage_cost() (the NumPy twin) against the reference-side
  fixtures (tests/golden/make_golden_team_proximity.py), against central differences, the
  second-order term symmetric and positive semidefinite, and an equal-member team's twin
  equal to the fleet's;
* the scope refusals, and make_team_crossing.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
NAMES = ["hop_mixed_prox_cost_true_f64", "hop_mixed_prox_forward_linesearch_f64",
         "hop_mixed_proximity_taylor_f64"]
# member ids, n, m, dt, D
SHAPES = {"pm_quad_di": ((3, 2, 0), 18, 7, 0.05, 3), "di2_pm2": ((0, 0, 3, 3), 12, 6, 0.05, 2),
          "quad_pm3": ((2, 3, 3, 3), 24, 10, 0.05, 3), "pm7_di": ((3,) * 7 + (0,), 30, 15, 0.05, 2),
          "all5": ((0, 1, 2, 3, 4), 26, 9, 0.02, 3)}
PDS = {0: 1, 1: 1, 2: 3, 3: 2, 4: 1}
NS = {0: 2, 1: 4, 2: 12, 3: 4, 4: 4}
SOLVE_TAGS = ["di2_pm2", "pm_quad_di", "quad_pm3"]


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


def _team(tag, d=None):
    from time_opt_ilqr_amd import systems
    ids, n, m, dt, D = SHAPES[tag]
    F = systems.Team(ids, dt=dt)
    if d is not None:
        F = F.with_proximity(systems.Proximity(d["prox_obs"], tuple(d["prox_sep"])))
    assert (F.n, F.m, F.pos_dim, F.pos_dims) == (n, m, D, tuple(PDS[s] for s in ids))
    return F


# ---------------------------------------------------------------- the ABI
def test_mixed_proximity_header_symbols_exported_and_separate(lib):
    from time_opt_ilqr_amd import _lib
    assert _functions("hop_mixed_proximity.h") == NAMES
    assert sorted(_lib.MIXED_PROXIMITY_SIGNATURES) == NAMES
    out = os.popen(f"nm -D {_lib.LIB_PATH}").read()
    headers = sorted(h for h in os.listdir(os.path.join(REPO, "include")) if h.endswith(".h"))
    for name in NAMES:
        assert hasattr(lib, name) and re.search(rf"\bT {name}\b", out), name
        for table in (_lib.SIGNATURES, _lib.WIDE_SIGNATURES, _lib.WIDE_JCURVE_SIGNATURES,
                      _lib.CHAIN_SIGNATURES, _lib.FLEET_SIGNATURES,
                      _lib.FLEET_PROXIMITY_SIGNATURES, _lib.TEAM_SIGNATURES,
                      _lib.ONEPASS_SIGNATURES, _lib.TESTHOOK_SIGNATURES):
            assert name not in table
        for h in headers:
            if h != "hop_mixed_proximity.h":
                assert name not in open(os.path.join(REPO, "include", h)).read(), (name, h)
    text = open(os.path.join(REPO, "include", "hop_mixed_proximity.h")).read()
    assert "hop_team" not in text
    assert '#include "hop_fleet_proximity.h"' in text and "hop_fleet_proximity*" in text
    # the headers the existing tests pin keep their lists
    assert len(_functions("hop_team.h")) == 6 and len(_functions("hop_fleet_proximity.h")) == 3
    assert len(_functions("hop.h")) == 40 and lib.hop_abi_version() == 1
    # the fleet proximity entries' lists after the flat composition
    S, Fp = _lib.MIXED_PROXIMITY_SIGNATURES, _lib.FLEET_PROXIMITY_SIGNATURES
    i32, ptr = C.c_int32, C.c_void_p
    assert S[NAMES[2]] == (C.c_int, [i32, ptr] + Fp["hop_fleet_proximity_taylor_f64"][1][1:])
    assert S[NAMES[0]] == (C.c_int, [i32, ptr] + Fp["hop_fleet_prox_cost_true_f64"][1][1:])
    assert S[NAMES[1]] == (C.c_int, [i32, ptr, C.c_double]
                           + Fp["hop_fleet_prox_forward_linesearch_f64"][1][1:])


def test_mixed_proximity_sources_are_in_the_build_lists():
    from time_opt_ilqr_amd import build
    assert "hop_mixed_proximity.h" in inspect.getsource(build._digest)
    assert "team_proximity.hpp" in build.HEADERS and "team.hip" in build.SOURCES
    src = open(os.path.join(build.CSRC, "team.hip")).read()
    assert src.index("struct TeamRow") < src.index('#include "team_proximity.hpp"')


# ---------------------------------------------------------------- validation
D = C.c_void_p(16)  # never dereferenced: every call here ends on the host


def _calls(lib, prox, *, ids=(3, 2, 0), members=None, null_ids=False, dt=0.05, batch=4,
           stride=64, wrap=0, only=None):
    """the three entries (or those named) with the cost under test: name -> rc.  Every call
    made here must end on the host: each is given an argument that the host refuses, or an
    empty batch."""
    arr = (C.c_int32 * max(len(ids), 1))(*ids)
    sp = None if null_ids else arr
    cnt = len(ids) if members is None else members
    px = C.byref(prox) if prox is not None else None
    al = (C.c_double * 8)(*([1.0] * 8))
    cost = (D, 0, D, 0, D, D, D, D, 0, wrap)
    fns = {
        "taylor": lambda: lib.hop_mixed_proximity_taylor_f64(cnt, sp, px, D, stride, batch, D, D,
                                                             D, None),
        "cost": lambda: lib.hop_mixed_prox_cost_true_f64(cnt, sp, D, D, D, *cost, px, batch, 10,
                                                         D, None),
        "linesearch": lambda: lib.hop_mixed_prox_forward_linesearch_f64(
            cnt, sp, dt, D, D, *cost, px, D, D, D, D, al, 5, batch, 10, D, 1 << 40, D, D, D, D, D,
            None),
    }
    return {k: f() for k, f in fns.items() if only is None or k in only}


def test_mixed_proximity_validation_without_gpu(lib):
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
    # the team's own checks come first and keep their codes
    good = P(D, 2, 0.4, 1.0)
    for members in (0, 16, -1):
        assert all(rc == -2 for rc in _calls(lib, good, members=members).values())
        assert b"count must be in [1, 15]" in err()
    assert all(rc == -2 for rc in _calls(lib, None, members=0).values())
    assert all(rc == -1 for rc in _calls(lib, good, ids=(3, 5)).values()) and b"unknown" in err()
    assert all(rc == -1 for rc in _calls(lib, good, ids=(-1,)).values())
    assert all(rc == -1 for rc in _calls(lib, good, null_ids=True).values()) and b"null member" in err()
    assert all(rc == -2 for rc in _calls(lib, good, ids=(2, 2, 2)).values()) and b"n must be" in err()
    assert all(rc == -2 for rc in _calls(lib, good, ids=(0,) * 15 + (0,), members=15,
                                         batch=1 << 40).values())
    for dt in (0.0, -0.05, nan):  # only the line search steps
        assert _calls(lib, good, dt=dt, only=("linesearch",)) == {"linesearch": -1}
        assert b"dt must be positive" in err()
    assert all(rc == -1 for rc in _calls(lib, good, batch=-1).values())
    assert all(rc == -2 for rc in _calls(lib, good, batch=1 << 40).values())
    r = _calls(lib, good, wrap=1 << 18, only=("cost", "linesearch"))
    assert r == {"cost": -1, "linesearch": -1} and b"wrap bits" in err()
    assert _calls(lib, good, stride=17, only=("taylor",)) == {"taylor": -1} and b"stride" in err()
    assert _calls(lib, good, stride=18, batch=0, only=("taylor",)) == {"taylor": 0}
    # null pointers with rows to process; no output asked for: nothing to do
    ids = (C.c_int32 * 3)(3, 2, 0)
    assert lib.hop_mixed_proximity_taylor_f64(3, ids, C.byref(good), None, 18, 4, D, D, D,
                                              None) == -1
    assert lib.hop_mixed_proximity_taylor_f64(3, ids, C.byref(good), None, 18, 4, None, None,
                                              None, None) == 0


# ---------------------------------------------------------------- the NumPy twin
def _inputs(tag):
    from test_gpu_team import case_inputs
    from test_gpu_team_proximity import prox_inputs
    ids, n, m, dt, Dw = SHAPES[tag]
    d = np.load(os.path.join(GOLDEN, f"team_prox_cases_{tag}.npz"))
    xo = [int(v) for v in np.cumsum([0] + [NS[s] for s in ids[:-1]])]
    c = case_inputs(int(d["seed"]), n, m, xo[1])
    obs, sep = prox_inputs(int(d["seed"]), c, xo, [PDS[s] for s in ids])
    return c, d, obs, sep


@pytest.mark.parametrize("tag", list(SHAPES))
def test_stage_cost_matches_the_fixtures(tag):
    ids, n, m, dt, Dw = SHAPES[tag]
    c, d, obs, sep = _inputs(tag)
    got = np.array([c["X"].sum(), c["U"].sum(), c["Q"].sum(), c["x0"].sum(), obs.sum()])
    assert np.array_equal(got, d["check"]) and np.array_equal(obs, d["prox_obs"])
    assert obs.shape == (4, Dw + 2) and tuple(d["prox_sep"]) == sep
    assert (obs[:, Dw + 1] == 0.0).sum() == 1
    assert d["members"].tolist() == list(ids) and float(d["dt"]) == dt
    F = _team(tag, d)
    cost = F.stage_cost()
    w_bump = max(float(obs[:, Dw + 1].max()), sep[1])
    assert d["tay_c"].max() >= 0.1 * w_bump  # the bumps are not all ~0
    worst = 0.0
    pos = np.zeros(n, dtype=bool)
    pos[F.position_idx] = True
    assert pos.sum() == sum(F.pos_dims)
    for b in range(len(d["tay_c"])):
        x = c["X"][b, 0]
        cc, cx, cxx = cost(x, None)
        for g, r in ((cc, d["tay_c"][b]), (cx, d["tay_cx"][b]), (cxx, d["tay_cxx"][b])):
            g, r = np.asarray(g), np.asarray(r)
            assert np.array_equal(g == 0.0, r == 0.0)
            nz = r != 0.0
            if nz.any():
                worst = max(worst, float(np.max(np.abs(g[nz] - r[nz]) / np.abs(r[nz]))))
        # off the position entries (a DI's absent y, a point mass's absent z): exact zeros
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
    print(f"team stage_cost {tag}: max elementwise rel err vs the fixture {worst:.2e}")
    assert worst <= 1e-13


def test_stage_cost_without_a_cost_is_zero():
    from time_opt_ilqr_amd import systems
    F = systems.Team([3, 2, 0])
    assert F.proximity is None and F.pos_dim == 3 and F.pos_dims == (2, 3, 1)
    c, cx, cxx = F.stage_cost()(np.ones(18), None)
    assert c == 0.0 and not cx.any() and not cxx.any() and cxx.shape == (18, 18)
    # a team of one with separation only: no pair
    F1 = systems.Team([3]).with_proximity(systems.Proximity(separation=(0.4, 2.0)))
    assert F1.stage_cost()(np.ones(4), None)[0] == 0.0


@pytest.mark.parametrize("sid,count", [(3, 4), (2, 2), (0, 15), (1, 5)])
def test_equal_member_team_stage_cost_is_the_fleets(sid, count):
    from time_opt_ilqr_amd import systems
    pd = PDS[sid]
    rng = np.random.default_rng(100 * sid + count)
    obs = np.concatenate([rng.uniform(-0.6, 0.6, (3, pd)), rng.uniform(0.3, 0.6, (3, 1)),
                          rng.uniform(0.5, 2.0, (3, 1))], axis=1)
    p = systems.Proximity(obs, (0.45, 1.3))
    Fl = systems.Fleet(sid, count, proximity=p)
    Tm = systems.Team([sid] * count).with_proximity(p)
    assert Tm.pos_dim == Fl.pos_dim == pd and Tm.position_idx == Fl.position_idx
    a, b = Fl.stage_cost(), Tm.stage_cost()
    for _ in range(5):
        x = rng.uniform(-0.8, 0.8, Fl.n)
        for g, r in zip(b(x), a(x)):
            assert np.array_equal(np.asarray(g), np.asarray(r))
    assert a(x)[0] > 0.0


# ---------------------------------------------------------------- the objects
def test_with_proximity_and_its_errors():
    from time_opt_ilqr_amd import engine, systems
    P = systems.Proximity
    F = systems.Team([3, 2, 0], dt=0.04)
    assert F.proximity is None and engine.team_proximity(F) is None
    p = P(np.ones((2, 5)), (0.4, 1.0))
    G = F.with_proximity(p)
    assert G is not F and F.proximity is None and G.proximity is p
    assert engine.team_proximity(G) is p and engine.fleet_proximity(G) is None
    assert engine.is_team(G) and not engine.is_fleet(G)
    for key in ("member_ids", "dt", "n", "m", "x_offsets", "u_offsets", "wrap_idx",
                "position_idx", "name", "pos_dims", "pos_dim"):
        assert getattr(G, key) == getattr(F, key), key
    assert G.team_params() == F.team_params()
    assert G.with_proximity(P()).proximity is not p
    # the table's columns are checked against D = the largest pd
    for ids, Dw in (((3, 2, 0), 3), ((0, 0, 3, 3), 2), ((0, 1, 4), 1), ((2,), 3)):
        T = systems.Team(ids, dt=0.05)
        assert T.pos_dim == Dw
        assert T.with_proximity(P(np.ones((2, Dw + 2)))).proximity is not None
        with pytest.raises(ValueError, match="columns"):
            T.with_proximity(P(np.ones((2, Dw + 3))))
    for bad in ([[0.0, 0.0, 0.0, 1.0, 1.0]], None, "proximity", (0.4, 1.0)):
        with pytest.raises(TypeError):
            F.with_proximity(bad)
    # the constructor keeps its signature
    with pytest.raises(TypeError):
        systems.Team([3, 2, 0], proximity=p)
    assert engine.team_proximity(systems.Fleet(3, 4, proximity=P(np.ones((1, 4))))) is None
    assert engine.team_proximity(3) is None
    assert "with_proximity" in systems.Team.__doc__ and "pos_dim" in systems.Team.__doc__


def test_refusals_stay():
    """onepass, the point-mass obstacle table and a Python stage cost still raise for a
    team with a proximity cost"""
    from time_opt_ilqr_amd import engine, solver, systems
    mk = systems.make_team_crossing([0, 0, 3, 3], N=80, seed=7000, w_scale=1600.0, T_min=10)
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
        engine.team_proximity_cost(systems.Team([0, 0, 3, 3]), np.zeros((2, 12)))


@pytest.mark.parametrize("tag", SOLVE_TAGS)
def test_make_team_crossing_rebuilds_the_fixture_problems(tag):
    """systems.make_team_crossing and the generator's problem() are one recipe"""
    from time_opt_ilqr_amd import systems
    ids, n, m, dt, Dw = SHAPES[tag]
    for trial in range(3):
        d = np.load(os.path.join(GOLDEN, f"team_prox_solve_{tag}_{trial}.npz"))
        assert d["members"].tolist() == list(ids)
        mk = systems.make_team_crossing(ids, N=int(d["N"]), seed=int(d["seed"]),
                                        w_scale=float(d["scale"]), q_pos=float(d["q_pos"]),
                                        bump_weight=float(d["bump_weight"]),
                                        T_min=int(d["T_min"]), dt=float(d["dt"]))
        for got, key in zip(mk[1:7], ("x0", "xg", "u_ref", "Q", "R", "Qf")):
            assert np.array_equal(got, d[key]), (tag, trial, key)
        assert mk[7] == float(d["w"]) and mk[8:11] == (int(d["N"]), int(d["T_min"]), int(d["T_max"]))
        assert mk[11] == d["wrap_idx"].tolist() == mk[0].wrap_idx and mk[12] is None
        prox = mk[0].proximity
        assert np.array_equal(prox.table(Dw), d["prox_obs"]) and prox.sep() == tuple(d["prox_sep"])
        assert d["prox_obs"][0, :Dw].tolist() == [0.3, 0.2, 0.0][:Dw]
        # the starts lie on the circle of radius 2, member a on its first pd_a coordinates
        F = mk[0]
        for xo, pd in zip(F.x_offsets, F.pos_dims):
            r = np.linalg.norm(mk[1][xo:xo + pd])
            assert r <= 2.0 + 1e-12 and (pd == 1 or abs(r - 2.0) <= 1e-12)
        # positions carry weight in Q (the select needs it); no coupling between members
        assert (np.diag(d["Q"])[F.position_idx] >= float(d["q_pos"])).all()
        a, b = F.x_offsets[0], F.x_offsets[1]
        assert d["Q"][a, b] == 0.0
        for method in ("propagator", "bruteforce"):
            assert float(d[f"gaps_{method}"].min()) >= 1e-3 and len(d[f"T_hist_{method}"]) >= 2
    # the defaults follow make_team's rules
    a, b = systems.make_team_crossing(ids, dt=dt), systems.make_team(ids, dt=dt)
    assert a[8:11] == b[8:11] and a[7] == b[7]


def test_generator_inputs_are_one_text():
    """the generator and the tests build the kernel-level inputs from the same functions"""
    def body(path, name):
        src = open(path).read()
        return src.split(f"# BEGIN {name}")[1].split(f"# END {name}")[0].split("\n", 1)[1]
    gen = os.path.join(GOLDEN, "make_golden_team_proximity.py")
    a = body(gen, "case_inputs")
    assert a == body(os.path.join(GOLDEN, "make_golden_team.py"), "case_inputs")
    assert a == body(os.path.join(REPO, "tests", "test_gpu_team.py"), "case_inputs")
    b = body(gen, "prox_inputs")
    assert b == body(os.path.join(REPO, "tests", "test_gpu_team_proximity.py"), "prox_inputs")
    assert "def prox_inputs(" in b
