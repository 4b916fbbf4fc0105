"""No kernel may read or write global memory outside its tensors (include/hop.h, "Memory
contract").

Every other GPU test hands the kernels tensors fresh from the PyTorch allocator: 512-byte
aligned and followed by slack nobody inspects.  Here each entry runs four times: once on
ordinary tensors (the baseline, held to the oracle bar of the entry's own test), and once
per pattern of tests/arena.py with every input placed in, and every output and workspace
carved from, an arena filled with that pattern (the engine's allocations are served from the
arena by arena.Arena.shim; product code is unchanged).  Every case asserts

  * bitwise invariance: the documented part of every output equals the baseline bit for
    bit under all three patterns (the kernels are deterministic);
  * write containment: Arena.check() reports nothing, every pad still holds its pattern;
  * documented extents: outside the extent the header documents an output still holds the
    pattern, and the union over the three runs of the elements that do not hold it is
    exactly that extent (an int32 0 holds two of the patterns, none holds all three);
  * inputs untouched: every placed input is bit-identical afterwards;
  * minimal alignment: every pointer is aligned to its element size and no more (% 16 == 8
    for f64, % 8 == 4 for f32 / int32; byte workspaces to 8, the trajectory-form workspace
    to 256 by the engine's own rounding).

Shapes are the smallest at which an off-by-one in problem, step or lane can happen: batch
tails (B = 5: an idle wave in the last wide workgroup; B = 70: no multiple of 64),
n_alloc = 5 odd (a problem stride of 8 mod 16 at s = 13) and n_use = 3 < n_alloc.
"""
import contextlib
import functools

import numpy as np
import pytest

from arena import PATTERNS, Arena
from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

NA, NU = 5, 3        # n_alloc (odd) and n_use < n_alloc of the sweeps
TOL = {"f64": 1e-9, "f32": 2e-3}   # the sweeps' bars (tests/test_gpu_z0.py)
ALL = True           # an output the header documents as written everywhere


def _tdt(dt):
    import torch
    return {"f64": torch.float64, "f32": torch.float32, "i32": torch.int32}[dt]


def _t(x, dev, dt="f64"):
    import torch
    return torch.as_tensor(np.array(x, order="C"), dtype=_tdt(dt), device=dev)


def _np(t):
    return t.double().cpu().numpy() if t.dtype.is_floating_point else t.cpu().numpy()


def _elem_rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _rel(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def _bits(t):
    import torch
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 1: torch.uint8}[t.element_size()])


def _is_tile(v):
    from time_opt_ilqr_amd import engine
    return isinstance(v, engine.Tile64)


def _placed(arena, inputs, inout):
    """the inputs with every tensor (Tile64 data included) copied into the arena"""
    import torch
    from time_opt_ilqr_amd import engine
    out = {}
    for k, v in inputs.items():
        if isinstance(v, torch.Tensor):
            out[k] = arena.place(v, name=k, inout=k in inout)
        elif _is_tile(v):
            out[k] = engine.Tile64(arena.place(v.data, name=k), v.batch, v.rows, v.cols)
        else:
            out[k] = v
    return out


def _flat(outs):
    return {k: (v.data if _is_tile(v) else v) for k, v in outs.items() if v is not None}


def run_case(dev, label, inputs, call, extents, inout=(), capacity=32 << 20):
    """_run_case; a HIP error (a fault leaves the device unusable for this process) ends the
    session instead of running the remaining tests on it"""
    try:
        return _run_case(dev, label, inputs, call, extents, inout, capacity)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"{label}: {e}", returncode=3)
        raise


def _run_case(dev, label, inputs, call, extents, inout, capacity):
    """Run call(inputs) -> {name: output tensor} on ordinary tensors and once per pattern
    in an arena, and assert what the module docstring lists.  extents[name] is ALL or a
    bool array of the output's shape: the elements the header documents as written (or a
    function of the baseline outputs returning those).  inout names the arguments the
    header documents as in/out: call returns them among its outputs (extent ALL), they are
    compared whole, and the baseline runs on copies.  Returns the baseline outputs."""
    import torch
    from time_opt_ilqr_amd import engine
    mine = {k: (v.clone() if k in inout else v) for k, v in inputs.items()}  # in/out: a copy
    base = {k: v.clone() for k, v in _flat(call(mine)).items()}
    torch.cuda.synchronize()
    if callable(extents):
        extents = extents(base)
    assert set(extents) == set(base), (sorted(extents), sorted(base))
    doc = {k: torch.ones(base[k].shape, dtype=torch.bool, device=dev) if extents[k] is ALL
           else torch.as_tensor(np.asarray(extents[k], dtype=bool), device=dev) for k in base}
    for k in base:
        assert doc[k].shape == base[k].shape, (k, doc[k].shape, base[k].shape)
    union = {k: torch.zeros_like(doc[k]) for k in base}
    problems = []
    for pat in PATTERNS:
        arena = Arena(pat, capacity, dev)
        placed = _placed(arena, inputs, inout)
        with arena.shim(engine):
            outs = _flat(call(placed))
        torch.cuda.synchronize()
        assert set(outs) == set(base)
        align = {}
        for v in arena.views:
            mod = 2 * max(v.tensor.element_size(), 8 if v.tensor.dtype == torch.uint8 else 0)
            key = f"{str(v.tensor.dtype).replace('torch.', '')}%{mod}"
            align.setdefault(key, set()).add(v.tensor.data_ptr() % mod)
        assert all(r == {int(k.split("%")[1]) // 2} for k, r in align.items()), align
        for s in arena.check():
            problems.append((hex(pat), "stray write", s))
        for name in arena.changed():
            problems.append((hex(pat), "input changed", name))
        summary = []
        for k, o in outs.items():
            view = arena.find(o)
            assert view is not None and view.role != "input", f"{k} is not in the arena"
            assert view.tensor.shape == o.shape and view.tensor.data_ptr() == o.data_ptr(), k
            if view.role == "inout":  # it held its input, not the pattern: no written mask
                union[k] |= True
                if not torch.equal(_bits(o), _bits(base[k])):
                    where = (_bits(o) != _bits(base[k])).nonzero()[:4].tolist()
                    problems.append((hex(pat), "differs from the baseline", k, where))
                summary.append(f"{k} in/out")
                continue
            wm = arena.written_mask(o)
            union[k] |= wm
            if bool((wm & ~doc[k]).any()):
                where = (wm & ~doc[k]).nonzero()[:4].tolist()
                problems.append((hex(pat), "written outside the documented extent", k, where))
            if not torch.equal(_bits(o)[doc[k]], _bits(base[k])[doc[k]]):
                where = ((_bits(o) != _bits(base[k])) & doc[k]).nonzero()[:4].tolist()
                problems.append((hex(pat), "differs from the baseline", k, where))
            summary.append(f"{k} {int(wm.sum())}/{wm.numel()}")
        print(f"{label} pattern {pat:#018x}: written " + ", ".join(summary)
              + f"; {len(arena.views)} views, address residues "
              + ", ".join(f"{k}={sorted(v)}" for k, v in sorted(align.items())))
        del arena, placed, outs
    for k in base:
        if not torch.equal(union[k], doc[k]):
            problems.append(("all patterns", "documented extent not written", k,
                             (doc[k] & ~union[k]).nonzero()[:4].tolist()))
    assert not problems, problems
    return base


# ---------------------------------------------------------------------------
# sweeps: hop_lft_sweep_* (narrow s = 13, generic, small s, wide) and the tile64 entries
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lft(seed, Bn, s, m, n_alloc=NA):
    out = orc.synth_lft_batch(seed, Bn, s, m, n_alloc)
    for x in out:
        x.setflags(write=False)
    return out


def _sweep(dev, label, A, Bm, Q, R, z0, QT, dt="f64", opts=None, n_use=NU, t_min=None,
           dbg=False, tile=False, capacity=32 << 20):
    """engine.propagate in the arena; returns the baseline outputs"""
    from time_opt_ilqr_amd import _lib, engine
    blocks = {k: _t(v, dev, dt) for k, v in (("A", A), ("B", Bm), ("Q", Q), ("QT", QT))}
    if tile:
        blocks = {k: engine.to_tile64(v) for k, v in blocks.items()}
    inputs = dict(blocks, R=_t(R, dev, dt), z0=_t(z0, dev, dt))
    fuse = t_min is not None

    def call(i):
        kw = dict(return_efg=True, return_prefix=True) if dbg else {}
        with _lib.options(**(opts or {})):
            r = engine.propagate(i["A"], i["B"], i["Q"], i["R"], i["z0"], i["QT"], n_use=n_use,
                                 t_min=t_min, t_max=n_use if fuse else None, **kw)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star, efg=r.efg,
                    prefix=r.prefix)
    # hop.h: J [batch][n_use], status [batch]; t_star / j_star only when the argmin is
    # fused; dbg_efg / dbg_prefix [batch][n_use][3][s][s] only when asked for
    ext = dict(J=ALL, status=ALL)
    if fuse:
        ext.update(t_star=ALL, j_star=ALL)
    if dbg:
        ext.update(efg=ALL, prefix=ALL)
    base = run_case(dev, label, inputs, call, ext, capacity=capacity)
    assert tuple(base["J"].shape) == (A.shape[0], n_use)
    return base


def _check_sweep(base, A, Bm, Q, Ri, z0, QT, dt="f64", n_use=NU, t_min=None, rows=None):
    Bn = A.shape[0]
    rows = list(range(Bn)) if rows is None else rows
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0, QT, n_use)
    assert sto[rows].tolist() == [0] * len(rows)
    assert _np(base["status"])[rows].tolist() == [0] * len(rows)
    err = _elem_rel(_np(base["J"])[rows], Jo[rows])
    print(f"J elementwise relative error {err:.3e}")
    assert err <= TOL[dt]
    if t_min is not None and dt == "f64":
        To, _ = orc.select_horizon(Jo, t_min, n_use)
        assert _np(base["t_star"])[rows].tolist() == To[rows].tolist()
    return Jo


@pytest.mark.parametrize("Bn", [1, 5])
@pytest.mark.parametrize("path", ["cond", "generic", "refassoc", "forced"])
def test_narrow_sweep_s13(dev, path, Bn):
    """lft_sweep_v2.hip (conditioned default; reference association; every problem handed
    to the rerun launch) and lft_sweep.hip at s = 13, m = 4, fp64 with the fused argmin"""
    opts = {"cond": {}, "generic": dict(force_generic=True),
            "refassoc": dict(reference_assoc=True), "forced": dict(force_handover=True)}[path]
    A, Bm, Q, R, Ri, z0, QT = _lft(7100, Bn, 13, 4)
    base = _sweep(dev, f"s13-{path}-B{Bn}", A, Bm, Q, Ri, z0[0], QT, opts=opts, t_min=2)
    _check_sweep(base, A, Bm, Q, Ri, z0[0], QT, t_min=2)


def test_narrow_sweep_s13_genuine_handover(dev):
    """one problem needs chol_inv's escalated jitter (the recipe of tests/test_gpu_rerun.py):
    the conditioned kernel hands it over and the rerun launch recomputes it, bitwise the
    reference-association kernel; the others stay healthy"""
    import torch
    from test_gpu_rerun import _escalate
    from time_opt_ilqr_amd import _lib, engine
    A, Bm, Q, R, Ri, z0, QT = _lft(7100, 5, 13, 4)
    Q = _escalate(Q, 3, 1)
    base = _sweep(dev, "s13-handover", A, Bm, Q, Ri, z0[0], QT, t_min=2)
    args = [_t(x, dev) for x in (A, Bm, Q, Ri, z0[0], QT)]
    with _lib.options(no_rerun=True):
        ho = _np(engine.propagate(*args, n_use=NU, t_min=2, t_max=NU).status)
    with _lib.options(reference_assoc=True):
        ref = engine.propagate(*args, n_use=NU, t_min=2, t_max=NU)
    torch.cuda.synchronize()
    assert np.nonzero(ho & _lib.ST_HANDOVER)[0].tolist() == [3]
    st = _np(base["status"])
    o = orc.lft_sweep(A[3], Bm[3], Q[3], Ri[3], z0[0], QT[3], NU)
    assert st[3] == o["status"] == orc.ST_JITTER
    assert torch.equal(_bits(base["J"][3]), _bits(ref.J[3]))
    assert torch.equal(base["t_star"][3], ref.t_star[3])
    _check_sweep(base, A, Bm, Q, Ri, z0[0], QT, t_min=2, rows=[0, 1, 2, 4])


@pytest.mark.parametrize("path", ["cond", "generic"])
def test_narrow_sweep_s13_per_problem_z0_per_step_R(dev, path):
    A, Bm, Q, R, Ri, z0, QT = _lft(7100, 5, 13, 4)
    zz = orc.synth_z0(("dense", "offset", "e_s", "big", "small"), 5, 13, 41)
    Rs, Ris = orc.synth_R_steps(77, 5, NA, 4)
    opts = dict(force_generic=True) if path == "generic" else {}
    base = _sweep(dev, f"s13-{path}-z0-Rstep", A, Bm, Q, Ris, zz, QT, opts=opts, t_min=2)
    _check_sweep(base, A, Bm, Q, Ris, zz, QT, t_min=2)


@pytest.mark.parametrize("dbg", [False, True])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("s,m", [(7, 3), (16, 6)])
def test_generic_narrow_sweep(dev, s, m, dt, dbg):
    """lft_sweep.hip: B = 5, n_alloc = n_use = 3, with and without the debug outputs"""
    A, Bm, Q, R, Ri, z0, QT = _lft(7200 + s, 5, s, m, 3)
    base = _sweep(dev, f"generic-s{s}-{dt}-dbg{int(dbg)}", A, Bm, Q, Ri, z0[0], QT, dt=dt,
                  n_use=3, t_min=1, dbg=dbg)
    _check_sweep(base, A, Bm, Q, Ri, z0[0], QT, dt=dt, n_use=3, t_min=1)
    if dbg and dt == "f64":
        efg, pre = _np(base["efg"]), _np(base["prefix"])
        for b in range(5):
            o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b], want_efg=True,
                              want_prefix=True)
            for i, (ke, kp) in enumerate((("E", "Ebar"), ("F", "Fbar"), ("G", "Gbar"))):
                assert _rel(efg[b, :, i], o[ke]) <= 1e-9 and _rel(pre[b, :, i], o[kp]) <= 1e-9


@pytest.mark.parametrize("Bn", [1, 70])
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("path", ["default", "lane", "refassoc", "forced", "tile64"])
def test_small_sweep_blocks(dev, path, dt, Bn):
    """lft_small.hip and the row-group kernel of lft_sweep_v2.hip at s = 5, m = 2: both
    layouts, both dtypes, a batch that is no multiple of the 64-lane wave"""
    opts = {"default": {}, "tile64": {}, "lane": dict(small_lane=True),
            "refassoc": dict(reference_assoc=True), "forced": dict(force_handover=True)}[path]
    A, Bm, Q, R, Ri, z0, QT = _lft(7300, Bn, 5, 2, 3)
    base = _sweep(dev, f"s5-{path}-{dt}-B{Bn}", A, Bm, Q, Ri, z0[0], QT, dt=dt, opts=opts,
                  n_use=3, t_min=1, tile=path == "tile64")
    _check_sweep(base, A, Bm, Q, Ri, z0[0], QT, dt=dt, n_use=3, t_min=1)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("inverse", [False, True])
def test_tile64_conversion(dev, dt, inverse):
    """hop_tile64_*: both directions at B = 70; the padding slots of the last tile are
    written 0, so the whole tile64 tensor is the documented extent"""
    import torch
    from time_opt_ilqr_amd import engine
    x = _t(np.random.default_rng(5).standard_normal((70, 3, 5, 2)), dev, dt)
    if inverse:
        src = engine.to_tile64(x)
        base = run_case(dev, f"from_tile64-{dt}", dict(t=src),
                        lambda i: dict(x=engine.from_tile64(i["t"])), dict(x=ALL))
        assert torch.equal(base["x"], x)
    else:
        base = run_case(dev, f"to_tile64-{dt}", dict(x=x),
                        lambda i: dict(t=engine.to_tile64(i["x"])), dict(t=ALL))
        t = base["t"]
        assert tuple(t.shape) == (2, 3, 10, 64)
        ref = torch.zeros((128, 3, 10), dtype=x.dtype, device=dev)
        ref[:70] = x.reshape(70, 3, 10)
        assert torch.equal(t, ref.reshape(2, 64, 3, 10).permute(0, 2, 3, 1))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_select_horizon(dev, dt):
    """hop_select_horizon_*: ld = 7 > t_max = 5, B = 5"""
    from time_opt_ilqr_amd import engine
    J = np.random.default_rng(11).standard_normal((5, 7))
    J[:, 5:] = -100.0  # past t_max: must not win
    J[1, 0] = -50.0    # before t_min: must not win
    base = run_case(dev, f"select-{dt}", dict(J=_t(J, dev, dt)),
                    lambda i: dict(zip(("t_star", "j_star"), engine.select_horizon(i["J"], 2, 5))),
                    dict(t_star=ALL, j_star=ALL))
    Jr = _np(_t(J, dev, dt))
    To, Jo = orc.select_horizon(Jr, 2, 5)
    assert _np(base["t_star"]).tolist() == To.tolist()
    assert np.array_equal(_np(base["j_star"]), Jo)


@pytest.mark.parametrize("Bn", [1, 5])
@pytest.mark.parametrize("s,m", [(17, 3), (32, 8)])
def test_wide_sweep(dev, s, m, Bn):
    """lft_wide_kernel with the debug outputs (the last workgroup of B = 5 has an idle wave)"""
    A, Bm, Q, R, Ri, z0, QT = _lft(7400 + s, Bn, s, m)
    base = _sweep(dev, f"wide-s{s}-B{Bn}", A, Bm, Q, Ri, z0[0], QT, t_min=2, dbg=True)
    _check_sweep(base, A, Bm, Q, Ri, z0[0], QT, t_min=2)
    efg, pre = _np(base["efg"]), _np(base["prefix"])
    for b in range(Bn):
        o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b], NU, want_efg=True,
                          want_prefix=True)
        for i, (ke, kp) in enumerate((("E", "Ebar"), ("F", "Fbar"), ("G", "Gbar"))):
            assert _rel(efg[b, :, i], o[ke]) <= 1e-9 and _rel(pre[b, :, i], o[kp]) <= 1e-9


# ---------------------------------------------------------------------------
# the builders and the trajectory form
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _traj(n, m, Bn=5, N=NA):
    from test_gpu_traj import _batch
    return _batch(range(900, 900 + Bn), n, m, N)


_TRAJ_KEYS = ("A", "B", "a_res", "X", "U", "xg", "u_ref", "Q")


@pytest.mark.parametrize("n,m,dt", [(16, 4, "f64"), (31, 8, "f64"), (12, 4, "f64"),
                                    (4, 1, "f64"), (4, 1, "f32")])
def test_augment(dev, n, m, dt):
    """hop_augment_wide_f64 (n >= 16) and hop_augment_f64 / _f32: blocks of steps < n_build
    = 3 of n_alloc = 5, z0 = e_s"""
    from test_gpu_traj import _blocks
    from time_opt_ilqr_amd import engine
    ps, st = _traj(n, m)
    inputs = {k: _t(st[k], dev, dt) for k in _TRAJ_KEYS}
    inputs.update(P=_t(st["P"], dev, dt), w=_t(st["w"], dev, dt))

    def call(i):
        o = engine.augment(*(i[k] for k in _TRAJ_KEYS), i["P"], i["w"], wrap_idx=st["wrap_idx"],
                           n_build=NU)
        return dict(A=o.A, B=o.B, Q=o.Q, QT=o.QT, z0=o.z0)
    base = run_case(dev, f"augment-n{n}-{dt}", inputs, call,
                    dict(A=ALL, B=ALL, Q=ALL, QT=ALL, z0=ALL))
    tol = 1e-14 if dt == "f64" else 1e-6
    for b, p in enumerate(ps):
        Aa, Ba, Qa, Ri, z0, QT = _blocks(p, 1e-12)
        for name, ref in (("A", Aa), ("B", Ba), ("Q", Qa), ("QT", QT)):
            assert _rel(_np(base[name][b]), np.array(ref)[:NU]) <= tol, (b, name)
    assert _np(base["z0"]).tolist() == [0.0] * n + [1.0]


@pytest.mark.parametrize("n,m,dt,opts", [
    (12, 4, "f64", {}),                       # blocks built inside the sweep, no workspace
    (12, 4, "f64", dict(traj_unfused=True)),  # hop_augment into the 256-byte workspace
    (24, 6, "f64", {}),                       # the wide builder and the wide sweep
    (4, 1, "f64", {}), (4, 1, "f64", dict(small_lane=True)), (4, 2, "f32", {})])
def test_trajectory_form(dev, n, m, dt, opts):
    from test_gpu_traj import _oracle
    from time_opt_ilqr_amd import _lib, engine
    ps, st = _traj(n, m)
    inputs = {k: _t(st[k], dev, dt) for k in _TRAJ_KEYS}
    inputs.update(R_inv=_t(st["R_inv"], dev, dt), P=_t(st["P"], dev, dt), w=_t(st["w"], dev, dt))

    def call(i):
        with _lib.options(**opts):
            r = engine.propagate_traj(*(i[k] for k in _TRAJ_KEYS), i["R_inv"], i["P"], i["w"],
                                      wrap_idx=st["wrap_idx"], rho_reg=1.0, n_use=NU, t_min=2,
                                      t_max=NU)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_case(dev, f"traj-n{n}-{dt}-{'-'.join(opts) or 'default'}", inputs, call,
                    dict(J=ALL, status=ALL, t_star=ALL, j_star=ALL))
    assert (_np(base["status"]) == 0).all()
    for b, p in enumerate(ps):
        _, o = _oracle(p, 1.0, NU)
        assert _rel(_np(base["J"][b]), o["J"]) <= TOL[dt], b
        if dt == "f64":
            assert int(base["t_star"][b]) == int(orc.select_horizon(o["J"][None], 2, NU)[0][0])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("Bn", [1, 70])
def test_trajectory_form_small_batch_major(dev, Bn, dt):
    """hop_lft_sweep_traj_* at s = 5, m = 2 on batch-major raw arrays: a batch that is no
    multiple of the 64-lane wave (fp64: hop_augment into the workspace and the row-group
    kernel; fp32: the fused lane kernel)"""
    from test_gpu_traj import _oracle
    from time_opt_ilqr_amd import engine
    ps, st = _traj(4, 2, Bn, 3)
    inputs = {k: _t(st[k], dev, dt) for k in _TRAJ_KEYS + ("R_inv", "P", "w")}

    def call(i):
        r = engine.propagate_traj(*(i[k] for k in _TRAJ_KEYS), i["R_inv"], i["P"], i["w"],
                                  wrap_idx=st["wrap_idx"], rho_reg=1.0, t_min=1, t_max=3)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_case(dev, f"traj-small-{dt}-B{Bn}", inputs, call,
                    dict(J=ALL, status=ALL, t_star=ALL, j_star=ALL))
    for b in sorted({0, Bn // 2, Bn - 1, min(63, Bn - 1), min(64, Bn - 1)}):
        _, o = _oracle(ps[b], 1.0)
        assert _rel(_np(base["J"][b]), o["J"]) <= TOL[dt], b


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("Bn", [1, 70])
def test_trajectory_form_tile64(dev, Bn, dt):
    """hop_lft_sweep_traj_tile64_*: the raw linearisation in the tile64 layout"""
    from test_gpu_traj import _oracle
    from time_opt_ilqr_amd import engine
    n, m = 4, 2
    ps, st = _traj(n, m, Bn, 3)
    raw = [_t(st[k], dev, dt) for k in _TRAJ_KEYS[:5]]
    inputs = {k: engine.to_tile64(x if x.dim() == 4 else x[..., None])
              for k, x in zip(_TRAJ_KEYS[:5], raw)}
    inputs.update({k: _t(st[k], dev, dt) for k in ("xg", "u_ref", "Q", "R_inv", "P", "w")})

    def call(i):
        r = engine.propagate_traj(*(i[k] for k in _TRAJ_KEYS), i["R_inv"], i["P"], i["w"],
                                  wrap_idx=st["wrap_idx"], rho_reg=1.0, t_min=1, t_max=3)
        return dict(J=r.J, status=r.status, t_star=r.t_star, j_star=r.j_star)
    base = run_case(dev, f"traj-tile64-{dt}-B{Bn}", inputs, call,
                    dict(J=ALL, status=ALL, t_star=ALL, j_star=ALL))
    for b in sorted({0, Bn // 2, Bn - 1, min(63, Bn - 1), min(64, Bn - 1)}):
        _, o = _oracle(ps[b], 1.0)
        assert _rel(_np(base["J"][b]), o["J"]) <= TOL[dt], b


# ---------------------------------------------------------------------------
# Riccati passes and J curves
# ---------------------------------------------------------------------------
RN, RB = 5, 5
R_T = np.array([1, 2, RN // 2, RN, RN], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _ric(n, m, n_alloc=RN):
    from test_gpu_lds_poison import _ric_problems
    return _ric_problems(n, m, n_alloc, RB, 9300)


def _steps_mask(shape, upto):
    """[B, L, ...] mask: step index < upto[b]"""
    mk = np.zeros(shape, dtype=bool)
    for b, u in enumerate(upto):
        mk[b, :u] = True
    return mk


def _riccati_case(dev, label, n, m, mode, opts=None, extra=False, legacy=False, dt="f64"):
    from test_gpu_lds_poison import _extra
    from time_opt_ilqr_amd import _lib, engine
    P = _ric(n, m)
    wrap, lm, w_stage = [1], 1e-3, (0.3 if mode == 1 else 0.0)
    ex, exo = _extra(P, n, RB, RN) if extra else (None, [None] * RB)
    names = ("A", "B", "X", "U", "xg", "u_ref", "Q", "R", "Qf")
    inputs = {k: _t(x, dev, dt) for k, x in zip(names, P[:9])}
    inputs.update(horizon=_t(R_T, dev, "i32"), lm=_t(np.full(RB, lm), dev, dt))
    if legacy:  # the legacy passes take Qf = alpha I
        inputs["Qf"] = _t(np.stack([a * np.eye(n) for a in P[9]]), dev, dt)
    if extra:
        inputs.update(qxx=_t(ex[0], dev, dt), qx=_t(ex[1], dev, dt), c=_t(ex[2], dev, dt))

    def call(i):
        with _lib.options(**(opts or {})):
            r = engine.riccati(*(i[k] for k in names), i["horizon"], i["lm"], mode=mode,
                               w_stage=w_stage, wrap_idx=wrap, qxx_extra=i.get("qxx"),
                               qx_extra=i.get("qx"), c_extra=i.get("c"), want_v=True,
                               legacy=legacy)
        return dict(K=r.K, k=r.k, status=r.status, Vxx=r.Vxx, Vx=r.Vx, V0=r.V0)
    # hop.h: K, k written for steps < horizon[b]; Vxx, Vx, V0 for steps <= horizon[b]
    ext = dict(K=_steps_mask((RB, RN, m, n), R_T), k=_steps_mask((RB, RN, m), R_T),
               Vxx=_steps_mask((RB, RN + 1, n, n), R_T + 1),
               Vx=_steps_mask((RB, RN + 1, n), R_T + 1), V0=_steps_mask((RB, RN + 1), R_T + 1),
               status=ALL)
    base = run_case(dev, label, inputs, call, ext)
    assert _np(base["status"]).tolist() == [0] * RB
    return base, P, (lm, w_stage, wrap, exo)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("path,n,m,extra", [("fast", 12, 4, False), ("fast", 12, 4, True),
                                            ("generic", 12, 4, False), ("generic", 7, 3, False),
                                            ("wide", 17, 4, False), ("wide", 31, 8, True)])
def test_riccati(dev, path, n, m, extra, mode):
    """riccati_fast.hip (n = 12, m = 4, fp64), riccati.hip (force_generic, and another
    shape) and riccati_wide.hip: horizons T = [1, 2, N // 2, N, N], every V output"""
    from test_gpu_lds_poison import SENTINEL, _check_riccati_oracle
    opts = dict(force_generic=True) if path == "generic" else {}
    base, P, (lm, w_stage, wrap, exo) = _riccati_case(
        dev, f"riccati-{path}-n{n}-mode{mode}-extra{int(extra)}", n, m, mode, opts, extra)
    for key, up in (("K", R_T), ("Vxx", R_T + 1)):  # the oracle helper's sentinel checks
        for b in range(RB):
            base[key][b, up[b]:] = SENTINEL
    _check_riccati_oracle(base, P, R_T, lm, mode, w_stage, wrap, exo, range(RB))


@pytest.mark.parametrize("mode", [0, 1])
def test_riccati_fp32(dev, mode):
    """hop_riccati_f32 (riccati.hip) against the fp64 oracle at the bar of
    test_riccati_fp32_generic_vs_oracle"""
    n, m = 7, 3
    base, P, (lm, w_stage, wrap, _) = _riccati_case(dev, f"riccati-f32-mode{mode}", n, m, mode,
                                                    dt="f32")
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    for i in range(RB):
        Ti = int(R_T[i])
        args = (list(A[i]), list(B[i]), X[i], U[i], xg[i], ur[i], Q[i], R[i], alpha[i], Ti)
        if mode == 0:
            _, Ks, ok = orc.riccati_truncated(*args, lm_lambda=lm, wrap_idx=wrap)
            assert ok
        else:
            Vxx, _, _, Ks, _ = orc.riccati_expand(*args, 0, lm_lambda=lm, w_stage=w_stage,
                                                  wrap_idx=wrap)
            assert _rel(_np(base["Vxx"][i, :Ti + 1]), np.array(Vxx)) <= 2e-3, i
        assert _rel(_np(base["K"][i, :Ti]), np.array(Ks)) <= 2e-3, i


@pytest.mark.parametrize("mode", [0, 1])
def test_riccati_legacy(dev, mode):
    """hop_riccati_legacy_f64 against the oracle's legacy passes at the bar of
    tests/test_gpu_forward.py's legacy cases (well-conditioned: 1e-10)"""
    n, m = 12, 4
    base, P, (lm, w_stage, wrap, _) = _riccati_case(dev, f"riccati-legacy-mode{mode}", n, m, mode,
                                                    legacy=True)
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    for i in range(RB):
        Ti = int(R_T[i])
        args = (list(A[i]), list(B[i]), X[i], U[i], xg[i], ur[i], Q[i], R[i], alpha[i], Ti)
        if mode == 0:
            ks, Ks, ok = orc.riccati_truncated_legacy(*args, lm_lambda=lm, wrap_idx=wrap)
            assert ok
        else:
            Vxx, Vx, V0, Ks, ks, st = orc.riccati_expand_legacy(
                *args, 0, lm_lambda=lm, w_stage=w_stage, wrap_idx=wrap)
            assert st == 0
            assert _rel(_np(base["Vxx"][i, :Ti + 1]), np.array(Vxx)) <= 1e-10
            assert _rel(_np(base["Vx"][i, :Ti + 1]), np.array(Vx)) <= 1e-10
            assert _rel(_np(base["V0"][i, :Ti + 1]), np.array(V0)) <= 1e-10
        assert _rel(_np(base["k"][i, :Ti]), np.array(ks).reshape(Ti, m)) <= 1e-10, i
        assert _rel(_np(base["K"][i, :Ti]), np.array(Ks)) <= 1e-10, i


@pytest.mark.parametrize("path,n,m", [("fast", 12, 4), ("fast-shared", 12, 4), ("generic", 12, 4),
                                      ("wide", 17, 4), ("legacy", 12, 4)])
def test_jcurve(dev, path, n, m):
    """hop_bruteforce_jcurve_* (the exact-size kernel's two builds: one wave per SIMD with a
    per-problem Q, two with a batch-shared Q; the generic kernel), _wide_f64 and _legacy_f64:
    B = 5, t_max = 5 < n_alloc = 6; J and status [B][t_max] are written everywhere"""
    from time_opt_ilqr_amd import _lib, engine
    P = _ric(n, m, 6)
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    names = ("A", "B", "X", "U", "xg", "u_ref", "Q", "R", "Qf")
    inputs = {k: _t(x, dev) for k, x in zip(names, P[:9])}
    wrap, lm, w_stage, t_max = [1], 1e-6, 0.7, 5
    if path == "legacy":  # the legacy passes take Qf = alpha I
        inputs["Qf"] = _t(np.stack([a * np.eye(n) for a in alpha]), dev)
    if path == "fast-shared":
        Q = np.stack([Q[0]] * RB)
        inputs["Q"] = _t(Q[0], dev)
    fn = engine.bruteforce_jcurve_wide if path == "wide" else engine.bruteforce_jcurve
    kw = dict(legacy=True) if path == "legacy" else {}

    def call(i):
        with _lib.options(force_generic=path == "generic"):
            J, st = fn(*(i[k] for k in names), t_max, lm_lambda=lm, w_stage=w_stage,
                       wrap_idx=wrap, **kw)
        return dict(J=J, status=st)
    base = run_case(dev, f"jcurve-{path}-n{n}", inputs, call, dict(J=ALL, status=ALL))
    assert tuple(base["J"].shape) == (RB, t_max)
    assert (_np(base["status"]) == 0).all()
    Jo = np.stack([orc.bruteforce_J(list(A[b]), list(B[b]), X[b], U[b], xg[b], ur[b], Q[b], R[b],
                                    float(alpha[b]), w_stage, t_max, lm_lambda=lm, wrap_idx=wrap,
                                    legacy=path == "legacy")
                   for b in range(RB)])
    if path == "legacy":  # the bar of tests/test_gpu_forward.py's legacy J curve
        assert _rel(_np(base["J"]), Jo) <= 1e-10
    else:                 # the bar of test_wide_jcurve_vs_oracle
        assert _elem_rel(_np(base["J"]), Jo) <= 1e-6


# ---------------------------------------------------------------------------
# the dynamics side: built-in systems (the segway's oracle is libm-free: bit-exact)
# ---------------------------------------------------------------------------
SEG = 4


def _steps(Bn, N, tail, n_use):
    return _steps_mask((Bn, N) + tail, [n_use] * Bn)


def _cost_params(i, wrap=None):
    from time_opt_ilqr_amd import engine
    return engine.CostParams(i["xg"], i["u_ref"], i["Q"], i["R"], i["Qf"], i["w"],
                             i.get("obstacles"), wrap)


@pytest.mark.parametrize("central", [False, True])
def test_linearize(dev, central):
    """hop_linearize_f64: B * N = 145 is no multiple of the 64-step tile; steps < n_use = 27
    of n_alloc = 29 are written, Fx included"""
    import torch
    from oracle import dyn_oracle as dyn
    from time_opt_ilqr_amd import engine
    Bn, N, nu = 5, 29, 27
    n, m = dyn.DIMS[SEG]
    rng = np.random.default_rng(504)
    X, U = 1.5 * rng.standard_normal((Bn, N + 1, n)), 1.5 * rng.standard_normal((Bn, N, m))
    dt = dyn.DEFAULT_DT[SEG]

    def call(i):
        r = engine.linearize(SEG, i["X"], i["U"], dt, central=central, n_use=nu, want_fx=True)
        return dict(A=r.A, B=r.B, a_res=r.a_res, Fx=r.Fx)
    ext = dict(A=_steps(Bn, N, (n, n), nu), B=_steps(Bn, N, (n, m), nu),
               a_res=_steps(Bn, N, (n,), nu), Fx=_steps(Bn, N, (n,), nu))
    Xt = _t(X, dev)
    base = run_case(dev, f"linearize-central{int(central)}", dict(X=Xt, U=_t(U, dev)), call, ext)
    ref = dyn.linearize(SEG, X[:, :nu + 1], U[:, :nu], dt, central=central)
    for key, r in zip(("A", "B", "a_res"), ref):
        assert np.array_equal(_np(base[key][:, :nu]), r, equal_nan=True), key
    assert torch.equal(base["Fx"][:, :nu] - Xt[:, 1:nu + 1], base["a_res"][:, :nu])


@pytest.mark.parametrize("nu", [29, 27])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_linearize_tile64(dev, dt, nu):
    """hop_linearize_tile64_*: the padding slots of the last tile are written 0; with n_use <
    n_alloc the engine zero-fills the rest, so every element of every output is written"""
    import torch
    from oracle import dyn_oracle as dyn
    from time_opt_ilqr_amd import engine
    Bn, N = 5, 29
    n, m = dyn.DIMS[SEG]
    rng = np.random.default_rng(505)
    X, U = _t(1.5 * rng.standard_normal((Bn, N + 1, n)), dev), \
        _t(1.5 * rng.standard_normal((Bn, N, m)), dev)
    step = dyn.DEFAULT_DT[SEG]
    odt = _tdt(dt)

    def call(i):
        r = engine.linearize(SEG, i["X"], i["U"], step, n_use=nu, tile64=True, tile64_dtype=odt)
        return dict(A=r.A, B=r.B, a_res=r.a_res, Xt=r.X, Ut=r.U)
    base = run_case(dev, f"linearize-tile64-{dt}-nuse{nu}", dict(X=X, U=U), call,
                    dict(A=ALL, B=ALL, a_res=ALL, Xt=ALL, Ut=ALL))
    bm = engine.linearize(SEG, X, U, step, n_use=nu)
    for key, ref, steps, r, c in (("A", bm.A, nu, n, n), ("B", bm.B, nu, n, m),
                                  ("a_res", bm.a_res, nu, n, 1), ("Xt", X, nu + 1, n, 1),
                                  ("Ut", U, nu, m, 1)):
        t = base[key]
        got = engine.from_tile64(engine.Tile64(t, Bn, r, c))
        assert torch.equal(got[:, :steps].reshape(Bn, steps, -1),
                           ref[:, :steps].to(odt).reshape(Bn, steps, -1)), key
        assert not bool(t[:, :, :, Bn:].any()), key  # the padding slots
        assert not bool(t[:, steps:].any()), key     # steps past n_use (zero-filled)


def _strided_dynamics(dev, label, entry, head, n, m, ref_fn):
    """hop_*_dynamics_f64 itself with row strides larger than n and m: only the n (m)
    leading entries of a row are read and written"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    rng = np.random.default_rng(5 + n)
    Xs, Us = _t(rng.uniform(-1, 1, (5, n + 3)), dev), _t(rng.uniform(-1, 1, (5, m + 2)), dev)
    fn = getattr(_lib.load(), entry)

    def call(i):
        out = engine._torch().empty((5, n + 1), dtype=torch.float64, device=dev)
        _lib.check(fn(*head, _lib.ptr(i["X"]), n + 3, _lib.ptr(i["U"]), m + 2, 5, _lib.ptr(out),
                      n + 1, _lib.stream_handle(dev)))
        return dict(Xn=out)
    ext = np.zeros((5, n + 1), dtype=bool)
    ext[:, :n] = True
    base = run_case(dev, label, dict(X=Xs, U=Us), call, dict(Xn=ext))
    ref = ref_fn(Xs[:, :n].contiguous(), Us[:, :m].contiguous())
    assert torch.equal(_bits(base["Xn"][:, :n]), _bits(ref))


def test_dynamics(dev):
    from oracle import dyn_oracle as dyn
    from time_opt_ilqr_amd import engine
    n, m = dyn.DIMS[SEG]
    rng = np.random.default_rng(44)
    X, U = 2.0 * rng.standard_normal((5, 7, n)), 2.0 * rng.standard_normal((5, 7, m))
    dt = dyn.DEFAULT_DT[SEG]
    base = run_case(dev, "dynamics", dict(X=_t(X, dev), U=_t(U, dev)),
                    lambda i: dict(Xn=engine.dynamics(SEG, i["X"], i["U"], dt)), dict(Xn=ALL))
    assert np.array_equal(_np(base["Xn"]), dyn.dynamics(SEG, X, U, dt), equal_nan=True)
    _strided_dynamics(dev, "dynamics-strided", "hop_dynamics_f64", (SEG, dt), n, m,
                      lambda x, u: engine.dynamics(SEG, x, u, dt))


@pytest.mark.parametrize("shared", [False, True])
def test_rollout(dev, shared):
    """hop_rollout_f64 with a per-problem and a shared x0 (batch stride 0); two rollouts
    leave max_state_norm and end in NaN rows, which are written too"""
    from oracle import dyn_oracle as dyn
    from oracle import ilqr_oracle as io
    from time_opt_ilqr_amd import engine
    n, m = dyn.DIMS[SEG]
    Bn, N, dt = 5, 6, dyn.DEFAULT_DT[SEG]
    rng = np.random.default_rng(45)
    x0 = 0.3 * rng.standard_normal((Bn, n))
    U = rng.standard_normal((Bn, N, m))
    U[1, 2], U[4, 0] = 1e9, 1e9
    x0 = x0[0] if shared else x0
    base = run_case(dev, f"rollout-shared{int(shared)}", dict(x0=_t(x0, dev), U=_t(U, dev)),
                    lambda i: dict(X=engine.rollout(SEG, i["x0"], i["U"], dt, max_state_norm=1e6)),
                    dict(X=ALL))
    X = _np(base["X"])
    ref = np.stack([io.rollout(SEG, dt, x0 if shared else x0[b], U[b]) for b in range(Bn)])
    assert np.array_equal(np.isnan(X), np.isnan(ref)) and np.isnan(ref[1, 3:]).all()
    assert _rel(np.nan_to_num(X), np.nan_to_num(ref)) <= 1e-13  # tests/test_gpu_forward.py


def _segway_cost(rng, Bn, per_problem):
    from oracle import dyn_oracle as dyn
    n, m = dyn.DIMS[SEG]
    G = rng.standard_normal((n, n))
    c = dict(xg=0.1 * rng.standard_normal((Bn, n) if per_problem else n), u_ref=np.zeros(m),
             Q=np.diag([1.0, 0.1, 2.0, 0.1]), R=np.eye(m) * 1e-2, Qf=G @ G.T + 5.0 * np.eye(n),
             w=np.array([0.02]))
    return c


def test_cost_true(dev):
    """hop_cost_true_f64: per-problem xg (a batch stride), T* = 0 (+inf) and T* > N (NaN)"""
    from oracle import dyn_oracle as dyn
    from oracle import ilqr_oracle as io
    from time_opt_ilqr_amd import engine
    n, m = dyn.DIMS[SEG]
    Bn, N = 5, 6
    rng = np.random.default_rng(46)
    X, U = rng.standard_normal((Bn, N + 1, n)), rng.standard_normal((Bn, N, m))
    T = np.array([1, 3, N, 0, N + 1], dtype=np.int32)
    c = _segway_cost(rng, Bn, True)
    inputs = dict(X=_t(X, dev), U=_t(U, dev), T=_t(T, dev, "i32"),
                  **{k: _t(v, dev) for k, v in c.items()})
    base = run_case(dev, "cost_true", inputs,
                    lambda i: dict(J=engine.cost_true(SEG, i["X"], i["U"], i["T"],
                                                      _cost_params(i, [2]))), dict(J=ALL))
    J = _np(base["J"])
    assert np.isposinf(J[3]) and np.isnan(J[4])
    for b in range(3):
        ref = io.cost_true(X[b], U[b], c["xg"][b], c["u_ref"], c["Q"], c["R"], c["Qf"], 0.02,
                           int(T[b]), wrap_idx=[2])
        assert abs(J[b] - ref) <= 1e-12 * max(1.0, abs(ref))


def _check_linesearch(base, sid, dt, X, U, K, k, T, active, c, wrap):
    """the bars of test_linesearch_mixed_batch_vs_oracle"""
    from oracle import ilqr_oracle as io
    acc, seen = _np(base["accepted"]), set()
    for b in range(len(T)):
        if not active[b]:
            assert acc[b] == -2 and np.array_equal(_np(base["X"][b]), X[b], equal_nan=True)
            assert np.array_equal(_np(base["U"][b]), U[b], equal_nan=True)
            continue
        Xo, Uo, Jo, ok, ai = io.forward_linesearch(sid, dt, X[b], U[b], c["xg"], c["u_ref"],
                                                   c["Q"], c["R"], c["Qf"], float(c["w"][0]),
                                                   int(T[b]), k[b], K[b], wrap_idx=wrap)
        seen.add(ai)
        assert acc[b] == ai, (b, acc[b], ai)
        Jg = float(base["J"][b])
        assert abs(Jg - Jo) <= 1e-12 * max(1.0, abs(Jo)) or (np.isinf(Jo) and np.isinf(Jg))
        assert _rel(_np(base["X"][b]), Xo) <= 1e-11 and _rel(_np(base["U"][b]), Uo) <= 1e-11
    return seen


def _linesearch_case(dev, label, sid, dt, X, U, K, k, T, active, c, wrap, capacity=32 << 20):
    """hop_forward_linesearch_f64.  hop.h: X_new, U_new, J, J_old and accepted are written
    for every problem (an inactive or rejected problem's rows are copies of X and U)"""
    from time_opt_ilqr_amd import engine
    inputs = dict(X=_t(X, dev), U=_t(U, dev), K=_t(K, dev), k=_t(k, dev), T=_t(T, dev, "i32"),
                  active=_t(active, dev, "i32"), **{key: _t(v, dev) for key, v in c.items()})

    def call(i):
        r = engine.forward_linesearch(sid, i["X"], i["U"], i["T"], i["K"], i["k"],
                                      _cost_params(i, wrap), dt, active=i["active"])
        return dict(X=r.X, U=r.U, J=r.J, J_old=r.J_old, accepted=r.accepted)
    return run_case(dev, label, inputs, call, dict(X=ALL, U=ALL, J=ALL, J_old=ALL, accepted=ALL),
                    capacity=capacity)


def test_forward_linesearch_segway(dev):
    from oracle import dyn_oracle as dyn
    from oracle import ilqr_oracle as io
    n, m = dyn.DIMS[SEG]
    Bn, N, dt = 5, 8, dyn.DEFAULT_DT[SEG]
    rng = np.random.default_rng(47)
    U = 0.5 * rng.standard_normal((Bn, N, m))
    X = np.stack([io.rollout(SEG, dt, np.array([0.5, 0.0, 0.2, 0.0]), U[b]) for b in range(Bn)])
    K = 0.05 * rng.standard_normal((Bn, N, m, n))
    k = -0.5 * U + 0.05 * rng.standard_normal((Bn, N, m))
    k[2] = -k[2] * 50.0
    T = np.array([N, 3, N, 5, 0], dtype=np.int32)
    active = np.array([1, 1, 1, 0, 1], dtype=np.int32)
    c = _segway_cost(rng, Bn, False)
    base = _linesearch_case(dev, "linesearch-segway", SEG, dt, X, U, K, k, T, active, c, [2])
    seen = _check_linesearch(base, SEG, dt, X, U, K, k, T, active, c, [2])
    print("accepted", _np(base["accepted"]).tolist())
    assert len(seen) >= 2, seen


def _quadrotor_linesearch_inputs(golden_dir, Bn):
    """the recipe of test_linesearch_mixed_batch_vs_oracle on the first steps of the
    captured line search: feed-forwards scaled per problem, T* = 0, one inactive problem"""
    from test_gpu_forward import _case
    d, sid, wrap, obs = _case(golden_dir, "quadrotor")
    g = lambda key: d[f"f1_{key}"]  # noqa: E731
    N, T0 = int(d["N"]), int(g("T_star"))
    sc = np.array([1, 300, -1, 3, 10, 30, 100])[np.arange(Bn) % 7]
    X, U = np.stack([g("X")] * Bn), np.stack([g("U")] * Bn)
    K, k = np.zeros((Bn, N, 4, 12)), np.zeros((Bn, N, 4))
    K[:, :T0] = g("K")
    k[:, :T0] = g("k")[None] * sc[:, None, None]
    T = np.full(Bn, T0, dtype=np.int32)
    T[np.arange(Bn) % 7 == 5] = 0
    T[np.arange(Bn) % 7 == 6] = N
    active = np.ones(Bn, dtype=np.int32)
    active[np.arange(Bn) % 7 == 4] = 0
    c = {key: np.asarray(d[key], dtype=float) for key in ("xg", "u_ref", "Q", "R", "Qf")}
    c["w"] = np.array([float(d["w"])])
    return sid, float(d["dt"]), X, U, K, k, T, active, c, wrap


def test_forward_linesearch_quadrotor(dev, golden_dir):
    """two lanes per (problem, step size) rollout"""
    sid, dt, X, U, K, k, T, active, c, wrap = _quadrotor_linesearch_inputs(golden_dir, 7)
    base = _linesearch_case(dev, "linesearch-quadrotor", sid, dt, X, U, K, k, T, active, c, wrap)
    seen = _check_linesearch(base, sid, dt, X, U, K, k, T, active, c, wrap)
    print("accepted", _np(base["accepted"]).tolist())
    assert -1 in seen and len(seen) >= 3, seen


def test_obstacle_cost(dev):
    from time_opt_ilqr_amd import engine, systems
    rng = np.random.default_rng(5)
    X = rng.uniform(-2.5, 2.5, (3, 17, 4))
    obs = np.array([[o[0], o[1], r, wt] for o, r, wt in systems.OBSTACLES])
    base = run_case(dev, "obstacle_cost", dict(X=_t(X, dev), obs=_t(obs, dev)),
                    lambda i: dict(zip(("c", "cx", "cxx"), engine.obstacle_cost(i["X"], i["obs"]))),
                    dict(c=ALL, cx=ALL, cxx=ALL))
    for idx in np.ndindex(3, 17):  # the bars of test_obstacle_cost_kernel
        rc, rcx, rcxx = systems.obstacle_stage_cost(X[idx])
        assert abs(float(base["c"][idx]) - rc) <= 1e-14 * max(1.0, abs(rc))
        assert np.allclose(_np(base["cx"][idx]), rcx, rtol=1e-13, atol=1e-15)
        assert np.allclose(_np(base["cxx"][idx]), rcxx, rtol=1e-13, atol=1e-15)


# ---------------------------------------------------------------------------
# the row systems: spring chain, fleet, fleet with a proximity cost, team
# ---------------------------------------------------------------------------
ROW_N = 12
TRAJ_TOL = 1e-9  # tests/test_gpu_chain.py, test_gpu_fleet.py, test_gpu_team.py


def _row_system(kind, golden_dir):
    """(F, members(t) -> [(system id, slice)] or None, quiet factor per input, case data)"""
    if kind == "chain":
        from test_gpu_chain import _chain
        return _chain(12, 3), None, 1.0, None
    if kind == "fleet":
        import test_gpu_fleet as tf
        F = tf._fleet("quad2")
        return (F, lambda t: [(F.base_id, x) for x in tf._members(F, t)], 0.05,
                tf._case("quad2", golden_dir))
    if kind == "prox":
        import test_gpu_fleet as tf
        import test_gpu_fleet_proximity as tp
        c, d, F, plain = tp._case("pm3", golden_dir)
        return F, lambda t: [(F.base_id, x) for x in tf._members(plain, t)], 1.0, (c, d)
    import test_gpu_team as tt
    F = tt._team("pm_quad_di")
    return F, lambda t: tt._members(F, t), tt._quiet(F), tt._case("pm_quad_di", golden_dir)


def _head(F):
    from time_opt_ilqr_amd import _lib, engine
    name = "team" if engine.is_team(F) else "fleet" if engine.is_fleet(F) else "chain"
    par = engine._object_entry(F, "dynamics_f64")[1]
    return name, (_lib.C.byref(par),), par


@pytest.mark.parametrize("kind", ["chain", "fleet", "prox", "team"])
def test_row_system_dynamics_rollout_linearize(dev, golden_dir, kind):
    """hop_{chain,fleet,team}_dynamics_f64 (row strides larger than n and m), _rollout_f64
    (a shared x0: batch stride 0) and _linearize_f64 (steps < n_use of n_alloc, both
    differences).  A fleet with a proximity cost steps with the fleet's own entries."""
    import torch
    from time_opt_ilqr_amd import engine, host_dynamics
    F, members, quiet, _ = _row_system(kind, golden_dir)
    n, m, N, Bn = F.n, F.m, ROW_N, 5
    name, head, par = _head(F)
    _strided_dynamics(dev, f"{kind}-dynamics-strided", f"hop_{name}_dynamics_f64", head, n, m,
                      lambda x, u: F.batch(x, u))
    rng = np.random.default_rng(17 + n)
    x0 = rng.uniform(-0.5, 0.5, n)
    U = rng.uniform(-1.0, 1.0, (Bn, N, m)) * quiet
    base = run_case(dev, f"{kind}-rollout-shared-x0", dict(x0=_t(x0, dev), U=_t(U, dev)),
                    lambda i: dict(X=engine.rollout(F, i["x0"], i["U"], F.dt)), dict(X=ALL))
    Xr = base["X"]
    if members is None:  # the chain: the host rollout at tests/test_gpu_chain.py's ROLL_TOL
        ref = host_dynamics.rollout_batch(F.host(), np.stack([x0] * Bn), U)
        assert float(np.abs(_np(Xr) - ref).max()) <= 1e-12
    else:               # bitwise the members' own kernels
        ref = torch.cat([engine.rollout(s, x, u, F.dt) for (s, x), (_, u) in
                         zip(members(_t(np.stack([x0] * Bn), dev)), members(_t(U, dev)))], -1)
        assert bool(torch.isfinite(ref).all()) and torch.equal(Xr, ref)
    nu = N - 2
    X = _t(rng.uniform(-1.0, 1.0, (Bn, N + 1, n)), dev)
    Ut = _t(U, dev)
    for central in (False, True):
        def call(i):
            r = engine.linearize(F, i["X"], i["U"], F.dt, central=central, n_use=nu, want_fx=True)
            return dict(A=r.A, B=r.B, a_res=r.a_res, Fx=r.Fx)
        ext = dict(A=_steps(Bn, N, (n, n), nu), B=_steps(Bn, N, (n, m), nu),
                   a_res=_steps(Bn, N, (n,), nu), Fx=_steps(Bn, N, (n,), nu))
        base = run_case(dev, f"{kind}-linearize-central{int(central)}", dict(X=X, U=Ut), call, ext)
        A, B, ar, Fx = (base[key][:, :nu] for key in ("A", "B", "a_res", "Fx"))
        if members is None:
            from test_chain_cpu import check_lin
            ref = host_dynamics.linearize_batch(F.host(), _np(X)[:, :nu + 1], _np(Ut)[:, :nu],
                                                central=central)
            check_lin(12, 3, (_np(A), _np(B), _np(ar)), ref, f"arena central={central}")
            continue
        ox = ou = 0
        for (s, x), (_, u) in zip(members(X), members(Ut)):
            ref = engine.linearize(s, x, u, F.dt, central=central, n_use=nu, want_fx=True)
            sl, su = slice(ox, ox + x.shape[-1]), slice(ou, ou + u.shape[-1])
            assert torch.equal(A[..., sl, sl], ref.A[:, :nu]) and \
                torch.equal(B[..., sl, su], ref.B[:, :nu])
            assert torch.equal(ar[..., sl], ref.a_res[:, :nu]) and \
                torch.equal(Fx[..., sl], ref.Fx[:, :nu])
            ox, ou = ox + x.shape[-1], ou + u.shape[-1]
        assert ox == n and ou == m


def _row_cost_inputs(c, dev):
    out = {key: _t(c[key], dev) for key in ("xg", "u_ref", "Q", "R", "Qf")}
    out["w"] = _t(np.array([c["w"]]), dev)
    return out


@contextlib.contextmanager
def _proximity_table(F, dev):
    """call(i) puts the fleet's obstacle table where the engine caches it, so that the
    table the kernels read is the arena's copy; the cache entry is dropped afterwards"""
    from time_opt_ilqr_amd import engine
    prox = engine.fleet_proximity(F)
    if prox is None:
        yield {}, lambda i: None
        return
    cache = prox.__dict__.setdefault("_device_tables", {})
    before = cache.pop(str(dev), None)
    rows = prox.table(int(F.pos_dim))
    assert len(rows)

    def use(i):
        cache[str(dev)] = i["table"]
    try:
        yield dict(table=_t(np.asarray(rows.tolist()), dev)), use
    finally:
        cache.pop(str(dev), None)
        if before is not None:
            cache[str(dev)] = before


@pytest.mark.parametrize("kind", ["chain", "fleet", "prox", "team"])
def test_row_system_cost_and_linesearch(dev, golden_dir, kind):
    """hop_{chain,fleet,fleet_prox,team}_cost_true_f64 and _forward_linesearch_f64 (with
    their byte workspace) on the stored cases of each system's own test"""
    from time_opt_ilqr_amd import engine, host_dynamics
    F, members, quiet, case = _row_system(kind, golden_dir)
    if kind == "chain":
        from test_gpu_chain import _dense_cost, _linesearch_case as chain_ls
        rng = np.random.default_rng(123)
        xg, ur, Q, R, Qf, w = _dense_cost(12, 3, rng)
        c = dict(xg=xg, u_ref=ur, Q=Q, R=R, Qf=Qf, w=w, X=rng.uniform(-1, 1, (5, ROW_N + 1, F.n)),
                 U=rng.uniform(-1, 1, (5, ROW_N, F.m)), T=np.array([1, 4, 7, ROW_N, ROW_N]))
        cost_ref = np.array([host_dynamics.cost_true(c["X"][b], c["U"][b], xg, ur, Q, R, Qf, w,
                                                     int(c["T"][b])) for b in range(5)])
        ls = chain_ls()
        lxg, lur, lQ, lR, lQf, lw = ls["cost"]
        lc = dict(xg=lxg, u_ref=lur, Q=lQ, R=lR, Qf=lQf, w=lw)
        Xo, Uo, J, J0, acc = ls["ref"]
        ls = dict(X=ls["X"], U=ls["U"], K=ls["K"], k=ls["k"], T=ls["T"], active=ls["active"],
                  Xo=Xo, Uo=Uo, J=J, J0=J0, acc=acc)
        wrap = None
    else:
        c, d = case
        cost_ref = d["cost_J"][:5]
        pick = d["ls_pick"]
        lc = c
        ls = dict(X=d["ls_X"], U=c["U0"][pick], K=d["ls_K"], k=d["ls_k"], T=c["T0"][pick],
                  active=np.array([1, 1, 0, 1]), Xo=d["ls_Xo"], Uo=d["ls_Uo"], J=d["ls_J"],
                  J0=d["ls_J0"], acc=d["ls_acc"])
        wrap = F.wrap_idx
    with _proximity_table(F, dev) as (table, use_table):
        inputs = dict(X=_t(c["X"][:5], dev), U=_t(c["U"][:5], dev),
                      T=_t(np.asarray(c["T"][:5]), dev, "i32"), **_row_cost_inputs(c, dev), **table)

        def call(i):
            use_table(i)
            return dict(J=engine.cost_true(F, i["X"], i["U"], i["T"], _cost_params(i, wrap)))
        base = run_case(dev, f"{kind}-cost_true", inputs, call, dict(J=ALL))
        assert _elem_rel(_np(base["J"]), cost_ref) <= TRAJ_TOL

        inputs = dict(X=_t(ls["X"], dev), U=_t(ls["U"], dev), K=_t(ls["K"], dev),
                      k=_t(ls["k"], dev), T=_t(ls["T"], dev, "i32"),
                      active=_t(ls["active"], dev, "i32"), **_row_cost_inputs(lc, dev), **table)

        def call(i):
            use_table(i)
            r = engine.forward_linesearch(F, i["X"], i["U"], i["T"], i["K"], i["k"],
                                          _cost_params(i, wrap), F.dt, active=i["active"])
            return dict(X=r.X, U=r.U, J=r.J, J_old=r.J_old, accepted=r.accepted)
        base = run_case(dev, f"{kind}-linesearch", inputs, call,
                        dict(X=ALL, U=ALL, J=ALL, J_old=ALL, accepted=ALL))
    on = np.asarray(ls["active"]) != 0
    got = _np(base["accepted"])
    print(f"{kind} line search accepted {got.tolist()} reference {np.asarray(ls['acc']).tolist()}")
    assert got[on].tolist() == np.asarray(ls["acc"])[on].tolist() and (got[~on] == -2).all()
    eJ = _elem_rel(_np(base["J"])[on], ls["J"][on])
    eJ0 = _elem_rel(_np(base["J_old"])[on], ls["J0"][on])
    # absolute, and relative where an entry is large (the chain's overflow problem)
    sx = np.where(np.abs(ls["Xo"]) > 10.0, np.abs(ls["Xo"]), 1.0)
    su = np.where(np.abs(ls["Uo"]) > 10.0, np.abs(ls["Uo"]), 1.0)
    eX = float((np.abs(_np(base["X"]) - ls["Xo"]) / sx)[on].max())
    eU = float((np.abs(_np(base["U"]) - ls["Uo"]) / su)[on].max())
    assert max(eJ, eJ0, eX, eU) <= TRAJ_TOL, (eJ, eJ0, eX, eU)
    assert np.array_equal(_np(base["X"])[~on], ls["X"][~on])
    assert np.array_equal(_np(base["U"])[~on], ls["U"][~on])


def test_fleet_proximity_taylor(dev, golden_dir):
    """hop_fleet_proximity_taylor_f64 through the engine and with a row stride larger than n"""
    import torch
    import test_gpu_fleet_proximity as tp
    from time_opt_ilqr_amd import _lib, engine
    c, d, F, _ = tp._case("pm3", golden_dir)
    n = F.n
    X = _t(c["X"][:5, 0], dev)
    with _proximity_table(F, dev) as (table, use_table):
        def call(i):
            use_table(i)
            return dict(zip(("c", "cx", "cxx"), engine.fleet_proximity_cost(F, i["X"])))
        base = run_case(dev, "prox-taylor", dict(X=X, **table), call, dict(c=ALL, cx=ALL, cxx=ALL))
        for key in ("c", "cx", "cxx"):  # the bar of test_taylor_kernel_vs_reference
            assert tp._elem_rel(_np(base[key]), d["tay_" + key][:5]) <= TRAJ_TOL, key
        Xs = torch.full((5, n + 3), 1e300, dtype=torch.float64, device=dev)
        Xs[:, :n] = X

        def direct(i):
            use_table(i)
            t_ = engine._torch()
            out = [t_.empty(s, dtype=torch.float64, device=dev) for s in ((5,), (5, n), (5, n, n))]
            px, tab = engine._proximity_struct(F, dev)
            _lib.check(_lib.load().hop_fleet_proximity_taylor_f64(
                _lib.C.byref(engine._fleet_params(F)), _lib.C.byref(px), _lib.ptr(i["X"]), n + 3, 5,
                *[_lib.ptr(o) for o in out], _lib.stream_handle(dev)))
            return dict(zip(("c", "cx", "cxx"), out))
        strided = run_case(dev, "prox-taylor-strided", dict(X=Xs, **table), direct,
                           dict(c=ALL, cx=ALL, cxx=ALL))
    for key in ("c", "cx", "cxx"):
        assert torch.equal(_bits(strided[key]), _bits(base[key])), key


# ---------------------------------------------------------------------------
# the one-pass window method's primitives on the stored double-integrator cases
# ---------------------------------------------------------------------------
def _onepass_cost_inputs(p, dev):
    d = p["d"]
    out = {key: _t(d[key], dev) for key in ("xg", "u_ref", "Q", "R", "Qf")}
    out["w"] = _t(np.array([float(d["w"])]), dev)
    return out


def test_onepass_nominal_curve(dev, golden_dir):
    """hop_onepass_nominal_curve_f64: J [B][T_max] (+inf before T_min) and T_bar"""
    import os
    from test_gpu_onepass import _problem
    from time_opt_ilqr_amd import engine
    p = _problem("di", golden_dir)
    d = np.load(os.path.join(golden_dir, "onepass_curve_cases.npz"))
    X = np.stack([p["d"]["X"]] * 2)
    X[1, p["T_max"] - 2:] = np.nan
    U = np.stack([p["d"]["U"]] * 2)
    inputs = dict(X=_t(X, dev), U=_t(U, dev), **_onepass_cost_inputs(p, dev))

    def call(i):
        J, Tb = engine.nominal_cost_curve(p["F"].system_id, i["X"], i["U"],
                                          _cost_params(i, p["wrap_idx"]), p["T_min"], p["T_max"])
        return dict(J=J, T_bar=Tb)
    base = run_case(dev, "onepass-curve", inputs, call, dict(J=ALL, T_bar=ALL))
    J, T_bar = _np(base["J"]), _np(base["T_bar"])
    for b, name in enumerate(("normal", "nan_tail")):  # the bars of test_nominal_curve_vs_reference
        Jr, Tr = d[f"di_{name}_J"], int(d[f"di_{name}_Tbar"])
        assert np.array_equal(np.isinf(J[b]), np.isinf(Jr)) and not np.isnan(J[b]).any()
        fin = np.isfinite(Jr)
        err = float(np.max(np.abs(J[b][fin] - Jr[fin]) / np.abs(Jr[fin]))) if fin.any() else 0.0
        assert err <= 1e-12 and int(T_bar[b]) == Tr


def test_onepass_extend_backward(dev, golden_dir):
    """hop_onepass_extend_backward_f64: X_ext and U_ext, prefix and copied tail"""
    import os
    from test_gpu_onepass import _problem
    from time_opt_ilqr_amd import engine
    p = _problem("di", golden_dir)
    F = p["F"]
    d = np.load(os.path.join(golden_dir, "onepass_prefix_cases.npz"))
    keys = [f"di_{name}_S4" for name in ("generic", "fixed", "overflow")]
    X, U = np.stack([d[k + "_X"] for k in keys]), np.stack([d[k + "_U"] for k in keys])
    inputs = dict(X=_t(X, dev), U=_t(U, dev), u_fill=_t(U[:, 0], dev))

    def call(i):
        Xe, Ue = engine.extend_nominal_backward(F.system_id, i["X"], i["U"], i["u_fill"], F.dt, 4,
                                                max_iter=4, damping=0.5)
        return dict(X_ext=Xe, U_ext=Ue)
    base = run_case(dev, "onepass-extend", inputs, call, dict(X_ext=ALL, U_ext=ALL))
    for b, k in enumerate(keys):  # the double integrator has no libm call: bitwise
        assert np.array_equal(_np(base["X_ext"][b]), d[k + "_Xe"], equal_nan=True), k
        assert np.array_equal(_np(base["U_ext"][b]), d[k + "_Ue"], equal_nan=True), k


def test_onepass_pick(dev, golden_dir):
    """hop_onepass_pick_f64: three stored n = 2 cases as one batch with per-problem T_bar;
    Jw [B][T_max] is written everywhere (NaN where not evaluated)"""
    import os
    from test_gpu_onepass import _check_pick
    from time_opt_ilqr_amd import engine
    d = np.load(os.path.join(golden_dir, "onepass_pick_cases.npz"))
    names = [str(s) for s in d["names"]]
    idx = [names.index(s) for s in ("n2_plain", "n2_cut_left", "n2_cut_right")]
    par = np.array([d[f"c{i}_par"] for i in idx])
    assert (par[:, [0, 1, 3, 4, 5, 6]] == par[0, [0, 1, 3, 4, 5, 6]]).all()
    n, L, _, T_min, T_max, S_left, S_right = (int(v) for v in par[0])
    inputs = {k: _t(np.stack([d[f"c{i}_{k}"] for i in idx]), dev)
              for k in ("Vxx", "Vx", "V0", "X_ext", "x0")}
    inputs["T_bar"] = _t(par[:, 2], dev, "i32")
    wrap = [int(j) for j in d[f"c{idx[0]}_wrap"]]

    def call(i):
        T, Jw = engine.onepass_pick(i["Vxx"], i["Vx"], i["V0"], i["X_ext"], i["x0"], i["T_bar"],
                                    T_min, T_max, S_left, S_right, wrap_idx=wrap)
        return dict(T_star=T, Jw=Jw)
    base = run_case(dev, "onepass-pick", inputs, call, dict(T_star=ALL, Jw=ALL))
    for b, i in enumerate(idx):
        _check_pick(names[i], int(base["T_star"][b]), _np(base["Jw"][b]), int(d[f"c{i}_T"]),
                    d[f"c{i}_Jw"])


def test_onepass_rollout(dev, golden_dir):
    """hop_onepass_rollout_f64 with its byte workspace: the stored centre, right and
    all-fail cases and an inactive problem as one batch"""
    import os
    from test_gpu_onepass import _problem
    from time_opt_ilqr_amd import engine
    p = _problem("di", golden_dir)
    F, N = p["F"], p["N"]
    d = np.load(os.path.join(golden_dir, "onepass_rollout_cases.npz"))
    X_ext, U_ext = d["di_X_ext"], d["di_U_ext"]
    n, m = X_ext.shape[1], U_ext.shape[1]
    keys = ["di_center", "di_right", "di_all_fail", "di_center"]
    Tb, Ts, S = (np.array([int(d[k + "_T"][j]) for k in keys]) for j in range(3))
    S = int(S[0])
    assert all(int(d[k + "_T"][2]) == S for k in keys)
    al = [float(a) for a in d["di_center_alphas"]]
    assert all([float(a) for a in d[k + "_alphas"]] == al for k in keys)
    K, k = np.zeros((4, S + N, m, n)), np.zeros((4, S + N, m))
    for b, key in enumerate(keys):
        K[b, :Tb[b] + S], k[b, :Tb[b] + S] = d[key + "_K"], d[key + "_k"].reshape(Tb[b] + S, m)
    active = np.array([1, 1, 1, 0], dtype=np.int32)
    inputs = dict(X_ext=_t(np.stack([X_ext] * 4), dev), U_ext=_t(np.stack([U_ext] * 4), dev),
                  K=_t(K, dev), k=_t(k, dev), T_bar=_t(Tb, dev, "i32"), T_star=_t(Ts, dev, "i32"),
                  active=_t(active, dev, "i32"), **_onepass_cost_inputs(p, dev))

    def call(i):
        r = engine.onepass_rollout(F.system_id, i["X_ext"], i["U_ext"], i["K"], i["k"],
                                   _cost_params(i, p["wrap_idx"]), F.dt, i["T_bar"], i["T_star"], S,
                                   alphas=al, active=i["active"])
        return dict(X=r.X, U=r.U, J=r.J, accepted=r.accepted)
    base = run_case(dev, "onepass-rollout", inputs, call, dict(X=ALL, U=ALL, J=ALL, accepted=ALL))
    acc = _np(base["accepted"])
    print("onepass rollout accepted", acc.tolist())
    for b, key in enumerate(keys[:3]):  # the bars of test_rollout_cases_vs_reference
        ok = bool(d[key + "_ok"])
        assert (acc[b] >= 0) == ok, key
        if not ok:
            assert acc[b] == -1 and float(base["J"][b]) == np.inf
            assert np.array_equal(_np(base["X"][b]), X_ext[S:])
            continue
        Jr = float(d[key + "_J"])
        assert abs(float(base["J"][b]) - Jr) <= 1e-9 * abs(Jr), key
        assert _rel(_np(base["X"][b]), d[key + "_Xn"]) <= 1e-9, key
        assert _rel(_np(base["U"][b]), d[key + "_Un"]) <= 1e-9, key
    assert acc[3] == -2 and np.array_equal(_np(base["X"][3]), X_ext[S:])
    assert np.array_equal(_np(base["U"][3]), U_ext[S:])


# ---------------------------------------------------------------------------
# batch-size switches: one case on each side of every dispatch that reads the batch size
# ---------------------------------------------------------------------------
def _cus(dev):
    import torch
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


@pytest.mark.parametrize("side", [0, 1])
def test_switch_conditioned_sweep_packed_layout(dev, side):
    """lft_sweep_v2.hip dispatch: more than 4 waves of 4 problems per compute unit (4,096
    problems on 256 compute units) takes the packed-image layout.  n_alloc = n_use = 1, the
    smallest the entry accepts; 128 distinct problems repeated"""
    Bn = 16 * _cus(dev) + side * 3  # a tail of 3 in the last wave
    A, Bm, Q, R, Ri, z0, QT = _lft(7500, 128, 13, 4, 1)
    idx = np.arange(Bn) % 128
    base = _sweep(dev, f"s13-cond-B{Bn}", A[idx], Bm[idx], Q[idx], Ri[idx], z0[0], QT[idx],
                  n_use=1, t_min=1, capacity=96 << 20)
    chk = np.array([0, 1, 127, Bn // 2 - 1, Bn // 2, Bn - 5, Bn - 4, Bn - 3, Bn - 2, Bn - 1])
    J, st = _np(base["J"]), _np(base["status"])
    Jo, sto = orc.lft_sweep_batch(A[idx[chk]], Bm[idx[chk]], Q[idx[chk]], Ri[idx[chk]], z0[0],
                                  QT[idx[chk]], 1)
    assert (st == 0).all() and (sto == 0).all()
    assert _elem_rel(J[chk], Jo) <= TOL["f64"]
    assert np.array_equal(J, J[:128][idx])  # every copy of a problem: the same bits


@pytest.mark.parametrize("side", [0, 1])
def test_switch_small_sweep_row_group(dev, side):
    """hop_kernels.hpp kSmallRowGroupMax = 16,384: fp64 s <= 5 blocks up to it run the
    row-group kernel, above it one problem per lane.  n_alloc = n_use = 1"""
    Bn = 16384 + side
    A, Bm, Q, R, Ri, z0, QT = _lft(7600, 128, 5, 2, 1)
    idx = np.arange(Bn) % 128
    base = _sweep(dev, f"s5-B{Bn}", A[idx], Bm[idx], Q[idx], Ri[idx], z0[0], QT[idx], n_use=1,
                  t_min=1, capacity=64 << 20)
    J = _np(base["J"])
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0[0], QT, 1)
    assert (_np(base["status"]) == 0).all() and (sto == 0).all()
    assert _elem_rel(J[:128], Jo) <= TOL["f64"]
    assert _elem_rel(J[-128:], Jo[idx[-128:]]) <= TOL["f64"]
    assert np.array_equal(J, J[:128][idx])


@pytest.mark.parametrize("side", [0, 1])
def test_switch_riccati_two_waves_per_simd(dev, side):
    """riccati_fast.hip launch: mode 0 without the V outputs and with a batch-shared Q runs
    two waves per SIMD above 4 waves of 4 problems per compute unit.  n_alloc = 2"""
    from gain_check import assert_per_step
    from time_opt_ilqr_amd import engine
    Bn, N, n, m = 16 * _cus(dev) + side * 3, 2, 12, 4
    P = _ric(n, m, N)
    A, B, X, U, xg, ur, Q, R, Qf, alpha = P
    idx = np.arange(Bn) % RB
    T = (np.arange(Bn) // RB % 2 + 1).astype(np.int32)  # horizons 1 and 2
    names = ("A", "B", "X", "U", "xg", "u_ref", "Q", "R", "Qf")
    inputs = {k: _t(x[idx], dev) for k, x in zip(names, P[:9])}
    inputs.update(Q=_t(Q[0], dev), horizon=_t(T, dev, "i32"), lm=_t(np.full(Bn, 1e-3), dev))

    def call(i):
        r = engine.riccati(*(i[k] for k in names), i["horizon"], i["lm"], mode=0, wrap_idx=[1])
        return dict(K=r.K, k=r.k, status=r.status)
    ext = dict(K=_steps_mask((Bn, N, m, n), T), k=_steps_mask((Bn, N, m), T), status=ALL)
    base = run_case(dev, f"riccati-mode0-B{Bn}", inputs, call, ext, capacity=96 << 20)
    assert (_np(base["status"]) == 0).all()
    for b in (0, 1, 4, 5, 9, Bn - 4, Bn - 3, Bn - 2, Bn - 1):
        i, Tb = idx[b], int(T[b])
        ks, Ks, ok = orc.riccati_truncated(list(A[i]), list(B[i]), X[i], U[i], xg[i], ur[i], Q[0],
                                           R[i], alpha[i], Tb, lm_lambda=1e-3, wrap_idx=[1])
        assert ok
        assert_per_step(_np(base["K"][b, :Tb]), np.array(Ks), 1e-6, f"{b} K")
        assert_per_step(_np(base["k"][b, :Tb]), np.array(ks), 1e-6, f"{b} k")


@pytest.mark.parametrize("side", [0, 1])
def test_switch_quadrotor_linesearch_lanes(dev, golden_dir, side):
    """forward.hip: the quadrotor line search runs two lanes per rollout while the launch
    (2 * n_alpha + 1 lanes per problem) fits 4 waves per compute unit, one lane beyond"""
    import torch
    cap = 4 * _cus(dev) * 64          # lanes of 4 waves per compute unit
    Bn = cap // 11 + side             # the largest batch with ceil(11 B / 64) waves <= cap / 64
    assert (11 * Bn + 63) // 64 <= cap // 64 if side == 0 else (11 * Bn + 63) // 64 > cap // 64
    sid, dt, X, U, K, k, T, active, c, wrap = _quadrotor_linesearch_inputs(golden_dir, 7)
    N = 3  # the first steps of the captured trajectory: every kernel path, small tensors
    idx = np.arange(Bn) % 7
    X, U, K, k = X[idx, :N + 1], U[idx, :N], K[idx, :N], k[idx, :N]
    T, active = np.minimum(T, N).astype(np.int32)[idx], active[idx]
    base = _linesearch_case(dev, f"linesearch-quadrotor-B{Bn}", sid, dt, X, U, K, k, T, active, c,
                            wrap, capacity=160 << 20)
    sl = np.r_[0:7, Bn - 7:Bn]
    _check_linesearch({key: v[sl] for key, v in base.items()}, sid, dt, X[sl], U[sl], K[sl], k[sl],
                      T[sl], active[sl], c, wrap)
    for key in ("X", "U", "J", "accepted"):  # every copy of a problem: the same bits
        first = base[key][:7]
        rep = first.repeat((Bn + 6) // 7, *([1] * (first.dim() - 1)))[:Bn]
        assert torch.equal(_bits(base[key]), _bits(rep)), key


# ---------------------------------------------------------------------------
# the outer loop's bookkeeping: the only entries with in/out arguments
# ---------------------------------------------------------------------------
def test_ilqr_accept_and_select_mask(dev):
    """hop_ilqr_accept_f64 (lm, T_bar, J_hist, T_hist, n_hist, done are in/out; J, accepted
    and T_star are inputs) and hop_ilqr_select_mask (done, crashed in/out; active out)
    against the rule include/hop.h states, problem by problem"""
    from types import SimpleNamespace
    from time_opt_ilqr_amd import engine
    Bn, H = 7, 4
    J = np.array([2.0, np.nan, 3.0, 1.0, 1.00001, 5.0, 4.0])
    acc = np.array([0, 1, -1, 2, 0, 0, 3], dtype=np.int32)
    T = np.array([5, 6, 7, 8, 9, 3, 4], dtype=np.int32)
    lm = np.array([1e-3, 1e-3, 1e-3, 1e-12, 1e-2, 1e-3, 1e-3])
    T_bar = np.full(Bn, 2, dtype=np.int32)
    n_hist = np.array([0, 1, 1, 2, 2, 1, H], dtype=np.int32)
    J_hist = np.tile(np.array([1.0, 1.00001, 0.0, 0.0]), (Bn, 1))
    T_hist = np.tile(np.array([9, 9, 0, 0], dtype=np.int32), (Bn, 1))
    done = np.array([0, 0, 0, 0, 0, 1, 0], dtype=np.int32)
    state = ("lm", "T_bar", "J_hist", "T_hist", "n_hist", "done")
    inputs = dict(J=_t(J, dev), accepted=_t(acc, dev, "i32"), T_star=_t(T, dev, "i32"),
                  lm=_t(lm, dev), T_bar=_t(T_bar, dev, "i32"), J_hist=_t(J_hist, dev),
                  T_hist=_t(T_hist, dev, "i32"), n_hist=_t(n_hist, dev, "i32"),
                  done=_t(done, dev, "i32"))

    def call(i):
        engine.ilqr_accept(SimpleNamespace(**{k: i[k] for k in state}), i["J"], i["accepted"],
                           i["T_star"])
        return {k: i[k] for k in state}
    base = run_case(dev, "ilqr_accept", inputs, call, {k: ALL for k in state}, inout=state)
    for b in range(Bn):
        nh, l, tb, dn = int(n_hist[b]), lm[b], int(T_bar[b]), int(done[b])
        Jh, Th = J_hist[b].copy(), T_hist[b].copy()
        if not dn:
            if acc[b] >= 0 and np.isfinite(J[b]) and nh < H:
                tb, Jh[nh], Th[nh], nh = int(T[b]), J[b], T[b], nh + 1
                l = max(l / 10.0, 1e-12)
            else:
                l = l * 10.0
            if nh >= 3 and abs(Jh[nh - 1] - Jh[nh - 2]) / (abs(Jh[nh - 2]) + 1e-12) < 1e-4 \
                    and Th[nh - 1] == Th[nh - 2] == Th[nh - 3]:
                dn = 1
        got = (float(base["lm"][b]), int(base["T_bar"][b]), int(base["n_hist"][b]),
               int(base["done"][b]))
        assert got == (l, tb, nh, dn), (b, got, (l, tb, nh, dn))
        assert np.array_equal(_np(base["J_hist"][b]), Jh)
        assert np.array_equal(_np(base["T_hist"][b]), Th)
    assert _np(base["done"]).tolist() == [0, 0, 0, 0, 1, 1, 0]

    sel = np.array([0, orc.ST_FAIL, orc.ST_NONFINITE, orc.ST_JITTER, 0, orc.ST_FAIL, 0],
                   dtype=np.int32)
    ric = np.array([0, 0, 0, 0, orc.ST_FAIL, 0, orc.ST_JITTER], dtype=np.int32)
    inputs = dict(sel=_t(sel, dev, "i32"), ric=_t(ric, dev, "i32"), done=_t(done, dev, "i32"),
                  crashed=_t(np.zeros(Bn), dev, "i32"))

    def call(i):
        st = SimpleNamespace(done=i["done"], crashed=i["crashed"])
        return dict(active=engine.ilqr_select_mask(st, i["sel"], i["ric"]), done=i["done"],
                    crashed=i["crashed"])
    base = run_case(dev, "ilqr_select_mask", inputs, call, dict(active=ALL, done=ALL, crashed=ALL),
                    inout=("done", "crashed"))
    assert _np(base["crashed"]).tolist() == [0, 1, 1, 0, 0, 0, 0]
    assert _np(base["done"]).tolist() == [0, 1, 1, 0, 0, 1, 0]
    assert _np(base["active"]).tolist() == [1, 0, 0, 1, 0, 0, 1]
