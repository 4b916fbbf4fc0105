"""General, per-problem z0 and per-step R on every sweep kernel.

propagator_all_Jt_aug evaluates J = 1/2 z0^T P0 z0 for whatever z0 it is handed
(the reference's horizon_selection.py:85); the builders only ever produce e_s
(augmented.py:57), and with z0 = e_s the query reads one entry of P0.  Here every
kernel family runs with a z0 of its own per problem (orc.synth_z0: e_s, dense,
[0.3 d; 1], [d; 0], 1e3 d, 1e-3 d, 0, e_0), reached by the option include/hop.h names
for it, and is held to

  * the oracle: J elementwise relative 1e-9 (fp64) / 2e-3 (fp32), the all-zero rows
    exactly 0.0, the status word equal;
  * T* on a batch whose minimising horizon moves with z0 (orc.synth_tstar_batch);
  * three invariants that need no reference: (a) a shared z0 as [s], [1, s] and
    [Bn, s] of equal rows gives the same bits (stride 0 against stride s); (b)
    permuting the problems with their z0 rows permutes J bitwise; (c) doubling one
    problem's z0 multiplies its J by exactly 4 and changes no other row;
  * a non-finite z0: that problem all NaN, ST_NONFINITE, T* = t_min, every other
    problem bitwise untouched.

The per-step control weight (r_step_stride; horizon_selection.py:52 inverts R_list[k]
per step) gets the same treatment at the end of the file: distinct R per (problem,
step), shared and per-problem strides, R^-1 and raw R.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-9, "f32": 2e-3}
N0 = 12          # stages of every case that has no reason for another count
T_MIN = 3        # the fused argmin's window [T_MIN, N]


def _tdt(dtype):
    import torch
    return torch.float64 if dtype == "f64" else torch.float32


def _t(x, dev, dtype="f64"):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), dtype=_tdt(dtype), device=dev)


def _np(t):
    return t.double().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _blocks(seed, Bn, s, m, N, tstar=False):
    """(A, Bm, Q, Ri [Bn, m, m], QT[, z0]) of Bn clean problems, made once."""
    if tstar:
        A, Bm, Q, R, Ri, z0, QT = orc.synth_tstar_batch(seed, Bn, s, m, N)
        return A, Bm, Q, Ri, QT, z0
    A, Bm, Q, R, Ri, z0, QT = orc.synth_lft_batch(seed, Bn, s, m, N)
    return A, Bm, Q, Ri, QT


class Path:
    """One product kernel path: the shape, batch and option that reach it."""

    def __init__(self, name, s, m, Bn, N=N0, dtype="f64", opts=None, tile=False, capi_wide=False,
                 dbg=False, rep=0):
        self.name, self.s, self.m, self.Bn, self.N = name, s, m, Bn, N
        self.dtype, self.opts, self.tile, self.capi_wide = dtype, opts or {}, tile, capi_wide
        self.dbg = dbg
        self.rep = rep  # > 0: the batch repeats `rep` base problems (the 4,100-problem case)
        self.seed = 3100 + 17 * s + m

    def __repr__(self):
        return self.name

    # -- data ---------------------------------------------------------------
    def base(self, tstar=False):
        nb = self.rep or self.Bn
        return _blocks(self.seed + (500 if tstar else 0), nb, self.s, self.m, self.N, tstar)

    def index(self):
        """base problem of every batch slot"""
        return np.arange(self.Bn) % (self.rep or self.Bn)

    def checked(self):
        """the batch slots compared with the oracle"""
        if not self.rep:
            return np.arange(self.Bn)
        edge = [2047, 2048, 4000, 4095, 4096, 4097, 4098, 4099]
        return np.array(list(range(self.rep - len(edge))) + edge)

    def tensors(self, dev, tstar=False, perm=None):
        blk = self.base(tstar)[:5]
        idx = self.index() if perm is None else self.index()[perm]
        return tuple(_t(x[idx], dev, self.dtype) for x in blk)

    def z0(self, zseed=41):
        return orc.synth_z0(orc.Z0_KINDS, self.Bn, self.s, zseed)

    def oracle(self, z0):
        """(J, status) of the checked slots for the [Bn, s] rows z0"""
        A, Bm, Q, Ri, QT = self.base()
        idx, chk = self.index(), self.checked()
        return orc.lft_sweep_batch(A[idx[chk]], Bm[idx[chk]], Q[idx[chk]], Ri[idx[chk]], z0[chk],
                                   QT[idx[chk]])

    # -- launch -------------------------------------------------------------
    def run(self, T, z0, dev, R=None, r_is_inverse=True, n_use=None, t_min=None, t_max=None):
        import torch
        from time_opt_ilqr_amd import _lib, engine
        A, Bm, Q, Ri, QT = T
        z = z0 if isinstance(z0, torch.Tensor) else _t(z0, dev, self.dtype)
        R = Ri if R is None else R
        n_eff = self.N if n_use is None else n_use
        t_max = n_eff if t_max is None else t_max
        t_min = min(T_MIN, t_max) if t_min is None else t_min
        if self.capi_wide:
            return _wide_capi(dev, A, Bm, Q, R, z, QT, n_eff, t_min, t_max)
        if self.tile:
            A, Bm, Q, QT = (engine.to_tile64(x) for x in (A, Bm, Q, QT))
        kw = dict(return_efg=True, return_prefix=True) if self.dbg else {}
        with _lib.options(**self.opts):
            res = engine.propagate(A, Bm, Q, R, z, QT, n_use=n_use, r_is_inverse=r_is_inverse,
                                   t_min=t_min, t_max=t_max, **kw)
        torch.cuda.synchronize()
        return res


def _wide_capi(dev, A, Bm, Q, R, z, QT, n_use, t_min, t_max):
    """hop_lft_sweep_wide_f64 itself (the engine gives s <= 16 to the narrow kernels)
    with the strides engine.propagate would pass."""
    import torch
    from time_opt_ilqr_amd import _lib
    Bn, N, s, _ = A.shape
    m = Bm.shape[-1]
    J = torch.empty((Bn, n_use), dtype=torch.float64, device=dev)
    st = torch.empty((Bn,), dtype=torch.int32, device=dev)
    ts = torch.empty((Bn,), dtype=torch.int32, device=dev)
    js = torch.empty((Bn,), dtype=torch.float64, device=dev)
    if R.dim() == 4:
        r_bs, r_ks = (0 if R.shape[0] == 1 else R.shape[1] * m * m), m * m
    else:
        r_bs, r_ks = (0 if R.dim() == 2 or R.shape[0] == 1 else m * m), 0
    z_bs = 0 if z.dim() == 1 or z.shape[0] == 1 else s
    assert z.shape[-1] == s and (z_bs == 0 or z.shape[0] == Bn) and z.is_contiguous()
    _lib.check(_lib.load().hop_lft_sweep_wide_f64(
        _lib.ptr(A), _lib.ptr(Bm), _lib.ptr(Q), _lib.ptr(R), r_bs, r_ks, 1, _lib.ptr(QT),
        _lib.ptr(z), z_bs, Bn, N, n_use, s, m, 8, t_min, t_max, _lib.ptr(J), _lib.ptr(st),
        _lib.ptr(ts), _lib.ptr(js), None, None, _lib.stream_handle(dev)))
    torch.cuda.synchronize()
    return SimpleNamespace(J=J, status=st, t_star=ts, j_star=js, efg=None, prefix=None)


SMALL = [(5, 2), (5, 1), (4, 2), (3, 1), (2, 1)]


def _all_paths():
    P = [Path("s13-cond", 13, 4, 37),
         Path("s13-cond-packed", 13, 4, 4100, N=4, rep=128),
         Path("s13-refassoc", 13, 4, 37, opts=dict(reference_assoc=True)),
         Path("s13-forced-pipe", 13, 4, 4, opts=dict(force_handover=True)),
         Path("s13-forced-body", 13, 4, 19, opts=dict(force_handover=True)),
         Path("s13-f32-cond", 13, 4, 37, dtype="f32"),
         Path("s13-f32-forced", 13, 4, 37, dtype="f32", opts=dict(force_handover=True)),
         Path("generic-s13", 13, 4, 9, opts=dict(force_generic=True)),
         Path("generic-s6", 6, 2, 9, dbg=True),
         Path("generic-s7", 7, 3, 9, dbg=True),
         Path("generic-s16", 16, 6, 9, dbg=True)]
    for s, m in SMALL:
        tag = f"s{s}m{m}"
        P += [Path(f"{tag}-rowgroup", s, m, 70),
              Path(f"{tag}-lane", s, m, 70, opts=dict(small_lane=True)),
              Path(f"{tag}-refassoc", s, m, 70, opts=dict(reference_assoc=True)),
              Path(f"{tag}-forced", s, m, 70, opts=dict(force_handover=True)),
              Path(f"{tag}-f32-lane", s, m, 70, dtype="f32"),
              Path(f"{tag}-f32-tile64", s, m, 70, dtype="f32", tile=True),
              Path(f"{tag}-tile64", s, m, 70, tile=True)]
    P += [Path("wide-s17", 17, 4, 5), Path("wide-s24", 24, 6, 5), Path("wide-s32", 32, 8, 5),
          Path("wide-s16-capi", 16, 6, 5, capi_wide=True)]
    return P


PATHS = _all_paths()
BY_NAME = {p.name: p for p in PATHS}
NONFINITE = [p for p in PATHS if p.name in ("s13-cond", "s13-refassoc")
             or p.name.startswith(("generic", "wide")) or (p.s <= 5 and "forced" not in p.name)]


def _elem_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _bitwise(a, b, what, rows=None):
    import torch
    sel = (lambda x: x) if rows is None else (lambda x: x[rows])  # noqa: E731
    nn = lambda x: sel(x).nan_to_num(7.0)  # noqa: E731
    assert torch.equal(nn(a.J), nn(b.J)), (what, "J", float((nn(a.J) - nn(b.J)).abs().max()))
    assert torch.equal(sel(a.status), sel(b.status)), (what, "status")
    assert torch.equal(sel(a.t_star), sel(b.t_star)), (what, "t_star")
    assert torch.equal(nn(a.j_star), nn(b.j_star)), (what, "j_star")


def _vs_oracle(path, res, z0, tag):
    """J of the checked slots against the oracle, each problem elementwise; the zero
    rows exactly 0.0; the status word the oracle's.  Returns the largest error."""
    Jo, sto = path.oracle(z0)
    chk = path.checked()
    J, st = _np(res.J)[chk], res.status.cpu().numpy()[chk]
    assert (sto == 0).all()
    worst = 0.0
    for i, b in enumerate(chk):
        if not z0[b].any():
            assert (Jo[i] == 0.0).all() and (J[i] == 0.0).all(), (tag, int(b), J[i])
            continue
        worst = max(worst, _elem_rel(J[i], Jo[i]))
    print(f"[z0] {path.name} {tag}: max elementwise rel J error {worst:.3e}")
    assert worst <= TOL[path.dtype], (tag, worst)
    assert np.array_equal(st, sto), (tag, st[st != sto][:8])
    return Jo


@pytest.mark.parametrize("path", PATHS, ids=repr)
def test_every_z0_kind_against_the_oracle(dev, path):
    """Row b of the batch carries z0 kind b % 8.  J, status and the fused argmin (T*
    the first minimiser of the device's own curve, J* that entry)."""
    T = path.tensors(dev)
    z0 = path.z0()
    res = path.run(T, z0, dev)
    Jo = _vs_oracle(path, res, z0, "kinds")
    J = _np(res.J)
    lo = min(T_MIN, path.N)
    Td, Jd = orc.select_horizon(J, lo, path.N)
    assert res.t_star.cpu().numpy().tolist() == Td.tolist()
    assert np.array_equal(_np(res.j_star), Jd)
    if path.dbg:  # the stage blocks and the prefix do not involve z0: the oracle's, 1e-9
        A, Bm, Q, Ri, QT = path.base()
        efg, pre = _np(res.efg), _np(res.prefix)
        for b in (0, path.Bn - 1):
            o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b], want_efg=True,
                              want_prefix=True)
            for i, key in enumerate(("E", "F", "G")):
                assert np.abs(efg[b, :, i] - o[key]).max() <= 1e-9 * np.abs(o[key]).max()
            for i, key in enumerate(("Ebar", "Fbar", "Gbar")):
                assert np.abs(pre[b, :, i] - o[key]).max() <= 1e-9 * np.abs(o[key]).max()
    assert Jo.shape[0] == len(path.checked())


@pytest.mark.parametrize("path", PATHS, ids=repr)
def test_tstar_moves_with_z0(dev, path):
    """z0 = [c delta; 1] with c cycling over 0, 1, 3, 10 and QT scaled by 50: the
    oracle's T* moves across the window with c, no window is within 1e-6 (relative) of
    a tie, every status is 0, and the kernel's fused argmin is the oracle's.  fp32
    resolves a gap only above its 2e-3 J bar: where the oracle's gap is under twice
    that, the horizon picked must be within twice the bar of the oracle's minimum."""
    blk = path.base(tstar=True)
    A, Bm, Q, Ri, QT, z0b = blk
    idx = path.index()
    lo = min(2, path.N)
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0b, QT)
    assert (sto == 0).all()
    gap = orc.argmin_gap(Jo, lo, path.N) if path.N > lo else np.ones(len(Jo))
    assert gap.min() >= 1e-6, gap.min()
    To, Jso = orc.select_horizon(Jo, lo, path.N)
    assert len(set(To.tolist())) >= 2, To  # T* is not a constant of the batch
    res = path.run(path.tensors(dev, tstar=True), z0b[idx], dev, t_min=lo)
    ts, js, J = res.t_star.cpu().numpy(), _np(res.j_star), _np(res.J)
    assert (res.status.cpu().numpy() == 0).all()
    err = _elem_rel(J, Jo[idx])
    by_c = [_elem_rel(J[c::4], Jo[idx][c::4]) for c in range(4)]  # c = 0 is z0 = e_s
    print(f"[z0] {path.name} tstar: max elementwise rel J error {err:.3e} (c = 0, 1, 3, 10: "
          f"{', '.join(f'{e:.1e}' for e in by_c)}), oracle T* {sorted(set(To.tolist()))}, "
          f"smallest gap {gap.min():.2e}")
    assert err <= TOL[path.dtype]
    if path.dtype == "f64":
        assert ts.tolist() == To[idx].tolist()
    else:
        for b in range(path.Bn):
            if gap[idx[b]] >= 2 * TOL["f32"]:
                assert ts[b] == To[idx[b]], b
            assert Jo[idx[b], ts[b] - 1] <= Jso[idx[b]] * (1 + 2 * TOL["f32"]), b
    assert _elem_rel(js, Jo[idx, ts - 1]) <= TOL[path.dtype]
    assert np.array_equal(js, J[np.arange(path.Bn), ts - 1])


@pytest.mark.parametrize("path", PATHS, ids=repr)
def test_z0_invariants_stride_permutation_scaling(dev, path):
    import torch
    T = path.tensors(dev)
    Bn, s = path.Bn, path.s
    z0 = path.z0()
    # (a) one z0 for every problem: [s], [1, s], and [Bn, s] of equal rows
    zs = orc.synth_z0(("offset",), 1, s, 43)[0]
    r1 = path.run(T, zs, dev)
    _bitwise(path.run(T, zs[None], dev), r1, "[1, s] against [s]")
    _bitwise(path.run(T, np.tile(zs, (Bn, 1)), dev), r1, "[Bn, s] of equal rows against [s]")
    # (b) the problems and their z0 rows permuted together
    base = path.run(T, z0, dev)
    perm = np.random.default_rng(7).permutation(Bn)
    pt = torch.as_tensor(perm, device=dev)
    rp = path.run(path.tensors(dev, perm=perm), z0[perm], dev)
    back = SimpleNamespace(J=base.J[pt], status=base.status[pt], t_star=base.t_star[pt],
                           j_star=base.j_star[pt])
    _bitwise(rp, back, "permutation")
    # (c) 2 z0 -> 4 J, bit for bit (a power of two commutes with every operation the
    # query performs on z0), on a problem of the first wave and on the last problem;
    # no other row moves
    rows = [1, Bn - 1]
    z2 = z0.copy()
    z2[rows] *= 2.0
    r2 = path.run(T, z2, dev)
    oth = torch.ones(Bn, dtype=torch.bool, device=dev)
    oth[rows] = False
    _bitwise(r2, base, "rows beside a scaled one", oth)
    for b in rows:
        d = (r2.J[b] - 4.0 * base.J[b]).abs().max().item()
        assert torch.equal(r2.J[b], 4.0 * base.J[b]), (b, "J(2 z0) != 4 J(z0)", d)
        assert int(r2.t_star[b]) == int(base.t_star[b])
        assert float(r2.j_star[b]) == 4.0 * float(base.j_star[b])
        assert int(r2.status[b]) == int(base.status[b])


# --------------------------------------------------------------------------
# the hand-over paths: the rerun launches read z0 per problem
# --------------------------------------------------------------------------

def test_s13_forced_handover_is_the_reference_association_bitwise(dev):
    """HOP_OPT_FORCE_HANDOVER with a z0 of its own per problem: the pipeline (Bn = 4:
    at most four per workgroup) writes z0 into row S of its twelve tiles, the LFT body
    (the full workgroup of Bn = 19) into its own; N = 37 and 21 as test_gpu_rerun.py.
    Bitwise HOP_OPT_REFERENCE_ASSOC."""
    for name, N in (("s13-forced-pipe", 37), ("s13-forced-body", 21), ("s13-forced-pipe", 8)):
        p = BY_NAME[name]
        q = Path(name, 13, 4, p.Bn, N=N, opts=p.opts)
        r = Path("ref", 13, 4, p.Bn, N=N, opts=dict(reference_assoc=True))
        T, z0 = q.tensors(dev), q.z0()
        _bitwise(q.run(T, z0, dev), r.run(T, z0, dev), (name, N))


def _escalate(Q, b, k, target=5e-7):
    """tests/test_gpu_rerun.py: chol_inv's tries at 1e-9 .. 1e-7 fail, 1e-6 succeeds"""
    lo = np.linalg.eigvalsh(orc.sym(Q[b, k])).min()
    Q[b, k] = Q[b, k] - np.eye(Q.shape[-1]) * (lo + target)


def test_s13_genuine_handovers_with_dense_z0(dev):
    """Workgroups of sixteen with 1, 2, 4 and 5 genuine hand-overs (the last above the
    pipeline's four: the LFT body), alternately chol_inv's LU slot (Q_k = -I) and an
    escalated jitter (utils.py:81-93), every problem with a dense z0: the recomputed
    problems are bitwise the reference-association kernel's, their status word the
    oracle's; the rest keep the conditioned curve (1e-9) and status 0."""
    import torch
    Bn, s, m, N = 96, 13, 4, 30
    p = Path("s13-cond", s, m, Bn, N=N)
    r = Path("ref", s, m, Bn, N=N, opts=dict(reference_assoc=True))
    A, Bm, Q, Ri, QT = (x.copy() for x in _blocks(4700, Bn, s, m, N))
    bad = [0, 16, 17, 32, 33, 34, 35, 48, 49, 50, 51, 52]
    for j, b in enumerate(bad):
        if j % 2:
            _escalate(Q, b, (3 * b) % N)
        else:
            Q[b, (3 * b) % N] = -np.eye(s)
    z0 = orc.synth_z0(("dense",), Bn, s, 47)
    T = tuple(_t(x, dev) for x in (A, Bm, Q, Ri, QT))
    d, ref = p.run(T, z0, dev, t_min=5), r.run(T, z0, dev, t_min=5)
    _bitwise(d, ref, "recomputed problems", bad)
    assert torch.equal(d.status, ref.status)
    st = d.status.cpu().numpy()
    for b in bad:
        o = orc.lft_sweep(A[b], Bm[b], Q[b], Ri[b], z0[b], QT[b])
        assert int(st[b]) == int(o["status"]) != 0, (b, int(st[b]), o["status"])
    ok = np.ones(Bn, dtype=bool)
    ok[bad] = False
    assert (st[ok] == 0).all()
    Jo, _ = orc.lft_sweep_batch(A[ok], Bm[ok], Q[ok], Ri[ok], z0[ok], QT[ok])
    assert _elem_rel(_np(d.J)[ok], Jo) <= 1e-9


@pytest.mark.parametrize("name", ["s13-cond", "s13-cond-packed", "s13-f32-cond", "s5m2-rowgroup",
                                  "s5m1-rowgroup", "s3m1-rowgroup", "s2m1-rowgroup",
                                  "s5m1-f32-lane", "s4m2-f32-tile64", "s4m2-tile64",
                                  "s5m2-tile64", "s5m1-tile64"])
def test_no_finite_z0_causes_a_handover(dev, name):
    """HOP_OPT_NO_RERUN on clean blocks: whatever finite z0 a problem carries (the zero
    vector and 1e+-3 scalings included), the conditioned kernel keeps it (status 0, no
    HOP_ST_HANDOVER), and its curve is the default launch pair's, bitwise."""
    from time_opt_ilqr_amd import _lib
    p = BY_NAME[name]
    q = Path(name, p.s, p.m, p.Bn, N=p.N, dtype=p.dtype, tile=p.tile, rep=p.rep,
             opts=dict(no_rerun=True))
    T, z0 = p.tensors(dev), p.z0()
    a, b = q.run(T, z0, dev), p.run(T, z0, dev)
    st = a.status.cpu().numpy()
    assert (st == 0).all(), (np.nonzero(st)[0][:8], st[st != 0][:8], _lib.ST_HANDOVER)
    _bitwise(a, b, "no_rerun against the launch pair")


@pytest.mark.parametrize("s,m", SMALL)
def test_small_handovers_with_dense_z0(dev, s, m):
    """fp64 s <= 5, Bn = 600: chol_inv LU slots (Q_k = -I) at one and two problems of a
    workgroup (the pipelined rerun, whose query wave reads z0 per problem) and at four
    (more than kSmallPipeMax: the one-lane body; s = 5, whose workgroups hold 192
    problems, has a fourth workgroup, with five), every problem with a dense z0; N = 65
    cuts a beat.  The pipeline, the one-lane rerun (HOP_OPT_RERUN_LANE) and
    the reference association alone agree bitwise on the handed-over problems, the
    others keep the conditioned kernel's bits and the oracle's J."""
    import torch
    Bn, N = 600, 65
    A, Bm, Q, Ri, QT = (x.copy() for x in _blocks(8100 + 7 * s + m, Bn, s, m, N))
    ppb = 192 if s == 5 else 256  # problems per workgroup (tests/test_gpu_small_rowgroup.py)
    bad = [3] + [ppb + 10, ppb + 70] + [2 * ppb + i for i in (0, 1, 63, 64)]
    if 3 * ppb + 5 < Bn:
        bad += [3 * ppb + i for i in (5, 6, 7, 8, 9)]
    for j, b in enumerate(bad):
        Q[b, (7 * j) % N] = -np.eye(s)
    z0 = orc.synth_z0(("dense",), Bn, s, 53)
    T = tuple(_t(x, dev) for x in (A, Bm, Q, Ri, QT))
    mk = lambda **o: Path("x", s, m, Bn, N=N, opts=o)  # noqa: E731
    t_min = N // 3
    d = mk().run(T, z0, dev, t_min=t_min)
    ln = mk(rerun_lane=True).run(T, z0, dev, t_min=t_min)
    ref = mk(reference_assoc=True).run(T, z0, dev, t_min=t_min)
    st = d.status.cpu().numpy()
    assert all(int(st[b]) & orc.ST_LU for b in bad), st[bad]
    _bitwise(d, ln, "pipeline against the one-lane rerun", bad)
    _bitwise(d, ref, "pipeline against the reference association", bad)
    ok = np.ones(Bn, dtype=bool)
    ok[bad] = False
    okt = torch.as_tensor(ok, device=dev)
    _bitwise(d, ln, "problems nobody handed over", okt)
    assert (st[ok] == 0).all()
    sub = np.nonzero(ok)[0][::9]  # the oracle on every ninth of them
    Jo, _ = orc.lft_sweep_batch(A[sub], Bm[sub], Q[sub], Ri[sub], z0[sub], QT[sub])
    assert _elem_rel(_np(d.J)[sub], Jo) <= 1e-9


def test_f32_forced_handover_is_the_generic_kernel(dev):
    """s = 13 fp32 blocks: the rerun launch is the generic fp32 kernel (its LaneDot of
    z0^T P0), bitwise HOP_OPT_FORCE_GENERIC on the same per-problem z0."""
    p = BY_NAME["s13-f32-forced"]
    g = Path("g", 13, 4, p.Bn, dtype="f32", opts=dict(force_generic=True))
    T, z0 = p.tensors(dev), p.z0()
    _bitwise(p.run(T, z0, dev), g.run(T, z0, dev), "forced against generic")


# --------------------------------------------------------------------------
# callers: the drop-in and the mixed batch
# --------------------------------------------------------------------------

@pytest.mark.parametrize("s,m", [(5, 1), (13, 4), (21, 4)])
def test_dropin_propagator_with_dense_z0(dev, s, m):
    """horizon_selection.propagator_all_Jt_aug (lists of NumPy blocks, one problem)
    with a dense z0 against the oracle: the small-s, the s = 13 and the wide kernel."""
    from time_opt_ilqr_amd import horizon_selection as hs
    A, Bm, Q, R, Ri, _, QT = orc.synth_lft_problem(6100 + s, s, m, N0)
    for kind in ("dense", "offset"):
        z0 = orc.synth_z0((kind,), 1, s, 61)[0]
        J = hs.propagator_all_Jt_aug(list(A), list(Bm), list(Q), [R] * N0, z0, list(QT),
                                     R_inv_cached=Ri)
        o = orc.lft_sweep(A, Bm, Q, Ri, z0, QT)
        err = _elem_rel(J, o["J"])
        print(f"[z0] dropin s={s} {kind}: {err:.3e}")
        assert err <= 1e-9 and o["status"] == 0


def test_mixed_batch_per_problem_z0(dev):
    """engine.propagate_groups (config 5's kinds: Segway and Cart-pole s = 5, m = 1,
    Quadrotor s = 13, m = 4) with a dense z0 per member: bitwise each group's own
    launch, the oracle at every member's true shape, and the padded launch of
    packing.pack_mixed (z0's pad entries 0) to 1e-9."""
    import torch
    from time_opt_ilqr_amd import engine
    from time_opt_ilqr_amd.packing import pack_mixed
    Bn, N = 23, N0
    probs = [orc.synth_config5_problem(6300, i, N) for i in range(Bn)]
    zs = [orc.synth_z0(("dense",), 1, p[0].shape[-1], 6400 + i)[0] for i, p in enumerate(probs)]
    order = np.arange(Bn) % 3
    groups = []
    for g in range(3):
        mem = [i for i in range(Bn) if i % 3 == g]
        st = lambda j: _t(np.stack([probs[i][j] for i in mem]), dev)  # noqa: E731
        groups.append((st(0), st(1), st(2), st(4), _t(np.stack([zs[i] for i in mem]), dev),
                       st(6)))
    res = engine.propagate_groups(groups, engine.mixed_plan(order, 3, dev), t_min=T_MIN, t_max=N)
    mb = pack_mixed(groups, order, 13, 4)
    pad = engine.propagate(mb.A, mb.B, mb.Q, mb.R_inv, mb.z0, mb.QT, t_min=T_MIN, t_max=N)
    torch.cuda.synchronize()
    assert int(res.status.abs().sum()) == 0 and int(pad.status.abs().sum()) == 0
    for g in range(3):
        own = engine.propagate(*groups[g], t_min=T_MIN, t_max=N)
        sl = torch.as_tensor([i for i in range(Bn) if i % 3 == g], device=dev)
        assert torch.equal(res.J[sl], own.J) and torch.equal(res.t_star[sl], own.t_star)
    Jo = np.stack([orc.lft_sweep(p[0], p[1], p[2], p[4], zs[i], p[6])["J"]
                   for i, p in enumerate(probs)])
    print(f"[z0] mixed groups {_elem_rel(_np(res.J), Jo):.3e} padded {_elem_rel(_np(pad.J), Jo):.3e}")
    assert _elem_rel(_np(res.J), Jo) <= 1e-9
    assert _elem_rel(_np(pad.J), Jo) <= 1e-9
    To, _ = orc.select_horizon(Jo, T_MIN, N)
    assert res.t_star.cpu().numpy().tolist() == To.tolist()


# --------------------------------------------------------------------------
# a non-finite z0
# --------------------------------------------------------------------------

@pytest.mark.parametrize("path", NONFINITE, ids=repr)
def test_nonfinite_z0(dev, path):
    """A NaN in z0[b, 0] of one problem and in z0[b', s - 1] of another (the reference:
    NaN from z0 @ P0 @ z0 at every horizon): the whole J row NaN, ST_NONFINITE, T* =
    t_min (a NaN wins at the window's first horizon), every other problem bitwise the
    unpoisoned run's.  An inf entry: non-finite J and ST_NONFINITE only (inf * 0 or
    inf - inf give NaN where the plain product gives +inf; what each path returns is
    printed)."""
    import torch
    Bn, s = path.Bn, path.s
    T, zc = path.tensors(dev), path.z0()
    bad = [2, Bn - 2]
    zc[bad[0]] = orc.synth_z0(("dense",), 1, s, 71)[0]
    zc[bad[1]] = orc.synth_z0(("offset",), 1, s, 72)[0]
    zp = zc.copy()
    zp[bad[0], 0] = np.nan
    zp[bad[1], s - 1] = np.nan
    clean = path.run(T, zc, dev)
    res = path.run(T, zp, dev)
    st = res.status.cpu().numpy()
    for b in bad:
        assert bool(res.J[b].isnan().all()), (b, res.J[b])
        assert int(st[b]) & orc.ST_NONFINITE, (b, int(st[b]))
        assert int(res.t_star[b]) == min(T_MIN, path.N) and bool(res.j_star[b].isnan())
    oth = torch.ones(Bn, dtype=torch.bool, device=dev)
    oth[bad] = False
    _bitwise(res, clean, "problems beside a poisoned z0", oth)
    zi = zc.copy()
    zi[bad[0], 1 % s] = np.inf
    ri = path.run(T, zi, dev)
    Ji = _np(ri.J)[bad[0]]
    print(f"[z0] {path.name} inf entry: status {int(ri.status[bad[0]])}, J "
          f"{'all NaN' if np.isnan(Ji).all() else 'all +inf' if (Ji == np.inf).all() else Ji}, "
          f"T* {int(ri.t_star[bad[0]])}")
    assert not np.isfinite(Ji).any() and int(ri.status[bad[0]]) & orc.ST_NONFINITE
    oth[bad[1]] = True
    oth[bad[0]] = False
    _bitwise(ri, clean, "problems beside an infinite z0", oth)


def test_nonfinite_z0_triage_equals_the_reference_association(dev):
    """s = 13 default: the conditioned kernel hands a NaN z0 over, the rerun launch's
    triage finds a non-finite shared input (h_poison = 1) and writes the outcome
    without a recompute: status, NaN pattern and T* of HOP_OPT_REFERENCE_ASSOC."""
    import torch
    p, r = BY_NAME["s13-cond"], BY_NAME["s13-refassoc"]
    T, z0 = p.tensors(dev), p.z0()
    z0[5, 0] = np.nan
    z0[17, 12] = np.nan
    z0[36, 7] = np.nan
    a, b = p.run(T, z0, dev), r.run(T, z0, dev)
    assert torch.equal(a.status, b.status)
    assert torch.equal(a.J.isnan(), b.J.isnan()) and int(a.J.isnan().sum()) == 3 * p.N
    assert torch.equal(a.t_star, b.t_star)
    assert torch.equal(a.j_star.isnan(), b.j_star.isnan())
    # HOP_OPT_NO_RERUN still runs the triage: nothing is left handed over
    q = Path("nr", 13, 4, p.Bn, opts=dict(no_rerun=True))
    assert torch.equal(q.run(T, z0, dev).status, b.status)


# --------------------------------------------------------------------------
# per-step, per-problem R
# --------------------------------------------------------------------------

R_CASES = [("generic-s7", 7, 3, 9, False), ("generic-s13", 13, 4, 9, False),
           ("generic-s16", 16, 6, 9, False), ("wide-s17", 17, 4, 5, True),
           ("wide-s32m16", 32, 16, 5, True)]


@pytest.mark.parametrize("name,s,m,Bn,wide", R_CASES, ids=[c[0] for c in R_CASES])
def test_per_step_R_every_stride(dev, name, s, m, Bn, wide):
    """R different at every (problem, step) (orc.synth_R_steps, SPD): [Bn, N, m, m] and
    [1, N, m, m] (r_batch_stride 0 with a step stride), as R^-1 and (narrow kernels) as
    raw R_k inverted in the kernel, n_use < N, with a per-problem z0; the oracle's J to
    1e-9.  A 4-D R sends s = 13 to the generic kernel (the conditioned kernels take no
    step stride)."""
    import torch
    N = N0
    p = Path(name, s, m, Bn, N=N)
    T = p.tensors(dev)
    A, Bm, Q, _, QT = p.base()
    z0 = p.z0()
    R, Ri = orc.synth_R_steps(7700 + s, Bn, N, m)
    assert np.linalg.eigvalsh(R).min() > 0.0
    flat = R.reshape(-1, m * m)
    assert len(np.unique(flat, axis=0)) == len(flat)  # differs at every (b, k)
    forms = [("R^-1", Ri, True)] + ([] if wide else [("raw R", R, False)])
    Jo, sto = orc.lft_sweep_batch(A, Bm, Q, Ri, z0, QT)
    Jo1, _ = orc.lft_sweep_batch(A, Bm, Q, Ri[3:4], z0, QT)
    assert (sto == 0).all()
    live = z0.any(axis=1)  # the all-zero z0 row: J exactly 0.0, compared absolutely
    assert (Jo[~live] == 0.0).all()
    full = None
    for tag, Rx, inv in forms:
        res = p.run(T, z0, dev, R=_t(Rx, dev), r_is_inverse=inv)
        assert (_np(res.J)[~live] == 0.0).all()
        err = _elem_rel(_np(res.J)[live], Jo[live])
        print(f"[z0] {name} per-step {tag} [Bn,N,m,m]: {err:.3e}")
        assert err <= 1e-9 and int(res.status.abs().sum()) == 0
        To, _ = orc.select_horizon(Jo, T_MIN, N)
        assert res.t_star.cpu().numpy().tolist() == To.tolist()
        full = res if inv else full
        one = p.run(T, z0, dev, R=_t(Rx[3:4], dev), r_is_inverse=inv)
        err = _elem_rel(_np(one.J)[live], Jo1[live])
        print(f"[z0] {name} per-step {tag} [1,N,m,m]: {err:.3e}")
        assert err <= 1e-9 and int(one.status.abs().sum()) == 0
        cut = p.run(T, z0, dev, R=_t(Rx, dev), r_is_inverse=inv, n_use=N - 5)
        assert torch.equal(cut.J, res.J[:, :N - 5])  # a prefix of the same curve, bitwise
    # two steps' R exchanged: the horizons before the earlier step never read either
    # (bitwise alone); from that step on every J moves
    k1, k2 = 4, 9
    Rs = Ri.copy()
    Rs[:, [k1, k2]] = Rs[:, [k2, k1]]
    sw = p.run(T, z0, dev, R=_t(Rs, dev))
    assert torch.equal(sw.J[:, :k1], full.J[:, :k1])
    lt = torch.as_tensor(live, device=dev)
    assert bool((sw.J[lt][:, k1:] != full.J[lt][:, k1:]).all())
    Js, _ = orc.lft_sweep_batch(A, Bm, Q, Rs, z0, QT)
    assert _elem_rel(_np(sw.J)[live], Js[live]) <= 1e-9


@pytest.mark.parametrize("s,m", [(7, 3), (17, 4)])
def test_dropin_raw_R_list_of_different_matrices(dev, s, m):
    """propagator_all_Jt_aug with R_list (no cached inverse): the generic kernel inverts
    R_k per step, the wide drop-in inverts on the host and passes the step stride."""
    from time_opt_ilqr_amd import horizon_selection as hs
    A, Bm, Q, _, _, _, QT = orc.synth_lft_problem(7800 + s, s, m, N0)
    R, _ = orc.synth_R_steps(7900 + s, 1, N0, m)
    z0 = orc.synth_z0(("offset",), 1, s, 79)[0]
    J = hs.propagator_all_Jt_aug(list(A), list(Bm), list(Q), list(R[0]), z0, list(QT))
    o = orc.lft_sweep(A, Bm, Q, None, z0, QT, R_list=R[0])
    print(f"[z0] dropin raw R_list s={s}: {_elem_rel(J, o['J']):.3e}")
    assert _elem_rel(J, o["J"]) <= 1e-9 and o["status"] == 0
