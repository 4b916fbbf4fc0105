"""Every instantiation of the Riccati kernels against the per-step oracle bar.

dispatch_riccati (csrc/riccati.hip) runs riccati_kernel<T, S, MM, mode> and
riccati_jcurve_kernel<T, S, MM> in five (S, MM) buckets, in fp64 and fp32; the exact-size
kernel (riccati_fast.hip) sits in front of them at (12, 4), the legacy twin's passes
behind legacy=True, the wide kernel (riccati_wide.hip, HR = 8 / 12 / 16) above n = 16.
The rows of tests/riccati_shapes.py reach both ends and a padded interior of every
bucket; each is run in mode 0, mode 1 and as the J curve on a batch of 19 (five distinct
problems with horizons 1, 2, N/2, N-1, N, repeated: one workgroup boundary, a tail of 3)
and compared per step with the NumPy oracle: 1e-6 in fp64 (V0 and J 1e-9), 2e-3 in fp32
against the fp64 oracle on the fp32-rounded inputs.  test_riccati_shapes_cpu.py proves
that these inputs keep the oracle inside what the assertions here presuppose.
"""
import contextlib

import numpy as np
import pytest

import riccati_shapes as rs
from gain_check import assert_per_step
from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

IDX = rs.batch_index()
ROWS = rs.TABLE + rs.WIDE_TABLE
# fp32 has no wide and no exact-size kernel: (12, 4) in fp32 is the <12,4> row's case
ROW_DTYPES = [(r, d) for r in ROWS for d in ("f64", "f32")
              if d == "f64" or not (r.wide or r.bucket == "fast")]
_ids = lambda v: v if isinstance(v, str) else v.id  # noqa: E731

WORST = {}  # (bucket, dtype, entry) -> worst error seen


@pytest.fixture(scope="module", autouse=True)
def _worst_table():
    yield
    print("\nworst error per (bucket, dtype, entry):")
    for (bucket, dtype, entry), v in sorted(WORST.items()):
        print(f"  WORST {bucket:12s} {dtype} {entry:8s} {v:.3e}")


def _note(row, dtype, entry, err):
    key = (row.bucket, dtype, entry)
    WORST[key] = max(WORST.get(key, 0.0), float(err))


def _torch_dtype(dtype):
    import torch
    return torch.float32 if dtype == "f32" else torch.float64


def _np(t):
    return t.double().cpu().numpy() if t.is_floating_point() else t.cpu().numpy()


def _options(row):
    from time_opt_ilqr_amd import _lib
    return _lib.options(force_generic=True) if row.force_generic else contextlib.nullcontext()


class Inputs:
    """the device tensors of one batch (rs.batch) and the three entries on them"""

    def __init__(self, row, dtype, dev, b=None):
        import torch
        self.row, self.dev = row, dev
        b = rs.batch(row, dtype) if b is None else b
        td = _torch_dtype(dtype)
        t = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=td, device=dev)  # noqa: E731
        self.T = b["T"]
        self.horizon = torch.as_tensor(b["T"], dtype=torch.int32, device=dev)
        self.args = {k: t(b[k]) for k in ("A", "B", "X", "U", "xg", "ur", "Q", "R", "Qf")}
        self.kw = {}
        if row.extra:
            self.kw = dict(qxx_extra=t(b["cxx"]), qx_extra=t(b["cx"]), c_extra=t(b["c0"]))
        self.wrap = rs.wrap_idx(row.n)

    def _a(self, over):
        a = dict(self.args, **over)
        return [a[k] for k in ("A", "B", "X", "U", "xg", "ur", "Q", "R", "Qf")]

    def mode0(self, lm=rs.LM0, want_v=True, legacy=False, **over):
        from time_opt_ilqr_amd import engine
        with _options(self.row):
            return engine.riccati(*self._a(over), self.horizon, lm, mode=0, wrap_idx=self.wrap,
                                  want_v=want_v, legacy=legacy, **self.kw)

    def mode1(self, lm=rs.LM1, legacy=False, **over):
        from time_opt_ilqr_amd import engine
        with _options(self.row):
            return engine.riccati(*self._a(over), self.horizon, lm, mode=1, w_stage=rs.W_STAGE,
                                  wrap_idx=self.wrap, legacy=legacy, **self.kw)

    def jcurve(self, legacy=False, **over):
        from time_opt_ilqr_amd import engine
        kw = dict(self.kw, lm_lambda=rs.LM1, w_stage=rs.W_STAGE, wrap_idx=self.wrap)
        with _options(self.row):
            if self.row.wide:  # the callers one level up route by n alone, as riccati() does
                return engine.bruteforce_jcurve_wide(*self._a(over), rs.N, **kw)
            return engine.bruteforce_jcurve(*self._a(over), rs.N, legacy=legacy, **kw)


def _written(res, T, fields):
    """the written part of a RiccatiResult per batch row: steps t < T (K, k), t <= T (V)"""
    out = []
    for b, Tb in enumerate(T):
        out.append({f: getattr(res, f)[b, :int(Tb) + (1 if f.startswith("V") else 0)]
                    for f in fields})
    return out


def _assert_same_bits(ra, rb, T, fields, what, rows=None):
    import torch
    wa, wb = _written(ra, T, fields), _written(rb, T, fields)
    for b in (range(len(T)) if rows is None else rows):
        for f in fields:
            assert torch.equal(wa[b][f], wb[b][f]), (what, b, f)


def _check_mode0(res, row, dtype, tol, what="mode 0"):
    ref = rs.reference(row, dtype)
    st = _np(res.status)
    assert st.tolist() == [0] * rs.BATCH, (what, st.tolist())
    worst = 0.0
    for b in range(rs.BATCH):
        k, K, ok, Vxx, Vx = ref[IDX[b]]["m0"]
        T = int(rs.HORIZONS[IDX[b]])
        assert ok
        for name, got, want in (("K", res.K[b, :T], K), ("k", res.k[b, :T], k),
                                ("Vxx", res.Vxx[b, :T + 1], Vxx), ("Vx", res.Vx[b, :T + 1], Vx)):
            worst = max(worst, assert_per_step(_np(got), want, tol, f"{row.id} {what} {b} {name}"))
    return worst


def _check_mode1(res, row, dtype, tol, what="mode 1"):
    ref = rs.reference(row, dtype)
    st = _np(res.status)
    assert st.tolist() == [0] * rs.BATCH, (what, st.tolist())
    worst = worst_v0 = 0.0
    for b in range(rs.BATCH):
        Vxx, Vx, V0, K, k = ref[IDX[b]]["m1"]
        T = int(rs.HORIZONS[IDX[b]])
        for name, got, want in (("K", res.K[b, :T], K), ("k", res.k[b, :T], k),
                                ("Vxx", res.Vxx[b, :T + 1], Vxx), ("Vx", res.Vx[b, :T + 1], Vx),
                                ("V0", res.V0[b, :T + 1], V0)):
            worst = max(worst, assert_per_step(_np(got), want, tol, f"{row.id} {what} {b} {name}"))
        if dtype == "f64":
            worst_v0 = max(worst_v0, assert_per_step(_np(res.V0[b, :T + 1]), V0, rs.BAR64_V0,
                                                     f"{row.id} {what} {b} V0 (1e-9)"))
    return worst, worst_v0


def _j_rel(J, row, dtype):
    Jo = np.stack([rs.reference(row, dtype)[i]["J"] for i in IDX])
    return float(np.max(np.abs(J - Jo) / np.abs(Jo)))


@pytest.mark.parametrize("row,dtype", ROW_DTYPES, ids=_ids)
def test_mode0_vs_oracle(dev, row, dtype):
    """backward_pass_truncated: K, k, Vxx, Vx per step, every status 0"""
    res = Inputs(row, dtype, dev).mode0()
    worst = _check_mode0(res, row, dtype, rs.BAR64 if dtype == "f64" else rs.BAR32)
    _note(row, dtype, "mode 0", worst)
    print(row.id, dtype, "mode 0 worst per-step error", worst)


@pytest.mark.parametrize("row,dtype", ROW_DTYPES, ids=_ids)
def test_mode1_vs_oracle(dev, row, dtype):
    """value_expansions_and_gains_prefix (S_right = 0): K, k, Vxx, Vx, V0 per step"""
    res = Inputs(row, dtype, dev).mode1()
    worst, worst_v0 = _check_mode1(res, row, dtype, rs.BAR64 if dtype == "f64" else rs.BAR32)
    _note(row, dtype, "mode 1", worst)
    print(row.id, dtype, "mode 1 worst per-step error", worst, "V0", worst_v0)


@pytest.mark.parametrize("row,dtype", ROW_DTYPES, ids=_ids)
def test_jcurve_vs_oracle(dev, row, dtype):
    """the brute-force curve, elementwise relative, every status 0"""
    J, st = Inputs(row, dtype, dev).jcurve()
    assert tuple(J.shape) == (rs.BATCH, rs.N)
    assert not _np(st).any(), _np(st).tolist()
    err = _j_rel(_np(J), row, dtype)
    _note(row, dtype, "J", err)
    print(row.id, dtype, "J elementwise relative error", err)
    assert err <= (rs.BAR64_V0 if dtype == "f64" else rs.BAR32)  # 1e-9 is inside the 1e-6 bar


M0, M1 = ("K", "k", "Vxx", "Vx"), ("K", "k", "Vxx", "Vx", "V0")


@pytest.mark.parametrize("row", ROWS, ids=_ids)
def test_invariants_without_a_reference(dev, row):
    """fp64, all three entries: a problem's repeats are bitwise equal wherever they sit in
    the batch; shared cost blocks (batch stride 0) and the same blocks repeated per
    problem give the same bits and statuses; so do a scalar lm and its [B] tensor (the J
    curve takes a scalar only)."""
    import torch
    inp = Inputs(row, "f64", dev)
    T = inp.T
    r0, r1 = inp.mode0(), inp.mode1()
    J, Jst = inp.jcurve()
    first = torch.as_tensor(IDX, device=dev)
    for res, fields in ((r0, M0), (r1, M1)):
        w = _written(res, T, fields)
        for b in range(rs.DISTINCT, rs.BATCH):
            for f in fields:
                assert torch.equal(w[b][f], w[IDX[b]][f]), (row.id, b, f)
        assert torch.equal(res.status, res.status[first])
    assert torch.equal(J, J[first]) and torch.equal(Jst, Jst[first])

    # a scalar lm and the [B] tensor of that value
    for run, lm, fields, ref in ((inp.mode0, rs.LM0, M0, r0), (inp.mode1, rs.LM1, M1, r1)):
        rt = run(lm=torch.full((rs.BATCH,), lm, dtype=torch.float64, device=dev))
        _assert_same_bits(rt, ref, T, fields, (row.id, "lm tensor"))
        assert torch.equal(rt.status, ref.status)

    # problem 0's cost blocks for everyone: shared [n, n] ... against [B, n, n] ...
    shared = {k: inp.args[k][0].contiguous() for k in ("xg", "ur", "Q", "R", "Qf")}
    rep = {k: v.unsqueeze(0).repeat(rs.BATCH, *([1] * v.dim())).contiguous()
           for k, v in shared.items()}
    if row.bucket == "fast":
        # a shared Q selects the exact-size kernel's two-wave layout; bit equality is
        # pinned for it where test_riccati_two_wave_layout_bitwise states it: K, k, status
        # of mode 0 (no value expansion asked for) and mode 1 with its value expansion
        cases = ((lambda **o: inp.mode0(want_v=False, **o), ("K", "k")), (inp.mode1, M1))
    else:
        cases = ((inp.mode0, M0), (inp.mode1, M1))
    for run, fields in cases:
        rs_, rr = run(**shared), run(**rep)
        assert torch.equal(rs_.status, rr.status), row.id
        assert _np(rs_.status).tolist() == [0] * rs.BATCH
        _assert_same_bits(rs_, rr, T, fields, (row.id, "shared"))
    if row.bucket != "fast":
        Js, Jss = inp.jcurve(**shared)
        Jr, Jsr = inp.jcurve(**rep)
        assert torch.equal(Js, Jr) and torch.equal(Jss, Jsr), row.id
        assert not _np(Jss).any()


@pytest.mark.parametrize("row", rs.FAILURE_ROWS, ids=_ids)
def test_failure_row_is_contained(dev, row):
    """one problem's R = -50 I: ST_FAIL in mode 0 (the oracle: ok is False), ST_FAIL and
    NaN at every horizon of its J curve, every other row bitwise what it was without it"""
    import torch
    from time_opt_ilqr_amd import _lib
    clean = Inputs(row, "f64", dev)
    b = rs.batch(row)
    b["R"][rs.BAD_ROW] = rs.bad_R(row.m)
    bad = Inputs(row, "f64", dev, b)
    i = int(IDX[rs.BAD_ROW])
    p = rs.problems(row.n, row.m)
    assert orc.riccati_truncated(list(p["A"][i]), list(p["B"][i]), p["X"][i], p["U"][i],
                                 p["xg"][i], p["ur"][i], p["Q"][i], rs.bad_R(row.m), p["Qf"][i],
                                 int(p["T"][i]), lm_lambda=rs.LM0, wrap_idx=rs.wrap_idx(row.n))[2] \
        is False
    others = [x for x in range(rs.BATCH) if x != rs.BAD_ROW]
    r0c, r0b = clean.mode0(), bad.mode0()
    st = _np(r0b.status)
    assert st[rs.BAD_ROW] & _lib.ST_FAIL, st.tolist()
    assert st[others].tolist() == [0] * len(others)
    _assert_same_bits(r0b, r0c, clean.T, M0, (row.id, "mode 0"), rows=others)
    (Jc, Jsc), (Jb, Jsb) = clean.jcurve(), bad.jcurve()
    Jsb_, Jb_ = _np(Jsb), _np(Jb)
    assert (Jsb_[rs.BAD_ROW] & _lib.ST_FAIL).all(), Jsb_[rs.BAD_ROW].tolist()
    assert np.isnan(Jb_[rs.BAD_ROW]).all()
    o = torch.as_tensor(others, device=dev)
    assert torch.equal(Jb[o], Jc[o]) and torch.equal(Jsb[o], Jsc[o])
    assert not Jsb_[others].any()


@pytest.mark.parametrize("row", rs.LEGACY_ROWS, ids=_ids)
def test_legacy_twin_vs_oracle(dev, row):
    """legacy=True in both modes and as the J curve against the oracle's legacy functions
    (Qf = alpha I with the scalar alpha), at the same bars"""
    inp = Inputs(row, "f64", dev)
    p = rs.problems(row.n, row.m)
    assert all(np.array_equal(p["Qf"][i], p["alpha"][i] * np.eye(row.n))
               for i in range(rs.DISTINCT))
    ref = rs.reference_legacy(row)
    r0, r1 = inp.mode0(want_v=False, legacy=True), inp.mode1(legacy=True)
    J, Jst = inp.jcurve(legacy=True)
    assert _np(r0.status).tolist() == [0] * rs.BATCH
    assert _np(r1.status).tolist() == [0] * rs.BATCH
    assert not _np(Jst).any()
    w0 = w1 = wv = 0.0
    for b in range(rs.BATCH):
        T = int(rs.HORIZONS[IDX[b]])
        k, K, ok = ref[IDX[b]]["m0"]
        assert ok
        for name, got, want in (("K", r0.K[b, :T], K), ("k", r0.k[b, :T], k)):
            w0 = max(w0, assert_per_step(_np(got), want, rs.BAR64, f"{row.id} legacy 0 {b} {name}"))
        Vxx, Vx, V0, K, k, st = ref[IDX[b]]["m1"]
        assert st == 0
        for name, got, want in (("K", r1.K[b, :T], K), ("k", r1.k[b, :T], k),
                                ("Vxx", r1.Vxx[b, :T + 1], Vxx), ("Vx", r1.Vx[b, :T + 1], Vx),
                                ("V0", r1.V0[b, :T + 1], V0)):
            w1 = max(w1, assert_per_step(_np(got), want, rs.BAR64, f"{row.id} legacy 1 {b} {name}"))
        wv = max(wv, assert_per_step(_np(r1.V0[b, :T + 1]), V0, rs.BAR64_V0,
                                     f"{row.id} legacy 1 {b} V0 (1e-9)"))
    Jo = np.stack([ref[i]["J"] for i in IDX])
    ej = float(np.max(np.abs(_np(J) - Jo) / np.abs(Jo)))
    for entry, v in (("mode 0", w0), ("mode 1", w1), ("J", ej)):
        WORST[("legacy", "f64", entry)] = max(WORST.get(("legacy", "f64", entry), 0.0), v)
    print(row.id, "legacy worst: mode 0", w0, "mode 1", w1, "V0", wv, "J", ej)
    assert ej <= rs.BAR64_V0


def _wide_riccati_direct(dev, inp, lm, mode):
    """hop_riccati_wide_f64 called directly (the engine routes n <= 16 to the narrow
    kernels), with engine.riccati's argument list and output shapes"""
    import torch
    from time_opt_ilqr_amd import _lib, engine
    lib = _lib.load()
    a = inp.args
    Bn, N, n, _ = a["A"].shape
    m = a["B"].shape[-1]
    f64 = torch.float64
    K = torch.empty((Bn, N, m, n), dtype=f64, device=dev)
    k = torch.empty((Bn, N, m), dtype=f64, device=dev)
    Vxx = torch.empty((Bn, N + 1, n, n), dtype=f64, device=dev)
    Vx = torch.empty((Bn, N + 1, n), dtype=f64, device=dev)
    V0 = torch.empty((Bn, N + 1), dtype=f64, device=dev)
    status = torch.empty((Bn,), dtype=torch.int32, device=dev)
    lmv = torch.full((Bn,), lm, dtype=f64, device=dev)
    for key, shape in (("A", (Bn, N, n, n)), ("B", (Bn, N, n, m)), ("X", (Bn, N + 1, n)),
                       ("U", (Bn, N, m)), ("xg", (Bn, n)), ("ur", (Bn, m)), ("Q", (Bn, n, n)),
                       ("R", (Bn, m, m)), ("Qf", (Bn, n, n))):
        assert tuple(a[key].shape) == shape and a[key].is_contiguous() and a[key].dtype == f64
    assert tuple(inp.horizon.shape) == (Bn,) and inp.horizon.dtype == torch.int32
    _lib.check(lib.hop_riccati_wide_f64(
        _lib.ptr(a["A"]), _lib.ptr(a["B"]), _lib.ptr(a["X"]), _lib.ptr(a["U"]),
        _lib.ptr(a["xg"]), n, _lib.ptr(a["ur"]), m, _lib.ptr(a["Q"]), n * n,
        _lib.ptr(a["R"]), m * m, _lib.ptr(a["Qf"]), n * n, None, None, None,
        _lib.ptr(inp.horizon), _lib.ptr(lmv), float(rs.W_STAGE if mode == 1 else 0.0),
        engine.wrap_mask(inp.wrap, n), mode, 12, Bn, N, n, m, _lib.ptr(K), _lib.ptr(k),
        _lib.ptr(Vxx), _lib.ptr(Vx), _lib.ptr(V0), _lib.ptr(status), _lib.stream_handle(dev)))
    torch.cuda.synchronize()
    return engine.RiccatiResult(K, k, status, Vxx, Vx, V0)


@pytest.mark.parametrize("row", rs.WIDE_HR8, ids=_ids)
def test_wide_hr8_direct_vs_oracle(dev, row):
    """the wide kernel's HR = 8 instantiation (n <= 16), both modes, against the oracle
    and against the narrow generic kernel's statuses"""
    import torch
    inp = Inputs(row, "f64", dev)
    r0 = _wide_riccati_direct(dev, inp, rs.LM0, 0)
    r1 = _wide_riccati_direct(dev, inp, rs.LM1, 1)
    w0 = _check_mode0(r0, row, "f64", rs.BAR64, "wide mode 0")
    w1, wv = _check_mode1(r1, row, "f64", rs.BAR64, "wide mode 1")
    _note(row, "f64", "mode 0", w0)
    _note(row, "f64", "mode 1", w1)
    print(row.id, "worst per-step error: mode 0", w0, "mode 1", w1, "V0", wv)
    assert torch.equal(r0.status, inp.mode0().status)
    assert torch.equal(r1.status, inp.mode1().status)
