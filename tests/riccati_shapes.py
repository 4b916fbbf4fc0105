"""The shape table of the Riccati instantiation tests (test infrastructure).

test_gpu_riccati_shapes.py holds every instantiation of the Riccati kernels to the
per-step oracle bar on the rows below; test_riccati_shapes_cpu.py proves on the CPU that
the same inputs keep the oracle inside the preconditions those assertions rely on.  Both
take the rows, the batches and the (cached) oracle results from here, so the two files
cannot drift apart.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

from oracle import hop_oracle as orc

N = 10          # steps allocated per problem
DISTINCT = 5    # distinct problems per shape
BATCH = 19      # 16 problems per 256-thread workgroup: one boundary and a tail of 3
HORIZONS = (1, 2, N // 2, N - 1, N)  # one per distinct problem; a repeat keeps its problem's
BAD_ROW = 9     # the batch row of the failure case (problem 4, horizon N, mid-wave)
W_STAGE = 0.3
LM0, LM1 = 1e-3, 1e-6

# The bars.  fp64 1e-6 per step is the per-gain claim of gain_check.py, fp32 2e-3 the bar
# of test_riccati_fp32_generic_vs_oracle.  V0 and J (fp64) are held to 1e-9 as well, the
# bar the sweep tests put on the same curve (test_wide_block_form_vs_oracle): at 1e-6 a
# stage term that is off by 1e-5 (3e-6 per step on values of 1 .. 300) would pass.  It
# rests on the oracle's own error, which test_riccati_shapes_cpu.py measures against the
# 40-digit recursion (<= 1e-12), and on fp64 running the same <= 10 well-conditioned steps.
BAR64, BAR64_V0, BAR32 = 1e-6, 1e-9, 2e-3

# Inclusive (n_min, n_max, m_min, m_max) of every bucket of dispatch_riccati
# (time_opt_ilqr_amd/csrc/riccati.hip:538-552: m <= 4 picks S = 4/8/12/16 by n, anything
# wider in m runs <16,16>), of the exact-size kernel in front of them
# (riccati_fast.hip:1346, n = 12 and m = 4 only) and of the wide entries
# (riccati_wide.hip:418-421, HR = 8/12/16 by n; the engine routes n > 16 there).
BUCKET_BOUNDS = {
    "<4,4>": (1, 4, 1, 4),
    "<8,4>": (5, 8, 1, 4),
    "<12,4>": (9, 12, 1, 4),
    "fast": (12, 12, 4, 4),
    "<16,4>": (13, 16, 1, 4),
    "<16,16>": (1, 16, 5, 16),
}
# n strictly inside a bucket is one that is neither bound; <16,16> also wants an interior m
NARROW_BUCKETS = tuple(BUCKET_BOUNDS)


class Row(NamedTuple):
    bucket: str
    n: int
    m: int
    force_generic: bool = False  # run under _lib.options(force_generic=True)
    extra: bool = False          # with the extra stage cost (qxx_extra, qx_extra, c_extra)

    @property
    def id(self):
        return (f"{self.bucket}-{self.n}x{self.m}" + ("-generic" if self.force_generic else "")
                + ("-extra" if self.extra else ""))

    @property
    def wide(self):
        return self.n > 16


TABLE = (
    Row("<4,4>", 1, 1), Row("<4,4>", 2, 1), Row("<4,4>", 3, 2), Row("<4,4>", 4, 1),
    Row("<4,4>", 4, 4), Row("<4,4>", 3, 2, extra=True),
    Row("<8,4>", 5, 1), Row("<8,4>", 7, 3), Row("<8,4>", 8, 4), Row("<8,4>", 7, 3, extra=True),
    Row("<12,4>", 9, 1), Row("<12,4>", 9, 2), Row("<12,4>", 11, 4), Row("<12,4>", 12, 3),
    Row("<12,4>", 12, 4, force_generic=True), Row("<12,4>", 12, 4, extra=True),
    Row("fast", 12, 4),  # the inputs of the <12,4> rows at (12, 4): fast and generic on one set
    Row("<16,4>", 13, 1), Row("<16,4>", 15, 3), Row("<16,4>", 16, 4),
    Row("<16,4>", 15, 3, extra=True),
    Row("<16,16>", 1, 5), Row("<16,16>", 5, 5), Row("<16,16>", 8, 8), Row("<16,16>", 9, 7), Row("<16,16>", 13, 13),
    Row("<16,16>", 16, 5), Row("<16,16>", 16, 16), Row("<16,16>", 9, 7, extra=True),
)
# the first size of the wide Riccati kernel's HR = 16 instantiation (n = 25 .. 31)
WIDE_TABLE = (Row("wide HR=16", 25, 9), Row("wide HR=16", 25, 9, extra=True))
# HR = 8 (n <= 16) is reachable only through hop_riccati_wide_f64 called directly
WIDE_HR8 = (Row("wide HR=8", 9, 7), Row("wide HR=8", 16, 16))
# one failure batch per bucket
FAILURE_ROWS = (Row("<4,4>", 3, 2), Row("<8,4>", 7, 3), Row("<12,4>", 11, 4), Row("fast", 12, 4),
                Row("<16,4>", 15, 3), Row("<16,16>", 9, 7), Row("wide HR=16", 25, 9))
# the legacy twin: m <= 11 (its pinv tile), no extras, one row per (n, m); it has no
# exact-size form, so (12, 4) runs <12,4> whatever the options say
LEGACY_ROWS = tuple(r for r in TABLE if r.m <= 11 and not r.extra and not r.force_generic)

BY_ID = {r.id: r for r in TABLE + WIDE_TABLE + WIDE_HR8}


def wrap_idx(n):
    """the highest wrap bit sits on the last live state"""
    return [0] if n == 1 else [0, n - 1]


def batch_index():
    """problem of every batch row"""
    return np.arange(BATCH) % DISTINCT


def _round(x, dtype):
    x = np.asarray(x, dtype=np.float64)
    return x.astype(np.float32).astype(np.float64) if dtype == "f32" else x


@functools.lru_cache(maxsize=None)
def problems(n, m, dtype="f64"):
    """DISTINCT problems of one shape as a dict of stacked fp64 arrays (for "f32" every
    value rounded to fp32 first, so the fp64 oracle sees what the fp32 kernel is given),
    the terminal weight as alpha [D] and as Qf = alpha I [D, n, n], the horizons T [D].
    Problems 1 and 3 carry whole turns on the wrapped states, so that the wrap (and its
    mask bit at the edge of the live block) changes the error vectors."""
    ps = [orc.synth_riccati_problem(100000 + 1000 * n + 20 * m + i, n, m, N)
          for i in range(DISTINCT)]
    out = {k: np.stack([p[j] for p in ps])
           for j, k in enumerate(("A", "B", "X", "U", "xg", "ur", "Q", "R"))}
    for i in (1, 3):
        out["X"][i, :, n - 1] += 2.0 * np.pi
        if n > 1:
            out["X"][i, :, 0] -= 2.0 * np.pi
    out["alpha"] = np.array([p[8] for p in ps])
    out["Qf"] = np.stack([orc.terminal_weight(a, n) for a in out["alpha"]])
    out = {k: _round(v, dtype) for k, v in out.items()}
    out["T"] = np.array(HORIZONS, dtype=np.int32)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def extras(n, m, dtype="f64"):
    """the extra stage cost per (problem, step): PSD cxx, cx and c (the recipe of
    test_wide_riccati_vs_oracle)"""
    rng = np.random.default_rng(6)
    M = rng.standard_normal((DISTINCT, N, n, n))
    out = dict(cxx=0.05 * M @ M.transpose(0, 1, 3, 2) / n,
               cx=0.1 * rng.standard_normal((DISTINCT, N, n)),
               c0=rng.uniform(0.0, 0.5, (DISTINCT, N)))
    out = {k: _round(v, dtype) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def extra_callable(row, i, dtype="f64"):
    """the oracle's extra= callable of problem i (None without the extra cost): the step
    is the one whose nominal state is x"""
    if not row.extra:
        return None
    ex = extras(row.n, row.m, dtype)
    Xb = problems(row.n, row.m, dtype)["X"][i]

    def f(x, u):
        k = int(np.argmin(np.abs(Xb[:N] - x).sum(axis=1)))
        return ex["c0"][i, k], ex["cx"][i, k], ex["cxx"][i, k]
    return f


def batch(row, dtype="f64"):
    """the BATCH-row inputs: every array of problems() and extras() repeated by
    batch_index(); fresh (writable) copies"""
    idx = batch_index()
    out = {k: np.array(v[idx]) for k, v in problems(row.n, row.m, dtype).items()}
    if row.extra:
        out.update({k: np.array(v[idx]) for k, v in extras(row.n, row.m, dtype).items()})
    return out


def _problem_args(p, i):
    return (list(p["A"][i]), list(p["B"][i]), p["X"][i], p["U"][i], p["xg"][i], p["ur"][i],
            p["Q"][i], p["R"][i])


@functools.lru_cache(maxsize=None)
def reference(row, dtype="f64"):
    """the oracle on every distinct problem of the row at its own horizon: a list of
    dicts with m0 = (k, K, ok, Vxx, Vx) of riccati_truncated, m1 = (Vxx, Vx, V0, K, k) of
    riccati_expand(S_right = 0) and J of bruteforce_J(T_max = N), each as arrays"""
    p = problems(row.n, row.m, dtype)
    wrap = wrap_idx(row.n)
    out = []
    for i in range(DISTINCT):
        T = int(p["T"][i])
        ex = extra_callable(row, i, dtype)
        a = _problem_args(p, i)
        k, K, ok, Vxx, Vx = orc.riccati_truncated(*a, p["Qf"][i], T, lm_lambda=LM0,
                                                  wrap_idx=wrap, want_v=True, extra=ex)
        m0 = (np.array(k), np.array(K), ok, np.array(Vxx), np.array(Vx)) if ok else \
            (None, None, ok, None, None)
        m1 = tuple(np.array(x) for x in orc.riccati_expand(
            *a, p["Qf"][i], T, 0, lm_lambda=LM1, w_stage=W_STAGE, wrap_idx=wrap, extra=ex))
        J = orc.bruteforce_J(*a, p["Qf"][i], W_STAGE, N, lm_lambda=LM1, wrap_idx=wrap, extra=ex)
        out.append(dict(m0=m0, m1=m1, J=np.asarray(J)))
    return out


@functools.lru_cache(maxsize=None)
def reference_legacy(row):
    """the legacy oracle functions on every distinct problem (fp64, Qf = alpha I with the
    scalar alpha): m0 = (k, K, ok), m1 = (Vxx, Vx, V0, K, k, status), J, J_status"""
    p = problems(row.n, row.m)
    wrap = wrap_idx(row.n)
    out = []
    for i in range(DISTINCT):
        T = int(p["T"][i])
        a = _problem_args(p, i)
        alpha = float(p["alpha"][i])
        k, K, ok = orc.riccati_truncated_legacy(*a, alpha, T, lm_lambda=LM0, wrap_idx=wrap)
        r1 = orc.riccati_expand_legacy(*a, alpha, T, 0, lm_lambda=LM1, w_stage=W_STAGE,
                                       wrap_idx=wrap)
        J, Jst = orc.bruteforce_J(*a, alpha, W_STAGE, N, lm_lambda=LM1, wrap_idx=wrap,
                                  legacy=True, want_status=True)
        out.append(dict(m0=(np.array(k), np.array(K), ok),
                        m1=tuple(np.array(x) for x in r1[:5]) + (int(r1[5]),),
                        J=np.asarray(J), J_status=np.asarray(Jst)))
    return out


def bad_R(m):
    """negative definite: Quu_reg fails the Cholesky gate at every step"""
    return -50.0 * np.eye(m)
