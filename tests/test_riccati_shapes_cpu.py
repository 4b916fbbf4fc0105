"""CPU companion of test_gpu_riccati_shapes.py: the inputs of every row of the shape table
(tests/riccati_shapes.py) keep the oracle inside the preconditions the GPU assertions
rely on, so none of them can pass vacuously; and the table reaches both ends and an
interior of every bucket of dispatch_riccati."""
import numpy as np
import pytest

import riccati_shapes as rs
from oracle import hop_oracle as orc

ALL_ROWS = rs.TABLE + rs.WIDE_TABLE + rs.WIDE_HR8


def test_table_reaches_both_ends_and_an_interior_of_every_bucket():
    for bucket, (n0, n1, m0, m1) in rs.BUCKET_BOUNDS.items():
        rows = [r for r in rs.TABLE if r.bucket == bucket]
        assert rows, bucket
        for r in rows:
            assert n0 <= r.n <= n1 and m0 <= r.m <= m1, r
            assert r.n <= 16 and r.m <= 16
        shapes = {(r.n, r.m) for r in rows}
        assert (n0, m0) in shapes and (n1, m1) in shapes, bucket
        if n1 - n0 >= 2:
            assert any(n0 < n < n1 for n, _ in shapes), bucket
        if m1 - m0 >= 2:
            assert any(m0 < m < m1 for _, m in shapes), bucket
        assert any(r.extra for r in rows) or bucket == "fast", bucket  # the fast kernel has none
    # (12, 4) runs fast by default and <12,4> under force_generic or with the extra cost
    at = {(r.bucket, r.force_generic, r.extra) for r in rs.TABLE if (r.n, r.m) == (12, 4)}
    assert at == {("fast", False, False), ("<12,4>", True, False), ("<12,4>", False, True)}
    for r in rs.TABLE:  # no other row can reach the exact-size kernel
        assert (r.bucket == "fast") == ((r.n, r.m) == (12, 4) and not r.force_generic
                                        and not r.extra), r
    assert {r.bucket for r in rs.FAILURE_ROWS} >= set(rs.BUCKET_BOUNDS)
    assert len({r.id for r in ALL_ROWS}) == len(ALL_ROWS)


def test_batch_layout():
    idx = rs.batch_index()
    assert len(idx) == rs.BATCH == 19 and rs.BATCH > 16 and rs.BATCH % 16 == 3
    assert sorted(set(idx.tolist())) == list(range(rs.DISTINCT))
    assert sorted(set(rs.HORIZONS)) == [1, 2, rs.N // 2, rs.N - 1, rs.N]
    b = rs.batch(rs.BY_ID["<8,4>-7x3-extra"])
    assert b["T"].tolist() == [rs.HORIZONS[i] for i in idx]  # a repeat keeps its horizon
    assert np.array_equal(b["A"][0], b["A"][5]) and not np.array_equal(b["A"][0], b["A"][1])
    assert b["cxx"].shape == (rs.BATCH, rs.N, 7, 7)
    assert b["T"][rs.BAD_ROW] == rs.N
    # the whole turns on the wrapped states are seen by the wrap and by nothing else
    p = rs.problems(7, 3)
    e = p["X"][1] - p["xg"][1]
    assert (np.abs(e[:, [0, 6]]) > np.pi).all()
    assert (np.abs(orc.wrap_angles(e, rs.wrap_idx(7))) < np.pi).all()


def _norms(x):
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(np.sum(x.reshape(x.shape[0], -1) ** 2, axis=1))


@pytest.mark.parametrize("row,dtype", [(r, d) for r in ALL_ROWS for d in ("f64", "f32")
                                       if d == "f64" or not r.bucket.startswith("wide")],
                         ids=lambda v: v if isinstance(v, str) else v.id)
def test_reference_is_inside_the_preconditions(row, dtype):
    """ok at horizon 1 and N, finite expansions and J with and without the extra cost,
    every per-step reference norm > 0 (assert_per_step takes its relative branch); the
    wide entries are float64 only"""
    p = rs.problems(row.n, row.m, dtype)
    wrap = rs.wrap_idx(row.n)
    for extra in (False, True):
        r = row._replace(extra=extra)
        for i, ref in enumerate(rs.reference(r, dtype)):
            T = int(p["T"][i])
            k, K, ok, Vxx, Vx = ref["m0"]
            assert ok is True, (r.id, i)
            for T2 in (1, rs.N):
                assert orc.riccati_truncated(
                    list(p["A"][i]), list(p["B"][i]), p["X"][i], p["U"][i], p["xg"][i],
                    p["ur"][i], p["Q"][i], p["R"][i], p["Qf"][i], T2, lm_lambda=rs.LM0,
                    wrap_idx=wrap, extra=rs.extra_callable(r, i, dtype))[2] is True
            assert K.shape == (T, row.m, row.n) and Vxx.shape == (T + 1, row.n, row.n)
            for name, x in (("k", k), ("K", K), ("Vxx", Vxx), ("Vx", Vx)):
                assert np.isfinite(x).all() and (_norms(x) > 0).all(), (r.id, i, name)
            Vxx1, Vx1, V01, K1, k1 = ref["m1"]
            assert V01.shape == (T + 1,)
            for name, x in (("k1", k1), ("K1", K1), ("Vxx1", Vxx1), ("Vx1", Vx1), ("V0", V01)):
                assert np.isfinite(x).all() and (_norms(x) > 0).all(), (r.id, i, name)
            J = ref["J"]
            assert J.shape == (rs.N,) and np.isfinite(J).all() and (np.abs(J) > 0).all()
            # the 1e-9 bar on V0 and J sees a stage term that is off by 1e-5
            shift = rs.W_STAGE * 1e-5
            assert shift / abs(V01[0]) >= 10 * rs.BAR64_V0, (r.id, i, V01[0])
            assert (shift * np.arange(1, rs.N + 1) / np.abs(J) >= 10 * rs.BAR64_V0).all()


@pytest.mark.parametrize("row", rs.FAILURE_ROWS, ids=lambda r: r.id)
def test_failure_row_fails_in_the_oracle(row):
    p = rs.problems(row.n, row.m)
    i = int(rs.batch_index()[rs.BAD_ROW])
    a = (list(p["A"][i]), list(p["B"][i]), p["X"][i], p["U"][i], p["xg"][i], p["ur"][i],
         p["Q"][i], rs.bad_R(row.m), p["Qf"][i])
    assert orc.riccati_truncated(*a, int(p["T"][i]), lm_lambda=rs.LM0,
                                 wrap_idx=rs.wrap_idx(row.n))[2] is False
    with pytest.raises(np.linalg.LinAlgError):
        orc.bruteforce_J(*a, rs.W_STAGE, rs.N, lm_lambda=rs.LM1, wrap_idx=rs.wrap_idx(row.n))


def test_legacy_oracle_never_reaches_lstsq(monkeypatch):
    def no_lstsq(*a, **k):
        raise AssertionError("the legacy chol_solve fell back to lstsq")
    monkeypatch.setattr(orc.np.linalg, "lstsq", no_lstsq)
    assert len(rs.LEGACY_ROWS) >= 20 and all(r.m <= 11 and r.n <= 16 for r in rs.LEGACY_ROWS)
    for row in rs.LEGACY_ROWS:
        for i, ref in enumerate(rs.reference_legacy.__wrapped__(row)):
            assert ref["m0"][2] is True, (row.id, i)
            assert ref["m1"][5] == 0 and not ref["J_status"].any(), (row.id, i)
            for x in ref["m0"][:2] + ref["m1"][:5]:
                assert np.isfinite(x).all() and (_norms(x) > 0).all(), (row.id, i)
            assert np.isfinite(ref["J"]).all() and (np.abs(ref["J"]) > 0).all()


@pytest.mark.parametrize("row_id", ["<4,4>-3x2", "fast-12x4", "<16,16>-9x7"])
def test_oracle_own_error_vs_40_digit(row_id):
    """what the 1e-9 bar on V0 and J rests on: the fp64 oracle is within 1e-12 of the
    40-digit recursion on these inputs (per step, the longest horizon)"""
    from gain_check import per_step_rel
    from riccati_hp import riccati_hp
    row = rs.BY_ID[row_id]
    p = rs.problems(row.n, row.m)
    i = rs.DISTINCT - 1
    T = int(p["T"][i])
    assert T == rs.N
    Vxx, Vx, V0, K = riccati_hp(list(p["A"][i]), list(p["B"][i]), p["X"][i], p["U"][i],
                                p["xg"][i], p["ur"][i], p["Q"][i], p["R"][i], p["Qf"][i], T,
                                rs.LM1, mode=1, w_stage=rs.W_STAGE, wrap_idx=rs.wrap_idx(row.n))
    ref = rs.reference(row)[i]
    errs = {name: per_step_rel(got, hp)[0] for name, got, hp in
            (("Vxx", ref["m1"][0], Vxx), ("Vx", ref["m1"][1], Vx), ("V0", ref["m1"][2], V0),
             ("K", ref["m1"][3], K))}
    errs["J"] = abs(ref["J"][T - 1] - V0[0]) / abs(V0[0])
    print(row_id, errs)
    assert max(errs.values()) <= 1e-12, errs
