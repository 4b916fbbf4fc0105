"""Timings of the wide fp64 path (include/hop_wide.h) on one GPU, device events, warmed.

    python tools/bench_wide.py [--batch 4096] [--N 100] [--rounds 5] [--iters 3]
                               [--only KIND[,KIND]] [--out profiles/wide_sweep.jsonl]

Writes one JSON line per measurement:
  * "wide_vs_generic": hop_lft_sweep_wide_f64 at s = 16, m = 4 against the narrow
    reference-association kernel (HOP_OPT_FORCE_GENERIC) on the same inputs, the two
    alternated round by round in this process (never rank timings from different
    processes); J compared before timing.
  * "wide_sweep": ms per sweep at s = 17, 24, 32 with m = 4 and m = 8.
  * "wide_riccati": hop_riccati_wide_f64 mode 0 at n = 31, m = 8, horizon N.
  * "wide_jcurve": hop_bruteforce_jcurve_wide_f64 at n = 31, m = 8, t_max = N (one
    launch) against the same curve from t_max successive hop_riccati_wide_f64 mode-1
    launches with horizon 1 .. t_max (reg_max_tries = 1), at B = 1 and at --batch, the two
    alternated round by round in this process; the curves are compared bit for bit
    before timing.  The row carries both ratios (loop over single launch) and the
    run-to-run spread of each side, (max - min) / median over the rounds.
  * "wide_ab" (only with --only wide_ab --ab-lib OTHER.so): another build of the library
    against this tree's on hop_riccati_wide_f64 mode 0 at n = 31 and n = 24 (m = 8), the J
    curve at n = 31 and the sweep at s = 24, m = 4: the two alternated round by round in this
    process (order flipped every round), outputs compared bit for bit; each row carries both
    sides' rounds and their spread, (max - min) / median.
--only measures the named kinds alone; the rewrite of --out replaces the rows of the
kinds measured in this run and keeps every other row.
Each line carries the FLOP and byte counts of bench.py's roofline (lft_flops /
lft_bytes / riccati_flops), the achieved TFLOP/s and GB/s, the least time either bound
allows and which one it is, and the fraction of the fp64 peak.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _timed(fn, rounds, iters):
    import torch
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms


def _roof(flops, nbytes, batch, ms, bench):
    t = ms * 1e-3
    t_flop = flops * batch / (bench.PEAK_F64_TFLOPS * 1e12)
    t_byte = nbytes * batch / (bench.PEAK_HBM_GBS * 1e9)
    return dict(flops_per_problem=flops, bytes_per_problem=nbytes,
                tflops=flops * batch / t / 1e12, gbs=nbytes * batch / t / 1e9,
                frac_fp64_peak=flops * batch / t / 1e12 / bench.PEAK_F64_TFLOPS,
                bound="fp64" if t_flop >= t_byte else "hbm",
                least_ms=max(t_flop, t_byte) * 1e3, frac_of_bound=max(t_flop, t_byte) / t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated row kinds to measure")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "wide_sweep.jsonl"))
    ap.add_argument("--ab-lib", default="", help="another build of libhop_amd.so (--only wide_ab)")
    args = ap.parse_args()
    import torch
    import bench
    from time_opt_ilqr_amd import _lib, engine, synth
    if not torch.cuda.is_available():
        raise SystemExit("bench_wide.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    Bn, N = args.batch, args.N
    rows = []
    kinds = ("wide_vs_generic", "wide_sweep", "wide_riccati", "wide_jcurve")
    only = tuple(k for k in args.only.split(",") if k) or kinds
    if set(only) - set(kinds) - {"wide_ab"}:
        raise SystemExit(f"--only takes {', '.join(kinds)}, wide_ab")
    if "wide_ab" in only and not args.ab_lib:
        raise SystemExit("--only wide_ab needs --ab-lib")

    def wide_call(A, Bm, Q, Ri, z0, QT, s, m):
        J = torch.empty((Bn, N), dtype=torch.float64, device=dev)
        st = torch.empty((Bn,), dtype=torch.int32, device=dev)
        r_bs = 0 if Ri.dim() == 2 else m * m

        def fn():
            _lib.check(_lib.load().hop_lft_sweep_wide_f64(  # the library of the moment (wide_ab)
                _lib.ptr(A), _lib.ptr(Bm), _lib.ptr(Q), _lib.ptr(Ri), r_bs, 0, 1, _lib.ptr(QT),
                _lib.ptr(z0), 0, Bn, N, N, s, m, 8, 0, 0, _lib.ptr(J), _lib.ptr(st), None, None,
                None, None, _lib.stream_handle(dev)))
        return fn, J, st

    if "wide_vs_generic" in only:
        # ---- wide against the narrow reference-association kernel at s = 16
        s, m = 16, 4
        A, Bm, Q, Ri, z0, QT = synth.device_batch(Bn, s, m, N, seed=5, device=dev)
        wfn, Jw, stw = wide_call(A, Bm, Q, Ri, z0, QT, s, m)

        def gfn():
            with _lib.options(force_generic=True):
                return engine.propagate(A, Bm, Q, Ri, z0, QT)
        wfn()
        ref = gfn()
        torch.cuda.synchronize()
        rel = float(((Jw - ref.J).abs() / ref.J.abs()).max())
        assert int(stw.abs().sum()) == 0 and int(ref.status.abs().sum()) == 0
        tw, tg = [], []
        for rnd in range(args.rounds):  # alternate, order flipped every round
            for which in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                (tw if which == 0 else tg).extend(_timed(wfn if which == 0 else gfn, 1, args.iters))
        mw, mg = statistics.median(tw), statistics.median(tg)
        rows.append(dict(kind="wide_vs_generic", s=s, m=m, N=N, batch=Bn, max_rel_J=rel,
                         wide_ms=mw, wide_ms_all=tw, generic_ms=mg, generic_ms_all=tg,
                         ratio_wide_over_generic=mw / mg,
                         wide=_roof(bench.lft_flops(N, s, m), bench.lft_bytes(N, s, m), Bn, mw, bench),
                         generic=_roof(bench.lft_flops(N, s, m), bench.lft_bytes(N, s, m), Bn, mg,
                                       bench)))
        print(json.dumps(rows[-1]), flush=True)
        del A, Bm, Q, QT

    if "wide_sweep" in only:
        # ---- wide shapes
        for s, m in ((17, 4), (17, 8), (24, 4), (24, 8), (32, 4), (32, 8)):
            A, Bm, Q, Ri, z0, QT = synth.device_batch(Bn, s, m, N, seed=5, device=dev)
            fn, J, st = wide_call(A, Bm, Q, Ri, z0, QT, s, m)
            fn()
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0 and bool(torch.isfinite(J).all())
            ms = _timed(fn, args.rounds, args.iters)
            med = statistics.median(ms)
            rows.append(dict(kind="wide_sweep", s=s, m=m, N=N, batch=Bn, ms=med, ms_all=ms,
                             **_roof(bench.lft_flops(N, s, m), bench.lft_bytes(N, s, m), Bn, med,
                                     bench)))
            print(json.dumps(rows[-1]), flush=True)
            del A, Bm, Q, QT, J

    # ---- wide Riccati, mode 0, n = 31
    n, m = 31, 8
    g = torch.Generator(device="cpu").manual_seed(11)
    rnd = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64)  # noqa: E731
    A = (torch.eye(n, dtype=torch.float64) + 0.05 * rnd(Bn, N, n, n)).to(dev)
    Bm = (0.1 * rnd(Bn, N, n, m)).to(dev)
    X = (0.5 * rnd(Bn, N + 1, n)).to(dev)
    U = (0.1 * rnd(Bn, N, m)).to(dev)
    xg, ur = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(m, dtype=torch.float64,
                                                                          device=dev)
    Qc = torch.eye(n, dtype=torch.float64, device=dev)
    Rc = 0.5 * torch.eye(m, dtype=torch.float64, device=dev)
    Qf = 10.0 * torch.eye(n, dtype=torch.float64, device=dev)
    T = torch.full((Bn,), N, dtype=torch.int32, device=dev)

    if "wide_riccati" in only:
        def rfn():
            return engine.riccati(A, Bm, X, U, xg, ur, Qc, Rc, Qf, T, 1e-3, mode=0)
        r = rfn()
        torch.cuda.synchronize()
        assert int(r.status.abs().sum()) == 0
        ms = _timed(rfn, args.rounds, args.iters)
        med = statistics.median(ms)
        rb = 8 * (N * (n * n + n * m + m + m * n + m) + (N + 1) * n)  # A, B, U in; K, k out; X
        rows.append(dict(kind="wide_riccati", mode=0, n=n, m=m, N=N, batch=Bn, ms=med, ms_all=ms,
                         **_roof(bench.riccati_flops(n, m, N, 0), rb, Bn, med, bench)))
        print(json.dumps(rows[-1]), flush=True)

    # ---- the brute-force J curve, n = 31: one launch against t_max mode-1 launches
    if "wide_jcurve" in only:
        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        def jcurve_row(b):
            a = (A[:b], Bm[:b], X[:b], U[:b], xg, ur, Qc, Rc, Qf)

            def one():
                return engine.bruteforce_jcurve_wide(*a, N, lm_lambda=1e-6, w_stage=0.5)

            def loop():
                return [engine.riccati(*a, T_, 1e-6, mode=1, w_stage=0.5, reg_max_tries=1).V0[:, 0]
                        for T_ in range(1, N + 1)]
            J, st = one()
            ref = torch.stack(loop(), 1)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0 and bool(torch.equal(J, ref))
            t1, tl = [], []
            for rnd_ in range(args.rounds):  # alternate, order flipped every round
                for which in ((0, 1) if rnd_ % 2 == 0 else (1, 0)):
                    (t1 if which == 0 else tl).extend(_timed(one if which == 0 else loop, 1, 1))
            m1, ml = statistics.median(t1), statistics.median(tl)
            return dict(batch=b, jcurve_ms=m1, jcurve_ms_all=t1, loop_ms=ml, loop_ms_all=tl,
                        ratio_loop_over_jcurve=ml / m1,
                        ratio_per_round=[x / y for x, y in zip(tl, t1)],
                        spread_jcurve=spread(t1), spread_loop=spread(tl))
        small, large = jcurve_row(1), jcurve_row(Bn)
        fl = sum(bench.riccati_flops(n, m, T_, 1) for T_ in range(1, N + 1))
        rows.append(dict(kind="wide_jcurve", n=n, m=m, N=N, t_max=N, bitwise_equal_to_loop=True,
                         b1=small, large=large,
                         tflops=fl * Bn / (large["jcurve_ms"] * 1e-3) / 1e12,
                         frac_fp64_peak=fl * Bn / (large["jcurve_ms"] * 1e-3) / 1e12
                         / bench.PEAK_F64_TFLOPS))
        print(json.dumps(rows[-1]), flush=True)

    # ---- another build of the library against this tree's, on the rows a change to the wide
    # Riccati kernel or to hop_wide_device.hpp touches
    if "wide_ab" in only:
        base = _lib.load(args.ab_lib)
        tree = _lib.load()

        def spread(v):
            return (max(v) - min(v)) / statistics.median(v)

        def ab_row(name, fn, out_of, iters, **shape):
            outs = []
            for lb in (base, tree):  # warm-up and the outputs of each side
                _lib._lib = lb
                outs.append(out_of(fn()).clone())
            torch.cuda.synchronize()
            tb, tt = [], []
            for rnd_ in range(args.rounds):  # alternate, order flipped every round
                for which in ((0, 1) if rnd_ % 2 == 0 else (1, 0)):
                    _lib._lib = base if which == 0 else tree
                    (tb if which == 0 else tt).extend(_timed(fn, 1, iters))
            _lib._lib = tree
            mb, mt = statistics.median(tb), statistics.median(tt)
            rows.append(dict(kind="wide_ab", workload=name, batch=Bn, N=N, **shape,
                             base_lib=os.path.basename(args.ab_lib), base_ms=mb, base_ms_all=tb,
                             tree_ms=mt, tree_ms_all=tt, ratio_tree_over_base=mt / mb,
                             spread_base=spread(tb), spread_tree=spread(tt),
                             bitwise_equal=bool(torch.equal(outs[0].nan_to_num(7.0),
                                                            outs[1].nan_to_num(7.0)))))
            print(json.dumps(rows[-1]), flush=True)

        ab_row("wide_riccati_mode0", lambda: engine.riccati(A, Bm, X, U, xg, ur, Qc, Rc, Qf, T, 1e-3,
                                                            mode=0), lambda r: r.K, args.iters,
               n=n, m=m)
        n2 = 24  # HR = 12, the instantiation whose padding lanes the symmetrisation read
        A2, B2 = A[:, :, :n2, :n2].contiguous(), Bm[:, :, :n2].contiguous()
        X2 = X[:, :, :n2].contiguous()
        e2 = torch.eye(n2, dtype=torch.float64, device=dev)
        ab_row("wide_riccati_mode0", lambda: engine.riccati(A2, B2, X2, U, xg[:n2], ur, e2, Rc,
                                                            10.0 * e2, T, 1e-3, mode=0),
               lambda r: r.K, args.iters, n=n2, m=m)
        ab_row("wide_jcurve", lambda: engine.bruteforce_jcurve_wide(
            A, Bm, X, U, xg, ur, Qc, Rc, Qf, N, lm_lambda=1e-6, w_stage=0.5), lambda r: r[0], 1,
            n=n, m=m, t_max=N)
        s2, m2 = 24, 4
        sw = synth.device_batch(Bn, s2, m2, N, seed=5, device=dev)
        fn, Jw, _ = wide_call(*sw, s2, m2)
        ab_row("wide_sweep", fn, lambda _r: Jw, args.iters, s=s2, m=m2)

    # rows of other kinds (counter runs, the parent benchmark, the resource table) stay
    keep = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            keep = [r for r in map(json.loads, filter(str.strip, f))
                    if r.get("kind") not in only]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        for r in rows + keep:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
