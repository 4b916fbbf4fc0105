"""The s = 13, m = 4 fp64 conditioned kernels' step loop at the shapes where its
bookkeeping can go wrong: odd and even horizons down to N = 1, ragged waves, prefixes of
an allocation, the first flagged horizon of the hand-over word at every step of the
first two pairs, the forced hand-over at an odd N, and the packed kernel (two waves per
SIMD) at B = 16 x CUs + 4.

Inputs: synthetic blocks from synth.device_batch (one draw per layout, shared and left
unchanged: every case clones what it edits).  J is held to the CPU oracle at 1e-12
relative (the oracle's NumPy inverses and the kernel agree to ~1e-14 on these
well-conditioned blocks, smoke(): 1.9e-14 at N = 24; 1e-12 leaves two digits for the
8 steps' growth; measured 3.1e-15 at B = 5 and 1.6e-14 on the packed batch); everything
else is bitwise.

A bad block is a stage or terminal block with entry (5, 5) = -1 (indefinite: pivot 5 of
either sweep is negative, finite inputs, so the triage of include/hop.h leaves the
hand-over standing), or a NaN in A_k0.  The NaN case under HOP_OPT_NO_RERUN is resolved
by the rerun launch's non-finite triage as hop.h defines it: status ST_NONFINITE, J the
conditioned kernel's before horizon k0 + 1 and NaN from there on (the triage accepts
only if the hand-over word's horizon is >= k0 + 1; an earlier flag would leave the
hand-over bit set).
"""
import numpy as np
import pytest

from oracle import hop_oracle as orc

pytestmark = pytest.mark.gpu

S, M = 13, 4
JTOL = 1e-12
BAD = 5  # the flagged problem of the B = 8 batch: row 1 of the second wave


def _np(x):
    return x.cpu().numpy()


def _oracle(args, rows=None):
    A, Bm, Q, Ri, z0, QT = (_np(x) for x in args)
    sel = slice(None) if rows is None else rows
    return orc.lft_sweep_batch(A[sel], Bm[sel], Q[sel], Ri[sel], z0, QT[sel])


def _cut(args, N):
    """The first N stages as their own allocation (n_alloc = N)."""
    A, Bm, Q, Ri, z0, QT = args
    return (A[:, :N].contiguous(), Bm[:, :N].contiguous(), Q[:, :N].contiguous(), Ri, z0,
            QT[:, :N].contiguous())


@pytest.fixture(scope="module")
def small(dev):
    """B = 8, n_alloc = 8 and the oracle's J / status for it."""
    from time_opt_ilqr_amd import synth
    args = synth.device_batch(8, S, M, 8, seed=61, device=dev)
    Jo, sto = _oracle(args)
    assert (sto == 0).all()
    return args, Jo


@pytest.fixture(scope="module")
def packed(dev):
    """B = 16 x CUs + 4 (more waves than SIMDs: the packed kernel), n_alloc = 4."""
    import torch
    from time_opt_ilqr_amd import synth
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    Bn = 16 * cus + 4
    args = synth.device_batch(Bn, S, M, 4, seed=62, device=dev)
    Jo, sto = _oracle(args)
    assert (sto == 0).all()
    return args, Jo, Bn


def _check_against_oracle(res, Jo, N, tag):
    J = _np(res.J)
    rel = float(np.max(np.abs(J - Jo[:, :N]) / np.abs(Jo[:, :N])))
    print(f"{tag}: N = {N}, B = {J.shape[0]}, max rel err of J against the oracle {rel:.3e}")
    assert _np(res.status).tolist() == [0] * J.shape[0]
    assert rel <= JTOL, (tag, N, rel)
    Ts, _ = orc.select_horizon(Jo[:, :N], 1, N)
    assert _np(res.t_star).tolist() == Ts.tolist(), (tag, N)


# 1. odd and even horizons, ragged waves ------------------------------------------------

@pytest.mark.parametrize("N", [1, 2, 3, 4, 7, 8])
def test_odd_and_even_horizons_ragged_wave(dev, small, N):
    """B = 5: one full wave and a wave with one valid row."""
    from time_opt_ilqr_amd import engine
    args, Jo = small
    a5 = tuple(x[:5].contiguous() if x.dim() > 1 else x for x in _cut(args, N))
    res = engine.propagate(*a5, t_min=1, t_max=N)
    _check_against_oracle(res, Jo[:5], N, "ragged")


# 2. prefix consistency -----------------------------------------------------------------

@pytest.mark.parametrize("n_use", range(1, 9))
def test_prefix_of_an_allocation(dev, small, n_use):
    """n_alloc = 8: J[:, :n_use] is bitwise the n_use = 8 run's; t_star / j_star are the
    first-index argmin of that row over the window."""
    import torch
    from time_opt_ilqr_amd import engine
    args, _ = small
    a5 = tuple(x[:5].contiguous() if x.dim() > 1 else x for x in args)
    full = engine.propagate(*a5, t_min=1, t_max=8)
    Jf = _np(full.J)
    windows = [(1, n_use), (n_use, n_use)]
    if n_use >= 3:
        windows.append((2, n_use - 1))
    for t_min, t_max in windows:
        res = engine.propagate(*a5, n_use=n_use, t_min=t_min, t_max=t_max)
        assert torch.equal(res.J, full.J[:, :n_use]), (n_use, t_min, t_max)
        assert _np(res.status).tolist() == [0] * 5
        win = Jf[:, t_min - 1:t_max]
        idx = np.argmin(win, axis=1)
        assert _np(res.t_star).tolist() == (idx + t_min).tolist(), (n_use, t_min, t_max)
        assert np.array_equal(_np(res.j_star), win[np.arange(5), idx]), (n_use, t_min, t_max)


# 3. first flagged horizon ----------------------------------------------------------------

def _spoil(args, kind, b, k0):
    A, Bm, Q, Ri, z0, QT = args
    if kind == "Q":
        Q = Q.clone()
        Q[b, k0, 5, 5] = -1.0
    elif kind == "QT":
        QT = QT.clone()
        QT[b, k0, 5, 5] = -1.0
    else:
        A = A.clone()
        A[b, k0, 3, 7] = float("nan")
    return (A, Bm, Q, Ri, z0, QT)


def _first_flag_case(args, N, kind, b, k0, n_use=None):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    Bn = args[0].shape[0]
    kw = dict(t_min=1, t_max=N, n_use=n_use)
    ok = torch.ones(Bn, dtype=torch.bool, device=args[0].device)
    ok[b] = False
    clean = engine.propagate(*args, **kw)
    assert int(clean.status.abs().sum()) == 0
    bad = _spoil(args, kind, b, k0)
    # the conditioned kernel alone (+ the non-finite triage)
    with _lib.options(no_rerun=True):
        alone = engine.propagate(*bad, **kw)
    st = _np(alone.status)
    assert (st[_np(ok)] == 0).all(), st[st != 0]
    assert torch.equal(alone.J[ok], clean.J[ok])
    if kind == "nanA":
        assert int(st[b]) == orc.ST_NONFINITE, int(st[b])
        assert torch.equal(alone.J[b, :k0], clean.J[b, :k0])
        assert bool(torch.isnan(alone.J[b, k0:]).all())
    else:
        low = (1 << _lib.HANDOVER_SHIFT) - 1
        assert (int(st[b]) & low) == _lib.ST_HANDOVER or _lib.dev_build(), int(st[b])
        assert int(_lib.handover_horizon(st[b:b + 1])[0]) == k0 + 1, int(st[b])
    # the default two launches: the flagged problem is the reference association's
    dflt = engine.propagate(*bad, **kw)
    with _lib.options(reference_assoc=True):
        ref = engine.propagate(*bad, **kw)
    assert torch.equal(dflt.status, ref.status)
    assert int(dflt.t_star[b]) == int(ref.t_star[b])
    if kind == "nanA":  # the triage keeps the conditioned kernel's finite prefix
        assert int(dflt.status[b]) == orc.ST_NONFINITE
        assert torch.equal(dflt.J[b, :k0], clean.J[b, :k0])
        assert bool(torch.isnan(dflt.J[b, k0:]).all()) and bool(torch.isnan(ref.J[b, k0:]).all())
        if k0 > 0:
            rel = float(((dflt.J[b, :k0] - ref.J[b, :k0]).abs() / ref.J[b, :k0].abs()).max())
            assert rel <= 1e-9, rel
        assert torch.equal(torch.isnan(dflt.j_star[b]), torch.isnan(ref.j_star[b]))
    else:
        assert torch.equal(dflt.J[b], ref.J[b])
        assert torch.equal(dflt.j_star[b], ref.j_star[b])
    assert torch.equal(dflt.J[ok], clean.J[ok])
    assert torch.equal(dflt.t_star[ok], clean.t_star[ok])
    assert torch.equal(dflt.j_star[ok], clean.j_star[ok])


@pytest.mark.parametrize("kind", ["Q", "QT", "nanA"])
@pytest.mark.parametrize("N", [5, 6])
@pytest.mark.parametrize("k0", [0, 1, 2, 3])
def test_first_flagged_horizon(dev, small, k0, N, kind):
    """One bad block at step k0 of one problem of a B = 8 batch: the hand-over word
    carries horizon k0 + 1, the other rows of its wave and the other wave are untouched,
    and the default two launches give the reference association's result for it."""
    args, _ = small
    _first_flag_case(_cut(args, N), N, kind, BAD, k0)


# 4. forced hand-over at an odd N ---------------------------------------------------------

def test_forced_handover_odd_horizon(dev, small):
    import torch
    from time_opt_ilqr_amd import _lib, engine
    args, _ = small
    a5 = tuple(x[:5].contiguous() if x.dim() > 1 else x for x in _cut(args, 3))
    with _lib.options(force_handover=True):
        f = engine.propagate(*a5, t_min=1, t_max=3)
    with _lib.options(reference_assoc=True):
        r = engine.propagate(*a5, t_min=1, t_max=3)
    assert torch.equal(f.J, r.J) and torch.equal(f.status, r.status)
    assert torch.equal(f.t_star, r.t_star) and torch.equal(f.j_star, r.j_star)


# 5. the packed kernel --------------------------------------------------------------------

@pytest.mark.parametrize("N", [3, 4])
def test_packed_odd_and_even_horizons(dev, packed, N):
    from time_opt_ilqr_amd import engine
    args, Jo, Bn = packed
    res = engine.propagate(*args, n_use=N, t_min=1, t_max=N)
    _check_against_oracle(res, Jo, N, "packed")


@pytest.mark.parametrize("kind", ["Q", "QT", "nanA"])
@pytest.mark.parametrize("N,k0", [(3, 0), (3, 1), (3, 2), (4, 0), (4, 1), (4, 2), (4, 3)])
def test_packed_first_flagged_horizon(dev, packed, N, k0, kind):
    """The same in the last workgroup of the packed layout (problem B - 3)."""
    args, _, Bn = packed
    _first_flag_case(args, N, kind, Bn - 3, k0, n_use=N)
