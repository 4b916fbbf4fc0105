"""The witness of tests/test_gpu_global_memory.py, tested on CPU tensors: a GPU case must
not be able to pass because the arena saw nothing."""
import types

import pytest
import torch

from arena import BYTE_ALIGN, PAD_MIN, PATTERNS, Arena


def _arena(pattern=PATTERNS[2], capacity=1 << 20):
    return Arena(pattern, capacity, "cpu")


@pytest.mark.parametrize("pattern", PATTERNS)
def test_views_have_exactly_the_minimal_alignment(pattern):
    a = _arena(pattern)
    f64 = a.carve((5, 5, 13, 13), torch.float64)
    f32 = a.carve((3, 7), torch.float32)
    i32 = a.carve((5,), torch.int32)
    one = a.carve((1,), torch.float64)
    ws = a.carve((1000,), torch.uint8, min_align=256)
    assert f64.data_ptr() % 16 == 8 and one.data_ptr() % 16 == 8
    assert f32.data_ptr() % 8 == 4 and i32.data_ptr() % 8 == 4
    assert ws.data_ptr() % 512 == 256
    for t in (f64, f32, i32, one, ws):
        assert t.is_contiguous()
    # back to back, each between two pads of at least its own size and PAD_MIN
    end = 0
    for v in a.views:
        size = v.stop - v.start
        assert v.start - end >= max(size, PAD_MIN)
        end = v.stop + max(size, PAD_MIN)
    assert a.capacity >= end
    assert a.carve((0, 4), torch.float64).numel() == 0 and len(a.views) == 5


@pytest.mark.parametrize("pattern", PATTERNS)
def test_pads_and_fresh_views_hold_the_pattern(pattern):
    a = _arena(pattern)
    v = a.carve((7, 3), torch.float64)
    w = a.carve((9,), torch.int32)
    x = a.carve((9,), torch.float32)  # a 4-byte view sees the half of the word it lies on
    assert a.check() == []
    words = a.bytes.view(torch.int64)
    signed = pattern - (1 << 64) if pattern >> 63 else pattern
    assert bool((words == signed).all())
    for t in (v, w, x):
        assert not bool(a.written_mask(t).any())
    v[2, 1] = 1.5
    w[4] = 3
    m = a.written_mask(v)
    assert m.shape == v.shape and m.sum() == 1 and bool(m[2, 1])
    assert a.written_mask(w).nonzero().flatten().tolist() == [4]
    assert a.check() == []  # writes inside a view are not stray


def test_a_result_equals_at_most_two_patterns():
    """an int32 0 or a float 0.0 holds the zero pattern and the low half of the third, so
    the written mask of a case is the union over the three runs"""
    hit = []
    for pattern in PATTERNS:
        a = _arena(pattern)
        w = a.carve((2,), torch.int32)
        w.zero_()
        hit.append(a.written_mask(w).tolist())
    assert [any(h) for h in hit] == [False, True, True]
    assert all(x or y or z for x, y, z in zip(*hit))


def test_stray_writes_are_reported_with_their_location():
    a = _arena()
    a.carve((4,), torch.float64, name="first")
    v = a.carve((6, 2), torch.float64, name="J")
    a.carve((3,), torch.int32, name="status")
    view = next(x for x in a.views if x.name == "J")
    a.bytes[view.start - 8:view.start] = 1  # one element before J
    got = a.check()
    assert len(got) == 1
    assert got[0][:2] == (view.start - 8, view.start)
    assert (got[0].near, got[0].side, got[0].distance) == ("J", "before", 8)
    a.bytes[view.stop + 3] = 0x55             # one byte of the element after J
    got = a.check()
    assert [g[:2] for g in got] == [(view.start - 8, view.start), (view.stop + 3, view.stop + 4)]
    assert (got[1].near, got[1].side, got[1].distance) == ("J", "after", 4)
    a.bytes[a.capacity - 1] = 0x55            # far from everything: still found
    assert len(a.check()) == 3
    assert not bool(a.written_mask(v).any())


def test_a_changed_input_is_reported():
    a = _arena(PATTERNS[1])
    src = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    src[1, 1] = float("nan")  # compared bit for bit: a NaN equals itself
    x = a.place(src, name="X")
    h = a.place(torch.tensor([1, 2, 3], dtype=torch.int32), name="horizon")
    s = a.place(torch.zeros(3), name="state", inout=True)
    assert x.data_ptr() % 16 == 8 and h.data_ptr() % 8 == 4
    assert torch.equal(x.nan_to_num(7.0), src.nan_to_num(7.0)) and a.changed() == []
    s[0] = 4.0          # an in/out argument may change
    assert a.changed() == [] and a.check() == []
    x[2, 3] = -x[2, 3]
    assert a.changed() == ["X"]
    h[0] = 0
    assert a.changed() == ["X", "horizon"]


def test_find_and_a_full_arena():
    a = Arena(PATTERNS[0], 64 << 10, "cpu")
    v = a.carve((10,), torch.float64, name="v")
    assert a.find(v).name == "v" and a.find(v[3:]).name == "v"
    assert a.find(torch.zeros(4)) is None
    with pytest.raises(ValueError):
        a.written_mask(v[3:])
    with pytest.raises(MemoryError):
        a.carve((64 << 10,), torch.uint8)


def test_the_shim_serves_the_five_allocation_calls_and_passes_the_rest():
    a = _arena()
    const = {"kept": 1}
    eng = types.SimpleNamespace(_torch=lambda: torch, _CONST=const)
    real = eng._torch
    like = torch.ones((2, 3), dtype=torch.float32)
    with a.shim(eng) as px:
        assert eng._torch() is px and eng._CONST == {}
        eng._CONST["made inside"] = 2
        e = px.empty((4, 5), dtype=torch.float64, device="cpu")
        e2 = px.empty(7, dtype=torch.int32, device=torch.device("cpu"))
        z = px.zeros((3,), dtype=torch.int32, device="cpu")
        f = px.full((6,), 2.5, dtype=torch.float64, device="cpu")
        el = px.empty_like(like)
        zl = px.zeros_like(like)
        ws = px.empty((100,), dtype=torch.uint8, device="cpu")
        for t in (e, e2, z, f, el, zl, ws):
            assert a.find(t) is not None
        assert e.shape == (4, 5) and e2.shape == (7,) and el.shape == (2, 3)
        assert e.data_ptr() % 16 == 8 and e2.data_ptr() % 8 == 4 and el.data_ptr() % 8 == 4
        assert ws.data_ptr() % (2 * BYTE_ALIGN) == BYTE_ALIGN
        assert z.tolist() == [0, 0, 0] and f.tolist() == [2.5] * 6 and not bool(zl.any())
        assert zl.dtype == torch.float32 and el.dtype == torch.float32
        # everything else is torch's own
        assert px.float64 is torch.float64 and px.Tensor is torch.Tensor
        assert px.as_tensor is torch.as_tensor and px.cuda is torch.cuda
        t = px.as_tensor([1.0, 2.0])
        assert isinstance(t, px.Tensor) and a.find(t) is None
        assert a.find(px.empty((3,), dtype=torch.float64)) is None  # no device named
        assert a.find(px.empty((3,), dtype=torch.float64, device="meta")) is None
    assert eng._torch is real and eng._CONST == {"kept": 1}
    assert a.check() == []


def test_a_row_stride_widened_to_n_alloc_is_seen_twice():
    """what a J store at b * n_alloc + k instead of b * n_use + k does to a [B, n_use]
    output: holes inside the view and a stray range right after it"""
    a = _arena(PATTERNS[1])
    Bn, n_use, n_alloc = 5, 3, 5
    J = a.carve((Bn, n_use), torch.float64, name="J")
    a.carve((Bn,), torch.int32, name="status")
    view = a.find(J)
    flat = a.bytes[view.start:view.start + 8 * Bn * n_alloc].view(torch.float64)
    for b in range(Bn):
        for k in range(n_use):
            flat[b * n_alloc + k] = 1.0 + b + 0.1 * k
    wm = a.written_mask(J)
    assert not bool(wm.all()) and int(wm.sum()) == 9  # elements 3, 4, 8, 9, 13, 14 are holes
    got = a.check()
    assert [(g.near, g.side, g.distance) for g in got] == [("J", "after", 1), ("J", "after", 41)]
    assert got[0][:2] == (view.stop, view.stop + 24) and got[1][:2] == (view.stop + 40, view.stop + 64)
