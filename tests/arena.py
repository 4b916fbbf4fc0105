"""A patterned arena: the witness of tests/test_gpu_global_memory.py.

One flat byte buffer (on the device, or on the CPU for the witness's own tests) is filled
with a 64-bit pattern, and tensors are carved out of it back to back:

  | pad | view | pad | pad | view | pad | ...

  * each pad is at least the view's own size and at least PAD_MIN bytes, so an access that
    is one problem, one step or one lane off the view lands in a pad, inside the allocation;
  * each pad is an odd number of elements after an even boundary, so a view's address is
    aligned to exactly its element size (% 16 == 8 for f64, % 8 == 4 for f32 / int32): what
    include/hop.h promises to accept, and no more.  min_align= raises that to an exact
    multiple for the arguments with a documented requirement;
  * check() lists every byte range outside the views that no longer holds the pattern,
    changed() every placed input whose bits differ from what was placed, and
    written_mask() the elements of a view that do not hold the pattern (what a kernel wrote).

shim(engine) serves the allocations of time_opt_ilqr_amd.engine (outputs and workspaces)
from the arena for the duration of a `with` block; product code does not change.
"""
import contextlib
from collections import namedtuple

PATTERNS = (0x0000000000000000, 0xFFFFFFFFFFFFFFFF, 0x7FE0000000000000)
PAD_MIN = 4096
BYTE_ALIGN = 8  # uint8 allocations are workspaces that the kernels read as doubles

Stray = namedtuple("Stray", "start stop near side distance")
Stray.__doc__ = """bytes [start, stop) of the arena, outside every view, that lost the pattern;
`near` is the closest view and the range begins `distance` bytes `side` ('before' its first
byte, or 'after' its last)"""

_View = namedtuple("_View", "name start stop tensor role")


class Arena:
    def __init__(self, pattern, capacity, device="cpu"):
        import torch
        self.torch = torch
        self.pattern = int(pattern) & 0xFFFFFFFFFFFFFFFF
        self.capacity = (int(capacity) + 7) // 8 * 8
        self.device = torch.device(device)
        self._storage = torch.empty((self.capacity + 512,), dtype=torch.uint8, device=self.device)
        off = (-self._storage.data_ptr()) % 512
        self.bytes = self._storage[off:off + self.capacity]  # the arena, byte by byte
        self.base = self.bytes.data_ptr()
        signed = self.pattern - (1 << 64) if self.pattern >> 63 else self.pattern
        self.bytes.view(torch.int64).fill_(signed)
        self.views = []
        self._saved = {}
        self._cursor = 0

    # -- carving ------------------------------------------------------------
    def carve(self, shape, dtype, name=None, min_align=None, role="output"):
        """a contiguous view of `shape` and `dtype` between two pads, its address an odd
        multiple of the element size (of min_align, if given)"""
        torch = self.torch
        shape = tuple(int(v) for v in shape)
        es = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for v in shape:
            numel *= v
        if numel == 0:  # nothing to read or write: no address to speak of
            return torch.empty(shape, dtype=dtype, device=self.device)
        unit = es if min_align is None else int(min_align)
        if unit % es:
            raise ValueError(f"min_align {unit} is no multiple of the element size {es}")
        size = numel * es
        k = (max(size, PAD_MIN) + unit - 1) // unit | 1  # pad: an odd count of units
        even = (self.base + self._cursor + 2 * unit - 1) // (2 * unit) * (2 * unit) - self.base
        start = even + k * unit
        stop = start + size
        if stop + k * unit > self.capacity:
            raise MemoryError(f"arena of {self.capacity} bytes is full: {name or shape} needs "
                              f"{stop + k * unit}")
        self._cursor = stop + k * unit
        t = self.bytes[start:stop].view(dtype).view(shape)
        assert t.data_ptr() == self.base + start and t.data_ptr() % (2 * unit) == unit
        name = name or f"#{len(self.views)}:{str(dtype).replace('torch.', '')}{list(shape)}"
        self.views.append(_View(name, start, stop, t, role))
        return t

    def place(self, tensor, name=None, min_align=None, inout=False):
        """carve a view for an input and copy it in; its bits are remembered for changed()
        unless it is an in/out argument"""
        v = self.carve(tensor.shape, tensor.dtype, name, min_align, "inout" if inout else "input")
        if v.numel():
            v.copy_(tensor)
            if not inout:
                self._saved[self.views[-1].name] = v.clone()
        return v

    def find(self, tensor):
        """the view that holds `tensor`'s first byte, or None"""
        if tensor.numel() == 0:
            return None
        off = tensor.data_ptr() - self.base
        for v in self.views:
            if v.start <= off < v.stop:
                return v
        return None

    # -- the witness --------------------------------------------------------
    def _expected(self, start=0, stop=None):
        """the pattern's bytes at arena offsets [start, stop)"""
        torch = self.torch
        stop = self.capacity if stop is None else stop
        pat = torch.tensor(list(self.pattern.to_bytes(8, "little")), dtype=torch.uint8,
                           device=self.device)
        lo = start // 8 * 8
        reps = (stop - lo + 7) // 8
        return pat.repeat(reps)[start - lo:stop - lo]

    def check(self):
        """every byte range outside the carved views that no longer holds the pattern"""
        bad = self.bytes != self._expected()
        for v in self.views:
            bad[v.start:v.stop] = False
        idx = bad.nonzero().flatten().cpu().tolist()
        out, i = [], 0
        while i < len(idx):
            j = i
            while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
                j += 1
            out.append(self._locate(idx[i], idx[j] + 1))
            i = j + 1
        return out

    def _locate(self, start, stop):
        best = None
        for v in self.views:
            if stop <= v.start:
                cand = (v.start - start, v.name, "before")
            elif start >= v.stop:
                cand = (start - v.stop + 1, v.name, "after")
            else:
                continue
            if best is None or cand[0] < best[0]:
                best = cand
        if best is None:
            return Stray(start, stop, None, None, None)
        return Stray(start, stop, best[1], best[2], best[0])

    def changed(self):
        """names of the placed inputs whose bits differ from what was placed"""
        torch = self.torch
        out = []
        for v in self.views:
            if v.name in self._saved:
                a = self.bytes[v.start:v.stop]
                b = self._saved[v.name].reshape(-1).view(torch.uint8)
                if not torch.equal(a, b):
                    out.append(v.name)
        return out

    def written_mask(self, tensor):
        """bool tensor of `tensor`'s shape (a carved view): True where the element does not
        hold the pattern"""
        v = self.find(tensor)
        if v is None or v.tensor.data_ptr() != tensor.data_ptr() or \
                v.tensor.numel() != tensor.numel():
            raise ValueError("written_mask takes a whole carved view")
        es = tensor.element_size()
        diff = self.bytes[v.start:v.stop] != self._expected(v.start, v.stop)
        return diff.view(-1, es).any(dim=1).view(tensor.shape)

    # -- the allocator shim -------------------------------------------------
    def proxy(self, torch=None):
        return TorchProxy(self, torch or self.torch)

    @contextlib.contextmanager
    def shim(self, engine):
        """engine._torch() returns the proxy inside the block: empty, zeros, full, empty_like
        and zeros_like on the arena's device come out of the arena (workspaces included).
        The engine's cached constant fills are set aside, so they are made anew inside."""
        real = engine._torch
        proxy = self.proxy(real())
        const = dict(engine._CONST)
        engine._CONST.clear()
        engine._torch = lambda: proxy
        try:
            yield proxy
        finally:
            engine._torch = real
            engine._CONST.clear()
            engine._CONST.update(const)


class TorchProxy:
    """`torch`, except that the five allocation calls on the arena's device are carved from
    the arena; everything else is passed through"""

    def __init__(self, arena, torch):
        self._arena = arena
        self._torch = torch

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def _mine(self, device):
        if device is None:
            return False
        d = self._torch.device(device)
        a = self._arena.device
        return d.type == a.type and (d.index is None or a.index is None or d.index == a.index)

    def _carve(self, size, dtype):
        if len(size) == 1 and isinstance(size[0], (tuple, list, self._torch.Size)):
            size = tuple(size[0])
        dtype = dtype or self._torch.get_default_dtype()
        align = BYTE_ALIGN if dtype == self._torch.uint8 else None
        return self._arena.carve(size, dtype, min_align=align)

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device) or kw:
            return self._torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._carve(size, dtype)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device) or kw:
            return self._torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._carve(size, dtype).zero_()

    def full(self, size, fill_value, *, dtype=None, device=None, **kw):
        if not self._mine(device) or kw or dtype is None:
            return self._torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        return self._carve((size,), dtype).fill_(fill_value)

    def empty_like(self, t, **kw):
        if not self._mine(t.device) or kw:
            return self._torch.empty_like(t, **kw)
        return self._carve((tuple(t.shape),), t.dtype)

    def zeros_like(self, t, **kw):
        if not self._mine(t.device) or kw:
            return self._torch.zeros_like(t, **kw)
        return self._carve((tuple(t.shape),), t.dtype).zero_()
