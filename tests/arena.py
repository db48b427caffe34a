"""One allocation, many buffers: the memory harness of tests/test_memory_contract_gpu.py (a plain module, no fixtures).

Every tensor a case passes to the library is a view into ONE torch.uint8 allocation, with a red zone of `guard` bytes in
front of it and behind it, at a base address whose remainder modulo 16 the case chooses.  Three things become visible
that separate torch allocations hide:

  * a store outside a buffer changes a red zone, which check() compares bit for bit with what poison() wrote there;
  * a load outside a buffer, or of a pad entry [..., D:] of a pixel-major volume, that reaches a result makes the result
    depend on the fill: run_twice() runs a case under two fills and compares the outputs bit for bit.  Fill A is -inf
    (0xFF800000; bytes 0xFF for integer and byte buffers): it wins every minimum.  Fill B is a NaN (0x7FC00001; bytes
    0x00 for integer and byte buffers): it poisons every sum, and as an integer it is as different from A as a word gets;
  * a base address that is a multiple of 4 and not of 16 (take(base_mod16=4 / 8 / 12)).

What the harness does NOT see.  The guard is 64 KiB by default: an access further than that from its buffer lands in
another buffer's red zone (still caught as a write, attributed to the wrong buffer) or in another buffer's contents (a
write there is caught only if it changes a result; a read only if the two runs hold different data there - inputs are the
same in both runs, so it is not).  A whole-row overrun of the widest pixel-major row used (775 x 772 x 4 bytes) is
therefore not covered; element, pixel and lane overruns are.  A read that does not change a result is invisible by
construction, and so is a write of the value that already stood there.

Everything poison() and check() touch lies inside the arena's own allocation."""
import numpy as np
import torch

GUARD = 65536
FILLS = ("A", "B")
_FLOAT_FILL = {"A": 0xFF800000, "B": 0x7FC00001}
_BYTE_FILL = {"A": 0xFF, "B": 0x00}


def _as_i32(pattern):
    return int(np.array([pattern], np.uint32).view(np.int32)[0])


def fill_tensor(t, fill):
    """Every element of `t` (any view of a 4-byte or 1-byte type) := fill "A" or "B"."""
    if t.dtype.is_floating_point:
        assert t.element_size() == 4
        t.view(torch.int32).fill_(_as_i32(_FLOAT_FILL[fill]))       # (a same-size dtype view keeps any strides)
    elif t.element_size() == 4:
        t.fill_(_as_i32(_BYTE_FILL[fill] * 0x01010101))
    else:
        assert t.element_size() == 1
        t.fill_(_BYTE_FILL[fill])


def holds_fill(t, fill):
    """True when every element of `t` still has the fill's bits."""
    want = torch.empty_like(t)
    fill_tensor(want, fill)
    return bool(torch.equal(t.contiguous().view(torch.uint8), want.contiguous().view(torch.uint8)))


class Violation(AssertionError):
    pass


class _Entry(object):
    def __init__(self, name, start, nbytes, guard, tensor, pads_from, is_float, output):
        self.name, self.start, self.nbytes, self.guard = name, start, nbytes, guard
        self.tensor, self.pads_from, self.is_float, self.output = tensor, pads_from, is_float, output


class Arena(object):
    """Arena(nbytes, device): one torch.uint8 allocation (`base`) that take() carves views out of."""

    def __init__(self, nbytes, device, fill=None):
        self.base = torch.zeros((int(nbytes),), dtype=torch.uint8, device=device)
        self.entries = []
        self.fill = fill          # what poison() uses when called without an argument (run_twice sets it)
        self._cursor = 0
        self._expect = None       # the bytes poison() wrote into the red zones, over the whole arena
        self._is_guard = None

    # ---- carving ----------------------------------------------------------------------------------------------------
    def take(self, shape, dtype, base_mod16=0, guard=GUARD, name=None, pads_from=None, output=False):
        """A contiguous view of `shape` / `dtype` whose data_ptr() % 16 == base_mod16, with `guard` bytes of red zone on
        either side.  pads_from=D declares the tensor pad-bearing: poison() fills [..., D:], and run_twice() compares
        [..., :D] only.  output=True: poison() fills the whole tensor (so an entry the call leaves unwritten differs
        between the two runs)."""
        if base_mod16 not in (0, 4, 8, 12):
            raise ValueError("base_mod16 must be 0, 4, 8 or 12")
        if guard % 16 != 0 or guard <= 0:
            raise ValueError("the guard is a positive multiple of 16 bytes")
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        itemsize = torch.empty((), dtype=dtype).element_size()
        if base_mod16 % itemsize != 0:
            raise ValueError("base_mod16=%d is below the alignment of %s" % (base_mod16, dtype))
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        ptr = self.base.data_ptr()
        start = self._cursor + guard
        start += (-(ptr + start)) % 16 + base_mod16
        end = start + nbytes
        if end + guard > self.base.numel():
            raise MemoryError("arena of %d bytes is full (%d more needed)" % (self.base.numel(), end + guard - self._cursor))
        t = self.base[start:end].view(dtype).view(shape)
        assert t.data_ptr() % 16 == base_mod16 and t.is_contiguous()
        self._cursor = end + guard
        e = _Entry(name or "buffer%d" % len(self.entries), start, nbytes, guard, t, pads_from,
                   dtype.is_floating_point, output)
        self.entries.append(e)
        return t

    def put(self, array, base_mod16=0, guard=GUARD, name=None, pads_from=None):
        """take() and copy a host array (NumPy or torch) in."""
        src = torch.from_numpy(np.ascontiguousarray(array)) if isinstance(array, np.ndarray) else array
        t = self.take(tuple(src.shape), src.dtype, base_mod16, guard, name, pads_from)
        t.copy_(src)
        return t

    def entry_of(self, tensor):
        for e in self.entries:
            if e.tensor is tensor or e.tensor.data_ptr() == tensor.data_ptr():
                return e
        raise KeyError("not a tensor of this arena")

    # ---- poisoning --------------------------------------------------------------------------------------------------
    def _fill_bytes(self, lo, hi, is_float, fill):
        """Bytes [lo, hi) of the arena := the fill.  Float patterns are laid on absolute 4-byte boundaries."""
        if hi <= lo:
            return
        if not is_float:
            self.base[lo:hi].fill_(_BYTE_FILL[fill])
            return
        word = np.array([_FLOAT_FILL[fill]], np.uint32).view(np.uint8)
        phase = (self.base.data_ptr() + lo) % 4
        if phase == 0 and (hi - lo) % 4 == 0 and lo % 4 == 0:
            self.base[lo:hi].view(torch.int32).fill_(_as_i32(_FLOAT_FILL[fill]))
            return
        pattern = torch.from_numpy(np.resize(np.roll(word, -phase), hi - lo).copy()).to(self.base.device)
        self.base[lo:hi].copy_(pattern)

    def poison(self, fill=None):
        """The fill into every red zone, into [..., D:] of every pad-bearing tensor and into the whole of every output."""
        fill = fill or self.fill
        if fill not in FILLS:
            raise ValueError("fill must be 'A' or 'B'")
        self.fill = fill
        for e in self.entries:
            self._fill_bytes(e.start - e.guard, e.start, e.is_float, fill)
            self._fill_bytes(e.start + e.nbytes, e.start + e.nbytes + e.guard, e.is_float, fill)
            if e.output:
                self._fill_bytes(e.start, e.start + e.nbytes, e.is_float, fill)
            elif e.pads_from is not None:
                self.fill_tensor(e.tensor[..., e.pads_from:], fill)
        self._expect = self.base.clone()
        self._is_guard = torch.zeros_like(self.base, dtype=torch.bool)
        for e in self.entries:
            self._is_guard[e.start - e.guard:e.start] = True
            self._is_guard[e.start + e.nbytes:e.start + e.nbytes + e.guard] = True

    def fill_tensor(self, t, fill=None):
        fill_tensor(t, fill or self.fill)

    def holds_fill(self, t, fill=None):
        return holds_fill(t, fill or self.fill)

    # ---- checking ---------------------------------------------------------------------------------------------------
    def check(self):
        """Every red zone still holds its fill, bit for bit; otherwise Violation names the buffer, the side and the first
        and the last touched byte, as offsets relative to the buffer's first byte."""
        if self._expect is None:
            raise RuntimeError("check() before poison()")
        if self.base.is_cuda:
            torch.cuda.synchronize(self.base.device)
        bad = (self.base != self._expect) & self._is_guard
        if not bool(bad.any()):
            return
        found = []
        for e in self.entries:
            for side, lo, hi in (("before", e.start - e.guard, e.start), ("after", e.start + e.nbytes, e.start + e.nbytes + e.guard)):
                idx = torch.nonzero(bad[lo:hi]).flatten()
                if idx.numel():
                    found.append("%s (%d bytes): red zone %s it written, bytes %+d .. %+d relative to the buffer"
                                 % (e.name, e.nbytes, side, int(idx[0]) + lo - e.start, int(idx[-1]) + lo - e.start))
        raise Violation("red zones changed (fill %s):\n  %s" % (self.fill, "\n  ".join(found)))


def _host_bits(t):
    a = t.detach().contiguous().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _defined(bits, how):
    if how is None:
        return bits
    if isinstance(how, (int, np.integer)):
        return bits[..., :int(how)]
    return bits[np.asarray(how, bool)]


def run_twice(case, nbytes, device):
    """case(arena) -> {name: tensor | (tensor, defined)} builds its buffers with arena.take() / put(), calls
    arena.poison() once they hold their inputs, launches, and returns its outputs.  `defined`: None (every entry), an int
    D ([..., :D]) or a boolean mask; a bare tensor that take() knows as pad-bearing is compared on [..., :D].  The case
    runs on a fresh arena under fill A and under fill B; check() follows each run; the outputs must have the same bits
    on every defined entry.  Returns ({name: host array} under A, the same under B): whole tensors, pads included."""
    runs = []
    for fill in FILLS:
        arena = Arena(nbytes, device, fill=fill)
        outs = case(arena)
        assert arena._expect is not None, "the case never called arena.poison()"
        arena.check()
        got = {}
        for name, v in outs.items():
            t, how = v if isinstance(v, tuple) else (v, None)
            if how is None:
                try:
                    how = arena.entry_of(t).pads_from
                except KeyError:
                    how = None
            got[name] = (_host_bits(t), how, t.detach().contiguous().cpu().numpy())
        runs.append(got)
        del arena
    a, b = runs
    differ = []
    for name in a:
        x, y = _defined(a[name][0], a[name][1]), _defined(b[name][0], b[name][1])
        if x.shape != y.shape or not np.array_equal(x, y):
            n = int((x != y).sum()) if x.shape == y.shape else -1
            differ.append("%s: %d of %d defined entries depend on the fill" % (name, n, x.size))
    if differ:
        raise Violation("outputs differ between fill A and fill B:\n  " + "\n  ".join(differ))
    return {k: v[2] for k, v in a.items()}, {k: v[2] for k, v in b.items()}
