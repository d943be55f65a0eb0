"""Guard-band / poisoned-memory harness for the C-ABI kernels (a plain helper module, like gpu_util.py; works on cpu and
cuda tensors).

The parity tests hand every kernel exactly-sized tensors out of torch's caching allocator, so a write past the end of an
output, a read past the end of an input, a read of memory the kernel should have written first and an output element that is
never written all land on finite floats of some earlier test and go unnoticed.  Here every device argument of a call is one
allocation ``[front guard | payload | back guard]`` that the test owns and fills with recognisable bit patterns:

* ``Guarded``       one such argument; ``check_after()`` verifies guards, inputs and "every output element was written";
* ``run_contract``  one C-ABI call three times on fresh buffers -- plain (ordinary exact-size tensors), variant A, variant B --
                    and the outputs must be finite and bit-identical across the three runs (the library has no atomics and
                    documents every reduction as fixed-order, so the same inputs give the same bits whatever the surrounding
                    memory holds).

Variants: A = quiet NaN with a recognisable payload everywhere, payload 256-byte aligned; B = another NaN pattern in outputs
(guards and payload), a large finite value (-1e30) in the guards of inputs and in workspaces, payload at the WEAKEST alignment the
header promises for the argument (aligned to ``align`` bytes and to nothing more).  A kernel that adds a stray read into its
result therefore gives NaN in A and a huge finite number in B: never the same bits as the plain run.

Guard size is a condition, not a measurement: each guard is at least max(64 KiB, 32 slices of the tensor's outermost index)
bytes (32 = the largest row / image tile of any kernel), capped at 64 MiB.
"""
import torch

IN, OUT, INOUT, WS = "IN", "OUT", "INOUT", "WS"

MIN_GUARD = 64 << 10
MAX_GUARD = 64 << 20
GUARD_SLICES = 32

# Poison patterns (little-endian 32-bit words, tiled).  Compared as bytes, never as floats.
_NAN_A = 0x7FC5A5A5          # quiet NaN, payload 0x45A5A5
_NAN_B = 0xFFE1B00B          # another quiet NaN (sign set), payload 0x61B00B
_BIG_B = 0xF149F2CA          # fp32 -1.0e30: large, finite
_INT_A = 0x5A5A5A5A          # int32 / int64 / uint8 tensors: recognisable integers (0x5A bytes / 0xC3 bytes)
_INT_B = 0xC3C3C3C3


def _pat64(p32):
    v = (p32 << 32) | p32
    return v - (1 << 64) if v >= (1 << 63) else v


def _poison_word(dtype, variant, kind):
    """kind: "out" (outputs: guards and payload) or "in" (guards of inputs / in-out arguments, workspaces)."""
    if dtype.is_floating_point:
        if variant == "A":
            return _NAN_A
        return _NAN_B if kind == "out" else _BIG_B
    return _INT_A if variant == "A" else _INT_B


class GuardError(AssertionError):
    """What went wrong, machine-readable: .arg (argument name), .side ("front guard", "back guard", "input modified",
    "unwritten payload", "differing bits", "non-finite output"), .variant, .offset (first offending element relative to the
    payload's first element), .count (elements affected)."""

    def __init__(self, contract, arg, side, variant, offset, count, extra=""):
        self.contract, self.arg, self.side, self.variant, self.offset, self.count = contract, arg, side, variant, offset, count
        AssertionError.__init__(self, "%s: argument '%s' (run %s): %s -- first at element %+d relative to the payload, %d element(s) "
                                "affected%s" % (contract, arg, variant, side, offset, count, extra))


def guard_bytes(shape, dtype):
    """Size condition of ONE guard of a tensor."""
    item = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for s in shape:
        numel *= int(s)
    outer = int(shape[0]) if len(shape) else 1
    slice_bytes = (numel // max(outer, 1)) * item
    return min(max(MIN_GUARD, GUARD_SLICES * slice_bytes), MAX_GUARD)


def _bytes_of(t):
    return t.contiguous().view(-1).view(torch.uint8)


class Guarded:
    """One device argument: [front guard | payload | back guard] in one allocation.

    shape, dtype   the payload (exposed as the contiguous view ``.t``; its device address is ``.ptr``)
    role           IN (data given, must come back bit-identical), OUT (payload poisoned, every element under ``written`` must be
                   overwritten), INOUT (data given, result compared across runs), WS (scratch: payload poisoned, only the guards
                   are checked)
    poison         "A" / "B" (see the module docstring) or "plain": an ordinary exact-size tensor, no guards, nothing checked
    align          variant B: the payload's address is a multiple of ``align`` bytes and NOT of 2 * align
    written        OUT / INOUT: bool tensor (broadcastable to shape) of the elements the call defines; default everything
    """

    def __init__(self, shape, dtype=torch.float32, role=OUT, poison="A", data=None, align=16, written=None, name="?",
                 device="cpu"):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.dtype, self.role, self.variant, self.name, self.align, self.device = dtype, role, poison, name, int(align), device
        assert role in (IN, OUT, INOUT, WS), role
        assert poison in ("A", "B", "plain"), poison
        self.item = torch.empty((), dtype=dtype).element_size()
        assert self.align >= self.item and self.align & (self.align - 1) == 0 and self.align <= 256, (name, align)
        self.numel = 1
        for s in self.shape:
            self.numel *= s
        self.nbytes = self.numel * self.item
        if (role in (IN, INOUT)) != (data is not None):
            raise ValueError("%s: IN / INOUT arguments take data, OUT / WS do not" % name)
        self.written = None
        if written is not None:
            self.written = torch.as_tensor(written, dtype=torch.bool).expand(self.shape).contiguous().view(-1).to(device)
        if poison == "plain":
            self.guard = 0
            self.base = torch.empty(max(self.nbytes, 1), dtype=torch.uint8, device=device)
            self.start = 0
        else:
            self.guard = guard_bytes(self.shape, dtype)
            self.base = torch.empty(2 * self.guard + self.nbytes + 1024, dtype=torch.uint8, device=device)
            addr = self.base.data_ptr() + self.guard
            addr = (addr + 255) & ~255
            if poison == "B" and self.align < 256:
                addr += self.align                 # a multiple of align, an odd one: the weakest alignment promised
            self.start = addr - self.base.data_ptr()
            self.base.copy_(self._pattern(self._word()))
        self.end = self.start + self.nbytes
        self.t = self.base[self.start:self.end].view(dtype).view(self.shape) if self.numel else \
            torch.empty(self.shape, dtype=dtype, device=device)
        self.orig = None
        if data is not None:
            d = torch.as_tensor(data).detach().to(device=device, dtype=dtype).contiguous()
            assert tuple(d.shape) == self.shape, (name, tuple(d.shape), self.shape)
            self.t.copy_(d)
            self.orig = d.clone() if poison != "plain" else None
        if poison != "plain":
            assert self.start >= self.guard and self.base.numel() - self.end >= self.guard
            assert self.ptr % (256 if poison == "A" else self.align) == 0
            assert poison == "A" or self.align == 256 or self.ptr % (2 * self.align) != 0

    # ---- poison
    def _word(self):
        return _poison_word(self.dtype, self.variant, "out" if self.role == OUT else "in")

    def _pattern(self, word):
        """uint8 tensor as long as the allocation, the 8-byte pattern tiled with its phase anchored at the payload start."""
        n = self.base.numel()
        tmp = torch.empty((n + 16 + 7) // 8, dtype=torch.int64, device=self.device)
        tmp.fill_(_pat64(word))
        shift = (8 - self.start % 8) % 8
        return tmp.view(torch.uint8)[shift:shift + n]

    @property
    def ptr(self):
        return self.base.data_ptr() + self.start

    def payload_bits(self):
        return self.base[self.start:self.end]

    # ---- checks
    def _elements(self, bad_bytes, origin):
        """bad_bytes: bool over a byte range starting `origin` bytes from the payload start -> (first element offset relative to
        the payload, number of elements touched)."""
        idx = torch.nonzero(bad_bytes).view(-1) + origin
        el = torch.div(idx, self.item, rounding_mode="floor")
        return int(el[0]), int(torch.unique(el).numel())

    def poisoned(self):
        """bool [numel]: payload elements that still hold this run's poison pattern."""
        pat = self._pattern(self._word())[self.start:self.end]
        return (self.payload_bits() == pat).view(self.numel, self.item).all(dim=1)

    def check_after(self, contract="contract", peer=None):
        """Guards bit-identical to the poison; IN payload bit-identical to what was put in; OUT payload holds the poison pattern
        nowhere under its `written` mask.  With `peer` (the same argument of the other poisoned run) an output element counts as
        unwritten only when it holds the poison of BOTH runs: a result that merely carries a NaN read from somewhere else, or a
        uint8 value that happens to equal one poison byte, is left to the comparison of the runs' bits."""
        if self.variant == "plain":
            return
        pat = self._pattern(self._word())
        front = self.base[:self.start] != pat[:self.start]
        if bool(front.any()):
            off, cnt = self._elements(front, -self.start)
            raise GuardError(contract, self.name, "front guard", self.variant, off, cnt, " (a write before the argument's first element)")
        back = self.base[self.end:] != pat[self.end:]
        if bool(back.any()):
            off, cnt = self._elements(back, self.nbytes)
            raise GuardError(contract, self.name, "back guard", self.variant, off, cnt,
                             " (a write past the argument's %d elements)" % self.numel)
        if self.role == IN and self.numel:
            diff = self.payload_bits() != _bytes_of(self.orig)
            if bool(diff.any()):
                off, cnt = self._elements(diff, 0)
                raise GuardError(contract, self.name, "input modified", self.variant, off, cnt)
        if self.role == OUT and self.numel:
            un = self.poisoned()
            if peer is not None:
                un = un & peer.poisoned()
            if self.written is not None:
                un = un & self.written
            if bool(un.any()):
                idx = torch.nonzero(un).view(-1)
                raise GuardError(contract, self.name, "unwritten payload", self.variant, int(idx[0]), int(idx.numel()),
                                 " (the element still holds the poison it was filled with)")


class Alloc:
    """What `build(alloc)` allocates device arguments through.  One instance per run (plain / A / B)."""

    def __init__(self, variant, device):
        self.variant, self.device = variant, device
        self.args = []          # Guarded objects in allocation order
        self.kept = []          # host structs that must outlive the call

    def _add(self, g):
        if any(a.name == g.name for a in self.args):
            raise ValueError("argument name '%s' used twice" % g.name)
        self.args.append(g)
        return g

    @staticmethod
    def _dtype(data, dtype):
        return dtype or (data.dtype if data.dtype in (torch.uint8, torch.int32, torch.int64) else torch.float32)

    def inp(self, name, data, align=16, dtype=None):
        data = torch.as_tensor(data)
        return self._add(Guarded(data.shape, self._dtype(data, dtype), IN, self.variant, data=data, align=align, name=name,
                                 device=self.device))

    def out(self, name, shape, dtype=torch.float32, align=16, written=None):
        return self._add(Guarded(shape, dtype, OUT, self.variant, align=align, written=written, name=name, device=self.device))

    def inout(self, name, data, align=16, written=None, dtype=None):
        data = torch.as_tensor(data)
        return self._add(Guarded(data.shape, self._dtype(data, dtype), INOUT, self.variant, data=data, align=align,
                                 written=written, name=name, device=self.device))

    def ws(self, name, shape, dtype=torch.float32, align=16):
        return self._add(Guarded(shape, dtype, WS, self.variant, align=align, name=name, device=self.device))

    def keep(self, obj):
        self.kept.append(obj)
        return obj


def _cabi_call(name, args):
    from disvae_amd import _lib
    _lib.call(name, *[a.ptr if isinstance(a, Guarded) else a for a in args])


def _sync(device):
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()


def run_contract(name, build, fn=None, device="cuda", contract=None):
    """`build(alloc)` returns the argument list of ONE call of the C-ABI entry point `name`, allocating every device argument
    through `alloc` (Guarded objects stand for their device pointers; host structs are rebuilt by every build() and kept alive
    with alloc.keep()).  `fn(args)` replaces the foreign call (the host self-tests pass small Python "kernels").

    The call runs three times on fresh buffers: plain, variant A, variant B.  Then: check_after() on A and B; every OUT / INOUT
    payload, under its mask, bit-identical across the three runs and finite."""
    contract = contract or name
    runs = []
    for variant in ("plain", "A", "B"):
        al = Alloc(variant, device)
        args = build(al)
        if fn is None:
            _cabi_call(name, args)
        else:
            fn(args)
        _sync(device)
        runs.append(al)
    plain, a, b = runs
    names = [g.name for g in plain.args]
    for al in (a, b):
        if [g.name for g in al.args] != names:
            raise ValueError("%s: build() allocated different arguments in different runs" % contract)
    for ga, gb in zip(a.args, b.args):
        ga.check_after(contract, peer=gb)
        gb.check_after(contract, peer=ga)
    for gp, ga, gb in zip(plain.args, a.args, b.args):
        if gp.role not in (OUT, INOUT) or gp.numel == 0:
            continue
        ref = gp.payload_bits()
        for g in (ga, gb):
            diff = (g.payload_bits() != ref).view(g.numel, g.item).any(dim=1)
            if g.written is not None:
                diff = diff & g.written
            if bool(diff.any()):
                idx = torch.nonzero(diff).view(-1)
                i0 = int(idx[0])
                raise GuardError(contract, g.name, "differing bits", g.variant, i0, int(idx.numel()),
                                 " (plain run %r, this run %r: the result depends on memory the call does not own or did not "
                                 "write first)" % (gp.t.view(-1)[i0].item(), g.t.view(-1)[i0].item()))
        if gp.dtype.is_floating_point:
            for g in (gp, ga, gb):
                bad = ~torch.isfinite(g.t.view(-1))
                if g.written is not None:
                    bad = bad & g.written
                if bool(bad.any()):
                    idx = torch.nonzero(bad).view(-1)
                    raise GuardError(contract, g.name, "non-finite output", g.variant, int(idx[0]), int(idx.numel()))
    return runs
