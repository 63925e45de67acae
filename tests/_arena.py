"""Operands surrounded by poison: the memory model of tests/test_gpu_poisoned_memory.py.

Every other GPU test hands the library exact-size tensors from torch's caching allocator, so a load that runs past an
operand lands in a neighbouring live tensor or in allocator slack: finite bytes that are usually multiplied by a zero
weight or a masked probability.  An `Arena` is one flat device buffer in which every operand sits between two guards
filled with a pattern of the operand's own type, and every output sits inside canary bytes:

* `place(t)` copies a host tensor in, at an address that is 16-byte aligned and deliberately NOT 256-byte aligned (16
  bytes is what the 16-byte vector loads need and the only alignment include/diffsensei_hip.h states), with a guard of
  at least 320 rows of the operand's own row length and at least 4 KiB on either side - the largest tile extent of any
  kernel here is 256 x 320, so an over-read of a whole tile stays inside the arena and meets poison, not foreign memory
  (a 1-D buffer such as a workspace or a packed byte buffer has no rows: 4 KiB stand for one);
* `out(shape, ld=...)` hands out an output view pre-filled with the same pattern, optionally with a leading dimension wider
  than the row (the columns behind the row are canary too);
* `ops` is `diffsensei_amd.ops` with its own allocations (outputs, the GroupNorm workspace, statistics buffers) routed
  through `out`: the wrappers do no arithmetic, so rerouting their `torch.empty` calls moves exactly the buffers the
  library writes into canaried memory without touching the product code;
* `check()` compares every guard and canary byte with its pattern through integer views (NaN != NaN) and names the region
  that changed.

Two fills: "nan" (quiet NaN: 0x7E00 fp16, 0x7FC0 bf16, 0x7FC00000 fp32) and "loud" (1000.0).  Integer operands get two
different in-range patterns (int8 127 / -128, uint8 255 / 1, int32 and int64 1 / 2: valid as a weight, a pixel, a box
corner, a tap, a counter and - by the tests' construction - as an index whose table row holds NaN).  `place(t, fill=v)`
overrides the value for one operand.  Padding that a documented contract makes the caller's belongs to the operand: the
test writes it into the host tensor (loud finite in both runs) before placing it.

`Plain` has the same interface on ordinary tensors: the reference run every poisoned result must equal bit for bit.
"""
from __future__ import annotations

import contextlib
from typing import Optional, Sequence

import torch

GUARD_ROWS = 320
GUARD_MIN_BYTES = 4096
ROWLESS_BYTES = 4096        # what counts as one row of a 1-D buffer
ALIGN = 16

# fill name -> dtype -> (integer view type, bit pattern as a signed integer of that width)
_INT_VIEW = {torch.float16: torch.int16, torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.int8: torch.int8,
             torch.uint8: torch.uint8, torch.int32: torch.int32, torch.int64: torch.int64}


def _bits(value: float, dtype) -> int:
    return int(torch.tensor([value], dtype=dtype).view(_INT_VIEW[dtype])[0])


PATTERNS = {
    "nan": {torch.float16: 0x7E00, torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000, torch.int8: 127, torch.uint8: 255,
            torch.int32: 1, torch.int64: 1},
    "loud": {torch.float16: _bits(1000.0, torch.float16), torch.bfloat16: _bits(1000.0, torch.bfloat16),
             torch.float32: _bits(1000.0, torch.float32), torch.int8: -128, torch.uint8: 1, torch.int32: 2, torch.int64: 2},
}


class _TorchShim:
    """`torch` as diffsensei_amd/ops.py sees it while an arena is allocating: empty / empty_like / zeros come out of the arena."""

    def __init__(self, arena: "Arena"):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def _shape(shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return tuple(int(s) for s in shape)

    def empty(self, *shape, dtype=torch.float32, device=None):
        return self._arena.out(self._shape(shape), dtype=dtype)

    def empty_like(self, t):
        return self._arena.out(tuple(t.shape), dtype=t.dtype)

    def zeros(self, *shape, dtype=torch.float32, device=None):
        return self._arena.out(self._shape(shape), dtype=dtype).zero_()


class _OpsProxy:
    """`diffsensei_amd.ops` whose allocations are the arena's for the duration of each call."""

    def __init__(self, arena: "Arena"):
        from diffsensei_amd import ops
        self._ops, self._shim = ops, _TorchShim(arena)

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if not callable(fn):
            return fn

        def call(*a, **kw):
            saved = self._ops.torch
            self._ops.torch = self._shim
            try:
                return fn(*a, **kw)
            finally:
                self._ops.torch = saved
        return call


class Arena:
    plain = False

    def __init__(self, device, fill: str, capacity: int = 96 << 20):
        assert fill in PATTERNS, fill
        self.fill, self.dev = fill, torch.device(device)
        self.buf = torch.empty(capacity + 256, dtype=torch.uint8, device=self.dev)
        self.buf.view(torch.int16).fill_(PATTERNS[fill][torch.float16])
        self.base = self.buf.data_ptr()
        self.top = 0
        self.regions = []          # (name, integer view of the guard / canary bytes, pattern)
        self.ops = _OpsProxy(self)

    # ---- patterns
    def pattern(self, dtype, fill=None) -> int:
        return PATTERNS[self.fill][dtype] if fill is None else _bits(fill, dtype)

    def poison(self, shape, dtype) -> torch.Tensor:
        """A host tensor of this run's poison: for rows of an operand that production leaves unwritten (KV-cache rows
        past the sequence, the neighbours of a column slice)."""
        t = torch.empty(tuple(shape), dtype=dtype)
        t.view(_INT_VIEW[dtype]).fill_(self.pattern(dtype))
        return t

    # ---- carving
    def _carve(self, nbytes: int, row_bytes: int, offset_bytes: int, what: str):
        guard = max(GUARD_ROWS * row_bytes, GUARD_MIN_BYTES)
        guard = (guard + 255) // 256 * 256
        start = self.top + guard
        addr = self.base + start
        start += (-addr) % 256 + offset_bytes                      # absolute address = 256 k + offset_bytes
        end = start + nbytes
        if end + guard + 16 > self.buf.numel():
            raise MemoryError(f"arena: {what} needs {end + guard + 16} bytes, the buffer has {self.buf.numel()}")
        lo = self.top
        self.top = (end + guard + 15) // 16 * 16                   # the next region starts behind this one's back guard
        assert (self.base + start) % ALIGN == 0 and (offset_bytes % 256 == 0 or (self.base + start) % 256 != 0)
        return lo, start, end, guard

    def _fill_guard(self, name: str, lo: int, hi: int, dtype, pattern: int):
        es = torch.empty(0, dtype=dtype).element_size()
        lo = (lo + es - 1) // es * es
        hi = hi // es * es
        if hi <= lo:
            return
        v = self.buf[lo:hi].view(_INT_VIEW[dtype])
        v.fill_(pattern)
        self.regions.append((name, v, pattern))

    def _view(self, start: int, numel: int, dtype):
        es = torch.empty(0, dtype=dtype).element_size()
        return self.buf[start:start + numel * es].view(dtype)

    def place(self, t: torch.Tensor, offset_bytes: int = ALIGN, fill=None, name: Optional[str] = None) -> torch.Tensor:
        """Copy the host tensor `t` into the arena between two guards; returns the contiguous device view."""
        t = t.contiguous()
        name = name or f"operand {len(self.regions) // 2} {tuple(t.shape)} {t.dtype}"
        es = t.element_size()
        row = (t.shape[-1] if t.dim() else 1) * es
        if t.dim() < 2:
            row = min(row, ROWLESS_BYTES)
        lo, start, end, guard = self._carve(t.numel() * es, row, offset_bytes, name)
        pat = self.pattern(t.dtype, fill)
        self._fill_guard(f"guard in front of {name}", lo, start, t.dtype, pat)
        view = self._view(start, t.numel(), t.dtype).view(t.shape)
        view.copy_(t)
        self._fill_guard(f"guard behind {name}", end, end + guard, t.dtype, pat)
        return view

    def out(self, shape: Sequence[int], ld: Optional[int] = None, dtype=torch.float16, offset_bytes: int = ALIGN,
            name: Optional[str] = None) -> torch.Tensor:
        """An output view inside canary bytes, itself pre-filled with the pattern.  `ld` > shape[-1]: a 2-D view
        [rows, shape[-1]] with row stride ld whose columns behind the row are canary as well."""
        shape = tuple(int(s) for s in shape)
        cols = shape[-1] if shape else 1
        rows = 1
        for s in shape[:-1]:
            rows *= s
        ld = cols if ld is None else int(ld)
        assert ld >= cols
        name = name or f"output {len(self.regions) // 2} {shape} {dtype}"
        es = torch.empty(0, dtype=dtype).element_size()
        lo, start, end, guard = self._carve(rows * ld * es, min(ld * es, ROWLESS_BYTES) if len(shape) < 2 else ld * es, offset_bytes, name)
        pat = self.pattern(dtype)
        self._fill_guard(f"canary in front of {name}", lo, start, dtype, pat)
        block = self._view(start, rows * ld, dtype)
        block.view(_INT_VIEW[dtype]).fill_(pat)
        self._fill_guard(f"canary behind {name}", end, end + guard, dtype, pat)
        if ld == cols:
            return block.view(shape)
        block = block.view(rows, ld)
        self.regions.append((f"canary columns {cols}..{ld} of {name}", block[:, cols:].view(_INT_VIEW[dtype]), pat))
        return block[:, :cols]

    # ---- verdict
    def check(self) -> None:
        """Every guard and canary byte still holds its pattern; raises naming the first region that changed."""
        if not self.regions:
            return
        bad = torch.stack([(v != p).any() for _, v, p in self.regions]).cpu().tolist()
        for (name, v, p), b in zip(self.regions, bad):
            if b:
                idx = int((v != p).reshape(-1).nonzero()[0])
                raise AssertionError(f"arena ({self.fill}): {name} was written: element {idx} of {v.numel()} no longer "
                                     f"holds the pattern {p:#x}")


class Plain:
    """The same interface on ordinary tensors from torch's allocator (the plain call)."""
    plain = True
    fill = "plain"

    def __init__(self, device):
        from diffsensei_amd import ops
        self.dev, self.ops = torch.device(device), ops

    def poison(self, shape, dtype) -> torch.Tensor:
        return torch.zeros(tuple(shape), dtype=dtype)

    def place(self, t: torch.Tensor, offset_bytes: int = ALIGN, fill=None, name=None) -> torch.Tensor:
        return t.contiguous().to(self.dev).clone()

    def out(self, shape, ld=None, dtype=torch.float16, offset_bytes: int = ALIGN, name=None) -> torch.Tensor:
        shape = tuple(int(s) for s in shape)
        if ld is None or ld == shape[-1]:
            return torch.zeros(shape, dtype=dtype, device=self.dev)
        rows = 1
        for s in shape[:-1]:
            rows *= s
        return torch.zeros((rows, int(ld)), dtype=dtype, device=self.dev)[:, :shape[-1]]

    def check(self) -> None:
        pass


@contextlib.contextmanager
def options(lib, opts):
    """ds_set_option(key, value) for every pair, restored afterwards to the defaults of include/diffsensei_hip.h: 0, except
    those listed here."""
    defaults = {"ip_attn_min_blocks": 1024, "gemm_pp_even": 1, "conv_deep_blocks": 1}
    try:
        for k, v in opts:
            assert lib.ds_set_option(k.encode(), int(v)) == 0, (k, v, lib.ds_last_error())
        yield
    finally:
        for k, _ in opts:
            lib.ds_set_option(k.encode(), defaults.get(k, 0))
