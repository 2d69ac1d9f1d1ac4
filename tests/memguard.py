"""Memory around a kernel's operands: guarded outputs, poisoned inputs, written sets, poisoned free blocks.

A plain module the footprint tests import (not a conftest).  Everything here allocates through torch's caching
allocator and writes with torch ops or ``hipMemsetD32Async``: no kernel of this project is involved, so the harness
cannot share a bug with what it checks.

* :class:`Guarded` -- one allocation ``[guard | data | guard]``.  The guards and (by default) the data hold a sentinel that
  no arithmetic produces: a NaN with a payload for float types (an arithmetic NaN is the canonical quiet NaN), the byte
  0xA5 repeated for integer types.  :meth:`Guarded.check` compares the guards bit for bit and names the first changed byte
  as an offset from the data's end (``+k``: k bytes past the end) or start (``-k``: k bytes before it).
* :func:`poisoned` -- an input copied into the middle of an allocation filled with a second NaN (the poison), optionally
  as a strided view whose row gaps hold it too: a NaN that reaches an output means an over-read entered the arithmetic,
  and since arithmetic keeps a NaN's payload, such an output never looks like the untouched sentinel.
* :func:`assert_written` / :func:`assert_untouched` -- the written set of an output pre-filled with the sentinel.
* :func:`poison_free_blocks` -- every free block of the caching allocator (a graph's private pool included) filled
  with a NaN pattern on the current stream.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import torch

GUARD_BYTES = 64 * 1024
# sentinel bit patterns per element size: quiet NaNs with a payload no arithmetic produces (canonical NaNs are
# 0x7FC00000 / 0x7FC0 / 0x7E00), 0xA5 bytes for integer buffers
SENTINEL_BITS = {torch.float32: 0x7FD1CE5A, torch.bfloat16: 0x7FDA, torch.float16: 0x7E5A}
# poisoned INPUTS carry a different NaN: arithmetic keeps a NaN's payload, so an output element computed from an over-read
# holds the poison, never the sentinel (an over-read written into a pad would otherwise look untouched)
POISON_BITS = {torch.float32: 0x7FE0BAD1, torch.bfloat16: 0x7FE1, torch.float16: 0x7E61}
INT_BYTE = 0xA5
INT_POISON_BYTE = 0x5C
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(v: int, bits: int) -> int:
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def sentinel_word(dtype: torch.dtype, poison: bool = False) -> int:
    """The sentinel (``poison``: the input poison) of one element of ``dtype`` as a signed integer of the same width."""
    size = torch.empty(0, dtype=dtype).element_size()
    bits = POISON_BITS if poison else SENTINEL_BITS
    if dtype in bits:
        return _signed(bits[dtype], 8 * size)
    return _signed(int.from_bytes(bytes([INT_POISON_BYTE if poison else INT_BYTE]) * size, "little"), 8 * size)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT_VIEW[t.element_size()])


def fill_sentinel(t: torch.Tensor, poison: bool = False) -> torch.Tensor:
    _bits(t).fill_(sentinel_word(t.dtype, poison))
    return t


def is_sentinel(t: torch.Tensor) -> torch.Tensor:
    """Elementwise: does ``t`` hold its dtype's sentinel bit pattern?"""
    return _bits(t) == sentinel_word(t.dtype)


class Guarded:
    """``[guard | data | guard]`` in one allocation; ``data`` is a contiguous tensor of ``shape``.

    ``align`` = 256: the data offset is a multiple of 256 bytes; 16: a multiple of 16 that is NOT a multiple of 32
    (launchers that need only 16-byte alignment).  ``guard`` is raised to the next multiple of 256 at or above
    ``min_guard_bytes`` (and never below 64 KiB).  ``fill``: 'sentinel' (default), 'zero', or a tensor copied in.
    ``poison``: an input allocation -- guards and default fill hold the input poison instead of the sentinel."""

    def __init__(self, shape, dtype: torch.dtype, device="cuda", align: int = 256, min_guard_bytes: int = 0,
                 fill="sentinel", memory_format=None, poison: bool = False):
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        self.dtype = dtype
        self.esize = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = math.prod(self.shape) * self.esize
        g = max(GUARD_BYTES, min_guard_bytes)
        self.guard = -(-g // 256) * 256
        self.off = self.guard + (16 if align == 16 else 0)
        assert align in (16, 256)
        tail = self.guard + (-(self.off + self.nbytes)) % 8   # whole 8-byte words in the raw buffer
        self.raw = torch.empty(self.off + self.nbytes + tail, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 256 == 0
        # the guards carry the data dtype's sentinel, aligned to the data's element grid
        self.raw.fill_(INT_POISON_BYTE if poison else INT_BYTE)
        if dtype in SENTINEL_BITS:
            head = self.raw[self.off % self.esize:self.off].view(_INT_VIEW[self.esize])
            end = self.off + self.nbytes
            n_tail = (len(self.raw) - end) // self.esize
            tailv = self.raw[end:end + n_tail * self.esize].view(_INT_VIEW[self.esize])
            head.fill_(sentinel_word(dtype, poison))
            tailv.fill_(sentinel_word(dtype, poison))
        self._want = self.raw.clone()
        flat = self.raw[self.off:self.off + self.nbytes].view(dtype)
        self.data = flat.view(self.shape)
        if memory_format is torch.channels_last:
            B, Cc, Hh, Ww = self.shape
            self.data = flat.view(B, Hh, Ww, Cc).permute(0, 3, 1, 2)
        if isinstance(fill, torch.Tensor):
            self.data.copy_(fill)
        elif fill == "zero":
            self.data.zero_()
        elif fill == "sentinel":
            fill_sentinel(flat, poison)
        else:
            raise ValueError(fill)

    @property
    def ptr(self) -> int:
        return self.data.data_ptr()

    def check(self, what: str = "") -> None:
        """Both guards bit-equal to what was written at construction; raises naming the first changed byte."""
        end = self.off + self.nbytes
        for lo, hi, side in ((0, self.off, "before"), (end, len(self.raw), "after")):
            diff = (self.raw[lo:hi] != self._want[lo:hi]).nonzero()
            if diff.numel():
                i = int(diff[0]) + lo
                rel = f"+{i - end}" if side == "after" else f"-{self.off - i}"
                n_bad = int(diff.numel())
                raise AssertionError(f"{what}: guard {side} the data changed: first changed byte at {rel} bytes from "
                                     f"the data's {'end' if side == 'after' else 'start'} ({n_bad} bytes changed; "
                                     f"byte {int(self.raw[i]):#04x}, want {int(self._want[i]):#04x})")


def guarded_like(t: torch.Tensor, **kw) -> Guarded:
    """A guarded copy of ``t`` (for in-place operands and accumulating outputs that start from known values)."""
    return Guarded(t.shape, t.dtype, t.device, fill=t, **kw)


def poisoned(src: torch.Tensor, ld: Optional[int] = None, align: int = 256) -> torch.Tensor:
    """``src`` copied into the middle of an allocation filled with the input poison (a NaN, for integers 0x5C bytes).  ``ld`` (2-D
    ``src`` only): a view of row stride ``ld`` >= columns whose row gaps hold the sentinel too.  The returned tensor
    keeps its allocation alive."""
    if ld is None:
        g = Guarded(src.shape, src.dtype, src.device, align=align, fill=src, poison=True)
        t = g.data
    else:
        M, K = src.shape
        assert ld >= K
        g = Guarded((M, ld), src.dtype, src.device, align=align, poison=True)
        t = g.data[:, :K]
        t.copy_(src)
    t._memguard = g   # keep the allocation with the view
    return t


def assert_written(t: torch.Tensor, what: str = "") -> None:
    """No element of ``t`` (a view: the written set) still holds the sentinel."""
    s = is_sentinel(t)
    if bool(s.any()):
        idx = s.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(s.sum())} of {t.numel()} elements of the written set still hold the "
                             f"sentinel (first at {idx})")


def assert_untouched(t: torch.Tensor, what: str = "") -> None:
    """Every element of ``t`` (a view: the elements the contract leaves alone) still holds the sentinel."""
    s = is_sentinel(t)
    if not bool(s.all()):
        idx = (~s).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int((~s).sum())} of {t.numel()} elements outside the written set changed "
                             f"(first at {idx})")


def assert_finite(*ts: torch.Tensor, what: str = "") -> None:
    for i, t in enumerate(ts):
        if not bool(torch.isfinite(t).all()):
            raise AssertionError(f"{what}: operand {i} holds {int((~torch.isfinite(t)).sum())} non-finite elements")


# ----------------------------------------------------------------------------- free blocks of the caching allocator
_HIP = [None]


def _hip():
    """The HIP runtime torch already loaded (no new library, no kernel of this project)."""
    if _HIP[0] is None:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        if path is None:
            raise RuntimeError("libamdhip64.so is not loaded in this process")
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        lib.hipMemsetD32Async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
        lib.hipMemsetD32Async.restype = ctypes.c_int
        _HIP[0] = lib
    return _HIP[0]


def read_words(ptr: int, n: int) -> torch.Tensor:
    """``n`` 32-bit words at device address ``ptr``, copied to the host by the runtime (no kernel); synchronises."""
    lib = _hip()
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.hipMemcpy.restype = ctypes.c_int
    torch.cuda.synchronize()
    host = torch.empty(n, dtype=torch.int32)
    rc = lib.hipMemcpy(ctypes.c_void_p(host.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(4 * n), 2)  # device->host
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed: {rc}")
    return host


POISON_WORD = 0x7FF0DEAD   # an f32 NaN; as two bf16 / f16 halves: 0x7FF0 (NaN) and 0xDEAD (a finite value)


def free_blocks(device=None) -> Sequence[tuple]:
    """(address, bytes) of every ``inactive`` block of the caching allocator on ``device``, private pools of captured
    graphs included.  Blocks ``active_pending_free`` (freed, still in use by a stream) are skipped.  When a snapshot
    block carries no ``address``, it is the segment's address plus the sizes of the blocks before it."""
    dev = torch.device(device if device is not None else "cuda").index
    dev = torch.cuda.current_device() if dev is None else dev
    out = []
    for seg in torch.cuda.memory_snapshot():
        if seg.get("device", dev) != dev:
            continue
        addr = int(seg["address"])
        for blk in seg["blocks"]:
            a = int(blk["address"]) if "address" in blk else addr
            if blk["state"] == "inactive":
                out.append((a, int(blk["size"])))
            addr = a + int(blk["size"])
    return out


def poison_free_blocks(device=None, word: int = POISON_WORD) -> int:
    """Fill every free block with ``word`` (whole 32-bit words) on the current stream; returns the bytes poisoned.
    A kernel that reads freed or never-written memory then computes with NaN."""
    lib = _hip()
    stream = torch.cuda.current_stream(device).cuda_stream
    total = 0
    for a, size in free_blocks(device):
        n = size // 4
        if n == 0:
            continue
        rc = lib.hipMemsetD32Async(ctypes.c_void_p(a), ctypes.c_int(_signed(word, 32)), ctypes.c_size_t(n),
                                   ctypes.c_void_p(stream))
        if rc != 0:
            raise RuntimeError(f"hipMemsetD32Async({a:#x}, {n}) failed: {rc}")
        total += 4 * n
    return total
