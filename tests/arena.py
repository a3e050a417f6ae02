"""A sentinel arena for the containment tests (tests/test_gpu_containment.py; self-tests in tests/test_arena_host.py).

The C ABI is "caller-owned memory, sizes from the headers".  An Arena is ONE uint8 allocation filled with the byte 0xFF (NaN
as fp16 / bf16 / fp32 / fp64, all ones as an integer); every buffer a call is handed is carved out of it at its exact size,
with guard bytes before and after that no call may change.  A write past a buffer therefore lands in memory the test owns
-- a guard or a neighbouring buffer -- and check() names it.  Works on any torch device, so the detector itself is tested
on the CPU.

Roles of a carve:
  in       filled by the test; bit-identical after the call
  out      left at the fill before the call
  scratch  no initialisation required by the header; the test runs once with it at 0x00 and once at 0xFF
  zeroed   "zeroed once by the caller, left zeroed by every launch": zero before, all zero after
  inout    filled by the test, rewritten by the call
"""
import torch

FILL = 0xFF
MIN_GUARD = 64 * 1024      # the least trailing guard: conditions, not measurements (a wider writer asks for more)
GUARD_BEFORE = 4096
ROLES = ("in", "out", "scratch", "zeroed", "inout")


class Buffer:
    """`nbytes` bytes of an arena at byte offset `start`; the guard bytes around it belong to the arena."""

    def __init__(self, arena, name, start, nbytes, guard_before, guard_after, role, align):
        self.arena, self.name, self.start, self.nbytes = arena, name, start, nbytes
        self.guard_before, self.guard_after, self.role, self.align = guard_before, guard_after, role, align
        self.snapshot = None      # what an `in` buffer held when freeze() was called

    def u8(self):
        return self.arena.mem[self.start:self.start + self.nbytes]

    def view(self, dtype):
        """A typed view of the whole buffer (its start must be aligned to the element, its size a multiple of it)."""
        return self.u8().view(dtype)

    def f32(self):
        return self.view(torch.float32)

    def f64(self):
        return self.view(torch.float64)

    def i32(self):
        return self.view(torch.int32)

    def i64(self):
        return self.view(torch.int64)

    def f16(self):
        return self.view(torch.float16)

    @property
    def dptr(self):
        """The absolute address of the first byte."""
        return self.arena.base + self.start

    def put(self, tensor):
        """Copy a tensor's bytes in (exactly nbytes of them)."""
        raw = tensor.contiguous().reshape(-1).view(torch.uint8)
        assert raw.numel() == self.nbytes, (self.name, raw.numel(), self.nbytes)
        self.u8().copy_(raw)

    def set_bytes(self, byte):
        self.u8().fill_(byte)

    def freeze(self):
        """Remember the contents: check() then requires them unchanged (role `in`)."""
        self.snapshot = self.u8().clone()


class Arena:
    def __init__(self, device, nbytes):
        self.mem = torch.full((int(nbytes),), FILL, dtype=torch.uint8, device=device)
        self.base = self.mem.data_ptr()
        self.cursor = 0
        self.buffers = {}

    @staticmethod
    def room(nbytes, align=256, guard_after=MIN_GUARD, guard_before=GUARD_BEFORE):
        """An upper bound of the arena bytes one carve takes (for sizing the allocation)."""
        return guard_before + align + nbytes + max(guard_after, MIN_GUARD)

    def carve(self, name, nbytes, align=256, guard_after=MIN_GUARD, guard_before=GUARD_BEFORE, role="out"):
        """A buffer of exactly `nbytes` bytes whose ABSOLUTE address is a multiple of `align` (and, for align < 256, of no
        larger power of two than the header allows where that is possible: an odd multiple of `align`).  The trailing guard
        begins at the first byte after `nbytes`, with no rounding; the next carve starts behind it."""
        assert role in ROLES, role
        assert name not in self.buffers, name
        assert align >= 1 and align & (align - 1) == 0, align
        nbytes, guard_after = int(nbytes), max(int(guard_after), MIN_GUARD)
        start = self.cursor + guard_before
        start += -(self.base + start) % align
        if align < 256 and (self.base + start) % (2 * align) == 0:
            start += align      # keep the start as ragged as the header allows
        end = start + nbytes + guard_after
        # never at the end of the allocation: the last guard is the arena's own memory
        assert end <= self.mem.numel(), f"arena of {self.mem.numel()} bytes is too small for `{name}` (needs {end})"
        buf = Buffer(self, name, start, nbytes, start - self.cursor, guard_after, role, align)
        self.cursor = end
        self.buffers[name] = buf
        if role == "zeroed":
            buf.set_bytes(0)
        return buf

    # -- the detector --------------------------------------------------------------------------------------------------
    def _guard_report(self, buf, lo, hi, side):
        region = self.mem[lo:hi]
        if bool((region == FILL).all()):      # (the common case in one reduction)
            return None
        changed = (region != FILL).nonzero().reshape(-1)
        first, last = int(changed[0]), int(changed[-1])
        if side == "after":
            where = f"first {first} and last {last} bytes past its end"
        else:
            where = f"first {hi - lo - first} and last {hi - lo - last} bytes before its start"
        return (f"`{buf.name}` ({buf.nbytes} bytes, {buf.role}): {int(changed.numel())} guard byte(s) changed {side} the "
                f"buffer, {where}")

    def problems(self):
        """Every violated condition, as a list of messages (empty: all is well)."""
        out = []
        for buf in self.buffers.values():
            for report in (self._guard_report(buf, buf.start - buf.guard_before, buf.start, "before"),
                           self._guard_report(buf, buf.start + buf.nbytes, buf.start + buf.nbytes + buf.guard_after, "after")):
                if report:
                    out.append(report)
            if buf.snapshot is not None and not torch.equal(buf.u8(), buf.snapshot):      # (frozen: a call only reads it)
                diff = (buf.u8() != buf.snapshot).nonzero().reshape(-1)
                if diff.numel():
                    out.append(f"`{buf.name}` ({buf.nbytes} bytes, in): input modified, {int(diff.numel())} byte(s), first at "
                               f"offset {int(diff[0])}, last at offset {int(diff[-1])}")
            if buf.role == "zeroed" and bool(buf.u8().any()):
                nz = buf.u8().nonzero().reshape(-1)
                if nz.numel():
                    out.append(f"`{buf.name}` ({buf.nbytes} bytes, zeroed): left non-zero, {int(nz.numel())} byte(s), first at "
                               f"offset {int(nz[0])}, last at offset {int(nz[-1])}")
        tail = self.mem[self.cursor:]
        changed = (tail != FILL).nonzero().reshape(-1) if not bool((tail == FILL).all()) else tail[:0]
        if changed.numel():
            out.append(f"arena tail: {int(changed.numel())} byte(s) changed, first {int(changed[0])} bytes past the last guard")
        return out

    def check(self):
        """Every guard byte still holds the fill, every frozen `in` buffer its contents, every `zeroed` buffer zeros."""
        problems = self.problems()
        assert not problems, "\n".join(problems)


def fill_words(tensor_u8):
    """Mask over the 4-byte words of a byte tensor (length a multiple of 4): True where the word still holds the fill."""
    return tensor_u8.view(torch.int32) == -1
