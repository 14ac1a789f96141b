"""Poisoned, guarded buffers for one kernel call.  TEST INFRASTRUCTURE, torch only.

A kernel test that hands its kernel exactly-sized fresh tensors judges the values inside them and nothing else.  An `Arena` owns
every device buffer of one call and judges the rest:

  place(cpu_tensor)   an input: the values in the middle of a slab whose two ends hold guard words
  out(shape)          an output: the same, the payload poisoned as well (both take fp32, fp64, int32, int64 and uint8)
  scratch(nbytes)     a workspace of exactly `nbytes` poisoned bytes between guards
  check()             every guard word intact (nothing written outside a buffer), every input bit-identical to what was placed
                      (unless declared in place), every output element overwritten (no poison word survives)

Guard and poison words are quiet NaNs with a payload, `transport_refs.NAN_BITS` with the buffer's ordinal in bits 8..15: a read
outside an input that reaches the result makes the result NaN, which no comparison against a reference survives; a missed
zero-fill adds to NaN.  Arithmetic hands a NaN's payload on, so a value computed from one buffer's guard words and stored into
another buffer's guard or payload still differs from what was there -- with one payload for all buffers, `out[numel + i] = a[numel +
i] + b[numel + i]` would store the very bits it overwrites.  (What no payload can show: a kernel that adds to its own poison, which
reads as "not written", or rewrites its own guard words with what it read there.)  `GUARD` = 4096 floats on each side, more than
one tile row of any kernel of the library.  A buffer starts GUARD + 4 floats into its slab: 16-byte
aligned, as the entry points demand, and no better (the slab itself is aligned by the allocator, GUARD floats are a multiple of
256 bytes, the four extra floats are one odd multiple of 16), so a kernel that assumes 256-byte bases meets the weakest pointer
the ABI accepts.  `align=256` drops the four floats for a buffer whose contract asks for that alignment.

A uint8 buffer (the masks of the loss rows and of the edge solver) has a payload of `numel` BYTES.  The bytes from there to the next
word boundary belong to the back guard: they carry the poison and are checked as guard, and inputs, "written" and "not written" are
judged byte by byte (the poison's bytes are 0xd1, 0xd0 ^ ordinal, 0xc0, 0x7f: none is the 0 or 1 a mask holds while the arena has
fewer than 208 buffers).  Its base follows the same rule as every other buffer's.

An Arena(poison=False) zero-fills outputs and workspaces instead (guards stay): the twin of a poisoned call for entry points that
promise bit-reproducible results, which must not depend on what their outputs and scratch held, not even in the last bit.

tests/test_arena.py holds the checker to its negative controls on the host.
"""
import torch

from transport_refs import NAN_BITS, same_bits, sentinel

GUARD = 4096                       # floats on each side of every buffer
SKEW = 4                           # floats: the odd multiple of 16 bytes that keeps a default buffer off every larger alignment
_WORD = {torch.float32: 1, torch.int32: 1, torch.float64: 2, torch.int64: 2}


class _Buffer:
    def __init__(self, name, kind, bits, slab, front, words, view, nbytes=None):
        self.name, self.kind, self.bits, self.slab, self.front, self.words, self.view = name, kind, bits, slab, front, words, view
        self.nbytes = nbytes       # a byte tensor's payload in bytes (the rest of its last word is back guard); None: whole words
        self.expected = None       # inputs: the placed words (int32, CPU; bytes of a byte tensor); None if declared in place
        self.written = None        # outputs: bool (words; bytes of a byte tensor) of what the call must overwrite; the rest keeps the poison


class Arena:
    def __init__(self, device, poison=True):
        self.device, self.poison = torch.device(device), poison
        self.buffers = {}

    # ------------------------------------------------------------------------------------------------------------ buffers
    def _slab(self, name, kind, words, dtype, shape, align, nbytes=None):
        assert name not in self.buffers, "two buffers named %r" % name
        assert align in (16, 256)
        assert len(self.buffers) < 256
        bits = NAN_BITS ^ (len(self.buffers) << 8)                 # this buffer's own payload; bit 22 keeps it a quiet NaN
        front = GUARD + (SKEW if align == 16 else 0)
        slab = sentinel(front + words + GUARD, bits).view(torch.int32).to(self.device)
        payload = slab[front:front + words]
        if dtype != torch.uint8:
            view = payload.view(dtype).view(shape)
        else:
            view = payload.view(torch.uint8) if nbytes is None else payload.view(torch.uint8)[:nbytes].view(shape)
        if self.device.type == "cuda":
            at = view.data_ptr() if words else slab.data_ptr() + 4 * front
            assert at % align == 0 and (align != 16 or at % 32 != 0), "%s: base %#x is not the alignment asked for" % (name, at)
        buf = self.buffers[name] = _Buffer(name, kind, bits, slab, front, words, view, nbytes)
        return buf

    def place(self, tensor, name, inplace=False, align=16):
        """Device view holding `tensor` (CPU; fp32, fp64, int32, int64 or uint8).  inplace: the call may write it (residual ==
        output, a running buffer): its payload is then not compared."""
        t = tensor.detach().contiguous()
        if t.dtype == torch.uint8:
            buf = self._slab(name, "input", (t.numel() + 3) // 4, t.dtype, tuple(t.shape), align, nbytes=t.numel())
            buf.view.copy_(t)
            buf.expected = None if inplace else t.reshape(-1).clone()
            return buf.view
        words = t.numel() * _WORD[t.dtype]
        buf = self._slab(name, "input", words, t.dtype, tuple(t.shape), align)
        buf.view.copy_(t)
        buf.expected = None if inplace else t.reshape(-1).view(torch.int32).clone()
        return buf.view

    def out(self, shape, name, dtype=torch.float32, written=None, align=16):
        """Poisoned device tensor the call must overwrite -- all of it, or where `written` (bool, CPU, of `shape`) is set; then the
        other elements must keep their bits."""
        shape = tuple(shape)
        numel = 1
        for s in shape:
            numel *= s
        if dtype == torch.uint8:
            buf = self._slab(name, "output", (numel + 3) // 4, dtype, shape, align, nbytes=numel)
        else:
            buf = self._slab(name, "output", numel * _WORD[dtype], dtype, shape, align)
        if written is not None:
            assert tuple(written.shape) == shape and written.dtype == torch.bool
            buf.written = written.reshape(-1).repeat_interleave(1 if dtype == torch.uint8 else _WORD[dtype])
        if not self.poison:
            buf.view.zero_() if written is None else buf.view.masked_fill_(written.to(self.device), 0)
        return buf.view

    def scratch(self, nbytes, name, align=16):
        """A workspace of exactly `nbytes` bytes (a multiple of 4) as a uint8 device tensor."""
        assert nbytes % 4 == 0, "%s: %d bytes" % (name, nbytes)
        buf = self._slab(name, "scratch", nbytes // 4, torch.uint8, None, align)
        if not self.poison:
            buf.view.zero_()
        return buf.view

    @staticmethod
    def ptr(view):
        """Device address of a view; a zero-size workspace still gets the address between its guards."""
        return view.data_ptr() if view.numel() else view.untyped_storage().data_ptr() + view.storage_offset() * view.element_size()

    # -------------------------------------------------------------------------------------------------------------- check
    def check(self, what=""):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for buf in self.buffers.values():
            if buf.nbytes is not None:
                self._check_bytes(buf, what)
                continue
            slab = buf.slab.cpu().view(torch.float32)
            poisoned = same_bits(slab, sentinel(slab.numel(), buf.bits))
            end = buf.front + buf.words
            for side, lo, hi, origin in (("front", 0, buf.front, buf.front), ("back", end, slab.numel(), buf.front)):
                bad = ~poisoned[lo:hi]
                if bad.any():
                    first = lo + int(torch.nonzero(bad)[0])
                    raise AssertionError("%s: %s guard of %s %r overwritten: %d words, the first at float offset %d from the buffer's "
                                         "start (now %#010x)" % (what, side, buf.kind, buf.name, int(bad.sum()), first - origin,
                                                                 int(slab.view(torch.int32)[first]) & 0xFFFFFFFF))
            payload = slab[buf.front:end]
            if buf.kind == "input" and buf.expected is not None:
                bad = ~same_bits(payload, buf.expected.view(torch.float32))
                if bad.any():
                    raise AssertionError("%s: input %r changed: %d words, the first at float offset %d" % (
                        what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))
            if buf.kind == "output" and self.poison:
                kept = poisoned[buf.front:end]
                must = buf.written if buf.written is not None else torch.ones(buf.words, dtype=torch.bool)
                bad = kept & must
                if bad.any():
                    raise AssertionError("%s: output %r not written: %d words keep the poison, the first at float offset %d" % (
                        what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))
                bad = ~kept & ~must
                if bad.any():
                    raise AssertionError("%s: output %r written outside its region: %d words, the first at float offset %d" % (
                        what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))

    def _check_bytes(self, buf, what):
        """`check` for a byte tensor: the same four judgements with the byte as the unit; offsets are in bytes from the payload."""
        slab = buf.slab.cpu()
        got = slab.view(torch.uint8)
        poisoned = got == sentinel(slab.numel(), buf.bits).view(torch.uint8)
        start = 4 * buf.front
        end = start + buf.nbytes
        for side, lo, hi in (("front", 0, start), ("back", end, got.numel())):
            bad = ~poisoned[lo:hi]
            if bad.any():
                first = lo + int(torch.nonzero(bad)[0])
                raise AssertionError("%s: %s guard of %s %r overwritten: %d bytes, the first at byte offset %d from the buffer's "
                                     "start (now %#04x)" % (what, side, buf.kind, buf.name, int(bad.sum()), first - start, int(got[first])))
        payload = got[start:end]
        if buf.kind == "input" and buf.expected is not None:
            bad = payload != buf.expected
            if bad.any():
                raise AssertionError("%s: input %r changed: %d bytes, the first at byte offset %d" % (
                    what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))
        if buf.kind == "output" and self.poison:
            kept = poisoned[start:end]
            must = buf.written if buf.written is not None else torch.ones(buf.nbytes, dtype=torch.bool)
            bad = kept & must
            if bad.any():
                raise AssertionError("%s: output %r not written: %d bytes keep the poison, the first at byte offset %d" % (
                    what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))
            bad = ~kept & ~must
            if bad.any():
                raise AssertionError("%s: output %r written outside its region: %d bytes, the first at byte offset %d" % (
                    what, buf.name, int(bad.sum()), int(torch.nonzero(bad)[0])))
