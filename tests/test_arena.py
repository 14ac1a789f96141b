"""tests/arena.py on the host: the checker that the poisoned-buffer GPU tests rely on, held to its negative controls on CPU
tensors.  A checker that passes a flipped guard word, a surviving poison word or a changed input would check nothing; one that
refuses an honest call would be wrong."""
import pytest
import torch

import arena as A
from transport_refs import NAN_BITS, same_bits, sentinel

CPU = torch.device("cpu")


def honest_call(poison=True):
    """y = 2 x + r written like a kernel would: every output element, nothing else; r accumulated in place; a workspace used."""
    ar = A.Arena(CPU, poison=poison)
    g = torch.Generator().manual_seed(3)
    x = ar.place(torch.randn(3, 5, 7, generator=g), "x")
    r = ar.place(torch.randn(3, 5, 7, generator=g), "r", inplace=True)
    n = ar.place(torch.tensor([7], dtype=torch.int64), "n", inplace=True)
    y = ar.out((3, 5, 7), "y")
    s = ar.out((5, 2), "stats", dtype=torch.float64)
    block = torch.zeros(6, 10, dtype=torch.bool)
    block[:, 2:5] = True
    gw = ar.out((6, 10), "gw", written=block)
    ws = ar.scratch(64, "ws")
    empty = ar.scratch(0, "empty")
    ws.fill_(9)
    y.copy_(2 * x + r)
    r.add_(x)
    n.add_(1)
    s.copy_(torch.arange(10, dtype=torch.float64).view(5, 2))
    gw[:, 2:5] = 1.0
    assert empty.numel() == 0
    return ar


def test_layout_is_what_the_module_promises():
    assert A.GUARD == 4096 and A.GUARD % 64 == 0 and A.SKEW * 4 == 16
    ar = A.Arena(CPU)
    x = ar.place(torch.arange(6, dtype=torch.float32).view(2, 3), "x")
    y = ar.out((4, 2), "y")
    d = ar.out((3,), "d", dtype=torch.float64)
    ws = ar.scratch(24, "ws")
    wide = ar.scratch(512, "wide", align=256)
    for name, view, nbytes in (("x", x, 24), ("y", y, 32), ("d", d, 24), ("ws", ws, 24), ("wide", wide, 512)):
        b = ar.buffers[name]
        lead = A.GUARD + (0 if name == "wide" else A.SKEW)
        assert view.numel() * view.element_size() == nbytes and b.words * 4 == nbytes
        assert b.slab.numel() == lead + b.words + A.GUARD
        assert view.data_ptr() - b.slab.data_ptr() == 4 * lead           # 16 bytes past a multiple of 256, or on it
        outside = torch.cat((b.slab[:lead], b.slab[lead + b.words:])).view(torch.float32)
        assert same_bits(outside, sentinel(outside.numel(), b.bits)).all() and torch.isnan(outside).all()
    assert len({b.bits for b in ar.buffers.values()}) == 5 and ar.buffers["x"].bits == NAN_BITS      # one payload per buffer
    assert torch.equal(x, torch.arange(6, dtype=torch.float32).view(2, 3))
    assert torch.isnan(y).all() and (d > 1e300).all()      # two poison words read as one double: 2.4e307, no sum survives it
    assert same_bits(y.reshape(-1), sentinel(8, ar.buffers["y"].bits)).all()
    zero = A.Arena(CPU, poison=False)
    assert (zero.out((4, 2), "y") == 0).all() and (zero.scratch(24, "ws") == 0).all()
    assert torch.isnan(zero.buffers["y"].slab.view(torch.float32)[:A.GUARD]).all()         # the guards stay


@pytest.mark.parametrize("poison", [True, False])
def test_an_honest_call_passes(poison):
    honest_call(poison).check("honest")


@pytest.mark.parametrize("name", ["x", "r", "y", "stats", "gw", "ws", "empty"])
@pytest.mark.parametrize("side", ["front", "back"])
def test_one_flipped_guard_word_is_refused(name, side):
    ar = honest_call()
    b = ar.buffers[name]
    at = b.front - 1 if side == "front" else b.front + b.words          # the words next to the payload ...
    b.slab[at] ^= 1
    with pytest.raises(AssertionError, match=r"%s guard of \w+ '%s' overwritten: 1 words, the first at float offset %d " % (
            side, name, -1 if side == "front" else b.words)):
        ar.check("flipped")
    ar = honest_call()
    b = ar.buffers[name]
    b.slab[0 if side == "front" else -1] = 0                            # ... and the farthest ones
    with pytest.raises(AssertionError, match="%s guard" % side):
        ar.check("flipped")


def test_one_output_element_left_at_the_poison_is_refused():
    ar = honest_call()
    ar.buffers["y"].view.view(-1)[37] = sentinel(1, ar.buffers["y"].bits)[0]
    with pytest.raises(AssertionError, match="output 'y' not written: 1 words keep the poison, the first at float offset 37"):
        ar.check("left")
    ar = honest_call()
    ar.buffers["stats"].slab[ar.buffers["stats"].front + 5] = ar.buffers["stats"].bits   # half of a double
    with pytest.raises(AssertionError, match="output 'stats' not written: 1 words keep the poison, the first at float offset 5"):
        ar.check("left")
    ar = honest_call()
    ar.buffers["gw"].view[3, 4] = sentinel(1, ar.buffers["gw"].bits)[0]
    with pytest.raises(AssertionError, match="output 'gw' not written: 1 words keep the poison, the first at float offset 34"):
        ar.check("left")
    ar = honest_call()
    ar.buffers["gw"].view[3, 5] = 0.0                                    # ... and a write outside the declared block
    with pytest.raises(AssertionError, match="output 'gw' written outside its region: 1 words, the first at float offset 35"):
        ar.check("outside")
    ar = honest_call()
    ar.buffers["y"].view.view(-1)[37] = float("nan")                     # another NaN is a value, not the poison: the reference's to judge
    ar.check("plain nan")


def test_a_nan_handed_on_from_another_buffers_guard_is_refused():
    """What a kernel that runs past the end of everything does: out[n + i] = x[n + i] + r[n + i], all three in guard words.  The sum
    of two NaNs carries the payload of one of them, never the one of the output's own guard."""
    ar = honest_call()
    x, y = ar.buffers["x"], ar.buffers["y"]
    past = slice(x.front + x.words, x.front + x.words + 4)
    summed = x.slab[past].view(torch.float32) + ar.buffers["r"].slab[past].view(torch.float32)
    assert torch.isnan(summed).all() and not same_bits(summed, y.slab[past].view(torch.float32)).any()
    y.slab[past] = summed.view(torch.int32)
    with pytest.raises(AssertionError, match="back guard of output 'y' overwritten: 4 words, the first at float offset 105 "):
        ar.check("past the end")
    ar = honest_call()
    y = ar.buffers["y"]
    y.view.view(-1)[:4] = ar.buffers["x"].slab[:4].view(torch.float32) * 2.0      # a result computed from an input's guard: written,
    ar.check("nan result")                                                         # and NaN for the reference to refuse
    assert torch.isnan(y.view.view(-1)[:4]).all()


def honest_byte_call(poison=True):
    """kmask = mask & other written like a kernel would, on byte tensors whose sizes are no multiple of a word (7 and 10 bytes)
    and one that is (8); `flags` only where declared."""
    ar = A.Arena(CPU, poison=poison)
    g = torch.Generator().manual_seed(5)
    m = ar.place(torch.randint(0, 2, (7,), generator=g, dtype=torch.uint8), "mask")
    o = ar.place(torch.randint(0, 2, (7,), generator=g, dtype=torch.uint8), "other", inplace=True)
    k = ar.out((7,), "kmask", dtype=torch.uint8)
    k8 = ar.out((2, 4), "kmask8", dtype=torch.uint8)
    part = torch.zeros(2, 5, dtype=torch.bool)
    part[:, 1:3] = True
    f = ar.out((2, 5), "flags", dtype=torch.uint8, written=part)
    k.copy_(m & o)
    k8.fill_(1)
    f[:, 1:3] = 0
    o.zero_()
    return ar


def test_byte_tensors_layout():
    """A uint8 buffer: `numel` bytes of payload on the base every buffer gets (16 bytes past a multiple of 256), the rest of its
    last word poisoned guard."""
    ar = honest_byte_call()
    for name, nbytes, words in (("mask", 7, 2), ("other", 7, 2), ("kmask", 7, 2), ("kmask8", 8, 2), ("flags", 10, 3)):
        b = ar.buffers[name]
        assert b.view.dtype == torch.uint8 and b.view.numel() == nbytes and b.nbytes == nbytes and b.words == words
        assert b.slab.numel() == A.GUARD + A.SKEW + words + A.GUARD
        assert b.view.data_ptr() - b.slab.data_ptr() == 4 * (A.GUARD + A.SKEW)
        pad = b.slab.view(torch.uint8)[4 * b.front + nbytes:4 * (b.front + words)]
        assert torch.equal(pad, sentinel(words, b.bits).view(torch.uint8)[nbytes:])
    fresh = A.Arena(CPU)
    k = fresh.out((7,), "kmask", dtype=torch.uint8)
    assert torch.equal(k, sentinel(2, NAN_BITS).view(torch.uint8)[:7]) and not ((k == 0) | (k == 1)).any()   # no poison byte is a mask value
    zero = A.Arena(CPU, poison=False)
    assert (zero.out((7,), "kmask", dtype=torch.uint8) == 0).all()
    assert (zero.buffers["kmask"].slab.view(torch.uint8)[4 * zero.buffers["kmask"].front + 7] != 0)        # the pad byte stays guard


@pytest.mark.parametrize("poison", [True, False])
def test_an_honest_byte_call_passes(poison):
    honest_byte_call(poison).check("honest bytes")


@pytest.mark.parametrize("name", ["mask", "other", "kmask", "flags"])
def test_a_write_into_the_pad_bytes_of_the_last_word_is_a_back_guard_overrun(name):
    """A kernel that stores its byte mask as whole words (or runs one element over) hits the bytes between `numel` and the word
    boundary: back guard, named by its byte offset.  Each pad byte on its own, the first word behind, and the byte in front."""
    nbytes = honest_byte_call().buffers[name].nbytes
    for at in range(nbytes, 4 * ((nbytes + 3) // 4)):
        ar = honest_byte_call()
        b = ar.buffers[name]
        b.slab.view(torch.uint8)[4 * b.front + at] = 1
        with pytest.raises(AssertionError, match=r"back guard of \w+ '%s' overwritten: 1 bytes, the first at byte offset %d " % (name, at)):
            ar.check("pad byte")
    ar = honest_byte_call()
    b = ar.buffers[name]
    b.slab[b.front + b.words] ^= 1
    with pytest.raises(AssertionError, match=r"back guard of \w+ '%s' overwritten: 1 bytes, the first at byte offset %d " % (name, 4 * b.words)):
        ar.check("word behind")
    ar = honest_byte_call()
    b = ar.buffers[name]
    b.slab.view(torch.uint8)[4 * b.front - 1] = 0
    with pytest.raises(AssertionError, match=r"front guard of \w+ '%s' overwritten: 1 bytes, the first at byte offset -1 " % name):
        ar.check("byte in front")


def test_one_changed_input_byte_is_refused():
    ar = honest_byte_call()
    ar.buffers["mask"].view[5] ^= 1
    with pytest.raises(AssertionError, match="input 'mask' changed: 1 bytes, the first at byte offset 5"):
        ar.check("changed byte")
    ar = honest_byte_call()
    ar.buffers["other"].view.fill_(9)                                    # declared in place
    ar.check("in place bytes")


def test_one_unwritten_output_byte_is_refused():
    """One byte of a word left at the poison while its three neighbours were written: a word-wise check would pass it."""
    ar = honest_byte_call()
    b = ar.buffers["kmask"]
    b.view[6] = sentinel(2, b.bits).view(torch.uint8)[6]
    with pytest.raises(AssertionError, match="output 'kmask' not written: 1 bytes keep the poison, the first at byte offset 6"):
        ar.check("left byte")
    ar = honest_byte_call()
    b = ar.buffers["kmask8"]
    b.view[0, 1] = sentinel(2, b.bits).view(torch.uint8)[1]
    with pytest.raises(AssertionError, match="output 'kmask8' not written: 1 bytes keep the poison, the first at byte offset 1"):
        ar.check("left byte")
    ar = honest_byte_call()
    b = ar.buffers["flags"]
    b.view[1, 2] = sentinel(3, b.bits).view(torch.uint8)[7]
    with pytest.raises(AssertionError, match="output 'flags' not written: 1 bytes keep the poison, the first at byte offset 7"):
        ar.check("left byte")
    ar = honest_byte_call()
    ar.buffers["flags"].view[1, 3] = 0                                   # ... and a byte written outside the declared block
    with pytest.raises(AssertionError, match="output 'flags' written outside its region: 1 bytes, the first at byte offset 8"):
        ar.check("outside")


def test_a_changed_input_is_refused_unless_declared_in_place():
    ar = honest_call()
    ar.buffers["x"].view[2, 4, 6] *= -1.0                                # one sign bit
    with pytest.raises(AssertionError, match="input 'x' changed: 1 words, the first at float offset 104"):
        ar.check("changed")
    ar = honest_call()
    ar.buffers["r"].view.zero_()                                         # declared in place: free to change
    ar.buffers["n"].view.add_(5)
    ar.check("in place")
