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


def test_a_changed_input_is_refused_unless_declared_in_place():
    ar = honest_call()
    ar.buffers["x"].view[2, 4, 6] *= -1.0                                # one sign bit
    with pytest.raises(AssertionError, match="input 'x' changed: 1 words, the first at float offset 104"):
        ar.check("changed")
    ar = honest_call()
    ar.buffers["r"].view.zero_()                                         # declared in place: free to change
    ar.buffers["n"].view.add_(5)
    ar.check("in place")
