"""Yardsticks for gradients whose parts differ in size by orders of magnitude.  TEST INFRASTRUCTURE, torch on the CPU.

The heads of this detector produce gradients that differ by four to five orders of magnitude (the dense key-point heads against
the 2-D box head), so `max|got - ref| <= tol * max|ref|` over a whole gradient tensor checks the largest head only.  The helpers
here judge every group of channels (a head), or every element, on its own scale.
"""
import numpy as np
import torch


def head_groups(loss):
    """[(name, ch0, ch1)] of the regression heads of a Loss_Computation, in channel order (channels ch0 .. ch1 - 1)."""
    k2c = loss.key2channel
    groups, o = [], 0
    for name, n in zip(k2c.keys, k2c.channels):
        groups.append((name, o, o + n))
        o += n
    return groups


def assert_close_by_group(got, ref, groups, tol, what):
    """`max|got - ref| <= tol * max|ref|` for every group (name, ch0, ch1) of the LAST axis, each on its own maximum.  Where the
    reference is identically zero in a group, `got` must be exactly zero there.  Returns the worst error / scale for the record."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    assert sorted(set(range(ref.shape[-1]))) == sorted(c for _, a, b in groups for c in range(a, b)), "groups must tile the last axis"
    worst = 0.0
    for name, a, b in groups:
        g, r = got[..., a:b], ref[..., a:b]
        scale = r.abs().max().item()
        if scale == 0.0:
            nz = g.abs()
            assert nz.max().item() == 0.0, "%s, %s: the reference is identically zero, got %.3e at %s" % (
                what, name, nz.max().item(), np.unravel_index(nz.argmax().item(), tuple(g.shape)))
            continue
        d = (g - r).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        err = d.max().item()
        at = np.unravel_index(d.argmax().item(), tuple(d.shape))
        assert err <= tol * scale, "%s, %s: error %.3e = %.3e of this group's maximum %.3e (bar %.1e), worst at %s (channel %d)" % (
            what, name, err, err / scale, scale, tol, tuple(int(i) for i in at), a + int(at[-1]))
        worst = max(worst, err / scale)
    return worst


def assert_close_by_element(got, ref, rtol, bound, what):
    """`|got - ref| <= rtol * |ref| + bound` element by element, `bound` a tensor of the same shape.  Returns the worst
    |got - ref| / (rtol * |ref| + bound) for the record (0 / 0 counts as 0)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    bound = torch.as_tensor(bound).detach().cpu().double()
    assert got.shape == ref.shape == bound.shape, (what, tuple(got.shape), tuple(ref.shape), tuple(bound.shape))
    d = (got - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    allowed = rtol * ref.abs() + bound
    ratio = torch.where(d == 0, torch.zeros_like(d), d / allowed)       # d > 0 with allowed == 0 gives inf
    worst = ratio.max().item()
    at = np.unravel_index(ratio.argmax().item(), tuple(ratio.shape))
    assert worst <= 1.0, "%s: |got - ref| = %.3e at %s where %.1e * |ref| + bound = %.3e (ref %.6e, got %.6e): ratio %.3f" % (
        what, d[at].item(), tuple(int(i) for i in at), rtol, allowed[at].item(), ref[at].item(), got[at].item(), worst)
    return worst
