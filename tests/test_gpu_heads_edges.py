"""The oldest kernels of csrc/heads.hip at their route boundaries and degenerate inputs, by element against the float64 references
of tests/heads_refs.py (held to loops, the oracle and closed forms in tests/test_heads_refs.py):

  gather / scatter  `dcd_poi_scatter_add` on both sides of its M >= 64 switch, `dcd_patch_scatter_add`, out-of-range indices, and the
                    autograd nodes built on them (`select_point_of_interest`, `scatter_add_at`, `head_out_and_gather`).
                    Bar: |got - ref| <= n 2^-24 S per cell (heads_refs: derived), untouched cells and the padding keep their bits.
  top-K             K = 128 = H W, K = 1, H W on both sides of the 1 024 threads, C K = 4 096, the switch between the ranked and the
                    serial tie path at 128 equal keys, negative scores, signed zeros, refusals.  Bit-exact.
  GIoU, focal       N around the 64-lane block with padded outputs; any exponents, targets outside [0, 1], an empty tensor.
  IoU-3D            known-answer geometry near the origin and at (20, 60) turned by 0.7 rad, and accuracy against float64 at 5, 40
                    and 80 m with the fp32 formula in a local frame as the yardstick.

Measured on an MI355X (pytest -s prints them):
    IoU-3D, 256 pairs per depth, worst |kernel - float64| (E) against the yardstick (E_ref), bar max(4 E_ref, 8 * 2^-24):
        5 m: E 2.81e-07, E_ref 2.17e-07;  40 m: E 2.41e-07, E_ref 2.41e-07;  80 m: E 1.97e-07, E_ref 2.61e-07
        (the kernel on absolute camera coordinates, as it was: over the bar at 40 and 80 m, and on the moved scenes)
    IoU-3D scenes: E 1.07e-07 near the origin, 1.91e-07 at (20, 60), corners there rounded by 3.3e-06 m
    scatter: worst |got - ref| / (n 2^-24 S) 0.75 .. 1.00 -- the cells with ONE term, where the bound is half a unit in the last
        place of the sum and is reached; focal gradient: 0.32 .. 0.45 of its bar at every exponent pair, `powf` included
"""
import functools

import numpy as np
import pytest
import torch

import heads_refs as R

pytestmark = pytest.mark.gpu

B, H, W = 2, 6, 11
HW = H * W
PAD = 256                                  # floats of padding on both sides of every buffer a kernel writes
ODD = 12345.678                            # the pre-fill of what must stay untouched


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Padded:
    """A device buffer of `numel` floats with PAD floats on both sides, everything pre-filled (a tensor or the constant ODD)."""

    def __init__(self, dev, shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), ODD, dtype=torch.float32, device=dev)
        self.view = self.buf[PAD:PAD + n].view(shape)
        if fill is not None:
            self.view.copy_(fill)
        self.before = self.buf.cpu().clone()

    def ptr(self):
        return self.view.data_ptr()

    def assert_padding_untouched(self, what):
        now = self.buf.cpu()
        assert torch.equal(_bits(now[:PAD]), _bits(self.before[:PAD])) and torch.equal(_bits(now[-PAD:]), _bits(self.before[-PAD:])), \
            "%s: wrote outside its output" % what

    def assert_untouched(self, what):
        assert torch.equal(_bits(self.buf), _bits(self.before)), "%s: wrote to its output" % what


def _call(name, like, *args):
    from dcd_amd import _lib
    return getattr(_lib.lib(), name)(_lib.stream_of(like), *args)


# ---- gather / scatter -------------------------------------------------------------------------------------------------------
def scatter_problem(M, C, seed, one_cell=False):
    """Random cells with forced duplicates (pairs, a run of four, the first and the last entry), a non-zero map to add into."""
    g = torch.Generator().manual_seed(seed)
    index = torch.randint(0, HW, (B, M), generator=g)
    if M >= 2:
        index[:, M - 1] = index[:, 0]
    if M >= 8:
        index[:, 1] = index[:, 0]
        index[0, M // 2:M // 2 + 4] = index[0, 2]
    if one_cell:
        index[1, :] = 17
    return torch.randn(B, C, HW, generator=g), torch.randn(B, M, C, generator=g), index


def run_scatter(cuda, base, vals, index, what):
    """`dcd_poi_scatter_add` through the C ABI into a padded, pre-filled map; checks the status and the padding."""
    C, M = base.shape[1], index.shape[1]
    out = Padded(cuda, base.shape, base)
    v, i = vals.to(cuda).contiguous(), index.to(cuda).contiguous()
    assert _call("dcd_poi_scatter_add", v, v.data_ptr(), i.data_ptr(), B, C, H, W, M, out.ptr()) == 0, what
    torch.cuda.synchronize()
    out.assert_padding_untouched(what)
    return out.view.cpu()


@pytest.mark.parametrize("C", [3, 70])
@pytest.mark.parametrize("M,one_cell", [(1, False), (63, False), (64, False), (65, False), (204, False), (65, True)])
def test_poi_scatter_add_on_both_sides_of_the_route_switch(cuda, M, C, one_cell):
    """M < 64 runs `poi_scatter_kernel` (lanes along the channels), M >= 64 `poi_scatter_rows_kernel` (lanes along the positions,
    another index arithmetic altogether): the same sum, into a map that is not zero, cell by cell within n 2^-24 S; cells that no
    index names keep their bits.  one_cell: all 65 entries of image 1 name cell 17 -- 65 atomics on one address per channel."""
    base, vals, index = scatter_problem(M, C, seed=100 + M + C, one_cell=one_cell)
    what = "poi scatter M=%d C=%d%s" % (M, C, " one cell" if one_cell else "")
    ref, n, S = R.scatter_ref(base, vals, index)
    assert int(n.max()) >= (65 if one_cell else min(M, 2))
    got = run_scatter(cuda, base, vals, index, what)
    print("%s: worst |got - ref| / (n 2^-24 S) = %.3f" % (what, R.assert_scatter(got, base, ref, n, S, what)))


@pytest.mark.parametrize("C", [3, 70])
def test_one_list_through_both_scatter_routes(cuda, C):
    """The M = 63 list, and the same list with one out-of-range entry of zero values appended (M = 64, the other kernel): the
    appended entry changes nothing, so both are held to the SAME reference, and to each other within the same bound."""
    base, vals, index = scatter_problem(63, C, seed=7 + C)
    ref, n, S = R.scatter_ref(base, vals, index)
    vals64 = torch.cat([vals, torch.zeros(B, 1, C)], 1)
    index64 = torch.cat([index, torch.full((B, 1), HW + 5)], 1)
    ref64, n64, S64 = R.scatter_ref(base, vals64, index64)
    assert torch.equal(ref, ref64) and torch.equal(n, n64) and torch.equal(S, S64)
    got63 = run_scatter(cuda, base, vals, index, "63 entries")
    got64 = run_scatter(cuda, base, vals64, index64, "64 entries")
    R.assert_scatter(got63, base, ref, n, S, "63 entries, C=%d" % C)
    R.assert_scatter(got64, base, ref, n, S, "64 entries, C=%d" % C)
    assert ((got63.double() - got64.double()).abs() <= n[:, None, :].double() * R.U * S).all()


OUTSIDE = (-1, HW, HW + 5)


@pytest.mark.parametrize("C", [3, 70])
@pytest.mark.parametrize("M", [40, 70])
def test_out_of_range_indices_gather_zero_and_scatter_nothing(cuda, M, C):
    """-1, H W and H W + 5 in the list (include/dcd_hip.h: not an error): the gather returns exactly 0.0 for those rows -- it
    WRITES the zero, the output is pre-filled -- and both scatter routes add nothing for them, in the map or around it."""
    base, vals, index = scatter_problem(M, C, seed=31 + M + C)
    for k, bad in enumerate(OUTSIDE):
        index[0, 3 + 5 * k] = bad
        index[1, M - 2 - 7 * k] = bad
    out = Padded(cuda, (B, M, C))
    f, i = base.to(cuda), index.to(cuda)
    assert _call("dcd_poi_gather", f, f.data_ptr(), i.data_ptr(), B, C, H, W, M, out.ptr()) == 0
    torch.cuda.synchronize()
    out.assert_padding_untouched("gather")
    got, ref = out.view.cpu(), R.gather_ref(base, index)
    assert torch.equal(got.double(), ref)
    bad_rows = (index < 0) | (index >= HW)
    assert int(bad_rows.sum()) == 6 and (got[bad_rows] == 0).all()
    sref, n, S = R.scatter_ref(base, vals, index)
    R.assert_scatter(run_scatter(cuda, base, vals, index, "scatter"), base, sref, n, S, "scatter with out-of-range entries M=%d C=%d" % (M, C))


PITCH, PLANE = W + 2, (H + 2) * (W + 2)


@pytest.mark.parametrize("C", [3, 70])
@pytest.mark.parametrize("M", [1, 7, 70])
def test_patch_scatter_add(cuda, M, C):
    """3x3 windows in a padded plane of (H + 2) (W + 2) cells: neighbouring and identical windows overlap, one window starts in the
    last row but one (its third row is past the plane), one at -1 (its first tap is in front of it), two lie outside altogether.
    Tap by tap within n 2^-24 S; a tap outside [0, plane) is dropped, and nothing is written around the output."""
    g0 = torch.Generator().manual_seed(50 + M + C)
    first = torch.randint(0, PLANE - 2 * PITCH - 2, (B, M), generator=g0)
    first[0, 0] = PLANE - 2 * PITCH + 3                   # rows H, H + 1 and one past the plane
    if M >= 7:
        first[:, 1] = first[:, 2] + 1                     # neighbours: six cells in common
        first[:, 3] = first[:, 2]                         # identical
        first[1, 0], first[1, 4], first[0, 5], first[1, 6] = -1, PLANE + 5, -100, PLANE - 1
    base = torch.randn(B, C, PLANE, generator=g0)
    g = torch.randn(B, C * 9, M, generator=g0)
    ref, n, S = R.patch_scatter_ref(base, g, first, PITCH)
    assert int(n[0].sum()) < 9 * M and (M < 7 or int(n.max()) >= 3)
    out = Padded(cuda, base.shape, base)
    gd, fd = g.to(cuda), first.to(cuda)
    assert _call("dcd_patch_scatter_add", gd, gd.data_ptr(), fd.data_ptr(), B, C, PLANE, PITCH, M, out.ptr()) == 0
    torch.cuda.synchronize()
    out.assert_padding_untouched("patch scatter")
    what = "patch scatter M=%d C=%d" % (M, C)
    print("%s: worst |got - ref| / (n 2^-24 S) = %.3f" % (what, R.assert_scatter(out.view.cpu(), base, ref, n, S, what)))


@pytest.mark.parametrize("M", [40, 70])
def test_select_point_of_interest_forward_and_backward(cuda, M):
    from dcd_amd import ops
    C = 70
    base, go, index = scatter_problem(M, C, seed=60 + M)
    f = base.view(B, C, H, W).to(cuda).requires_grad_()
    got = ops.select_point_of_interest(B, index.to(cuda), f)
    assert torch.equal(got.detach().cpu().double(), R.gather_ref(base, index))
    got.backward(go.to(cuda))
    zero = torch.zeros_like(base)
    ref, n, S = R.scatter_ref(zero, go, index)
    R.assert_scatter(f.grad.cpu().view(B, C, HW), zero, ref, n, S, "select_point_of_interest backward M=%d" % M)


@pytest.mark.parametrize("M", [40, 70])
def test_scatter_add_at(cuda, M):
    """In place on a non-zero map and returning that map; d/d map is the identity, d/d vals the gather of the map's gradient."""
    from dcd_amd import ops
    C = 3
    base, vals, index = scatter_problem(M, C, seed=70 + M)
    leaf = base.view(B, C, H, W).to(cuda).requires_grad_()
    v = vals.to(cuda).requires_grad_()
    fmap = leaf.clone()
    out = ops.scatter_add_at(fmap, v, index.to(cuda))
    assert out.data_ptr() == fmap.data_ptr() and out.shape == fmap.shape
    ref, n, S = R.scatter_ref(base, vals, index)
    R.assert_scatter(fmap.detach().cpu().view(B, C, HW), base, ref, n, S, "scatter_add_at M=%d" % M)
    g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1))
    out.backward(g.to(cuda))
    assert torch.equal(leaf.grad.cpu(), g)
    assert torch.equal(v.grad.cpu().double(), R.gather_ref(g.view(B, C, HW), index))
    for bad in (base.view(B, C, H, W).to(cuda).transpose(2, 3), base.view(B, C, H, W).to(cuda).double(),
                base.view(B, C, H, W).to(cuda).half()):
        before = bad.clone()
        with pytest.raises(RuntimeError):
            ops.scatter_add_at(bad, vals.to(cuda), index.to(cuda))
        assert torch.equal(bad, before)


@pytest.mark.parametrize("M", [40, 70])
@pytest.mark.parametrize("O,bias", [(1, True), (3, True), (1, False), (3, False)])
def test_head_out_and_gather(cuda, M, O, bias):
    """(conv1x1(x), x at listed cells) and the hand-written backward -- W^T g as a GEMM with the gathered rows' gradient scatter-added
    into it in place, the weight gradient as a GEMM, the bias gradient through `channel_sums` -- against float64 conv2d + gather under
    autograd, both outputs receiving a gradient in ONE backward.  GEMM-backed tensors: 2e-5 of the tensor's scale (fp32 sums in
    another order, the project's bar); the scatter-added part of grad x: n 2^-24 S on top."""
    from dcd_amd import ops
    C = 16
    g0 = torch.Generator().manual_seed(80 + M + O)
    _, gg, index = scatter_problem(M, C, seed=80 + M + O)
    x, w = torch.randn(B, C, H, W, generator=g0), torch.randn(O, C, 1, 1, generator=g0)
    bv = torch.randn(O, generator=g0) if bias else None
    go = torch.randn(B, O, H, W, generator=g0)
    xd, wd = x.to(cuda).requires_grad_(), w.to(cuda).requires_grad_()
    bd = bv.to(cuda).requires_grad_() if bias else None
    out, gat = ops.head_out_and_gather(xd, wd, bd, index.to(cuda))
    ((out * go.to(cuda)).sum() + (gat * gg.to(cuda)).sum()).backward()
    x64, w64 = x.double().requires_grad_(), w.double().requires_grad_()
    b64 = bv.double().requires_grad_() if bias else None
    out64 = torch.nn.functional.conv2d(x64, w64, b64)
    gat64 = x64.view(B, C, HW).permute(0, 2, 1).gather(1, index[:, :, None].expand(B, M, C))
    ((out64 * go.double()).sum() + (gat64 * gg.double()).sum()).backward()

    def close(a, b, what):
        err, scale = (a.detach().cpu().double() - b.detach()).abs().max().item(), b.detach().abs().max().item()
        assert a.shape == b.shape and err <= 2e-5 * scale, (what, err, scale)
    close(out, out64, "output")
    assert torch.equal(gat.detach().cpu().double(), gat64.detach())
    close(wd.grad, w64.grad, "grad weight")
    if bias:
        close(bd.grad, b64.grad, "grad bias")
    gemm = torch.einsum("oc,bop->bcp", w.double().view(O, C), go.double().view(B, O, HW))       # W^T g: what is scattered into
    ref, n, S = R.scatter_ref(gemm, gg, index)
    assert (ref - x64.grad.view(B, C, HW)).abs().max().item() <= 1e-12 * ref.abs().max().item()
    err = (xd.grad.cpu().view(B, C, HW).double() - ref).abs()
    allowed = 2e-5 * gemm.abs().max().item() + n[:, None, :].double() * R.U * S
    assert (err <= allowed).all(), ("grad x", (err / allowed).max().item())


# ---- top-K ------------------------------------------------------------------------------------------------------------------
NAMES = ("scores", "inds", "clses", "ys", "xs")


def assert_topk(cuda, heat, K, fuse, what):
    """ops.select_topk == topk_ref, every output, every element; scores by ==, so the two zeros are one value."""
    from dcd_amd import ops
    ref = R.topk_ref(R.nms_ref(heat) if fuse else heat, K)
    got = ops.select_topk(torch.from_numpy(heat).to(cuda), K, fuse_nms=fuse)
    for g_, r_, nm in zip(got, ref, NAMES):
        g_ = g_.cpu().numpy()
        assert g_.dtype == r_.dtype and g_.shape == r_.shape, (what, nm, g_.dtype, g_.shape)
        assert np.array_equal(g_, r_), "%s: %s (fuse_nms=%s) differs at %s" % (what, nm, fuse, np.argwhere(g_ != r_)[:4].tolist())
    return ref


def sigmoid_heat(shape, seed):
    rng = np.random.RandomState(seed)
    return np.clip(1 / (1 + np.exp(-rng.normal(-2, 1.5, shape))), 1e-4, 1 - 1e-4).astype(np.float32)


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("shape", [(2, 1, 8, 16, 128), (1, 1, 25, 40, 1), (2, 1, 25, 41, 128), (1, 32, 12, 20, 128)])
def test_topk_at_the_limits_of_k_and_of_the_map(cuda, shape, fuse):
    """K = 128 = TOPK_MAXK = H W (every cell is a winner), K = 1, H W = 1 000 < 1 024 threads and 1 025 (a second sweep with one
    cell), C K = 4 096 (the merge's limit) with one class's map copied into two others, so that equal scores meet in the merge and
    its rule -- lower position in the class-major list first -- decides."""
    Bt, C, Ht, Wt, K = shape
    heat = sigmoid_heat(shape[:4], seed=sum(shape))
    heat[:, :, 2:4, 3:6] = 0.77                                   # a plateau: ties inside a class, with and without the NMS
    if C == 32:
        heat[0, 5] = heat[0, 0]
        heat[0, 17] = heat[0, 0]
    ref = assert_topk(cuda, heat, K, fuse, str(shape))
    if C == 32:
        cls = np.floor(ref[2][0]).astype(int)
        assert {0, 5, 17} <= set(cls.tolist())
        for s in np.unique(ref[0][0]):
            mine = cls[ref[0][0] == s]
            assert (np.diff(mine) >= 0).all()


def tie_map(n_tie, fill_rest):
    """40 x 40: five distinct peaks, 0.25 on n_tie scattered cells (or on every other cell), everything else lower and distinct."""
    rng = np.random.RandomState(n_tie)
    cells = rng.permutation(1600)
    heat = (0.01 + 0.19 * rng.permutation(1600) / 1600.0).astype(np.float32)
    peaks, ties = cells[:5], np.sort(cells[5:] if fill_rest else cells[5:5 + n_tie])
    heat[peaks] = [0.9, 0.8, 0.7, 0.6, 0.5]
    heat[ties] = 0.25
    return heat.reshape(1, 1, 40, 40), peaks, ties


@pytest.mark.parametrize("n_tie,fill_rest", [(128, False), (129, False), (1595, True)])
def test_topk_tie_paths_switch_at_128_equal_keys(cuda, n_tie, fill_rest):
    """K = 100 takes the 5 peaks and 95 of the cells that hold 0.25: up to 128 equal keys are ranked from a list in LDS, more are
    taken by a serial ballot scan.  On both sides of the switch, and with every remaining cell in the tie: the 95 LOWEST indices."""
    heat, peaks, ties = tie_map(n_tie, fill_rest)
    assert len(ties) == n_tie and (np.sort(heat.ravel())[::-1][5:5 + n_tie] == np.float32(0.25)).all()
    ref = assert_topk(cuda, heat, 100, False, "%d equal keys" % n_tie)
    assert ref[1][0, :5].tolist() == peaks.tolist() and ref[1][0, 5:].tolist() == ties[:95].tolist()


def test_topk_orders_negative_scores(cuda):
    """Logits, not probabilities: every key goes through the negative branch of `f2key` somewhere, also at the K-th place."""
    heat = np.random.RandomState(11).normal(-2.5, 1.0, (2, 3, 24, 40)).astype(np.float32)       # ~6 positive scores per class
    heat[0, 1] = -np.abs(heat[0, 1])                               # a class without a positive score
    heat[:, :, 5, 5:9] = -0.5                                      # equal negative scores
    ref = assert_topk(cuda, heat, 50, False, "negative scores")
    assert (ref[0] < 0).any() and (ref[0] > 0).any()
    assert_topk(cuda, -np.abs(heat) - 0.125, 50, False, "all scores negative")


def test_topk_signed_zeros_tie_by_index(cuda):
    """The top-K has to take SOME of the zeros, and +0.0 and -0.0 alternate in index order: lower index first among zeros of either
    sign (include/dcd_hip.h: ties by lower linear index; -0.0 == +0.0).  Directly, and through the fused NMS, which writes -0.0
    for a negative non-maximum (v * 0) and +0.0 for a positive one.
    The kernel failed this before `f2key` added 0.0 to its argument: the keys of -0.0 (0x7fffffff) and +0.0 (0x80000000) differ, so
    the radix select took every +0.0 in front of every -0.0 whatever their indices."""
    heat = np.full((1, 1, 8, 16), -1.0, np.float32)
    flat = heat.reshape(-1)
    flat[[100, 7, 55]] = [0.9, 0.5, 0.25]
    zeros = np.arange(3, 123, 3)                                   # 40 cells
    flat[zeros[0::2]] = -0.0
    flat[zeros[1::2]] = 0.0
    flat[8:10] = [0.0, -0.0]
    ref = assert_topk(cuda, heat, 20, False, "signed zeros")
    want = sorted(set(zeros.tolist()) | {8, 9})[:17]
    assert ref[1][0].tolist() == [100, 7, 55] + want and (ref[0][0, 3:] == 0).all()
    assert np.signbit(flat[want]).any() and not np.signbit(flat[want]).all()
    # through the NMS: signs of the non-maxima decide the sign of their zero
    rng = np.random.RandomState(5)
    heat = rng.normal(0.0, 1.0, (2, 2, 8, 16)).astype(np.float32)
    nms = R.nms_ref(heat)
    zero = nms == 0
    assert (np.signbit(nms[zero])).any() and (~np.signbit(nms[zero])).any()
    K = 40
    for b in range(2):
        for c in range(2):
            assert (nms[b, c] > 0).sum() < K < (nms[b, c] >= 0).sum()
    ref = assert_topk(cuda, heat, K, True, "signed zeros from the fused NMS")
    assert (ref[0] == 0).any()
    assert_topk(cuda, nms, K, False, "signed zeros from nms_hm")


@pytest.mark.parametrize("shape", [(1, 1, 25, 40, 129), (1, 1, 8, 8, 65), (1, 33, 12, 20, 128)])
def test_topk_refuses_what_it_cannot_hold(cuda, shape):
    """K > 128, K > H W and C K > 4 096: DCD_ERR_BAD_ARG from the C ABI with every output buffer untouched, an exception from ops."""
    from dcd_amd import _lib, ops
    Bt, C, Ht, Wt, K = shape
    heat = torch.from_numpy(sigmoid_heat(shape[:4], seed=1)).to(cuda)
    outs = [Padded(cuda, (Bt, K)) for _ in range(4)]
    inds = torch.full((Bt, K + 8), -7, dtype=torch.int64, device=cuda)
    ws = torch.full((Bt * C * K * 8 + 256,), 0x5A, dtype=torch.uint8, device=cuda)
    st = _call("dcd_heatmap_topk", heat, heat.data_ptr(), Bt, C, Ht, Wt, K, 0, outs[0].ptr(), inds.data_ptr(), outs[1].ptr(),
               outs[2].ptr(), outs[3].ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    assert st == 1
    for o in outs:
        o.assert_untouched("refused top-K")
    assert (inds == -7).all() and (ws == 0x5A).all()
    with pytest.raises(_lib.DcdHipError):
        ops.select_topk(heat, K)


# ---- GIoU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 65, 200])
def test_giou_around_the_block_size(cuda, N):
    """One lane per box in blocks of 64: N = 1, 63, 65 and 200 with N + 64 pre-filled rows in every output.  Rows < N against
    `_giou64` of test_gpu_heads.py under autograd at that test's bars (losses rtol 1e-5 + 1e-6, gradient rows 1e-4 of the row's
    maximum + 1e-7); rows >= N untouched; without a gradient buffer the same bits."""
    import test_gpu_heads as TH
    from oracle import heads_oracle as ho
    rng = np.random.RandomState(N)
    pred = rng.uniform(0, 30, (N, 4)).astype(np.float32)
    tgt = rng.uniform(0.5, 30, (N, 4)).astype(np.float32)
    pred[0] = 0.0
    pred[N - 1, 0] = tgt[N - 1, 0]                                 # a tie in the last row of the last block
    p, t = torch.from_numpy(pred).to(cuda), torch.from_numpy(tgt).to(cuda)
    rows = N + 64
    losses, ious, grad = Padded(cuda, (rows,)), Padded(cuda, (rows,)), Padded(cuda, (rows, 4))
    assert _call("dcd_giou_loss", p, p.data_ptr(), t.data_ptr(), N, losses.ptr(), ious.ptr(), grad.ptr()) == 0
    losses2, ious2 = Padded(cuda, (rows,)), Padded(cuda, (rows,))
    assert _call("dcd_giou_loss", p, p.data_ptr(), t.data_ptr(), N, losses2.ptr(), ious2.ptr(), None) == 0
    torch.cuda.synchronize()
    for o, rest in ((losses, N), (ious, N), (grad, N), (losses2, N), (ious2, N)):
        o.assert_padding_untouched("giou N=%d" % N)
        assert (o.view[rest:] == ODD).all(), "giou N=%d: rows >= N written" % N
    assert torch.equal(_bits(losses.view[:N]), _bits(losses2.view[:N])) and torch.equal(_bits(ious.view[:N]), _bits(ious2.view[:N]))
    pt, tt = torch.from_numpy(pred).double().requires_grad_(), torch.from_numpy(tgt).double()
    l64 = TH._giou64(pt, tt)
    l64.sum().backward()
    np.testing.assert_allclose(losses.view[:N].cpu().numpy(), l64.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(ious.view[:N].cpu().numpy(), ho.giou_loss(pred, tgt)[1], rtol=1e-5, atol=1e-6)
    row_err = (grad.view[:N].cpu().double() - pt.grad).abs().max(dim=1).values
    row_bar = 1e-4 * pt.grad.abs().max(dim=1).values + 1e-7
    assert (row_err <= row_bar).all(), (N, (row_err / row_bar).max().item(), int((row_err / row_bar).argmax()))


def test_giou_of_nothing(cuda):
    p = torch.zeros(4, 4, device=cuda)
    outs = [Padded(cuda, (64,)), Padded(cuda, (64,)), Padded(cuda, (64, 4))]
    assert _call("dcd_giou_loss", p, p.data_ptr(), p.data_ptr(), 0, outs[0].ptr(), outs[1].ptr(), outs[2].ptr()) == 0
    torch.cuda.synchronize()
    for o in outs:
        o.assert_untouched("giou N=0")


# ---- focal loss -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def focal_case(shape, alpha, beta):
    pred, tgt, outside, mz = R.focal_inputs(shape)
    return (pred, tgt, outside, mz) + R.focal_ref(pred, tgt, alpha, beta)


@pytest.mark.parametrize("shape", R.FOCAL_SHAPES)
@pytest.mark.parametrize("alpha,beta", R.FOCAL_EXPONENTS)
def test_focal_loss_at_any_exponents(cuda, alpha, beta, shape):
    """(2, 4) is the only pair the other tests run: x * x and x2 * x2.  (1, 4) takes `x` and powf(x, 0); (3, 2) powf(x, 3) next to
    x * x; (1.5, 2.5) `powf` everywhere.  Loss (1e-4 relative, as test_focal_loss), positive count, and the gradient by element:
    |g - ref| <= rtol |ref| + bound with FOCAL_RTOL at integer exponents and heads_refs.FOCAL_POW_RTOL = 4 x 1.96e-7 (measured on
    the host, see there) at (1.5, 2.5).  Targets 1.5 and -0.1 take no part; -0.0 is a 0."""
    import test_gpu_heads as TH
    from dcd_amd import ops
    from grad_scales import assert_close_by_element
    pred, tgt, outside, mz, ref_loss, ref_np, g64, bound = focal_case(shape, alpha, beta)
    p = torch.from_numpy(pred).to(cuda).requires_grad_()
    loss, npos = ops.focal_loss(p, torch.from_numpy(tgt).to(cuda), alpha, beta)
    assert npos.item() == ref_np
    assert abs(loss.item() - ref_loss) <= 1e-4 * abs(ref_loss), (loss.item(), ref_loss)
    loss.backward()
    for cell in outside:
        assert p.grad[cell] == 0 and g64[cell] == 0
    assert p.grad[mz] != 0
    integer = float(alpha).is_integer() and float(beta).is_integer()
    rtol = TH.FOCAL_RTOL if integer else R.FOCAL_POW_RTOL
    what = "focal (%s, %s) %s" % (alpha, beta, shape)
    worst = assert_close_by_element(p.grad, g64, rtol, bound, what)
    print("%s: worst |g - ref| / (%.2e |ref| + bound) = %.3f" % (what, rtol, worst))


@pytest.mark.parametrize("alpha,beta", R.FOCAL_EXPONENTS)
def test_focal_targets_outside_the_unit_interval_and_nothing_at_all(cuda, alpha, beta):
    """One block, so the sums are exact statements: targets 1.5 and -0.1 give a loss of exactly 0, no gradient, no positive;
    -0.0 gives the bits of 0.0; an empty tensor gives (0, 0)."""
    from dcd_amd import ops
    p = torch.tensor([0.3, 0.7, 0.9], device=cuda).requires_grad_()
    loss, npos = ops.focal_loss(p, torch.tensor([1.5, -0.1, 1.0 + 2.0 ** -23], device=cuda), alpha, beta)
    loss.backward()
    assert loss.item() == 0 and npos.item() == 0 and (p.grad == 0).all()
    res = []
    for z in (0.0, -0.0):
        p = torch.tensor([0.3, 0.6], device=cuda).requires_grad_()
        loss, npos = ops.focal_loss(p, torch.tensor([z, 1.0], device=cuda), alpha, beta)
        loss.backward()
        res.append((loss.detach(), npos, p.grad))
        assert npos.item() == 1 and loss.item() > 0 and (p.grad != 0).all()
    for a, b_ in zip(*res):
        assert torch.equal(_bits(a.reshape(-1)), _bits(b_.reshape(-1)))
    for shape in ((0,), (0, 1, 24, 80)):
        p = torch.empty(shape, device=cuda).requires_grad_()
        loss, npos = ops.focal_loss(p, torch.empty(shape, device=cuda), alpha, beta)
        assert loss.item() == 0 and npos.item() == 0
        loss.backward()
        assert p.grad.shape == p.shape


# ---- IoU-3D -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder():
    import test_host_golden as HG
    from dcd_amd.model.anno_encoder import Anno_Encoder
    return Anno_Encoder(HG.small_cfg("cpu"))


@functools.lru_cache(maxsize=None)
def scene_case(where):
    """(scenes, boxes, fp32 corners a and b, float64 oracle on those corners, E_ref, delta) -- computed once."""
    scenes = R.iou3d_scenes()
    A, Bx = [s["a"] for s in scenes], [s["b"] for s in scenes]
    if where == "moved":
        A, Bx = [R.moved(x, 0.7, 20.0, 60.0) for x in A], [R.moved(x, 0.7, 20.0, 60.0) for x in Bx]
    a, b = R.encode(encoder(), A), R.encode(encoder(), Bx)
    ref = R.oracle_iou3d(a, b).numpy()
    e_ref = np.abs(R.iou3d_fp32(a.numpy(), b.numpy()).astype(np.float64) - ref).max()
    delta = max(np.abs(a.double().numpy() - R.corners64(A)).max(), np.abs(b.double().numpy() - R.corners64(Bx)).max())
    return scenes, A, Bx, a, b, ref, e_ref, delta


def run_iou3d(cuda, a, b, N=None):
    """`dcd_iou3d` on the first N pairs into N + 64 pre-filled rows; rows >= N and the padding must stay."""
    N = a.shape[0] if N is None else N
    out = Padded(cuda, (N + 64,))
    ad, bd = a.to(cuda).contiguous(), b.to(cuda).contiguous()
    assert _call("dcd_iou3d", ad, ad.data_ptr(), bd.data_ptr(), N, out.ptr()) == 0
    torch.cuda.synchronize()
    out.assert_padding_untouched("iou3d N=%d" % N)
    assert (out.view[N:] == ODD).all(), "iou3d N=%d: rows >= N written" % N
    return out.view[:N].cpu().double().numpy()


@pytest.mark.parametrize("where", ["origin", "moved"])
def test_iou3d_known_answers(cuda, where):
    """Answers that need no clipping (heads_refs.iou3d_scenes; the oracle is held to the same table on the host): identical,
    disjoint, a shared edge, a shared corner, contained either way, a quarter turn, crossed bars, the octagon, half and no common
    height -- near the origin, and the same scenes turned by 0.7 rad and moved to (x, z) = (20, 60).
    Against the float64 oracle on the SAME fp32 corners: max(4 E_ref, 8 * 2^-24), E_ref the fp32 formula in a local frame on these
    scenes.  Against the closed form: that plus `corner_rounding_bound` of the corners' measured distance from their float64
    values (zero near the origin but for the octagon; 60 m away a corner is rounded by up to 2e-6 m, which the kernel cannot undo).
    The zeros are exact.  With the target's bottom corners in reverse order the clip's sign rule turns over: the same value."""
    scenes, A, Bx, a, b, ref, e_ref, delta = scene_case(where)
    bar = max(4 * e_ref, R.FLOOR)
    got = run_iou3d(cuda, a, b)
    rev = b.clone()
    rev[:, 0:4], rev[:, 4:8] = b[:, [3, 2, 1, 0]], b[:, [7, 6, 5, 4]]
    got_rev = run_iou3d(cuda, a, rev)
    print("iou3d scenes, %s: E %.2e, reversed %.2e, E_ref %.2e, bar %.2e, corner rounding %.2e m" % (
        where, np.abs(got - ref).max(), np.abs(got_rev - ref).max(), e_ref, bar, delta))
    for i, s in enumerate(scenes):
        for g_, nm in ((got[i], s["name"]), (got_rev[i], s["name"] + ", reversed")):
            assert abs(g_ - ref[i]) <= bar, (nm, g_, ref[i], bar)
            assert abs(g_ - s["expected"]) <= bar + R.corner_rounding_bound(A[i], Bx[i], delta), (nm, g_, s["expected"])
            if s["zero"]:
                assert g_ == 0.0, (nm, g_)


@pytest.mark.parametrize("N", [1, 64, 65])
def test_iou3d_around_the_block_size(cuda, N):
    """One lane per pair in blocks of 64: the first N of 65 pairs (the scenes, repeated) give the values of the full run, bit for
    bit, and nothing is written behind them."""
    _, _, _, a, b, ref, _, _ = scene_case("moved")
    reps = -(-65 // a.shape[0])
    a65, b65 = a.repeat(reps, 1, 1)[:65], b.repeat(reps, 1, 1)[:65]
    full = run_iou3d(cuda, a65, b65)
    assert np.array_equal(run_iou3d(cuda, a65, b65, N), full[:N])
    assert np.abs(full - np.tile(ref, reps)[:65]).max() <= R.FLOOR * 4
    assert _call("dcd_iou3d", torch.zeros(1, device=cuda), None, None, 0, None) == 0          # nothing to do, nothing to read


@functools.lru_cache(maxsize=None)
def depth_case(z):
    A, Bx = R.random_pairs(z, 256, seed=int(z))
    a, b = R.encode(encoder(), A), R.encode(encoder(), Bx)
    ref = R.oracle_iou3d(a, b).numpy()
    return a, b, ref, np.abs(R.iou3d_fp32(a.numpy(), b.numpy()).astype(np.float64) - ref).max()


@pytest.mark.parametrize("z", [5.0, 40.0, 80.0])
def test_iou3d_accuracy_with_depth(cuda, z):
    """256 random car-sized pairs at depth z (heads_refs.random_pairs) against `oracle/torch_ops.iou_3d` in float64 on the same
    corners.  Yardstick E_ref: the kernel's formula in numpy fp32 on corners translated by the target's corner 0; bar
    max(4 E_ref, 8 * 2^-24) absolute (the idiom of test_gpu_gmw_refine.py).  On absolute camera coordinates the products of the edge
    functions and the shoelace sums are of order z^2 and their roundings do not cancel: the same formula then loses about 1e-5 at 40 m
    and 2e-5 to 6e-5 at 80 m (iou3d_fp32(local=False); test_heads_refs.py), 10 to 60 times the bar."""
    a, b, ref, e_ref = depth_case(z)
    assert (ref > 0.05).sum() >= 128 and (ref == 0).sum() < 64
    got = run_iou3d(cuda, a, b)
    err, bar = np.abs(got - ref).max(), max(4 * e_ref, R.FLOOR)
    print("iou3d at %g m: E %.2e (pair %d, IoU %.4f), E_ref %.2e, bar %.2e" % (z, err, int(np.abs(got - ref).argmax()),
                                                                                ref[np.abs(got - ref).argmax()], e_ref, bar))
    assert err <= bar, (z, err, e_ref, bar)
