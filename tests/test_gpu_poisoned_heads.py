"""The kernels of csrc/heads.hip and csrc/loss_rows.hip through the C ABI on poisoned, guarded buffers (tests/arena.py).

As tests/test_gpu_poisoned_backbone.py does for the backbone: every input lies between guard words of NaN, every output and every
workspace (of exactly the advertised byte count) is poisoned, the status is 0, and `Arena.check` judges what the value tests
cannot see -- a write outside a buffer, a changed input, an output element that was not written.  The result is then held to the
SAME reference at the SAME bound as the kernel's value test, cited at each assert.

Where the code promises sums in a fixed order (head_rows: "rows in order (reproducible)"; context_norm; the loss rows' column sums)
the call runs a second time on zero-filled outputs and must give the same bits.  dcd_focal_loss, dcd_edge_depth_backward and the
scatters combine partial sums with atomics and are held to their bounds only.

No index here makes a kernel address memory outside its buffers, except those include/dcd_hip.h documents as dropped
(dcd_poi_gather, dcd_poi_scatter_add, dcd_patch_scatter_add).  dcd_edge_depth_backward gets the forward's own pair_idx.

Top-K: (2, 3, 6, 11, 50) with more than 128 equal keys (198 over the image) runs the ranked tie path and the merge's rule; the
serial tie path counts equal keys inside ONE class map, and H W = 66 cannot reach it, so (1, 2, 10, 20, 50) with 150 equal keys
in one class map of 200 cells runs beside it.

The negative controls were tried on an MI355X on copies of this file.  With the top-K workspace four bytes short
(`ar.scratch(n - 4, ...)`, the size argument as before) test_heatmap_topk[case0] fails with "back guard of scratch 'workspace'
overwritten: 1 words, the first at float offset 599" -- the last entry of the class index list; the same copy without
`ar.check(what)` passes: every value is still right, only the arena sees it.  An output element that a call does not write, an
input it changes and a write into the pad bytes of a byte mask are stopped in host stand-ins, in tests/test_arena.py."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import heads_refs as R
from arena import Arena
from test_gpu_poisoned_backbone import _close, _lib_and_stream, _ptr, _same

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ edge depth
@functools.lru_cache(maxsize=None)
def edge_problem(N, K, topk):
    """tests/test_gpu_heads.py's `synth_objects` and the oracle's answer, once per case (do not modify)."""
    import test_gpu_heads as TH
    from oracle import heads_oracle as ho
    kps, k3, rot, P, _ = TH.synth_objects(N, K, seed=N + K, noise=0.3)
    with_mask = topk > 0 and K != 92
    kmask = (np.random.RandomState(K).rand(N, K) > 0.2) if with_mask else None
    ref, rmask, ridx = ho.pairs_kpts_depth(kps, k3, rot, P, kmask=kmask, training=topk > 0, num_k=topk)
    return kps, k3, rot.reshape(N), P, kmask, ref, rmask, ridx


def _edge_forward(cuda, N, K, topk, poison=True):
    L, st = _lib_and_stream(cuda)
    kps, k3, rot, P, kmask, _, _, _ = edge_problem(N, K, topk)
    M = topk if topk else K * (K - 1) // 2
    ar = Arena(cuda, poison)
    d = [ar.place(torch.from_numpy(a), n) for a, n in ((kps, "kps"), (k3, "kps3d"), (rot, "rot_y"), (P, "P"))]
    km = ar.place(torch.from_numpy(kmask.astype(np.uint8)), "kmask") if kmask is not None else None
    depth = ar.out((N, M), "depth")
    idx = ar.out((N, M), "pair_idx", dtype=torch.int32) if topk else None
    pm = ar.out((N, M), "pair_mask") if km is not None else None
    status = L.dcd_edge_depth_forward(st, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), _ptr(km), N, K, topk,
                                      2.0, 80.0, 0, 1, depth.data_ptr(), _ptr(idx), _ptr(pm))
    what = "dcd_edge_depth_forward N=%d K=%d topk=%d" % (N, K, topk)
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    return depth.cpu(), None if idx is None else idx.cpu(), None if pm is None else pm.cpu()


EDGE_CASES = [(3, 2, 0), (3, 2, 1),                   # one pair
              (3, 10, 0), (3, 10, 45),                # every pair selected
              (2, 73, 1500),                          # kmask given, pair_mask taken; the register network (4 096 padded pairs)
              (2, 92, 1500),                          # kmask and pair_mask NULL; the LDS network (8 192 padded pairs)
              (2, 128, 0), (2, 128, 200)]             # the header's K <= 128, with a top-k: 99 584 bytes of dynamic LDS


@pytest.mark.parametrize("N,K,topk", EDGE_CASES)
def test_edge_depth_forward(cuda, N, K, topk):
    """oracle.heads_oracle.pairs_kpts_depth on `synth_objects`: pair indices and pair mask bit-exact, depth rtol = atol = 2e-4
    (test_edge_depth_eval, test_edge_depth_train_topk_exact)."""
    _, _, _, _, kmask, ref, rmask, ridx = edge_problem(N, K, topk)
    depth, idx, pm = _edge_forward(cuda, N, K, topk)
    if topk:
        assert np.array_equal(_np(idx).astype(np.int64), ridx), "pair indices must be bit-exact"
    if kmask is not None:
        assert np.array_equal(_np(pm), rmask), "pair mask must be bit-exact"
    np.testing.assert_allclose(_np(depth), ref, rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("N,K,topk", [(3, 10, 0), (2, 73, 1500), (2, 128, 200)])
def test_edge_depth_backward(cuda, N, K, topk):
    """Against the float64 autograd restatement of test_edge_depth_backward_matches_autograd at 1e-3 of each object's own maximum;
    grad_kps[..., 0] exactly 0.  A third of grad_depth is exactly 0; pair_idx is the forward's own output."""
    L, st = _lib_and_stream(cuda)
    kps, k3, rot, P, _, _, _, _ = edge_problem(N, K, topk)
    _, idx, _ = _edge_forward(cuda, N, K, topk)
    M = topk if topk else K * (K - 1) // 2
    g = torch.Generator().manual_seed(K)
    gd = torch.randn(N, M, generator=g)
    gd.view(-1)[::3] = 0.0
    ar = Arena(cuda)
    d = [ar.place(torch.from_numpy(a), n) for a, n in ((kps, "kps"), (k3, "kps3d"), (rot, "rot_y"), (P, "P"))]
    dgd = ar.place(gd, "grad_depth")
    didx = ar.place(idx, "pair_idx") if topk else None
    gk, gk3 = ar.out((N, K, 2), "grad_kps"), ar.out((N, K, 3), "grad_kps3d")
    status = L.dcd_edge_depth_backward(st, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), dgd.data_ptr(), _ptr(didx),
                                       N, K, topk, 2.0, 80.0, 0, gk.data_ptr(), gk3.data_ptr())
    assert status == 0, status
    ar.check("dcd_edge_depth_backward N=%d K=%d topk=%d" % (N, K, topk))
    A = torch.from_numpy(kps).double().requires_grad_()
    Bk = torch.from_numpy(k3).double().requires_grad_()
    Pt, r = torch.from_numpy(P).double(), torch.from_numpy(rot).double().view(N, 1)
    v = (A[:, :, 1] - Pt[:, None, 1, 2]) / Pt[:, None, 1, 1]
    C = Bk[:, :, 0] * torch.sin(r) - Bk[:, :, 2] * torch.cos(r)
    H2 = v * C
    iu = torch.triu_indices(K, K, 1)
    hm = (Bk[:, iu[0], 1] - Bk[:, iu[1], 1]) + (H2[:, iu[0]] - H2[:, iu[1]])
    dv = (v[:, iu[0]] - v[:, iu[1]]).abs()
    zz = (hm.abs() / dv.clamp_min(1e-10)).clamp_min(2.0).clamp_max(80.0)
    if topk:
        zz = zz.gather(-1, idx.long())
    (zz * gd.double()).sum().backward()
    for got, ref, nm in ((gk.cpu(), A.grad, "kps"), (gk3.cpu(), Bk.grad, "kps3d")):
        obj_err = (got.double() - ref).abs().amax(dim=(1, 2))
        obj_scale = ref.abs().amax(dim=(1, 2))
        print("edge depth backward %s K=%d topk=%d: worst per-object error / maximum %.2e" % (nm, K, topk, (obj_err / obj_scale).max().item()))
        assert (obj_scale > 0).all() and (obj_err <= 1e-3 * obj_scale).all(), (nm, (obj_err / obj_scale).tolist())
    assert A.grad[..., 0].abs().max().item() == 0 and gk.cpu()[..., 0].abs().max().item() == 0


# ------------------------------------------------------------------------------------------------------ pointwise losses
@functools.lru_cache(maxsize=None)
def focal_case(n):
    """n elements of `heat_and_target` with a positive in front, and heads_refs.focal_ref at (2, 4) (do not modify)."""
    import test_gpu_heads as TH
    pred, tgt = TH.heat_and_target(1, 24, 80, seed=n)
    pred, tgt = pred.reshape(-1)[:n].copy(), tgt.reshape(-1)[:n].copy()
    tgt[0] = 1.0
    return (pred, tgt) + R.focal_ref(pred, tgt, 2, 4)


@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("n", [1, 255, 1030])
def test_focal_loss(cuda, n, with_grad):
    """`out` (two floats) enters as NaN: the callee's zero-fill is what is tested.  heads_refs.focal_ref as in
    test_focal_loss_at_any_exponents: positives exact, loss 1e-4 relative, gradient by element within FOCAL_RTOL |ref| + bound."""
    import test_gpu_heads as TH
    from grad_scales import assert_close_by_element
    L, st = _lib_and_stream(cuda)
    pred, tgt, ref_loss, ref_np, g64, bound = focal_case(n)
    ar = Arena(cuda)
    p, t = ar.place(torch.from_numpy(pred), "pred"), ar.place(torch.from_numpy(tgt), "target")
    out = ar.out((2,), "out")
    grad = ar.out((n,), "grad_pred") if with_grad else None
    assert L.dcd_focal_loss(st, p.data_ptr(), t.data_ptr(), n, 2.0, 4.0, out.data_ptr(), _ptr(grad)) == 0
    ar.check("dcd_focal_loss n=%d grad=%s" % (n, with_grad))
    loss, npos = out.cpu().tolist()
    assert npos == ref_np
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss), (loss, ref_loss)
    if with_grad:
        assert_close_by_element(grad, g64, TH.FOCAL_RTOL, bound, "focal gradient n=%d" % n)


@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("N", [1, 63, 65])
def test_giou_loss(cuda, N, with_grad):
    """`_giou64` under autograd at test_giou_loss's bars (losses and ious rtol 1e-5 + 1e-6, gradient rows 1e-4 of the row's
    maximum + 1e-7), inputs of test_giou_around_the_block_size."""
    import test_gpu_heads as TH
    from oracle import heads_oracle as ho
    L, st = _lib_and_stream(cuda)
    rng = np.random.RandomState(N)
    pred = rng.uniform(0, 30, (N, 4)).astype(np.float32)
    tgt = rng.uniform(0.5, 30, (N, 4)).astype(np.float32)
    pred[0] = 0.0
    pred[N - 1, 0] = tgt[N - 1, 0]
    ar = Arena(cuda)
    p, t = ar.place(torch.from_numpy(pred), "pred"), ar.place(torch.from_numpy(tgt), "target")
    losses, ious = ar.out((N,), "losses"), ar.out((N,), "ious")
    grad = ar.out((N, 4), "grad_pred") if with_grad else None
    assert L.dcd_giou_loss(st, p.data_ptr(), t.data_ptr(), N, losses.data_ptr(), ious.data_ptr(), _ptr(grad)) == 0
    ar.check("dcd_giou_loss N=%d grad=%s" % (N, with_grad))
    pt, tt = torch.from_numpy(pred).double().requires_grad_(), torch.from_numpy(tgt).double()
    l64 = TH._giou64(pt, tt)
    l64.sum().backward()
    np.testing.assert_allclose(_np(losses), l64.detach().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(_np(ious), ho.giou_loss(pred, tgt)[1], rtol=1e-5, atol=1e-6)
    if with_grad:
        row_err = (grad.cpu().double() - pt.grad).abs().max(dim=1).values
        row_bar = 1e-4 * pt.grad.abs().max(dim=1).values + 1e-7
        assert (row_err <= row_bar).all(), (N, (row_err / row_bar).max().item())


def test_iou3d(cuda):
    """65 pairs of heads_refs.random_pairs at 40 m against the float64 oracle on the same corners at max(4 E_ref, 8 * 2^-24)
    (test_iou3d_accuracy_with_depth)."""
    import test_gpu_heads_edges as HE
    L, st = _lib_and_stream(cuda)
    A, Bx = R.random_pairs(40.0, 65, seed=40)
    a, b = R.encode(HE.encoder(), A), R.encode(HE.encoder(), Bx)
    ref = R.oracle_iou3d(a, b).numpy()
    e_ref = np.abs(R.iou3d_fp32(a.numpy(), b.numpy()).astype(np.float64) - ref).max()
    ar = Arena(cuda)
    da, db = ar.place(a, "pred_corners"), ar.place(b, "target_corners")
    out = ar.out((65,), "iou")
    assert L.dcd_iou3d(st, da.data_ptr(), db.data_ptr(), 65, out.data_ptr()) == 0
    ar.check("dcd_iou3d")
    err, bar = np.abs(_np(out).astype(np.float64) - ref).max(), max(4 * e_ref, R.FLOOR)
    assert err <= bar, (err, e_ref, bar)


# -------------------------------------------------------------------------------------------------------- heat-map decode
def _heat(shape, seed):
    import test_gpu_heads_edges as HE
    heat = HE.sigmoid_heat(shape, seed)
    heat[..., :2, :3] = 0.77                          # a plateau: ties with and without the NMS
    return heat


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 1, 1, 9), (1, 2, 9, 1)])
def test_nms_hm(cuda, shape):
    """Bit-exact against heads_refs.nms_ref (test_heatmap_decode_exact)."""
    L, st = _lib_and_stream(cuda)
    heat = _heat(shape, sum(shape))
    ar = Arena(cuda)
    h = ar.place(torch.from_numpy(heat), "heat")
    out = ar.out(shape, "out")
    assert L.dcd_nms_hm(st, h.data_ptr(), *shape, out.data_ptr()) == 0
    ar.check("dcd_nms_hm %s" % (shape,))
    assert np.array_equal(_np(out), R.nms_ref(heat))


def _topk_heat(case):
    B, C, H, W, K, ties = case
    heat = _heat((B, C, H, W), B + C + H + W + K)
    if ties == "image":                               # 198 equal keys over the image, 33 per class map
        heat.reshape(B, C, -1)[:, :, ::2] = 0.25
    elif ties == "class":                             # 150 equal keys in ONE class map of 200 cells: the serial ballot scan
        heat = (0.01 + 0.19 * np.random.RandomState(3).permutation(B * C * H * W) / (B * C * H * W)).astype(np.float32).reshape(B, C, H, W)
        heat[0, 1].reshape(-1)[5:155] = 0.25
        heat[0, 1].reshape(-1)[[0, 160, 199]] = [0.9, 0.8, 0.7]
    return heat


TOPK_CASES = [(2, 3, 6, 11, 50, None), (1, 1, 8, 16, 128, None), (1, 32, 8, 16, 128, None), (2, 3, 6, 11, 50, "image"),
              (1, 2, 10, 20, 50, "class")]


@pytest.mark.parametrize("short", [0, 256])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("case", TOPK_CASES)
def test_heatmap_topk(cuda, case, fuse, short):
    """Bit-exact against heads_refs.topk_ref (tests/test_gpu_heads_edges.py `assert_topk`), with a workspace of exactly
    dcd_heatmap_topk_workspace_bytes and of that minus the 256 bytes the entry point does not insist on."""
    L, st = _lib_and_stream(cuda)
    B, C, H, W, K, ties = case
    heat = _topk_heat(case)
    if ties == "class" and not fuse:
        assert (np.sort(heat[0, 1].ravel())[::-1][3:153] == np.float32(0.25)).all()
    ref = R.topk_ref(R.nms_ref(heat) if fuse else heat, K)
    n = L.dcd_heatmap_topk_workspace_bytes(B, C, H, W, K) - short
    ar = Arena(cuda)
    h = ar.place(torch.from_numpy(heat), "heat")
    outs = [ar.out((B, K), nm, dtype=torch.int64 if nm == "inds" else torch.float32) for nm in ("scores", "inds", "clses", "ys", "xs")]
    ws = ar.scratch(n, "workspace")
    status = L.dcd_heatmap_topk(st, h.data_ptr(), B, C, H, W, K, fuse, *[o.data_ptr() for o in outs], ar.ptr(ws), n)
    what = "dcd_heatmap_topk %s fuse=%d workspace %d" % (case, fuse, n)
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    for got, want, nm in zip(outs, ref, ("scores", "inds", "clses", "ys", "xs")):
        got = _np(got)
        assert got.dtype == want.dtype and np.array_equal(got, want), "%s: %s differs at %s" % (what, nm, np.argwhere(got != want)[:4].tolist())


# -------------------------------------------------------------------------------------------------------- gather, scatter
def test_poi_gather(cuda):
    """Exact against heads_refs.gather_ref; -1, H W and duplicates in the list, rows with out-of-range indices exactly 0
    (test_out_of_range_indices_gather_zero_and_scatter_nothing)."""
    L, st = _lib_and_stream(cuda)
    B, C, H, W, M = 2, 5, 6, 11, 7
    g = torch.Generator().manual_seed(1)
    feat = torch.randn(B, C, H, W, generator=g)
    index = torch.tensor([[3, -1, 65, 3, H * W, 0, 3], [10, 10, H * W, 64, -1, 20, 10]])
    ar = Arena(cuda)
    f, i = ar.place(feat, "feat"), ar.place(index, "index")
    out = ar.out((B, M, C), "out")
    assert L.dcd_poi_gather(st, f.data_ptr(), i.data_ptr(), B, C, H, W, M, out.data_ptr()) == 0
    ar.check("dcd_poi_gather")
    got = out.cpu()
    assert torch.equal(got.double(), R.gather_ref(feat.view(B, C, H * W), index))
    bad = (index < 0) | (index >= H * W)
    assert int(bad.sum()) == 4 and (got[bad] == 0).all()


@pytest.mark.parametrize("M", [63, 64])
def test_scatter_adds(cuda, M):
    """dcd_poi_scatter_add (both routes: M < 64 and M >= 64) and dcd_patch_scatter_add onto a non-zero map placed in place; the
    values and the index list must not change.  Bar: heads_refs.assert_scatter, |got - ref| <= n 2^-24 S per cell and the bits of
    the pre-fill elsewhere (test_poi_scatter_add_on_both_sides_of_the_route_switch, test_patch_scatter_add)."""
    import test_gpu_heads_edges as HE
    L, st = _lib_and_stream(cuda)
    B, H, W, C = HE.B, HE.H, HE.W, 5
    base, vals, index = HE.scatter_problem(M, C, seed=M)
    index[0, 5], index[1, 7] = -1, H * W                  # documented as dropped
    ref, n, S = R.scatter_ref(base, vals, index)
    ar = Arena(cuda)
    v, i = ar.place(vals, "grad_out"), ar.place(index, "index")
    out = ar.place(base, "grad_feat", inplace=True)
    assert L.dcd_poi_scatter_add(st, v.data_ptr(), i.data_ptr(), B, C, H, W, M, out.data_ptr()) == 0
    ar.check("dcd_poi_scatter_add M=%d" % M)
    R.assert_scatter(out.cpu(), base, ref, n, S, "poi scatter M=%d" % M)

    g0 = torch.Generator().manual_seed(50 + M)
    first = torch.randint(0, HE.PLANE - 2 * HE.PITCH - 2, (B, M), generator=g0)
    first[0, 0], first[1, 0], first[1, 4], first[0, 5] = HE.PLANE - 2 * HE.PITCH + 3, -1, HE.PLANE + 5, -100    # taps dropped one by one
    first[:, 3] = first[:, 2]
    pbase = torch.randn(B, C, HE.PLANE, generator=g0)
    gp = torch.randn(B, C * 9, M, generator=g0)
    ref, n, S = R.patch_scatter_ref(pbase, gp, first, HE.PITCH)
    ar = Arena(cuda)
    dg, df = ar.place(gp, "grad_patches"), ar.place(first, "base")
    out = ar.place(pbase, "out", inplace=True)
    assert L.dcd_patch_scatter_add(st, dg.data_ptr(), df.data_ptr(), B, C, HE.PLANE, HE.PITCH, M, out.data_ptr()) == 0
    ar.check("dcd_patch_scatter_add M=%d" % M)
    R.assert_scatter(out.cpu(), pbase, ref, n, S, "patch scatter M=%d" % M)


# ----------------------------------------------------------------------------------------------------------- context norm
@pytest.mark.parametrize("rows,K", [(5, 37), (5, 64), (3, 4), (3, 100), (2, 2628), (1, 4096), (2, 4100)])
def test_context_norm(cuda, rows, K):
    """Forward, backward and relu-add against the stock formula in fp64: 2e-6 forward (and `inv`, the same expression), 1e-5
    backward (test_context_norm_kernel_against_stock_formula), relu-add at max(4 E_ref, 8 * 2^-24) of the largest |y|
    (test_context_norm_relu_add_against_float64); all three with the same bits from poisoned and from zero-filled outputs."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(rows * 10000 + K)
    x = torch.randn(rows, K, generator=g) * 2 + 0.5
    gy, res = torch.randn(rows, K, generator=g), torch.randn(rows, K, generator=g)

    def stock(x, r=None):
        m, v = torch.mean(x, 1, keepdim=True), torch.var(x, 1, keepdim=True)
        inv = 1.0 / torch.sqrt(v + 1e-3)
        y = (x - m) * inv
        return (y, inv) if r is None else F.relu(y) + r
    xd = x.double().requires_grad_()
    ref, ref_inv = stock(xd)
    ref.backward(gy.double())
    ref = ref.detach()
    got = []
    for poison in (True, False):
        ar = Arena(cuda, poison)
        dx = ar.place(x, "x")
        y, inv = ar.out((rows, K), "y"), ar.out((rows,), "inv")
        assert L.dcd_context_norm_forward(st, dx.data_ptr(), y.data_ptr(), inv.data_ptr(), rows, K, 1e-3) == 0
        ar.check("dcd_context_norm_forward (%d, %d) poison %d" % (rows, K, poison))
        y_cpu, inv_cpu = y.cpu(), inv.cpu()
        ar = Arena(cuda, poison)
        dgy, dy, dinv = ar.place(gy, "grad_y"), ar.place(y_cpu, "y"), ar.place(inv_cpu, "inv")
        gx = ar.out((rows, K), "grad_x")
        assert L.dcd_context_norm_backward(st, dgy.data_ptr(), dy.data_ptr(), dinv.data_ptr(), gx.data_ptr(), rows, K) == 0
        ar.check("dcd_context_norm_backward (%d, %d) poison %d" % (rows, K, poison))
        ar = Arena(cuda, poison)
        dx, dr = ar.place(x, "x"), ar.place(res, "residual")
        ya = ar.out((rows, K), "y")
        assert L.dcd_context_norm_relu_add_forward(st, dx.data_ptr(), dr.data_ptr(), ya.data_ptr(), rows, K, 1e-3) == 0
        ar.check("dcd_context_norm_relu_add_forward (%d, %d) poison %d" % (rows, K, poison))
        got.append((y_cpu, inv_cpu, gx.cpu(), ya.cpu()))
    y, inv, gx, ya = got[0]
    _close(y, ref, "context_norm forward", 2e-6)
    _close(inv, ref_inv.detach().view(rows), "context_norm inv", 2e-6)
    _close(gx, xd.grad, "context_norm backward", 1e-5)
    ref_a = stock(x.double(), res.double())
    scale = ref_a.abs().max().item()
    e_ref = (stock(x, res).double() - ref_a).abs().max().item() / scale
    err = (ya.double() - ref_a).abs().max().item() / scale
    assert err <= max(4 * e_ref, R.FLOOR), (err, e_ref)
    for a, b, nm in zip(got[0], got[1], ("y", "inv", "grad_x", "relu-add y")):
        _same(a, b, "context_norm %s (%d, %d)" % (nm, rows, K))


# -------------------------------------------------------------------------------------------------------------- head rows
SIX_HEADS = ([0, 0, 1, 2, 2, 2], [4, 2, 20, 3, 1, 219])
HEAD_ROWS_CASES = [(3, 7, 64) + SIX_HEADS + (None,),                      # ragged R
                   (3, 257, 256) + SIX_HEADS + (None,),                   # the weight gradient's second 256-row chunk holds one row
                   (3, 5, 4, [0, 2], [3, 2], 1),                          # trunk 1 feeds no head: zeros; the second head has no bias
                   (1, 5, 8, [0], [1024], None),                          # the C limit and the g[4][1024] tile
                   (16, 5, 256, list(range(16)), [2] * 16, None)]         # the T limit: exactly 64 KB of LDS in the forward


@pytest.mark.parametrize("T,R,K,trunk_of,outs,no_bias", HEAD_ROWS_CASES)
def test_head_rows(cuda, T, R, K, trunk_of, outs, no_bias):
    """dcd_head_rows_forward / _backward against one fp64 F.linear per head: 2e-6 forward, 5e-6 each gradient, the feature
    gradient trunk by trunk (test_head_rows_equal_one_linear_per_head); the same bits from poisoned and zero-filled outputs."""
    from dcd_amd import _lib
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(T * 1000 + R)
    H, C = len(outs), sum(outs)
    feat = torch.randn(T, R, K, generator=g)
    ws = [torch.randn(o, K, generator=g) * 0.1 for o in outs]
    bs = [None if j == no_bias else torch.randn(o, generator=g) for j, o in enumerate(outs)]
    gy = torch.randn(R, C, generator=g)
    fd = feat.double().requires_grad_()
    wd = [w.double().requires_grad_() for w in ws]
    bd = [None if b is None else b.double().requires_grad_() for b in bs]
    ref = torch.cat([F.linear(fd[t], w, b) for t, w, b in zip(trunk_of, wd, bd)], dim=1)
    ref.backward(gy.double())

    def args(ar, backward):
        a = _lib.HeadRowsArgs()
        a.n_heads, a.T, a.R, a.K, a.C = H, T, R, K, C
        c = 0
        for j in range(H):
            a.trunk[j], a.ch0[j], a.out[j] = trunk_of[j], c, outs[j]
            a.weight[j] = ar.place(ws[j], "weight %d" % j).data_ptr()
            a.bias[j] = None if bs[j] is None else ar.place(bs[j], "bias %d" % j).data_ptr()
            c += outs[j]
        a.feat = ar.place(feat, "feat").data_ptr()
        return a

    got = []
    for poison in (True, False):
        ar = Arena(cuda, poison)
        a = args(ar, False)
        y = ar.out((R, C), "y")
        a.y = y.data_ptr()
        assert L.dcd_head_rows_forward(st, ctypes.byref(a)) == 0
        ar.check("dcd_head_rows_forward T=%d R=%d K=%d poison %d" % (T, R, K, poison))
        ar = Arena(cuda, poison)
        a = args(ar, True)
        a.grad_y = ar.place(gy, "grad_y").data_ptr()
        gf = ar.out((T, R, K), "grad_feat")
        a.grad_feat = gf.data_ptr()
        gws = [ar.out((o, K), "grad_weight %d" % j) for j, o in enumerate(outs)]
        gbs = [None if bs[j] is None else ar.out((o,), "grad_bias %d" % j) for j, o in enumerate(outs)]
        for j in range(H):
            a.grad_weight[j], a.grad_bias[j] = gws[j].data_ptr(), _ptr(gbs[j])
        assert L.dcd_head_rows_backward(st, ctypes.byref(a)) == 0
        ar.check("dcd_head_rows_backward T=%d R=%d K=%d poison %d" % (T, R, K, poison))
        got.append([y.cpu(), gf.cpu()] + [t.cpu() for t in gws] + [t.cpu() for t in gbs if t is not None])
    y, gf = got[0][0], got[0][1]
    _close(y, ref.detach(), "head rows forward", 2e-6)
    for a_, b_ in zip(got[0][2:], [w.grad for w in wd] + [b.grad for b in bd if b is not None]):
        assert a_.shape == b_.shape and (a_.double() - b_).abs().max().item() <= 5e-6 * max(b_.abs().max().item(), 1e-3)
    assert (gf.double() - fd.grad).abs().max().item() <= 5e-6 * max(fd.grad.abs().max().item(), 1e-3)
    for t in range(T):
        if t in trunk_of:
            assert (gf[t].double() - fd.grad[t]).abs().max().item() <= 5e-6 * fd.grad[t].abs().max().item(), t
        else:
            assert not gf[t].any() and not fd.grad[t].any(), "a trunk that feeds no head has a zero gradient, every element written"
    for i, (a_, b_) in enumerate(zip(got[0], got[1])):
        _same(a_, b_, "head rows output %d" % i)


# -------------------------------------------------------------------------------------------------------------- loss rows
from test_host_rows import host_rows  # noqa: E402,F401  (the fixture: the host build of csrc/loss_rows_math.h)

LR_IOU3D = 10                                             # include/dcd_hip.h: column 10 is the 3-D IoU, a logging metric


@functools.lru_cache(maxsize=None)
def rows_problem(variant):
    """test_host_rows._rows_inputs for one variant, the spec and typed targets of the product, and seeded weights of the column
    sums (do not modify)."""
    import test_host_rows as TR
    empty_image, mixed_flags, all_empty = variant
    loss, tv, pois = TR._rows_inputs(empty_image, mixed_flags)
    if all_empty:
        tv = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in tv.items()}
        tv['reg_mask'].zero_()
    keep = []
    _, spec = TR._host_args(loss, tv, pois.detach().contiguous(), keep)
    gs = torch.from_numpy(np.random.RandomState(5).uniform(0.5, 1.5, 25).astype(np.float32))
    return loss, tv, pois.detach().contiguous(), spec, tuple(keep[:-1]), keep[-1].contiguous(), gs


def _rows_chain(cuda, variant, poison):
    """The header's call order, each call in its own arena, the outputs of one call re-placed as inputs of the next."""
    from dcd_amd import ops
    L, st = _lib_and_stream(cuda)
    _, _, pois, spec, targets, dim_mean, gs = rows_problem(variant)
    B, M, C = pois.shape
    BM, K, NP = B * M, spec["K"], spec["NP"]
    what = "loss rows %s poison %d: " % (variant, poison)

    def begin():
        ar = Arena(cuda, poison)
        dev = [ar.place(t, name) for (name, _), t in zip(ops._ROWS_TARGETS, targets)]
        return ar, ops._LossRows._args(spec, ar.place(pois, "pois"), dev, ar.place(dim_mean, "dim_mean"))

    ar, a = begin()
    kps, kps3d = ar.out((2, BM, K, 2), "kps_pred | kps_tgt"), ar.out((2, BM, K, 3), "kps3d_pred | kps3d_tgt")
    rot, P_rows = ar.out((2, BM), "rot"), ar.out((2, BM, 3, 4), "P_rows")
    kmask = ar.out((2, BM, K), "kmask", dtype=torch.uint8)
    a.kps_pred, a.kps_tgt, a.kps3d_pred, a.kps3d_tgt = kps[0].data_ptr(), kps[1].data_ptr(), kps3d[0].data_ptr(), kps3d[1].data_ptr()
    a.rot, a.P_rows, a.kmask = rot.data_ptr(), P_rows.data_ptr(), kmask.data_ptr()
    assert L.dcd_loss_rows_prepare(st, ctypes.byref(a)) == 0
    ar.check(what + "dcd_loss_rows_prepare")
    kps_c, kps3d_c, rot_c, P_c, kmask_c = kps.cpu(), kps3d.cpu(), rot.cpu(), P_rows.cpu(), kmask.cpu()
    assert torch.equal(rot_c[0], rot_c[1]) and torch.equal(P_c[0], P_c[1]) and torch.equal(kmask_c[0], kmask_c[1])
    assert ((kmask_c == 0) | (kmask_c == 1)).all()
    ov = rows_problem(variant)[1]['reg_mask'].bool().reshape(-1)
    first = int(ov.nonzero()[0]) if ov.any() else 0      # include/dcd_hip.h: an empty slot holds what the first annotated object gives
    assert not kmask_c[:, ~ov].any()
    for t in (kps_c, kps3d_c, P_c):
        assert torch.equal(t[:, ~ov], t[:, first:first + 1].expand(-1, int((~ov).sum()), *t.shape[2:])), what + "an empty slot of prepare"
    assert torch.equal(rot_c[:, ~ov], rot_c[:, first:first + 1].expand(-1, int((~ov).sum())))

    ar = Arena(cuda, poison)
    d = [ar.place(t.view(2 * BM, *t.shape[2:]), n) for t, n in ((kps_c, "kps"), (kps3d_c, "kps3d"), (rot_c, "rot_y"), (P_c, "P"), (kmask_c, "kmask"))]
    depth, pmask = ar.out((2, BM, NP), "depth"), ar.out((2, BM, NP), "pair_mask")
    idx = ar.out((2, BM, NP), "pair_idx", dtype=torch.int32)
    assert L.dcd_edge_depth_forward(st, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), 2 * BM, K, NP,
                                    2.0, 80.0, 0, 1, depth.data_ptr(), idx.data_ptr(), pmask.data_ptr()) == 0
    ar.check(what + "dcd_edge_depth_forward over 2 B M rows")
    depth_c, pmask_c, idx_c = depth.cpu()[0].contiguous(), pmask.cpu()[1].contiguous(), idx.cpu()[0].contiguous()

    ar, a = begin()
    a.pair_depth, a.pair_mask = ar.place(depth_c, "pair_depth").data_ptr(), ar.place(pmask_c, "pair_mask").data_ptr()
    cols, iou3d, sums = ar.out((25, BM), "cols"), ar.out((BM,), "iou3d"), ar.out((25,), "sums")
    cp, ct = ar.out((BM, 8, 3), "corners_pred"), ar.out((BM, 8, 3), "corners_tgt")
    a.cols, a.corners_pred, a.corners_tgt, a.iou3d, a.sums = cols.data_ptr(), cp.data_ptr(), ct.data_ptr(), iou3d.data_ptr(), sums.data_ptr()
    assert L.dcd_loss_rows_forward(st, ctypes.byref(a)) == 0
    ar.check(what + "dcd_loss_rows_forward")

    ar, a = begin()
    a.pair_depth, a.pair_mask = ar.place(depth_c, "pair_depth").data_ptr(), ar.place(pmask_c, "pair_mask").data_ptr()
    a.grad_sums = ar.place(gs, "grad_sums").data_ptr()
    gpois, gpair = ar.out((BM, C), "grad_pois"), ar.out((BM, NP), "grad_pair")
    a.grad_pois, a.grad_pair = gpois.data_ptr(), gpair.data_ptr()
    assert L.dcd_loss_rows_backward(st, ctypes.byref(a)) == 0
    ar.check(what + "dcd_loss_rows_backward")
    gpois_c, gpair_c = gpois.cpu(), gpair.cpu()

    ar = Arena(cuda, poison)
    d = [ar.place(t, n) for t, n in ((kps_c[0], "kps"), (kps3d_c[0], "kps3d"), (rot_c[0], "rot_y"), (P_c[0], "P"), (gpair_c, "grad_depth"),
                                     (idx_c, "pair_idx"))]
    gk, gk3 = ar.out((BM, K, 2), "grad_kps"), ar.out((BM, K, 3), "grad_kps3d")
    assert L.dcd_edge_depth_backward(st, *[t.data_ptr() for t in d], BM, K, NP, 2.0, 80.0, 0, gk.data_ptr(), gk3.data_ptr()) == 0
    ar.check(what + "dcd_edge_depth_backward")

    ar, a = begin()
    gp = ar.place(gpois_c, "grad_pois", inplace=True)
    a.grad_pois, a.grad_kps, a.grad_kps3d = gp.data_ptr(), ar.place(gk.cpu(), "grad_kps").data_ptr(), ar.place(gk3.cpu(), "grad_kps3d").data_ptr()
    assert L.dcd_loss_rows_finish(st, ctypes.byref(a)) == 0
    ar.check(what + "dcd_loss_rows_finish")
    return SimpleNamespace(sums=sums.cpu(), cols=cols.cpu(), corners=torch.stack((cp.cpu(), ct.cpu())), iou3d=iou3d.cpu(), gpois=gp.cpu(),
                           gpair=gpair_c)


ROWS_VARIANTS = [(False, False, False), (True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.parametrize("variant", ROWS_VARIANTS, ids=["plain", "empty_image", "mixed_flags", "all_empty"])
def test_loss_rows_chain(cuda, host_rows, variant):
    """prepare -> edge solver -> forward -> backward -> edge solver backward -> finish against the host build of the same header
    (test_host_rows._run_host): column sums at 2e-5 max(|ref|, 1) but for the 3-D IoU column, grad_pois at 2e-5 of the reference's
    maximum, rows of empty slots exactly 0 (test_row_kernel_arithmetic_equals_the_op_by_op_rows); the corners, the same fp32
    statements with the device's sinf / cosf / atan2f, at 2e-5 of their maximum.  Every output of every call is written for every
    slot, empty ones included (include/dcd_hip.h): no `written` mask anywhere.  The column sums run in a fixed order: the same bits
    from poisoned and from zero-filled outputs."""
    import test_host_rows as TR
    loss, tv, pois, spec, _, _, gs = rows_problem(variant)
    B, M, C = pois.shape
    sums_ref, gpois_ref, corners_ref = TR._run_host(host_rows, loss, tv, pois, gs)
    got, twin = _rows_chain(cuda, variant, True), _rows_chain(cuda, variant, False)
    _same(got.sums, twin.sums, "loss rows column sums")
    _same(got.cols, twin.cols, "loss rows columns")
    ov = tv['reg_mask'].bool().reshape(-1)
    for c in range(25):
        if c == LR_IOU3D:
            continue
        ref = float(sums_ref[c])
        assert abs(float(got.sums[c]) - ref) <= 2e-5 * max(abs(ref), 1.0), (c, float(got.sums[c]), ref)
        assert (got.cols[c][~ov] == 0).all(), "column %d: an empty slot carries a value" % c
    assert torch.isfinite(got.sums).all() and (got.cols[LR_IOU3D][~ov] == 0).all()
    _close(got.corners, corners_ref.double(), "corners", 2e-5)
    scale = gpois_ref.abs().max().item()
    err = (got.gpois.view(B, M, C) - gpois_ref).abs().max().item()
    assert err <= 2e-5 * scale, (err, scale)
    assert (got.gpois[~ov] == 0).all() and (got.gpair[~ov] == 0).all()
    if variant[2]:
        assert (got.sums == 0).all() and (got.gpois == 0).all() and (sums_ref == 0).all()
