"""Plain float64 reference of DCNv2 (3x3 / stride 1 / pad 1 / dilation 1, any deformable_groups) with the rounding points of the
one-product bf16 kernels (DCD_PREC_BF16, MODEL.FP16) made explicit.  TEST INFRASTRUCTURE, torch on the CPU.

The model.  With r(t) = t rounded to bf16 (nearest even) and col[b, c, tap, y, x] = mask * bilinear(x) (the masked sampled columns):

    forward    y    = r(W) . r(col) + b
    backward   gW   = r(dY) . r(col)^T        gcol = r(W)^T . r(dY)        gb = sum dY   (unrounded)

and everything upstream of col (grad_input, grad_offset, grad_mask) is float64 autograd of `columns` applied to gcol: sampling,
coordinate arithmetic and every sum are unrounded.  Accumulation is float64 here, fp32 in the kernels: that difference is what a
test against this reference has left to allow for.

Where the kernels round (read from the sources, dcd_amd/csrc):

  * tiled forward `dcn_fwd_tile_bf16x3<., 1>` (dcn_v2_bf16x3.inc): the weights are rounded once when they are laid out
    (`dcn_prep_weights_tile_bf16`, :113-118, the hi half of `split_pair`); a sample is v = sum of four corners times wq, where wq
    already holds the mask (:210-212, :252), and `round8(v)` (:255) rounds the finished masked column.  The mask is applied BEFORE
    the rounding.  EXCEPTION: a sample whose 2 x 2 footprint leaves the staged window (rows r0 - 4 .. r0 + TR + 3, columns
    c0 - 4 .. c0 + 35 of its TR x 32 tile) is gathered from global memory by its lane and enters through the fp32 matrix
    instruction with the UNROUNDED weights of the rescue layout (:271-304): no rounding at all for those products.  `fwd_exact`
    below is the switch for them, `tiled_forward_exact_samples` restates the window test.  And a call (or a tile) in which far samples
    dominate is computed by the exact fp32 kernel `dcn_fwd9_f32<., true>` altogether (:140-143, :230-233; dcn_v2.hip, the
    rescue pass behind `dcn_fwd_far_count`): `rounded=False`.
  * one-pass backward `dcn_bwd_sweep<DCD_PREC_BF16, 1|2|4, .>` (dcn_bwd_sweep.inc): weights rounded by
    `sweep_prep_weights_bf16_body` (:97-99, hi half), dY by `sw_round16` (:485, :711) for gcol = dcol and by `sw_round4` (:488,
    :940) for grad_weight; the masked sample `pend_col = m * val` (:698) is rounded by `sw_round4` (:705, :741) -- mask BEFORE the
    rounding again.  The far samples of a call the kernel keeps go through the same `full_dcol` / `add_dw` (:757-769, :739-756,
    :882, :902): rounded like the near ones.  Cout > 64 (NOB = 2, 4): the masked samples leave the kernel as fp32 (`col_store`,
    :495-498, :701) and grad_weight is `sgemm_bf16x3(..., one = true)` (dcn_v2.hip:2744), which rounds both operands when it
    stages them (sgemm_bf16x3.inc:60, `round8`).  A far-DOMINATED call with the hand-over armed (unknown layer, or the layer's last
    call reported many far coordinates) leaves the kernel at once (:284) and the generic fp32 kernels `dcn_bwd_input_f32` /
    `dcn_bwd_data_f32` / `dcn_bwd_weight_f32` do the whole call (dcn_v2.hip:2753-2800): `rounded=False`.
  * column-buffer path (dcn_dense.inc): `dcn_dense_im2col` writes a0 m x + ... in fp32 (:49, :67: mask before the rounding); the
    three products (forward :351-360, T = W^T dY :376-380, grad_weight :388-393) are `sgemm_bf16x3(..., one = true)` through
    `dense_gemm` (:337-341), rounding both operands as above.  T stays fp32 for col2im and the coordinate gradients.
  * the generic kernels (small maps, deformable_groups > 1, other geometries) have no one-product form: the forward is the exact
    fp32 kernel, the backward runs the split form (dcn_v2.hip:2573) -- `rounded=False`, held to the split form's 1e-4.
"""
import torch


def bf16_round(t):
    """float64 -> nearest bf16 (ties to even) -> float64.  The float32 step in between is exact whenever t is representable in
    fp32, which `exactly_fp32` asserts for the inputs this is used on; otherwise it is the double rounding the kernels also do
    (they see fp32 columns)."""
    return t.float().bfloat16().double()


def identity(t):
    return t


def columns(x, off, m, dtype=torch.float64, dg=1):
    """col[b, c, tap, y, x] = m * bilinear sample of x, evaluated in `dtype`.  The oracle's rules (oracle/dcn_v2_oracle.c, after
    cuda/dcn_v2_im2col_cuda.cu:25-54, 125-195): a sample counts iff -1 < h < H and -1 < w < W (open interval); each of the four
    corners contributes only if it lies inside the image; the cell is floor(h), floor(w).  The floor is detached: autograd then
    yields the reference's one-sided coordinate derivative (d val / d h from the corners of the cell the sample is in)."""
    B, C, H, W = x.shape
    assert C % dg == 0 and off.shape[1] == 18 * dg and m.shape[1] == 9 * dg
    x, off, m = x.to(dtype), off.to(dtype), m.to(dtype)
    cpg = C // dg
    ys = (torch.arange(H, dtype=dtype) - 1).view(1, H, 1)
    xs = (torch.arange(W, dtype=dtype) - 1).view(1, 1, W)
    groups = []
    for g in range(dg):
        xf = x[:, g * cpg:(g + 1) * cpg].reshape(B, cpg, H * W)
        taps = []
        for k in range(9):
            i, j = divmod(k, 3)
            h = ys + i + off[:, g * 18 + 2 * k]
            w = xs + j + off[:, g * 18 + 2 * k + 1]
            valid = ((h > -1) & (w > -1) & (h < H) & (w < W)).to(dtype)
            h0, w0 = torch.floor(h).detach(), torch.floor(w).detach()
            lh, lw = h - h0, w - w0
            val = 0
            for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                hh, ww = h0 + dy, w0 + dx
                inside = ((hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)).to(dtype)
                idx = (hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)).long().view(B, 1, H * W).expand(B, cpg, H * W)
                v = torch.gather(xf, 2, idx).view(B, cpg, H, W)
                val = val + v * (wt * inside).unsqueeze(1)
            taps.append(val * (valid * m[:, g * 9 + k]).unsqueeze(1))
        groups.append(torch.stack(taps, dim=2))             # B, cpg, 9, H, W
    return torch.cat(groups, dim=1)


class _Contract(torch.autograd.Function):
    """The weight contraction as the one-product kernels perform it: every operand of a matrix product passes through `r`, the
    sums are float64.  `exact` (bool, B x 9 x H x W or None): forward products of these samples are NOT rounded, neither side
    (the tiled forward's per-lane far samples); the backward never has such an exception."""

    @staticmethod
    def forward(ctx, w, col, b, r, exact):
        B, C, T, H, W = col.shape
        Co = w.shape[0]
        ctx.r = r
        ctx.save_for_backward(w, col)
        wk = w.reshape(Co, C * T)
        ck = col.reshape(B, C * T, H * W)
        if exact is None:
            y = torch.einsum("ok,bkp->bop", r(wk), r(ck))
        else:
            e = exact.view(B, 1, T, H, W).expand(B, C, T, H, W).reshape(B, C * T, H * W)
            zero = torch.zeros((), dtype=ck.dtype)
            y = torch.einsum("ok,bkp->bop", r(wk), r(torch.where(e, zero, ck))) + torch.einsum("ok,bkp->bop", wk, torch.where(e, ck, zero))
        return y.view(B, Co, H, W) + b.view(1, Co, 1, 1)

    @staticmethod
    def backward(ctx, gy):
        w, col = ctx.saved_tensors
        r = ctx.r
        B, C, T, H, W = col.shape
        Co = w.shape[0]
        g = r(gy.reshape(B, Co, H * W))
        gw = torch.einsum("bop,bkp->ok", g, r(col.reshape(B, C * T, H * W))).view_as(w)
        gcol = torch.einsum("ok,bop->bkp", r(w.reshape(Co, C * T)), g).view_as(col)
        return gw, gcol, gy.sum(dim=(0, 2, 3)), None, None


def dcn_reference(x, w, b, off, m, gy=None, dg=1, rounded=True, col_dtype=torch.float64, fwd_exact=None):
    """-> (y, grads): y float64; grads = (grad_input, grad_offset, grad_mask, grad_weight, grad_bias) in float64, or None without gy.
    rounded=False: r = identity, the plain float64 DCNv2.  col_dtype=torch.float32: the columns are evaluated in fp32 (as the
    kernels do) before they are rounded -- the two settings differ where an fp32 column and its float64 twin round to different
    bf16 neighbours."""
    xd, od, md = (t.detach().double().requires_grad_(gy is not None) for t in (x, off, m))
    wd, bd = (t.detach().double().requires_grad_(gy is not None) for t in (w, b))
    col = columns(xd, od, md, col_dtype, dg).double()
    y = _Contract.apply(wd, col, bd, bf16_round if rounded else identity, fwd_exact)
    if gy is None:
        return y.detach(), None
    grads = torch.autograd.grad(y, (xd, od, md, wd, bd), gy.double())
    return y.detach(), grads


def exactly_fp32(x, off, m, dg=1):
    """True iff the columns come out bit-identical in float32 and float64: every intermediate fits fp32's 24 bits, so the kernel's
    fp32 columns -- whatever its evaluation order, lerp form or FMA use -- ARE these values."""
    with torch.no_grad():
        return torch.equal(columns(x, off, m, torch.float32, dg).double(), columns(x, off, m, torch.float64, dg))


def bf16_statistics(x, off, m, dg=1):
    """-> (share of the non-zero columns that are not bf16 values, share that lie exactly half-way between two bf16 values)."""
    with torch.no_grad():
        c = columns(x, off, m, torch.float64, dg)
        c = c[c != 0]
        bits = c.float().view(torch.int32) & 0xFFFF
        return (bits != 0).double().mean().item(), (bits == 0x8000).double().mean().item()


def tiled_forward_exact_samples(off, B, Co, H, W, layer_known_near=False, rescue_taps=5):
    """bool B x 9 x H x W: the samples whose forward products the tiled kernel route computes in exact fp32, unrounded
    (`fwd_exact` of dcn_reference).  Restates the kernel's own tests (dcn_fwd_tile_bf16x3, dcn_v2_bf16x3.inc; host side
    dcd_dcn_v2_forward, dcn_v2.hip):

      * per lane (:195-213, :271-304): a sample whose 2 x 2 footprint leaves the window staged for its TR x 32 tile -- rows
        r0 - 4 .. r0 + TR + 3, columns c0 - 4 .. c0 + 35.  TR is 8 once the launch has 512 tiles, else 4 (`rows8`);
      * per tile (:221-233): a tile in which some row of 32 pixels has far samples in `rescue_taps` (5) or more of its nine taps is
        left to the rescue pass `dcn_fwd9_f32<., true>` as a whole;
      * per call (:140-143): more than 1 in 32 offset coordinates displaced by 3 px or more -> every tile goes to the rescue pass.

    layer_known_near: the layer's last backward reported few far coordinates (`forward_keeps_far_samples`): the kernel then runs
    without the far count and hands no tile over -- only the per-lane rule is left."""
    tiles_x, nz = (W + 31) // 32, (Co + 63) // 64
    TR = 8 if tiles_x * ((H + 7) // 8) * B * nz >= 512 else 4
    ys = torch.arange(H).view(1, H, 1)
    xs = torch.arange(W).view(1, 1, W)
    far = torch.zeros(B, 9, H, W, dtype=torch.bool)
    o = off.float()                                           # the kernel's own arithmetic: (float)(ho - 1 + i) + offset
    for k in range(9):
        i, j = divmod(k, 3)
        h = (ys - 1 + i).float() + o[:, 2 * k]
        w = (xs - 1 + j).float() + o[:, 2 * k + 1]
        valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        ly = torch.floor(h) - ((ys // TR) * TR - 4)
        lx = torch.floor(w) - ((xs // 32) * 32 - 4)
        inside = (ly >= 0) & (lx >= 0) & (ly <= TR + 6) & (lx <= 38)
        far[:, k] = valid & ~inside
    if layer_known_near:
        return far
    if (~(o.abs() < 3.0)).sum().item() > off.numel() // 32:
        return torch.ones_like(far)
    exact = far.clone()
    for y0 in range(0, H, TR):
        for x0 in range(0, W, 32):
            taps_with_far = far[:, :, y0:y0 + TR, x0:x0 + 32].any(dim=3).sum(dim=1)          # B x rows
            handed = taps_with_far.max(dim=1).values >= rescue_taps                          # B
            exact[handed, :, y0:y0 + TR, x0:x0 + 32] = True
    return exact
