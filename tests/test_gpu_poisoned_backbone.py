"""The backbone's kernels through the C ABI on poisoned, guarded buffers (tests/arena.py): the convolution family of csrc/conv.hip,
csrc/stem.hip, csrc/upsample.hip and csrc/norm.hip.

Each case places its inputs between guard words of NaN, poisons its outputs, poisons a workspace of exactly the advertised byte
count, calls, and lets `Arena.check` judge what the value tests cannot see: a write outside a buffer, a changed input, an output
element that was not written.  The result is then held to the SAME fp64 reference at the SAME bound as the kernel's value test
(cited at each `_close`); a read outside an input or a sum into stale scratch brings NaN in, which no bound survives.

Where include/dcd_hip.h promises reproducible bits (the Winograd forward / backward-data with their split contractions,
dcd_conv3x3_wrw, both 1x1 weight gradients, dcd_conv3x3_s2_f32_wrw: "partial sums in a fixed order") the call runs a second time
on zero-filled outputs and scratch and must give the same bits.  dcd_conv_stem_wrw ("partials are combined with float atomics:
order-dependent rounding") and the up-sampling weight gradient (atomicAdd, csrc/upsample.hip) are held to their bounds only.

Base pointers are 16-byte aligned and no better; dcd_channel_sums gets its arrival counters zeroed as its contract asks and the
rest of its workspace poisoned.  No kernel of csrc/ waits on a memory word, so poisoned scratch cannot hang one."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch
from torch.nn import functional as F

from arena import Arena
from transport_refs import same_bits

pytestmark = pytest.mark.gpu

PREC_F32, PREC_BF16X3, PREC_BF16 = 0, 1, 2


def _close(a, ref, what, tol=2e-5):
    """tests/test_gpu_conv.py `_close` (and tests/test_gpu_norm.py's): max error against the reference's scale."""
    err = (a.double().cpu() - ref).abs().max().item()
    scale = max(ref.abs().max().item(), 1e-6)
    assert err <= tol * scale, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


def _same(a, b, what):
    eq = same_bits(a.cpu().reshape(-1), b.cpu().reshape(-1))
    assert eq.all(), "%s: %d of %d elements depend on what the outputs / scratch held before the call, the first at %d" % (
        what, int((~eq).sum()), eq.numel(), int(torch.nonzero(~eq)[0]))


def _lib_and_stream(cuda):
    from dcd_amd import _lib
    return _lib.lib(), torch._C._cuda_getCurrentRawStream(cuda.index if cuda.index is not None else torch.cuda.current_device())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bf16(t):
    return t.bfloat16().double()


# ------------------------------------------------------------------------------------- the arena's controls on the device
def test_the_arena_sees_on_the_device_what_it_sees_on_the_host(cuda):
    """tests/test_arena.py's controls where the kernels run, without any overrun: the device hands a NaN's payload on like the host
    (the sum of two buffers' guard words differs from a third buffer's), and an entry point that is DOCUMENTED to add to its output
    (dcd_poi_scatter_add: "the call ADDS to grad_feat") reads as "not written" on a poisoned one -- what a kernel that forgot its
    zero-fill would do."""
    L, st = _lib_and_stream(cuda)
    ar = Arena(cuda)
    a, b = ar.place(torch.randn(100), "a"), ar.place(torch.randn(100), "b")
    out = ar.out((100,), "out")
    out.copy_(a + b)
    ar.check("honest")
    ga, gb, go = (ar.buffers[n].slab[-4:].view(torch.float32) for n in ("a", "b", "out"))
    summed = ga + gb
    assert torch.isnan(summed).all() and not same_bits(summed, go).any()
    go.copy_(summed)
    with pytest.raises(AssertionError, match="back guard of output 'out' overwritten: 4 words"):
        ar.check("a sum of guard words stored past the end")

    ar = Arena(cuda)
    go = ar.place(torch.randn(1, 3, 4), "grad_out")
    idx = ar.place(torch.tensor([[0, 5, 7]], dtype=torch.int64), "index")
    gf = ar.out((1, 4, 3, 4), "grad_feat")
    assert L.dcd_poi_scatter_add(st, go.data_ptr(), idx.data_ptr(), 1, 4, 3, 4, 3, gf.data_ptr()) == 0
    with pytest.raises(AssertionError, match="output 'grad_feat' not written: 48 words keep the poison"):
        ar.check("an accumulating call on a poisoned output")


# ----------------------------------------------------------------------------------------------------- 3x3 convolutions
@functools.lru_cache(maxsize=None)
def conv_problem(B, C, K, H, W):
    """One seeded problem per shape, shared by every test of that shape (do not modify): forward with bias and residual,
    backward-data accumulated onto a residual, weight gradient."""
    g = torch.Generator().manual_seed(C * 7 + K)
    p = SimpleNamespace(dims=(B, C, K, H, W))
    p.x = torch.randn(B, C, H, W, generator=g)
    p.w = torch.randn(K, C, 3, 3, generator=g) / (C * 9) ** 0.5
    p.bias = torch.randn(K, generator=g)
    p.res = torch.randn(B, K, H, W, generator=g)
    p.gy = torch.randn(B, K, H, W, generator=g)
    p.res_b = torch.randn(B, C, H, W, generator=g)
    return p


@functools.lru_cache(maxsize=None)
def conv_reference(B, C, K, H, W, rounded=False):
    """(forward, backward-data) of conv_problem in fp64; rounded: of the bf16-rounded operands (bias and residuals stay fp32)."""
    p = conv_problem(B, C, K, H, W)
    r = _bf16 if rounded else (lambda t: t.double())
    y = F.conv2d(r(p.x), r(p.w), p.bias.double(), padding=1) + p.res.double()
    gx = torch.nn.grad.conv2d_input(p.x.shape, r(p.w), r(p.gy), padding=1) + p.res_b.double()
    return y, gx


@functools.lru_cache(maxsize=None)
def wrw_reference(B, C, K, H, W, rounded):
    p = conv_problem(B, C, K, H, W)
    r = _bf16 if rounded else (lambda t: t.double())
    return torch.nn.grad.conv2d_weight(r(p.x), p.w.shape, r(p.gy), padding=1)


def _conv_run(cuda, entry, p, backward, weights, nbytes, poison, prec=None):
    """One call of a dcd_conv3x3* entry point: forward with bias and residual, or backward-data with residual == output."""
    L, st = _lib_and_stream(cuda)
    B, C, K, H, W = p.dims
    ar = Arena(cuda, poison)
    wt = ar.place(weights, "weights")
    ws = ar.scratch(nbytes, "workspace")
    if backward:
        inp = ar.place(p.gy, "grad_output")
        out = res = ar.place(p.res_b, "grad_input (residual == output)", inplace=True)
        bias = None
    else:
        inp, bias, res = ar.place(p.x, "input"), ar.place(p.bias, "bias"), ar.place(p.res, "residual")
        out = ar.out(p.res.shape, "output")
    extra = () if prec is None else (prec,)
    status = getattr(L, entry)(st, inp.data_ptr(), wt.data_ptr(), _ptr(bias), res.data_ptr(), out.data_ptr(), B, C, H, W, K,
                               int(backward), *extra, ar.ptr(ws), nbytes)
    what = "%s %s %s%s" % (entry, p.dims, "backward-data" if backward else "forward", "" if poison else " (zero-filled)")
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    return out.cpu()


def _transform(cuda, kind, w, table_of=None):
    """dcd_conv3x3[_split|_bf16]_transform_weights into buffers of exactly *_weights_bytes (both directions, guarded, poisoned);
    table_of: the same through the `_table` entry for a list of weights in ONE launch.  Returns [(forward, backward)] on the CPU."""
    L, st = _lib_and_stream(cuda)
    mid = {"f32": "", "split": "_split", "bf16": "_bf16"}[kind]
    nbytes = getattr(L, "dcd_conv3x3%s_weights_bytes" % mid)
    ws_list = [w] if table_of is None else table_of
    ar = Arena(cuda)
    rows, outs = [], []
    for i, wi in enumerate(ws_list):
        K, C = wi.shape[0], wi.shape[1]
        d = ar.place(wi, "weight %d" % i)
        tf = ar.out((nbytes(C, K, 0) // 4,), "forward_out %d (%d -> %d)" % (i, C, K), dtype=torch.int32)
        tb = ar.out((nbytes(C, K, 1) // 4,), "backward_out %d (%d -> %d)" % (i, C, K), dtype=torch.int32)
        assert nbytes(C, K, 0) % 4 == 0 and nbytes(C, K, 1) % 4 == 0
        rows.append([d.data_ptr(), tf.data_ptr(), tb.data_ptr(), C, K])
        outs.append((tf, tb))
    if table_of is None:
        (d_ptr, f_ptr, b_ptr, C, K), = rows
        status = getattr(L, "dcd_conv3x3%s_transform_weights" % mid)(st, d_ptr, C, K, f_ptr, b_ptr)
    else:
        table = ar.place(torch.tensor(rows, dtype=torch.int64), "table")
        status = getattr(L, "dcd_conv3x3%s_transform_weights_table" % mid)(st, table.data_ptr(), len(rows))
    what = "dcd_conv3x3%s_transform_weights%s %s" % (mid, "" if table_of is None else "_table", [tuple(wi.shape[:2]) for wi in ws_list])
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    return [(tf.cpu(), tb.cpu()) for tf, tb in outs]


CONV_SHAPES = [(2, 72, 80, 10, 36),       # ragged regions, partial channel chunk and output slice
               (1, 256, 64, 8, 32),       # split contraction
               (1, 512, 72, 12, 40),      # 8-way split
               (2, 64, 27, 24, 64)]       # one output block, bias
CONV_ROUTES = [s + (None,) for s in CONV_SHAPES] + [(1, 64, 64, 26, 36, "0"), (1, 64, 64, 26, 36, "1")]


@pytest.mark.parametrize("B,C,K,H,W,geom", CONV_ROUTES)
def test_conv3x3_and_prepared(cuda, monkeypatch, B, C, K, H, W, geom):
    """dcd_conv3x3 and dcd_conv3x3_prepared against conv2d in fp64 at 2e-5 (test_conv3x3_forward_and_input_grad,
    test_conv3x3_region_shapes), the same bits from poisoned and from zero-filled memory, and from both entry points
    (test_conv3x3_prepared_weights_equal_per_call_transform)."""
    L, _ = _lib_and_stream(cuda)
    if geom is not None:
        monkeypatch.setenv("DCD_CONV_GEOM", geom)
    p = conv_problem(B, C, K, H, W)
    n = L.dcd_conv3x3_workspace_bytes(B, C, H, W, K)
    (tf, tb), = _transform(cuda, "f32", p.w)
    for backward, ref, tw in zip((False, True), conv_reference(B, C, K, H, W), (tf, tb)):
        got = _conv_run(cuda, "dcd_conv3x3", p, backward, p.w, n, True)
        _close(got, ref, "dcd_conv3x3 %s" % ("grad_input" if backward else "forward"))
        _same(got, _conv_run(cuda, "dcd_conv3x3", p, backward, p.w, n, False), "dcd_conv3x3 backward=%d" % backward)
        prepared = _conv_run(cuda, "dcd_conv3x3_prepared", p, backward, tw, n, True)
        _same(prepared, got, "dcd_conv3x3_prepared against dcd_conv3x3, backward=%d" % backward)
        _same(prepared, _conv_run(cuda, "dcd_conv3x3_prepared", p, backward, tw, n, False), "dcd_conv3x3_prepared backward=%d" % backward)


@pytest.mark.parametrize("kind", ["f32", "split", "bf16"])
def test_conv3x3_weight_transforms_fill_exactly_their_buffers(cuda, kind):
    """The three weight layouts into buffers of exactly *_weights_bytes: every word written, none outside, per layer and for three
    layers in one `_table` launch, bitwise equal (test_prepared_weight_table_one_launch_for_all_layers)."""
    g = torch.Generator().manual_seed(3)
    ws = [torch.randn(k, c, 3, 3, generator=g) / (c * 9) ** 0.5 for c, k in ((72, 80), (256, 64), (64, 27))]
    single = [_transform(cuda, kind, w)[0] for w in ws]
    table = _transform(cuda, kind, None, table_of=ws)
    for i, ((sf, sb), (tf, tb)) in enumerate(zip(single, table)):
        assert torch.equal(sf, tf) and torch.equal(sb, tb), "layer %d: the table launch differs from the per-layer transform" % i


@pytest.mark.parametrize("prec", [PREC_BF16X3, PREC_BF16])
@pytest.mark.parametrize("B,C,K,H,W", CONV_SHAPES[:3])
def test_conv3x3_split_prepared(cuda, B, C, K, H, W, prec):
    """dcd_conv3x3_split_prepared against conv2d in fp64: 1e-4 in split-bf16 (test_conv3x3_split_bf16_form), 1.5e-2 in the
    one-product form (test_conv3x3_mixed_bf16_form); the same bits from poisoned and zero-filled memory."""
    L, _ = _lib_and_stream(cuda)
    p = conv_problem(B, C, K, H, W)
    n = L.dcd_conv3x3_split_workspace_bytes(B, C, H, W, K)
    (tf, tb), = _transform(cuda, "split", p.w)
    tol = 1e-4 if prec == PREC_BF16X3 else 1.5e-2
    for backward, ref, tw in zip((False, True), conv_reference(B, C, K, H, W), (tf, tb)):
        got = _conv_run(cuda, "dcd_conv3x3_split_prepared", p, backward, tw, n, True, prec)
        _close(got, ref, "split prec %d %s" % (prec, "grad_input" if backward else "forward"), tol)
        _same(got, _conv_run(cuda, "dcd_conv3x3_split_prepared", p, backward, tw, n, False, prec), "split backward=%d" % backward)


@pytest.mark.parametrize("B,C,K,H,W", [(2, 72, 80, 10, 36), (3, 27, 64, 14, 44), (1, 256, 64, 9, 32), (1, 512, 72, 12, 40)])
def test_conv3x3_bf16_prepared(cuda, B, C, K, H, W):
    """dcd_conv3x3_bf16_prepared against conv2d in fp64 of the bf16-rounded operands at 2e-5
    (test_conv3x3_direct_bf16_is_the_exact_product_of_rounded_operands): 27 and 72 contraction channels, whose last chunk reads
    past the tensor and must get zeros -- here the neighbour is NaN."""
    L, _ = _lib_and_stream(cuda)
    p = conv_problem(B, C, K, H, W)
    n = L.dcd_conv3x3_bf16_workspace_bytes(B, C, H, W, K)
    (tf, tb), = _transform(cuda, "bf16", p.w)
    r_y, r_gx = conv_reference(B, C, K, H, W, True)
    _close(_conv_run(cuda, "dcd_conv3x3_bf16_prepared", p, False, tf, n, True), r_y, "direct forward")
    _close(_conv_run(cuda, "dcd_conv3x3_bf16_prepared", p, True, tb, n, True), r_gx, "direct grad_input")


@pytest.mark.parametrize("prec", [PREC_F32, PREC_BF16])
@pytest.mark.parametrize("B,C,K,H,W", [(2, 72, 80, 10, 36), (1, 256, 64, 8, 32), (2, 64, 27, 24, 64), (2, 128, 256, 24, 80)])
def test_conv3x3_wrw(cuda, B, C, K, H, W, prec):
    """dcd_conv3x3_wrw: exact fp32 at 2e-5 (test_conv3x3_forward_and_input_grad); DCD_PREC_BF16 against the bf16-rounded operands at
    2e-5 on the direct kernel (Cout > 32) and 1.5e-2 on the Winograd-domain form
    (test_conv3x3_direct_bf16_is_the_exact_product_of_rounded_operands); the same bits from poisoned and zero-filled memory."""
    L, st = _lib_and_stream(cuda)
    p = conv_problem(B, C, K, H, W)
    n = L.dcd_conv3x3_wrw_workspace_bytes(B, C, H, W, K)
    got = []
    for poison in (True, False):
        ar = Arena(cuda, poison)
        x, gy = ar.place(p.x, "input"), ar.place(p.gy, "grad_output")
        gw = ar.out(p.w.shape, "grad_weight")
        ws = ar.scratch(n, "workspace")
        assert L.dcd_conv3x3_wrw(st, x.data_ptr(), gy.data_ptr(), gw.data_ptr(), B, C, H, W, K, prec, ar.ptr(ws), n) == 0
        ar.check("dcd_conv3x3_wrw %s prec %d poison %d" % (p.dims, prec, poison))
        got.append(gw.cpu())
    if prec == PREC_F32:
        _close(got[0], wrw_reference(B, C, K, H, W, False), "grad_weight")
    else:
        _close(got[0], wrw_reference(B, C, K, H, W, True), "bf16 grad_weight", 2e-5 if K > 32 else 1.5e-2)
    _same(got[0], got[1], "dcd_conv3x3_wrw prec %d" % prec)


# ------------------------------------------------------------------------------------------------------ 1x1 convolutions
@functools.lru_cache(maxsize=None)
def pointwise_problem(B, cs, O, H, W):
    g = torch.Generator().manual_seed(sum(cs) + O + 1)
    p = SimpleNamespace()
    p.xs = [torch.randn(B, c, H, W, generator=g) for c in cs]
    C = sum(cs)
    p.w = torch.randn(O, C, generator=g) / C ** 0.5
    p.gy = torch.randn(B, O, H, W, generator=g)
    xcat = torch.cat(p.xs, 1)
    p.ref, p.r_ref = {}, {}
    for r, d in ((lambda t: t.double(), p.ref), (_bf16, p.r_ref)):
        w4 = r(p.w).view(O, C, 1, 1)
        d["y"] = F.conv2d(r(xcat), w4)
        d["gx"] = torch.nn.grad.conv2d_input(xcat.shape, w4, r(p.gy))
        d["gw"] = torch.nn.grad.conv2d_weight(r(xcat), w4.shape, r(p.gy)).view(O, C)
    return p


@pytest.mark.parametrize("kind", ["f32", "bf16"])
@pytest.mark.parametrize("B,cs,O,H,W", [(2, (80, 16), 96, 10, 14), (3, (16, 32), 48, 6, 10), (1, (16,), 16, 2, 2),
                                        (1, (128, 128, 64, 128), 128, 12, 40)])
def test_conv1x1(cuda, kind, B, cs, O, H, W):
    """dcd_conv1x1_{f32,bf16} forward over all inputs and `transposed` on each column slice (weight + col0, ldw > M), and
    dcd_conv1x1_wrw_* into the O x C block of a wider poisoned matrix whose other columns must keep their bits.  fp32 against conv2d
    in fp64 at 2e-5 (test_conv1x1_of_cat_on_the_fp32_pointwise_kernels), bf16 against the rounded operands at 2e-5
    (test_conv1x1_of_cat_in_the_bf16_scope); the weight gradients bitwise the same from poisoned and zero-filled memory."""
    L, st = _lib_and_stream(cuda)
    p = pointwise_problem(B, cs, O, H, W)
    ref = p.ref if kind == "f32" else p.r_ref
    fwd, wrw, wrw_bytes = (getattr(L, n % kind) for n in ("dcd_conv1x1_%s", "dcd_conv1x1_wrw_%s", "dcd_conv1x1_wrw_%s_workspace_bytes"))
    Ct, HW, n_in = sum(cs), H * W, len(cs)

    ar = Arena(cuda)
    w = ar.place(p.w, "weight")
    xs = [ar.place(x, "input %d" % i) for i, x in enumerate(p.xs)]
    y = ar.out((B, O, H, W), "output")
    ptrs = (ctypes.c_void_p * n_in)(*[x.data_ptr() for x in xs])
    chs = (ctypes.c_int * n_in)(*cs)
    assert fwd(st, w.data_ptr(), Ct, 0, n_in, ptrs, chs, y.data_ptr(), B, O, HW) == 0
    ar.check("conv1x1 %s forward" % kind)
    _close(y, ref["y"], "1x1 %s forward" % kind)

    c0 = 0
    for i, Ci in enumerate(cs):
        ar = Arena(cuda)
        w, gy = ar.place(p.w, "weight"), ar.place(p.gy, "grad_output")
        gx = ar.out((B, Ci, H, W), "grad_input %d" % i)
        one_p, one_c = (ctypes.c_void_p * 1)(gy.data_ptr()), (ctypes.c_int * 1)(O)
        assert fwd(st, w.data_ptr() + 4 * c0, Ct, 1, 1, one_p, one_c, gx.data_ptr(), B, Ci, HW) == 0
        ar.check("conv1x1 %s transposed, columns %d..%d" % (kind, c0, c0 + Ci))
        _close(gx, ref["gx"][:, c0:c0 + Ci], "1x1 %s grad_input %d" % (kind, i))

        n = wrw_bytes(B, O, Ci, HW)
        block = torch.zeros(O, Ct, dtype=torch.bool)
        block[:, c0:c0 + Ci] = True
        got = []
        for poison in (True, False):
            ar = Arena(cuda, poison)
            gy, x = ar.place(p.gy, "grad_output"), ar.place(p.xs[i], "input %d" % i)
            gw = ar.out((O, Ct), "grad_weight", written=block)
            ws = ar.scratch(n, "workspace")
            assert wrw(st, gy.data_ptr(), x.data_ptr(), gw.data_ptr() + 4 * c0, Ct, B, O, Ci, HW, ar.ptr(ws), n) == 0
            ar.check("conv1x1_wrw %s, columns %d..%d, poison %d" % (kind, c0, c0 + Ci, poison))
            got.append(gw[:, c0:c0 + Ci].cpu())
        _close(got[0], ref["gw"][:, c0:c0 + Ci], "1x1 %s grad_weight %d" % (kind, i))
        _same(got[0], got[1], "dcd_conv1x1_wrw_%s slice %d" % (kind, i))
        c0 += Ci


# ------------------------------------------------------------------------------------------------- stride-2 convolutions
@pytest.mark.parametrize("B,C,K,H,W", [(3, 16, 48, 8, 16), (1, 32, 64, 24, 80), (1, 256, 512, 12, 40)])
def test_conv3x3_stride2(cuda, B, C, K, H, W):
    """dcd_conv3x3_s2_f32, _backward_data and _wrw against conv2d in fp64 at 2e-5 (test_stride2_conv_native_fp32_kernels); the
    weight gradient bitwise the same from poisoned and zero-filled memory."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(C * 3 + K)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(K, C, 3, 3, generator=g) / (C * 9) ** 0.5
    gy = torch.randn(B, K, H // 2, W // 2, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1)
    ref_gx = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), stride=2, padding=1)
    ref_gw = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), stride=2, padding=1)

    ar = Arena(cuda)
    dx, dw = ar.place(x, "input"), ar.place(w, "weight")
    y = ar.out(gy.shape, "output")
    assert L.dcd_conv3x3_s2_f32(st, dx.data_ptr(), dw.data_ptr(), y.data_ptr(), B, C, H, W, K) == 0
    ar.check("dcd_conv3x3_s2_f32")
    _close(y, ref, "native stride-2 forward")

    ar = Arena(cuda)
    dgy, dw = ar.place(gy, "grad_output"), ar.place(w, "weight")
    gx = ar.out(x.shape, "grad_input")
    assert L.dcd_conv3x3_s2_f32_backward_data(st, dgy.data_ptr(), dw.data_ptr(), gx.data_ptr(), B, C, H, W, K) == 0
    ar.check("dcd_conv3x3_s2_f32_backward_data")
    _close(gx, ref_gx, "native stride-2 grad_input")

    n = L.dcd_conv3x3_s2_f32_wrw_workspace_bytes(B, C, H, W, K)
    got = []
    for poison in (True, False):
        ar = Arena(cuda, poison)
        dx, dgy = ar.place(x, "input"), ar.place(gy, "grad_output")
        gw = ar.out(w.shape, "grad_weight")
        ws = ar.scratch(n, "workspace")
        assert L.dcd_conv3x3_s2_f32_wrw(st, dx.data_ptr(), dgy.data_ptr(), gw.data_ptr(), B, C, H, W, K, ar.ptr(ws), n) == 0
        ar.check("dcd_conv3x3_s2_f32_wrw poison %d" % poison)
        got.append(gw.cpu())
    _close(got[0], ref_gw, "native stride-2 grad_weight")
    _same(got[0], got[1], "dcd_conv3x3_s2_f32_wrw")


# ------------------------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("B,Ci,k,H,W", [(2, 16, 3, 19, 260), (1, 3, 7, 21, 196)])
def test_conv_stem(cuda, B, Ci, k, H, W):
    """dcd_conv_stem (forward; backward-data for the 16 -> 16 layer) and dcd_conv_stem_wrw against conv2d in fp64 at 1e-5 / 1e-5 /
    2e-5 (test_stem_convolutions)."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(Ci * 100 + k)
    x = torch.randn(B, Ci, H, W, generator=g)
    w = torch.randn(16, Ci, k, k, generator=g) / (Ci * k * k) ** 0.5
    gy = torch.randn(B, 16, H, W, generator=g)
    ref = F.conv2d(x.double(), w.double(), padding=k // 2)
    ref_gw = torch.nn.grad.conv2d_weight(x.double(), w.shape, gy.double(), padding=k // 2)
    n = L.dcd_conv_stem_workspace_bytes(Ci, 16, k)

    ar = Arena(cuda)
    dx, dw = ar.place(x, "input"), ar.place(w, "weight")
    y = ar.out(gy.shape, "output")
    ws = ar.scratch(n, "workspace")
    assert L.dcd_conv_stem(st, dx.data_ptr(), dw.data_ptr(), y.data_ptr(), B, Ci, H, W, 16, k, 0, ar.ptr(ws), n) == 0
    ar.check("dcd_conv_stem forward")
    _close(y, ref, "forward", 1e-5)

    if Ci == 16:
        ref_gx = torch.nn.grad.conv2d_input(x.shape, w.double(), gy.double(), padding=k // 2)
        ar = Arena(cuda)
        dgy, dw = ar.place(gy, "grad_output"), ar.place(w, "weight")
        gx = ar.out(x.shape, "grad_input")
        ws = ar.scratch(n, "workspace")
        assert L.dcd_conv_stem(st, dgy.data_ptr(), dw.data_ptr(), gx.data_ptr(), B, Ci, H, W, 16, k, 1, ar.ptr(ws), n) == 0
        ar.check("dcd_conv_stem backward-data")
        _close(gx, ref_gx, "grad_input", 1e-5)

    n = L.dcd_conv_stem_wrw_workspace_bytes(Ci, 16, k)
    ar = Arena(cuda)
    dx, dgy = ar.place(x, "input"), ar.place(gy, "grad_output")
    gw = ar.out(w.shape, "grad_weight")
    ws = ar.scratch(n, "workspace")
    assert L.dcd_conv_stem_wrw(st, dx.data_ptr(), dgy.data_ptr(), gw.data_ptr(), B, Ci, H, W, 16, k, ar.ptr(ws), n) == 0
    ar.check("dcd_conv_stem_wrw")
    _close(gw, ref_gw, "grad_weight", 2e-5)


# ------------------------------------------------------------------------------------------- up-sampling, pooling, sums
UP_SHAPES = [(2, 8, 5, 6, 2), (1, 64, 24, 80, 4),
             (1, 2, 7, 300, 2), (1, 2, 7, 300, 4),        # the backward's row chunks: 3, 3 and a ragged last one of 1 row
             (1, 3, 9, 40, 8)]                            # f = 8 on more than one workgroup, forward and backward


@pytest.mark.parametrize("B,C,H,W,f", UP_SHAPES)
def test_upsample_dw(cuda, B, C, H, W, f):
    """dcd_upsample_dw_forward, _forward_add and _backward against conv_transpose2d in fp64 at 1e-6 / 1e-5 / 2e-5
    (test_depthwise_upsample_matches_conv_transpose, test_depthwise_upsample_with_skip_sum).  grad_weight is accumulated with
    atomicAdd into what the callee zero-fills: it starts as NaN here."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(C + f)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, 1, 2 * f, 2 * f, generator=g)
    gy = torch.randn(B, C, H * f, W * f, generator=g)
    skip = torch.randn(B, C, H * f, W * f, generator=g)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    ref = F.conv_transpose2d(xd, wd, stride=f, padding=f // 2, groups=C)
    ref.backward(gy.double())
    ref = ref.detach()

    ar = Arena(cuda)
    dx, dw = ar.place(x, "x"), ar.place(w, "weight")
    y = ar.out(gy.shape, "y")
    assert L.dcd_upsample_dw_forward(st, dx.data_ptr(), dw.data_ptr(), y.data_ptr(), B, C, H, W, f) == 0
    ar.check("dcd_upsample_dw_forward")
    _close(y, ref, "forward", 1e-6)

    ar = Arena(cuda)
    dx, dw, ds = ar.place(x, "x"), ar.place(w, "weight"), ar.place(skip, "skip")
    y = ar.out(gy.shape, "y")
    assert L.dcd_upsample_dw_forward_add(st, dx.data_ptr(), dw.data_ptr(), ds.data_ptr(), y.data_ptr(), B, C, H, W, f) == 0
    ar.check("dcd_upsample_dw_forward_add")
    _close(y, ref + skip.double(), "forward_add", 1e-6)

    ar = Arena(cuda)
    dx, dw, dgy = ar.place(x, "x"), ar.place(w, "weight"), ar.place(gy, "grad_y")
    gx, gw = ar.out(x.shape, "grad_x"), ar.out(w.shape, "grad_weight")
    assert L.dcd_upsample_dw_backward(st, dx.data_ptr(), dw.data_ptr(), dgy.data_ptr(), gx.data_ptr(), gw.data_ptr(), B, C, H, W, f) == 0
    ar.check("dcd_upsample_dw_backward")
    _close(gx, xd.grad, "grad_input", 1e-5)
    _close(gw, wd.grad, "grad_weight", 2e-5)


def test_maxpool2x2(cuda):
    """dcd_maxpool2x2_forward / _backward on (2, 5, 6, 12) as 10 planes: values and gradient exact, a four-way tie and a NaN
    included (test_maxpool2x2_matches_stock)."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 5, 6, 12, generator=g)
    x[0, 0, 0:2, 0:2] = 1.5
    x[-1, -1, 2:4, 4:6] = torch.tensor([[0.1, float("nan")], [0.3, 0.2]])
    gy = torch.randn(2, 5, 3, 6, generator=g)
    xr = x.clone().requires_grad_()
    ref = F.max_pool2d(xr, 2, 2)
    ref.backward(gy)

    ar = Arena(cuda)
    dx = ar.place(x, "x")
    y = ar.out(gy.shape, "y")
    assert L.dcd_maxpool2x2_forward(st, dx.data_ptr(), y.data_ptr(), 10, 6, 12) == 0
    ar.check("dcd_maxpool2x2_forward")
    assert torch.equal(torch.nan_to_num(y.cpu(), nan=7.0), torch.nan_to_num(ref.detach(), nan=7.0))

    ar = Arena(cuda)
    dx, dgy = ar.place(x, "x"), ar.place(gy, "grad_y")
    gx = ar.out(x.shape, "grad_x")
    assert L.dcd_maxpool2x2_backward(st, dx.data_ptr(), dgy.data_ptr(), gx.data_ptr(), 10, 6, 12) == 0
    ar.check("dcd_maxpool2x2_backward")
    assert torch.equal(gx.cpu(), xr.grad)


@pytest.mark.parametrize("numel", [1000, 630])
def test_sum_tensors(cuda, numel):
    """dcd_sum_tensors of three sources (test_fan_out_sums_gradients_in_one_pass: 1e-6 absolute); 630 elements end in a tail of two,
    and the words past `numel` are guard words."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(numel)
    srcs = [torch.randn(numel, generator=g) for _ in range(3)]
    ar = Arena(cuda)
    dev = [ar.place(s, "source %d" % i) for i, s in enumerate(srcs)]
    out = ar.out((numel,), "out")
    arr = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in dev])
    assert L.dcd_sum_tensors(st, arr, 3, out.data_ptr(), numel) == 0
    ar.check("dcd_sum_tensors %d" % numel)
    assert torch.allclose(out.cpu(), srcs[0] + srcs[1] + srcs[2], atol=1e-6)


# ------------------------------------------------------------------------------------------------------------ batch norm
@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (1, 300, 4, 4), (2, 27, 12, 40)])
def test_channel_sums(cuda, shape):
    """dcd_channel_sums against the fp64 sum at 1e-6 (test_channel_sums_one_launch_equals_fp64_sum_and_repeats).  The C arrival
    counters at the start of the workspace's second half enter zeroed, as the contract asks, everything else of it as NaN; the
    call must leave the counters at zero."""
    L, st = _lib_and_stream(cuda)
    B, C = shape[0], shape[1]
    HW = shape[2] * shape[3]
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(3))
    ref = x.double().sum(dim=(0, 2, 3))
    n = L.dcd_bn_workspace_bytes(C)
    ar = Arena(cuda)
    dx = ar.place(x, "x")
    sums = ar.out((C,), "sums")
    ws = ar.scratch(n, "workspace")
    counters = ws[n // 2:n // 2 + 4 * C]
    counters.zero_()
    assert L.dcd_channel_sums(st, dx.data_ptr(), B, C, HW, sums.data_ptr(), ar.ptr(ws), n) == 0
    ar.check("dcd_channel_sums %s" % (shape,))
    assert (sums.cpu().double() - ref).abs().max().item() <= 1e-6 * max(ref.abs().max().item(), 1.0)
    assert not counters.any(), "the arrival counters must be zero again after the call"


@functools.lru_cache(maxsize=None)
def bn_problem(B, C, H, W, use_res, relu):
    """tests/test_gpu_norm.py's inputs and `_reference` for one case (do not modify)."""
    g = torch.Generator().manual_seed(B * 1000 + C)
    p = SimpleNamespace()
    p.x = torch.randn(B, C, H, W, generator=g) * 1.7 + 0.8
    p.res = torch.randn(B, C, H, W, generator=g) if use_res else None
    p.gy = torch.randn(B, C, H, W, generator=g)
    p.w = torch.rand(C, generator=g) + 0.5
    p.b = torch.randn(C, generator=g) * 0.3
    xd = p.x.double().requires_grad_()
    rd = None if p.res is None else p.res.double().requires_grad_()
    wd, bd = p.w.double().requires_grad_(), p.b.double().requires_grad_()
    p.rm, p.rv = torch.zeros_like(wd), torch.ones_like(wd)
    y = F.batch_norm(xd, p.rm, p.rv, wd, bd, True, 0.1, 1e-5)
    if rd is not None:
        y = y + rd
    if relu:
        y = F.relu(y)
    y.backward(p.gy.double())
    p.y, p.gx, p.gr, p.gw, p.gb = y.detach(), xd.grad, None if rd is None else rd.grad, wd.grad, bd.grad
    return p


@pytest.mark.parametrize("B,C,H,W,use_res,relu", [(2, 5, 7, 9, True, True),            # HW % 4 != 0: scalar path
                                                  (3, 33, 12, 40, True, False),
                                                  (2, 512, 12, 40, False, True),       # one launch per direction
                                                  (1, 64, 128, 132, True, True)])      # just above that route's limit: two launches
def test_batch_norm(cuda, B, C, H, W, use_res, relu):
    """dcd_bn_train_forward, dcd_bn_backward and (ReLU, no residual) dcd_bn_backward_relu_from_x against batch_norm + add + relu in
    fp64 at 2e-5, the residual's gradient at 1e-7 (test_bn_act_train_matches_stock_ops); the running buffers and
    num_batches_tracked are guarded buffers updated in place."""
    L, st = _lib_and_stream(cuda)
    p = bn_problem(B, C, H, W, use_res, relu)
    HW = H * W
    n = L.dcd_bn_workspace_bytes(C)

    ar = Arena(cuda)
    x, w, b = ar.place(p.x, "x"), ar.place(p.w, "weight"), ar.place(p.b, "bias")
    res = ar.place(p.res, "residual") if use_res else None
    rm = ar.place(torch.zeros(C), "running_mean", inplace=True)
    rv = ar.place(torch.ones(C), "running_var", inplace=True)
    nbt = ar.place(torch.zeros(1, dtype=torch.int64), "num_batches_tracked", inplace=True)
    y, mean, invstd = ar.out(p.x.shape, "y"), ar.out((C,), "save_mean"), ar.out((C,), "save_invstd")
    ws = ar.scratch(n, "workspace")
    assert L.dcd_bn_train_forward(st, x.data_ptr(), _ptr(res), w.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr(),
                                  0.1, 1e-5, int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), B, C, HW, ar.ptr(ws), n) == 0
    ar.check("dcd_bn_train_forward")
    _close(y, p.y, "y")
    _close(rm, p.rm, "running_mean")
    _close(rv, p.rv, "running_var")
    assert int(nbt.cpu()) == 1
    y_cpu, mean_cpu, invstd_cpu = y.cpu(), mean.cpu(), invstd.cpu()

    def backward(entry):
        ar = Arena(cuda)
        gy, x, w = ar.place(p.gy, "grad_y"), ar.place(p.x, "x"), ar.place(p.w, "weight")
        mean, invstd = ar.place(mean_cpu, "save_mean"), ar.place(invstd_cpu, "save_invstd")
        gx, gw, gb = ar.out(p.x.shape, "grad_x"), ar.out((C,), "grad_weight"), ar.out((C,), "grad_bias")
        ws = ar.scratch(n, "workspace")
        gres = None
        if entry == "dcd_bn_backward":
            y = ar.place(y_cpu, "y") if relu else None
            gres = ar.out(p.x.shape, "grad_residual") if use_res else None
            status = L.dcd_bn_backward(st, gy.data_ptr(), _ptr(y), x.data_ptr(), w.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                       gx.data_ptr(), _ptr(gres), gw.data_ptr(), gb.data_ptr(), B, C, HW, ar.ptr(ws), n)
        else:
            b = ar.place(p.b, "bias")
            status = L.dcd_bn_backward_relu_from_x(st, gy.data_ptr(), x.data_ptr(), w.data_ptr(), b.data_ptr(), mean.data_ptr(),
                                                   invstd.data_ptr(), gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), B, C, HW, ar.ptr(ws), n)
        assert status == 0, "%s: status %d" % (entry, status)
        ar.check(entry)
        _close(gx, p.gx, entry + " grad_x")
        if gres is not None:
            _close(gres, p.gr, entry + " grad_residual", 1e-7)
        _close(gw, p.gw, entry + " grad_weight")
        _close(gb, p.gb, entry + " grad_bias")

    backward("dcd_bn_backward")
    if relu and not use_res:
        backward("dcd_bn_backward_relu_from_x")
