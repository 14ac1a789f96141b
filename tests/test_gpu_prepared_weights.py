"""What a parameter update leaves for the next forward: the table of prepared 3x3 weights (`ops._PreparedWeights`) passes an entry for
current while `weight._version` is the one its last `refresh_conv_weights()` saw, so every writer of parameters either bumps that
counter or must be followed by `ops.invalidate_conv_weights()`.  `trainer.train_step` refreshes before every forward and hides a
writer that does neither; a custom loop, a gradient probe or a twin model stepped by hand does not.  Two writers did neither when
this test was written: `ClipAdamW.clip_and_step` on csrc/optim.hip (raw pointers), and the library's FUSED AdamW `step()`, whose
kernel leaves the version counters alone -- the forward after such a step ran on the weights of before it, off by 0.2 to 0.7 of the
output's scale here.  The first now ends with the invalidation, the second is caught by the table's optimizer-step hook.

The model is the smallest that takes every consumer of the table: two `layers.conv.Conv2d(64, 64, 3, padding=1, bias=False)` in
sequence (`_Conv3x3`, and `_Conv3x3Skip` through `forward_with_skip`), then `DCN(64, 64)`, whose offset convolution reads the table
inside `_DCNWithOffsets`; input (1, 64, 12, 40), the smallest map `conv3x3_supported` accepts; in the three weight layouts.

Per case: two steps by hand (refresh, forward, backward, writer) at a learning rate of 1e-2 -- one update moves a weight by far
more than any kernel bound -- then, WITHOUT a refresh, a forward and backward on fixed inputs; `invalidate_conv_weights()`; the same
again.  The two runs must be bit-equal wherever the kernels are (tests/test_gpu_conv.py::
test_conv3x3_prepared_weights_equal_per_call_transform holds the table's transform to the per-call transform bit for bit): the three
outputs, and the gradients of the second convolution's output with respect to the input and both weights.  The gradients THROUGH the
DCN node are compared at 1e-5 of each tensor's largest value instead: dcd_dcn_v2_backward sums grad_input and grad_weight with
fp32 atomics in no fixed order (include/dcd_hip.h), i.e. sums of 64 x 9 terms reordered, sqrt(576) x 2^-24 = 1.4e-6 of their
scale, where weights stale by one update of 1e-2 against weights of ~4e-2 change them by tens of per cent.  Independently of the
second run, the plain convolutions' outputs of the first run are held to conv2d in float64 on the CURRENT weights at the bounds of
tests/test_gpu_conv.py.
"""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu

LR = 1e-2
LAYOUTS = ["f32", "bf16x3", "bf16"]
WRITERS = ["own_kernels", "class_library_path", "library_adamw", "load_state_dict", "data_add_then_invalidate"]


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from dcd_amd.model.backbone.DCNv2.dcn_v2 import DCN
        from dcd_amd.model.layers.conv import Conv2d
        self.c1 = Conv2d(64, 64, 3, padding=1, bias=False)
        self.c2 = Conv2d(64, 64, 3, padding=1, bias=False)
        self.dcn = DCN(64, 64, kernel_size=(3, 3), stride=1, padding=1, dilation=1, deformable_groups=1)

    def forward(self, x):
        y1 = self.c1(x)
        y2, skip = self.c2.forward_with_skip(y1)
        return y1, y2, self.dcn(y2 + skip)


def _probe(model, x0, gy2, gout):
    """Grad-enabled forward and backward on fixed inputs.  Returns (exact, loose): what must repeat bit for bit, and the gradients
    through the DCN node (atomically summed)."""
    x = x0.clone().requires_grad_(True)
    y1, y2, out = model(x)
    assert type(y1.grad_fn).__name__ == "_Conv3x3Backward" and type(y2.grad_fn).__name__ == "_Conv3x3SkipBackward"
    assert type(out.grad_fn).__name__ == "_DCNWithOffsetsBackward"
    gx2, gw1, gw2 = torch.autograd.grad(y2, [x, model.c1.weight, model.c2.weight], gy2, retain_graph=True)
    names = [n for n, _ in model.named_parameters()]
    full = torch.autograd.grad(out, [x] + [p for _, p in model.named_parameters()], gout)
    exact = {"y1": y1.detach(), "y2": y2.detach(), "out": out.detach(), "d y2 / d x": gx2, "d y2 / d w1": gw1, "d y2 / d w2": gw2}
    loose = {"d out / d " + n: g for n, g in zip(["x"] + names, full)}
    return exact, loose


def _optimizer(cls, model, cuda):
    weights = [p for n, p in model.named_parameters() if "bias" not in n]
    biases = [p for n, p in model.named_parameters() if "bias" in n]
    groups = [{"params": weights, "lr": torch.tensor(LR, device=cuda)}, {"params": biases, "lr": torch.tensor(LR, device=cuda)}]
    return cls(groups, lr=LR, weight_decay=1e-5, betas=(0.9, 0.99), fused=True, capturable=True)


@pytest.mark.parametrize("writer", WRITERS)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_no_writer_leaves_stale_prepared_weights(cuda, monkeypatch, layout, writer):
    from dcd_amd import _ext, ops
    from dcd_amd.engine import trainer
    gen = torch.Generator().manual_seed(LAYOUTS.index(layout) * 10 + WRITERS.index(writer))
    torch.manual_seed(3)
    model = _Tiny().to(cuda)
    x0 = torch.randn(1, 64, 12, 40, generator=gen).to(cuda)
    assert ops.conv3x3_supported(x0, model.c1.weight) and not ops.conv3x3_supported(x0[:, :, :10], model.c1.weight)
    gy2, gout = torch.randn(1, 64, 12, 40, generator=gen).to(cuda), torch.randn(1, 64, 12, 40, generator=gen).to(cuda)
    if layout == "bf16x3":
        monkeypatch.setattr(ops, "_CONV_SPLIT_MIN_MAP", 0)
    if writer == "class_library_path":
        monkeypatch.setattr(trainer, "_OWN_ADAMW", False)
    opt = None
    if writer in ("own_kernels", "class_library_path"):
        opt = _optimizer(trainer.ClipAdamW, model, cuda)
        assert opt.own_kernels_ok() == (writer == "own_kernels")
    elif writer == "library_adamw":
        opt = _optimizer(torch.optim.AdamW, model, cuda)

    def write():
        if writer in ("own_kernels", "class_library_path"):
            trainer.clip_and_step(model, opt, 15.0)
        elif writer == "library_adamw":
            opt.step()
        elif writer == "load_state_dict":
            model.load_state_dict({k: v + LR * torch.randn(v.shape, generator=gen).to(cuda) for k, v in model.state_dict().items()})
        else:
            for p in model.parameters():
                p.data.add_(LR * torch.randn(p.shape, generator=gen).to(cuda))
            ops.invalidate_conv_weights()                        # the documented contract of a write that bypasses the counters

    before = _ext.get_precision()
    _ext.set_precision(layout)
    try:
        assert ops._layout(ops._conv_prec(x0)) == {"f32": "f32", "bf16x3": "split", "bf16": "bf16" if ops._BF16_DIRECT else "split"}[layout]
        key = (x0.device.index, {"f32": False, "split": True, "bf16": "bf16"}[ops._layout(ops._conv_prec(x0))])
        for it in range(2):                                      # trainer.train_step by hand
            model.zero_grad(set_to_none=True)
            ops.refresh_conv_weights()
            xs = torch.randn(1, 64, 12, 40, generator=gen).to(cuda).requires_grad_(True)
            out = model(xs)[2]
            out.backward(torch.randn(out.shape, generator=gen).to(cuda))
            if it == 1:                                          # the second step ran on the table: the three layers are in it, current
                table = ops._PREPARED[key]
                assert all(table.lookup(w) is not None for w in (model.c1.weight, model.c2.weight, model.dcn.conv_offset_mask.weight))
            w_before = model.c1.weight.detach().clone()
            write()
            moved = (model.c1.weight.detach() - w_before).abs().max().item()
            assert moved > 0.2 * LR, "the writer must move the weights by about one update (%.3e)" % moved
        # no refresh
        first = _probe(model, x0, gy2, gout)
        ops.invalidate_conv_weights()
        second = _probe(model, x0, gy2, gout)
        current = {n: p.detach().clone() for n, p in model.named_parameters()}
    finally:
        _ext.set_precision(before)
    for name in first[0]:
        a, b = first[0][name], second[0][name]
        d = (a - b).abs().max().item()
        print("prepared-weights %s %s %-12s run 1 vs run 2: %.3e of %.3e" % (layout, writer, name, d, b.abs().max().item()))
    for name in first[1]:
        a, b = first[1][name], second[1][name]
        print("prepared-weights %s %s %-40s run 1 vs run 2: %.3e of %.3e" % (layout, writer, name, (a - b).abs().max().item(),
                                                                              b.abs().max().item()))
    for name in first[0]:
        assert torch.equal(first[0][name], second[0][name]), "%s differs between the run after the writer and the run after invalidate_conv_weights()" % name
    for name in first[1]:
        a, b = first[1][name], second[1][name]
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item(), name
    # the first run against float64 on the CURRENT weights
    r = (lambda t: t.bfloat16().double()) if layout == "bf16" and ops._BF16_DIRECT else (lambda t: t.double())
    # f32: test_conv3x3_forward_and_input_grad (2e-5); bf16x3: test_conv3x3_split_bf16_form (1e-4); bf16 on the direct kernel, against
    # the bf16-rounded operands: test_conv3x3_direct_bf16_is_the_exact_product_of_rounded_operands (2e-5); bf16 on the Winograd form:
    # test_conv3x3_mixed_bf16_form (1.5e-2)
    tol = {"f32": 2e-5, "bf16x3": 1e-4, "bf16": 2e-5 if ops._BF16_DIRECT else 1.5e-2}[layout]
    for name, inp, w in (("y1", x0, current["c1.weight"]), ("y2", first[0]["y1"], current["c2.weight"])):
        ref = F.conv2d(r(inp.cpu()), r(w.cpu()), padding=1)
        err = (first[0][name].cpu().double() - ref).abs().max().item()
        print("prepared-weights %s %s %s against float64 on the current weights: %.3e of %.3e" % (layout, writer, name, err, ref.abs().max().item()))
        assert err <= tol * ref.abs().max().item(), "%s: %.3e vs scale %.3e" % (name, err, ref.abs().max().item())
