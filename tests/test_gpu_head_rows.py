"""ops.head_rows (csrc/heads.hip, dcd_head_rows_*): the regression heads' 1x1 output layers at listed rows in one launch against
one F.linear per head, values and every gradient; and the predictor through it against the predictor through F.linear."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.nn import functional as F

sys.path.insert(0, os.path.dirname(__file__))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,K", [(50, 256), (320, 256), (7, 64)])
def test_head_rows_equal_one_linear_per_head(cuda, R, K):
    from dcd_amd import ops
    g = torch.Generator().manual_seed(4)
    trunk_of, outs = [0, 0, 1, 2, 2, 2], [4, 2, 20, 3, 1, 219]
    T = 3
    feat = torch.randn(T, R, K, generator=g).to(cuda).requires_grad_()
    ws = [(torch.randn(o, K, 1, 1, generator=g) * 0.1).to(cuda).requires_grad_() for o in outs]
    bs = [torch.randn(o, generator=g).to(cuda).requires_grad_() for o in outs]
    y = ops.head_rows(feat, trunk_of, ws, bs)
    ref = torch.cat([F.linear(feat[t], w.view(w.shape[0], K), b) for t, w, b in zip(trunk_of, ws, bs)], dim=1)
    assert y.shape == ref.shape == (R, sum(outs))
    scale = ref.abs().max().item()
    assert (y - ref).abs().max().item() <= 2e-6 * scale
    gy = torch.randn(R, sum(outs), generator=g).to(cuda)
    got = torch.autograd.grad(y, [feat] + ws + bs, gy)
    want = torch.autograd.grad(ref, [feat] + ws + bs, gy)
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() <= 5e-6 * max(b.abs().max().item(), 1e-3)
    # the feature gradient trunk by trunk: trunk 2 feeds 223 outputs, trunk 0 feeds 6 -- one scale over all three judges trunk 2
    for t in range(T):
        a, b = got[0][t], want[0][t]
        ratio = (a - b).abs().max().item() / b.abs().max().item()
        print("head rows R=%d K=%d: feature gradient of trunk %d, error / maximum %.2e" % (R, K, t, ratio))
        assert ratio <= 5e-6, (t, ratio)
    # reproducible: fixed summation order in all three kernels
    again = torch.autograd.grad(ops.head_rows(feat, trunk_of, ws, bs), [feat] + ws + bs, gy)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_head_rows_reject_heads_out_of_trunk_order(cuda):
    from dcd_amd import ops
    from dcd_amd._lib import DcdHipError
    feat = torch.zeros(2, 4, 64, device=cuda)
    ws = [torch.zeros(3, 64, device=cuda), torch.zeros(2, 64, device=cuda)]
    with pytest.raises(DcdHipError):
        ops.head_rows(feat, [1, 0], ws, [None, None])


def test_predictor_through_head_rows_equals_predictor_through_linears(cuda, monkeypatch):
    import golden_inputs as gi
    from test_host_golden import small_cfg
    from dcd_amd.model.head import detector_predictor as dp
    torch.manual_seed(0)
    cfg = small_cfg(str(cuda))
    pred = dp.make_predictor(cfg, 64).to(cuda).train()
    gi.name_hashed_init(pred)
    _, targets = gi.model_inputs()
    targets = [t.to(cuda) for t in targets]
    feats = torch.randn(2, 64, 24, 80, generator=torch.Generator().manual_seed(1)).to(cuda)
    res = {}
    for mode in (True, False):
        monkeypatch.setattr(dp, "_HEAD_ROWS", mode)
        gi.name_hashed_init(pred)                       # also resets the BatchNorm running estimates
        pred.zero_grad()
        x = feats.clone().requires_grad_()
        out = pred(x, targets)
        w = torch.randn(out['reg_pois'].shape, generator=torch.Generator().manual_seed(2)).to(cuda)
        ((out['reg_pois'] * w).sum() + out['cls'].sum()).backward()
        res[mode] = (out['reg_pois'].detach(), out['cls'].detach(), x.grad, {n: p.grad.clone() for n, p in pred.named_parameters()
                                                                            if p.grad is not None})
    a, b = res[True], res[False]
    assert (a[0] - b[0]).abs().max().item() <= 2e-6 * b[0].abs().max().item()
    assert (a[1] - b[1]).abs().max().item() <= 1e-6          # same kernels on both sides; the border scatter adds with atomics
    assert (a[2] - b[2]).abs().max().item() <= 1e-5 * b[2].abs().max().item()
    assert a[3].keys() == b[3].keys()
    top = max(v.abs().max().item() for v in b[3].values())
    for n in a[3]:                  # biases in front of a BatchNorm have a zero gradient: rounding noise on both sides
        assert (a[3][n] - b[3][n]).abs().max().item() <= 1e-5 * max(b[3][n].abs().max().item(), 1e-3 * top), n


# ---- every sparse route of the predictor against the dense map ----------------------------------------------------------------
# route -> (configuration, detector_predictor._HEAD_ROWS, trunk_moments.ENABLED, frozen)
ROUTES = {
    "default": ((), True, True, False),
    "head_rows_off": ((), False, True, False),
    "moments_off": ((), True, False, False),             # fan_out, batch_norm_act_at and one linear per head
    "leaky_relu": (("MODEL.HEAD.ACTIVE_FUNC", "leaky_relu"), True, True, False),      # dense trunks and the POI gather
    "no_edge_fusion": (("MODEL.HEAD.ENABLE_EDGE_FUSION", False), True, True, False),
    "frozen": ((), True, True, True),                    # BatchNorm layers in eval mode under no_grad: outputs only
}
ROUTE_FEATURE_GRAD_BOUND = 3e-6
ROUTE_PARAM_GRAD_BOUND = 3e-5
_DENSE = {}


def predictor_run(cuda, opts, frozen, sparse, seed=0):
    """One forward (and, unless frozen, backward under seeded output weights) of the predictor alone: 2 images, map 24x80."""
    import golden_inputs as gi
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head import detector_predictor as dp
    from dcd_amd.structures.params_3d import stack_field
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", str(cuda), "MODEL.USE_SYNC_BN", False, "INPUT.WIDTH_TRAIN", 320,
                        "INPUT.HEIGHT_TRAIN", 96] + list(opts))
    torch.manual_seed(0)
    pred = dp.make_predictor(cfg, 64).to(cuda).train()
    gi.name_hashed_init(pred)
    pred.sparse_training_heads = sparse
    if frozen:
        for m in pred.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    _, targets = gi.model_inputs()
    targets = [t.to(cuda) for t in targets]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 64, 24, 80, generator=g).to(cuda).requires_grad_(not frozen)
    with torch.set_grad_enabled(not frozen):
        out = pred(x, targets)
        if sparse:
            assert out["reg"] is None
            reg_pois = out["reg_pois"]
        else:
            c = stack_field(targets, "target_centers").long()
            lin = c[:, :, 1] * out["reg"].shape[3] + c[:, :, 0]
            reg_pois = out["reg"].flatten(2).gather(2, lin.unsqueeze(1).expand(-1, out["reg"].shape[1], -1)).transpose(1, 2)
        res = {"reg_pois": reg_pois.detach(), "cls": out["cls"].detach()}
        if not frozen:
            w_reg = torch.randn(reg_pois.shape, generator=g).to(cuda)
            w_cls = torch.randn(out["cls"].shape, generator=g).to(cuda)
            ((reg_pois * w_reg).sum() + (out["cls"] * w_cls).sum()).backward()
            res["x"] = x.grad
            res["params"] = {n: p.grad for n, p in pred.named_parameters() if p.grad is not None}
    return res


def route_deviations(a, b):
    """(reg_pois, cls, feature gradient, parameter gradients, its parameter): the gradients in the measure of the test above."""
    d_reg = (a["reg_pois"] - b["reg_pois"]).abs().max().item()
    d_cls = (a["cls"] - b["cls"]).abs().max().item()
    if "x" not in b:
        return d_reg, d_cls, None, None, None
    fx = (a["x"] - b["x"]).abs().max().item() / b["x"].abs().max().item()
    assert a["params"].keys() == b["params"].keys()
    top = max(v.abs().max().item() for v in b["params"].values())
    fp, worst = 0.0, None
    for n, ref in b["params"].items():
        d = (a["params"][n] - ref).abs().max().item() / max(ref.abs().max().item(), 1e-3 * top)
        if d > fp:
            fp, worst = d, n
    return d_reg, d_cls, fx, fp, worst


@pytest.mark.parametrize("trunk_form", ["shift", "bmm"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_predictor_sparse_route_equals_the_dense_map(cuda, monkeypatch, route, trunk_form):
    """Each sparse route of `_predictor._forward_sparse`, in both forms of the trunk statistics, against the dense map of the same
    weights gathered at the object centres: outputs at the project's bounds (tests/test_host_golden.py, check_model), gradients
    at 4x the worst deviation measured on an MI355X at commit e5d332c over seeds 0 to 2 (the border scatter adds with atomics, and
    the Winograd and patch products sum in other orders).  MODEL.HEAD.DEEPER_HEAD is not in this matrix (the host test runs it).
    Measured, feature gradient / parameter gradients (shift | bmm):
        default         5.1e-7 / 5.6e-6 | 5.1e-7 / 5.6e-6        head_rows_off   5.1e-7 / 5.6e-6 | 5.1e-7 / 5.6e-6
        moments_off     4.7e-7 / 5.6e-6 | 4.5e-7 / 6.4e-6        leaky_relu      4.5e-7 / 6.2e-6 | 5.1e-7 / 6.2e-6
        no_edge_fusion  5.7e-7 / 4.5e-6 | 4.8e-7 / 8.9e-7
    hence 4 x 5.7e-7 -> 3e-6 and 4 x 6.4e-6 -> 3e-5.  Outputs there: reg_pois <= 1.2e-6, cls <= 1.8e-7 (frozen: 5.4e-7, 1.2e-7)."""
    from dcd_amd.model.head import detector_predictor as dp, trunk_moments
    opts, head_rows, moments, frozen = ROUTES[route]
    monkeypatch.setenv("DCD_TRUNK_GRAM", trunk_form)
    monkeypatch.setattr(dp, "_HEAD_ROWS", head_rows)
    monkeypatch.setattr(trunk_moments, "ENABLED", moments)
    if (opts, frozen) not in _DENSE:                  # the dense route looks at none of the three switches
        _DENSE[(opts, frozen)] = predictor_run(cuda, opts, frozen, sparse=False)
    a, b = predictor_run(cuda, opts, frozen, sparse=True), _DENSE[(opts, frozen)]
    d_reg, d_cls, fx, fp, worst = route_deviations(a, b)
    print("%s/%s: reg_pois %.2e (largest %.2e), cls %.2e, gradients %s" % (
        route, trunk_form, d_reg, b["reg_pois"].abs().max().item(), d_cls,
        "not compared" if fx is None else "feature %.2e, parameters %.2e (%s)" % (fx, fp, worst)))
    assert d_reg <= 1e-4 * max(b["reg_pois"].abs().max().item(), 1.0)
    assert d_cls <= 1e-5
    if not frozen:
        assert fx <= ROUTE_FEATURE_GRAD_BOUND
        assert fp <= ROUTE_PARAM_GRAD_BOUND, worst
