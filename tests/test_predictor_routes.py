"""The sparse training routes of the prediction head (dcd_amd/model/head/detector_predictor.py) against the dense map of the same
weights, on the host: the predictor alone in train mode, features (2, 64, 24, 80), the golden targets.  Every configuration the
sparse forward branches on is one case -- the trunks from the patch moments and trunk by trunk, edge fusion on and off, leaky
ReLU, GroupNorm, the deeper head -- and each is held to the dense route (`sparse_training_heads = False`, gathered at
`target_centers`) in `reg_pois`, `cls`, the gradient of the features and of every parameter under seeded output weights, and the
BatchNorm buffers.

Bounds.  Outputs: the project's own (tests/test_host_golden.py, check_model).  The two sparse routes of one configuration
(moments on / off) against each other in float64: 1e-9 of each tensor's largest value, the bound tests/test_trunk_moments.py
holds the same algebra to.  Gradients against the dense route cannot be that tight: the dense route hands its map out in float32
and sums the gradients of duplicate centre cells there.  Measured at commit e5d332c over seeds 0 to 2, worst |a - b|max / |b|max:
    feature gradient       default, moments off and both cases without edge fusion 1.2e-7, leaky ReLU 1.2e-7, GN 1.1e-7,
                           deeper head (float32) 5.9e-7
    parameter gradients    8.5e-7 in every float64 case (reg_heads.6.0.bias)
    deeper-head parameters 3.9e-3 floored (reg_head_pre.3.bias; 3.7e-1 unfloored)
The committed bounds are 10x the worst value of each kind (another seed puts other cells on top of each other).  In the deeper
head the per-parameter deviation is floored like check_model floors its norms, at 1e-4 of the largest gradient over all
parameters: the biases in front of a BatchNorm have an exactly zero gradient, and what float32 leaves there is noise on both
sides."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))

FEATURE_GRAD_BOUND = 6e-6
PARAM_GRAD_BOUND = 9e-6
DEEPER_PARAM_GRAD_BOUND = 4e-2         # of max(|ref|max, 1e-4 of the largest gradient)
SEED = 0

# name -> (configuration, trunk_moments.ENABLED, dtype)
CASES = {
    "default": ((), True, torch.float64),
    "moments_off": ((), False, torch.float64),
    "no_edge_fusion": (("MODEL.HEAD.ENABLE_EDGE_FUSION", False), True, torch.float64),
    "no_edge_fusion_moments_off": (("MODEL.HEAD.ENABLE_EDGE_FUSION", False), False, torch.float64),
    "leaky_relu": (("MODEL.HEAD.ACTIVE_FUNC", "leaky_relu"), True, torch.float64),
    "group_norm": (("MODEL.HEAD.USE_NORMALIZATION", "GN"), True, torch.float64),
    "deeper_head": (("MODEL.HEAD.DEEPER_HEAD", True), True, torch.float32),      # the oracle DCN is float32
}
_RESULTS = {}          # (configuration, route) -> result: every route is run once, whichever test asks first


def run_route(opts, dtype, sparse, moments, seed=SEED):
    """One forward and backward of the predictor alone -> outputs at the object centres, gradients, buffers."""
    import golden_inputs as gi
    from dcd_amd.config import get_cfg
    from dcd_amd.model.head import detector_predictor as dp, trunk_moments
    from dcd_amd.structures.params_3d import stack_field
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.DEVICE", "cpu", "MODEL.USE_SYNC_BN", False, "INPUT.WIDTH_TRAIN", 320,
                        "INPUT.HEIGHT_TRAIN", 96] + list(opts))
    torch.manual_seed(0)
    pred = dp.make_predictor(cfg, 64)
    gi.name_hashed_init(pred)
    pred = pred.to(dtype).train()
    pred.sparse_training_heads = sparse
    _, targets = gi.model_inputs()
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 64, 24, 80, generator=g).to(dtype).requires_grad_()
    was = trunk_moments.ENABLED
    trunk_moments.ENABLED = moments
    try:
        out = pred(x, targets)
        if sparse:
            assert out["reg"] is None
            reg_pois = out["reg_pois"]
        else:
            c = stack_field(targets, "target_centers").long()
            lin = c[:, :, 1] * out["reg"].shape[3] + c[:, :, 0]
            reg_pois = out["reg"].flatten(2).gather(2, lin.unsqueeze(1).expand(-1, out["reg"].shape[1], -1)).transpose(1, 2)
        w_reg = torch.randn(reg_pois.shape, generator=g)
        w_cls = torch.randn(out["cls"].shape, generator=g)
        ((reg_pois * w_reg).sum() + (out["cls"] * w_cls).sum()).backward()
    finally:
        trunk_moments.ENABLED = was
    assert reg_pois.dtype == out["cls"].dtype == torch.float32
    return {"reg_pois": reg_pois.detach(), "cls": out["cls"].detach(), "x": x.grad,
            "params": {n: p.grad for n, p in pred.named_parameters() if p.grad is not None},
            "buffers": {n: b.clone() for n, b in pred.named_buffers()}}


def route(name, sparse, moments=None):
    opts, case_moments, dtype = CASES[name]
    moments = case_moments if moments is None else moments
    key = (opts, dtype, sparse, moments if sparse else True)         # the dense route does not look at the switch
    if key not in _RESULTS:
        _RESULTS[key] = run_route(opts, dtype, sparse, key[3])
    return _RESULTS[key]


def deviations(a, b, floored):
    """Worst |a - b|max / |b|max of the feature gradient and over the parameters (floored: on at least 1e-4 of the largest)."""
    fx = (a["x"] - b["x"]).abs().max().item() / b["x"].abs().max().item()
    assert a["params"].keys() == b["params"].keys()
    top = max(v.abs().max().item() for v in b["params"].values())
    fp, worst = 0.0, None
    for n, ref in b["params"].items():
        d = (a["params"][n] - ref).abs().max().item() / max(ref.abs().max().item(), 1e-4 * top if floored else 1e-300)
        if d > fp:
            fp, worst = d, n
    return fx, fp, worst


@pytest.mark.parametrize("name", list(CASES))
def test_sparse_route_equals_the_dense_map_at_the_centres(cpu_backend, name):
    dtype = CASES[name][2]
    a, b = route(name, True), route(name, False)
    d_reg = (a["reg_pois"] - b["reg_pois"]).abs().max().item()
    d_cls = (a["cls"] - b["cls"]).abs().max().item()
    fx, fp, worst = deviations(a, b, floored=dtype == torch.float32)
    print("%s: reg_pois %.2e (largest %.2e), cls %.2e, feature gradient %.2e, parameter gradients %.2e (%s)"
          % (name, d_reg, b["reg_pois"].abs().max().item(), d_cls, fx, fp, worst))
    assert d_reg <= 1e-4 * max(b["reg_pois"].abs().max().item(), 1.0)
    assert d_cls <= 1e-5
    assert fx <= FEATURE_GRAD_BOUND
    assert fp <= (DEEPER_PARAM_GRAD_BOUND if dtype == torch.float32 else PARAM_GRAD_BOUND), worst
    # BatchNorm buffers: statistics of the same maps in the working precision (float32: the bound of the class map)
    assert a["buffers"].keys() == b["buffers"].keys()
    tol = 1e-9 if dtype == torch.float64 else 1e-5
    for n, ref in b["buffers"].items():
        if n.endswith("num_batches_tracked"):
            assert torch.equal(a["buffers"][n], ref) and int(ref) == 1, n
        else:
            assert (a["buffers"][n] - ref).abs().max().item() <= tol * max(ref.abs().max().item(), 1.0), n


@pytest.mark.parametrize("name", ["default", "no_edge_fusion"])
def test_moments_route_equals_the_route_trunk_by_trunk(cpu_backend, name):
    """The same algebra in float64: trunks from the patch moments against conv + BatchNorm at positions, 1e-9 of each tensor's
    largest value (round-off of the two summation orders is some 1e-15)."""
    a, b = route(name, True, moments=True), route(name, True, moments=False)
    for key in ("reg_pois", "cls", "x"):
        assert (a[key] - b[key]).abs().max().item() <= 1e-9 * b[key].abs().max().item(), key
    for kind in ("params", "buffers"):
        assert a[kind].keys() == b[kind].keys()
        for n, ref in b[kind].items():
            assert (a[kind][n] - ref).abs().max().item() <= 1e-9 * ref.abs().max().item(), n
