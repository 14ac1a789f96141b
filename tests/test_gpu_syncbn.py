"""Synchronised batch normalisation at world size > 1 on ONE GPU: the split HIP kernels of csrc/norm.hip (statistics ->
[all-reduce of the fp64 sums] -> apply, forward and backward) and the plumbing around them in dcd_amd/ops.py and
dcd_amd/model/head/trunk_moments.py, against torch's stock ops in fp64 on the CONCATENATED batch of all ranks.

Two ranks cannot share a GPU under RCCL, but the split entry points take the combined sums and the global count as inputs
and every reduction in norm.hip has a fixed order, so tests/lockstep_ranks.py runs the R ranks one after the other, exactly
(proved on the CPU by tests/test_lockstep_ranks.py).  No process group, no RCCL, the default stream.

Which test reaches which entry point (asserted with a call-counting wrapper around the loaded library where it says "counted"):
  dcd_bn_stats                                test_split_kernels_*, test_emulated_ranks_equal_the_local_path (module, counted);
                                              by name: test_abi_*
  dcd_bn_train_apply                          the same (counted); by name with NULL weight / bias / running buffers: test_abi_null_*
  dcd_bn_backward_stats_params_relu_from_x,   ReLU without residual (counted)
  dcd_bn_backward_apply_relu_from_x
  dcd_bn_backward_stats_params,               the three other variants (counted): with the forward output and grad_residual
  dcd_bn_backward_apply                       (residual + ReLU), `gres = gy` (residual, no ReLU), y = NULL (neither);
                                              by name with grad_weight / grad_bias: test_abi_backward_apply_parameter_gradients
  dcd_bn_backward_stats                       by name: test_abi_backward_stats_equals_the_params_form
  dcd_bn_at_forward(stats != NULL),           test_forward_at_under_a_group (module, counted)
  dcd_bn_backward_apply(grad_y = NULL)
  dcd_trunk_finalize_forward / _backward      test_head_trunks_under_a_group (module, counted: the run took _TrunkScaleShift)
  all of them across two layers               test_basic_block_under_a_group

Bars.  None is read off the code under test:
  TOL = 2e-5 of the reference tensor's max magnitude, grad_residual 1e-7    tests/test_gpu_norm.py (TOL, _close): same kernels,
                                                                            same data, the sums combined in another order in fp64
  emulated ranks vs the local path: 1e-6 forward / running, 1e-5 gradients  test_bn_sync_group_world_size_1_equals_local
  forward_at: 2e-5                                                          test_bn_relu_at_positions_matches_dense_then_gather
  trunks: 1e-5 outputs, 1e-4 gradients, 1e-6 running estimates              test_fused_scale_shift_node_equals_tensor_operation_form
  block: 8e-5 = 4 stages x 2e-5                                             tests/test_gpu_conv.py + tests/test_gpu_norm.py
  dcd_bn_stats over B images vs its B one-image calls: 1e-14                fp64 rounding of a sum of B terms
  everything else: torch.equal

Worst measured error / scale per compared quantity on an MI355X, over all cases, variants and ranks (the module prints this
table at the end of a run with -s; "vs local" = against the one-launch path on the GPU, the others against fp64 on the CPU):
  quantity                                                   worst     bar
  y                                                          1.27e-07  2e-05
  grad_x                                                     2.25e-07  2e-05
  local grad_weight                                          3.11e-07  2e-05
  local grad_bias                                            1.21e-07  2e-05
  running_mean                                               9.61e-08  2e-05
  running_var                                                7.21e-08  2e-05
  grad_residual                                              0.00e+00  1e-07
  vs local: y                                                1.31e-07  1e-06
  vs local: grad_x                                           1.64e-07  1e-05
  vs local: running_mean                                     1.33e-07  1e-06
  vs local: running_var                                      0.00e+00  1e-06
  vs local: grad_weight                                      2.34e-07  1e-05
  vs local: grad_bias                                        8.21e-08  1e-05
  vs local: grad_residual                                    0.00e+00  1e-05
  forward_at: y_at                                           1.17e-07  2e-05
  forward_at: grad_x                                         1.32e-07  2e-05
  forward_at: running_mean                                   1.01e-07  2e-05
  forward_at: running_var                                    7.06e-08  2e-05
  forward_at: grad_weight                                    1.09e-07  2e-05
  forward_at: grad_bias                                      3.68e-08  2e-05
  trunks: outputs                                            0.00e+00  1e-05
  trunks: grad_input                                         2.98e-07  1e-04
  trunks: running estimates                                  0.00e+00  1e-06
  trunks: parameter gradients                                1.82e-07  1e-04
  block: output                                              3.16e-07  8e-05
  block: grad_x                                              2.52e-07  8e-05
  block: parameter gradients                                 5.18e-07  8e-05
  abi: y without weight / bias                               7.26e-08  2e-05
  abi: save_mean                                             2.98e-08  2e-05
  abi: save_invstd                                           5.48e-08  2e-05
  abi: local grad_weight                                     1.64e-07  2e-05
  abi: local grad_bias                                       3.06e-08  2e-05
  abi: grad_weight of the combined sums                      1.11e-07  2e-05
  abi: grad_bias of the combined sums                        4.02e-08  2e-05
  abi: grad_x                                                1.14e-07  2e-05
  abi: grad_residual                                         0.00e+00  1e-07
  abi: running_mean                                          7.25e-08  2e-05
  abi: running_var                                           4.84e-08  2e-05
  abi: stats of B images vs B calls, sum x                   0.00e+00  1e-14
  abi: stats of B images vs B calls, sum x^2                 0.00e+00  1e-14
"""
import collections

import pytest
import torch
from torch.nn import functional as F

from lockstep_ranks import lockstep

pytestmark = pytest.mark.gpu

TOL = 2e-5          # tests/test_gpu_norm.py
EPS = 1e-5

_WORST = collections.OrderedDict()      # quantity -> (worst err / scale, bar)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    print("\nworst error / scale per compared quantity (bar):")
    for what, (rel, tol) in _WORST.items():
        print("  %-58s %.2e  (%.0e)" % (what, rel, tol))


def _close(a, ref, what, tol=TOL, scale=None, family=None):
    """max |a - ref| <= tol * max |ref| (tests/test_gpu_norm.py `_close`); scale: the magnitude to use instead of ref's own.
    family: the row of the worst-error table the figure goes to (default: `what`)."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    assert a.shape == ref.shape, (what, tuple(a.shape), tuple(ref.shape))
    diff = (a - ref).abs()
    err = diff.max().item()
    scale = max(ref.abs().max().item() if scale is None else scale, 1e-6)
    key = family or what
    if err / scale > _WORST.get(key, (-1.0, tol))[0]:
        _WORST[key] = (err / scale, tol)
    assert err <= tol * scale, "%s: max abs err %.3e vs scale %.3e (%.2e of it, bar %.0e; %d of %d elements over the bar)" % (
        what, err, scale, err / scale, tol, int((diff > tol * scale).sum()), diff.numel())


class _Counting:
    """Wrapper around the loaded library object that counts the calls per entry point."""

    def __init__(self, real):
        self._real = real
        self.count = collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.count[name] += 1
            return fn(*args)
        return call


@pytest.fixture()
def counted(monkeypatch):
    from dcd_amd import _lib
    proxy = _Counting(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", proxy)
    return proxy.count


# ---------------------------------------------------------------------------------------------------------------------------
# inputs: equal shards whose statistics differ from rank to rank by tens of per cent
# ---------------------------------------------------------------------------------------------------------------------------
def _sigma_mu(rank):
    return 0.6 + 0.5 * (rank % 3), 0.8 - 0.7 * (rank % 4)


def _seed(B, C, H, W, R):
    return ((B * 1000 + C) * 1000 + H) * 1000 + W * 10 + R


def _shards(B, C, H, W, R, use_res):
    """[(x, residual or None, grad_y)] per rank, CPU fp32, and (weight, bias)."""
    g = torch.Generator(device="cpu").manual_seed(_seed(B, C, H, W, R))
    weight = torch.rand(C, generator=g) + 0.5
    bias = torch.randn(C, generator=g) * 0.3
    out = []
    for r in range(R):
        s, m = _sigma_mu(r)
        x = torch.randn(B, C, H, W, generator=g) * s + m
        res = torch.randn(B, C, H, W, generator=g) if use_res else None
        gy = torch.randn(B, C, H, W, generator=g)
        out.append((x, res, gy))
    return out, weight, bias


def _reference(shards, weight, bias, relu):
    """fp64 on the CPU: F.batch_norm(training) on the concatenated batch, + residual, relu, autograd with the concatenated grad_y
    (tests/test_gpu_norm.py `_reference`), and from dz = d loss / d pre-activation the per-rank LOCAL parameter gradients
    gw_r = sum over rank r of dz * xhat, gb_r = sum over rank r of dz, xhat with the GLOBAL statistics: what SyncBN leaves on
    each rank before DDP averages (include/dcd_hip.h, above dcd_bn_backward_stats_params).

    (With ReLU the derivative jumps at pre-activation z = 0 and the kernels evaluate z in fp32, so an element whose fp64 |z| is
    below the fp32 rounding of its own evaluation, about 1e-7, could take the other branch: grad_x / grad_residual would then
    be off by that element's whole grad_y -- the message of `_close` says "1 of N elements over the bar".  No element of these
    cases does; nothing here allows for it.)"""
    R, B = len(shards), shards[0][0].shape[0]
    xd = torch.cat([s[0] for s in shards]).double().requires_grad_()
    rd = None if shards[0][1] is None else torch.cat([s[1] for s in shards]).double().requires_grad_()
    gy = torch.cat([s[2] for s in shards]).double()
    wd, bd = weight.double().requires_grad_(), bias.double().requires_grad_()
    rm, rv = torch.zeros_like(wd), torch.ones_like(wd)
    z = F.batch_norm(xd, rm, rv, wd, bd, True, 0.1, EPS)
    if rd is not None:
        z = z + rd
    y = F.relu(z) if relu else z * 1.0
    z.retain_grad()
    y.backward(gy)
    dz = z.grad
    with torch.no_grad():
        mean = xd.mean((0, 2, 3), keepdim=True)
        var = xd.var((0, 2, 3), unbiased=False, keepdim=True)
        dzx = dz * ((xd - mean) * torch.rsqrt(var + EPS))
        gw_r = [dzx[r * B:(r + 1) * B].sum((0, 2, 3)) for r in range(R)]
        gb_r = [dz[r * B:(r + 1) * B].sum((0, 2, 3)) for r in range(R)]
    return dict(y=y.detach(), gx=xd.grad, gres=None if rd is None else rd.grad, gw=wd.grad, gb=bd.grad, gw_r=gw_r, gb_r=gb_r,
                rm=rm, rv=rv)


def _run_ranks(monkeypatch, cuda, shards, weight, bias, relu, fault=None):
    """The R ranks through BatchNorm2d with `sync_group` set, one after the other: per rank a dict of device tensors."""
    from dcd_amd.model.layers.norm import BatchNorm2d
    C = weight.numel()
    with lockstep(monkeypatch, fault=fault) as ranks:
        def fn(rank):
            x, res, gy = shards[rank]
            bn = BatchNorm2d(C, fuse_relu=relu).to(cuda).train()           # afresh: the forward updates the running buffers
            with torch.no_grad():
                bn.weight.copy_(weight)
                bn.bias.copy_(bias)
            bn.sync_group = ranks.group
            xg = x.to(cuda, copy=True).requires_grad_()
            rg = None if res is None else res.to(cuda, copy=True).requires_grad_()
            y = bn(xg, rg)
            y.backward(gy.to(cuda))
            return dict(y=y.detach(), gx=xg.grad, gres=None if rg is None else rg.grad, gw=bn.weight.grad, gb=bn.bias.grad,
                        rm=bn.running_mean.detach(), rv=bn.running_var.detach(), nbt=int(bn.num_batches_tracked))
        out = ranks.run(fn, len(shards))
        assert ranks.collectives == 2 and ranks.calls == 3 * len(shards)
    return out


def _compare_with_reference(out, ref, B):
    """Per rank: y, grad_x, grad_residual, the LOCAL grad_weight / grad_bias; on every rank the running estimates."""
    for r, o in enumerate(out):
        sl = slice(r * B, (r + 1) * B)
        _close(o["y"], ref["y"][sl], "y")
        _close(o["gx"], ref["gx"][sl], "grad_x")
        if ref["gres"] is not None:
            _close(o["gres"], ref["gres"][sl], "grad_residual", 1e-7)
        # scaled by the full-batch gradient: a rank with a small share is not held to a tighter bar than the sum
        _close(o["gw"], ref["gw_r"][r], "local grad_weight", scale=ref["gw"].abs().max().item())
        _close(o["gb"], ref["gb_r"][r], "local grad_bias", scale=ref["gb"].abs().max().item())
        _close(o["rm"], ref["rm"], "running_mean")
        _close(o["rv"], ref["rv"], "running_var")
        assert o["nbt"] == 1


CASES = [  # per-rank B, C, H, W; world size R
    (1, 64, 96, 320, 8),      # the DLA-34 levels at one image per rank: one slice per channel (B*HW <= 32768) ...
    (1, 128, 48, 160, 8),
    (1, 256, 24, 80, 8),
    (1, 512, 12, 40, 8),
    (1, 32, 192, 640, 4),     # ... and the two largest, two-stage; R keeps every fp64 reference tensor at or under 2^24 elements
    (1, 16, 384, 1280, 2),
    (1, 16, 128, 256, 2),     # the form boundary: B*HW = 32768 exactly, one slice
    (1, 16, 128, 260, 2),     # just above: two-stage
    (2, 16, 96, 320, 4),      # two-stage with two images per rank
    (2, 5, 7, 9, 3),          # HW % 4 != 0: scalar path
    (3, 33, 12, 40, 2),
    (1, 1, 3, 5, 2),          # small counts: the unbiased factor is 30/29 globally, 15/14 locally -- 3.6 % apart in running_var
    (1, 4, 4, 4, 8),
]
VARIANTS = [(False, True), (True, True), (True, False), (False, False)]      # residual, relu


def _expected_entry_points(use_res, relu):
    if relu and not use_res:
        return ("dcd_bn_stats", "dcd_bn_train_apply", "dcd_bn_backward_stats_params_relu_from_x", "dcd_bn_backward_apply_relu_from_x")
    return ("dcd_bn_stats", "dcd_bn_train_apply", "dcd_bn_backward_stats_params", "dcd_bn_backward_apply")


@pytest.mark.parametrize("use_res,relu", VARIANTS)
@pytest.mark.parametrize("B,C,H,W,R", CASES)
def test_split_kernels_match_fp64_full_batch(cuda, monkeypatch, counted, B, C, H, W, R, use_res, relu):
    shards, weight, bias = _shards(B, C, H, W, R, use_res)
    out = _run_ranks(monkeypatch, cuda, shards, weight, bias, relu)
    for name in _expected_entry_points(use_res, relu):
        assert counted[name] == 3 * R, (name, dict(counted))
    assert counted["dcd_bn_train_forward"] == 0 and counted["dcd_bn_backward"] == 0 and counted["dcd_bn_backward_relu_from_x"] == 0
    _compare_with_reference(out, _reference(shards, weight, bias, relu), B)


@pytest.mark.parametrize("use_res,relu", VARIANTS)
@pytest.mark.parametrize("B,C,H,W,R", CASES)
def test_emulated_ranks_equal_the_local_path(cuda, monkeypatch, B, C, H, W, R, use_res, relu):
    """R emulated ranks against the local one-launch path on the concatenated batch, both on the GPU: the same sums up to their
    order, so the bars of test_bn_sync_group_world_size_1_equals_local apply (1e-6 forward and running estimates, 1e-5
    gradients; parameter gradients summed over the ranks)."""
    from dcd_amd.model.layers.norm import BatchNorm2d
    shards, weight, bias = _shards(B, C, H, W, R, use_res)
    out = _run_ranks(monkeypatch, cuda, shards, weight, bias, relu)
    bn = BatchNorm2d(C, fuse_relu=relu).to(cuda).train()
    with torch.no_grad():
        bn.weight.copy_(weight)
        bn.bias.copy_(bias)
    xg = torch.cat([s[0] for s in shards]).to(cuda).requires_grad_()
    rg = torch.cat([s[1] for s in shards]).to(cuda).requires_grad_() if use_res else None
    y = bn(xg, rg)
    y.backward(torch.cat([s[2] for s in shards]).to(cuda))
    for r, o in enumerate(out):
        sl = slice(r * B, (r + 1) * B)
        _close(o["y"], y[sl], "y", 1e-6, family="vs local: y")
        _close(o["gx"], xg.grad[sl], "grad_x", 1e-5, family="vs local: grad_x")
        if use_res:
            _close(o["gres"], rg.grad[sl], "grad_residual", 1e-5, family="vs local: grad_residual")
        _close(o["rm"], bn.running_mean, "running_mean", 1e-6, family="vs local: running_mean")
        _close(o["rv"], bn.running_var, "running_var", 1e-6, family="vs local: running_var")
        assert o["nbt"] == 1
    _close(sum(o["gw"].double() for o in out), bn.weight.grad, "grad_weight summed over the ranks", 1e-5, family="vs local: grad_weight")
    _close(sum(o["gb"].double() for o in out), bn.bias.grad, "grad_bias summed over the ranks", 1e-5, family="vs local: grad_bias")


# ---------------------------------------------------------------------------------------------------------------------------
# negative controls: the same comparison must SEE a sum left unreduced and a count left unscaled
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", ["no_reduce:0", "no_reduce:1", "world_size_1"])
@pytest.mark.parametrize("B,C,H,W,R", [(1, 1, 3, 5, 2), (1, 128, 48, 160, 8)])
def test_negative_controls_fail_the_comparison(cuda, monkeypatch, B, C, H, W, R, fault):
    """Forward statistics left local, backward sums left local, the count not multiplied by the world size: ordinary launches
    with valid arguments whose results `_compare_with_reference` must refuse (nothing enters the worst-error table)."""
    shards, weight, bias = _shards(B, C, H, W, R, True)
    out = _run_ranks(monkeypatch, cuda, shards, weight, bias, True, fault=fault)
    ref = _reference(shards, weight, bias, True)
    saved = collections.OrderedDict(_WORST)
    try:
        with pytest.raises(AssertionError):
            _compare_with_reference(out, ref, B)
    finally:
        _WORST.clear()
        _WORST.update(saved)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm2d.forward_at (the regression-head trunks' BN evaluated at listed positions) under a group
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 8])
@pytest.mark.parametrize("B,C,H,W,N", [(2, 16, 12, 40, 7), (8, 256, 24, 80, 40), (1, 5, 7, 9, 3)])
def test_forward_at_under_a_group(cuda, monkeypatch, counted, B, C, H, W, N, R):
    """dcd_bn_at_forward with the combined sums and dcd_bn_backward_apply(grad_y = NULL) with the all-reduced sums, against fp64
    batch_norm -> relu -> gather on the concatenated batch (test_bn_relu_at_positions_matches_dense_then_gather, its 2e-5),
    a repeated position on every rank."""
    from dcd_amd.model.layers.norm import BatchNorm2d
    g = torch.Generator(device="cpu").manual_seed(B * 100 + C + 7 * R)
    w0, b0 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    per_rank = []
    for r in range(R):
        s, m = _sigma_mu(r)
        x = torch.randn(B, C, H, W, generator=g) * s + m
        pos = torch.randint(0, H * W, (B, N), generator=g)
        pos[:, -1] = pos[:, 0]
        per_rank.append((x, pos, torch.randn(B, N, C, generator=g)))
    xd = torch.cat([p[0] for p in per_rank]).double().requires_grad_()
    pos_all = torch.cat([p[1] for p in per_rank])
    wd, bd = w0.double().requires_grad_(), b0.double().requires_grad_()
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    y = F.relu(F.batch_norm(xd, rm, rv, wd, bd, True, 0.1, EPS))
    ref = y.flatten(2).gather(2, pos_all.unsqueeze(1).expand(R * B, C, N)).transpose(1, 2)
    ref.backward(torch.cat([p[2] for p in per_rank]).double())

    with lockstep(monkeypatch) as ranks:
        def fn(rank):
            x, pos, gout = per_rank[rank]
            bn = BatchNorm2d(C, fuse_relu=True).to(cuda).train()
            with torch.no_grad():
                bn.weight.copy_(w0)
                bn.bias.copy_(b0)
            bn.sync_group = ranks.group
            xg = x.to(cuda, copy=True).requires_grad_()
            out = bn.forward_at(xg, pos.to(cuda))
            out.backward(gout.to(cuda))
            return out.detach(), xg.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.detach(), bn.running_var.detach(), \
                int(bn.num_batches_tracked)
        out = ranks.run(fn, R)
        assert ranks.collectives == 2
    assert counted["dcd_bn_at_forward"] == 3 * R and counted["dcd_bn_stats"] == 3 * R and counted["dcd_bn_backward_apply"] == 3 * R
    for r, o in enumerate(out):
        sl = slice(r * B, (r + 1) * B)
        _close(o[0], ref.detach()[sl], "y_at", family="forward_at: y_at")
        _close(o[1], xd.grad[sl], "grad_x", family="forward_at: grad_x")
        _close(o[4], rm, "running_mean", family="forward_at: running_mean")
        _close(o[5], rv, "running_var", family="forward_at: running_var")
        assert o[6] == 1
    _close(sum(o[2].double() for o in out), wd.grad, "grad_weight summed over the ranks", family="forward_at: grad_weight")
    _close(sum(o[3].double() for o in out), bd.grad, "grad_bias summed over the ranks", family="forward_at: grad_bias")


# ---------------------------------------------------------------------------------------------------------------------------
# the head's regression trunks under a group, on the fused device path (_TrunkScaleShift)
# ---------------------------------------------------------------------------------------------------------------------------
def _trunk_modules(cuda, C, O, T, seed, group=None):
    from torch import nn
    from dcd_amd.model.layers.norm import BatchNorm2d
    g = torch.Generator(device="cpu").manual_seed(seed)
    trunks = nn.ModuleList([nn.Sequential(nn.Conv2d(C, O, 3, padding=1, bias=False), BatchNorm2d(O, fuse_relu=True), nn.Identity())
                            for _ in range(T)])
    with torch.no_grad():
        for t in trunks:
            t[0].weight.copy_(torch.randn(O, C, 3, 3, generator=g) / (9 * C) ** 0.5)
            t[1].weight.copy_(torch.rand(O, generator=g) + 0.5)
            t[1].bias.copy_(torch.rand(O, generator=g) - 0.5)
            t[1].sync_group = group
    return trunks.to(cuda).train()


@pytest.mark.parametrize("R,B", [(2, 2), (8, 1)])
def test_head_trunks_under_a_group(cuda, monkeypatch, counted, R, B):
    """trunk_moments.trunks_at with `sync_group` on every trunk's BN (dcd_trunk_finalize_forward / _backward with the global n,
    the all-reduce of the sums and of their gradients) against the same fused path at world size 1 on the concatenated batch,
    both on the GPU, at the bars of test_fused_scale_shift_node_equals_tensor_operation_form.  The two runs differ only in how
    the per-image pieces of G and S1 are grouped before the fp64 sum.  Input relu(randn) * sigma_r, no per-rank mean shift."""
    from dcd_amd.model.head import trunk_moments as TM
    C, H, W, O, T, M, Ke = 64, 24, 40, 32, 3, 7, 11
    monkeypatch.setenv("DCD_TRUNK_GRAM", "shift")
    g = torch.Generator(device="cpu").manual_seed(40 + R)
    per_rank = []
    for r in range(R):
        x = torch.relu(torch.randn(B, C, H, W, generator=g)) * _sigma_mu(r)[0]
        centers = torch.randint(0, H * W, (B, M), generator=g)
        extra = torch.randint(0, H * W, (B, Ke), generator=g)
        wts = [torch.randn(B, M + (Ke if i == 1 else 0), O, generator=g) for i in range(T)]
        per_rank.append((x, centers, extra, wts))

    def step(trunks, x, centers, extra, wts):
        xg = x.to(cuda, copy=True).requires_grad_()
        outs = TM.trunks_at(xg, trunks, centers.to(cuda), extra=(1, extra.to(cuda)))
        sum((o * w.to(cuda)).sum() for o, w in zip(outs, wts)).backward()
        return ([o.detach() for o in outs], xg.grad, [p.grad for p in trunks.parameters()],
                [t[1].running_mean.detach() for t in trunks] + [t[1].running_var.detach() for t in trunks],
                [int(t[1].num_batches_tracked) for t in trunks])

    with lockstep(monkeypatch) as ranks:
        out = ranks.run(lambda rank: step(_trunk_modules(cuda, C, O, T, 9, ranks.group), *per_rank[rank]), R)
        assert ranks.collectives == 2 and ranks.calls == 3 * R
        assert all(tuple(c.shape) == (T * O, 2) for col in ranks.recorded for c in col)
    # the run took _TrunkScaleShift, not the tensor-operation branch
    assert counted["dcd_trunk_finalize_forward"] == 3 * R and counted["dcd_trunk_finalize_backward"] == 3 * R, dict(counted)
    whole = step(_trunk_modules(cuda, C, O, T, 9), torch.cat([p[0] for p in per_rank]), torch.cat([p[1] for p in per_rank]),
                 torch.cat([p[2] for p in per_rank]), [torch.cat([p[3][i] for p in per_rank]) for i in range(T)])
    assert counted["dcd_trunk_finalize_forward"] == 3 * R + 1
    for r, o in enumerate(out):
        sl = slice(r * B, (r + 1) * B)
        for a, b in zip(o[0], whole[0]):
            _close(a, b[sl], "outputs", 1e-5, family="trunks: outputs")
        _close(o[1], whole[1][sl], "grad_input", 1e-4, family="trunks: grad_input")
        for a, b in zip(o[3], whole[3]):
            _close(a, b, "running estimate", 1e-6, family="trunks: running estimates")
        assert o[4] == [1] * T
    for i, b in enumerate(whole[2]):
        _close(sum(o[2][i].double() for o in out), b, "parameter gradient summed over the ranks", 1e-4, family="trunks: parameter gradients")


# ---------------------------------------------------------------------------------------------------------------------------
# a BasicBlock under a group: one layer's saved output and the next layer's residual gradient meet
# ---------------------------------------------------------------------------------------------------------------------------
BLOCK_TOL = 8e-5        # the four stages' own bars of 2e-5 (tests/test_gpu_conv.py, tests/test_gpu_norm.py) added up


def test_basic_block_under_a_group(cuda, monkeypatch):
    """dla_dcn.BasicBlock(64, 64) (conv -> BN + ReLU -> conv -> BN + residual -> ReLU) with both BN layers synchronised, per rank
    (1, 64, 24, 80), R = 2: four collectives, 10 calls.  Reference: the same block from stock ops in fp64 on the CPU on the
    concatenated batch with the same weights."""
    from dcd_amd.model.backbone.dla_dcn import BasicBlock
    R, B, C, H, W = 2, 1, 64, 24, 80
    g = torch.Generator(device="cpu").manual_seed(64)
    params = {"conv1.weight": torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5,
              "conv2.weight": torch.randn(C, C, 3, 3, generator=g) / (9 * C) ** 0.5,
              "bn1.weight": torch.rand(C, generator=g) + 0.5, "bn1.bias": torch.randn(C, generator=g) * 0.3,
              "bn2.weight": torch.rand(C, generator=g) + 0.5, "bn2.bias": torch.randn(C, generator=g) * 0.3}
    per_rank = []
    for r in range(R):
        s, m = _sigma_mu(r)
        per_rank.append((torch.randn(B, C, H, W, generator=g) * s + m, torch.randn(B, C, H, W, generator=g)))

    pd = {k: v.double().requires_grad_() for k, v in params.items()}
    xd = torch.cat([p[0] for p in per_rank]).double().requires_grad_()
    a = F.relu(F.batch_norm(F.conv2d(xd, pd["conv1.weight"], padding=1), None, None, pd["bn1.weight"], pd["bn1.bias"], True, 0.1, EPS))
    ref = F.relu(F.batch_norm(F.conv2d(a, pd["conv2.weight"], padding=1), None, None, pd["bn2.weight"], pd["bn2.bias"], True, 0.1, EPS) + xd)
    ref.backward(torch.cat([p[1] for p in per_rank]).double())

    with lockstep(monkeypatch) as ranks:
        def fn(rank):
            block = BasicBlock(C, C)
            block.load_state_dict(params, strict=False)
            block = block.to(cuda).train()
            block.bn1.sync_group = block.bn2.sync_group = ranks.group
            xg = per_rank[rank][0].to(cuda, copy=True).requires_grad_()
            out = block(xg)
            out.backward(per_rank[rank][1].to(cuda))
            named = dict(block.named_parameters())
            return out.detach(), xg.grad, {k: named[k].grad for k in params}
        out = ranks.run(fn, R)
        assert ranks.collectives == 4 and ranks.calls == 10
    for r, o in enumerate(out):
        sl = slice(r * B, (r + 1) * B)
        _close(o[0], ref.detach()[sl], "block output", BLOCK_TOL, family="block: output")
        _close(o[1], xd.grad[sl], "block grad_x", BLOCK_TOL, family="block: grad_x")
    for k in params:
        _close(sum(o[2][k].double() for o in out), pd[k].grad, "block %s.grad summed over the ranks" % k, BLOCK_TOL,
               family="block: parameter gradients")


# ---------------------------------------------------------------------------------------------------------------------------
# the C ABI forms that ops.py never passes: straight through the library, the shards' sums added on the device by the test
# ---------------------------------------------------------------------------------------------------------------------------
ABI_SHAPES = [(2, 5, 7, 9), (1, 64, 24, 80)]        # per rank, R = 2


class _Abi:
    """Two ranks' split forward straight through the C entry points; everything stays on the device."""

    def __init__(self, cuda, B, C, H, W, use_res, relu, affine=True, running=True, R=2):
        from dcd_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.B, self.C, self.HW, self.R, self.relu = B, C, H * W, R, relu
        self.count = float(R * B * H * W)
        self.shards, self.weight, self.bias = _shards(B, C, H, W, R, use_res)
        if not affine:
            self.weight = self.bias = None
        self.dev = [tuple(None if t is None else t.to(cuda) for t in s) for s in self.shards]
        self.w = None if self.weight is None else self.weight.to(cuda)
        self.b = None if self.bias is None else self.bias.to(cuda)
        self.ws = torch.empty(self.L.dcd_bn_workspace_bytes(C), dtype=torch.uint8, device=cuda)
        self.st = _lib.stream_of(self.ws)
        self.running = running
        self.cuda = cuda

    def stats(self, x):
        out = torch.empty((self.C, 2), dtype=torch.float64, device=self.cuda)
        assert self.L.dcd_bn_stats(self.st, x.data_ptr(), x.shape[0], self.C, self.HW, out.data_ptr(), self.ws.data_ptr(), self.ws.numel()) == 0
        return out

    def forward(self):
        p = self.lib.ptr
        self.total = sum(self.stats(d[0]) for d in self.dev)
        self.fwd = []
        for x, res, _ in self.dev:
            y = torch.empty_like(x)
            sm = torch.empty(self.C, device=self.cuda)
            si = torch.empty(self.C, device=self.cuda)
            rm = torch.zeros(self.C, device=self.cuda) if self.running else None
            rv = torch.ones(self.C, device=self.cuda) if self.running else None
            nbt = torch.zeros((), dtype=torch.int64, device=self.cuda) if self.running else None
            assert self.L.dcd_bn_train_apply(self.st, x.data_ptr(), p(res), p(self.w), p(self.b), self.total.data_ptr(), self.count,
                                             p(rm), p(rv), p(nbt), 0.1, EPS, int(self.relu), y.data_ptr(), sm.data_ptr(), si.data_ptr(),
                                             self.B, self.C, self.HW) == 0
            self.fwd.append(dict(y=y, save_mean=sm, save_invstd=si, rm=rm, rv=rv, nbt=nbt))
        return self.fwd

    def reference(self):
        w = torch.ones(self.C) if self.weight is None else self.weight
        b = torch.zeros(self.C) if self.bias is None else self.bias
        return _reference(self.shards, w, b, self.relu)


@pytest.mark.parametrize("B,C,H,W", ABI_SHAPES)
def test_abi_null_affine_and_null_running_buffers(cuda, B, C, H, W):
    """dcd_bn_train_apply with weight = bias = NULL (1 / 0) and running_mean = running_var = num_batches_tracked = NULL."""
    abi = _Abi(cuda, B, C, H, W, use_res=True, relu=True, affine=False, running=False)
    fwd = abi.forward()
    ref = abi.reference()
    xd = torch.cat([s[0] for s in abi.shards]).double()
    mean, var = xd.mean((0, 2, 3)), xd.var((0, 2, 3), unbiased=False)
    for r, f in enumerate(fwd):
        _close(f["y"], ref["y"][r * B:(r + 1) * B], "y", family="abi: y without weight / bias")
        _close(f["save_mean"], mean, "save_mean", family="abi: save_mean")
        _close(f["save_invstd"], torch.rsqrt(var + EPS), "save_invstd", family="abi: save_invstd")


@pytest.mark.parametrize("B,C,H,W", ABI_SHAPES)
def test_abi_backward_apply_parameter_gradients(cuda, B, C, H, W):
    """dcd_bn_backward_apply with grad_weight / grad_bias: S1 * invstd and S0 OF THE SUMS PASSED IN (include/dcd_hip.h: "of THIS
    call's sums") -- with the all-reduced sums that is the full-batch gradient, whichever rank computes it."""
    abi = _Abi(cuda, B, C, H, W, use_res=True, relu=True)
    fwd = abi.forward()
    ref = abi.reference()
    L, p = abi.L, abi.lib.ptr
    sums, local = [], []
    for (x, res, gy), f in zip(abi.dev, fwd):
        s = torch.empty((C, 2), dtype=torch.float64, device=cuda)
        gw, gb = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        assert L.dcd_bn_backward_stats_params(abi.st, gy.data_ptr(), f["y"].data_ptr(), x.data_ptr(), f["save_mean"].data_ptr(),
                                              f["save_invstd"].data_ptr(), B, C, abi.HW, s.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                                              abi.ws.data_ptr(), abi.ws.numel()) == 0
        sums.append(s)
        local.append((gw, gb))
    total = sums[0] + sums[1]
    for r, ((x, res, gy), f) in enumerate(zip(abi.dev, fwd)):
        # the stats form's own parameter gradients are those of ITS sums: the local ones
        assert torch.equal(local[r][0], (sums[r][:, 1] * f["save_invstd"].double()).float())
        assert torch.equal(local[r][1], sums[r][:, 0].float())
        _close(local[r][0], ref["gw_r"][r], "local grad_weight", scale=ref["gw"].abs().max().item(), family="abi: local grad_weight")
        _close(local[r][1], ref["gb_r"][r], "local grad_bias", scale=ref["gb"].abs().max().item(), family="abi: local grad_bias")
        gx, gres = torch.empty_like(x), torch.empty_like(x)
        gw, gb = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        assert L.dcd_bn_backward_apply(abi.st, gy.data_ptr(), f["y"].data_ptr(), x.data_ptr(), p(abi.w), f["save_mean"].data_ptr(),
                                       f["save_invstd"].data_ptr(), total.data_ptr(), abi.count, gx.data_ptr(), gres.data_ptr(),
                                       gw.data_ptr(), gb.data_ptr(), B, C, abi.HW) == 0
        assert torch.equal(gw, (total[:, 1] * f["save_invstd"].double()).float())
        assert torch.equal(gb, total[:, 0].float())
        _close(gw, ref["gw"], "grad_weight of the combined sums", family="abi: grad_weight of the combined sums")
        _close(gb, ref["gb"], "grad_bias of the combined sums", family="abi: grad_bias of the combined sums")
        _close(gx, ref["gx"][r * B:(r + 1) * B], "grad_x", family="abi: grad_x")
        _close(gres, ref["gres"][r * B:(r + 1) * B], "grad_residual", 1e-7, family="abi: grad_residual")
        _close(f["rm"], ref["rm"], "running_mean", family="abi: running_mean")
        _close(f["rv"], ref["rv"], "running_var", family="abi: running_var")
        assert int(f["nbt"]) == 1


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,C,H,W", ABI_SHAPES + [(1, 16, 128, 260)])       # ... and one two-stage shape (bn_combine writes the sums)
def test_abi_backward_stats_equals_the_params_form(cuda, B, C, H, W, relu):
    """dcd_bn_backward_stats (no parameter gradients) gives the `sums` of dcd_bn_backward_stats_params bit for bit."""
    abi = _Abi(cuda, B, C, H, W, use_res=True, relu=relu)
    fwd = abi.forward()
    L, p = abi.L, abi.lib.ptr
    for (x, res, gy), f in zip(abi.dev, fwd):
        y = f["y"] if relu else None
        a = torch.full((C, 2), float("nan"), dtype=torch.float64, device=cuda)
        b = torch.full((C, 2), float("nan"), dtype=torch.float64, device=cuda)
        gw, gb = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        assert L.dcd_bn_backward_stats(abi.st, gy.data_ptr(), p(y), x.data_ptr(), f["save_mean"].data_ptr(), B, C, abi.HW, a.data_ptr(),
                                       abi.ws.data_ptr(), abi.ws.numel()) == 0
        assert L.dcd_bn_backward_stats_params(abi.st, gy.data_ptr(), p(y), x.data_ptr(), f["save_mean"].data_ptr(),
                                              f["save_invstd"].data_ptr(), B, C, abi.HW, b.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                                              abi.ws.data_ptr(), abi.ws.numel()) == 0
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize("B,C,H,W", ABI_SHAPES + [(2, 16, 96, 320)])        # ... and one whose B images take the two-stage form
def test_abi_stats_of_a_shard_equal_the_sum_of_its_images(cuda, B, C, H, W):
    """What is exchanged does not depend on how the images are partitioned, beyond fp64 rounding: dcd_bn_stats over B images
    against the fp64 sum of its B one-image calls, 1e-14 of the largest sum."""
    abi = _Abi(cuda, B, C, H, W, use_res=False, relu=True)
    for x, _, _ in abi.dev:
        whole = abi.stats(x)
        pieces = sum(abi.stats(x[i:i + 1]) for i in range(B))
        for k, what in ((0, "sum x"), (1, "sum x^2")):
            _close(whole[:, k], pieces[:, k], what, 1e-14, family="abi: stats of B images vs B calls, " + what)


def test_abi_argument_checks(cuda):
    """The argument checks the split entry points implement today: NULL `stats` / `sums`, count < 1 and NaN count
    (`!(count >= 1.0)`), running_mean without running_var, a short workspace.  All are refused before any launch."""
    from dcd_amd import _lib
    L = _lib.lib()
    B, C, HW, N = 2, 4, 9, 3
    x = torch.randn(B, C, 3, 3, device=cuda)
    y, gy, gx = torch.empty_like(x), torch.randn_like(x), torch.empty_like(x)
    v = [torch.ones(C, device=cuda) for _ in range(4)]            # save_mean, save_invstd, running_mean, running_var
    d = torch.ones((C, 2), dtype=torch.float64, device=cuda)
    ws = torch.empty(L.dcd_bn_workspace_bytes(C), dtype=torch.uint8, device=cuda)
    st, X, Y, GY, GX, D, WS, n = _lib.stream_of(x), x.data_ptr(), y.data_ptr(), gy.data_ptr(), gx.data_ptr(), d.data_ptr(), ws.data_ptr(), ws.numel()
    SM, SI, RM, RV = (t.data_ptr() for t in v)
    BAD, SHORT = 1, 2
    nan = float("nan")

    def apply(stats, count, rm=None, rv=None):
        return L.dcd_bn_train_apply(st, X, None, None, None, stats, count, rm, rv, None, 0.1, EPS, 1, Y, SM, SI, B, C, HW)
    assert apply(None, 18.0) == BAD
    assert apply(D, 0.5) == BAD and apply(D, 0.0) == BAD and apply(D, -3.0) == BAD and apply(D, nan) == BAD
    assert apply(D, 18.0, rm=RM) == BAD and apply(D, 18.0, rv=RV) == BAD
    assert apply(D, 1.0, rm=RM, rv=RV) == 0                       # count = 1 is the smallest the check admits

    assert L.dcd_bn_stats(st, X, B, C, HW, None, WS, n) == BAD
    assert L.dcd_bn_stats(st, X, B, C, HW, D, WS, n - 1) == SHORT and L.dcd_bn_stats(st, X, B, C, HW, D, None, n) == SHORT
    assert L.dcd_bn_backward_stats(st, GY, None, X, SM, B, C, HW, None, WS, n) == BAD
    assert L.dcd_bn_backward_stats(st, GY, None, X, SM, B, C, HW, D, WS, n - 1) == SHORT
    assert L.dcd_bn_backward_stats_params(st, GY, None, X, SM, SI, B, C, HW, None, None, None, WS, n) == BAD
    assert L.dcd_bn_backward_stats_params(st, GY, None, X, SM, None, B, C, HW, D, SM, None, WS, n) == BAD     # grad_weight needs invstd
    assert L.dcd_bn_backward_stats_params(st, GY, None, X, SM, SI, B, C, HW, D, None, None, WS, n - 1) == SHORT
    assert L.dcd_bn_backward_stats_params_relu_from_x(st, GY, X, None, None, SM, SI, B, C, HW, None, None, None, WS, n) == BAD
    assert L.dcd_bn_backward_stats_params_relu_from_x(st, GY, X, None, None, SM, None, B, C, HW, D, None, None, WS, n) == BAD
    assert L.dcd_bn_backward_stats_params_relu_from_x(st, GY, X, None, None, SM, SI, B, C, HW, D, None, None, WS, n - 1) == SHORT
    for count in (0.5, 0.0, nan):
        assert L.dcd_bn_backward_apply(st, GY, None, X, None, SM, SI, D, count, GX, None, None, None, B, C, HW) == BAD
        assert L.dcd_bn_backward_apply_relu_from_x(st, GY, X, None, None, SM, SI, D, count, GX, B, C, HW) == BAD
    assert L.dcd_bn_backward_apply(st, GY, None, X, None, SM, SI, None, 18.0, GX, None, None, None, B, C, HW) == BAD
    assert L.dcd_bn_backward_apply_relu_from_x(st, GY, X, None, None, SM, SI, None, 18.0, GX, B, C, HW) == BAD

    pos = torch.zeros((B, N), dtype=torch.int64, device=cuda)
    xa, ya = torch.empty(B, N, C, device=cuda), torch.empty(B, N, C, device=cuda)

    def at(stats, count, rm=None, rv=None, ws_bytes=n):
        return L.dcd_bn_at_forward(st, X, pos.data_ptr(), None, None, stats, count, rm, rv, None, 0.1, EPS, 1, xa.data_ptr(), ya.data_ptr(),
                                   SM, SI, B, C, HW, N, WS, ws_bytes)
    assert at(D, 0.5) == BAD and at(D, nan) == BAD and at(D, 18.0, rm=RM) == BAD
    assert at(None, 18.0, ws_bytes=n - 1) == SHORT                # the workspace is needed only when the statistics are computed here
    assert at(D, 18.0, ws_bytes=0) == 0

    R = 6
    f = [torch.ones(R, device=cuda) for _ in range(4)]
    d2 = torch.ones((R, 2), dtype=torch.float64, device=cuda)
    d3 = torch.ones((R, 3), dtype=torch.float64, device=cuda)
    for count in (0.5, nan):
        assert L.dcd_trunk_finalize_forward(st, d2.data_ptr(), f[0].data_ptr(), f[1].data_ptr(), count, 1e-5, R, f[2].data_ptr(),
                                            f[3].data_ptr(), d3.data_ptr()) == BAD
        assert L.dcd_trunk_finalize_backward(st, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), d3.data_ptr(), count, R, d2.data_ptr(),
                                             f[3].data_ptr(), f[3].data_ptr()) == BAD
    assert L.dcd_trunk_finalize_forward(st, None, f[0].data_ptr(), f[1].data_ptr(), 18.0, 1e-5, R, f[2].data_ptr(), f[3].data_ptr(),
                                        d3.data_ptr()) == BAD
    torch.cuda.synchronize()
