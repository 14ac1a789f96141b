"""The rest of csrc/norm.hip, the DCN glue and the shifted GEMM through the C ABI on poisoned, guarded buffers (tests/arena.py):
the synchronised (split) batch-norm calls at one rank, dcd_bn_eval_apply, the dcd_bn_at_* pair, the four dcd_trunk_* calls,
dcd_dcn_offset_mask_split / _merge and dcd_sgemm_shifted.

The pattern of tests/test_gpu_poisoned_backbone.py: inputs between guard words of NaN, outputs and workspaces (of exactly the
advertised byte count) poisoned, status 0, `Arena.check`, then the SAME reference at the SAME bound as the kernel's value test,
cited at each assert.  The outputs of one call are re-placed as the inputs of the next.  The statistics ("fp64 two-stage sum,
rounded once", sums in a fixed order) run a second time on zero-filled outputs and scratch and must give the same bits.

dcd_sgemm_shifted reads shifted views that reach outside the plane by design: the padded buffer is ONE input of exactly
2 * guard + B * C * Lp floats, as trunk_moments._ShiftCorr allocates it, so the reads may use the caller's zero margin and must not
reach the NaN beyond it.  With the product's own rule (nsplit = max(1, min(16, Lp // 1024))) both shapes here run unsplit, so the
second one also runs with nsplit = 2.

The negative controls were tried on an MI355X on copies of this file, in test_sgemm_shifted[2-64-6-10-0].  With `dxp` one float
short the backward fails with "back guard of output 'dxp' overwritten: 1 words, the first at float offset 20479"; the same copy
without `ar.check(what)` (and the reference cut to match) passes.  With the margin of the padded buffer cut from 2 * Wp + 8 to
2 * Wp floats the shifted reads reach the arena's NaN and the forward's R is NaN.  (No batch-norm workspace is a control here: the
statistics of these shapes use the first C * S * 16 of its C * 256 * 16 bytes, so four bytes less at its end change nothing.)"""
import functools
from types import SimpleNamespace

import pytest
import torch
from torch.nn import functional as F

from arena import Arena
from test_gpu_poisoned_backbone import _close, _lib_and_stream, _ptr, _same, bn_problem

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- split batch norm chain
@functools.lru_cache(maxsize=None)
def plain_bn_problem(B, C, H, W):
    """bn_problem's x, residual and grad_y without weight and bias (NULL: 1 and 0), residual and ReLU on (do not modify)."""
    q = bn_problem(B, C, H, W, True, True)
    p = SimpleNamespace(x=q.x, res=q.res, gy=q.gy, w=None, b=None)
    xd, rd = p.x.double().requires_grad_(), p.res.double().requires_grad_()
    y = F.relu(F.batch_norm(xd, None, None, None, None, True, 0.1, 1e-5) + rd)
    y.backward(p.gy.double())
    p.y, p.gx, p.gr, p.gw, p.gb = y.detach(), xd.grad, rd.grad, None, None
    return p


def _stats(cuda, p, B, C, HW, poison):
    L, st = _lib_and_stream(cuda)
    n = L.dcd_bn_workspace_bytes(C)
    ar = Arena(cuda, poison)
    x = ar.place(p.x, "x")
    stats = ar.out((C, 2), "stats", dtype=torch.float64)
    ws = ar.scratch(n, "workspace")
    assert L.dcd_bn_stats(st, x.data_ptr(), B, C, HW, stats.data_ptr(), ar.ptr(ws), n) == 0
    ar.check("dcd_bn_stats poison %d" % poison)
    return stats.cpu()


BN_SHAPES = [(2, 5, 7, 9, True, True, True),              # HW % 4 != 0: scalar path
             (2, 5, 7, 9, True, True, False),             # the same without weight, bias and running buffers (NULL)
             (3, 33, 12, 40, True, False, True),
             (2, 64, 12, 40, False, True, True),          # ReLU without residual: the mask recomputed from x
             (1, 5, 129, 256, False, True, True),         # B HW = 33 024 > 32 768: the statistics go through the workspace and a combine
             (1, 3, 181, 183, True, True, True)]          # past 32 768 with HW % 4 != 0


@pytest.mark.parametrize("B,C,H,W,use_res,relu,affine", BN_SHAPES)
def test_split_batch_norm_chain(cuda, B, C, H, W, use_res, relu, affine):
    """dcd_bn_stats -> dcd_bn_train_apply -> dcd_bn_backward_stats_params (or _relu_from_x) -> dcd_bn_backward_apply (or
    _relu_from_x), dcd_bn_backward_stats alone and dcd_bn_eval_apply at count = B HW, against batch_norm + add + relu in fp64 at
    2e-5, the residual's gradient at 1e-7 (test_batch_norm of tests/test_gpu_poisoned_backbone.py, test_bn_act_train_matches_stock_ops);
    statistics and sums bitwise the same from poisoned and zero-filled memory."""
    L, st = _lib_and_stream(cuda)
    p = bn_problem(B, C, H, W, use_res, relu) if affine else plain_bn_problem(B, C, H, W)
    HW, count = H * W, float(B * H * W)
    n = L.dcd_bn_workspace_bytes(C)
    xd = p.x.double()
    stats = _stats(cuda, p, B, C, HW, True)
    _same(stats.view(torch.float32), _stats(cuda, p, B, C, HW, False).view(torch.float32), "dcd_bn_stats")
    _close(stats, torch.stack((xd.sum(dim=(0, 2, 3)), (xd * xd).sum(dim=(0, 2, 3))), 1), "stats")

    ar = Arena(cuda)
    x, dstats = ar.place(p.x, "x"), ar.place(stats, "stats")
    w, b = (ar.place(p.w, "weight"), ar.place(p.b, "bias")) if affine else (None, None)
    res = ar.place(p.res, "residual") if use_res else None
    rm = ar.place(torch.zeros(C), "running_mean", inplace=True) if affine else None
    rv = ar.place(torch.ones(C), "running_var", inplace=True) if affine else None
    nbt = ar.place(torch.zeros(1, dtype=torch.int64), "num_batches_tracked", inplace=True) if affine else None
    y, mean, invstd = ar.out(p.x.shape, "y"), ar.out((C,), "save_mean"), ar.out((C,), "save_invstd")
    assert L.dcd_bn_train_apply(st, x.data_ptr(), _ptr(res), _ptr(w), _ptr(b), dstats.data_ptr(), count, _ptr(rm), _ptr(rv), _ptr(nbt),
                                0.1, 1e-5, int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), B, C, HW) == 0
    ar.check("dcd_bn_train_apply")
    _close(y, p.y, "y")
    var = xd.var(dim=(0, 2, 3), unbiased=False)
    _close(mean, xd.mean(dim=(0, 2, 3)), "save_mean")
    _close(invstd, 1.0 / torch.sqrt(var + 1e-5), "save_invstd")
    if affine:
        _close(rm, p.rm, "running_mean")
        _close(rv, p.rv, "running_var")
        assert int(nbt.cpu()) == 1
    y_cpu, mean_cpu, invstd_cpu = y.cpu(), mean.cpu(), invstd.cpu()

    def backward(from_x):
        got = []
        for poison in (True, False):
            ar = Arena(cuda, poison)
            gy, x = ar.place(p.gy, "grad_y"), ar.place(p.x, "x")
            mean, invstd = ar.place(mean_cpu, "save_mean"), ar.place(invstd_cpu, "save_invstd")
            w, b = (ar.place(p.w, "weight"), ar.place(p.b, "bias")) if affine else (None, None)
            y = ar.place(y_cpu, "y") if relu and not from_x else None
            sums = ar.out((C, 2), "sums", dtype=torch.float64)
            gw, gb = ar.out((C,), "grad_weight"), ar.out((C,), "grad_bias")
            ws = ar.scratch(n, "workspace")
            if from_x:
                status = L.dcd_bn_backward_stats_params_relu_from_x(st, gy.data_ptr(), x.data_ptr(), _ptr(w), _ptr(b), mean.data_ptr(),
                                                                    invstd.data_ptr(), B, C, HW, sums.data_ptr(), gw.data_ptr(),
                                                                    gb.data_ptr(), ar.ptr(ws), n)
            else:
                status = L.dcd_bn_backward_stats_params(st, gy.data_ptr(), _ptr(y), x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), B, C, HW,
                                                        sums.data_ptr(), gw.data_ptr(), gb.data_ptr(), ar.ptr(ws), n)
            what = "dcd_bn_backward_stats_params%s poison %d" % ("_relu_from_x" if from_x else "", poison)
            assert status == 0, "%s: status %d" % (what, status)
            ar.check(what)
            got.append((sums.cpu(), gw.cpu(), gb.cpu()))
        for a_, b_, nm in zip(got[0], got[1], ("sums", "grad_weight", "grad_bias")):
            _same(a_.view(torch.float32), b_.view(torch.float32), "backward statistics: %s" % nm)
        sums_cpu, gw_cpu, gb_cpu = got[0]
        if affine:
            _close(gw_cpu, p.gw, "stats_params grad_weight")
            _close(gb_cpu, p.gb, "stats_params grad_bias")

        if not from_x:                                      # dcd_bn_backward_stats alone: the same sums, no parameter gradients
            ar = Arena(cuda)
            gy, x, mean = ar.place(p.gy, "grad_y"), ar.place(p.x, "x"), ar.place(mean_cpu, "save_mean")
            y = ar.place(y_cpu, "y") if relu else None
            sums = ar.out((C, 2), "sums", dtype=torch.float64)
            ws = ar.scratch(n, "workspace")
            assert L.dcd_bn_backward_stats(st, gy.data_ptr(), _ptr(y), x.data_ptr(), mean.data_ptr(), B, C, HW, sums.data_ptr(), ar.ptr(ws), n) == 0
            ar.check("dcd_bn_backward_stats")
            _same(sums.cpu().view(torch.float32), sums_cpu.view(torch.float32), "dcd_bn_backward_stats against _stats_params")

        ar = Arena(cuda)
        gy, x = ar.place(p.gy, "grad_y"), ar.place(p.x, "x")
        mean, invstd = ar.place(mean_cpu, "save_mean"), ar.place(invstd_cpu, "save_invstd")
        w, b = (ar.place(p.w, "weight"), ar.place(p.b, "bias")) if affine else (None, None)
        dsums = ar.place(sums_cpu, "sums")
        gx = ar.out(p.x.shape, "grad_x")
        gres = gw = gb = None
        if from_x:
            status = L.dcd_bn_backward_apply_relu_from_x(st, gy.data_ptr(), x.data_ptr(), _ptr(w), _ptr(b), mean.data_ptr(), invstd.data_ptr(),
                                                         dsums.data_ptr(), count, gx.data_ptr(), B, C, HW)
        else:
            y = ar.place(y_cpu, "y") if relu else None
            gres = ar.out(p.x.shape, "grad_residual") if use_res else None
            gw, gb = ar.out((C,), "grad_weight"), ar.out((C,), "grad_bias")
            status = L.dcd_bn_backward_apply(st, gy.data_ptr(), _ptr(y), x.data_ptr(), _ptr(w), mean.data_ptr(), invstd.data_ptr(),
                                             dsums.data_ptr(), count, gx.data_ptr(), _ptr(gres), gw.data_ptr(), gb.data_ptr(), B, C, HW)
        what = "dcd_bn_backward_apply%s" % ("_relu_from_x" if from_x else "")
        assert status == 0, "%s: status %d" % (what, status)
        ar.check(what)
        _close(gx, p.gx, what + " grad_x")
        if gres is not None:
            _close(gres, p.gr, what + " grad_residual", 1e-7)
        if gw is not None:
            _same(gw, gw_cpu, what + " grad_weight against the statistics call's")
            _same(gb, gb_cpu, what + " grad_bias against the statistics call's")

    backward(False)
    if relu and not use_res:
        backward(True)

    if affine:                                              # eval mode on running statistics that are not (0, 1)
        g = torch.Generator().manual_seed(C)
        rmean, rvar = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) + 0.5
        ref = F.batch_norm(xd, rmean.double(), rvar.double(), p.w.double(), p.b.double(), False, 0.1, 1e-5)
        ref = ref + p.res.double() if use_res else ref
        ref = F.relu(ref) if relu else ref
        ar = Arena(cuda)
        x, w, b = ar.place(p.x, "x"), ar.place(p.w, "weight"), ar.place(p.b, "bias")
        res = ar.place(p.res, "residual") if use_res else None
        rm, rv = ar.place(rmean, "running_mean"), ar.place(rvar, "running_var")
        y = ar.out(p.x.shape, "y")
        assert L.dcd_bn_eval_apply(st, x.data_ptr(), _ptr(res), w.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), 1e-5, int(relu),
                                   y.data_ptr(), B, C, HW) == 0
        ar.check("dcd_bn_eval_apply")
        _close(y, ref, "eval y")


# ------------------------------------------------------------------------------------------------------ BN at positions
@pytest.mark.parametrize("B,C,H,W,N", [(1, 5, 7, 9, 3), (2, 16, 12, 40, 7)])
def test_bn_at_positions(cuda, B, C, H, W, N):
    """dcd_bn_at_forward (statistics computed here, and given), dcd_bn_at_backward_sums and dcd_bn_backward_apply(grad_y = NULL,
    y = NULL) + the scatter of dzk against batch_norm -> relu -> gather in fp64 at 2e-5
    (test_bn_relu_at_positions_matches_dense_then_gather), with a repeated position."""
    L, st = _lib_and_stream(cuda)
    HW, count = H * W, float(B * H * W)
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.4
    pos = torch.randint(0, HW, (B, N), generator=g)
    pos[:, -1] = pos[:, 0]
    gout = torch.randn(B, N, C, generator=g)
    w0, b0 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    xd, wd, bd = x.double().requires_grad_(), w0.double().requires_grad_(), b0.double().requires_grad_()
    rm_ref, rv_ref = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    yd = F.relu(F.batch_norm(xd, rm_ref, rv_ref, wd, bd, True, 0.1, 1e-5))
    ref = yd.flatten(2).gather(2, pos.unsqueeze(1).expand(B, C, N)).transpose(1, 2)
    ref.backward(gout.double())
    x_at_ref = x.flatten(2).gather(2, pos.unsqueeze(1).expand(B, C, N)).transpose(1, 2)
    n = L.dcd_bn_workspace_bytes(C)
    stats_cpu = _stats(cuda, SimpleNamespace(x=x), B, C, HW, True)

    kept = None
    for given in (False, True):
        ar = Arena(cuda)
        dx, dpos, w, b = ar.place(x, "x"), ar.place(pos, "pos"), ar.place(w0, "weight"), ar.place(b0, "bias")
        dstats = ar.place(stats_cpu, "stats") if given else None
        rm = ar.place(torch.zeros(C), "running_mean", inplace=True)
        rv = ar.place(torch.ones(C), "running_var", inplace=True)
        nbt = ar.place(torch.zeros(1, dtype=torch.int64), "num_batches_tracked", inplace=True)
        x_at, y_at = ar.out((B, N, C), "x_at"), ar.out((B, N, C), "y_at")
        mean, invstd = ar.out((C,), "save_mean"), ar.out((C,), "save_invstd")
        ws = None if given else ar.scratch(n, "workspace")
        status = L.dcd_bn_at_forward(st, dx.data_ptr(), dpos.data_ptr(), w.data_ptr(), b.data_ptr(), _ptr(dstats), count, rm.data_ptr(),
                                     rv.data_ptr(), nbt.data_ptr(), 0.1, 1e-5, 1, x_at.data_ptr(), y_at.data_ptr(), mean.data_ptr(),
                                     invstd.data_ptr(), B, C, HW, N, None if given else ar.ptr(ws), 0 if given else n)
        what = "dcd_bn_at_forward, stats %s" % ("given" if given else "NULL")
        assert status == 0, "%s: status %d" % (what, status)
        ar.check(what)
        assert torch.equal(x_at.cpu(), x_at_ref), what
        _close(y_at, ref.detach(), what + " y_at")
        _close(rm, rm_ref, what + " running_mean")
        _close(rv, rv_ref, what + " running_var")
        assert int(nbt.cpu()) == 1
        now = (x_at.cpu(), y_at.cpu(), mean.cpu(), invstd.cpu())
        if kept is not None:
            for a_, b_ in zip(kept, now):
                _close(a_, b_.double(), what + " against the other form")
        kept = now
    x_at_cpu, y_at_cpu, mean_cpu, invstd_cpu = kept

    ar = Arena(cuda)
    dg, dxa, dya = ar.place(gout, "grad_at"), ar.place(x_at_cpu, "x_at"), ar.place(y_at_cpu, "y_at")
    w, mean, invstd = ar.place(w0, "weight"), ar.place(mean_cpu, "save_mean"), ar.place(invstd_cpu, "save_invstd")
    sums, dzk = ar.out((C, 2), "sums", dtype=torch.float64), ar.out((B * N, C), "dzk")
    assert L.dcd_bn_at_backward_sums(st, dg.data_ptr(), dxa.data_ptr(), dya.data_ptr(), w.data_ptr(), mean.data_ptr(), invstd.data_ptr(), 1,
                                     B * N, C, sums.data_ptr(), dzk.data_ptr()) == 0
    ar.check("dcd_bn_at_backward_sums")
    sums_cpu, dzk_cpu = sums.cpu(), dzk.cpu()

    ar = Arena(cuda)
    dx, w, mean, invstd = ar.place(x, "x"), ar.place(w0, "weight"), ar.place(mean_cpu, "save_mean"), ar.place(invstd_cpu, "save_invstd")
    dsums = ar.place(sums_cpu, "sums")
    gx, gw, gb = ar.out(x.shape, "grad_x"), ar.out((C,), "grad_weight"), ar.out((C,), "grad_bias")
    assert L.dcd_bn_backward_apply(st, None, None, dx.data_ptr(), w.data_ptr(), mean.data_ptr(), invstd.data_ptr(), dsums.data_ptr(), count,
                                   gx.data_ptr(), None, gw.data_ptr(), gb.data_ptr(), B, C, HW) == 0
    ar.check("dcd_bn_backward_apply(grad_y = NULL, y = NULL)")
    gx_cpu = gx.cpu()

    ar = Arena(cuda)
    dz, dpos = ar.place(dzk_cpu.view(B, N, C), "dzk"), ar.place(pos, "pos")
    gx = ar.place(gx_cpu, "grad_x", inplace=True)
    assert L.dcd_poi_scatter_add(st, dz.data_ptr(), dpos.data_ptr(), B, C, H, W, N, gx.data_ptr()) == 0
    ar.check("dcd_poi_scatter_add of dzk")
    _close(gx, xd.grad, "grad_x")
    _close(gw, wd.grad, "grad_weight")
    _close(gb, bd.grad, "grad_bias")


# -------------------------------------------------------------------------------------------------------- trunk statistics
@pytest.mark.parametrize("R,K", [(5, 18), (70, 576), (257, 63)])
def test_trunk_statistics(cuda, R, K):
    """dcd_trunk_row_sums, _finalize_forward, _finalize_backward and _grad_wg on fp64 buffers against the closed forms of
    include/dcd_hip.h evaluated in fp64 on the host: fp64 outputs to 1e-12, fp32 outputs to 2e-6 of the output's scale.  Row 1 has a
    raw variance below zero: the clamp gives it variance 0 and no variance gradient."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(R + K)
    count, eps = 960.0, 1e-5
    Wd = torch.randn(R, K, generator=g, dtype=torch.float64) * 0.1
    WG = torch.cat((Wd * (count * (1.0 + torch.rand(R, K, generator=g, dtype=torch.float64))),
                    count * torch.randn(R, 1, generator=g, dtype=torch.float64) * 0.2), 1)
    gamma, beta = torch.rand(R, generator=g) + 0.5, torch.randn(R, generator=g) * 0.3
    gsc, gsh = torch.randn(R, generator=g), torch.randn(R, generator=g)

    ar = Arena(cuda)
    dWG, dWd = ar.place(WG, "WG"), ar.place(Wd, "Wd")
    sums = ar.out((R, 2), "sums", dtype=torch.float64)
    assert L.dcd_trunk_row_sums(st, dWG.data_ptr(), dWd.data_ptr(), R, K, sums.data_ptr()) == 0
    ar.check("dcd_trunk_row_sums")
    ref_sums = torch.stack((WG[:, K], (WG[:, :K] * Wd).sum(1)), 1)
    _close(sums, ref_sums, "row sums", 1e-12)
    zero = Arena(cuda, poison=False)
    zWG, zWd = zero.place(WG, "WG"), zero.place(Wd, "Wd")
    zsums = zero.out((R, 2), "sums", dtype=torch.float64)
    assert L.dcd_trunk_row_sums(st, zWG.data_ptr(), zWd.data_ptr(), R, K, zsums.data_ptr()) == 0
    zero.check("dcd_trunk_row_sums (zero-filled)")
    _same(sums.view(torch.float32), zsums.view(torch.float32), "dcd_trunk_row_sums")

    sums_cpu = sums.cpu()
    sums_cpu[1] = torch.tensor([2.0 * count, 3.0 * count], dtype=torch.float64)         # mean 2, raw variance 3 - 4 < 0
    s = sums_cpu.clone().requires_grad_()
    gm, bt = gamma.double().requires_grad_(), beta.double().requires_grad_()
    mean = s[:, 0] / count
    raw = s[:, 1] / count - mean * mean
    assert (raw[1] < 0) and (raw.detach()[torch.arange(R) != 1] > 0).all()
    var = raw.clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    scale_ref = gm * inv
    shift_ref = bt - mean * scale_ref
    ((scale_ref * gsc.double()).sum() + (shift_ref * gsh.double()).sum()).backward()

    ar = Arena(cuda)
    dsums, dgm, dbt = ar.place(sums_cpu, "sums"), ar.place(gamma, "gamma"), ar.place(beta, "beta")
    scale, shift, stats = ar.out((R,), "scale"), ar.out((R,), "shift"), ar.out((R, 3), "stats", dtype=torch.float64)
    assert L.dcd_trunk_finalize_forward(st, dsums.data_ptr(), dgm.data_ptr(), dbt.data_ptr(), count, eps, R, scale.data_ptr(), shift.data_ptr(),
                                        stats.data_ptr()) == 0
    ar.check("dcd_trunk_finalize_forward")
    _close(stats, torch.stack((mean, var, inv), 1).detach(), "stats", 1e-12)
    _close(scale, scale_ref.detach(), "scale", 2e-6)
    _close(shift, shift_ref.detach(), "shift", 2e-6)
    stats_cpu = stats.cpu()
    assert stats_cpu[1, 1] == 0

    ar = Arena(cuda)
    dgs, dgh, dgm, dstats = ar.place(gsc, "grad_scale"), ar.place(gsh, "grad_shift"), ar.place(gamma, "gamma"), ar.place(stats_cpu, "stats")
    gsums = ar.out((R, 2), "grad_sums", dtype=torch.float64)
    ggm, gbt = ar.out((R,), "grad_gamma"), ar.out((R,), "grad_beta")
    assert L.dcd_trunk_finalize_backward(st, dgs.data_ptr(), dgh.data_ptr(), dgm.data_ptr(), dstats.data_ptr(), count, R, gsums.data_ptr(),
                                         ggm.data_ptr(), gbt.data_ptr()) == 0
    ar.check("dcd_trunk_finalize_backward")
    _close(gsums, s.grad, "grad_sums", 1e-12)
    _close(ggm, gm.grad, "grad_gamma", 2e-6)
    _close(gbt, bt.grad, "grad_beta", 2e-6)
    gsums_cpu = gsums.cpu()
    assert gsums_cpu[1, 1] == 0 and s.grad[1, 1] == 0, "a clamped variance passes no gradient"

    ar = Arena(cuda)
    dgsums, dWd = ar.place(gsums_cpu, "grad_sums"), ar.place(Wd, "Wd")
    gWG = ar.out((R, K + 1), "grad_WG", dtype=torch.float64)
    assert L.dcd_trunk_grad_wg(st, dgsums.data_ptr(), dWd.data_ptr(), R, K, gWG.data_ptr()) == 0
    ar.check("dcd_trunk_grad_wg")
    _close(gWG, torch.cat((gsums_cpu[:, 1:2] * Wd, gsums_cpu[:, 0:1]), 1), "grad_WG", 1e-12)


# ----------------------------------------------------------------------------------------------------------------- DCN glue
@pytest.mark.parametrize("B,taps,HW", [(2, 9, 240), (3, 18, 63)])
def test_dcn_offset_mask_glue(cuda, B, taps, HW):
    """dcd_dcn_offset_mask_split / _merge against slicing + sigmoid and their autograd in fp64 at the bounds of
    test_offset_mask_glue_matches_stock_ops: the offsets exact, the mask within 2e-7, the gradient within 1e-6 of its maximum."""
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(17)
    out = torch.randn(B, 3 * taps, HW, generator=g) * 2
    w1, w2 = torch.randn(B, 2 * taps, HW, generator=g), torch.randn(B, taps, HW, generator=g)
    od = out.double().requires_grad_()
    off_ref, m_ref = od[:, :2 * taps], torch.sigmoid(od[:, 2 * taps:])
    ((off_ref * w1.double()).sum() + (m_ref * w2.double()).sum()).backward()

    ar = Arena(cuda)
    do = ar.place(out, "out")
    off, mask = ar.out((B, 2 * taps, HW), "offset"), ar.out((B, taps, HW), "mask")
    assert L.dcd_dcn_offset_mask_split(st, do.data_ptr(), off.data_ptr(), mask.data_ptr(), B, taps, HW) == 0
    ar.check("dcd_dcn_offset_mask_split")
    assert torch.equal(off.cpu(), out[:, :2 * taps])
    assert (mask.cpu().double() - m_ref.detach()).abs().max().item() <= 2e-7
    mask_cpu = mask.cpu()

    ar = Arena(cuda)
    g1, g2, dm = ar.place(w1, "grad_offset"), ar.place(w2, "grad_mask"), ar.place(mask_cpu, "mask")
    gout = ar.out((B, 3 * taps, HW), "grad_out")
    assert L.dcd_dcn_offset_mask_merge(st, g1.data_ptr(), g2.data_ptr(), dm.data_ptr(), gout.data_ptr(), B, taps, HW) == 0
    ar.check("dcd_dcn_offset_mask_merge")
    assert (gout.cpu().double() - od.grad).abs().max().item() <= 1e-6 * od.grad.abs().max().item()


# ------------------------------------------------------------------------------------------------------------ shifted GEMM
@pytest.mark.parametrize("B,C,H,W,force_split", [(2, 64, 6, 10, 0), (1, 64, 30, 36, 0), (1, 64, 30, 36, 2)])
def test_sgemm_shifted(cuda, B, C, H, W, force_split):
    """Both calls of trunk_moments._ShiftCorr as it makes them: the forward (b_kcontig = 1, split partials summed in fp64) against
    the einsum form of that function's host branch in fp64 at the bar of test_shift_correlations_match_host_float64
    (2e-6 sqrt(n) max(|R| / sqrt(n), 1)), the backward (b_kcontig = 0, the row bias) at 2e-5 of the largest gradient.  `part` and
    `dxp`, padding included, are fully written."""
    from dcd_amd.model.head.trunk_moments import ALL25, HALF
    L, st = _lib_and_stream(cuda)
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, C, H, W, generator=g)
    Hp, Wp = H + 4, (W + 4 + 3) // 4 * 4
    Lp, guard = Hp * Wp, 2 * Wp + 8
    nsplit = force_split or max(1, min(16, Lp // 1024))
    buf = torch.zeros(2 * guard + B * C * Lp)
    xp = buf[guard:guard + B * C * Lp].view(B, C, Hp, Wp)
    xp[:, :, 2:2 + H, 2:2 + W] = x
    xi = xp.double()[:, :, 2:2 + H, 2:2 + W]
    R_ref = torch.stack([torch.einsum('bcyx,bkyx->ck', xi, xp.double()[:, :, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W]) for (dy, dx) in HALF])

    NH = len(HALF)
    off = torch.tensor([c * Lp + dy * Wp + dx for (dy, dx) in HALF for c in range(C)], dtype=torch.int64)
    ar = Arena(cuda)
    dbuf, doff = ar.place(buf, "padded x with its margins"), ar.place(off, "b_off")
    part = ar.out((B * nsplit, C, NH * C), "part")
    A = dbuf.data_ptr() + 4 * guard
    status = L.dcd_sgemm_shifted(st, A, Lp, C * Lp, A, doff.data_ptr(), C * Lp, 1, None, part.data_ptr(), NH * C, nsplit * C * NH * C,
                                 C * NH * C, C, NH * C, Lp, B, nsplit)
    what = "dcd_sgemm_shifted forward %s nsplit %d" % ((B, C, H, W), nsplit)
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    R = part.cpu().double().sum(0).view(C, NH, C).transpose(0, 1)
    n = B * H * W
    err = (R - R_ref).abs().max().item()
    assert err <= 2e-6 * n ** 0.5 * max(R_ref.abs().max().item() / n ** 0.5, 1.0), (what, err)

    if force_split:
        return
    K1 = torch.randn(C, 25 * C, generator=g) / (25 * C) ** 0.5
    bias = torch.randn(C, generator=g)
    off = torch.tensor([c * Lp + dy * Wp + dx for (dy, dx) in ALL25 for c in range(C)], dtype=torch.int64)
    # the header's definition on the whole padded plane: B[z](k, n) = Bbase[z strideB + b_off[k] + n], the margins read as they lie
    cols = torch.arange(Lp)
    ref = torch.stack([K1.double() @ buf.double()[guard + z * C * Lp + off[:, None] + cols[None, :]] for z in range(B)]) + bias.double()[None, :, None]
    ref = ref.view(B, C, Hp, Wp)
    inner = bias.double().view(1, C, 1, 1) + sum(torch.einsum('ck,bkyx->bcyx', K1.double().view(C, 25, C)[:, j, :],
                                                              xp.double()[:, :, 2 + dy:2 + dy + H, 2 + dx:2 + dx + W])
                                                 for j, (dy, dx) in enumerate(ALL25))
    assert (ref[:, :, 2:2 + H, 2:2 + W] - inner).abs().max().item() <= 1e-12 * inner.abs().max().item()     # the host branch's einsum form
    ar = Arena(cuda)
    dbuf, doff = ar.place(buf, "padded x with its margins"), ar.place(off, "b_off")
    dK, dbias = ar.place(K1, "K1"), ar.place(bias, "bias")
    dxp = ar.out((B, C, Hp, Wp), "dxp")
    A = dbuf.data_ptr() + 4 * guard
    status = L.dcd_sgemm_shifted(st, dK.data_ptr(), 25 * C, 0, A, doff.data_ptr(), C * Lp, 0, dbias.data_ptr(), dxp.data_ptr(), Lp, C * Lp, 0,
                                 C, Lp, 25 * C, B, 1)
    what = "dcd_sgemm_shifted backward %s" % ((B, C, H, W),)
    assert status == 0, "%s: status %d" % (what, status)
    ar.check(what)
    _close(dxp, ref, what, 2e-5)
