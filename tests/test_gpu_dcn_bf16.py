"""GPU parity of the one-product bf16 DCNv2 kernels (DCD_PREC_BF16, MODEL.FP16) against the EXACT product of rounded operands.

tests/test_gpu_dcn.py compares these kernels with the unrounded fp32 oracle at 1e-2 of scale: that bar is the operand rounding
itself (~2e-3) and cannot see a wrong k-tail, a swapped half or a tap that is a few per cent off.  Here the reference
(tests/dcn_bf16_reference.py, float64 on the CPU) rounds W, the masked sampled columns and dY to bf16 exactly where the kernels
do -- its docstring lists the places, file and line -- so what is left between kernel and reference is fp32 accumulation, and
the kernels are held at the fp32 bars of test_gpu_dcn.py: 2e-5 of the tensor's max norm forward, 5e-5 for each gradient.

Two kinds of input:
  * `grid_case`: x in 1/16, offsets in 1/4, mask in 1/8.  Every bilinear weight is a multiple of 1/16 and every intermediate of
    a column has fewer than 24 significant bits, so the kernel's fp32 column IS the reference's float64 one whatever the order
    of evaluation, and both round to the same bf16 value.  Each case asserts that premise (`exactly_fp32`) and that at least
    5 % of its columns are not bf16 values (the rounding is exercised).
  * `make_case` (generic fractions): an fp32 column and its float64 twin can round to different bf16 neighbours.  E_flip measures
    that on the reference alone (columns evaluated in fp32 on the CPU against float64) and is added, twice, to the bar of the two
    tensors that contain r(col).

Every test prints its measured ratios before it asserts (pytest -s).
"""
import ctypes

import pytest
import torch

from dcn_bf16_reference import bf16_statistics, dcn_reference, exactly_fp32, tiled_forward_exact_samples
from test_gpu_dcn import BF16X3_TOL, make_case

pytestmark = pytest.mark.gpu

FWD_BAR = 2e-5            # test_gpu_dcn.py::test_forward_matches_oracle
GRAD_BAR = 5e-5           # test_gpu_dcn.py::test_backward_matches_oracle
GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


@pytest.fixture(autouse=True)
def _fresh_launch_policy(cuda):
    """As in test_gpu_dcn.py: the per-layer launch policy is keyed by the weight's device address; every test starts without history."""
    from dcd_amd import _lib
    _lib.lib().dcd_dcn_v2_forget(None)
    yield


def grid_case(B, C, Co, H, W, dg, reach, seed=0):
    """x = integers in [-40, 40] / 16, offsets = integers in [-4 reach, 4 reach] / 4, mask = integers in [1, 7] / 8; w, b, gy as
    make_case (random normal)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-40, 41, (B, C, H, W), generator=g).float() / 16
    n = int(round(4 * reach))
    off = torch.randint(-n, n + 1, (B, 18 * dg, H, W), generator=g).float() / 4
    m = torch.randint(1, 8, (B, 9 * dg, H, W), generator=g).float() / 8
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    b = torch.randn(Co, generator=g)
    gy = torch.randn(B, Co, H, W, generator=g)
    return x, w, b, off, m, gy


def assert_grid_premise(x, off, m, dg=1):
    assert exactly_fp32(x, off, m, dg), "the columns of this case are not exact in fp32: the grid premise does not hold"
    inexact, ties = bf16_statistics(x, off, m, dg)
    assert inexact >= 0.05, "only %.1f %% of the columns are not bf16 values" % (100 * inexact)
    return inexact, ties


def ratio(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return (got - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def hold(what, names, got, ref, bars):
    """Prints every measured ratio, then asserts each against its bar."""
    rs = [ratio(g_, r_) for g_, r_ in zip(got, ref)]
    print("%s: %s" % (what, "  ".join("%s %.2e" % (n, r) for n, r in zip(names, rs))))
    for n, r, bar in zip(names, rs, bars):
        assert r <= bar, "%s %s: %.3e of scale > %.1e" % (what, n, r, bar)
    return rs


def differs_from_f32(what, names, got, f32):
    """The call really ran the one-product form: every result that passes through a weight contraction is more than 1e-4 of scale
    away from the exact-fp32 kernels' (as test_gpu_dcn.py::test_bf16_path_is_the_one_product_kernel)."""
    for n, g_, f_ in zip(names, got, f32):
        if n == "grad_bias":
            continue
        r = ratio(g_, f_)
        assert r > 1e-4, "%s %s: %.3e of scale from the f32 result -- the bf16 form did not run" % (what, n, r)


def run_and_hold(cuda, case, inputs, what, layer_known_near=False):
    """Forward and backward at precision bf16 against the rounded reference at the fp32 bars; then against the f32 kernels."""
    from dcd_amd import _ext
    B, C, Co, H, W = case
    x, w, b, off, m, gy = inputs
    a = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    dev = [t.to(cuda) for t in inputs]
    tiled_forward = W >= 32 and W % 4 == 0 and H >= 8 and C < 256
    exact = tiled_forward_exact_samples(off, B, Co, H, W, layer_known_near) if tiled_forward else None
    if exact is not None and not exact.any():
        exact = None
    y_ref, g_ref = dcn_reference(x, w, b, off, m, gy, fwd_exact=exact)
    y = _ext.dcn_v2_forward(*dev[:5], *a, precision="bf16")
    g = _ext.dcn_v2_backward(*dev, *a, precision="bf16")
    rs = hold(what, ("forward",) + GRADS, (y,) + tuple(g), (y_ref,) + tuple(g_ref), (FWD_BAR,) + (GRAD_BAR,) * 5)
    y32 = _ext.dcn_v2_forward(*dev[:5], *a, precision="f32")
    g32 = _ext.dcn_v2_backward(*dev, *a, precision="f32")
    differs_from_f32(what, ("forward",) + GRADS, (y,) + tuple(g), (y32,) + tuple(g32))
    return rs


# ---- exact-grid inputs, near offsets: one call per route --------------------------------------------------------------------------
TILED_CASES = [
    # B, C, Co, H, W, reach
    (2, 64, 64, 24, 64, 0.75),       # everything from the staged windows
    (1, 12, 70, 17, 36, 1.5),        # ragged: C % 16 != 0, a partial output slice, partial tiles and strips
    (1, 40, 50, 19, 44, 1.5),        # 2.5 channel chunks, 50 outputs, 19 rows
]


@pytest.mark.parametrize("case", TILED_CASES)
def test_tiled_forward_and_one_pass_backward(cuda, case):
    """Kernels: `dcn_fwd_tile_bf16x3<4, 1>` and `dcn_bwd_sweep<DCD_PREC_BF16, 1, true>` (Cout <= 64 per slice: grad_weight inside
    the kernel; 70 outputs: two forward slices and the NOB = 2 backward).  Rounding model: y = r(W) r(col) + b, gW = r(dY) r(col)^T,
    gcol = r(W)^T r(dY), mask applied before r; no sample leaves the windows at these offsets.  Bars: 2e-5 / 5e-5 (fp32 accumulation
    only).  Measured ratios: printed per case (pytest -s)."""
    B, C, Co, H, W, reach = case
    inputs = grid_case(B, C, Co, H, W, 1, reach, seed=C)
    assert_grid_premise(*[inputs[i] for i in (0, 3, 4)])
    run_and_hold(cuda, (B, C, Co, H, W), inputs, "tiled %s" % (case,))


WIDE_CASES = [
    (2, 32, 128, 12, 36, 1.0),       # two output blocks, partial strip
    (1, 16, 256, 9, 32, 1.0),        # four full blocks, one channel chunk
    (1, 48, 200, 10, 40, 1.0),       # four blocks with zero-padded weights
]


@pytest.mark.parametrize("case", WIDE_CASES)
def test_wide_one_pass_backward(cuda, case):
    """Kernels: `dcn_bwd_sweep<DCD_PREC_BF16, 2 | 4, false>` -- dcol over 2 / 4 blocks of 64 outputs, the masked samples leave as fp32
    columns and grad_weight is `sgemm_bf16x3(..., one = true)`, which rounds dY and the columns as it stages them -- and the tiled
    forward over 2 / 4 output slices.  Rounding model: as above (the column buffer in between is fp32, so r(col) is the same value).
    Bars: 2e-5 / 5e-5.  Measured ratios: printed per case (pytest -s)."""
    B, C, Co, H, W, reach = case
    inputs = grid_case(B, C, Co, H, W, 1, reach, seed=Co)
    assert_grid_premise(*[inputs[i] for i in (0, 3, 4)])
    run_and_hold(cuda, (B, C, Co, H, W), inputs, "wide %s" % (case,))


DENSE_CASES = [
    (2, 256, 72, 12, 20, 1.0),       # tile edges of the GEMMs, k-tail of the split-K chunks
    (1, 256, 128, 6, 10, 1.0),
]


@pytest.mark.parametrize("case", DENSE_CASES)
def test_column_buffer_path(cuda, case):
    """Kernels: the column-buffer path (dcn_dense.inc, Cin >= 256): `dcn_dense_im2col` (fp32 columns, mask inside) and the three
    products forward / T = W^T dY / grad_weight on `sgemm_bf16x3(..., one = true)`.  Rounding model: as above, every GEMM operand
    rounded when staged; T stays fp32 for col2im and the coordinate gradients.  Bars: 2e-5 / 5e-5.  Measured ratios: printed per case (pytest -s)."""
    B, C, Co, H, W, reach = case
    inputs = grid_case(B, C, Co, H, W, 1, reach, seed=Co)
    assert_grid_premise(*[inputs[i] for i in (0, 3, 4)])
    run_and_hold(cuda, (B, C, Co, H, W), inputs, "column buffer %s" % (case,))


def test_quarter_collisions(cuda):
    """Kernel: `dcn_bwd_sweep<DCD_PREC_BF16, 1, true>`, the fix-up loop: neighbouring pixel groups pushed 1.5 px towards each other
    (still on the grid, still nearer than 3 px) make the four quarters of a pixel step meet in one cell, so those steps are redone
    after the taps (`full_dcol`, `add_dw`: the same roundings).  Rounding model and bars as above.  Measured ratios: printed per case (pytest -s)."""
    B, C, Co, H, W = 1, 128, 64, 16, 48
    inputs = grid_case(B, C, Co, H, W, 1, 1.0, seed=5)
    off = inputs[3]
    off[..., 1::4] += 1.5
    off[..., 3::4] -= 1.5
    assert_grid_premise(*[inputs[i] for i in (0, 3, 4)])
    run_and_hold(cuda, (B, C, Co, H, W), inputs, "quarter collisions")


# ---- exact-grid inputs, far samples --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(1, 32, 64, 16, 32), (2, 64, 64, 16, 64)])
def test_far_samples(cuda, case):
    """Offsets up to 6 px: more than half of the coordinates are displaced by 3 px or more.  One weight tensor (the launch policy's
    key) through the states of the policy; which kernels run, and therefore which rounding model applies, depends on the state:

    (a) unknown layer.  The forward's offset count sends every tile to the rescue pass `dcn_fwd9_f32<., true>`, and the backward --
        hand-over armed, far samples dominating -- leaves `dcn_bwd_sweep` at once for the generic `dcn_bwd_input_f32` /
        `dcn_bwd_data_f32` / `dcn_bwd_weight_f32`.  These are the exact fp32 kernels: precision bf16 PERMITS the one-product form,
        a call handed to kernels without it is computed in fp32.  Reference: r = identity, at the fp32 bars.  (This call cannot
        differ from the f32 result; (c) is where the case shows that the bf16 form ran.)
    (b) a near call (offsets within 0.75 px) on the same weight: the layer's report says "near".
    (c) the far offsets again.  Forward `dcn_fwd_tile_bf16x3<4, 1>` without far count and rescue launch: samples inside the staged
        window rounded, samples outside it gathered per lane and multiplied in exact fp32 with unrounded weights -- reference
        switch `fwd_exact` = `tiled_forward_exact_samples(..., layer_known_near=True)`.  Backward `dcn_bwd_sweep<DCD_PREC_BF16, 1,
        true>` alone (no hand-over): far samples one by one from global memory through the same `full_dcol` / `add_dw`, rounded
        like near ones -- reference fully rounded.  Fp32 bars; more than 1e-4 away from the f32 kernels.
    Measured ratios: printed per case (pytest -s)."""
    from dcd_amd import _ext
    B, C, Co, H, W = case
    a = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    x, w, b, off, m, gy = grid_case(B, C, Co, H, W, 1, 6.0, seed=C + W)
    off_near = grid_case(B, C, Co, H, W, 1, 0.75, seed=C + W + 1)[3]
    assert_grid_premise(x, off, m)
    assert (off.abs() >= 3).float().mean().item() > 0.5
    dev = [t.to(cuda) for t in (x, w, b, off, m, gy)]
    names = ("forward",) + GRADS
    bars = (FWD_BAR,) + (GRAD_BAR,) * 5
    # (a)
    y_ref, g_ref = dcn_reference(x, w, b, off, m, gy, rounded=False)
    y = _ext.dcn_v2_forward(*dev[:5], *a, precision="bf16")
    g = _ext.dcn_v2_backward(*dev, *a, precision="bf16")
    hold("far %s (a) unknown layer: fp32 kernels" % (case,), names, (y,) + tuple(g), (y_ref,) + tuple(g_ref), bars)
    # (b)
    torch.cuda.synchronize()
    _ext.dcn_v2_backward(dev[0], dev[1], dev[2], off_near.to(cuda), dev[4], dev[5], *a, precision="bf16")
    torch.cuda.synchronize()                                   # the call has reported: the next ones read "near"
    # (c)
    exact = tiled_forward_exact_samples(off, B, Co, H, W, layer_known_near=True)
    assert 0.05 < exact.float().mean().item() < 0.95           # both kinds of sample in numbers (measured on the CPU: 8 % / 10 %)
    y_ref, g_ref = dcn_reference(x, w, b, off, m, gy, fwd_exact=exact)
    y = _ext.dcn_v2_forward(*dev[:5], *a, precision="bf16")
    g = _ext.dcn_v2_backward(*dev, *a, precision="bf16")
    hold("far %s (c) known as near: tiled forward + per-lane far samples, one-pass backward alone" % (case,), names, (y,) + tuple(g),
         (y_ref,) + tuple(g_ref), bars)
    y32 = _ext.dcn_v2_forward(*dev[:5], *a, precision="f32")
    g32 = _ext.dcn_v2_backward(*dev, *a, precision="f32")
    differs_from_f32("far %s (c)" % (case,), names, (y,) + tuple(g), (y32,) + tuple(g32))


def test_far_dominated_wide_layer(cuda):
    """A layer both the one-pass kernel and the column-buffer path take (Cin, Cout >= 128), four backward calls on one weight -- near,
    far, far, near -- each against the rounded reference (the sequencing of
    test_gpu_dcn.py::test_far_dominated_wide_layers_take_the_column_buffer_path):
      1. near, unknown layer: `dcn_bwd_sweep<DCD_PREC_BF16, 2, false>` + the one-product grad_weight GEMM; reports 0 far coordinates;
      2. far, the report says near: the same kernels alone, far samples one by one (rounded like near ones); reports the far count;
      3. far, the report is above the limit: column-buffer backward (`sgemm_bf16x3(..., one = true)` three times); reports again;
      4. near, still routed by the last report: column buffer; reports 0.
    Rounding model: gW = r(dY) r(col)^T, gcol = r(W)^T r(dY) on both routes.  Bars: 5e-5.  Measured ratios: printed per case (pytest -s)."""
    from dcd_amd import _ext, _lib
    L = _lib.lib()
    B, C, Co, H, W = 1, 128, 128, 12, 36
    a = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    x, w, b, off_near, m, gy = grid_case(B, C, Co, H, W, 1, 0.5, seed=31)
    off_far = grid_case(B, C, Co, H, W, 1, 6.0, seed=131)[3]
    for o in (off_near, off_far):
        assert_grid_premise(x, o, m)
    dev = [t.to(cuda) for t in (x, w, b, off_near, m, gy)]
    ref = {id(o): dcn_reference(x, w, b, o, m, gy)[1] for o in (off_near, off_far)}
    limit = B * 18 * H * W // 8                                  # far_count_limit: wide outputs, fewer than four images

    def far_reported():
        torch.cuda.synchronize()
        far = ctypes.c_uint(0)
        assert L.dcd_dcn_v2_policy_state(dev[1].data_ptr(), ctypes.byref(far)) == 2
        return far.value

    got = {}
    try:
        L.dcd_dcn_v2_forget(dev[1].data_ptr())
        for call, o in enumerate((off_near, off_far, off_far, off_near), 1):
            g = _ext.dcn_v2_backward(dev[0], dev[1], dev[2], o.to(cuda), dev[4], dev[5], *a, precision="bf16")
            hold("far-dominated wide layer, call %d" % call, GRADS, g, ref[id(o)], (GRAD_BAR,) * 5)
            got[call] = g
            n = far_reported()
            assert (n > limit) == (o is off_far), (call, n, limit)
        L.dcd_dcn_v2_forget(dev[1].data_ptr())
        for o, calls in ((off_near, (1, 4)), (off_far, (2, 3))):
            g32 = _ext.dcn_v2_backward(dev[0], dev[1], dev[2], o.to(cuda), dev[4], dev[5], *a, precision="f32")
            torch.cuda.synchronize()
            for call in calls:
                differs_from_f32("far-dominated wide layer, call %d" % call, GRADS, got[call], g32)
    finally:
        L.dcd_dcn_v2_forget(dev[1].data_ptr())


@pytest.mark.parametrize("case", [(2, 5, 4, 7, 9, 1), (2, 64, 32, 9, 11, 2)])
def test_generic_kernels_run_the_split_form(cuda, case):
    """Small maps and deformable_groups > 1 have no one-product kernel: under DCD_PREC_BF16 the forward is the exact fp32 kernel
    (`dcn_fwd9_f32`) and the backward runs the generic three-pass kernels, of which only the tiled grad_weight kernel has a matrix
    form other than fp32 -- the SPLIT one (dcn_v2.hip, dcd_dcn_v2_backward: "the generic kernels: DCD_PREC_BF16 runs their split
    form"; maps narrower than 32 columns, as here, do not reach it either).  Nothing is rounded to one bf16.  Reference:
    r = identity, held at the split form's BF16X3_TOL = 1e-4 -- the documented behaviour as a tested one.  (No distance from the
    f32 result is asked: the split form is within 3e-5 of it by construction.)  Measured ratios: printed per case (pytest -s)."""
    from dcd_amd import _ext
    B, C, Co, H, W, dg = case
    inputs = grid_case(B, C, Co, H, W, dg, 1.0, seed=C)
    x, w, b, off, m, gy = inputs
    assert_grid_premise(x, off, m, dg)
    a = (3, 3, 1, 1, 1, 1, 1, 1, dg)
    dev = [t.to(cuda) for t in inputs]
    y_ref, g_ref = dcn_reference(x, w, b, off, m, gy, dg=dg, rounded=False)
    y = _ext.dcn_v2_forward(*dev[:5], *a, precision="bf16")
    g = _ext.dcn_v2_backward(*dev, *a, precision="bf16")
    hold("generic %s" % (case,), ("forward",) + GRADS, (y,) + tuple(g), (y_ref,) + tuple(g_ref), (BF16X3_TOL,) * 6)


# ---- generic inputs: the reference's own rounding ambiguity as the yardstick ----------------------------------------------------------
GENERIC_INPUT_CASES = [c[:5] for c in TILED_CASES + WIDE_CASES + DENSE_CASES]


@pytest.mark.parametrize("case", GENERIC_INPUT_CASES)
def test_generic_inputs(cuda, case):
    """The routes of the first four tests on make_case inputs (random normal x, offsets of 1 px, sigmoid masks): generic fractional
    bilinear weights, which the grid never produces.  The kernel's fp32 column and the reference's float64 one can now round to
    different bf16 neighbours; E_flip = |ref(columns evaluated in fp32) - ref(columns in float64)| / scale measures that on the CPU
    alone, per tensor.  Bars: forward 2e-5 + 2 E_flip and grad_weight 5e-5 + 2 E_flip (the only tensors that contain r(col); twice,
    because the kernel's fp32 order of evaluation is a third one); the other gradients the plain 5e-5.  E_flip must be above 0 and
    below 1e-3, else the inputs have to change: these are conditions, not measurements.
    At 1 px a few samples (|offset| >= 3 px, 0.3 % of the coordinates) leave the forward's staged windows: the tiled kernel takes
    them per lane in exact fp32, or hands a tile with many of them to the fp32 rescue pass -- `tiled_forward_exact_samples` marks
    them for the reference (dcn_bf16_reference.py, `fwd_exact`); the one-pass backward rounds them like any other sample.
    Measured ratios: printed per case (pytest -s)."""
    from dcd_amd import _ext
    B, C, Co, H, W = case
    x, w, b, off, m, gy = make_case(B, C, Co, H, W, off_scale=1.0, seed=C + Co)
    a = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    dev = [t.to(cuda) for t in (x, w, b, off, m, gy)]
    exact = tiled_forward_exact_samples(off, B, Co, H, W) if (W >= 32 and C < 256) else None
    if exact is not None and not exact.any():
        exact = None
    y64, g64 = dcn_reference(x, w, b, off, m, gy, fwd_exact=exact)
    y32, g32 = dcn_reference(x, w, b, off, m, gy, fwd_exact=exact, col_dtype=torch.float32)
    flip_y, flip_w = ratio(y32, y64), ratio(g32[3], g64[3])
    for what, e in (("forward", flip_y), ("grad_weight", flip_w)):
        assert 0 < e < 1e-3, "E_flip of %s is %.3e: these inputs do not serve" % (what, e)
    y = _ext.dcn_v2_forward(*dev[:5], *a, precision="bf16")
    g = _ext.dcn_v2_backward(*dev, *a, precision="bf16")
    bars = (FWD_BAR + 2 * flip_y, GRAD_BAR, GRAD_BAR, GRAD_BAR, GRAD_BAR + 2 * flip_w, GRAD_BAR)
    hold("generic inputs %s (E_flip forward %.2e, grad_weight %.2e)" % (case, flip_y, flip_w), ("forward",) + GRADS,
         (y,) + tuple(g), (y64,) + tuple(g64), bars)
    yf = _ext.dcn_v2_forward(*dev[:5], *a, precision="f32")
    gf = _ext.dcn_v2_backward(*dev, *a, precision="f32")
    differs_from_f32("generic inputs %s" % (case,), ("forward",) + GRADS, (y,) + tuple(g), (yf,) + tuple(gf))


# ---- the module under the precision scope ----------------------------------------------------------------------------------------
class _Spy:
    """dcd_amd._ext with the arguments and results of the two DCN calls recorded."""

    def __init__(self, ext):
        self._ext = ext
        self.fwd, self.bwd = [], []

    def __getattr__(self, name):
        return getattr(self._ext, name)

    def dcn_v2_forward(self, *args, **kw):
        out = self._ext.dcn_v2_forward(*args, **kw)
        self.fwd.append((args, kw, out.clone()))
        return out

    def dcn_v2_backward(self, *args, **kw):
        out = self._ext.dcn_v2_backward(*args, **kw)
        self.bwd.append((args, kw, tuple(t.clone() for t in out)))      # the one-node backward adds into grad_input afterwards
        return out


@pytest.mark.parametrize("one_node", [True, False])
@pytest.mark.parametrize("B,C,Co,H,W", [(2, 64, 64, 24, 80), (2, 64, 72, 14, 44)])
def test_dcn_module_under_the_precision_scope(cuda, monkeypatch, B, C, Co, H, W, one_node):
    """`DCN(C, Co, 3, 1, 1)` (offset convolution initialised as in test_dcn_module_as_one_node_equals_three_nodes), as one autograd
    node and as three, forward inside `_ext.precision_scope("bf16")`, backward outside it:
      * the deformable part IS `_ext.dcn_v2_forward / _backward(..., precision="bf16")` on the offsets and masks the module
        computed -- equal to summation order (2e-6, the bar of the one-node test) -- and was called with that precision both ways;
      * grad_weight is more than 1e-4 of scale away from the module's fp32 run: the backward kept the forward's precision;
      * the precision is "f32" again after the scope."""
    from dcd_amd import _ext
    from dcd_amd.model.backbone.DCNv2 import dcn_v2
    torch.manual_seed(C + H)
    mod = dcn_v2.DCN(C, Co, (3, 3), 1, 1).to(cuda)
    mod.conv_offset_mask.weight.data.normal_(0, 0.02)
    mod.conv_offset_mask.bias.data.normal_(0, 0.3)
    x = torch.randn(B, C, H, W, device=cuda)
    gy = torch.randn(B, Co, H, W, device=cuda)
    monkeypatch.setattr(dcn_v2, "_ONE_NODE", one_node)
    spy = _Spy(_ext)
    monkeypatch.setattr(dcn_v2, "_backend", spy)

    def run(prec):
        xi = x.clone().requires_grad_()
        mod.zero_grad()
        if prec is None:
            y = mod(xi)
        else:
            with _ext.precision_scope(prec):
                y = mod(xi)
        assert (type(y.grad_fn).__name__ == "_DCNWithOffsetsBackward") == one_node
        assert _ext.get_precision() == "f32"
        y.backward(gy)
        return y.detach(), mod.weight.grad.clone()

    y16, gw16 = run("bf16")
    assert len(spy.fwd) == 1 and len(spy.bwd) == 1
    (fa, fkw, fout), (ba, bkw, bout) = spy.fwd[0], spy.bwd[0]
    assert fkw == {"precision": "bf16"} and bkw == {"precision": "bf16"}
    geo = (3, 3, 1, 1, 1, 1, 1, 1, 1)
    xin, wt, bs, off, msk = (t.detach().contiguous() for t in fa[:5])
    assert off.shape == (B, 18, H, W) and msk.shape == (B, 9, H, W)
    direct_y = _ext.dcn_v2_forward(xin, wt, bs, off, msk, *geo, precision="bf16")
    direct_g = _ext.dcn_v2_backward(xin, wt, bs, off, msk, gy, *geo, precision="bf16")
    hold("module (one node: %s) %s deformable part vs direct bf16 calls" % (one_node, (B, C, Co, H, W)), ("forward",) + GRADS,
         (fout,) + tuple(bout), (direct_y,) + tuple(direct_g), (2e-6,) * 6)
    assert torch.equal(y16, fout)
    assert ratio(gw16, bout[3]) <= 2e-6
    y32, gw32 = run(None)
    assert not spy.fwd[1][1] and not spy.bwd[1][1]               # exact fp32 passes no precision argument
    r = ratio(gw16, gw32)
    print("module grad_weight, bf16 scope vs fp32 run: %.2e of scale" % r)
    assert r > 1e-4, r
    assert _ext.get_precision() == "f32"
