"""csrc/loss_rows.hip on the GPU: the per-object rows of the loss as one kernel against the same terms evaluated op by op
(Loss_Computation._rows on the HIP ops), values and gradients, and the whole loss through both."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import golden_inputs as gi  # noqa: E402
from test_host_golden import small_cfg, LOSS_KEYS  # noqa: E402
from test_host_rows import _rows_inputs  # noqa: E402

pytestmark = pytest.mark.gpu


def _losses(cuda, monkeypatch, rows, tv_cpu, pois_cpu, cls_cpu, hm_cpu):
    from dcd_amd.model.head.detector_loss import Loss_Computation
    monkeypatch.setenv("DCD_LOSS_ROWS", rows)
    monkeypatch.setenv("DCD_LOSS_GRAPH", "0")
    loss = Loss_Computation(small_cfg(str(cuda)))
    assert loss.fused_rows is (rows == "1")
    tv = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in tv_cpu.items()}
    pois = pois_cpu.to(cuda).requires_grad_()
    cls = cls_cpu.to(cuda).requires_grad_()
    loss_dict, names, packed = loss._core({'cls': cls, 'reg': None, 'reg_pois': pois}, hm_cpu.to(cuda), tv)
    loss_dict.total.backward()
    return loss_dict, dict(zip(names, packed.tolist())), pois.grad, cls.grad


@pytest.mark.parametrize("empty_image,mixed_flags", [(False, False), (True, False), (False, True)])
def test_loss_through_the_row_kernel_equals_the_op_by_op_loss(cuda, monkeypatch, empty_image, mixed_flags):
    monkeypatch.setenv("DCD_LOSS_ROWS", "0")
    host_loss, tv, pois = _rows_inputs(empty_image, mixed_flags)
    preds, targets = gi.loss_inputs()
    hm, _ = host_loss.prepare_targets(targets)
    cls = torch.from_numpy(preds["cls"])
    a = _losses(cuda, monkeypatch, "0", tv, pois, cls, hm)
    b = _losses(cuda, monkeypatch, "1", tv, pois, cls, hm)
    assert list(a[0].keys()) == list(b[0].keys()) == LOSS_KEYS
    for k in LOSS_KEYS:
        ref = float(a[0][k])
        assert abs(float(b[0][k]) - ref) <= 2e-5 * max(abs(ref), 1e-3), (k, float(b[0][k]), ref)
    assert a[1].keys() == b[1].keys()
    for k, ref in a[1].items():
        if ref != ref:                                           # mean over an empty set: NaN in both (as the reference)
            assert b[1][k] != b[1][k], k
            continue
        assert abs(b[1][k] - ref) <= 2e-5 * max(abs(ref), 1e-3), ("log " + k, b[1][k], ref)
    scale = a[2].abs().max().item()
    assert (a[2] - b[2]).abs().max().item() <= 2e-5 * scale
    assert torch.equal(a[3], b[3])                               # the heat-map term does not pass through the rows
    assert (b[2][~tv['reg_mask'].bool()] == 0).all()


@pytest.mark.parametrize("empty_image,mixed_flags", [(False, False), (True, False), (False, True)])
def test_row_kernel_gradient_of_every_column_on_every_head(cuda, monkeypatch, empty_image, mixed_flags):
    """csrc/loss_rows.hip (lane reductions, masking of empty slots, the `finish` pass) column by column: the 25 column sums are
    weighted with a one-hot vector, and the gradient w.r.t. the head outputs is compared with float64 autograd of the op-by-op
    rows on the host (test_host_rows.column_reference), every head at 2e-5 of its OWN maximum in that column.  The gradients of the
    heads differ by four to five orders of magnitude: one scale over the whole tensor (the test above) judges extra_kpts_2d only
    and lets a 50 % error in the 2-D box head pass.  Columns without a gradient path and slots without an object: exactly zero.
    The reference alone (fp32 op-by-op rows against float64) is at most 1.7e-6 on this yardstick; the mixed-flags variant uses the
    noise seed at which the fp32 and float64 top-k pair choices agree (test_host_rows.COLUMN_SEED).
    The worst (column, head) ratio of a run is printed (pytest -s); the host build of the same header measures 1.8e-6, 1.4e-6 and
    1.7e-6 for the three variants."""
    from test_host_rows import check_column_gradients, column_reference
    from dcd_amd.model.head.detector_loss import Loss_Computation
    _, tv_cpu, pois_cpu, names, G64 = column_reference(monkeypatch, empty_image, mixed_flags)    # (the oracle patch is undone here)
    monkeypatch.setenv("DCD_LOSS_ROWS", "1")
    loss = Loss_Computation(small_cfg(str(cuda)))
    assert loss.fused_rows
    tv = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in tv_cpu.items()}
    pois = pois_cpu.to(cuda).requires_grad_()
    got = []
    for c in range(25):
        S, ix = loss._fused_rows({'reg_pois': pois}, tv, 1.0)
        assert {v: k for k, v in ix.items()} == names
        got.append(torch.autograd.grad(S, pois, torch.eye(25, device=cuda)[c])[0])
    worst = check_column_gradients(torch.stack(got).cpu(), G64, names, loss, tv_cpu, "row kernel")
    print("worst (column, head) error / maximum: %.2e" % worst)


def test_row_kernel_rejects_a_channel_map_that_does_not_cover_the_heads(cuda):
    from dcd_amd import _lib
    a = _lib.LossRowsArgs()
    a.B, a.M, a.C, a.K, a.NP, a.num_classes = 1, 4, 415, 73, 1500, 3
    st = _lib.lib().dcd_loss_rows_forward(None, a)
    assert st == 1


def test_batch_without_any_object_trains_on_the_heat_map_only(cuda, monkeypatch):
    """No annotated object in the batch: the per-object losses are exactly 0 with zero gradient w.r.t. the head outputs, the
    heat-map loss and its gradient are unaffected, nothing is non-finite (the op-by-op form divides by the zero depth target of
    slot 0 in a logging column; the kernel never forms that quotient for an empty slot)."""
    monkeypatch.setenv("DCD_LOSS_ROWS", "0")
    host_loss, tv, pois = _rows_inputs()
    tv = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in tv.items()}
    tv['reg_mask'].zero_()
    preds, targets = gi.loss_inputs()
    hm, _ = host_loss.prepare_targets(targets)
    loss_dict, log, gp, gc = _losses(cuda, monkeypatch, "1", tv, pois, torch.from_numpy(preds["cls"]), hm)
    for k in LOSS_KEYS:
        v = float(loss_dict[k])
        assert v == v and abs(v) != float("inf"), k
        if k != "hm_loss":
            assert v == 0.0, (k, v)
    assert float(loss_dict["hm_loss"]) > 0
    assert (gp == 0).all() and torch.isfinite(gc).all() and gc.abs().max().item() > 0
