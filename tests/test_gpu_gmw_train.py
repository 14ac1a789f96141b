"""Training GMW on the device (dcd_amd/gmw/train.py, dcd_amd/gmw/data.py): the loop's losses against the parent's step, batches
out of the resident tables, no host synchronisation inside an iteration, and the non-finite guard."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_gmw import inputs  # noqa: E402  (seeded GMW batch; pure numpy)

pytestmark = pytest.mark.gpu
KEYS = ("kpts_2d", "kpts_3d", "pred_rot", "gt_location")


def records(n, seed=7):
    return dict(zip(KEYS, inputs(seed=seed, B=n)))


def fresh_model(device, **kw):
    from dcd_amd.gmw import GMW
    torch.manual_seed(0)
    return GMW(**kw).train().to(device)


def hand_rolled(device, data, compute_z, order_of):
    """The parent's step in `epoch_order`'s batches: epoch 1 at (1, 0), epoch 2 at (0.1, 1) -> [(loss, cls, reg), ...]."""
    from dcd_amd.gmw import gmw_train_step
    model = fresh_model(device)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-5)
    out = []
    for epoch, (cw, rw) in ((1, (1.0, 0.0)), (2, (0.1, 1.0))):
        idx = order_of(epoch)
        batch = [torch.from_numpy(data[k][idx]).to(device) for k in KEYS]
        loss, cls, reg, _ = gmw_train_step(model, opt, *batch, cw, rw, compute_z=compute_z)
        out.append((float(loss), float(cls), float(reg)))
    return out


def test_trajectory_against_the_parents_step(cuda, tmp_path):
    """Yardstick D_k: the parent's `gmw_train_step` loop on the GPU against the same loop on the CPU.  `train_gmw` differs from the
    GPU loop by the plan's rounding and the optimiser kernel only, so its values lie within 2 D_k of the CPU loop's, floored at the
    tolerances tests/test_gmw.py holds one step to (2e-5 relative for loss and reg_loss, 2e-6 absolute for cls_loss)."""
    from dcd_amd import ops
    from dcd_amd.gmw.data import epoch_order
    from dcd_amd.gmw.train import train_gmw
    from oracle import torch_ops
    data = records(3)

    def order_of(epoch):
        return epoch_order(3, epoch, 5)[:2]

    on_cpu = hand_rolled(torch.device("cpu"), data, torch_ops.compute_z, order_of)
    on_gpu = hand_rolled(cuda, data, ops.compute_z, order_of)
    out = train_gmw(fresh_model(cuda), data, str(tmp_path), epochs=2, batch_size=2, reg_loss_start_epoch=2, print_freq=10, seed=5)
    assert [h[:2] for h in out["history"]] == [(1, 0), (2, 0)]
    floors = (lambda v: 2e-5 * abs(v), lambda v: 2e-6, lambda v: 2e-5 * abs(v))
    ok = True
    for k, h in enumerate(out["history"]):
        for name, got, ref, dev, floor in zip(("loss", "cls_loss", "reg_loss"), h[2:5], on_cpu[k], on_gpu[k], floors):
            d = abs(dev - ref)
            bar = max(2 * d, floor(ref))
            print("step %d %s: train_gmw %.9g, CPU loop %.9g, GPU loop %.9g, D %.3e, |train_gmw - CPU| %.3e, bar %.3e"
                  % (k, name, got, ref, dev, d, abs(got - ref), bar))
            ok = ok and abs(got - ref) <= bar
    assert ok
    assert os.path.exists(os.path.join(str(tmp_path), "checkpoint_epoch_2.pth.tar"))


@pytest.mark.parametrize("index", [[3], [4, 0, 2, 1, 3], [2, 2, 0, 2]])
def test_resident_batches_are_the_hosts_rows(cuda, index):
    from dcd_amd.gmw.data import ResidentRecords
    data = records(5)
    rec = ResidentRecords(data, cuda)
    for _ in range(3):                                   # both pinned slots, and a slot's second use
        got = rec.batch(index)
        for k, t in zip(KEYS, got):
            want = torch.from_numpy(data[k]).index_select(0, torch.tensor(index))
            assert t.dtype == torch.float32 and t.shape == want.shape
            assert torch.equal(t.cpu().view(torch.int32), want.view(torch.int32)), k
    with pytest.raises(IndexError):
        rec.batch([5])


def _setup(cuda, n=4):
    from dcd_amd.gmw.data import ResidentRecords
    from dcd_amd.gmw.train import build_gmw_optimizer
    model = fresh_model(cuda, device_sinkhorn=True)
    return model, build_gmw_optimizer(model, 1e-4, 1e-5), ResidentRecords(records(n), cuda)


def test_an_iteration_does_not_synchronise(cuda):
    from dcd_amd.gmw.train import _Ring, train_iteration
    model, opt, rec = _setup(cuda)
    ring = _Ring(4, cuda)
    for idx in ([0, 1], [2, 3]):                          # warm-up: graph capture, both pinned slots, optimiser state
        ring.append(train_iteration(model, opt, rec.batch(idx), 0.1, 1.0), 2, 0.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        caught = False
        try:
            torch.ones(1, device=cuda).item()
        except RuntimeError:
            caught = True
        if caught:
            ring.append(train_iteration(model, opt, rec.batch([1, 2]), 0.1, 1.0), 2, 0.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not caught:
        pytest.skip("this build's sync debug mode does not flag .item()")
    rows = ring.flush()
    assert len(rows) == 3 and all(np.isfinite(r[0]).all() for r in rows)


def test_a_non_finite_batch_changes_nothing(cuda):
    from dcd_amd.gmw.train import train_iteration
    model, opt, rec = _setup(cuda)
    assert opt.own_kernels_ok()

    def snapshot():
        state = [opt.state[p] for p in opt.param_groups[0]["params"]]
        return ([p.detach().clone() for p in model.parameters()], [s["exp_avg"].clone() for s in state],
                [s["exp_avg_sq"].clone() for s in state], [float(s["step"]) for s in state])

    first = train_iteration(model, opt, rec.batch([0, 1]), 0.1, 1.0)
    assert torch.isfinite(first).all()
    before = snapshot()
    assert set(before[3]) == {1.0}
    bad = list(rec.batch([2, 3]))
    bad[3] = bad[3].clone()
    bad[3][0, 2] = float("nan")
    values = train_iteration(model, opt, tuple(bad), 0.1, 1.0)
    assert torch.isnan(values[0])
    after = snapshot()
    for a, b in zip(before[:3], after[:3]):
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))
    assert after[3] == before[3]
    values = train_iteration(model, opt, rec.batch([2, 3]), 0.1, 1.0)
    assert torch.isfinite(values).all()
    trained = snapshot()
    assert set(trained[3]) == {2.0}
    assert any(not torch.equal(x, y) for x, y in zip(after[0], trained[0]))
    assert all(torch.isfinite(x).all() for x in trained[0])
