"""Training GMW from generated records, the host side (dcd_amd/gmw/data.py, dcd_amd/gmw/train.py): the loader against the
reference's own `load_data` (tests/golden/gmw_train.npz, made by tests/golden/make_golden_gmw_train.py), the sampler rule against
torch's DistributedSampler, and `train_gmw` on the CPU against a loop written out here from the parent's `gmw_train_step`."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from make_golden_gmw_train import COUNTS, records  # noqa: E402  (seeded JSON builder shared with the generator; pure numpy)

K = 10                     # keypoints of the small model: 45 edges
N, B = 5, 2


def compute_z_stand_in(kpts_2d, kpts_3d, pred_rot, num_k=20):
    """A torch stand-in for the edge-depth solver with its interface: a depth per keypoint pair and the `num_k` pairs that are
    furthest apart vertically.  Differentiable nowhere it matters: the step detaches nothing from it."""
    n = kpts_2d.shape[1]
    iu = torch.triu_indices(n, n, offset=1)
    cos, sin = torch.cos(pred_rot), torch.sin(pred_rot)
    h = kpts_3d[:, :, 1] + kpts_2d[:, :, 1] * (kpts_3d[:, :, 0] * sin - kpts_3d[:, :, 2] * cos)
    dv = kpts_2d[:, iu[0], 1] - kpts_2d[:, iu[1], 1]
    z = ((h[:, iu[0]] - h[:, iu[1]]).abs() / dv.abs().clamp_min(1e-10)).clamp(0.1, 80.0)
    return z, dv.abs().topk(num_k, dim=-1)[1]


def small_records(seed=1):
    g = torch.Generator().manual_seed(seed)
    return {"kpts_2d": (torch.rand(N, K, 2, generator=g) - 0.5).numpy(),
            "kpts_3d": ((torch.rand(N, K, 3, generator=g) - 0.5) * 3).numpy(),
            "pred_rot": (torch.rand(N, 1, generator=g) * 6 - 3).numpy(),
            "gt_location": (torch.rand(N, 3, generator=g) * 30 + 5).numpy()}


def small_model(seed=0):
    from dcd_amd.gmw import GMW
    torch.manual_seed(seed)
    return GMW(num_kpts=K).train()


def test_loader_equals_the_reference_load_data(tmp_path):
    from dcd_amd.gmw.data import load_train_data
    fx = np.load(os.path.join(HERE, "golden", "gmw_train.npz"))
    data = records()
    assert [len(x) for x in data["kpts_2d"]] == list(COUNTS) == [2, 0, 3]
    path = tmp_path / "gen_data_train.json"
    path.write_text(json.dumps(data))
    for source in (data, str(path)):
        got = load_train_data(source)
        assert sorted(got) == ["gt_location", "kpts_2d", "kpts_3d", "pred_rot"]
        for k, shape in (("kpts_2d", (5, 73, 2)), ("kpts_3d", (5, 73, 3)), ("pred_rot", (5, 1)), ("gt_location", (5, 3))):
            assert got[k].dtype == np.float32 and got[k].shape == shape, k
            assert np.array_equal(got[k], fx[k]), k
    # the reference's order: iteration after iteration, object after object
    assert np.array_equal(load_train_data(data)["gt_location"][2], np.float32(data["gt_location"][2][0]))


def test_loader_takes_iterations_without_objects_only():
    from dcd_amd.gmw.data import load_train_data
    got = load_train_data({"kpts_2d": [[], []], "kpts_3d": [[], []], "pred_rot": [[], []], "gt_location": [[], []]})
    assert got["kpts_2d"].shape == (0, 73, 2) and got["gt_location"].shape == (0, 3)


@pytest.mark.parametrize("world_size", [1, 3])
@pytest.mark.parametrize("epoch", [0, 1])
def test_epoch_order_is_the_distributed_sampler(world_size, epoch):
    from torch.utils.data import DistributedSampler
    from dcd_amd.gmw.data import epoch_order
    for seed in (0, 7):
        for rank in range(world_size):
            sampler = DistributedSampler(range(10), num_replicas=world_size, rank=rank, shuffle=True, seed=seed)
            sampler.set_epoch(epoch)
            assert epoch_order(10, epoch, seed, rank, world_size) == list(sampler)


def test_resident_records_on_the_host_are_an_index_select():
    from dcd_amd.gmw.data import KEYS, ResidentRecords
    data = small_records()
    rec = ResidentRecords(data, "cpu")
    got = rec.batch([4, 0, 4])
    for k, t in zip(KEYS, got):
        assert torch.equal(t, torch.from_numpy(data[k])[[4, 0, 4]])
    with pytest.raises(IndexError):
        rec.batch([5])


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """`train_gmw` for two epochs on the CPU, the weight switch at the second: (result, model, log directory)."""
    from dcd_amd.gmw.train import train_gmw
    log_dir = str(tmp_path_factory.mktemp("gmw_straight"))
    model = small_model()
    out = train_gmw(model, small_records(), log_dir, epochs=2, batch_size=B, reg_loss_start_epoch=2, print_freq=1, seed=3,
                    compute_z=compute_z_stand_in)
    return out, model, log_dir


def test_train_gmw_is_the_parents_step_in_epoch_order(straight):
    from dcd_amd.gmw import gmw_train_step
    from dcd_amd.gmw.data import epoch_order
    from dcd_amd.gmw.train import build_gmw_optimizer
    out, trained, _ = straight
    data = {k: torch.from_numpy(v) for k, v in small_records().items()}
    model = small_model()
    opt = build_gmw_optimizer(model, 1e-4, 1e-5)
    assert type(opt) is type(out["optimizer"])
    logged = []
    for epoch, (cls_w, reg_w) in ((1, (1.0, 0.0)), (2, (0.1, 1.0))):
        order = epoch_order(N, epoch, 3)
        for k in range(N // B):
            idx = order[k * B:(k + 1) * B]
            k2, k3, rot, loc = (data[key][idx] for key in ("kpts_2d", "kpts_3d", "pred_rot", "gt_location"))
            loss, cls, reg, z = gmw_train_step(model, opt, k2, k3, rot, loc, cls_w, reg_w, compute_z=compute_z_stand_in)
            mae = ((z - loc[:, 2]).abs() / loc[:, 2]).mean()
            logged.append((epoch, k, float(loss), float(cls), float(reg), float(mae)))
    assert len(out["history"]) == len(logged) == 4
    assert out["history"] == logged                                      # every logged value, bit for bit
    assert logged[0][2] == logged[0][3] and logged[2][2] != logged[2][3]      # (1, 0), then (0.1, 1)
    for (name, p), q in zip(trained.named_parameters(), model.parameters()):
        assert torch.equal(p, q), name
    assert out["epoch"] == 2
    assert [float(g["lr"]) for g in out["optimizer"].param_groups] == [1e-4]      # the scheduler is never stepped


def test_resume_continues_the_stream(straight, tmp_path):
    from dcd_amd.gmw.train import train_gmw
    _, trained, _ = straight
    model = small_model()
    kw = dict(batch_size=B, reg_loss_start_epoch=2, print_freq=1, seed=3, compute_z=compute_z_stand_in)
    train_gmw(model, small_records(), str(tmp_path), epochs=1, **kw)
    again = small_model(seed=99)                                          # everything must come from the file
    out = train_gmw(again, small_records(), str(tmp_path), epochs=2, resume=str(tmp_path / "checkpoint_epoch_1.pth.tar"), **kw)
    assert [h[0] for h in out["history"]] == [2, 2]
    for (name, p), q in zip(trained.named_parameters(), again.parameters()):
        assert torch.equal(p, q), name


def test_checkpoint_layout(straight):
    _, trained, log_dir = straight
    assert sorted(f for f in os.listdir(log_dir) if f.endswith(".tar")) == ["checkpoint_epoch_2.pth.tar"]
    ck = torch.load(os.path.join(log_dir, "checkpoint_epoch_2.pth.tar"), map_location="cpu", weights_only=False)
    assert sorted(ck) == ["best_mAP", "epoch", "optimizer", "scheduler", "state_dict"]
    assert ck["epoch"] == 2 and ck["best_mAP"] == 0.0
    fx = np.load(os.path.join(HERE, "golden", "gmw.npz"))
    assert list(ck["state_dict"]) == list(fx["param_names"])              # loads into the reference's GMW
    for name, p in trained.named_parameters():
        assert torch.equal(ck["state_dict"][name], p.detach())
    # what the reference's plain AdamW adopts verbatim: floats and host tensors only, one group in parameter order
    (group,) = ck["optimizer"]["param_groups"]
    assert group["params"] == list(range(len(fx["param_names"]))) and isinstance(group["lr"], float) and group["lr"] == 1e-4
    assert not group["capturable"] and not group["fused"]
    for st in ck["optimizer"]["state"].values():
        assert all(not v.is_cuda for v in st.values() if torch.is_tensor(v)) and float(st["step"]) == 4.0
    ref_opt = torch.optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in trained.parameters()], lr=1.0)
    ref_opt.load_state_dict(ck["optimizer"])
    assert ref_opt.param_groups[0]["lr"] == 1e-4 and ref_opt.param_groups[0]["betas"] == (0.9, 0.999)
    assert ck["scheduler"]["T_max"] == 2 and ck["scheduler"]["last_epoch"] == 0


def test_log_lines_have_the_references_format(straight):
    """`ProgressMeter.display` (GMW/main.py:597-601) writes ''.join(entries): prefix + [batch/total], then every meter as
    'name val (avg)' with %6.4f, no separator in the file."""
    _, _, log_dir = straight
    lines = open(os.path.join(log_dir, "log.txt")).read().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    num = r" *-?\d+\.\d{4}"
    meter = lambda name: re.escape(name) + " (" + num + r") \((" + num + r")\)"      # noqa: E731
    pattern = re.compile(r"^Epoch: \[(\d)\]\[(\d)/2\]" + "".join(meter(n) for n in ("Time", "Loss", "cls Loss", "reg Loss", "Depth_MAE")) + "$")
    out, _, _ = straight
    seen = []
    for line, h in zip(lines[:4], out["history"]):
        m = pattern.match(line)
        assert m, line
        seen.append((int(m.group(1)), int(m.group(2))))
        vals = [float(v) for v in m.groups()[4::2]]                        # Loss, cls Loss, reg Loss, Depth_MAE: the current values
        assert vals == [float("%6.4f" % v) for v in h[2:]]
    assert seen == [(1, 0), (1, 1), (2, 0), (2, 1)]
    first = pattern.match(lines[0]).groups()
    assert first[4] == first[5]                                            # after one batch the average is the value
