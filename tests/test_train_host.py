"""Host side of a training run, without a GPU: the samplers (dcd_amd/data/samplers.py) against index streams the REFERENCE's
own samplers produced (tests/golden/make_golden_sampler.py -> sampler.npz), the batch definition of dcd_amd/data/batches.py
over a stub split and a stub pipeline, the meters, and `do_train` (dcd_amd/engine/train.py) around a stub source and a stub step.
Every comparison is exact: integer streams, or the same float operations in the same order."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

SIZES, SEEDS, WORLDS = (1, 7, 64), (0, 63), (1, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- samplers
def test_samplers_equal_the_reference_streams():
    """1. Every recorded case; `indices(start)` from inside epoch 0, from an epoch boundary and from inside epoch 2."""
    from dcd_amd.data.samplers import InferenceSampler, TrainingSampler
    g = np.load(os.path.join(GOLDEN, "sampler.npz"))
    assert g["train_s7_seed63_sh1_w1_r0"][:16].tolist() == [0, 3, 2, 6, 1, 5, 4, 0, 5, 6, 2, 1, 4, 3, 4, 1]
    seen = 0
    for size, world in itertools.product(SIZES, WORLDS):
        for rank in range(world):
            for seed, shuffle in itertools.product(SEEDS, (True, False)):
                ref = g["train_s%d_seed%d_sh%d_w%d_r%d" % (size, seed, int(shuffle), world, rank)].tolist()
                assert len(ref) >= 3 * (size // world) + 5
                s = TrainingSampler(size, shuffle=shuffle, seed=seed, rank=rank, world_size=world)
                assert list(itertools.islice(s.indices(), len(ref))) == ref, (size, seed, shuffle, world, rank)
                assert list(itertools.islice(iter(s), 5)) == ref[:5]
                per_epoch = -(-size // world)                           # about one epoch of this rank's stream
                for start in (min(2, len(ref) - 1), per_epoch, size, 2 * per_epoch + 1):
                    if start < len(ref):
                        assert s.take(start, len(ref) - start) == ref[start:], (size, seed, shuffle, world, rank, start)
                seen += 1
            shard = g["infer_s%d_w%d_r%d" % (size, world, rank)].tolist()
            inf = InferenceSampler(size, rank, world)
            assert list(inf) == shard and len(inf) == len(shard)
    assert seen == 3 * 6 * 4
    # the shards of a world partition the range; shuffled streams are not the identity
    for size, world in itertools.product(SIZES, WORLDS):
        assert sum((list(InferenceSampler(size, r, world)) for r in range(world)), []) == list(range(size))
    assert g["train_s64_seed0_sh1_w1_r0"][:64].tolist() != list(range(64))
    assert sorted(g["train_s64_seed0_sh1_w1_r0"][:64].tolist()) == list(range(64))
    with pytest.raises(ValueError):
        TrainingSampler(0)
    with pytest.raises(ValueError):
        TrainingSampler(4, rank=2, world_size=2)


# ------------------------------------------------------------------------------------------------------ batch definition
class StubFiles:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def img_id(self, i):
        return "%06d" % i

    def frame(self, i):
        return i

    def sample(self, i):
        return {"i": i}


class StubSplit:
    """What `ResidentBatches` uses of a `ResidentSplit`; `batch` hands back what it was asked for."""

    def __init__(self, n, cfg):
        self.files, self.cfg = StubFiles(n), cfg

    def __len__(self):
        return len(self.files)

    def batch(self, indices, flips, img_ids=None, stream=None):
        return list(indices), (list(flips), list(img_ids))


class StubPipeline:
    def __init__(self, cfg, is_train=True):
        self.is_train, self.flip_p = is_train, float(cfg.INPUT.AUG_PARAMS[0][0]) if is_train else 0.0

    def __call__(self, frames, samples, img_ids=None, flip=None, stream=None):
        assert [s["i"] for s in samples] == list(frames)
        return list(frames), (list(flip), list(img_ids))


def sources(kind, n, B, seed, cfg, rank=0, world=1, is_train=True):
    from dcd_amd.data.batches import ResidentBatches, StreamingBatches
    if kind == "resident":
        return ResidentBatches(StubSplit(n, cfg), B, seed, rank, world, is_train=is_train)
    return StreamingBatches(StubFiles(n), StubPipeline(cfg, is_train), B, seed, rank, world, workers=2)


@pytest.mark.parametrize("kind", ["resident", "streaming"])
@pytest.mark.parametrize("n,B", [(7, 3), (64, 8)])
def test_batch_k_is_a_function_of_k(kind, n, B):
    """2. Batches 0..9 of a fresh source == batches 5..9 of a second source that is asked for nothing else (a restart); the
    indices are the sampler's stream, the flips one seeded stream; both sources define the same batches."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.samplers import TrainingSampler
    cfg = get_cfg()
    a = sources(kind, n, B, 63, cfg)
    assert a.batch_size == B and len(a) == n
    full = [a.get(k) for k in range(10)]
    b = sources(kind, n, B, 63, cfg)
    assert [b.get(k) for k in range(5, 10)] == full[5:]
    assert b.get(2) == full[2] and b.get(3) == full[3] and a.get(0) == full[0]           # backwards jumps too
    stream = TrainingSampler(n, seed=63).take(0, 10 * B)
    assert [i for idx, _ in full for i in idx] == stream
    flips = [f for _, (fl, _) in full for f in fl]
    assert all(isinstance(f, bool) for f in flips) and 0.25 * len(flips) < sum(flips) < 0.75 * len(flips)
    assert [ids for _, (_, ids) in full] == [["%06d" % i for i in idx] for idx, _ in full]
    other = "streaming" if kind == "resident" else "resident"
    assert [sources(other, n, B, 63, cfg).get(k) for k in (0, 4, 9)] == [full[0], full[4], full[9]]
    assert sources(kind, n, B, 64, cfg).get(0) != full[0] or n == 1
    for s in (a, b):
        if hasattr(s, "close"):
            s.close()


def test_ranks_cover_the_stream_and_evaluation_never_flips():
    from dcd_amd.config import get_cfg
    cfg = get_cfg()
    n, B = 64, 8
    one = sources("resident", n, 2 * B, 5, cfg)
    r0, r1 = sources("resident", n, B, 5, cfg, 0, 2), sources("streaming", n, B, 5, cfg, 1, 2)
    for k in range(10):                                                # batch k of the two ranks interleaved == batch k of world 1
        i0, i1 = r0.get(k)[0], r1.get(k)[0]
        assert [v for pair in zip(i0, i1) for v in pair] == one.get(k)[0]
    r1.close()
    for kind in ("resident", "streaming"):
        ev = sources(kind, 7, 3, 5, cfg, is_train=False)
        got = [ev.get(k) for k in range(6)]
        assert all(fl == [False] * 3 for _, (fl, _) in got)
        assert [i for idx, _ in got for i in idx] == [j % 7 for j in range(18)]          # in order, wrapping round
        if hasattr(ev, "close"):
            ev.close()


def test_decoding_threads_never_follow_the_cpu_count(monkeypatch):
    from dcd_amd.data.resident import default_workers
    monkeypatch.setattr(os, "cpu_count", lambda: 512)
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert default_workers() == 16
    monkeypatch.setenv("OMP_NUM_THREADS", "6")
    assert default_workers() == 6 and default_workers(64) == 16 and default_workers(3) == 3
    monkeypatch.setenv("OMP_NUM_THREADS", "96")
    assert default_workers() == 16


# ------------------------------------------------------------------------------------------------------------------ meters
def test_meters_in_blocks_equal_meters_one_by_one():
    """3. Recorded per-iteration rows fed in blocks of `log_every` == fed one by one: medians (window 20), global averages."""
    from dcd_amd.engine.train import MetricLogger
    rng = np.random.RandomState(4)
    names = ["loss", "hm_loss", "2D_IoU", "extra_all_MAE"]
    rows = rng.rand(57, len(names)).astype(np.float32).tolist()
    for log_every in (1, 10, 23):
        single, block = MetricLogger(), MetricLogger()
        for start in range(0, len(rows), log_every):
            chunk = rows[start:start + log_every]
            for r in chunk:
                single.update(**dict(zip(names, r)))
            block.update_block(names, chunk)
            for k in single.meters:
                a, b = single[k], block[k]
                assert (a.median, a.avg, a.global_avg, a.value, a.count) == (b.median, b.avg, b.global_avg, b.value, b.count)
            assert str(single) == str(block)
    col = [r[0] for r in rows]
    m = block["loss"]
    assert m.count == 57 and m.global_avg == sum(col) / 57                # same order of additions: exact
    assert m.median == torch.tensor(col[-20:]).median().item() and m.value == col[-1]
    assert "loss: %.4f (%.4f)" % (m.median, m.global_avg) in str(block)


# ---------------------------------------------------------------------------------------------------------------- do_train
class StubSource:
    batch_size = 2

    def __init__(self, n=8):
        self.n, self.asked = n, []

    def __len__(self):
        return self.n

    def get(self, k):
        self.asked.append(k)
        g = torch.Generator().manual_seed(1000 + k)
        return torch.randn(2, 4, generator=g), torch.randn(2, 1, generator=g)


class LossEvaluator:
    def __init__(self):
        self.gen_data = {"img_idx": []}


class StubModel(nn.Module):
    """`nn.Linear(4, 1)` behind the detector's calling convention: model(images, targets) -> (loss_dict, log_loss_dict)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.fc = nn.Linear(4, 1)
        self.bn = nn.BatchNorm1d(1)
        self.heads = nn.Module()
        self.heads.loss_evaluator = LossEvaluator()
        self.calls = 0

    def forward(self, images, targets):
        self.calls += 1
        self.heads.loss_evaluator.gen_data["img_idx"].append(self.calls)
        loss = (self.bn(self.fc(images)) - targets).pow(2).mean()
        return {"fit_loss": loss}, {"fit_loss": loss.detach(), "metric": images.detach().abs().sum()}


def setup_run(tmp_path, name, opts):
    from dcd_amd.config import get_cfg
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    cfg = get_cfg(opts=["SOLVER.MAX_ITERATION", 6, "SOLVER.SAVE_CHECKPOINT_INTERVAL", 2, "SOLVER.IMS_PER_BATCH", 2, "SOLVER.STEPS", (4,),
                        "SOLVER.WARMUP_STEPS", 3] + list(opts))
    model = StubModel()
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    lrs = []

    def step(images, targets):
        optimizer.zero_grad()
        loss_dict, log = model(images, targets)
        loss_dict["fit_loss"].backward()
        lrs.append([float(g["lr"]) for g in optimizer.param_groups])
        optimizer.step()
        return loss_dict, log
    out = str(tmp_path / name)
    return cfg, model, optimizer, scheduler, warmup, step, lrs, out


def params_of(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


@pytest.mark.parametrize("warm", [False, True], ids=["no-warmup", "warmup"])
def test_do_train_iterations_schedule_and_checkpoints(tmp_path, warm):
    """4a/4b. Six iterations, a checkpoint every two: the named files and `last_checkpoint`; the iteration count; the learning
    rate every step used == a hand-written loop over `step_schedulers`."""
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, step_schedulers
    cfg, model, optimizer, scheduler, warmup, step, lrs, out = setup_run(tmp_path, "run", ["SOLVER.LR_WARMUP", warm])
    source = StubSource()
    args = do_train(cfg, model, optimizer, scheduler, warmup, source, {"iteration": 0, "iter_per_epoch": 2}, out, step=step, log_every=4)
    assert args["iteration"] == 6 and args["iter_per_epoch"] == 2 and source.asked == list(range(6))
    assert sorted(os.listdir(out)) == ["last_checkpoint", "model_checkpoint_1.pth", "model_checkpoint_2.pth", "model_checkpoint_3.pth",
                                       "model_final.pth"]                     # iteration // iter_per_epoch at 2, 4 and 6
    assert open(os.path.join(out, "last_checkpoint")).read() == os.path.join(out, "model_final.pth")
    final = torch.load(os.path.join(out, "model_final.pth"), weights_only=False)
    assert final["iteration"] == 6 and final["iter_per_epoch"] == 2 and set(final) >= {"model", "optimizer", "scheduler"}
    assert [torch.load(os.path.join(out, "model_checkpoint_%d.pth" % e), weights_only=False)["iteration"] for e in (1, 2, 3)] == [2, 4, 6]
    for k, v in final["model"].items():
        assert torch.equal(v, model.state_dict()[k]), k
    # the learning-rate trace by hand
    ref_model = StubModel()
    ref_opt = build_optimizer(ref_model, cfg)
    ref_sched, ref_warm = build_scheduler(ref_opt, cfg)
    want = []
    for it in range(6):
        want.append([float(g["lr"]) for g in ref_opt.param_groups])
        ref_opt.step()
        step_schedulers(ref_sched, ref_warm, it, cfg)
    assert lrs == want
    assert len({tuple(v) for v in want}) > 1                               # the schedule does move inside six iterations
    if warm:
        assert want[1][0] < want[3][0]                                     # the cosine warm-up rises towards the base rate


def test_do_train_resumed_equals_straight(tmp_path):
    """4c. Three iterations, `resume`, three more == six straight: parameters, BN buffers, iteration, batches asked for."""
    from dcd_amd.engine.train import do_train, resume
    cfg, model, optimizer, scheduler, warmup, step, lrs, out = setup_run(tmp_path, "straight", ["SOLVER.LR_WARMUP", True])
    do_train(cfg, model, optimizer, scheduler, warmup, StubSource(), {"iteration": 0}, out, step=step)
    straight = params_of(model)

    cfg3, m1, o1, s1, w1, step1, lrs1, out1 = setup_run(tmp_path, "first", ["SOLVER.LR_WARMUP", True, "SOLVER.MAX_ITERATION", 3])
    a1 = do_train(cfg3, m1, o1, s1, w1, StubSource(), {"iteration": 0}, out1, step=step1)
    assert a1["iteration"] == 3
    _, m2, o2, s2, w2, step2, lrs2, _ = setup_run(tmp_path, "second", ["SOLVER.LR_WARMUP", True])
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)                                                    # resume must bring the parameters back
    args = resume(out1, m2, o2, s2)                                        # the directory: through `last_checkpoint`
    assert args["iteration"] == 3 and args["iter_per_epoch"] == 4
    source = StubSource()
    args = do_train(cfg, m2, o2, s2, w2, source, args, out1, step=step2)
    assert args["iteration"] == 6 and source.asked == [3, 4, 5]
    assert lrs1 + lrs2 == lrs
    resumed = params_of(m2)
    assert set(resumed) == set(straight)
    for k in straight:
        assert torch.equal(resumed[k], straight[k]), k
    assert not torch.equal(straight["fc.weight"], StubModel().fc.weight)


def test_do_train_collection_pass_changes_nothing(tmp_path):
    """4d. TEST.GENERATE_GMW: BatchNorm frozen inside a model in train mode, no gradient, no optimizer / scheduler step, no
    checkpoint; start + len(batches) // IMS_PER_BATCH iterations; the collected records are dumped."""
    import copy
    import json
    from dcd_amd.engine.train import do_train
    cfg, model, optimizer, scheduler, warmup, step, lrs, out = setup_run(
        tmp_path, "gen", ["SOLVER.LR_WARMUP", True, "TEST.GENERATE_GMW", True, "SOLVER.MAX_ITERATION", 1000])
    before = params_of(model)
    opt_before = copy.deepcopy(optimizer.state_dict())
    sched_before, warm_before = copy.deepcopy(scheduler.state_dict()), copy.deepcopy(warmup.state_dict())
    source = StubSource(n=9)
    args = do_train(cfg, model, optimizer, scheduler, warmup, source, {"iteration": 5}, out, step=step)
    assert args["iteration"] == 5 + 9 // 2 and source.asked == [5, 6, 7, 8]
    assert model.training and not model.bn.training
    assert lrs == [] and model.calls == 4                                   # the step was never called, the model was
    after = params_of(model)
    for k in before:
        assert torch.equal(before[k], after[k]), k                          # running statistics included: BN is frozen
    assert all(p.grad is None for p in model.parameters())
    assert optimizer.state_dict()["state"] == opt_before["state"] == {}
    assert [g["lr"] for g in optimizer.state_dict()["param_groups"]] == [g["lr"] for g in opt_before["param_groups"]]
    drop = ("lr_lambdas",)
    assert {k: v for k, v in scheduler.state_dict().items() if k not in drop} == {k: v for k, v in sched_before.items() if k not in drop}
    assert warmup.state_dict() == warm_before
    assert os.listdir(out) == ["gen_data"] and os.listdir(os.path.join(out, "gen_data")) == ["gen_data_train.json"]
    assert json.load(open(os.path.join(out, "gen_data", "gen_data_train.json"))) == {"img_idx": [1, 2, 3, 4]}


def test_do_train_reports_a_non_finite_loss_and_needs_its_warmup(tmp_path):
    from dcd_amd.engine.train import do_train
    cfg, model, optimizer, scheduler, warmup, step, lrs, out = setup_run(tmp_path, "bad", ["SOLVER.LR_WARMUP", True])
    with pytest.raises(ValueError):
        do_train(cfg, model, optimizer, scheduler, None, StubSource(), {"iteration": 0}, out, step=step)

    class Log(dict):
        def unread(self):
            return ["fit_loss"], torch.tensor([float("nan")]), ["fit_loss"]
    with pytest.raises(FloatingPointError):
        do_train(cfg, model, optimizer, scheduler, warmup, StubSource(), {"iteration": 0}, out, step=lambda i, t: ({}, Log()))
