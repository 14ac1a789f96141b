"""The batched evaluation (`engine.inference.inference(batch_size > 1 | gen_out_dir=...)`) on the four-image fixture directory:
against the one-image loop file by file, the records of the same pass against `generate_infer_data`, one model call per
validation image from `do_train`, no host synchronisation inside the loop, the walker under both passes (`eval_batches`), and the
command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_input_host as IH  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.GENERATE_GMW", True, "TEST.DETECTIONS_THRESHOLD", 0.0]


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """The fixture directory as test_inference_from_a_kitti_directory builds it, and one initialised detector for every test here
    (nothing below changes its weights).  Threshold 0: every image keeps its 50 rows, so the comparisons have something to compare."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    root, _ = IH.write_kitti_dir(tmp_path_factory.mktemp("eval_batched"), [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=OPTS)
    files = KittiFiles(root, "train", cfg, is_train=False)
    assert len(files) == 4
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    return dict(root=root, cfg=cfg, files=files, model=model, pipe=DeviceInputPipeline(cfg, cuda, is_train=False),
                ids=[files.img_id(i) for i in range(4)])


def _columns(anno):
    return np.concatenate([anno["alpha"][:, None], anno["bbox"], anno["dimensions"], anno["location"], anno["rotation_y"][:, None],
                           anno["score"][:, None]], 1)


def test_batches_of_three_and_one_write_what_the_one_image_loop_writes(world, tmp_path):
    from dcd_amd.engine.inference import inference
    from dcd_amd.eval import kitti_annos
    one, three = str(tmp_path / "one"), str(tmp_path / "three")
    r1 = inference(world["model"], world["files"], world["pipe"], one, batch_size=1)
    r3 = inference(world["model"], world["files"], world["pipe"], three, batch_size=3)
    assert world["model"].heads.predictor.sparse_eval_heads is False                      # restored after the pass
    names = [i + ".txt" for i in world["ids"]]
    assert sorted(os.listdir(os.path.join(one, "data"))) == names == sorted(os.listdir(os.path.join(three, "data")))
    a1 = kitti_annos.read_annos(os.path.join(one, "data"), world["ids"])
    a3 = kitti_annos.read_annos(os.path.join(three, "data"), world["ids"])
    total, worst = 0, 0.0
    for x, y in zip(a1, a3):
        assert len(x["name"]) == len(y["name"]) and x["name"].tolist() == y["name"].tolist()
        total += len(x["name"])
        cx, cy = _columns(x), _columns(y)
        if len(cx):
            # 1e-4 of the column's scale plus 1e-4: one unit of the last decimal `write_detections` keeps
            bar = 1e-4 * np.abs(cx).max(0) + 1e-4
            worst = max(worst, float((np.abs(cx - cy) / bar).max()))
            assert (np.abs(cx - cy) <= bar).all(), (np.abs(cx - cy) / bar).max(0)
    print("rows compared: %d, worst difference / bar: %.3f" % (total, worst))
    assert total == 4 * world["cfg"].TEST.DETECTIONS_PER_IMG
    assert set(r1) == set(r3) == {"R40"} and list(r1["R40"]) == list(r3["R40"])


def test_records_come_out_of_the_same_pass(world, tmp_path):
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.train import generate_infer_data
    want = json.load(open(generate_infer_data(world["model"], world["files"], world["pipe"], str(tmp_path / "two_pass"))))
    out = str(tmp_path / "gen")
    inference(world["model"], world["files"], world["pipe"], str(tmp_path / "out"), batch_size=3, gen_out_dir=out)
    got = json.load(open(os.path.join(out, "gen_data_infer.json")))
    assert list(got) == list(want) == world["ids"]
    for img_id in want:
        assert len(got[img_id]) == len(want[img_id]) == world["cfg"].TEST.DETECTIONS_PER_IMG
        for a, b in zip(got[img_id], want[img_id]):
            assert a.keys() == b.keys() and a["cat"] == b["cat"]
            for k in a:
                if k != "cat":
                    assert np.asarray(a[k]).shape == np.asarray(b[k]).shape
                    assert np.allclose(np.asarray(a[k]), np.asarray(b[k]), rtol=1e-5, atol=1e-5), (img_id, k)
    # batch_size = 1 with gen_out_dir is the batched loop as well
    out1 = str(tmp_path / "gen1")
    inference(world["model"], world["files"], world["pipe"], str(tmp_path / "out1"), gen_out_dir=out1)
    assert json.load(open(os.path.join(out1, "gen_data_infer.json"))).keys() == want.keys()


def test_do_train_walks_the_validation_split_once(world, cuda, tmp_path):
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    from dcd_amd.config import get_cfg
    cfg, model = get_cfg(opts=OPTS + ["SOLVER.IMS_PER_BATCH", 1]), world["model"]
    train_files = KittiFiles(world["root"], cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    split = ResidentSplit(train_files, cfg, cuda, workers=2)
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    seen = []
    hook = model.backbone.register_forward_hook(lambda m, inp, out: seen.append((model.training, int(inp[0].shape[0]))))
    out = str(tmp_path / "out")
    try:
        args = do_train(cfg, model, optimizer, scheduler, warmup, ResidentBatches(split, 1, seed=0), {"iteration": 0}, out,
                        val=(world["files"], world["pipe"]), val_batch_size=3)
    finally:
        hook.remove()
    assert [n for training, n in seen if not training] == [3, 1]               # every validation image once: batches of 3 and 1
    assert sum(n for training, n in seen if training) == len(train_files)
    assert sorted(os.listdir(os.path.join(out, "gen_data"))) == ["gen_data_infer.json", "gen_data_train.json"]
    infer = json.load(open(os.path.join(out, "gen_data", "gen_data_infer.json")))
    assert sorted(infer) == world["ids"] and all(len(v) == cfg.TEST.DETECTIONS_PER_IMG for v in infer.values())
    assert "R40" in args["eval"]
    assert sorted(os.listdir(os.path.join(out, "inference", "data"))) == [i + ".txt" for i in world["ids"]]


def test_the_loop_never_waits_on_an_image(world, tmp_path, monkeypatch):
    """`.item()`, `.cpu()`, `nonzero` and `torch.cuda.synchronize` are counted while the batched pass runs: none.  Its waits are
    the pinned copy-out slots' events: one `Event.synchronize` per batch and no more.  (`DeviceInputPipeline` guards its two
    pinned UPLOAD slots the same way -- `slot.event.synchronize()` on the copy that read the slot two calls earlier, at most one
    per call; those are told apart by the calling file and held to that.)"""
    from dcd_amd.data import input_pipeline
    from dcd_amd.engine import inference as inf
    counts = {"item": 0, "cpu": 0, "nonzero": 0, "synchronize": 0, "event": 0, "upload slot": 0, "other event": 0}
    event_sync = torch.cuda.Event.synchronize

    def counted_event(self):
        caller = os.path.abspath(sys._getframe(1).f_code.co_filename)
        where = {os.path.abspath(inf.__file__): "event", os.path.abspath(input_pipeline.__file__): "upload slot"}
        counts[where.get(caller, "other event")] += 1
        return event_sync(self)

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapper
    model = world["model"]
    folder = str(tmp_path / "data")
    os.makedirs(folder)
    model.eval()
    with torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
        mp.setattr(torch.Tensor, "cpu", counted("cpu", torch.Tensor.cpu))
        mp.setattr(torch.Tensor, "nonzero", counted("nonzero", torch.Tensor.nonzero))
        mp.setattr(torch, "nonzero", counted("nonzero", torch.nonzero))
        mp.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
        mp.setattr(torch.cuda.Event, "synchronize", counted_event)
        records = inf._batched_pass(model, world["files"], world["pipe"], folder, 3, None, True)
    uploads = counts.pop("upload slot")
    assert counts == {"item": 0, "cpu": 0, "nonzero": 0, "synchronize": 0, "event": 2, "other event": 0}, counts
    assert uploads <= 2
    assert list(records) == world["ids"] and sorted(os.listdir(folder)) == [i + ".txt" for i in world["ids"]]


def _same_batch(got, want):
    """Two batches of the input pipeline, bit for bit: the images and every tensor or string field of every target."""
    def bits(t):
        return t.contiguous().reshape(-1).view(torch.uint8)
    (images, targets), (ref_images, ref_targets) = got, want
    assert images.dtype == ref_images.dtype and images.shape == ref_images.shape and torch.equal(bits(images), bits(ref_images))
    assert len(targets) == len(ref_targets)
    compared = 0
    for t, r in zip(targets, ref_targets):
        assert t.fields() == r.fields() and tuple(t.size) == tuple(r.size)
        for name in t.fields():
            a, b = t.get_field(name), r.get_field(name)
            assert type(a) is type(b), name
            if torch.is_tensor(a):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), name
                compared += 1
            elif isinstance(a, str):
                assert a == b, name
    assert compared >= len(targets)                                    # (the targets do carry tensors)


def test_eval_batches_walks_the_split_and_stops_its_threads(world):
    """`eval_batches` at batch size 3 over the four images: batches [0, 1, 2] and [3], bit-equal to `EvalBatches.get(k)`; and a
    loop body that raises leaves no thread pool behind: the executor refuses further work by the time the exception is out."""
    from dcd_amd.data.batches import EvalBatches, eval_batches
    plain = EvalBatches(world["files"], world["pipe"], 3, 2)
    try:
        want = [plain.get(k) for k in range(plain.num_batches)]
    finally:
        plain.close()
    torch.cuda.synchronize()
    assert len(want) == 2
    seen = []
    with eval_batches(world["files"], world["pipe"], 3, 2) as walk:
        for k, indices, images, targets in walk:
            seen.append((k, indices))
            torch.cuda.synchronize()
            _same_batch((images, targets), want[k])
        pool = walk.source._pool
        pool.submit(int).result()                                      # still open inside the block
    assert seen == [(0, [0, 1, 2]), (1, [3])]
    with pytest.raises(RuntimeError, match="shutdown"):
        pool.submit(int)

    class Stop(Exception):
        pass
    pools = []
    with pytest.raises(Stop):
        with eval_batches(world["files"], world["pipe"], 3, 2) as walk:
            for k, indices, images, targets in walk:
                pools.append(walk.source._pool)
                raise Stop()
    assert len(pools) == 1 and pools[0]._shutdown
    with pytest.raises(RuntimeError, match="shutdown"):
        pools[0].submit(int)


def test_command_line_evaluates_a_checkpoint(world, tmp_path):
    from dcd_amd.engine.train import save_checkpoint
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    optimizer = build_optimizer(world["model"], world["cfg"])
    scheduler, _ = build_scheduler(optimizer, world["cfg"])
    ckpt = save_checkpoint(str(tmp_path / "ckpt"), "model_final", world["model"], optimizer, scheduler, {"iteration": 1})
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "dcd_amd.engine.inference", "--root", world["root"], "--split", "train", "--ckpt", ckpt,
           "--output-dir", out, "--batch", "3", "--gen-data"] + [str(v) for v in OPTS]
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert sorted(os.listdir(os.path.join(out, "inference", "data"))) == [i + ".txt" for i in world["ids"]]
    assert os.path.exists(os.path.join(out, "gen_data", "gen_data_infer.json"))
    assert "R40" in json.loads(done.stdout.strip().splitlines()[-1])
