"""The one-pass evaluation of the whole system, `engine.inference.inference(gmw=...)`, on the four-image fixture directory,
against the two-step route it replaces: `inference(gen_out_dir=...)` -> `gen_data_infer.json` -> `gmw.load_infer_data` ->
`gmw.evaluate`.  With the same refinement partition the two routes' files are compared byte for byte."""
import json
import logging
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_input_host as IH  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0]


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """The fixture directory of tests/test_gpu_eval_batched.py, an initialised detector, a seeded GMW, and the fixture's labels in
    the layout `gmw.evaluate` reads (<root>/training/label_2, ImageSets/val.txt)."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.gmw import GMW
    from dcd_amd.model.detector import KeypointDetector
    g = np.load(os.path.join(IH.GOLDEN, "kitti_files", "kitti_files.npz"))
    base = tmp_path_factory.mktemp("dcd_eval")
    root, _ = IH.write_kitti_dir(base, [tuple(int(v) for v in s) for s in g["image_sizes"]], noise_seed=9)
    cfg = get_cfg(opts=OPTS)
    files = KittiFiles(root, "train", cfg, is_train=False)
    ids = [files.img_id(i) for i in range(len(files))]
    assert len(ids) == 4
    gmw_root = base / "for_gmw"
    (gmw_root / "training" / "ImageSets").mkdir(parents=True)
    shutil.copytree(os.path.join(root, "label_2"), str(gmw_root / "training" / "label_2"))
    (gmw_root / "training" / "ImageSets" / "val.txt").write_text("".join(i + "\n" for i in ids))
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)
    init_like_trained(model)
    torch.manual_seed(0)
    gmw = GMW().to(cuda).eval()
    return dict(root=root, gmw_root=str(gmw_root), cfg=cfg, files=files, model=model, gmw=gmw, ids=ids, base=base,
                pipe=DeviceInputPipeline(cfg, cuda, is_train=False))


def _two_step(world, out, threshold=None, gmw_batch=64, raw=None):
    """The parent route at batch 3: the detector's pass with its JSON, the file parsed back, `gmw.evaluate`.  Returns the result
    folder and the AP text.  raw: a list that receives every image's raw scores (what the pass cuts at the threshold)."""
    from dcd_amd.engine import inference as inf
    from dcd_amd.gmw import evaluate, load_infer_data
    original = inf.write_image_rows

    def spy(rows, raw_scores, threshold, path):
        raw.append(np.array(raw_scores, np.float64))
        return original(rows, raw_scores, threshold, path)
    if raw is not None:
        inf.write_image_rows = spy
    try:
        with _threshold(world, threshold):
            results = inf.inference(world["model"], world["files"], world["pipe"], os.path.join(out, "det"), batch_size=3,
                                    gen_out_dir=os.path.join(out, "gen"))
    finally:
        inf.write_image_rows = original
    data = load_infer_data(os.path.join(out, "gen", "gen_data_infer.json"))
    text, result, _ = evaluate(world["gmw"], data, world["gmw_root"], None, os.path.join(out, "gmw"), device=world["pipe"].device,
                               batch_size=gmw_batch)
    return dict(dir=os.path.join(out, "gmw", "kitti_results_for_eval"), text=text, result=result, det=os.path.join(out, "det", "data"),
                det_results=results, n=len(data["img_idx"]), raw=raw)


class _threshold:
    """The post-processor's score threshold for the length of a `with` (None: as configured)."""

    def __init__(self, world, value):
        self.pp, self.value = world["model"].heads.post_processor, value

    def __enter__(self):
        self.before = self.pp.det_threshold
        if self.value is not None:
            self.pp.det_threshold = self.value

    def __exit__(self, *exc):
        self.pp.det_threshold = self.before


def _one_pass(world, out, caplog, threshold=None, gmw_batch=64):
    from dcd_amd.engine.inference import inference
    with _threshold(world, threshold), caplog.at_level(logging.INFO, logger="dcd_amd.inference"):
        caplog.clear()
        results = inference(world["model"], world["files"], world["pipe"], out, batch_size=3, gmw=world["gmw"], gmw_batch=gmw_batch)
    texts = [r.args[1] for r in caplog.records if r.msg.startswith("GMW ")]
    assert len(texts) == 1
    return dict(dir=os.path.join(out, "kitti_results_for_eval"), text=texts[0], results=results, det=os.path.join(out, "data"))


@pytest.fixture(scope="module")
def two_step(world):
    return _two_step(world, str(world["base"] / "two_step"), raw=[])


def _read(folder, ids):
    assert sorted(os.listdir(folder)) == [i + ".txt" for i in ids]
    return {i: open(os.path.join(folder, i + ".txt"), "rb").read() for i in ids}


def _same(a, b):
    """Result dicts of `official_eval` (numbers and arrays) compared exactly."""
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_same_partition_same_bytes(world, two_step, tmp_path, caplog):
    """200 records in groups of 64: flushes of 64, 64, 64 and 8, and the image batches' 150 and 50 records straddle them."""
    from dcd_amd.engine.inference import inference
    assert two_step["n"] == 4 * world["cfg"].TEST.DETECTIONS_PER_IMG == 200
    one = _one_pass(world, str(tmp_path / "one"), caplog)
    want, got = _read(two_step["dir"], world["ids"]), _read(one["dir"], world["ids"])
    for i in world["ids"]:
        assert got[i] == want[i] and len(got[i].splitlines()) == 50, i
    assert one["text"] == two_step["text"]
    _same(one["results"]["gmw"]["R40"], two_step["result"])
    assert set(one["results"]) == {"R40", "gmw"} and set(one["results"]["gmw"]) == {"R40"}
    # the detector's own outputs are those of a run without gmw
    plain = inference(world["model"], world["files"], world["pipe"], str(tmp_path / "plain"), batch_size=3)
    assert _read(one["det"], world["ids"]) == _read(str(tmp_path / "plain" / "data"), world["ids"]) == _read(two_step["det"], world["ids"])
    _same(one["results"]["R40"], plain["R40"])
    assert not os.path.exists(str(tmp_path / "plain" / "kitti_results_for_eval")) and "gmw" not in plain
    assert world["gmw"].training is False and world["model"].heads.predictor.sparse_eval_heads is False


def _parse(blob):
    lines = [l.split() for l in blob.decode().splitlines()]
    assert all(l[0] == "Car" and len(l) == 16 for l in lines)
    return np.array([[float(v) for v in l[1:]] for l in lines], np.float64).reshape(len(lines), 15)


def test_another_partition(world, two_step, tmp_path, caplog):
    """One group of 200 (gmw_batch = 256) against the files refined in groups of 64: the location columns within rtol 2e-5, the
    bar tests/test_gpu_gmw_refine.py holds this chain to against the reference's fixture; box, dimensions, yaw and score equal."""
    one = _one_pass(world, str(tmp_path / "one"), caplog, gmw_batch=256)
    want, got = _read(two_step["dir"], world["ids"]), _read(one["dir"], world["ids"])
    worst = 0.0
    for i in world["ids"]:
        a, b = _parse(got[i]), _parse(want[i])                         # truncated, occluded | alpha | box 4 | hwl | xyz | ry | score
        assert a.shape == b.shape == (50, 15)
        assert np.array_equal(a[:, [0, 1, 3, 4, 5, 6, 7, 8, 9, 13, 14]], b[:, [0, 1, 3, 4, 5, 6, 7, 8, 9, 13, 14]]), i
        worst = max(worst, float((np.abs(a[:, 10:13] - b[:, 10:13]) / np.abs(b[:, 10:13])).max()))
        assert np.allclose(a[:, 10:13], b[:, 10:13], rtol=2e-5, atol=0), i
    print("worst relative difference of a location between the partitions: %.3g" % worst)


def test_short_and_empty_prefixes(world, two_step, tmp_path, caplog):
    """A threshold from the threshold-0 run's own raw scores (descending per image): half-way between two neighbouring scores of
    the image with the best candidate, above every other image's best, so that the others keep nothing and that image keeps some
    rows but not all."""
    raw = two_step["raw"]
    assert len(raw) == 4 and all(len(s) == 50 for s in raw)
    order = sorted(range(4), key=lambda i: raw[i][0])
    top, runner_up = raw[order[-1]], float(raw[order[-2]][0])
    assert top[0] > runner_up
    r = max(i for i in range(49) if top[i] > runner_up and top[i] > top[i + 1])      # the last row kept
    threshold = (float(top[r]) + max(float(top[r + 1]), runner_up)) / 2
    assert max(float(top[r + 1]), runner_up) < threshold < float(top[r])
    ref = _two_step(world, str(tmp_path / "two"), threshold=threshold)
    one = _one_pass(world, str(tmp_path / "one"), caplog, threshold=threshold)
    want, got = _read(ref["dir"], world["ids"]), _read(one["dir"], world["ids"])
    kept = [len(want[i].splitlines()) for i in world["ids"]]
    print("threshold %.6f keeps %s rows" % (threshold, kept))
    assert min(kept) == 0 and any(0 < k < 50 for k in kept), kept
    for i, k in zip(world["ids"], kept):
        assert got[i] == want[i], i
        if k == 0:
            assert got[i] == b""
    assert one["text"] == ref["text"]
    assert _read(one["det"], world["ids"]) == _read(ref["det"], world["ids"])


def test_the_pass_with_gmw_never_waits_on_an_image(world, tmp_path, monkeypatch):
    """The counting harness of tests/test_gpu_eval_batched.py on the pass with a refiner: no `.item()`, `.cpu()`, `nonzero` or
    `torch.cuda.synchronize`; one event wait per image batch from engine/inference.py; from the refiner's file at most one per
    flush plus one."""
    from dcd_amd.data import input_pipeline
    from dcd_amd.engine import inference as inf
    from dcd_amd.gmw import inference as ginf
    counts = {"item": 0, "cpu": 0, "nonzero": 0, "synchronize": 0, "event": 0, "upload slot": 0, "refiner": 0, "other event": 0}
    event_sync = torch.cuda.Event.synchronize

    def counted_event(self):
        caller = os.path.abspath(sys._getframe(1).f_code.co_filename)
        where = {os.path.abspath(inf.__file__): "event", os.path.abspath(input_pipeline.__file__): "upload slot",
                 os.path.abspath(ginf.__file__): "refiner"}
        counts[where.get(caller, "other event")] += 1
        return event_sync(self)

    def counted(name, fn):
        def wrapper(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return wrapper
    model, gmw = world["model"], world["gmw"]
    folder = str(tmp_path / "data")
    os.makedirs(folder)
    model.eval()
    refiner = ginf.RecordRefiner(gmw, world["pipe"].device, batch_size=64)
    with torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "item", counted("item", torch.Tensor.item))
        mp.setattr(torch.Tensor, "cpu", counted("cpu", torch.Tensor.cpu))
        mp.setattr(torch.Tensor, "nonzero", counted("nonzero", torch.Tensor.nonzero))
        mp.setattr(torch, "nonzero", counted("nonzero", torch.nonzero))
        mp.setattr(torch.cuda, "synchronize", counted("synchronize", torch.cuda.synchronize))
        mp.setattr(torch.cuda.Event, "synchronize", counted_event)
        records = inf._batched_pass(model, world["files"], world["pipe"], folder, 3, None, False, refiner)
        location = refiner.finish()
    uploads, waits = counts.pop("upload slot"), counts.pop("refiner")
    assert counts == {"item": 0, "cpu": 0, "nonzero": 0, "synchronize": 0, "event": 2, "other event": 0}, counts
    assert uploads <= 2
    assert refiner.flushes == 4 and waits <= refiner.flushes + 1, (refiner.flushes, waits)
    assert records == {} and tuple(location.shape) == (200, 3) and len(refiner.host_ids) == 200
    assert bool(torch.isfinite(location).all())


def test_refiner_refuses_another_key_point_count(world):
    from dcd_amd.gmw.inference import RecordRefiner
    with pytest.raises(ValueError):
        RecordRefiner(world["gmw"], world["pipe"].device, nk=72)


def test_gmw_needs_the_fused_decode(world, tmp_path, monkeypatch):
    """A configuration `decode_fused` refuses is an error with `gmw`, not a fall-back to the one-image loop."""
    from dcd_amd.engine.inference import inference
    pp = world["model"].heads.post_processor

    def refuse():
        raise NotImplementedError("decode_fused: refused for the test")
    monkeypatch.setattr(pp, "decode_spec", refuse)
    with pytest.raises(NotImplementedError, match="fused decode"):
        inference(world["model"], world["files"], world["pipe"], str(tmp_path / "out"), batch_size=3, gmw=world["gmw"])


def test_do_train_reports_the_refined_tables(world, cuda, tmp_path):
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    cfg = get_cfg(opts=OPTS + ["TEST.GENERATE_GMW", True, "SOLVER.IMS_PER_BATCH", 1])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda)                             # its own detector: the shared one keeps its weights
    init_like_trained(model)
    train_files = KittiFiles(world["root"], cfg.DATASETS.TRAIN_SPLIT, cfg, is_train=True)
    split = ResidentSplit(train_files, cfg, cuda, workers=2)
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    seen = []
    hook = model.backbone.register_forward_hook(lambda m, inp, out: seen.append((model.training, int(inp[0].shape[0]))))
    out = str(tmp_path / "out")
    try:
        args = do_train(cfg, model, optimizer, scheduler, warmup, ResidentBatches(split, 1, seed=0), {"iteration": 0}, out,
                        val=(world["files"], world["pipe"]), val_batch_size=3, val_gmw=world["gmw"])
    finally:
        hook.remove()
    assert [n for training, n in seen if not training] == [3, 1]               # every validation image once
    assert "R40" in args["eval"] and "Car_3d_0.70/moderate" in args["eval"]["gmw"]["R40"]
    assert sorted(os.listdir(os.path.join(out, "inference", "kitti_results_for_eval"))) == [i + ".txt" for i in world["ids"]]


def test_command_line_evaluates_both_checkpoints(world, tmp_path):
    from dcd_amd.engine.train import save_checkpoint
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    optimizer = build_optimizer(world["model"], world["cfg"])
    scheduler, _ = build_scheduler(optimizer, world["cfg"])
    ckpt = save_checkpoint(str(tmp_path / "ckpt"), "model_final", world["model"], optimizer, scheduler, {"iteration": 1})
    gmw_ckpt = str(tmp_path / "checkpoint_epoch_1.pth.tar")                    # the keys of gmw.train's save_checkpoint
    torch.save({"epoch": 1, "state_dict": {"module." + k: v.detach().cpu() for k, v in world["gmw"].state_dict().items()},
                "best_mAP": 0.0}, gmw_ckpt)
    out = str(tmp_path / "cli")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "dcd_amd.engine.inference", "--root", world["root"], "--split", "train", "--ckpt", ckpt,
           "--output-dir", out, "--batch", "3", "--gmw-ckpt", gmw_ckpt, "--gmw-batch", "64"] + [str(v) for v in OPTS]
    done = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    last = json.loads(done.stdout.strip().splitlines()[-1])
    assert "R40" in last and "R40" in last["gmw"]
    assert sorted(os.listdir(os.path.join(out, "inference", "kitti_results_for_eval"))) == [i + ".txt" for i in world["ids"]]
    assert not os.path.exists(os.path.join(out, "gen_data"))
