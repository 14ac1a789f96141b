"""Right-camera views and the unlabelled `test` split on the GPU.  Nothing here is a new kernel: the feature arrives as more rows
and more frames of the kind the device already handles, and these tests prove that on right-view rows and on object-free rows --
`DeviceInputPipeline` against the REFERENCE's own targets of tests/golden/right_views.npz, `ResidentSplit` against the pipeline
bit for bit, two real training iterations and the record collection over a both-cameras split, and `inference` over a split
without labels.

Targets are compared at the bars of tests/test_gpu_input.py (integers exact, floats 1e-6 of the field's range), images and
resident batches with no tolerance."""
import json
import logging
import math
import os
import re
import shutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_input_host as IH  # noqa: E402
import test_oracle_targets as OT  # noqa: E402
import test_right_views_host as RH  # noqa: E402
from test_gpu_dcd_eval import world  # noqa: E402,F401  (the seeded detector and GMW of the one-pass evaluation tests)
from test_gpu_input import tensor_fields  # noqa: E402
from test_gpu_resident import assert_same_batch  # noqa: E402

SMALL = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "INPUT.WIDTH_TRAIN", 96, "INPUT.HEIGHT_TRAIN", 32,
         "DATASETS.USE_RIGHT_IMAGE", True]
FULL = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "DATASETS.USE_RIGHT_IMAGE", True]


def both_cameras(opts):
    """(cfg, files, frames, samples) of tests/golden/kitti_right/ as a training split with both cameras: 2 N = 6 views."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    cfg = get_cfg(opts=opts)
    files = KittiFiles(RH.RIGHT_ROOT, "train", cfg, is_train=True)
    assert len(files) == 6 and [files.is_right(i) for i in range(6)] == [False] * 3 + [True] * 3
    return cfg, files, [files.frame(i) for i in range(6)], [files.sample(i) for i in range(6)]


@pytest.fixture(scope="module")
def small(cuda):
    """The split at the fixture's own 96 x 32 canvas, read once and made resident."""
    from dcd_amd.data.resident import ResidentSplit
    cfg, files, frames, samples = both_cameras(SMALL)
    return dict(cfg=cfg, files=files, frames=frames, samples=samples, split=ResidentSplit(files, cfg, cuda, workers=2))


@pytest.fixture(scope="module")
def full(cuda):
    """The split at the default 384 x 1280 canvas, resident, and an initialised detector: what the two real iterations of
    tests/test_gpu_resident.py run on."""
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    cfg, files, frames, samples = both_cameras(FULL + ["SOLVER.MAX_ITERATION", 2, "SOLVER.IMS_PER_BATCH", 2])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).to(cuda).train()
    init_like_trained(model)
    return dict(cfg=cfg, files=files, split=ResidentSplit(files, cfg, cuda, workers=2), model=model)


def test_targets_of_both_views_equal_the_reference(cuda, small):
    """1. All six views through `DeviceInputPipeline`, each flipped and unflipped (two mixed flag vectors): every `ParamsList`
    field against the reference's, `calib.P` and `Calib_P` the view's own matrix (P3 for a right view, flipped where flagged), the
    images equal to the restatement of the image kernel's formula on the view's own file.  Then the four images as the unlabelled
    split: the fields of the reference's test-mode target."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    g = RH.load_right()
    cfg, frames, samples = small["cfg"], small["frames"], small["samples"]
    ids = [small["files"].img_id(i) for i in range(6)]
    pipe = DeviceInputPipeline(cfg, cuda, is_train=True, seed=0)
    kept = 0
    for flags in ([True, False, True, False, True, False], [False, True, False, True, False, True]):
        images, targets = pipe(frames, samples, img_ids=ids, flip=flags)
        assert images.shape == (6, 3, 32, 96) and images.dtype == torch.float32
        ref = IH.restate_images(frames, flags, 32, 96, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR)
        assert torch.equal(images.cpu(), ref)
        for i, (t, f) in enumerate(zip(targets, flags)):
            got = tensor_fields(t)
            OT.compare(got, RH.Fields(g, "flip" if f else "out"), i, 1e-6)
            P = g["flipP%d" % i] if f else g["in%d_P" % i]
            np.testing.assert_array_equal(t.get_field("calib").P, P)
            mask = got["reg_mask"].astype(bool)
            assert mask.any()
            np.testing.assert_array_equal(got["Calib_P"][mask], np.broadcast_to(P.astype(np.float32), (int(mask.sum()), 3, 4)))
            assert t.get_field("img_idx") == ids[i]
            kept += int(mask.sum())
    assert kept == 2 * sum(int(g["out%d_reg_mask" % i].sum()) for i in range(6)) >= 24
    with pytest.raises(AssertionError):                                        # a right view's targets are not its left view's
        OT.compare(tensor_fields(targets[3]), RH.Fields(g, "out"), 0, 1e-6)
    ev_cfg = get_cfg(opts=SMALL[:8])
    test = KittiFiles(RH.RIGHT_ROOT, "test", ev_cfg, is_train=False)
    assert not test.has_labels and len(test) == int(g["test_n"]) == 4
    t_frames, t_samples = [test.frame(j) for j in range(4)], [test.sample(j) for j in range(4)]
    images, targets = DeviceInputPipeline(ev_cfg, cuda, is_train=False)(t_frames, t_samples, img_ids=[test.img_id(j) for j in range(4)])
    assert torch.equal(images.cpu(), IH.restate_images(t_frames, [False] * 4, 32, 96, ev_cfg.INPUT.PIXEL_MEAN, ev_cfg.INPUT.PIXEL_STD,
                                                        ev_cfg.INPUT.TO_BGR))
    for j, t in enumerate(targets):
        got = tensor_fields(t)
        for name in ("pad_size", "edge_len", "edge_indices", "final_output_w", "final_output_h"):
            np.testing.assert_array_equal(got[name].astype(np.int64), g["test%d_%s" % (j, name)].astype(np.int64), err_msg="%d %s" % (j, name))
        np.testing.assert_array_equal(t.get_field("calib").P, g["test%d_P" % j])
        assert int(got["reg_mask"].sum()) == 0 and float(got["hm"].max()) == 0.0


@pytest.mark.parametrize("indices,flags", [
    ([3], [True]),
    ([2, 3, 5], [False, True, False]),
    ([0, 3, 3, 1, 4, 2, 5, 0], [True, True, False, False, True, True, False, False])], ids=["B1", "B3", "B8"])
def test_resident_rows_of_both_views_equal_the_pipeline(cuda, small, indices, flags):
    """2. `ResidentSplit.batch` over 2 N views == `DeviceInputPipeline` on the same frames, samples and flags, bit for bit: left
    and right views of one image in one batch, a repeated row, indices N - 1, N and 2 N - 1."""
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    cfg, split = small["cfg"], small["split"]
    N = len(split) // 2
    assert N == 3 and len(split) == 6
    if len(indices) > 1:
        assert {N - 1, N, 2 * N - 1} <= set(indices)
    ids = [small["files"].img_id(i) for i in indices]
    got = split.batch(indices, flags, img_ids=ids)
    frames, samples = [small["frames"][i] for i in indices], [small["samples"][i] for i in indices]
    want = DeviceInputPipeline(cfg, cuda)(frames, samples, ids, flip=flags)
    assert_same_batch(got, want, (indices, flags))
    ref = IH.restate_images(frames, flags, 32, 96, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR)
    assert torch.equal(got[0].cpu(), ref)
    if len(indices) == 8:                                                      # the two views of image 0 are different rows
        assert ids[0] == ids[1] and not torch.equal(got[0][0], got[0][1])
        assert not np.array_equal(got[1][0].get_field("calib").P, got[1][1].get_field("calib").P)
    with pytest.raises(IndexError):
        split.batch([2 * N], [False])


def test_resident_byte_count_covers_both_cameras(cuda, small):
    """The byte count, and with it the `max_bytes` refusal, is that of 2 N frames and 4 N table rows."""
    from dcd_amd import _lib
    from dcd_amd.config import get_cfg
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    split = small["split"]
    left_cfg = get_cfg(opts=SMALL[:8])
    left = ResidentSplit(KittiFiles(RH.RIGHT_ROOT, "train", left_cfg, is_train=True), left_cfg, cuda, workers=2)
    assert len(left) == 3 and split.frame_bytes == 2 * left.frame_bytes == split.frames.numel()
    assert split.nbytes == 2 * left.nbytes and all(t.shape[0] == 12 for t in split._tables)
    assert split.frame_bytes >= sum(f.size for f in small["frames"])
    with pytest.raises(_lib.DcdHipError, match=str(split.nbytes)):
        ResidentSplit(small["files"], small["cfg"], cuda, max_bytes=split.nbytes - 1)


def test_two_real_iterations_with_both_cameras(cuda, full, tmp_path, caplog):
    """3. `do_train` for two iterations of batch 2 over the 2 N views: the sampler's first two batches reach into the right half,
    the logged losses are finite, and `model_final` loads."""
    from dcd_amd.data.batches import Prefetcher, ResidentBatches
    from dcd_amd.engine.train import do_train, resume
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler
    from dcd_amd.model.detector import KeypointDetector
    cfg, model, split = full["cfg"], full["model"], full["split"]
    N, seed = len(split) // 2, 0
    source = ResidentBatches(split, 2, seed=seed)
    assert len(source) == 2 * N == 6
    drawn = [i for k in range(2) for i in ResidentBatches(split, 2, seed=seed).plan(k)[0]]
    assert len(drawn) == 4 and any(i >= N for i in drawn) and all(0 <= i < 2 * N for i in drawn), drawn
    optimizer = build_optimizer(model, cfg)
    scheduler, warmup = build_scheduler(optimizer, cfg)
    with caplog.at_level(logging.INFO, logger="dcd_amd.trainer"):
        args = do_train(cfg, model, optimizer, scheduler, warmup, Prefetcher(source, cuda), {"iteration": 0}, str(tmp_path))
    assert args["iteration"] == 2
    line = [r.getMessage() for r in caplog.records if "iter: 2" in r.getMessage()][-1]
    logged = {k: float(v) for k, v in re.findall(r"(\S+): (\S+) \(", line)}
    losses = {k: v for k, v in logged.items() if "loss" in k}
    assert "loss" in losses and "hm_loss" in losses and len(losses) >= 8 and all(math.isfinite(v) for v in losses.values()), line
    assert losses["loss"] > 0
    torch.manual_seed(1)
    fresh = KeypointDetector(cfg).to(cuda).train()
    loaded = resume(os.path.join(str(tmp_path), "model_final.pth"), fresh)
    assert loaded["iteration"] == 2
    final, got = model.state_dict(), fresh.state_dict()
    assert set(got) == set(final)
    for k in final:
        assert torch.equal(got[k], final[k]), k


def test_record_collection_keeps_both_views_of_an_image(cuda, full):
    """4. `collect_gmw_records` over the six views in order (three batches of two): the records are counted per row, so the two
    rows that share an image id both keep theirs -- the total is the sum over the six rows of the objects their targets mark."""
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.engine.train import collect_gmw_records
    cfg, model, split, files = full["cfg"], full["model"], full["split"], full["files"]
    N = len(split) // 2
    per_row = [int(split.batch([i], [False])[1][0].get_field("reg_mask").sum()) for i in range(2 * N)]
    assert all(n >= 1 for n in per_row)
    records = collect_gmw_records(model, ResidentBatches(split, 2, seed=0, is_train=False), N, cfg=cfg)
    rows = records.collector.images().cpu().tolist()
    assert len(records) == len(rows) == sum(per_row)
    assert [rows.count(i) for i in range(2 * N)] == per_row                    # by row number: 0 and N are one id, two sets of records
    assert files.img_id(0) == files.img_id(N) and rows.count(0) > 0 and rows.count(N) > 0
    by_id = {}
    for i in range(2 * N):
        by_id[files.img_id(i)] = by_id.get(files.img_id(i), 0) + per_row[i]
    assert len(by_id) == N and sum(by_id.values()) == len(records) > max(sum(per_row[:N]), sum(per_row[N:]))
    names = [n for call in records.collector.gen_data()["img_idx"] for n in call]       # the file's lists keep both views too
    assert len(names) == len(records) and names.count(files.img_id(0)) == per_row[0] + per_row[N]


def _labelled_twin(src, dst):
    """The unlabelled directory once more as a labelled split whose images hold no object: `label_2` files with one 'DontCare'
    line and empty key-point annotations."""
    shutil.copytree(src, dst)
    os.makedirs(os.path.join(dst, "label_2"))
    os.makedirs(os.path.join(dst, "kpts_ann"))
    with open(os.path.join(dst, "ImageSets", "test.txt")) as f:
        ids = [line.strip() for line in f if line.strip()]
    shutil.copy(os.path.join(dst, "ImageSets", "test.txt"), os.path.join(dst, "ImageSets", "val.txt"))
    for i in ids:
        with open(os.path.join(dst, "label_2", i + ".txt"), "w") as f:
            f.write("DontCare -1 -1 -10 10.00 10.00 20.00 20.00 -1 -1 -1 -1000 -1000 -1000 -10\n")
    with open(os.path.join(dst, "kpts_ann", "kpts_ann_val.json"), "w") as f:
        json.dump({str(int(i)): [] for i in ids}, f)
    return ids


def test_inference_over_a_split_without_labels(cuda, world, tmp_path):  # noqa: F811
    """5. Four images, batch 3 (one full batch and the ragged tail), detector and GMW in one pass: {"gmw": {}}, both folders hold
    exactly the split's ids, and the detector's files equal, byte for byte, those of the same frames presented as a labelled
    split without objects."""
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import inference
    cfg, model, gmw, pipe = world["cfg"], world["model"], world["gmw"], world["pipe"]
    root = str(tmp_path / "testing")
    for d in ("ImageSets", "calib", "image_2"):
        shutil.copytree(os.path.join(RH.RIGHT_ROOT, d), os.path.join(root, d))
    files = KittiFiles(root, "test", cfg, is_train=False)
    ids = [files.img_id(i) for i in range(len(files))]
    assert len(ids) == 4 and not files.has_labels
    out = str(tmp_path / "out")
    assert inference(model, files, pipe, out, batch_size=3, gmw=gmw) == {"gmw": {}}
    assert sorted(os.listdir(out)) == ["data", "kitti_results_for_eval"]
    names = [i + ".txt" for i in ids]
    assert sorted(os.listdir(os.path.join(out, "data"))) == sorted(os.listdir(os.path.join(out, "kitti_results_for_eval"))) == names
    twin_root = str(tmp_path / "labelled")
    assert _labelled_twin(root, twin_root) == ids
    twin = KittiFiles(twin_root, "val", cfg, is_train=False)
    assert twin.has_labels and [twin.img_id(i) for i in range(len(twin))] == ids
    twin_out = str(tmp_path / "twin")
    scored = inference(model, twin, pipe, twin_out, batch_size=3, gmw=gmw)
    assert "R40" in scored and "R40" in scored["gmw"]
    rows = 0
    for n in names:
        for folder in ("data", "kitti_results_for_eval"):
            a, b = open(os.path.join(out, folder, n), "rb").read(), open(os.path.join(twin_out, folder, n), "rb").read()
            assert a == b, (folder, n)
        rows += len(open(os.path.join(out, "data", n)).read().split("\n")) - 1
    assert rows == 4 * cfg.TEST.DETECTIONS_PER_IMG                               # threshold 0: the files are not empty ones
    assert world["model"].heads.predictor.sparse_eval_heads is False and gmw.training is False
    # the records of the same pass need no labels either (`--gen-data` on the test split)
    gen = str(tmp_path / "gen")
    assert inference(model, files, pipe, str(tmp_path / "out_gen"), batch_size=3, gen_out_dir=gen) == {}
    infer = json.load(open(os.path.join(gen, "gen_data_infer.json")))
    assert sorted(infer) == ids and sum(len(v) for v in infer.values()) == rows
    for n in names:
        assert open(os.path.join(str(tmp_path / "out_gen"), "data", n), "rb").read() == open(os.path.join(out, "data", n), "rb").read()
