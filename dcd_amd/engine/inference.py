"""From a KITTI directory to the AP table: the use DGDE/engine/inference.py:19-125 makes of the model, the result writer and
the evaluator.  One image per model call, as the reference runs its evaluation (TEST.IMS_PER_BATCH = 1); every image's
`PostProcessor` rows go to `<output_folder>/data/<id>.txt`, then the files are read back and evaluated against `label_2`
on the device.

With `batch_size > 1` or `gen_out_dir` the split is walked in batches instead (`_batched_pass`): frames decoded by a thread
pool, batch k + 1 prepared on a side stream while batch k runs, backbone -> predictor (heads at the top-K cells only) ->
`PostProcessor.decode_fused` (ONE kernel for the whole decode of the batch), the outputs copied to pinned host memory
asynchronously, and the host cuts each image's rows at the score threshold and writes its file while the next batch runs.
The loop never waits on one image: its only waits are one event per batch, a batch late.  With `gen_out_dir` the same pass
also collects the GMW records (`gen_data_infer.json`).

With `gmw=` (a `dcd_amd.gmw.GMW` model) the same pass is the whole two-stage system: the kept candidates of every image batch
stay on the device, `gmw.RecordRefiner` gathers them into GMW's input layout (`ops.gmw_pack_records`) and refines them in groups
of `gmw_batch`, and after the last batch the refined files go to `<output_folder>/kitti_results_for_eval` and are scored; the
result is `results["gmw"]`.  No `gen_data_infer.json` lies between the stages.

With `render_dir=` the same pass also leaves `<render_dir>/<id>.png` for every image: the frame with the kept detections' 2-D
boxes, projected 3-D boxes and labels (with `render_keypoints` the dense key points too) over the ground truth, and a bird's-eye
panel beside it -- drawn on the device from the decode's outputs and the staged frames (`dcd_amd.engine.render`),
copied out once per batch and PNG-encoded by a thread pool.  Rows under TEST.DETECTIONS_THRESHOLD, rows an NMS suppressed and rows
whose score is not above TEST.VISUALIZE_THRESHOLD are not drawn; with `gmw=` the pictures show the detector's rows.

    python -m dcd_amd.engine.inference --root DIR --split val --ckpt FILE --output-dir OUT [--batch N] [--gen-data]
                                       [--gmw-ckpt FILE [--gmw-batch N]] [--render-dir DIR [--render-keypoints]]
                                       [--tta [--tta-match 2d|bev|3d] [--tta-thresh X] [--tta-unmatched X]] [KEY VALUE ...]

evaluates a saved checkpoint (or, with --gmw-ckpt, a detector and a GMW checkpoint together) on its own.  `--split test` reads
`ImageSets/test.txt`, the images and `calib` only and writes one result file per id, in `inference/data` and, with --gmw-ckpt,
in `inference/kitti_results_for_eval`: the files of a leaderboard entry.  Nothing is scored then and the printed result is `{}`
or `{"gmw": {}}`.  `DATASETS.INFER_ON_RIGHT_IMG True` runs either kind of split on `image_3` with `P3`.

With `tta=` (a `TTASpec`; `--tta`, or DATASETS.USE_TTA True for the default spec) the batched pass sees every image twice, as it is
and mirrored: the 2 B records of a batch name B staged frames, the decode runs on 2 B images with each view's own P, and one
launch (`ops.tta_merge_detections`) un-mirrors the second view's rows, matches them to the first's and fuses the pairs, before
TEST.USE_NMS and everything after it.  A detection the mirrored view does not confirm keeps its box and loses part of its score;
a detection only the mirrored view has is dropped, because the key points that GMW and the records need exist in the frame's own
view only."""
import logging
import os

import numpy as np
import torch

from dcd_amd.engine.passes import load_detector, load_gmw, parse_overrides, restored_modes
from dcd_amd.eval import kitti_annos, kitti_ap


class TTASpec:
    """How the mirrored view's detections are merged into the frame's (DESIGN.md "Mirrored-view test-time augmentation";
    `ops.tta_merge_detections`): mode, the overlap a pair is matched by ('2d', 'bev' or '3d'); match_thresh in [0, 1), the overlap a
    pair must exceed; unmatched_scale in [0, 1], what the scores of a candidate without a partner are multiplied by."""

    def __init__(self, mode='2d', match_thresh=0.5, unmatched_scale=0.5):
        if mode not in ('2d', 'bev', '3d'):
            raise ValueError("TTA match mode %r: one of '2d', 'bev', '3d'" % (mode,))
        match_thresh, unmatched_scale = float(match_thresh), float(unmatched_scale)
        if not 0.0 <= match_thresh < 1.0:
            raise ValueError("TTA match threshold %r: 0 <= threshold < 1" % (match_thresh,))
        if not 0.0 <= unmatched_scale <= 1.0:
            raise ValueError("TTA unmatched scale %r: 0 <= scale <= 1" % (unmatched_scale,))
        self.mode, self.match_thresh, self.unmatched_scale = mode, match_thresh, unmatched_scale

    def __repr__(self):
        return "TTASpec(mode=%r, match_thresh=%r, unmatched_scale=%r)" % (self.mode, self.match_thresh, self.unmatched_scale)

    def __eq__(self, other):
        return isinstance(other, TTASpec) and repr(self) == repr(other)

    __hash__ = None


def resolve_tta(cfg, tta=None):
    """The spec a pass runs with: `tta` when given, the default spec when DATASETS.USE_TTA is set, else None (no TTA code runs).
    DATASETS.TTA_AUG_PARAMS keeps its one meaning -- more than one entry is the reference's multi-scale resize, which the
    input pipeline refuses -- and its probability entry is not read: with TTA every image is seen both ways."""
    if tta is not None:
        if not isinstance(tta, TTASpec):
            raise TypeError("tta: a TTASpec or None, not %r" % (tta,))
        return tta
    return TTASpec() if cfg is not None and bool(cfg.DATASETS.USE_TTA) else None


def _widths(targets, device, cache):
    """(B,) int32 on the device: every image's own width, from the targets' host-side "image_size"; one copy per distinct set of
    values (cached by value, as `PostProcessor._image_table`)."""
    host = np.array([int(t.get_field("image_size")[0]) for t in targets], np.int32)
    key = (host.tobytes(), str(device))
    if cache.get("key") != key:
        cache["key"], cache["widths"] = key, torch.as_tensor(host).to(device, non_blocking=True)
    return cache["widths"]


def keep_prefix(raw_scores, threshold):
    """How many of an image's candidates stay: the raw scores come out of the top-K in descending order, so the rows with
    score >= threshold are a prefix; returns its length (the first score below the threshold ends it)."""
    below = ~(np.asarray(raw_scores) >= threshold)                     # (a NaN score is not kept, as `scores >= threshold` drops it)
    return int(below.argmax()) if below.any() else len(below)


def write_image_rows(rows, raw_scores, threshold, path):
    """One image's decoded candidates (K, 14) -> its result file: the prefix at or above the threshold (an empty file when none).
    Returns the number of rows kept."""
    n = keep_prefix(raw_scores, threshold)
    kitti_annos.write_detections(np.asarray(rows)[:n], path)
    return n


def _records(rows, k2, k3, cat="Car"):
    """The kept rows of one image in `gen_data.infer_records_batch`'s record layout (numpy views of copies of the pinned slot)."""
    return [{'kpts_2d': k2[i], 'kpts_3d': k3[i], 'pred_rot': r[12:13], 'box': r[2:6], 'dim': r[6:9], 'pred_location': r[9:12],
             'score': r[13:14], 'cat': cat} for i, r in enumerate(rows)]


def _batched_pass(model, files, pipeline, predict_folder, batch_size, workers, want_records, refiner=None, renderer=None, tta=None):
    """The batched loop.  Returns {img_id: records} (empty without `want_records`).  Raises NotImplementedError, before anything
    runs, when the configuration is one `decode_fused` does not cover.  refiner: a `gmw.RecordRefiner`; the decode then always
    leaves the key points on the device, every batch's kept rows are handed to it (`refiner.add`, a batch late, with the host
    rows appended to `refiner.host_rows` / `refiner.host_ids` for the writer), and the key points go to the host only with
    `want_records`.  renderer: a `dcd_amd.engine.render.Renderer`; the walker then keeps the staged frames with the targets and every
    batch is drawn right after its decode (`renderer.add`); a renderer that draws key points makes the decode leave them on the
    device as the refiner does.  tta: a `TTASpec`; every batch then goes through the model as 2 B images -- the frames and their
    mirrored views, staged once -- and `ops.tta_merge_detections` brings the 2 B decoded blocks back to B before TEST.USE_NMS and
    everything else, which see merged blocks with the same prefix contract."""
    from dcd_amd.data.batches import eval_batches
    pp, predictor = model.heads.post_processor, model.heads.predictor
    spec = pp.decode_spec()                                            # refuses here, before the walker and its threads exist
    K, nk = pp.max_detection, spec["nk"]
    width = 18 + (nk * 5 if want_records else 0)                       # rows (14) | aux (4) | kpts_2d | kpts_3d
    threshold = pp.det_threshold
    slots = [torch.empty((batch_size * K, width), dtype=torch.float32).pin_memory() for _ in range(2)]
    views = [s.numpy() for s in slots]
    events = [torch.cuda.Event() for _ in range(2)]
    infer_data = {}

    def finish(k, ids, device_out):
        """Host side of batch k, run while batch k + 1 is on the device."""
        events[k % 2].synchronize()
        host = views[k % 2]
        kept_src = []
        for b, img_id in enumerate(ids):
            block = host[b * K:(b + 1) * K]
            n = write_image_rows(block[:, :14], block[:, 14], threshold, os.path.join(predict_folder, img_id + ".txt"))
            if refiner is not None:
                kept_src.extend(range(b * K, b * K + n))
                refiner.host_rows.append(block[:n, :14].copy())
                refiner.host_ids.extend([img_id] * n)
            if want_records:
                kept = block[:n].copy()                                # (the slot is overwritten two batches later)
                infer_data[img_id] = _records(kept[:, :14], kept[:, 18:18 + nk * 2].reshape(n, nk, 2),
                                              kept[:, 18 + nk * 2:].reshape(n, nk, 3))
        if refiner is not None:
            refiner.add(*device_out, kept_src)                          # (batch k's device tensors are let go after this)

    sparse_before = predictor.sparse_eval_heads
    predictor.sparse_eval_heads = True
    try:
        keep = {"keep_frames": True} if renderer is not None else {}
        if tta is not None:
            from dcd_amd import ops
            keep["mirrored"] = True
            width_cache = {}
        device_records = want_records or refiner is not None or (renderer is not None and renderer.keypoints)
        with eval_batches(files, pipeline, batch_size, workers, **keep) as walk:
            pending = None
            for k, indices, images, targets in walk:
                feats = model.backbone(images)
                preds = predictor(feats, targets)
                if tta is None:
                    rows, aux, recs = pp.decode_fused(preds, targets, test=model.test, records=device_records)
                else:
                    rows, aux, recs = pp.decode_fused(preds, targets, test=model.test, records=device_records, nms=False)
                    targets = targets[:len(indices)]                     # the frames as they are: what everything below works on
                    k2, k3 = recs if recs is not None else (None, None)
                    rows, aux, k2, k3 = ops.tta_merge_detections(rows, aux, k2, k3, K, _widths(targets, rows.device, width_cache), tta.mode,
                                                                 tta.match_thresh, threshold, tta.unmatched_scale)[:4]
                    rows, aux, k2, k3 = pp.nms_fused(rows, aux, k2, k3, K)
                    recs = (k2, k3) if recs is not None else None
                if renderer is not None:
                    renderer.add(k, [files.img_id(i) for i in indices], targets[0].get_field("frames"), rows, aux, recs,
                                 pp._image_table(targets, rows.device), targets)
                n = rows.shape[0]
                parts = [rows, aux] + ([recs[0].reshape(n, nk * 2), recs[1].reshape(n, nk * 3)] if want_records else [])
                slots[k % 2][:n].copy_(torch.cat(parts, dim=1), non_blocking=True)
                events[k % 2].record()
                if pending is not None:
                    finish(*pending)
                pending = (k, [files.img_id(i) for i in indices], (rows, recs[0], recs[1]) if refiner is not None else None)
            if pending is not None:
                finish(*pending)
    finally:
        predictor.sparse_eval_heads = sparse_before
    return infer_data


def inference(model, files, pipeline, output_folder, metrics=("R40",), batch_size=1, workers=None, gen_out_dir=None, gmw=None,
              gmw_batch=256, render_dir=None, render_keypoints=False, tta=None):
    """model: a `KeypointDetector`; files: a `KittiFiles`; pipeline: a `DeviceInputPipeline(is_train=False)`.
    batch_size = 1 and gen_out_dir = None: one image per model call, as the reference.  Otherwise the batched pass (see the
    module docstring); gen_out_dir: where the same pass leaves `gen_data_infer.json`.  A configuration the fused decode does
    not cover (head-axis orientation, ...) falls back to the one-image loop, and to `generate_infer_data` for the records.
    gmw: a `dcd_amd.gmw.GMW` model on the pipeline's device: the pass is then always the batched one, the kept candidates are
    refined on the device in groups of `gmw_batch` (the partition `gmw.refine(data, batch_size=gmw_batch)` makes of the same
    records), `<output_folder>/kitti_results_for_eval` gets the files of `gmw.write_results` (class "Car", one file per id of
    the split) and their tables are `results["gmw"] = {metric: dict}`.  With `gmw` a configuration the fused decode does not
    cover is an error (NotImplementedError): no other route can feed the second stage.
    render_dir: where the pass leaves one picture per id, `<render_dir>/<id>.png` (`dcd_amd.engine.render`): the pass is then always
    the batched one and, as with `gmw`, a configuration the fused decode refuses is an error.  render_keypoints: draw the dense key
    points as well.  An unlabelled split draws no ground truth.  With render_dir = None nothing of this is launched, allocated or kept.
    tta: a `TTASpec`, or None with DATASETS.USE_TTA True for the default one: mirrored-view test-time augmentation.  The pass is
    then always the batched one; every image is decoded as it is and mirrored (the mirrored records name the same staged pixels),
    and the two views' candidates are merged on the device before TEST.USE_NMS, `gmw`, `gen_out_dir` and `render_dir`, which work
    on the merged blocks unchanged.  A configuration the fused decode refuses is an error.  With tta = None and USE_TTA False
    nothing of this is launched, allocated or packed.
    Returns {metric: the dict of `kitti_ap.official_eval`}.
    A `files` whose `has_labels` is false (KITTI's `test` split; an object without the attribute counts as labelled) goes through
    the same pass and only leaves its files behind: see `finish_pass`."""
    if pipeline.is_train:
        raise ValueError("inference needs a DeviceInputPipeline(is_train=False): evaluation never flips")
    if batch_size < 1:
        raise ValueError("batch size %d" % batch_size)
    logger = logging.getLogger("dcd_amd.inference")
    predict_folder = os.path.join(output_folder, "data")
    os.makedirs(predict_folder, exist_ok=True)
    ids = [files.img_id(i) for i in range(len(files))]
    with restored_modes(model, gmw), torch.no_grad():
        model.eval()
        tta = resolve_tta(getattr(model, "cfg", None), tta)                # (a model without a configuration: the argument alone)
        batched = batch_size > 1 or gen_out_dir is not None or gmw is not None or render_dir is not None or tta is not None
        refiner = renderer = None
        if render_dir is not None:
            from dcd_amd.engine.render import Renderer
            renderer = Renderer(model.cfg, pipeline.device, keypoints=render_keypoints,
                                render_dir=render_dir, workers=workers, labelled=getattr(files, "has_labels", True))
        if gmw is not None:
            from dcd_amd.gmw.inference import RecordRefiner
            gmw.eval()
            refiner = RecordRefiner(gmw, pipeline.device, batch_size=gmw_batch, nk=model.heads.post_processor.extra_kpts_num + 10)
        if batched:
            try:
                extra = {"renderer": renderer} if renderer is not None else {}
                if tta is not None:
                    extra["tta"] = tta
                try:
                    infer_data = _batched_pass(model, files, pipeline, predict_folder, batch_size, workers, gen_out_dir is not None,
                                               refiner, **extra)
                finally:
                    if renderer is not None:
                        renderer.finish()
                if gen_out_dir is not None:
                    from dcd_amd.engine import gen_data
                    gen_data.dump_gen_data_infer(infer_data, gen_out_dir)
            except NotImplementedError as e:
                if gmw is not None:
                    raise NotImplementedError("inference(gmw=...) needs the fused decode, which refuses this configuration: %s" % e)
                if renderer is not None:
                    raise NotImplementedError("inference(render_dir=...) needs the fused decode, which refuses this configuration: %s" % e)
                if tta is not None:
                    raise NotImplementedError("inference with TTA (tta=... / DATASETS.USE_TTA) needs the fused decode, which refuses "
                                              "this configuration: %s" % e)
                logger.info("batched evaluation is not available (%s): one image per call", e)
                batched = False
                if gen_out_dir is not None:
                    from dcd_amd.engine.train import generate_infer_data
                    generate_infer_data(model, files, pipeline, gen_out_dir)
        if not batched:
            for i, img_id in enumerate(ids):
                images, targets = pipeline([files.frame(i)], [files.sample(i)], img_ids=[img_id])
                rows = model(images, targets)[0]
                kitti_annos.write_detections(rows, os.path.join(predict_folder, img_id + ".txt"))
        if refiner is not None:
            pred_location = refiner.finish()
    refined = None
    if refiner is not None:
        rows = np.concatenate(refiner.host_rows, 0) if refiner.host_rows else np.zeros((0, 14), np.float32)
        refined = (rows, refiner.host_ids, pred_location)
    return finish_pass(files, ids, output_folder, metrics, pipeline.device, refined)


def finish_pass(files, ids, output_folder, metrics, device, refined=None):
    """The host half that follows the pass over the split: `<output_folder>/data` holds the detector's files by now.
    refined: (rows (n, 14) float32 on the host, each row's image id, the refined locations (n, 3)) of a pass with `gmw`; the files
    of `gmw.write_results` then go to `<output_folder>/kitti_results_for_eval`, one per id of the split.
    A labelled split is scored against `label_2`: {metric: dict}, and `results["gmw"] = {metric: dict}` for the refined files.
    A split without labels (`files.has_labels` false: KITTI's `test`) is only written: every id must have its file in `data`
    (an empty one where nothing passed the threshold), no label file is opened, nothing is scored, and the result is {} -- with
    `refined`, {"gmw": {}} -- which is what the reference's `--test` / `--test_all` leave behind for the upload."""
    logger = logging.getLogger("dcd_amd.inference")
    predict_folder = os.path.join(output_folder, "data")
    labelled = getattr(files, "has_labels", True)
    results = {}
    if labelled:
        dt_annos = kitti_annos.read_annos(predict_folder, ids)
        gt_annos = kitti_annos.read_annos(os.path.join(files.root, "label_2"), ids)
        for metric in metrics:
            text, results[metric] = kitti_ap.official_eval(gt_annos, dt_annos, list(files.classes), metric=metric, device=device)
            logger.info("%s\n%s", metric, text)
    else:
        missing = [i for i in ids if not os.path.isfile(os.path.join(predict_folder, i + ".txt"))]
        if missing:
            raise RuntimeError("the pass left no result file for %d of %d ids (first: %s)" % (len(missing), len(ids), missing[0]))
        logger.info("%d result files in %s; the split has no labels, nothing is scored", len(ids), predict_folder)
    if refined is not None:
        from dcd_amd.gmw.inference import write_results, writer_fields
        rows, host_ids, pred_location = refined
        result_dir = write_results(writer_fields(rows, host_ids), pred_location, os.path.join(output_folder, "kitti_results_for_eval"), ids)
        results["gmw"] = {}
        if labelled:
            refined_annos = kitti_annos.read_annos(result_dir, ids)
            for metric in metrics:                                     # class 0, "Car": the one name GMW's files carry
                text, results["gmw"][metric] = kitti_ap.official_eval(gt_annos, refined_annos, 0, metric=metric, device=device)
                logger.info("GMW %s\n%s", metric, text)
    return results


def add_tta_arguments(ap):
    ap.add_argument("--tta", action="store_true", help="mirrored-view test-time augmentation: decode every image as it is and "
                    "mirrored, merge the two on the device (also switched on by DATASETS.USE_TTA True)")
    ap.add_argument("--tta-match", choices=("2d", "bev", "3d"), default=None, help="with --tta: the overlap pairs are matched by (2d)")
    ap.add_argument("--tta-thresh", type=float, default=None, help="with --tta: the overlap a pair must exceed (0.5)")
    ap.add_argument("--tta-unmatched", type=float, default=None, help="with --tta: the factor on the scores of a detection the "
                    "mirrored view does not confirm (0.5)")


def tta_from_arguments(ap, args):
    """The `TTASpec` of the command line, or None without --tta (DATASETS.USE_TTA then decides, with the default spec)."""
    given = {k: v for k, v in (("mode", args.tta_match), ("match_thresh", args.tta_thresh), ("unmatched_scale", args.tta_unmatched))
             if v is not None}
    if not args.tta:
        if given:
            ap.error("--tta-match / --tta-thresh / --tta-unmatched need --tta")
        return None
    try:
        return TTASpec(**given)
    except ValueError as e:
        ap.error(str(e))


def main(argv=None):
    """`python -m dcd_amd.engine.inference --root KITTI_DIR --split val --ckpt FILE --output-dir OUT [--batch N] [--gen-data]
    [--gmw-ckpt FILE [--gmw-batch N]] [--render-dir DIR [--render-keypoints]] [KEY VALUE ...]`: evaluate a saved checkpoint (a file, or a directory with `last_checkpoint`) on one GPU."""
    import argparse
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--root", required=True, help="KITTI directory: ImageSets, image_2, label_2, calib, kpts_ann (for --split test: "
                    "ImageSets, image_2, calib)")
    ap.add_argument("--split", default="val", help="ImageSets/<split>.txt; 'test' is the split without labels: written, not scored")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--batch", type=int, default=1, help="images per model call (1: the one-image loop)")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--gen-data", action="store_true", help="also write gen_data/gen_data_infer.json from the same pass")
    ap.add_argument("--gmw-ckpt", default=None, help="a GMW checkpoint (checkpoint_epoch_N.pth.tar of dcd_amd.gmw.train): refine the "
                    "kept detections in the same pass and score the refined files as well")
    ap.add_argument("--gmw-batch", type=int, default=256, help="records per refinement call")
    ap.add_argument("--render-dir", default=None, help="also leave one picture per image here, <id>.png: detections over ground truth "
                    "and a bird's-eye panel, drawn on the device in the same pass")
    ap.add_argument("--render-keypoints", action="store_true", help="with --render-dir: draw the dense key points too")
    add_tta_arguments(ap)
    ap.add_argument("opts", nargs="*", help="configuration overrides: KEY VALUE ...")
    args = ap.parse_args(argv)
    if args.render_keypoints and not args.render_dir:
        ap.error("--render-keypoints needs --render-dir")
    tta = tta_from_arguments(ap, args)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(name)s %(message)s")
    cfg = get_cfg(opts=parse_overrides(args.opts))
    device = torch.device("cuda", torch.cuda.current_device())
    model, _ = load_detector(cfg, args.ckpt, device)
    gmw = load_gmw(args.gmw_ckpt, device) if args.gmw_ckpt else None
    files = KittiFiles(args.root, args.split, cfg, is_train=False)
    pipeline = DeviceInputPipeline(cfg, device, is_train=False)
    gen_out_dir = os.path.join(args.output_dir, "gen_data") if args.gen_data else None
    results = inference(model, files, pipeline, os.path.join(args.output_dir, "inference"), metrics=tuple(cfg.TEST.METRIC),
                        batch_size=args.batch, workers=args.workers, gen_out_dir=gen_out_dir, gmw=gmw, gmw_batch=args.gmw_batch,
                        render_dir=args.render_dir, render_keypoints=args.render_keypoints, tta=tta)

    def plain(v):
        return {k: plain(x) for k, x in v.items()} if isinstance(v, dict) else (v.tolist() if hasattr(v, "tolist") else v)
    print(json.dumps(plain(results), default=str))
    return results


if __name__ == "__main__":
    main()
