"""Which head loses the 3-D overlap: the disentangled IoU report (the MonoDIS / MonoFlex test the reference names with
`TEST.EVAL_DIS_IOUS` and never defines) at the labelled objects of a KITTI split, by class and range bin.

At every labelled object the pass builds fifteen boxes in which ONE component is the prediction's and the rest is the label's
(`ops.DIS_VARIANTS`: full, location, offset, dims, orient, and depth:<m> for the ten `ops.DEPTH_METHODS`) and measures each box's
BEV and 3-D IoU with the label, by the KITTI evaluator's own arithmetic.  A component whose box keeps IoU ~ 1 costs nothing; the one
whose box falls below the class's AP threshold is the one to work on.  Like the depth report it asks at the GROUND-TRUTH centres --
no top-K, no threshold, no matching --

    backbone -> predictor.heads_at(the targets' `target_centers`) -> [GMW's depth of every slot] -> ops.dis_iou_estimates
             -> ops.dis_iou_accumulate

per batch, walked with `EvalPlan` and prepared one batch ahead.  The tables stay on the device; nothing is read back inside the
loop, and ONE copy brings them to the host at the end.  Every (class, bin, variant, metric) cell adds its objects in slot order in
double, and the backbone runs one image at a time by default (`backbone_batch`, for the depth report's reason), so the result has
the same bits for every batch size and from run to run.

A hit is IoU > threshold, the evaluator's comparison; `thresholds=None` takes each class's strict and loose pair from
`eval.kitti_ap.MIN_OVERLAPS` (rows 0 and 1, the BEV and 3-D columns).  With `gmw=` (a `dcd_amd.gmw.GMW` model) the `depth:gmw`
variant is placed at GMW's refined depth (`depth_report._GmwColumn`); without it that variant is NaN and its cells count non-finite
overlaps only.  When one of a variant's seven box numbers is not finite, or an overlap comes out non-finite, both overlaps of that
variant are NaN and are counted as such.

    python -m dcd_amd.engine.dis_iou_report --root KITTI --split val --ckpt OUT [--batch 8] [--backbone-batch 1]
                                            [--edges 0 10 20 ...] [--gmw-ckpt FILE [--gmw-batch N]] [--output-dir DIR] [KEY VALUE ...]

prints the table and, with --output-dir, writes `dis_iou_report.json` and `dis_iou_report.txt` there."""
import logging
import os

import numpy as np
import torch

from dcd_amd import ops
from dcd_amd.engine.depth_report import DEFAULT_EDGES, MAX_SLOTS, _GmwColumn
from dcd_amd.engine.passes import load_detector, load_gmw, parse_overrides, restored_modes
from dcd_amd.structures.params_3d import stack_field


def default_thresholds(num_classes):
    """(num_classes, 2, 2) nested lists: per class and metric (bev, 3d) the strict and the loose threshold of KITTI's evaluator."""
    from dcd_amd.eval.kitti_ap import MIN_OVERLAPS
    if num_classes > MIN_OVERLAPS.shape[2]:
        raise ValueError("%d classes: the evaluator has thresholds for %d; pass thresholds=" % (num_classes, MIN_OVERLAPS.shape[2]))
    return [[[float(MIN_OVERLAPS[0, 1 + k, c]), float(MIN_OVERLAPS[1, 1 + k, c])] for k in range(len(ops.DIS_METRICS))]
            for c in range(num_classes)]


def report_batch(model, images, targets, spec, edges, thresholds, table, outside, gmw_column=None, backbone_batch=1):
    """The loop body: one batch's rows (B M, 33), booked into `table` / `outside` in place.  Everything is enqueued on the
    current stream and nothing is read back.  backbone_batch: images per backbone call (None: the whole batch in one)."""
    pp, predictor = model.heads.post_processor, model.heads.predictor
    B = images.shape[0]
    if backbone_batch is None or backbone_batch >= B:
        feats = model.backbone(images)
    else:
        feats = torch.cat([model.backbone(images[s:s + backbone_batch]) for s in range(0, B, backbone_batch)])
    centers = stack_field(targets, "target_centers")                   # (B, M, 2) cells (x, y)
    if centers.shape[1] > MAX_SLOTS:
        raise NotImplementedError("dis_iou_report: %d object slots per image (%d at most)" % (centers.shape[1], MAX_SLOTS))
    xs, ys = centers[:, :, 0], centers[:, :, 1]
    lin = ys.long() * feats.shape[3] + xs.long()
    vectors = predictor.heads_at(feats, targets, lin)
    classes, valid = stack_field(targets, "cls_ids").float(), stack_field(targets, "reg_mask")
    gt = torch.cat((stack_field(targets, "offset_3D"), stack_field(targets, "locations"), stack_field(targets, "dimensions"),
                    stack_field(targets, "rotys").unsqueeze(-1)), dim=2).float()
    ys, xs = ys.float(), xs.float()
    image_table = pp._image_table(targets, vectors.device)
    gmw_z = None if gmw_column is None else gmw_column(vectors, lin, classes, ys, xs, image_table, spec)
    dis = ops.dis_iou_estimates(vectors, ys, xs, classes, gt, valid, image_table, spec, gmw_z=gmw_z)
    ops.dis_iou_accumulate(dis, edges, thresholds, table, outside)
    return dis


def summarise(table, outside, edges, classes, thresholds):
    """The host half: the (class, bin, variant, metric, stat) sums and the `outside` counts -> the result dict.  The extra last bin
    is "all": the per-bin sums added in bin order.  A cell without a finite overlap has NaN for the mean and the rates."""
    table = np.asarray(table, np.float64)
    total = table[:, 0].copy()
    for i in range(1, table.shape[1]):
        total = total + table[:, i]
    sums = np.concatenate((table, total[:, None]), axis=1)             # (class, bin + 1, variant, metric, stat)
    count = sums[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean, hit, hit_loose = sums[..., 1] / count, sums[..., 3] / count, sums[..., 4] / count
    return {"edges": [float(e) for e in edges], "classes": list(classes), "variants": list(ops.DIS_VARIANTS), "metrics": list(ops.DIS_METRICS),
            "thresholds": np.asarray(thresholds, np.float64), "mean_iou": mean, "hit_rate": hit, "hit_rate_loose": hit_loose,
            "count": count.astype(np.int64), "nonfinite": sums[..., 5].astype(np.int64), "outside": np.asarray(outside, np.int64).copy()}


def format_report(result):
    """The fixed-width table: one block per class and metric, one line per variant; the bins' mean IoU, then mean / both hit
    rates / n of the "all" bin (n: the objects with a finite overlap)."""
    edges = result["edges"]
    bins = ["%g-%g" % (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]

    def num(v):
        return "%8.3f" % v if np.isfinite(v) else "%8s" % "-"
    lines = []
    seen = result["count"][:, -1, 0, 0] + result["nonfinite"][:, -1, 0, 0] + result["outside"]
    for c, name in enumerate(result["classes"]):
        if seen[c] == 0 and seen.sum() > 0:
            continue                                                   # a class the split holds no object of
        objects = int(result["count"][c, -1, 0, 0] + result["nonfinite"][c, -1, 0, 0])
        for k, metric in enumerate(result["metrics"]):
            strict, loose = result["thresholds"][c, k]
            lines.append("%s, %s IoU: %d objects in the bins, %d outside [%g, %g)" % (name, metric, objects, int(result["outside"][c]),
                                                                                     edges[0], edges[-1]))
            lines.append("%-18s" % "mean IoU" + "".join("%8s" % b for b in bins) + "%8s%8s%8s%7s" % ("all", ">%g" % strict, ">%g" % loose, "n"))
            for v, variant in enumerate(result["variants"]):
                lines.append("%-18s" % variant + "".join(num(x) for x in result["mean_iou"][c, :, v, k])
                             + num(result["hit_rate"][c, -1, v, k]) + num(result["hit_rate_loose"][c, -1, v, k])
                             + "%7d" % int(result["count"][c, -1, v, k]))
            lines.append("")
    return "\n".join(lines)


def dis_iou_report(model, files, pipeline, batch_size=8, edges=DEFAULT_EDGES, gmw=None, gmw_batch=256, thresholds=None, per_object=False,
                   workers=None, backbone_batch=1):
    """model: a `KeypointDetector`; files: a labelled `KittiFiles`; pipeline: a `DeviceInputPipeline(is_train=False)`.
    backbone_batch: images per backbone call inside a batch; 1 (the default) makes the result the same bits for every `batch_size`
    and from run to run, None runs the backbone once per batch (see `depth_report`).
    thresholds: (class, 2, 2) -- per class and metric (bev, 3d) the strict and the loose IoU threshold, each in [0, 1]; None: the
    evaluator's `MIN_OVERLAPS`.
    Returns (text, result): result = {"edges", "classes", "variants", "metrics", "thresholds", and "mean_iou", "hit_rate",
    "hit_rate_loose", "count", "nonfinite" as arrays (class, bin + 1, variant, metric) whose last bin is "all", "outside" (class)};
    text is `format_report(result)`, logged as well.
    per_object=True adds result["dis"] (N, 33) -- every slot's row [valid, class, gt_z, bev[15], iou3d[15]] in split order, one bulk
    copy -- and result["img_ids"], each row's image id.
    Raises ValueError for a split without labels, NotImplementedError for a configuration the kernels do not cover."""
    from dcd_amd.data.batches import eval_batches
    if not getattr(files, "has_labels", True):
        raise ValueError("dis_iou_report needs a labelled split: %r has no labels to measure against" % getattr(files, "split", files))
    if pipeline.is_train:
        raise ValueError("dis_iou_report needs a DeviceInputPipeline(is_train=False): evaluation never flips")
    if batch_size < 1 or (backbone_batch is not None and backbone_batch < 1):
        raise ValueError("batch size %d, backbone batch %s" % (batch_size, backbone_batch))
    edges = [float(e) for e in edges]
    n_bins = len(edges) - 1
    if not 1 <= n_bins <= ops.DEPTH_MAX_BINS or any(not lo < hi for lo, hi in zip(edges[:-1], edges[1:])):
        raise ValueError("edges %s: 2 to %d increasing numbers" % (edges, ops.DEPTH_MAX_BINS + 1))
    logger = logging.getLogger("dcd_amd.dis_iou_report")
    pp = model.heads.post_processor
    spec = pp.decode_spec()                                            # refuses here, not in the middle of the split
    from dcd_amd.data.kitti_files import TYPE_ID_CONVERSION
    names = {v: k for k, v in TYPE_ID_CONVERSION.items() if v >= 0}
    classes = [names.get(c, "class %d" % c) for c in range(len(spec["dim_mean"]))]
    thresholds = default_thresholds(len(classes)) if thresholds is None else np.asarray(thresholds, np.float64).tolist()
    if np.asarray(thresholds).shape != (len(classes), len(ops.DIS_METRICS), 2) or not all(
            0.0 <= t <= 1.0 for t in np.asarray(thresholds).reshape(-1)):
        raise ValueError("thresholds %s: (%d classes, %d metrics, strict and loose), each in [0, 1]"
                         % (thresholds, len(classes), len(ops.DIS_METRICS)))
    device = pipeline.device
    table, outside = ops.dis_iou_tables(len(classes), n_bins, device)
    gmw_column = None
    kept, ids = [], []
    with restored_modes(model, gmw), torch.no_grad():
        model.eval()
        if gmw is not None:
            gmw.eval()
            gmw_column = _GmwColumn(gmw, device, gmw_batch, spec["nk"])
        with eval_batches(files, pipeline, batch_size, workers) as walk:
            for k, indices, images, targets in walk:
                dis = report_batch(model, images, targets, spec, edges, thresholds, table, outside, gmw_column, backbone_batch)
                if per_object:
                    kept.append(dis)
                    slots = dis.shape[0] // len(targets)
                    ids.extend(files.img_id(i) for i in indices for _ in range(slots))
        # the one copy: the sums and, as the same 8-byte words, the counters
        flat = torch.cat((table.reshape(-1), outside.view(torch.float64))).cpu().numpy()
        dis_host = torch.cat(kept).cpu().numpy() if kept else np.zeros((0, ops.DIS_ROW), np.float32)
    result = summarise(flat[:table.numel()].reshape(tuple(table.shape)), flat[table.numel():].view(np.int64), edges, classes, thresholds)
    if per_object:
        result["dis"], result["img_ids"] = dis_host, ids
    text = format_report(result)
    logger.info("disentangled IoU at the labelled objects of %d images\n%s", len(files), text)
    return text, result


def main(argv=None):
    """`python -m dcd_amd.engine.dis_iou_report --root KITTI_DIR --split val --ckpt FILE [--batch N] [--backbone-batch 1]
    [--edges 0 10 ...] [--gmw-ckpt FILE [--gmw-batch N]] [--output-dir DIR] [KEY VALUE ...]`: the disentangled IoU report of a saved
    checkpoint (a file, or a directory with `last_checkpoint`) on one GPU."""
    import argparse
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--root", required=True, help="KITTI directory: ImageSets, image_2, label_2, calib, kpts_ann")
    ap.add_argument("--split", default="val", help="ImageSets/<split>.txt; it must have labels")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--output-dir", default=None, help="where dis_iou_report.json and dis_iou_report.txt go (default: printed only)")
    ap.add_argument("--batch", type=int, default=8, help="images per model call; the result does not depend on it")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--backbone-batch", type=int, default=1, help="images per backbone call (1: the same bits for every --batch; "
                    "0: the whole batch in one call, faster, equal to about 1e-6)")
    ap.add_argument("--edges", nargs="+", default=None, metavar="M", help="range bin edges in metres, increasing (default %s)"
                    % " ".join(str(e) for e in DEFAULT_EDGES))
    ap.add_argument("--gmw-ckpt", default=None, help="a GMW checkpoint: place the `depth:gmw` variant at its refined depth")
    ap.add_argument("--gmw-batch", type=int, default=256, help="slots per refinement call")
    ap.add_argument("opts", nargs="*", help="configuration overrides: KEY VALUE ...")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.WARNING, format="%(asctime)s %(name)s %(message)s")

    def is_number(s):
        try:
            float(s)
            return True
        except ValueError:
            return False
    # `--edges 0 10 20 KEY VALUE ...`: the list ends at the first token that is not a number; the rest are the overrides
    edges = list(DEFAULT_EDGES)
    if args.edges is not None:
        n = next((i for i, s in enumerate(args.edges) if not is_number(s)), len(args.edges))
        edges, args.opts = [float(s) for s in args.edges[:n]], args.edges[n:] + args.opts
    cfg = get_cfg(opts=parse_overrides(args.opts))
    device = torch.device("cuda", torch.cuda.current_device())
    model, _ = load_detector(cfg, args.ckpt, device)
    gmw = load_gmw(args.gmw_ckpt, device) if args.gmw_ckpt else None
    files = KittiFiles(args.root, args.split, cfg, is_train=False)
    pipeline = DeviceInputPipeline(cfg, device, is_train=False)
    text, result = dis_iou_report(model, files, pipeline, batch_size=args.batch, edges=edges, gmw=gmw, gmw_batch=args.gmw_batch,
                                  workers=args.workers, backbone_batch=args.backbone_batch or None)
    print(text)
    if args.output_dir:
        os.makedirs(args.output_dir, exist_ok=True)

        def plain(v):
            if isinstance(v, np.ndarray):
                return plain(v.tolist())
            if isinstance(v, (list, tuple)):
                return [plain(x) for x in v]
            return None if isinstance(v, float) and not np.isfinite(v) else v
        with open(os.path.join(args.output_dir, "dis_iou_report.json"), "w") as f:
            json.dump({k: plain(v) for k, v in result.items()}, f)
        with open(os.path.join(args.output_dir, "dis_iou_report.txt"), "w") as f:
            f.write(text)
    return text, result


if __name__ == "__main__":
    main()
