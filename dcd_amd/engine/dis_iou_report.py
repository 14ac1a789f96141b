"""Which head loses the 3-D overlap: the disentangled IoU report (the MonoDIS / MonoFlex test the reference names with
`TEST.EVAL_DIS_IOUS` and never defines) at the labelled objects of a KITTI split, by class and range bin.

At every labelled object the pass builds fifteen boxes in which ONE component is the prediction's and the rest is the label's
(`ops.DIS_VARIANTS`: full, location, offset, dims, orient, and depth:<m> for the ten `ops.DEPTH_METHODS`) and measures each box's
BEV and 3-D IoU with the label, by the KITTI evaluator's own arithmetic.  A component whose box keeps IoU ~ 1 costs nothing; the one
whose box falls below the class's AP threshold is the one to work on.  Like the depth report it asks at the GROUND-TRUTH centres --
no top-K, no threshold, no matching --

    backbone -> predictor.heads_at(the targets' `target_centers`) -> [GMW's depth of every slot] -> ops.dis_iou_estimates
             -> ops.dis_iou_accumulate

per batch, by the depth report's driver (`engine.object_report`, which also holds the slot gathering, the host half's frame and
the command line): nothing is read back inside the loop, every (class, bin, variant, metric) cell adds its objects in slot order
in double and the backbone runs one image at a time by default, so the result has the same bits for every batch size and from run
to run.

A hit is IoU > threshold, the evaluator's comparison; `thresholds=None` takes each class's strict and loose pair from
`eval.kitti_ap.MIN_OVERLAPS` (rows 0 and 1, the BEV and 3-D columns).  With `gmw=` (a `dcd_amd.gmw.GMW` model) the `depth:gmw`
variant is placed at GMW's refined depth (`object_report.GmwColumn`); without it that variant is NaN and its cells count non-finite
overlaps only.  When one of a variant's seven box numbers is not finite, or an overlap comes out non-finite, both overlaps of that
variant are NaN and are counted as such.

    python -m dcd_amd.engine.dis_iou_report --root KITTI --split val --ckpt OUT [--batch 8] [--backbone-batch 1]
                                            [--edges 0 10 20 ...] [--gmw-ckpt FILE [--gmw-batch N]] [--output-dir DIR] [KEY VALUE ...]

prints the table and, with --output-dir, writes `dis_iou_report.json` and `dis_iou_report.txt` there."""
import logging

import numpy as np
import torch

from dcd_amd import ops
from dcd_amd.engine.object_report import DEFAULT_EDGES, MAX_SLOTS  # noqa: F401  (this module's names too)
from dcd_amd.engine.object_report import class_blocks, labelled_slots, num, run_cli, run_report, summarise_table
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
    vectors, lin, ys, xs, classes, valid, image_table = labelled_slots(model, images, targets, backbone_batch, "dis_iou_report")
    gt = torch.cat((stack_field(targets, "offset_3D"), stack_field(targets, "locations"), stack_field(targets, "dimensions"),
                    stack_field(targets, "rotys").unsqueeze(-1)), dim=2).float()
    gmw_z = None if gmw_column is None else gmw_column(vectors, lin, classes, ys, xs, image_table, spec)
    dis = ops.dis_iou_estimates(vectors, ys, xs, classes, gt, valid, image_table, spec, gmw_z=gmw_z)
    ops.dis_iou_accumulate(dis, edges, thresholds, table, outside)
    return dis


def summarise(table, outside, edges, classes, thresholds):
    """The host half: the (class, bin, variant, metric, stat) sums and the `outside` counts -> the result dict, the "all" bin last.
    A cell without a finite overlap has NaN for the mean and the rates."""
    return summarise_table(table, outside, edges, classes, lambda sums, count: {
        "variants": list(ops.DIS_VARIANTS), "metrics": list(ops.DIS_METRICS), "thresholds": np.asarray(thresholds, np.float64),
        "mean_iou": sums[..., 1] / count, "hit_rate": sums[..., 3] / count, "hit_rate_loose": sums[..., 4] / count})


def format_report(result):
    """The fixed-width table: one block per class and metric, one line per variant; the bins' mean IoU, then mean / both hit
    rates / n of the "all" bin (n: the objects with a finite overlap)."""
    bins, blocks = class_blocks(result)
    lines = []
    for c, name, objects in blocks:
        for k, metric in enumerate(result["metrics"]):
            strict, loose = result["thresholds"][c, k]
            lines.append("%s, %s IoU: %s" % (name, metric, objects))
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
    def open_tables(spec, edges, classes, device):
        nonlocal thresholds
        thresholds = default_thresholds(len(classes)) if thresholds is None else np.asarray(thresholds, np.float64).tolist()
        if np.asarray(thresholds).shape != (len(classes), len(ops.DIS_METRICS), 2) or not all(
                0.0 <= t <= 1.0 for t in np.asarray(thresholds).reshape(-1)):
            raise ValueError("thresholds %s: (%d classes, %d metrics, strict and loose), each in [0, 1]"
                             % (thresholds, len(classes), len(ops.DIS_METRICS)))
        table, outside = ops.dis_iou_tables(len(classes), len(edges) - 1, device)
        return table, outside, lambda images, targets, gmw_column: report_batch(model, images, targets, spec, edges, thresholds, table,
                                                                                 outside, gmw_column, backbone_batch)
    table, outside, edges, classes, rows = run_report("dis_iou_report", model, files, pipeline, batch_size, edges, gmw, gmw_batch, per_object,
                                                      workers, backbone_batch, open_tables, "dis", ops.DIS_ROW)
    result = {**summarise(table, outside, edges, classes, thresholds), **rows}
    text = format_report(result)
    logging.getLogger("dcd_amd.dis_iou_report").info("disentangled IoU at the labelled objects of %d images\n%s", len(files), text)
    return text, result


def main(argv=None):
    """`python -m dcd_amd.engine.dis_iou_report --root KITTI_DIR --split val --ckpt FILE [--batch N] [--backbone-batch 1]
    [--edges 0 10 ...] [--gmw-ckpt FILE [--gmw-batch N]] [--output-dir DIR] [KEY VALUE ...]`: the disentangled IoU report of a saved
    checkpoint (a file, or a directory with `last_checkpoint`) on one GPU."""
    return run_cli("dis_iou_report", dis_iou_report, "where dis_iou_report.json and dis_iou_report.txt go (default: printed only)",
                   "a GMW checkpoint: place the `depth:gmw` variant at its refined depth", main.__doc__, argv)


if __name__ == "__main__":
    main()
