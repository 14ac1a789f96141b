"""How far off is each depth estimate, and at which range: the error of every depth the decode forms, at the labelled objects of a
KITTI split, by class and range bin.

The decode (csrc/decode_math.h) computes a direct depth, three key-point depths, their sigmas, the inverse-sigma fusion and the
all-pairs edge-constraint depth for every candidate and reports the last one.  This pass asks for all of them at the GROUND-TRUTH
centres of a labelled split -- no top-K, no threshold, no matching: the object the estimate belongs to is known -- and books
e = estimate - label depth:

    backbone -> predictor.heads_at(the targets' `target_centers`) -> ops.depth_estimates -> ops.depth_accumulate

per batch, by the driver of `engine.object_report` (shared with `engine.dis_iou_report`, as are the slot gathering, the host half's
frame and the command line).  The tables stay on the device; nothing is read back inside the loop, and ONE copy brings them to the
host at the end.  Every (class, bin, method) cell adds its objects in slot order in double, and the backbone -- the one stage whose
bits depend on how many images it is given -- runs one image at a time by default (`backbone_batch`), so the result has the same
bits for every batch size and from run to run.

The methods (`ops.DEPTH_METHODS`): direct, kpt_center, kpt_02, kpt_13 (the four estimates), soft (their inverse-sigma weighted
mean), hard (the one with the smallest sigma), mean (their plain mean), edges (what inference reports), oracle (the one of the four
closest to the label: the bound of any selection rule) and gmw.  With `gmw=` (a `dcd_amd.gmw.GMW` model) the last column is GMW's
refined depth: the fused decode runs at the same cells with `records=True`, `ops.gmw_pack_records` lays every slot of the batch out
for the extractors and `gmw.inference.refine_packed` refines them in groups of `gmw_batch`; empty slots are refined too (and
discarded), because leaving them out would need their count on the host.  Without `gmw` the column is NaN and its cells count
non-finite estimates only.

    python -m dcd_amd.engine.depth_report --root KITTI --split val --ckpt OUT [--batch 8] [--gmw-ckpt FILE [--gmw-batch N]]
                                          [--edges 0 10 20 ...] [--backbone-batch 1] [--output-dir DIR] [KEY VALUE ...]

prints the table and, with --output-dir, writes `depth_report.json` and `depth_report.txt` there."""
import logging

import numpy as np
import torch

from dcd_amd import ops
from dcd_amd.engine.object_report import DEFAULT_EDGES, MAX_SLOTS  # noqa: F401  (this module's names too)
from dcd_amd.engine.object_report import class_blocks, labelled_slots, num, run_cli, run_report, summarise_table
from dcd_amd.structures.params_3d import stack_field


def report_batch(model, images, targets, spec, edges, table, outside, gmw_column=None, backbone_batch=1):
    """The loop body: one batch's estimates (B M, 13), booked into `table` / `outside` in place.  Everything is enqueued on the
    current stream and nothing is read back.  backbone_batch: images per backbone call (None: the whole batch in one)."""
    vectors, lin, ys, xs, classes, valid, image_table = labelled_slots(model, images, targets, backbone_batch, "depth_report")
    gt_z = stack_field(targets, "locations")[:, :, 2]
    est = ops.depth_estimates(vectors, ys, xs, classes, gt_z, valid, image_table, spec)
    if gmw_column is not None:
        z = gmw_column(vectors, lin, classes, ys, xs, image_table, spec)
        est[:, ops.DEPTH_ROW - 1] = torch.where(valid.reshape(-1) != 0, z, torch.zeros_like(z))      # (an empty slot's row stays zero)
    ops.depth_accumulate(est, edges, table, outside)
    return est


def summarise(table, outside, edges, classes):
    """The host half: the (class, bin, method, stat) sums and the `outside` counts -> the result dict, the "all" bin last.
    A cell without a finite estimate has NaN for mae / bias / rmse."""
    return summarise_table(table, outside, edges, classes, lambda sums, count: {
        "methods": list(ops.DEPTH_METHODS), "mae": sums[..., 1] / count, "bias": sums[..., 2] / count, "rmse": np.sqrt(sums[..., 3] / count)})


def format_report(result):
    """The fixed-width table: one block per class, one line per method; the bins' MAE, then all / bias / RMSE / n of the "all" bin
    (n: the objects with a finite estimate)."""
    bins, blocks = class_blocks(result)
    lines = []
    for c, name, objects in blocks:
        lines.append("%s: %s" % (name, objects))
        lines.append("%-12s" % "MAE [m]" + "".join("%8s" % b for b in bins) + "%8s%8s%8s%7s" % ("all", "bias", "RMSE", "n"))
        for m, method in enumerate(result["methods"]):
            lines.append("%-12s" % method + "".join(num(v) for v in result["mae"][c, :, m])
                         + num(result["bias"][c, -1, m]) + num(result["rmse"][c, -1, m]) + "%7d" % int(result["count"][c, -1, m]))
        lines.append("")
    return "\n".join(lines)


def depth_report(model, files, pipeline, batch_size=8, edges=DEFAULT_EDGES, gmw=None, gmw_batch=256, per_object=False, workers=None,
                 backbone_batch=1):
    """model: a `KeypointDetector`; files: a labelled `KittiFiles`; pipeline: a `DeviceInputPipeline(is_train=False)`.
    backbone_batch: images per backbone call inside a batch.  1 (the default) makes the result the same bits for every
    `batch_size` and from run to run: the backbone's kernels are chosen by problem size, and above one image some of its library
    GEMMs are not reproducible from run to run, while everything after it -- `heads_at`, the two kernels, the summary -- does not
    depend on the batch size.  None runs the backbone once per batch: faster, equal to about 1e-6 of an estimate.
    Returns (text, result): result = {"edges", "classes", "methods", and "mae", "bias", "rmse", "count", "nonfinite" as arrays
    (class, bin + 1, method) whose last bin is "all", "outside" (class)}; text is `format_report(result)`, logged as well.
    per_object=True adds result["est"] (N, 13) -- every slot's row [valid, class, gt_z, the methods] in split order, one bulk copy --
    and result["img_ids"], each row's image id.
    Raises ValueError for a split without labels, NotImplementedError for a configuration the kernels do not cover."""
    def open_tables(spec, edges, classes, device):
        table, outside = ops.depth_tables(len(classes), len(edges) - 1, device)
        return table, outside, lambda images, targets, gmw_column: report_batch(model, images, targets, spec, edges, table, outside,
                                                                                 gmw_column, backbone_batch)
    table, outside, edges, classes, rows = run_report("depth_report", model, files, pipeline, batch_size, edges, gmw, gmw_batch, per_object,
                                                      workers, backbone_batch, open_tables, "est", ops.DEPTH_ROW)
    result = {**summarise(table, outside, edges, classes), **rows}
    text = format_report(result)
    logging.getLogger("dcd_amd.depth_report").info("depth errors at the labelled objects of %d images\n%s", len(files), text)
    return text, result


def main(argv=None):
    """`python -m dcd_amd.engine.depth_report --root KITTI_DIR --split val --ckpt FILE [--batch N] [--gmw-ckpt FILE [--gmw-batch N]]
    [--edges 0 10 ...] [--output-dir DIR] [KEY VALUE ...]`: the depth report of a saved checkpoint (a file, or a directory with
    `last_checkpoint`) on one GPU."""
    return run_cli("depth_report", depth_report, "where depth_report.json and depth_report.txt go (default: printed only)",
                   "a GMW checkpoint: fill the `gmw` column with its refined depth", main.__doc__, argv)


if __name__ == "__main__":
    main()
