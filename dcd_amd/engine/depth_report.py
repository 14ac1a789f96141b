"""How far off is each depth estimate, and at which range: the error of every depth the decode forms, at the labelled objects of a
KITTI split, by class and range bin.

The decode (csrc/decode_math.h) computes a direct depth, three key-point depths, their sigmas, the inverse-sigma fusion and the
all-pairs edge-constraint depth for every candidate and reports the last one.  This pass asks for all of them at the GROUND-TRUTH
centres of a labelled split -- no top-K, no threshold, no matching: the object the estimate belongs to is known -- and books
e = estimate - label depth:

    backbone -> predictor.heads_at(the targets' `target_centers`) -> ops.depth_estimates -> ops.depth_accumulate

per batch, walked with `EvalPlan` and prepared one batch ahead as `engine.inference` does.  The tables stay on the device; nothing
is read back inside the loop, and ONE copy brings them to the host at the end.  Every (class, bin, method) cell adds its objects
in slot order in double, and the backbone -- the one stage whose bits depend on how many images it is given -- runs one image at a
time by default (`backbone_batch`), so the result has the same bits for every batch size and from run to run.

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
import os

import numpy as np
import torch

from dcd_amd import ops
from dcd_amd.engine.passes import load_detector, load_gmw, parse_overrides, restored_modes
from dcd_amd.structures.params_3d import stack_field

DEFAULT_EDGES = (0, 10, 20, 30, 40, 50, 60, 80)
MAX_SLOTS = 128                        # object slots per image the kernel takes (one workgroup's K)


class _GmwColumn:
    """GMW's refined depth of every slot of a batch, on the device: the decode at the slots' cells with `records=True`, then the
    slots in groups of `cap` through `ops.gmw_pack_records` and `refine_packed`."""

    def __init__(self, gmw, device, cap, nk):
        from dcd_amd.gmw.inference import PackBuffers
        self.packs = PackBuffers(gmw, device, cap, nk, "depth_report(gmw=...)")
        self.src = torch.arange(8 * MAX_SLOTS, dtype=torch.int32, device=device)

    def __call__(self, vectors, lin, classes, ys, xs, table, spec):
        B, M = lin.shape
        n = B * M
        if self.src.numel() < n:
            self.src = torch.arange(n, dtype=torch.int32, device=self.src.device)
        topk = (torch.zeros((B, M), dtype=torch.float32, device=lin.device), lin, classes, ys, xs)
        rows, _, k2, k3 = ops.decode_detections(vectors, topk, table, spec, records=True)
        z = torch.empty(n, dtype=torch.float32, device=lin.device)
        cap = self.packs.cap
        for s in range(0, n, cap):
            count = min(cap, n - s)
            self.packs.pack(rows, k2, k3, self.src[s:s + count], 0)
            z[s:s + count] = self.packs.refine(count)[0]
        return z


def report_batch(model, images, targets, spec, edges, table, outside, gmw_column=None, backbone_batch=1):
    """The loop body: one batch's estimates (B M, 13), booked into `table` / `outside` in place.  Everything is enqueued on the
    current stream and nothing is read back.  backbone_batch: images per backbone call (None: the whole batch in one)."""
    pp, predictor = model.heads.post_processor, model.heads.predictor
    B = images.shape[0]
    if backbone_batch is None or backbone_batch >= B:
        feats = model.backbone(images)
    else:
        feats = torch.cat([model.backbone(images[s:s + backbone_batch]) for s in range(0, B, backbone_batch)])
    centers = stack_field(targets, "target_centers")                   # (B, M, 2) cells (x, y)
    if centers.shape[1] > MAX_SLOTS:
        raise NotImplementedError("depth_report: %d object slots per image (%d at most)" % (centers.shape[1], MAX_SLOTS))
    xs, ys = centers[:, :, 0], centers[:, :, 1]
    lin = ys.long() * feats.shape[3] + xs.long()
    vectors = predictor.heads_at(feats, targets, lin)
    classes, valid = stack_field(targets, "cls_ids").float(), stack_field(targets, "reg_mask")
    gt_z = stack_field(targets, "locations")[:, :, 2]
    ys, xs = ys.float(), xs.float()
    image_table = pp._image_table(targets, vectors.device)
    est = ops.depth_estimates(vectors, ys, xs, classes, gt_z, valid, image_table, spec)
    if gmw_column is not None:
        z = gmw_column(vectors, lin, classes, ys, xs, image_table, spec)
        est[:, ops.DEPTH_ROW - 1] = torch.where(valid.reshape(-1) != 0, z, torch.zeros_like(z))      # (an empty slot's row stays zero)
    ops.depth_accumulate(est, edges, table, outside)
    return est


def summarise(table, outside, edges, classes):
    """The host half: the (class, bin, method, stat) sums and the `outside` counts -> the result dict.  The extra last bin is
    "all": the per-bin sums added in bin order.  A cell without a finite estimate has NaN for mae / bias / rmse."""
    table = np.asarray(table, np.float64)
    total = table[:, 0].copy()
    for i in range(1, table.shape[1]):
        total = total + table[:, i]
    sums = np.concatenate((table, total[:, None]), axis=1)             # (class, bin + 1, method, stat)
    count = sums[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        mae, bias, rmse = sums[..., 1] / count, sums[..., 2] / count, np.sqrt(sums[..., 3] / count)
    return {"edges": [float(e) for e in edges], "classes": list(classes), "methods": list(ops.DEPTH_METHODS), "mae": mae, "bias": bias,
            "rmse": rmse, "count": count.astype(np.int64), "nonfinite": sums[..., 4].astype(np.int64),
            "outside": np.asarray(outside, np.int64).copy()}


def format_report(result):
    """The fixed-width table: one block per class, one line per method; the bins' MAE, then all / bias / RMSE / n of the "all" bin
    (n: the objects with a finite estimate)."""
    edges = result["edges"]
    bins = ["%g-%g" % (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]

    def num(v):
        return "%8.3f" % v if np.isfinite(v) else "%8s" % "-"
    lines = []
    seen = result["count"][:, -1, 0] + result["nonfinite"][:, -1, 0] + result["outside"]
    for c, name in enumerate(result["classes"]):
        if seen[c] == 0 and seen.sum() > 0:
            continue                                                   # a class the split holds no object of
        objects = int(result["count"][c, -1, 0] + result["nonfinite"][c, -1, 0])    # every object is one or the other, per method
        lines.append("%s: %d objects in the bins, %d outside [%g, %g)" % (name, objects, int(result["outside"][c]), edges[0], edges[-1]))
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
    from dcd_amd.data.batches import eval_batches
    if not getattr(files, "has_labels", True):
        raise ValueError("depth_report needs a labelled split: %r has no labels to measure against" % getattr(files, "split", files))
    if pipeline.is_train:
        raise ValueError("depth_report needs a DeviceInputPipeline(is_train=False): evaluation never flips")
    if batch_size < 1 or (backbone_batch is not None and backbone_batch < 1):
        raise ValueError("batch size %d, backbone batch %s" % (batch_size, backbone_batch))
    edges = [float(e) for e in edges]
    n_bins = len(edges) - 1
    if not 1 <= n_bins <= ops.DEPTH_MAX_BINS or any(not lo < hi for lo, hi in zip(edges[:-1], edges[1:])):
        raise ValueError("edges %s: 2 to %d increasing numbers" % (edges, ops.DEPTH_MAX_BINS + 1))
    logger = logging.getLogger("dcd_amd.depth_report")
    pp = model.heads.post_processor
    spec = pp.decode_spec()                                            # refuses here, not in the middle of the split
    # one table row per class id the targets can carry (the rows of the dimension statistics), named as the label files name them;
    # DATASETS.DETECT_CLASSES decides which of them the split's targets hold
    from dcd_amd.data.kitti_files import TYPE_ID_CONVERSION
    names = {v: k for k, v in TYPE_ID_CONVERSION.items() if v >= 0}
    classes = [names.get(c, "class %d" % c) for c in range(len(spec["dim_mean"]))]
    device = pipeline.device
    table, outside = ops.depth_tables(len(classes), n_bins, device)
    gmw_column = None
    kept, ids = [], []
    with restored_modes(model, gmw), torch.no_grad():
        model.eval()
        if gmw is not None:
            gmw.eval()
            gmw_column = _GmwColumn(gmw, device, gmw_batch, spec["nk"])
        with eval_batches(files, pipeline, batch_size, workers) as walk:
            for k, indices, images, targets in walk:
                est = report_batch(model, images, targets, spec, edges, table, outside, gmw_column, backbone_batch)
                if per_object:
                    kept.append(est)
                    slots = est.shape[0] // len(targets)
                    ids.extend(files.img_id(i) for i in indices for _ in range(slots))
        # the one copy: the sums and, as the same 8-byte words, the counters
        flat = torch.cat((table.reshape(-1), outside.view(torch.float64))).cpu().numpy()
        est_host = torch.cat(kept).cpu().numpy() if kept else np.zeros((0, ops.DEPTH_ROW), np.float32)
    result = summarise(flat[:table.numel()].reshape(tuple(table.shape)), flat[table.numel():].view(np.int64), edges, classes)
    if per_object:
        result["est"], result["img_ids"] = est_host, ids
    text = format_report(result)
    logger.info("depth errors at the labelled objects of %d images\n%s", len(files), text)
    return text, result


def main(argv=None):
    """`python -m dcd_amd.engine.depth_report --root KITTI_DIR --split val --ckpt FILE [--batch N] [--gmw-ckpt FILE [--gmw-batch N]]
    [--edges 0 10 ...] [--output-dir DIR] [KEY VALUE ...]`: the depth report of a saved checkpoint (a file, or a directory with
    `last_checkpoint`) on one GPU."""
    import argparse
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--root", required=True, help="KITTI directory: ImageSets, image_2, label_2, calib, kpts_ann")
    ap.add_argument("--split", default="val", help="ImageSets/<split>.txt; it must have labels")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--output-dir", default=None, help="where depth_report.json and depth_report.txt go (default: printed only)")
    ap.add_argument("--batch", type=int, default=8, help="images per model call; the result does not depend on it")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--backbone-batch", type=int, default=1, help="images per backbone call (1: the same bits for every --batch; "
                    "0: the whole batch in one call, faster, equal to about 1e-6)")
    ap.add_argument("--edges", nargs="+", default=None, metavar="M", help="range bin edges in metres, increasing (default %s)"
                    % " ".join(str(e) for e in DEFAULT_EDGES))
    ap.add_argument("--gmw-ckpt", default=None, help="a GMW checkpoint: fill the `gmw` column with its refined depth")
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
    text, result = depth_report(model, files, pipeline, batch_size=args.batch, edges=edges, gmw=gmw, gmw_batch=args.gmw_batch,
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
        with open(os.path.join(args.output_dir, "depth_report.json"), "w") as f:
            json.dump({k: plain(v) for k, v in result.items()}, f)
        with open(os.path.join(args.output_dir, "depth_report.txt"), "w") as f:
            f.write(text)
    return text, result


if __name__ == "__main__":
    main()
