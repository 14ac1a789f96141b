"""What the passes over the LABELLED OBJECTS of a split share (`engine.depth_report`, `engine.dis_iou_report`): each asks what the
model says at the ground-truth cells -- no top-K, no threshold, no matching -- and books it by class and range bin.  Here, once: the
front of the loop body (`labelled_slots`), GMW's depth of every slot (`GmwColumn`), the driver (`run_report`: the refusals, the walk
with `data.batches.eval_batches`, the tables on the device and ONE copy), the host half (`summarise_table`, `class_blocks`, `num`) and
the command line (`parse_args`, `run_cli`).  A report keeps what is its own: its kernels' rows, its columns, its table lines.  Like
`engine.passes`, nothing here needs the built library to be imported."""
import logging
import os

import numpy as np
import torch

from dcd_amd import ops
from dcd_amd.engine.passes import load_detector, load_gmw, parse_overrides, restored_modes
from dcd_amd.structures.params_3d import stack_field

DEFAULT_EDGES = (0, 10, 20, 30, 40, 50, 60, 80)
MAX_SLOTS = 128                        # object slots per image the kernels take (one workgroup's K)


class GmwColumn:
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


def labelled_slots(model, images, targets, backbone_batch, who):
    """The front of a loop body: the head outputs at the targets' centres and what the kernels want per slot --
    (vectors (B, M, C), lin (B, M) int64 cell numbers, ys, xs, classes (B, M) float, valid (B, M), image_table (B, 16)).
    backbone_batch: images per backbone call (None: the whole batch in one); who: the report, for the refusal of too many slots."""
    B = images.shape[0]
    if backbone_batch is None or backbone_batch >= B:
        feats = model.backbone(images)
    else:
        feats = torch.cat([model.backbone(images[s:s + backbone_batch]) for s in range(0, B, backbone_batch)])
    centers = stack_field(targets, "target_centers")                   # (B, M, 2) cells (x, y)
    if centers.shape[1] > MAX_SLOTS:
        raise NotImplementedError("%s: %d object slots per image (%d at most)" % (who, centers.shape[1], MAX_SLOTS))
    xs, ys = centers[:, :, 0], centers[:, :, 1]
    lin = ys.long() * feats.shape[3] + xs.long()
    vectors = model.heads.predictor.heads_at(feats, targets, lin)
    classes, valid = stack_field(targets, "cls_ids").float(), stack_field(targets, "reg_mask")
    return vectors, lin, ys.float(), xs.float(), classes, valid, model.heads.post_processor._image_table(targets, vectors.device)


def run_report(who, model, files, pipeline, batch_size, edges, gmw, gmw_batch, per_object, workers, backbone_batch, open_tables, rows_key, row):
    """The driver of a report called `who`: refuses what cannot be measured, names the classes, walks the split and brings the
    tables to the host in ONE copy.  open_tables(spec, edges, classes, device) -> (table float64, outside int64, body) is called
    once everything else is settled and before anything is allocated; body(images, targets, gmw_column) books one batch into the
    tables on the current stream, reads nothing back and returns the batch's rows (n, row).
    Returns (table, outside as host arrays, edges as floats, classes, what per_object adds to the result: {} or {rows_key: the
    rows (N, row) in split order, "img_ids": each row's image id})."""
    from dcd_amd.data.batches import eval_batches
    if not getattr(files, "has_labels", True):
        raise ValueError("%s needs a labelled split: %r has no labels to measure against" % (who, getattr(files, "split", files)))
    if pipeline.is_train:
        raise ValueError("%s needs a DeviceInputPipeline(is_train=False): evaluation never flips" % who)
    if batch_size < 1 or (backbone_batch is not None and backbone_batch < 1):
        raise ValueError("batch size %d, backbone batch %s" % (batch_size, backbone_batch))
    edges = [float(e) for e in edges]
    if not 1 <= len(edges) - 1 <= ops.DEPTH_MAX_BINS or any(not lo < hi for lo, hi in zip(edges[:-1], edges[1:])):
        raise ValueError("edges %s: 2 to %d increasing numbers" % (edges, ops.DEPTH_MAX_BINS + 1))
    spec = model.heads.post_processor.decode_spec()                    # refuses here, not in the middle of the split
    # one table row per class id the targets can carry (the rows of the dimension statistics), named as the label files name them;
    # DATASETS.DETECT_CLASSES decides which of them the split's targets hold
    from dcd_amd.data.kitti_files import TYPE_ID_CONVERSION
    names = {v: k for k, v in TYPE_ID_CONVERSION.items() if v >= 0}
    classes = [names.get(c, "class %d" % c) for c in range(len(spec["dim_mean"]))]
    table, outside, body = open_tables(spec, edges, classes, pipeline.device)
    gmw_column, kept, ids = None, [], []
    with restored_modes(model, gmw), torch.no_grad():
        model.eval()
        if gmw is not None:
            gmw.eval()
            gmw_column = GmwColumn(gmw, pipeline.device, gmw_batch, spec["nk"])
        with eval_batches(files, pipeline, batch_size, workers) as walk:
            for k, indices, images, targets in walk:
                rows = body(images, targets, gmw_column)
                if per_object:
                    kept.append(rows)
                    slots = rows.shape[0] // len(targets)
                    ids.extend(files.img_id(i) for i in indices for _ in range(slots))
        # the one copy: the sums and, as the same 8-byte words, the counters
        flat = torch.cat((table.reshape(-1), outside.view(torch.float64))).cpu().numpy()
        extra = {rows_key: torch.cat(kept).cpu().numpy() if kept else np.zeros((0, row), np.float32), "img_ids": ids} if per_object else {}
    return flat[:table.numel()].reshape(tuple(table.shape)), flat[table.numel():].view(np.int64), edges, classes, extra


# ---- the host half -----------------------------------------------------------------------------------------------------------
def summarise_table(table, outside, edges, classes, columns):
    """The (class, bin, ..., stat) sums and the `outside` counts -> the result dict.  The extra last bin is "all": the per-bin sums
    added in bin order.  columns(sums, count) -> the report's own entries, evaluated with division warnings off (a cell without a
    finite value divides by zero: NaN); stat 0 is the count, the last stat the non-finite count."""
    table = np.asarray(table, np.float64)
    total = table[:, 0].copy()
    for i in range(1, table.shape[1]):
        total = total + table[:, i]
    sums = np.concatenate((table, total[:, None]), axis=1)             # (class, bin + 1, ..., stat)
    count = sums[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        own = columns(sums, count)
    return {"edges": [float(e) for e in edges], "classes": list(classes), **own, "count": count.astype(np.int64),
            "nonfinite": sums[..., -1].astype(np.int64), "outside": np.asarray(outside, np.int64).copy()}


def num(v):
    return "%8.3f" % v if np.isfinite(v) else "%8s" % "-"


def class_blocks(result):
    """What the printed tables share: (the bins' labels, [(class index, name, "N objects in the bins, N outside [lo, hi)")]) with
    a class the split holds no object of left out.  Every object of a bin is finite or non-finite, in each column alike, so the
    first column counts them."""
    edges = result["edges"]
    bins = ["%g-%g" % (lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]
    objects = (result["count"][:, -1] + result["nonfinite"][:, -1]).reshape(len(result["classes"]), -1)[:, 0]
    seen = objects + result["outside"]
    blocks = []
    for c, name in enumerate(result["classes"]):
        if seen[c] == 0 and seen.sum() > 0:
            continue                                                   # a class the split holds no object of
        blocks.append((c, name, "%d objects in the bins, %d outside [%g, %g)" % (int(objects[c]), int(result["outside"][c]),
                                                                              edges[0], edges[-1])))
    return bins, blocks


# ---- the command line --------------------------------------------------------------------------------------------------------
def parse_args(output_help, gmw_help, doc, argv=None):
    """argv -> (the parsed arguments, the edges, the `KEY VALUE ...` override tokens).  Needs no GPU."""
    import argparse
    ap = argparse.ArgumentParser(description=doc)
    ap.add_argument("--root", required=True, help="KITTI directory: ImageSets, image_2, label_2, calib, kpts_ann")
    ap.add_argument("--split", default="val", help="ImageSets/<split>.txt; it must have labels")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--output-dir", default=None, help=output_help)
    ap.add_argument("--batch", type=int, default=8, help="images per model call; the result does not depend on it")
    ap.add_argument("--workers", type=int, default=None)
    ap.add_argument("--backbone-batch", type=int, default=1, help="images per backbone call (1: the same bits for every --batch; "
                    "0: the whole batch in one call, faster, equal to about 1e-6)")
    ap.add_argument("--edges", nargs="+", default=None, metavar="M", help="range bin edges in metres, increasing (default %s)"
                    % " ".join(str(e) for e in DEFAULT_EDGES))
    ap.add_argument("--gmw-ckpt", default=None, help=gmw_help)
    ap.add_argument("--gmw-batch", type=int, default=256, help="slots per refinement call")
    ap.add_argument("opts", nargs="*", help="configuration overrides: KEY VALUE ...")
    args = ap.parse_args(argv)
    if args.edges is None:
        return args, list(DEFAULT_EDGES), args.opts
    # `--edges 0 10 20 KEY VALUE ...`: the list ends at the first token that is not a number; the rest are the overrides
    edges = []
    for s in args.edges:
        try:
            edges.append(float(s))
        except ValueError:
            break
    return args, edges, args.edges[len(edges):] + args.opts


def run_cli(name, driver, output_help, gmw_help, doc, argv=None):
    """The command line of the report `name`: `driver` on a saved checkpoint on one GPU, the table printed and, with
    --output-dir, written there as <name>.json and <name>.txt."""
    import json
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    args, edges, tokens = parse_args(output_help, gmw_help, doc, argv)
    logging.basicConfig(level=logging.WARNING, format="%(asctime)s %(name)s %(message)s")
    cfg = get_cfg(opts=parse_overrides(tokens))
    device = torch.device("cuda", torch.cuda.current_device())
    model, _ = load_detector(cfg, args.ckpt, device)
    gmw = load_gmw(args.gmw_ckpt, device) if args.gmw_ckpt else None
    files = KittiFiles(args.root, args.split, cfg, is_train=False)
    pipeline = DeviceInputPipeline(cfg, device, is_train=False)
    text, result = driver(model, files, pipeline, batch_size=args.batch, edges=edges, gmw=gmw, gmw_batch=args.gmw_batch,
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
        with open(os.path.join(args.output_dir, name + ".json"), "w") as f:
            json.dump({k: plain(v) for k, v in result.items()}, f)
        with open(os.path.join(args.output_dir, name + ".txt"), "w") as f:
            f.write(text)
    return text, result
