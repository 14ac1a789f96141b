"""What the disentangled IoU report costs next to the depth report over the same frames, in one process:
  (a) seconds end to end of `engine.dis_iou_report.dis_iou_report(batch_size=8)` -- without and with `gmw=` -- against
      `engine.depth_report.depth_report(batch_size=8)` -- the latter timed TWICE per round, the two series' medians give the
      run-to-run spread -- on a seeded split of --frames KITTI-size frames (noise PNGs at the four KITTI sizes, the labels of
      tests/golden/kitti_files repeated; nothing is downloaded), `init_like_trained` weights, a seeded GMW; the variants alternate,
      medians over --reps rounds after one warm-up pass of each.  "End to end" is the whole call: PNG decode, forward, the kernels,
      the one copy and the summary;
  (b) from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child, `--once`: one batch of 8 through the loop body
      ONCE_CALLS times): the time per launch of dis_iou_estimates and dis_iou_accumulate.
Writes the figures to --out (default profiles/dis_iou.txt).  The one expectation: both passes run the same backbone per image and
differ in two small kernels, so the report without GMW costs no more than the depth report beyond the spread of (a); the file
says whether that holds.

    python tools/time_dis_iou.py [--frames 64] [--reps 3] [--no-trace] [--out profiles/dis_iou.txt]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from tools.kernel_trace import traced_child
from tools.time_detector_eval import KITTI_SIZES, write_split

ONCE_CALLS = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", choices=("loop",), default=None, help="what a traced child runs: the loop body ONCE_CALLS times")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dis_iou.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_dis_iou.py measures on the GPU; none found")
    from dcd_amd import ops
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.depth_report import DEFAULT_EDGES, depth_report
    from dcd_amd.engine.dis_iou_report import default_thresholds, dis_iou_report, report_batch
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.gmw import GMW
    from dcd_amd.model.detector import KeypointDetector

    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="dis_iou_")
    try:
        n = 8 if args.once else args.frames
        write_split(os.path.join(work, "kitti"), n)
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0])
        files = KittiFiles(os.path.join(work, "kitti"), "train", cfg, is_train=False)
        pipe = DeviceInputPipeline(cfg, dev, is_train=False)
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev)
        init_like_trained(model)
        model.eval()
        if args.once:
            with torch.no_grad():
                images, targets = pipe([files.frame(i) for i in range(8)], [files.sample(i) for i in range(8)],
                                       img_ids=[files.img_id(i) for i in range(8)])
                spec = model.heads.post_processor.decode_spec()
                num_classes = len(spec["dim_mean"])
                tables = ops.dis_iou_tables(num_classes, len(DEFAULT_EDGES) - 1, dev)
                for _ in range(ONCE_CALLS):
                    report_batch(model, images, targets, spec, DEFAULT_EDGES, default_thresholds(num_classes), *tables)
                torch.cuda.synchronize()
            return
        torch.manual_seed(0)
        gmw = GMW().to(dev).eval()
        variants = (("depth report (first series)", lambda: depth_report(model, files, pipe, batch_size=8)),
                    ("depth report (second series)", lambda: depth_report(model, files, pipe, batch_size=8)),
                    ("dis-IoU report", lambda: dis_iou_report(model, files, pipe, batch_size=8)),
                    ("depth report with gmw=", lambda: depth_report(model, files, pipe, batch_size=8, gmw=gmw)),
                    ("dis-IoU report with gmw=", lambda: dis_iou_report(model, files, pipe, batch_size=8, gmw=gmw)))
        for _, fn in variants[1:]:                                                 # one warm-up pass of each
            fn()
        seconds = {name: [] for name, _ in variants}
        for r in range(args.reps):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
        med = {name: float(np.median(v)) for name, v in seconds.items()}
        slots = n * cfg.DATASETS.MAX_OBJECTS
        lines = ["the disentangled IoU report against the depth report: %d frames %s, batch 8, backbone one image at a time, %d object "
                 "slots (GMW refines every one, in groups of 256), %s, %d alternating rounds after warm-up; end to end"
                 % (n, sorted(set(KITTI_SIZES)), slots, torch.cuda.get_device_name(0), args.reps),
                 "  %-44s %12s %12s %12s" % ("route", "median s", "min s", "images/s")]
        for name, _ in variants:
            lines.append("  %-44s %12.3f %12.3f %12.1f" % (name, med[name], np.min(seconds[name]), n / med[name]))
        base = (med["depth report (first series)"], med["depth report (second series)"])
        spread = abs(base[0] - base[1]) / min(base)
        lines.append("  run-to-run spread of the depth report (its two series): %.1f %%" % (100 * spread))
        ok = med["dis-IoU report"] <= max(base) * (1 + spread)
        lines.append("  dis-IoU report (no GMW) against the depth report: %.2fx the time -- no more than it beyond the spread: %s"
                     % (med["dis-IoU report"] / float(np.mean(base)), "holds" if ok else "REFUTED"))
        lines.append("  with gmw=: %.2fx the depth report with gmw="
                     % (med["dis-IoU report with gmw="] / med["depth report with gmw="]))
        if not args.no_trace:
            found = traced_child(__file__, "loop", work, 600)
            lines.append("one batch of 8 x %d slots (rocprofv3 --kernel-trace --stats, a child of its own, %d calls):"
                         % (cfg.DATASETS.MAX_OBJECTS, ONCE_CALLS))
            for kernel in ("dis_iou_estimates", "dis_iou_accumulate"):
                k = [v for name, v in found.items() if kernel in name]
                if not k:
                    sys.exit("the kernel trace does not list %s" % kernel)
                lines.append("  %s: %.1f us per launch (%d launches)" % (kernel, k[0][1] / k[0][0], k[0][0]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
