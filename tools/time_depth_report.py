"""What the depth report costs next to the detector's evaluation pass over the same frames, in one process:
  (a) seconds end to end of `engine.depth_report.depth_report(batch_size=8)` -- with the backbone one image at a time (the
      default, reproducible bit for bit) and once per batch (`backbone_batch=None`) -- and with `gmw=`, against
      `engine.inference.inference(batch_size=8)` -- the latter timed TWICE per round, the two series' medians give the run-to-run
      spread -- on a seeded split of --frames KITTI-size frames (noise PNGs at the four KITTI sizes, the labels of
      tests/golden/kitti_files repeated; nothing is downloaded), `init_like_trained` weights, a seeded GMW; the variants alternate,
      medians over --reps rounds after one warm-up pass of each.  "End to end" is the whole call: PNG decode, forward, the kernels,
      the copy, and for `inference` the result files, reading them back and the AP tables;
  (b) from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child, `--once`: one batch of 8 through the loop body
      ONCE_CALLS times): the time per launch of depth_estimates and depth_accumulate.
Writes the figures to --out (default profiles/depth_report.txt).  The one expectation: the report without GMW costs no more than
the detector's evaluation pass beyond the spread of (a); the file says whether that holds.

    python tools/time_depth_report.py [--frames 64] [--reps 3] [--no-trace] [--out profiles/depth_report.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_report.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_depth_report.py measures on the GPU; none found")
    from dcd_amd import ops
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.depth_report import DEFAULT_EDGES, depth_report, report_batch
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.gmw import GMW
    from dcd_amd.model.detector import KeypointDetector

    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="depth_report_")
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
                tables = ops.depth_tables(len(spec["dim_mean"]), len(DEFAULT_EDGES) - 1, dev)
                for _ in range(ONCE_CALLS):
                    report_batch(model, images, targets, spec, DEFAULT_EDGES, *tables)
                torch.cuda.synchronize()
            return
        torch.manual_seed(0)
        gmw = GMW().to(dev).eval()
        out = os.path.join(work, "out")
        variants = (("inference (first series)", lambda: inference(model, files, pipe, out, batch_size=8)),
                    ("inference (second series)", lambda: inference(model, files, pipe, out, batch_size=8)),
                    ("depth report", lambda: depth_report(model, files, pipe, batch_size=8)),
                    ("depth report, one backbone call per batch", lambda: depth_report(model, files, pipe, batch_size=8, backbone_batch=None)),
                    ("depth report with gmw=", lambda: depth_report(model, files, pipe, batch_size=8, gmw=gmw)))
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
        lines = ["the depth report against the detector's evaluation pass: %d frames %s, batch 8, %d object slots (GMW refines every one, "
                 "in groups of 256), %s, %d alternating rounds after warm-up; end to end"
                 % (n, sorted(set(KITTI_SIZES)), slots, torch.cuda.get_device_name(0), args.reps),
                 "  %-44s %12s %12s %12s" % ("route", "median s", "min s", "images/s")]
        for name, _ in variants:
            lines.append("  %-44s %12.3f %12.3f %12.1f" % (name, med[name], np.min(seconds[name]), n / med[name]))
        base = (med["inference (first series)"], med["inference (second series)"])
        spread = abs(base[0] - base[1]) / min(base)
        lines.append("  run-to-run spread of the evaluation pass (its two series): %.1f %%" % (100 * spread))
        for name in ("depth report", "depth report, one backbone call per batch"):
            ok = med[name] <= max(base) * (1 + spread)
            lines.append("  %s (no GMW) against the evaluation pass: %.2fx the time -- no more than it beyond the spread: %s"
                         % (name, med[name] / float(np.mean(base)), "holds" if ok else "REFUTED"))
        lines.append("  the gmw column: %.3f s on top of the report, %.2f ms per slot refined"
                     % (med["depth report with gmw="] - med["depth report"],
                        1e3 * (med["depth report with gmw="] - med["depth report"]) / slots))
        if not args.no_trace:
            found = traced_child(__file__, "loop", work, 600)
            lines.append("one batch of 8 x %d slots (rocprofv3 --kernel-trace --stats, a child of its own, %d calls):"
                         % (cfg.DATASETS.MAX_OBJECTS, ONCE_CALLS))
            for kernel in ("depth_estimates", "depth_accumulate"):
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
