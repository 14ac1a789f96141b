"""What collecting GMW's training records from a detector costs, in one process, up to the same `ResidentRecords`:
  (a) today's route: `do_train` under TEST.GENERATE_GMW (the 13-term loss op by op, `nonzero`, a `.cpu()` per iteration), then
      `dump_gen_data_train` (json, indent 4), `gmw.data.load_train_data` and `ResidentRecords` -- timed TWICE per round, the two
      series' medians give the run-to-run spread;
  (b) the device route: `engine.train.collect_gmw_records` (backbone -> predictor -> `dcd_gmw_train_records`, one host read at
      the end);
      both over --frames seeded KITTI-size frames (tools/time_detector_eval.py's split) resident in device memory, batch 8,
      `init_like_trained` detector weights; the routes alternate, medians over --reps rounds after one warm-up pass of each;
  (c) from `rocprofv3 --kernel-trace --stats` runs of their own (two fresh children, `--once base | collect`: ONCE_CALLS calls
      of `TrainRecordCollector.add` on a seeded batch of 8): kernel launches and kernel time per call = (collect - base) /
      ONCE_CALLS.
Writes the figures to --out (default profiles/gmw_collect.txt).  No ratio is asked for in advance; the file says what was found.

    python tools/time_gmw_collect.py [--frames 64] [--reps 3] [--no-trace] [--out profiles/gmw_collect.txt]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from time_detector_eval import KITTI_SIZES, write_split
from tools.kernel_trace import traced_child

ONCE_CALLS = 20
BATCH = 8


def once(mode, dev):
    """A traced child: a seeded batch of 8 images with 3 objects each; `base` stops after the set-up."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.synthetic import make_batch
    from dcd_amd.gmw.collect import TrainRecordCollector
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False])
    _, targets = make_batch(BATCH, seed=0, n_objects=3, device=dev)
    col = TrainRecordCollector(cfg, dev, BATCH * 3 * ONCE_CALLS, ONCE_CALLS)
    g = torch.Generator().manual_seed(0)
    pois = (torch.randn((BATCH, col.spec["M"], col.spec["C"]), generator=g) * 0.5).to(dev)
    numbers = torch.arange(BATCH, dtype=torch.int32).to(dev)
    torch.cuda.synchronize()
    for _ in range(ONCE_CALLS if mode != "base" else 0):
        col.add(pois, targets, numbers)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", choices=("base", "collect"), default=None, help="what a traced child runs")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmw_collect.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_gmw_collect.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    if args.once:
        return once(args.once, dev)
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.train import collect_gmw_records, do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, init_like_trained
    from dcd_amd.gmw.data import ResidentRecords, load_train_data
    from dcd_amd.model.detector import KeypointDetector

    work = tempfile.mkdtemp(prefix="gmw_collect_")
    try:
        n = args.frames
        kitti = os.path.join(work, "kitti")
        write_split(kitti, n)
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.GENERATE_GMW", True, "SOLVER.IMS_PER_BATCH", BATCH])
        files = KittiFiles(kitti, "train", cfg, is_train=True)
        split = ResidentSplit(files, cfg, dev)
        iterations = len(files) // BATCH
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev)
        init_like_trained(model)
        optimizer = build_optimizer(model, cfg)
        scheduler, warmup = build_scheduler(optimizer, cfg)
        out = os.path.join(work, "out")
        counts = {}

        def file_route():
            lc = model.heads.loss_evaluator
            lc.gen_data = {k: [] for k in lc.gen_data}
            do_train(cfg, model, optimizer, scheduler, warmup, ResidentBatches(split, BATCH, seed=0), {"iteration": 0}, out)
            records = ResidentRecords(load_train_data(os.path.join(out, "gen_data", "gen_data_train.json")), dev)
            counts["file"] = len(records)

        def device_route():
            counts["device"] = len(collect_gmw_records(model, ResidentBatches(split, BATCH, seed=0), iterations, cfg=cfg))

        variants = (("file route (first series)", file_route), ("file route (second series)", file_route), ("device route", device_route))
        file_route()
        device_route()
        seconds = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
                print("%s: %.3f s" % (name, seconds[name][-1]), file=sys.stderr, flush=True)
        med = {name: float(np.median(v)) for name, v in seconds.items()}
        base = (med["file route (first series)"], med["file route (second series)"])
        spread = abs(base[0] - base[1]) / max(base)
        lines = ["collecting GMW's training records: %d frames %s (%d with objects), batch %d, %d iterations, %s, %d alternating rounds "
                 "after warm-up; up to the same ResidentRecords (%d records by the file route, %d by the device route)"
                 % (n, sorted(set(KITTI_SIZES)), len(files), BATCH, iterations, torch.cuda.get_device_name(0), args.reps,
                    counts["file"], counts["device"])]
        lines.append("  %-28s %12s %12s %12s" % ("route", "median s", "min s", "images/s"))
        for name, _ in variants:
            lines.append("  %-28s %12.3f %12.3f %12.1f" % (name, med[name], np.min(seconds[name]), iterations * BATCH / med[name]))
        ratio = float(np.mean(base)) / med["device route"]
        verdict = "faster" if med["device route"] < min(base) * (1 - spread) else (
            "slower" if med["device route"] > max(base) * (1 + spread) else "within the spread")
        lines.append("  run-to-run spread of the file route (its two series): %.1f %%; the device route against it: %.2fx -- %s"
                     % (100 * spread, ratio, verdict))
        if not args.no_trace:
            found = {mode: traced_child(__file__, mode, work, 300) for mode in ("base", "collect")}
            calls = {m: sum(c for c, _ in f.values()) for m, f in found.items()}
            us = {m: sum(t for _, t in f.values()) for m, f in found.items()}
            lines.append("TrainRecordCollector.add on a batch of %d (rocprofv3 --kernel-trace --stats, children of their own, %d calls): "
                         "%.1f kernel launches and %.1f us of kernel time per call" % (
                             BATCH, ONCE_CALLS, (calls["collect"] - calls["base"]) / ONCE_CALLS, (us["collect"] - us["base"]) / ONCE_CALLS))
            for kernel in ("records_prepare", "edge_depth_fwd", "records_finish"):
                for name, (c, t) in sorted(found["collect"].items()):
                    if kernel in name:
                        lines.append("  %s: %.1f us per launch (%d launches)" % (kernel, t / c, c))
            rest = sorted(name for name in found["collect"] if not any(k in name for k in ("records_prepare", "edge_depth_fwd", "records_finish"))
                          and found["collect"][name][0] > found["base"].get(name, (0, 0.0))[0])
            if rest:
                lines.append("  other kernels of the calls: %s" % "; ".join(n[:80] for n in rest))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
