"""What evaluating the whole two-stage system (DGDE detector, then GMW) over a split costs, in one process:
  (a) the two-step route: `engine.inference.inference(batch_size=8, gen_out_dir=...)` writes `gen_data_infer.json`,
      `gmw.load_infer_data` parses it back, `gmw.evaluate` refines, writes and scores -- timed TWICE per round, the two series'
      medians give the run-to-run spread;
  (b) the one-pass route: `inference(batch_size=8, gmw=model)`: the kept candidates stay on the device
      (`ops.gmw_pack_records` -> `gmw.refine_packed`), no JSON;
      both end to end (PNG decode, both models, result files, both AP tables), on a seeded split of --frames KITTI-size frames
      (tools/time_detector_eval.py's), `init_like_trained` detector weights and a seeded GMW; once at threshold 0 (every image
      keeps its 50 candidates) and once at a threshold taken from the run's own raw scores that keeps as near to 5 rows per image as its distinct values allow; the
      routes alternate, medians over --reps rounds after one warm-up pass of each;
  (c) from `rocprofv3 --kernel-trace --stats` runs of their own (three fresh children, `--once base | pack | chain`: 256 records
      gathered out of 400 decoded candidates ONCE_CALLS times by `ops.gmw_pack_records`, or by the torch chain it replaces --
      the gather of the kept rows, `index_select` x4, `cat` x2, `transpose().contiguous()` x2 and the row slices): kernel time and
      kernel launches per call = (that child - the base child) / ONCE_CALLS.
Writes the figures to --out (default profiles/dcd_eval.txt).  No ratio is asked for in advance; the file says what was found.

    python tools/time_dcd_eval.py [--frames 192] [--reps 3] [--no-trace] [--out profiles/dcd_eval.txt]"""
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
PACKED = 256


def once(mode, dev):
    """A traced child: 400 decoded candidates (8 images x 50), 256 of them kept; `base` stops after the set-up."""
    from dcd_amd import ops
    from dcd_amd.gmw import GMW
    g = torch.Generator().manual_seed(0)
    rows, k2, k3 = (torch.randn(s, generator=g).to(dev) for s in ((400, 14), (400, 73, 2), (400, 73, 3)))
    model = GMW().to(dev)
    src = torch.randperm(400, generator=g)[:PACKED].sort().values.to(dev)
    src32, pi32, pj32 = src.int(), model.pair_i.int(), model.pair_j.int()
    P = pi32.numel()
    bufs = [torch.zeros((PACKED,) + s, device=dev) for s in ((4, P), (6, P), (73, 2), (73, 3), (1,), (3,), (3,))]
    torch.cuda.synchronize()
    for _ in range(ONCE_CALLS if mode != "base" else 0):
        if mode == "pack":
            ops.gmw_pack_records(rows, k2, k3, src32, 0, pi32, pj32, *bufs)
        else:
            r, a, b = rows.index_select(0, src), k2.index_select(0, src), k3.index_select(0, src)
            out = (model.edge_expand(a).transpose(-2, -1).contiguous(), model.edge_expand(b).transpose(-2, -1).contiguous(),
                   r[:, 12:13].contiguous(), r[:, 9:12].contiguous(), r[:, 6:9].contiguous())
            del out
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--once", choices=("base", "pack", "chain"), default=None, help="what a traced child runs")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dcd_eval.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_dcd_eval.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    if args.once:
        return once(args.once, dev)
    from dcd_amd import gmw as G
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine import inference as inf
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector

    work = tempfile.mkdtemp(prefix="dcd_eval_")
    try:
        n = args.frames
        kitti = os.path.join(work, "kitti")
        write_split(kitti, n)
        gmw_root = os.path.join(work, "for_gmw")                                   # the layout `gmw.evaluate` reads
        os.makedirs(os.path.join(gmw_root, "training", "ImageSets"))
        shutil.copytree(os.path.join(kitti, "label_2"), os.path.join(gmw_root, "training", "label_2"))
        shutil.copy(os.path.join(kitti, "ImageSets", "train.txt"), os.path.join(gmw_root, "training", "ImageSets", "val.txt"))
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0])
        files = KittiFiles(kitti, "train", cfg, is_train=False)
        pipe = DeviceInputPipeline(cfg, dev, is_train=False)
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev)
        init_like_trained(model)
        torch.manual_seed(0)
        gmw = G.GMW().to(dev).eval()
        pp = model.heads.post_processor
        out = os.path.join(work, "out")

        def two_step():
            inf.inference(model, files, pipe, os.path.join(out, "det"), batch_size=8, gen_out_dir=os.path.join(out, "gen"))
            data = G.load_infer_data(os.path.join(out, "gen", "gen_data_infer.json"))
            G.evaluate(gmw, data, gmw_root, None, os.path.join(out, "gmw"), device=dev, batch_size=256)
            return len(data["img_idx"])

        def one_pass():
            inf.inference(model, files, pipe, os.path.join(out, "one"), batch_size=8, gmw=gmw, gmw_batch=256)

        # the raw scores of the split, for the second threshold: the value that leaves 5 n rows (scores descend per image)
        raw, original = [], inf.write_image_rows

        def spy(rows, raw_scores, threshold, path):
            raw.append(np.array(raw_scores, np.float64))
            return original(rows, raw_scores, threshold, path)
        inf.write_image_rows = spy
        try:
            inf.inference(model, files, pipe, os.path.join(out, "scores"), batch_size=8)
        finally:
            inf.write_image_rows = original
        ranked = np.sort(np.concatenate(raw))[::-1]
        values, first = np.unique(-ranked, return_index=True)                      # descending distinct scores; a threshold v keeps
        kept = np.append(first[1:], len(ranked))                                   # every score >= v: `kept` rows
        best = int(np.argmin(np.abs(kept - 5 * n)))                                # (ties -- a plateau of equal scores -- move it off 5 n)
        realistic = float(-values[best])

        variants = (("two-step (first series)", two_step), ("two-step (second series)", two_step), ("one pass", one_pass))
        lines = ["evaluating the two-stage system: %d frames %s, detector batch 8, GMW groups of 256, %s, %d alternating rounds after "
                 "warm-up; end to end, both AP tables included" % (n, sorted(set(KITTI_SIZES)), torch.cuda.get_device_name(0), args.reps)]
        for label, threshold in (("threshold 0", 0.0), ("threshold %.6g (the distinct score whose kept rows, %d of %d, are nearest to 5 per image)"
                                                        % (realistic, int(kept[best]), len(ranked)), realistic)):
            pp.det_threshold = threshold
            records = two_step()                                                   # warm-up of both routes at this record count
            one_pass()
            seconds = {name: [] for name, _ in variants}
            for _ in range(args.reps):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    seconds[name].append(time.perf_counter() - t0)
                    print("%s, %s: %.3f s" % (label.split(" (")[0], name, seconds[name][-1]), file=sys.stderr, flush=True)
            med = {name: float(np.median(v)) for name, v in seconds.items()}
            base = (med["two-step (first series)"], med["two-step (second series)"])
            spread = abs(base[0] - base[1]) / max(base)
            lines.append("%s: %d records" % (label, records))
            lines.append("  %-28s %12s %12s %12s" % ("route", "median s", "min s", "images/s"))
            for name, _ in variants:
                lines.append("  %-28s %12.3f %12.3f %12.1f" % (name, med[name], np.min(seconds[name]), n / med[name]))
            ratio = float(np.mean(base)) / med["one pass"]
            verdict = "faster" if med["one pass"] < min(base) * (1 - spread) else ("slower" if med["one pass"] > max(base) * (1 + spread)
                                                                                   else "within the spread")
            lines.append("  run-to-run spread of the two-step route (its two series): %.1f %%; one pass against it: %.2fx -- %s"
                         % (100 * spread, ratio, verdict))
        pp.det_threshold = 0.0
        if not args.no_trace:
            found = {mode: traced_child(__file__, mode, work, 300) for mode in ("base", "pack", "chain")}
            calls = {m: sum(c for c, _ in f.values()) for m, f in found.items()}
            us = {m: sum(t for _, t in f.values()) for m, f in found.items()}
            k = [v for name, v in found["pack"].items() if "gmw_pack_records" in name]
            if not k:
                sys.exit("the kernel trace does not list gmw_pack_records")
            lines.append("%d records out of 400 candidates (rocprofv3 --kernel-trace --stats, children of their own, %d calls each):"
                         % (PACKED, ONCE_CALLS))
            lines.append("  gmw_pack_records: %.1f us per launch (%d launches), %.1f kernel launches per call"
                         % (k[0][1] / k[0][0], k[0][0], (calls["pack"] - calls["base"]) / ONCE_CALLS))
            lines.append("  the torch chain (row gather, index_select x4, cat x2, transpose().contiguous() x2, row slices): %.1f us of "
                         "kernel time per call, %.1f kernel launches per call"
                         % ((us["chain"] - us["base"]) / ONCE_CALLS, (calls["chain"] - calls["base"]) / ONCE_CALLS))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
