"""What evaluating the detector over a split costs, one image per call against the batched pass, in one process:
  (a) images/s end to end of `engine.inference.inference(batch_size=1)` -- timed TWICE per round, the two series' medians give the
      run-to-run spread -- against `batch_size` 8 and 16, on a seeded split of --frames KITTI-size frames (noise PNGs at the four
      KITTI sizes, the labels of tests/golden/kitti_files repeated; nothing is downloaded), `init_like_trained` weights and a zero
      threshold so that every image decodes its 50 candidates; the variants alternate, medians over --reps rounds after one
      warm-up pass of each shape.  "End to end" is the whole call: PNG decode, forward, decode, copy, result files, reading them
      back and the AP tables;
  (b) the decode alone on the same predictions (heads at the top-K cells of a batch of 8): `PostProcessor.decode_fused` against
      `forward_batch`, device events around each call, medians of --decode-reps alternating repetitions;
  (c) from `rocprofv3 --kernel-trace --stats` runs of their own (three fresh children, `--once predictor | fused | chain`: the
      predictor on one batch of 8 alone, or followed by ONCE_CALLS decodes of one route): the decode kernel's time, and the
      kernel launches of one decode call of either route = (launches of that child - launches of the predictor child) / ONCE_CALLS.
Writes the figures to --out (default profiles/detector_eval.txt).  Acceptance: the batched route not slower than the one-image
route beyond the spread of (a) at any batch size; the file says whether that holds.

    python tools/time_detector_eval.py [--frames 192] [--reps 3] [--no-trace] [--out profiles/detector_eval.txt]"""
import argparse
import json
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

KITTI_SIZES = ((1242, 375), (1224, 370), (1238, 374), (1280, 384))        # (w, h)
ONCE_CALLS = 20


def write_split(root, n):
    """n images under `root` in KITTI's layout: the three fixture scenes that keep an object, repeated; noise PNGs."""
    from PIL import Image
    fixture = os.path.join(ROOT, "tests", "golden", "kitti_files")
    for d in ("image_2", "label_2", "calib", "ImageSets", "kpts_ann"):
        os.makedirs(os.path.join(root, d))
    ann = json.load(open(os.path.join(fixture, "kpts_ann", "kpts_ann_train.json")))
    rng = np.random.RandomState(0)
    out_ann = {}
    for i in range(n):
        src, name = "%06d" % (i % 3), "%06d" % i
        for d in ("label_2", "calib"):
            shutil.copy(os.path.join(fixture, d, src + ".txt"), os.path.join(root, d, name + ".txt"))
        out_ann[str(i)] = ann[str(i % 3)]
        w, h = KITTI_SIZES[i % len(KITTI_SIZES)]
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), mode="RGB").save(os.path.join(root, "image_2", name + ".png"))
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(n)))
    with open(os.path.join(root, "kpts_ann", "kpts_ann_train.json"), "w") as f:
        json.dump(out_ann, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--decode-reps", type=int, default=100)
    ap.add_argument("--once", choices=("predictor", "fused", "chain"), default=None,
                    help="what a traced child runs: the predictor alone, or followed by ONCE_CALLS decodes of one route")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_eval.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_detector_eval.py measures on the GPU; none found")
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector

    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="detector_eval_")
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
        pp, predictor = model.heads.post_processor, model.heads.predictor

        # the predictions of one batch of 8, for (b) and (c)
        with torch.no_grad():
            images, targets = pipe([files.frame(i) for i in range(8)], [files.sample(i) for i in range(8)],
                                   img_ids=[files.img_id(i) for i in range(8)])
            predictor.sparse_eval_heads = True
            preds = predictor(model.backbone(images), targets)
            predictor.sparse_eval_heads = False
            routes = {"fused": lambda: pp.decode_fused(preds, targets), "chain": lambda: pp.forward_batch(preds, targets)}
            if args.once:
                if args.once != "predictor":
                    for _ in range(ONCE_CALLS):
                        routes[args.once]()
                torch.cuda.synchronize()
                return
            for fn in routes.values():
                for _ in range(5):
                    fn()
            torch.cuda.synchronize()
            events = {k: [] for k in routes}
            for _ in range(args.decode_reps):
                for name, fn in routes.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    fn()
                    e1.record()
                    events[name].append((e0, e1))
            torch.cuda.synchronize()
        decode_us = {k: float(np.median([a.elapsed_time(b) * 1e3 for a, b in v])) for k, v in events.items()}

        # (a) end to end, alternating
        variants = (("batch 1 (first series)", 1), ("batch 1 (second series)", 1), ("batch 8", 8), ("batch 16", 16))
        for _, b in variants[1:]:                                                  # one warm-up pass of each shape
            inference(model, files, pipe, os.path.join(work, "warm%d" % b), batch_size=b)
        seconds = {name: [] for name, _ in variants}
        for r in range(args.reps):
            for name, b in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference(model, files, pipe, os.path.join(work, "out"), batch_size=b)
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
        rate = {name: n / float(np.median(v)) for name, v in seconds.items()}
        lines = ["evaluating the detector: %d frames %s, %d candidates per image (threshold 0), %s, %d alternating rounds after warm-up"
                 % (n, sorted(set(KITTI_SIZES)), cfg.TEST.DETECTIONS_PER_IMG, torch.cuda.get_device_name(0), args.reps),
                 "%-28s %12s %12s %12s" % ("inference(...), end to end", "images/s", "median s", "min s")]
        for name, _ in variants:
            lines.append("%-28s %12.1f %12.3f %12.3f" % (name, rate[name], np.median(seconds[name]), np.min(seconds[name])))
        base = (rate["batch 1 (first series)"], rate["batch 1 (second series)"])
        spread = abs(base[0] - base[1]) / max(base)
        lines.append("run-to-run spread of the one-image route (its two series): %.1f %%" % (100 * spread))
        for name in ("batch 8", "batch 16"):
            ok = rate[name] >= min(base) * (1 - spread)
            lines.append("%s against the one-image route: %.2fx -- not slower beyond the spread: %s"
                         % (name, rate[name] / float(np.mean(base)), "holds" if ok else "REFUTED"))
        lines.append("the decode alone on one batch of 8 (device events, medians of %d alternating calls): decode_fused %.1f us, "
                     "forward_batch %.1f us (%.1fx)" % (args.decode_reps, decode_us["fused"], decode_us["chain"],
                                                       decode_us["chain"] / decode_us["fused"]))
        # (c) kernel trace, children of their own
        if not args.no_trace:
            found = {mode: traced_child(__file__, mode, work, 600) for mode in ("predictor", "fused", "chain")}
            base_calls = sum(c for c, _ in found["predictor"].values())
            for mode in ("fused", "chain"):
                calls = sum(c for c, _ in found[mode].values())
                lines.append("kernel launches of one %s decode of 8 images (rocprofv3 --kernel-trace --stats, children of their own, "
                             "%d calls): %.1f" % (mode, ONCE_CALLS, (calls - base_calls) / ONCE_CALLS))
            k = [(name, v) for name, v in found["fused"].items() if "decode_detections" in name]
            if not k:
                sys.exit("the kernel trace does not list decode_detections")
            lines.append("decode_detections, 8 x %d candidates: %.1f us per launch (%d launches)"
                         % (cfg.TEST.DETECTIONS_PER_IMG, k[0][1][1] / k[0][1][0], k[0][1][0]))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
