"""What the box NMS on decoded detections (TEST.USE_NMS, csrc/nms.hip) costs, in one process:
  (a) the kernel alone on 8 x 50 and 8 x 128 seeded candidates (clustered boxes: half of them jittered copies of the others, 73 key
      points per row), every candidate over the score threshold, NMS threshold 0 -- so every pair that touches suppresses --, for
      each mode: device events around `ops.nms_detections`, medians of --kernel-reps alternating repetitions;
  (b) the same kernel from `rocprofv3 --kernel-trace --stats` runs of their own (fresh children, `--once kernel50 | kernel128`,
      ONCE_CALLS launches of mode 3d each);
  (c) the kernel launches of the decode of ONE batched evaluation batch (`PostProcessor.decode_fused` on the predictions of 8
      images), traced children `--once batch_predictor | batch_none | batch_3d`: the predictor alone, or followed by ONCE_CALLS
      decodes with TEST.USE_NMS none / 3d; per decode the launches of kernels the predictor child never launches, the difference between the two decode
      children, and the launches of nms_detections itself by name;
  (d) `engine.inference.inference(batch_size=8)` end to end on the seeded frames of tools/time_detector_eval.py with TEST.USE_NMS
      'none' against '3d' (threshold 0.5), the two alternating, medians over --reps rounds after one warm-up pass.
Writes the figures to --out (default profiles/nms.txt).

    python tools/time_nms.py [--frames 192] [--reps 3] [--no-trace] [--out profiles/nms.txt]"""
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
NK = 73
MODES = ("2d", "bev", "3d")


def candidates(B, K, device, seed=0):
    """(rows (B K, 14), aux (B K, 4), k2, k3): per image K / 2 boxes of `eval.synthetic.random_boxes` and a jittered copy of each,
    shuffled; raw scores descending in (0.3, 0.95), the final score the raw one."""
    from dcd_amd.eval.synthetic import random_boxes
    rng = np.random.RandomState(seed)
    rows = np.zeros((B, K, 14), np.float32)
    aux = np.zeros((B, K, 4), np.float32)
    for b in range(B):
        g = random_boxes(rng, (K + 1) // 2)
        src = np.concatenate([np.arange((K + 1) // 2), np.arange(K // 2)])
        copy = (np.arange(K) >= (K + 1) // 2)[:, None]
        blk = rows[b]
        blk[:, 0] = rng.randint(0, 3, (K + 1) // 2)[src]
        blk[:, 1] = g["alpha"][src]
        blk[:, 2:6] = g["bbox"][src] + copy * rng.normal(0, 1.5, (K, 4))
        d = g["dimensions"][src] + copy * rng.normal(0, 0.03, (K, 3))
        blk[:, 6], blk[:, 7], blk[:, 8] = d[:, 1], d[:, 2], d[:, 0]
        blk[:, 9:12] = g["location"][src] + copy * rng.normal(0, 0.08, (K, 3))
        blk[:, 12] = g["rotation_y"][src] + copy[:, 0] * rng.normal(0, 0.04, K)
        blk[:] = blk[rng.permutation(K)]
        aux[b, :, 0] = -np.sort(-rng.uniform(0.3, 0.95, K))
        blk[:, 13] = aux[b, :, 0]
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return (t(rows.reshape(B * K, 14)), t(aux.reshape(B * K, 4)), t(rng.normal(0, 1, (B * K, NK, 2)).astype(np.float32)),
            t(rng.normal(0, 1, (B * K, NK, 3)).astype(np.float32)))


def note(text):
    print("[time_nms] " + text, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=100)
    ap.add_argument("--once", choices=("kernel50", "kernel128", "batch_predictor", "batch_none", "batch_3d"), default=None,
                    help="what a traced child runs: ONCE_CALLS launches of the kernel, or the predictor on one batch, alone or "
                         "followed by ONCE_CALLS decodes")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nms.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_nms.py measures on the GPU; none found")
    from dcd_amd import ops
    dev = torch.device("cuda:0")
    sets = {K: candidates(8, K, dev) for K in (50, 128)}

    def kernel(K, mode):
        return ops.nms_detections(*sets[K], K, mode, 0.0, 0.0, False)

    if args.once in ("kernel50", "kernel128"):
        for _ in range(ONCE_CALLS):
            kernel(int(args.once[6:]), "3d")
        torch.cuda.synchronize()
        return

    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    work = tempfile.mkdtemp(prefix="nms_")
    try:
        n = 8 if args.once else args.frames
        write_split(os.path.join(work, "kitti"), n)
        models = {}
        for name, opts in (("none", []), ("3d", ["TEST.USE_NMS", "3d", "TEST.NMS_THRESH", 0.5])):
            if args.once and name != ("3d" if args.once == "batch_3d" else "none"):
                continue                                                 # (a traced child builds the one model it runs)
            cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0] + opts)
            torch.manual_seed(0)
            models[name] = KeypointDetector(cfg).to(dev)
            init_like_trained(models[name])
            models[name].eval()
        files = KittiFiles(os.path.join(work, "kitti"), "train", cfg, is_train=False)
        pipe = DeviceInputPipeline(cfg, dev, is_train=False)

        if args.once:                                                    # one batched evaluation batch, as `_batched_pass` runs it
            model = models["3d" if args.once == "batch_3d" else "none"]
            with torch.no_grad():
                images, targets = pipe([files.frame(i) for i in range(8)], [files.sample(i) for i in range(8)],
                                       img_ids=[files.img_id(i) for i in range(8)])
                model.heads.predictor.sparse_eval_heads = True
                preds = model.heads.predictor(model.backbone(images), targets)
                for _ in range(0 if args.once == "batch_predictor" else ONCE_CALLS):
                    model.heads.post_processor.decode_fused(preds, targets)
            torch.cuda.synchronize()
            return

        # (a) the kernel alone
        note("the kernel alone")
        cases = [(K, mode) for K in (50, 128) for mode in MODES]
        for c in cases:
            for _ in range(5):
                kernel(*c)
        torch.cuda.synchronize()
        events = {c: [] for c in cases}
        for _ in range(args.kernel_reps):
            for c in cases:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                kernel(*c)
                e1.record()
                events[c].append((e0, e1))
        torch.cuda.synchronize()
        lines = ["box NMS on decoded detections: %s; 8 images, every candidate over the score threshold, NMS threshold 0, %d key points"
                 % (torch.cuda.get_device_name(0), NK),
                 "ops.nms_detections, device events around the call (allocation of the outputs included), medians of %d alternating calls:"
                 % args.kernel_reps]
        for K in (50, 128):
            lines.append("  8 x %3d candidates: " % K + ", ".join(
                "%s %.1f us" % (m, float(np.median([a.elapsed_time(b) * 1e3 for a, b in events[(K, m)]]))) for m in MODES))
        survivors = {K: int((kernel(K, "3d")[1][:, 0] >= 0).sum()) for K in (50, 128)}
        lines.append("  survivors of mode 3d: %d of 400, %d of 1024" % (survivors[50], survivors[128]))

        # (b), (c) kernel traces, children of their own
        if not args.no_trace:
            found = {}
            for m in ("kernel50", "kernel128", "batch_predictor", "batch_none", "batch_3d"):
                note("traced child: " + m)
                found[m] = traced_child(__file__, m, work, 600)
            for m, K in (("kernel50", 50), ("kernel128", 128)):
                k = [v for name, v in found[m].items() if "nms_detections" in name]
                if not k:
                    sys.exit("the kernel trace does not list nms_detections")
                lines.append("nms_detections, mode 3d, 8 x %d candidates (rocprofv3 --kernel-trace --stats, a child of its own): %.1f us per "
                             "launch (%d launches)" % (K, k[0][1] / k[0][0], k[0][0]))
            calls = {m: sum(c for c, _ in found[m].values()) for m in ("batch_none", "batch_3d")}
            nms_calls = {m: sum(c for name, (c, _) in found[m].items() if "nms_detections" in name) for m in calls}
            lines.append("kernel launches of one decode_fused call on the predictions of 8 images (traced children of their own: the "
                         "predictor alone, and followed by %d decodes with TEST.USE_NMS none / 3d):" % ONCE_CALLS)
            only = {m: sum(c for name, (c, _) in found[m].items() if name not in found["batch_predictor"]) / ONCE_CALLS
                    for m in ("batch_none", "batch_3d")}
            lines.append("  of kernels the predictor child never launches: %.2f with none, %.2f with 3d"
                         % (only["batch_none"], only["batch_3d"]))
            lines.append("  all launches of the 3d child minus all of the none child, per decode: %.2f; of nms_detections itself: %.2f with "
                         "none, %.2f with 3d"
                         % ((calls["batch_3d"] - calls["batch_none"]) / ONCE_CALLS, nms_calls["batch_none"] / ONCE_CALLS,
                            nms_calls["batch_3d"] / ONCE_CALLS))

        # (d) end to end, alternating
        note("end to end")
        variants = (("none (first series)", "none"), ("none (second series)", "none"), ("3d", "3d"))
        inference(models["none"], files, pipe, os.path.join(work, "warm"), batch_size=8)
        inference(models["3d"], files, pipe, os.path.join(work, "warm"), batch_size=8)
        seconds = {name: [] for name, _ in variants}
        for r in range(args.reps):
            for name, key in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference(models[key], files, pipe, os.path.join(work, "out"), batch_size=8)
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
        kept = sum(len(open(os.path.join(work, "out", "data", f)).read().splitlines()) for f in os.listdir(os.path.join(work, "out", "data")))
        lines.append("inference(batch_size=8), end to end, %d frames %s, 50 candidates per image (threshold 0), %d alternating rounds after "
                     "warm-up:" % (n, sorted(set(KITTI_SIZES)), args.reps))
        lines.append("  %-24s %12s %12s %12s" % ("TEST.USE_NMS", "images/s", "median s", "min s"))
        for name, _ in variants:
            lines.append("  %-24s %12.1f %12.3f %12.3f" % (name, n / float(np.median(seconds[name])), np.median(seconds[name]),
                                                           np.min(seconds[name])))
        base = [float(np.median(seconds[k])) for k in ("none (first series)", "none (second series)")]
        lines.append("  run-to-run spread of 'none' (its two series): %.1f %%; 3d against their mean: %+.1f %%; rows written with 3d at "
                     "threshold 0.5: %d of %d" % (100 * abs(base[0] - base[1]) / max(base),
                                                  100 * (float(np.median(seconds["3d"])) / float(np.mean(base)) - 1), kept, 50 * n))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
