"""What feeding the train step costs, from a KITTI directory of 64 frames (seeded noise PNGs at the four KITTI sizes, the labels of
tests/golden/kitti_files repeated), at batch 8, in one process:
  (a) `ResidentSplit.batch` (dcd_amd/data/resident.py), the whole call with an idle device: B row numbers up, one gather, the image
      kernel on the resident frames, the target encoding;
  (b) `DeviceInputPipeline.__call__` on the same images, decoded beforehand: packing, the 11 MB copy, the same two kernels;
  (a) and (b) alternate, device events bracket each call (host work inside a call counts), medians over --reps repetitions;
  (c) the kernels of the resident call (gather, images, the target encoding's two), from a `rocprofv3 --kernel-trace --stats`
      run of its own (a fresh child process running `--once`);
  (d) what `do_train`'s `data` meter shows -- the time it waits in `batches.get`, taken here by a wrapper around the source -- over
      --iters iterations with the real step
      (`KeypointDetector`, `train_step`), for `ResidentBatches` and `StreamingBatches`, each with and without `Prefetcher`;
  (e) the one-off load: `ResidentSplit(...)` wall time (PNG decode in the thread pool, upload) and its `nbytes`.
Writes the figures to --out (default profiles/train_input.txt).  The expectation was that (a) costs less host time than (b),
since it drops the packing and the copy; the file says whether it does.

With --right the tool measures something else and nothing of the above: `ResidentSplit.batch` on the both-cameras split
(DATASETS.USE_RIGHT_IMAGE, 128 views of the same 64 images plus an `image_3` folder) against the left-only split, as two left-only
series around the both-cameras one, the kernels of either call from a kernel trace of its own (`--once`, `--once --right`), and
the load time and bytes of either split; see `measure_right`.

    python tools/time_train_input.py [--reps 100] [--iters 50] [--no-trace] [--out profiles/train_input.txt]
    python tools/time_train_input.py --right [--reps 100] [--no-trace] [--out profiles/train_input_right.txt]"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

KITTI_SIZES = ((1242, 375), (1224, 370), (1238, 374), (1280, 384))        # (w, h)
N_IMAGES, BATCH = 64, 8
KERNELS = ("gather_rows", "preprocess_images", "target_encode_objects", "target_edge_indices")    # the encoding is two launches


def write_split(root, right=False):
    """64 images under `root` in KITTI's layout: the three fixture scenes that keep an object, repeated; noise PNGs.
    right: also `image_3`, other noise at the same sizes (the fixture's calibration files carry a `P3` line)."""
    from PIL import Image
    fixture = os.path.join(ROOT, "tests", "golden", "kitti_files")
    for d in ("image_2", "label_2", "calib", "ImageSets", "kpts_ann") + (("image_3",) if right else ()):
        os.makedirs(os.path.join(root, d))
    ann = json.load(open(os.path.join(fixture, "kpts_ann", "kpts_ann_train.json")))
    rng = np.random.RandomState(0)
    out_ann = {}
    for i in range(N_IMAGES):
        src, name = "%06d" % (i % 3), "%06d" % i
        for d in ("label_2", "calib"):
            shutil.copy(os.path.join(fixture, d, src + ".txt"), os.path.join(root, d, name + ".txt"))
        out_ann[str(i)] = ann[str(i % 3)]
        w, h = KITTI_SIZES[i % len(KITTI_SIZES)]
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8), mode="RGB").save(os.path.join(root, "image_2", name + ".png"))
        if right:
            noise = np.random.RandomState(1000 + i).randint(0, 256, (h, w, 3)).astype(np.uint8)      # (its own stream: image_2 stays as it was)
            Image.fromarray(noise, mode="RGB").save(os.path.join(root, "image_3", name + ".png"))
    with open(os.path.join(root, "ImageSets", "train.txt"), "w") as f:
        f.write("".join("%06d\n" % i for i in range(N_IMAGES)))
    with open(os.path.join(root, "kpts_ann", "kpts_ann_train.json"), "w") as f:
        json.dump(out_ann, f)


def trace(work, extra=()):
    """{kernel: (calls, total us)} of 20 resident batches, from a kernel trace of a child process (`--once` plus `extra`)."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", "resident", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--once"] + list(extra)
    r = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
    found = {}
    for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row["Name"]:
                    calls, total = found.get(k, (0, 0.0))
                    found[k] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]) / 1e3)
    return found


class Timed:
    """A batch source whose `get` is clocked on the host: the wait `do_train` books under `data`, and the time between two
    consecutive calls (one iteration)."""

    def __init__(self, source):
        self.source, self.batch_size, self.wait, self.starts = source, source.batch_size, [], []

    def __len__(self):
        return len(self.source)

    def get(self, k):
        t0 = time.perf_counter()
        batch = self.source.get(k)
        self.starts.append(t0)
        self.wait.append(time.perf_counter() - t0)
        return batch


def stats(v):
    v = np.asarray(v)
    return "%10.1f %10.1f %10.1f %10.1f" % (np.median(v), np.percentile(v, 10), np.percentile(v, 90), v.min())


def measure_right(args):
    """--right: `ResidentSplit.batch` on the both-cameras split (DATASETS.USE_RIGHT_IMAGE: 128 views of the 64 images) against the
    same call on the left-only split, in one process.  Every repetition runs left, both, left again: the two left series are the
    baseline and the distance of their medians is the spread a difference has to exceed to mean anything.  The batches of either
    split are those of its own `ResidentBatches(seed=0)` plan, so the both-cameras batches mix the two halves.  Also the one-off
    load of the both-cameras split and its resident bytes."""
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import ResidentBatches
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="train_input_right_")
    try:
        root = os.path.join(work, "kitti")
        write_split(root, right=True)
        base = ["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False]
        cfg_left, cfg_both = get_cfg(opts=base), get_cfg(opts=base + ["DATASETS.USE_RIGHT_IMAGE", True])
        torch.zeros(1, device=dev)
        torch.cuda.synchronize()
        splits, load_s = {}, {}
        for name, cfg in (("left", cfg_left), ("both", cfg_both)):
            if args.once and name == "left":
                continue
            files = KittiFiles(root, "train", cfg, is_train=True)
            assert len(files) == (N_IMAGES if name == "left" else 2 * N_IMAGES)
            t0 = time.perf_counter()
            splits[name] = ResidentSplit(files, cfg, dev)
            torch.cuda.synchronize()
            load_s[name] = time.perf_counter() - t0
        plans = {}
        for name, split in splits.items():
            plan = ResidentBatches(split, BATCH, seed=0).plan
            plans[name] = [plan(k) for k in range(len(split) // BATCH)]
        if args.once:                                                  # the traced child: 20 batches of the both-cameras split
            for k in range(20):
                splits["both"].batch(*plans["both"][k % len(plans["both"])])
            torch.cuda.synchronize()
            return None
        right_rows = sum(i >= N_IMAGES for idx, _ in plans["both"] for i in idx)
        series = (("left-only, first series", "left"), ("both cameras", "both"), ("left-only, second series", "left"))
        for k in range(10):
            for _, which in series:
                splits[which].batch(*plans[which][k % len(plans[which])])
        torch.cuda.synchronize()
        events, host = {n: [] for n, _ in series}, {n: [] for n, _ in series}
        for k in range(args.reps):
            for name, which in series:
                idx, fl = plans[which][k % len(plans[which])]
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                splits[which].batch(idx, fl)
                host[name].append((time.perf_counter() - t0) * 1e6)
                e1.record()
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        lines = ["ResidentSplit.batch with both cameras: %d images %s, %d views, batch %d -> (%d, 3, %d, %d) fp32, %s, %d repetitions of "
                 "(left, both, left) after warm-up; %d of the %d rows drawn from the both-cameras split are right views"
                 % (N_IMAGES, sorted(set(KITTI_SIZES)), 2 * N_IMAGES, BATCH, BATCH, cfg_both.INPUT.HEIGHT_TRAIN, cfg_both.INPUT.WIDTH_TRAIN,
                    torch.cuda.get_device_name(0), args.reps, right_rows, BATCH * len(plans["both"])),
                 "%-44s %10s %10s %10s %10s   (us)" % ("", "median", "p10", "p90", "min")]
        med = {}
        for name, _ in series:
            dev_us = [a.elapsed_time(b) * 1e3 for a, b in events[name]]
            med[name] = float(np.median(dev_us))
            lines.append("%-44s %s" % (name + ", device events", stats(dev_us)))
            lines.append("%-44s %s" % (name + ", host time in the call", stats(host[name])))
        first, second, both = med["left-only, first series"], med["left-only, second series"], med["both cameras"]
        spread, diff = abs(first - second), both - (first + second) / 2
        lines.append("both cameras - mean of the two left-only medians: %+.1f us; spread between the two left-only medians: %.1f us; "
                     "the difference %s the spread" % (diff, spread, "EXCEEDS" if abs(diff) > spread else "is within"))
        if not args.no_trace:                                          # the kernels of either call, each traced in a run of its own
            found = {}
            for name, extra in (("left", ()), ("both", ("--right",))):
                tdir = os.path.join(work, "trace_" + name)
                os.makedirs(tdir)
                found[name] = trace(tdir, extra)
            lines.append("kernels of the call (rocprofv3 --kernel-trace --stats, a run of its own per split, 20 calls), us each:")
            lines.append("  %-28s %12s %12s" % ("", "left-only", "both cameras"))
            for k in KERNELS:
                if k in found["left"] and k in found["both"]:
                    lines.append("  %-28s %12.2f %12.2f" % (k, found["left"][k][1] / max(1, found["left"][k][0]),
                                                            found["both"][k][1] / max(1, found["both"][k][0])))
        for name in ("left", "both"):
            s = splits[name]
            lines.append("one-off load, %-4s: %3d frames (PNG decode in %d threads + upload) %.2f s;  resident bytes: %d (%.1f MB), "
                         "of which frames %d" % (name, len(s), s.workers, load_s[name], s.nbytes, s.nbytes / 1e6, s.frame_bytes))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--right", action="store_true", help="compare the both-cameras split (DATASETS.USE_RIGHT_IMAGE) with the left-only "
                    "split instead: ResidentSplit.batch, load time and bytes; writes profiles/train_input_right.txt")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--once", action="store_true", help="load, 20 resident batches and exit (what the traced child runs)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=None, help="default profiles/train_input.txt (with --right: profiles/train_input_right.txt)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "train_input_right.txt" if args.right else "train_input.txt")
    if not torch.cuda.is_available():
        sys.exit("time_train_input.py measures on the GPU; none found")
    if args.right:
        lines = measure_right(args)
        if lines is None:
            return
        text = "\n".join(lines) + "\n"
        print(text, end="")
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
        return
    from dcd_amd.config import get_cfg
    from dcd_amd.data.batches import Prefetcher, ResidentBatches, StreamingBatches
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import ResidentSplit
    from dcd_amd.engine.train import do_train
    from dcd_amd.engine.trainer import build_optimizer, build_scheduler, init_like_trained
    from dcd_amd.model.detector import KeypointDetector

    dev = torch.device("cuda:0")
    work = tempfile.mkdtemp(prefix="train_input_")
    try:
        write_split(os.path.join(work, "kitti"))
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "SOLVER.MAX_ITERATION", args.iters,
                            "SOLVER.IMS_PER_BATCH", BATCH, "SOLVER.SAVE_CHECKPOINT_INTERVAL", 10 ** 9])
        files = KittiFiles(os.path.join(work, "kitti"), "train", cfg, is_train=True)
        assert len(files) == N_IMAGES
        torch.zeros(1, device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        split = ResidentSplit(files, cfg, dev)
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t0
        plan = ResidentBatches(split, BATCH, seed=0).plan
        batches = [plan(k) for k in range(N_IMAGES // BATCH)]
        if args.once:
            for k in range(20):
                split.batch(*batches[k % len(batches)])
            torch.cuda.synchronize()
            return

        # (a) / (b): the same images through both paths, alternating
        pipe = DeviceInputPipeline(cfg, dev, is_train=True, seed=0)
        frames = [files.frame(i) for i in range(N_IMAGES)]
        samples = [files.sample(i) for i in range(N_IMAGES)]

        def resident(k):
            idx, fl = batches[k % len(batches)]
            return split.batch(idx, fl)

        def pipeline(k):
            idx, fl = batches[k % len(batches)]
            return pipe([frames[i] for i in idx], [samples[i] for i in idx], flip=fl)
        variants = (("a ResidentSplit.batch", resident), ("b DeviceInputPipeline call", pipeline))
        same = all(torch.equal(resident(k)[0], pipeline(k)[0]) for k in range(len(batches)))
        for k in range(10):
            for _, fn in variants:
                fn(k)
        torch.cuda.synchronize()
        events, host = {n: [] for n, _ in variants}, {n: [] for n, _ in variants}
        for k in range(args.reps):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                t0 = time.perf_counter()
                fn(k)
                host[name].append((time.perf_counter() - t0) * 1e6)
                e1.record()
                events[name].append((e0, e1))
        torch.cuda.synchronize()
        lines = ["feeding the train step: %d frames %s, batch %d -> (%d, 3, %d, %d) fp32, %s, %d alternating repetitions after warm-up"
                 % (N_IMAGES, sorted(set(KITTI_SIZES)), BATCH, BATCH, cfg.INPUT.HEIGHT_TRAIN, cfg.INPUT.WIDTH_TRAIN,
                    torch.cuda.get_device_name(0), args.reps),
                 "%-44s %10s %10s %10s %10s   (us)" % ("", "median", "p10", "p90", "min")]
        for name, _ in variants:
            lines.append("%-44s %s" % (name + ", device events", stats([a.elapsed_time(b) * 1e3 for a, b in events[name]])))
            lines.append("%-44s %s" % (name + ", host time in the call", stats(host[name])))
        med = {n: float(np.median([a.elapsed_time(b) * 1e3 for a, b in events[n]])) for n, _ in variants}
        a, b = med["a ResidentSplit.batch"], med["b DeviceInputPipeline call"]
        lines.append("(a) < (b): %s (%.2fx);  images of (a) == images of (b) on all %d batches: %s"
                     % ("holds" if a < b else "REFUTED", b / a, len(batches), same))

        # (c) the kernels, traced in a run of their own
        if not args.no_trace:
            tdir = os.path.join(work, "trace")
            os.makedirs(tdir)
            found = trace(tdir)
            if not found:
                sys.exit("the kernel trace lists none of %s" % (KERNELS,))
            lines.append("kernels of the resident call (rocprofv3 --kernel-trace --stats, a run of its own, 20 calls):")
            for k in KERNELS:
                if k in found:
                    lines.append("  %-28s %3d launch(es) %10.1f us each" % (k, found[k][0], found[k][1] / max(1, found[k][0])))

        # (d) the data meter of do_train with the real step
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev).train()
        init_like_trained(model)
        optimizer = build_optimizer(model, cfg)
        scheduler, warmup = build_scheduler(optimizer, cfg)
        lines.append("`data` meter of %d do_train iterations with the real step (ms waiting in batches.get; host clock):" % args.iters)
        lines.append("  %-44s %10s %10s %10s" % ("", "median", "mean", "step median"))

        def sources():
            yield "ResidentBatches", lambda: ResidentBatches(split, BATCH, seed=0)
            yield "StreamingBatches", lambda: StreamingBatches(files, DeviceInputPipeline(cfg, dev, is_train=True), BATCH, seed=0)
        for name, make in sources():
            for prefetch in (False, True):
                source = make()
                timed = Timed(Prefetcher(source, dev) if prefetch else source)
                do_train(cfg, model, optimizer, scheduler, warmup, timed, {"iteration": 0}, os.path.join(work, "out"))
                torch.cuda.synchronize()
                lines.append("  %-44s %10.2f %10.2f %10.2f" % (name + (" + Prefetcher" if prefetch else ""), np.median(timed.wait) * 1e3,
                                                              np.mean(timed.wait) * 1e3, np.median(np.diff(timed.starts)) * 1e3))
                if hasattr(source, "close"):
                    source.close()

        # (e) the load
        lines.append("one-off load of the %d frames (PNG decode in %d threads + upload): %.2f s;  resident bytes: %d (%.1f MB)"
                     % (N_IMAGES, split.workers, load_s, split.nbytes, split.nbytes / 1e6))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
