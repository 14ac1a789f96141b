"""What the KITTI evaluation costs on a split of the val set's size: 3 769 synthetic images with the statistics of the test
fixtures' scene generator (dcd_amd/eval/synthetic.py: 2-8 ground-truth boxes, jittered detections, false positives), three
classes, bbox / BEV / 3-D / AOS.
  (a) `official_eval` end to end from annotation dicts to the result text: host clock around a call that ends in device-to-host
      copies, median of --reps repetitions after one warm-up call;
  (b) the kernels of csrc/eval.hip, from a `rocprofv3 --kernel-trace --stats` run of their own (a fresh child process running
      this file with --once; tracing slows the host, so (a) is taken with the profiler off).
There is no reference figure: the reference's evaluator is numba.cuda and cannot run on this hardware.
Writes the figures with the commit (tools/.commit, see tools/stamp_commit.sh) to --out (default profiles/kitti_eval.txt).

    python tools/time_kitti_eval.py [--reps 7] [--images 3769] [--no-trace] [--out profiles/kitti_eval.txt]"""
import argparse
import csv
import glob
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

KERNELS = ("eval_overlaps", "eval_match", "eval_sum_similarity")


def commit():
    try:
        return open(os.path.join(ROOT, "tools", ".commit")).read().strip() or "unknown"
    except OSError:
        return "unknown"


def trace(images, work):
    """{kernel label: (calls, total us)} from a kernel trace of one evaluation in a child process."""
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", work, "-o", "eval", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--once", "--images", str(images)]
    r = subprocess.run(cmd, cwd=work, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run failed (%d):\n%s" % (r.returncode, r.stdout[-2000:]))
    found = {}
    for path in glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            for k in KERNELS:
                if k in row["Name"]:
                    label = k + ("<counts>" if "Lb1" in row["Name"] or "<true>" in row["Name"] else
                                 "<scores>" if k == "eval_match" else "")
                    calls, total = found.get(label, (0, 0.0))
                    found[label] = (calls + int(row["Calls"]), total + float(row["TotalDurationNs"]) / 1e3)
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--images", type=int, default=3769)
    ap.add_argument("--once", action="store_true", help="one evaluation and exit (what the traced child runs)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_eval.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_kitti_eval.py measures on the GPU; none found")
    from dcd_amd.eval import kitti_ap, synthetic

    gts, dts = synthetic.make_scene(np.random.RandomState(0), args.images)
    stages = {}
    text, _ = kitti_ap.official_eval(gts, dts, [0, 1, 2], stages=stages)            # warm-up: code objects, allocator
    if args.once:
        return
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        again, _ = kitti_ap.official_eval(gts, dts, [0, 1, 2])
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        assert again == text
    times = np.array(times) * 1e3
    n_gt, n_dt = sum(len(g["name"]) for g in gts), sum(len(d["name"]) for d in dts)
    pairs = sum(len(g["name"]) * len(d["name"]) for g, d in zip(gts, dts))
    lines = ["KITTI AP on %d synthetic images (%d ground-truth boxes, %d detections, %d pairs), classes Car / Pedestrian / Cyclist, "
             "%d combinations, up to %d thresholds; %s; commit %s"
             % (args.images, n_gt, n_dt, pairs, len(stages["comb"]), max(len(t) for t in stages["thresholds"]),
                torch.cuda.get_device_name(0), commit()),
             "official_eval end to end, host clock, %d repetitions after warm-up: median %.1f ms, min %.1f ms, max %.1f ms"
             % (args.reps, np.median(times), times.min(), times.max())]
    if not args.no_trace:
        work = tempfile.mkdtemp(prefix="kitti_eval_trace_")
        try:
            found = trace(args.images, work)
        finally:
            shutil.rmtree(work, ignore_errors=True)
        if not found:
            sys.exit("the kernel trace lists none of %s" % (KERNELS,))
        lines.append("kernels of one evaluation (rocprofv3 --kernel-trace --stats, a run of its own):")
        for label in sorted(found):
            lines.append("  %-28s %3d launch(es) %10.1f us" % (label, found[label][0], found[label][1]))
    lines += ["result text of the scene:", text.rstrip("\n")]
    out = "\n".join(lines) + "\n"
    print(out, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
