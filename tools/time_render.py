"""What drawing the detections on the device (csrc/render.hip, `inference(render_dir=...)`) costs, in one process:
  (a) the two kernels on 8 KITTI-sized frames x 50 seeded candidates with 73 key points and 5 ground-truth objects each, every
      candidate drawn, from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child, `--once kernels`, ONCE_CALLS calls
      of `ops.render_detections`), and device events around the call in this process;
  (b) `engine.inference.inference(batch_size=8)` end to end on the seeded frames of tools/time_detector_eval.py without and with
      `render_dir` (TEST.VISUALIZE_THRESHOLD -1: every kept row of the fresh detector is drawn), alternating, medians over --reps
      rounds after one warm-up pass, with the spread of the two series without;
  (c) the PNG encoding alone: Pillow on the 8 pictures of (a), one thread, at the writer's compression level and at Pillow's default;
  (d) the comparison: the same primitive table drawn on the host with a Pillow `ImageDraw` loop (table and frames already there).
Writes the figures to --out (default profiles/render.txt).

    python tools/time_render.py [--frames 192] [--reps 3] [--no-trace] [--out profiles/render.txt]"""
import argparse
import io
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
B, K, NK, M = 8, 50, 73, 5
IN_H, IN_W = 384, 1280


def scene(device, seed=0):
    """Arguments of `ops.render_detections` for B frames of KITTI's sizes: K candidates in front of the camera, all drawn."""
    from dcd_amd import ops
    rng = np.random.RandomState(seed)
    sizes = [KITTI_SIZES[i % len(KITTI_SIZES)] for i in range(B)]
    sizes = [(min(w, IN_W), min(h, IN_H)) for w, h in sizes]
    frames = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for w, h in sizes]
    P = np.array([721.5377, 0, 609.5593, 44.85728, 0, 721.5377, 172.854, 0.2163791, 0, 0, 1, 0.002745884], np.float32)
    table = np.zeros((B, 16), np.float32)
    table[:, 2], table[:, 3], table[:, 4:] = IN_W, IN_H, P
    rows, aux = np.zeros((B * K, 14), np.float32), np.zeros((B * K, 4), np.float32)
    z = rng.uniform(5, 60, B * K)
    rows[:, 0] = rng.randint(0, 3, B * K)
    rows[:, 6:9] = rng.uniform(1.4, 4.2, (B * K, 3))
    rows[:, 9], rows[:, 10], rows[:, 11] = rng.uniform(-0.5, 0.5, B * K) * z, rng.uniform(1.2, 1.9, B * K), z
    rows[:, 12] = rng.uniform(-np.pi, np.pi, B * K)
    x0, y0 = rng.uniform(0, 1100, B * K), rng.uniform(100, 300, B * K)
    rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5] = x0, y0, x0 + rng.uniform(20, 120, B * K), y0 + rng.uniform(15, 70, B * K)
    rows[:, 13] = aux[:, 0] = np.tile(-np.sort(-rng.uniform(0.3, 0.95, K)), B)
    k2 = (rng.uniform(-0.6, 0.6, (B * K, NK, 2)) * np.array([1.0, 0.2])).astype(np.float32)
    dims, locs = rng.uniform(1.4, 4.2, (B, M, 3)).astype(np.float32), np.zeros((B, M, 3), np.float32)
    locs[:, :, 2] = rng.uniform(6, 50, (B, M))
    locs[:, :, 0], locs[:, :, 1] = rng.uniform(-0.4, 0.4, (B, M)) * locs[:, :, 2], 1.0
    gt = (dims, locs, rng.uniform(-np.pi, np.pi, (B, M)).astype(np.float32), np.ones((B, M), np.uint8))
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return dict(frames=frames, sizes=sizes, staged=ops.stage_frames(frames, device), rows=t(rows), aux=t(aux), k2=t(k2), table=t(table),
                gt=tuple(t(a) for a in gt))


def note(text):
    print("[time_render] " + text, file=sys.stderr, flush=True)


def pillow_draw(frames, sizes, entries, counts):
    """The comparison: every drawn entry of the device's table with Pillow's own line / point calls (its raster, not the rule's)."""
    from PIL import Image, ImageDraw
    out = []
    for b, (frame, (w, h)) in enumerate(zip(frames, sizes)):
        img = Image.new("RGB", (w + h, h), (230, 230, 230))
        img.paste(Image.fromarray(frame), (0, 0))
        draw = ImageDraw.Draw(img)
        for e in entries[b, :counts[b]]:
            if e[1] < 0:
                continue
            left = w if e[0] else 0
            rgb = (int(e[7]), int(e[8]), int(e[9]))
            if e[1] == 0:
                draw.line((int(e[2]) + left, int(e[3]), int(e[4]) + left, int(e[5])), fill=rgb, width=int(e[6]))
            else:
                draw.rectangle((int(e[2]), int(e[3]), int(e[4]), int(e[5])), outline=rgb)
        out.append(img)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--once", choices=("kernels",), default=None, help="what a traced child runs: ONCE_CALLS calls of the op")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_render.py measures on the GPU; none found")
    from dcd_amd import ops
    dev = torch.device("cuda:0")
    s = scene(dev)

    def render(want_table=False):
        return ops.render_detections(s["staged"], s["rows"], s["aux"], s["k2"], None, s["table"], s["gt"], K, 0.2, 0.0, keypoints=True,
                                     want_table=want_table, in_h=IN_H, in_w=IN_W)

    if args.once:
        for _ in range(ONCE_CALLS):
            render()
        torch.cuda.synchronize()
        return

    from PIL import Image
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.data.resident import default_workers
    from dcd_amd.engine.inference import inference
    from dcd_amd.engine.render import PngWriter
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    work = tempfile.mkdtemp(prefix="render_")
    try:
        # (a) the op
        note("the op alone")
        for _ in range(5):
            render()
        torch.cuda.synchronize()
        events = []
        for _ in range(args.kernel_reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            render()
            e1.record()
            events.append((e0, e1))
        torch.cuda.synchronize()
        canvas, (entries, counts, _) = render(want_table=True)
        canvas, entries, counts = canvas.cpu().numpy(), entries.cpu().numpy(), counts.cpu().numpy()
        drawn = int((entries[:, :, 1] >= 0).sum())
        lines = ["detections drawn on the device: %s; %d frames %s in %d x %d, %d candidates with %d key points and %d ground-truth objects "
                 "each, all drawn: %d primitives, %.2f Mpx of pictures"
                 % (torch.cuda.get_device_name(0), B, sorted(set(s["sizes"])), IN_H, IN_W, K, NK, M, drawn,
                    sum(h * (w + h) for w, h in s["sizes"]) / 1e6),
                 "ops.render_detections, device events around the call (allocation of table and canvas included), median of %d calls: "
                 "%.1f us" % (args.kernel_reps, float(np.median([a.elapsed_time(b) * 1e3 for a, b in events])))]
        if not args.no_trace:
            note("traced child")
            found = traced_child(__file__, "kernels", work, 600)
            for kernel in ("render_setup", "render_raster"):
                k = [v for name, v in found.items() if kernel in name]
                if not k:
                    sys.exit("the kernel trace does not list " + kernel)
                lines.append("%s (rocprofv3 --kernel-trace --stats, a child of its own): %.1f us per launch (%d launches)"
                             % (kernel, k[0][1] / k[0][0], k[0][0]))

        # (c) PNG encoding alone, (d) the host's drawing
        note("PNG encoding and the Pillow loop")
        pictures = [np.ascontiguousarray(canvas[b, :h, :w + h]) for b, (w, h) in enumerate(s["sizes"])]
        for level, what in ((1, "the writer's compress_level 1"), (6, "Pillow's default 6")):
            t0 = time.perf_counter()
            size = 0
            for p in pictures:
                buf = io.BytesIO()
                Image.fromarray(p).save(buf, format="PNG", compress_level=level)
                size += buf.tell()
            lines.append("PNG encoding alone, one thread, %s: %.1f ms per picture (%.2f MB each; noise frames, which do not compress)"
                         % (what, (time.perf_counter() - t0) * 1e3 / B, size / B / 1e6))
        t0 = time.perf_counter()
        pillow_draw(s["frames"], s["sizes"], entries, counts)
        lines.append("the same table drawn on the host, Pillow ImageDraw (table and frames already on the host): %.1f ms per picture"
                     % ((time.perf_counter() - t0) * 1e3 / B))
        t0 = time.perf_counter()
        writer = PngWriter(os.path.join(work, "pool"))
        for _ in range(4):
            writer.submit(canvas, ["%06d" % i for i in range(B)], s["sizes"])
        writer.close()
        lines.append("PngWriter, its thread pool, %d pictures: %.1f ms per picture" % (4 * B, (time.perf_counter() - t0) * 1e3 / (4 * B)))

        # (b) end to end, alternating
        note("end to end")
        n = args.frames
        write_split(os.path.join(work, "kitti"), n)
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0,
                            "TEST.VISUALIZE_THRESHOLD", -1.0])
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev)
        init_like_trained(model)
        model.eval()
        files = KittiFiles(os.path.join(work, "kitti"), "train", cfg, is_train=False)
        pipe = DeviceInputPipeline(cfg, dev, is_train=False)
        variants = (("without (first series)", {}), ("without (second series)", {}), ("render_dir", {"render_dir": os.path.join(work, "png")}),
                    ("render_dir, key points", {"render_dir": os.path.join(work, "png"), "render_keypoints": True}))
        inference(model, files, pipe, os.path.join(work, "warm"), batch_size=8)
        inference(model, files, pipe, os.path.join(work, "warm"), batch_size=8, render_dir=os.path.join(work, "png"))
        seconds = {name: [] for name, _ in variants}
        for r in range(args.reps):
            for name, extra in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                inference(model, files, pipe, os.path.join(work, "out"), batch_size=8, **extra)
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
        written = len(os.listdir(os.path.join(work, "png")))
        lines.append("inference(batch_size=8), end to end, %d frames %s, 50 rows drawn per image, %d alternating rounds after warm-up "
                     "(decoding and encoding pools of %d threads):" % (n, sorted(set(KITTI_SIZES)), args.reps, default_workers(None)))
        lines.append("  %-26s %12s %12s %12s" % ("", "images/s", "median s", "min s"))
        for name, _ in variants:
            lines.append("  %-26s %12.1f %12.3f %12.3f" % (name, n / float(np.median(seconds[name])), np.median(seconds[name]),
                                                           np.min(seconds[name])))
        base = [float(np.median(seconds[k])) for k in ("without (first series)", "without (second series)")]
        lines.append("  run-to-run spread of 'without' (its two series): %.1f %%; render_dir against their mean: %+.1f %%, with key points "
                     "%+.1f %%; %d pictures in the directory"
                     % (100 * abs(base[0] - base[1]) / max(base), 100 * (float(np.median(seconds["render_dir"])) / float(np.mean(base)) - 1),
                        100 * (float(np.median(seconds["render_dir, key points"])) / float(np.mean(base)) - 1), written))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
