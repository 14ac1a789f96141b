"""What the device input pipeline costs at eight KITTI-size frames (384 x 1280 input), in one process, with device events over
alternating repetitions after warm-up; the device is idle when a window opens, so host work inside a call counts:
  (a) the image kernel alone (`dcd_preprocess_images`, csrc/images.hip) on frames already staged on the device (50 launches
      per event pair, so the figure is the kernel and not the launch path);
  (b) the whole `DeviceInputPipeline` call: packing into the pinned slot, the 11 MB uint8 copy, the kernel, the label flip and
      the target encoding (host time included: the events bracket the call);
  (c) what one would write without the kernel: the stock torch chain per image on the device (`flip`, `pad`,
      `.float().div(255)`, normalise, channel index, `stack`) on the same staged uint8 bytes;
  (d) the 47 MB pinned fp32 copy that ready-made fp32 inputs (`synthetic.make_batch`-style) imply.
Writes the four times with their spread, and the kernel's bytes over its time as GB/s and as a share of the 8 TB/s HBM
yardstick, to --out (default profiles/input_pipeline.txt).  Exits non-zero when (a) is slower than (c): (c) is a dozen
launches per image, so that would mean the kernel is wrong, not slow.

    python tools/time_input_pipeline.py [--reps 200] [--out profiles/input_pipeline.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from torch.nn import functional as F

SIZES = ((1242, 375), (1224, 370), (1242, 375), (1238, 374), (1242, 375), (1224, 370), (1242, 375), (1242, 375))    # (w, h)
FLIPS = (1, 0, 1, 0, 0, 1, 1, 0)


def samples_for(sizes, rng):
    """A few objects per image, drawn like tests/test_gpu_heads.py's random scenes: the target encoder's share of (b)."""
    from dcd_amd.data.calibration import KITTI_P2
    out = []
    for w, h in sizes:
        n = 5
        z = rng.uniform(8, 50, n)
        t = np.stack([rng.uniform(-0.3, 0.3, n) * z, np.full(n, 1.65), z], 1).astype(np.float32)
        u = (721.5377 * t[:, 0] + 609.5593 * t[:, 2]) / t[:, 2]
        box = np.stack([np.clip(u - 400 / z, 0, w - 1), np.clip(172 - 500 / z, 0, h - 1), np.clip(u + 400 / z, 0, w - 1),
                        np.clip(172 + 700 / z, 0, h - 1)], 1)
        ry = rng.uniform(-np.pi, np.pi, n)
        alpha = (ry - np.arctan2(t[:, 0], t[:, 2]) + np.pi) % (2 * np.pi) - np.pi
        hwl = np.stack([rng.normal(1.5, 0.1, n), rng.normal(1.6, 0.1, n), rng.normal(3.9, 0.3, n)], 1)
        out.append(dict(image_size=np.array([w, h]), P=KITTI_P2, trunc_occ=np.zeros((n, 2)), box2d=box, hwl=hwl, t=t, ry=ry, alpha=alpha,
                        find_pcl=np.ones(n, np.int32), kpts3d=rng.uniform(-0.5, 0.5, (n, 63, 3)) * hwl[:, None, [2, 0, 1]]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "input_pipeline.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_input_pipeline.py measures on the GPU; none found")
    from dcd_amd import _lib
    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline

    dev = torch.device("cuda:0")
    cfg = get_cfg(opts=["MODEL.PRETRAIN", False])
    in_w, in_h, B = cfg.INPUT.WIDTH_TRAIN, cfg.INPUT.HEIGHT_TRAIN, len(SIZES)
    rng = np.random.RandomState(0)
    frames = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for w, h in SIZES]
    samples = samples_for(SIZES, rng)
    pipe = DeviceInputPipeline(cfg, dev, is_train=True, seed=0)
    L = _lib.lib()

    # frames staged once, in the pipeline's own layout, for (a) and (c)
    slot, nbytes = pipe._pack(frames, FLIPS)
    staged = slot.buf[:nbytes].to(dev)
    rec = slot.buf[:B * 40].numpy().view(np.int64).reshape(B, 5).copy()
    table = pipe._table_host.to(dev)
    out = torch.empty((B, 3, in_h, in_w), dtype=torch.float32, device=dev)
    stream = _lib.stream_of(out)
    mean = torch.tensor(cfg.INPUT.PIXEL_MEAN, device=dev)[:, None, None]
    std = torch.tensor(cfg.INPUT.PIXEL_STD, device=dev)[:, None, None]
    bgr = torch.tensor([2, 1, 0], device=dev)
    fp32_host = torch.empty((B, 3, in_h, in_w), dtype=torch.float32).pin_memory()
    fp32_dev = torch.empty_like(out)

    def kernel():
        _lib.check(L.dcd_preprocess_images(stream, staged.data_ptr(), nbytes, staged.data_ptr(), table.data_ptr(), B, in_h, in_w,
                                           int(cfg.INPUT.TO_BGR), out.data_ptr()), "dcd_preprocess_images")
        return out

    def whole():
        return pipe(frames, samples, flip=FLIPS)[0]

    def stock():
        xs = []
        for (off, pitch, h, w, flip) in rec:
            img = staged[off:off + h * pitch].view(h, w, 3)
            if flip:
                img = img.flip(1)
            px, py = (in_w - w) // 2, (in_h - h) // 2
            x = F.pad(img.permute(2, 0, 1), (px, in_w - w - px, py, in_h - h - py))
            x = x.float().div(255).sub(mean).div(std)
            if cfg.INPUT.TO_BGR:
                x = x[bgr]
            xs.append(x)
        return torch.stack(xs)

    def copy47():
        fp32_dev.copy_(fp32_host, non_blocking=True)
        return fp32_dev

    variants = (("a kernel alone", kernel), ("b whole pipeline call", whole), ("c stock torch chain", stock), ("d 47 MB fp32 copy", copy47))
    inner = {"a kernel alone": 50}          # launches per event pair: one ~10 us kernel between two events times the launch path
    diff = (kernel() - stock()).abs().max().item()
    same_b = torch.equal(whole(), kernel())
    for _ in range(10):
        for _, fn in variants:
            fn()
    torch.cuda.synchronize()
    events = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(inner.get(name, 1)):
                fn()
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    us = {name: np.array([a.elapsed_time(b) * 1e3 / inner.get(name, 1) for a, b in ev]) for name, ev in events.items()}

    in_mb, out_mb = sum(w * h * 3 for w, h in SIZES) / 1e6, B * 3 * in_h * in_w * 4 / 1e6
    med = {name: float(np.median(v)) for name, v in us.items()}
    a, c = med["a kernel alone"], med["c stock torch chain"]
    gbs = (in_mb + out_mb) * 1e6 / (a * 1e-6) / 1e9
    lines = ["input pipeline at %d frames %s -> (%d, 3, %d, %d) fp32, %s, %d alternating repetitions after warm-up, device events"
             % (B, sorted(set(SIZES)), B, in_h, in_w, torch.cuda.get_device_name(0), args.reps),
             "%-24s %10s %10s %10s %10s   (us)" % ("", "median", "p10", "p90", "min")]
    for name, _ in variants:
        v = us[name]
        lines.append("%-24s %10.1f %10.1f %10.1f %10.1f" % (name, np.median(v), np.percentile(v, 10), np.percentile(v, 90), v.min()))
    lines += ["kernel traffic: %.1f MB in + %.1f MB out over the median = %.0f GB/s = %.1f %% of the 8 TB/s yardstick (floor %.1f us)"
              % (in_mb, out_mb, gbs, gbs / 80.0, (in_mb + out_mb) / 8.0),
              "(a) <= (c): %s (%.1fx);  max |kernel - stock chain| = %.3g;  pipeline images == kernel images: %s"
              % ("holds" if a <= c else "VIOLATED", c / a, diff, same_b)]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if a > c or not same_b:
        sys.exit(1)


if __name__ == "__main__":
    main()
