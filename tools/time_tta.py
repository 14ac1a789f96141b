"""What mirrored-view test-time augmentation (`inference(tta=...)`, csrc/tta.hip) costs, in one process:
  (a) the merge kernel alone on 8 x 50 and 8 x 128 seeded candidates per view (the clustered boxes of tools/time_nms.py as view A;
      view M their mirror images, jittered, a third of them moved away, shuffled; 73 key points per row), every candidate of A over
      the score threshold, match threshold 0.5, for each mode: device events around `ops.tta_merge_detections`, medians of
      --kernel-reps alternating repetitions;
  (b) the same kernel from `rocprofv3 --kernel-trace --stats` runs of their own (fresh children, `--once kernel<K>_<mode>`,
      ONCE_CALLS launches each);
  (c) the bytes one batch of 8 frames stages with the mirrored records naming the same pixels, against listing every frame twice;
  (d) `engine.inference.inference(batch_size=8)` end to end on the seeded frames of tools/time_detector_eval.py without TTA (two
      series: nothing of the TTA code runs in them) against TTA in mode bev, alternating, medians over --reps rounds after one
      warm-up pass each.  The AP tables of seeded frames and a fresh detector say nothing about accuracy: they are only reported as
      having been computed.
Writes the figures to --out (default profiles/tta.txt).

    python tools/time_tta.py [--frames 192] [--reps 3] [--no-trace] [--out profiles/tta.txt]"""
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
from tools.time_nms import MODES, NK, candidates

ONCE_CALLS = 20
WIDTH = 1242


def two_views(B, K, device, seed=0):
    """(rows (2 B K, 14), aux (2 B K, 4), k2, k3, widths (B,)): view A = `time_nms.candidates`, view M = its mirror image with a
    second look's jitter, a third of the rows moved away, shuffled, with descending raw scores of its own."""
    rows, aux, _, _ = (t.cpu().numpy() for t in candidates(B, K, device, seed))
    rng = np.random.RandomState(seed + 1)
    m = rows.copy().reshape(B, K, 14)
    m[:, :, 2], m[:, :, 4] = (WIDTH - 1) - rows.reshape(B, K, 14)[:, :, 4], (WIDTH - 1) - rows.reshape(B, K, 14)[:, :, 2]
    m[:, :, 9] = -m[:, :, 9]
    m[:, :, 12] = np.where(m[:, :, 12] < 0, -np.pi - m[:, :, 12], np.pi - m[:, :, 12])
    m[:, :, 2:6] += rng.normal(0, 0.4, (B, K, 4))
    m[:, :, 9:12] += rng.normal(0, 0.02, (B, K, 3))
    gone = rng.rand(B, K) < 1 / 3
    m[:, :, 9] += gone * 25.0
    m[:, :, 2] += gone * 400.0
    m[:, :, 4] += gone * 400.0
    xm = aux.copy().reshape(B, K, 4)
    for b in range(B):
        m[b] = m[b][rng.permutation(K)]
        xm[b, :, 0] = -np.sort(-rng.uniform(0.05, 0.95, K))
    m[:, :, 13] = xm[:, :, 0]
    aux[:, 1] = rng.uniform(0.05, 2.0, B * K)
    xm[:, :, 1] = rng.uniform(0.05, 2.0, (B, K))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
    return (t(np.concatenate([rows, m.reshape(B * K, 14)])), t(np.concatenate([aux, xm.reshape(B * K, 4)])),
            t(rng.normal(0, 1, (2 * B * K, NK, 2))), t(rng.normal(0, 1, (2 * B * K, NK, 3))),
            torch.full((B,), WIDTH, dtype=torch.int32, device=device))


def note(text):
    print("[time_tta] " + text, file=sys.stderr, flush=True)


def main():
    once = ["kernel%d_%s" % (K, m) for K in (50, 128) for m in MODES]
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=192)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=100)
    ap.add_argument("--once", choices=once, default=None, help="what a traced child runs: ONCE_CALLS launches of the kernel")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tta.py measures on the GPU; none found")
    from dcd_amd import ops
    dev = torch.device("cuda:0")
    sets = {K: two_views(8, K, dev) for K in (50, 128)}

    def kernel(K, mode):
        rows, aux, k2, k3, widths = sets[K]
        return ops.tta_merge_detections(rows, aux, k2, k3, K, widths, mode, 0.5, 0.0, 0.5)

    if args.once:
        K, mode = args.once[6:].split("_")
        for _ in range(ONCE_CALLS):
            kernel(int(K), mode)
        torch.cuda.synchronize()
        return

    from dcd_amd.config import get_cfg
    from dcd_amd.data.input_pipeline import DeviceInputPipeline
    from dcd_amd.data.kitti_files import KittiFiles
    from dcd_amd.engine.inference import TTASpec, inference
    from dcd_amd.engine.trainer import init_like_trained
    from dcd_amd.model.detector import KeypointDetector
    work = tempfile.mkdtemp(prefix="tta_")
    try:
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
        lines = ["mirrored-view merge of decoded detections: %s; 8 images, every candidate of view A over the score threshold, match "
                 "threshold 0.5, %d key points" % (torch.cuda.get_device_name(0), NK),
                 "ops.tta_merge_detections, device events around the call (allocation of the outputs included), medians of %d "
                 "alternating calls:" % args.kernel_reps]
        for K in (50, 128):
            lines.append("  8 x %3d candidates per view: " % K + ", ".join(
                "%s %.1f us" % (m, float(np.median([a.elapsed_time(b) * 1e3 for a, b in events[(K, m)]]))) for m in MODES))
        matched = {K: {m: int((kernel(K, m)[5] >= 0).sum()) for m in MODES} for K in (50, 128)}
        lines.append("  matched pairs (2d / bev / 3d): %s of 400, %s of 1024" % tuple(
            " / ".join(str(matched[K][m]) for m in MODES) for K in (50, 128)))

        # (b) kernel traces, children of their own
        if not args.no_trace:
            for m in once:
                note("traced child: " + m)
                found = traced_child(__file__, m, work, 600)
                k = [v for name, v in found.items() if "tta_merge" in name]
                if not k:
                    sys.exit("the kernel trace does not list tta_merge")
                K, mode = m[6:].split("_")
                lines.append("tta_merge, mode %s, 8 x %s candidates per view (rocprofv3 --kernel-trace --stats, a child of its own): %.1f us "
                             "per launch (%d launches)" % (mode, K, k[0][1] / k[0][0], k[0][0]))

        # (c), (d) the pass
        n = args.frames
        write_split(os.path.join(work, "kitti"), n)
        cfg = get_cfg(opts=["MODEL.PRETRAIN", False, "MODEL.USE_SYNC_BN", False, "TEST.DETECTIONS_THRESHOLD", 0.0])
        torch.manual_seed(0)
        model = KeypointDetector(cfg).to(dev)
        init_like_trained(model)
        model.eval()
        files = KittiFiles(os.path.join(work, "kitti"), "train", cfg, is_train=False)
        pipe = DeviceInputPipeline(cfg, dev, is_train=False)
        frames, samples = [files.frame(i) for i in range(8)], [files.sample(i) for i in range(8)]
        ids = [files.img_id(i) for i in range(8)]
        staged = {}
        for name, kw in (("plain", dict(frames=frames, samples=samples, img_ids=ids)),
                         ("shared", dict(frames=frames, samples=samples + samples, img_ids=ids + ids, flip=[False] * 8 + [True] * 8,
                                         frame_of=list(range(8)) * 2)),
                         ("twice", dict(frames=frames + frames, samples=samples + samples, img_ids=ids + ids, flip=[False] * 8 + [True] * 8))):
            _, targets = pipe(kw.pop("frames"), kw.pop("samples"), keep_frames=True, **kw)
            staged[name] = targets[0].get_field("frames").numel()
        torch.cuda.synchronize()
        lines.append("bytes staged for one batch of 8 frames: %d without TTA; with TTA %d when the mirrored records name the same pixels, "
                     "%d if every frame were listed twice" % (staged["plain"], staged["shared"], staged["twice"]))

        note("end to end")
        spec = TTASpec("bev", 0.3, 0.5)
        variants = (("none (first series)", None), ("none (second series)", None), ("tta bev", spec))
        inference(model, files, pipe, os.path.join(work, "warm"), batch_size=8)
        inference(model, files, pipe, os.path.join(work, "warm"), batch_size=8, tta=spec)
        seconds = {name: [] for name, _ in variants}
        tables = {}
        for r in range(args.reps):
            for name, tta in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tables[name] = inference(model, files, pipe, os.path.join(work, "out"), batch_size=8, tta=tta)
                torch.cuda.synchronize()
                seconds[name].append(time.perf_counter() - t0)
        lines.append("inference(batch_size=8), end to end (AP evaluation included), %d frames %s, 50 candidates per image (threshold 0), "
                     "%d alternating rounds after warm-up:" % (n, sorted(set(KITTI_SIZES)), args.reps))
        lines.append("  %-24s %12s %12s %12s" % ("pass", "images/s", "median s", "min s"))
        for name, _ in variants:
            lines.append("  %-24s %12.1f %12.3f %12.3f" % (name, n / float(np.median(seconds[name])), np.median(seconds[name]),
                                                           np.min(seconds[name])))
        base = [float(np.median(seconds[k])) for k in ("none (first series)", "none (second series)")]
        lines.append("  run-to-run spread of 'none' (its two series): %.1f %%; TTA against their mean: x %.2f"
                     % (100 * abs(base[0] - base[1]) / max(base), float(np.median(seconds["tta bev"])) / float(np.mean(base))))
        lines.append("  the AP tables of both passes were computed (%s); seeded frames and a fresh detector: no accuracy figure is claimed"
                     % ", ".join(sorted(tables["tta bev"])))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
