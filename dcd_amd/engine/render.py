"""Pictures of an evaluation pass: every image's detections drawn ON THE DEVICE (`ops.render_detections`, two launches per batch;
the rule is DESIGN.md 6d) from what the batched pass already holds there -- decoded rows, the prefix / NMS marks, key points,
image table, ground-truth tables, the staged uint8 frames -- and written as `<render_dir>/<id>.png` by a small thread pool while
the next batches run.  The layout, colours and projection are those of the reference's `show_image_with_boxes`
(DGDE/engine/visualize_infer.py:190-312): the frame with 2-D boxes, projected 3-D boxes and labels, beside it the bird's-eye
panel, ground truth under detections.

    renderer = Renderer(cfg, device, keypoints=False, render_dir=DIR)
    renderer.add(k, ids, frames, rows, aux, recs, table, targets)      # batch k: launches, one asynchronous copy, no wait on it
    renderer.finish()                                                  # the last batch, then every file is on disk

`add` copies batch k's canvas to one of two pinned slots behind an event and then hands batch k - 1 -- whose event has long
fired -- to the writer: the loop waits on one event per batch, a batch late, as the result writer of the pass does.  The host
cuts `canvas[b, :h, :w + h]` out of the slot (a copy: the slot is free again) and the pool encodes.  PNG encoding is the cost
of the feature (profiles/render.txt); when the pool falls more than `MAX_PENDING` pictures behind, `add` waits for the oldest."""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from dcd_amd.data.resident import default_workers
from dcd_amd.structures.params_3d import stack_field

MAX_PENDING = 64


def _write_png(path, picture, compress_level):
    from PIL import Image
    Image.fromarray(picture).save(path, format="PNG", compress_level=compress_level)


class PngWriter:
    """`submit(canvas, ids, sizes)`: canvas (B, H, W, 3) uint8 on the host, sizes [(w, h)] -> `<directory>/<id>.png` of
    canvas[b, :h, :w + h], encoded by `workers` threads.  The pictures are copied out before `submit` returns.  `close()` waits
    for every file and raises the first error of a worker."""

    def __init__(self, directory, workers=None, compress_level=1):
        os.makedirs(directory, exist_ok=True)
        self.directory, self.compress_level = directory, int(compress_level)
        self._pool = ThreadPoolExecutor(max_workers=default_workers(workers))
        self._pending = deque()

    def submit(self, canvas, ids, sizes):
        for b, (img_id, (w, h)) in enumerate(zip(ids, sizes)):
            picture = np.ascontiguousarray(canvas[b, :h, :w + h])
            while len(self._pending) >= MAX_PENDING:
                self._pending.popleft().result()
            self._pending.append(self._pool.submit(_write_png, os.path.join(self.directory, img_id + ".png"), picture, self.compress_level))

    def close(self):
        try:
            while self._pending:
                self._pending.popleft().result()
        finally:
            self._pool.shutdown(wait=True)


def ground_truth_tables(targets):
    """(dimensions (B, M, 3), locations (B, M, 3), rotys (B, M), reg_mask (B, M)) of a batch's targets, on their device."""
    return tuple(stack_field(targets, name) for name in ("dimensions", "locations", "rotys", "reg_mask"))


class Renderer:
    def __init__(self, cfg, device, keypoints=False, render_dir=None, workers=None, labelled=True):
        if render_dir is None:
            raise ValueError("Renderer needs a render_dir")
        self.device = torch.device(device)
        self.keypoints, self.labelled = bool(keypoints), bool(labelled)
        self.in_h, self.in_w = cfg.INPUT.HEIGHT_TRAIN, cfg.INPUT.WIDTH_TRAIN
        self.K = cfg.TEST.DETECTIONS_PER_IMG
        self.det_threshold, self.vis_threshold = cfg.TEST.DETECTIONS_THRESHOLD, cfg.TEST.VISUALIZE_THRESHOLD
        self.writer = PngWriter(render_dir, workers)
        self._slots, self._events, self._pending = [None, None], [None, None], None

    def add(self, k, ids, frames, rows, aux, recs, table, targets):
        """Batch k of the pass.  frames: the targets' "frames" field (the staged buffer); rows, aux, recs: what `decode_fused`
        returned; table: the decode's image table (B, 16); targets: the batch's, with "frame_size" and -- on a labelled split -- the
        ground-truth tables."""
        from dcd_amd import ops
        if self.keypoints and recs is None:
            raise ValueError("Renderer(keypoints=True) needs the decode's records (decode_fused(records=True))")
        B = len(ids)
        gt = ground_truth_tables(targets) if self.labelled else None
        k2, k3 = recs if recs is not None else (None, None)
        canvas, _ = ops.render_detections(frames, rows, aux, k2, k3, table, gt, self.K, self.det_threshold, self.vis_threshold,
                                          keypoints=self.keypoints, in_h=self.in_h, in_w=self.in_w)
        s = k % 2
        if self._slots[s] is None or self._slots[s].shape[0] < B:
            self._slots[s] = torch.empty((B,) + tuple(canvas.shape[1:]), dtype=torch.uint8).pin_memory()
        self._slots[s][:B].copy_(canvas, non_blocking=True)
        self._events[s] = torch.cuda.Event()
        self._events[s].record()
        self._flush()
        self._pending = (s, list(ids), [tuple(int(v) for v in t.get_field("frame_size")) for t in targets])
        return canvas

    def _flush(self):
        if self._pending is not None:
            s, ids, sizes = self._pending
            self._pending = None
            self._events[s].synchronize()
            self.writer.submit(self._slots[s].numpy(), ids, sizes)

    def finish(self):
        try:
            self._flush()
        finally:
            self.writer.close()
